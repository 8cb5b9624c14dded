"""Ranks of a node-sharded cluster whose shards DIFFER (tests/_seqgen.py sharded_mixed: unpadded names inserted in shuffled order,
identical empty nodes whose keys tie, zone values that live on one shard only, hostname-keyed spread and pod (anti)affinity, host
ports, a nodeName pin) against the ORACLE on the whole cluster. Launched by tests/test_gpu_sequential.py through
torch.distributed.run with SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>: the ranks share cuda:0.

  argv: <case> <seed>   (case = a key of CASES)
Before the first evaluation the ranks compare the shapes of their encoded topology dictionaries over gloo (KD, KS, domains per
key): shards that disagree would sum misaligned histogram cells, so the worker reports the difference and exits 3 on every rank.
Then, every rank:
  snapshot path  evaluate_into + gather_bitmap (plain and class-compressed) + exchange_decisions: every gathered row equals the
                 oracle's grid row, counts its row sums, decisions Oracle.decide;
  rounds         allocate_round over the first half of the asks (apply), then the rest (no apply) on top: together equal to the
                 oracle's sequential loop over all asks, in cluster indices, and both ran on the device;
  incremental    on a second set of engines: a few asks assumed by the shards that own their nodes, ONE collective evaluate_dirty
                 on every rank, the gathered rows of the other asks equal to the oracle's grid on the changed cluster;
  mismatch       (topology keys present) a node update on rank 0 brings a zone value no other shard knows: the next collective
                 step fails on EVERY rank with the same error, and nobody hangs or sums misaligned histograms."""
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("yunikorn-k8shim_amd")
sharding = importlib.import_module("yunikorn-k8shim_amd.sharding")
import _oracle as orc  # noqa: E402
import _seqgen  # noqa: E402

CASES = {
    # keys tie inside and across shards, no topology: the replay's tie-break between shards and inside a shuffled one
    "ties": dict(ties=True, zones_by_range=True, spread=False, ipa=False, ports=False, pin=True),
    # zone-keyed spread only, zones by name range: the shards' zone sets differ (one zone has a single node)
    "zones": dict(ties=True, zones_by_range=True, spread=True, ipa=False, ports=False, pin=False),
    # hostname anti-affinity (and zone affinity) between asks and towards resident pods, shards of unequal size
    # resident pods with anti-affinity terms on the first shard only: their count classes exist on every shard after comm_init
    "hostname": dict(ties=False, zones_by_range=False, spread=False, ipa=True, resident_anti=True, ports=False, pin=False),
    "everything": dict(ties=True, zones_by_range=True, spread=True, ipa=True, resident_anti=True, ports=True, pin=True),
}


def bits(rows, n):
    """[P][words] uint64 → [P][n] 0/1 (bit j % 64 of word j // 64 = node j)."""
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :n]


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    case, seed = sys.argv[1], int(sys.argv[2])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    n_nodes, n_pods = 300, 600
    snap, shards = _seqgen.sharded_mixed(seed, world, n_nodes=n_nodes, n_pods=n_pods, **CASES[case])
    ranges = sharding.shard_ranges(n_nodes, world)
    first, count = ranges[rank]
    assert len(shards[rank]) == count
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot({"nodes": shards[rank], "pods": snap["pods"]})
    pm.set_row_stride(sharding.common_row_stride(ranges))
    pm.set_row_capacity(sharding.common_row_capacity(n_pods))
    assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    t = pm.encoded_tables()
    shape = {"KD": t["KD"], "KS": t["KS"], "domains": t["domain_sizes"], "keys": t["topology_keys"]}
    shapes = [None] * world
    dist.all_gather_object(shapes, shape)
    if any(s != shapes[0] for s in shapes):
        print(f"rank {rank}/{world} {case}: topology dictionaries differ across shards: {shapes}", flush=True)
        dist.barrier()
        pm.comm_destroy()
        pm.close()
        dist.destroy_process_group()
        sys.exit(3)
    o = orc.Oracle(snap)
    want_fit = o.eval_grid(threads=8, prefilter_once=True)
    want_dec = np.array([o.decide(p, prefilter_once=True)[1] for p in range(n_pods)], dtype=np.int32)
    o.close()
    # ---- snapshot path through the C-ABI collectives
    dev = torch.device("cuda", 0)
    counts = torch.empty(n_pods, dtype=torch.int32, device=dev)
    decisions = torch.empty(n_pods, dtype=torch.int32, device=dev)
    keys = torch.empty(n_pods, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    pm.evaluate_into(counts=counts, decisions=decisions, keys=keys, stream=stream.cuda_stream)
    pm.gather_bitmap(stream=stream.cuda_stream)
    pm.exchange_decisions(stream=stream.cuda_stream)
    pm.synchronize()
    shard_rows = [pm.read_gathered(g) for g in range(world)]
    pm.gather_bitmap(stream=stream.cuda_stream, compressed=True)
    pm.synchronize()
    compressed_ok = all(np.array_equal(pm.read_gathered(g), shard_rows[g]) for g in range(world))
    got_fit = np.concatenate([bits(shard_rows[g], c) for g, (_, c) in enumerate(ranges) if c > 0], axis=1)
    rows_ok = got_fit.shape == want_fit.shape and np.array_equal(got_fit, want_fit)
    counts_ok = np.array_equal(counts.cpu().numpy(), want_fit.sum(axis=1).astype(np.int32))
    dec_ok = np.array_equal(decisions.cpu().numpy(), want_dec)
    detail = ""
    if not rows_ok and got_fit.shape == want_fit.shape:
        bad = np.argwhere(got_fit != want_fit)
        detail += f" first row difference at (ask {bad[0][0]}, node {bad[0][1]}) ({len(bad)} pairs differ)"
    if not dec_ok:
        bad = np.flatnonzero(decisions.cpu().numpy() != want_dec)
        detail += f" first decision difference at ask {bad[0]}: got {decisions.cpu().numpy()[bad[0]]} want {want_dec[bad[0]]} ({len(bad)} differ)"
    # ---- two batched rounds on top of a fresh evaluation (the exchange above rewrote the decisions in place)
    pm.evaluate(allocate=True)
    o = orc.Oracle(snap)
    want = o.allocate_sequential(prefilter_once=True)
    o.close()
    half = n_pods // 2
    asks = np.arange(n_pods, dtype=np.int32)
    before = pm.round_stats()
    got = np.concatenate([pm.allocate_round(asks=asks[:half], apply=True), pm.allocate_round(asks=asks[half:], apply=False)])
    after = pm.round_stats()
    rounds_ok = np.array_equal(got, want)
    on_device = after["rounds_on_device"] == before["rounds_on_device"] + 2 and after["asks_one_by_one"] == before["asks_one_by_one"]
    if not rounds_ok:
        bad = np.flatnonzero(got != want)
        detail += f" first round difference at ask {bad[0]}: got {got[bad[0]]} want {want[bad[0]]} ({len(bad)} differ)"
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    # ---- one collective incremental step, on fresh engines and a fresh communicator
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot({"nodes": shards[rank], "pods": snap["pods"]})
    pm.set_row_stride(sharding.common_row_stride(ranges))
    pm.set_row_capacity(sharding.common_row_capacity(n_pods))
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate(allocate=True)
    moved, used = [], set()
    for p in range(n_pods):
        if want_dec[p] >= 0 and int(want_dec[p]) not in used and len(moved) < 4:
            used.add(int(want_dec[p]))
            moved.append((snap["pods"][p]["metadata"]["uid"], snap["nodes"][int(want_dec[p])]["metadata"]["name"]))
    mine = {n["metadata"]["name"] for n in shards[rank]}
    for uid, node in moved:
        if node in mine:
            pm.assume_pod(uid, node)
    pm.evaluate_dirty(allocate=True)  # collective: every rank, changed or not
    pm.gather_bitmap()
    pm.synchronize()
    rows2 = np.concatenate([bits(pm.read_gathered(g), c) for g, (_, c) in enumerate(ranges) if c > 0], axis=1)
    changed = json.loads(json.dumps(snap))
    by_name = {n["metadata"]["name"]: n for n in changed["nodes"]}
    by_uid = {q["metadata"]["uid"]: q for q in changed["pods"]}
    for uid, node in moved:
        q = by_uid.pop(uid)
        q["spec"]["nodeName"] = node
        by_name[node]["pods"].append(q)
    changed["pods"] = [q for q in changed["pods"] if q["metadata"]["uid"] in by_uid]
    o = orc.Oracle(changed)
    want2 = o.eval_grid(threads=8, prefilter_once=True)
    o.close()
    keep = [pm.pod_index(q["metadata"]["uid"]) for q in changed["pods"]]
    incremental_ok = np.array_equal(rows2[keep], want2)
    if not incremental_ok:
        bad = np.argwhere(rows2[keep] != want2)
        detail += f" first incremental difference at (ask {keep[bad[0][0]]}, node {bad[0][1]}) ({len(bad)} pairs differ)"
    mismatch_ok = True
    if "zone" in shape["keys"]:
        if rank == 0:
            node = json.loads(json.dumps(shards[0][0]))
            node["metadata"]["labels"]["zone"] = "z-only-on-shard-0"
            pm.update_node(node)
        try:
            pm.evaluate_dirty(allocate=True)
            mismatch_ok = False
            detail += " a node update that brought a zone to one shard only was not refused"
        except RuntimeError as err:
            mismatch_ok = "do not share the topology-domain dictionaries" in str(err)
            if not mismatch_ok:
                detail += f" unexpected error: {err}"
    ok = rows_ok and counts_ok and dec_ok and compressed_ok and rounds_ok and on_device and incremental_ok and mismatch_ok
    print(f"rank {rank}/{world} {case}: rows {rows_ok} counts {counts_ok} decisions {dec_ok} compressed {compressed_ok} "
          f"rounds {rounds_ok} on_device {on_device} incremental {incremental_ok} mismatch {mismatch_ok} ({n_pods} asks x {n_nodes} nodes, "
          f"shard {count}, {int((want >= 0).sum())} allocated){detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if ok else 3)


if __name__ == "__main__":
    main()
