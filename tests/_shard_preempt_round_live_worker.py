"""Two ranks of a node-sharded cluster planning a LIVE preemption round together (ykpred_preempt_round_live on a sharded engine: the
step, the apply, then per applied turn the owner of the node fills the dense [2][G] record, ONE all-reduce SUM carries it to every rank
and every rank moves its cluster-wide copy of the histograms) against a single engine over the whole cluster. Launched by
tests/test_gpu_preempt_round_live.py through torch.distributed.run with SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared
library>: the ranks share cuda:0.

The cluster is the `victim_min` round of tests/_liveroundgen.py on 70 nodes, cut at node 35: vm-a1 (63), vm-b (64) and vm-c (69) — the
nodes every spread ask of the round is placed on but one — lie on rank 1, with their victims; rank 0 learns of the counts of zones a, b
and c only through the records. Every rank checks its cells == the single engine's == the model's, its round-local histograms == the
single engine's, and that a readback asked for on one rank only makes EVERY rank return the same error instead of blocking in a reduce."""
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
import _liveroundgen as gen  # noqa: E402
import _oracle as orc  # noqa: E402

SEED = 20266


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    assert world == 2
    snapshot, bounds, meta = gen.round_("victim_min", SEED)
    nodes, asks, turns = snapshot["nodes"], snapshot["pods"], meta["turns"]
    for i, node in enumerate(nodes):   # (shards are ranges of the name-sorted node list; the scenes select by label, not by name)
        node["metadata"]["name"] = f"{i:03d}.{node['metadata']['name']}"
    model = gen.LiveModel(snapshot, bounds)
    want_model = np.array(model.run(turns)[0], dtype=np.int64)
    ranges = [(0, 35), (35, 35)]
    first, count = ranges[rank]
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot(json.dumps({"nodes": nodes[first:first + count], "pods": asks}))
    pm.set_row_stride(sharding.common_row_stride(ranges))
    pm.set_row_capacity(sharding.common_row_capacity(len(asks)))
    assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate(allocate=True)   # collective: the topology histograms become the cluster's
    pm.set_preemption_tiers(bounds)
    got, summary, counts, minima = pm.preempt_round_live(turns, histograms=True)
    again, _ = pm.preempt_round_live(turns)
    # the agreement step: the last rank asks for no readback — every rank must come back with an error, nobody blocks
    idx = np.array([pm.pod_index(u) for u in turns], dtype=np.int32)
    limits = np.ascontiguousarray(got[:, 5], dtype=np.int32)
    out = np.zeros((len(turns), 8), dtype=np.int64)
    out_summary = np.zeros(8, dtype=np.int64)
    c2, m2 = np.zeros(max(len(counts), 1), dtype=np.int32), np.zeros(max(len(minima), 1), dtype=np.int32)
    rc = pm._P.ykpred_preempt_round_live(pm.engine, len(turns), idx.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data, out_summary.ctypes.data,
                                         None if rank == world - 1 else c2.ctypes.data, m2.ctypes.data)
    after, _ = pm.preempt_round_live(turns)   # ... and the communicator is still in step afterwards
    # the whole cluster on one engine
    full = pkg.GpuPredicateManager(device=0)
    full.load_snapshot(json.dumps(snapshot))
    full.set_preemption_tiers(bounds)
    want, want_summary, want_counts, want_minima = full.preempt_round_live(turns, histograms=True)
    full.close()
    remote = sum(1 for r in want if r[1] >= 35)
    cells_ok = (np.array_equal(got, want) and np.array_equal(again, want) and np.array_equal(after, want) and np.array_equal(want, want_model)
                and summary.tolist() == want_summary.tolist() and summary[7] > 0 and remote >= 5)
    hist_ok = np.array_equal(counts, want_counts) and np.array_equal(minima, want_minima) and len(counts) > 0
    ok = cells_ok and hist_ok and rc == -1
    detail = "" if ok else f" rc {rc} got {got.tolist()} want {want.tolist()} summary {summary.tolist()} {want_summary.tolist()} counts {counts.tolist()} {want_counts.tolist()}"
    print(f"rank {rank}/{world}: cells {cells_ok} histograms {hist_ok} agreement {rc == -1}{detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if ok else 3)


if __name__ == "__main__":
    main()
