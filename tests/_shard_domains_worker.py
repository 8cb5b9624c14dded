"""Ranks of a node-sharded cluster answering "which domain still takes the gang" together (ykpred_headroom_groups on a sharded engine:
every shard sums its own nodes per cluster-wide group id, one all-reduce SUM per table chunk, the summaries derived after it) against a
single engine over the WHOLE cluster. Launched by tests/test_gpu_domain_headroom.py through torch.distributed.run.

  SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>: the ranks share cuda:0 and the engine loads the stub instead of
  librccl (ykpred_comm_use_library); with >= world GPUs visible and no stub: one GPU per rank over RCCL.
Groups: blocks of BLOCK consecutive GLOBAL node indices — most groups lie wholly on one shard, so every rank sums groups none of whose
nodes it holds — and, through the host library, the zone label (every shard unites the value lists first). Every rank checks: rows and
summaries == the single engine's for every ask at two wants, in three table chunks; some group with copies lies wholly on another shard
and some ask's tightest group does; and — the agreement step — that a rank handing in another want makes EVERY rank return an error."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["YKPRED_TUNE"] = "group_chunk_tasks=" + sys.argv[4]
pkg = importlib.import_module("yunikorn-k8shim_amd")
sharding = importlib.import_module("yunikorn-k8shim_amd.sharding")
BLOCK = 37
ZONE = "topology.kubernetes.io/zone"


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    total_nodes, n_pods, n_templates = (int(a) for a in sys.argv[1:4])
    stub = os.environ.get("SHARD_RCCL_STUB")
    device = 0 if stub else rank
    torch.cuda.set_device(device)
    dist.init_process_group("gloo")
    kw = dict(seed=0x59554E49 + 321, num_pods=n_pods, num_templates=n_templates, node_affinity=1, spread=0)
    first, count = sharding.shard_ranges(total_nodes, world)[rank]
    pm = pkg.GpuPredicateManager(device=device)
    pm.generate_kwok(num_nodes=count, node_index_offset=first, total_nodes=total_nodes, **kw)
    if stub:
        assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    G = (total_nodes + BLOCK - 1) // BLOCK
    mine = (first + np.arange(count, dtype=np.int32)) // BLOCK
    mine[(first + np.arange(count)) % 29 == 5] = -1  # some nodes in no group, on every shard
    # the whole cluster on one engine
    full = pkg.GpuPredicateManager(device=device)
    full.generate_kwok(num_nodes=total_nodes, **kw)
    whole = np.arange(total_nodes, dtype=np.int32) // BLOCK
    whole[np.arange(total_nodes) % 29 == 5] = -1
    ones, rows1 = full.headroom_domains(node_group=whole, num_groups=G, groups=True)
    middle = np.maximum(1, np.sort(rows1[:, :G, 0], axis=1)[:, G // 2])  # per ask: a want that half of the groups hold
    want_mid, want_rows = full.headroom_domains(node_group=whole, num_groups=G, want=middle, groups=True)
    zone_want, zone_rows = full.headroom_domains(label_key=ZONE, want=3, groups=True)
    zones = full.domain_values(ZONE)
    full.close()
    got1, got_rows1 = pm.headroom_domains(node_group=mine, num_groups=G, groups=True)
    got_mid, got_rows_mid = pm.headroom_domains(node_group=mine, num_groups=G, want=middle, groups=True)
    only = pm.headroom_domains(node_group=mine, num_groups=G, want=middle)  # (summaries alone: no table comes back)
    ok = (np.array_equal(got1, ones) and np.array_equal(got_rows1, rows1) and np.array_equal(got_mid, want_mid)
          and np.array_equal(got_rows_mid, want_rows) and np.array_equal(only, want_mid))
    got_zone, got_zone_rows = pm.headroom_domains(label_key=ZONE, want=3, groups=True)
    by_key = pm.domain_values(ZONE) == zones and np.array_equal(got_zone, zone_want) and np.array_equal(got_zone_rows, zone_rows)
    # groups none of whose nodes this shard holds: some take copies, and some ask's tightest group is one of them
    here = np.zeros(G, dtype=bool)
    here[mine[mine >= 0]] = True
    computed = got_mid[:, 0] == 0
    elsewhere = bool((got_rows_mid[computed][:, :G, 0][:, ~here] > 0).any())
    tight = got_mid[computed & (got_mid[:, 5] >= 0), 5]
    tight_elsewhere = bool(len(tight) and (~here[tight]).any())
    # the agreement step: the last rank asks for another want — every rank must come back with an error, nobody blocks
    other = middle.copy()
    other[1] += 1
    errors = 0
    try:
        pm.headroom_domains(node_group=mine, num_groups=G, want=other if rank == world - 1 else middle)
    except RuntimeError:
        errors = 1
    again = pm.headroom_domains(node_group=mine, num_groups=G, want=middle)  # ... and the communicator is still in step afterwards
    ok = ok and np.array_equal(again, want_mid)
    print(f"rank {rank}/{world} {'rccl-stub' if stub else 'rccl'}: domains {ok} by-key {by_key} elsewhere {elsewhere} tightest-elsewhere "
          f"{tight_elsewhere} mismatch {errors == 1} ({n_pods} asks x {total_nodes} nodes, {G} groups, {int(computed.sum())} computed, "
          f"{len(zones)} zones)", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (ok and by_key and elsewhere and tight_elsewhere and errors == 1) else 3)


if __name__ == "__main__":
    main()
