"""Two ranks of a node-sharded cluster planning a preemption round together (ykpred_preempt_round on a sharded engine: per ask every
shard steps over its own nodes, ONE all-reduce takes the minimum of the packed key, ONE sums the two counts, every rank applies the same
decision and the owning shard moves its state) against a single engine over the whole cluster. Launched by
tests/test_gpu_preempt_round.py through torch.distributed.run with SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>:
the ranks share cuda:0.

The cluster of tests/_shard_victims_worker.py (global node order; rank 0 holds the first two nodes, rank 1 the last two), every resident
in tier 0, nothing free:
  s0-many   four 50m residents, 1 byte of memory        s0-pair   two 100m residents, 1 byte
  s1-pair   two 100m residents, 8 bytes of memory       s1-five   five 20m residents, 8 bytes
The round, in order:
  a-tie     200m: extra 2 on s0-pair AND on s1-pair — the tie across shards goes to the lower global index 1
  a-tie     again: s0-pair has nobody left; s1-pair (extra 2, global 2) beats s0-many (extra 4): for rank 0 the node sits wholly on the
            other shard
  a-routed  a persistent volume claim: the ENGINE settles it (outcome 3: on a sharded handle every ask goes to the engine), no step, no
            reduce, on either rank; its neighbours are unchanged
  a-remote  100m + 8 bytes: only rank 1's nodes have the memory. s1-pair would cost one victim — but the second ask sits there now, with
            both victims taken: rank 0 learns of that placement only through the round; the ask goes to s1-five with five victims
  a-low     100m, limit 0: nowhere
Every rank checks its cells == the single engine's == the plan above, and that a limit list that differs on one rank makes EVERY rank
return the same error instead of blocking in a reduce."""
import importlib
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
from _reachgen import asker  # noqa: E402
from _shard_victims_worker import cluster  # noqa: E402

TURNS = ["a-tie", "a-tie", "a-routed", "a-remote", "a-low"]
PLAN = [[1, 1, 0, 2, 1, 3, 3, 8], [1, 2, 0, 2, 1, 3, 2, 6], [3, -1, 0, 0, 0, 3, 0, 0], [1, 3, 0, 5, 1, 3, 1, 5], [2, -1, 0, 0, 0, 0, 0, 0]]


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    assert world == 2
    nodes, asks, bounds = cluster()
    asks.append(asker("a-routed", bounds, 3, {"cpu": 100}, volumes=[{"name": "data", "persistentVolumeClaim": {"claimName": "pvc-1"}}]))
    ranges = [(0, 2), (2, 2)]
    first, count = ranges[rank]
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot({"nodes": nodes[first:first + count], "pods": asks})
    pm.set_row_stride(sharding.common_row_stride(ranges))
    pm.set_row_capacity(sharding.common_row_capacity(len(asks)))
    assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate(allocate=True)   # collective: the topology histograms become the cluster's
    pm.set_preemption_tiers(bounds)
    got, summary = pm.preempt_round(TURNS)
    again, _ = pm.preempt_round(TURNS)
    # the agreement step: the last rank hands in another limit for one ask — every rank must come back with an error, nobody blocks
    idx = np.array([pm.pod_index(u) for u in TURNS], dtype=np.int32)
    limits = np.ascontiguousarray(got[:, 5], dtype=np.int32)
    if rank == world - 1:
        limits[0] -= 1
    out = np.zeros((len(TURNS), 8), dtype=np.int64)
    out_summary = np.zeros(8, dtype=np.int64)
    rc = pm._P.ykpred_preempt_round(pm.engine, len(TURNS), idx.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data, out_summary.ctypes.data)
    after, _ = pm.preempt_round(TURNS)   # ... and the communicator is still in step afterwards
    # the whole cluster on one engine
    full = pkg.GpuPredicateManager(device=0)
    full.load_snapshot({"nodes": nodes, "pods": asks})
    full.set_preemption_tiers(bounds)
    want, want_summary = full.preempt_round(TURNS)
    full.close()
    cells_ok = (np.array_equal(got, want) and np.array_equal(again, want) and np.array_equal(after, want)
                and summary.tolist() == want_summary.tolist() == [0, 3, 1, 1, 0, 9, 3, 0])
    plan_ok = got.tolist() == PLAN
    ok = cells_ok and plan_ok and rc == -1
    detail = "" if ok else f" rc {rc} got {got.tolist()} want {want.tolist()} summary {summary.tolist()}"
    print(f"rank {rank}/{world}: cells {cells_ok} plan {plan_ok} agreement {rc == -1}{detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if ok else 3)


if __name__ == "__main__":
    main()
