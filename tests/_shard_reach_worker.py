"""Two ranks of a node-sharded cluster answering preemption reach together (ykpred_preempt_reach on a sharded engine: every shard walks
its own nodes, ONE all-reduce sums the cells, ONE all-reduce takes the minimum of the packed best-node keys, every rank returns
cluster-wide cells with a GLOBAL best-node index) against a single engine over the whole cluster. Launched by
tests/test_gpu_preempt_reach.py through torch.distributed.run with SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>:
the ranks share cuda:0.

The cluster (global node order; rank 0 holds the first two nodes, rank 1 the last two):
  s0-high   nothing free, two 100m residents in tier 2, 1 byte of memory      s0-low   nothing free, one 100m resident in tier 0, 1 byte
  s1-low    nothing free, one 100m resident in tier 0, 8 bytes of memory      s1-two   nothing free, two 50m residents in tier 0, 8 bytes
  a-tie     100m:            level 1 with one victim on s0-low AND on s1-low — the tie across shards goes to the lower global index
  a-remote  100m + 8 bytes:  only rank 1's nodes can take it: for rank 0 the curing tier's pods and the best node sit wholly on the other
                             shard; s1-low (one victim) beats s1-two (two)
  a-low     100m, limit 0:   never anywhere
Every rank checks its cells == the single engine's for every ask, the best nodes by index, its own per-node levels, and that a limit
list that differs on one rank makes EVERY rank return the same error instead of blocking in the reduce."""
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
from _preemptgen import make_node  # noqa: E402
from _reachgen import BOUNDS, NEVER, asker, victim  # noqa: E402


def cluster():
    b = BOUNDS[3]
    nodes = [make_node("s0-high", {"cpu": 200, "memory": 1}, [victim(f"s0-high-r{i}", b, 2, {"cpu": 100}) for i in range(2)]),
             make_node("s0-low", {"cpu": 100, "memory": 1}, [victim("s0-low-r", b, 0, {"cpu": 100})]),
             make_node("s1-low", {"cpu": 100, "memory": 8}, [victim("s1-low-r", b, 0, {"cpu": 100})]),
             make_node("s1-two", {"cpu": 100, "memory": 8}, [victim(f"s1-two-r{i}", b, 0, {"cpu": 50}) for i in range(2)])]
    asks = [asker("a-tie", b, 3, {"cpu": 100}), asker("a-remote", b, 3, {"cpu": 100, "memory": 8}), asker("a-low", b, 0, {"cpu": 100})]
    return nodes, asks, list(b)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    assert world == 2
    nodes, asks, bounds = cluster()
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
    got = pm.preempt_reach()
    again = pm.preempt_reach([2, 0, 0, 1])
    levels = np.array([pm.preempt_reach_nodes(a) for a in range(len(asks))])
    # the agreement step: the last rank hands in another limit for one ask — every rank must come back with an error, nobody blocks
    idx = np.arange(len(asks), dtype=np.int32)
    limits = np.ascontiguousarray(got[:, 11], dtype=np.int32)
    if rank == world - 1:
        limits[0] -= 1
    out = np.zeros((len(asks), 16), dtype=np.int64)
    rc = pm._P.ykpred_preempt_reach(pm.engine, len(asks), idx.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data)
    after = pm.preempt_reach()   # ... and the communicator is still in step afterwards
    # the whole cluster on one engine
    full = pkg.GpuPredicateManager(device=0)
    full.load_snapshot({"nodes": nodes, "pods": asks})
    full.set_preemption_tiers(bounds)
    want = full.preempt_reach()
    want_levels = np.array([full.preempt_reach_nodes(a) for a in range(len(asks))])
    full.close()
    cells_ok = np.array_equal(got, want) and np.array_equal(again, want[[2, 0, 0, 1]]) and np.array_equal(after, want) and bool((got[:, :10].sum(axis=1) == 4).all())
    # a-tie: level 1, one victim, global node 1 (s0-low, not s1-low); a-remote: global node 2 (s1-low); a-low: no node
    best_ok = got[0, 12:15].tolist() == [1, 1, 1] and got[1, 12:15].tolist() == [1, 2, 1] and got[2, 12:15].tolist() == [0, -1, 0]
    levels_ok = np.array_equal(levels, want_levels[:, first:first + count]) and want_levels.tolist() == [[3, 1, 1, 1], [NEVER, NEVER, 1, 1], [NEVER] * 4]
    detail = "" if cells_ok and best_ok and levels_ok else f" got {got.tolist()} want {want.tolist()} levels {levels.tolist()}"
    print(f"rank {rank}/{world}: cells {cells_ok} best {best_ok} levels {levels_ok} mismatch {rc == -1}{detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (cells_ok and best_ok and levels_ok and rc == -1) else 3)


if __name__ == "__main__":
    main()
