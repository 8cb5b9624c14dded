"""Two ranks of a node-sharded cluster answering preemption victims together (ykpred_preempt_victims on a sharded engine: every shard
bisects its own nodes, ONE all-reduce sums the cells, ONE all-reduce takes the minimum of the packed best-node keys, every rank returns
cluster-wide cells with a GLOBAL best-node index) against a single engine over the whole cluster. Launched by
tests/test_gpu_preempt_victims.py through torch.distributed.run with SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>:
the ranks share cuda:0.

The cluster (global node order; rank 0 holds the first two nodes, rank 1 the last two), every resident in tier 0, nothing free:
  s0-many   four 50m residents, 1 byte of memory        s0-pair   two 100m residents, 1 byte
  s1-pair   two 100m residents, 8 bytes of memory       s1-five   five 20m residents, 8 bytes
  a-tie     200m:            need 2 on s0-pair AND on s1-pair (4 on s0-many, never on s1-five) — the tie across shards goes to the lower
                             global index; [8] = 2 + 2 + 4 sums victims of both shards
  a-remote  100m + 8 bytes:  only rank 1's nodes can take it: for rank 0 the best node sits wholly on the other shard; s1-pair (one
                             victim) beats s1-five (five)
  a-low     100m, limit 0:   never anywhere
Every rank checks its cells == the single engine's for every ask, the best nodes by index, its own per-node needs, and that a limit list
that differs on one rank makes EVERY rank return the same error instead of blocking in the reduce."""
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
    nodes = [make_node("s0-many", {"cpu": 200, "memory": 1}, [victim(f"s0-many-r{i}", b, 0, {"cpu": 50}) for i in range(4)]),
             make_node("s0-pair", {"cpu": 200, "memory": 1}, [victim(f"s0-pair-r{i}", b, 0, {"cpu": 100}) for i in range(2)]),
             make_node("s1-pair", {"cpu": 200, "memory": 8}, [victim(f"s1-pair-r{i}", b, 0, {"cpu": 100}) for i in range(2)]),
             make_node("s1-five", {"cpu": 100, "memory": 8}, [victim(f"s1-five-r{i}", b, 0, {"cpu": 20}) for i in range(5)])]
    asks = [asker("a-tie", b, 3, {"cpu": 200}), asker("a-remote", b, 3, {"cpu": 100, "memory": 8}), asker("a-low", b, 0, {"cpu": 100})]
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
    got = pm.preempt_victims()
    again = pm.preempt_victims([2, 0, 0, 1])
    needs = np.array([pm.preempt_victims_nodes(a) for a in range(len(asks))])
    # the agreement step: the last rank hands in another limit for one ask — every rank must come back with an error, nobody blocks
    idx = np.arange(len(asks), dtype=np.int32)
    limits = np.ascontiguousarray(got[:, 4], dtype=np.int32)
    if rank == world - 1:
        limits[0] -= 1
    out = np.zeros((len(asks), 16), dtype=np.int64)
    rc = pm._P.ykpred_preempt_victims(pm.engine, len(asks), idx.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data)
    after = pm.preempt_victims()   # ... and the communicator is still in step afterwards
    # the whole cluster on one engine
    full = pkg.GpuPredicateManager(device=0)
    full.load_snapshot({"nodes": nodes, "pods": asks})
    full.set_preemption_tiers(bounds)
    want = full.preempt_victims()
    want_needs = np.array([full.preempt_victims_nodes(a) for a in range(len(asks))])
    full.close()
    cells_ok = (np.array_equal(got, want) and np.array_equal(again, want[[2, 0, 0, 1]]) and np.array_equal(after, want)
                and bool((got[:, :3].sum(axis=1) == 4).all()) and got[:, 8].tolist() == [8, 6, 0])
    # a-tie: level 1, need 2, global node 1 (s0-pair, not s1-pair); a-remote: global node 2 (s1-pair, need 1); a-low: no node
    best_ok = got[0, 5:8].tolist() == [1, 1, 2] and got[1, 5:8].tolist() == [1, 2, 1] and got[2, 5:8].tolist() == [0, -1, 0]
    needs_ok = np.array_equal(needs, want_needs[:, first:first + count]) and want_needs.tolist() == [[4, 2, 2, NEVER], [NEVER, NEVER, 1, 5], [NEVER] * 4]
    detail = "" if cells_ok and best_ok and needs_ok and rc == -1 else f" rc {rc} got {got.tolist()} want {want.tolist()} needs {needs.tolist()}"
    print(f"rank {rank}/{world}: cells {cells_ok} best {best_ok} needs {needs_ok}{detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (cells_ok and best_ok and needs_ok and rc == -1) else 3)


if __name__ == "__main__":
    main()
