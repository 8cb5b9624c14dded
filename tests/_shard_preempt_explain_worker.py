"""Two ranks of a node-sharded cluster answering preemption explain together (ykpred_preempt_explain on a sharded engine: every shard
walks its own nodes, ONE all-reduce sums the cells, every rank returns cluster-wide cells) against a single engine over the whole
cluster. Launched by tests/test_gpu_preempt_explain.py through torch.distributed.run with SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built
as a shared library>: the ranks share cuda:0.

The cluster (global node order; rank 0 holds the first two nodes, rank 1 the last three):
  s0-bare   nothing free, nobody on it                       s0-kept   nothing free, one 100m resident in no tier
  s1-cure   nothing free, one 100m resident in tier 0        s1-short  nothing free, one 40m resident in tier 0, one 60m in no tier
  s1-slots  full by pod count, one zero-request pod in tier 1, two in no tier, allowed 2
  a-100     100m, limit 3:  for rank 0 the curing tier's pods AND the not-enough nodes sit wholly on the other shard — its own nodes
                            are no-victims nodes; s1-cure is at level 1, s1-short and s1-slots are not enough (cpu; too many pods)
  a-low     100m, limit 0:  never anywhere, nothing eligible
  a-tiny    1m, limit 1:    s1-slots' pod sits in tier 1: no victims there for this limit
Every rank checks its cells == the single engine's for every ask, its own per-node words, and that a limit list that differs on one rank
makes EVERY rank return the same error instead of blocking in the reduce."""
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
from _reachgen import BOUNDS, asker, victim  # noqa: E402


def cluster():
    b = BOUNDS[3]
    mem = {"memory": 1 << 30}
    nodes = [make_node("s0-bare", dict(mem, cpu=10), []),
             make_node("s0-kept", dict(mem, cpu=100), [victim("s0-kept-r", b, 3, {"cpu": 100})]),
             make_node("s1-cure", dict(mem, cpu=100), [victim("s1-cure-r", b, 0, {"cpu": 100})]),
             make_node("s1-short", dict(mem, cpu=100), [victim("s1-short-r", b, 0, {"cpu": 40}), victim("s1-short-k", b, 3, {"cpu": 60})]),
             make_node("s1-slots", dict(mem, cpu=1000), [victim("s1-slots-r", b, 1, {})] + [victim(f"s1-slots-k{i}", b, 3, {}) for i in range(2)], allowed=2)]
    asks = [asker("a-100", b, 3, {"cpu": 100}), asker("a-low", b, 0, {"cpu": 100}), asker("a-tiny", b, 1, {"cpu": 1})]
    return nodes, asks, list(b)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    assert world == 2
    nodes, asks, bounds = cluster()
    ranges = [(0, 2), (2, 3)]
    first, count = ranges[rank]
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot({"nodes": nodes[first:first + count], "pods": asks})
    pm.set_row_stride(sharding.common_row_stride(ranges))
    pm.set_row_capacity(sharding.common_row_capacity(len(asks)))
    assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate(allocate=True)   # collective: the topology histograms become the cluster's
    pm.set_preemption_tiers(bounds)
    got = pm.preempt_explain()
    again = pm.preempt_explain([2, 0, 0, 1])
    words = np.array([pm.preempt_explain_nodes(a) for a in range(len(asks))])
    # the agreement step: the last rank hands in another limit for one ask — every rank must come back with an error, nobody blocks
    idx = np.arange(len(asks), dtype=np.int32)
    limits = np.ascontiguousarray(got[:, 29], dtype=np.int32)
    if rank == world - 1:
        limits[0] -= 1
    out = np.zeros((len(asks), 32), dtype=np.int64)
    rc = pm._P.ykpred_preempt_explain(pm.engine, len(asks), idx.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data)
    after = pm.preempt_explain()   # ... and the communicator is still in step afterwards
    # the whole cluster on one engine
    full = pkg.GpuPredicateManager(device=0)
    full.load_snapshot({"nodes": nodes, "pods": asks})
    full.set_preemption_tiers(bounds)
    want = full.preempt_explain()
    want_words = np.array([full.preempt_explain_nodes(a) for a in range(len(asks))])
    full.close()
    cells_ok = np.array_equal(got, want) and np.array_equal(again, want[[2, 0, 0, 1]]) and np.array_equal(after, want) and bool((got[:, :12].sum(axis=1) == 5).all())
    # a-100: s1-cure opens; two no-victims nodes (rank 0's), two not-enough nodes (rank 1's) short of cpu / of a slot, 1 + 1 wasted pods
    design_ok = (got[0, [6, 11, 24, 25, 26, 28]].tolist() == [4, 1, 2, 0, 2, 2] and got[0, 12] == 1 and got[0, 16] == 1
                 and got[1, [6, 24, 26]].tolist() == [5, 5, 0] and got[2, [6, 9, 11, 24, 26]].tolist() == [2, 1, 2, 2, 0])
    words_ok = np.array_equal(words, want_words[:, first:first + count])
    detail = "" if cells_ok and design_ok and words_ok else f" got {got.tolist()} want {want.tolist()} words {words.tolist()}"
    print(f"rank {rank}/{world}: cells {cells_ok} design {design_ok} words {words_ok} mismatch {rc == -1}{detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (cells_ok and design_ok and words_ok and rc == -1) else 3)


if __name__ == "__main__":
    main()
