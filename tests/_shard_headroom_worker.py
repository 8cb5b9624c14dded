"""Ranks of a node-sharded cluster answering "how many copies of this ask still fit" together (ykpred_headroom on a sharded engine:
every shard reduces its own nodes, one all-reduce SUM of the [tasks][16] table and one all-reduce MAX of the [tasks] maxima, every rank
returns cluster-wide cells) against a single engine over the WHOLE cluster. Launched by tests/test_gpu_headroom.py through
torch.distributed.run.

  SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>: the ranks share cuda:0 and the engine loads the stub instead of
  librccl (ykpred_comm_use_library); with >= world GPUs visible and no stub: one GPU per rank over RCCL.
Every rank checks: its cells == the single engine's for EVERY ask (all asks, then a shuffled subset with repeats); cell [2] is the
maximum — not the sum — of the shards' own maxima, which it gathers through headroom_nodes (this shard's nodes only); and — the
agreement step in front of the reduces — that a rank handing in a different list makes EVERY rank return an error instead of blocking."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("yunikorn-k8shim_amd")
sharding = importlib.import_module("yunikorn-k8shim_amd.sharding")


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    total_nodes, n_pods, n_templates, spread = (int(a) for a in sys.argv[1:5])
    stub = os.environ.get("SHARD_RCCL_STUB")
    device = 0 if stub else rank
    torch.cuda.set_device(device)
    dist.init_process_group("gloo")
    kw = dict(seed=0x59554E49 + 123, num_pods=n_pods, num_templates=n_templates, node_affinity=1, spread=spread)
    ranges = sharding.shard_ranges(total_nodes, world)
    first, count = ranges[rank]
    pm = pkg.GpuPredicateManager(device=device)
    pm.generate_kwok(num_nodes=count, node_index_offset=first, total_nodes=total_nodes, **kw)
    if stub:
        assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate()  # (collective: the topology histograms a coupled ask's fit count reads become cluster-wide)
    got = pm.headroom()
    rng = np.random.default_rng(5)  # the same list on every rank
    pick = rng.integers(0, n_pods, size=min(n_pods, 97)).astype(np.int32)
    got_pick = pm.headroom(pick)
    # the agreement step: the last rank hands in a list with one ask replaced — every rank must come back with an error, nobody blocks
    other = pick.copy()
    other[3] = (other[3] + 1) % n_pods
    errors = 0
    try:
        pm.headroom(other if rank == world - 1 else pick)
    except RuntimeError:
        errors = 1
    again = pm.headroom(pick)  # ... and the communicator is still in step afterwards
    # the shards' own maxima of three computed asks: the cluster's [2] is their maximum
    probes = [int(p) for p in np.flatnonzero((got[:, pkg.HEADROOM_STATUS] == 0) & (got[:, pkg.HEADROOM_NODES] > 0))[:3]]
    mine = torch.tensor([int(pm.headroom_nodes(p).max()) for p in probes] + [0] * (3 - len(probes)), dtype=torch.int64)
    mine_sum = torch.tensor([int(pm.headroom_nodes(p).sum()) for p in probes] + [0] * (3 - len(probes)), dtype=torch.int64)
    top = mine.clone()
    dist.all_reduce(top, op=dist.ReduceOp.MAX)
    dist.all_reduce(mine_sum, op=dist.ReduceOp.SUM)
    maxima = all(int(got[p, pkg.HEADROOM_MAX]) == int(top[k]) and int(got[p, pkg.HEADROOM_TOTAL]) == int(mine_sum[k]) for k, p in enumerate(probes))
    # the whole cluster on one engine
    full = pkg.GpuPredicateManager(device=device)
    full.generate_kwok(num_nodes=total_nodes, **kw)
    want = full.headroom()
    full.close()
    ok = got.shape == want.shape and np.array_equal(got, want) and np.array_equal(got_pick, want[pick]) and np.array_equal(again, want[pick])
    computed = want[want[:, pkg.HEADROOM_STATUS] == 0]
    sums = bool((computed[:, 4] + computed[:, 5] + computed[:, 8:].sum(axis=1) == computed[:, 1]).all() and len(probes) == 3
                and (spread == 0 or (want[:, 3] == 2).any()))  # (with spread constraints some asks are coupled, on every rank alike)
    bad = np.flatnonzero((got != want).any(axis=1)) if got.shape == want.shape else np.array([-1])
    detail = "" if ok else f" first difference at ask {bad[0] if len(bad) else 'subset'}: {got[bad[0]].tolist() if len(bad) else ''} != {want[bad[0]].tolist() if len(bad) else ''}"
    print(f"rank {rank}/{world} {'rccl-stub' if stub else 'rccl'}: headroom {ok} sums {sums} maxima {maxima} mismatch {errors == 1} "
          f"({n_pods} asks x {total_nodes} nodes, {len(computed)} computed, {int((want[:, 3] == 2).sum())} coupled, "
          f"largest total {int(want[:, 0].max())}){detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (ok and sums and maxima and errors == 1) else 3)


if __name__ == "__main__":
    main()
