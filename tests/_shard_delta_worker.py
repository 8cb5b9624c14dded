"""Two ranks of a node-sharded cluster at the limit of a delta record (kDeltaMax = 10 histogram cells per assumed pod), launched by
tests/test_gpu_rounds_designed.py through torch.distributed.run like tests/_shard_round_worker.py (SHARD_RCCL_STUB: the ranks share
cuda:0, the collectives go through tests/c/rccl_stub.cpp). The cluster is tests/_roundgen.py many_constraints(10, extra_label=True) on 192 nodes (shards of 128 and 64):
  round 1 (apply = 1)  asks whose pods add to exactly 10 cells: every decision equals the oracle's loop over the whole cluster;
  round 2 (apply = 0)  asks whose pods add to 11: every rank gets the engine's refusal (YKPRED_E_UNSUPPORTED), nothing else;
  round 3 (apply = 0)  asks that add to none, on top of round 1: equal to the oracle again."""
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
import _roundgen  # noqa: E402


YKHOST_E_UNSUPPORTED = -13  # include/ykhost.h


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    snap, meta = _roundgen.many_constraints(_roundgen.DELTA_MAX, extra_label=True, n_nodes=_roundgen.DELTA_NODES)
    n_nodes, n_pods = len(snap["nodes"]), len(snap["pods"])
    ranges = sharding.shard_ranges(n_nodes, world)
    first, count = ranges[rank]
    assert count > 0, "a rank without nodes: shards are cut at multiples of 64"
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot({"nodes": snap["nodes"][first:first + count], "pods": snap["pods"]})
    pm.set_row_stride(sharding.common_row_stride(ranges))
    pm.set_row_capacity(sharding.common_row_capacity(n_pods))
    assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate(allocate=True)  # (collective: the rounds start from a current evaluation on every rank)
    asks = np.arange(n_pods, dtype=np.int32)
    ten, eleven, none = asks[:meta["extra_from"]], asks[meta["extra_from"]:meta["plain_from"]], asks[meta["plain_from"]:]
    o = orc.Oracle(snap)
    want1 = o.allocate_sequential(pods=ten, prefilter_once=True)
    want3 = o.allocate_sequential(pods=none, prefilter_once=True)  # (on top of round 1; round 2 is never applied)
    o.close()
    before = pm.round_stats()
    errors = []
    got1 = got3 = np.zeros(0, dtype=np.int32)
    try:
        got1 = pm.allocate_round(asks=ten, apply=True)
    except RuntimeError as err:
        errors.append(f"round of ten cells raised: {err}")
    # (the C call itself: its return code is the refusal the Go side routes on)
    arr, out = np.ascontiguousarray(eleven, dtype=np.int32), np.full(len(eleven), -1, dtype=np.int32)
    code = pm._L.ykhost_allocate_round(pm._h, len(arr), arr.ctypes.data, 0, out.ctypes.data)
    message = pm._L.ykhost_last_error(pm._h).decode() if code < 0 else ""
    refused = code == YKHOST_E_UNSUPPORTED and "more histogram cells than a delta record holds (10)" in message
    try:
        got3 = pm.allocate_round(asks=none, apply=False)
    except RuntimeError as err:
        errors.append(f"round behind the refusal raised: {err}")
    after = pm.round_stats()
    ten_ok, after_ok = np.array_equal(got1, want1), np.array_equal(got3, want3)
    on_device = after["rounds_on_device"] == before["rounds_on_device"] + 2 and after["asks_one_by_one"] == before["asks_one_by_one"]
    detail = "".join(" " + e for e in errors)
    for name, got, want in (("ten", got1, want1), ("after", got3, want3)):
        bad = np.flatnonzero(got != want) if len(got) == len(want) else np.zeros(0, dtype=np.int64)
        if bad.size:
            detail += f" {name}: first difference at ask {bad[0]}: got {got[bad[0]]} want {want[bad[0]]} ({bad.size} differ)"
    if not refused:
        detail += f" eleven cells were not refused as expected: code {code} {message!r}"
    print(f"rank {rank}/{world} delta limit: ten {ten_ok} eleven_refused {refused} after {after_ok} on_device {on_device} "
          f"({int((want1 >= 0).sum())} + {int((want3 >= 0).sum())} allocated){detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (ten_ok and refused and after_ok and on_device) else 3)


if __name__ == "__main__":
    main()
