"""Ranks of a node-sharded cluster answering "how many copies of an ask with a hard spread constraint still fit" together
(ykpred_headroom_spread on a sharded engine: every shard sums cap and nodes of its own nodes per cluster-wide domain id, one all-reduce
SUM per table chunk over table and flags, the copies derived after it from the cluster-wide histograms) against a single engine over the
WHOLE cluster and the model of tests/_spreadgen.py. Launched by tests/test_gpu_spread_headroom.py through torch.distributed.run.

  SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>: the ranks share cuda:0 and the engine loads the stub instead of
  librccl (ykpred_comm_use_library).
The key "b" labels blocks of up to 32 consecutive nodes of ONE shard: every domain lies wholly on one of the two shards. Every rank checks: its
cells == the single engine's == the model's for every ask, in two table chunks; the rows of two asks; for some ask the domain that pins
the floor holds none of this rank's nodes; an ask that does not match itself (the fill reads minv); and that a rank handing in another list makes EVERY rank return an error."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["YKPRED_TUNE"] = "group_chunk_tasks=7"
pkg = importlib.import_module("yunikorn-k8shim_amd")
sharding = importlib.import_module("yunikorn-k8shim_amd.sharding")
import _spreadgen as sg  # noqa: E402

N, BLOCK, EXTRA = 200, 32, 11


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    ranges = sharding.shard_ranges(N, world)

    def block(i):
        g = max(k for k, (f, _) in enumerate(ranges) if f <= i)
        return f"b{g}{(i - ranges[g][0]) // BLOCK}"
    c = sg.case("shard", N, key="b", label=block, tolerate=True, req={"cpu": 900}, max_skew=2, extra_asks=EXTRA,
                seeded=lambda i: 1 if (i % 31 == 4 or i == 110) else 0)
    # ... and one ask whose selector matches the resident pods, not itself: its fill reads minv, reduced across the shards
    res = sg.case("shard-res", N, key="b", label=block, tolerate=True, req={"cpu": 700}, max_skew=3, app="res",
                  seeded=lambda i: 1 if (i % 31 == 4 or i == 110) else 0)
    assert res["snapshot"]["nodes"] == c["snapshot"]["nodes"]
    c["snapshot"]["pods"].append(res["snapshot"]["pods"][0])
    P = 2 + EXTRA
    first, count = ranges[rank]
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot({"nodes": c["snapshot"]["nodes"][first:first + count], "pods": c["snapshot"]["pods"]})
    assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate()  # (collective: the topology histograms become cluster-wide)
    got = pm.headroom_spread()
    probe = [0, P - 2, P - 1]
    got_rows = [pm.headroom_spread_domains(j, pre_mask=pm._masks[1], filt_mask=pm._masks[3])[1] for j in probe]
    # the agreement step: the last rank hands in another list
    errors = 0
    try:
        pm.headroom_spread([0, 1] if rank == world - 1 else [0, 2])
    except RuntimeError:
        errors = 1
    again = pm.headroom_spread()
    # the whole cluster on one engine, and the model
    full = pkg.GpuPredicateManager(device=0)
    full.load_snapshot(c["snapshot"])
    want = full.headroom_spread()
    want_rows = [full.headroom_spread_domains(j)[1] for j in probe]
    kd = full.encoded_tables()["topology_keys"].index("b")
    full.close()
    ok = np.array_equal(got, want) and np.array_equal(again, want) and bool((want[:, 3] == 0).all())
    models = [sg.model(c, j) for j in range(P - 1)] + [sg.model(res)]
    res_ok = want[P - 1, 7] == -1 and want[P - 1, 6] > 0 and 0 < want[P - 1, 0] < want[P - 1, 4]  # (minv above 0, some domain shut by it)
    model_ok = all(want[j].tolist() == models[j][1][:12] + [kd] + models[j][1][13:] for j in range(P))
    rows_ok = all(np.array_equal(a, b) and a.tolist() == models[j][0] for a, b, j in zip(got_rows, want_rows, probe))
    values = sg.domain_values(c)
    mine = {values.index(v) for v in c["labels"][first:first + count]}
    pinned = [int(want[j, 7]) for j in range(P) if want[j, 7] >= 0]
    elsewhere = any(d not in mine for d in pinned) and len(mine) < len(values)
    detail = "" if ok else f" first difference at ask {int(np.flatnonzero((got != want).any(axis=1))[0])}"
    print(f"rank {rank}/{world} rccl-stub: spread-headroom {ok} model {model_ok} rows {rows_ok} pinned-elsewhere {elsewhere} no-self-match {bool(res_ok)} mismatch {errors == 1} "
          f"({P} asks x {N} nodes, floors {sorted(set(want[:, 6].tolist()))}, pinned in {sorted(set(pinned))}){detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (ok and model_ok and rows_ok and elsewhere and res_ok and errors == 1) else 3)


if __name__ == "__main__":
    main()
