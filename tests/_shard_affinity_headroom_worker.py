"""Ranks of a node-sharded cluster answering "how many copies of an ask with required pod (anti-)affinity still fit" together
(ykpred_headroom_affinity on a sharded engine: every shard sums cap and nodes of its own nodes per cluster-wide domain id and in the
outside row, one all-reduce SUM per table chunk over table and flags, bootstrap and the copies derived after it from the cluster-wide
histograms) against a single engine over the WHOLE cluster and the model of tests/_affgen.py. Launched by
tests/test_gpu_affinity_headroom.py through torch.distributed.run.

  SHARD_RCCL_STUB=<tests/c/rccl_stub.cpp built as a shared library>: the ranks share cuda:0 and the engine loads the stub instead of
  librccl (ykpred_comm_use_library).
Three groups of asks over the same 200 nodes, zone z0 lying across both shards (nodes 0..63 and 192..199): self anti-affinity on the zone
(role=za; the one matching resident, on node 3 of the first shard, shuts z0 for the second shard's nodes too), required affinity to
role=svc on the zone (the one such resident, on node 196 of the second shard, opens z0 for the first shard's nodes and nothing else), and
a self-matching affinity term nobody matches (bootstrap: decided from the cluster-wide minv). Every rank checks: its cells == the
single engine's == the model's for every ask, in two table chunks; the rows of three asks; a deciding resident of the other shard
stands in a zone this shard has nodes of; and that a rank handing in another list makes EVERY rank return an error."""
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
import _affgen as ag  # noqa: E402

N, EXTRA = 200, 5
RESIDENTS = {3: [({"role": "za"}, [])], 196: [ag.SVC]}


def residents(i):
    return RESIDENTS.get(i, [])


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    stub = os.environ["SHARD_RCCL_STUB"]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    ranges = sharding.shard_ranges(N, world)
    groups = [ag.case("shard-anti", N, extra_asks=EXTRA, anti=[ag.term(ag.ZONE, role="za")], ask_labels={"role": "za"}, residents=residents),
              ag.case("shard-aff", N, extra_asks=EXTRA, req={"cpu": 900}, aff=[ag.term(ag.ZONE, role="svc")], residents=residents),
              ag.case("shard-boot", N, req={"cpu": 1500}, aff=[ag.term(ag.ZONE, role="boot")], ask_labels={"role": "boot"}, residents=residents)]
    assert all(g["snapshot"]["nodes"] == groups[0]["snapshot"]["nodes"] for g in groups)
    pods, owner = [], []
    for g in groups:
        for j, pod in enumerate(g["snapshot"]["pods"]):
            pods.append(pod)
            owner.append((g, j))
    snapshot = {"nodes": groups[0]["snapshot"]["nodes"], "pods": pods}
    P = len(pods)
    first, count = ranges[rank]
    pm = pkg.GpuPredicateManager(device=0)
    pm.load_snapshot({"nodes": snapshot["nodes"][first:first + count], "pods": pods})
    assert pm._P.ykpred_comm_use_library(stub.encode()) == 0
    sharding.attach_communicator(pm, dist, rank, world, first)
    pm.evaluate()  # (collective: the topology histograms become cluster-wide)
    got = pm.headroom_affinity()
    probe = [0, EXTRA + 1, P - 1]
    got_rows = [pm.headroom_affinity_domains(j, pre_mask=pm._masks[1], filt_mask=pm._masks[3])[1] for j in probe]
    # the agreement step: the last rank hands in another list
    errors = 0
    try:
        pm.headroom_affinity([0, 1] if rank == world - 1 else [0, 2])
    except RuntimeError:
        errors = 1
    again = pm.headroom_affinity()
    # the whole cluster on one engine, and the model
    full = pkg.GpuPredicateManager(device=0)
    full.load_snapshot(snapshot)
    want = full.headroom_affinity()
    want_rows = [full.headroom_affinity_domains(j)[1] for j in probe]
    kd = full.encoded_tables()["topology_keys"].index(ag.ZONE)
    full.close()
    ok = np.array_equal(got, want) and np.array_equal(again, want)
    models = [ag.model(g, j) for g, j in owner]
    model_ok = all(want[j].tolist() == models[j][4][:12] + [kd] + models[j][4][13:] for j in range(P))
    rows_ok = all(np.array_equal(a, b) and a.tolist() == models[j][3] for a, b, j in zip(got_rows, want_rows, probe))
    boot_ok = want[P - 1, 3] == 4 and want[P - 1, 0] == -1 and want[P - 1, 13] == 2 and bool((want[:P - 1, 3] == 0).all())
    zones = [n["metadata"]["labels"]["zone"] for n in snapshot["nodes"]]
    mine = set(zones[first:first + count])
    elsewhere = any(zones[i] in mine and not first <= i < first + count for i in RESIDENTS)  # a deciding resident of the other shard
    shut = want[0, 5] == 1 and want[0, 0] == 2 and want[EXTRA + 1, 1] == 1  # (z0 shut for the first group, the only open zone for the second)
    detail = "" if ok else f" first difference at ask {int(np.flatnonzero((got != want).any(axis=1))[0])}"
    print(f"rank {rank}/{world} rccl-stub: affinity-headroom {ok} model {model_ok} rows {rows_ok} decided-elsewhere {bool(elsewhere and shut)} bootstrap {bool(boot_ok)} "
          f"mismatch {errors == 1} ({P} asks x {N} nodes, totals {want[:, 0].tolist()}){detail}", flush=True)
    dist.barrier()
    pm.comm_destroy()
    pm.close()
    dist.destroy_process_group()
    sys.exit(0 if (ok and model_ok and rows_ok and elsewhere and shut and boot_ok and errors == 1) else 3)


if __name__ == "__main__":
    main()
