"""Allocation rounds on DESIGNED clusters (tests/_roundgen.py): each population sits on a limit the round's device code branches
on — run lengths decided by arithmetic and the 64-ask header window, the widths at which the scan over the moved nodes leaves its
flat form, more moved nodes than one load round of the bitsets covers, the point where the batched replay has to stop, the cells of
a delta record — and tests/test_round_inputs.py holds every population to those claims on the CPU. Here the device is held against the
oracle's sequential loop with round_against_oracle of tests/test_gpu_sequential.py as it stands (every decision, the round
counters, the whole grid and every node's node_info after the assumes), under the sequential kernel and under the batched form.
A default engine picks the form itself (lists of 512 asks or more with a mean run shorter than four go in batches), so both
tests pin it with YKPRED_TUNE round_batched=0 / round_batched=1 (set for the whole test) and every case asserts through
round_info() which form its round took."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as orc
import _roundgen as gen
from test_gpu_sequential import pkg, round_against_oracle

pytestmark = pytest.mark.gpu
FORMS = ["sequential", "batched"]


@pytest.fixture(scope="module")
def managers():
    made = {}
    yield lambda form: made[form] if form in made else made.setdefault(form, pkg.GpuPredicateManager())
    for m in made.values():
        m.close()


@pytest.fixture
def pm(managers, form, monkeypatch):
    """The manager of the form, with the knob in place for the whole test: the host creates a new engine whenever a snapshot
    changes the table dimensions, and every engine reads YKPRED_TUNE when it is created."""
    monkeypatch.setenv("YKPRED_TUNE", "round_batched=1" if form == "batched" else "round_batched=0")
    return managers(form)


@contextlib.contextmanager
def recorded_rounds(pm, form):
    """What round_info() counts for every allocate_round call made inside (read around the call itself, on the engine that ran it);
    on leaving, every call must have taken the form asked for."""
    seen, inner = [], pm.allocate_round

    def recording(*a, **kw):
        pm.sync()
        before = pm.round_info()
        got = inner(*a, **kw)
        after = pm.round_info()
        seen.append({k: after[k] - before[k] for k in after})
        return got

    pm.allocate_round = recording
    try:
        yield seen
    finally:
        del pm.allocate_round
    taken, other = ("rounds_batched", "rounds_sequential") if form == "batched" else ("rounds_sequential", "rounds_batched")
    assert seen and all(info[taken] == 1 and info[other] == 0 for info in seen), seen


def checked_round(pm, form, snap, meta, **kw):
    """round_against_oracle, the generator's intention on top, and the form the round really took."""
    with recorded_rounds(pm, form) as seen:
        got = round_against_oracle(pm, snap, **kw)
    if meta is not None:
        assert np.array_equal(got, np.asarray(meta["expect"]))
    return got, seen[0]


@pytest.mark.parametrize("form", FORMS)
def test_runs(pm, form):
    """Run lengths at free = k req, k req - 1, k req + 1 in each of 8 dimensions, at pod slots around the quotient, without any
    request, beside 2^53; runs starting at header offsets 0, 1, 62, 63, ending with their window, crossing two windows, cut by pins,
    by another spec with 0 and 1 copies left, by the end of the list; a host port (no run)."""
    snap, meta = gen.runs()
    checked_round(pm, form, snap, meta)
    assert pm.stats()["R"] == 8


@pytest.mark.parametrize("form", FORMS)
def test_runs_in_two_calls_split_inside_a_run(pm, form):
    """The same list as two consecutive rounds cut 40 asks into the run of 130: the second starts with first_ask != 0 inside it."""
    snap, meta = gen.runs()
    pm.load_snapshot(snap)
    o = orc.Oracle(pm.dump_snapshot())
    asks = np.arange(len(snap["pods"]), dtype=np.int32)
    parts = [asks[:meta["split"]], asks[meta["split"]:]]
    want = np.concatenate([o.allocate_sequential(pods=p) for p in parts])
    with recorded_rounds(pm, form) as seen:
        got = np.concatenate([pm.allocate_round(asks=p) for p in parts])
    assert len(seen) == 2
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{len(bad)} decisions differ, first at position {bad[0]}: gpu={got[bad[0]]} oracle={want[bad[0]]}"
    assert np.array_equal(got, np.asarray(meta["expect"]))
    o2 = orc.Oracle(pm.dump_snapshot())
    for n in range(o.num_nodes):
        assert o.node_info(n) == o2.node_info(n), n


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("variant", gen.WIDE)
def test_wide(pm, form, variant):
    """One table dimension at the limit of the flat form of the scan over the moved nodes and one beyond (R 4 / 5, KT 1 / 2, W 4 / 5
    and 8 / 9, KP 1 / 2, term rows and PreFilter name rows of 64 / 68 lanes); what decides a pair sits in the LAST word or dimension,
    on nodes that already took a pod this round."""
    snap, meta = gen.wide(variant)
    checked_round(pm, form, snap, meta)
    dim, value, _ = meta["dims"]
    dims = dict(pm.stats(), KP=pm.encoded_tables()["KP"])  # (KP: the width of the port words of the encoded tables)
    assert dims[dim] == value
    assert all(dims[k] <= limit for k, limit in (("R", 4), ("KT", 1), ("W", 4), ("KP", 1)) if k != dim)


def apply_decisions(snap, decisions):
    """The snapshot with every decided ask bound to its node (what the mirror must hold after the assumes)."""
    nodes = [dict(n, pods=list(n["pods"])) for n in snap["nodes"]]
    pods = []
    for p, d in zip(snap["pods"], decisions):
        if d < 0:
            pods.append(p)
        else:
            q = json.loads(json.dumps(p))
            q["spec"]["nodeName"] = nodes[d]["metadata"]["name"]
            nodes[d]["pods"].append(q)
    return {"nodes": nodes, "pods": pods}


@pytest.mark.parametrize("form", FORMS)
def test_many_moved_at_full_size(pm, form):
    """32 768 + 192 moved nodes: the scan over the moved slots reloads its bitset words (64 steps x 512 slots per load round).
    Winners in slots >= 32 768 and < 512, dead slots in both halves. The device against the closed form that
    tests/test_round_inputs.py holds equal to the oracle's loop at this size; then every node's node_info."""
    snap, meta = gen.many_moved()
    pm.load_snapshot(snap)
    before = pm.round_stats()
    with recorded_rounds(pm, form):
        got = pm.allocate_round()
    want = np.asarray(meta["expect"])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{len(bad)} decisions differ, first at position {bad[0]}: gpu={got[bad[0]]} closed form={want[bad[0]]}"
    st = pm.round_stats()
    assert st["rounds_on_device"] == before["rounds_on_device"] + 1 and st["asks_one_by_one"] == before["asks_one_by_one"]
    o, o2 = orc.Oracle(apply_decisions(snap, want)), orc.Oracle(pm.dump_snapshot())
    assert o2.num_pods == int((want < 0).sum())
    for n in range(o.num_nodes):
        assert o.node_info(n) == o2.node_info(n), n


@pytest.mark.parametrize("form", FORMS)
def test_many_moved_at_4000_nodes(pm, form):
    """The same generator below the reload, through the oracle itself."""
    snap, meta = gen.many_moved(4000)
    checked_round(pm, form, snap, meta)


@pytest.mark.parametrize("form", FORMS)
def test_batched_cut(pm, form):
    """14 distinct specs that rank the same candidates and fill a node each: from the ninth ask on, all 8 proposed candidates are
    accepted and full and the lists were cut — the replay must stop there and propose again."""
    snap, meta = gen.batched_cut()
    _, info = checked_round(pm, form, snap, meta)
    if form == "batched":
        assert info["batches"] > 1


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_asks", [255, 256, 257, 513])
def test_batched_lists(pm, form, n_asks):
    """List lengths around the 256 asks of a batch, a run of one spec across position 256, a host-port ask directly behind accepted
    pods on its best node."""
    snap, meta = gen.batched_lists(n_asks)
    _, info = checked_round(pm, form, snap, meta)
    if form == "batched":
        assert info["batches"] > 1 and info["batched_asks"] == n_asks


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_constraints", [16, 17])
def test_spread_minima_that_move_in_one_assume(pm, form, n_constraints):
    """16 and 17 spread constraints count the same pods: their minima rise in the same assume — as many as the workgroup's shared
    list holds (kRoundDirty = 16), and one more."""
    snap, _ = gen.many_constraints(n_constraints)
    got, _ = checked_round(pm, form, snap, None)
    assert (got >= 0).sum() > 60


def test_delta_record_limit_on_a_node_sharded_cluster(tmp_path):
    """Two ranks on one GPU (tests/_shard_delta_worker.py, the collectives through tests/c/rccl_stub.cpp): pods that add to exactly
    10 histogram cells — every decision equals the oracle; pods that add to 11 — every rank gets the engine's refusal
    (YKPRED_E_UNSUPPORTED: "more histogram cells than a delta record holds"); a following round without them equals the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(root, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29787", os.path.join(root, "tests", "_shard_delta_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    lines = [ln for ln in (out.stdout + out.stderr).splitlines() if "delta limit" in ln or "Error" in ln]
    assert out.returncode == 0, lines[-8:]
    assert out.stdout.count("ten True eleven_refused True after True on_device True") == 2, lines[-8:]
