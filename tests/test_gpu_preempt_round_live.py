"""ykpred_preempt_round_live on the MI355X against the model of tests/_liveroundgen.py — which tests/test_live_round_inputs.py pins to the
reference step by step: all 8 cells of every turn and the summary on every designed round and plugin list; the three identities (the host
loop with real remove_pod / assume_pod, coupled asks included, and the histograms that loop leaves behind against out_counts /
out_minima; ykpred_preempt_round's cells where nothing is coupled and nothing contributes; ykpred_headroom_spread's and
ykpred_headroom_affinity's copies at limit 0); device against the loop at 4 100 nodes; an empty list, two calls in a row, nothing resident
touched, the two error codes, the effects plane and its patching, sharded."""
import copy
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _affgen
import _liveroundgen as gen
import _oracle as orc
import _preemptroundgen
import _spreadgen
from test_gpu_preempt_round import host_loop, same
from test_gpu_preempt_victims import manager, upload
from test_live_round_inputs import FORMS, ROUNDS, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu
CELLS = 8


def loaded(c, form="default"):
    m = manager(form)
    m.load_snapshot(c.text)
    m.set_preemption_tiers(c.bounds)
    return m


@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("name", ROUNDS)
def test_cells_and_summary_on_every_round(name, form):
    c = case(name)
    want, want_summary = c.cells(form)
    m = loaded(c, form)
    try:
        got, summary, counts, minima = m.preempt_round_live(c.turns, histograms=True)
        same(got, want, c.turns, f"{name} / {form}")
        assert summary.tolist() == want_summary.tolist() and summary[4] == 0 and summary[7] > 0   # [7]: the model's (turn, row) pairs that moved a cell
        # the round-local histograms against the model's, whatever the lists hold. The model keeps its rows by meaning, the engine by
        # signature and domain id: the cells are compared as the sorted non-zero values — of the start, of the end, of end - start (cell
        # by cell on either side) and of the minima. Cell by cell in the layout's order: the host-loop identity below, on every list.
        start_counts, start_minima = m.preempt_round_live([], histograms=True)[2:]
        (m_start, m_start_min), (m_end, m_end_min), _ = c.histograms(form)
        fs, fe = gen.flat(m_start), gen.flat(m_end)
        assert gen.nonzero(start_counts) == gen.nonzero(fs.values()) and gen.nonzero(start_minima) == gen.nonzero(m_start_min)
        assert gen.nonzero(counts) == gen.nonzero(fe.values()), (gen.nonzero(counts), gen.nonzero(fe.values()))
        assert gen.nonzero(counts - start_counts) == gen.nonzero(fe.get(k, 0) - fs.get(k, 0) for k in set(fs) | set(fe))
        assert gen.nonzero(minima) == gen.nonzero(m_end_min) and len(minima) == len(c.model.hist_rows())
        assert gen.nonzero(minima - start_minima) == gen.nonzero(a - b for a, b in zip(m_end_min, m_start_min))
        if form == "default":
            before, frozen = m.preempt_victims(), m.preempt_round(c.turns)[0]
            # the round without the feature settles the coupled asks (outcome 4) or plans them on frozen histograms: it differs
            assert not np.array_equal(frozen, got)
            # by key, one crossing: the same cells, the node by name, the victims by uid
            cells, summary2, names, victims = m.preempt_round_live_by_keys(c.turns)
            same(cells, want, c.turns, name)
            assert summary2.tolist() == summary.tolist()
            for i, row in enumerate(want):
                assert names[i] == (c.nodes[row[1]] if row[1] >= 0 else ""), c.turns[i]
                assert victims[i] == (c.model.victims_of(row) if row[1] >= 0 else []), c.turns[i]
            # state starts from the engine's histograms in every call, and nothing resident was touched
            again, summary3 = m.preempt_round_live(c.turns)
            assert np.array_equal(again, got) and summary3.tolist() == summary.tolist()
            assert np.array_equal(m.preempt_victims(), before) and np.array_equal(m.preempt_round(c.turns)[0], frozen)
            assert m.counters()["full_evals"] == 0
    finally:
        m.close()


def loop_rows(loop, c, turns):
    """The host loop over the turns the engine evaluates; a routed ask takes no turn there."""
    routed = {uid for uid in turns if c.model.settled(uid) == 3}
    rows = iter(host_loop(loop, [uid for uid in turns if uid not in routed], c.snapshot))
    return [[3, -1, 0, 0, 0] if uid in routed else next(rows) for uid in turns]


@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("name", ROUNDS)
def test_identity_with_the_host_loop_and_the_histograms_it_leaves(name, form):
    """(1) The live round equals the loop preempt_victims_nodes → remove_pod per victim → assume_pod, step by step, coupled asks
    included — and its round-local histograms after the last turn are the histograms the loop's mirror ends with."""
    c = case(name)
    m, loop = loaded(c, form), loaded(c, form)
    try:
        cells, summary, counts, minima = m.preempt_round_live(c.turns, histograms=True)
        start_counts, start_minima = m.preempt_round_live([], histograms=True)[2:]
        assert len(counts) == m.layout().spread_cells > 0 and len(minima) > 0
        rows = loop_rows(loop, c, c.turns)
        assert cells[:, :5].tolist() == rows
        end_counts, end_minima = loop.preempt_round_live([], histograms=True)[2:]
        assert np.array_equal(counts, end_counts) and np.array_equal(minima, end_minima)
        assert not np.array_equal(counts, start_counts)
        assert summary[7] >= np.count_nonzero(counts != start_counts)   # (every moved cell was moved by a step; a cell can move back)
        # the engine's own histograms are what they were
        assert np.array_equal(m.preempt_round_live([], histograms=True)[2], start_counts)
        assert np.array_equal(m.spread_tensors()[0].cpu().numpy()[:len(start_counts)], start_counts)
    finally:
        m.close()
        loop.close()


def test_a_victim_alone_moves_a_cell_and_the_minimum():
    """One uncoupled ask that claims a pod matching a spread selector: a cell falls by one, nothing rises; the constraint's minimum falls."""
    c = case("victim_min")
    m = loaded(c)
    try:
        cells, summary, counts, minima = m.preempt_round_live(["claim"], histograms=True)
        start_counts, start_minima = m.preempt_round_live([], histograms=True)[2:]
        assert cells[0, [0, 3]].tolist() == [1, 1] and summary[7] >= 1
        assert (counts - start_counts).min() == -1 and (counts - start_counts).max() == 0
        assert (minima - start_minima).min() == -1 and (minima - start_minima).max() <= 0
    finally:
        m.close()


@pytest.mark.parametrize("name", ("gang_eq", "places", "bisect"))
def test_identity_with_the_plain_round_where_nothing_is_coupled(name):
    """(2) No coupled ask, specs and victims that contribute to no class: the cells of ykpred_preempt_round, and no step."""
    snapshot, bounds, meta = _preemptroundgen.round_(name, 20265)
    m = manager()
    try:
        m.load_snapshot(copy.deepcopy(snapshot))
        m.set_preemption_tiers(bounds)
        plain, plain_summary = m.preempt_round(meta["turns"])
        live, summary = m.preempt_round_live(meta["turns"])
        assert np.array_equal(live, plain) and summary.tolist() == plain_summary.tolist() and summary[7] == 0
        fx = m.victim_effects()
        assert fx["cum"].shape[0] == 0 and (fx["class_col"] == -1).all()
    finally:
        m.close()


def test_identity_with_the_spread_headroom_at_limit_0():
    """(3) W repeats of an ask that ykpred_headroom_spread answers with status 0 place exactly min(W, its copies)."""
    c = _spreadgen.case("live", req={"cpu": 900}, max_skew=2, tolerate=True, label=lambda i: f"z{i % 4}" if i % 9 else None, key="b",
                        seeded=lambda i: 1 if i % 13 == 4 else 0)
    m = manager()
    try:
        m.load_snapshot(copy.deepcopy(c["snapshot"]))
        m.set_preemption_tiers([1])   # (no priority: limit 0)
        head = m.headroom_spread([0])[0]
        copies = int(head[0])
        assert head[3] == 0 and 2 <= copies <= 600, head.tolist()
        for W in (copies - 1, copies, copies + 2):
            cells, summary = m.preempt_round_live([0] * W)
            assert summary[0] == min(W, copies) and summary[1] == 0 and summary[2] == W - min(W, copies) and (cells[:, 5] == 0).all()
            assert (cells[:min(W, copies), 0] == 0).all()
    finally:
        m.close()


def test_identity_with_the_affinity_headroom_at_limit_0():
    cases = {c["name"]: c for c in _affgen.designed_cases()}
    checked = 0
    for c in list(cases.values())[:6]:
        m = manager()
        try:
            m.load_snapshot(copy.deepcopy(c["snapshot"]))
            m.set_preemption_tiers([1])
            head = m.headroom_affinity([c["ask"]])[0]
            copies = int(head[0])
            if head[3] != 0 or not 1 <= copies <= 300:
                continue
            for W in (copies, copies + 2):
                cells, summary = m.preempt_round_live([c["ask"]] * W)
                assert summary[0] == copies and summary[2] == W - copies, (c["name"], W, copies, summary.tolist())
            checked += 1
        finally:
            m.close()
    assert checked >= 2


def coupled_geometry(seed, n_nodes):
    """_preemptroundgen.geometry with five zones, every third resident labelled app=web, every third ask a zone-spread ask over them
    (maxSkew 2) that matches itself, and every seventh ask shut out of the hosts that hold a web pod."""
    snapshot, bounds, meta = _preemptroundgen.geometry(seed, n_nodes)
    for i, node in enumerate(snapshot["nodes"]):
        node["metadata"]["labels"]["zone"] = f"z{i % 5}"
        for j, pod in enumerate(node["pods"]):
            if (i + j) % 3 == 0:
                pod["metadata"]["labels"] = {"app": "web"}
    for i, pod in enumerate(snapshot["pods"]):
        if i % 3 == 0:
            pod["metadata"]["labels"] = {"app": "web"}
            pod["spec"]["topologySpreadConstraints"] = [gen.spread("web", skew=2)]
        elif i % 7 == 0:
            pod["spec"]["affinity"] = gen.affinity(anti=[gen.term("web", gen.HOST)])
    return snapshot, bounds, meta


def test_device_against_the_loop_at_4100_nodes_with_70_asks():
    snapshot, bounds, meta = coupled_geometry(20266, 4100)
    uids = meta["turns"]
    m, loop = manager(), manager()
    try:
        m.load_snapshot(copy.deepcopy(snapshot))
        m.set_preemption_tiers(bounds)
        cells, summary, counts, minima = m.preempt_round_live(uids, histograms=True)
        loop.load_snapshot(copy.deepcopy(snapshot))
        loop.set_preemption_tiers(bounds)
        rows = host_loop(loop, uids, snapshot)
        assert cells[:, :5].tolist() == rows
        end_counts, end_minima = loop.preempt_round_live([], histograms=True)[2:]
        assert np.array_equal(counts, end_counts) and np.array_equal(minima, end_minima)
        assert summary[0] > 0 and summary[1] > 0 and summary[4] == 0 and summary[7] > 0 and (np.diff(cells[:, 5]) <= 0).all()
        assert not np.array_equal(m.preempt_round(uids)[0], cells)
    finally:
        m.close()
        loop.close()


def engine_live(m, asks, limits, hist=True):
    asks = np.ascontiguousarray(asks, dtype=np.int32)
    limits = np.ascontiguousarray(limits, dtype=np.int32)
    out = np.full((max(len(asks), 1), CELLS), 7, dtype=np.int64)
    summary = np.full(8, 7, dtype=np.int64)
    dims = np.zeros(2, dtype=np.int64)
    assert m._P.ykpred_histogram_dims(m.engine, dims.ctypes.data) == 0
    counts, minima = np.full(max(int(dims[0]), 1), 7, dtype=np.int32), np.full(max(int(dims[1]), 1), 7, dtype=np.int32)
    rc = m._P.ykpred_preempt_round_live(m.engine, len(asks), asks.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data, summary.ctypes.data,
                                        counts.ctypes.data if hist else None, minima.ctypes.data if hist else None)
    return rc, out[:len(asks)], summary, counts, minima


def test_the_two_error_codes_an_empty_list_and_the_bare_abi():
    c = case("victim_min")
    m = loaded(c)
    try:
        want = c.cells()[0]
        asks = [m.pod_index(uid) for uid in c.turns]
        limits = [c.model.asks[uid][2] for uid in c.turns]
        t = m.victim_table()
        # the tables are there, the specs' effects and the plane are not: UNSUPPORTED comes first
        rc, out, summary, _, _ = engine_live(m, asks, limits)
        assert rc == -5 and (out == 7).all() and (summary == 7).all()
        got, _ = m.preempt_round_live(c.turns)          # (the host uploads both)
        same(got, want, c.turns)
        rc, out, summary, counts, minima = engine_live(m, asks, limits)
        assert rc == 0
        same(out, want, c.turns)
        rc, out2, _, _, _ = engine_live(m, asks, limits, hist=False)   # NULL readbacks
        assert rc == 0 and np.array_equal(out2, out)
        # an empty list: the engine's histograms come back
        rc, _, summary, counts0, minima0 = engine_live(m, [], [])
        assert rc == 0 and not summary.any() and not np.array_equal(counts0, counts)
        assert np.array_equal(counts0, m.spread_tensors()[0].cpu().numpy()[:len(counts0)])
        got, summary = m.preempt_round_live([])
        assert got.shape == (0, CELLS) and not summary.any()
        # errors as ykpred_preempt_round: nothing written
        T = len(c.bounds)
        for bad in (T + 1, -1):
            rc, out2, summary2, _, _ = engine_live(m, asks, limits[:-1] + [bad])
            assert rc == -1 and (out2 == 7).all() and (summary2 == 7).all()
        assert engine_live(m, asks[:-1] + [len(c.asks)], limits)[0] == -1
        q = m.counters()["queries"]
        engine_live(m, asks, limits)
        assert m.counters()["queries"] == q + 1
        # a victim table uploaded anew drops the plane: STATE until the plane follows
        assert upload(m, T, t["seg_base"], t["seg_cap"], np.ascontiguousarray(t["tier_end"]), t["cum"], t["ports_after"]) == 0
        rc, out, summary, _, _ = engine_live(m, asks, limits)
        assert rc == -4 and (out == 7).all() and "victim-effects plane" in m._P.ykpred_last_error(m.engine).decode()
        assert m.preempt_round(c.turns)[0].shape == (len(c.turns), CELLS)   # the plain round does not need it
        # a plane of another shape is refused
        fx = m.victim_effects()
        bad = importlib.import_module("yunikorn-k8shim_amd._ffi").YkpredVictimEffects(len(fx["class_col"]), fx["cum"].shape[0], fx["cum"].shape[1] + 1,
                                                                                     fx["class_col"].ctypes.data, fx["cum"].ctypes.data)
        assert m._P.ykpred_set_victim_effects(m.engine, bad) == -1
        good = importlib.import_module("yunikorn-k8shim_amd._ffi").YkpredVictimEffects(len(fx["class_col"]), fx["cum"].shape[0], fx["cum"].shape[1],
                                                                                      fx["class_col"].ctypes.data, np.ascontiguousarray(fx["cum"]).ctypes.data)
        assert m._P.ykpred_set_victim_effects(m.engine, good) == 0
        rc, out, _, _, _ = engine_live(m, asks, limits)
        assert rc == 0
        same(out, want, c.turns)
        with pytest.raises(RuntimeError, match="no preemption tiers"):
            m.set_preemption_tiers([])
            m.preempt_round_live([0])
    finally:
        m.close()


def test_the_plane_is_patched_with_the_mirror_and_the_round_follows():
    """A live call, then pods leave and arrive (remove_pod, assume_pod): the plane is patched segment by segment — not derived anew — and
    the next live call equals a fresh manager's on the same mirror state."""
    c = case("victim_min")
    m = loaded(c)
    try:
        first, _ = m.preempt_round_live(c.turns)
        fx = m.victim_effects()
        assert fx["derived"] == 1 and fx["patches"] == 0 and fx["cum"].shape[0] == 1    # one class has a contributing victim: web
        assert m.remove_pod("vm-a0-web")
        m.assume_pod("web-1", "vm-a0")
        rest = c.turns[3:]   # (behind claim, web-1 and the routed ask)
        second, _ = m.preempt_round_live(rest)
        fx = m.victim_effects()
        assert fx["derived"] == 1 and fx["patches"] >= 1 and m.victim_table()["derived"] == 1
        fresh = manager()
        try:
            fresh.load_snapshot(m.dump_snapshot())
            fresh.set_preemption_tiers(c.bounds)
            want, _ = fresh.preempt_round_live(rest)
        finally:
            fresh.close()
        assert np.array_equal(second, want) and not np.array_equal(second, first[3:])
    finally:
        m.close()


def test_a_gang_by_key_is_the_round_of_its_copies():
    c = case("zone_gang_p2")
    m = loaded(c)
    try:
        W = len(c.turns)
        cells, summary = m.preempt_round_live(["gang"] * W)
        same(cells, c.cells()[0], c.turns)
        gang = m.preempt_gang_live("gang", W)
        assert np.array_equal(gang[0], cells) and gang[1].tolist() == summary.tolist()
        assert summary[0] + summary[1] == c.meta["copies"] and summary[2] == 2
        assert [len(v) for v in gang[3]] == cells[:, 3].tolist() and all(n for n in gang[2][:c.meta["copies"]])
        with pytest.raises(KeyError):
            m.preempt_round_live_by_keys(["gang", "no-such-pod"])
    finally:
        m.close()


def test_node_sharded_engines_plan_the_live_round_together(tmp_path):
    """World 2 on one GPU over tests/c/rccl_stub.cpp (tests/_shard_preempt_round_live_worker.py): for rank 0 the chosen nodes, their
    victims and the deciding domain counts are on the other shard."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29749",
           os.path.join(ROOT, "tests", "_shard_preempt_round_live_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("cells True histograms True agreement True") == 2, (out.stdout[-1500:], out.stderr[-1500:])
