"""ykpred_preempt_headroom on the MI355X against the model of tests/_gangreachgen.py — which tests/test_preempt_headroom_inputs.py pins
to the reference's allocation loop: all 32 cells and every [limit + 1][N] row on every designed population and plugin list, at the launch
shapes that can go wrong (N off the wave width and across the 256-node block, 70 tasks = three chunks of 32), device against device at
4 100 nodes, the evaluation state untouched, current after cache changes with no evaluation, list semantics, errors, a gang placed
after the preemption the answer names, sharded."""
import copy
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _gangreachgen as gg
import _headgen
import _oracle as orc
import _preemptgen
import _reachgen
from _reachgen import NEVER, victim
from test_preempt_headroom_inputs import FORMS, POPULATIONS, SEED, Case, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu
CELLS = 32


def manager(form="default"):
    if form == "default":
        return pkg.GpuPredicateManager()
    names = list(FORMS[form])
    return pkg.GpuPredicateManager.internal(names, names, names, names)


def check(m, c, form="default", every_ask=True, what=""):
    """All 32 cells of every ask with its designed want, every ask again with every want it can aim at, and the per-node rows."""
    rows, statuses, wants, want_cells = c.form(form)
    got = m.preempt_headroom(wants=wants)
    assert got.shape == (len(c.asks), CELLS)
    bad = np.flatnonzero((got != want_cells).any(axis=1))
    assert len(bad) == 0, (what, c.asks[bad[0]], got[bad[0]].tolist(), want_cells[bad[0]].tolist(), len(bad))
    idx, aims, aim_cells = c.every_aim(form)
    assert np.array_equal(m.preempt_headroom(idx, wants=aims), aim_cells), what
    asks = range(len(c.asks)) if every_ask else range(0, len(c.asks), max(1, len(c.asks) // 16))
    for a in asks:
        per_node = m.preempt_headroom_nodes(a)
        want = np.full_like(rows[a], -1) if statuses[a] == 2 else rows[a]
        assert per_node.shape == want.shape and np.array_equal(per_node, want), (what, c.asks[a], np.argwhere(per_node != want)[:5].tolist())
    return got


@pytest.mark.parametrize("name", POPULATIONS)
def test_cells_and_rows_on_every_population(name):
    """Under the default lists and under subsets: without NodePorts the port cut disappears; with BOTH topology plugins off the coupled
    asks are computed (status 0); with one of them off they stay coupled by ykpred_headroom's rule, and their node counts follow the
    frozen verdicts of the plugin that is left."""
    c = case(name)
    for form in FORMS:
        m = manager(form)
        try:
            m.load_snapshot(c.text)
            m.set_preemption_tiers(c.bounds)
            got = check(m, c, form, what=f"{name} / {form}")
            if form == "default":
                head = m.headroom()
                live = got[:, gg.STATUS] == 0
                assert np.array_equal(got[live, 0], head[live, pkg.HEADROOM_TOTAL]) and np.array_equal(got[:, gg.STATUS], head[:, pkg.HEADROOM_STATUS])
                reach = m.preempt_reach()
                assert np.array_equal(got[:, 9:18], np.cumsum(reach[:, 0:9], axis=1))
                uid = c.asks[0]
                assert np.array_equal(m.preempt_headroom_by_key(uid, int(got[0, gg.WANT])), got[0])
        finally:
            m.close()
    statuses = {form: c.form(form)[1] for form in FORMS}
    if name == "coupled":
        assert set(statuses["default"]) == {0, 2} and set(statuses["no-spread"]) == {0, 2} and set(statuses["no-topology"]) == {0}
    if name == "ports":
        a = c.asks.index("a-port")
        assert c.form("no-ports")[3][a, 0] > c.form("default")[3][a, 3] >= 1   # the whole quotient against one copy per open node


@pytest.mark.parametrize("n_nodes", (1, 63, 64, 65, 257, 300))
def test_launch_shapes_seventy_tasks(n_nodes):
    snapshot, bounds, meta = gg.geometry(SEED, n_nodes)
    c = Case(snapshot=snapshot, bounds=bounds, meta=meta)
    m = manager()
    try:
        m.load_snapshot(c.text)
        m.set_preemption_tiers(bounds)
        got = check(m, c, every_ask=False, what=f"geometry {n_nodes}")
        assert len({tuple(r) for r in got.tolist()}) > 8 or n_nodes == 1
        # repeats and any order: a task's table is finished for every ask of it, with the ask's own want
        rng = np.random.default_rng(n_nodes)
        pick = rng.integers(0, 70, size=150)
        wants = np.array(c.form()[2], dtype=np.int64)
        assert np.array_equal(m.preempt_headroom(pick, wants=wants[pick]), got[pick])
        assert np.array_equal(m.preempt_headroom([c.asks[i] for i in pick[:9]], wants=wants[pick[:9]]), got[pick[:9]])
    finally:
        m.close()


def test_device_against_device_at_4100_nodes():
    snapshot, bounds, _ = gg.geometry(SEED + 1, 4100, n_asks=8)
    m = manager()
    try:
        m.load_snapshot(snapshot)
        m.set_preemption_tiers(bounds)
        req, cnt, _ = m.reclaim_table()
        below = np.concatenate([np.zeros((1, 4100), dtype=np.int64), np.cumsum(cnt, axis=0)])   # [L][n] pods in tiers < L
        cells = m.preempt_headroom()
        reach = m.preempt_reach()
        head = m.headroom()
        seen = set()
        for a in range(8):
            rows = m.preempt_headroom_nodes(a).astype(np.int64)
            limit = int(cells[a, gg.LIMIT])
            assert rows.shape == (limit + 1, 4100) and (np.diff(rows, axis=0) >= 0).all()
            assert np.array_equal(rows[0], m.headroom_nodes(a))
            first = np.where(rows[-1] >= 1, np.argmax(rows >= 1, axis=0), NEVER)
            assert np.array_equal(first, m.preempt_reach_nodes(a))
            for L in range(9):
                at = min(L, limit)
                assert cells[a, L] == rows[at].sum() and cells[a, 9 + L] == (rows[at] >= 1).sum()
                paid = np.argmax(rows[:at + 1] == rows[at], axis=0)   # the first level that already gives the node its level-L copies
                assert cells[a, 18 + L] == below[paid, np.arange(4100)].sum()
            assert np.array_equal(cells[a, 9:18], np.cumsum(reach[a, 0:9])) and cells[a, 0] == head[a, pkg.HEADROOM_TOTAL]
            seen |= set(np.unique(first).tolist())
        assert seen >= {NEVER, 0, 1, 2, 3} and (cells[:, 3] > cells[:, 0]).any()
    finally:
        m.close()


def small_scene():
    """li: nothing free, one 100m resident per tier; kept: nothing free, its one 100m resident sits in no tier; roomy: 1000m free."""
    b = _reachgen.BOUNDS[3]
    nodes = [_preemptgen.make_node("li", {"cpu": 300, "memory": 1 << 40}, [victim(f"li-t{t}", b, t, {"cpu": 100}) for t in range(3)]),
             _preemptgen.make_node("kept", {"cpu": 100, "memory": 1 << 40}, [victim("kept-r", b, 3, {"cpu": 100})]),
             _preemptgen.make_node("roomy", {"cpu": 1000, "memory": 1 << 40}, [])]
    asks = [_reachgen.asker(f"a-{cpu}-{limit}", b, limit, {"cpu": cpu}) for cpu in (100, 200, 300) for limit in (1, 3)]
    asks.append(_reachgen.asker("a-filler", b, 2, {"cpu": 950}))
    return {"nodes": nodes, "pods": asks}, list(b)


def test_reads_the_tables_and_disturbs_no_evaluation():
    """Answers before any evaluation; ykpred_answer_state, the bitmap checksum and the resident answer are the same after a call as
    before; and the answer follows a resident added to / removed from a tier on one node through the one-column patch, with NO evaluation."""
    snapshot, bounds = small_scene()
    snap = copy.deepcopy(snapshot)
    node = {n["metadata"]["name"]: n for n in snap["nodes"]}
    m = manager()
    try:
        m.load_snapshot(snapshot)
        m.set_preemption_tiers(bounds)
        assert m.counters()["full_evals"] == 0
        first = check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="before any evaluation")
        assert m.counters()["full_evals"] == 0
        m.evaluate()

        def state():
            classes = ctypes.c_int32(-1)
            assert m._P.ykpred_answer_state(m.engine, orc.ALL, orc.ALL, ctypes.byref(classes)) == 0
            return (m.checksum(), classes.value, m.read_counts().tolist(), m.read_decisions().tolist(), m.counters()["full_evals"],
                    m.counters()["node_patches"], m.counters()["row_patches"])
        before = state()
        wants = Case(snapshot=snap, bounds=bounds, meta={}).form()[2]
        assert np.array_equal(m.preempt_headroom(wants=wants), first)
        m.preempt_headroom_nodes(0)
        assert state() == before
        evals = m.counters()["full_evals"]
        kept, a100 = m.node_index("kept"), m.pod_index("a-100-3")
        assert m.preempt_headroom_nodes(a100)[:, kept].tolist() == [0, 0, 0, 0]
        # a priority update: the resident of `kept` drops into tier 0 — the node takes a copy from level 1 on
        moved = node["kept"]["pods"][0]
        moved["spec"]["priority"] = bounds[0] - 1
        m.update_pod(dict(copy.deepcopy(moved), spec=dict(moved["spec"], nodeName="kept"), status={"phase": "Running"}))
        assert m.preempt_headroom_nodes(a100)[:, kept].tolist() == [0, 1, 1, 1]
        after = check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after the priority update")
        assert not np.array_equal(after, first)
        # assume_pod: the filler (tier 2) takes 950m of roomy — ten copies of the 100m ask become none, and ten again at level 3
        filler = next(p for p in snap["pods"] if p["metadata"]["uid"] == "a-filler")
        m.assume_pod("a-filler", "roomy")
        node["roomy"]["pods"].append(copy.deepcopy(filler))
        check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after assume_pod")
        assert m.preempt_headroom_nodes(a100)[:, m.node_index("roomy")].tolist() == [0, 0, 0, 10]
        # remove_pod: tier 0 of li leaves for good — what level 1 gave there is there as the node stands
        gone = next(p for p in node["li"]["pods"] if p["metadata"]["uid"] == "li-t0")
        assert m.remove_pod("li-t0")
        node["li"]["pods"].remove(gone)
        check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after remove_pod")
        assert m.preempt_headroom_nodes(a100)[:, m.node_index("li")].tolist() == [1, 1, 2, 3]
        assert m.counters()["full_evals"] == evals
    finally:
        m.close()


def test_list_semantics_statuses_and_errors():
    snapshot, bounds = small_scene()
    routed = _reachgen.asker("a-routed", bounds, 2, {"cpu": 100})
    routed["spec"]["volumes"] = [{"name": "data", "persistentVolumeClaim": {"claimName": "pvc-1"}}]
    snapshot["pods"].insert(2, routed)
    m = manager()
    try:
        m.load_snapshot(snapshot)
        m.sync()
        n = len(snapshot["pods"])
        asks = np.arange(n, dtype=np.int32)
        limits = np.ones(n, dtype=np.int32)
        wants = np.full(n, 2, dtype=np.int64)
        out = np.full((n, CELLS), 7, dtype=np.int64)
        rows = np.zeros((4, 3), dtype=np.int32)

        def engine(pre=orc.ALL, filt=orc.ALL, count=n, **given):
            idx, lim, w = (given.get(k, now) for k, now in (("idx", asks), ("lim", limits), ("w", wants)))   # (the lists as they are NOW)
            return m._P.ykpred_preempt_headroom(m.engine, count, None if idx is None else idx.ctypes.data, None if lim is None else lim.ctypes.data,
                                                None if w is None else w.ctypes.data, pre, filt, out.ctypes.data)
        # no table: YKPRED_E_STATE, from the engine and from the host
        assert engine() == -4 and m._P.ykpred_preempt_headroom_pod(m.engine, 0, 1, orc.ALL, orc.ALL, rows.ctypes.data) == -4
        assert (out == 7).all()
        with pytest.raises(RuntimeError, match="no preemption tiers"):
            m.preempt_headroom()
        with pytest.raises(RuntimeError, match="no preemption tiers"):
            m.preempt_headroom_nodes(0)
        m.set_preemption_tiers(bounds)
        got = m.preempt_headroom(wants=wants)
        # a routed ask: status 1, every cell but [27..29] is 0; from the host without a device call, from the engine by its flag
        assert got[2].tolist() == [0] * 27 + [1, 2, 2, 0, 0] and (got[np.arange(n) != 2, gg.STATUS] == 0).all()
        with pytest.raises(pkg.UnsupportedAsk):
            m.preempt_headroom_by_key("a-routed", 2)
        with pytest.raises(KeyError):
            m.preempt_headroom_by_key("no-such-pod", 2)
        limits = np.ascontiguousarray(got[:, gg.LIMIT], dtype=np.int32)
        assert engine() == 0 and np.array_equal(out, got)
        assert np.array_equal(m.preempt_headroom(wants=wants, pre_mask=orc.ALL, filt_mask=orc.ALL), got)
        assert m._P.ykpred_preempt_headroom_pod(m.engine, 2, 2, orc.ALL, orc.ALL, rows.ctypes.data) == 0 and not rows[:3].any()
        # wants=None is 1 for every ask; one ask with three wants is one task finished three times
        ones = m.preempt_headroom()
        assert (ones[:, gg.WANT] == 1).all() and np.array_equal(ones[:, :29], got[:, :29])
        assert engine(w=None) == 0 and np.array_equal(out, ones)
        a = m.pod_index("a-100-3")   # li 0, 1, 2, 3 + roomy 10: copies 10, 11, 12, 13
        three = m.preempt_headroom([a, a, a], wants=[10, 12, 14])
        assert three[:, gg.LEVEL].tolist() == [0, 2, -1] and three[:, gg.WANT].tolist() == [10, 12, 14] and three[0, 0:4].tolist() == [10, 11, 12, 13]
        assert np.array_equal(three[:, :29], np.repeat(got[a:a + 1, :29], 3, axis=0))
        assert m.preempt_headroom([]).shape == (0, CELLS) and engine(idx=None, lim=None, w=None, count=0) == 0
        # every error of the contract: a limit outside 0..T, a want below 1, an index out of range, a null list, NodeResourcesFit missing
        out[:] = 7
        for bad in (len(bounds) + 1, -1):
            wrong = limits.copy()
            wrong[n - 1] = bad
            assert engine(lim=wrong) == -1
            assert m._P.ykpred_preempt_headroom_pod(m.engine, 0, bad, orc.ALL, orc.ALL, rows.ctypes.data) == -1
        for bad in (0, -5):
            wrong = wants.copy()
            wrong[1] = bad
            assert engine(w=wrong) == -1
            with pytest.raises(RuntimeError, match="want below 1"):
                m.preempt_headroom(wants=wrong)
        far = asks.copy()
        far[0] = n
        assert engine(idx=far) == -1 and engine(idx=None) == -1 and engine(lim=None) == -1
        no_fit = orc.ALL & ~orc.mask_of({"NodeResourcesFit"})
        assert engine(pre=no_fit) == -1 and engine(filt=no_fit) == -1
        assert m._P.ykpred_preempt_headroom_pod(m.engine, 0, 1, no_fit, orc.ALL, rows.ctypes.data) == -1
        assert m._P.ykpred_preempt_headroom_pod(m.engine, n, 1, orc.ALL, orc.ALL, rows.ctypes.data) == -1
        assert (out == 7).all()
        with pytest.raises(RuntimeError, match="out of range"):
            m.preempt_headroom([n])
        # counts as one query
        q = m.counters()["queries"]
        m.preempt_headroom()
        assert m.counters()["queries"] == q + 1
        # the table goes with the tiers
        m.set_preemption_tiers([])
        assert engine() == -4
        # no nodes at all: zero rows, no level
        m.load_snapshot({"nodes": [], "pods": snapshot["pods"][:2]})
        m.set_preemption_tiers(bounds)
        empty = m.preempt_headroom(wants=[1, 3])
        assert m.num_nodes == 0 and not empty[:, :28].any() and empty[:, gg.LEVEL].tolist() == [-1, -1] and empty[:, gg.WANT].tolist() == [1, 3]
        assert m.preempt_headroom_nodes(0).shape[1] == 0
    finally:
        m.close()


def test_a_gang_fits_after_the_preemption_the_answer_names():
    """An ask whose want is first met at level L >= 1: delete the pods of tiers < L through the cache API; headroom now equals
    copies(L), and an allocation round over `want` clones of the ask places every one of them."""
    c = case("limits")
    rows, _, _, _ = c.form()
    a = c.asks.index("a-li-50-3")
    copies = rows[a].sum(axis=1)
    L = 2
    want = int(copies[L])
    assert copies[L - 1] < want
    m = manager()
    try:
        m.load_snapshot(c.text)
        m.set_preemption_tiers(c.bounds)
        got = m.preempt_headroom([a], wants=[want])[0]
        assert got[gg.LEVEL] == L and got[gg.COPIES + L] == want
        victims = [p["metadata"]["uid"] for n in c.snapshot["nodes"] for p in n["pods"] if 0 <= c.model.tier(p) < L]
        assert len(victims) >= got[gg.VICTIMS + L] > 0
        for uid in victims:
            assert m.remove_pod(uid)
        assert m.headroom([a])[0, pkg.HEADROOM_TOTAL] == want
        assert m.preempt_headroom([a], wants=[want])[0, gg.LEVEL] == 0
        gang = _headgen.clones(c.snapshot, a, want + 1)["pods"]
        assert m.update_pods_batch(gang) == want + 1
        members = np.array([m.pod_index(p["metadata"]["uid"]) for p in gang], dtype=np.int32)
        placed = m.allocate_round(asks=members)
        assert int((placed >= 0).sum()) == want and placed[-1] == -1   # the whole gang, and not one copy more
        per_node = m.preempt_headroom_nodes(a)
        assert not per_node[0].any() and per_node[3].any()             # ... after which only the tier that is left opens anything
    finally:
        m.close()


def test_node_sharded_engines_return_cluster_wide_cells(tmp_path):
    """World 2 on one GPU over tests/c/rccl_stub.cpp (tests/_shard_preempt_headroom_worker.py): the tiers that add copies on the other
    shard, a want that neither shard meets alone and the cluster meets at level 2, a differing want list as the same error on every rank."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29747",
           os.path.join(ROOT, "tests", "_shard_preempt_headroom_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("cells True design True rows True mismatch True") == 2, (out.stdout[-1500:], out.stderr[-1500:])
