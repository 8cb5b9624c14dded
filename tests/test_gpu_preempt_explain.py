"""ykpred_preempt_explain on the MI355X against the model and the oracle of tests/test_preempt_explain_inputs.py: all 32 cells and the
per-node words on every designed population and plugin list; device against device on the same engine (preempt_reach, explain, the
per-node words aggregated in numpy); the launch shapes that can go wrong (N off the wave width and across the 256-node block, 70 tasks
= three chunks of 32), 4 100 nodes device against device; the six reduce calls sharing one table buffer; current after a change
through the mirror with no evaluation; the evaluation state untouched; errors; sharded."""
import copy
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as orc
import _preemptexplaingen as gen
import _preemptgen
import _reachgen
from _reachgen import victim
from test_gpu_explain import QUERIES, tiered_engine
from test_preempt_explain_inputs import FORMS, POPULATIONS, SEED, Case, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu
CELLS = 32
NEVER_BITS = 15


def manager(form="default"):
    if form == "default":
        return pkg.GpuPredicateManager()
    names = list(FORMS[form])
    return pkg.GpuPredicateManager.internal(names, names, names, names)


def masks_of(form):
    names = set(_preemptgen.PLUGINS) if "*" in FORMS[form] else set(FORMS[form])
    return orc.mask_of(names)


def dims_of(m):
    """The engine's dimension order by name, read off the call that prints them."""
    names = []
    for r in range(8):
        cells = np.zeros(CELLS, dtype=np.int64)
        cells[6] = cells[26] = cells[16 + r] = 1
        names.append(m.preempt_explain_format(cells)[len("preemption: 0/1 nodes are available: 1 Insufficient "):-1])
    return names


def aggregate(words, stands, limit):
    """The 32 cells of one ask from its per-node words and ykpred_query_pod_packed's words of the nodes as they stand (the class of a
    never node reads the code as the node stands), in numpy. [28] is not in the words: left 0."""
    words, stands = words.astype(np.int64), stands.astype(np.int64)
    level, code = (words >> 24) & 15, words & 0xff
    out = np.zeros(CELLS, dtype=np.int64)
    evaluated = code != 255
    never = (level == NEVER_BITS) & evaluated
    for c in range(9):
        out[c] = (never & (code == c)).sum()
    out[9] = ((level == 0) & evaluated).sum()
    out[10] = (~evaluated).sum()
    out[11] = ((level >= 1) & (level < NEVER_BITS)).sum()
    walked = np.isin(stands & 0xff, (5, 6))
    elig = (words >> 28) & 1
    short = never & walked & (elig == 1)
    out[24], out[25], out[26] = (never & walked & (elig == 0)).sum(), (never & ~walked).sum(), short.sum()
    for b in range(4):
        out[12 + b] = (short & ((words >> (9 + b)) & 1 == 1)).sum()
    for r in range(8):
        out[16 + r] = (short & ((words >> (13 + r)) & 1 == 1)).sum()
    out[27] = (short & (code == 5)).sum()
    out[29] = limit
    return out


def device_against_device(m, got, asks=None, pre=None, filt=None):
    """[9], [11] and the classes against preempt_reach; the level bits against preempt_reach_nodes; the cells against the per-node words;
    the limit-0 identities against explain — all on the same engine."""
    n = len(got)
    asks = list(range(n)) if asks is None else list(asks)
    kw = {} if pre is None else dict(pre_mask=pre, filt_mask=filt)
    reach = m.preempt_reach(asks, **kw)
    assert np.array_equal(got[:, 9], reach[:, 0]) and np.array_equal(got[:, 11], reach[:, 1:9].sum(axis=1))
    assert np.array_equal(got[:, 24:27].sum(axis=1), reach[:, 9]) and np.array_equal(got[:, :9].sum(axis=1), reach[:, 9])
    assert np.array_equal(got[:, 29], reach[:, 11]) and np.array_equal(got[:, 30], reach[:, 10])
    assert (got[:, 27] <= got[:, 26]).all() and (got[:, :12].sum(axis=1) == m.num_nodes).all() and not got[:, 31].any()
    explain = m.explain(asks, **kw)
    for i in np.flatnonzero(got[:, 29] == 0):
        assert np.array_equal(got[i, :10], explain[i, :10]) and not got[i, 26:29].any() and not got[i, 12:24].any()
        assert got[i, 24] == explain[i, 5] + explain[i, 6] and got[i, 25] == explain[i, :5].sum() + explain[i, 7] + explain[i, 8]
    if pre is None:
        for i, a in enumerate(asks):
            words = m.preempt_explain_nodes(a)
            levels = m.preempt_reach_nodes(a)
            assert np.array_equal(np.where(((words >> 24) & 15) == NEVER_BITS, -1, (words >> 24) & 15).astype(np.int32), levels), a
            want = aggregate(words, m.query_pod_packed(a), got[i, 29])
            want[28] = got[i, 28]
            assert np.array_equal(got[i], want), (a, got[i].tolist(), want.tolist())
            assert got[i, 28] >= got[i, 26]   # every not-enough node holds at least one eligible pod


def check(m, c, form="default", what=""):
    """All 32 cells of every ask and the per-node words against the model (held to the oracle on the CPU)."""
    assert all(name == d or name.startswith("resource #") for name, d in zip(dims_of(m), _preemptgen.DIMS))   # (the model's bit order)
    want = c.cells(form)
    got = m.preempt_explain()
    assert got.shape == (len(c.asks), CELLS)
    order = [m.node_index(n) for n in c.nodes]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, c.asks[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad))
    words = c.words(form)
    for a in range(len(c.asks)):
        mine = m.preempt_explain_nodes(a)[order]
        assert np.array_equal(mine, words[a]), (what, c.asks[a], [(c.nodes[n], hex(mine[n]), hex(words[a][n])) for n in np.flatnonzero(mine != words[a])[:4]])
    return got


@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("name", POPULATIONS)
def test_cells_and_words_on_every_population(name, form):
    c = case(name)
    model, oracle = c.by_model(form), c.by_oracle(form)
    assert all(oracle[a][n] == model[a][n][:2] for a in range(len(c.asks)) for n in range(len(c.nodes)))
    m = manager(form)
    try:
        m.load_snapshot(c.text)
        m.set_preemption_tiers(c.bounds)
        got = check(m, c, form, what=f"{name} / {form}")
        device_against_device(m, got)
        if form == "default":
            uid = "a-ts"
            text = m.preempt_explain_message(uid)
            assert text == m.explain_format(m.explain([uid])[0]) + " " + m.preempt_explain_format(got[c.asks.index(uid)])
            assert " preemption: " in text and "Insufficient memory" in text.split(" preemption: ")[1]
    finally:
        m.close()


@pytest.mark.parametrize("n_nodes", (63, 65, 257))
def test_launch_shapes_seventy_tasks(n_nodes):
    snapshot, bounds, meta = gen.geometry(SEED, n_nodes)
    c = Case(snapshot=snapshot, bounds=bounds, meta=meta)
    m = manager()
    try:
        m.load_snapshot(c.text)
        m.set_preemption_tiers(bounds)
        want = c.cells()
        got = m.preempt_explain()
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:5]
        assert len({tuple(r) for r in got.tolist()}) > 8 and got[:, 26].any() and got[:, 24].any() and got[:, 11].any()
        pick = np.arange(0, 70, 9)
        device_against_device(m, got[pick], pick)
        # repeats and any order: a row is copied to every ask of its task
        rng = np.random.default_rng(n_nodes)
        pick = rng.integers(0, 70, size=150)
        assert np.array_equal(m.preempt_explain(pick), got[pick])
        assert np.array_equal(m.preempt_explain([c.asks[i] for i in pick[:9]]), got[pick[:9]])
    finally:
        m.close()


def test_device_against_device_at_4100_nodes():
    snapshot, bounds, _ = gen.geometry(SEED + 1, 4100, n_asks=8)
    m = manager()
    try:
        m.load_snapshot(snapshot)
        m.set_preemption_tiers(bounds)
        got = m.preempt_explain()
        device_against_device(m, got)
        assert got[:, 26].any() and got[:, 24].any() and got[:, 11].any() and got[:, 28].sum() > got[:, 26].sum()
    finally:
        m.close()


def test_the_six_reduce_calls_share_one_table_buffer():
    """ykpred_preempt_explain carves its table out of the buffer of the five other reduce calls. Back to back with them on one engine,
    lists of 70 tasks, then 1, then 33: every result equals the same call on a fresh engine that makes no other call."""
    queries = dict(QUERIES, preempt_explain=lambda m, asks: m.preempt_explain(asks))
    want, lists = {}, {}
    for name, query in queries.items():   # the references, computed once
        m, own = tiered_engine()
        try:
            lists = {1: np.array([5, 5, 5], dtype=np.int32), 33: own[:36:-1].copy(), 70: own}
            for k, asks in lists.items():
                want[name, k] = query(m, asks).copy()
        finally:
            m.close()
    assert len({tuple(r) for r in want["preempt_explain", 70].tolist()}) > 8 and want["preempt_explain", 70][:, 26].any()
    m, _ = tiered_engine()
    try:
        order = [(name, k) for k in (70, 1, 33) for name in queries] + [("preempt_explain", k) for k in (33, 70, 1)]
        for step, (name, k) in enumerate(order):
            got = queries[name](m, lists[k])
            assert got.dtype == want[name, k].dtype and np.array_equal(got, want[name, k]), (step, name, k)
    finally:
        m.close()


def small_scene():
    """li: nothing free, one 100m resident per tier; kept: nothing free, its one 100m resident sits in no tier; roomy: 1000m free."""
    b = _reachgen.BOUNDS[3]
    nodes = [_preemptgen.make_node("li", {"cpu": 300, "memory": 1 << 40}, [victim(f"li-t{t}", b, t, {"cpu": 100}) for t in range(3)]),
             _preemptgen.make_node("kept", {"cpu": 100, "memory": 1 << 40}, [victim("kept-r", b, 3, {"cpu": 100})]),
             _preemptgen.make_node("roomy", {"cpu": 1000, "memory": 1 << 40}, [])]
    asks = [_reachgen.asker(f"a-{cpu}-{limit}", b, limit, {"cpu": cpu}) for cpu in (100, 200, 300, 2000) for limit in (1, 3)]
    return {"nodes": nodes, "pods": asks}, list(b)


def test_follows_the_mirror_and_disturbs_no_evaluation():
    """Answers before any evaluation; ykpred_answer_state and the bitmap checksum are the same after a call as before; one victim added
    and one removed through the mirror show in the next call with NO evaluation in between."""
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
        assert np.array_equal(m.preempt_explain(), first)
        m.preempt_explain_nodes(0)
        assert state() == before
        evals = m.counters()["full_evals"]
        big = m.pod_index("a-2000-3")
        kept = m.node_index("kept")
        # kept is a no-victims node for every ask that does not fit it
        assert first[big, 24] == 2 and first[big, 26] == 1 and first[big, 28] == 3
        assert not m.preempt_explain_nodes(big)[kept] & pkg.PREEMPT_EXPLAIN_ELIGIBLE
        # one victim ADDED: a 50m pod of tier 0 lands on kept (over-committing it) — eligible now, and still not enough for 2000m
        added = victim("kept-new", bounds, 0, {"cpu": 50})
        m.update_pod(dict(copy.deepcopy(added), spec=dict(added["spec"], nodeName="kept"), status={"phase": "Running"}))
        node["kept"]["pods"].append(added)
        after = check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after a victim was added")
        assert after[big, 24] == 1 and after[big, 26] == 2 and after[big, 28] == 4
        assert m.preempt_explain_nodes(big)[kept] & pkg.PREEMPT_EXPLAIN_ELIGIBLE
        # one victim REMOVED: tier 0 of li leaves for good — one wasted eviction fewer
        gone = next(p for p in node["li"]["pods"] if p["metadata"]["uid"] == "li-t0")
        assert m.remove_pod("li-t0")
        node["li"]["pods"].remove(gone)
        last = check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after a victim was removed")
        assert last[big, 26] == 2 and last[big, 28] == 3
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
        out = np.full((n, CELLS), 7, dtype=np.int64)
        words = np.zeros(3, dtype=np.uint32)
        # no table: YKPRED_E_STATE, from the engine and from the host
        assert m._P.ykpred_preempt_explain(m.engine, n, asks.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data) == -4
        assert m._P.ykpred_preempt_explain_pod(m.engine, 0, 1, orc.ALL, orc.ALL, words.ctypes.data) == -4
        assert (out == 7).all()
        with pytest.raises(RuntimeError, match="no preemption tiers"):
            m.preempt_explain()
        m.set_preemption_tiers(bounds)
        rows = m.preempt_explain()
        # a routed ask: [10] = N, status 1, the limit; from the host without a device call, from the engine by its flag
        want = [0] * CELLS
        want[10], want[29], want[30] = 3, 2, 1
        assert rows[2].tolist() == want and (rows[np.arange(n) != 2, 30] == 0).all()
        with pytest.raises(pkg.UnsupportedAsk):
            m.preempt_explain_message("a-routed")
        limits = np.ascontiguousarray(rows[:, 29], dtype=np.int32)
        assert m._P.ykpred_preempt_explain(m.engine, n, asks.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data) == 0
        assert np.array_equal(out, rows)
        assert np.array_equal(m.preempt_explain(pre_mask=orc.ALL, filt_mask=orc.ALL), rows)
        assert m._P.ykpred_preempt_explain_pod(m.engine, 2, 2, orc.ALL, orc.ALL, words.ctypes.data) == 0
        assert (words & 0xff == 255).all() and ((words >> 24) & 15 == NEVER_BITS).all()
        # a limit of T + 1, a negative one, an ask index out of range: YKPRED_E_INVALID, nothing written
        out[:] = 7
        for bad in (len(bounds) + 1, -1):
            wrong = limits.copy()
            wrong[n - 1] = bad
            assert m._P.ykpred_preempt_explain(m.engine, n, asks.ctypes.data, wrong.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data) == -1
            assert m._P.ykpred_preempt_explain_pod(m.engine, 0, bad, orc.ALL, orc.ALL, words.ctypes.data) == -1
        far = asks.copy()
        far[0] = n
        assert m._P.ykpred_preempt_explain(m.engine, n, far.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data) == -1
        assert m._P.ykpred_preempt_explain(m.engine, n, None, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data) == -1
        assert (out == 7).all()
        assert m._P.ykpred_preempt_explain(m.engine, 0, None, None, orc.ALL, orc.ALL, None) == 0
        # counts as one query
        q = m.counters()["queries"]
        m.preempt_explain()
        assert m.counters()["queries"] == q + 1
        # no nodes at all: zero counts
        m.load_snapshot({"nodes": [], "pods": snapshot["pods"][:2]})
        m.set_preemption_tiers(bounds)
        empty = m.preempt_explain()
        assert m.num_nodes == 0 and not empty[:, :29].any() and m.preempt_explain_nodes(0).shape == (0,)
        assert m.preempt_explain_format(empty[0]) == "preemption: 0/0 nodes are available."
    finally:
        m.close()


def test_node_sharded_engines_return_cluster_wide_cells(tmp_path):
    """World 2 on one GPU over tests/c/rccl_stub.cpp (tests/_shard_preempt_explain_worker.py): the curing tier's pods and the not-enough
    nodes on the other shard, a differing limit list as the same error on every rank."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29747",
           os.path.join(ROOT, "tests", "_shard_preempt_explain_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("cells True design True words True mismatch True") == 2, (out.stdout[-1500:], out.stderr[-1500:])
