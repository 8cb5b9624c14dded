"""ykpred_preempt_victims on the MI355X against the model and the oracle of tests/test_preempt_victims_inputs.py — which pins need
through the reference's Predicates and PreemptionPredicates: all 16 cells and the per-node needs on every designed population and plugin
list, through the bare engine ABI with a hand-built table whose slack rows would change an answer if read, at the launch shapes that can
go wrong, device against device at 4 100 nodes, the level identity against preempt_reach_nodes, current after cache changes with no
evaluation, the capacity error, victims really removed one at a time, sharded."""
import copy
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as orc
import _preemptgen
import _victimgen
from _victimgen import NEVER, placed
from test_preempt_victims_inputs import FORMS, POPULATIONS, SEED, Case, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
ffi = importlib.import_module("yunikorn-k8shim_amd._ffi")
pytestmark = pytest.mark.gpu
CELLS = 16


def manager(form="default"):
    if form == "default":
        return pkg.GpuPredicateManager()
    names = list(FORMS[form])
    return pkg.GpuPredicateManager.internal(names, names, names, names)


def check(m, c, form="default", every_ask=True, what=""):
    """All 16 cells of every ask and the per-node needs against the oracle and the model."""
    by_oracle, by_model = c.needs(form)
    assert np.array_equal(by_oracle, by_model), what
    want = c.cells(form)
    got = m.preempt_victims()
    assert got.shape == (len(c.asks), CELLS)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, c.asks[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad))
    assert (got[:, :3].sum(axis=1) == len(c.nodes)).all() and not got[:, 9:].any()
    asks = range(len(c.asks)) if every_ask else range(0, len(c.asks), max(1, len(c.asks) // 16))
    for a in asks:
        needs = m.preempt_victims_nodes(a)
        assert np.array_equal(needs, by_oracle[a]), (what, c.asks[a], np.flatnonzero(needs != by_oracle[a])[:5])
    return got


@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("name", POPULATIONS)
def test_cells_and_needs_on_every_population(name, form):
    c = case(name)
    m = manager(form)
    try:
        m.load_snapshot(c.text)
        m.set_preemption_tiers(c.bounds)
        got = check(m, c, form, what=f"{name} / {form}")
        assert np.array_equal(got[:, 0], m.explain()[:, pkg.EXPLAIN_FIT])   # need 0 == the fit bin of explain
        if form == "default":
            # the level identity against the reach call, node by node; need never above the whole-tier count reach charges
            needs, levels = c.needs()[0], c.levels()
            reach = m.preempt_reach()
            for a in range(len(c.asks)):
                by_reach = m.preempt_reach_nodes(a)
                assert np.array_equal(np.where(needs[a] >= 1, levels[a], np.where(needs[a] == 0, 0, NEVER)), by_reach), c.asks[a]
                assert got[a, pkg.VICTIM_BEST_LEVEL] == reach[a, pkg.REACH_BEST_LEVEL]
                if got[a, pkg.VICTIM_BEST_NODE] == reach[a, pkg.REACH_BEST_NODE]:
                    assert got[a, pkg.VICTIM_BEST_NEED] <= reach[a, pkg.REACH_BEST_PODS]
            T = len(c.bounds)
            for node in c.nodes[:6]:
                assert m.victim_list(node, T) == c.model.victim_uids(node, T)
        if name == "order" and form == "default":
            uid, (node, level, need) = next(iter(c.meta["best"].items()))
            row, best, victims = m.preempt_victims_by_key(uid)
            assert best == node and (row[5], row[7]) == (level, need) and np.array_equal(row, got[c.asks.index(uid)])
            assert victims == c.model.victim_uids(node, len(c.bounds))[:need]
            assert m.preempt_reach_by_key(uid)[1] == "bn-b"   # (the whole-tier count names the other node)
    finally:
        m.close()


def engine_call(m, n_asks, limits):
    asks = np.arange(n_asks, dtype=np.int32)
    out = np.full((n_asks, CELLS), 7, dtype=np.int64)
    rc = m._P.ykpred_preempt_victims(m.engine, n_asks, asks.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data)
    return rc, out


def upload(m, T, base, cap, tier_end, cum, ports):
    t = ffi.YkpredVictims(T, cum.shape[1], base.ctypes.data, cap.ctypes.data, tier_end.ctypes.data, cum.ctypes.data,
                          ports.ctypes.data if ports.size else None)
    return m._P.ykpred_set_victims(m.engine, ctypes.byref(t))


@pytest.mark.parametrize("name", ("lengths", "ports", "resource_exact_8", "gaps"))
def test_bare_engine_abi_with_a_hand_built_table(name):
    """The mirror's planes laid out anew by hand — segments in REVERSE node order, three slack rows behind each and one in front of the
    first, every slack row holding 2^62 in each dimension and all-ones port words — uploaded through ykpred_set_victims: a read outside a
    segment would open (2^62 more of everything) or shut (every port taken) a pair. Then the same cells as the oracle's."""
    c = case(name)
    m = manager()
    try:
        m.load_snapshot(c.text)
        m.set_preemption_tiers(c.bounds)
        t = m.victim_table()
        T, N = t["tier_end"].shape
        R, KP = t["cum"].shape[0], t["ports_after"].shape[0]
        count = t["tier_end"][T - 1]
        cap = (count + 3).astype(np.int32)
        base = np.zeros(N, dtype=np.int32)
        at = 1
        for n in reversed(range(N)):
            base[n] = at
            at += int(cap[n])
        cum = np.full((R, at), 1 << 62, dtype=np.int64)
        ports = np.full((KP, at), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        for n in range(N):
            src = slice(int(t["seg_base"][n]), int(t["seg_base"][n]) + int(count[n]))
            cum[:, base[n]:base[n] + count[n]] = t["cum"][:, src]
            ports[:, base[n]:base[n] + count[n]] = t["ports_after"][:, src]
        tier_end = np.ascontiguousarray(t["tier_end"])
        assert upload(m, T, base, cap, tier_end, cum, ports) == 0
        limits = np.array(c.limits, dtype=np.int32)
        rc, out = engine_call(m, len(c.asks), limits)
        assert rc == 0
        want = c.cells()
        bad = np.flatnonzero((out != want).any(axis=1))
        assert len(bad) == 0, (c.asks[bad[0]], out[bad[0]].tolist(), want[bad[0]].tolist())
        needs = np.zeros(N, dtype=np.int32)
        for a in range(0, len(c.asks), 3):
            assert m._P.ykpred_preempt_victims_pod(m.engine, a, int(limits[a]), orc.ALL, orc.ALL, needs.ctypes.data) == 0
            assert np.array_equal(needs, c.needs()[0][a]), c.asks[a]
        # what the upload refuses: a segment past the rows, a tier_end past its capacity, a descending tier_end, another tier count
        far = base.copy()
        far[0] = at - int(cap[0]) + 1
        assert upload(m, T, far, cap, tier_end, cum, ports) == -1
        tight = cap.copy()
        full = int(np.argmax(count))
        tight[full] = count[full] - 1
        assert upload(m, T, base, tight, tier_end, cum, ports) == -1
        if T > 1:
            down = tier_end.copy()
            down[T - 1, full] = down[0, full] - 1
            assert upload(m, T, base, cap, down, cum, ports) == -1
        assert upload(m, T + 1, base, cap, np.vstack([tier_end, tier_end[-1:]]), cum, ports) == -4
        # ... and each refusal left the resident table as it was
        rc, again = engine_call(m, len(c.asks), limits)
        assert rc == 0 and np.array_equal(again, out)
    finally:
        m.close()


@pytest.mark.parametrize("n_nodes", (63, 64, 65, 257))
def test_launch_shapes_seventy_tasks(n_nodes):
    snapshot, bounds, meta = _victimgen.geometry(SEED, n_nodes)
    c = Case(snapshot=snapshot, bounds=bounds, meta=meta)
    m = manager()
    try:
        m.load_snapshot(c.text)
        m.set_preemption_tiers(bounds)
        got = check(m, c, every_ask=False, what=f"geometry {n_nodes}")
        assert len({tuple(r) for r in got.tolist()}) > 8
        # repeats and any order: a row is copied to every ask of its task
        rng = np.random.default_rng(n_nodes)
        pick = rng.integers(0, 70, size=150)
        assert np.array_equal(m.preempt_victims(pick), got[pick])
        assert np.array_equal(m.preempt_victims([c.asks[i] for i in pick[:9]]), got[pick[:9]])
        assert np.array_equal(m.preempt_victims(pre_mask=orc.ALL, filt_mask=orc.ALL), got)
    finally:
        m.close()


def test_device_against_device_at_4100_nodes():
    """need == preemption_predicates_batch on order(n) cut at the limit, for eight asks on every one of 4 100 nodes with up to 12 victims."""
    snapshot, bounds, _ = _victimgen.geometry(SEED + 1, 4100, n_asks=8, most=12)
    model = _victimgen.VictimModel(snapshot, bounds)
    m = manager()
    try:
        m.load_snapshot(snapshot)
        m.set_preemption_tiers(bounds)
        cells = m.preempt_victims()
        queries = []
        for a, ask in enumerate(snapshot["pods"]):
            limit = model.asks[ask["metadata"]["uid"]][2]
            for n in snapshot["nodes"]:
                queries.append((a, m.node_index(n["metadata"]["name"]), model.victim_uids(n["metadata"]["name"], limit), 0))
        index = np.array(m.preemption_predicates_batch(queries), dtype=np.int32).reshape(len(snapshot["pods"]), 4100)
        seen = set()
        for a in range(len(snapshot["pods"])):
            needs = m.preempt_victims_nodes(a)
            fit = (m.query_pod_packed(a) >> 8) & 1
            want = np.where(fit == 1, 0, np.where(index[a] < 0, NEVER, index[a] + 1)).astype(np.int32)
            assert np.array_equal(needs, want), (a, np.flatnonzero(needs != want)[:5])
            assert cells[a, :3].tolist() == [int((needs == 0).sum()), int((needs >= 1).sum()), int((needs == NEVER).sum())]
            assert cells[a, 8] == int(needs[needs >= 1].sum())
            seen |= set(needs.tolist())
        assert seen >= {NEVER, 0, 1, 2, 3, 4, 5}
    finally:
        m.close()


def small_scene():
    """li: nothing free, two 100m residents per tier; kept: nothing free, its one 100m resident sits in no tier; roomy: 1000m free."""
    b = _victimgen.BOUNDS[3]
    nodes = [_preemptgen.make_node("li", {"cpu": 600, "memory": 1 << 40}, [placed(f"li-t{t}-{i}", b[t] - 1 - i, {"cpu": 100}) for t in range(3) for i in range(2)]),
             _preemptgen.make_node("kept", {"cpu": 100, "memory": 1 << 40}, [placed("kept-r", b[2], {"cpu": 100})]),
             _preemptgen.make_node("roomy", {"cpu": 1000, "memory": 1 << 40}, [])]
    asks = [_victimgen.asker(f"a-{cpu}-{limit}", b, limit, {"cpu": cpu}) for cpu in (100, 300, 500) for limit in (1, 3)]
    asks.append(_victimgen.asker("a-filler", b, 2, {"cpu": 950}))
    return {"nodes": nodes, "pods": asks}, list(b)


def running(pod, node):
    doc = copy.deepcopy(pod)
    doc["spec"]["nodeName"] = node
    doc["status"] = {"phase": "Running"}
    return doc


def test_cache_changes_with_no_evaluation_patched_equals_fresh():
    """Answers before any evaluation; after update / add / assume / remove with NO evaluation in between the patched table answers as
    the oracle on the changed snapshot does, and as a fresh manager; a segment that outgrows its capacity brings a whole upload."""
    snapshot, bounds = small_scene()
    snap = copy.deepcopy(snapshot)
    node = {n["metadata"]["name"]: n for n in snap["nodes"]}
    m = manager()
    try:
        m.load_snapshot(snapshot)
        m.set_preemption_tiers(bounds)
        m.preempt_reach()
        assert m.counters()["full_evals"] == 0
        first = check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="before any evaluation")
        stats = m.victim_table()
        assert (stats["derived"], stats["patches"]) == (1, 0) and m.counters()["full_evals"] == 0
        kept = m.node_index("kept")
        assert m.preempt_victims_nodes(m.pod_index("a-100-1"))[kept] == NEVER
        # a priority update: the resident of `kept` drops into tier 0 — never turns into need 1
        moved = node["kept"]["pods"][0]
        moved["spec"]["priority"] = bounds[0] - 1
        m.update_pod(running(moved, "kept"))
        assert m.preempt_victims_nodes(m.pod_index("a-100-1"))[kept] == 1
        after = check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after the priority update")
        assert not np.array_equal(after, first)
        # add: a pod of the lowest priority on li goes first in its order
        new = placed("li-new", bounds[0] - 9, {"cpu": 0})
        m.update_pod(running(new, "li"))
        node["li"]["pods"].append(new)
        check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after the add")
        assert m.victim_list("li", 3)[0] == "li-new"
        # assume_pod: the filler takes 950m of roomy; it is a tier-2 victim there
        filler = next(p for p in snap["pods"] if p["metadata"]["uid"] == "a-filler")
        m.assume_pod("a-filler", "roomy")
        node["roomy"]["pods"].append(copy.deepcopy(filler))
        check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after assume_pod")
        roomy = m.node_index("roomy")
        assert m.preempt_victims_nodes(m.pod_index("a-100-3"))[roomy] == 1 and m.preempt_victims_nodes(m.pod_index("a-100-1"))[roomy] == NEVER
        # remove_pod
        gone = next(p for p in node["li"]["pods"] if p["metadata"]["uid"] == "li-t0-0")
        assert m.remove_pod("li-t0-0")
        node["li"]["pods"].remove(gone)
        patched = check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after remove_pod")
        stats = m.victim_table()
        assert stats["derived"] == 1 and stats["patches"] >= 4 and m.counters()["full_evals"] == 0
        fresh = manager()
        try:
            fresh.load_snapshot(snap)
            fresh.set_preemption_tiers(bounds)
            assert np.array_equal(fresh.preempt_victims(), patched)
        finally:
            fresh.close()
        # growth past the capacity of kept's segment (1 + 0 + 4 rows): the whole table again, and still the oracle's answers
        for i in range(6):
            extra = placed(f"kept-x{i}", bounds[1] - 1 - i, {"cpu": 0})
            m.update_pod(running(extra, "kept"))
            node["kept"]["pods"].append(extra)
        check(m, Case(snapshot=snap, bounds=bounds, meta={}), what="after the growth")
        assert m.victim_table()["derived"] == 2
    finally:
        m.close()


def test_update_past_the_capacity_is_refused_and_changes_nothing():
    """ykpred_update_victims_node with count > seg_cap: YKPRED_E_INVALID, the answers as before; the other errors of the group."""
    snapshot, bounds = small_scene()
    m = manager()
    try:
        m.load_snapshot(snapshot)
        n = len(snapshot["pods"])
        limits = np.ones(n, dtype=np.int32)
        needs = np.zeros(3, dtype=np.int32)
        m.sync()
        assert engine_call(m, n, limits)[0] == -4 and m._P.ykpred_preempt_victims_pod(m.engine, 0, 1, orc.ALL, orc.ALL, needs.ctypes.data) == -4
        with pytest.raises(RuntimeError, match="no preemption tiers"):
            m.preempt_victims()
        m.set_preemption_tiers(bounds)
        before = m.preempt_victims()
        t = m.victim_table()
        li = m.node_index("li")
        cap = int(t["seg_cap"][li])
        assert cap == 6 + 3 + 4
        count = cap + 1
        tier_end = np.array([2, 4, count], dtype=np.int32)
        cum = np.zeros((t["cum"].shape[0], count), dtype=np.int64)
        ports = np.zeros((max(t["ports_after"].shape[0], 1), count), dtype=np.uint64)
        one = ffi.YkpredVictims(3, count, None, None, tier_end.ctypes.data, cum.ctypes.data, ports.ctypes.data if t["ports_after"].shape[0] else None)
        assert m._P.ykpred_update_victims_node(m.engine, li, count, ctypes.byref(one)) == -1
        assert m._P.ykpred_update_victims_node(m.engine, 99, 1, ctypes.byref(one)) == -1
        limits = np.ascontiguousarray(before[:, 4], dtype=np.int32)
        rc, out = engine_call(m, n, limits)
        assert rc == 0 and np.array_equal(out, before)
        # a count inside the capacity is taken: li with its first two victims freeing 500m each
        tier_end[:] = (2, 2, 2)
        two = np.zeros((t["cum"].shape[0], 2), dtype=np.int64)
        two[0] = (500, 1000)
        one = ffi.YkpredVictims(3, 2, None, None, tier_end.ctypes.data, two.ctypes.data, ports.ctypes.data if t["ports_after"].shape[0] else None)
        assert m._P.ykpred_update_victims_node(m.engine, li, 2, ctypes.byref(one)) == 0
        rc, out = engine_call(m, n, limits)
        assert rc == 0 and not np.array_equal(out, before)
        assert m._P.ykpred_preempt_victims_pod(m.engine, m.pod_index("a-500-1"), 1, orc.ALL, orc.ALL, needs.ctypes.data) == 0 and needs[li] == 1
        # limits outside 0..T, an index out of range: YKPRED_E_INVALID, nothing written
        for bad in (len(bounds) + 1, -1):
            wrong = limits.copy()
            wrong[n - 1] = bad
            rc, out = engine_call(m, n, wrong)
            assert rc == -1 and (out == 7).all()
            assert m._P.ykpred_preempt_victims_pod(m.engine, 0, bad, orc.ALL, orc.ALL, needs.ctypes.data) == -1
        # counts as one query
        q = m.counters()["queries"]
        m.preempt_victims()
        assert m.counters()["queries"] == q + 1
        # a routed ask: status 1 from the host without a device call
        routed = _victimgen.asker("a-routed", bounds, 2, {"cpu": 100})
        routed["spec"]["volumes"] = [{"name": "data", "persistentVolumeClaim": {"claimName": "pvc-1"}}]
        m.update_pod(routed)
        rows = m.preempt_victims()
        r = m.pod_index("a-routed")
        assert rows[r].tolist() == [0, 0, 0, 1, 2, 0, -1] + [0] * 9
        with pytest.raises(pkg.UnsupportedAsk):
            m.preempt_victims_by_key("a-routed")
        with pytest.raises(KeyError):
            m.preempt_victims_by_key("no-such-pod")
        # the table goes with the tiers
        m.set_preemption_tiers([])
        assert engine_call(m, n, limits)[0] == -4
    finally:
        m.close()


def test_victims_removed_one_at_a_time_turn_predicates_to_fit_exactly_at_need():
    """On the best node of three asks: remove_pod the victims of the prefix in order; Predicates() says no until `need` are gone.
    n0 holds 10m + 5 x 100m, n1 9 x 50m, all of one priority (the uids order them), nothing free."""
    b = _victimgen.BOUNDS[3]
    lo = b[0] - 1
    nodes = [_preemptgen.make_node("n0", {"cpu": 510, "memory": 1 << 40}, [placed(f"n0-v{i}", lo, {"cpu": 10 if i == 0 else 100}) for i in reversed(range(6))]),
             _preemptgen.make_node("n1", {"cpu": 450, "memory": 1 << 40}, [placed(f"n1-v{i}", lo, {"cpu": 50}) for i in range(9)])]
    asks = [_victimgen.asker(f"a-{cpu}", b, 3, {"cpu": cpu}) for cpu in (60, 250, 450)]
    for uid, best_want, need_want in (("a-60", "n0", 2), ("a-250", "n0", 4), ("a-450", "n0", 6)):
        m = manager()
        try:
            m.load_snapshot({"nodes": copy.deepcopy(nodes), "pods": copy.deepcopy(asks)})
            m.set_preemption_tiers(b)
            row, best, victims = m.preempt_victims_by_key(uid)
            need = int(row[pkg.VICTIM_BEST_NEED])
            assert (best, need) == (best_want, need_want) and len(victims) == need == m.preempt_victims_nodes(uid)[m.node_index(best)]
            assert victims == m.victim_list(best, int(row[pkg.VICTIM_LIMIT]))[:need] == [f"{best}-v{i}" for i in range(need)]
            for i, v in enumerate(victims):
                assert m.predicates(uid, best, True)[1] is not None, (uid, best, i)
                assert m.remove_pod(v)
                assert m.preempt_victims_nodes(uid)[m.node_index(best)] == need - i - 1
            assert m.predicates(uid, best, True) == ("", None)
        finally:
            m.close()


def test_node_sharded_engines_return_cluster_wide_cells(tmp_path):
    """World 2 on one GPU over tests/c/rccl_stub.cpp (tests/_shard_victims_worker.py): the best node on the other shard, a tie across
    shards to the lower global index, [8] cluster-wide."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29747",
           os.path.join(ROOT, "tests", "_shard_victims_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("cells True best True needs True") == 2, (out.stdout[-1500:], out.stderr[-1500:])
