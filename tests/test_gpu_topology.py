"""PodTopologySpread and InterPodAffinity on the device — k_spread_count, k_spread_min, constraints_fail, plane_spread and, on the
incremental path, k_spread_diff / k_mark_dirty_classes — on the designed clusters of tests/_topogen.py, at their rule boundaries.

Every case loads a Python-built snapshot; the oracle is built from the same JSON text, never from dump_snapshot. Two references:
the oracle (the PreFilter pass once per ask) and the model of tests/_topogen.py, which tests/test_topology_inputs.py holds equal to
the oracle and which says WHY a bit is what it is (sibling templates, the absent domain, the closed form of the skew ladder).
Compared per case: the whole bitmap, all counts, all decisions — again after evaluate(direct=True) —, for representative asks every
node's (fit, failing plugin, missing-label bit) from query_pod_packed and the explain bins, and the sums of the histograms the
engine keeps (spread_tensors). Nothing here has a tolerance."""
import importlib

import numpy as np
import pytest

import _oracle as orc
import _topogen
from test_topology_inputs import LISTS, Edited, case, interpod_steps, interpod_steps_hold, ladder_steps, ladder_steps_hold

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("yunikorn-k8shim_amd")
REASON_MISSING_LABEL = 3   # YKPRED_REASON_MISSING_TOPOLOGY_LABEL = 1 << 3
FORMS = ("default", "spread", "interpod", "topology", "spread-filter-only", "interpod-filter-only")


def unpack(bitmap, n):
    return np.unpackbits(bitmap.view(np.uint8), axis=1, bitorder="little")[:, :n]


def manager(form):
    if form == "default":
        return pkg.GpuPredicateManager()
    pre, filt = LISTS[form]
    return pkg.GpuPredicateManager.internal(list(pre), list(pre), list(filt), list(filt))


def layout_line(what, m, c, which):
    lay = m.layout()
    keys = ("num_pods", "num_nodes", "num_classes", "num_rows", "plane_rows", "spread_cells")
    print(f"TOPO-LAYOUT {what} " + " ".join(f"{k}={getattr(lay, k)}" for k in keys) + f" signatures={c.model(which)['signatures']}")


def decisions_of(c, fit):
    """First fitting node in bin-pack order (ascending score, ties by NodeID) per ask, -1 = none."""
    scores = c.oracle.binpack_scores()
    order = np.lexsort((np.array([n.encode() for n in c.names], dtype="S"), scores))
    rank = np.empty(c.n, dtype=np.int64)
    rank[order] = np.arange(c.n)
    masked = np.where(fit.astype(bool), rank[None, :], c.n)
    return np.where(fit.any(axis=1), order[np.minimum(masked.min(axis=1), c.n - 1)], -1)


def check_answers(m, c, which, what, pods=None, nodes=None):
    """Bitmap, counts and decisions of the evaluation just run against both references. pods / nodes: the engine's index of every
    ask / node of the case (None: the identity — a freshly loaded snapshot)."""
    fit, _ = c.grid(which)
    mod = c.model(which)
    assert np.array_equal(fit, mod["fit"]), f"{what}: the two references differ"
    lay = m.layout()
    assert lay.num_nodes == c.n
    if pods is None:
        assert lay.num_pods == len(c.uids)
        got = m.read_bitmap()
        for name, want in (("oracle", fit), ("model", mod["fit"])):   # every word, the padding bits of the last word included
            bad = np.argwhere(got != orc.pack_bits(want))
            assert bad.size == 0, f"{what}: {len(bad)} bitmap words differ from the {name}, first ask {c.uids[bad[0][0]]} word {bad[0][1]}"
        pods = np.arange(len(c.uids))
    else:
        got = unpack(m.read_bitmap(), c.n)[pods][:, nodes]
        bad = np.argwhere(got != fit)
        assert bad.size == 0, f"{what}: {len(bad)} bits differ, first ask {c.uids[bad[0][0]]} node {bad[0][1]}: gpu {got[tuple(bad[0])]}"
    cnt = m.read_counts()[pods]
    bad = np.flatnonzero(cnt != fit.sum(axis=1))
    assert bad.size == 0, f"{what}: count of {c.uids[bad[0]]}: {cnt[bad[0]]} want {fit[bad[0]].sum()}"
    dec = m.read_decisions()[pods]
    if nodes is not None:
        inverse = np.empty(c.n, dtype=np.int64)
        inverse[nodes] = np.arange(c.n)
        dec = np.where(dec >= 0, inverse[np.maximum(dec, 0)], -1)
    want = decisions_of(c, fit)
    bad = np.flatnonzero(dec != want)
    assert bad.size == 0, f"{what}: decision of {c.uids[bad[0]]}: {dec[bad[0]]} want {want[bad[0]]}"
    pre, filt = (orc.mask_of(_topogen._masks(LISTS[which])[k]) for k in (0, 1))
    for p in (0, len(c.uids) // 2, len(c.uids) - 1):   # the decision rule itself, by the oracle
        assert c.oracle.decide(p, pre, filt, prefilter_once=True) == (int(fit[p].sum()), int(want[p])), f"{what}: o.decide({c.uids[p]})"


def representatives(c):
    """One ask per template: every ask of the small populations; of the ladder every 64th rung, the rungs around every zone's
    threshold, and the asks that are no rungs."""
    if "ladder" not in c.meta:
        return [k for k, u in enumerate(c.uids) if not u.endswith("-twin")]
    rung = {s: c.at[u] for u, s, _ in c.meta["ladder"]}
    near = {s for off in c.meta["offsets"].values() for s in range(off - 1, off + 3)} | set(range(1, len(rung) + 1, 64)) | {len(rung)}
    others = set(range(len(c.uids))) - set(rung.values())
    return sorted({rung[s] for s in near if s in rung} | others)


def check_queries(m, c, which, what, allocate=True):
    """query_pod_packed over all nodes and the explain bins of the representatives against the model."""
    mod = c.model(which)
    prefiltered = "filter-only" not in which
    reps = representatives(c)
    bins = m.explain(reps, allocate=allocate)
    for k, p in enumerate(reps):
        word = m.query_pod_packed(p, allocate=allocate)
        fit, code, miss = (word >> 8) & 1, word & 0xFF, (word >> (9 + REASON_MISSING_LABEL)) & 1
        assert np.array_equal(fit, mod["fit"][p]), f"{what}: query fit of {c.uids[p]}"
        bad = np.flatnonzero(code != mod["code"][p])
        assert bad.size == 0, f"{what}: failing plugin of {c.uids[p]} on node {bad[0]}: {code[bad[0]]} want {mod['code'][p][bad[0]]}"
        want = np.zeros(11, dtype=np.int64)
        want[:9] = np.bincount(mod["code"][p][mod["fit"][p] == 0], minlength=9)
        want[9] = mod["fit"][p].sum()
        assert np.array_equal(bins[k][:11], want), f"{what}: explain bins of {c.uids[p]}: {bins[k][:11].tolist()} want {want.tolist()}"
        if prefiltered:
            assert np.array_equal(miss.astype(bool), mod["missing"][p]), f"{what}: missing-label bit of {c.uids[p]}"
            assert bins[k][12 + REASON_MISSING_LABEL] == mod["missing"][p].sum(), f"{what}: missing-label bin of {c.uids[p]}"
    return len(reps)


def check_histograms(m, c, which, what):
    """The engine keeps one histogram per distinct signature; the order of its cells is its business, their sums are not."""
    m.synchronize()
    counts, present = m.spread_tensors()
    got = (int(counts.sum().item()), int(present.sum().item()))
    print(f"TOPO-HIST {what} count cells sum {got[0]} present cells sum {got[1]} (model {c.model(which)['sums']})")
    assert got == c.model(which)["sums"], f"{what}: sums of the histogram cells {got}, model {c.model(which)['sums']}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["skew_ladder", "policies", "hostname", "interpod"])
def test_designed_population(name, form):
    """One population under one manager: the default one in both phases, managers limited to PodTopologySpread, InterPodAffinity and
    both, and the two Filter-without-PreFilter forms (every pair fails with the plugin's code)."""
    c = case(name)
    m = manager(form)
    try:
        m.load_snapshot(c.text)
        phases = (("all", True), ("reservation", False)) if form == "default" else ((form, True),)
        for which, allocate in phases:
            what = f"{name} [{which}]"
            m.evaluate(allocate=allocate)
            if allocate:
                layout_line(what, m, c, which)
            check_answers(m, c, which, what)
            if "filter-only" not in which:
                check_histograms(m, c, which, what)
            n = check_queries(m, c, which, what, allocate)
            m.evaluate(allocate=allocate, direct=True)
            check_answers(m, c, which, what + " direct")
            print(f"TOPO-CASE {what}: {len(c.uids)} asks x {c.n} nodes, fit share {c.grid(which)[0].mean():.3f}, {n} asks queried and explained")
        if form == "default":   # nothing of these populations may be routed to the CPU manager
            routed = [u for u in c.uids if not m.ask_supported(u)[0]]
            assert not routed and m.routing_stats()["unsupported_asks"] == 0, f"{name}: routed as unsupported: {routed[:3]} {m.ask_supported(routed[0]) if routed else ''}"
            if name == "skew_ladder":
                # kManySigs: plane_spread packs 64 signatures per block from here on. The engine's own number of signatures: every
                # rung is one zone constraint, and a signature's histogram has one cell per zone
                zones = len(c.meta["offsets"])
                assert c.model("all")["signatures"] > 4096 and m.layout().spread_cells == zones * c.model("all")["signatures"] > zones * 4096
    finally:
        m.close()


# ---- incremental steps -----------------------------------------------------------------------------------------------------------
def check_edited(m, ed, what):
    now = ed.case(what)
    pods = np.array([m.pod_index(u) for u in now.uids], dtype=np.int64)
    nodes = np.array([m.node_index(x) for x in now.names], dtype=np.int64)
    assert pods.min() >= 0 and len(set(pods.tolist())) == len(pods) and sorted(nodes.tolist()) == list(range(now.n))
    check_answers(m, now, "all", what, pods, nodes)
    return now


def run_steps(m, c, steps, what):
    """From a full evaluation: every step, then evaluate_dirty(decisions=True) and the whole answer against both references built from
    the EDITED snapshot. → (cases after each step, what evaluate_dirty returned)."""
    m.load_snapshot(c.text)
    m.evaluate()
    check_answers(m, c, "all", what)
    ed = Edited(c, m)
    after, patched = [], []
    full = m.counters()["full_evals"]
    for step, (label, edit) in enumerate(steps):
        before = m.counters()["node_patches"]
        edit(ed)
        patched.append(m.evaluate_dirty(decisions=True))
        print(f"TOPO-STEP {what}, step {step + 1} ({label}): evaluate_dirty returned {patched[-1]}")
        after.append(check_edited(m, ed, f"{what}, step {step + 1} ({label})"))
        if patched[-1] >= 0:
            assert m.counters()["node_patches"] > before and m.counters()["full_evals"] == full, f"{what}, step {step + 1}: no column patch counted"
        full = m.counters()["full_evals"]
    m.evaluate()
    layout_line(what + ", full evaluation at the end", m, after[-1], "all")
    check_edited(m, ed, what + ", full evaluation at the end")
    return after, patched


def test_incremental_steps_on_the_skew_ladder():
    """The ladder with a ninth zone of one node and the minDomains siblings, 4203 topology signatures. In order: an assume that takes
    the offset-63 zone to 64 (every rung's histogram moves, the minimum does not); an assume onto the minimum zone (B → B + 1: the
    global minimum rises); an assume of a pod nobody selects (no histogram moves: one column); RemovePod of the first; ForgetPod of
    the second (its ask is back, pinned); the ninth zone's only node loses its zone label (nine domains → eight: md-9 flips to its
    minDomains branch). tests/test_topology_inputs.py holds the steps to these claims; here every step must be patched."""
    c = case("skew_ladder+ninth")
    m = pkg.GpuPredicateManager()
    try:
        after, patched = run_steps(m, c, ladder_steps(c), "skew_ladder+ninth")
    finally:
        m.close()
    ladder_steps_hold(c, after)
    assert patched[2] == 1, f"a pod nobody selects: evaluate_dirty returned {patched[2]}"
    assert [p >= 0 for p in patched] == [True] * 6, f"evaluate_dirty returned {patched}"


def test_incremental_steps_on_the_interpod_population():
    """In order: an assume of a `fresh` pod into z0 (the "no match anywhere" escape ends: its siblings fit z0 only); an assume of a pod
    nobody selects (one column); RemovePod of the first (the escape is back); an assume of a `fresh` pod onto a node WITHOUT the zone
    label (a match exists, but in no domain: the escape still holds); ForgetPod of it. Every step must be patched."""
    c = case("interpod")
    m = pkg.GpuPredicateManager()
    try:
        after, patched = run_steps(m, c, interpod_steps(c), "interpod")
    finally:
        m.close()
    interpod_steps_hold(c, after)
    assert patched[1] == 1, f"a pod nobody selects: evaluate_dirty returned {patched[1]}"
    assert [p >= 0 for p in patched] == [True] * 5, f"evaluate_dirty returned {patched}"
