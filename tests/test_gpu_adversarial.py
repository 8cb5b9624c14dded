"""The row writers on clusters the product neither generated nor serialised (tests/_advgen.py), whole grids against the oracle.

Every case loads a Python-built snapshot, and the oracle is built from the same JSON text — never from dump_snapshot. Compared per
case: every word of the bitmap (padding words zero), every count, every decision, the reservation phase, a second allocation
pass, failing-plugin codes of 20 000 random pairs; and the layout counters prove that the intended kernel wrote the rows, so no
case silently tests a fallback. Every knob setting is compared with the ORACLE, not with another knob setting; the oracle's grids
are built once per (population, size) and reused across the knob settings (the parametrisation keeps them adjacent).

Decisions of all asks come from a numpy statement of the bin-pack rule (ascending score, ties by NodeID string, first fitting
node of the oracle's grid); that statement is first held equal to o.decide on 120 sampled asks, so the rule is pinned by the
oracle and not by the engine.

tests/test_adversarial_inputs.py shows on the CPU that these populations contain what the writers special-case.
"""
import importlib
import json
import os
import random

import numpy as np
import pytest

import _advgen
import _oracle as orc

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("yunikorn-k8shim_amd")
THREADS = min(16, os.cpu_count() or 8)
NAMES = orc.PLUGIN_NAMES


class Expect:
    """What the oracle says about one snapshot. rows_*: one row per distinct expectation, row_of[p]: the row of ask p (the
    identity, except for population (d) where an ask's row is its template's)."""

    def __init__(self, snap, meta, row_of=None, reps=None, check_members=0):
        self.snap, self.meta = snap, meta
        self.text = json.dumps(snap)
        self.uids = [p["metadata"]["uid"] for p in snap["pods"]]
        o = orc.Oracle(self.text)
        self.num_nodes, self.num_pods = o.num_nodes, o.num_pods
        assert self.num_pods == len(self.uids)
        self.row_of = np.arange(self.num_pods) if row_of is None else np.asarray(row_of)
        self.want, self.plug = o.eval_grid(pods=reps, threads=THREADS, want_plugin=True)
        self.reserve = o.eval_grid(pods=reps, pre_mask=orc.RESERVE_PRE, filt_mask=orc.RESERVE_FILT, threads=THREADS)
        rng = np.random.default_rng(17)
        if check_members:   # asks that are not their template's representative, evaluated by the oracle themselves
            others = np.setdiff1d(np.arange(self.num_pods), np.asarray(reps))
            sample = rng.choice(others, size=check_members, replace=False).astype(np.int32)
            assert np.array_equal(o.eval_grid(pods=sample, threads=THREADS), self.want[self.row_of[sample]])
        # the bin-pack rule in numpy, pinned by o.decide
        self.scores = o.binpack_scores()
        ids = np.array([n["metadata"]["name"] for n in snap["nodes"]], dtype="S")
        order = np.lexsort((ids, self.scores))
        w = self.want[:, order]
        first = w.argmax(axis=1)
        self.dec = np.where(w[np.arange(len(w)), first] > 0, order[first], -1).astype(np.int32)
        self.cnt = self.want.sum(axis=1).astype(np.int32)
        for p in rng.choice(self.num_pods, size=min(120, self.num_pods), replace=False):
            assert o.decide(int(p)) == (int(self.cnt[self.row_of[p]]), int(self.dec[self.row_of[p]])), int(p)
        self.packed = orc.pack_bits(self.want)
        self.packed_reserve = orc.pack_bits(self.reserve)
        self.cnt_reserve = self.reserve.sum(axis=1).astype(np.int32)
        o.close()


_cache = {}


def expectation(key, build):
    """One population at a time (the cases of one (population, size) are adjacent): the CPU cost is paid once, the memory too."""
    if key not in _cache:
        _cache.clear()
        _cache[key] = build()
    return _cache[key]


def per_ask(generate):
    snap, meta = generate()
    return Expect(snap, meta)


def per_template(snap, meta):
    t = np.asarray(meta["template_of"])
    reps = np.full(len(meta["templates"]), -1, dtype=np.int32)
    reps[t[::-1]] = np.arange(len(t) - 1, -1, -1, dtype=np.int32)   # the first member of every template
    assert reps.min() >= 0
    return Expect(snap, meta, row_of=t, reps=reps, check_members=600)


def compare_bitmap(m, packed_rows, counts_rows, row_of, idx=None, what=""):
    """Every word of every ask's row. idx: the engine row of ask k (None: ask order = engine order)."""
    lay = m.layout()
    words = packed_rows.shape[1]
    assert lay.row_words == words
    got = m.read_bitmap()
    cnt = m.read_counts()
    if idx is not None:
        got, cnt = got[idx], cnt[idx]
    assert got.shape == (len(row_of), words), (got.shape, len(row_of), words)
    for lo in range(0, len(row_of), 8192):
        sl = slice(lo, lo + 8192)
        exp = packed_rows[row_of[sl]]
        if not np.array_equal(got[sl], exp):
            bad = np.argwhere(got[sl] != exp)[0]
            p, w = lo + int(bad[0]), int(bad[1])
            diff = int(got[p, w]) ^ int(exp[bad[0], w])
            node = w * 64 + (diff & -diff).bit_length() - 1
            raise AssertionError(f"{what}: bitmap differs, first at ask {p} word {w} (node {node}): got {int(got[p, w]):#018x} want {int(exp[bad[0], w]):#018x}")
    assert np.array_equal(cnt, counts_rows[row_of]), f"{what}: counts differ"


def layout_line(case, lay):
    keys = ("num_pods", "num_nodes", "num_classes", "num_rows", "band_rows", "band_steps", "index_rows", "index_rows_walked", "sweep_rows", "run_rows",
            "fused_rows")
    print("ADV-LAYOUT " + case + " " + " ".join(f"{k}={getattr(lay, k)}" for k in keys))


def full_check(m, ex, case, layout_check, scores=False):
    m.load_snapshot(ex.text)
    m.evaluate()
    lay = m.layout()
    layout_line(case, lay)
    assert lay.num_nodes == ex.num_nodes and lay.num_pods == ex.num_pods
    layout_check(lay)
    compare_bitmap(m, ex.packed, ex.cnt, ex.row_of, what="allocation pass")
    assert m.check_class_rows() == 0
    dec = m.read_decisions()
    bad = np.flatnonzero(dec != ex.dec[ex.row_of])
    assert bad.size == 0, f"{len(bad)} decisions differ, first ask {bad[0]}: got {dec[bad[0]]} want {ex.dec[ex.row_of[bad[0]]]}"
    if scores:
        assert np.array_equal(m.read_scores().view(np.uint64), ex.scores.view(np.uint64))
    m.evaluate(allocate=False)   # the reservation phase: no request rows
    compare_bitmap(m, ex.packed_reserve, ex.cnt_reserve, ex.row_of, what="reservation pass")
    m.evaluate()                 # ... and the allocation writers are back
    compare_bitmap(m, ex.packed, ex.cnt, ex.row_of, what="second allocation pass")
    assert np.array_equal(m.read_decisions(), ex.dec[ex.row_of])
    assert m.check_class_rows() == 0
    # failing-plugin codes
    rng = np.random.default_rng(23)
    pods = rng.integers(0, ex.num_pods, size=20_000).astype(np.int32)
    nodes = rng.integers(0, ex.num_nodes, size=20_000).astype(np.int32)
    fit, code, _ = m.query(pods, nodes)
    assert np.array_equal(fit, ex.want[ex.row_of[pods], nodes])
    want_code = ex.plug[ex.row_of[pods], nodes]
    mism = np.flatnonzero((code != want_code) & (fit == 0))
    assert mism.size == 0, f"failing plugin differs at (ask,node)=({pods[mism[0]]},{nodes[mism[0]]}): gpu={NAMES[code[mism[0]]]} oracle={NAMES[want_code[mism[0]]]}"
    return lay


def run_case(monkeypatch, tune, ex, case, layout_check, scores=False, after=None):
    if tune:
        monkeypatch.setenv("YKPRED_TUNE", tune)
    else:
        monkeypatch.delenv("YKPRED_TUNE", raising=False)
    m = pkg.GpuPredicateManager()
    try:
        full_check(m, ex, case, layout_check, scores)
        if after:
            after(m)
    finally:
        m.close()


def knobs(tune):
    return dict(item.split("=") for item in tune.split(",") if item)


def cases(sizes, tunes):
    return [(n, p, t) for n, p in sizes for t in tunes]


def ident(v):
    return str(v) if not isinstance(v, str) else (v or "defaults")


# ---- (a) one walked dimension ---------------------------------------------------------------------------------------
SWEEP_TUNES = ["", "sweep_min_run=2", "sweep_min_run=0", "sweep_min_run=0,combine_slices=0", "run_decide=0"]


def sweep_expectation(n_nodes, n_asks):
    def build():
        ex = per_ask(lambda: _advgen.sweep(7100 + n_nodes, n_nodes, n_asks, families=6))
        # (the CPU module's condition on the whole population, here at the size the writers see)
        assert len({r.tobytes() for r in ex.packed}) >= min(n_asks, n_nodes) // 2
        return ex
    return expectation(("sweep", n_nodes, n_asks), build)


@pytest.mark.parametrize("n_nodes,n_asks,tune", cases([(1537, 5000), (8300, 5000), (29001, 3000)], SWEEP_TUNES), ids=ident)
def test_sweep_population(monkeypatch, n_nodes, n_asks, tune):
    """Population (a): k_sweep_rows on runs of hundreds of rows whose steps clear whole words, single bits and nothing; runs that
    start above every free value; node counts that end inside a word (1 537), inside a 4-word group (8 300) and just past an LDS
    segment (29 001). sweep_min_run=0 hands the same rows to k_walk_rows (+ combine_slices=0: k_combine_wave), run_decide=0
    decides the swept classes by the scan."""
    ex = sweep_expectation(n_nodes, n_asks)
    k = knobs(tune)

    def layout_check(lay):
        assert lay.index_rows >= n_asks - 30
        if k.get("sweep_min_run") == "0":
            assert lay.sweep_rows == 0 and lay.index_rows_walked == lay.index_rows, (lay.sweep_rows, lay.index_rows_walked)
        else:
            assert lay.sweep_rows >= n_asks // 2 and lay.index_rows_walked < lay.index_rows, (lay.sweep_rows, lay.index_rows_walked)

    run_case(monkeypatch, tune, ex, f"sweep {n_nodes}x{n_asks} [{tune or 'defaults'}]", layout_check)


def edit_and_compare(m, snap, removed, added, what=""):
    """remove_pod / update_pods_batch, evaluate_dirty, the whole grid against a fresh oracle on the edited object (rows matched by
    uid: removals and additions reorder the engine's asks); then a full evaluation, and again."""
    gone = set(removed)
    for uid in removed:
        assert m.remove_pod(uid)
    m.update_pods_batch(added)
    edited = {"nodes": snap["nodes"], "pods": [p for p in snap["pods"] if p["metadata"]["uid"] not in gone] + added}
    o = orc.Oracle(json.dumps(edited))
    want = o.eval_grid(threads=THREADS)
    packed, cnt = orc.pack_bits(want), want.sum(axis=1).astype(np.int32)
    scores = o.binpack_scores()
    order = np.lexsort((np.array([n["metadata"]["name"] for n in snap["nodes"]], dtype="S"), scores))
    w = want[:, order]
    first = w.argmax(axis=1)
    dec = np.where(w[np.arange(len(w)), first] > 0, order[first], -1).astype(np.int32)
    ident_rows = np.arange(len(edited["pods"]))

    def rows():
        idx = np.array([m.pod_index(p["metadata"]["uid"]) for p in edited["pods"]])
        assert idx.min() >= 0 and len(set(idx.tolist())) == len(idx) == m.layout().num_pods
        return idx

    m.evaluate_dirty()
    compare_bitmap(m, packed, cnt, ident_rows, idx=rows(), what=what + " after evaluate_dirty")
    m.evaluate()
    idx = rows()
    compare_bitmap(m, packed, cnt, ident_rows, idx=idx, what=what + " after the full evaluation")
    assert np.array_equal(m.read_decisions()[idx], dec)
    assert m.check_class_rows() == 0
    return m.layout()


def test_sweep_population_incremental(monkeypatch):
    """After the full check: 3 % of the asks leave, as many new ones of the same families arrive (cpu values nobody had)."""
    n_nodes, n_asks = 1537, 5000
    ex = sweep_expectation(n_nodes, n_asks)

    def after(m):
        rng = random.Random(5)
        removed = rng.sample(ex.uids, n_asks * 3 // 100)
        lay = edit_and_compare(m, ex.snap, removed, _advgen.sweep_more(ex.meta, len(removed)), what="sweep population")
        layout_line("sweep incremental, edited", lay)

    run_case(monkeypatch, "", ex, "sweep incremental", lambda lay: None, after=after)


# ---- (b) two walked dimensions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes,n_asks,tune", cases([(1537, 6000)], ["", "sweep_min_run=0", "walk_rows=1"]) + cases([(8300, 6000)], ["", "sweep_min_run=0"]),
                         ids=ident)
def test_two_walked_dimensions_population(monkeypatch, n_nodes, n_asks, tune):
    """Population (b): one k_sweep_rows launch per walked dimension, classes with two index rows left to k_walk_rows, a third
    many-valued dimension on ballot planes (more rows than the writers stage), and memory values at the int64 edges — 2^53 ± 1,
    2^62, 2^63 - 1 — next to the sentinels of k_dim_sort / k_dim_walk; the float64 bin-pack scores of those nodes bit for bit."""
    ex = expectation(("two_dims", n_nodes, n_asks), lambda: per_ask(lambda: _advgen.two_dims(7200 + n_nodes, n_nodes, n_asks)))
    k = knobs(tune)
    groups = ex.meta["groups"]

    def layout_check(lay):
        assert lay.index_rows > 0 and lay.index_rows_walked > 0, (lay.index_rows, lay.index_rows_walked)
        if k.get("sweep_min_run") == "0":
            assert lay.sweep_rows == 0
        else:   # more swept rows than either group alone has: both dimensions have runs
            assert lay.sweep_rows > max(groups["cpu"], groups["mem"]), (lay.sweep_rows, groups)

    run_case(monkeypatch, tune, ex, f"two_dims {n_nodes}x{n_asks} [{tune or 'defaults'}]", layout_check, scores=True)


# ---- (c) no walked dimension ----------------------------------------------------------------------------------------
OWN_TUNES = ["", "class_runs_min_rows=1", "class_runs=0", "fuse_rows=0", "fuse_wpl=1", "fuse_wpl=2", "fuse_wpl=5", "fuse_combine=0"]


@pytest.mark.parametrize("n_nodes,n_asks,tune", cases([(1537, 6000), (8300, 5000), (29001, 3000)], OWN_TUNES), ids=ident)
def test_own_templates_population(monkeypatch, n_nodes, n_asks, tune):
    """Population (c): k_class_runs on three signatures with thousands of asks, k_fused_rows / k_combine_wave on hundreds of
    signatures with 1-7 asks and a selector of their own and on asks with five request dimensions. The smallest size has at most
    16 request-value rows (all staged), the larger ones 40 x 30 values (classes with unstaged rows stay out of the runs)."""
    big = n_nodes != 1537
    ex = expectation(("own", n_nodes, n_asks), lambda: per_ask(lambda: _advgen.own_templates(7300 + n_nodes, n_nodes, n_asks, big_palette=big)))
    k = knobs(tune)

    def layout_check(lay):
        assert lay.index_rows == 0 and lay.sweep_rows == 0
        if k.get("class_runs") == "0":
            assert lay.run_rows == 0
        else:
            assert lay.run_rows >= n_asks // 4, lay.run_rows
        if k.get("fuse_rows") == "0":
            assert lay.fused_rows == 0
        else:
            assert lay.fused_rows > 0

    run_case(monkeypatch, tune, ex, f"own_templates {n_nodes}x{n_asks} [{tune or 'defaults'}]", layout_check)


# ---- (d) uneven classes: zone A -------------------------------------------------------------------------------------
# At 333 nodes a row is 128 bytes and a band of S windows holds S * 8 192 rows; zone A needs a quarter of a band from classes of
# at least 2 * piece_min(S) rows (921 at S = 32, 3 667 at S = 128, and the automatic choice is 128 there): 60 000 asks reach that
# for 4 and 8 steps only, so the 32-step case has 120 000 asks and the 128-step and automatic cases 400 000.
UNEVEN = ([(333, 60_000, t) for t in ("band_steps=4", "band_steps=8", "band_steps=-1")] + [(333, 120_000, "band_steps=32")]
          + [(333, 400_000, t) for t in ("band_steps=0", "band_steps=128")]
          + cases([(8300, 120_000), (50_000, 60_000)], ["band_steps=0", "band_steps=4", "band_steps=8", "band_steps=32", "band_steps=128", "band_steps=-1"]))


def uneven_expectation(n_nodes, n_asks):
    return expectation(("uneven", n_nodes, n_asks), lambda: per_template(*_advgen.uneven_classes(7400 + n_nodes, n_nodes, n_asks)))


def band_layout_check(tune):
    def check(lay):
        if tune == "band_steps=-1":
            assert lay.band_rows == 0
        else:   # zone A exists, and some classes stay in zone B
            assert 0 < lay.band_rows < lay.num_rows, (lay.band_rows, lay.num_rows, lay.band_steps)
    return check


@pytest.mark.parametrize("n_nodes,n_asks,tune", UNEVEN, ids=ident)
def test_uneven_classes_population(monkeypatch, n_nodes, n_asks, tune):
    """Population (d): k_expand_bands / k_class_rows / k_fix_rows on class sizes from 1 to tens of thousands — every size up to
    64, a ladder of at most 8 % steps across every admission threshold the band heights set, pieces split between bands, a
    shortened last band, straddling rows; band_steps=-1 writes the same grid through zone B alone. The expected row of an ask is
    its template's oracle row; 600 asks that are not representatives are evaluated by the oracle themselves."""
    ex = uneven_expectation(n_nodes, n_asks)
    run_case(monkeypatch, tune, ex, f"uneven {n_nodes}x{n_asks} [{tune}]", band_layout_check(tune))


def test_uneven_classes_population_incremental(monkeypatch):
    """After the full check: 3 % of the asks leave and as many new members of existing templates arrive."""
    n_nodes, n_asks = 333, 60_000
    ex = uneven_expectation(n_nodes, n_asks)

    def after(m):
        rng = random.Random(6)
        removed = rng.sample(ex.uids, n_asks * 3 // 100)
        added, _ = _advgen.uneven_more(ex.meta, len(removed))
        lay = edit_and_compare(m, ex.snap, removed, added, what="uneven classes")
        layout_line("uneven incremental, edited", lay)

    run_case(monkeypatch, "band_steps=8", ex, "uneven incremental", band_layout_check("band_steps=8"), after=after)
