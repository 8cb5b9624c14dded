"""The designed clusters of tests/_advgen.py are what they claim — through the oracle alone, no device.

tests/test_gpu_adversarial.py compares the engine with the oracle on these populations at the sizes where the row writers differ;
that comparison only discriminates if the inputs really contain the cases the writers special-case (a step that clears a whole
word, a step that clears one bit, free == request, empty rows, values on both sides of 2^53, class sizes on either side of every
admission threshold). Those properties are asserted here at small sizes, as conditions on the oracle's grid."""
import json
import os

import numpy as np
import pytest

import _advgen
import _oracle as orc

THREADS = min(16, os.cpu_count() or 8)
FIT = orc.PLUGIN_BITS["NodeResourcesFit"]


def _index(snap):
    return {p["metadata"]["uid"]: k for k, p in enumerate(snap["pods"])}


def test_generators_are_deterministic_and_names_are_not_in_index_order():
    a = json.dumps(_advgen.sweep(5, 200, 400)[0], sort_keys=True)
    assert a == json.dumps(_advgen.sweep(5, 200, 400)[0], sort_keys=True)
    assert a != json.dumps(_advgen.sweep(6, 200, 400)[0], sort_keys=True)
    for fn in (_advgen.two_dims, _advgen.own_templates):
        assert json.dumps(fn(5, 200, 600)[0]) == json.dumps(fn(5, 200, 600)[0])
    assert json.dumps(_advgen.uneven_classes(5, 100, 20000)[0]) == json.dumps(_advgen.uneven_classes(5, 100, 20000)[0])
    names = [_advgen.node_name(i) for i in range(2000)]
    assert len(set(names)) == 2000 and sorted(names) != names
    order = np.argsort(np.array(names, dtype="S"))
    assert (np.diff(order) < 0).sum() >= 100   # the string order jumps back in index order again and again


@pytest.mark.parametrize("nodes,asks,families", [(1500, 1000, 4), (1345, 900, 5)])
def test_sweep_population_has_the_steps_the_sweep_special_cases(nodes, asks, families):
    snap, meta = _advgen.sweep(11, nodes, asks, families=families)
    assert len(snap["pods"]) == asks and len(snap["nodes"]) == nodes
    assert set(meta["word_kind"]) == set(_advgen.WORD_KINDS)
    uids = [p["metadata"]["uid"] for p in snap["pods"]]
    cpu = [meta["cpu_of"][u] for u in uids if u.startswith("a-")]
    assert len(set(cpu)) == len(cpu) == asks - 24 and sorted(cpu) != cpu   # all distinct, row order is not value order
    steps = np.diff(sorted(cpu))
    assert steps.min() >= 1 and len(set(steps.tolist())) >= 5               # an irregular grid, not consecutive integers
    o = orc.Oracle(snap)
    want = o.eval_grid(threads=THREADS)
    elig = o.eval_grid(pre_mask=orc.ALL & ~FIT, filt_mask=orc.ALL & ~FIT, threads=THREADS)
    assert len(np.unique(want, axis=0)) >= min(asks, nodes) // 2
    runs = {}
    for k, u in enumerate(uids):
        if u.startswith("a-"):
            runs.setdefault(meta["run_of"][u], []).append(k)
    assert len(runs) == families * len(_advgen.MEM_PALETTE)
    pairs = differing = 0
    whole_word = one_node = empty = full = False
    for run, rows in runs.items():
        if len(rows) < 2:
            continue
        rows.sort(key=lambda k: meta["cpu_of"][uids[k]])
        g = want[rows].astype(np.int8)
        assert (np.diff(g, axis=0) <= 0).all(), run   # a larger request never gains a node
        d = np.diff(g, axis=0) != 0
        per_pair = d.sum(axis=1)
        pairs += len(per_pair)
        differing += int((per_pair > 0).sum())
        if run[0] in ("plain", "all") and len(rows) >= 20:   # (every run together below; one by one where the family is wide)
            assert (per_pair > 0).sum() * 2 >= len(per_pair), (run, int((per_pair > 0).sum()), len(per_pair))
        padded = np.zeros((d.shape[0], (nodes + 63) // 64 * 64), dtype=bool)
        padded[:, :nodes] = d
        whole_word |= bool((padded.reshape(d.shape[0], -1, 64).sum(axis=2) == 64).any())
        one_node |= bool((per_pair == 1).any())
        empty |= bool((g.sum(axis=1) == 0).any())
        full |= bool(any(np.array_equal(want[k], elig[k]) and elig[k].any() for k in rows))
    assert differing * 2 >= pairs, (differing, pairs)
    assert whole_word and one_node and empty and full, (whole_word, one_node, empty, full)
    # the run that starts above the largest free value of its nodes: every row empty although nodes are eligible
    low = [k for k, u in enumerate(uids) if u.startswith("a-") and meta["run_of"][u][0] == "iso-low"]
    assert low and not want[low].any() and elig[low].any(axis=1).all()
    # free == request fits, free == request - 1 does not (NodeResourcesFit alone decides; read back from the oracle's own bookkeeping)
    fit_only = o.eval_grid(pre_mask=FIT, filt_mask=FIT, threads=THREADS)
    free = np.array([o.node_info(j)["alloc"][0] - o.node_info(j)["requested"][0] for j in range(nodes)], dtype=np.int64)
    assert np.array_equal(free, np.array(meta["free_cpu"], dtype=np.int64))
    exact = short = 0
    for k, u in enumerate(uids):
        if not u.startswith("a-") or meta["run_of"][u][1] != 0:
            continue   # (no memory request: the cpu value alone decides)
        req = o.pod_request(k)["cpu"]
        assert req == meta["cpu_of"][u]
        at = np.flatnonzero(free == req)
        exact += len(at)
        assert fit_only[k, at].all()
        below = np.flatnonzero(free == req - 1)
        short += len(below)
        assert not fit_only[k, below].any()
    assert exact >= 64 and short >= 10, (exact, short)


def test_sweep_more_draws_new_values_of_the_same_families():
    snap, meta = _advgen.sweep(3, 300, 500)
    more = _advgen.sweep_more(meta, 40)
    new = [int(p["spec"]["containers"][0]["resources"]["requests"]["cpu"][:-1]) for p in more]
    assert len(set(new)) == 40 and not set(new) & set(meta["values"])
    assert len({p["metadata"]["uid"] for p in more} | {p["metadata"]["uid"] for p in snap["pods"]}) == 540


def test_two_dims_population_groups_and_int64_edges():
    nodes, asks = 1100, 1800
    snap, meta = _advgen.two_dims(21, nodes, asks)
    uids = [p["metadata"]["uid"] for p in snap["pods"]]
    at = _index(snap)
    o = orc.Oracle(snap)
    fit_only = o.eval_grid(pre_mask=FIT, filt_mask=FIT, threads=THREADS)
    info = [o.node_info(j) for j in range(nodes)]
    free = np.array([[n["alloc"][d] - n["requested"][d] for d in range(3)] for n in info], dtype=object)
    eph_values = set()
    for g, dims in (("cpu", ["cpu"]), ("mem", ["memory"]), ("both", ["cpu", "memory"])):
        rows = [k for k, u in enumerate(uids) if meta["group_of"][u] == g]
        assert len(rows) == meta["groups"][g] > 0
        fits = fails = 0
        for k in rows:
            req = o.pod_request(k)
            eph_values.add(req.get("ephemeral-storage", 0))
            if g != "both" and set(req) - set(dims):
                continue   # (a second dimension could decide: only the asks where the walked one decides alone are counted)
            want = np.ones(nodes, dtype=bool)
            for d in dims:
                want &= np.array([f >= req[d] for f in free[:, 0 if d == "cpu" else 1]])
            assert np.array_equal(fit_only[k].astype(bool), want), (g, uids[k])
            fits += int(want.sum())
            fails += int((~want).sum())
        assert fits > 100 and fails > 100, (g, fits, fails)
    assert len(eph_values) > 256   # more distinct values than walk_rows: the third dimension must stay on ballot planes
    cpu_vals = {o.pod_request(k).get("cpu", 0) for k in range(asks)}
    mem_vals = {o.pod_request(k).get("memory", 0) for k in range(asks)}
    assert len(cpu_vals) > 256 and len(mem_vals) > 256
    # the int64-edge slice: exact values, fitting and failing pairs on both sides of 2^53, nothing decided by a rounded double
    assert orc.lib().orc_quantity_value(b"8Ei") == _advgen.I64_MAX
    edge_nodes = meta["edge_nodes"]
    assert len(edge_nodes) >= 64
    efree = [int(free[j, 1]) for j in edge_nodes]
    assert all(-(1 << 63) <= f <= _advgen.I64_MAX for f in efree)
    sides = {"below": [0, 0], "above": [0, 0]}
    seen_requests = set()
    for u in meta["edge_asks"]:
        k = at[u]
        req = o.pod_request(k)["memory"]
        seen_requests.add(req)
        for j, f in zip(edge_nodes, efree):
            assert bool(fit_only[k, j]) == (f >= req), (u, j, f, req)
            if abs(f - req) <= 2 and abs(req - (1 << 53)) <= 2:   # neighbours that a double cannot tell apart above 2^53
                side = "below" if req < (1 << 53) else "above"
                sides[side][0 if f >= req else 1] += 1
    assert seen_requests >= {(1 << 53) - 1, 1 << 53, (1 << 53) + 1, 1 << 62, _advgen.I64_MAX}
    assert all(v[0] > 0 and v[1] > 0 for v in sides.values()), sides


@pytest.mark.parametrize("big", [False, True])
def test_own_templates_population_shape(big):
    snap, meta = _advgen.own_templates(31, 1000, 2000, big_palette=big)
    assert len(snap["pods"]) == 2000
    sizes = {}
    for s in meta["sig_of"].values():
        sizes[s] = sizes.get(s, 0) + 1
    popular = sorted(sizes.values(), reverse=True)[:3]
    own = [n for s, n in sizes.items() if s.startswith("own-")]
    assert sum(popular) >= 2000 * 0.7 and min(popular) >= 200
    assert len(own) >= 100 and max(own) <= 7 and min(own) >= 1
    o = orc.Oracle(snap)
    rows = set()
    for k in range(2000):
        req = o.pod_request(k)
        rows |= {(name, value) for name, value in req.items() if value > 0}
    assert (len(rows) > 16) == big and len(rows) < 256   # ballot rows: all staged / some classes have unstaged rows; nothing walked
    want = o.eval_grid(threads=THREADS)
    assert 0.02 < want.mean() < 0.9
    assert len(np.unique(want, axis=0)) >= 400


def test_uneven_classes_population_sizes_and_distinct_templates():
    nodes, asks = 333, 20000
    snap, meta = _advgen.uneven_classes(41, nodes, asks)
    assert len(snap["pods"]) == asks
    counts = np.bincount(meta["template_of"], minlength=len(meta["templates"]))
    assert np.array_equal(counts, np.array(meta["sizes"]))
    sizes = sorted(counts.tolist())
    assert set(range(1, 65)) <= set(sizes)
    ladder = [s for s in sorted(set(sizes)) if 64 <= s <= meta["ladder_top"]]
    assert len(ladder) > 10 and all(b <= a * 1.08 + 1e-9 or b == a + 1 for a, b in zip(ladder, ladder[1:]))
    assert sizes.count(1) >= min(asks // 20, 1500) and sizes[-1] >= asks // 10
    # members are interleaved: no template's asks are contiguous
    t = np.array(meta["template_of"])
    assert (t[1:] == t[:-1]).mean() < 0.5
    # one oracle row per template; templates the generator calls different differ unless its own model says "equal"
    first = {}
    for k, tpl in enumerate(meta["template_of"]):
        first.setdefault(tpl, k)
    reps = [first[tpl] for tpl in range(len(meta["templates"]))]
    o = orc.Oracle(snap)
    want = o.eval_grid(pods=reps, threads=THREADS)
    model = _advgen.model_rows(snap, meta)
    for tpl in range(len(reps)):
        assert frozenset(np.flatnonzero(want[tpl]).tolist()) == model[tpl], meta["templates"][tpl]
    groups = {}
    for tpl, row in enumerate(want):
        groups.setdefault(row.tobytes(), []).append(tpl)
    equal_by_construction = {}
    for tpl, m in enumerate(model):
        equal_by_construction.setdefault(m, []).append(tpl)
    assert sorted(map(tuple, groups.values())) == sorted(map(tuple, equal_by_construction.values()))
    assert len(groups) >= len(reps) // 2
    # a sample of non-representative asks answers like its template's representative
    rng = np.random.default_rng(1)
    others = rng.choice(asks, size=300, replace=False)
    got = o.eval_grid(pods=others, threads=THREADS)
    assert np.array_equal(got, want[t[others]])
    more, tmpl = _advgen.uneven_more(meta, 50)
    assert all(p["spec"] is meta["specs"][k] for p, k in zip(more, tmpl))
