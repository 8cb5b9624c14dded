"""GPU parity tests: the HIP engine (through the C ABI: libykhost → libykpred) against the CPU oracle.

Bar: BIT-EXACT. Every fit bit, every failing-plugin code, every feasible count, every decision and every float64
bin-pack score must equal the oracle's on the same snapshot (the oracle is fed the JSON that the host library
serialises from its own object model, or the same Python-built snapshot).
"""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import _gen
import _oracle as orc

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("yunikorn-k8shim_amd")
sharding = importlib.import_module("yunikorn-k8shim_amd.sharding")
_ffi = importlib.import_module("yunikorn-k8shim_amd._ffi")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = orc.PLUGIN_NAMES


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pm():
    m = pkg.GpuPredicateManager()
    yield m
    m.close()


def unpack(bitmap, n_nodes):
    """[P][row_words] uint64 → [P][N] 0/1 (bit n%64 of word n//64 = node n)."""
    bits = np.unpackbits(bitmap.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :n_nodes]


# ------------------------------------------------------------------------------------------------------------
# the reference's own table tests, replayed through PredicateManager.Predicates on the GPU
# ------------------------------------------------------------------------------------------------------------
PRED = load("predicate_cases.json")


@pytest.mark.parametrize("case", PRED, ids=[f"{c['test']}:{c['name']}" for c in PRED])
def test_reference_table_tests(case):
    ep = case["plugins"]
    m = pkg.GpuPredicateManager.internal(ep, ep, ep, ep)  # predicate_manager_test.go:341
    try:
        m.load_snapshot({"nodes": [case["node"]], "pods": [case["pod"]]})
        plugin, err = m.predicates(0, 0, case["allocate"])
        assert (err is None) == case["fits"], f"{case['source']}: plugin={plugin!r} err={err}"
    finally:
        m.close()


@pytest.mark.parametrize("case", load("taint_cases.json"), ids=lambda c: c["name"][:60])
def test_reference_taint_behaviour(case):
    """TaintToleration as the reference's e2e suite and KWOK tooling pin it (test/e2e/predicates/predicates_test.go:334-447,
    deployments/kwok-perf-test/*): default manager, allocation phase; the failing plugin and the `.*taint.*` log text too —
    through Predicates() and through the scheduler-interface callback (Context.IsPodFitNode)."""
    import re
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot({"nodes": [case["node"]], "pods": [case["pod"]]})
        plugin, err = m.predicates(0, 0, True)
        assert (err is None) == case["fits"], f"{case['source']}: plugin={plugin!r} err={err}"
        text = m.is_pod_fit_node(case["pod"]["metadata"]["uid"], case["node"]["metadata"]["name"], True)
        assert (text is None) == case["fits"]
        if not case["fits"]:
            assert plugin == case["plugin"] and re.match(case.get("message_regex", ".*taint.*"), err.message)
            assert text.startswith(f"failed plugin: '{case['plugin']}'") and re.search("taint", text)
        m.evaluate()
        assert int(m.read_counts()[0]) == (1 if case["fits"] else 0)
    finally:
        m.close()


@pytest.mark.parametrize("case", load("preemption_cases.json"), ids=lambda c: c["source"])
def test_reference_preemption_tests(case):
    ep = case["plugins"]
    m = pkg.GpuPredicateManager.internal(ep, ep, ep, ep)
    try:
        m.load_snapshot({"nodes": [case["node"]], "pods": [case["pod"]]})
        uids = [case["node"]["pods"][i]["metadata"]["uid"] for i in case["victims"]]
        assert m.preemption_predicates(0, 0, uids, case["start_index"]) == case["index"], case["source"]
    finally:
        m.close()


@pytest.mark.parametrize("case", load("request_cases.json"), ids=lambda c: c["name"])
def test_reference_request_vectors(pm, case):
    pm.load_snapshot({"nodes": [], "pods": [case["pod"]]})
    got = {k: v for k, v in pm.pod_request(0).items() if v != 0 or k in case["expect"]}
    assert got == case["expect"], case["source"]


def test_default_manager_phases_and_messages(pm):
    node = {"metadata": {"name": "n0"}, "spec": {"taints": [{"key": "k", "value": "v", "effect": "NoSchedule"}]},
            "status": {"allocatable": {"cpu": "1", "memory": "1Gi", "pods": "10"}}}
    pod = {"metadata": {"name": "p", "uid": "p"}, "spec": {"containers": [{"resources": {"requests": {"cpu": "2"}}}],
                                                           "tolerations": [{"key": "k", "operator": "Exists"}]}}
    pm.load_snapshot({"nodes": [node], "pods": [pod]})
    plugin, err = pm.predicates(0, 0, True)
    assert plugin == "NodeResourcesFit" and "Insufficient cpu" in err.message
    assert pm.predicates(0, 0, False) == ("", None)  # reservation phase skips NodeResourcesFit (predicate_manager.go:326,363)
    pod["spec"].pop("tolerations")
    pm.load_snapshot({"nodes": [node], "pods": [pod]})
    plugin, err = pm.predicates("p", "n0", True)
    assert plugin == "TaintToleration" and "taint" in err.message  # e2e `.*taint.*`, test/e2e/predicates/predicates_test.go:439


def test_concurrent_readers(pm):
    """Several core goroutines may sit in Predicates() at once (context.go:697,709 hold read locks only): 8 threads ask
    for interleaved pairs in both phases while another evaluates the whole grid; every answer must equal the oracle's."""
    import threading
    snap = _gen.random_snapshot(4242, n_nodes=130, n_pods=48, spread=True, interpod=True)
    pm.load_snapshot(snap)
    o = orc.Oracle(snap)
    want = {True: o.eval_grid(threads=8, want_plugin=True),
            False: o.eval_grid(pre_mask=orc.RESERVE_PRE, filt_mask=orc.RESERVE_FILT, threads=8, want_plugin=True)}
    P, N = want[True][0].shape
    errors = []

    def reader(tid):
        try:
            rng = np.random.default_rng(tid)
            for _ in range(400):
                p, n, allocate = int(rng.integers(P)), int(rng.integers(N)), bool(rng.integers(2))
                plugin, err = pm.predicates(p, n, allocate)
                fit, code = want[allocate][0][p, n], want[allocate][1][p, n]
                # a PreFilter rejection returns an error with an EMPTY plugin name (predicate_manager.go:236-238)
                if (err is None) != bool(fit) or (not fit and plugin != NAMES[code]):
                    errors.append((tid, p, n, allocate, plugin, NAMES[code] if not fit else ""))
        except Exception as exc:  # noqa: BLE001 - reported by the main thread
            errors.append((tid, repr(exc)))

    def evaluator():
        try:
            for i in range(20):
                pm.evaluate(allocate=bool(i & 1))
                got = unpack(pm.read_bitmap(), N)
                if not np.array_equal(got, want[bool(i & 1)][0]):
                    errors.append(("evaluate", i))
        except Exception as exc:  # noqa: BLE001
            errors.append(("evaluate", repr(exc)))

    threads = [threading.Thread(target=reader, args=(t,)) for t in range(8)] + [threading.Thread(target=evaluator)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]


def test_scheduler_interface_callbacks(pm):
    """The callbacks as the core issues them (scheduler_callback.go:203-216 → context.go:696-742): allocation key + node id
    in, error text / {Success, Index} out."""
    node = {"metadata": {"name": "node-1"}, "status": {"allocatable": {"cpu": "1", "memory": "100M", "pods": "10"}},
            "pods": [{"metadata": {"name": f"v{i}", "uid": f"v{i}"}, "spec": {"nodeName": "node-1", "containers": [
                {"resources": {"requests": {"cpu": c, "memory": m}}}]}} for i, (c, m) in
                enumerate([("100m", "1M"), ("100m", "1M"), ("300m", "3M"), ("500m", "5M")])]}
    small = {"metadata": {"name": "small", "uid": "task-1"}, "spec": {"containers": [{"resources": {"requests": {"cpu": "500m", "memory": "5M"}}}]}}
    none = {"metadata": {"name": "none", "uid": "task-0"}, "spec": {"containers": []}}
    pm.load_snapshot({"nodes": [node], "pods": [small, none]})
    assert pm.is_pod_fit_node("unknown", "node-1", True) == "predicates were not run because pod was not found in cache"
    assert pm.is_pod_fit_node("task-1", "unknown", True) == "predicates were not run because node was not found in cache"
    assert pm.is_pod_fit_node("task-0", "node-1", True) is None
    err = pm.is_pod_fit_node("task-1", "node-1", True)  # 1000m used of 1000m
    assert err.startswith("failed plugin: 'NodeResourcesFit'\n") and "Insufficient cpu" in err
    assert pm.is_pod_fit_node("task-1", "node-1", False) is None  # reservation phase has no NodeResourcesFit
    # TestPreemptionPredicates' node (predicate_manager_test.go:71-117) through the callback form
    assert pm.is_pod_fit_node_via_preemption("task-1", "node-1", ["v0", "v1", "v2", "v3"], 1) == (2, True)
    assert pm.is_pod_fit_node_via_preemption("task-1", "node-1", [], 0) == (-1, False)
    assert pm.is_pod_fit_node_via_preemption("unknown", "node-1", ["v0"], 0) == (-1, False)
    assert pm.is_pod_fit_node_via_preemption("task-1", "node-1", ["not-cached", "v3"], 0) == (1, True)  # unknown victim = nil pod


# ------------------------------------------------------------------------------------------------------------
# randomized edge-case clusters: full grid, both phases, bits + failing plugin
# ------------------------------------------------------------------------------------------------------------
def check_against_oracle(pm, snapshot, allocate, pre=None, filt=None, check_plugins=True):
    o = orc.Oracle(snapshot)
    if pre is None:
        pre, filt = (orc.ALL, orc.ALL) if allocate else (orc.RESERVE_PRE, orc.RESERVE_FILT)
    want, want_plugin = o.eval_grid(pre_mask=pre, filt_mask=filt, threads=8, want_plugin=True)
    pm.evaluate(allocate=allocate)
    lay = pm.layout()
    assert lay.num_nodes == o.num_nodes and lay.num_pods == o.num_pods
    got = unpack(pm.read_bitmap(), lay.num_nodes)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} differing bits, first (pod,node)={bad[0].tolist()} want={want[tuple(bad[0])]}"
    # feasible counts
    assert np.array_equal(pm.read_counts(), want.sum(axis=1).astype(np.int32))
    if check_plugins:
        P, N = want.shape
        pods, nodes = np.divmod(np.arange(P * N, dtype=np.int64), N)
        fit, code, _ = pm.query(pods.astype(np.int32), nodes.astype(np.int32), pre_mask=pre, filt_mask=filt)
        assert np.array_equal(fit.reshape(P, N), want)
        codes = code.reshape(P, N)
        mism = np.argwhere((codes != want_plugin) & (want == 0))
        assert mism.size == 0, (f"failing plugin differs at (pod,node)={mism[0].tolist()}: "
                                f"gpu={NAMES[codes[tuple(mism[0])]]} oracle={NAMES[want_plugin[tuple(mism[0])]]}")
    return o, want


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("allocate", [True, False])
def test_random_clusters_full_grid(pm, seed, allocate):
    snap = _gen.random_snapshot(1000 + seed, n_nodes=70 + 13 * seed, n_pods=60)
    pm.load_snapshot(snap)
    check_against_oracle(pm, snap, allocate)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("walk_rows", [1, 3])
def test_request_value_planes_sorted_walk(monkeypatch, seed, walk_rows):
    """NodeResourcesFit planes are kept per (dimension, distinct request value); dimensions with many distinct values are
    evaluated by the sorted walk (k_dim_sort / k_dim_walk) instead of one compare per (value, node). YKPRED_TUNE walk_rows=… forces
    that path at test sizes: random clusters with scalar resources (> 4 dimensions), over-committed nodes (negative free),
    zero and absent requests, word-boundary node counts — bits, counts, failing plugins and decisions against the oracle,
    both phases, and NodeResourcesFit alone (so that every verdict is that plugin's)."""
    monkeypatch.setenv("YKPRED_TUNE", f"walk_rows={walk_rows}")
    snap = _gen.random_snapshot(8800 + seed, n_nodes=[63, 64, 65, 129, 200, 333][seed], n_pods=90, scalars=True)
    for plugins in (["*"], ["NodeResourcesFit"]):
        m = pkg.GpuPredicateManager.internal(plugins, plugins, plugins, plugins)
        try:
            m.load_snapshot(snap)
            mask = orc.ALL if plugins == ["*"] else orc.mask_of(plugins)
            o, want = check_against_oracle(m, snap, True, pre=mask, filt=mask)
            dec = m.read_decisions()
            for p in range(0, len(snap["pods"]), 7):
                assert o.decide(p, mask, mask) == (int(want[p].sum()), int(dec[p]))
        finally:
            m.close()


def test_pending_pod_in_the_middle_of_a_resize_on_the_device(pm):
    """Divergence ledger 1: NodeResourcesFit sees yunikorn's GetPodResource — max(spec, allocatedResources,
    actual requests), or the status requests alone when the resize is infeasible — for a pending pod mid-resize."""
    import test_host_encoder as enc
    snap, want = enc._resize_snapshot()
    pm.load_snapshot(snap)
    check_against_oracle(pm, snap, True)
    bits = unpack(pm.read_bitmap(), 3)
    for p, pod in enumerate(snap["pods"]):
        assert bits[p].tolist() == want[pod["metadata"]["name"]]


@pytest.mark.parametrize("wpl", [1, 2, 4])
@pytest.mark.parametrize("n_nodes", [63, 200, 4100])
def test_sig_planes_words_per_lane(monkeypatch, wpl, n_nodes):
    """k_sig_planes<WPL>: a lane owns 1, 2 or 4 words of the row, 64 apart (chosen from the row width; forced here) — rows much
    shorter than one wave's span, rows ending inside a lane's second / fourth word, both dictionary families, rank-ordered
    planes with their first-word table (decisions) — against the oracle."""
    monkeypatch.setenv("YKPRED_TUNE", f"sig_wpl={wpl}")
    snap = _gen.random_snapshot(4200 + wpl, n_nodes=n_nodes, n_pods=70)
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(snap)
        if n_nodes < 1000:
            o, want = check_against_oracle(m, snap, True)
            pods = range(0, len(snap["pods"]), 5)
        else:
            m.evaluate()
            o = orc.Oracle(snap)
            pods = list(range(0, len(snap["pods"]), 9))
            want_s = o.eval_grid(pods=pods, threads=os.cpu_count() or 8)
            assert np.array_equal(unpack(m.read_rows(np.array(pods, dtype=np.int32)), n_nodes), want_s)
            want = {p: want_s[k] for k, p in enumerate(pods)}
        dec = m.read_decisions()
        for p in pods:
            assert o.decide(p) == (int(want[p].sum()), int(dec[p]))
    finally:
        m.close()


@pytest.mark.parametrize("walk_rows,n_nodes", [(1, 333), (3, 129), (1, 8300)])
def test_slice_writer_equals_wave_writer_and_oracle(monkeypatch, walk_rows, n_nodes):
    """The zone-B writer of populations with index rows (k_slice_desc + k_walk_rows: a wave writes whole row segments, index bytes
    decoded through the rank planes, ballot rows staged in LDS; everything else through the descriptor-filtered k_combine_wave)
    against the plain wave-per-chunk writer (YKPRED_TUNE combine_slices=0) on the same snapshot: one / two walked dimensions, pinned
    pods, duplicated pods (several member rows), rows of one partial word group up to several segments — bitmap, counts, decisions,
    and the oracle."""
    snap = _gen.random_snapshot(9900 + walk_rows, n_nodes=n_nodes, n_pods=150, scalars=True)
    got = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("YKPRED_TUNE", f"walk_rows={walk_rows},combine_slices={knob}")
        m = pkg.GpuPredicateManager()
        try:
            m.load_snapshot(snap)
            m.evaluate()
            assert m.layout().index_rows > 0
            got[knob] = (unpack(m.read_bitmap(), n_nodes), m.read_counts(), m.read_decisions())
            if knob == "1" and n_nodes < 1000:
                check_against_oracle(m, snap, True)
        finally:
            m.close()
    for a, b in zip(got["0"], got["1"]):
        assert np.array_equal(a, b)
    # the wide rows (several slices per row): sampled asks against the oracle, decisions included
    o = orc.Oracle(snap)
    sample = np.random.default_rng(5).choice(len(snap["pods"]), size=24, replace=False).astype(np.int32)
    want = o.eval_grid(pods=sample, threads=os.cpu_count() or 8, prefilter_once=True)
    assert np.array_equal(got["1"][0][sample], want)
    for k, p in enumerate(sample[:8]):
        assert o.decide(int(p), prefilter_once=True) == (int(want[k].sum()), int(got["1"][2][p]))


def test_unique_request_vectors_midsize(pm):
    """bench.py's adversarial variant in small: every ask a distinct cpu request (5 000 values in one dimension → the sorted
    walk at its default threshold), full grid against the oracle."""
    pm.generate_kwok(seed=4711, num_nodes=1500, num_pods=5000, num_templates=0, node_affinity=1, unique_requests=1)
    pm.evaluate()
    lay = pm.layout()
    assert lay.num_classes >= 4990
    o = orc.Oracle(pm.dump_snapshot(compact=True))
    want = o.eval_grid(threads=os.cpu_count() or 8)
    assert np.array_equal(unpack(pm.read_bitmap(), 1500), want)
    assert np.array_equal(pm.read_counts(), want.sum(axis=1))
    dec = pm.read_decisions()
    for p in range(0, 5000, 250):
        assert o.decide(p) == (int(want[p].sum()), int(dec[p]))


@pytest.mark.parametrize("n_nodes,n_pods,min_run", [(1500, 5000, 2), (1500, 5000, 16), (4100, 6000, 4), (8300, 4000, 2), (29000, 3000, 3)],
                         ids=["one-group", "one-group-default-runs", "two-groups-tail", "three-groups", "two-segments"])
def test_sweep_writer_equals_chunk_writers_and_oracle(monkeypatch, n_nodes, n_pods, min_run):
    """k_sweep_rows (round 6): zone-B classes of one signature in ascending order of their walked request value are written as a RUN —
    a lane keeps its word of the row in registers and only clears the nodes the next value loses (cursor lists of k_dim_sort in
    LDS), no index row is decoded or even written for them. Against the chunk writers (YKPRED_TUNE sweep_min_run=0: k_walk_rows +
    k_combine_wave, every index row walked) on the same cluster — bitmap, counts, decisions, both phases — and against the oracle:
    rows of one partial word group up to two LDS segments, short runs forced in (min_run 2), the default threshold."""
    got = {}
    for knob in (0, min_run):
        monkeypatch.setenv("YKPRED_TUNE", f"sweep_min_run={knob}")
        m = pkg.GpuPredicateManager()
        try:
            m.generate_kwok(seed=4711 + n_nodes, num_nodes=n_nodes, num_pods=n_pods, num_templates=0, node_affinity=1, unique_requests=1)
            m.evaluate()
            lay = m.layout()
            assert lay.index_rows >= n_pods - 10
            if knob:
                assert lay.sweep_rows > n_pods // 3 and lay.index_rows_walked < lay.index_rows, (lay.sweep_rows, lay.index_rows_walked)
            else:
                assert lay.sweep_rows == 0 and lay.index_rows_walked == lay.index_rows
            assert m.check_class_rows() == 0
            got[knob] = [unpack(m.read_bitmap(), n_nodes), m.read_counts(), m.read_decisions()]
            m.evaluate(allocate=False)  # the reservation phase has no request rows: the chunk writers take every class
            got[knob] += [unpack(m.read_bitmap(), n_nodes), m.read_counts()]
            m.evaluate()                # ... and the sweep is back for the next allocation pass
            assert np.array_equal(unpack(m.read_bitmap(), n_nodes), got[knob][0]) and np.array_equal(m.read_counts(), got[knob][1])
            if knob:
                o = orc.Oracle(m.dump_snapshot(compact=True))
                sample = np.arange(n_pods) if n_nodes <= 1500 else np.random.default_rng(5).choice(n_pods, size=64, replace=False).astype(np.int32)
                want = o.eval_grid(pods=sample, threads=os.cpu_count() or 8)
                assert np.array_equal(got[knob][0][sample], want)
                assert np.array_equal(got[knob][1][sample], want.sum(axis=1))
                for k, p in enumerate(sample[:12]):
                    assert o.decide(int(p)) == (int(want[k].sum()), int(got[knob][2][p]))
        finally:
            m.close()
    for a, b in zip(got[0], got[min_run]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_nodes,n_pods", [(1500, 6000), (8300, 5000), (29000, 3000)], ids=["one-group", "three-groups", "two-segments"])
def test_class_runs_writer_equals_chunk_writers_and_oracle(monkeypatch, n_nodes, n_pods):
    """k_class_runs (round 6): the zone-B classes of one (toleration, affinity, spread) signature are written as a RUN — the AND of
    the signature's rows once per run, a class = that & the request-value rows staged in LDS, stored to its member rows. Against
    the chunk writers (YKPRED_TUNE class_runs=0) on the own-template population (every ask its own template: thousands of small
    classes, one to a few rows each) — bitmap, counts, decisions, both phases — and against the oracle."""
    got = {}
    for knob in (0, 1):
        monkeypatch.setenv("YKPRED_TUNE", f"class_runs={knob},class_runs_min_rows={1 if n_nodes == 8300 else 8}")
        m = pkg.GpuPredicateManager()
        try:
            m.generate_kwok(seed=815 + n_nodes, num_nodes=n_nodes, num_pods=n_pods, num_templates=0, node_affinity=1)
            m.evaluate()
            lay = m.layout()
            assert (lay.run_rows > n_pods // 4) if knob else (lay.run_rows == 0), lay.run_rows
            assert m.check_class_rows() == 0
            got[knob] = [unpack(m.read_bitmap(), n_nodes), m.read_counts(), m.read_decisions()]
            m.evaluate(allocate=False)
            got[knob] += [unpack(m.read_bitmap(), n_nodes), m.read_counts()]
            m.evaluate()
            assert np.array_equal(unpack(m.read_bitmap(), n_nodes), got[knob][0]) and np.array_equal(m.read_counts(), got[knob][1])
            if knob:
                o = orc.Oracle(m.dump_snapshot(compact=True))
                sample = np.arange(n_pods) if n_nodes <= 1500 else np.random.default_rng(5).choice(n_pods, size=64, replace=False).astype(np.int32)
                want = o.eval_grid(pods=sample, threads=os.cpu_count() or 8)
                assert np.array_equal(got[knob][0][sample], want)
                assert np.array_equal(got[knob][1][sample], want.sum(axis=1))
                for k, p in enumerate(sample[:12]):
                    assert o.decide(int(p)) == (int(want[k].sum()), int(got[knob][2][p]))
        finally:
            m.close()
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_nodes,n_pods", [(1500, 6000), (8300, 5000), (29000, 3000), (50_000, 4000)],
                         ids=["one-group", "three-groups", "two-segments", "configs2-width"])
def test_fused_rows_equal_chunk_writers_and_oracle(monkeypatch, n_nodes, n_pods):
    """k_fused_rows (round 6): the zone-B classes no run kernel takes — signatures with a handful of rows, asks with a selector of
    their own — written from records resolved at class-build time (the plane rows to AND, the member rows to store; compute waves
    that only load, a store wave that only stores). Against the chunk writers (YKPRED_TUNE fuse_rows=0) on the own-template
    population — bitmap, counts, decisions, both phases, further allocation passes — and against the oracle."""
    got = {}
    for knob in (0, 1):
        monkeypatch.setenv("YKPRED_TUNE", f"fuse_rows={knob},class_runs_min_rows=8")
        m = pkg.GpuPredicateManager()
        try:
            m.generate_kwok(seed=2718 + n_nodes, num_nodes=n_nodes, num_pods=n_pods, num_templates=0, node_affinity=1)
            m.evaluate()
            lay = m.layout()
            assert (lay.fused_rows > n_pods // 100) if knob else (lay.fused_rows == 0), lay.fused_rows
            assert m.check_class_rows() == 0
            got[knob] = [unpack(m.read_bitmap(), n_nodes), m.read_counts(), m.read_decisions()]
            m.evaluate(allocate=False)  # the reservation phase: no request rows, no run kernels, no fused rows
            got[knob] += [unpack(m.read_bitmap(), n_nodes), m.read_counts()]
            m.evaluate()
            assert np.array_equal(unpack(m.read_bitmap(), n_nodes), got[knob][0]) and np.array_equal(m.read_counts(), got[knob][1])
            m.evaluate(decisions=False)
            assert np.array_equal(unpack(m.read_bitmap(), n_nodes), got[knob][0]) and np.array_equal(m.read_counts(), got[knob][1])
            if knob:
                o = orc.Oracle(m.dump_snapshot(compact=True))
                sample = np.arange(n_pods) if n_nodes <= 1500 else np.random.default_rng(5).choice(n_pods, size=64, replace=False).astype(np.int32)
                want = o.eval_grid(pods=sample, threads=os.cpu_count() or 8)
                assert np.array_equal(got[knob][0][sample], want)
                assert np.array_equal(got[knob][1][sample], want.sum(axis=1))
                for k, p in enumerate(sample[:12]):
                    assert o.decide(int(p)) == (int(want[k].sum()), int(got[knob][2][p]))
        finally:
            m.close()
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", range(4))
def test_sweep_writer_random_clusters_two_walked_dimensions(monkeypatch, seed):
    """Random edge-case clusters with every request dimension walked (walk_rows=1) and runs from two rows on: two walked dimensions
    in one request vector (no run: the chunk writers), pinned and duplicated pods, scalar resources, over-committed nodes, zero
    requests — the whole grid, counts, failing plugins and decisions against the oracle."""
    monkeypatch.setenv("YKPRED_TUNE", "walk_rows=1,sweep_min_run=2")
    snap = _gen.random_snapshot(9950 + seed, n_nodes=[64, 130, 333, 700][seed], n_pods=260, scalars=True)
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(snap)
        check_against_oracle(m, snap, True)
        check_against_oracle(m, snap, False)
    finally:
        m.close()


def test_sweep_runs_survive_row_patches(monkeypatch):
    """An ask of a sweep run that leaves (ykpred_update_pods) invalidates the run's row list: the passes after it fall back to the
    chunk writers (which know every chunk) until the next class build; new asks, dirty-column patches and a full re-evaluation
    in between — always the oracle's grid."""
    monkeypatch.setenv("YKPRED_TUNE", "sweep_min_run=2")
    m = pkg.GpuPredicateManager()
    try:
        m.generate_kwok(seed=99, num_nodes=700, num_pods=1500, num_templates=0, node_affinity=1, unique_requests=1)
        m.evaluate()
        assert m.layout().sweep_rows > 500
        snap = json.loads(m.dump_snapshot())
        uids = [p["metadata"]["uid"] for p in snap["pods"]]
        for uid in uids[10:400:13]:
            m.remove_pod(uid)
        m.evaluate_dirty()
        o = orc.Oracle(m.dump_snapshot())
        assert m.layout().sweep_rows == 0  # (the row lists are stale: no sweep until the classes are built again)
        assert np.array_equal(unpack(m.read_bitmap(), 700), o.eval_grid(threads=8))
        m.evaluate()
        lay = m.layout()
        o = orc.Oracle(m.dump_snapshot())
        want = o.eval_grid(threads=8)
        assert lay.num_pods == o.num_pods and np.array_equal(unpack(m.read_bitmap(), 700), want)
        assert np.array_equal(m.read_counts(), want.sum(axis=1))
    finally:
        m.close()


@pytest.mark.parametrize("plugins", [["NodeResourcesFit"], ["TaintToleration", "NodeUnschedulable"], ["NodeAffinity"], ["NodeName"], []])
def test_random_clusters_plugin_subsets(plugins):
    snap = _gen.random_snapshot(77, n_nodes=130, n_pods=80)
    m = pkg.GpuPredicateManager.internal(plugins, plugins, plugins, plugins)
    try:
        m.load_snapshot(snap)
        mask = orc.mask_of(plugins)
        check_against_oracle(m, snap, True, pre=mask, filt=mask)
    finally:
        m.close()


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("allocate", [True, False])
def test_random_clusters_with_topology_spread(pm, seed, allocate):
    """PodTopologySpread (hard constraints, inclusion policies, minDomains, nil/empty selectors, terminating pods,
    other namespaces) — PARITY UNPINNED in the reference; GPU ≡ oracle bit for bit, incl. the failing plugin."""
    snap = _gen.random_snapshot(5000 + seed, n_nodes=60 + 17 * seed, n_pods=70, spread=True)
    pm.load_snapshot(snap)
    check_against_oracle(pm, snap, allocate)


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("allocate", [True, False])
def test_random_clusters_with_inter_pod_affinity(pm, seed, allocate):
    """InterPodAffinity: required affinity (all terms on one pod, self-match escape), anti-affinity, and the symmetry rule
    from existing pods' anti-affinity; namespaces, nil/empty selectors, missing topology keys — combined with spread."""
    snap = _gen.random_snapshot(7000 + seed, n_nodes=50 + 19 * seed, n_pods=70, spread=(seed % 2 == 0), interpod=True)
    pm.load_snapshot(snap)
    check_against_oracle(pm, snap, allocate)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("plugins", [["InterPodAffinity"], ["PodTopologySpread"], ["InterPodAffinity", "PodTopologySpread", "NodePorts"]])
def test_topology_plugins_alone(seed, plugins):
    """Only the topology plugins enabled, so that every verdict of the grid is theirs (with the full default set most
    random pairs already fail an earlier plugin)."""
    snap = _gen.random_snapshot(7200 + seed, n_nodes=64 + 21 * seed, n_pods=80, spread=True, interpod=True)
    m = pkg.GpuPredicateManager.internal(plugins, plugins, plugins, plugins)
    try:
        m.load_snapshot(snap)
        mask = orc.mask_of(plugins)
        o, want = check_against_oracle(m, snap, True, pre=mask, filt=mask)
        assert 0 < want.sum() < want.size, "degenerate case: the plugins accept or reject everything"
    finally:
        m.close()


def test_inter_pod_affinity_filter_without_prefilter():
    snap = _gen.random_snapshot(7100, n_nodes=60, n_pods=40, interpod=True)
    m = pkg.GpuPredicateManager.internal([], [], ["InterPodAffinity"], ["InterPodAffinity"])
    try:
        m.load_snapshot(snap)
        check_against_oracle(m, snap, True, pre=0, filt=orc.PLUGIN_BITS["InterPodAffinity"])
    finally:
        m.close()


def test_topology_spread_filter_without_prefilter():
    snap = _gen.random_snapshot(5100, n_nodes=80, n_pods=40, spread=True)
    m = pkg.GpuPredicateManager.internal([], [], ["PodTopologySpread"], ["PodTopologySpread"])
    try:
        m.load_snapshot(snap)
        check_against_oracle(m, snap, True, pre=0, filt=orc.PLUGIN_BITS["PodTopologySpread"])
    finally:
        m.close()


def test_kwok_with_spread_constraints(pm):
    """configs[4] plugin mix at oracle-feasible size: 10 % of the asks carry one DoNotSchedule zone constraint."""
    # (small on purpose: the oracle re-runs the PreFilter histogram over all nodes for every pair, like the reference)
    pm.generate_kwok(seed=4242, num_nodes=300, num_pods=900, num_templates=200, node_affinity=1, spread=1)
    snap = pm.dump_snapshot()
    assert '"topologySpreadConstraints"' in snap
    check_against_oracle(pm, snap, True, check_plugins=False)
    # incremental: binding an ask changes the selector counts of its node and therefore the histograms
    uid = json.loads(snap)["pods"][5]["metadata"]["uid"]
    pm.assume_pod(uid, "kwok-node-000007")
    assert pm.evaluate_dirty() == 1, "one column patched; the rows of the classes whose histograms moved are rewritten"
    _compare_live_rows(pm, json.loads(pm.dump_snapshot()))


@pytest.mark.parametrize("seed", range(4))
def test_incremental_node_changes_with_topology_constraints(pm, seed):
    """AssumePod / ForgetPod / RemovePod with hard spread constraints AND inter-pod (anti)affinity in the ask population:
    the histograms couple all nodes, so ykpred_eval_nodes rebuilds them, finds the signatures whose PreFilter state moved
    and rewrites the whole rows of their classes — without a full pass. Every live row, count and decision against the
    oracle after every step."""
    import random
    rng = random.Random(100 + seed)
    snap = _gen.random_snapshot(9100 + seed, n_nodes=90 + 20 * seed, n_pods=70, spread=True, interpod=(seed % 2 == 0))
    pm.load_snapshot(snap)
    pm.evaluate()
    names = [n["metadata"]["name"] for n in snap["nodes"] if n["metadata"]["name"]]
    cur, bound, incremental = snap, [], 0
    for step in range(12):
        if bound and rng.random() < 0.3:
            uid, target = bound.pop(rng.randrange(len(bound)))
            pm.remove_pod(uid)
            nodes = json.loads(json.dumps(cur["nodes"]))
            tn = next(n for n in nodes if n["metadata"]["name"] == target)
            tn["pods"] = [q for q in tn["pods"] if q["metadata"]["uid"] != uid]
            cur = {"nodes": nodes, "pods": cur["pods"]}
        else:
            uid = rng.choice([p for p in cur["pods"] if not p["spec"].get("nodeName")])["metadata"]["uid"]
            target = rng.choice(names)
            pm.assume_pod(uid, target)
            bound.append((uid, target))
            cur = _move(cur, uid, target)
        patched = pm.evaluate_dirty(decisions=(step % 2 == 0))
        incremental += patched >= 0
        _compare_live_rows(pm, cur, decisions=(step % 2 == 0))
    # a pod with anti-affinity terms of its own landing on a node extends the dictionaries (full pass); everything else patches
    assert incremental >= 6, f"only {incremental} of 12 steps were incremental"


def test_empty_and_ragged_inputs(pm):
    node = _gen.random_snapshot(5, 1, 0)["nodes"][0]
    pod = _gen.random_snapshot(5, 1, 1)["pods"][0]
    for snap in ({"nodes": [], "pods": []}, {"nodes": [node], "pods": []}, {"nodes": [], "pods": [pod]}):
        pm.load_snapshot(snap)
        pm.evaluate()
        lay = pm.layout()
        assert lay.num_nodes == len(snap["nodes"]) and lay.num_pods == len(snap["pods"])
    # 64 / 65 / 127 / 128 nodes: word boundaries of the bitmap rows
    for n in (63, 64, 65, 127, 128, 129):
        snap = _gen.random_snapshot(300 + n, n_nodes=n, n_pods=20)
        pm.load_snapshot(snap)
        check_against_oracle(pm, snap, True, check_plugins=False)


def test_direct_kernel_matches_plane_path(pm):
    snap = _gen.random_snapshot(4242, n_nodes=333, n_pods=200)
    pm.load_snapshot(snap)
    pm.evaluate()
    a = pm.read_bitmap().copy()
    ca = pm.checksum()
    pm.evaluate(direct=True)
    b = pm.read_bitmap()
    assert np.array_equal(a, b)
    assert pm.checksum() == ca


# ------------------------------------------------------------------------------------------------------------
# KWOK-style clusters from the product's generator; oracle fed the serialised snapshot
# ------------------------------------------------------------------------------------------------------------
def test_kwok_config1_shape_fit_only():
    """configs[0]: 100 nodes × 1k pods, NodeResourcesFit only."""
    ep = ["NodeResourcesFit"]
    m = pkg.GpuPredicateManager.internal(ep, ep, ep, ep)
    try:
        m.generate_kwok(seed=0x59554E49 + 1, num_nodes=100, num_pods=1000, node_affinity=0, tolerations=0)
        snap = m.dump_snapshot()
        mask = orc.mask_of(ep)
        check_against_oracle(m, snap, True, pre=mask, filt=mask)
    finally:
        m.close()


@pytest.mark.parametrize("affinity,templates", [(0, 0), (1, 0), (1, 50)])
def test_kwok_midsize_full_grid(pm, affinity, templates):
    """configs[1]/[2] plugin mixes at a size the oracle finishes in seconds (1.5k nodes × 3k pods = 4.5M pairs)."""
    pm.generate_kwok(seed=0x59554E49 + 2 + affinity, num_nodes=1500, num_pods=3000, num_templates=templates, node_affinity=affinity)
    snap = pm.dump_snapshot()
    o, want = check_against_oracle(pm, snap, True, check_plugins=False)
    # decisions + scores
    scores = pm.read_scores()
    assert np.array_equal(scores.view(np.uint64), o.binpack_scores().view(np.uint64)), "float64 bin-pack score differs bitwise"
    dec = pm.read_decisions()
    order = np.lexsort((np.arange(len(scores)), scores))
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    masked = np.where(want.astype(bool), rank[None, :], np.iinfo(np.int64).max)
    best = np.where(want.any(axis=1), order[np.clip(masked.min(axis=1), 0, len(order) - 1)], -1)
    assert np.array_equal(dec, best.astype(np.int32))
    for p in (0, 17, 2999):
        assert o.decide(p) == (int(want[p].sum()), int(dec[p]))
    # reservation phase on the same cluster
    check_against_oracle(pm, snap, False, check_plugins=False)


def test_kwok_gang_placeholders_share_rows(pm):
    """configs[3] shape: gang placeholder asks — all members of a task group are one pod class (placeholder.go:113-157)."""
    pm.generate_kwok(seed=99, num_nodes=700, num_pods=4000, gang_size=100, node_affinity=1)
    pm.evaluate()
    lay = pm.layout()
    assert lay.num_classes <= 40 + 8  # 40 groups (+ the few pods pinned by nodeName)
    bm = pm.read_bitmap()
    snap = pm.dump_snapshot(pods=np.arange(0, 4000, 37))
    o = orc.Oracle(snap)
    want = o.eval_grid(threads=8)
    assert np.array_equal(unpack(bm[0:4000:37], lay.num_nodes), want)


def test_task_group_placeholders_are_one_class_per_group(pm):
    """configs[3] shape from the real input: the task-groups annotation (pkg/cache/amprotocol.go:47-57) expands into
    minMember identical placeholder asks per group (placeholder.go:40-157) = one pod class, one plane set, shared rows."""
    snap = _gen.random_snapshot(4321, n_nodes=150, n_pods=10, scalars=False)
    pm.load_snapshot(snap)
    groups = [{"name": f"tg-{k}", "minMember": 40 + k, "minResource": {"cpu": f"{250 * (k + 1)}m", "memory": f"{64 * (k + 1)}Mi"},
               "tolerations": [{"operator": "Exists"}] if k % 2 else [],
               "nodeSelector": ({"kubernetes.io/os": "linux"} if k == 2 else {})} for k in range(4)]
    before = pm.num_pods
    pm.evaluate()
    classes_before = pm.layout().num_classes
    assert pm.add_task_groups("spark-app-0001", "root.batch", "default", groups) == sum(g["minMember"] for g in groups)
    # new templates, one of them with a nodeSelector requirement nobody used before: spec rows are appended, the requirement
    # takes a spare dictionary bit (in-place growth), 166 rows join 4 new classes in one ykpred_update_pods call
    pm.evaluate()
    assert pm.check_class_rows() == 0
    assert pm.layout().num_classes <= classes_before + len(groups)
    bm = pm.read_bitmap()
    row = before
    for g in groups:
        assert (bm[row:row + g["minMember"]] == bm[row]).all()
        row += g["minMember"]
    _compare_with_mirror_dump(pm, decisions=True)


def _compare_live_rows(pm, snap_now, decisions=False):
    """Rows of the asks that are still pending (assumed asks keep their row but are skipped) against the oracle."""
    o = orc.Oracle(snap_now)
    want = o.eval_grid(threads=8)
    idx = [pm.pod_index(p["metadata"]["uid"]) for p in snap_now["pods"]]
    lay = pm.layout()
    got = unpack(pm.read_bitmap(), lay.num_nodes)[idx]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} differing bits, first (live pod,node)={bad[0].tolist()}"
    assert np.array_equal(pm.read_counts()[idx], want.sum(axis=1))
    if decisions:
        dec = pm.read_decisions()[idx]
        for k in range(0, len(idx), 7):
            assert o.decide(k) == (int(want[k].sum()), int(dec[k]))


def _move(snap, uid, target):
    """The snapshot after AssumePod(uid → target): the ask leaves the pending list and joins the node's pods."""
    pod = next(p for p in snap["pods"] if p["metadata"]["uid"] == uid)
    moved = dict(pod, spec=dict(pod["spec"], nodeName=target))
    nodes = json.loads(json.dumps(snap["nodes"]))
    next(n for n in nodes if n["metadata"]["name"] == target).setdefault("pods", []).append(moved)
    return {"nodes": nodes, "pods": [p for p in snap["pods"] if p["metadata"]["uid"] != uid]}


def test_incremental_assume_forget(pm):
    """AssumePod / ForgetPod patch one node row and ONE bitmap column (ykpred_eval_nodes) instead of a full pass; asks
    keep their rows (context.go:828-898: the core binds asks one by one between predicate calls)."""
    import random
    rng = random.Random(3)
    snap = _gen.random_snapshot(2024, n_nodes=150, n_pods=60, scalars=False)
    pm.load_snapshot(snap)
    pm.evaluate()
    names = [n["metadata"]["name"] for n in snap["nodes"] if n["metadata"]["name"]]
    cur = snap
    bound = []
    for step in range(14):
        r = rng.random()
        if bound and r < 0.2:
            # ForgetPod (scheduler_cache.go:463-484): the cached pod keeps spec.nodeName and stays accounted on the node; its
            # row now answers like Predicates(cache.GetPod(uid), ...) would: only that node can pass the NodeName filter
            uid, target = bound.pop(rng.randrange(len(bound)))
            pm.forget_pod(uid)
            pod = next(p for p in snap["pods"] if p["metadata"]["uid"] == uid)
            cur = {"nodes": cur["nodes"], "pods": cur["pods"] + [dict(pod, spec=dict(pod["spec"], nodeName=target))]}
            expect_patched = 1  # the node's row is re-accounted (one column) and the ask's row gets its node pin (one row)
        elif bound and r < 0.4:
            # RemovePod of a bound pod (:390-417): it leaves the node and the ask table
            uid, target = bound.pop(rng.randrange(len(bound)))
            pm.remove_pod(uid)
            nodes = json.loads(json.dumps(cur["nodes"]))
            tn = next(n for n in nodes if n["metadata"]["name"] == target)
            tn["pods"] = [q for q in tn["pods"] if q["metadata"]["uid"] != uid]
            cur = {"nodes": nodes, "pods": cur["pods"]}
            expect_patched = 1  # one node column; the vacated row is refilled with the last row's ask
        else:
            uid = rng.choice([p for p in cur["pods"] if not p["spec"].get("nodeName")])["metadata"]["uid"]
            target = rng.choice(names)
            pm.assume_pod(uid, target)
            bound.append((uid, target))
            cur = _move(cur, uid, target)
            expect_patched = 1  # exactly one node column changed
        patched = pm.evaluate_dirty(decisions=(step % 3 == 0))
        assert patched == expect_patched
        _compare_live_rows(pm, cur, decisions=(step % 3 == 0))
    # several nodes touched between two evaluations, some sharing a bitmap word
    free = [p["metadata"]["uid"] for p in cur["pods"] if not p["spec"].get("nodeName")]
    for k in range(5):
        uid = free[k]
        target = names[k * 2]
        pm.assume_pod(uid, target)
        cur = _move(cur, uid, target)
    assert pm.evaluate_dirty() == 5
    _compare_live_rows(pm, cur)
    # a full evaluation afterwards agrees with the patched state
    before = pm.read_bitmap().copy()
    pm.evaluate()
    assert np.array_equal(before, pm.read_bitmap())


def _compare_with_mirror_dump(pm, decisions=False):
    """Every live ask row (uid → row) against the oracle run on the mirror's own snapshot dump. The mirror's bookkeeping
    itself is pinned by tests/test_host_cache.py."""
    snap = json.loads(pm.dump_snapshot())
    o = orc.Oracle(snap)
    want = o.eval_grid(threads=8)
    idx = [pm.pod_index(p["metadata"]["uid"]) for p in snap["pods"]]
    assert min(idx, default=0) >= 0 and len(set(idx)) == len(idx)
    lay = pm.layout()
    assert lay.num_pods == pm.num_pods
    got = unpack(pm.read_bitmap(), lay.num_nodes)[idx]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} differing bits, first (ask,node)={bad[0].tolist()} uid={snap['pods'][bad[0][0]]['metadata']['uid']}"
    assert np.array_equal(pm.read_counts()[idx], want.sum(axis=1))
    if decisions:
        dec = pm.read_decisions()[idx]
        for k in range(len(idx)):
            assert o.decide(k) == (int(want[k].sum()), int(dec[k])), snap["pods"][k]["metadata"]["uid"]
    return snap


@pytest.mark.parametrize("topology", [False, True])
def test_incremental_ask_rows(pm, topology):
    """New asks, finished binds, removed asks and node-pin changes move single rows of the ask table between pod classes
    (ykpred_update_pods) and only those bitmap rows are re-evaluated (ykpred_eval_pods) — no table re-upload, no full pass."""
    import copy
    import random
    rng = random.Random(11)
    snap = _gen.random_snapshot(777, n_nodes=140, n_pods=50, scalars=False, spread=topology, interpod=topology)
    pm.load_snapshot(snap)
    pm.evaluate()
    names = [n["metadata"]["name"] for n in snap["nodes"] if n["metadata"]["name"]]
    asks = [p for p in snap["pods"] if not p["spec"].get("nodeName")]
    live = {p["metadata"]["uid"] for p in snap["pods"]}
    bound = []
    serial = 0
    for step in range(24):
        r = rng.random()
        want_dec = step % 2 == 0
        if r < 0.35:  # a new ask whose template is already known (a deployment scaling up): row appended
            src = copy.deepcopy(rng.choice(asks))
            serial += 1
            src["metadata"].update(uid=f"new-{serial}", name=f"new-{serial}")
            pm.update_pod(src)
            live.add(src["metadata"]["uid"])
        elif r < 0.55 and live:  # an ask goes away (deleted): its row is refilled with the last row's ask
            uid = rng.choice(sorted(live))
            pm.remove_pod(uid)
            live.discard(uid)
            bound = [b for b in bound if b != uid]
        elif r < 0.8:  # AssumePod, later completed by the informer update (Running) which drops the row
            cands = sorted(u for u in live if u not in bound and pm.pod_state(u) and not pm.pod_state(u)["node"])
            if not cands:
                continue
            uid = rng.choice(cands)
            pm.assume_pod(uid, rng.choice(names))
            bound.append(uid)
        elif bound:
            uid = bound.pop(0)
            if rng.random() < 0.5:
                pm.forget_pod(uid)  # row pinned to the node it was assumed on
            else:
                pod = next((p for p in snap["pods"] if p["metadata"]["uid"] == uid), None)
                if pod is None:
                    continue
                pm.update_pod(dict(pod, status={"phase": "Running"}))
                live.discard(uid)
        else:
            continue
        patched = pm.evaluate_dirty(decisions=want_dec, profile=True)
        kernels = [k for k, _ in pm.timing()["kernels"]]
        if patched >= 0:
            assert "k_combine" not in kernels, kernels
        _compare_with_mirror_dump(pm, decisions=want_dec)
    # the patched state equals a full evaluation of the same tables
    before = pm.read_bitmap().copy()
    pm.evaluate()
    assert np.array_equal(before, pm.read_bitmap())
    _compare_with_mirror_dump(pm, decisions=True)


def test_incremental_node_object_updates(pm):
    """SchedulerCache.UpdateNode of a known node (scheduler_cache.go:173-177): allocatable, labels, taints, unschedulable.
    As long as no dictionary grows only that node's row is re-encoded and ONE bitmap column is re-evaluated."""
    snap = _gen.random_snapshot(99, n_nodes=120, n_pods=60, scalars=False)
    pm.load_snapshot(snap)
    pm.evaluate()
    nodes = {n["metadata"]["name"]: n for n in snap["nodes"] if n["metadata"]["name"]}
    names = sorted(nodes)
    donor_taints = next(n["spec"]["taints"] for n in snap["nodes"] if n["spec"].get("taints"))
    donor_labels = next(n["metadata"]["labels"] for n in snap["nodes"] if n["metadata"].get("labels"))

    def strip(n):
        return {k: v for k, v in n.items() if k != "pods"}

    edits = [
        lambda n: n["status"]["allocatable"].update(cpu="1", memory="1Mi"),
        lambda n: n["metadata"].update(labels=dict(donor_labels)),
        lambda n: n["spec"].update(unschedulable=True),
        lambda n: n["spec"].update(taints=list(donor_taints)),
        lambda n: n["spec"].update(taints=[], unschedulable=False),
        lambda n: n["metadata"].update(labels={}),
    ]
    for k, edit in enumerate(edits):
        n = json.loads(json.dumps(strip(nodes[names[(k * 17) % len(names)]])))
        n.setdefault("spec", {})
        n.setdefault("status", {}).setdefault("allocatable", {})
        n.setdefault("metadata", {})
        edit(n)
        assert pm.update_node(n) == 0
        assert pm.evaluate_dirty(decisions=True) == 1
        _compare_with_mirror_dump(pm, decisions=True)
    # a taint nobody carried before extends the taint dictionary: everything is re-encoded, and still exact
    n = json.loads(json.dumps(strip(nodes[names[3]])))
    n.setdefault("spec", {})["taints"] = [{"key": "brand-new", "value": "x", "effect": "NoSchedule"}]
    pm.update_node(n)
    assert pm.evaluate_dirty(decisions=True) == -1
    _compare_with_mirror_dump(pm, decisions=True)


def test_update_pods_argument_checks(pm):
    """The C entry point itself: bad row lists are refused and leave the table untouched."""
    snap = _gen.random_snapshot(5, n_nodes=70, n_pods=20, scalars=False)
    pm.load_snapshot(snap)
    pm.evaluate()
    P = pm.num_pods
    before = pm.read_bitmap().copy()

    def call(after, rows, specs, pins):
        r, sp, pi = (np.asarray(x, dtype=np.int32) for x in (rows, specs, pins))
        return pm._P.ykpred_update_pods(pm.engine, after, len(r), r.ctypes.data, sp.ctypes.data, pi.ctypes.data)

    assert call(P, [1, 1], [0, 0], [-1, -1]) < 0          # a row listed twice
    assert call(P + 2, [P], [0], [-1]) < 0                 # an appended row is not listed
    assert call(P, [P], [0], [-1]) < 0                     # row beyond the table
    assert call(P, [0], [10_000], [-1]) < 0                # unknown spec
    assert call(P, [0], [0], [10_000]) < 0                 # node index out of range
    assert pm.layout().num_pods == P
    assert np.array_equal(before, pm.read_bitmap())
    # a valid call straight at the C ABI: row 2 takes spec 0 unpinned, the row patch then equals the per-pair answers
    import ctypes
    ffi = importlib.import_module("yunikorn-k8shim_amd._ffi")
    assert call(P, [2], [0], [-1]) == 0
    a = ffi.YkpredEvalArgs()
    a.prefilter_plugins, a.filter_plugins = pm._masks[1], pm._masks[3]
    a.options = 1 | 2
    row = np.array([2], dtype=np.int32)
    assert pm._P.ykpred_eval_pods(pm.engine, ctypes.byref(a), 1, row.ctypes.data) == 0
    N = pm.num_nodes
    fit, _, _ = pm.query(np.full(N, 2, dtype=np.int32), np.arange(N, dtype=np.int32))
    assert np.array_equal(unpack(pm.read_bitmap(2, 1), N)[0], fit)
    assert pm.read_counts()[2] == fit.sum()


def test_column_patch_never_reads_a_stale_representative_row(pm):
    """Found by scripts/fuzz_incremental.py: when the LAST row is the representative of its class and moves into a vacated
    row in the same batch that touches a node, the column patch must take the class's old word from a member whose bitmap
    row is current — not from the moved row, which still holds the vacated ask's bits."""
    def ask(uid, cpu):
        return {"metadata": {"name": uid, "uid": uid}, "spec": {"containers": [{"resources": {"requests": {"cpu": cpu}}}]}}

    nodes = [{"metadata": {"name": f"n{i:02d}"}, "status": {"allocatable": {"cpu": "8", "memory": "8Gi", "pods": "20"}}} for i in range(70)]
    pods = [ask("x0", "1"), ask("x1", "2"), ask("x2", "1000"), ask("x3", "3"), ask("x4", "4"), ask("b2", "500m")]
    pm.load_snapshot({"nodes": nodes, "pods": pods})
    pm.evaluate()
    pm.update_pod(ask("b3", "500m"))  # same class as b2, appended as row 6
    pm.remove_pod("x1")                # row 1 is refilled with the last row: b3
    assert pm.evaluate_dirty(decisions=True) == 0
    assert (pm.pod_index("b3"), pm.pod_index("b2")) == (1, 5)  # b2, the class's representative, is now the last row
    pm.assume_pod("x3", "n03")         # touches a node of bitmap word 0 ...
    pm.remove_pod("x2")                # ... and vacates row 2 (an ask that fits nowhere): b2 moves there
    assert pm.evaluate_dirty(decisions=True) == 1
    assert pm.pod_index("b2") == 2
    _compare_with_mirror_dump(pm, decisions=True)
    before = pm.read_bitmap().copy()
    pm.evaluate()
    assert np.array_equal(before, pm.read_bitmap())


def test_graph_replay_matches_plain_launches(monkeypatch):
    """YKPRED_TUNE graph=1: a pass that repeats unchanged is captured into a hipGraph the second time and replayed afterwards;
    table changes in between invalidate the capture. Results must not depend on the launch mode."""
    monkeypatch.setenv("YKPRED_TUNE", "graph=1")
    m = pkg.GpuPredicateManager()
    try:
        snap = _gen.random_snapshot(808, n_nodes=130, n_pods=50, spread=True, interpod=True)
        m.load_snapshot(snap)
        for _ in range(4):  # plain, capture + replay, replay, replay
            check_against_oracle(m, snap, True, check_plugins=False)
        check_against_oracle(m, snap, False, check_plugins=False)  # other plugin lists: another graph
        free = next(p["metadata"]["uid"] for p in snap["pods"] if not p["spec"].get("nodeName"))
        m.assume_pod(free, snap["nodes"][3]["metadata"]["name"] or snap["nodes"][4]["metadata"]["name"])
        for _ in range(3):
            m.evaluate()
            _compare_with_mirror_dump(m, decisions=True)
    finally:
        m.close()


def test_new_template_covered_by_the_dictionaries_is_a_row_patch(pm):
    """A new pod template whose selector requirements, scalar resources, host ports and topology classes are already in the
    dictionaries only appends a spec row (ykpred_set_specs keeps the pod classes for an append): no re-encode, no full pass."""
    snap = _gen.random_snapshot(515, n_nodes=120, n_pods=40, scalars=False)
    pm.load_snapshot(snap)
    pm.evaluate()
    stats = pm.stats()
    donor = next(p for p in snap["pods"] if p["spec"].get("nodeSelector") or p["spec"].get("affinity"))
    new = json.loads(json.dumps(donor))
    new["metadata"].update(uid="fresh", name="fresh", labels={"only": "here"})   # a template nobody has ...
    new["spec"].pop("nodeName", None)
    new["spec"]["containers"] = [{"resources": {"requests": {"cpu": "123m", "memory": "77Mi"}}}]  # ... with its own requests
    pm.update_pod(new)
    assert pm.evaluate_dirty(decisions=True, profile=True) == 0
    assert [k for k, _ in pm.timing()["kernels"]] == ["k_rows", "k_rows_finish"]
    after = pm.stats()
    assert after["specs"] == stats["specs"] + 1 and after["requirements"] == stats["requirements"]
    _compare_with_mirror_dump(pm, decisions=True)
    # a requirement nobody used before takes a spare dictionary bit in place (one label-word column uploaded): still a row patch
    other = json.loads(json.dumps(new))
    other["metadata"].update(uid="fresh-2", name="fresh-2")
    other["spec"]["nodeSelector"] = {"never-seen-key": "v"}
    pm.update_pod(other)
    assert pm.evaluate_dirty(decisions=True) == 0
    assert pm.stats()["requirements"] == stats["requirements"] + 1
    _compare_with_mirror_dump(pm, decisions=True)
    # a scalar resource nobody requested before adds a resource dimension: that does re-encode everything, still exact
    third = json.loads(json.dumps(new))
    third["metadata"].update(uid="fresh-3", name="fresh-3")
    third["spec"]["containers"] = [{"resources": {"requests": {"example.com/never-seen": "1"}}}]
    pm.update_pod(third)
    assert pm.evaluate_dirty(decisions=True) == -1
    _compare_with_mirror_dump(pm, decisions=True)
    before = pm.read_bitmap().copy()
    pm.evaluate()
    assert np.array_equal(before, pm.read_bitmap())


@pytest.mark.parametrize("tune,first,count,steps", [("", 710040, 10, 25), ("walk_rows=1,sweep_min_run=1,class_runs_min_rows=1", 108, 10, 40)],
                         ids=["default", "every-dimension-walked-every-class-in-a-run"])
def test_incremental_fuzz_seeds(tune, first, count, steps):
    """A short slice of scripts/fuzz_incremental.py (random cache-operation sequences, every live row / count / decision
    checked against the oracle after every evaluate_dirty) so that every GPU run of the suite re-plays it. The second slice forces
    index rows and the run writers / run-level decisions on these small clusters (round 6: seeds 111 and 115 found the classes that
    row patches add after a build in neither of k_run_decide's and k_decide's lists — their decisions stayed what they were)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "fuzz_incremental.py"), str(first), str(count), str(steps)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, YKPRED_TUNE=tune) if tune else None)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 failures" in r.stdout


def test_incremental_rows_use_the_row_kernels(pm):
    snap = _gen.random_snapshot(31, n_nodes=100, n_pods=30, scalars=False)
    pm.load_snapshot(snap)
    pm.evaluate()
    src = json.loads(json.dumps(snap["pods"][3]))
    src["metadata"].update(uid="extra", name="extra")
    src["spec"].pop("nodeName", None)
    pm.update_pod(src)
    assert pm.evaluate_dirty(decisions=True, profile=True) == 0  # no node column, one row
    assert [k for k, _ in pm.timing()["kernels"]] == ["k_rows", "k_rows_finish"]
    assert pm.num_pods == len(snap["pods"]) + 1 and pm.pod_index("extra") == len(snap["pods"])
    _compare_with_mirror_dump(pm, decisions=True)


def test_incremental_at_full_size(pm):
    """configs[2] size: AssumePod → one column patch; new asks / finished binds → single row patches. Checked against the
    per-pair kernel on that column and against a full re-evaluation (checksum of the whole bitmap)."""
    pm.generate_kwok(seed=0x59554E49 + 21, num_nodes=50_000, num_pods=1_000_000, num_templates=2000, node_affinity=1)
    pm.evaluate()
    node = "kwok-node-012345"
    n_idx = pm.node_index(node)
    for uid in ("pod-0000017", "pod-0000018", "pod-0000019"):
        pm.assume_pod(uid, node)
    assert pm.evaluate_dirty() == 1
    patched_sum = pm.checksum()
    col = pm.read_bitmap(0, 4096)[:, n_idx >> 6]
    fit, _, _ = pm.query(np.arange(4096, dtype=np.int32), np.full(4096, n_idx, dtype=np.int32))
    assert np.array_equal((col >> np.uint64(n_idx & 63)) & np.uint64(1), fit.astype(np.uint64))
    pm.evaluate()
    assert pm.checksum() == patched_sum
    # ask rows: three new asks of known templates are appended, one bind completes (its row is refilled with the last ask)
    classes = pm.layout().num_classes
    for k, src_row in enumerate((5, 123_456, 999_999)):
        ask = json.loads(pm.dump_snapshot(pods=[src_row], nodes=[]))["pods"][0]
        ask["metadata"].update(uid=f"late-{k}", name=f"late-{k}")
        ask["spec"].pop("nodeName", None)
        pm.update_pod(ask)
    done = json.loads(pm.dump_snapshot(pods=[40], nodes=[]))["pods"][0]
    pm.assume_pod(done["metadata"]["uid"], node)
    pm.update_pod(dict(done, status={"phase": "Running"}))
    assert pm.num_pods == 1_000_002 and pm.pod_index("late-2") == 40 and pm.pod_index(done["metadata"]["uid"]) == -1
    assert pm.evaluate_dirty(decisions=True, profile=True) == 1
    assert "k_combine" not in [k for k, _ in pm.timing()["kernels"]]
    assert pm.layout().num_pods == 1_000_002 and pm.layout().num_classes <= classes + 3
    rows = np.array([40, 1_000_000, 1_000_001, 7], dtype=np.int32)
    nodes = np.random.default_rng(5).integers(0, 50_000, size=(4, 3000)).astype(np.int32)
    fit, _, _ = pm.query(np.repeat(rows, 3000), nodes.reshape(-1))
    bm = pm.read_bitmap(0, 1_000_002)
    got = (bm[np.repeat(rows, 3000), nodes.reshape(-1) >> 6] >> (nodes.reshape(-1) & 63).astype(np.uint64)) & np.uint64(1)
    assert np.array_equal(got, fit.astype(np.uint64))
    counts, dec = pm.read_counts(), pm.read_decisions()
    patched_sum = pm.checksum()
    pm.evaluate()
    assert pm.checksum() == patched_sum
    assert np.array_equal(counts, pm.read_counts()) and np.array_equal(dec, pm.read_decisions())


def test_decisions_break_score_ties_by_node_id(pm):
    """Bin-pack order = ascending score, ties by NodeID STRING (yunikorn-core sorts nodes by score, then node id —
    recollection, parity unpinned): the host uploads each node's position in name order (ykpred_nodes_t.name_rank)."""
    names = ["node-b", "node-10", "node-9", "node-a", "node-1"]
    alloc = {"cpu": "4", "memory": "8Gi", "pods": "10"}
    busy = {"metadata": {"name": "busy", "uid": "busy"}, "spec": {"containers": [{"resources": {"requests": {"cpu": "1"}}}]}}
    nodes = [{"metadata": {"name": n, "labels": {"g": "x" if i % 2 else "y"}}, "status": {"allocatable": alloc}} for i, n in enumerate(names)]
    nodes.append({"metadata": {"name": "node-0", "labels": {"g": "x"}}, "status": {"allocatable": alloc}, "pods": [busy]})  # better score, alone
    pods = [{"metadata": {"name": "any", "uid": "any"}, "spec": {"containers": []}},
            {"metadata": {"name": "y", "uid": "y"}, "spec": {"nodeSelector": {"g": "y"}, "containers": []}},
            {"metadata": {"name": "idle", "uid": "idle"}, "spec": {"containers": [],
                                                              "affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
                                                                  {"matchFields": [{"key": "metadata.name", "operator": "NotIn", "values": ["node-0"]}]}]}}}}}]
    snap = {"nodes": nodes, "pods": pods}
    pm.load_snapshot(snap)
    pm.evaluate()
    o = orc.Oracle(snap)
    dec = pm.read_decisions()
    assert [o.decide(p)[1] for p in range(3)] == dec.tolist()
    # "any": the busier node-0 wins on score; "y": among the idle g=y nodes (node-b, node-9, node-1) the smallest NAME is node-1;
    # "idle": all idle nodes tie → node-1 ("node-1" < "node-10" < "node-9" < "node-a" < "node-b")
    assert dec.tolist() == [5, 4, 4]


def test_unsupported_asks_are_routed_individually(pm):
    """Asks the engine does not evaluate (a PVC volume, a DRA claim, a pod-affinity namespaceSelector WITH requirements, a repeated topologyKey)
    are marked one by one: their rows are all zero, count 0, decision -1, Predicates() answers "route to the CPU manager"
    (YKHOST_E_UNSUPPORTED) — and every OTHER ask of the same snapshot is evaluated as usual, bit for bit the oracle's."""
    snap = _gen.random_snapshot(3131, n_nodes=90, n_pods=40)
    def odd(i, spec_extra):
        p = json.loads(json.dumps(snap["pods"][i]))
        p["metadata"]["uid"] = p["metadata"]["name"] = f"odd-{i}"
        p.setdefault("spec", {}).update(spec_extra)
        return p
    odd_pods = [
        odd(0, {"volumes": [{"name": "data", "persistentVolumeClaim": {"claimName": "pvc-1"}}]}),
        odd(1, {"resourceClaims": [{"name": "gpu", "resourceClaimName": "claim-1"}]}),
        odd(2, {"affinity": {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
            {"topologyKey": "zone", "labelSelector": {}, "namespaceSelector": {"matchLabels": {"team": "a"}}}]}}}),
        odd(3, {"topologySpreadConstraints": [
            {"maxSkew": 1, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": {"a": "b"}}},
            {"maxSkew": 2, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": {"c": "d"}}}]}),
        odd(4, {"volumes": [{"name": "scratch", "emptyDir": {}}, {"name": "cfg", "configMap": {"name": "x"}}]}),  # node-local: supported
    ]
    mixed = {"nodes": snap["nodes"], "pods": snap["pods"] + odd_pods}
    pm.load_snapshot(mixed)
    pm.evaluate()
    P0 = len(snap["pods"])
    want = orc.Oracle(snap).eval_grid(threads=8)
    rows = unpack(pm.read_bitmap(), len(snap["nodes"]))
    assert np.array_equal(rows[:P0], want)
    counts, dec = pm.read_counts(), pm.read_decisions()
    reasons = []
    for k in range(4):
        ok, why = pm.ask_supported(P0 + k)
        assert not ok and why
        reasons.append(why)
        assert rows[P0 + k].sum() == 0 and counts[P0 + k] == 0 and dec[P0 + k] == -1
        with pytest.raises(pkg.UnsupportedAsk):
            pm.predicates(P0 + k, 0, True)
        with pytest.raises(pkg.UnsupportedAsk):
            pm.is_pod_fit_node(f"odd-{k}", snap["nodes"][0]["metadata"]["name"], True)
    assert "persistentVolumeClaim" in reasons[0] and "resourceClaims" in reasons[1] and "namespaceSelector" in reasons[2] and "topologyKey" in reasons[3]
    assert pm.ask_supported(P0 + 4) == (True, "")
    assert np.array_equal(rows[P0 + 4], want[4])  # emptyDir / configMap volumes change nothing
    fit, code, _ = pm.query(np.full(5, P0, dtype=np.int32), np.arange(5, dtype=np.int32))
    assert not fit.any() and (code == 255).all()
    st = pm.routing_stats()
    assert st["unsupported_asks"] == 4 and st["routed_to_cpu"] >= 8


@pytest.mark.parametrize("count", [700, 2100])
def test_large_requirement_dictionaries_and_overflow(pm, count):
    """`count` asks that each select a different kubernetes.io/hostname need `count` requirement bits. 700 of them
    (the probe that used to take the engine away from every ask) fit: the bit-sliced plane kernels size the
    dictionary at run time and the per-pair kernels read label words beyond their 8 register-held ones from the node table.
    The dictionary holds 2048 requirements: beyond that the overflowing asks — and only they — are routed to the CPU manager."""
    nodes = [{"metadata": {"name": f"n{i}", "labels": {"kubernetes.io/hostname": f"n{i}", "zone": f"z{i % 3}"}},
              "status": {"allocatable": {"cpu": "8", "memory": "16Gi", "pods": "20"}}} for i in range(count)]
    pods = [{"metadata": {"name": f"p{i}", "uid": f"p{i}"},
             "spec": {"nodeSelector": {"kubernetes.io/hostname": f"n{i}"}, "containers": [{"resources": {"requests": {"cpu": "1"}}}]}} for i in range(count)]
    pods.insert(0, {"metadata": {"name": "plain", "uid": "plain"}, "spec": {"nodeSelector": {"zone": "z1"}, "containers": []}})
    snap = {"nodes": nodes, "pods": pods}
    pm.load_snapshot(snap)
    pm.evaluate()
    supported = np.array([pm.ask_supported(i)[0] for i in range(count + 1)])
    fit_in = min(count + 1, 2048)  # first come, first served: "plain" takes one bit, the hostname selectors the rest
    assert supported[:fit_in].all() and not supported[fit_in:].any()
    want = orc.Oracle(snap).eval_grid(threads=os.cpu_count() or 8)
    rows = unpack(pm.read_bitmap(), count)
    assert np.array_equal(rows[supported], want[supported]) and rows[~supported].sum() == 0
    assert pm.predicates("plain", "n1", True) == ("", None)
    for i in (5, 511, 512, 640, 699):  # requirement bits below and above the 8 register-held words, per-pair path
        assert pm.predicates(f"p{i}", f"n{i}", True) == ("", None)
        plugin, err = pm.predicates(f"p{i}", f"n{(i + 1) % count}", True)
        assert plugin == "NodeAffinity" and err is not None
    if count > 2048:
        assert "requirements" in pm.ask_supported(2090)[1]
        with pytest.raises(pkg.UnsupportedAsk):
            pm.predicates("p2090", "n2090", True)


def test_dictionary_growth_in_place(pm):
    """An ask whose nodeSelector / affinity uses requirements nobody used before: the requirement gets a spare dictionary bit,
    the bit is evaluated on every node and ONE label-word column is uploaded (ykpred_update_label_word) — the cluster is not
    re-encoded, the engine keeps its bitmap, the new ask is an ordinary appended row."""
    snap = _gen.random_snapshot(616, n_nodes=140, n_pods=50, scalars=False)
    for i, n in enumerate(snap["nodes"]):
        n["metadata"].setdefault("labels", {})["rack"] = f"r{i % 7}"
        n["metadata"]["labels"]["tier"] = str(i % 5)
    pm.load_snapshot(snap)
    pm.evaluate()
    growths_before = pm.routing_stats()["dictionary_growths"]  # the fixture is shared: the counter is cumulative
    late = [
        {"metadata": {"name": "late-0", "uid": "late-0"}, "spec": {"nodeSelector": {"rack": "r3"}, "containers": []}},
        {"metadata": {"name": "late-1", "uid": "late-1"}, "spec": {"containers": [], "affinity": {"nodeAffinity": {
            "requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
                {"matchExpressions": [{"key": "tier", "operator": "Gt", "values": ["2"]}, {"key": "rack", "operator": "NotIn", "values": ["r1", "r2"]}]},
                {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [snap["nodes"][9]["metadata"]["name"]]}]}]}}}}},
        {"metadata": {"name": "late-2", "uid": "late-2"}, "spec": {"nodeSelector": {"rack": "r3"}, "containers": [{"resources": {"requests": {"cpu": "100m"}}}]}},
    ]
    cur = snap
    for k, ask in enumerate(late):
        pm.update_pod(ask)
        assert pm.evaluate_dirty(decisions=True) >= 0, "a new selector requirement must not force a full pass"
        cur = {"nodes": cur["nodes"], "pods": cur["pods"] + [ask]}
        _compare_live_rows(pm, cur, decisions=True)
    st = pm.routing_stats()
    assert st["dictionary_growths"] == growths_before + 2, st  # late-2 reuses late-0's requirement
    before = pm.read_bitmap().copy()
    pm.evaluate()
    assert np.array_equal(before, pm.read_bitmap())


def test_node_ports_preemption(pm):
    """PreemptionPredicates with NodePorts: removing the victim that holds the port frees it (NodeInfo.UsedPorts)."""
    def holder(uid, port):
        return {"metadata": {"name": uid, "uid": uid}, "spec": {"containers": [{"ports": [{"hostPort": port, "protocol": "TCP"}]}]}}
    node = {"metadata": {"name": "n0"}, "status": {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": "10"}},
            "pods": [holder("v0", 81), holder("v1", 80), holder("v2", 82)]}
    ask = {"metadata": {"name": "ask", "uid": "ask"}, "spec": {"containers": [{"ports": [{"hostPort": 80, "hostIP": "10.0.0.1"}]}]}}
    snap = {"nodes": [node], "pods": [ask]}
    pm.load_snapshot(snap)
    o = orc.Oracle(snap)
    for victims, start in ((["v0", "v1", "v2"], 0), (["v0", "v2"], 0), (["v1"], 0), (["v0", None, "v1"], 1), ([], 0)):
        idx = [-1 if v is None else ["v0", "v1", "v2"].index(v) for v in victims]
        assert pm.preemption_predicates("ask", "n0", victims, start) == o.preemption(0, 0, idx, start), (victims, start)
    assert pm.preemption_predicates("ask", "n0", ["v0", "v1", "v2"], 0) == 1


# ------------------------------------------------------------------------------------------------------------
# BASELINE.json sizes: properties + oracle on a sample (the oracle cannot finish 5e10 pairs)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes,n_pods,affinity", [(10_000, 100_000, 0), (50_000, 1_000_000, 1)])
def test_full_size_configs(pm, n_nodes, n_pods, affinity):
    """configs[1] (10k × 100k, Fit + TaintToleration) and configs[2] (50k × 1M, + NodeAffinity)."""
    pm.generate_kwok(seed=0x59554E49 + 10 + affinity, num_nodes=n_nodes, num_pods=n_pods, num_templates=2000, node_affinity=affinity)
    pm.evaluate()
    lay = pm.layout()
    assert (lay.num_nodes, lay.num_pods) == (n_nodes, n_pods)
    sum_plane = pm.checksum()
    rng = np.random.default_rng(7)
    pods = np.sort(rng.choice(n_pods, 96, replace=False)).astype(np.int32)
    nodes = np.sort(rng.choice(n_nodes, 1200, replace=False)).astype(np.int32)
    rows = np.stack([pm.read_bitmap(int(p), 1)[0] for p in pods])
    counts = pm.read_counts()
    # (1) sampled pods × sampled nodes against the oracle, per pair
    o = orc.Oracle(pm.dump_snapshot(pods=pods, nodes=nodes))
    want = o.eval_grid(threads=8)
    got = unpack(rows, n_nodes)[:, nodes]
    assert np.array_equal(got, want)
    # (2) popcount of every sampled row == the reported feasible count; padding bits are zero
    assert np.array_equal(unpack(rows, lay.row_words * 64).sum(axis=1), counts[pods])
    assert unpack(rows, lay.row_words * 64)[:, n_nodes:].sum() == 0
    # (3) the device per-pair kernel (k_query) agrees on 200k random pairs
    qp = rng.integers(0, n_pods, 200_000).astype(np.int32)
    qn = rng.integers(0, n_nodes, 200_000).astype(np.int32)
    fit, _, _ = pm.query(qp, qn)
    sample_rows = {int(p): None for p in np.unique(qp[:2000])}
    for p in sample_rows:
        sample_rows[p] = pm.read_bitmap(p, 1)[0]
    for i in range(2000):
        w = sample_rows[int(qp[i])][qn[i] >> 6]
        assert ((int(w) >> int(qn[i] & 63)) & 1) == fit[i]
    # (4) checksum of checksums: the independent per-pair formulation (k_direct) reproduces the whole bitmap
    pm.evaluate(direct=True, counts=False, decisions=False)
    assert pm.checksum() == sum_plane


@pytest.mark.parametrize("unique", [1, 0], ids=["a-request-of-its-own-per-ask", "a-template-of-its-own-per-ask"])
def test_full_size_small_class_populations(pm, unique):
    """The two small-class populations of bench.py at configs[2] size (50 000 nodes x 10^6 asks) — the run writers (k_sweep_rows /
    k_class_runs), the run-level decisions and what is left to the chunk writers: every member row = its class's row
    (k_check_class_rows), the whole bitmap's checksum = the independent per-pair kernel's (k_direct evaluates every one of the
    5e10 pairs from the tables), 48 sampled classes x all nodes, their counts and their decisions against the oracle."""
    pm.generate_kwok(seed=0x59554E49 + 40 + unique, num_nodes=50_000, num_pods=1_000_000, num_templates=0, node_affinity=1, unique_requests=unique)
    pm.evaluate()
    lay = pm.layout()
    assert (lay.sweep_rows > 900_000) if unique else (lay.run_rows > 250_000), (lay.sweep_rows, lay.run_rows)
    assert pm.check_class_rows() == 0
    plane_sum = pm.checksum()
    counts, dec = pm.read_counts(), pm.read_decisions()
    pod_class, rep = pm.pod_classes()
    sample = np.sort(np.random.default_rng(11).choice(len(rep), 48, replace=False))
    reps = rep[sample].astype(np.int32)
    o = orc.Oracle(pm.dump_snapshot(pods=reps, compact=True))
    want = o.eval_grid(threads=os.cpu_count() or 8)
    assert np.array_equal(unpack(pm.read_rows(reps), 50_000), want)
    assert np.array_equal(counts[reps], want.sum(axis=1))
    for k in range(len(reps)):
        assert o.decide(k) == (int(want[k].sum()), int(dec[reps[k]])), k
    assert np.array_equal(dec, dec[rep][pod_class]) and np.array_equal(counts, counts[rep][pod_class])
    pm.evaluate(direct=True, counts=False, decisions=False)
    assert pm.checksum() == plane_sum
    o.close()


@pytest.mark.parametrize("n_nodes,n_pods,affinity,gang,spread", [(10_000, 100_000, 0, 0, 0), (50_000, 1_000_000, 1, 0, 0), (50_000, 1_000_000, 1, 100, 0),
                                                                 (100_000, 1_000_000, 1, 0, 1), (100_000, 5_000_000, 1, 0, 1)],
                         ids=["configs1", "configs2", "configs3-gang", "configs4-shape", "configs4-size"])
def test_full_grid_oracle_parity(pm, n_nodes, n_pods, affinity, gang, spread):
    """EVERY (pod, node) pair of configs[1], configs[2], the configs[3] gang shape and the configs[4] shape (100 000 nodes,
    the full Filter set incl. hard PodTopologySpread constraints, 10^6 asks) against the oracle (predicate_manager.go:206-283
    per pair): the oracle evaluates one representative ask per pod class against all N nodes — C x N Predicates() calls, 1e8
    for configs[2] — and the device proves that each of the P rows equals the row of its class's representative (and that
    every padding word is zero). Together: all P x N bits are the oracle's. configs4-size is BASELINE configs[4] at its own size —
    100 000 nodes x 5 000 000 asks, a 62.6 GB bitmap of 7.8e9 words: the first layout past 2^32 words, where an index-width
    defect would live (the oracle's cost is per class, not per ask). The DECISIONS (the metric's second half) are
    checked at the same size: for every class the first feasible node of the oracle's row in the oracle's bin-pack order
    (score, then NodeID) must be the decision of every member."""
    import time
    pm.generate_kwok(seed=0x59554E49 + 20 + affinity + gang + 7 * spread, num_nodes=n_nodes, num_pods=n_pods, num_templates=2000,
                     node_affinity=affinity, gang_size=gang, spread=spread)
    pm.evaluate()
    lay = pm.layout()
    assert (lay.num_nodes, lay.num_pods) == (n_nodes, n_pods)
    pod_class, rep = pm.pod_classes()
    assert len(rep) == lay.num_classes and (rep >= 0).all()
    assert np.array_equal(pod_class[rep], np.arange(len(rep))), "a representative must belong to its own class"
    assert pm.check_class_rows() == 0
    t0 = time.perf_counter()
    o = orc.Oracle(pm.dump_snapshot(pods=rep, compact=True))
    assert (o.num_pods, o.num_nodes) == (len(rep), n_nodes)
    # hard spread constraints: the per-pair form of the oracle costs O(N) node visits per PAIR; the per-pod form gives the same
    # verdicts (tests/test_oracle_golden.py::test_prefilter_once_form_equals_the_per_pair_form)
    want = o.eval_grid(threads=os.cpu_count() or 8, prefilter_once=bool(spread))
    t_oracle = time.perf_counter() - t0
    got = unpack(pm.read_rows(rep), n_nodes)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} representative pairs differ from the oracle"
    counts = pm.read_counts()
    assert np.array_equal(counts, want.sum(axis=1)[pod_class])
    # ---- decisions at the metric's size. Bin-pack order of the ORACLE: ascending score, ties by NodeID string (KWOK node names
    # are zero-padded: name order = index order); decision of a class = first feasible node of its oracle row in that order.
    scores = o.binpack_scores()
    assert np.array_equal(scores, pm.read_scores()), "float64 bin-pack scores must be bit-identical"
    order = np.lexsort((np.arange(n_nodes), scores))
    in_order = want[:, order]
    first = in_order.argmax(axis=1)
    want_dec = np.where(in_order[np.arange(len(rep)), first] != 0, order[first], -1).astype(np.int32)
    for c in np.random.default_rng(3).choice(len(rep), 24, replace=False):  # the shortcut above IS the oracle's decide()
        assert o.decide(int(c), prefilter_once=bool(spread)) == (int(want[c].sum()), int(want_dec[c]))
    dec = pm.read_decisions()
    assert np.array_equal(dec, want_dec[pod_class]), f"{int((dec != want_dec[pod_class]).sum())} of {n_pods} decisions differ from the oracle"
    print(f"full grid {n_pods} x {n_nodes}: {len(rep)} classes x {n_nodes} nodes = {want.size} oracle calls in {t_oracle:.1f} s, "
          f"{int((want_dec >= 0).sum())} classes with a feasible node")
    if n_pods > 1_000_000 or gang:
        return
    # ---- the RESERVATION phase at the same size (predicate_manager.go:321-368: no NodeResourcesFit, NodeUnschedulable first): the
    # same proof — one representative per class x all nodes on the oracle under the reservation lists, every member row equal to its
    # class's row — and the counts (this phase was only ever checked on clusters of a few hundred nodes)
    pm.evaluate(allocate=False)
    pod_class, rep = pm.pod_classes()
    assert pm.check_class_rows() == 0
    o.close()
    o = orc.Oracle(pm.dump_snapshot(pods=rep, compact=True))
    want = o.eval_grid(pre_mask=orc.RESERVE_PRE, filt_mask=orc.RESERVE_FILT, threads=os.cpu_count() or 8, prefilter_once=bool(spread))
    got = unpack(pm.read_rows(rep), n_nodes)
    assert np.array_equal(got, want), f"reservation phase: {int((got != want).sum())} of {want.size} representative pairs differ from the oracle"
    assert np.array_equal(pm.read_counts(), want.sum(axis=1)[pod_class])
    assert want.sum() > 0
    o.close()


@pytest.mark.parametrize("weak", [False, True])
def test_bench_two_ranks_on_one_gpu(tmp_path, weak):
    """The N>1 paths of bench.py end to end: 2 ranks share this box's GPU, gloo carries the reference exchanges (RCCL needs
    one GPU per rank; the driver's multi-GPU runs go through the C ABI). Default = configs[3] shape, strong scaling with the
    bitmap all-gather in the step; --weak = round 1's variant."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29577", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--nodes", "4000", "--pods", "50000", "--cpu-seconds", "0", "--profile-steps", "1", "--full"] + (["--weak"] if weak else [])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["pods"] == 50000
    if weak:
        assert d["scaling"] == "weak" and d["config"]["nodes_per_gpu"] == 4000 and d["config"]["total_nodes"] == 8000
    else:
        assert d["scaling"] == "strong" and d["config"]["total_nodes"] == 4000 and d["config"]["gang_size"] == 100
        rows_cap = importlib.import_module("yunikorn-k8shim_amd.sharding").common_row_capacity(50000)
        assert d["config"]["nodes_per_gpu"] == 2048 and d["bitmap_allgather"]["shard_bytes"] == rows_cap * 32 * 8
    assert "reference" in d["config"]["collectives"]


@pytest.mark.parametrize("world,total_nodes", [(2, 200), (2, 5000), (3, 1000)])
def test_sharded_cluster_ranks(world, total_nodes):
    """BASELINE configs[3] in small: `world` processes hold node shards (unequal, one common row stride) and all asks; the
    gathered bitmap [G][P][row_stride] must reassemble to the single-engine rows for EVERY ask, the exchanged counts and
    decisions must equal the single engine's, with hard spread constraints on (cluster-wide histograms). On a box with
    >= world GPUs the exchanges run through the C ABI over RCCL; on one GPU the torch.distributed reference forms run over
    gloo (tests/_shard_worker.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29600 + world * 7 + total_nodes % 89), os.path.join(root, "tests", "_shard_worker.py"),
           str(total_nodes), "700"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("rows True counts True decisions True") == world, out.stdout[-1500:]


@pytest.mark.parametrize("world,total_nodes", [(2, 200), (3, 1000), (2, 5000)])
def test_sharded_cluster_ranks_through_the_c_abi_collectives(tmp_path, world, total_nodes):
    """The SAME check with the exchanges going through the C ABI with world > 1 on this box's one GPU: ykpred_comm_init,
    ykpred_gather_bitmap, ykpred_gather_bitmap_compressed (per-peer header exchange: the shards' class partitions differ),
    ykpred_exchange_decisions and the in-place histogram all-reduces inside ykpred_eval — libykpred loads tests/c/rccl_stub.cpp
    (the collectives' entry points over shared memory between the rank processes) instead of librccl, which refuses two ranks on
    one device. What RCCL itself does over xGMI stays the driver's 8-GPU run; every line of libykpred's side of it runs here."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(root, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29700 + world * 7 + total_nodes % 89), os.path.join(root, "tests", "_shard_worker.py"),
           str(total_nodes), "700"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("rccl-stub: rows True counts True decisions True") == world, out.stdout[-1500:]
    assert out.stdout.count("class-compressed gather True") == world


def test_rccl_communicator_single_rank():
    """The C-ABI communicator with world = 1 on this box's GPU: librccl is loaded on first use, the all-gather of a
    one-shard cluster is the bitmap itself, the decision exchange maps local to global node indices (node_offset)."""
    import torch
    pm = pkg.GpuPredicateManager()
    pm.generate_kwok(seed=99, num_nodes=300, num_pods=400, num_templates=50, node_affinity=1, spread=1)
    uid = pm.comm_unique_id()
    assert len(uid) == 128
    pm.comm_init(uid, 0, 1, 1000)
    dev = torch.device("cuda", 0)
    counts = torch.empty(400, dtype=torch.int32, device=dev)
    decisions = torch.empty(400, dtype=torch.int32, device=dev)
    keys = torch.empty(400, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    pm.evaluate_into(counts=counts, decisions=decisions, keys=keys, stream=stream.cuda_stream)
    pm.synchronize()
    want_rows, local_dec, local_counts = pm.read_bitmap(), decisions.cpu().numpy().copy(), counts.cpu().numpy().copy()
    pm.gather_bitmap(stream=stream.cuda_stream)
    pm.exchange_decisions(stream=stream.cuda_stream)
    pm.synchronize()
    lay = pm.layout()
    assert np.array_equal(pm.read_gathered(0)[:, :lay.row_words], want_rows)
    assert np.array_equal(counts.cpu().numpy(), local_counts)
    assert np.array_equal(decisions.cpu().numpy(), np.where(local_dec >= 0, local_dec + 1000, -1))
    o = orc.Oracle(pm.dump_snapshot())
    assert np.array_equal(unpack(want_rows, 300), o.eval_grid(threads=8))
    # the class-compressed form of the same gather: class rows through the all-gather, slabs expanded by the writer kernels
    gathered = torch.full((1, lay.num_rows, lay.row_stride), -1, dtype=torch.int64, device=dev)  # all ones: every word must be rewritten
    torch.cuda.synchronize()
    pm.gather_bitmap(gathered=gathered, stream=stream.cuda_stream, compressed=True)
    pm.synchronize()
    rows = gathered[0].cpu().numpy().view(np.uint64)[pm.row_map()]
    assert np.array_equal(rows[:, :lay.row_words], want_rows) and not rows[:, lay.row_words:].any()
    pm.gather_bitmap(stream=stream.cuda_stream, compressed=True)  # engine-owned
    pm.synchronize()
    assert np.array_equal(pm.read_gathered(0)[:, :lay.row_words], want_rows)
    pm.comm_destroy()
    pm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,n_pods,templates,gang", [(300, 400, 50, 0), (50_000, 200_000, 400, 0), (6_250, 300_000, 2000, 100)])
def test_class_rows_expand_to_the_bitmap(n_nodes, n_pods, templates, gang):
    """The building blocks of the compressed gather on one engine, with and without the band layout: collect the class rows
    of an evaluation, expand them into a fresh buffer, and every ask's row (through row_of_pod) must be the evaluated one.
    A second engine over OTHER nodes but the same asks expands the first engine's class rows to the first engine's bitmap in
    its own row order — what a shard does with a peer's class rows."""
    import torch
    dev = torch.device("cuda", 0)
    a, b = pkg.GpuPredicateManager(), pkg.GpuPredicateManager()
    try:
        kw = dict(seed=4242, num_pods=n_pods, num_templates=templates, node_affinity=1, gang_size=gang, total_nodes=2 * n_nodes)
        a.generate_kwok(num_nodes=n_nodes, node_index_offset=0, **kw)
        b.generate_kwok(num_nodes=n_nodes, node_index_offset=n_nodes, **kw)
        for m in (a, b):
            m.set_row_capacity(sharding.common_row_capacity(n_pods))
            m.evaluate()
        la, lb = a.layout(), b.layout()
        assert (la.num_rows, la.row_stride) == (lb.num_rows, lb.row_stride)
        want_a, want_b = a.read_bitmap(), b.read_bitmap()
        assert not np.array_equal(want_a, want_b)  # different nodes: different bits
        rows_a = torch.empty((la.num_classes, la.row_stride), dtype=torch.int64, device=dev)
        a.collect_class_rows(rows_a)
        a.synchronize()
        map_a = torch.from_numpy(a.pod_classes()[0].astype(np.int32)).to(dev)
        # own class rows with the writer kernels; own class rows ask by ask; a peer's (the peer may merge signatures differently:
        # its class count and layout digest need not equal this engine's — then only the ask-by-ask form applies)
        cases = [(a, None), (a, map_a), (b, map_a)]
        if a.layout_hash() == b.layout_hash():
            cases.append((b, None))
        for engine, pod_class in cases:
            out = torch.full((la.num_rows, la.row_stride), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()  # the fill runs on torch's stream, the expansion on the engine's
            engine.expand_class_rows(rows_a, out, pod_class=pod_class)
            engine.synchronize()
            got = out.cpu().numpy().view(np.uint64)[engine.row_map()]
            assert np.array_equal(got[:, :la.row_words], want_a) and not got[:, la.row_words:].any()
    finally:
        a.close()
        b.close()


def test_topology_spread_sharded_histograms():
    """Node-sharded PodTopologySpread: two engines hold half of the nodes each; the partial histograms are summed
    (what sharding.exchange_spread_histograms does over RCCL) and both halves of the bitmap must equal the oracle's
    verdicts on the whole cluster."""
    import torch
    full = pkg.GpuPredicateManager()
    a, b = pkg.GpuPredicateManager(), pkg.GpuPredicateManager()
    try:
        full.generate_kwok(seed=777, num_nodes=256, num_pods=400, num_templates=80, node_affinity=1, spread=1)
        snap = json.loads(full.dump_snapshot())
        half = 128
        a.load_snapshot({"nodes": snap["nodes"][:half], "pods": snap["pods"]})
        b.load_snapshot({"nodes": snap["nodes"][half:], "pods": snap["pods"]})
        for m in (a, b):
            m.evaluate_into(spread_count_only=True)
            m.synchronize()
        (ca, pa), (cb, pb) = a.spread_tensors(), b.spread_tensors()
        assert ca.numel() == cb.numel() and ca.numel() > 1, "shards must share the topology-domain dictionaries"
        total, present = ca + cb, torch.maximum(pa, pb)
        for c, p in ((ca, pa), (cb, pb)):
            c.copy_(total)
            p.copy_(present)
        torch.cuda.synchronize()
        for m in (a, b):
            m.evaluate_into(spread_counts_ready=True)
        want = orc.Oracle(snap).eval_grid(threads=8)
        got = np.concatenate([unpack(a.read_bitmap(), half), unpack(b.read_bitmap(), len(snap["nodes"]) - half)], axis=1)
        assert np.array_equal(got, want)
        assert np.array_equal(a.read_counts() + b.read_counts(), want.sum(axis=1))
    finally:
        for m in (full, a, b):
            m.close()


def test_sharded_decisions_match_single_engine():
    """Node-axis sharding: two engines hold half of the nodes each; merging their (count, decision, key) outputs the way
    sharding.exchange_decisions does (SUM / MIN key / MIN global node id) must reproduce the single-engine result."""
    import torch
    full, a, b = pkg.GpuPredicateManager(), pkg.GpuPredicateManager(), pkg.GpuPredicateManager()
    try:
        full.generate_kwok(seed=31337, num_nodes=1024, num_pods=3000, num_templates=150, node_affinity=1)
        snap = json.loads(full.dump_snapshot())
        half = 512
        a.load_snapshot({"nodes": snap["nodes"][:half], "pods": snap["pods"]})
        b.load_snapshot({"nodes": snap["nodes"][half:], "pods": snap["pods"]})
        full.evaluate()
        want_counts, want_dec = full.read_counts(), full.read_decisions()
        outs = []
        for m in (a, b):
            P = m.num_pods
            c = torch.empty(P, dtype=torch.int32, device="cuda")
            d = torch.empty(P, dtype=torch.int32, device="cuda")
            k = torch.empty(P, dtype=torch.int64, device="cuda")
            m.evaluate_into(counts=c, decisions=d, keys=k)
            m.synchronize()
            outs.append((c.cpu().numpy(), d.cpu().numpy(), k.cpu().numpy()))
        (ca, da, ka), (cb, db, kb) = outs
        counts = ca + cb
        best_key = np.minimum(ka, kb)
        big = np.iinfo(np.int32).max
        cand_a = np.where((ka == best_key) & (da >= 0), da, big)
        cand_b = np.where((kb == best_key) & (db >= 0), db + half, big)
        cand = np.minimum(cand_a, cand_b)
        dec = np.where(cand == big, -1, cand)
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(dec, want_dec)
    finally:
        for m in (full, a, b):
            m.close()


@pytest.mark.parametrize("plugins", [["NodeResourcesFit", "NodePorts"], ["*"]])
def test_preemption_predicates_batch(plugins):
    """Random PreemptionPredicates queries (victim prefixes, nil and foreign victims, host ports) in ONE launch, each
    against the oracle's sequential restatement of predicate_manager.go:141-179."""
    import random
    rng = random.Random(9)
    snap = _gen.random_snapshot(4321, n_nodes=120, n_pods=60, scalars=True)
    pm = pkg.GpuPredicateManager.internal(plugins, plugins, plugins, plugins)
    mask = orc.ALL if plugins == ["*"] else orc.mask_of(plugins)
    pm.load_snapshot(snap)
    o = orc.Oracle(snap)
    queries, want = [], []
    for _ in range(300):
        p = rng.randrange(len(snap["pods"]))
        n = rng.randrange(len(snap["nodes"]))
        on_node = []
        for e in snap["nodes"][n].get("pods", []):
            reps = e.get("replicas", 1)
            on_node += [e["metadata"]["uid"] + (f"#{r}" if reps > 1 else "") for r in range(reps)]
        k = rng.randrange(0, len(on_node) + 1)
        idx = rng.sample(range(len(on_node)), k)
        victims = [on_node[i] for i in idx]
        oidx = list(idx)
        if rng.random() < 0.3:
            pos = rng.randrange(len(victims) + 1)
            victims.insert(pos, None)  # nil victim
            oidx.insert(pos, -1)
        start = rng.randrange(0, len(victims) + 1)
        queries.append((p, n, victims, start))
        want.append(o.preemption(p, n, oidx, start, mask, mask))
    got = pm.preemption_predicates_batch(queries)
    pm.close()
    assert got == want
    if plugins != ["*"]:
        assert sum(1 for w in want if w >= 0) >= 10, "degenerate: hardly any query finds a victim index"


# ------------------------------------------------------------------------------------------------------------
# round 3: driver-shaped bench launches, the resident answer behind Predicates(), capacity rules, collective column patches
# ------------------------------------------------------------------------------------------------------------
def _bench(args, env=None, timeout=900):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, env=dict(os.environ, **(env or {})), capture_output=True,
                         text=True, timeout=timeout)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    return out, (json.loads(lines[-1]) if lines else None)


def test_bench_gpus_flag_launches_the_ranks_itself():
    """`python bench.py --gpus 2` exactly as the driver types it (no torchrun in front): the script re-executes itself as 2
    ranks. On this one-GPU box the ranks share cuda:0 and the exchanges take the torch.distributed reference forms (gloo);
    with the default backend the same command must REFUSE rather than measure one GPU and call it two."""
    import torch
    small = ["--steps", "2", "--warmup", "1", "--nodes", "4000", "--pods", "50000", "--cpu-seconds", "0", "--profile-steps", "1", "--full"]
    out, d = _bench(["--gpus", "2"] + small, env={"BENCH_BACKEND": "gloo"})
    assert out.returncode == 0, out.stderr[-2000:]
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["total_nodes"] == 4000 and d["config"]["gang_size"] == 100
    assert "bitmap_allgather" in d and d["value"] > 0
    if torch.cuda.device_count() < 2:
        out, d = _bench(["--gpus", "2"] + small)
        assert out.returncode != 0 and d is None and "needs 2 GPUs" in out.stderr
    out, d = _bench(["--gpus", "1", "--no-variants"] + small)
    assert out.returncode == 0, out.stderr[-2000:]
    assert d["n_gpus"] == 1 and d["scaling"] is None and d["value"] > 0


def test_bench_plain_line_dumps_the_last_step(tmp_path):
    """A plain bench run times exactly --steps steps, runs none of the --full legs, and --dump-outputs writes what the last
    step computed: counts and decisions of every ask and the sampled bitmap rows equal a fresh engine's on the same workload."""
    out, d = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--nodes", "4000", "--pods", "50000", "--dump-outputs", str(tmp_path)])
    assert out.returncode == 0, out.stderr[-2000:]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "evals/s" and d["higher_is_better"] is True and d["dtype"] == "int64"
    assert d["verification"] is None and d["roofline"] is None and d["cpu_baseline"] is None and d["kernel_ms"] == {}
    assert "variants" not in d and "allocation_round" not in d and "predicates_callback" not in d
    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(files) == {"counts", "decisions", "bitmap_rows", "bitmap_row_pods"}
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
    m = pkg.GpuPredicateManager(device=0)
    try:
        m.generate_kwok(seed=0x59554E49 + 2, num_nodes=4000, num_pods=50000, num_templates=2000, node_affinity=1, unique_requests=0, spread=0,
                        gang_size=0, node_index_offset=0, total_nodes=4000)
        m.evaluate()
        m.synchronize()
        assert np.array_equal(files["counts"], m.read_counts()) and np.array_equal(files["decisions"], m.read_decisions())
        pods = files["bitmap_row_pods"].astype(np.int32)
        assert len(pods) > 0
        assert np.array_equal(files["bitmap_rows"], unpack(m.read_rows(pods), 4000).astype(np.float32))
    finally:
        m.close()


@pytest.mark.skipif("__import__('torch').cuda.device_count() < 2")
def test_rccl_world_two_through_the_c_abi():
    """Two GPUs: the node-sharded worker with every exchange through the C ABI over RCCL (communicator, plain and
    class-compressed gather, decision exchange, histogram all-reduce inside ykpred_eval) against a single engine."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29655", os.path.join(root, "tests", "_shard_worker.py"), "5000", "900"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count(" rccl: rows True counts True decisions True") == 2, out.stdout[-1500:]
    _, d = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--nodes", "8000", "--pods", "100000", "--cpu-seconds", "0", "--profile-steps", "1",
                   "--full"])
    assert d["n_gpus"] == 2 and d["config"]["collectives"] == "c-abi rccl"


def test_predicates_are_served_from_the_resident_answer(pm):
    """Context.IsPodFitNode's seam (context.go:696-716): after an evaluation every callback is a lookup in the mirrored
    class rows — equal, pair by pair, to the independent per-pair kernel (k_query) and to the oracle — a column that changes
    (AssumePod) is answered per pair until the next evaluation, and ykhost_candidates walks the ask's row in bin-pack order."""
    pm.generate_kwok(seed=4242, num_nodes=3000, num_pods=20000, num_templates=300, node_affinity=1)
    pm.evaluate()
    base = pm.resident_stats()
    rng = np.random.default_rng(5)
    qp = rng.integers(0, 20000, 4000).astype(np.int32)
    qn = rng.integers(0, 3000, 4000).astype(np.int32)
    fit, code, _ = pm.query(qp, qn)
    names = ["", "NodeUnschedulable", "NodeName", "TaintToleration", "NodeAffinity", "NodePorts", "NodeResourcesFit", "PodTopologySpread",
             "InterPodAffinity"]
    for i in range(len(qp)):
        plugin, err = pm.predicates(int(qp[i]), int(qn[i]), True)
        assert (err is None) == bool(fit[i]), (i, plugin, err)
        if err is not None:
            assert plugin == names[code[i]]
    st = pm.resident_stats()
    assert st["served_resident"] - base["served_resident"] == len(qp) and st["served_query"] == base["served_query"]
    assert st["answer_fetches"] - base["answer_fetches"] == 1, "the class rows are mirrored once per evaluation"
    # oracle on a slice of the same pairs
    pods = np.unique(qp[:40])
    o = orc.Oracle(pm.dump_snapshot(pods=pods))
    want = o.eval_grid(threads=8)
    for i in range(40):
        plugin, err = pm.predicates(int(qp[i]), int(qn[i]), True)
        assert (err is None) == bool(want[int(np.searchsorted(pods, qp[i])), qn[i]])
    # candidates = the decision, then further feasible nodes in bin-pack order
    dec = pm.read_decisions()
    scores = pm.read_scores()
    node_names = np.array([n["metadata"]["name"] for n in json.loads(pm.dump_snapshot(pods=np.zeros(1, dtype=np.int32)))["nodes"]], dtype="S")
    assert len(node_names) == 3000
    order = np.lexsort((node_names, scores))  # ascending score, ties by NodeID
    for p in rng.integers(0, 20000, 50):
        cand = pm.candidates(int(p), 5)
        row, cnt, d1 = pm.peek_row(int(p))
        fits = unpack(row[None, :], 3000)[0]
        assert d1 == dec[p] and cnt == int(fits.sum())
        assert np.array_equal(cand, order[fits[order] > 0][:5])  # the first five feasible nodes of THE order: no tie the wrong way, none skipped
        assert dec[p] == (cand[0] if len(cand) else -1)
    # AssumePod: the node's column is answered per pair (fresh), every other column still from the mirror
    snap = json.loads(pm.dump_snapshot(pods=np.arange(8, dtype=np.int32), nodes=np.arange(4, dtype=np.int32)))
    uid = snap["pods"][0]["metadata"]["uid"]
    node0 = snap["nodes"][0]["metadata"]["name"]
    pm.assume_pod(uid, node0)
    before = pm.resident_stats()
    f1, c1, _ = pm.query(np.arange(1, 200, dtype=np.int32), np.zeros(199, dtype=np.int32))
    for p in range(1, 200):
        plugin, err = pm.predicates(p, 0, True)
        assert (err is None) == bool(f1[p - 1])
    after = pm.resident_stats()
    assert after["served_dirty_column"] - before["served_dirty_column"] == 199
    plugin, err = pm.predicates(5, 7, True)
    assert pm.resident_stats()["served_resident"] == after["served_resident"] + 1
    with pytest.raises(RuntimeError):
        pm.candidates(5, 3)  # a node changed: the bin-pack order of the last evaluation is stale
    pm.evaluate_dirty(decisions=True)
    d5, c5 = int(pm.read_decisions()[5]), pm.candidates(5, 1)  # the ask's CURRENT row (ykpred_peek_row) in the refreshed order
    assert (len(c5) == 0 and d5 < 0) or int(c5[0]) == d5


def test_resident_answer_with_more_classes_than_the_mirror_budget(pm, monkeypatch):
    """Above YKHOST_RESIDENT_MB the host keeps one row per ask (ykpred_peek_row) instead of the class-row table."""
    monkeypatch.setenv("YKHOST_RESIDENT_MB", "0")
    m = pkg.GpuPredicateManager()
    try:
        m.generate_kwok(seed=4243, num_nodes=700, num_pods=900, num_templates=0, node_affinity=1)
        m.evaluate()
        want = unpack(m.read_bitmap(), 700)
        rng = np.random.default_rng(6)
        for p in rng.integers(0, 900, 60):
            for n in rng.integers(0, 700, 5):
                plugin, err = m.predicates(int(p), int(n), True)
                assert (err is None) == bool(want[p, n])
        st = m.resident_stats()
        assert st["served_resident"] == 300 and st["served_query"] == 0 and st["answer_fetches"] <= 61
    finally:
        m.close()


def test_caller_owned_bitmap_states_its_rows():
    """the engine must never write past a buffer it does not own. A caller-owned bitmap without a row count (and
    without ykpred_set_row_capacity) is refused; one that is too small is refused; ask-table patches that outgrow it
    invalidate the evaluation (the next call fails with E_STATE) instead of storing out of bounds."""
    import torch
    m = pkg.GpuPredicateManager()
    try:
        m.generate_kwok(seed=11, num_nodes=500, num_pods=2000, num_templates=40, node_affinity=1)
        m.sync()
        m.evaluate()
        lay = m.layout()
        a = _ffi.YkpredEvalArgs()
        a.prefilter_plugins = a.filter_plugins = 0xFF
        a.options = 7
        small = torch.zeros((lay.num_rows - 1, lay.row_stride), dtype=torch.int64, device="cuda")
        a.bitmap = small.data_ptr()
        assert m._P.ykpred_eval(m.engine, C.byref(a)) == -1 and b"bitmap_rows" in m._P.ykpred_last_error(m.engine)
        a.bitmap_rows = lay.num_rows - 1
        assert m._P.ykpred_eval(m.engine, C.byref(a)) == -1 and b"fewer rows" in m._P.ykpred_last_error(m.engine)
        exact = torch.zeros((lay.num_rows + 3, lay.row_stride), dtype=torch.int64, device="cuda")
        guard = exact[lay.num_rows:]
        guard.fill_(-1)
        a.bitmap, a.bitmap_rows = exact.data_ptr(), lay.num_rows
        assert m._P.ykpred_eval(m.engine, C.byref(a)) == 0
        # two changed asks take two fresh rows: more than the caller's buffer holds -> nothing is patched in place
        rows = np.array([3, 4], dtype=np.int32)
        spec = np.array([1, 2], dtype=np.int32)
        pin = np.array([-1, -1], dtype=np.int32)
        assert m._P.ykpred_update_pods(m.engine, 2000, 2, rows.ctypes.data, spec.ctypes.data, pin.ctypes.data) == 0
        assert m._P.ykpred_eval_pods(m.engine, C.byref(a), 2, rows.ctypes.data) == -4  # E_STATE: run a full evaluation
        m.synchronize()
        assert bool((guard == -1).all()), "rows beyond bitmap_rows were written"
        # the full evaluation re-packs the rows and fits again
        assert m._P.ykpred_eval(m.engine, C.byref(a)) == 0
        m.synchronize()
        assert bool((guard == -1).all())
    finally:
        m.close()


def test_row_capacity_overflow_repacks_instead_of_failing():
    """with a row capacity (node-sharded hosts) the patch that would exceed it no longer fails with the mirrors
    half-updated: the class index is dropped, the tables are replaced, the next evaluation re-packs and answers correctly."""
    m = pkg.GpuPredicateManager()
    try:
        m.generate_kwok(seed=12, num_nodes=300, num_pods=1000, num_templates=30, node_affinity=1)
        m.sync()
        m.evaluate()
        cap = m.layout().num_rows + 5
        m.set_row_capacity(cap)
        m.evaluate()
        snap = json.loads(m.dump_snapshot())
        for i in range(12):  # 12 changed asks > 5 spare rows
            pod = snap["pods"][i]
            pod["spec"]["nodeName"] = ""
            pod["metadata"]["labels"] = dict(pod["metadata"].get("labels", {}), touched=str(i))
            m.update_pod(pod)
        m.evaluate_dirty()
        assert m.layout().num_rows == cap
        o = orc.Oracle(m.dump_snapshot())
        assert np.array_equal(unpack(m.read_bitmap(), 300), o.eval_grid(threads=8))
    finally:
        m.close()


def test_sharded_column_patch_with_topology_constraints():
    """Weak #8 of round 2: incremental + node-sharded + topology constraints. Two engines hold half of the nodes each; a pod
    is assumed on a node of shard A. BOTH shards take the step (ykpred_eval_nodes is collective there): histograms rebuilt
    per shard, summed (here by the test, like the RCCL all-reduce inside the engine), dirty classes rewritten — and both
    halves equal the oracle on the changed cluster without a full pass on either shard."""
    import torch
    full = pkg.GpuPredicateManager()
    a, b = pkg.GpuPredicateManager(), pkg.GpuPredicateManager()
    try:
        full.generate_kwok(seed=778, num_nodes=256, num_pods=500, num_templates=80, node_affinity=1, spread=1)
        snap = json.loads(full.dump_snapshot())
        half = 128
        a.load_snapshot({"nodes": snap["nodes"][:half], "pods": snap["pods"]})
        b.load_snapshot({"nodes": snap["nodes"][half:], "pods": snap["pods"]})

        def exchange():
            (ca, pa), (cb, pb) = a.spread_tensors(), b.spread_tensors()
            total, present = ca + cb, torch.maximum(pa, pb)
            for c, p in ((ca, pa), (cb, pb)):
                c.copy_(total)
                p.copy_(present)
            torch.cuda.synchronize()

        for m in (a, b):
            m.evaluate_into(spread_count_only=True)
            m.synchronize()
        exchange()
        for m in (a, b):
            m.evaluate(allocate=True)  # host-level evaluation so that the mirrors know the phase ...
        # ... (it rebuilt shard-local histograms): put the cluster-wide ones back and run the exact pass
        for m in (a, b):
            m.evaluate_into(spread_count_only=True)
            m.synchronize()
        exchange()
        for m in (a, b):
            m.evaluate_into(spread_counts_ready=True)
            m.synchronize()
        evals = [m.counters()["full_evals"] for m in (a, b)]
        # assume several spread-carrying asks on nodes of shard A
        moved = 0
        for i, pod in enumerate(snap["pods"]):
            if pod["spec"].get("topologySpreadConstraints") and moved < 3:
                node = snap["nodes"][7 + moved]["metadata"]["name"]
                for m in (a, b, full):
                    try:
                        m.assume_pod(pod["metadata"]["uid"], node)
                    except RuntimeError:
                        pass  # shard B does not hold the node: its mirror only learns about it through the histograms
                moved += 1
        assert moved == 3
        for m in (a, b):
            m.evaluate_dirty(spread_count_only=True)
            m.synchronize()
        exchange()
        for m in (a, b):
            m.evaluate_dirty(spread_counts_ready=True)
            m.synchronize()
        assert [m.counters()["full_evals"] for m in (a, b)] == evals, "no shard may fall back to a full pass"
        want = orc.Oracle(full.dump_snapshot()).eval_grid(threads=8)
        live = [i for i, pod in enumerate(json.loads(full.dump_snapshot())["pods"])]
        got = np.concatenate([unpack(a.read_bitmap(), half), unpack(b.read_bitmap(), len(snap["nodes"]) - half)], axis=1)
        # assumed asks keep their rows in the engines but leave the oracle's pending list: compare the rows of the others
        pending_uids = [p["metadata"]["uid"] for p in json.loads(full.dump_snapshot())["pods"]]
        rows = [a.pod_index(u) for u in pending_uids]
        assert np.array_equal(got[rows], want)
    finally:
        for m in (full, a, b):
            m.close()


@pytest.mark.parametrize("seed", range(5))
def test_decisions_of_the_sub_wave_decide_kernel(monkeypatch, seed):
    """k_decide_groups (four classes per wave) is what runs from 16 384 classes on; YKPRED_TUNE decide_groups_from=0 forces it at
    test sizes: every decision of random clusters (NodeName pins, unknown pins, spread constraints, asks without a feasible
    node, node counts around the 16-word group size) against the oracle's decide()."""
    monkeypatch.setenv("YKPRED_TUNE", "decide_groups_from=0")
    snap = _gen.random_snapshot(9300 + seed, n_nodes=[63, 1024, 1025, 2111, 700][seed], n_pods=150, scalars=True, spread=seed % 2 == 1)
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(snap)
        o, want = check_against_oracle(m, snap, True, check_plugins=False)
        dec = m.read_decisions()
        for p in range(len(snap["pods"])):
            assert o.decide(p) == (int(want[p].sum()), int(dec[p])), p
    finally:
        m.close()


@pytest.mark.parametrize("seed", range(3))
def test_match_label_keys_and_all_namespace_selectors_against_the_oracle(pm, seed):
    """Round 3: two fields that used to route an ask away are evaluated. topologySpreadConstraints.matchLabelKeys are folded
    into the selector (podtopologyspread mergeLabelSetWithSelector: for every listed key the pod carries, key = the pod's
    value), and a pod (anti)affinity term with namespaceSelector: {} matches pods of EVERY namespace. Random clusters with
    both sprinkled over asks and running pods, full grid + failing plugins + decisions against the oracle."""
    import random
    rng = random.Random(700 + seed)
    snap = _gen.random_snapshot(9500 + seed, n_nodes=90 + 30 * seed, n_pods=60, spread=True, interpod=True)
    hashes = ["h1", "h2", "h3"]
    for node in snap["nodes"]:
        for pod in node.get("pods", []):
            pod.setdefault("metadata", {}).setdefault("labels", {})["pod-template-hash"] = rng.choice(hashes)
            if rng.random() < 0.3:
                pod["metadata"]["namespace"] = rng.choice(["default", "other", "infra"])
    touched = 0
    for pod in snap["pods"] + [p for n in snap["nodes"] for p in n.get("pods", [])]:
        spec = pod.setdefault("spec", {})
        pod.setdefault("metadata", {}).setdefault("labels", {})["pod-template-hash"] = rng.choice(hashes)
        for c in spec.get("topologySpreadConstraints") or []:
            if c.get("labelSelector") is not None and rng.random() < 0.7:
                c["matchLabelKeys"] = rng.choice([["pod-template-hash"], ["pod-template-hash", "no-such-label"], ["no-such-label"]])
                touched += 1
        aff = spec.get("affinity") or {}
        for kind in ("podAffinity", "podAntiAffinity"):
            for term in (aff.get(kind) or {}).get("requiredDuringSchedulingIgnoredDuringExecution") or []:
                if rng.random() < 0.5:
                    term["namespaceSelector"] = {}
                    touched += 1
    assert touched > 5
    pm.load_snapshot(snap)
    for p in range(len(snap["pods"])):
        assert pm.ask_supported(p)[0], pm.ask_supported(p)
    for allocate in (True, False):
        o, want = check_against_oracle(pm, snap, allocate)
    dec = pm.read_decisions()
    for p in range(0, len(snap["pods"]), 3):
        assert o.decide(p, orc.RESERVE_PRE, orc.RESERVE_FILT) == (int(want[p].sum()), int(dec[p]))


@pytest.mark.parametrize("fail_after", [1, 2, 5, 9, 14, 20, 27, 35, 44, 54, 65, 80, 100, 130])
def test_device_failure_injection_degrades_and_recovers(monkeypatch, fail_after):
    """"if the GPU engine errors it must degrade to the CPU path, never fail scheduling" (the reference's pattern for
    fault injection is a mock function, pkg/client/apifactory_mock.go:137-165). YKPRED_TUNE fail_after=n makes the n-th checked
    device call of a LIVE engine fail (allocation, copy, launch check — wherever n lands: uploads, class build, any stage of the
    evaluation, the incremental patch). The failing entry point reports it, the host marks every device table stale, a callback
    in that state errors (the Go manager counts it RoutedOnError and asks the CPU manager), and the next evaluation re-uploads
    and is bit-exact again."""
    monkeypatch.setenv("YKPRED_TUNE", f"fail_after={fail_after}")
    snap = _gen.random_snapshot(7700 + fail_after, n_nodes=150, n_pods=60, scalars=True, spread=bool(fail_after % 2), interpod=bool(fail_after % 3 == 0))
    m = pkg.GpuPredicateManager()
    try:
        failed = 0
        steps = [lambda: m.load_snapshot(snap), lambda: m.evaluate(),
                 lambda: (m.assume_pod(snap["pods"][0]["metadata"]["uid"], snap["nodes"][1]["metadata"]["name"]), m.evaluate_dirty(decisions=True)),
                 lambda: m.evaluate()]
        for step in steps:
            try:
                step()
            except RuntimeError as e:
                failed += 1
                assert "hip" in str(e).lower() or "ykpred" in str(e).lower(), e
        assert m.device_errors() == failed <= 1
        # whatever failed: the mirror is intact, the next evaluation re-uploads what is stale and agrees with the oracle
        m.evaluate()
        lay = m.layout()
        o = orc.Oracle(m.dump_snapshot())
        want = o.eval_grid(threads=8)
        idx = np.array([m.pod_index(p["metadata"]["uid"]) for p in json.loads(m.dump_snapshot())["pods"]])
        assert np.array_equal(unpack(m.read_bitmap(), lay.num_nodes)[idx], want)
    finally:
        m.close()
