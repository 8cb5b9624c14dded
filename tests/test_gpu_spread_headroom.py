"""ykpred_headroom_spread on the device: headroom of asks with ONE hard topology spread constraint (k_headroom_spread, k_spread_fill),
through the C ABI and the host library — every cell and every per-domain row against the model over Python ints of tests/_spreadgen.py
AND the reference's own clone loop on designed clusters; the statuses under plugin subsets; both accumulation forms at domain counts on
either side of the LDS limit, node counts off the wave width, three task chunks and two table chunks; the invariants against
ykpred_headroom; independence of the evaluation state; AssumePod step by step and a round over the clones; errors; node-sharded engines."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _headgen as hg
import _oracle as orc
import _spreadgen as sg

pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = orc.PLUGIN_BITS
SPREAD, IPA, AFFINITY, FIT = BITS["PodTopologySpread"], BITS["InterPodAffinity"], BITS["NodeAffinity"], BITS["NodeResourcesFit"]
CELLS, ROW = 16, 4
INVALID, UNSUPPORTED = -1, -5
CASES = {c["name"]: c for c in sg.designed_cases()}


@pytest.fixture(scope="module")
def pm():
    m = pkg.GpuPredicateManager()
    yield m
    m.close()


def expected(m, c, ask=None):
    rows, cells = sg.model(c, ask)
    cells = list(cells)
    cells[12] = m.encoded_tables()["topology_keys"].index(c["key"])
    return rows, cells


@pytest.mark.parametrize("name", sorted(CASES))
def test_designed_cases_every_cell_and_row_against_the_model_and_the_clone_loop(pm, name):
    c = CASES[name]
    pm.load_snapshot(c["snapshot"])
    rows, cells = expected(pm, c)
    got = pm.headroom_spread([0])
    print(name, got[0].tolist())
    assert got.shape == (1, CELLS) and got.dtype == np.int64 and got[0].tolist() == cells
    got_cells, got_rows, values = pm.headroom_spread_domains(0)
    assert got_cells.tolist() == cells and got_rows.tolist() == rows and values == sg.domain_values(c)
    # where the constraint's row lies in the engine's histograms: its cells hold the cnt column
    where = pm.headroom_spread_constraint(0)
    assert where.tolist() == [0, cells[12], where[2], len(rows), c["max_skew"], where[5], c["self_match"], where[7]]
    assert where[5] == (c["min_domains"] if c["min_domains"] > 1 else where[5])
    counts, present = pm.spread_tensors()
    assert counts[int(where[2]):int(where[2]) + len(rows)].cpu().tolist() == [r[0] for r in rows]
    assert int(present[int(where[2]):int(where[2]) + len(rows)].cpu().sum()) == cells[5]
    # the engine itself, explicit lists
    assert pm.headroom_spread([0], pre_mask=orc.ALL, filt_mask=orc.ALL)[0].tolist() == cells
    direct = pm.headroom_spread_domains(0, pre_mask=orc.ALL, filt_mask=orc.ALL)
    assert direct[0].tolist() == cells and direct[1].tolist() == rows
    # the reference's own loop over clones, bincounted by domain
    placed, unplaced = sg.clone_loop(c)
    assert unplaced == 3 and np.array_equal(got_rows[:, 3], placed) and got[0, 0] == placed.sum()
    # the invariants, and ykpred_headroom without the topology plugins in the Filter list
    assert got[0, 8] + got[0, 9] + got[0, 10] == (got_rows[:, 1] >= 1).sum() and got[0, 0] <= got[0, 4]
    plain = pm.headroom([0], pre_mask=orc.ALL & ~IPA, filt_mask=orc.ALL & ~SPREAD & ~IPA)[0]
    assert plain[3] == 0 and got[0, 4] <= plain[0] and got[0, 14] <= plain[1]
    if all(v is not None for v in c["labels"]):
        assert got[0, 4] == plain[0] and got[0, 14] == plain[1]
    else:
        assert got[0, 4] < plain[0]
    assert pm.headroom([0])[0, 3] == 2  # (ykpred_headroom keeps calling the ask coupled)


def test_statuses_under_plugin_subsets_and_the_host_calls(pm):
    snap, index = sg.status_cluster()
    pm.load_snapshot(snap)
    P = pm.num_pods
    coupled, routed, plain = [-1, 0, -1, 2] + [0] * 12, [0, 0, 0, 1] + [0] * 12, [0, 0, 0, 3] + [0] * 12
    for way in ("host", "engine"):
        kw = {} if way == "host" else dict(pre_mask=orc.ALL, filt_mask=orc.ALL)
        got = pm.headroom_spread(**kw)
        assert got.shape == (P, CELLS)
        assert got[index["s-one"], 3] == 0 and got[index["s-one"], 0] == 4 and got[index["s-selector"], 3] == 0
        assert got[index["s-two"]].tolist() == coupled and got[index["s-anti"]].tolist() == coupled
        assert got[index["s-routed"]].tolist() == routed and got[index["s-plain"]].tolist() == plain
    # without NodeAffinity in the lists the nodes outside the selector's zone take copies and do not count: still coupled
    no_aff = pm.headroom_spread(pre_mask=orc.ALL & ~AFFINITY, filt_mask=orc.ALL & ~AFFINITY)
    assert no_aff[index["s-selector"]].tolist() == coupled and no_aff[index["s-one"], 3] == 0
    assert no_aff[index["s-one"]].tolist() == pm.headroom_spread([index["s-one"]])[0].tolist()
    # InterPodAffinity absent from the PreFilter list: its terms are not live, the spread constraint is the only one
    no_ipa = pm.headroom_spread(pre_mask=orc.ALL & ~IPA, filt_mask=orc.ALL)
    assert no_ipa[index["s-anti"], 3] == 0 and no_ipa[index["s-two"]].tolist() == coupled
    both = pm.headroom_spread(pre_mask=orc.ALL & ~IPA, filt_mask=orc.ALL & ~IPA)
    assert both[index["s-anti"]].tolist() == pm.headroom_spread([index["s-one"]])[0].tolist()
    # PodTopologySpread without its PreFilter: every Filter call is an error, nothing qualifies
    assert pm.headroom_spread(pre_mask=orc.ALL & ~SPREAD, filt_mask=orc.ALL)[index["s-one"]].tolist() == coupled
    # the verdicts from the tables alone, without a launch
    for uid, status in (("s-one", 0), ("s-selector", 0), ("s-two", 2), ("s-anti", 2), ("s-routed", 1), ("s-plain", 3)):
        where = pm.headroom_spread_constraint(index[uid])
        assert where[0] == status and (status == 0 or not where[1:].any()), uid
    assert pm.headroom_spread_constraint(index["s-one"])[3:7].tolist() == [3, 2, pm.headroom_spread_constraint(index["s-one"])[5], 1]
    with pytest.raises(RuntimeError):
        pm.headroom_spread_constraint(index["s-one"], pre_mask=orc.ALL, filt_mask=orc.ALL & ~SPREAD)
    # rows only for status 0
    for uid in ("s-two", "s-routed", "s-plain"):
        cells, rows, values = pm.headroom_spread_domains(index[uid])
        assert rows.shape == (0, ROW) and values == [] and cells[3] != 0
        count = ctypes.c_int32(-7)
        out = np.zeros((8, ROW), dtype=np.int64)
        assert pm._P.ykpred_headroom_spread_pod(pm.engine, index[uid], orc.ALL, orc.ALL, 8, out.ctypes.data, ctypes.byref(count)) == UNSUPPORTED
    # one crossing by allocation key
    call = pm._L.ykhost_headroom_spread_by_key
    out, best = np.zeros(CELLS, dtype=np.int64), ctypes.create_string_buffer(64)
    assert call(pm._h, b"s-one", out.ctypes.data, best, 64) == 0
    assert out.tolist() == pm.headroom_spread([index["s-one"]])[0].tolist() and out[11] == 0 and best.value == b"z0"
    assert call(pm._h, b"s-two", out.ctypes.data, best, 64) == 0 and out.tolist() == coupled and best.value == b""
    assert call(pm._h, b"s-routed", out.ctypes.data, best, 64) == -13 and out.tolist() == routed
    assert call(pm._h, b"no-such-pod", out.ctypes.data, best, 64) == -10
    assert call(pm._h, b"res-3", out.ctypes.data, best, 64) == -12


def _width_cases(n_nodes):
    tasks = 69
    limit = pkg.GROUP_LDS_MAX_GROUPS
    return [sg.case("w-zone", n_nodes, extra_asks=tasks, tolerate=True, seeded=lambda i: 1 if i % 40 == 3 else 0),
            sg.case("w-63", n_nodes, key="m", label=lambda i: f"m{i % limit:03d}", extra_asks=tasks, tolerate=True, max_skew=2,
                    seeded=lambda i: 1 if i % 9 == 0 else 0),
            sg.case("w-64", n_nodes, key="m", label=lambda i: None if i % 50 == 1 else f"m{i % (limit + 1):03d}", extra_asks=tasks, tolerate=True),
            sg.case("w-host", n_nodes, key=sg.HOST, extra_asks=tasks, tolerate=True, max_skew=2, min_domains=n_nodes if n_nodes == 264 else None)]


_WIDTH_MODELS = {}


@pytest.mark.parametrize("n_nodes", [200, 264, 330])
def test_kernel_widths_both_accumulation_forms_task_and_table_chunks(monkeypatch, n_nodes):
    """Node counts off the wave width; 70 distinct tasks in table chunks of 66 + 4 (group_chunk_tasks), so the first launch walks three
    task chunks; 3, 63, 64 and N domains — the LDS form's limit from both sides — each with the adds forced into the global table
    (group_lds=0) and in LDS wherever the chunk fits: both equal the model. Then asks of two keys in one call: a ragged table."""
    cases = _width_cases(n_nodes)
    assert len(cases[0]["snapshot"]["pods"]) == 70
    answers = []
    for lds in (0, 1):
        monkeypatch.setenv("YKPRED_TUNE", f"group_lds={lds},group_chunk_tasks=66")
        m = pkg.GpuPredicateManager()
        try:
            for c in cases:
                m.load_snapshot(c["snapshot"])
                key = (n_nodes, c["name"])
                if key not in _WIDTH_MODELS:
                    _WIDTH_MODELS[key] = [expected(m, c, j) for j in range(70)]
                got = m.headroom_spread()
                assert len(sg.domain_values(c)) == {"w-zone": 3, "w-63": 63, "w-64": 64, "w-host": n_nodes}[c["name"]]
                for j, (rows, cells) in enumerate(_WIDTH_MODELS[key]):
                    assert got[j].tolist() == cells, (lds, c["name"], j, got[j].tolist(), cells)
                for j in (0, 31, 32, 65, 66, 69):
                    assert m.headroom_spread_domains(j, pre_mask=orc.ALL, filt_mask=orc.ALL)[1].tolist() == _WIDTH_MODELS[key][j][0], (lds, c["name"], j)
                answers.append(got)
            # two keys in one call: the zone asks and the hostname asks over the same nodes
            zone, host = cases[0], cases[3]
            if not any(zone["matching"]):
                pytest.fail("the zone case lost its seeds")
            mixed = {"nodes": zone["snapshot"]["nodes"], "pods": zone["snapshot"]["pods"] + host["snapshot"]["pods"][:6]}
            m.load_snapshot(mixed)
            got = m.headroom_spread()
            host_seeded = dict(host, matching=zone["matching"])
            for j in range(70):
                assert got[j].tolist() == _WIDTH_MODELS[(n_nodes, "w-zone")][j][1]
            for j in range(6):
                rows, cells = expected(m, host_seeded, j)
                assert got[70 + j].tolist() == cells
                assert m.headroom_spread_domains(70 + j, pre_mask=orc.ALL, filt_mask=orc.ALL)[1].tolist() == rows
        finally:
            m.close()
    for a, b in zip(answers[:4], answers[4:]):
        assert np.array_equal(a, b)


def test_a_scratch_budget_below_one_task_gives_one_task_per_table_chunk(monkeypatch):
    c = sg.case("budget", 130, key=sg.HOST, extra_asks=8, tolerate=True)
    monkeypatch.setenv("YKPRED_TUNE", "group_scratch_mb=0")
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(c["snapshot"])
        got = m.headroom_spread()
        for j in range(9):
            assert got[j].tolist() == expected(m, c, j)[1]
    finally:
        m.close()


def test_list_semantics_errors_and_one_query(pm):
    c = CASES["q7"]
    snap = {"nodes": c["snapshot"]["nodes"], "pods": c["snapshot"]["pods"] + sg.status_cluster()[0]["pods"]}
    pm.load_snapshot(snap)
    P = pm.num_pods
    pm.sync()
    q0 = pm.counters()["queries"]
    full = pm.headroom_spread()
    assert pm.counters()["queries"] == q0 + 1  # one query, however many asks
    assert sorted(set(full[:, 3].tolist())) == [0, 1, 2, 3]
    pick = np.random.default_rng(3).integers(0, P, size=4 * P)
    assert np.array_equal(pm.headroom_spread(pick), full[pick])
    assert np.array_equal(pm.headroom_spread(pick, pre_mask=orc.ALL, filt_mask=orc.ALL), full[pick])
    uids = [snap["pods"][i]["metadata"]["uid"] for i in pick[:5]]
    assert np.array_equal(pm.headroom_spread(uids), full[pick[:5]])
    assert pm.headroom_spread([]).shape == (0, CELLS)
    call = pm._P.ykpred_headroom_spread
    out, asks = np.zeros((2, CELLS), dtype=np.int64), np.array([0, 1], dtype=np.int32)

    def run(n=2, a=asks, pre=orc.ALL, filt=orc.ALL, o=out):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return call(pm.engine, n, ptr(a), pre, filt, ptr(o))
    assert run(n=0, a=None, o=None) == 0 and run() == 0 and np.array_equal(out, full[:2])
    assert run(a=None) == INVALID and run(o=None) == INVALID and run(n=-1) == INVALID
    assert run(a=np.array([0, P], dtype=np.int32)) == INVALID and run(a=np.array([-1, 0], dtype=np.int32)) == INVALID
    assert run(filt=orc.ALL & ~SPREAD) == INVALID  # ykpred_headroom answers without the plugin
    assert run(pre=orc.ALL & ~FIT) == INVALID and run(filt=orc.ALL & ~FIT) == INVALID
    assert run() == 0 and np.array_equal(out, full[:2])
    # the rows of one ask: the size comes back when the caller's table is too small
    pod = pm._P.ykpred_headroom_spread_pod
    count, rows = ctypes.c_int32(-7), np.zeros((7, ROW), dtype=np.int64)
    assert pod(pm.engine, 0, orc.ALL, orc.ALL, 6, rows.ctypes.data, ctypes.byref(count)) == INVALID and count.value == 7 and not rows.any()
    assert pod(pm.engine, 0, orc.ALL, orc.ALL, 7, rows.ctypes.data, ctypes.byref(count)) == 0 and rows.tolist() == sg.model(c)[0]
    assert pod(pm.engine, 0, orc.ALL, orc.ALL & ~SPREAD, 7, rows.ctypes.data, ctypes.byref(count)) == INVALID
    assert pod(pm.engine, P, orc.ALL, orc.ALL, 7, rows.ctypes.data, ctypes.byref(count)) == INVALID
    assert pod(pm.engine, 0, orc.ALL, orc.ALL, 7, rows.ctypes.data, None) == INVALID
    with pytest.raises(RuntimeError):
        pm.headroom_spread([P])
    # no nodes at all: the verdicts alone
    pm.load_snapshot({"nodes": [], "pods": snap["pods"]})
    empty = pm.headroom_spread()
    assert pm.num_nodes == 0 and np.array_equal(empty[:, 3], full[:, 3])
    assert empty[0].tolist() == [0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 0, -1, empty[0, 12], c["max_skew"], 0, 0]
    assert np.array_equal(pm.headroom_spread(pre_mask=orc.ALL, filt_mask=orc.ALL), empty)  # the engine itself: a routed ask is 1 here too


def test_needs_no_evaluation_disturbs_none_and_follows_assume_pod():
    """Before any evaluation; ykpred_answer_state and the bitmap checksum unchanged by the call; then 12 steps of AssumePod of one copy on
    the node a round picks for it: [0] falls by exactly 1 each time, with no evaluation between the assume and the call."""
    c = CASES["tol-32"]
    snap = hg.clones(c["snapshot"], 0, 14)
    uid = lambda k: f"s-tol-32-copy-{k}"  # noqa: E731
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(snap)
        rows, cells = expected(m, c)
        assert m.counters()["full_evals"] == 0
        assert m.headroom_spread([13])[0].tolist() == cells  # before any evaluation
        assert m.counters()["full_evals"] == 0
        m.evaluate()

        def state():
            classes = ctypes.c_int32(-1)
            assert m._P.ykpred_answer_state(m.engine, orc.ALL, orc.ALL, ctypes.byref(classes)) == 0
            return (m.checksum(), classes.value, m.read_counts().tolist(), m.read_decisions().tolist(),
                    {k: v for k, v in m.counters().items() if k != "queries"})
        before = state()
        assert m.headroom_spread()[5].tolist() == cells and m.headroom_spread_domains(3)[1].tolist() == rows
        assert state() == before
        total = cells[0]
        for step in range(12):
            ask = m.pod_index(uid(step))
            node = int(m.allocate_round(asks=np.array([ask], dtype=np.int32), apply=False)[0])
            assert node >= 0
            m.assume_pod(uid(step), snap["nodes"][node]["metadata"]["name"])
            evals = m.counters()["full_evals"]
            got = m.headroom_spread([m.pod_index(uid(13))])[0]
            assert m.counters()["full_evals"] == evals
            assert got[3] == 0 and got[0] == total - 1, (step, got.tolist())
            total -= 1
    finally:
        m.close()


@pytest.mark.parametrize("name", ["skew1", "tol-30", "q7-min9", "seed-z0"])
def test_a_round_over_the_clones_places_exactly_the_answer(pm, name):
    c = CASES[name]
    total = sg.model(c)[1][0]
    pm.load_snapshot(hg.clones(c["snapshot"], 0, total + 2))
    assert pm.headroom_spread([0])[0, 0] == total
    placed = pm.allocate_round()
    assert int((placed >= 0).sum()) == total and int((placed == -1).sum()) == 2
    dom = np.array(sg.domain_of_nodes(c))
    assert np.bincount(dom[placed[placed >= 0]], minlength=len(sg.domain_values(c))).tolist() == [r[3] for r in sg.model(c)[0]]


def test_node_sharded_engines_return_cluster_wide_rows(tmp_path):
    """World 2 on one GPU, the collectives through tests/c/rccl_stub.cpp (tests/_shard_spread_headroom_worker.py): both ranks equal a
    single engine over all nodes and the model; the domain that pins an ask's floor lies wholly on the other shard."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29671", os.path.join(ROOT, "tests", "_shard_spread_headroom_worker.py")]
    env = {k: v for k, v in os.environ.items() if k != "YKPRED_TUNE"}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, SHARD_RCCL_STUB=stub))
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("spread-headroom True model True rows True pinned-elsewhere True no-self-match True mismatch True") == 2, (out.stdout[-1500:], out.stderr[-1500:])
