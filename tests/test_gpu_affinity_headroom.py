"""ykpred_headroom_affinity on the device: headroom of asks with required pod (anti-)affinity (k_headroom_affinity, k_affinity_fill),
through the C ABI and the host library — every cell and every per-domain row, the outside row included, against the model over Python
ints of tests/_affgen.py AND the reference's own clone loop on designed clusters; the statuses under plugin subsets; both accumulation
forms and both fill forms at domain counts on either side of the LDS limit, node counts off the wave width, three task chunks and two
table chunks; independence of the evaluation state; AssumePod and a round over the clones; errors; host calls; node-sharded engines."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _affgen as ag
import _headgen as hg
import _oracle as orc
import _spreadgen as sg

pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = orc.PLUGIN_BITS
SPREAD, IPA, FIT = BITS["PodTopologySpread"], BITS["InterPodAffinity"], BITS["NodeResourcesFit"]
CELLS, ROW = 16, 4
INVALID, UNSUPPORTED = -1, -5
CASES = {c["name"]: c for c in ag.designed_cases()}
COUPLED, ROUTED, PLAIN = [-1, 0, -1, 2] + [0] * 12, [0, 0, 0, 1] + [0] * 12, [0, 0, 0, 3] + [0] * 12


@pytest.fixture(scope="module")
def pm():
    m = pkg.GpuPredicateManager()
    yield m
    m.close()


def expected(m, c, ask=None):
    status, key, mode, rows, cells = ag.model(c, ask)
    cells = list(cells)
    if status in (0, 4):
        cells[12] = m.encoded_tables()["topology_keys"].index(key)
    return rows, cells


@pytest.mark.parametrize("name", sorted(CASES))
def test_designed_cases_every_cell_and_row_against_the_model_and_the_clone_loop(pm, name):
    c = CASES[name]
    pm.load_snapshot(c["snapshot"])
    rows, cells = expected(pm, c)
    got = pm.headroom_affinity([0])
    print(name, got[0].tolist())
    assert got.shape == (1, CELLS) and got.dtype == np.int64 and got[0].tolist() == cells
    got_cells, got_rows, values = pm.headroom_affinity_domains(0)
    assert got_cells.tolist() == cells and got_rows.tolist() == rows
    # the engine itself, explicit lists
    assert pm.headroom_affinity([0], pre_mask=orc.ALL, filt_mask=orc.ALL)[0].tolist() == cells
    direct = pm.headroom_affinity_domains(0, pre_mask=orc.ALL, filt_mask=orc.ALL)
    assert direct[0].tolist() == cells and direct[1].tolist() == rows
    assert pm.headroom([0])[0, 3] == 2  # (ykpred_headroom keeps calling the ask coupled)
    where = pm.headroom_affinity_constraint(0)
    if cells[3] == 2:
        assert values == [] and got_rows.shape == (0, ROW) and where.tolist() == [2] + [0] * 15
        return
    assert values == ag.domain_values(c) and len(got_rows) == len(values) + 1
    # where the anti rows on the key lie in the engine's histograms: their cells sum to the cnt column (bootstrap is not seen there)
    D = len(values)
    assert where[:4].tolist() == [0, cells[12], 0 if cells[3] == 4 else cells[13], D] and 0 <= where[4] <= 11
    counts = pm.spread_tensors()[0].cpu().numpy()
    cnt = np.zeros(D, dtype=np.int64)
    for off in where[5:5 + where[4]]:
        cnt += counts[off:off + D]
    assert cnt.tolist() == [r[0] for r in rows[:-1]] and (where[4] > 0 or not c["anti"])
    if cells[3] == 4:  # bootstrap: the loop ends with the capacity of the domain its first copy picked
        placed, unplaced, first = ag.clone_loop(c, count=cells[4] + 3)
        d1 = ag.domain_of_nodes(c, ag.model(c)[1])[first]
        assert placed.sum() == placed[d1] == got_rows[d1, 1] and got[0, 2] == got_rows[:-1, 1].max() == got_rows[got[0, 11], 1]
        return
    # the reference's own loop over clones, bincounted by domain with the outside row last
    placed, unplaced, _ = ag.clone_loop(c)
    assert unplaced == 3 and np.array_equal(got_rows[:, 3], placed) and got[0, 0] == placed.sum()
    # the invariants, and ykpred_headroom without the plugin: the static verdict can only take nodes away
    assert got[0, 8] + got[0, 9] == (got_rows[:-1, 1] >= 1).sum() and got[0, 0] <= got[0, 4] + got[0, 6]
    if got[0, 13] == 1:
        assert got[0, 0] == got[0, 1] + got[0, 6] and not got_rows[got_rows[:, 0] > 0, 1].any()
    plain = pm.headroom([0], pre_mask=orc.ALL & ~IPA, filt_mask=orc.ALL & ~IPA & ~SPREAD)[0]
    assert plain[3] == 0 and got[0, 4] + got[0, 6] <= plain[0] and got[0, 14] <= plain[1]
    if not got[0, 5] and not c["aff"]:
        assert got[0, 4] + got[0, 6] == plain[0] and got[0, 14] == plain[1]


def test_statuses_under_plugin_subsets_and_the_host_calls(pm):
    snap, index = sg.status_cluster()
    pm.load_snapshot(snap)
    P = pm.num_pods
    host_key = pm.encoded_tables()["topology_keys"].index(sg.HOST)
    for way in ("host", "engine"):
        kw = {} if way == "host" else dict(pre_mask=orc.ALL, filt_mask=orc.ALL)
        got = pm.headroom_affinity(**kw)
        assert got.shape == (P, CELLS)
        # a live spread constraint, alone or beside the anti-affinity term: still coupled here (ykpred_headroom_spread answers the first)
        for uid in ("s-one", "s-selector", "s-two", "s-anti"):
            assert got[index[uid]].tolist() == COUPLED, uid
        assert got[index["s-routed"]].tolist() == ROUTED and got[index["s-plain"]].tolist() == PLAIN
    # without PodTopologySpread in the Filter list the spread constraint is not live: s-anti is one executor per host, the others plain
    no_spread = pm.headroom_affinity(pre_mask=orc.ALL, filt_mask=orc.ALL & ~SPREAD)
    anti = no_spread[index["s-anti"]]
    fits = pm.headroom([index["s-anti"]], pre_mask=orc.ALL & ~IPA, filt_mask=orc.ALL & ~SPREAD & ~IPA)[0]
    assert anti[3] == 0 and anti[13] == 1 and anti[12] == host_key and anti[0] == anti[1] == anti[14] == fits[1] > 0 and anti[6] == 0
    assert no_spread[index["s-one"]].tolist() == PLAIN and no_spread[index["s-two"]].tolist() == PLAIN
    assert no_spread[index["s-routed"]].tolist() == ROUTED and no_spread[index["s-plain"]].tolist() == PLAIN
    # InterPodAffinity must be in both lists, NodeResourcesFit too
    call = pm._P.ykpred_headroom_affinity
    out, asks = np.zeros((2, CELLS), dtype=np.int64), np.array([0, index["s-anti"]], dtype=np.int32)
    for pre, filt in ((orc.ALL & ~IPA, orc.ALL), (orc.ALL, orc.ALL & ~IPA), (orc.ALL & ~FIT, orc.ALL), (orc.ALL, orc.ALL & ~FIT)):
        assert call(pm.engine, 2, asks.ctypes.data, pre, filt, out.ctypes.data) == INVALID
    # rows only for status 0 and 4
    for uid in ("s-two", "s-routed", "s-plain"):
        got_cells, got_rows, values = pm.headroom_affinity_domains(index[uid])
        assert got_rows.shape == (0, ROW) and values == [] and got_cells[3] not in (0, 4)
        count = ctypes.c_int32(-7)
        out8 = np.zeros((9, ROW), dtype=np.int64)
        assert pm._P.ykpred_headroom_affinity_pod(pm.engine, index[uid], orc.ALL, orc.ALL, 8, out8.ctypes.data, ctypes.byref(count)) == UNSUPPORTED
    by_key = pm._L.ykhost_headroom_affinity_by_key
    out16, best = np.zeros(CELLS, dtype=np.int64), ctypes.create_string_buffer(64)
    assert by_key(pm._h, b"s-two", out16.ctypes.data, best, 64) == 0 and out16.tolist() == COUPLED and best.value == b""
    assert by_key(pm._h, b"s-routed", out16.ctypes.data, best, 64) == -13 and out16.tolist() == ROUTED
    assert by_key(pm._h, b"no-such-pod", out16.ctypes.data, best, 64) == -10
    assert by_key(pm._h, b"res-3", out16.ctypes.data, best, 64) == -12
    # the host calls at status 0: rows with the label values, and one crossing by allocation key
    host = CASES["host-self-1500"]
    pm.load_snapshot(host["snapshot"])
    rows, cells = expected(pm, host)
    got_cells, got_rows, values = pm.headroom_affinity_domains("a-host-self-1500")
    assert got_cells.tolist() == cells and got_rows.tolist() == rows and values == ag.domain_values(host) and "hn0000" not in values
    assert by_key(pm._h, b"a-host-self-1500", out16.ctypes.data, best, 64) == 0
    assert out16.tolist() == cells and best.value.decode() == values[cells[11]]


def _width_cases(n_nodes):
    tasks = 69
    limit = pkg.GROUP_LDS_MAX_GROUPS
    return [ag.case("w-zone", n_nodes, extra_asks=tasks, anti=[ag.SELF_ZONE]),
            ag.case("w-63", n_nodes, extra_asks=tasks, anti=[ag.term("m", app="ask")], label=("m", lambda i: None if i % 50 == 1 else f"m{i % limit:03d}"),
                    residents=lambda i: [ag.BLOCKER] if i % 70 == 6 else []),
            ag.case("w-64", n_nodes, extra_asks=tasks, anti=[ag.term("m", role="blk")], label=("m", lambda i: None if i % 50 == 1 else f"m{i % (limit + 1):03d}"),
                    residents=lambda i: [ag.OTHER] if i % 70 == 6 else []),
            ag.case("w-host", n_nodes, extra_asks=tasks, anti=[ag.SELF_HOST], unlabel=lambda i: i % 17 == 0,
                    residents=lambda i: [ag.BLOCKER] if i in (62, 63, 64, 65, 255, 256, 329) else [])]


_WIDTH_MODELS = {}


@pytest.mark.parametrize("n_nodes", [200, 264, 330])
def test_kernel_widths_both_accumulation_forms_both_fills_task_and_table_chunks(monkeypatch, n_nodes):
    """Node counts off the wave width; 70 distinct tasks in table chunks of 66 + 4 (group_chunk_tasks), so the first launch walks three
    task chunks; 3, 63, 64 and about N domains — the LDS form's limit from both sides, the outside row in LDS row 63 and behind the
    domains of the global table — with the adds forced into the global table and the workgroup fill, in LDS wherever the chunk fits
    with the one-wave fill, and as the engine chooses by itself: all equal the model. Then asks of two keys in one call."""
    cases = _width_cases(n_nodes)
    assert len(cases[0]["snapshot"]["pods"]) == 70
    answers = {}
    for tune in ("group_lds=0,affinity_fill_waves=4,", "group_lds=1,affinity_fill_waves=1,", ""):
        monkeypatch.setenv("YKPRED_TUNE", tune + "group_chunk_tasks=66")
        m = pkg.GpuPredicateManager()
        try:
            for c in cases:
                m.load_snapshot(c["snapshot"])
                key = (n_nodes, c["name"])
                if key not in _WIDTH_MODELS:
                    _WIDTH_MODELS[key] = [expected(m, c, j) for j in range(70)]
                    assert len(_WIDTH_MODELS[key][0][0]) - 1 == {"w-zone": 3, "w-63": 63, "w-64": 64}.get(c["name"], n_nodes - (n_nodes + 16) // 17)
                    assert _WIDTH_MODELS[key][0][1][6] > 0 or c["name"] == "w-zone"  # copies outside
                got = m.headroom_affinity()
                for j, (rows, cells) in enumerate(_WIDTH_MODELS[key]):
                    assert got[j].tolist() == cells, (tune, c["name"], j, got[j].tolist(), cells)
                for j in (0, 31, 32, 65, 66, 69):
                    assert m.headroom_affinity_domains(j, pre_mask=orc.ALL, filt_mask=orc.ALL)[1].tolist() == _WIDTH_MODELS[key][j][0], (tune, c["name"], j)
                answers.setdefault(c["name"], []).append(got)
            # two keys in one call: the zone asks and the hostname asks over the same nodes (those of the hostname case)
            zone, host = cases[0], cases[3]
            mixed = {"nodes": host["snapshot"]["nodes"], "pods": host["snapshot"]["pods"] + zone["snapshot"]["pods"][:6]}
            m.load_snapshot(mixed)
            got = m.headroom_affinity()
            zone_here = dict(zone, labels=host["labels"], pods_on=host["pods_on"])
            zone_here.pop("_verdict", None)
            for j in range(70):
                assert got[j].tolist() == _WIDTH_MODELS[(n_nodes, "w-host")][j][1]
            for j in range(6):
                rows, cells = expected(m, zone_here, j)
                assert got[70 + j].tolist() == cells
                assert m.headroom_affinity_domains(70 + j, pre_mask=orc.ALL, filt_mask=orc.ALL)[1].tolist() == rows
        finally:
            m.close()
    for name, (a, b, c) in answers.items():
        assert np.array_equal(a, b) and np.array_equal(a, c), name


def test_a_scratch_budget_below_one_task_gives_one_task_per_table_chunk(monkeypatch):
    c = ag.case("budget", 130, extra_asks=8, anti=[ag.SELF_HOST], residents=lambda i: [ag.BLOCKER] if i % 11 == 3 else [])
    monkeypatch.setenv("YKPRED_TUNE", "group_scratch_mb=0")
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(c["snapshot"])
        got = m.headroom_affinity()
        for j in range(9):
            assert got[j].tolist() == expected(m, c, j)[1]
    finally:
        m.close()


def test_list_semantics_errors_and_one_query(pm):
    # (a term that matches the ask's own role alone: the asks of the status cluster gain no existing-anti-affinity constraint from it)
    c = ag.case("list", req=hg.MAIN_REQ, anti=[ag.term(ag.HOST, role="exec")], ask_labels={"role": "exec"}, unlabel=lambda i: i % 17 == 0,
                residents=lambda i: [({"role": "exec"}, [])] if i % 9 == 2 else [])
    assert ag.model(c)[4][:2] == [166, 120]
    snap = {"nodes": c["snapshot"]["nodes"], "pods": c["snapshot"]["pods"] + sg.status_cluster()[0]["pods"]}
    pm.load_snapshot(snap)
    P = pm.num_pods
    full = pm.headroom_affinity()  # (syncs and uploads the spec effects)
    q0 = pm.counters()["queries"]
    assert np.array_equal(pm.headroom_affinity(), full)
    assert pm.counters()["queries"] == q0 + 1  # one query, however many asks
    assert sorted(set(full[:, 3].tolist())) == [0, 1, 2, 3]
    pick = np.random.default_rng(3).integers(0, P, size=4 * P)
    assert np.array_equal(pm.headroom_affinity(pick), full[pick])
    assert np.array_equal(pm.headroom_affinity(pick, pre_mask=orc.ALL, filt_mask=orc.ALL), full[pick])
    uids = [snap["pods"][i]["metadata"]["uid"] for i in pick[:5]]
    assert np.array_equal(pm.headroom_affinity(uids), full[pick[:5]])
    assert pm.headroom_affinity([]).shape == (0, CELLS)
    call = pm._P.ykpred_headroom_affinity
    out, asks = np.zeros((2, CELLS), dtype=np.int64), np.array([0, 1], dtype=np.int32)

    def run(n=2, a=asks, pre=orc.ALL, filt=orc.ALL, o=out):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return call(pm.engine, n, ptr(a), pre, filt, ptr(o))
    assert run(n=0, a=None, o=None) == 0 and run() == 0 and np.array_equal(out, full[:2])
    assert run(a=None) == INVALID and run(o=None) == INVALID and run(n=-1) == INVALID
    assert run(a=np.array([0, P], dtype=np.int32)) == INVALID and run(a=np.array([-1, 0], dtype=np.int32)) == INVALID
    assert run(filt=orc.ALL & ~IPA) == INVALID and run(pre=orc.ALL & ~IPA) == INVALID
    assert run(pre=orc.ALL & ~FIT) == INVALID and run(filt=orc.ALL & ~FIT) == INVALID
    assert run() == 0 and np.array_equal(out, full[:2])
    # the rows of one ask: the size comes back when the caller's table is too small
    rows_model = ag.model(c)[3]
    D = len(rows_model) - 1
    pod = pm._P.ykpred_headroom_affinity_pod
    count, rows = ctypes.c_int32(-7), np.zeros((D + 1, ROW), dtype=np.int64)
    assert pod(pm.engine, 0, orc.ALL, orc.ALL, D - 1, rows.ctypes.data, ctypes.byref(count)) == INVALID and count.value == D and not rows.any()
    assert pod(pm.engine, 0, orc.ALL, orc.ALL, D, rows.ctypes.data, ctypes.byref(count)) == 0 and rows.tolist() == rows_model
    assert pod(pm.engine, 0, orc.ALL, orc.ALL & ~IPA, D, rows.ctypes.data, ctypes.byref(count)) == INVALID
    assert pod(pm.engine, P, orc.ALL, orc.ALL, D, rows.ctypes.data, ctypes.byref(count)) == INVALID
    assert pod(pm.engine, 0, orc.ALL, orc.ALL, D, rows.ctypes.data, None) == INVALID
    with pytest.raises(RuntimeError):
        pm.headroom_affinity([P])
    # without the spec effects of the current spec table the engine does not know what a copy adds: the rule of ykpred_allocate_round
    assert pm._P.ykpred_set_spec_effects(pm.engine, None) == 0
    assert run() == UNSUPPORTED
    # no nodes at all: the verdicts alone (a fresh load: the host uploads the effects again)
    pm.load_snapshot({"nodes": [], "pods": snap["pods"]})
    empty = pm.headroom_affinity()
    assert pm.num_nodes == 0 and np.array_equal(empty[:, 3], full[:, 3])
    assert empty[0].tolist() == [0] * 11 + [-1, empty[0, 12], 1, 0, 0]
    assert np.array_equal(pm.headroom_affinity(pre_mask=orc.ALL, filt_mask=orc.ALL), empty)  # the engine itself: a routed ask is 1 here too


def test_needs_no_evaluation_disturbs_none_and_follows_assume_pod():
    """Before any evaluation; ykpred_answer_state and the bitmap checksum unchanged by the call; then AssumePod of one copy on the host
    a round picks for it: that domain is shut — cnt > 0 on its row, copies 0 — every other row is as before and [0] falls by exactly 1,
    with no evaluation between the assume and the call; and the same by the model with the copy as a resident of that node."""
    c = CASES["host-self-1500"]
    snap = hg.clones(c["snapshot"], 0, 6)
    uid = lambda k: f"a-host-self-1500-copy-{k}"  # noqa: E731
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(snap)
        rows, cells = expected(m, c)
        assert m.counters()["full_evals"] == 0
        assert m.headroom_affinity([5])[0].tolist() == cells  # before any evaluation
        assert m.counters()["full_evals"] == 0
        m.evaluate()

        def state():
            classes = ctypes.c_int32(-1)
            assert m._P.ykpred_answer_state(m.engine, orc.ALL, orc.ALL, ctypes.byref(classes)) == 0
            return (m.checksum(), classes.value, m.read_counts().tolist(), m.read_decisions().tolist(),
                    {k: v for k, v in m.counters().items() if k != "queries"})
        before = state()
        assert m.headroom_affinity()[3].tolist() == cells and m.headroom_affinity_domains(2)[1].tolist() == rows
        assert state() == before
        total, now = cells[0], c
        dom = ag.domain_of_nodes(c, ag.HOST)
        for step in range(4):
            ask = m.pod_index(uid(step))
            node = int(m.allocate_round(asks=np.array([ask], dtype=np.int32), apply=False)[0])
            assert node >= 0
            m.assume_pod(uid(step), snap["nodes"][node]["metadata"]["name"])
            evals = m.counters()["full_evals"]
            last = m.pod_index(uid(5))
            got = m.headroom_affinity([last])[0]
            got_rows = m.headroom_affinity_domains(last)[1]
            assert m.counters()["full_evals"] == evals
            assert got[3] == 0 and got[0] == total - 1, (step, got.tolist())
            total -= 1
            d = dom[node]
            if d < len(rows) - 1:  # a labelled host: its row is shut now
                print("assumed on domain", d, got_rows[d].tolist())
                assert got_rows[d, 0] >= 1 and got_rows[d, 1:].tolist() == [0, 0, 0]
            # the model with the copy standing there (its request is taken off the node's free values by hand: cpu alone binds here)
            now = ag.with_resident(now, node, now["ask_labels"], now["anti"])
            now["meta"] = {"templates": now["meta"]["templates"], "nodes": [dict(n) for n in now["meta"]["nodes"]]}
            info = now["meta"]["nodes"][node]
            info["free"] = dict(info["free"], cpu=info["free"]["cpu"] - 1500)
            info["slots"] -= 1
            want_rows, want_cells = expected(m, now)
            assert got.tolist() == want_cells and got_rows.tolist() == want_rows, step
    finally:
        m.close()


@pytest.mark.parametrize("name", ["host-self-1500", "zone-self-res", "host-other", "aff-svc-host-self", "zone-existing"])
def test_a_round_over_the_clones_places_exactly_the_answer(pm, name):
    c = CASES[name]
    status, key, mode, rows, cells = ag.model(c)
    total = cells[0]
    pm.load_snapshot(hg.clones(c["snapshot"], 0, total + 2))
    assert pm.headroom_affinity([0])[0, 0] == total
    placed = pm.allocate_round()
    assert int((placed >= 0).sum()) == total and int((placed == -1).sum()) == 2
    dom = np.array(ag.domain_of_nodes(c, key))
    assert np.bincount(dom[placed[placed >= 0]], minlength=len(rows)).tolist() == [r[3] for r in rows]


def test_node_sharded_engines_return_cluster_wide_rows(tmp_path):
    """World 2 on one GPU, the collectives through tests/c/rccl_stub.cpp (tests/_shard_affinity_headroom_worker.py): both ranks equal a
    single engine over all nodes and the model; the residents that decide an ask's rows stand on the other shard."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29673", os.path.join(ROOT, "tests", "_shard_affinity_headroom_worker.py")]
    env = {k: v for k, v in os.environ.items() if k != "YKPRED_TUNE"}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, SHARD_RCCL_STUB=stub))
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("affinity-headroom True model True rows True decided-elsewhere True bootstrap True mismatch True") == 2, (out.stdout[-1500:], out.stderr[-1500:])
