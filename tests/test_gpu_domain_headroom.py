"""ykpred_headroom_groups on the device: headroom per topology domain (k_headroom_groups, k_group_summary), through the host library
(label key) and the explicit group column — against the model over Python ints of tests/_domaingen.py and the reference's own clone
loop on designed clusters, at the kernel's widths in both accumulation forms and three table chunks, against the existing per-node
calls on adversarial clusters, its list semantics and errors, its independence of the evaluation state, node-sharded engines, and a gang
end to end."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _advgen
import _domaingen as dg
import _headgen as hg
import _oracle as orc

pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = orc.PLUGIN_BITS["NodeResourcesFit"]
CELLS, SUMMARY = 2, 8
INVALID, STATE = -1, -4


@pytest.fixture(scope="module")
def pm():
    m = pkg.GpuPredicateManager()
    yield m
    m.close()


def uid_index(meta, uid):
    return [t["uid"] for t in meta["templates"]].index(uid)


def ask_list(g, thin=False):
    """→ (pods, wants, tables): every template with every want of dg.wants (thin: four of them, the ends included)."""
    meta, column, G = g["meta"], g["column"], g["G"]
    pods, wants, tables = [], [], []
    for j in range(len(meta["templates"])):
        table = dg.rows(meta, j, column, G)
        ws = dg.wants_of(table, G)
        if thin and len(ws) > 4:
            ws = ws[::max(1, len(ws) // 3)][:3] + [ws[-1]]
        tables.append(table)
        pods += [j] * len(ws)
        wants += ws
    return pods, wants, tables


def check_against_the_model(m, g, ways=("column", "key"), thin=False):
    meta, column, G = g["meta"], g["column"], g["G"]
    pods, wants, tables = ask_list(g, thin)
    for way in ways:
        if way == "key":
            if not g["label_key"]:
                continue
            summary, rows = m.headroom_domains(pods, label_key=g["label_key"], want=wants, groups=True)
        else:
            summary, rows = m.headroom_domains(pods, node_group=column, num_groups=G, want=wants, groups=True)
        assert summary.shape == (len(pods), SUMMARY) and rows.shape == (len(pods), G + 1, CELLS) and rows.dtype == np.int64
        for i, (j, w) in enumerate(zip(pods, wants)):
            status = meta["templates"][j]["status"]
            want_summary = dg.summary_of(tables[j], status, G, w)
            assert summary[i].tolist() == want_summary, (way, meta["templates"][j]["uid"], w, summary[i].tolist(), want_summary)
            if status == 2:
                assert (rows[i, :, 0] == -1).all() and rows[i, :, 1].sum() > 0
            else:
                assert rows[i].tolist() == tables[j], (way, meta["templates"][j]["uid"], np.argwhere(rows[i] != np.array(tables[j]))[:4].tolist())
    return pods, wants, tables


GROUPINGS = {"a-zone": dg.zone, "b-holes": dg.zone_holes, "c-hostname": dg.hostname, "d-tie": dg.tie, "e-empty": dg.empty_group}


@pytest.mark.parametrize("name", sorted(GROUPINGS))
def test_designed_groupings_every_row_and_summary_against_the_model_and_the_clone_loop(pm, name):
    g = GROUPINGS[name]()
    meta, column, G = g["meta"], g["column"], g["G"]
    pm.load_snapshot(g["snapshot"])
    if g["label_key"]:
        values = pm.domain_values(g["label_key"])
        assert values == sorted(values) and len(values) == G
        have = [node["metadata"]["labels"].get(g["label_key"]) for node in g["snapshot"]["nodes"]]
        assert [values.index(v) if v is not None else -1 for v in have] == column
    check_against_the_model(pm, g)
    # the rows against the reference's clone loop, node counts bincounted by group — over the cluster the loop ran on
    if name == "b-holes":
        pm.load_snapshot(dg.zone()["snapshot"])
    loops = hg.clone_loop()
    ids = np.array([c if c >= 0 else G for c in column])
    computed = sorted(loops)
    _, rows = pm.headroom_domains(computed, node_group=column, num_groups=G, groups=True)
    for i, j in enumerate(computed):
        copies = np.bincount(ids, weights=loops[j], minlength=G + 1).astype(np.int64)  # (at most 2000 copies: exact in float64)
        nodes = np.bincount(ids[loops[j] >= 1], minlength=G + 1)
        assert np.array_equal(rows[i, :, 0], copies) and np.array_equal(rows[i, :, 1], nodes), (name, meta["templates"][j]["uid"])
    if name == "d-tie":  # the tie, spelled out: both tied groups hold `top`, the lower id is the answer to both questions
        top = dg.rows(meta, 0, column, G)[1][0]
        s = pm.headroom_domains(["t-main"], label_key=dg.TIE_KEY, want=top)[0]
        assert s.tolist() == [0, 4, 2, 1, top, 1, top, s[7]] and s[7] > 0
        out, best, tight = np.zeros(SUMMARY, dtype=np.int64), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        call = pm._L.ykhost_headroom_domain_by_key
        assert call(pm._h, b"t-main", dg.TIE_KEY.encode(), top, out.ctypes.data, best, 64, tight, 64) == 0
        assert out.tolist() == s.tolist() and best.value == b"d1" and tight.value == b"d1"
        assert call(pm._h, b"t-main", dg.TIE_KEY.encode(), top + 1, out.ctypes.data, best, 64, tight, 64) == 0
        assert out[2] == 0 and best.value == b"d1" and tight.value == b""
        assert call(pm._h, b"t-routed", dg.TIE_KEY.encode(), 1, out.ctypes.data, best, 64, tight, 64) == -13 and out.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
        assert call(pm._h, b"no-such-pod", dg.TIE_KEY.encode(), 1, out.ctypes.data, best, 64, tight, 64) == -10
        assert call(pm._h, b"res-3", dg.TIE_KEY.encode(), 1, out.ctypes.data, best, 64, tight, 64) == -12
        # a key no node carries: no domain, every copy on ungrouped nodes
        s, rows = pm.headroom_domains(["t-main"], label_key="no-such-label", want=1, groups=True)
        assert pm.domain_values("no-such-label") == [] and rows.shape == (1, 1, CELLS)
        assert s[0].tolist() == [0, 0, 0, -1, 0, -1, 0, hg.expected_cells(meta, 0)[0]] and rows[0, 0].tolist() == hg.expected_cells(meta, 0)[:2]


@pytest.mark.parametrize("n_nodes", [63, 64, 65, 191, 257])
def test_kernel_widths_both_accumulation_forms_three_table_chunks(monkeypatch, n_nodes):
    """One node short of a wave, a full wave, one node past it, short of three waves, one node past a workgroup; 70 distinct tasks =
    three kernel task chunks, and three TABLE chunks of 24, 24 and 22 tasks (group_chunk_tasks: the budget itself counts in MB, which a
    table of this size never fills). The zones (one to three of them at these sizes), G = N and G on either side of the LDS-form limit, each with the adds forced straight into
    the global table (group_lds=0) and into LDS wherever the table fits (group_lds=1): both equal the model."""
    groupings = [dg.zone(n_nodes, 56), dg.hostname(n_nodes, 56)] + [dg.modulo(n_nodes, G, 56) for G in (dg.LDS_LIMIT - 1, dg.LDS_LIMIT, dg.LDS_LIMIT + 1)]
    assert len(groupings[0]["meta"]["templates"]) == 70
    answers = []
    for lds in (0, 1):
        monkeypatch.setenv("YKPRED_TUNE", f"group_lds={lds},group_chunk_tasks=24")
        m = pkg.GpuPredicateManager()
        try:
            m.load_snapshot(groupings[0]["snapshot"])
            for g in groupings:
                pods, wants, _ = check_against_the_model(m, g, ways=("column",), thin=True)
                answers.append(m.headroom_domains(pods, node_group=g["column"], num_groups=g["G"], want=wants, groups=True))
            check_against_the_model(m, groupings[0], ways=("key",), thin=True)
        finally:
            m.close()
    half = len(groupings)
    for a, b in zip(answers[:half], answers[half:]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_scratch_budget_below_one_task_gives_one_task_per_table_chunk(monkeypatch):
    """group_scratch_mb=0: the budget holds no task, the chunk size falls back to one task — 70 table chunks, each with a one-task kernel
    grid, a summary launch of its own and a copy back — in both accumulation forms (G = 2 zones, G = N), equal to the model."""
    groupings = [dg.zone(65, 56), dg.hostname(65, 56)]
    monkeypatch.setenv("YKPRED_TUNE", "group_scratch_mb=0")
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(groupings[0]["snapshot"])
        for g in groupings:
            check_against_the_model(m, g, ways=("column",), thin=True)
        check_against_the_model(m, groupings[0], ways=("key",), thin=True)
    finally:
        m.close()


@pytest.mark.parametrize("population", ["sweep", "two-dims"])
def test_adversarial_clusters_against_the_per_node_calls(pm, population):
    """tests/_advgen.py clusters (free == request ties; the int64-edge slice of two_dims): the rows equal bincount(headroom_nodes, group)
    ask by ask, and the invariants against headroom() hold — for a column with ungrouped nodes and for one group per node."""
    snap, _ = _advgen.sweep(8100, 333, 90) if population == "sweep" else _advgen.two_dims(8200, 300, 90)
    pm.load_snapshot(snap)
    P, N = pm.num_pods, pm.num_nodes
    per_node = np.stack([pm.headroom_nodes(p) for p in range(P)]).astype(np.int64)
    cells = pm.headroom()
    assert (cells[:, 3] == 0).any() and per_node.max() > 1
    for G, column in ((7, np.where(np.arange(N) % 11 == 0, -1, np.arange(N) % 7)), (N, np.arange(N))):
        ids = np.where(column < 0, G, column)
        want = np.maximum(1, cells[:, 2])  # what the fullest node takes: some group holds it
        summary, rows = pm.headroom_domains(node_group=column, num_groups=G, want=want, groups=True)
        for p in range(P):
            if cells[p, 3] == 2:
                assert summary[p, 0] == 2 and (rows[p, :, 0] == -1).all()
                continue
            copies = np.zeros(G + 1, dtype=np.int64)
            np.add.at(copies, ids, per_node[p])
            assert np.array_equal(rows[p, :, 0], copies) and np.array_equal(rows[p, :, 1], np.bincount(ids[per_node[p] >= 1], minlength=G + 1)), p
            assert summary[p, 0] == cells[p, 3]
        done = cells[:, 3] == 0
        assert np.array_equal(rows[done][:, :G, 0].sum(axis=1) + summary[done, 7], cells[done, 0])
        assert np.array_equal(rows[done][:, :, 1].sum(axis=1), cells[done, 1])
        assert (summary[done, 4] <= cells[done, 0]).all() and (summary[done, 6] <= summary[done, 4]).all()
        assert ((summary[done, 2] > 0) == (summary[done, 5] >= 0)).all() and (summary[done, 2] <= summary[done, 1]).all()
        if G == N:  # one group per node: the group with the most copies is the fullest node, lowest index first
            fits = done & (cells[:, 1] > 0)
            assert np.array_equal(summary[fits, 3], per_node[fits].argmax(axis=1)) and np.array_equal(summary[fits, 4], cells[fits, 2])


def test_list_semantics_statuses_and_errors(pm):
    g = dg.zone_holes(131)
    snap, meta, column, G = g["snapshot"], g["meta"], np.array(g["column"], dtype=np.int32), g["G"]
    pm.load_snapshot(snap)
    P, N = pm.num_pods, pm.num_nodes
    pm.sync()
    q0 = pm.counters()["queries"]
    full, full_rows = pm.headroom_domains(label_key="zone", want=2, groups=True)
    assert pm.counters()["queries"] == q0 + 1  # one query, however many asks (the group ids come from the mirror)
    rng = np.random.default_rng(12)
    pick = rng.integers(0, P, size=3 * P)
    assert len(set(pick.tolist())) < len(pick)
    s, r = pm.headroom_domains(pick, label_key="zone", want=2, groups=True)
    assert np.array_equal(s, full[pick]) and np.array_equal(r, full_rows[pick])
    s, r = pm.headroom_domains(pick, node_group=column, num_groups=G, want=2, groups=True, pre_mask=orc.ALL, filt_mask=orc.ALL)
    assert np.array_equal(s, full[pick]) and np.array_equal(r, full_rows[pick])  # the engine itself, routed ask included
    uids = [snap["pods"][i]["metadata"]["uid"] for i in pick[:7]]
    assert np.array_equal(pm.headroom_domains(uids, label_key="zone", want=2), full[pick[:7]])
    assert np.array_equal(pm.headroom_domains(pick, label_key="zone", want=2), full[pick])  # no table asked for: the same summaries
    # one ask listed with two wants: the same rows, each want's own summary
    main = dg.rows(meta, 0, g["column"], G)
    low, high = min(r[0] for r in main[:G] if r[0] > 0), max(r[0] for r in main[:G])
    assert low < high
    s, r = pm.headroom_domains([0, 0, 0], node_group=column, num_groups=G, want=[low, high, high + 1], groups=True)
    assert [row.tolist() for row in s] == [dg.summary_of(main, 0, G, w) for w in (low, high, high + 1)]
    assert s[0, 5] != s[1, 5] and s[2, 5] == -1 and np.array_equal(r[0], r[1]) and np.array_equal(r[1], r[2]) and r[0].tolist() == main
    # a routed ask: status 1 and zeros, by the host and by the engine alike; a coupled one: status 2, copies -1, nodes = the fits by group
    routed, coupled = uid_index(meta, "t-routed"), uid_index(meta, "t-spread")
    assert full[routed].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and not full_rows[routed].any()
    assert full[coupled].tolist() == [2, 0, 0, -1, 0, -1, 0, -1] and (full_rows[coupled, :, 0] == -1).all()
    fit, _, _ = pm.query(np.full(N, coupled, dtype=np.int32), np.arange(N, dtype=np.int32))
    assert np.array_equal(full_rows[coupled, :, 1], np.bincount(np.where(column < 0, G, column)[fit != 0], minlength=G + 1)) and fit.sum() > 0
    assert full_rows[coupled, :, 1].sum() == pm.headroom([coupled])[0, 1]
    # n = 0 is OK; the YKPRED_E_INVALID cases, each on its own
    assert pm.headroom_domains([], label_key="zone").shape == (0, SUMMARY)
    assert pm.headroom_domains([], node_group=column, num_groups=G).shape == (0, SUMMARY)
    call = pm._P.ykpred_headroom_groups
    out, table = np.zeros((2, SUMMARY), dtype=np.int64), np.zeros((2, G + 1, CELLS), dtype=np.int64)
    asks, want = np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.int64)

    def run(n=2, a=asks, w=want, groups=G, col=column, pre=orc.ALL, filt=orc.ALL, o=out, t=table):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return call(pm.engine, n, ptr(a), ptr(w), groups, ptr(col), pre, filt, ptr(o), ptr(t))
    assert run(n=0, a=None, w=None, col=None, o=None, t=None) == 0
    assert run() == 0 and np.array_equal(out[0], pm.headroom_domains([0], label_key="zone", want=1)[0])
    assert run(w=None) == 0 and run(t=None) == 0
    assert run(a=None) == INVALID and run(o=None) == INVALID and run(col=None) == INVALID and run(n=-1) == INVALID
    assert run(a=np.array([0, P], dtype=np.int32)) == INVALID and run(a=np.array([-1, 0], dtype=np.int32)) == INVALID
    assert run(groups=0) == INVALID and run(groups=-3) == INVALID
    assert run(w=np.array([1, 0], dtype=np.int64)) == INVALID and run(w=np.array([-5, 1], dtype=np.int64)) == INVALID
    bad = column.copy()
    bad[N - 1] = G
    assert run(col=bad) == INVALID
    bad[N - 1] = -2
    assert run(col=bad) == INVALID
    assert run(pre=orc.ALL & ~FIT) == INVALID and run(filt=orc.ALL & ~FIT) == INVALID
    assert run() == 0  # (none of them left anything behind)
    host = pm._L.ykhost_headroom_domains
    assert host(pm._h, 2, np.array([0, P], dtype=np.int32).ctypes.data, None, b"zone", out.ctypes.data, None, 0) == INVALID
    assert host(pm._h, 2, asks.ctypes.data, np.array([1, 0], dtype=np.int64).ctypes.data, b"zone", out.ctypes.data, None, 0) == INVALID
    assert host(pm._h, 2, asks.ctypes.data, None, b"zone", out.ctypes.data, table.ctypes.data, table.size - 1) == INVALID
    assert host(pm._h, 2, asks.ctypes.data, None, b"zone", out.ctypes.data, table.ctypes.data, table.size) == G
    assert host(pm._h, 2, asks.ctypes.data, None, None, out.ctypes.data, None, 0) == -1
    with pytest.raises(RuntimeError):
        pm.headroom_domains([P], label_key="zone")
    with pytest.raises(RuntimeError):
        pm.headroom_domains([0], node_group=column, num_groups=G, pre_mask=orc.RESERVE_PRE, filt_mask=orc.RESERVE_FILT)
    # YKPRED_E_STATE before the tables are uploaded: an engine of its own that was handed nothing
    ffi = importlib.import_module("yunikorn-k8shim_amd._ffi")
    bare = ctypes.c_void_p()
    cfg = ffi.YkpredConfig(abi_version=4, device=0, num_resources=4, taint_words=1, label_words=1, topology_keys=0, selector_classes=0, port_words=1)
    assert pm._P.ykpred_create(ctypes.byref(cfg), ctypes.byref(bare)) == 0
    try:
        assert call(bare, 2, asks.ctypes.data, want.ctypes.data, G, column.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data, None) == STATE
        assert call(bare, 2, asks.ctypes.data, want.ctypes.data, G, column.ctypes.data, orc.ALL & ~FIT, orc.ALL, out.ctypes.data, None) == INVALID
    finally:
        pm._P.ykpred_destroy(bare)
    # no nodes at all: zero rows, no group
    pm.load_snapshot({"nodes": [], "pods": snap["pods"][:3]})
    s, r = pm.headroom_domains(node_group=np.zeros(0, dtype=np.int32), num_groups=2, want=1, groups=True)
    assert pm.num_nodes == 0 and not r.any() and [row.tolist() for row in s] == [[0, 0, 0, -1, 0, -1, 0, 0]] * 3
    s = pm.headroom_domains(label_key="zone")
    assert [row.tolist() for row in s] == [[0, 0, 0, -1, 0, -1, 0, 0]] * 3 and pm.domain_values("zone") == []


def test_needs_no_evaluation_and_disturbs_none():
    g = dg.zone()
    snap, meta, column, G = g["snapshot"], g["meta"], g["column"], g["G"]
    clone = json.loads(json.dumps(snap["pods"][0]))
    clone["metadata"]["name"] = clone["metadata"]["uid"] = "t-main-again"
    snap = {"nodes": snap["nodes"], "pods": snap["pods"] + [clone]}
    m = pkg.GpuPredicateManager()
    try:
        m.load_snapshot(snap)
        want_rows = np.array([dg.rows(meta, j, column, G) for j in range(12)], dtype=np.int64)
        assert m.counters()["full_evals"] == 0
        assert np.array_equal(m.headroom_domains(range(12), label_key="zone", groups=True)[1], want_rows)  # before any evaluation
        assert m.counters()["full_evals"] == 0
        m.evaluate()

        def state():
            classes = ctypes.c_int32(-1)
            assert m._P.ykpred_answer_state(m.engine, orc.ALL, orc.ALL, ctypes.byref(classes)) == 0
            counters = m.counters()
            return (m.checksum(), classes.value, m.read_counts().tolist(), m.read_decisions().tolist(),
                    {k: v for k, v in counters.items() if k != "queries"})
        before, queries = state(), m.counters()["queries"]
        summary, rows = m.headroom_domains(range(12), label_key="zone", want=5, groups=True)
        assert np.array_equal(rows, want_rows)
        by_column = m.headroom_domains(range(12), node_group=column, num_groups=G, want=5, groups=True)
        assert np.array_equal(by_column[0], summary) and np.array_equal(by_column[1], rows)
        assert state() == before and m.counters()["queries"] == queries + 2
        # AssumePod of the main template on a node that takes several copies, NO evaluation: exactly that node's group loses one copy
        # for the same template (a clone of it: the assumed ask left the ask table)
        per_node = m.headroom_nodes(0)
        node = int(np.flatnonzero(per_node >= 3)[0])
        evals = m.counters()["full_evals"]
        m.assume_pod("t-main", meta["nodes"][node]["name"])
        again = m.pod_index("t-main-again")
        after = m.headroom_domains([again], label_key="zone", groups=True)[1][0]
        assert m.counters()["full_evals"] == evals
        expect = want_rows[0].copy()
        expect[column[node], 0] -= 1
        assert np.array_equal(after, expect) and after[column[node], 1] == want_rows[0, column[node], 1]
    finally:
        m.close()


@pytest.mark.parametrize("world,total_nodes,n_pods,n_templates,chunk_tasks", [(2, 333, 300, 40, 16), (3, 1000, 250, 60, 24)],
                         ids=["two-shards", "three-shards"])
def test_node_sharded_engines_return_cluster_wide_rows_and_summaries(tmp_path, world, total_nodes, n_pods, n_templates, chunk_tasks):
    """World 2 and 3 on one GPU, the collectives through tests/c/rccl_stub.cpp (tests/_shard_domains_worker.py): every rank's rows and
    summaries equal a single engine's over the whole cluster, through the explicit column (groups of consecutive global nodes: most lie
    wholly on one shard) and through the zone label; some ask's tightest group lies on another shard; a rank that hands in another want
    makes every rank return an error."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29500 + world * 19 + total_nodes % 83), os.path.join(ROOT, "tests", "_shard_domains_worker.py"),
           str(total_nodes), str(n_pods), str(n_templates), str(chunk_tasks)]
    env = {k: v for k, v in os.environ.items() if k != "YKPRED_TUNE"}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=540, env=dict(env, SHARD_RCCL_STUB=stub))
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("rccl-stub: domains True by-key True elsewhere True tightest-elsewhere True mismatch True") == world, (out.stdout[-1500:], out.stderr[-1500:])


def test_gang_with_the_tightest_zone_as_its_selector(pm):
    """The answer used as the issue's shim would: a probe placeholder of the task group, headroom per zone for want members, the
    tightest zone as the group's nodeSelector with minMember = want — a round places all of them. With the selector on the zone whose
    copies are want - 1 instead it places exactly want - 1."""
    snap, _ = hg.designed()
    pm.load_snapshot({"nodes": snap["nodes"], "pods": []})
    group = {"name": "workers", "minResource": {"cpu": "700m", "memory": "1536Mi"}}
    assert pm.add_task_groups("app-probe", "root.batch", "default", [dict(group, minMember=1)]) == 1
    values = pm.domain_values("zone")
    _, rows = pm.headroom_domains([0], label_key="zone", groups=True)
    copies = rows[0, :len(values), 0]
    small, large = sorted(int(c) for c in copies if c > 0)[:2]
    assert values == ["z0", "z1", "z2"] and 10 < small < large < 1500
    want = small + 1
    summary = pm.headroom_domains([0], label_key="zone", want=want)[0]
    assert summary[0] == 0 and summary[2] == 1 and summary[6] == large and copies[summary[5]] == large
    tightest, short = values[int(summary[5])], values[int(np.flatnonzero(copies == small)[0])]
    assert pm.add_task_groups("app-gang", "root.batch", "default", [dict(group, minMember=want, nodeSelector={"zone": tightest})]) == want
    members = np.arange(1, want + 1, dtype=np.int32)
    placed = pm.allocate_round(asks=members, apply=False)  # (decided as a round, not applied: the ask table keeps its rows)
    assert int((placed >= 0).sum()) == want
    zone_of = np.array([values.index(n["metadata"]["labels"]["zone"]) for n in snap["nodes"]])
    assert (zone_of[placed] == summary[5]).all()
    assert pm.add_task_groups("app-short", "root.batch", "default", [dict(group, name="short", minMember=want, nodeSelector={"zone": short})]) == want
    members = np.arange(want + 1, 2 * want + 1, dtype=np.int32)
    assert pm.headroom_domains([int(members[0])], label_key="zone", want=want)[0, 2] == 0  # its own zone alone, and that holds want - 1
    placed = pm.allocate_round(asks=members)
    assert int((placed >= 0).sum()) == want - 1 and int((placed == -1).sum()) == 1
    assert (zone_of[placed[placed >= 0]] == values.index(short)).all()
