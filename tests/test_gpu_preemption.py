"""PreemptionPredicates on the device — preempt_one / k_preempt, ykpred_preemption_batch, and the host's append_victims — on the
designed populations of tests/_preemptgen.py.

Every case loads the JSON text of a Python-built snapshot. Expected answers are the oracle's and the model's (held equal, and to
the generator's intentions, by tests/test_preemption_inputs.py — which also asserts that fewer than half of them are -1), never
another engine call. One cross-check does not go through the preemption kernel at all: the victims are really removed from the
cache one at a time and Predicates() must turn to "fits" exactly at the index the kernel returned. All inputs are valid; argument
errors are asked of the host library only, which (with the engine's argument check behind it) refuses them before anything is
launched. Nothing here has a tolerance."""
import copy
import importlib
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import _preemptgen
from test_preemption_inputs import FORMS, LISTS, POPULATIONS, TOPOLOGY_FORMS, Case, case, histogram

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("yunikorn-k8shim_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE = 200


def manager(form):
    if form == "default":
        return pkg.GpuPredicateManager()
    pre, filt = LISTS[form]
    return pkg.GpuPredicateManager.internal(list(pre), list(pre), list(filt), list(filt))


def check_batch(m, c, form, what, queries=None, expected=None):
    """One launch for all the queries; the whole array against the oracle and against the model."""
    by_oracle, by_model = expected if expected is not None else c.answers(form, queries)
    got = np.array(m.preemption_predicates_batch(c.queries if queries is None else queries), dtype=np.int32)
    assert np.array_equal(by_oracle, by_model), f"{what}: the two references differ"
    bad = np.flatnonzero(got != by_oracle)
    if bad.size:
        q = (c.queries if queries is None else queries)[bad[0]]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} answers differ, first at query {bad[0]} (ask {q[0]}, node {q[1]}, {len(q[2])} victims, "
                             f"start {q[3]}): gpu {got[bad[0]]} want {by_oracle[bad[0]]}")
    return got


@pytest.mark.parametrize("name,form", [(n, f) for n in POPULATIONS for f in FORMS + (TOPOLOGY_FORMS if n == "topology_frozen" else ())])
def test_designed_population(name, form):
    """One population under one manager (the default one, NodeResourcesFit alone, NodeResourcesFit + NodePorts; topology_frozen
    also under the managers limited to either topology plugin and the two Filter-without-PreFilter forms): the whole batch in one
    launch, a fixed sample of 200 one by one through preemption_predicates, the same sample through
    is_pod_fit_node_via_preemption by keys."""
    c = case(name)
    by_oracle, _ = c.answers(form)
    m = manager(form)
    t0 = time.perf_counter()
    try:
        m.load_snapshot(c.text)
        check_batch(m, c, form, f"{name} [{form}]")
        sample = sorted(random.Random(1).sample(range(len(c.queries)), min(SAMPLE, len(c.queries))))
        for q in sample:
            uid, node, victims, start = c.queries[q]
            one = m.preemption_predicates(uid, node, victims, start)
            assert one == by_oracle[q], f"{name} [{form}]: query {q} alone (ask {uid}, node {node}, start {start}): gpu {one} want {by_oracle[q]}"
            by_key = m.is_pod_fit_node_via_preemption(uid, node, victims, start)
            assert by_key == (by_oracle[q], by_oracle[q] != -1), f"{name} [{form}]: query {q} by keys: {by_key} want {by_oracle[q]}"
        uid, node, victims, start = c.queries[sample[0]]
        assert m.is_pod_fit_node_via_preemption("no-such-ask", node, victims, start) == (-1, False)
        assert m.is_pod_fit_node_via_preemption(uid, "no-such-node", victims, start) == (-1, False)
        if form == "default":
            routed = [p["metadata"]["uid"] for p in c.snapshot["pods"] if not m.ask_supported(p["metadata"]["uid"])[0]]
            assert not routed, f"{name}: routed as unsupported: {routed[:3]}"
            lay, tables = m.layout(), m.stats()
            if name == "resource_edges":
                assert tables["R"] == 8, tables
            if name == "ports":
                assert m.encoded_tables()["KP"] == 2
            assert lay.num_nodes == len(c.snapshot["nodes"]) and lay.num_pods == len(c.snapshot["pods"])
    finally:
        m.close()
    print(f"PREEMPT-CASE {name} [{form}]: {len(c.queries)} queries in one launch + {len(sample)} alone + {len(sample)} by keys, "
          f"answers {histogram(by_oracle)}, {time.perf_counter() - t0:.2f} s")


def test_batch_lengths():
    """k_preempt is one thread per query in blocks of 64 over flattened victim arrays whose int pieces are padded to 8 bytes:
    batches of 1, 63, 64, 65, 129 and 1001 queries whose neighbours differ in answer and in victim count (0, 1, 300, 2, 0, ...)."""
    c = case("batch_geometry")
    by_oracle, by_model = c.answers()
    m = manager("default")
    try:
        m.load_snapshot(c.text)
        for n in c.meta["counts"]:
            check_batch(m, c, "default", f"batch of {n}", c.queries[:n], (by_oracle[:n], by_model[:n]))
        for first in (1, 2, 3):   # a batch of one that is not the empty list, and windows that start inside the cycle
            for n in (1, 63, 65):
                check_batch(m, c, "default", f"batch of {n} from query {first}", c.queries[first:first + n], (by_oracle[first:first + n], by_model[first:first + n]))
        assert m.preemption_predicates_batch([]) == []
    finally:
        m.close()


# ---- the chain: victims really removed, Predicates() asked -----------------------------------------------------------------------
def chain_sample(c, by_oracle, count=40, long_lists=2):
    """Queries with an index and start 0: every rule of the population first, then spread evenly; at most `long_lists` of 300."""
    eligible = [q for q in range(len(c.queries)) if by_oracle[q] >= 0 and c.queries[q][3] == 0]
    by_rule = {}
    for q in eligible:
        by_rule.setdefault(c.meta["rule"][q], []).append(q)
    picked = [qs[len(qs) // 2] for qs in by_rule.values()] + [qs[0] for qs in by_rule.values()]
    rest = [q for q in eligible if q not in picked]
    picked += rest[::max(len(rest) // count, 1)]
    out, long_seen = [], 0
    for q in dict.fromkeys(picked):
        if len(c.queries[q][2]) > 100:
            long_seen += 1
            if long_seen > long_lists:
                continue
        out.append(q)
    return out[:count]


@pytest.mark.parametrize("name", ["resource_edges", "slot_edges", "ports"])
def test_monotone_chain(name):
    """For 40 queries with an index k >= 0 and start 0: RemovePod of victims 0..j, one at a time, on a freshly loaded cache, and
    Predicates(ask, node, allocate) after each — it fits exactly from j = k on. Nil entries remove nothing; a uid of another node is
    really removed there; an unknown or repeated uid is refused by the cache. The identical-triple node of `ports` is among them:
    the cache's own RemovePod frees a host port with its first holder, as NodeInfo.UsedPorts does."""
    c = case(name)
    by_oracle, _ = c.answers()
    sample = chain_sample(c, by_oracle)
    assert len(sample) >= 30
    if name == "ports":
        assert any(c.meta["rule"][q] == c.meta["identical_triple"] for q in sample)
    m = manager("default")
    steps = 0
    try:
        for q in sample:
            uid, node, victims, _ = c.queries[q]
            m.load_snapshot(c.text)
            assert m.predicates(uid, node, True)[1] is not None or by_oracle[q] == 0, f"{name}: {uid} fits {node} before any removal"
            for j, v in enumerate(victims):
                if v is not None:
                    m.remove_pod(v)
                fits = m.predicates(uid, node, True)[1] is None
                assert fits == (j >= by_oracle[q]), f"{name}: query {q} (ask {uid}, node {node}, {c.meta['rule'][q]}): after removing victims 0..{j} fits={fits}, index {by_oracle[q]}"
                steps += 1
    finally:
        m.close()
    print(f"PREEMPT-CHAIN {name}: {len(sample)} queries, {steps} removals each followed by Predicates()")


# ---- state -------------------------------------------------------------------------------------------------------------------------
class Edited:
    """The Python snapshot of a case under cache operations; every edit is applied to the manager and to the snapshot."""

    def __init__(self, c, m):
        self.m, self.snapshot, self.queries, self.meta = m, copy.deepcopy(c.snapshot), list(c.queries), c.meta

    def node(self, name):
        return next(n for n in self.snapshot["nodes"] if n["metadata"]["name"] == name)

    def assume(self, uid, node):
        self.m.assume_pod(uid, node)
        ask = next(p for p in self.snapshot["pods"] if p["metadata"]["uid"] == uid)
        self.snapshot["pods"].remove(ask)
        ask["spec"]["nodeName"] = node
        self.node(node)["pods"].append(ask)
        self.queries = [q for q in self.queries if q[0] != uid]

    def forget(self, uid):
        assert self.m.forget_pod(uid)   # the pod stays accounted on its node

    def update_node(self, name, allowed):
        node = self.node(name)
        node["status"]["allocatable"]["pods"] = str(allowed)
        self.m.update_node({k: v for k, v in node.items() if k != "pods"})

    def remove(self, uid):
        assert self.m.remove_pod(uid)
        for n in self.snapshot["nodes"]:
            n["pods"] = [p for p in n["pods"] if p["metadata"]["uid"] != uid]

    def case(self):
        return Case(snapshot=copy.deepcopy(self.snapshot), queries=self.queries, meta=self.meta)


# one pod per phase: the holder of the wanted port (the ask fits from start on), a resident of start-cpu, and the ask that phase 1
# assumed there
REMOVED = ("start-port-r2", "start-cpu-r0", "state-extra-1")


def test_answers_follow_the_cache():
    """assume_pod, forget_pod, update_node and remove_pod on the queried nodes with NO evaluation in between: after each, the batch
    equals the oracle on the changed snapshot — and the answers did move (forget_pod excepted: the pod stays accounted). The same
    four again after an evaluate(), and again after an explain()."""
    base = case("start_rules")
    snapshot = copy.deepcopy(base.snapshot)
    snapshot["pods"] += [_preemptgen.make_ask(f"state-extra-{i}", {"cpu": 50 * (i + 1)}) for i in range(3)]
    c = Case(snapshot=snapshot, queries=base.queries, meta=base.meta)
    m = manager("default")
    try:
        m.load_snapshot(c.text)
        ed = Edited(c, m)
        before = check_batch(m, c, "default", "start_rules as loaded")
        for i, phase in enumerate(("no evaluation yet", "after evaluate()", "after explain()")):
            if i == 1:
                m.evaluate()
            if i == 2:
                m.explain([0, 1])
            steps = (("assume_pod", lambda: ed.assume(f"state-extra-{i}", "start-cpu"), True), ("forget_pod", lambda: ed.forget(f"state-extra-{i}"), False),
                     ("update_node", lambda: ed.update_node("start-slot", 4 + i), True), ("remove_pod", lambda: ed.remove(REMOVED[i]), True))
            for label, edit, moves in steps:
                edit()
                now = ed.case()
                got = check_batch(m, now, "default", f"{phase}, {label}")
                assert len(got) == len(before) and (not np.array_equal(got, before)) == moves, f"{phase}, {label}: answers {'did not move' if moves else 'moved'}"
                before = got
    finally:
        m.close()


@pytest.mark.parametrize("evaluated", [False, True], ids=["no-evaluation", "after-evaluate"])
def test_stale_histograms_are_rebuilt(evaluated):
    """The zone histogram of app=web reads za 3, all on y0; the asks with maxSkew 2 get -1 on x0. RemovePod of one of y0's web pods
    — a change on ANOTHER node — takes za to 2: with no evaluation in between the same asks get their cpu index (the rebuild branch
    of ensure_histograms on a single engine)."""
    c = case("topology_frozen")
    m = manager("default")
    try:
        m.load_snapshot(c.text)
        if evaluated:
            m.evaluate()
        before = check_batch(m, c, "default", "topology_frozen as loaded")
        ed = Edited(c, m)
        ed.remove(c.meta["remote_web"][0])
        now = ed.case()
        after = check_batch(m, now, "default", "topology_frozen, one web pod of y0 removed")
        flips = [q for q, query in enumerate(c.queries) if query[0] in c.meta["flips"]]
        assert len(flips) == 5 and all(before[q] == -1 and after[q] == int(c.queries[q][0].rsplit("-", 1)[1]) for q in flips)
        assert all(before[q] == after[q] for q in range(len(before)) if q not in flips)
    finally:
        m.close()


# ---- node-sharded engines ----------------------------------------------------------------------------------------------------------
def test_node_sharded_preemption_reads_the_cluster_wide_histograms(tmp_path):
    """World 2 on one GPU over tests/c/rccl_stub.cpp (tests/_shard_preempt_worker.py): x0, the queried node, sits on rank 0, the web
    pods that decide its zone verdict on rank 1. After the collective evaluate() rank 0's answers equal the oracle's on the whole
    cluster; after an update_node with no evaluation the call reports the state error, not an index."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29731",
           os.path.join(ROOT, "tests", "_shard_preempt_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("preemption True local-only-differs True stale True") == 1, (out.stdout[-1500:], out.stderr[-1500:])


# ---- argument errors: refused before any launch ------------------------------------------------------------------------------------
def test_argument_errors_are_refused_before_any_launch():
    """Indices out of range and descending offsets stop in the host, a negative start and offsets that do not begin at 0 in the
    engine's argument check; none reaches the launch, `out` stays untouched and the next valid batch is answered as ever."""
    c = case("start_rules")
    m = manager("default")
    try:
        m.load_snapshot(c.text)
        expected = check_batch(m, c, "default", "start_rules before the refused calls")
        L = m._L
        n_asks, n_nodes = len(c.snapshot["pods"]), len(c.snapshot["nodes"])
        cases = (("ask index", [n_asks, 0], [0, 0], [0, 0, 0], [0, 0]), ("node index", [0, 0], [0, n_nodes], [0, 0, 0], [0, 0]),
                 ("negative ask", [-1, 0], [0, 0], [0, 0, 0], [0, 0]), ("descending offsets", [0, 0], [0, 0], [0, 1, 0], [0, 0]),
                 ("negative start", [0, 0], [0, 0], [0, 0, 0], [0, -1]), ("offsets from 1", [0, 0], [0, 0], [1, 1, 1], [0, 0]))
        for what, p, n, off, st in cases:
            pods, nodes, offsets, starts = (np.array(x, dtype=np.int32) for x in (p, n, off, st))
            out = np.full(2, -77, dtype=np.int32)
            rc = L.ykhost_preemption_predicates_batch(m._h, 2, pods.ctypes.data, nodes.ctypes.data, offsets.ctypes.data, None, starts.ctypes.data, out.ctypes.data)
            assert rc < 0 and out.tolist() == [-77, -77], (what, rc, out.tolist())
        assert L.ykhost_preemption_predicates_batch(m._h, -1, None, None, None, None, None, None) < 0
        assert L.ykhost_preemption_predicates_batch(m._h, 1, None, None, None, None, None, None) < 0
        with pytest.raises(RuntimeError):
            m.preemption_predicates(c.queries[0][0], c.queries[0][1], [], -1)
        assert np.array_equal(check_batch(m, c, "default", "start_rules after the refused calls"), expected)
    finally:
        m.close()
