"""ykpred_preempt_round on the MI355X against the model of tests/_preemptroundgen.py — which tests/test_preempt_round_inputs.py pins to
the reference step by step: all 8 cells of every turn and the summary on every designed round and plugin list, the bare engine ABI on a
hand-built victim table whose slack rows would change an answer if read, the three identities (the host loop with real remove_pod /
assume_pod, preempt_headroom's copies, preempt_victims' best node), device against device at 4 100 nodes, an empty list, two calls in a
row, nothing resident touched, sharded."""
import copy
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as orc
import _preemptgen
import _preemptroundgen as gen
import _victimgen
from _victimgen import placed
from test_gpu_preempt_victims import manager, upload
from test_preempt_round_inputs import FORMS, ROUNDS, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu
CELLS = 8


def loaded(c, form="default"):
    m = manager(form)
    m.load_snapshot(c.text)
    m.set_preemption_tiers(c.bounds)
    return m


def same(got, want, turns, what=""):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.shape == want.shape and len(bad) == 0, (what, turns[bad[0]], int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad))


@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("name", ROUNDS)
def test_cells_and_summary_on_every_round(name, form):
    c = case(name)
    want, want_summary = c.cells(form)
    m = loaded(c, form)
    try:
        got, summary = m.preempt_round(c.turns)
        same(got, want, c.turns, f"{name} / {form}")
        assert summary.tolist() == want_summary.tolist()
        if form == "default":
            before = m.preempt_victims()
            # by key, one crossing: the same cells, the node by name, the victims by uid
            cells, summary2, names, victims = m.preempt_round_by_keys(c.turns)
            same(cells, want, c.turns, name)
            assert summary2.tolist() == want_summary.tolist()
            for i, row in enumerate(want):
                assert names[i] == (c.nodes[row[1]] if row[1] >= 0 else ""), c.turns[i]
                assert victims[i] == (c.model.victims_of(row) if row[1] >= 0 else []), c.turns[i]
                assert len(victims[i]) == row[3]
            # state starts at zero in every call, and nothing resident was touched
            again, _ = m.preempt_round(c.turns)
            assert np.array_equal(again, got) and np.array_equal(m.preempt_victims(), before)
            assert m.counters()["full_evals"] == 0
        if "no-fit" not in form:
            # outcomes 3 and 4 are ykpred_headroom's statuses 1 and 2 under the same lists: the rule is the engine's, not the model's
            status = manager(form)
            try:
                status.load_snapshot(c.text)
                head = status.headroom(c.turns)[:, pkg.HEADROOM_STATUS]
            finally:
                status.close()
            assert np.array_equal(np.where(got[:, 0] >= 3, got[:, 0] - 2, 0), head), f"{name} / {form}"
    finally:
        m.close()


def engine_round(m, asks, limits):
    asks = np.ascontiguousarray(asks, dtype=np.int32)
    limits = np.ascontiguousarray(limits, dtype=np.int32)
    out = np.full((max(len(asks), 1), CELLS), 7, dtype=np.int64)
    summary = np.full(8, 7, dtype=np.int64)
    rc = m._P.ykpred_preempt_round(m.engine, len(asks), asks.ctypes.data, limits.ctypes.data, orc.ALL, orc.ALL, out.ctypes.data, summary.ctypes.data)
    return rc, out[:len(asks)], summary


@pytest.mark.parametrize("name", ("conflicts", "exact_hi", "bisect", "gang_p2"))
def test_bare_engine_abi_with_a_hand_built_table(name):
    """The mirror's planes laid out anew by hand — segments in REVERSE node order, three slack rows behind each and one in front of the
    first, every slack row holding 2^62 in each dimension and all-ones port words — uploaded through ykpred_set_victims, then the round
    through ykpred_preempt_round itself: a read outside a segment would open or shut a pair."""
    c = case(name)
    m = loaded(c)
    try:
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
        assert upload(m, T, base, cap, np.ascontiguousarray(t["tier_end"]), cum, ports) == 0
        # (the routed ask goes to the engine too: it settles an unsupported spec itself, without a step)
        turns = c.turns
        want, want_summary = c.cells()
        assert name != "conflicts" or 3 in want[:, 0]
        asks = [m.pod_index(uid) for uid in turns]
        limits = [c.model.asks[uid][2] for uid in turns]
        rc, out, summary = engine_round(m, asks, limits)
        assert rc == 0
        same(out, want, turns, name)
        assert summary.tolist() == want_summary.tolist()
        # errors as ykpred_preempt_victims: a limit outside 0..T, an index out of range — nothing written; an empty list is fine
        for bad in (T + 1, -1):
            rc, out2, summary2 = engine_round(m, asks, limits[:-1] + [bad])
            assert rc == -1 and (out2 == 7).all() and (summary2 == 7).all()
        assert engine_round(m, asks[:-1] + [len(c.asks)], limits)[0] == -1
        rc, _, summary = engine_round(m, [], [])
        assert rc == 0 and not summary.any()
        q = m.counters()["queries"]
        engine_round(m, asks, limits)
        assert m.counters()["queries"] == q + 1
    finally:
        m.close()


def test_without_a_victim_table_and_with_an_empty_list():
    c = case("gang_eq")
    m = manager()
    try:
        m.load_snapshot(c.text)
        m.sync()
        assert engine_round(m, [0], [0])[0] == -4   # YKPRED_E_STATE: no victim table
        with pytest.raises(RuntimeError, match="no preemption tiers"):
            m.preempt_round([0])
        m.set_preemption_tiers(c.bounds)
        got, summary = m.preempt_round([])
        assert got.shape == (0, CELLS) and not summary.any()
        cells, summary, names, victims = m.preempt_round_by_keys([])
        assert cells.shape == (0, CELLS) and names == [] and victims == []
        with pytest.raises(KeyError):
            m.preempt_round_by_keys(["gang", "no-such-pod"])
    finally:
        m.close()


def gang_scene(copies):
    """The gang round's two nodes and a third that costs a higher tier, with `copies` DISTINCT asks of one spec."""
    b = _victimgen.BOUNDS[3]
    lo, mid = b[0] - 1, b[1] - 1
    nodes = [_preemptgen.make_node("g-a", {"cpu": 500, "memory": 1 << 30}, [placed(f"g-a-v{i}", lo, {"cpu": 100}) for i in range(3)] + [placed("g-a-top", b[2], {"cpu": 100})]),
             _preemptgen.make_node("g-b", {"cpu": 200, "memory": 1 << 30}, [placed(f"g-b-v{i}", lo - i, {"cpu": 100}) for i in range(2)]),
             _preemptgen.make_node("g-c", {"cpu": 250, "memory": 1 << 30}, [placed("g-c-v0", lo, {"cpu": 50}), placed("g-c-v1", mid, {"cpu": 200})])]
    asks = [_victimgen.asker(f"gang-{i:02d}", b, 2, {"cpu": 100}) for i in range(copies)]
    return {"nodes": nodes, "pods": asks}, list(b)


def host_loop(m, uids, snapshot):
    """What the round replaces: per ask the need of every node, the best by (level, need, index), remove_pod per victim, assume_pod.
    → rows [outcome, node, victims removed from the node before, need, level]."""
    removed = {}
    rows = []
    name_of = {m.node_index(n["metadata"]["name"]): n["metadata"]["name"] for n in snapshot["nodes"]}
    for uid in uids:
        needs, levels = m.preempt_victims_nodes(uid), m.preempt_reach_nodes(uid)
        keys = [(int(levels[n]) if needs[n] else 0, int(needs[n]), n) for n in range(len(needs)) if needs[n] >= 0]
        if not keys:
            rows.append([2, -1, 0, 0, 0])
            continue
        level, need, n = min(keys)
        name = name_of[n]
        limit = int(m.preempt_victims([uid])[0, pkg.VICTIM_LIMIT])
        for v in m.victim_list(n, limit)[:need]:
            assert m.remove_pod(v)
        m.assume_pod(uid, name)
        rows.append([1 if need else 0, n, removed.get(n, 0), need, level])
        removed[n] = removed.get(n, 0) + need
    return rows


def test_identity_with_the_host_loop_on_distinct_pods_of_one_spec():
    """(1) The round equals the loop preempt_victims_nodes → remove_pod per victim → assume_pod, step by step; (2) it places
    min(W, preempt_headroom copies(limit)) of W copies."""
    snapshot, bounds = gang_scene(11)
    uids = [p["metadata"]["uid"] for p in snapshot["pods"]]
    m = manager()
    try:
        m.load_snapshot(copy.deepcopy(snapshot))
        m.set_preemption_tiers(bounds)
        head = m.preempt_headroom([uids[0]])[0]
        limit = int(head[pkg.PREEMPT_HEADROOM_LIMIT])
        copies = int(head[pkg.PREEMPT_HEADROOM_COPIES + limit])
        assert limit == 2 and copies == 8   # g-a 1 + 3, g-b 2, g-c 2 once both of its victims are gone
        for W in (copies - 1, copies, copies + 2):
            cells, summary = m.preempt_round(uids[:W])
            assert summary[0] + summary[1] == min(W, copies) and summary[2] == W - min(W, copies)
            gang = m.preempt_gang(uids[0], W)
            assert np.array_equal(gang[0], cells) and gang[1].tolist() == summary.tolist()
        cells, summary, names, victims = m.preempt_round_by_keys(uids)
        assert m.counters()["full_evals"] == 0
        rows = host_loop(m, uids, snapshot)
        assert cells[:, :5].tolist() == rows
        assert len({r[1] for r in rows}) == 4 and {r[0] for r in rows} == {0, 1, 2}
    finally:
        m.close()


@pytest.mark.parametrize("name", ("conflicts", "places", "exact_lo"))
def test_identity_with_preempt_victims_for_a_round_of_one_ask(name):
    c = case(name)
    m = loaded(c)
    try:
        victims = m.preempt_victims()
        seen = set()
        for a, uid in enumerate(c.asks):
            if c.model.settled(uid):
                continue
            row = m.preempt_round([uid])[0][0]
            if victims[a, pkg.VICTIM_FIT] == 0:
                assert row[[4, 1, 3]].tolist() == victims[a, 5:8].tolist(), uid
                assert row[6] == victims[a, pkg.VICTIM_OPEN] and row[7] == victims[a, pkg.VICTIM_TOTAL] and row[0] == (1 if row[3] else 2)
            else:
                assert row[[0, 3, 4]].tolist() == [0, 0, 0] and row[6] == victims[a, pkg.VICTIM_FIT] + victims[a, pkg.VICTIM_OPEN]
                assert row[1] == int(np.flatnonzero(m.preempt_victims_nodes(a) == 0)[0])
            seen.add(int(row[0]))
        assert 1 in seen and (name != "conflicts" or seen == {0, 1, 2})
    finally:
        m.close()


def test_device_against_device_at_4100_nodes_with_70_asks():
    """70 asks of 70 distinct tasks in non-increasing limit order over 4 100 nodes with up to 12 victims each: the round against the
    loop of need per node, real remove_pod and assume_pod on a second manager."""
    snapshot, bounds, meta = gen.geometry(20265, 4100)
    uids = meta["turns"]
    m, loop = manager(), manager()
    try:
        m.load_snapshot(copy.deepcopy(snapshot))
        m.set_preemption_tiers(bounds)
        cells, summary = m.preempt_round(uids)
        loop.load_snapshot(copy.deepcopy(snapshot))
        loop.set_preemption_tiers(bounds)
        rows = host_loop(loop, uids, snapshot)
        assert cells[:, :5].tolist() == rows
        assert summary[0] > 0 and summary[1] > 0 and summary[2] > 0 and (cells[:, 2] > 0).sum() >= 5 and summary[5] == cells[:, 3].sum()
        assert len(set(cells[:, 5].tolist())) == 4 and (np.diff(cells[:, 5]) <= 0).all()
    finally:
        m.close()
        loop.close()


def test_node_sharded_engines_plan_the_round_together(tmp_path):
    """World 2 on one GPU over tests/c/rccl_stub.cpp (tests/_shard_preempt_round_worker.py): the best node on the other shard, a
    cross-shard tie to the lower global index, the second ask sees the first's placement on the remote shard."""
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-std=c++17", os.path.join(ROOT, "tests", "c", "rccl_stub.cpp"), "-o", stub, "-lrt"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29748",
           os.path.join(ROOT, "tests", "_shard_preempt_round_worker.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, SHARD_RCCL_STUB=stub))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    assert out.stdout.count("cells True plan True agreement True") == 2, (out.stdout[-1500:], out.stderr[-1500:])
