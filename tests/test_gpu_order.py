"""The bin-pack ORDER of the engine — k_score, the four k_rank_* kernels, sortable_key, the signed decision keys — as a whole
permutation on designed score clusters (tests/_ordergen.py), bit for bit against two CPU statements of the contract.

Every case loads a Python-built snapshot; the oracle is built from the same JSON text, never from dump_snapshot. The reference
order is np.lexsort((name, score)) over scores restated in plain Python floats; tests/test_order_inputs.py holds those scores
bit-equal to the oracle's, the order equal to o.decide, and shows that the populations contain what the rank kernels special-case
(negative scores, zero allocatable, a bucket of more than 1024 distinct keys, tiles of one key, bucket boundaries, int64 edges).
Compared per case: read_scores, read_order (element for element), candidates of every ask for k in {1, 5, N} in both phases,
decisions, counts, the whole bitmap, and the signed decision keys written by evaluate_into. Nothing here has a tolerance."""
import importlib
import json

import numpy as np
import pytest

import _oracle as orc
import _ordergen
from test_gpu_sequential import pm, pm_batched, round_against_oracle   # noqa: F401 (pm, pm_batched: module fixtures)
from test_order_inputs import CASES, ROUND_SEED, Reference, bits, reference

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("yunikorn-k8shim_amd")
NO_NODE_KEY = 0x7FFF_FFFF_FFFF_FFFF


def sortable_key(scores):
    """sortable_key of kernels.hip.h in numpy: the bits of a double as an unsigned integer that sorts like the double."""
    b = bits(scores)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def unpack(bitmap, n):
    return np.unpackbits(bitmap.view(np.uint8), axis=1, bitorder="little")[:, :n]


def manager(monkeypatch, tune=""):
    if tune:
        monkeypatch.setenv("YKPRED_TUNE", tune)
    else:
        monkeypatch.delenv("YKPRED_TUNE", raising=False)
    return pkg.GpuPredicateManager()


def layout_line(case, m):
    lay = m.layout()
    keys = ("num_pods", "num_nodes", "num_classes", "num_rows", "index_rows", "sweep_rows", "run_rows", "fused_rows")
    print("ORDER-LAYOUT " + case + " " + " ".join(f"{k}={getattr(lay, k)}" for k in keys))


class Indices:
    """Engine index of every node / pending ask of the reference, by name (node changes may renumber)."""

    def __init__(self, m, ref):
        n = len(ref.names)
        self.node = np.array([m.node_index(x.decode()) for x in ref.names], dtype=np.int64)
        assert m.layout().num_nodes == n and sorted(self.node.tolist()) == list(range(n))
        self.node_inv = np.empty(n, dtype=np.int64)
        self.node_inv[self.node] = np.arange(n)
        self.pod = np.array([m.pod_index(u) for u in ref.uids], dtype=np.int64)
        assert self.pod.min() >= 0 and len(set(self.pod.tolist())) == len(self.pod)
        self.identity = np.array_equal(self.node, np.arange(n)) and np.array_equal(self.pod, np.arange(len(self.pod))) and m.layout().num_pods == len(self.pod)

    def nodes_to_ref(self, engine_nodes):
        e = np.asarray(engine_nodes, dtype=np.int64)
        return np.where(e >= 0, self.node_inv[np.maximum(e, 0)], -1)


def check_order(m, ref, ix, what):
    """Scores and the whole permutation."""
    assert np.array_equal(bits(ref.scores), bits(ref.oracle_scores)), f"{what}: the two CPU statements of the score differ"
    got = m.read_scores()[ix.node]
    bad = np.flatnonzero(bits(got) != bits(ref.scores))
    assert bad.size == 0, f"{what}: {len(bad)} scores differ, first node {ref.names[bad[0]]}: gpu {got[bad[0]]!r} want {ref.scores[bad[0]]!r}"
    raw = m.read_order()
    assert sorted(raw.tolist()) == list(range(len(ref.names))), f"{what}: read_order is no permutation"
    order = ix.nodes_to_ref(raw)
    bad = np.flatnonzero(order != ref.order)
    assert bad.size == 0, (f"{what}: {len(bad)} positions of the order differ, first at {bad[0]}: gpu {ref.names[order[bad[0]]]} "
                           f"(score {ref.scores[order[bad[0]]]!r}) want {ref.names[ref.order[bad[0]]]} (score {ref.scores[ref.order[bad[0]]]!r})")


def check_answers(m, ref, ix, what, allocate=True, bitmap=True):
    """Candidates of every ask for k in {1, 5, N}, decisions, counts, the bitmap — of the phase last evaluated."""
    grid = ref.grid if allocate else ref.reserve
    n = len(ref.names)
    dec = ix.nodes_to_ref(m.read_decisions()[ix.pod])
    cnt = m.read_counts()[ix.pod]
    for p, uid in enumerate(ref.uids):
        want = ref.candidates(p, n, grid)
        for k in (1, 5, n):
            got = ix.nodes_to_ref(m.candidates(int(ix.pod[p]), k, allocate=allocate))
            assert np.array_equal(got, want[:k]), f"{what}: candidates({uid}, {k}) = {ref.names[got][:8]} want {ref.names[want[:k]][:8]}"
        assert dec[p] == (want[0] if len(want) else -1), f"{what}: decision of {uid}: {dec[p]} want {want[:1]}"
        assert cnt[p] == len(want) == grid[p].sum(), f"{what}: count of {uid}"
    if allocate:
        at = {u: k for k, u in enumerate(ref.uids)}
        assert cnt[at["nowhere"]] == 0 and cnt[at["fits-all"]] == n
    if bitmap:
        if ix.identity:   # every word, the padding bits of the last word included
            assert np.array_equal(m.read_bitmap(), orc.pack_bits(grid)), f"{what}: bitmap"
        else:
            assert np.array_equal(unpack(m.read_bitmap(), n)[ix.pod][:, ix.node], grid), f"{what}: bitmap"


def check_decision_keys(m, ref, ix, what):
    """evaluate_into with device outputs: keys[p] = int64(sortable_key(score of the decided node) ^ 2^63), or the no-node key."""
    import torch
    dev = torch.device("cuda", 0)
    lay = m.layout()
    counts = torch.full((lay.num_pods,), -7, dtype=torch.int32, device=dev)
    decisions = torch.full((lay.num_pods,), -7, dtype=torch.int32, device=dev)
    keys = torch.full((lay.num_pods,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    m.evaluate_into(counts=counts, decisions=decisions, keys=keys)
    m.synchronize()
    dec = ix.nodes_to_ref(decisions.cpu().numpy()[ix.pod])
    got = keys.cpu().numpy()[ix.pod]
    want_dec = np.array([(ref.candidates(p, 1).tolist() or [-1])[0] for p in range(len(ref.uids))])
    assert np.array_equal(dec, want_dec), f"{what}: decisions of evaluate_into"
    assert np.array_equal(counts.cpu().numpy()[ix.pod], ref.grid.sum(axis=1)), f"{what}: counts of evaluate_into"
    signed = (sortable_key(ref.scores) ^ np.uint64(1 << 63)).view(np.int64)
    want = np.where(want_dec >= 0, signed[np.maximum(want_dec, 0)], np.int64(NO_NODE_KEY))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: decision key of {ref.uids[bad[0]]} (node score {ref.scores[want_dec[bad[0]]]!r}): {int(got[bad[0]]):#x} want {int(want[bad[0]]):#x}"
    assert (want_dec < 0).any() and (got[want_dec < 0] == NO_NODE_KEY).all()
    return want_dec, (counts, decisions, keys)


def full_check(m, ref, case):
    m.load_snapshot(ref.text)
    m.evaluate()
    layout_line(case, m)
    ix = Indices(m, ref)
    assert ix.identity
    check_order(m, ref, ix, case)
    check_answers(m, ref, ix, case)
    m.evaluate(allocate=False)   # the reservation phase: same order, other rows
    check_order(m, ref, ix, case + " (reservation)")
    check_answers(m, ref, ix, case + " (reservation)", allocate=False)
    m.evaluate()
    decided, outputs = check_decision_keys(m, ref, ix, case)
    check_order(m, ref, ix, case + " (after evaluate_into)")
    m.evaluate()   # back on the engine's own outputs before the caller's tensors go away
    del outputs
    check_answers(m, ref, ix, case + " (second allocation pass)")
    return decided


@pytest.mark.parametrize("population,n", CASES, ids=lambda v: str(v))
def test_order_of_designed_population(monkeypatch, population, n):
    """One population at one size (the list of tests/test_order_inputs.py): 1, 63, 64, 65, 257, 1025, 2500, 4100 nodes — a 64-node
    word, a 256-thread block, the 1024-entry tile of k_rank_final, several tiles and several passes."""
    _, meta, ref = reference(population, n)
    m = manager(monkeypatch)
    try:
        decided = full_check(m, ref, f"{population} {n}")
        if population == "signs":   # the signed key of a negative score, through a decision
            assert (ref.scores[decided[decided >= 0]] < 0).any()
    finally:
        m.close()


@pytest.mark.parametrize("tune", ["run_decide=0", "walk_rows=1"])
def test_order_of_the_mixed_population_under_other_deciders(monkeypatch, tune):
    """Settings that change which kernel decides (the scan instead of the run-level decision; every request value walked): each
    against the oracle, not against another setting."""
    _, meta, ref = reference("mixed", 1025)
    m = manager(monkeypatch, tune)
    try:
        full_check(m, ref, f"mixed 1025 [{tune}]")
    finally:
        m.close()


# ---- order after node changes ----------------------------------------------------------------------------------------------
def _strip(node):
    return {k: v for k, v in node.items() if k != "pods"}


def _assume(snap, usage, uid, node):
    """The snapshot object after AssumePod(uid → node index): the ask joins the node's pods (as tests/test_gpu_parity.py _move)."""
    pod = next(p for p in snap["pods"] if p["metadata"]["uid"] == uid)
    name = snap["nodes"][node]["metadata"]["name"]
    snap["nodes"][node]["pods"].append(dict(pod, spec=dict(pod["spec"], nodeName=name)))
    snap["pods"] = [p for p in snap["pods"] if p["metadata"]["uid"] != uid]
    req = pod["spec"]["containers"][0]["resources"]["requests"]
    tc, tm, uc, um = usage[node]
    usage[node] = (tc, tm, uc + int(req["cpu"][:-1]), um + int(req["memory"]))
    return name


@pytest.mark.parametrize("topology", [False, True], ids=["resources", "zone-spread"])
def test_order_after_node_changes(monkeypatch, topology):
    """Mixed at 1025 nodes; after the full check, in order: an assume that moves a node exactly onto another node's score, an
    assume that moves a node across a bucket boundary, a node whose allocatable cpu turns 0, a node removed from inside the big tie
    group, a node added whose name sorts into the middle of that group. After each step evaluate_dirty(decisions=True), then
    scores, order, candidates of all asks and decisions against an oracle on the EDITED Python object; at the end a full evaluation
    and the same again. zone-spread: two asks carry a hard zone spread constraint on their own label and the assumed pods match
    its selector (the topology branch of the column patch)."""
    snap, meta, ref = reference("mixed", 1025, topology)
    snap = json.loads(json.dumps(snap))
    usage = list(meta["usage"])
    a, b, c = meta["pairs"]
    case = "mixed 1025 edited" + (" zone-spread" if topology else "")
    m = manager(monkeypatch)
    try:
        full_check(m, ref, case)
        idle = sorted(n["metadata"]["name"].encode() for n, u in zip(snap["nodes"], usage) if u == _ordergen.IDLE)
        pinned_to = next(p["spec"]["nodeName"] for p in snap["pods"] if p["metadata"]["uid"] == "pinned")
        gone = next(x.decode() for x in idle[len(idle) // 2:] if x.decode() != pinned_to)
        before = idle[len(idle) // 3]
        new_name = before.decode() + "-0"
        assert before < new_name.encode() < idle[len(idle) // 3 + 1]

        def eq_score():
            m.assume_pod("move-eq", _assume(snap, usage, "move-eq", a))
            assert _ordergen.score(usage[a]) == _ordergen.score(usage[b])

        def cross_bucket():
            was = _ordergen.bucket(_ordergen.score(usage[c]))
            m.assume_pod("move-bucket", _assume(snap, usage, "move-bucket", c))
            assert _ordergen.bucket(_ordergen.score(usage[c])) == was - 1

        def cpu_zero():
            z = usage.index(_ordergen.HALF)
            snap["nodes"][z]["status"]["allocatable"]["cpu"] = "0"
            usage[z] = (0,) + usage[z][1:]
            m.update_node(_strip(snap["nodes"][z]))

        def remove():
            z = next(i for i, n in enumerate(snap["nodes"]) if n["metadata"]["name"] == gone)
            assert not snap["nodes"][z]["pods"]
            del snap["nodes"][z], usage[z]
            m.remove_node(gone)

        def add():
            node = _ordergen.make_node(new_name, _ordergen.IDLE, pool="a", zone="z1")
            snap["nodes"].append(node)
            usage.append(_ordergen.IDLE)
            m.update_nodes_batch([_strip(node)])

        for step, edit in enumerate((eq_score, cross_bucket, cpu_zero, remove, add)):
            patches = m.counters()["node_patches"]
            edit()
            patched = m.evaluate_dirty(decisions=True)
            if step < 3:   # an assume and update_node of a known node patch columns: a quiet full evaluation would hide that path
                assert patched >= 1, f"{case}, step {step + 1} ({edit.__name__}): evaluate_dirty returned {patched}"
                assert m.counters()["node_patches"] > patches, f"{case}, step {step + 1} ({edit.__name__}): no column patch counted"
            now = Reference(snap, usage, reserve=False)
            ix = Indices(m, now)
            what = f"{case}, step {step + 1} ({edit.__name__}, {patched} columns)"
            check_order(m, now, ix, what)
            check_answers(m, now, ix, what)
        position = now.order.tolist().index(len(usage) - 1)
        assert now.scores[now.order[position - 1]] == now.scores[now.order[position + 1]] == 1.0   # inside the tie group
        m.evaluate()
        ix = Indices(m, now)
        check_order(m, now, ix, case + ", full evaluation at the end")
        check_answers(m, now, ix, case + ", full evaluation at the end")
        layout_line(case + ", at the end", m)
    finally:
        m.close()


# ---- rounds on tie-heavy clusters ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sequential", "batched"])
@pytest.mark.parametrize("cluster", ["key-ties", "signs-and-zeros"])
def test_round_on_tie_heavy_cluster(request, cluster, form):
    """(key-ties) totals 1024 / 1024, asks of 1, 2 and 4 units: assumes keep landing moved nodes exactly on the keys of unmoved
    ones — the winner is the smaller (key, NodeID rank) of a moved and an unmoved candidate, dozens of times on a shared key
    (tests/test_order_inputs.py replays it and counts them). (signs-and-zeros) overcommitted and zero-allocatable nodes take pods during the round.
    Every decision and the state left behind against the oracle's sequential loop — on the snapshot text itself too."""
    snap, meta = (_ordergen.round_ties if cluster == "key-ties" else _ordergen.round_signs)(ROUND_SEED)
    text = json.dumps(snap)
    want = orc.Oracle(text).allocate_sequential()
    m = request.getfixturevalue("pm" if form == "sequential" else "pm_batched")   # only the engine this case uses is opened
    before = m.round_info()
    got = round_against_oracle(m, text)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{len(bad)} decisions differ from the oracle on the snapshot text, first at ask {bad[0]}: gpu={got[bad[0]]} oracle={want[bad[0]]}"
    info = m.round_info()   # fewer than 512 asks: the default manager decides them in the sequential kernel
    assert info["rounds_batched"] - before["rounds_batched"] == (form == "batched")
    assert info["rounds_sequential"] - before["rounds_sequential"] == (form == "sequential")
    print(f"ORDER-ROUND {cluster} {form}: {len(got)} asks, {(got >= 0).sum()} placed on {len(set(got[got >= 0].tolist()))} nodes")
