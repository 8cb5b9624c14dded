"""The designed clusters of tests/_ordergen.py are what they claim, and the bin-pack order is stated twice — on the CPU alone.

tests/test_gpu_order.py holds the device to a reference permutation, np.lexsort((name, score)). That only discriminates if
  * the score every node gets is right: the contract is restated here in plain Python floats (_ordergen.score) and held bit-equal
    to the oracle's C++ statement (Oracle.binpack_scores) on every node of every population at every size used;
  * the permutation is the oracle's order: the first feasible node of it is o.decide of every ask;
  * the inputs contain what the rank kernels special-case: a bucket with more than 1024 distinct keys, a bucket of more than two
    tiles, negative scores (one tied), 0.0 and 1.0, scores on and 2^-40 beside a bucket boundary, distinct integers that become
    one double, tie groups whose name order is not their index order.
Round cluster (i) is replayed in plain Python first: the replay equals o.allocate_sequential and shows the moved / unmoved key
ties the cluster was built for."""
import json

import numpy as np
import pytest

import _oracle as orc
import _ordergen

# (population, nodes): every size sits at an edge of the rank kernels — a 64-node word, a 256-thread block, the 1024-entry tile,
# several tiles and several passes. tests/test_gpu_order.py runs the same list.
CASES = [("ties", 1), ("ties", 1025), ("ties", 2500), ("dense", 2500), ("dense", 4100), ("edges", 65), ("edges", 257), ("signs", 63),
         ("signs", 257), ("int64", 64), ("mixed", 1025), ("mixed", 2500), ("mixed", 4100)]
SEED = 3


class Reference:
    """Scores (Python floats), the reference permutation and the oracle's grids of one snapshot object."""

    def __init__(self, snap, usage, reserve=True):
        self.text = json.dumps(snap)
        self.names = np.array([n["metadata"]["name"] for n in snap["nodes"]], dtype="S")
        self.uids = [p["metadata"]["uid"] for p in snap["pods"]]
        self.scores = np.array([_ordergen.score(u) for u in usage], dtype=np.float64)
        self.order = np.lexsort((self.names, self.scores)).astype(np.int32)
        o = orc.Oracle(self.text)
        self.oracle_scores = o.binpack_scores()
        self.grid = o.eval_grid(threads=4)
        self.reserve = o.eval_grid(pre_mask=orc.RESERVE_PRE, filt_mask=orc.RESERVE_FILT, threads=4) if reserve else None
        self.decide = [o.decide(p) for p in range(o.num_pods)]
        o.close()

    def candidates(self, p, k, grid=None):
        row = (self.grid if grid is None else grid)[p][self.order]
        return self.order[row > 0][:k]


_cache = {}


def reference(population, n, topology=False):
    key = (population, n, topology)
    if key not in _cache:
        snap, meta = _ordergen.cluster(population, SEED, n, topology)
        _cache[key] = (snap, meta, Reference(snap, meta["usage"]))
    return _cache[key]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("population,n", CASES)
def test_two_statements_of_the_score_and_of_the_order_agree(population, n):
    snap, meta, ref = reference(population, n)
    assert len(snap["nodes"]) == n and len(set(meta["names"])) == n and 30 <= len(snap["pods"]) <= 50
    bad = np.flatnonzero(bits(ref.scores) != bits(ref.oracle_scores))
    assert bad.size == 0, f"node {bad[0]} {meta['usage'][bad[0]]}: python {ref.scores[bad[0]]!r} oracle {ref.oracle_scores[bad[0]]!r}"
    assert sorted(ref.order.tolist()) == list(range(n))
    for p, (count, best) in enumerate(ref.decide):
        cand = ref.candidates(p, 1)
        assert count == int(ref.grid[p].sum()) and best == (int(cand[0]) if len(cand) else -1), ref.uids[p]
    # the asks are what they are meant to be
    at = {u: k for k, u in enumerate(ref.uids)}
    assert ref.grid[at["fits-all"]].all() and not ref.grid[at["nowhere"]].any() and ref.grid[at["pinned"]].sum() <= 1
    if n >= 63:
        counts = ref.grid.sum(axis=1)
        assert len(set(counts.tolist())) >= 12, "the asks cut the nodes in too few ways"
        assert ref.grid[at["pinned"]].sum() == 1
        for pool in "abc":
            assert 0 < counts[at[f"pool-{pool}"]] < n
        assert counts[at["pool-a"]] > counts[at["pool-b"]] > counts[at["pool-c"]] or n < 200
        assert 0 < counts[at["ded-0"]] < n   # the toleration-gated group has nodes on every population ...
        assert counts[at["ded-untolerated"]] == 0 and counts[at["pool-a-tol"]] > 0   # ... and is gated by the toleration
        assert (ref.reserve.sum(axis=1) >= counts).all() and (ref.reserve.sum(axis=1) > counts).any()


def test_first_k_of_the_order_equal_repeated_decisions():
    """120 sampled (ask, k) pairs: the first k feasible nodes of the reference order are what repeating o.decide gives when the
    earlier winners are taken out of the cluster. 100 pairs on the clusters of up to 257 nodes with k in 2..6; 20 on mixed, ties
    and dense at 1025 to 2500 nodes with k up to 12: deeper into the big tie group and the dense bucket."""
    import random
    rng = random.Random(9)
    small = [(population, n) for population, n in CASES if 63 <= n <= 257]
    large = {("mixed", 1025): 12, ("ties", 1025): 4, ("dense", 2500): 4}
    assert len(small) == 5 and set(large) <= set(CASES)
    pairs = 0
    for population, n in small + list(large):
        snap, meta, ref = reference(population, n)
        for _ in range(large.get((population, n), 20)):
            p, k = rng.randrange(len(ref.uids)), rng.randint(2, 6 if n <= 257 else 12)
            left, winners = list(snap["nodes"]), []
            for _ in range(k):
                o = orc.Oracle({"nodes": left, "pods": snap["pods"]})
                best = o.decide(p)[1]
                o.close()
                if best < 0:
                    break
                winners.append(left.pop(best)["metadata"]["name"].encode())
            assert winners == ref.names[ref.candidates(p, k)].tolist(), (population, n, ref.uids[p], k)
            pairs += 1
    assert pairs == 120


def tie_groups(ref):
    groups = {}
    for i, b in enumerate(bits(ref.scores).tolist()):
        groups.setdefault(b, []).append(i)
    return [g for g in groups.values() if len(g) > 1]


def inverted_share(ref):
    """Of the pairs of nodes adjacent (by index) inside a tie group: how many does the name order invert?"""
    pairs = inverted = 0
    for g in tie_groups(ref):
        for a, b in zip(g, g[1:]):
            pairs += 1
            inverted += ref.names[a] > ref.names[b]
    return pairs, inverted


def by_bucket(ref):
    members, keys = {}, {}
    for s in ref.scores.tolist():
        b = _ordergen.bucket(s)
        members[b] = members.get(b, 0) + 1
        keys.setdefault(b, set()).add(s)
    return members, {b: len(v) for b, v in keys.items()}


@pytest.mark.parametrize("n", [1025, 2500])
def test_ties_population(n):
    _, meta, ref = reference("ties", n)
    members, keys = by_bucket(ref)
    assert (ref.scores == 1.0).sum() >= n * 8 // 10 and (ref.scores == 0.5).sum() >= n // 20
    assert members[1023] == (ref.scores == 1.0).sum() and keys[1023] == 1
    if n >= 2500:
        assert members[1023] >= 2049   # more than two tiles of one key
    pairs, inverted = inverted_share(ref)
    assert pairs >= n * 8 // 10 and 2 * inverted >= pairs, (pairs, inverted)
    order_of_names = np.argsort(ref.names)
    assert not np.array_equal(order_of_names, np.arange(n)) and not np.array_equal(order_of_names, np.arange(n)[::-1])


@pytest.mark.parametrize("n", [2500, 4100])
def test_dense_bucket_population(n):
    _, meta, ref = reference("dense", n)
    members, keys = by_bucket(ref)
    assert keys[511] >= 1100 and members[511] == keys[511]          # pairwise distinct keys, all in one bucket
    assert members[1023] >= 1025 and keys[1023] == 1                   # the clamped last bucket is multi-tile too
    if n >= 4100:
        assert keys[511] >= 2049 and members[1023] >= 2049           # more than two tiles: of distinct keys, and of one key
    in_bucket = np.flatnonzero((ref.scores < 0.5) & (ref.scores > 0.499))
    assert len(in_bucket) == keys[511]
    want = [0.5 - (meta["usage"][i][2] - (1 << 29)) / (1 << 30) for i in in_bucket]
    assert ref.scores[in_bucket].tolist() == want                     # 0.5 - i / 2^30, exactly


@pytest.mark.parametrize("n", [65, 257])
def test_bucket_edges_population(n):
    _, meta, ref = reference("edges", n)
    x = ref.scores * 1024.0
    on = np.flatnonzero(x == np.floor(x))
    assert len(on) >= n // 3 and 0.0 in ref.scores and 1.0 in ref.scores
    below = above = 0
    for s in ref.scores.tolist():
        nearest = round(s * 1024.0) / 1024.0
        if 0 < abs(s - nearest) <= 2.0 ** -39:
            below += s < nearest
            above += s > nearest
            assert _ordergen.bucket(s) == int(nearest * 1024) - (s < nearest)   # the two sides land in different buckets
    assert below >= 5 and above >= 5


@pytest.mark.parametrize("n", [63, 257])
def test_signs_and_zeros_population(n):
    _, meta, ref = reference("signs", n)
    neg = ref.scores[ref.scores < 0]
    assert len(set(neg.tolist())) >= 3 and len(neg) > len(set(neg.tolist())), neg
    assert (ref.scores == 0.0).sum() >= 2 and (ref.scores == 1.0).sum() >= 2 and not np.signbit(ref.scores[ref.scores == 0.0]).any()
    usage = meta["usage"]
    cpu0 = [i for i, u in enumerate(usage) if u[0] == 0 and u[1] > 0]
    mem0 = [i for i, u in enumerate(usage) if u[1] == 0 and u[0] > 0]
    both0 = [i for i, u in enumerate(usage) if u[0] == 0 and u[1] == 0]
    assert len(cpu0) >= 2 and len(mem0) >= 2 and len(both0) >= 2
    assert all(ref.scores[i] == 1.0 - (1.0 - float(usage[i][1] - usage[i][3]) / float(usage[i][1])) for i in cpu0)   # memory alone
    assert all(ref.scores[i] == 0.75 for i in mem0) and all(ref.scores[i] == 1.0 for i in both0)
    assert any(u[2] > u[0] > 0 and u[3] == 0 for u in usage)   # one dimension overcommitted, the other idle
    # the most overcommitted node wins every ask that fits everywhere: a decided node with a negative score
    at = ref.uids.index("fits-all")
    assert ref.scores[ref.decide[at][1]] == ref.scores.min() < 0
    # a negative tie on different integer usage
    assert any(len({usage[i] for i in g}) > 1 and ref.scores[g[0]] < 0 for g in tie_groups(ref))


def test_int64_population():
    _, meta, ref = reference("int64", 64)
    usage = meta["usage"]
    assert {u[1] for u in usage} >= {1 << 62, (1 << 63) - 1} and {u[3] for u in usage} >= {(1 << 53) - 1, 1 << 53, (1 << 53) + 1}
    mixed_groups = [g for g in tie_groups(ref) if len({usage[i] for i in g}) > 1]
    assert len(mixed_groups) >= 3, "distinct integers that become one double must tie"
    pairs, inverted = inverted_share(ref)
    assert pairs >= 20 and 2 * inverted >= pairs, (pairs, inverted)


@pytest.mark.parametrize("n", [1025, 2500, 4100])
def test_mixed_population(n):
    _, meta, ref = reference("mixed", n)
    usage = set(meta["usage"])
    assert usage >= set(_ordergen.SIGNS) and usage >= set(_ordergen.PAIRS) and _ordergen.IDLE in usage and _ordergen.HALF in usage
    members, keys = by_bucket(ref)
    assert keys[511] >= (1025 if n >= 2500 else 200) and (ref.scores < 0).sum() >= 6 and max(members.values()) >= n // 4
    assert any(u[1] == (1 << 63) - 1 for u in usage) and any(u[0] == 1 << 40 for u in usage)
    pairs, inverted = inverted_share(ref)
    assert 2 * inverted >= pairs, (pairs, inverted)
    # the designed pairs of the node-change sequence
    a, b, c = meta["pairs"]
    eq, bk = _ordergen.MOVE_EQ, _ordergen.MOVE_BUCKET
    moved = tuple(v + d for v, d in zip(meta["usage"][a], (0, 0, eq, eq)))
    assert ref.scores[a] != ref.scores[b] and _ordergen.score(moved) == ref.scores[b]
    moved = tuple(v + d for v, d in zip(meta["usage"][c], (0, 0, bk, bk)))
    assert _ordergen.bucket(_ordergen.score(moved)) == _ordergen.bucket(ref.scores[c]) - 1
    at = {u: k for k, u in enumerate(ref.uids)}
    assert ref.grid[at["move-eq"], a] and ref.grid[at["move-bucket"], c]


def test_some_population_has_each_property_the_rank_kernels_special_case():
    """The list of the issue, each on the population that claims it (asserted there in detail): here only that none is lost."""
    seen = set()
    for population, n in CASES:
        _, meta, ref = reference(population, n)
        members, keys = by_bucket(ref)
        if max(keys.values()) >= 1025:
            seen.add("1025 distinct keys in one bucket")
        if max(members.values()) >= 2049:
            seen.add("2049 members in one bucket")
        if any(len({meta["usage"][i] for i in g}) > 1 for g in tie_groups(ref)):
            seen.add("different integers, one score")
        seen.add(f"{n} nodes")
    assert seen >= {"1025 distinct keys in one bucket", "2049 members in one bucket", "different integers, one score"}
    assert seen >= {f"{n} nodes" for n in (1, 63, 64, 65, 257, 1025, 2500, 4100)}
    assert {p for p, n in CASES if n >= 2500} >= {"dense", "ties", "mixed"}


def test_generators_are_deterministic_per_seed():
    for population, n in [("ties", 65), ("edges", 65), ("signs", 63), ("int64", 64), ("mixed", 300), ("dense", 2200)]:
        a = json.dumps(_ordergen.cluster(population, 5, n)[0], sort_keys=True)
        assert a == json.dumps(_ordergen.cluster(population, 5, n)[0], sort_keys=True)
        if population in ("ties", "signs", "mixed", "dense"):
            assert a != json.dumps(_ordergen.cluster(population, 6, n)[0], sort_keys=True)
    assert json.dumps(_ordergen.cluster("mixed", 5, 300, topology=True)[0]) == json.dumps(_ordergen.cluster("mixed", 5, 300, topology=True)[0])
    for fn in (_ordergen.round_ties, _ordergen.round_signs):
        assert json.dumps(fn(2)[0]) == json.dumps(fn(2)[0]) and json.dumps(fn(2)[0]) != json.dumps(fn(3)[0])
    names = _ordergen.node_names(300)
    assert len(set(names)) == 300 and {"node-9", "node-10", "n1", "n10", "n1-a"} <= set(names) and all(x.isascii() for x in names)


ROUND_SEED = 1


def test_round_cluster_of_key_ties_replayed_in_python():
    """Round cluster (i): the plain Python replay equals the oracle's sequential loop, and it shows what the cluster is for — at
    least 20 steps whose minimal key is shared by a moved and an unmoved feasible node, the name deciding each way 5 times."""
    snap, meta = _ordergen.round_ties(ROUND_SEED)
    assert 200 <= len(snap["nodes"]) <= 400 and 300 <= len(snap["pods"]) <= 600
    got, shared, moved_won, unmoved_won = _ordergen.replay_round(meta)
    o = orc.Oracle(json.dumps(snap))
    assert np.array_equal(o.binpack_scores().view(np.uint64), bits([_ordergen.score(u) for u in meta["usage"]]))
    want = o.allocate_sequential()
    assert got == want.tolist()
    assert shared >= 20 and moved_won >= 5 and unmoved_won >= 5, (shared, moved_won, unmoved_won)
    assert -1 in got and len(set(got)) > 100 and len(got) < 512   # nodes fill up and leave; below 512 asks the default manager runs the sequential kernel


def test_round_cluster_of_signs_and_zeros_on_the_oracle():
    """Round cluster (ii): overcommitted and zero-allocatable nodes take pods during the round."""
    snap, meta = _ordergen.round_signs(ROUND_SEED)
    assert 200 <= len(snap["nodes"]) <= 400 and 300 <= len(snap["pods"]) <= 600
    o = orc.Oracle(json.dumps(snap))
    scores = o.binpack_scores()
    assert np.array_equal(scores.view(np.uint64), bits([_ordergen.score(u) for u in meta["usage"]]))
    want = o.allocate_sequential()
    assert len(want) < 512
    took = set(want[want >= 0].tolist())
    usage = meta["usage"]
    assert any(scores[i] < 0 for i in took) and any(usage[i][0] == 0 for i in took) and any(usage[i][1] == 0 for i in took)
    assert want[0] == int(np.lexsort((np.array(meta["names"], dtype="S"), scores))[0]) and scores[want[0]] < 0
