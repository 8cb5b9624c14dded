"""The designed PreemptionPredicates populations of tests/_preemptgen.py held to their claims, and their model held to the oracle
— on the CPU. tests/test_gpu_preemption.py relies on every property asserted here: a population in which most answers were -1, or
a batch whose neighbours all agreed, would let a wrong kernel pass."""
import collections
import functools
import json

import numpy as np
import pytest

import _oracle as orc
import _preemptgen

SEED = 20261
POPULATIONS = tuple(_preemptgen.POPULATIONS)
TOPOLOGY = ("PodTopologySpread", "InterPodAffinity")
# plugin lists by name: (PreFilter list, Filter list); the last two are the Filter-without-PreFilter forms
LISTS = {"default": (("*",), ("*",)), "fit": (("NodeResourcesFit",),) * 2, "fit+ports": (("NodeResourcesFit", "NodePorts"),) * 2,
         "spread": (TOPOLOGY[:1], TOPOLOGY[:1]), "interpod": (TOPOLOGY[1:], TOPOLOGY[1:]), "spread-filter-only": ((), TOPOLOGY[:1]),
         "interpod-filter-only": ((), TOPOLOGY[1:])}
FORMS = ("default", "fit", "fit+ports")
TOPOLOGY_FORMS = ("spread", "interpod", "spread-filter-only", "interpod-filter-only")


def masks(form):
    pre, filt = (set(_preemptgen.PLUGINS) if "*" in names else set(names) for names in LISTS[form])
    return orc.mask_of(pre), orc.mask_of(filt), orc.mask_of(pre & set(_preemptgen.FROZEN)), orc.mask_of(filt & set(_preemptgen.FROZEN))


class Case:
    """One population: the snapshot, the JSON text both sides load, its queries, and the two references per plugin list."""

    def __init__(self, name=None, snapshot=None, queries=None, meta=None):
        if snapshot is None:
            snapshot, queries, meta = _preemptgen.POPULATIONS[name](SEED)
        self.name, self.snapshot, self.queries, self.meta = name, snapshot, queries, meta
        self.text = json.dumps(snapshot)
        self.oracle = orc.Oracle(self.text)
        self.model = _preemptgen.Model(snapshot)
        self.ask_at = {p["metadata"]["uid"]: i for i, p in enumerate(snapshot["pods"])}
        self.node_at = {n["metadata"]["name"]: i for i, n in enumerate(snapshot["nodes"])}
        self.pods_of = {n["metadata"]["name"]: [p["metadata"]["uid"] for p in n["pods"]] for n in snapshot["nodes"]}
        self._answers = {}

    def victim_indices(self, node, victims):
        """What the oracle takes: positions in the node's pod list; -1 for a nil victim and for everything removePodFromNodeNoFail
        ignores — the pod of another node, a uid nobody has, a uid named before."""
        on_node, seen, out = self.pods_of[node], set(), []
        for v in victims:
            out.append(on_node.index(v) if v in on_node and v not in seen else -1)
            seen.add(v)
        return out

    def answers(self, form="default", queries=None):
        """→ (oracle's answers, model's answers) for the population's queries (cached) or the ones given."""
        if queries is None and form in self._answers:
            return self._answers[form]
        pre, filt, frozen_pre, frozen_filt = masks(form)
        frozen = self.oracle.eval_grid(pre_mask=frozen_pre, filt_mask=frozen_filt)
        by_oracle, by_model = [], []
        for q in self.queries if queries is None else queries:
            uid, node, victims, start = q
            a, n = self.ask_at[uid], self.node_at[node]
            by_oracle.append(self.oracle.preemption(a, n, self.victim_indices(node, victims), start, pre, filt))
            by_model.append(self.model.answer(q, bool(frozen[a, n]), LISTS[form]))
        out = (np.array(by_oracle, dtype=np.int32), np.array(by_model, dtype=np.int32))
        if queries is None:
            self._answers[form] = out
        return out


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def histogram(values, most=16):
    """Answer -> number of queries; beyond `most` different answers the ones from 2 on are summed up under one key."""
    h = dict(sorted(collections.Counter(int(v) for v in values).items()))
    if len(h) <= most:
        return h
    rest = {k: v for k, v in h.items() if k > 1}
    out = {k: v for k, v in h.items() if k <= 1}
    out[f"{min(rest)}..{max(rest)}"] = f"{sum(rest.values())} queries, {len(rest)} different answers"
    return out


@pytest.mark.parametrize("form", FORMS + TOPOLOGY_FORMS)
@pytest.mark.parametrize("name", POPULATIONS)
def test_model_equals_oracle(name, form):
    """Every query of every population under every plugin list the GPU tests use."""
    c = case(name)
    by_oracle, by_model = c.answers(form)
    bad = np.flatnonzero(by_oracle != by_model)
    assert bad.size == 0, f"{name} [{form}]: {len(bad)} answers differ, first {c.queries[bad[0]][:2]} ({c.meta['rule'][bad[0]]}): oracle {by_oracle[bad[0]]} model {by_model[bad[0]]}"


@pytest.mark.parametrize("name", POPULATIONS)
def test_generator_meets_its_intentions(name):
    """Under the full plugin list the oracle answers what the generator meant; every rule name is met; the answers the population
    claims occur; fewer than half are -1 (`incurable` excepted: there half of them must be)."""
    c = case(name)
    by_oracle, _ = c.answers()
    intended = np.array(c.meta["intended"])
    bad = np.flatnonzero(by_oracle != intended)
    assert bad.size == 0, f"{name}: {len(bad)} answers are not the intended ones, first {c.queries[bad[0]][:2]} ({c.meta['rule'][bad[0]]}): {by_oracle[bad[0]]} intended {intended[bad[0]]}"
    assert set(c.meta["rule"]) == set(c.meta["rules"]) and len(c.meta["rules"]) >= 3
    for v in by_oracle:
        assert -1 <= v < max(len(q[2]) for q in c.queries)
    missing = [a for a in c.meta["claims"] if a not in set(by_oracle.tolist())]
    assert not missing, f"{name}: claimed answers that never occur: {missing}"
    share = float((by_oracle == -1).mean())
    print(f"PREEMPT-POPULATION {name}: {len(c.snapshot['nodes'])} nodes, {sum(len(p) for p in c.pods_of.values())} residents, {len(c.snapshot['pods'])} asks, "
          f"{len(c.queries)} queries, share of -1 {share:.3f}, answers {histogram(by_oracle)}")
    if name == "incurable":
        assert share == 0.5
    else:
        assert share < 0.5, f"{name}: {share:.2f} of the expected answers are -1"


def test_resource_edges_triples():
    """The three asks of a (node, dimension, k) triple — S_k - 1, S_k, S_k + 1 — get three different answers for every k >= 1. At
    k = 0 no correct answer can tell S_0 - 1 from S_0: for a non-empty list and start 0 every request up to S_0 is answered with 0.
    There the triple gets two answers, (0, 0, 1) — or (0, 0, -1) for a list of one."""
    c = case("resource_edges")
    by_oracle, _ = c.answers()
    triples = collections.defaultdict(dict)
    for q, d in enumerate(c.meta["detail"]):
        if "delta" in d:
            triples[(c.queries[q][1], d["dim"], d["k"])][d["delta"]] = (int(by_oracle[q]), d)
    assert len(triples) == 8 * (4 * (1 + 2 + 3) + 3)
    seen = set()
    for (node, dim, k), t in triples.items():
        got = [t[delta][0] for delta in (-1, 0, 1)]
        length = t[0][1]["length"]
        assert got[1] == k and got[2] == (k + 1 if k + 1 < length else -1), (node, dim, k, got)
        assert got[0] == (k - 1 if k else 0) and len(set(got)) == (3 if k else 2), (node, dim, k, got)
        seen.add((dim, t[0][1]["magnitude"], length))
    # every dimension under every magnitude, the last of the eight included, and every dimension with the list of 300
    assert {(d, m) for d, m, _ in seen} == {(d, m) for d in _preemptgen.DIMS for m in _preemptgen.MAGNITUDES}
    assert {d for d, _, length in seen if length == 300} == set(_preemptgen.DIMS)
    # the sums the asks request lie on both sides of 2^53 and reach 2^63 - 1
    requested = [v for p in c.snapshot["pods"] for v in _preemptgen._requests(p).values()]
    assert max(requested) == _preemptgen.I64_MAX and {_preemptgen.P53 - 1, _preemptgen.P53, _preemptgen.P53 + 1} <= set(requested)


def test_slot_edges_count_only_victims_that_leave():
    """Every pattern symbol occurs in lists that get an index, and the nodes are at allowed - 1, allowed and allowed + 1."""
    c = case("slot_edges")
    by_oracle, _ = c.answers()
    for n in c.snapshot["nodes"][1:]:
        allowed, need = (int(x) for x in n["metadata"]["name"].split("-")[1:])
        assert len(n["pods"]) == allowed - 1 + need and int(n["status"]["allocatable"]["pods"]) == allowed
    for symbol in "PNFUR":
        assert any(symbol in d["pattern"] and by_oracle[q] > 0 for q, d in enumerate(c.meta["detail"])), symbol
    foreign = set(c.pods_of["elsewhere"])
    assert any(foreign & set(q[2]) for q in c.queries) and any(None in q[2] for q in c.queries)
    assert any(len(q[2]) != len(set(q[2])) and None not in q[2] for q in c.queries), "no list names a uid twice"


def test_start_rules_cover_every_start():
    c = case("start_rules")
    by_oracle, _ = c.answers()
    for cause in ("cpu", "slot", "port"):
        got = {c.queries[q][3]: int(by_oracle[q]) for q, d in enumerate(c.meta["detail"]) if d.get("cause") == cause}
        assert got == {0: 3, 1: 3, 2: 3, 3: 3, 4: 4, 5: 5, 6: -1, 7: -1, 8: -1}, (cause, got)


def test_incurable_siblings():
    """Each incurable ask is -1, its sibling — one attribute apart, same node, same victims, same start — gets an index."""
    c = case("incurable")
    by_oracle, _ = c.answers()
    at = {q[0]: i for i, q in enumerate(c.queries)}
    bad = [q for q in range(len(c.queries)) if not c.meta["rule"][q].startswith("sibling")]
    assert len(bad) == len(c.queries) // 2
    for q in bad:
        s = at[c.meta["detail"][q]["sibling"]]
        assert by_oracle[q] == -1 and by_oracle[s] >= 0 and c.queries[q][1:] == c.queries[s][1:], c.queries[q][:2]
    # and it is the frozen plugins that say no: with NodeResourcesFit and NodePorts alone the incurable asks get their sibling's index
    fit_only, _ = c.answers("fit+ports")
    assert all(fit_only[q] == by_oracle[at[c.meta["detail"][q]["sibling"]]] for q in bad)


def test_ports_population_designs():
    c = case("ports")
    by_oracle, _ = c.answers()
    wanted = {t for p in c.snapshot["pods"] for t in _preemptgen._host_ports(p)}
    assert len(wanted) == c.meta["dictionary_ports"] > 64, "the wanted ports must need two dictionary words"
    # the identical-triple node: two residents hold the same (ip, protocol, port), and a list that names one of them gets its position
    rule = c.meta["identical_triple"]
    qs = [q for q in range(len(c.queries)) if c.meta["rule"][q] == rule]
    node = next(n for n in c.snapshot["nodes"] if n["metadata"]["name"] == c.queries[qs[0]][1])
    held = [tuple(_preemptgen._host_ports(p)) for p in node["pods"]]
    assert max(collections.Counter(held).values()) == 2
    holders = [p["metadata"]["uid"] for p, h in zip(node["pods"], held) if h == max(held, key=held.count)]
    assert any(by_oracle[q] >= 0 and len(set(holders) & set(c.queries[q][2][:by_oracle[q] + 1])) == 1 for q in qs), "no query frees the port with ONE removal"
    # without NodePorts every answer of the population that waits for a port comes earlier or stays
    fit_only, _ = c.answers("fit")
    assert (fit_only != by_oracle).sum() > len(c.queries) // 2


def test_topology_state_is_frozen():
    """The -1 answers of the population are the topology plugins' doing (NodeResourcesFit alone gives every query an index), and they
    stay -1 although the list names every pod the term or constraint counts."""
    c = case("topology_frozen")
    by_oracle, _ = c.answers()
    fit_only, _ = c.answers("fit")
    assert (fit_only >= 0).all() and (by_oracle == -1).sum() == 15
    victims = {"x0-r0", "x0-r2", "x0-r4"}
    for q in np.flatnonzero(by_oracle == -1):
        assert victims <= set(c.queries[q][2])
    assert c.meta["shards"] == ([n["metadata"]["name"] for n in c.snapshot["nodes"][:2]], [n["metadata"]["name"] for n in c.snapshot["nodes"][2:]])
    for form, dead in (("spread-filter-only", "PodTopologySpread"), ("interpod-filter-only", "InterPodAffinity")):
        assert (c.answers(form)[0] == -1).all(), dead


def test_batch_geometry():
    """Neighbours never share both answer and victim count; victim counts cycle 0, 1, 300, 2; inside a block of 64 the queries with
    300 victims get pairwise different answers; no query index is the index of its ask or of its node."""
    c = case("batch_geometry")
    by_oracle, _ = c.answers()
    counts = [len(q[2]) for q in c.queries]
    assert len(c.queries) == max(c.meta["counts"]) == 1001 and counts[:8] == [0, 1, 300, 2, 0, 1, 300, 2]
    assert all(counts[q] == _preemptgen.VICTIM_CYCLE[q % 4] for q in range(len(counts)))
    for q in range(1, len(counts)):
        assert (by_oracle[q], counts[q]) != (by_oracle[q - 1], counts[q - 1]), q
    for block in range(0, len(counts), 64):
        long = [int(by_oracle[q]) for q in range(block, min(block + 64, len(counts))) if counts[q] == 300]
        assert len(set(long)) == len(long) and min(long) >= 0, block
        if len(long) == 16:
            assert {0, 299} <= set(long)
            short = {(counts[q], int(by_oracle[q])) for q in range(block, block + 64) if counts[q] < 300}
            assert short == {(0, -1), (1, 0), (1, -1), (2, 0), (2, 1), (2, -1)}
    for q, (uid, node, _, _) in enumerate(c.queries):
        assert c.ask_at[uid] != q and c.node_at[node] != q % len(c.node_at), q
    for n in c.meta["counts"]:   # every batch length the GPU test launches is a prefix with fewer than half -1
        assert (by_oracle[:n] == -1).mean() < 0.5 or n == 1
