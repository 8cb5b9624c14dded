"""The designed preemption-reach populations of tests/_reachgen.py held to their claims, and their model held to the oracle — on the
CPU. The reference has no call that returns a level: it is pinned through PreemptionPredicates by the identity of DESIGN.md §4.16 —
with victims = the node's pods of tiers < limit in ascending tier order, level = tier(victims[i]) + 1 for i = PreemptionPredicates(ask,
node, victims, 0), i == -1 <=> never, and level 0 <=> Predicates fits. tests/test_gpu_preempt_reach.py relies on every property
asserted here: a population in which most pairs were never, or whose neighbouring asks all agreed, would let a wrong kernel pass."""
import functools
import json

import numpy as np
import pytest

import _oracle as orc
import _preemptgen
import _reachgen
from _reachgen import NEVER

SEED = 20263
POPULATIONS = tuple(_reachgen.POPULATIONS)
FORMS = {"default": ("*",), "no-ports": tuple(p for p in _preemptgen.PLUGINS if p != "NodePorts"),
         "no-topology": tuple(p for p in _preemptgen.PLUGINS if p not in ("PodTopologySpread", "InterPodAffinity"))}


def masks(form):
    names = set(_preemptgen.PLUGINS) if "*" in FORMS[form] else set(FORMS[form])
    return orc.mask_of(names), orc.mask_of(names & set(_preemptgen.FROZEN))


class Case:
    """One population: the snapshot, the JSON text both sides load, and per plugin list the levels by the oracle and by the model."""

    def __init__(self, name=None, snapshot=None, bounds=None, meta=None):
        if snapshot is None:
            snapshot, bounds, meta = _reachgen.population(name, SEED)
        self.name, self.snapshot, self.bounds, self.meta = name, snapshot, bounds, meta
        self.text = json.dumps(snapshot)
        self.oracle = orc.Oracle(self.text)
        self.model = _reachgen.ReachModel(snapshot, bounds)
        self.asks = [p["metadata"]["uid"] for p in snapshot["pods"]]
        self.nodes = [n["metadata"]["name"] for n in snapshot["nodes"]]
        self.tiers = [[self.model.tier(p) for p in n["pods"]] for n in snapshot["nodes"]]
        self.limits = [self.model.asks[uid][2] for uid in self.asks]
        self._levels = {}

    def victims(self, n, limit):
        """Positions in the node's pod list of its pods of tiers < limit, in ascending tier order (any order inside a tier)."""
        return sorted((i for i, t in enumerate(self.tiers[n]) if 0 <= t < limit), key=lambda i: self.tiers[n][i])

    def levels(self, form="default"):
        """→ (by the oracle through the identity, by the model), each int32[asks][nodes], NEVER = -1."""
        if form in self._levels:
            return self._levels[form]
        mask, frozen_mask = masks(form)
        fits = self.oracle.eval_grid(pre_mask=mask, filt_mask=mask)
        frozen = self.oracle.eval_grid(pre_mask=frozen_mask, filt_mask=frozen_mask)
        by_oracle = np.zeros((len(self.asks), len(self.nodes)), dtype=np.int32)
        by_model = np.zeros_like(by_oracle)
        for a, uid in enumerate(self.asks):
            for n, node in enumerate(self.nodes):
                by_model[a, n] = self.model.level(uid, node, bool(frozen[a, n]), FORMS[form])
                if fits[a, n]:
                    continue
                victims = self.victims(n, self.limits[a])
                i = self.oracle.preemption(a, n, victims, 0, mask, mask)
                by_oracle[a, n] = NEVER if i < 0 else self.tiers[n][victims[i]] + 1
        self._levels[form] = (by_oracle, by_model)
        return self._levels[form]

    def cells(self, form="default"):
        levels = self.levels(form)[0]
        out = []
        for a in range(len(self.asks)):
            victims = [self.model.victims_below(node, int(lv)) if lv >= 1 else 0 for node, lv in zip(self.nodes, levels[a])]
            out.append(_reachgen.cells([int(x) for x in levels[a]], victims, self.limits[a]))
        return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.parametrize("name", POPULATIONS)
@pytest.mark.parametrize("form", tuple(FORMS))
def test_model_agrees_with_the_oracle(name, form):
    by_oracle, by_model = case(name).levels(form)
    bad = np.argwhere(by_oracle != by_model)
    assert len(bad) == 0, [(case(name).asks[a], case(name).nodes[n], int(by_oracle[a, n]), int(by_model[a, n])) for a, n in bad[:8]]


@pytest.mark.parametrize("name", POPULATIONS)
def test_designed_pairs_land_on_their_level(name):
    c = case(name)
    by_oracle, _ = c.levels()
    ask_at = {uid: i for i, uid in enumerate(c.asks)}
    node_at = {n: i for i, n in enumerate(c.nodes)}
    assert len(c.meta["intended"]) >= 10
    wrong = {k: (want, int(by_oracle[ask_at[k[0]], node_at[k[1]]])) for k, want in c.meta["intended"].items()
             if by_oracle[ask_at[k[0]], node_at[k[1]]] != want}
    assert not wrong, (c.meta["rule"][next(iter(wrong))], wrong)


@pytest.mark.parametrize("name", POPULATIONS)
def test_population_conditions(name):
    """Every level 0..T and never occurs; fewer than half of the pairs are never; no two neighbouring asks share all 16 cells."""
    c = case(name)
    by_oracle, _ = c.levels()
    T = len(c.bounds)
    assert T == c.meta["T"] and T in (1, 3, 8)
    assert set(np.unique(by_oracle).tolist()) == set(range(-1, T + 1))
    assert (by_oracle == NEVER).sum() * 2 < by_oracle.size, float((by_oracle == NEVER).mean())
    cells = c.cells()
    same = [(c.asks[i], c.asks[i + 1]) for i in range(len(cells) - 1) if np.array_equal(cells[i], cells[i + 1])]
    assert not same, same
    assert (cells[:, :10].sum(axis=1) == len(c.nodes)).all()


def test_the_tier_counts_cover_one_three_and_eight():
    assert {T for _, T in _reachgen.POPULATIONS.values()} == {1, 3, 8}


def test_best_node_scene():
    """Equal (level, victim pods) goes to the lower index; fewer pods beat an equal level; a lower level beats fewer pods."""
    c = case("best_ties")
    cells = c.cells()
    for uid, names in c.meta["best"].items():
        row = cells[c.asks.index(uid)]
        assert row[13] == min(c.nodes.index(n) for n in names), (uid, row.tolist())
    tie = cells[c.asks.index("a-bt-tie")]
    assert (tie[12], tie[14]) == (2, 3)
    assert tuple(cells[c.asks.index("a-bt-pods")][[12, 14]]) == (2, 2)
    assert tuple(cells[c.asks.index("a-bt-level")][[12, 14]]) == (1, 5)


def test_limit_siblings():
    """The same node at level 3 for an ask of limit 3, never for its sibling of limit 2; preemptionPolicy: Never is limit 0."""
    c = case("limits")
    by_oracle, _ = c.levels()
    li = c.nodes.index("li")
    assert by_oracle[c.asks.index("a-li-3-3"), li] == 3 and by_oracle[c.asks.index("a-li-3-2"), li] == NEVER
    assert c.limits[c.asks.index("a-li-3-policy")] == 0 and by_oracle[c.asks.index("a-li-3-policy"), li] == NEVER


def test_resource_boundaries_reach_the_large_magnitudes():
    c = case("resource_boundaries_8")
    requests = [q for uid in c.asks for q in c.model.asks[uid][0].values()]
    assert any(q > (1 << 62) for q in requests) and any((1 << 53) - 64 < q < (1 << 53) + 64 for q in requests)
    for alloc, _, _ in c.model.nodes.values():
        assert all(0 <= v <= _preemptgen.I64_MAX for v in alloc.values())


@pytest.mark.parametrize("n_nodes", (1, 63, 64, 65, 257, 300))
def test_geometry_has_seventy_distinct_tasks(n_nodes):
    snapshot, bounds, _ = _reachgen.geometry(SEED, n_nodes)
    assert len(snapshot["nodes"]) == n_nodes and len(snapshot["pods"]) == 70
    model = _reachgen.ReachModel(snapshot, bounds)
    assert len({(tuple(sorted(model.asks[p["metadata"]["uid"]][0].items())), model.asks[p["metadata"]["uid"]][2]) for p in snapshot["pods"]}) == 70
