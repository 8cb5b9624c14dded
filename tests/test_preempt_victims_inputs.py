"""The designed preemption-victim populations of tests/_victimgen.py held to their claims, and their model held to the oracle — on the
CPU. need(ask, node) is pinned through the reference's two calls: 0 <=> Predicates fits; otherwise need - 1 == PreemptionPredicates(ask,
node, order(node) cut at the ask's limit, 0), and -1 <=> that call returns -1. tests/test_gpu_preempt_victims.py relies on every property
asserted here: a population without long lists, or whose neighbouring asks all agreed, would let a wrong bisection pass."""
import functools
import json

import numpy as np
import pytest

import _oracle as orc
import _preemptgen
import _reachgen
import _victimgen
from _victimgen import LONG, NEVER, SHORT, midpoints

SEED = 20264
POPULATIONS = tuple(_victimgen.POPULATIONS)
TOPOLOGY = ("PodTopologySpread", "InterPodAffinity")
FORMS = {"default": ("*",), "no-ports": tuple(p for p in _preemptgen.PLUGINS if p != "NodePorts"),
         "no-fit": tuple(p for p in _preemptgen.PLUGINS if p != "NodeResourcesFit"),
         "no-spread": tuple(p for p in _preemptgen.PLUGINS if p != "PodTopologySpread"),
         "no-affinity": tuple(p for p in _preemptgen.PLUGINS if p != "InterPodAffinity"),
         "no-topology": tuple(p for p in _preemptgen.PLUGINS if p not in TOPOLOGY),
         "removal-only": _preemptgen.REMOVAL}


def masks(form):
    names = set(_preemptgen.PLUGINS) if "*" in FORMS[form] else set(FORMS[form])
    return orc.mask_of(names), orc.mask_of(names & set(_preemptgen.FROZEN))


class Case:
    """One population: the snapshot, the JSON text both sides load, and per plugin list the needs by the oracle and by the model."""

    def __init__(self, name=None, snapshot=None, bounds=None, meta=None):
        if snapshot is None:
            snapshot, bounds, meta = _victimgen.population(name, SEED)
        self.name, self.snapshot, self.bounds, self.meta = name, snapshot, bounds, meta
        self.text = json.dumps(snapshot)
        self.oracle = orc.Oracle(self.text)
        self.model = _victimgen.VictimModel(snapshot, bounds)
        self.asks = [p["metadata"]["uid"] for p in snapshot["pods"]]
        self.nodes = [n["metadata"]["name"] for n in snapshot["nodes"]]
        self.limits = [self.model.asks[uid][2] for uid in self.asks]
        self._needs = {}

    def needs(self, form="default"):
        """→ (by the oracle, by the model), each int32[asks][nodes], NEVER = -1."""
        if form in self._needs:
            return self._needs[form]
        mask, frozen_mask = masks(form)
        fits = self.oracle.eval_grid(pre_mask=mask, filt_mask=mask)
        frozen = self.oracle.eval_grid(pre_mask=frozen_mask, filt_mask=frozen_mask) if frozen_mask else np.ones_like(fits)
        by_oracle = np.zeros((len(self.asks), len(self.nodes)), dtype=np.int32)
        by_model = np.zeros_like(by_oracle)
        for a, uid in enumerate(self.asks):
            for n, node in enumerate(self.nodes):
                by_model[a, n] = self.model.need(uid, node, bool(frozen[a, n]), FORMS[form])
                if fits[a, n]:
                    continue
                i = self.oracle.preemption(a, n, self.model.victims(node, self.limits[a]), 0, mask, mask)
                by_oracle[a, n] = NEVER if i < 0 else i + 1
        self._needs[form] = (by_oracle, by_model)
        return self._needs[form]

    def levels(self, form="default"):
        """The reach level of every need >= 1 (0 elsewhere): tier(order[need - 1]) + 1."""
        needs = self.needs(form)[0]
        out = np.zeros_like(needs)
        for a, n in np.argwhere(needs >= 1):
            out[a, n] = self.model.level_of(self.nodes[n], self.limits[a], int(needs[a, n]))
        return out

    def cells(self, form="default"):
        needs, levels = self.needs(form)[0], self.levels(form)
        return np.array([_victimgen.cells(needs[a].tolist(), levels[a].tolist(), self.limits[a]) for a in range(len(self.asks))], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.parametrize("name", POPULATIONS)
@pytest.mark.parametrize("form", tuple(FORMS))
def test_model_agrees_with_the_oracle(name, form):
    by_oracle, by_model = case(name).needs(form)
    bad = np.argwhere(by_oracle != by_model)
    assert len(bad) == 0, [(case(name).asks[a], case(name).nodes[n], int(by_oracle[a, n]), int(by_model[a, n])) for a, n in bad[:8]]


@pytest.mark.parametrize("name", POPULATIONS)
def test_designed_pairs_land_on_their_need(name):
    c = case(name)
    by_oracle, _ = c.needs()
    ask_at = {uid: i for i, uid in enumerate(c.asks)}
    node_at = {n: i for i, n in enumerate(c.nodes)}
    assert len(c.meta["intended"]) >= 10
    wrong = {k: (want, int(by_oracle[ask_at[k[0]], node_at[k[1]]])) for k, want in c.meta["intended"].items()
             if by_oracle[ask_at[k[0]], node_at[k[1]]] != want}
    assert not wrong, (c.meta["rule"][next(iter(wrong))], wrong)


@pytest.mark.parametrize("name", POPULATIONS)
def test_population_conditions(name):
    """Every outcome occurs (fits, a prefix, never); fewer than half of the pairs are never; no two neighbouring asks share all 16 cells;
    [0] + [1] + [2] == N."""
    c = case(name)
    by_oracle, _ = c.needs()
    T = len(c.bounds)
    assert T == c.meta["T"] and T in (1, 3, 8)
    assert (by_oracle == 0).any() and (by_oracle >= 1).any() and (by_oracle == NEVER).any()
    assert (by_oracle == NEVER).sum() * 2 < by_oracle.size, float((by_oracle == NEVER).mean())
    cells = c.cells()
    same = [(c.asks[i], c.asks[i + 1]) for i in range(len(cells) - 1) if np.array_equal(cells[i], cells[i + 1])]
    assert not same, same
    assert (cells[:, :3].sum(axis=1) == len(c.nodes)).all()
    assert set(c.limits) >= ({0, T} if name != "gaps" else {T})


@pytest.mark.parametrize("name", POPULATIONS)
def test_level_identity_from_the_oracle_alone(name):
    """tier(order[need - 1]) + 1 is the level ReachModel gives (frozen verdicts from the oracle), need == -1 <=> level never, need 0 <=>
    level 0, and need <= the whole-tier pod count of that level."""
    c = case(name)
    needs, levels = c.needs()[0], c.levels()
    _, frozen_mask = masks("default")
    frozen = c.oracle.eval_grid(pre_mask=frozen_mask, filt_mask=frozen_mask)
    reach = _reachgen.ReachModel(c.snapshot, c.bounds)
    for a, uid in enumerate(c.asks):
        for n, node in enumerate(c.nodes):
            level = reach.level(uid, node, bool(frozen[a, n]))
            k = int(needs[a, n])
            assert (level == NEVER) == (k == NEVER) and (level == 0) == (k == 0), (uid, node, level, k)
            if k >= 1:
                assert levels[a, n] == level and k <= reach.victims_below(node, level), (uid, node, level, k)


def test_every_short_length_has_every_answer():
    """Lists of 0, 1, 2, 3, 4, 5, 7, 8, 9 victims; on each every need 1..len and never."""
    for name in ("lengths", "lengths_1", "lengths_8"):
        c = case(name)
        needs = c.needs()[0]
        T = len(c.bounds)
        assert c.meta["short"] == SHORT == (0, 1, 2, 3, 4, 5, 7, 8, 9)
        for length in SHORT:
            n = c.nodes.index(f"ln-{length}")
            assert len(c.model.victims(f"ln-{length}", T)) == length
            seen = {int(needs[a, n]) for a in range(len(c.asks)) if c.limits[a] == T}
            assert seen >= set(range(1, length + 1)) | {NEVER}, (name, length, seen)


def test_long_lengths_hit_both_sides_of_the_first_two_midpoints():
    assert midpoints(63) == (31, 15, 47) and midpoints(64) == (32, 16, 48) and midpoints(65) == (32, 16, 48)
    for name in ("lengths", "lengths_1", "lengths_8"):
        c = case(name)
        needs = c.needs()[0]
        T = len(c.bounds)
        for length in LONG:
            n = c.nodes.index(f"lg-{length}")
            assert len(c.model.victims(f"lg-{length}", T)) == length
            seen = {int(needs[a, n]) for a in range(len(c.asks)) if c.limits[a] == T}
            want = {1, length} | {m + s for m in midpoints(length) for s in (0, 1)}
            assert seen >= want, (name, length, sorted(want - seen))


def test_resources_sit_on_the_prefix_sum_in_every_dimension():
    """Per dimension: requests equal to free + the prefix sum, one below and one above; magnitudes beside 2^53 and up to 2^63 - 1."""
    for name in ("resource_exact", "resource_exact_8"):
        c = case(name)
        rules = {c.meta["rule"][k] for k in c.meta["intended"]}
        assert rules >= {"one below", "exact", "one above"}
        for j, d in enumerate(_preemptgen.DIMS):
            for k in (1, 3, 5):
                node = f"rx-{j}-{k}"
                alloc, _, pods = c.model.nodes[node]
                order = c.model.victims(node, len(c.bounds))
                assert len(order) == 5
                free = alloc[d] - sum(req.get(d, 0) for req, _, _ in pods)
                S = free + sum(pods[i][0].get(d, 0) for i in order[:k])
                got = [c.model.asks[f"a-{node}-{s}"][0][d] for s in range(3)]
                assert got == [S - 1, S, S + 1], (node, got, S)
                want = [c.meta["intended"][(f"a-{node}-{s}", node)] for s in range(3)]
                assert want[0] == k and want[1] == k and want[2] == (k + 1 if k < 5 else NEVER), (node, want)
        requests = [q for uid in c.asks for q in c.model.asks[uid][0].values()]
        assert any(q > (1 << 62) for q in requests) and max(requests) <= _preemptgen.I64_MAX
        assert any((1 << 53) - 64 < q < (1 << 53) + 64 for q in requests)
        for alloc, _, _ in c.model.nodes.values():
            assert all(0 <= v <= _preemptgen.I64_MAX for v in alloc.values())


def test_slots_are_the_only_binder():
    c = case("slots")
    needs = c.needs()[0]
    nothing = c.asks.index("a-slot-nothing")
    assert c.model.asks["a-slot-nothing"][0] == {}
    for k in range(1, 7):
        assert needs[nothing, c.nodes.index(f"sl-{k}")] == k
    assert needs[nothing, c.nodes.index("sl-7")] == NEVER
    # with NodeResourcesFit off nothing counts the slots: every such node takes the ask as it stands
    assert (c.needs("no-fit")[0][nothing, [c.nodes.index(f"sl-{k}") for k in range(1, 8)]] == 0).all()


def test_the_first_holder_frees_the_port():
    for name in ("ports", "ports_1"):
        c = case(name)
        needs = c.needs()[0]
        a = c.asks.index("a-port")
        T = len(c.bounds)
        same = c.model.victim_uids("pp-same", T)
        assert same == ["pp-same-x", "pp-same-h-a", "pp-same-h-b"] and needs[a, c.nodes.index("pp-same")] == 2
        tiers = [c.model.nodes["pp-same"][2][i][2] for i in c.model.victims("pp-same", T)]
        assert tiers[1] == tiers[2]   # two holders in ONE tier
        two = c.model.victim_uids("pp-two", T)
        assert two[0] == "pp-two-h0" and needs[a, c.nodes.index("pp-two")] == 1
        if T > 1:
            held = [c.model.nodes["pp-two"][2][i] for i in c.model.victims("pp-two", T)]
            assert {p[2] for p in held if _reachgen.T80 in p[1]} == {0, T - 1}   # ... and in TWO tiers
        assert needs[a, c.nodes.index("pp-last")] == 3
        assert needs[a, c.nodes.index("pp-uid-late")] == 2 and needs[a, c.nodes.index("pp-uid-early")] == 1
        assert needs[a, c.nodes.index("pp-kept")] == NEVER and needs[a, c.nodes.index("pp-out")] == NEVER
        assert (c.needs("no-ports")[0][a, [n for n, node in enumerate(c.nodes) if node.startswith("pp-")]] == 0).all()


def test_uid_order_decides_and_ineligible_pods_are_in_no_list():
    c = case("order")
    needs = c.needs()[0]
    T = len(c.bounds)
    listed = [p["metadata"]["uid"] for p in next(n for n in c.snapshot["nodes"] if n["metadata"]["name"] == "eq")["pods"]]
    assert listed.index("eq-b") < listed.index("eq-a")
    assert c.model.victim_uids("eq", T) == ["eq-a", "eq-b"]
    eq = c.nodes.index("eq")
    assert needs[c.asks.index("a-eq-300"), eq] == 2 and needs[c.asks.index("a-eq-100"), eq] == 1 and needs[c.asks.index("a-eq-101"), eq] == 2
    for node in c.nodes:
        assert not set(c.model.victim_uids(node, T)) & set(c.meta["absent"])
    # the best node by the exact count, where the whole-tier count names the other
    row = c.cells()[c.asks.index("a-bn")]
    name, level, need = c.meta["best"]["a-bn"]
    assert (c.nodes[row[6]], row[5], row[7]) == (name, level, need)
    reach = _reachgen.ReachModel(c.snapshot, c.bounds)
    assert reach.victims_below("bn-b", 1) < reach.victims_below("bn-a", 1)


def test_a_prefix_ends_mid_tier():
    """need strictly below reach's whole-tier count somewhere in every population with more than one victim per tier."""
    for name in ("lengths", "resource_exact", "limits", "order"):
        c = case(name)
        needs, levels = c.needs()[0], c.levels()
        reach = _reachgen.ReachModel(c.snapshot, c.bounds)
        assert any(needs[a, n] < reach.victims_below(c.nodes[n], int(levels[a, n])) for a, n in np.argwhere(needs >= 1)), name


def test_limits_cover_zero_to_T_and_the_tier_counts_one_three_eight():
    assert {T for _, T in _victimgen.POPULATIONS.values()} == {1, 3, 8}
    for name in ("limits_1", "limits", "limits_8"):
        c = case(name)
        T = len(c.bounds)
        assert set(c.limits) == set(range(T + 1))
        needs = c.needs()[0]
        li = c.nodes.index("li")
        assert needs[c.asks.index(f"a-li-{2 * T}-{T}"), li] == 2 * T and needs[c.asks.index(f"a-li-1-0"), li] == NEVER
        assert c.limits[c.asks.index("a-li-policy")] == 0 and needs[c.asks.index("a-li-policy"), li] == NEVER


def test_shut_pairs_and_the_empty_node_between_full_ones():
    c = case("shut")
    rules = set(c.meta["rules"])
    assert {"untolerated taint", "zone skew exceeded by another node's pods", "anti-affinity against the victims"} <= rules
    assert (c.needs("no-topology")[0] != c.needs()[0]).any()   # the frozen topology verdict is what shuts those pairs
    g = case("gaps")
    assert g.nodes == ["gp-0", "gp-1", "gp-2", "gp-3"]
    T = len(g.bounds)
    assert [len(g.model.victims(n, T)) for n in g.nodes] == [4, 0, 4, 0]


@pytest.mark.parametrize("n_nodes", (63, 64, 65, 257))
def test_geometry_has_seventy_distinct_tasks(n_nodes):
    snapshot, bounds, _ = _victimgen.geometry(SEED, n_nodes)
    assert len(snapshot["nodes"]) == n_nodes and len(snapshot["pods"]) == 70
    model = _victimgen.VictimModel(snapshot, bounds)
    assert len({(tuple(sorted(model.asks[p["metadata"]["uid"]][0].items())), model.asks[p["metadata"]["uid"]][2]) for p in snapshot["pods"]}) == 70
    assert {len(model.victims(n["metadata"]["name"], len(bounds))) for n in snapshot["nodes"]} >= {0, 1, 2, 3}
