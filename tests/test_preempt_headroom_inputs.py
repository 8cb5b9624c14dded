"""The designed preemption-headroom populations of tests/_gangreachgen.py held to their claims, and their model held to the reference
path — on the CPU. The reference has no call that returns copies per level; rep_L is pinned the way tests/_headgen.clone_loop pins
headroom: delete the residents of tiers < L from the snapshot, hand the oracle's sequential allocation loop (the reference's node loop
+ AssumePod) Σ model + 3 clones of the ask, and exactly 3 stay unplaced while every node holds the model's count.
tests/test_gpu_preempt_headroom.py relies on every property asserted here."""
import functools
import json

import numpy as np
import pytest

import _gangreachgen as gg
import _headgen
import _oracle as orc
import _preemptgen
from _reachgen import NEVER

SEED = 20277
POPULATIONS = tuple(gg.POPULATIONS)
TOPOLOGY = ("PodTopologySpread", "InterPodAffinity")
FORMS = {"default": ("*",), "no-ports": tuple(p for p in _preemptgen.PLUGINS if p != "NodePorts"),
         "no-spread": tuple(p for p in _preemptgen.PLUGINS if p != "PodTopologySpread"),
         "no-affinity": tuple(p for p in _preemptgen.PLUGINS if p != "InterPodAffinity"),
         "no-topology": tuple(p for p in _preemptgen.PLUGINS if p not in TOPOLOGY)}


def names_of(form):
    return set(_preemptgen.PLUGINS) if "*" in FORMS[form] else set(FORMS[form])


class Case:
    """One population: the snapshot, the JSON text both sides load, the model, and per plugin list the copies per (ask, level, node),
    the statuses, the designed wants and the 32 expected cells."""

    def __init__(self, name=None, snapshot=None, bounds=None, meta=None):
        if snapshot is None:
            snapshot, bounds, meta = gg.population(name, SEED)
        self.name, self.snapshot, self.bounds, self.meta = name, snapshot, bounds, meta
        self.text = json.dumps(snapshot)
        self.oracle = orc.Oracle(self.text)
        self.model = gg.GangModel(snapshot, bounds)
        self.asks = [p["metadata"]["uid"] for p in snapshot["pods"]]
        self.nodes = self.model.names
        self.limits = [self.model.asks[uid][2] for uid in self.asks]
        self.T = len(bounds)
        self.gone = [[self.model.gone(node, L) for node in self.nodes] for L in range(self.T + 1)]
        self._forms = {}

    def status(self, a, form="default"):
        """ykpred_headroom's rule: 2 when the ask carries a hard spread constraint or a required (anti-)affinity term and EITHER topology
        plugin is in the list (the engine keeps one signature per spec for both kinds)."""
        spec = self.snapshot["pods"][a]["spec"]
        on = names_of(form)
        spread = any(c.get("whenUnsatisfiable") == "DoNotSchedule" for c in spec.get("topologySpreadConstraints", []))
        aff = spec.get("affinity") or {}
        ipa = any((aff.get(k) or {}).get("requiredDuringSchedulingIgnoredDuringExecution") for k in ("podAffinity", "podAntiAffinity"))
        return 2 if (spread or ipa) and (on & set(TOPOLOGY)) else 0

    def form(self, form="default"):
        """→ (rows[a] = int32[limit + 1][N] by the model, statuses, wants, cells int64[asks][32])."""
        if form in self._forms:
            return self._forms[form]
        on = names_of(form)
        frozen_mask = orc.mask_of(on & set(_preemptgen.FROZEN))
        frozen = self.oracle.eval_grid(pre_mask=frozen_mask, filt_mask=frozen_mask)
        rows = [np.array(self.model.rows(uid, frozen[a], FORMS[form]), dtype=np.int32).reshape(self.limits[a] + 1, len(self.nodes))
                for a, uid in enumerate(self.asks)]
        statuses = [self.status(a, form) for a in range(len(self.asks))]
        copies = [[0] * (self.limits[a] + 1) if statuses[a] else rows[a].sum(axis=1).tolist() for a in range(len(self.asks))]
        wants = gg.wants_for(copies, self.limits)
        cells = np.array([self.cells_of(rows[a], self.limits[a], wants[a], statuses[a]) for a in range(len(self.asks))], dtype=np.int64)
        self._forms[form] = (rows, statuses, wants, cells)
        return self._forms[form]

    def cells_of(self, rows, limit, want, status):
        return gg.expected_cells(rows.tolist(), self.gone, limit, want, status, fit_rows=(rows >= 1).tolist())

    def every_aim(self, form="default"):
        """→ (ask indices, wants, cells): every ask once per level it can aim at — the want that level's copies meet first — and once
        with a want nothing meets. One task per ask, however many wants."""
        rows, statuses, _, _ = self.form(form)
        idx, wants = [], []
        for a in range(len(self.asks)):
            copies = [0] if statuses[a] else rows[a].sum(axis=1).tolist()
            for w in sorted({c for c in copies if c >= 1} | {max(copies) + 1}):
                idx.append(a)
                wants.append(w)
        cells = np.array([self.cells_of(rows[a], self.limits[a], w, statuses[a]) for a, w in zip(idx, wants)], dtype=np.int64)
        return idx, wants, cells

    def without_tiers_below(self, L):
        """The snapshot with the residents of tiers < L deleted."""
        nodes = [dict(n, pods=[p for p in n["pods"] if not 0 <= self.model.tier(p) < L]) for n in self.snapshot["nodes"]]
        return {"nodes": nodes, "pods": self.snapshot["pods"]}


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.parametrize("name", POPULATIONS)
def test_model_and_intended_copies_are_what_the_clone_loop_places(name):
    c = case(name)
    rows, statuses, _, _ = c.form()
    checked = 0
    for a, uid in enumerate(c.asks):
        if statuses[a]:
            continue
        for L in range(c.limits[a] + 1):
            want = rows[a][L].astype(np.int64)
            # (where the model follows RemovePod's set of used ports, the snapshot with the residents deleted still shows the second holder)
            for n, node in enumerate(c.nodes):
                if (uid, node, L) in c.meta["set_pairs"]:
                    assert want[n] == 1
                    want[n] = 0
            total = int(want.sum())
            placed = orc.Oracle(_headgen.clones(c.without_tiers_below(L), a, total + 3)).allocate_sequential()
            assert int((placed < 0).sum()) == 3, (uid, L, total, int((placed < 0).sum()))
            got = np.bincount(placed[placed >= 0], minlength=len(c.nodes))
            assert np.array_equal(got, want), (uid, L, [(c.nodes[n], int(got[n]), int(want[n])) for n in np.flatnonzero(got != want)[:6]])
            checked += 1
    assert checked >= 2 * sum(1 for s in statuses if s == 0) - 8
    for (uid, node), reps in c.meta["intended"].items():
        a, n = c.asks.index(uid), c.nodes.index(node)
        assert rows[a][:, n].tolist() == reps, (uid, node, rows[a][:, n].tolist(), reps)
    assert len(c.meta["intended"]) >= 10


@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("name", POPULATIONS)
def test_first_level_with_a_copy_is_the_reach_level(name, form):
    c = case(name)
    on = names_of(form)
    frozen_mask = orc.mask_of(on & set(_preemptgen.FROZEN))
    frozen = c.oracle.eval_grid(pre_mask=frozen_mask, filt_mask=frozen_mask)
    rows = c.form(form)[0]
    for a, uid in enumerate(c.asks):
        for n, node in enumerate(c.nodes):
            level = c.model.level(uid, node, bool(frozen[a, n]), FORMS[form])
            first = next((L for L in range(c.limits[a] + 1) if rows[a][L, n] >= 1), NEVER)
            assert first == level, (uid, node, first, level)
        assert (np.diff(rows[a], axis=0) >= 0).all(), uid   # non-decreasing in L


@pytest.mark.parametrize("name", POPULATIONS)
def test_population_conditions(name):
    c = case(name)
    rows, statuses, wants, cells = c.form()
    assert c.T == c.meta["T"] and all(w >= 1 for w in wants)
    live = [a for a in range(len(c.asks)) if statuses[a] == 0]
    rising = [a for a in live if cells[a, gg.COPIES + c.limits[a]] > cells[a, gg.COPIES]]
    assert 2 * len(rising) >= len(live), (len(rising), len(live))
    same = [(c.asks[i], c.asks[i + 1]) for i in range(len(cells) - 1) if np.array_equal(cells[i], cells[i + 1])]
    assert not same, same
    # every level occurs as the first level of some copy (the ladder)
    firsts = {int(np.argmax(rows[a][:, n] >= 1)) for a in live for n in range(len(c.nodes)) if rows[a][-1, n] >= 1}
    assert firsts == set(range(c.T + 1))
    # the invariants of the contract hold for the expected cells themselves
    for a in live:
        row = cells[a]
        assert (np.diff(row[0:9]) >= 0).all() and (np.diff(row[9:18]) >= 0).all() and (np.diff(row[18:27]) >= 0).all()
        assert (row[9:18] <= row[0:9]).all() and row[18] == 0
    assert {s for s in statuses} == ({0, 2} if name == "coupled" else {0})


def test_every_outcome_of_the_level_cell_occurs():
    """Per tier count: -1, 0 and every level 1..T occur in cell [30] — with the wants of Case.every_aim — and with the per-ask wants of
    Case.form at least -1, 0 and one level above 0."""
    seen = {1: set(), 3: set(), 8: set()}
    for name in POPULATIONS:
        c = case(name)
        seen[c.T] |= set(c.every_aim()[2][:, gg.LEVEL].tolist())
        assert {-1, 0} <= set(c.form()[3][:, gg.LEVEL].tolist()) and c.form()[3][:, gg.LEVEL].max() >= 1, name
    for T, levels in seen.items():
        assert levels == set(range(-1, T + 1)), (T, levels)


def test_flat_tiers_charges_only_the_tiers_that_add_a_copy():
    c = case("flat_tiers")
    rows, _, _, cells = c.form()
    a, n = c.asks.index("a-ft-100"), c.nodes.index("ft-short")
    assert rows[a][:, n].tolist() == [1, 1, 2, 2] and [c.gone[L][n] for L in range(4)] == [0, 1, 2, 2]
    alone = {"nodes": [c.snapshot["nodes"][n]], "pods": [c.snapshot["pods"][a]]}
    one = Case(snapshot=alone, bounds=c.bounds, meta=dict(c.meta, intended={}))
    row = one.form()[3][0]
    assert row[gg.VICTIMS:gg.VICTIMS + 4].tolist() == [0, 0, 2, 2]    # level 1 frees 50m of the 100m: not charged; level 2 pays for both
    assert [one.gone[L][0] for L in range(4)] != row[gg.VICTIMS:gg.VICTIMS + 4].tolist()
    late = c.nodes.index("ft-late")
    assert rows[a][:, late].tolist() == [0, 0, 0, 1]
    assert any(cells[a, gg.VICTIMS + L] != sum(c.gone[L][m] for m in range(len(c.nodes)) if rows[a][L, m] >= 1) for L in range(1, 4))


def test_limit_siblings_and_policy_never():
    c = case("limits")
    rows, _, _, cells = c.form()
    li = c.nodes.index("li")
    full, two, never = (c.asks.index(u) for u in ("a-li-100-3", "a-li-100-2", "a-li-100-policy"))
    assert rows[full][:, li].tolist() == [0, 1, 2, 3] and rows[two][:, li].tolist() == [0, 1, 2]
    assert cells[two, gg.COPIES + 2] == cells[two, gg.COPIES + 8] < cells[full, gg.COPIES + 3]
    assert c.limits[never] == 0 and len(set(cells[never, 0:9].tolist())) == 1


def test_quotient_edges_reach_the_large_magnitudes():
    c = case("quotient_edges")
    requests = [q for uid in c.asks for q in c.model.asks[uid][0].values()]
    assert any(q > (1 << 62) for q in requests) and any((1 << 53) - 64 < q < (1 << 53) + 64 for q in requests)
    for alloc, _, _ in c.model.nodes.values():
        assert all(0 <= v <= _preemptgen.I64_MAX for v in alloc.values())
    assert len({d for uid in c.asks if uid.startswith("a-qe-") for d in c.model.asks[uid][0]}) == 8


def test_the_tier_counts_cover_one_three_and_eight():
    assert {T for _, T in gg.POPULATIONS.values()} == {1, 3, 8}


@pytest.mark.parametrize("n_nodes", (1, 63, 64, 65, 257, 300))
def test_geometry_has_seventy_distinct_tasks(n_nodes):
    snapshot, bounds, _ = gg.geometry(SEED, n_nodes)
    assert len(snapshot["nodes"]) == n_nodes and len(snapshot["pods"]) == 70
    model = gg.GangModel(snapshot, bounds)
    assert len({(tuple(sorted(model.asks[p["metadata"]["uid"]][0].items())), model.asks[p["metadata"]["uid"]][2]) for p in snapshot["pods"]}) == 70
