"""The designed rounds of tests/_liveroundgen.py held to their claims, and their model held to the oracle — on the CPU. A turn is pinned
through the reference's two calls on a snapshot EDITED step by step (the victims of every earlier turn deleted, the placed pods added),
under every plugin list: extra == 0 <=> Predicates fits; otherwise extra - 1 == PreemptionPredicates(ask, node, what is left of
order(node) below the ask's limit, 0), and never <=> that call returns -1. The topology plugins read the edited snapshot: that IS the
live histogram. tests/test_gpu_preempt_round_live.py relies on every property asserted here."""
import copy
import functools
import json

import numpy as np
import pytest

import _liveroundgen as gen
import _oracle as orc
from _preemptroundgen import RoundModel, edited
from test_preempt_victims_inputs import FORMS, masks

SEED = 20266
ROUNDS = tuple(gen.ROUNDS)


class LiveCase:
    def __init__(self, name):
        self.name = name
        self.snapshot, self.bounds, self.meta = gen.round_(name, SEED)
        self.text = json.dumps(self.snapshot)
        self.model = gen.LiveModel(self.snapshot, self.bounds)
        self.frozen_model = gen.LiveModel(self.snapshot, self.bounds, live=False)
        self.asks = [p["metadata"]["uid"] for p in self.snapshot["pods"]]
        self.ask_index = {uid: i for i, uid in enumerate(self.asks)}
        self.nodes = self.model.names
        self.turns = self.meta["turns"]
        self._cells = {}

    def histograms(self, form="default"):
        """After cells(form): the model's histograms at the start and the end of the round, and what the placed pods alone contribute →
        ((counts, minima) start, end, placed)."""
        if ("hist", form) not in self._cells:
            m = gen.LiveModel(self.snapshot, self.bounds)
            m.run(self.turns, FORMS[form])
            self._cells[("hist", form)] = (m.hist_start, m.hist_end, m.hist_placed)
        return self._cells[("hist", form)]

    def cells(self, form="default", live=True):
        """→ (int64[turns][8], int64[8]) by the model; live=False: the same model on the histograms of the start of the round."""
        if (form, live) not in self._cells:
            cells, summary = (self.model if live else self.frozen_model).run(self.turns, FORMS[form])
            self._cells[(form, live)] = (np.array(cells, dtype=np.int64).reshape(-1, 8), np.array(summary, dtype=np.int64))
        return self._cells[(form, live)]

    def by_oracle(self, form="default"):
        """The round with every verdict taken from the oracle on the edited snapshot."""
        mask, _ = masks(form)
        snap = copy.deepcopy(self.snapshot)
        book = RoundModel(self.snapshot, self.bounds)   # (only its tables and `taken`: no verdict of its own is used)
        T = len(self.bounds)
        out = []
        for i, uid in enumerate(self.turns):
            limit = book.asks[uid][2]
            if book.settled(uid, ()) == 3:
                out.append([3, -1, 0, 0, 0, limit, 0, 0])
                continue
            o = orc.Oracle(snap)
            a = self.ask_index[uid]
            fits = o.eval_grid(pods=[a], pre_mask=mask, filt_mask=mask)[0]
            keys = []
            for n, node in enumerate(self.nodes):
                taken = book.taken[node]
                if fits[n]:
                    keys.append((0, 0, n))
                    continue
                order = book.victims(node, T)
                rest = order[taken:max(taken, len(book.victims(node, limit)))]
                if not rest:
                    continue
                at = {p["metadata"]["uid"]: j for j, p in enumerate(snap["nodes"][n]["pods"])}
                index = o.preemption(a, n, [at[book.uids[node][j]] for j in rest], 0, mask, mask)
                if index >= 0:
                    keys.append((book.nodes[node][2][rest[index]][2] + 1, index + 1, n))
            o.close()
            if not keys:
                out.append([2, -1, 0, 0, 0, limit, 0, 0])
                continue
            level, extra, n = min(keys)
            row = [1 if extra else 0, n, book.taken[self.nodes[n]], extra, level, limit, len(keys), sum(k[1] for k in keys)]
            edited(snap, book, uid, row, i)
            book.taken[self.nodes[n]] += extra
            out.append(row)
        return np.array(out, dtype=np.int64).reshape(-1, 8)


@functools.lru_cache(maxsize=None)
def case(name):
    return LiveCase(name)


@pytest.mark.parametrize("name", ROUNDS)
@pytest.mark.parametrize("form", tuple(FORMS))
def test_model_agrees_with_the_oracle_step_by_step(name, form):
    c = case(name)
    by_model, by_oracle = c.cells(form)[0], c.by_oracle(form)
    bad = np.flatnonzero((by_model != by_oracle).any(axis=1))
    assert len(bad) == 0, (c.turns[bad[0]], int(bad[0]), by_model[bad[0]].tolist(), by_oracle[bad[0]].tolist())


@pytest.mark.parametrize("name", ROUNDS)
def test_turns_land_on_their_intent(name):
    c = case(name)
    cells = c.cells()[0]
    assert len(c.meta["intended"]) == len(c.turns) == len(cells)
    for i, intent in enumerate(c.meta["intended"]):
        if intent is None:
            continue
        outcome, node, start, extra = intent
        want = [outcome, c.nodes.index(node) if node else -1, start, extra]
        assert cells[i, :4].tolist() == want, (c.turns[i], i, cells[i].tolist(), want)
    if "copies" in c.meta:   # a gang: exactly its copies are placed, the rest goes nowhere
        mine = cells[[i for i, uid in enumerate(c.turns) if uid.split(".")[0] == c.meta["gang"]]]
        assert (mine[:, 0] <= 1).sum() == min(len(mine), c.meta["copies"]) and (mine[c.meta["copies"]:, 0] == 2).all()
        assert len(mine) - c.meta["copies"] in (-1, 0, 2) and (mine[:, 0] == 1).any()


@pytest.mark.parametrize("name", ROUNDS)
def test_round_conditions(name):
    """At most 40 turns on 70 or 130 nodes, at most a third of them nowhere, non-increasing limits (identity 1), the summary adds up —
    and the same model on FROZEN histograms differs in at least one cell: a no-op feature cannot pass."""
    c = case(name)
    cells, summary = c.cells()
    assert len(c.nodes) in (70, 130) and len(c.turns) <= gen.MAX_ASKS and len(c.bounds) in (1, 3)
    assert (cells[:, 0] == 2).sum() * 3 <= len(cells)
    assert (np.diff(cells[:, 5]) <= 0).all()
    assert summary[:5].sum() == len(cells) and summary[4] == 0 and summary[5] == cells[:, 3].sum()
    assert not np.array_equal(c.cells(live=False)[0], cells)
    assert (cells[cells[:, 0] >= 2][:, 1:5] == [-1, 0, 0, 0]).all()


def test_every_outcome_shape_and_designed_index_occurs():
    seen, T, N, chosen = set(), set(), set(), {}
    for name in ROUNDS:
        c = case(name)
        cells = c.cells()[0]
        seen |= set(cells[:, 0].tolist())
        T.add(len(c.bounds))
        N.add(len(c.nodes))
        chosen[name] = set(cells[:, 1].tolist())
    assert seen == {0, 1, 2, 3} and T == {1, 3} and N == {70, 130}
    assert {63, 64, 69} <= chosen["victim_min"] and {63, 64, 129} <= chosen["victim_min_130"] and {63, 64, 129} <= chosen["host_gang_eq"]


def test_the_named_turns_hold_what_they_name():
    c = case("victim_min")
    live, frozen = c.cells()[0], c.cells(live=False)[0]
    at = {uid: i for i, uid in enumerate(c.turns)}
    # the spread ask after the claim: in by a victim on a full node of zone a, while frozen histograms give it a free node of zone b
    assert live[at["web-1"]][[0, 3]].tolist() == [1, 1] and c.nodes[live[at["web-1"]][1]] == "vm-a1"
    assert frozen[at["web-1"]][0] == 0 and c.nodes[frozen[at["web-1"]][1]] == "vm-b"
    assert live[at["web-1"]][6] == 2    # vm-a1 and vm-a2: every free node of the crowded zones is never
    assert live[at["routed"]][0] == 3
    # without the claim nothing differs up to there: the victim alone moved the cell
    m = gen.LiveModel(c.snapshot, c.bounds)
    alone = m.run([uid for uid in c.turns if uid != "claim"])[0]
    assert alone[0][0] == 0 and alone[0][3] == 0
    # the opener's host takes a copy of the gang; the claimer itself was placed under the histograms of its own turn
    g = case("host_gang_eq")
    rows = g.cells()[0]
    assert g.nodes.index("hg-x") in rows[1:, 1].tolist() and g.nodes.index("hg-x") not in g.cells(live=False)[0][1:, 1].tolist()
    # the policy round: the stray pod moved no cell of pol's constraint
    p = case("policy")
    assert [p.nodes[r[1]] if r[1] >= 0 else None for r in p.cells()[0][:4]] == ["out", "p-a", "p-b", None]
    multi = next(x for x in p.snapshot["pods"] if x["metadata"]["uid"] == "multi")
    hit = sum(1 for x in p.snapshot["pods"] for k in x["spec"].get("topologySpreadConstraints") or []
              if all(multi["metadata"]["labels"].get(a) == b for a, b in k["labelSelector"]["matchLabels"].items()))
    assert hit == 12


@pytest.mark.parametrize("name", ROUNDS)
def test_histograms_move_and_the_steps_are_counted(name):
    """The model's histograms: every round moves cells, the steps are at least the moved cells, and the plugin lists do not touch them where
    they leave the plan alone (the round applies its effects whatever the lists hold)."""
    c = case(name)
    (start, _), (end, _), _ = c.histograms()
    moved = sum(1 for k, v in gen.flat(end).items() if v != gen.flat(start).get(k, 0))
    assert moved > 0 and c.cells()[1][7] >= moved
    assert len(c.model.hist_rows()) >= 1


def test_final_cells_moved_by_a_victim_alone_exist():
    """A final histogram cell BELOW its start value in a (row, domain) to which no placed pod contributes: only a claimed victim moved it."""
    found = {}
    for name in ROUNDS:
        c = case(name)
        (start, _), (end, _), (placed, _) = c.histograms()
        s, e, p = gen.flat(start), gen.flat(end), gen.flat(placed)
        found[name] = [k for k in s if e.get(k, 0) < s[k] and p.get(k, 0) == 0]
    # (victim_min and the host gangs get copies back into the domain the victim left; the affinity round's victims are not replaced:
    # the only db pod of zone c under nodb's row, the hater's term in zone b under shy's)
    assert (0, "z-c") in found["affinity"] and len(found["affinity"]) >= 2, found
    # the policy round pins what a step is: the stray pod lands outside the pool and moves NO cell of pol's row; two pol copies move one
    # cell each, each of the two multi copies moves twelve rows, the s-asks match nothing
    assert case("policy").cells()[1][7] == 2 + 2 * 12
