"""The designed rounds of tests/_preemptroundgen.py held to their claims, and their model held to the oracle — on the CPU. A turn is pinned
through the reference's two calls on a snapshot EDITED step by step (the victims of every earlier turn deleted, the placed pods added):
extra == 0 <=> Predicates fits; otherwise extra - 1 == PreemptionPredicates(ask, node, what is left of order(node) below the ask's limit,
0), and never <=> that call returns -1. The choice (lowest level, fewest further victims, lowest index) and the bookkeeping are the
definition's. tests/test_gpu_preempt_round.py relies on every property asserted here."""
import copy
import functools
import json

import numpy as np
import pytest

import _oracle as orc
import _preemptgen
import _preemptroundgen as gen
from test_preempt_victims_inputs import FORMS, masks

SEED = 20265
ROUNDS = tuple(gen.ROUNDS)


class RoundCase:
    def __init__(self, name=None, built=None):
        snapshot, bounds, meta = built if built is not None else gen.round_(name, SEED)
        self.name, self.snapshot, self.bounds, self.meta = name, snapshot, bounds, meta
        self.text = json.dumps(snapshot)
        self.oracle = orc.Oracle(self.text)
        self.model = gen.RoundModel(snapshot, bounds)
        self.asks = [p["metadata"]["uid"] for p in snapshot["pods"]]
        self.ask_index = {uid: i for i, uid in enumerate(self.asks)}
        self.nodes = self.model.names
        self.turns = meta["turns"]
        self._cells, self._frozen = {}, {}

    def frozen(self, form="default"):
        if form not in self._frozen:
            _, frozen_mask = masks(form)
            shape = (len(self.asks), len(self.nodes))
            self._frozen[form] = self.oracle.eval_grid(pre_mask=frozen_mask, filt_mask=frozen_mask) if frozen_mask else np.ones(shape, dtype=np.uint8)
        return self._frozen[form]

    def cells(self, form="default", turns=None):
        """→ (int64[turns][8], int64[8]) by the model."""
        key = (form, None if turns is None else tuple(turns))
        if key not in self._cells:
            cells, summary = self.model.run(self.turns if turns is None else turns, self.frozen(form), self.ask_index, FORMS[form])
            self._cells[key] = (np.array(cells, dtype=np.int64).reshape(-1, 8), np.array(summary, dtype=np.int64))
        return self._cells[key]

    def by_oracle(self, form="default"):
        """The round again with every verdict taken from the oracle on the edited snapshot."""
        mask, _ = masks(form)
        snap = copy.deepcopy(self.snapshot)
        book = gen.RoundModel(self.snapshot, self.bounds)   # (only its tables and `taken`: no verdict of its own is used)
        T = len(self.bounds)
        out = []
        for i, uid in enumerate(self.turns):
            limit = book.asks[uid][2]
            settled = book.settled(uid, FORMS[form])
            if settled:
                out.append([settled, -1, 0, 0, 0, limit, 0, 0])
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
            gen.edited(snap, book, uid, row, i)
            book.taken[self.nodes[n]] += extra
            out.append(row)
        return np.array(out, dtype=np.int64).reshape(-1, 8)


@functools.lru_cache(maxsize=None)
def case(name):
    return RoundCase(name)


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
    for i, (outcome, node, start, extra) in enumerate(c.meta["intended"]):
        want = [outcome, c.nodes.index(node) if node else -1, start, extra]
        assert cells[i, :4].tolist() == want, (c.turns[i], i, cells[i].tolist(), want)


@pytest.mark.parametrize("name", ROUNDS)
def test_round_conditions(name):
    """N off the wave width, at most 40 turns, fewer than half of them nowhere, no two neighbouring turns share all 8 cells, the summary
    adds up."""
    c = case(name)
    cells, summary = c.cells()
    assert len(c.nodes) in (70, 130) and len(c.turns) <= gen.MAX_ASKS and len(c.bounds) in (1, 3, 8)
    assert (cells[:, 0] == 2).sum() * 2 < len(cells)
    same = [(c.turns[i], c.turns[i + 1]) for i in range(len(cells) - 1) if np.array_equal(cells[i], cells[i + 1])]
    assert not same, same
    assert summary[:5].sum() == len(cells) and summary[5] == cells[:, 3].sum() and summary[6] == len(set(cells[cells[:, 1] >= 0, 1].tolist()))
    assert (cells[:, 5] == [c.model.asks[uid][2] for uid in c.turns]).all()
    assert (cells[cells[:, 0] >= 2][:, 1:5] == [-1, 0, 0, 0]).all()


def test_every_outcome_and_a_continued_prefix_occur():
    seen, T, N = set(), set(), set()
    for name in ROUNDS:
        c = case(name)
        seen |= set(c.cells()[0][:, 0].tolist())
        T.add(len(c.bounds))
        N.add(len(c.nodes))
        assert (c.cells()[0][:, 2] > 0).any(), name   # some turn continues a prefix an earlier one began
    assert seen == {0, 1, 2, 3, 4} and T == {1, 3, 8} and N == {70, 130}
    assert set(case("conflicts").cells()[0][:, 0].tolist()) == {0, 1, 2, 3, 4}


def test_the_conflicts_round_holds_what_it_names():
    c = case("conflicts")
    cells = c.cells()[0]
    at = {uid: i for i, uid in reversed(list(enumerate(c.turns)))}   # (the first turn of each ask)
    row = lambda uid: cells[at[uid]]   # noqa: E731
    # the independent best node of cs-1 and cs-2 coincides (a round of one ask each), and so does that of ca-1 and ca-2
    for first, second in (("cs-1", "cs-2"), ("ca-1", "ca-2")):
        alone = [c.cells(turns=[uid])[0][0] for uid in (first, second)]
        assert alone[0][1] == alone[1][1] and alone[0][2] == alone[1][2] == 0
    assert row("cs-2")[1] == row("cs-1")[1] and row("cs-2")[2] > 0
    assert row("ca-2")[1] != row("ca-1")[1]
    # su did not fit su-2 at round start
    assert c.cells(turns=["su-2"])[0][0][3] >= 1 and row("su-2")[[0, 3]].tolist() == [0, 0] and row("su-2")[2] == 1
    # ll-lo: taken beyond the ask's own tier_end
    ll = "ll"
    assert row("ll-lo")[2] == 2 > len(c.model.victims(ll, c.model.asks["ll-lo"][2])) == 1
    # slots are the only binder on sl
    assert c.model.asks["sl-1"][0] == {} and (c.cells("no-fit")[0][at["sl-1"]][[0, 3]] == 0).all()
    # the second copy is shut out by the first; with NodePorts off it is not
    assert row("po-2")[0] == 2 and c.cells("no-ports")[0][at["po-2"]][0] == 0
    assert c.model.victim_uids("pt", 3) == ["pt-h0", "pt-h1"] and row("pt-1")[3] == 1
    # the neighbours of the routed and the coupled ask are what they are without them
    without = [uid for uid in c.turns if uid not in ("routed", "coupled")]
    assert np.array_equal(c.cells(turns=without)[0], cells[[i for i, uid in enumerate(c.turns) if uid not in ("routed", "coupled")]])
    assert row("routed")[0] == 3 and row("coupled")[0] == 4 and c.cells("no-topology")[0][at["coupled"]][0] in (0, 1) and c.cells("no-spread")[0][at["coupled"]][0] == 4
    assert c.snapshot["pods"][c.ask_index["pin"]]["spec"]["nodeName"] == "cs-b" and c.nodes[row("pin")[1]] == "cs-b"
    assert {c.model.asks[uid][2] for uid in ("su-0", "l0-0")} == {0} and row("su-0")[0] == 0 and row("l0-0")[0] == 2
    # a repeat is one more copy
    assert c.turns.count("cs-1") == 2


def test_requests_sit_on_free_plus_cum_minus_placed_in_every_dimension():
    seen = set()
    for name in ("exact_lo", "exact_hi"):
        c = case(name)
        cells = c.cells()[0]
        for i in range(0, len(c.turns), 2):
            opener, probe = c.turns[i], c.turns[i + 1]
            node = c.nodes[cells[i, 1]]
            j, delta = int(node.split("-")[1]), int(node.split("-")[2]) - 1
            d = _preemptgen.DIMS[j]
            seen.add(j)
            alloc, _, pods = c.model.nodes[node]
            order = c.model.victims(node, len(c.bounds))
            free = alloc[d] - sum(req.get(d, 0) for req, _, _ in pods)
            S = free + sum(pods[k][0].get(d, 0) for k in order[:2]) - c.model.asks[opener][0][d]
            assert c.model.asks[probe][0] == {d: S + delta} and cells[i + 1, 2] == 1 and cells[i + 1, 3] == (1 if delta <= 0 else 2)
        requests = [q for uid in c.asks for q in c.model.asks[uid][0].values()]
        assert any(q > (1 << 62) for q in requests) and max(requests) <= _preemptgen.I64_MAX
        assert any((1 << 53) - 64 < q < (1 << 53) + 64 for q in requests)
    assert seen == set(range(8))


def test_the_probes_land_on_both_sides_of_the_first_two_midpoints():
    assert gen.mids(5, 63) == (34, 19, 48) and gen.mids(5, 64) == (34, 19, 49) and gen.mids(5, 65) == (35, 20, 50)
    for name in ("bisect", "bisect_8"):
        c = case(name)
        cells = c.cells()[0]
        taken = c.meta["taken"]
        for length in (63, 64, 65):
            m, m_lo, m_hi = gen.mids(taken, length)
            ends = {int(r[2] + r[3]) for r, uid in zip(cells, c.turns) if uid.startswith(f"a-lg-{length}-") and uid.endswith("probe")}
            assert ends == {m, m + 1, m_lo + 1, m_hi} and all(len(c.model.victims(n, len(c.bounds))) == length for n in c.nodes if n.startswith(f"lg-{length}-"))
        assert (cells[1::2, 2] == taken).all()


def test_best_nodes_sit_at_the_designed_indices_and_ties_go_down():
    c = case("places")
    cells = c.cells()[0]
    N = len(c.nodes)
    assert cells[:3, 1].tolist() == [63, 64, N - 1]
    by = dict(zip(c.turns, cells))
    assert [by[f"a-tie-{i}"][1] for i in (1, 2, 3)] == [10, 10, 20] and [by[f"a-wv-{i}"][1] for i in (1, 2, 3)] == [127, 127, 128]
    # an exact tie: both nodes carry the same (level, extra) at the first and second turn
    c.model.start()
    needs = [c.model.need_more("a-tie-1", n, True) for n in ("tie-a", "tie-b")]
    assert needs[0] == needs[1] == (1, 1)


def test_gangs_place_copies_and_no_more():
    for name, beyond in (("gang_m1", -1), ("gang_eq", 0), ("gang_p2", 2)):
        c = case(name)
        cells = c.cells()[0]
        copies = c.meta["copies"]
        mine = cells[[i for i, uid in enumerate(c.turns) if uid == c.meta["gang"]]]
        assert len(mine) == copies + beyond and (mine[:, 0] <= 1).sum() == min(len(mine), copies)
        many = c.cells(turns=[c.meta["gang"]] * (copies + 3))[0]
        assert (many[:, 0] <= 1).sum() == copies and (many[copies:, 0] == 2).all()
