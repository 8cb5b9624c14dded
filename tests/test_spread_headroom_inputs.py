"""The designed inputs of the spread-headroom tests, without a device: the model over Python ints of tests/_spreadgen.py equals the
reference's own sequential loop over clones domain by domain, and the inputs hold the situations they claim to hold. The oracle alone
satisfies every assertion here."""
import pytest

import _spreadgen as sg

CASES = {c["name"]: c for c in sg.designed_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_the_clone_loop_per_domain(name):
    c = CASES[name]
    rows, cells = sg.model(c)
    placed, unplaced = sg.clone_loop(c)
    assert unplaced == 3  # exactly 3 of total + 3 clones stay unplaced
    assert placed.tolist() == [r[3] for r in rows], name
    assert int(placed.sum()) == cells[0]
    # the summary's own invariants
    assert cells[8] + cells[9] + cells[10] == sum(1 for r in rows if r[1] >= 1)
    assert cells[0] <= cells[4] and cells[1] == sum(1 for r in rows if r[3] >= 1)


def test_the_inputs_hold_what_they_claim():
    models = {name: sg.model(c) for name, c in CASES.items()}
    # a domain with cap == 0 that pins the floor (the tainted zone): ten members fit where the plain quotient says hundreds
    rows, cells = models["skew1"]
    assert rows[cells[7]][1] == 0 and cells[6] == 0 and cells[0] == 2 and cells[4] > 700
    # a floor above 0, at 30 and at 32
    assert models["tol-30"][1][6] == 30 and models["tol-32"][1][6] == 32
    # a domain with cnt > floor + max_skew: shut although it has room
    rows, cells = models["seed-z0"]
    assert any(r[0] > cells[6] + CASES["seed-z0"]["max_skew"] and r[1] >= 1 and r[3] == 0 for r in rows) and cells[10] >= 1
    # minDomains above the present count: the floor is 0 although every present domain could rise
    for name in ("seed-min4", "q7-min9"):
        rows, cells = models[name]
        assert CASES[name]["min_domains"] > cells[5] and cells[6] == 0 and cells[7] == -1
    assert min(r[0] + r[1] for r in models["q7-min9"][0]) > 0
    assert models["min3"][1][5] == 3 and models["min3"][1][7] >= 0  # ... and exactly met: the rule does not apply
    # a domain id on each side of 63 / 64, with copies
    rows, _ = models["host2"]
    assert len(rows) == 200 and rows[63][3] == 2 and rows[64][3] == 2  # cut by the skew on both sides
    rows, _ = models["host1"]  # the seeded hosts 62 .. 65 have room and are shut, their neighbours take one copy
    assert len(rows) == 200 and [rows[d][0] for d in (62, 63, 64, 65)] == [1, 1, 1, 1]
    assert all(rows[d][1] >= 1 and rows[d][3] == 0 for d in (62, 63, 64, 65)) and rows[61][3] == 1 and rows[66][3] == 1
    # unlabelled nodes that would take copies; cut, filled and shut domains in one case
    c = CASES["q7"]
    assert sum(1 for v in c["labels"] if v is None) >= 10 and models["q7"][1][4] < sg.model(dict(c, labels=["q0"] * len(c["labels"])))[1][4]
    assert models["r14"][1][8] >= 1 and models["r14"][1][9] >= 1
    # the selector that does not match the ask itself: z0 is shut up to skew 7 and opens at 8
    assert [models[n][0][0][3] > 0 for n in ("res1", "res7", "res8")] == [False, False, True]
    assert models["res1"][0][0][0] - models["res1"][1][6] == 8
    # only the selected zone counts: one present domain
    assert models["sel-z2"][1][5] == 1 and models["sel-z2"][1][0] == models["sel-z2"][1][4]


def test_the_rule_is_sensitive_to_each_of_its_parts():
    """Each mutation of the rule changes some designed case's rows: the cases can tell the rule from its near misses."""
    def mutated(c, drop_min_domains=False, use_minv=False, count_absent=False, no_clamp=False):
        rows, cells = sg.model(c)
        if not c["self_match"]:
            return [r[3] for r in rows]
        D = len(rows)
        dom = sg.domain_of_nodes(c)
        tmpl = c["meta"]["templates"][c["ask"]]
        present = [any(dom[i] == d and sg.counts(n, tmpl) for i, n in enumerate(c["meta"]["nodes"])) for d in range(D)]
        here = [d for d in range(D) if present[d] or count_absent]
        under = len(here) < c["min_domains"] and not drop_min_domains
        if under or not here:
            floor = 0
        elif use_minv:
            floor = min(rows[d][0] for d in here)
        else:
            floor = min(rows[d][0] + rows[d][1] for d in here)
        out = []
        for r in rows:
            v = floor + c["max_skew"] - r[0]
            out.append(min(v if no_clamp else max(v, 0), r[1]))
        return out
    for kw in ("drop_min_domains", "use_minv", "count_absent", "no_clamp"):
        differs = [name for name, c in CASES.items() if mutated(c, **{kw: True}) != [r[3] for r in sg.model(c)[0]]]
        assert differs, kw
    assert all(mutated(c) == [r[3] for r in sg.model(c)[0]] for c in CASES.values())
