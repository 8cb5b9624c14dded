"""The designed inputs of the affinity-headroom tests, without a device: the model over Python ints of tests/_affgen.py equals the
reference's own sequential loop over clones domain by domain, the outside row included; the bootstrap case ends with the capacity of
the domain its first copy picked; the two-key case is NOT what the one-key rule says. The oracle alone satisfies every assertion here."""
import pytest

import _affgen as ag

CASES = {c["name"]: c for c in ag.designed_cases()}
MODELS = {name: ag.model(c) for name, c in CASES.items()}
COMPUTED = sorted(name for name, m in MODELS.items() if m[0] == 0)


@pytest.mark.parametrize("name", COMPUTED)
def test_model_equals_the_clone_loop_per_domain(name):
    c = CASES[name]
    status, key, mode, rows, cells = MODELS[name]
    placed, unplaced, _ = ag.clone_loop(c)
    assert unplaced == 3  # exactly 3 of total + 3 clones stay unplaced
    assert placed.tolist() == [r[3] for r in rows], name
    assert int(placed.sum()) == cells[0]
    # the summary's own invariants
    inside = rows[:-1]
    assert cells[8] + cells[9] == sum(1 for r in inside if r[1] >= 1)
    assert cells[0] <= cells[4] + cells[6] and cells[1] == sum(1 for r in inside if r[3] >= 1)
    if mode == 1:
        assert cells[0] == cells[1] + cells[6]
        assert all(r[1] == 0 for r in inside if r[0] > 0)  # a domain with cnt > 0 is shut already


def test_the_pins_of_the_rule():
    """Key, mode and totals of every case, as they were found on the oracle's loop when the rule was written down."""
    got = {name: (m[0], m[1], m[2], m[4][0]) for name, m in MODELS.items()}
    assert got == {
        "host-self": (0, ag.HOST, 1, 151), "zone-self": (0, ag.ZONE, 1, 3), "zone-self-res": (0, ag.ZONE, 1, 2),
        "host-self-1500": (0, ag.HOST, 1, 116), "host-self-main": (0, ag.HOST, 1, 166), "host-other": (0, ag.HOST, 0, 225),
        "zone-existing": (0, ag.ZONE, 0, 100), "aff-svc-host-self": (0, ag.HOST, 1, 98), "aff-res": (0, ag.ZONE, 0, 52),
        "aff-res-self": (0, ag.ZONE, 0, 52), "boot": (4, ag.ZONE, 2, -1), "two-keys": (2, None, 0, -1)}
    cells = {name: m[4] for name, m in MODELS.items()}
    assert len(MODELS["host-self"][3]) == 201 and cells["host-self"][14] == 151 and cells["host-self"][6] == 0
    assert (cells["host-self-1500"][1], cells["host-self-1500"][6]) == (106, 10) and len(MODELS["host-self-1500"][3]) == 189
    assert (cells["host-self-main"][1], cells["host-self-main"][6]) == (120, 46)
    assert cells["host-other"][14] == 113 and cells["zone-existing"][14] == 73 and cells["aff-res"][14] == 36
    assert cells["zone-self-res"][5] == 1 and MODELS["zone-self-res"][3][0][:2] == [1, 0]  # z0 shut by the resident
    assert cells["boot"][4] == 228


def test_the_inputs_hold_what_they_claim():
    rows = MODELS["host-self-1500"][3]
    values = ag.domain_values(CASES["host-self-1500"])
    # blocked hosts with room on both sides of domain ids 63 / 64 of a table of 188 domains, their neighbours open
    blocked = [d for d, r in enumerate(rows[:-1]) if r[0] > 0]
    assert [values[d] for d in blocked] == ["hn0062", "hn0063", "hn0064", "hn0065"] and all(rows[d][1:] == [0, 0, 0] for d in blocked)
    assert min(blocked) < 63 < max(blocked) + 5 and rows[-1][1] == rows[-1][3] == 10 and rows[-1][2] >= 1
    # the outside row of a mode-1 case holds more copies than nodes: nothing shuts it
    out = MODELS["host-self-main"][3][-1]
    assert out[3] == out[1] > out[2] >= 1
    # mode 0 with a term that does not match the ask: a domain takes several copies
    assert MODELS["host-other"][4][2] > 1 and MODELS["host-other"][4][9] == 0
    # an existing pod's term shuts its zone for the ask, and the ask's copies do not add to it
    assert MODELS["zone-existing"][3][0][:2] == [1, 0] and MODELS["zone-existing"][4][5] == 1
    # affinity: only the zone of the matching resident takes copies, self-matching or not
    for name in ("aff-res", "aff-res-self"):
        assert [r[1] > 0 for r in MODELS[name][3]] == [False, False, True, False]
    # affinity on zone beside self anti-affinity on hostname: the rows lie on the hostname key, the zones without a match are shut
    assert MODELS["aff-svc-host-self"][4][14] == 98 and MODELS["aff-svc-host-self"][4][2] == 1


def test_bootstrap_ends_with_the_capacity_of_the_domain_its_first_copy_picked():
    c = CASES["boot"]
    status, key, mode, rows, cells = MODELS["boot"]
    assert (status, mode, cells[0]) == (4, 2, -1) and cells[4] == sum(r[1] for r in rows[:-1]) and rows[-1][1] == 0
    placed, unplaced, first = ag.clone_loop(c, count=cells[4] + 3)
    d1 = ag.domain_of_nodes(c, key)[first]
    assert placed[d1] == rows[d1][1] == int(placed.sum()) and unplaced == cells[4] + 3 - rows[d1][1]
    assert rows[d1][1] < cells[4]  # order-dependent: another start gives another total
    assert len({r[1] for r in rows[:-1]}) > 1 and cells[2] == max(r[1] for r in rows[:-1]) and rows[cells[11]][1] == cells[2]


def test_two_self_contributing_keys_are_not_the_one_key_rule():
    c = CASES["two-keys"]
    assert MODELS["two-keys"][0] == 2 and MODELS["two-keys"][4][:4] == [-1, 0, -1, 2]
    by_host = ag.model(c, one_key=ag.HOST)[4][0]
    placed, unplaced, _ = ag.clone_loop(c, count=by_host + 3, key=ag.ZONE)
    assert int(placed.sum()) == 3 and placed.tolist() == [1, 1, 1, 0] and by_host == 151  # the loop places one per zone
