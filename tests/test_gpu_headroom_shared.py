"""The headroom calls share one engine driver, one scratch buffer and one node walk: calls of different kinds on ONE
manager, one after another, must each return what a fresh manager returns for that call alone — nothing of a call (task table, table
chunk, summaries) may reach the next one, whatever its kind and however much smaller its table is."""
import importlib

import numpy as np
import pytest

import _affgen as ag
import _spreadgen as sg

pkg = importlib.import_module("yunikorn-k8shim_amd")
pytestmark = pytest.mark.gpu

N_NODES, AFF_ASKS = 130, 70  # (two node blocks, the second one 2 nodes wide; 70 tasks: table chunks of 66 + 4)


def _flat(result):
    return list(result) if isinstance(result, tuple) else [result]


@pytest.mark.parametrize("tune", ["group_chunk_tasks=66", "group_chunk_tasks=66,group_lds=0"])
def test_interleaved_calls_on_one_manager_equal_fresh_managers(monkeypatch, tune):
    """70 anti-affinity asks of tests/_affgen.py and two spread asks of tests/_spreadgen.py over the same 130 nodes."""
    monkeypatch.setenv("YKPRED_TUNE", tune)
    # (an anti term that matches the residents' role and none of the asks: a pending ask's anti term is an existing one for every ask
    # it matches — the spread asks would stay coupled. 63 domains and the outside row: the LDS form's last row, unless group_lds=0)
    limit = pkg.GROUP_LDS_MAX_GROUPS
    c = ag.case("w-63", N_NODES, extra_asks=AFF_ASKS - 1, anti=[ag.term("m", role="blk")],
                label=("m", lambda i: None if i % 50 == 1 else f"m{i % limit:03d}"), residents=lambda i: [ag.OTHER] if i % 35 == 6 else [])
    spread = sg.case("shared", N_NODES, tolerate=True, extra_asks=1)["snapshot"]["pods"]
    snap = {"nodes": c["snapshot"]["nodes"], "pods": c["snapshot"]["pods"] + spread}
    assert len(c["snapshot"]["pods"]) == AFF_ASKS
    some = [AFF_ASKS, 3, AFF_ASKS + 1]  # (a spread ask, an affinity ask, the other spread ask: a table far smaller than the one before)
    calls = [("affinity", lambda m: m.headroom_affinity()),
             ("spread", lambda m: m.headroom_spread()),
             ("domains", lambda m: m.headroom_domains(label_key=sg.ZONE, groups=True)),
             ("affinity rows", lambda m: m.headroom_affinity_domains(67)),
             ("spread of three", lambda m: m.headroom_spread(some)),
             ("affinity again", lambda m: m.headroom_affinity())]
    shared = pkg.GpuPredicateManager()
    try:
        shared.load_snapshot(snap)
        got = [_flat(call(shared)) for _, call in calls]
        key = shared.encoded_tables()["topology_keys"].index("m")
    finally:
        shared.close()
    for (name, call), mine in zip(calls, got):
        fresh = pkg.GpuPredicateManager()
        try:
            fresh.load_snapshot(snap)
            alone = _flat(call(fresh))
        finally:
            fresh.close()
        assert len(mine) == len(alone), name
        for a, b in zip(mine, alone):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, (tune, name)
    first, spread_all, _, rows, spread_some, last = got
    assert np.array_equal(first[0], last[0])
    # the affinity answers are the model's; the spread asks are still coupled there, and computed by the spread call
    for j in range(AFF_ASKS):
        status, _, _, want_rows, cells = ag.model(c, j)
        cells = list(cells)
        cells[12] = key
        assert status == 0 and first[0][j].tolist() == cells, (tune, j)
        if j == 67:
            assert rows[0].tolist() == cells and rows[1].tolist() == want_rows and rows[2] == ag.domain_values(c)
    assert first[0][AFF_ASKS:, 3].tolist() == [2, 2]
    assert spread_all[0][:AFF_ASKS, 3].tolist() == [2] * AFF_ASKS and spread_all[0][AFF_ASKS:, 3].tolist() == [0, 0]
    assert np.array_equal(spread_some[0], spread_all[0][some])
