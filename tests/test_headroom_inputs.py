"""The designed clusters of tests/_headgen.py held to what they claim, without a device: the model over Python ints equals the
reference's own loop — Σ replicas + 3 clones of a template through Oracle.allocate_sequential, counted per node — and the expectation
exercises every cell the device writes."""
import numpy as np

import _headgen as hg


def test_model_equals_the_clone_loop_node_by_node_for_every_template():
    _, meta = hg.designed()
    loops = hg.clone_loop()
    assert sorted(loops) == [j for j, t in enumerate(meta["templates"]) if t["status"] == 0] and len(loops) >= 12
    for j, counts in loops.items():
        want = np.array([k for k, _ in hg.model(meta, j)], dtype=np.int64)
        bad = np.flatnonzero(counts != want)
        assert not len(bad), (meta["templates"][j]["uid"], bad[:5], counts[bad[:5]], want[bad[:5]])
        assert want.sum() <= 2000  # (the clone loop stays within a second per template)


def test_expectation_exercises_every_cell_and_every_designed_boundary():
    _, meta = hg.designed()
    total = np.zeros(hg.CELLS, dtype=object)
    for j in range(len(meta["templates"])):
        cells = hg.expected_cells(meta, j)
        if cells[3] == 0:
            assert cells[4] + cells[5] + sum(cells[8:]) == cells[1] <= cells[0] and cells[2] <= cells[0]
        total += np.array(cells, dtype=object)
    for c in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):
        assert total[c] > 0, (c, total.tolist())
    assert total[6] == total[7] == 0 and sum(total[12:]) == 0
    assert sorted(t["status"] for t in meta["templates"])[-2:] == [1, 2]
    # the boundaries of the main template: free = k·req, k·req − 1 and k·req + 1 in each of the four dimensions, with k >= 1
    main = meta["templates"][0]["req"]
    seen = set()
    for node in meta["nodes"]:
        for r, res in enumerate(hg.RES):
            free, q = node["free"][res], main[res]
            for delta in (0, -1, 1):
                if free >= q and (free - delta) % q == 0:
                    seen.add((r, delta))
    assert seen >= {(r, d) for r in range(4) for d in (0, -1, 1)}
    # slots below every quotient, on the smallest one, and none, among nodes the main template is otherwise eligible for
    kinds = set()
    for node in meta["nodes"]:
        if node["tainted"] or node["unsched"]:
            continue
        q = min(node["free"][res] // main[res] for res in hg.RES)
        kinds.add("none" if node["slots"] == 0 else "below" if node["slots"] < q else "equal" if node["slots"] == q else "above")
    assert kinds == {"none", "below", "equal", "above"}
    # values a float64 cannot hold decide a quotient: 5·(2^53 + 1) − 1 over 2^53 + 1 is 4, in floating point 5
    big = [n for n in meta["nodes"] if n["free"]["memory"] == 5 * (hg.BIG + 1) - 1]
    assert big and hg.replicas(big[0], meta["templates"][6])[0] == 4 and int(float(5 * (hg.BIG + 1) - 1) / float(hg.BIG + 1)) == 5
    assert any(n["free"]["memory"] == (1 << 63) - 1 for n in meta["nodes"])
