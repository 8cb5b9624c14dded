#!/usr/bin/env python3
"""Cost of "can preemption place the whole gang, at which level, for how many victims" at configs[2] size (50 000 nodes x 1 000 000
asks): ykhost_preempt_headroom — the copies of every node per preemption level reduced on the device — against what it replaces:
preempt_reach_nodes for the ask, the reclaim planes (reclaim_table) and the free columns on the host, and the per-level quotients, the
port cut, the sums over the nodes and cell [30] in numpy.

The cluster is bench_preempt_reach.py's: bench_explain.py's nodes and asks, three more residents per node with priorities -300 / -200 /
-100, bounds (-250, -150, -50), T = 3; the asks have no priority: limit 3. The want of an ask is copies(0) + 1, so that a level is needed.
The free columns and the request vectors are read from the encoded tables ONCE, outside the timed windows (which favours the replaced
way: a caller would have to pull them again after every change of a node).

  (a) one ask                      preempt_headroom  vs  the host loop — the class representative whose copies grow most
  (b) one representative per class preempt_headroom  vs  the host loop over --baseline-asks of them
  --trace: (b) alone, with ykhost_preempt_reach for the same tasks after every call: the run for a kernel trace (k_preempt_headroom
           beside k_preempt_reach)

Host clock around calls that end in a synchronise; every timed window lasts at least --window seconds; the two ways alternate in one
process and every measurement is taken --repeats times. The cells of the two ways are compared at the timed size ("verified") before
anything is timed. Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_preempt_reach import BOUNDS, extra_residents, summary, timed  # noqa: E402

CELLS = 32


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--baseline-asks", type=int, default=8, help="class representatives the host loop is timed over in (b)")
    ap.add_argument("--trace", action="store_true", help="only (b) without the baseline, ykhost_preempt_reach beside it")
    a = ap.parse_args(argv)
    if a.nodes < 1 or a.pods < 1 or a.repeats < 5 or a.window <= 0 or a.baseline_asks < 1:
        ap.error("--nodes, --pods, --baseline-asks must be positive, --repeats at least 5, --window positive")
    return a


def cells_of(rows, below, limit, want):
    """The 32 cells from rows[L][n] = copies at level L (L = 0..limit) and below[L][n] = the node's pods in tiers < L."""
    out = np.zeros(CELLS, dtype=np.int64)
    n = np.arange(rows.shape[1])
    for L in range(9):
        at = min(L, limit)
        out[L] = rows[at].sum()
        out[9 + L] = np.count_nonzero(rows[at] >= 1)
        paid = np.argmax(rows[:at + 1] == rows[at], axis=0)   # the first level that already gives the node its level-L copies
        out[18 + L] = below[paid, n].sum()
    out[28], out[29], out[30] = limit, want, -1
    met = np.flatnonzero(out[:limit + 1] >= want)
    if len(met):
        out[30] = met[0]
    return out


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1)
    node_names = [json.loads(line)["metadata"]["name"] for line in pm.dump_documents(0).splitlines() if line]
    docs = extra_residents(node_names, np.random.default_rng(7))
    assert pm.update_pods_batch(docs) == len(docs)
    pm.set_preemption_tiers(BOUNDS)
    # the host's copy of what the replaced way divides: free[r][n], free slots[n], the request vector and the port wish of every spec
    tables = pm.encoded_tables()
    N, R, KP, S = tables["N"], tables["R"], tables["KP"], tables["S"]
    free = (np.array(tables["allocatable"], dtype=np.int64) - np.array(tables["requested"], dtype=np.int64)).reshape(R, N)
    slots = np.array(tables["allowed_pods"], dtype=np.int64) - np.array(tables["pod_count"], dtype=np.int64)
    spec_req = np.array(tables["requests"], dtype=np.int64).reshape(S, R)
    spec_port = np.array([any(tables["wanted_ports"][s * KP:(s + 1) * KP]) for s in range(S)], dtype=bool)
    pod_spec = np.array(tables["pod_spec"], dtype=np.int64)
    del tables
    pm.evaluate()  # (the class representatives come from the class build; the call itself needs no evaluation)
    _, reps = pm.pod_classes()
    reps = np.ascontiguousarray(reps[reps >= 0], dtype=np.int32)
    limit = len(BOUNDS)
    t0 = time.perf_counter()
    per_class = pm.preempt_headroom(reps)  # the first call uploads the whole reclaim table
    first_call_s = time.perf_counter() - t0
    computed = per_class[:, 27] == 0   # (a class whose copies interact through a topology constraint has no count: status 2)
    reps, per_class = reps[computed], per_class[computed]
    wants = per_class[:, 0] + 1
    assert len(reps) and (per_class[:, 28] == limit).all()
    grower = int(np.argmax(per_class[:, 3] - per_class[:, 0]))
    one, one_want = reps[grower:grower + 1], wants[grower:grower + 1]
    result = {"nodes": N, "asks": pm.num_pods, "classes": int(len(computed)), "classes_computed": int(len(reps)), "tiers": limit, "residents_added": len(docs),
              "first_call_with_table_upload_ms": round(first_call_s * 1e3, 3), "window_s": a.window}

    def baseline(asks, ask_wants):
        out = np.zeros((len(asks), CELLS), dtype=np.int64)
        for k, (p, want) in enumerate(zip(asks, ask_wants)):
            levels = pm.preempt_reach_nodes(int(p))
            req, cnt, _ = pm.reclaim_table()
            q = spec_req[pod_spec[p]]
            dims = np.flatnonzero(q > 0)
            below = np.concatenate([np.zeros((1, N), dtype=np.int64), np.cumsum(cnt, axis=0, dtype=np.int64)])
            rows = np.zeros((limit + 1, N), dtype=np.int64)
            freed = free.copy()
            for L in range(limit + 1):
                if L:
                    freed += req[L - 1]
                k0 = slots + below[L]
                for r in dims:
                    k0 = np.minimum(k0, freed[r] // q[r])
                k0 = np.maximum(k0, 1)   # (an open node takes one: its level says so)
                if spec_port[pod_spec[p]]:
                    k0 = np.minimum(k0, 1)
                rows[L] = np.where((levels >= 0) & (levels <= L), k0, 0)
            out[k] = cells_of(rows, below, limit, int(want))
        return out

    if a.trace:
        def both():
            pm.preempt_headroom(reps, wants=wants)
            pm.preempt_reach(reps)
        both()
        result["trace_b"] = summary([timed(both, a.window) for _ in range(a.repeats)])
        pm.close()
        print(json.dumps(result))
        return 0

    verified = True
    for name, asks, ask_wants, nb in (("one_ask", one, one_want, 1), ("one_per_class", reps, wants, a.baseline_asks)):
        got = pm.preempt_headroom(asks, wants=ask_wants)
        want_cells = baseline(asks[:nb], ask_wants[:nb])
        same = bool(np.array_equal(got[:nb], want_cells))
        if not same:
            bad = int(np.flatnonzero((got[:nb] != want_cells).any(axis=1))[0])
            result[name + "_first_difference"] = {"ask": int(asks[bad]), "device": got[bad].tolist(), "host_loop": want_cells[bad].tolist()}
        verified = verified and same
        t_new, t_base = [], []
        for _ in range(a.repeats):  # the two ways alternate
            t_new.append(timed(lambda: pm.preempt_headroom(asks, wants=ask_wants), a.window))
            t_base.append(timed(lambda: baseline(asks[:nb], ask_wants[:nb]), a.window))
        entry = {"asks": int(len(asks)), "preempt_headroom": summary(t_new), "baseline_asks": nb, "baseline_reach_nodes_planes_numpy": summary(t_base)}
        per_ask_base = entry["baseline_reach_nodes_planes_numpy"]["median_ms"] / nb
        entry["baseline_ms_per_ask"] = round(per_ask_base, 4)
        entry["preempt_headroom_ms_per_ask"] = round(entry["preempt_headroom"]["median_ms"] / len(asks), 6)
        entry["speedup_per_ask_median"] = round(per_ask_base / (entry["preempt_headroom"]["median_ms"] / len(asks)), 1)
        entry["faster_beyond_spread"] = bool(max(t_new) / len(asks) < min(t_base) / nb)
        entry["cells_of_the_first_ask"] = got[0].tolist()
        result[name] = entry
    result["classes_by_level_of_the_want"] = np.bincount(got[:, 30] + 1, minlength=limit + 2).tolist()   # ([0]: no level meets copies(0) + 1, [1 + L]: level L)
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified else 1


if __name__ == "__main__":
    sys.exit(main())
