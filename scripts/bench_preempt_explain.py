#!/usr/bin/env python3
"""Cost of "why is this ask still pending with preemption on" at configs[2] size (50 000 nodes x 1 000 000 asks): ykhost_preempt_explain —
the never nodes of preemption reach classified and their final verdicts reduced on the device — beside the two calls whose work its
kernel combines (preempt_reach and explain on the same tasks) and beside the nearest existing route to the same answer:
preempt_reach_nodes for the levels, query_pod_packed for the verdict as the node stands, ykhost_reclaim_table for the eligible pods,
and the class split in numpy. That baseline is HOST-BOUND (two per-node copies and one table copy-out per ask, then numpy over N), and
it computes LESS than the call: the levels [9] / [11], the classes [24..26], [28] and the never nodes by their code as they stand; the
final-state codes and the reason bins [12..23] and [27] of the not-enough nodes would need every node's free values as well, which no
bulk call hands out.

The cluster is bench_preempt_reach.py's: three more residents per node with priorities -300 / -200 / -100, bounds (-250, -150, -50).

  (a) one ask                      the class representative with the most not-enough nodes
  (b) one representative per class the baseline over --baseline-asks of them
  --trace: (b) alone, preempt_explain, preempt_reach and explain one after the other: the run for a kernel trace

Host clock around calls that end in a synchronise; every timed window lasts at least --window seconds; the ways alternate in one process
and every measurement is taken --repeats times. The cells the baseline computes are compared at the timed size ("verified"), and
[9], [11] and the class sum against preempt_reach. For each shape the JSON states whether the ranges of two ways are disjoint.
Prints one JSON line."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_preempt_reach import BOUNDS, extra_residents, parse_args, summary, timed  # noqa: E402

CELLS = 32
COMPARED = [9, 10, 11, 24, 25, 26, 28]   # and the sum of [0..8]


def disjoint(a, b):
    return bool(max(a) < min(b) or max(b) < min(a))


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1)
    node_names = [json.loads(line)["metadata"]["name"] for line in pm.dump_documents(0).splitlines() if line]
    docs = extra_residents(node_names, np.random.default_rng(7))
    assert pm.update_pods_batch(docs) == len(docs)
    pm.set_preemption_tiers(BOUNDS)
    pm.evaluate()  # (the class representatives come from the class build; the call itself needs no evaluation)
    _, reps = pm.pod_classes()
    reps = np.ascontiguousarray(reps[reps >= 0], dtype=np.int32)
    N = pm.num_nodes
    per_class = pm.preempt_explain(reps)  # the first call uploads the whole reclaim table
    one = reps[int(np.argmax(per_class[:, 26])):][:1]
    result = {"nodes": N, "asks": pm.num_pods, "classes": int(len(reps)), "tiers": len(BOUNDS), "window_s": a.window,
              "never_nodes_per_ask_min_max": [int(per_class[:, :9].sum(axis=1).min()), int(per_class[:, :9].sum(axis=1).max())],
              "baseline_is_host_bound": True, "baseline_cells": COMPARED}

    def baseline(asks):
        out = np.zeros((len(asks), CELLS), dtype=np.int64)
        for k, p in enumerate(asks):
            levels = pm.preempt_reach_nodes(int(p))
            stands = pm.query_pod_packed(int(p)).astype(np.int64)
            _, pods, _ = pm.reclaim_table()
            limit = len(BOUNDS)
            elig = pods[:limit].sum(axis=0)
            code = stands & 0xff
            never = levels < 0
            walked = (code == 5) | (code == 6)
            row = out[k]
            row[9], row[11] = np.count_nonzero(levels == 0), np.count_nonzero(levels >= 1)
            # the verdict of an unresolvable or a no-victims node is the one as it stands; a not-enough node's final code is 5 or 6 on
            # this cluster (no frozen plugin behind NodeResourcesFit fails): counted under the code as it stands
            row[:9] = np.bincount(code[never], minlength=9)[:9]
            row[25] = np.count_nonzero(never & ~walked)
            row[24] = np.count_nonzero(never & walked & (elig == 0))
            row[26] = np.count_nonzero(never & walked & (elig > 0))
            row[28] = elig[never & walked & (elig > 0)].sum()
        return out

    if a.trace:
        def three():
            pm.preempt_explain(reps)
            pm.preempt_reach(reps)
            pm.explain(reps)
        three()
        result["trace_b"] = summary([timed(three, a.window) for _ in range(a.repeats)])
        pm.close()
        print(json.dumps(result))
        return 0

    verified = True
    for name, asks, base_asks in (("one_ask", one, one), ("one_per_class", reps, reps[:a.baseline_asks])):
        got = pm.preempt_explain(asks)
        reach = pm.preempt_reach(asks)
        want = baseline(base_asks)
        same = got[:len(base_asks)][:, COMPARED] == want[:, COMPARED]
        verified = verified and bool(same.all()) and bool(np.array_equal(got[:len(base_asks), :9].sum(axis=1), want[:, :9].sum(axis=1)))
        verified = verified and bool(np.array_equal(got[:, 9], reach[:, 0]) and np.array_equal(got[:, 11], reach[:, 1:9].sum(axis=1))
                                     and np.array_equal(got[:, 24:27].sum(axis=1), reach[:, 9]))
        t = {"preempt_explain": [], "preempt_reach": [], "explain": [], "baseline": []}
        for _ in range(a.repeats):  # the ways alternate
            t["preempt_explain"].append(timed(lambda: pm.preempt_explain(asks), a.window))
            t["preempt_reach"].append(timed(lambda: pm.preempt_reach(asks), a.window))
            t["explain"].append(timed(lambda: pm.explain(asks), a.window))
            t["baseline"].append(timed(lambda: baseline(base_asks), a.window))
        entry = {"asks": int(len(asks)), "baseline_asks": int(len(base_asks))}
        for way, samples in t.items():
            entry[way] = summary(samples)
        per_ask = {way: [s / (len(base_asks) if way == "baseline" else len(asks)) for s in samples] for way, samples in t.items()}
        entry["baseline_ms_per_ask"] = round(sorted(per_ask["baseline"])[len(per_ask["baseline"]) // 2] * 1e3, 4)
        entry["preempt_explain_ms_per_ask"] = round(sorted(per_ask["preempt_explain"])[len(per_ask["preempt_explain"]) // 2] * 1e3, 6)
        entry["ranges_disjoint"] = {other: disjoint(per_ask["preempt_explain"], per_ask[other]) for other in ("preempt_reach", "explain", "baseline")}
        entry["cells_of_the_first_ask"] = got[0].tolist()
        result[name] = entry
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified else 1


if __name__ == "__main__":
    sys.exit(main())
