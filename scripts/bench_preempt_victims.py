#!/usr/bin/env python3
"""Cost of "the shortest victim prefix on every node" at configs[2] size (50 000 nodes x 1 000 000 asks): ykhost_preempt_victims — need
of every node bisected on the device from the resident victim table and reduced there — against what it replaces, one
PreemptionPredicates query per node for the same ask with order(n) as victims (ykhost_preemption_predicates_batch: the victims' uids
looked up and their request vectors uploaded again for every ask), ykpred_query_pod_packed for need 0, and the reduction to the 16 cells
in numpy.

The cluster is bench_preempt_reach.py's; every node gets --residents more pods through update_pods_batch (3: one per tier, a bisection of
at most two steps; 32: ten, ten and twelve per tier, five steps), with priorities -300 / -200 / -100 and requests that over-commit every
fourth node, and the bounds (-250, -150, -50) cut them into three tiers (the generated residents have no priority: tier none; the asks
have none either: limit 3).

  (a) one ask                      victims  vs  the batch loop — the class representative with the most nodes at need >= 1
  (b) one representative per class victims  vs  the batch loop over --baseline-asks of them
  --trace: (b) alone, with ykpred_preempt_reach for the same tasks after every call: the run for a kernel trace (k_preempt_victims
           beside k_preempt_reach)

Host clock around calls that end in a synchronise; every timed window lasts at least --window seconds; the two ways alternate in one
process and every measurement is taken --repeats times. The cells of the two ways are compared at the timed size ("verified").
Prints one JSON line."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = 16
BOUNDS = (-250, -150, -50)
PRIORITIES = (-300, -200, -100)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--baseline-asks", type=int, default=8, help="class representatives the batch loop is timed over in (b)")
    ap.add_argument("--residents", type=int, default=3, help="tiered residents added per node (>= 3), split over the three tiers")
    ap.add_argument("--trace", action="store_true", help="only (b) without the baseline, ykpred_preempt_reach beside it")
    a = ap.parse_args(argv)
    if a.nodes < 1 or a.pods < 1 or a.repeats < 5 or a.window <= 0 or a.baseline_asks < 1 or a.residents < 3:
        ap.error("--nodes, --pods, --baseline-asks must be positive, --repeats at least 5, --window positive")
    return a


def timed(fn, window):
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= window:
            return dt / calls


def summary(samples):
    s = sorted(samples)
    med = s[len(s) // 2]
    return {"median_ms": round(med * 1e3, 4), "min_ms": round(s[0] * 1e3, 4), "max_ms": round(s[-1] * 1e3, 4),
            "spread_pct": round((s[-1] - s[0]) / med * 100, 1), "n": len(s)}


def tier_counts(K):
    return (K // 3, K // 3, K - 2 * (K // 3))


def uid_of(t, n, i):
    return f"tier{t}-{n}-{i:02d}"


def extra_residents(node_names, K, rng):
    """K residents per node over the three tiers, uids ascending inside a tier (so order(n) is tier, then i); the requests are scaled by
    3 / K, so a node carries the same load whatever K; every fourth node gets large ones (over-committed until victims go)."""
    docs = []
    for n, name in enumerate(node_names):
        for t, i, prio in ((t, i, prio) for t, prio in enumerate(PRIORITIES) for i in range(tier_counts(K)[t])):
            cpu = max(int(rng.integers(200, 900)) * (8 if n % 4 == 0 else 1) * 3 // K, 1)
            mem = max((int(rng.integers(1, 8)) << (33 if n % 4 == 0 else 28)) * 3 // K, 1)
            uid = uid_of(t, n, i)
            docs.append(json.dumps({"metadata": {"name": uid, "uid": uid, "namespace": "bench", "labels": {"app": "tiered"}},
                                    "spec": {"nodeName": name, "priority": prio,
                                             "containers": [{"name": "c", "resources": {"requests": {"cpu": f"{cpu}m", "memory": str(mem)}}}]},
                                    "status": {"phase": "Running"}}).encode())
    return docs


def cells_of(needs, levels, limit):
    """The 16 cells from per-node needs (-1 = never) and the levels of the needs >= 1 — the numpy side of the baseline."""
    out = np.zeros(CELLS, dtype=np.int64)
    out[0], out[1], out[2] = np.count_nonzero(needs == 0), np.count_nonzero(needs >= 1), np.count_nonzero(needs < 0)
    out[4] = limit
    out[6] = -1
    opened = np.flatnonzero(needs >= 1)
    if len(opened):
        key = (levels[opened].astype(np.int64) << 59) | (needs[opened].astype(np.int64) << 31) | opened
        best = opened[np.argmin(key)]
        out[5], out[6], out[7] = levels[best], best, needs[best]
        out[8] = needs[opened].sum()
    return out


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1)
    node_names = [json.loads(line)["metadata"]["name"] for line in pm.dump_documents(0).splitlines() if line]
    t0 = time.perf_counter()
    docs = extra_residents(node_names, a.residents, np.random.default_rng(7))
    assert pm.update_pods_batch(docs) == len(docs)
    ingest_s = time.perf_counter() - t0
    pm.set_preemption_tiers(BOUNDS)
    pm.evaluate()  # (the class representatives come from the class build; the reach call itself needs no evaluation)
    _, reps = pm.pod_classes()
    reps = np.ascontiguousarray(reps[reps >= 0], dtype=np.int32)
    N = pm.num_nodes
    t0 = time.perf_counter()
    pm.preempt_reach(reps)  # (the reclaim table goes up here: the victims call below pays for the victim table alone)
    t0 = time.perf_counter()
    per_class = pm.preempt_victims(reps)  # the first call derives and uploads the whole victim table
    first_call_s = time.perf_counter() - t0
    # "one ask" is the class representative with the most nodes at need >= 1: the ask whose lanes bisect most
    walker = int(np.argmax(per_class[:, 1]))
    one = reps[walker:walker + 1]
    K, counts = a.residents, tier_counts(a.residents)
    result = {"nodes": N, "asks": pm.num_pods, "classes": int(len(reps)), "tiers": len(BOUNDS), "residents_per_node": K, "residents_added": len(docs),
              "ingest_s": round(ingest_s, 3), "first_call_with_table_derived_and_uploaded_ms": round(first_call_s * 1e3, 3), "window_s": a.window}

    # the baseline's inputs, built once: query q = (ask, node q) with order(q) — the node's K tiered residents by (priority, uid)
    uids = (C.c_char_p * (K * N))(*[uid_of(t, n, i).encode() for n in range(N) for t in range(3) for i in range(counts[t])])
    nodes = np.arange(N, dtype=np.int32)
    off = np.arange(0, K * N + 1, K, dtype=np.int32)
    start = np.zeros(N, dtype=np.int32)
    index = np.zeros(N, dtype=np.int32)
    words = np.zeros(N, dtype=np.uint32)

    def baseline(asks):
        out = np.zeros((len(asks), CELLS), dtype=np.int64)
        for k, p in enumerate(asks):
            pods = np.full(N, int(p), dtype=np.int32)
            rc = pm._L.ykhost_preemption_predicates_batch(pm._h, N, pods.ctypes.data, nodes.ctypes.data, off.ctypes.data, uids, start.ctypes.data, index.ctypes.data)
            if rc != 0:
                raise RuntimeError("ykhost_preemption_predicates_batch failed")
            rc = pm._P.ykpred_query_pod_packed(pm.engine, int(p), pkg.ALL_PLUGINS, pkg.ALL_PLUGINS, words.ctypes.data)  # level 0 = fits as it stands
            if rc != 0:
                raise RuntimeError("ykpred_query_pod_packed failed")
            fit = (words >> 8) & 1
            needs = np.where(fit == 1, 0, np.where(index < 0, -1, index + 1)).astype(np.int64)
            levels = 1 + (needs > counts[0]) + (needs > counts[0] + counts[1])   # (the tier of victim need - 1, plus one)
            out[k] = cells_of(needs, levels, len(BOUNDS))
        return out

    if a.trace:
        def both():
            pm.preempt_victims(reps)
            pm.preempt_reach(reps)
        both()
        result["trace_b"] = summary([timed(both, a.window) for _ in range(a.repeats)])
        pm.close()
        print(json.dumps(result))
        return 0

    verified = True
    for name, asks, base_asks in (("one_ask", one, one), ("one_per_class", reps, reps[:a.baseline_asks])):
        got = pm.preempt_victims(asks)
        want = baseline(base_asks)
        verified = verified and bool(np.array_equal(got[:len(base_asks)], want))
        t_reach, t_base = [], []
        for _ in range(a.repeats):  # the two ways alternate
            t_reach.append(timed(lambda: pm.preempt_victims(asks), a.window))
            t_base.append(timed(lambda: baseline(base_asks), a.window))
        entry = {"asks": int(len(asks)), "victims": summary(t_reach), "baseline_asks": int(len(base_asks)),
                 "baseline_preemption_batch_per_node": summary(t_base)}
        per_ask_base = entry["baseline_preemption_batch_per_node"]["median_ms"] / len(base_asks)
        entry["baseline_ms_per_ask"] = round(per_ask_base, 4)
        entry["victims_ms_per_ask"] = round(entry["victims"]["median_ms"] / len(asks), 6)
        entry["speedup_per_ask_median"] = round(per_ask_base / (entry["victims"]["median_ms"] / len(asks)), 1)
        entry["faster_beyond_spread"] = bool(max(t_reach) / len(asks) < min(t_base) / len(base_asks))
        entry["cells_of_the_first_ask"] = got[0, :9].tolist()  # (need 0, need >= 1, never, status, limit, best level / node / need, sum of need)
        result[name] = entry
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified else 1


if __name__ == "__main__":
    sys.exit(main())
