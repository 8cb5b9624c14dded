#!/usr/bin/env python3
"""Cost of "why does this ask fit nowhere" at configs[2] size (50 000 nodes x 1 000 000 asks): ykpred_explain — the per-ask
histogram of verdicts reduced on the device — against the only way there was before it, one ykpred_query_pod_packed per ask
(4 bytes x N over PCIe and a synchronise) plus np.bincount on the host.

  (a) one ask                      explain  vs  baseline
  (b) one representative per class explain  vs  baseline loop
  (c) all asks                     explain only

Host clock around calls that end in a synchronise; every timed window lasts at least --window seconds (the call is repeated
inside it); the two ways alternate in one process and every measurement is taken --repeats times, so the spread is in the line.
The bins of the two ways are compared at the timed size ("verified"). No CPU path: without a GPU the manager's constructor raises.
Prints one JSON line.  --only b --no-baseline: just (b), for a kernel trace of its own."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = 32


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--only", choices=["all", "a", "b", "c"], default="all")
    ap.add_argument("--no-baseline", action="store_true", help="skip the query_pod_packed loop (and with it the verification)")
    a = ap.parse_args(argv)
    if a.nodes < 1 or a.pods < 1 or a.templates < 0:
        ap.error("--nodes and --pods must be positive")
    if a.repeats < 5:
        ap.error("--repeats must be at least 5: the spread is part of the result")
    if a.window <= 0:
        ap.error("--window must be positive")
    return a


def bins_of_packed(words):
    """ykpred_query_pod_packed's word per node -> the 32 bins of ykpred_explain."""
    c = np.bincount(words & 0x1ff, minlength=512)  # plugin code | fit << 8
    out = np.zeros(BINS, dtype=np.int32)
    out[:9] = c[:9]
    out[9] = c[256:].sum()
    out[10] = c[255]
    r = words >> 9
    if r.any():
        for b in range(12):
            out[12 + b] = np.count_nonzero(r & (1 << b))
    return out


def timed(fn, window):
    """Seconds per call over a window of at least `window` seconds."""
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


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1)
    pm.evaluate()  # (the class representatives come from the class build; explain itself needs no evaluation)
    _, reps = pm.pod_classes()
    reps = np.ascontiguousarray(reps[reps >= 0], dtype=np.int32)
    one = reps[len(reps) // 2:len(reps) // 2 + 1]
    N = pm.layout().num_nodes
    words = np.zeros(N, dtype=np.uint32)
    engine, P = pm.engine, pm._P

    def baseline(asks):
        out = np.zeros((len(asks), BINS), dtype=np.int32)
        for k, p in enumerate(asks):
            rc = P.ykpred_query_pod_packed(engine, int(p), pkg.ALL_PLUGINS, pkg.ALL_PLUGINS, words.ctypes.data)
            if rc != 0:
                raise RuntimeError("ykpred_query_pod_packed failed")
            out[k] = bins_of_packed(words)
        return out

    shapes = {"a": ("one_ask", one), "b": ("one_per_class", reps), "c": ("all_asks", None)}
    wanted = ["a", "b", "c"] if a.only == "all" else [a.only]
    result = {"nodes": N, "asks": pm.num_pods, "classes": int(len(reps)), "window_s": a.window}
    verified = None
    for key in wanted:
        name, asks = shapes[key]
        with_base = asks is not None and not a.no_baseline
        got = pm.explain(asks)  # warm-up of the shape (buffers, histogram preparation)
        if with_base:
            want = baseline(asks)
            verified = (verified is not False) and bool(np.array_equal(got, want))
        t_explain, t_base = [], []
        for _ in range(a.repeats):  # the two ways alternate
            t_explain.append(timed(lambda: pm.explain(asks), a.window))
            if with_base:
                t_base.append(timed(lambda: baseline(asks), a.window))
        entry = {"asks": int(pm.num_pods if asks is None else len(asks)), "explain": summary(t_explain)}
        if with_base:
            entry["baseline_query_pod_packed_loop"] = summary(t_base)
            entry["speedup_median"] = round(entry["baseline_query_pod_packed_loop"]["median_ms"] / entry["explain"]["median_ms"], 1)
            # faster by more than the run-to-run spread: the slowest explain window against the fastest baseline window
            entry["faster_beyond_spread"] = bool(max(t_explain) < min(t_base))
        result[name] = entry
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified is not False else 1


if __name__ == "__main__":
    sys.exit(main())
