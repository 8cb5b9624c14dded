#!/usr/bin/env python3
"""Cost of "how many copies of this ask still fit" at configs[2] size (50 000 nodes x 1 000 000 asks): ykpred_headroom — per ask the
per-node replicas reduced on the device to 16 integers — against what a host has to do without it: one ykpred_query_pod_packed per
ask (4 bytes x N over PCIe and a synchronise) plus the quotient arithmetic in numpy on host copies of the node columns.

  (a) one ask                      headroom  vs  baseline
  (b) one representative per class headroom  vs  baseline loop

Same cluster, windows and alternation as bench_explain.py: host clock around calls that end in a synchronise; every timed window
lasts at least --window seconds; the two ways alternate in one process and every measurement is taken --repeats times, so the spread
is in the line. The cells of the two ways are compared at the timed size ("verified"). No CPU path: without a GPU the manager's
constructor raises. Prints one JSON line.
--only b --no-baseline --beside-explain: (b) only, with ykpred_explain called for the same tasks after every headroom call — the run
for a kernel trace that shows k_headroom beside k_explain."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELLS = 16


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--only", choices=["all", "a", "b"], default="all")
    ap.add_argument("--no-baseline", action="store_true", help="skip the query_pod_packed loop (and with it the verification)")
    ap.add_argument("--beside-explain", action="store_true", help="call ykpred_explain for the same asks after every headroom call")
    a = ap.parse_args(argv)
    if a.nodes < 1 or a.pods < 1 or a.templates < 0:
        ap.error("--nodes and --pods must be positive")
    if a.repeats < 5:
        ap.error("--repeats must be at least 5: the spread is part of the result")
    if a.window <= 0:
        ap.error("--window must be positive")
    if a.beside_explain and not a.no_baseline:
        ap.error("--beside-explain is the trace run: it goes with --no-baseline")
    return a


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
    pm.evaluate()  # (the class representatives come from the class build; headroom itself needs no evaluation)
    _, reps = pm.pod_classes()
    reps = np.ascontiguousarray(reps[reps >= 0], dtype=np.int32)
    one = reps[len(reps) // 2:len(reps) // 2 + 1]
    N = pm.layout().num_nodes
    words = np.zeros(N, dtype=np.uint32)
    engine, P = pm.engine, pm._P
    # the host's copies of the columns the quotients read (what a host without the call would keep beside the engine)
    t = pm.encoded_tables()
    R = t["R"]
    free = (np.array(t["allocatable"], dtype=np.int64) - np.array(t["requested"], dtype=np.int64)).reshape(R, N)
    slots = np.array(t["allowed_pods"], dtype=np.int64) - np.array(t["pod_count"], dtype=np.int64)
    requests = np.array(t["requests"], dtype=np.int64).reshape(-1, R)
    wants_port = np.array([w != 0 for w in t["wanted_ports"]]).reshape(len(requests), -1).any(axis=1) if t["KP"] else np.zeros(len(requests), dtype=bool)
    pod_spec = np.array(t["pod_spec"], dtype=np.int64)
    del t

    def baseline(asks):
        out = np.zeros((len(asks), CELLS), dtype=np.int64)
        for i, p in enumerate(asks):
            rc = P.ykpred_query_pod_packed(engine, int(p), pkg.ALL_PLUGINS, pkg.ALL_PLUGINS, words.ctypes.data)
            if rc != 0:
                raise RuntimeError("ykpred_query_pod_packed failed")
            fit = np.flatnonzero(words & 0x100)
            if not len(fit):
                continue
            spec = pod_spec[p]
            k = slots[fit]
            binder = np.full(len(fit), 4)
            for r in range(R - 1, -1, -1):  # (downwards: of equal quotients the lowest r stays)
                q = requests[spec, r]
                if q > 0:
                    quo = free[r, fit] // q
                    binder = np.where(quo <= k, 8 + r, binder)
                    k = np.minimum(k, quo)
            if wants_port[spec]:
                binder = np.where(k > 1, 5, binder)
                k = np.minimum(k, 1)
            out[i, 0], out[i, 1], out[i, 2] = k.sum(), len(fit), k.max()
            out[i, 4:] = np.bincount(binder, minlength=CELLS)[4:]
        return out

    shapes = {"a": ("one_ask", one), "b": ("one_per_class", reps)}
    wanted = ["a", "b"] if a.only == "all" else [a.only]
    result = {"nodes": N, "asks": pm.num_pods, "classes": int(len(reps)), "window_s": a.window}
    verified = None
    for key in wanted:
        name, asks = shapes[key]
        with_base = not a.no_baseline

        def device():
            cells = pm.headroom(asks, pre_mask=pkg.ALL_PLUGINS, filt_mask=pkg.ALL_PLUGINS)
            if a.beside_explain:
                pm.explain(asks, pre_mask=pkg.ALL_PLUGINS, filt_mask=pkg.ALL_PLUGINS)
            return cells
        got = device()  # warm-up of the shape (buffers, histogram preparation)
        if with_base:
            want = baseline(asks)
            verified = (verified is not False) and bool(np.array_equal(got, want))
        t_dev, t_base = [], []
        for _ in range(a.repeats):  # the two ways alternate
            t_dev.append(timed(device, a.window))
            if with_base:
                t_base.append(timed(lambda: baseline(asks), a.window))
        entry = {"asks": int(len(asks)), "headroom" + ("_then_explain" if a.beside_explain else ""): summary(t_dev),
                 "copies_total_median": int(np.median(got[:, 0])), "asks_that_fit_nowhere": int((got[:, 1] == 0).sum())}
        if with_base:
            entry["baseline_query_pod_packed_plus_numpy"] = summary(t_base)
            entry["speedup_median"] = round(entry["baseline_query_pod_packed_plus_numpy"]["median_ms"] / entry["headroom"]["median_ms"], 1)
            # faster by more than the run-to-run spread: the slowest headroom window against the fastest baseline window
            entry["faster_beyond_spread"] = bool(max(t_dev) < min(t_base))
        result[name] = entry
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified is not False else 1


if __name__ == "__main__":
    sys.exit(main())
