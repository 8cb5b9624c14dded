#!/usr/bin/env python3
"""Cost of "which domain still takes the gang" at configs[2] size (50 000 nodes x 1 000 000 asks): ykpred_headroom_groups — per ask the
per-node replicas summed per group on the device and reduced to 8 integers — against what a host does without it: one
ykpred_headroom_pod per ask (4 bytes x N over PCIe and a synchronise), np.bincount by group on its own copy of the column, and the
arg-max / arg-min in numpy.

  shapes   (a) one ask   (b) one representative per class
  columns  n % G for G in {16, 1024, N}: few groups (the LDS form), many, one per node (adds straight into the global table)

Same cluster, windows and alternation as bench_headroom.py: host clock around calls that end in a synchronise; every timed window lasts
at least --window seconds; the two ways alternate in one process and every measurement is taken --repeats times, so the spread is in the
line. The summaries of the two ways are compared at the timed size ("verified"). want = the copies of the median group of each ask (from
the baseline's own rows), so that the tightest-fit search has something to find. No CPU path. Prints one JSON line.
--trace: (b) only, no baseline, every G once per window with ykpred_headroom called for the same asks — the run for a kernel trace that
shows k_headroom_groups (both forms) and k_group_summary beside k_headroom."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUMMARY = 8


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape, column and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--trace", action="store_true", help="the kernel-trace run: (b) only, no baseline, ykpred_headroom beside it")
    a = ap.parse_args(argv)
    if a.nodes < 1 or a.pods < 1 or a.templates < 0:
        ap.error("--nodes and --pods must be positive")
    if a.repeats < 5:
        ap.error("--repeats must be at least 5: the spread is part of the result")
    if a.window <= 0:
        ap.error("--window must be positive")
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


def manager(pkg, a):
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1)
    pm.evaluate()  # (the class representatives come from the class build; the call itself needs no evaluation)
    return pm


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pm = manager(pkg, a)
    _, reps = pm.pod_classes()
    reps = np.ascontiguousarray(reps[reps >= 0], dtype=np.int32)
    one = reps[len(reps) // 2:len(reps) // 2 + 1]
    N = pm.layout().num_nodes
    ALL = pkg.ALL_PLUGINS
    per_node = np.zeros(N, dtype=np.int32)

    def device(m, asks, want, column, G):
        out = np.zeros((len(asks), SUMMARY), dtype=np.int64)
        rc = m._P.ykpred_headroom_groups(m.engine, len(asks), asks.ctypes.data, want.ctypes.data, G, column.ctypes.data, ALL, ALL, out.ctypes.data, None)
        if rc != 0:
            raise RuntimeError("ykpred_headroom_groups failed")
        return out

    def baseline(asks, want, column, G, status, rows_out=None):
        """headroom_nodes per ask, bincount by group, arg-max / arg-min in numpy → the same 8 cells."""
        out = np.zeros((len(asks), SUMMARY), dtype=np.int64)
        for i, p in enumerate(asks):
            if status[i] == 1:
                out[i, 0] = 1
                continue
            rc = pm._P.ykpred_headroom_pod(pm.engine, int(p), ALL, ALL, per_node.ctypes.data)
            if rc != 0:
                raise RuntimeError("ykpred_headroom_pod failed")
            if status[i] == 2:
                out[i] = (2, 0, 0, -1, 0, -1, 0, -1)
                continue
            copies = np.bincount(column, weights=per_node, minlength=G).astype(np.int64)  # (sums far below 2^53: exact)
            if rows_out is not None:
                rows_out[i] = copies
            holds = copies >= want[i]
            best = int(copies.argmax())  # (the first of equal maxima: the lowest id)
            out[i, 1], out[i, 2] = (copies >= 1).sum(), holds.sum()
            out[i, 3], out[i, 4] = (best, copies[best]) if copies[best] >= 1 else (-1, 0)
            if out[i, 2]:
                tight = int(np.where(holds, copies, np.iinfo(np.int64).max).argmin())
                out[i, 5], out[i, 6] = tight, copies[tight]
            else:
                out[i, 5] = -1
        return out

    columns = {f"G={G}": (G, np.ascontiguousarray(np.arange(N) % G, dtype=np.int32)) for G in (16, 1024, N)}
    shapes = [("one_per_class", reps)] if a.trace else [("one_ask", one), ("one_per_class", reps)]
    result = {"nodes": N, "asks": pm.num_pods, "classes": int(len(reps)), "window_s": a.window}
    verified = None
    for name, asks in shapes:
        status = pm.headroom(asks, pre_mask=ALL, filt_mask=ALL)[:, 3]
        entry = {"asks": int(len(asks))}
        for label, (G, column) in columns.items():
            # want: what the median group of the ask holds — from the baseline's own rows, outside the timed windows
            rows = np.zeros((len(asks), G), dtype=np.int64)
            ones = np.ones(len(asks), dtype=np.int64)
            if a.trace:
                want = ones
            else:
                baseline(asks, ones, column, G, status, rows)
                want = np.maximum(1, np.sort(rows, axis=1)[:, G // 2])
            got = device(pm, asks, want, column, G)  # warm-up of the shape (buffers, histogram preparation)
            if a.trace:
                pm.headroom(asks, pre_mask=ALL, filt_mask=ALL)
                timed(lambda: (device(pm, asks, want, column, G), pm.headroom(asks, pre_mask=ALL, filt_mask=ALL)), a.window)
                continue
            expect = baseline(asks, want, column, G, status)
            same = bool(np.array_equal(got, expect))
            verified = (verified is not False) and same
            t_dev, t_base = [], []
            for _ in range(a.repeats):  # the two ways alternate
                t_dev.append(timed(lambda: device(pm, asks, want, column, G), a.window))
                t_base.append(timed(lambda: baseline(asks, want, column, G, status), a.window))
            entry[label] = {"headroom_groups": summary(t_dev), "baseline_headroom_pod_plus_numpy": summary(t_base),
                            "speedup_median": round(summary(t_base)["median_ms"] / summary(t_dev)["median_ms"], 1),
                            # faster by more than the run-to-run spread: the slowest device window against the fastest baseline window
                            "faster_beyond_spread": bool(max(t_dev) < min(t_base)), "equal": same,
                            "asks_with_a_group_that_holds_want": int((got[:, 2] > 0).sum())}
        result[name] = entry
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified is not False else 1


if __name__ == "__main__":
    sys.exit(main())
