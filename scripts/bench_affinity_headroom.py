#!/usr/bin/env python3
"""Cost of "how many executors with one-per-host anti-affinity still fit" at configs[2] size (50 000 nodes x 1 000 000 asks, plus
--host-asks asks with required podAntiAffinity on kubernetes.io/hostname against the pods of one of the generator's apps, which they
belong to themselves): ykpred_headroom_affinity — cap per host under the static verdict, the fill and the 16 cells on the device —
against what a host does without the call: ykpred_headroom_groups with the topology plugins masked out of the lists over the hostname id
column (cap per host and on the unlabelled nodes), a readback of the anti rows' histogram cells (layout.spread_counts), and the fill in
numpy: copies = min(cap, 1) where the cells are all 0, else 0.

  shapes   (a) one ask   (b) one ask per hostname anti-affinity class (status 0, mode 1)
  fills    the engine's choice (a workgroup per task from 256 domains on) and, for (b), YKPRED_TUNE affinity_fill_waves=1 in a second
           process (--fill-waves 1): what the workgroup form buys

Host clock around calls that end in a synchronise; every timed window lasts at least --window seconds; the two ways alternate in one
process and every measurement is taken --repeats times, so the spread is in the line. The copies per domain of the two ways are compared
for every ask at the timed size ("equal" per shape, "verified" for the run). Outside the timed windows, once: the hostname id column
from the node labels (dump_snapshot) and per ask where its anti rows lie in the histograms (ykpred_headroom_affinity_constraint) — what
a host keeps from its own encoder. No CPU path. Prints one JSON line.
--trace: (b) only, no baseline — the run for a kernel trace of k_headroom_affinity and k_affinity_fill."""
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
HOST = "kubernetes.io/hostname"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--host-asks", type=int, default=64, help="asks with hostname self anti-affinity, one class each")
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--fill-waves", type=int, default=0, help="YKPRED_TUNE affinity_fill_waves for this process (0 = the engine's choice)")
    ap.add_argument("--trace", action="store_true", help="the kernel-trace run: (b) only, no baseline")
    a = ap.parse_args(argv)
    if a.nodes < 1 or a.pods < 1 or a.templates < 0 or a.host_asks < 1:
        ap.error("--nodes, --pods and --host-asks must be positive")
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


def host_ask(k):
    """An executor of one of the generator's apps that refuses a host where a pod of that app runs, and tolerates the generator's taint."""
    app = f"app-{k % 8}"
    return {"metadata": {"name": f"host-anti-{k}", "uid": f"host-anti-{k}", "namespace": "default", "labels": {"app": app}},
            "spec": {"containers": [{"name": "main", "resources": {"requests": {"cpu": f"{100 + 50 * k}m", "memory": "128Mi"}}}],
                     "tolerations": [{"key": "kwok.x-k8s.io/node", "operator": "Exists", "effect": "NoSchedule"}],
                     "affinity": {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
                         {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": HOST}]}}}}


def main(argv=None):
    a = parse_args(argv)
    if a.fill_waves:
        os.environ["YKPRED_TUNE"] = ",".join(x for x in (os.environ.get("YKPRED_TUNE", ""), f"affinity_fill_waves={a.fill_waves}") if x)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1, spread=0)
    pm.update_pods_batch([host_ask(k) for k in range(a.host_asks)])
    P0 = pm.num_pods - a.host_asks
    asks_all = np.arange(P0, P0 + a.host_asks, dtype=np.int32)
    N = pm.num_nodes
    ALL = pkg.ALL_PLUGINS
    TOPOLOGY = pkg.PLUGIN_BITS["PodTopologySpread"] | pkg.PLUGIN_BITS["InterPodAffinity"]
    pm.headroom_affinity(asks_all[:1])  # (syncs, uploads the spec effects)

    def device(asks):
        out = np.zeros((len(asks), CELLS), dtype=np.int64)
        if pm._P.ykpred_headroom_affinity(pm.engine, len(asks), asks.ctypes.data, ALL, ALL, out.ctypes.data) != 0:
            raise RuntimeError("ykpred_headroom_affinity failed: " + pm._P.ykpred_last_error(pm.engine).decode())
        return out

    first = device(asks_all)
    if not ((first[:, 3] == 0) & (first[:, 13] == 1)).all():
        raise RuntimeError("a hostname anti-affinity ask did not come out at status 0, mode 1")
    where = np.stack([pm.headroom_affinity_constraint(int(p), pre_mask=ALL, filt_mask=ALL) for p in asks_all])
    kd = int(where[0, 1])
    values = pm.domain_values(HOST)
    G = len(values)
    if not ((where[:, 0] == 0) & (where[:, 1] == kd) & (where[:, 3] == G) & (where[:, 4] >= 1) & (where[:, 4] <= 11)).all():
        raise RuntimeError("the anti rows of an ask are not where the key's domains are")
    # the hostname id column, once, from the node labels: ids are the ranks of the sorted values, -1 = the node has no such label
    labels = [n["metadata"].get("labels", {}) for n in json.loads(pm.dump_snapshot(pods=np.zeros(1, dtype=np.int32), nodes=np.arange(N, dtype=np.int32), compact=True))["nodes"]]
    rank = {v: i for i, v in enumerate(values)}
    column = np.ascontiguousarray([rank.get(lab.get(HOST), -1) for lab in labels], dtype=np.int32)

    def baseline(asks, info):
        """cap per host by ykpred_headroom_groups without the topology plugins, the anti rows read back, the fill in numpy."""
        sums = np.zeros((len(asks), 8), dtype=np.int64)
        table = np.zeros((len(asks), G + 1, 2), dtype=np.int64)
        rc = pm._P.ykpred_headroom_groups(pm.engine, len(asks), asks.ctypes.data, None, G, column.ctypes.data, ALL & ~TOPOLOGY, ALL & ~TOPOLOGY,
                                          sums.ctypes.data, table.ctypes.data)
        if rc != 0:
            raise RuntimeError("ykpred_headroom_groups failed: " + pm._P.ykpred_last_error(pm.engine).decode())
        counts = pm.spread_tensors()[0].cpu().numpy()
        out = []
        for i in range(len(asks)):
            cnt = np.zeros(G, dtype=np.int64)
            for r in range(int(info[i, 4])):
                cnt += counts[info[i, 5 + r]:info[i, 5 + r] + G]
            copies = np.where(cnt > 0, 0, np.minimum(table[i, :G, 0], 1))
            out.append((copies, int(table[i, G, 0])))
        return out

    result = {"nodes": N, "asks": pm.num_pods, "host_asks": a.host_asks, "domains": G, "window_s": a.window, "fill_waves": a.fill_waves,
              "form": "LDS" if G <= pkg.GROUP_LDS_MAX_GROUPS else "global table"}
    verified = None
    mid = len(asks_all) // 2
    shapes = [("one_per_class", asks_all, where)] if a.trace else [("one_ask", asks_all[mid:mid + 1], where[mid:mid + 1]), ("one_per_class", asks_all, where)]
    for name, asks, info in shapes:
        got = device(asks)  # warm-up of the shape
        if a.trace:
            timed(lambda: device(asks), a.window)
            continue
        expect = baseline(asks, info)
        same = True
        for i, p in enumerate(asks):
            cells, rows, _ = pm.headroom_affinity_domains(int(p), pre_mask=ALL, filt_mask=ALL)
            copies, outside = expect[i]
            same = (same and np.array_equal(cells, got[i]) and np.array_equal(rows[:-1, 3], copies) and int(rows[-1, 3]) == outside
                    and int(copies.sum()) + outside == int(got[i, 0]))
        verified = (verified is not False) and bool(same)
        t_dev, t_base = [], []
        for _ in range(a.repeats):  # the two ways alternate
            t_dev.append(timed(lambda: device(asks), a.window))
            t_base.append(timed(lambda: baseline(asks, info), a.window))
        result[name] = {"asks": int(len(asks)), "headroom_affinity": summary(t_dev), "baseline_groups_readback_numpy": summary(t_base),
                        "ratio_baseline_over_call": round(summary(t_base)["median_ms"] / summary(t_dev)["median_ms"], 2),
                        "call_faster_beyond_spread": bool(max(t_dev) < min(t_base)), "call_slower_beyond_spread": bool(min(t_dev) > max(t_base)),
                        "equal": bool(same), "copies_total": int(got[:, 0].sum()), "blocked_total": int(got[:, 5].sum()),
                        "outside_total": int(got[:, 6].sum())}
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified is not False else 1


if __name__ == "__main__":
    sys.exit(main())
