#!/usr/bin/env python3
"""Cost of "how many placeholders with a hard spread constraint still fit" at configs[2] size (50 000 nodes x 1 000 000 asks, 10 % of the
templates with one DoNotSchedule zone constraint, plus --host-asks asks with a DoNotSchedule kubernetes.io/hostname constraint of their
own): ykpred_headroom_spread — cap per domain and the fill on the device, 16 integers per ask back — against what a host does without
the call: ykpred_headroom_groups with the topology plugins masked out of the lists over the key's id column (cap per domain), a
readback of the engine's spread histograms (layout.spread_counts / spread_present), and the fill in numpy.

  keys     the zone key (16 domains: the LDS form) and kubernetes.io/hostname (one domain per node: adds straight into the global table)
  shapes   (a) one ask   (b) one representative per class whose one live constraint is a spread constraint on that key (status 0)

Host clock around calls that end in a synchronise; every timed window lasts at least --window seconds; the two ways alternate in one
process and every measurement is taken --repeats times, so the spread is in the line. The copies per domain of the two ways are compared
for every ask at the timed size ("equal" per shape, "verified" for the run). Outside the timed windows, once: the key's id column from
the node labels (dump_snapshot) and per ask where its constraint's row lies in the histograms (ykpred_headroom_spread_constraint) —
what a host keeps from its own encoder. No CPU path. Prints one JSON line.
--trace: (b) only, no baseline — the run for a kernel trace that shows both forms of k_headroom_spread and k_spread_fill."""
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
ZONE, HOST = "topology.kubernetes.io/zone", "kubernetes.io/hostname"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--host-asks", type=int, default=64, help="asks with a hostname spread constraint, one class each")
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
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
    """An ask that spreads over hosts among the pods of one of the generator's apps, and tolerates the generator's node taint."""
    app = f"app-{k % 8}"
    return {"metadata": {"name": f"host-spread-{k}", "uid": f"host-spread-{k}", "namespace": "default", "labels": {"app": app}},
            "spec": {"containers": [{"name": "main", "resources": {"requests": {"cpu": f"{100 + 50 * k}m", "memory": "128Mi"}}}],
                     "tolerations": [{"key": "kwok.x-k8s.io/node", "operator": "Exists", "effect": "NoSchedule"}],
                     "topologySpreadConstraints": [{"maxSkew": 1 + k % 3, "topologyKey": HOST, "whenUnsatisfiable": "DoNotSchedule",
                                                    "labelSelector": {"matchLabels": {"app": app}}}]}}


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1, spread=1)
    pm.update_pods_batch([host_ask(k) for k in range(a.host_asks)])
    pm.evaluate()  # (the class representatives come from the class build; the call itself needs no evaluation)
    _, reps = pm.pod_classes()
    reps = np.ascontiguousarray(reps[reps >= 0], dtype=np.int32)
    N = pm.layout().num_nodes
    ALL = pkg.ALL_PLUGINS
    TOPOLOGY = pkg.PLUGIN_BITS["PodTopologySpread"] | pkg.PLUGIN_BITS["InterPodAffinity"]

    def device(asks):
        out = np.zeros((len(asks), CELLS), dtype=np.int64)
        if pm._P.ykpred_headroom_spread(pm.engine, len(asks), asks.ctypes.data, ALL, ALL, out.ctypes.data) != 0:
            raise RuntimeError("ykpred_headroom_spread failed")
        return out

    computed = np.ascontiguousarray(reps[device(reps)[:, 3] == 0])
    where = np.stack([pm.headroom_spread_constraint(int(p), pre_mask=ALL, filt_mask=ALL) for p in computed])
    keys = pm.encoded_tables()["topology_keys"]
    # the id column of each key, once, from the node labels: ids are the ranks of the sorted values, -1 = the node has no such label
    labels = [n["metadata"].get("labels", {}) for n in json.loads(pm.dump_snapshot(pods=np.zeros(1, dtype=np.int32), nodes=np.arange(N, dtype=np.int32), compact=True))["nodes"]]
    result = {"nodes": N, "asks": pm.num_pods, "classes": int(len(reps)), "window_s": a.window}
    verified = None

    def baseline(asks, info, column, G):
        """cap per domain by ykpred_headroom_groups without the topology plugins, the histograms read back, the fill in numpy."""
        sums = np.zeros((len(asks), 8), dtype=np.int64)
        table = np.zeros((len(asks), G + 1, 2), dtype=np.int64)
        rc = pm._P.ykpred_headroom_groups(pm.engine, len(asks), asks.ctypes.data, None, G, column.ctypes.data, ALL & ~TOPOLOGY, ALL & ~TOPOLOGY,
                                          sums.ctypes.data, table.ctypes.data)
        if rc != 0:
            raise RuntimeError("ykpred_headroom_groups failed")
        counts, present = pm.spread_tensors()
        counts, present = counts.cpu().numpy(), present.cpu().numpy()
        out = []
        for i in range(len(asks)):
            _, _, off, D, skew, min_domains, self_match, _ = info[i]
            cnt, here, cap = counts[off:off + D].astype(np.int64), present[off:off + D] != 0, table[i, :G, 0]
            ruled = here.sum() >= max(min_domains, 1)  # (enough present domains: the minimum over them is the floor, else 0)
            if self_match:
                floor = int((cnt + cap)[here].min()) if ruled else 0
                out.append(np.clip(floor + skew - cnt, 0, cap))
            else:
                floor = int(cnt[here].min()) if ruled else 0
                out.append(np.where(cnt - floor <= skew, cap, 0))
        return out

    for key in (ZONE, HOST):
        kd = keys.index(key)
        values = pm.domain_values(key)
        rank = {v: i for i, v in enumerate(values)}
        column = np.ascontiguousarray([rank.get(lab.get(key), -1) for lab in labels], dtype=np.int32)
        G = len(values)
        mine = where[:, 1] == kd
        asks_all, info_all = np.ascontiguousarray(computed[mine]), where[mine]
        if len(asks_all) == 0:
            raise RuntimeError(f"no class with one hard spread constraint on {key}")
        if not (info_all[:, 3] == G).all():
            raise RuntimeError("the key's domains differ from the histogram row's")
        mid = len(asks_all) // 2
        entry = {"domains": G, "form": "LDS" if G <= pkg.GROUP_LDS_MAX_GROUPS else "global table"}
        for name, asks, info in ([("one_per_spread_class", asks_all, info_all)] if a.trace else
                                 [("one_ask", asks_all[mid:mid + 1], info_all[mid:mid + 1]), ("one_per_spread_class", asks_all, info_all)]):
            got = device(asks)  # warm-up of the shape
            if a.trace:
                timed(lambda: device(asks), a.window)
                continue
            expect = baseline(asks, info, column, G)
            same = True
            for i, p in enumerate(asks):
                cells, rows, _ = pm.headroom_spread_domains(int(p), pre_mask=ALL, filt_mask=ALL)
                same = same and np.array_equal(cells, got[i]) and np.array_equal(rows[:, 3], expect[i]) and int(expect[i].sum()) == int(got[i, 0])
            verified = (verified is not False) and bool(same)
            t_dev, t_base = [], []
            for _ in range(a.repeats):  # the two ways alternate
                t_dev.append(timed(lambda: device(asks), a.window))
                t_base.append(timed(lambda: baseline(asks, info, column, G), a.window))
            entry[name] = {"asks": int(len(asks)), "headroom_spread": summary(t_dev), "baseline_groups_readback_numpy": summary(t_base),
                           "ratio_baseline_over_call": round(summary(t_base)["median_ms"] / summary(t_dev)["median_ms"], 2),
                           "call_faster_beyond_spread": bool(max(t_dev) < min(t_base)), "call_slower_beyond_spread": bool(min(t_dev) > max(t_base)),
                           "equal": bool(same), "copies_total": int(got[:, 0].sum()), "cap_total": int(got[:, 4].sum())}
        result["zone" if key == ZONE else "hostname"] = entry
    result["verified"] = verified
    pm.close()
    print(json.dumps(result))
    return 0 if verified is not False else 1


if __name__ == "__main__":
    sys.exit(main())
