#!/usr/bin/env python3
"""Cost of a preemption round with LIVE topology histograms at configs[2] size (50 000 nodes x 1 000 000 asks, 10 % of the templates
with one DoNotSchedule zone-spread constraint): ykhost_preempt_round_live_by_keys — the whole list planned on the device in one call,
coupled asks included, nothing changed — against the host loop it replaces, per ask: ykhost_preempt_victims_by_key (and, for an ask
that fits somewhere as the cluster stands, ykhost_preempt_victims_nodes for the first node at need 0), ykhost_remove_pod for each
victim, ykhost_assume_pod — after which the topology histograms are rebuilt on the device at the next ask.

Two clusters, both bench_preempt_round.py's with the generator's spread templates switched on (--residents 3 or 32 tiered residents
per node, T = 3; every ask has limit 3, so any order is non-increasing):
  plain    as it is: most asks fit some node as it stands
  starved  every node with memory left gets one more tier-0 resident that requests exactly that memory: no ask fits anywhere as the
           cluster stands
Shapes, on each cluster:
  zone_gang             --gang DISTINCT asks of the zone-spread class with the most members
  one_per_spread_class  the representative of every class whose verdicts read the topology histograms
  host_gang             --gang DISTINCT asks of one template with a required anti-affinity term against its own label on
                        kubernetes.io/hostname ("one per host"), added to the generator's asks
The loop CHANGES the cluster, so every repeat builds both clusters afresh, the round timed on the same asks just before the loop in a
window of at least --window seconds. Node and victims of every ask are compared between the two ways in every repeat ("verified").
  --trace: one build of each cluster, the rounds alone, for a kernel trace (k_preempt_round_effects, k_preempt_round_topo).
Prints one JSON line; --out FILE also merges it into FILE (profiles/preempt_round_live_bench.json is made of such runs)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_preempt_round import host_loop  # noqa: E402
from bench_preempt_victims import BOUNDS, PRIORITIES, extra_residents, summary, timed  # noqa: E402

HOST = "kubernetes.io/hostname"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--templates", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5, help="measurements per shape and way (>= 5)")
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window of the round")
    ap.add_argument("--gang", type=int, default=256)
    ap.add_argument("--residents", type=int, default=3, help="tiered residents added per node (>= 3), split over the three tiers")
    ap.add_argument("--trace", action="store_true", help="only the rounds, no loop")
    ap.add_argument("--out", help="a JSON file: the result is merged into it under [trace_]residents_<K>")
    a = ap.parse_args(argv)
    if a.nodes < 1 or a.pods < 1 or a.repeats < 5 or a.window <= 0 or a.gang < 1 or a.residents < 3:
        ap.error("--nodes, --pods, --gang must be positive, --repeats at least 5, --window positive")
    return a


def host_gang_ask(k):
    """One copy of the "one per host" gang: every copy is a pod of its own with the same template."""
    return json.dumps({"metadata": {"name": f"solo-{k:05d}", "uid": f"solo-{k:05d}", "namespace": "default", "labels": {"app": "solo"}},
                       "spec": {"priority": BOUNDS[-1],
                                "containers": [{"name": "main", "resources": {"requests": {"cpu": "250m", "memory": "256Mi"}}}],
                                "tolerations": [{"key": "kwok.x-k8s.io/node", "operator": "Exists", "effect": "NoSchedule"}],
                                "affinity": {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
                                    {"labelSelector": {"matchLabels": {"app": "solo"}}, "topologyKey": HOST}]}}}}).encode()


def build(pkg, a, docs, starved):
    pm = pkg.GpuPredicateManager()  # raises without a GPU
    pm.generate_kwok(seed=0x59554E49 + 2, num_nodes=a.nodes, num_pods=a.pods, num_templates=a.templates, node_affinity=1, spread=1)
    node_names = [json.loads(line)["metadata"]["name"] for line in pm.dump_documents(0).splitlines() if line]
    if "residents" not in docs:
        docs["residents"] = extra_residents(node_names, a.residents, np.random.default_rng(7))
    assert pm.update_pods_batch(docs["residents"]) == len(docs["residents"])
    fillers = 0
    if starved:
        if "fillers" not in docs:
            t = pm.encoded_tables()
            N = t["N"]
            free = np.array(t["allocatable"][N:2 * N], dtype=np.int64) - np.array(t["requested"][N:2 * N], dtype=np.int64)   # (row 1: memory)
            docs["fillers"] = [json.dumps({"metadata": {"name": f"fill-{n}", "uid": f"fill-{n}", "namespace": "bench", "labels": {"app": "fill"}},
                                           "spec": {"nodeName": node_names[n], "priority": PRIORITIES[0],
                                                    "containers": [{"name": "c", "resources": {"requests": {"memory": str(int(free[n]))}}}]},
                                           "status": {"phase": "Running"}}).encode() for n in range(N) if free[n] > 0]
        fillers = len(docs["fillers"])
        assert pm.update_pods_batch(docs["fillers"]) == fillers
    pm.update_pods_batch([host_gang_ask(k) for k in range(a.gang)])
    pm.set_preemption_tiers(BOUNDS)
    pm.evaluate()  # (the classes come from the class build; the round itself needs no evaluation)
    return pm, node_names, fillers


def shapes_of(pm, pkg, a):
    """→ {shape: uids}. The generator's uids are pod-<index>; a class is coupled when ykpred_headroom says so (status 2)."""
    pod_class, reps = pm.pod_classes()
    classes = np.flatnonzero(reps >= 0)
    status = pm.headroom(np.ascontiguousarray(reps[classes], dtype=np.int32))[:, pkg.HEADROOM_STATUS]
    order = np.argsort(pod_class, kind="stable")
    starts = np.searchsorted(pod_class[order], np.arange(len(reps) + 1))
    uid_of = lambda i: f"pod-{int(i):07d}" if i < a.pods else f"solo-{int(i) - a.pods:05d}"   # noqa: E731
    solo = int(pod_class[pm.pod_index("solo-00000")])
    coupled = [k for k in np.flatnonzero(status == 2) if classes[k] != solo]
    assert coupled, "no zone-spread class: was the generator's spread option on?"
    sizes = starts[classes + 1] - starts[classes]
    k = max(coupled, key=lambda j: sizes[j])
    c = classes[k]
    gang = [i for i in order[starts[c]:starts[c + 1]] if i != reps[c]][:a.gang]
    return {"zone_gang": [uid_of(i) for i in gang], "one_per_spread_class": [uid_of(reps[classes[j]]) for j in coupled],
            "host_gang": [f"solo-{k:05d}" for k in range(a.gang)]}


def main(argv=None):
    a = parse_args(argv)
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    docs, result, times = {}, {"window_s": a.window, "residents_per_node": a.residents}, {}
    verified = True
    for r in range(1 if a.trace else a.repeats):
        for cluster in ("plain", "starved"):
            pm, node_names, fillers = build(pkg, a, docs, cluster == "starved")
            shapes = shapes_of(pm, pkg, a)
            result.update(nodes=pm.num_nodes, asks=pm.num_pods, tiers=len(BOUNDS))
            result.setdefault(cluster, {}).update(fillers=fillers)
            for name, uids in shapes.items():
                t_round, t_loop = times.setdefault((cluster, name), ([], []))
                cells, tally, nodes, victims = pm.preempt_round_live_by_keys(uids)
                for _ in range(4 if a.trace else 1):
                    t_round.append(timed(lambda: pm.preempt_round_live_by_keys(uids), a.window))
                entry = result[cluster].setdefault(name, {"asks": len(uids)})
                entry["round_summary"] = tally.tolist()   # (asks per outcome 0..4, victims in all, distinct nodes, histogram steps)
                entry["frozen_round_differs"] = bool(not np.array_equal(pm.preempt_round_by_keys(uids)[0], cells))
                if a.trace:
                    continue
                t0 = time.perf_counter()
                plan = host_loop(pm, pkg, uids, node_names)
                t_loop.append(time.perf_counter() - t0)
                same = plan == list(zip(nodes, victims))
                entry["equal_plans"] = bool(entry.get("equal_plans", True) and same)
                verified = verified and same
            pm.close()
    for (cluster, name), (t_round, t_loop) in times.items():
        entry = result[cluster][name]
        entry["round"] = summary(t_round)
        if not a.trace:
            entry["host_loop"] = summary(t_loop)
            entry["speedup_median"] = round(entry["host_loop"]["median_ms"] / entry["round"]["median_ms"], 2)
            entry["ranges_disjoint"] = bool(max(t_round) < min(t_loop) or min(t_round) > max(t_loop))
            entry["round_faster"] = bool(entry["round"]["median_ms"] < entry["host_loop"]["median_ms"])
            entry["round_ms_per_ask"] = round(entry["round"]["median_ms"] / entry["asks"], 5)
            entry["loop_ms_per_ask"] = round(entry["host_loop"]["median_ms"] / entry["asks"], 5)
    result["verified"] = verified
    print(json.dumps(result))
    if a.out:
        merged = json.load(open(a.out)) if os.path.exists(a.out) else {}
        merged[("trace_" if a.trace else "") + f"residents_{a.residents}"] = result
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
    return 0 if verified else 1


if __name__ == "__main__":
    sys.exit(main())
