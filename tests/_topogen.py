"""Designed clusters (Kubernetes-JSON snapshots) for the two plugins whose verdict on one (ask, node) pair depends on EVERY node —
PodTopologySpread and InterPodAffinity — and a plain model of their rules.

Independent of the product's generators and of `_gen.py`'s palettes: `random.Random(seed)` only, node names from
`_ordergen.node_names`, existing pods with chosen counts through the snapshot format's "replicas" field. Where `_gen.rand_spread`
draws maxSkew from {1, 2, 3} against zone counts in the tens (so that the skew comparison hardly decides a verdict), the populations
here put counts EXACTLY at the thresholds:

  skew_ladder(...)   8 zones whose counts lie B + {0, 1, 63, 64, 65, 1000, 4095, 4200}; ask k carries maxSkew k + 1: thousands of
                     distinct (constraints, self-match) signatures, a closed form for every bit
  policies(...)      sibling templates that differ in exactly ONE attribute (maxSkew s / s + 1, minDomains D / D + 1, the two
                     inclusion policies, one constraint / two, self-match, selector forms, namespace, matchLabelKeys)
  hostname(...)      one domain per node: the unique minimum on the first and the last node, on either side of a wavefront boundary in
                     node order and on either side of a 64-lane stride in the order of the histogram's cells
  interpod(...)      required affinity (one term, two terms, the "no match anywhere" escape), anti-affinity, the symmetry rule,
                     namespaces lists, nodes without the key, a template that fails both plugins

Each returns (snapshot, meta). meta names every sibling pair ("pairs": (rule, uid, uid, visible under the full plugin list)), the
templates whose rows are equal by design ("same"), the rows that are constant by design ("degenerate") and the designed properties.

model(snapshot, meta, plugins) states the rules of SURVEY.md §A (A.6 for PodTopologySpread; the comment above constraints_fail and
the upstream functions it names for InterPodAffinity) in numpy, ONE histogram per template — affordable at any size. The verdicts
are written from the rules. Two of its outputs are not: "signatures" and "sums" count the histograms of the templates that ask
the same of the same nodes only once, so that they can be held against the engine's spread_tensors(); the key they use (maxSkew,
minDomains, self-match, the two policies, which nodes are eligible) restates the one the engine de-duplicates by in set_specs, not
anything in §A.6. The model imports nothing from the package and nothing from the oracle."""
import json
import random

import numpy as np

from _ordergen import node_names

HOST = "kubernetes.io/hostname"
INT32_MAX = 2147483647
PLUGINS = ("NodeUnschedulable", "NodeName", "TaintToleration", "NodeAffinity", "NodePorts", "NodeResourcesFit", "PodTopologySpread",
           "InterPodAffinity")
CODE = {name: k + 1 for k, name in enumerate(PLUGINS)}
SPREAD, INTERPOD = CODE["PodTopologySpread"], CODE["InterPodAffinity"]
# NewPredicateManager's reservation lists (predicate_manager.go:321-368), restricted to the plugins of this path
RESERVE = (("NodeAffinity", "NodePorts", "PodTopologySpread", "InterPodAffinity"),
           ("NodeUnschedulable", "NodeName", "TaintToleration", "NodeAffinity", "NodePorts", "PodTopologySpread", "InterPodAffinity"))
TAINT_X = {"key": "dedicated", "value": "x", "effect": "NoSchedule"}
TOL_X = {"key": "dedicated", "operator": "Equal", "value": "x", "effect": "NoSchedule"}
WEB = {"matchLabels": {"app": "web"}}


# ---- snapshot pieces ---------------------------------------------------------------------------------------------------------
def make_node(name, labels, taints=(), hostname=True):
    labels = dict(labels)
    if hostname:
        labels[HOST] = name
    return {"metadata": {"name": name, "labels": labels}, "spec": {"taints": list(taints), "unschedulable": False},
            "status": {"allocatable": {"cpu": "64", "memory": "256Gi", "pods": "100000"}}, "pods": []}


def resident(uid, labels, ns="default", replicas=1, terminating=False, anti=None):
    meta = {"name": uid, "uid": uid, "namespace": ns, "labels": dict(labels)}
    if terminating:
        meta["deletionTimestamp"] = "2026-01-01T00:00:00Z"
    spec = {"containers": [{"name": "c", "resources": {"requests": {}}}]}
    if anti:
        spec["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": list(anti)}}
    out = {"metadata": meta, "spec": spec}
    if replicas != 1:
        out["replicas"] = replicas
    return out


def make_ask(uid, labels, ns="default", spread=None, affinity=None, anti=None, node_selector=None, tolerations=None):
    spec = {"containers": [{"name": "main", "resources": {"requests": {}}}]}
    if spread:
        spec["topologySpreadConstraints"] = list(spread)
    if affinity or anti:
        a = {}
        if affinity:
            a["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": list(affinity)}
        if anti:
            a["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": list(anti)}
        spec["affinity"] = a
    if node_selector:
        spec["nodeSelector"] = dict(node_selector)
    if tolerations:
        spec["tolerations"] = list(tolerations)
    return {"metadata": {"name": uid, "uid": uid, "namespace": ns, "labels": dict(labels)}, "spec": spec}


def constraint(key, max_skew, selector=WEB, **more):
    """One DoNotSchedule constraint; selector=None leaves labelSelector out (a nil selector matches nothing)."""
    c = {"maxSkew": max_skew, "topologyKey": key, "whenUnsatisfiable": "DoNotSchedule"}
    if selector is not None:
        c["labelSelector"] = selector
    c.update(more)
    return c


def term(app, key, namespaces=None):
    t = {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": key}
    if namespaces is not None:
        t["namespaces"] = list(namespaces)
    return t


def _split(rng, total, parts):
    """`total` as `parts` positive integers (fewer when total is smaller)."""
    parts = min(parts, total)
    cuts = sorted(rng.sample(range(1, total), parts - 1)) if parts > 1 else []
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


# ---- (a) the skew ladder -----------------------------------------------------------------------------------------------------
OFFSETS = (0, 1, 63, 64, 65, 1000, 4095, 4200)
NINTH_OFFSET = 2


def skew_ladder(seed, n_nodes=330, n_asks=4200, ninth_zone=False):
    """Zone j (nodes i % 8 == j) holds B + OFFSETS[j] pods app=web, every zone's pods cut into pieces on its first node, its last
    node (another 256-node block from 257 nodes on) and one in between; every 41st node has no zone label. Ask `ladder-k`: one hard
    zone constraint, selector app=web, maxSkew k + 1, labelled app=web for even k (self-match 1) and app=batch for odd k.
    Closed form under the topology plugins: fit ⇔ the node carries the label ∧ offset(zone) + self ≤ k + 1.
    What must NOT count sits next to it: web pods in another namespace, terminating web pods, web pods on nodes without the label.
    ninth_zone: node 17 becomes the only node of zone z8 (B + 2 pods), and three templates md-8 / md-9 / md-10 (maxSkew 1,
    minDomains 8 / 9 / 10, self-match 0) are added: with nine zones md-8 and md-9 see the minimum B, md-10 sees 0."""
    rng = random.Random(seed)
    names = node_names(n_nodes)
    base = rng.randrange(2, 7)
    zone_of = [None if i % 41 == 40 else f"z{i % 8}" for i in range(n_nodes)]
    offsets = {f"z{j}": off for j, off in enumerate(OFFSETS)}
    if ninth_zone:
        zone_of[17] = "z8"
        offsets["z8"] = NINTH_OFFSET
    nodes = [make_node(names[i], {"zone": z} if z else {}) for i, z in enumerate(zone_of)]
    zone_nodes, pieces = {}, {}
    for z in offsets:
        members = [i for i in range(n_nodes) if zone_of[i] == z]
        zone_nodes[z] = members
        where = [members[0], members[-1], members[rng.randrange(1, max(len(members) - 1, 2)) % len(members)]]
        where = list(dict.fromkeys(where))
        pieces[z] = list(zip(where, _split(rng, base + offsets[z], len(where))))
        for i, count in pieces[z]:
            nodes[i]["pods"].append(resident(f"web-{z}-{i}", {"app": "web"}, replicas=count))
    for i in range(n_nodes):   # nothing below counts for selector app=web in namespace default on a labelled node
        if i % 7 == 3:
            nodes[i]["pods"].append(resident(f"api-{i}", {"app": "api"}, replicas=rng.randrange(1, 4)))
        if i % 16 == 0:
            nodes[i]["pods"].append(resident(f"web-other-{i}", {"app": "web"}, ns="other", replicas=50))
        if i % 16 == 9:
            nodes[i]["pods"].append(resident(f"web-leaving-{i}", {"app": "web"}, replicas=40, terminating=True))
        if zone_of[i] is None:
            nodes[i]["pods"].append(resident(f"web-nolabel-{i}", {"app": "web"}, replicas=7))
    asks, ladder = [], []
    for k in range(n_asks):
        self_match = 1 - k % 2
        asks.append(make_ask(f"ladder-{k}", {"app": "web" if self_match else "batch"}, spread=[constraint("zone", k + 1)]))
        ladder.append((f"ladder-{k}", k + 1, self_match))
    for k in range(3):   # asks nobody selects and nothing constrains
        asks.insert((k * n_asks) // 3, make_ask(f"idle-{k}", {"app": "idle"}))
    siblings = []
    if ninth_zone:
        for md in (8, 9, 10):
            asks.append(make_ask(f"md-{md}", {"app": "batch"}, spread=[constraint("zone", 1, minDomains=md)]))
        siblings = [("minDomains D / D + 1", "md-9", "md-10", True)]
    meta = {"population": "skew_ladder", "base": base, "zone_of": zone_of, "offsets": offsets, "zone_nodes": zone_nodes, "pieces": pieces,
            "ladder": ladder, "pairs": siblings, "same": [("md-8", "md-9")] if ninth_zone else [],
            "degenerate": [f"idle-{k}" for k in range(3)] + (["md-10"] if ninth_zone else [])}
    return {"nodes": nodes, "pods": asks}, meta


def ladder_closed_form(meta):
    """[len(ladder)][N] fits of the ladder asks under the topology plugins alone, from the offsets — no histogram."""
    off = np.array([-1 if z is None else meta["offsets"][z] for z in meta["zone_of"]], dtype=np.int64)
    skew = np.array([s for _, s, _ in meta["ladder"]], dtype=np.int64)
    self_match = np.array([m for _, _, m in meta["ladder"]], dtype=np.int64)
    return ((off[None, :] >= 0) & (off[None, :] + self_match[:, None] <= skew[:, None])).astype(np.uint8)


# ---- (b) sibling templates ---------------------------------------------------------------------------------------------------
POLICY_ZONES = ("z0", "z1", "z2", "z3", "z4", "z5", "zx", "zm")
# web pods in namespace default by (zone, pool, tainted, has a rack label): totals z0 5, z1 8, z2 11, z3 9, z4 9, z5 7, zx 20, zm 1
POLICY_COUNTS = (("z0", "p1", False, True, 5), ("z1", "p1", False, True, 6), ("z2", "p1", False, True, 8), ("z3", "p1", False, True, 4),
                 ("z4", "p1", False, True, 5), ("z5", "p1", False, True, 7), ("z3", "p1", False, False, 5), ("z2", "p1", True, True, 3),
                 ("z1", "p2", False, True, 2), ("z4", "p2", False, True, 4), ("zx", "p2", False, True, 20), ("zm", "p2", False, True, 1))
POLICY_TOTALS = {"z0": 5, "z1": 8, "z2": 11, "z3": 9, "z4": 9, "z5": 7, "zx": 20, "zm": 1}


def policies(seed, n_nodes=1537):
    """Nodes: zone by i % 8 (zx and zm only in pool p2), pool p2 for every third group of eight, no rack label when i % 13 == 6,
    taint dedicated=x:NoSchedule when i % 11 == 5. The web pods of every (zone, pool, tainted, racked) cell sit on the first and the
    last node of the cell, half of them ver=v1, half ver=v2. zm — the global minimum, 1 pod — also holds 30 web pods of namespace
    `other` and 30 terminating ones. The templates come in siblings that differ in ONE attribute, with the counts placed so that the
    attribute decides nodes (the arithmetic is in the comments next to each pair)."""
    rng = random.Random(seed)
    names = node_names(n_nodes)
    attr = []
    for i in range(n_nodes):
        zone = POLICY_ZONES[i % 8]
        pool = "p2" if i % 8 >= 6 or (i // 8) % 3 == 2 else "p1"
        attr.append({"zone": zone, "pool": pool, "rack": None if i % 13 == 6 else f"r{(i // 8) % 5}", "tainted": i % 11 == 5})
    nodes = []
    for i, a in enumerate(attr):
        labels = {"zone": a["zone"], "pool": a["pool"]}
        if a["rack"]:
            labels["rack"] = a["rack"]
        nodes.append(make_node(names[i], labels, taints=[TAINT_X] if a["tainted"] else []))
    placed = {}
    for zone, pool, tainted, racked, count in POLICY_COUNTS:
        cell = [i for i, a in enumerate(attr) if (a["zone"], a["pool"], a["tainted"], a["rack"] is not None) == (zone, pool, tainted, racked)]
        assert len(cell) >= 2, (zone, pool, tainted, racked)
        for ver, i, c in (("v1", cell[0], count // 2), ("v2", cell[-1], count - count // 2)):
            if c:
                nodes[i]["pods"].append(resident(f"web-{zone}-{i}-{ver}", {"app": "web", "ver": ver}, replicas=c))
                placed.setdefault(zone, []).append((i, ver, c))
    zm = next(i for i, a in enumerate(attr) if a["zone"] == "zm" and a["rack"] and not a["tainted"])
    nodes[zm]["pods"].append(resident("web-other-zm", {"app": "web", "ver": "v1"}, ns="other", replicas=30))
    nodes[zm]["pods"].append(resident("web-leaving-zm", {"app": "web", "ver": "v2"}, replicas=30, terminating=True))
    for i in range(0, n_nodes, 9):
        nodes[i]["pods"].append(resident(f"api-{i}", {"app": "api", "ver": "v1"}, replicas=rng.randrange(1, 5)))
    P1 = {"pool": "p1"}
    batch, web = {"app": "batch"}, {"app": "web"}
    T = [
        # totals minus the minimum 1: z0 4, z5 6, z1 7, z3 8, z4 8, z2 10, zx 19, zm 0
        make_ask("skew-6", batch, spread=[constraint("zone", 6)]),             # z1: 7 > 6
        make_ask("skew-7", batch, spread=[constraint("zone", 7)]),             # z1: 7 ≤ 7
        make_ask("skew-7-self", web, spread=[constraint("zone", 7)]),          # z1: 7 + 1 > 7
        make_ask("skew-8-self", web, spread=[constraint("zone", 8)]),          # z1: 7 + 1 ≤ 8
        make_ask("md-8", batch, spread=[constraint("zone", 4, minDomains=8)]),            # 8 domains: min 1, z0 4 ≤ 4
        make_ask("md-9", batch, spread=[constraint("zone", 4, minDomains=9)]),            # min 0: z0 5 > 4, only zm
        make_ask("md-max", batch, spread=[constraint("zone", 4, minDomains=INT32_MAX)]),
        make_ask("skew-max", web, spread=[constraint("zone", INT32_MAX)]),
        make_ask("skew-19-self", web, spread=[constraint("zone", 19)]),        # zx: 19 + 1 > 19
        # nodeSelector pool=p1. Honor: p1 counts z0 5, z1 6, z2 11, z3 9, z4 5, z5 7, min 5, zx and zm are no domains at all.
        # Ignore: the totals, min 1 (zm, outside the selection)
        make_ask("aff-honor", batch, node_selector=P1, spread=[constraint("zone", 3, nodeAffinityPolicy="Honor")]),
        make_ask("aff-ignore", batch, node_selector=P1, spread=[constraint("zone", 3, nodeAffinityPolicy="Ignore")]),
        make_ask("aff-none", batch, spread=[constraint("zone", 3, nodeAffinityPolicy="Honor")]),
        # Honor without the toleration: the 3 pods of z2 on tainted nodes leave, z2 = 8: 7 ≤ 8; everybody else z2 = 11: 10 > 8
        make_ask("taint-honor", batch, spread=[constraint("zone", 8, nodeTaintsPolicy="Honor")]),
        make_ask("taint-ignore", batch, spread=[constraint("zone", 8, nodeTaintsPolicy="Ignore")]),
        make_ask("taint-honor-tol", batch, tolerations=[TOL_X], spread=[constraint("zone", 8, nodeTaintsPolicy="Honor")]),
        make_ask("taint-ignore-tol", batch, tolerations=[TOL_X], spread=[constraint("zone", 8, nodeTaintsPolicy="Ignore")]),
        # one constraint: z3 = 9, 8 > 5. With the rack constraint the 5 pods of z3 on a rack-less node leave: z3 = 4, 3 ≤ 5
        make_ask("one-c", batch, spread=[constraint("zone", 5)]),
        make_ask("two-c", batch, spread=[constraint("zone", 5), constraint("rack", INT32_MAX)]),
        make_ask("sel-nil", batch, spread=[constraint("rack", 1, selector=None)]),
        make_ask("sel-empty", batch, spread=[constraint("rack", 1, selector={})]),
        make_ask("sel-web", batch, spread=[constraint("rack", 1)]),
        # namespace other: zm 30, every other zone 0
        make_ask("ns-default", batch, spread=[constraint("zone", 2)]),
        make_ask("ns-other", batch, ns="other", spread=[constraint("zone", 2)]),
        # ver=v1: z0 2, z1 4, z2 5, z3 4, z4 4, z5 3, zx 10, zm 0 (min 0); ver=v2: z0 3, z1 4, z2 6, z3 5, z4 5, z5 4, zx 10, zm 1
        make_ask("mlk-v1", {"app": "batch", "ver": "v1"}, spread=[constraint("zone", 3, matchLabelKeys=["ver"])]),
        make_ask("mlk-v2", {"app": "batch", "ver": "v2"}, spread=[constraint("zone", 3, matchLabelKeys=["ver"])]),
        make_ask("mlk-none", {"app": "batch", "ver": "v1"}, spread=[constraint("zone", 3)]),
        make_ask("plain", batch), make_ask("plain-tol", batch, tolerations=[TOL_X]),
    ]
    asks = T + [dict(json.loads(json.dumps(t)), metadata=dict(t["metadata"], name=t["metadata"]["uid"] + "-twin", uid=t["metadata"]["uid"] + "-twin"))
                for t in T[::3]]
    rng.shuffle(asks)
    pairs = [("maxSkew s / s + 1", "skew-6", "skew-7", True), ("maxSkew s / s + 1 with self-match", "skew-7-self", "skew-8-self", True),
             ("self-match 0 / 1", "skew-7", "skew-7-self", True), ("minDomains D / D + 1", "md-8", "md-9", True),
             ("minDomains D / int32 max", "md-8", "md-max", True), ("maxSkew int32 max", "skew-max", "skew-19-self", True),
             ("nodeAffinityPolicy Honor / Ignore", "aff-honor", "aff-ignore", True), ("nodeSelector under Honor", "aff-honor", "aff-none", True),
             ("nodeTaintsPolicy Honor / Ignore", "taint-honor", "taint-ignore", True),
             ("tolerations under nodeTaintsPolicy Honor", "taint-honor", "taint-honor-tol", True),
             ("one constraint / two", "one-c", "two-c", True), ("nil selector / matchLabels", "sel-nil", "sel-web", True),
             ("empty selector / matchLabels", "sel-empty", "sel-web", True), ("namespace", "ns-default", "ns-other", True),
             ("matchLabelKeys value", "mlk-v1", "mlk-v2", True), ("matchLabelKeys / none", "mlk-v1", "mlk-none", True)]
    meta = {"population": "policies", "attr": attr, "placed": placed, "pairs": pairs,
            "same": [("md-9", "md-max"), ("taint-ignore", "taint-ignore-tol"), ("taint-honor-tol", "taint-ignore-tol"), ("sel-nil", "sel-empty")],
            "degenerate": ["skew-max", "plain", "plain-tol"],
            # (template, zones that are no domain for it, a sibling for which they are): the nodes of those zones fit the first — an
            # absent domain counts 0 and the minimum is taken over the present ones — and those of the first zone fail the second
            "absent_domain": ("aff-honor", ("zx", "zm"), "aff-ignore"), "rackless_zone": ("one-c", "two-c", "z3"),
            "domains": 8, "minimum": {"skew-6": 1, "aff-honor": 5, "aff-ignore": 1, "md-9": 0, "ns-other": 0, "mlk-v1": 0, "mlk-v2": 1}}
    return {"nodes": nodes, "pods": asks}, meta


# ---- (c) one domain per node -------------------------------------------------------------------------------------------------
HOSTNAME_MINIMA = {"first": 0, "last": -1, "left": 8255, "right": 8256}   # by node index (snapshot order)
HOSTNAME_CELLS = ("cell-left", "cell-right")                                # by rank of the node's name (see hostname)


def hostname(seed, n_nodes=8300):
    """Constraints on kubernetes.io/hostname, maxSkew 1. For each of six labels every node holds 2 matching pods (3 when i % 5 == 0),
    except ONE node that holds 1. Label `flat`: 2 pods on every node. Self-match 0: fit ⇔ count ≤ 2; self-match 1: only the minimum
    node fits (count + 1 − 1 ≤ 1). Three nodes carry no hostname label, which leaves D = n_nodes − 3 domains.
    Where the minimum sits is chosen in TWO orders, because the engine walks two:
      by node index (HOSTNAME_MINIMA) — the first node, the last node, nodes 8255 and 8256: two wavefronts (8256 = 129 * 64) of the
        last, partial 256-node block of a pass with one thread per node (k_spread_count);
      by domain (HOSTNAME_CELLS) — a key's domains are numbered by the byte order of their values, and `node_names` gives node i a
        name of rank about n − 1 − i, so a walk over the cells of a histogram (k_spread_min, 64 lanes) meets the nodes in another
        order: `cell-left` / `cell-right` put the minimum on the labelled nodes whose names have rank D // 64 * 64 − 1 and D // 64 * 64
        among the labelled nodes' names, the last cell of the last full stride and the first of the partial one.
    meta["cells"] gives that rank for all six labels; with these names `first` is the last cell (D − 1) and `last` is cell 0."""
    rng = random.Random(seed)
    names = node_names(n_nodes)
    minima = {k: (v % n_nodes) for k, v in HOSTNAME_MINIMA.items()}
    nolabel = sorted({100 % n_nodes, (n_nodes // 2 + 7) % n_nodes, n_nodes - 300 if n_nodes > 300 else 1} - set(minima.values()))
    by_name = sorted((i for i in range(n_nodes) if i not in nolabel), key=lambda i: names[i].encode())
    partial = len(by_name) // 64 * 64
    minima.update(zip(HOSTNAME_CELLS, (by_name[max(partial - 1, 0)], by_name[min(partial, len(by_name) - 1)])))
    cells = {k: by_name.index(at) for k, at in minima.items()}
    nodes = []
    for i in range(n_nodes):
        node = make_node(names[i], {"zone": f"z{i % 4}"}, hostname=i not in nolabel)
        above = {k: "y" for k, at in minima.items() if at != i}
        node["pods"].append(resident(f"all-{i}", dict({k: "y" for k in minima}, flat="y")))
        node["pods"].append(resident(f"more-{i}", dict(above, flat="y")))
        if i % 5 == 0 and above:
            node["pods"].append(resident(f"most-{i}", above))
        nodes.append(node)
    asks = []
    for key in list(minima) + ["flat"]:
        for self_match in (0, 1):
            for copy in range(3):
                asks.append(make_ask(f"{key}-{self_match}-{copy}", {key: "y"} if self_match else {"app": "ask"},
                                     spread=[constraint(HOST, 1, selector={"matchLabels": {key: "y"}})]))
    asks += [make_ask("plain-0", {"app": "ask"}), make_ask("plain-1", {"flat": "y"})]
    rng.shuffle(asks)
    pairs = [(f"self-match 0 / 1 ({key})", f"{key}-0-0", f"{key}-1-0", True) for key in minima]
    pairs += [("where the minimum sits", "first-1-0", "last-1-0", True), ("where the minimum sits (wavefront boundary of the nodes)", "left-1-0", "right-1-0", True),
              ("where the minimum sits (stride boundary of the cells)", "cell-left-1-0", "cell-right-1-0", True)]
    meta = {"population": "hostname", "minima": minima, "cells": cells, "nolabel": nolabel, "pairs": pairs, "same": [("flat-0-0", "flat-1-0")],
            "degenerate": ["plain-0", "plain-1"]}
    return {"nodes": nodes, "pods": asks}, meta


# ---- (d) inter-pod affinity ----------------------------------------------------------------------------------------------------
def interpod(seed, n_nodes=1537):
    """Zones z0..z5 by i % 6; no zone label when i % 29 == 7, no hostname label when i % 97 == 11. Existing pods: app=db on one node of
    z1 and one of z3 (different 256-node blocks), app=cache on one node of z2 (no pod is both), app=solo ONLY on a node without the
    zone label, app=queue in namespace `other` on a node of z4; guards whose required anti-affinity names app=intruder (zone key, on
    z5; a second one on z0 whose term lists namespace `other`) and app=hintruder (hostname key; on the first and last node, on nodes
    255 and 256 and on a node without the zone label)."""
    rng = random.Random(seed)
    names = node_names(n_nodes)
    zone_of = [None if i % 29 == 7 else f"z{i % 6}" for i in range(n_nodes)]
    has_host = [i % 97 != 11 for i in range(n_nodes)]
    nodes = [make_node(names[i], {"zone": z} if z else {}, hostname=has_host[i]) for i, z in enumerate(zone_of)]

    def pick(zone, low, need_host=True):
        return next(i for i in range(low, n_nodes) if zone_of[i] == zone and (has_host[i] or not need_host))

    at = {"db-z1": pick("z1", 10), "db-z3": pick("z3", n_nodes - 200), "cache": pick("z2", 300), "solo": 7, "queue": pick("z4", 600),
          "guard": pick("z5", 900), "nsguard": pick("z0", 1100)}
    assert zone_of[at["solo"]] is None and has_host[at["solo"]]
    nodes[at["db-z1"]]["pods"].append(resident("db-a", {"app": "db"}, replicas=2))
    nodes[at["db-z3"]]["pods"].append(resident("db-b", {"app": "db"}))
    nodes[at["cache"]]["pods"].append(resident("cache-a", {"app": "cache"}, replicas=3))
    nodes[at["solo"]]["pods"].append(resident("solo-a", {"app": "solo"}))
    nodes[at["queue"]]["pods"].append(resident("queue-a", {"app": "queue"}, ns="other", replicas=2))
    nodes[at["guard"]]["pods"].append(resident("guard-a", {"app": "guard"}, anti=[term("intruder", "zone")]))
    nodes[at["nsguard"]]["pods"].append(resident("nsguard-a", {"app": "guard"}, anti=[term("intruder", "zone", namespaces=["other"])]))
    hguards = [0, n_nodes - 1, 255, 256, 36]
    assert zone_of[36] is None and all(has_host[i] for i in hguards)
    for i in hguards:
        nodes[i]["pods"].append(resident(f"hguard-{i}", {"app": "guard"}, anti=[term("hintruder", HOST)]))
    for i in range(5, n_nodes, 11):
        nodes[i]["pods"].append(resident(f"api-{i}", {"app": "api"}, replicas=rng.randrange(1, 4)))
    ask = {"app": "ask"}
    T = [
        make_ask("aff-db-zone", ask, affinity=[term("db", "zone")]),                          # the labelled nodes of z1 and z3
        make_ask("aff-db-host", ask, affinity=[term("db", HOST)]),                            # the two nodes that hold db
        make_ask("aff-db-self", {"app": "db"}, affinity=[term("db", "zone")]),                # matches itself, but matches exist: no escape, z1 and z3
        make_ask("aff-two", ask, affinity=[term("db", "zone"), term("cache", "zone")]),       # no single pod matches both: nowhere
        make_ask("aff-two-keys", ask, affinity=[term("db", "zone"), term("db", HOST)]),       # the two db nodes
        make_ask("escape-self", {"app": "fresh"}, affinity=[term("fresh", "zone")]),          # no match anywhere, matches itself: every labelled node
        make_ask("escape-noself", ask, affinity=[term("fresh", "zone")]),                     # nowhere
        make_ask("solo-self", {"app": "solo"}, affinity=[term("solo", "zone")]),              # the only match has no zone label: the escape holds
        make_ask("solo-noself", ask, affinity=[term("solo", "zone")]),
        make_ask("ns-default", ask, affinity=[term("queue", "zone")]),                        # queue lives in `other`: nowhere
        make_ask("ns-listed", ask, affinity=[term("queue", "zone", namespaces=["other"])]),   # z4
        make_ask("ns-both", ask, affinity=[term("queue", "zone", namespaces=["default", "other"])]),
        make_ask("anti-db-zone", ask, anti=[term("db", "zone")]),                             # everything but z1 and z3, label-less nodes fit
        make_ask("anti-db-host", ask, anti=[term("db", HOST)]),
        make_ask("anti-queue-default", ask, anti=[term("queue", "zone")]),                    # everywhere
        make_ask("anti-queue-listed", ask, anti=[term("queue", "zone", namespaces=["other"])]),
        make_ask("intruder", {"app": "intruder"}),                                            # symmetry: not z5
        make_ask("intruder-other", {"app": "intruder"}, ns="other"),                          # not z0 (the guard that lists `other`)
        make_ask("hintruder", {"app": "hintruder"}),                                          # not the five guarded nodes
        # spread (selector db, self-match 1: z1 and z3 fail, 1 + 1 − 0 > 1 and 2 + 1 > 1) and affinity to cache (only z2 passes)
        make_ask("both", {"app": "db"}, spread=[constraint("zone", 1, selector={"matchLabels": {"app": "db"}})], affinity=[term("cache", "zone")]),
        make_ask("plain", ask),
    ]
    asks = T + [make_ask(f"fresh-{k}", {"app": "fresh"}, affinity=[term("fresh", "zone")]) for k in range(3)]
    asks += [make_ask("nobody", {"app": "nobody"})]
    rng.shuffle(asks)
    pairs = [("affinity key zone / hostname", "aff-db-zone", "aff-db-host", True), ("the escape with / without self-match", "escape-self", "escape-noself", True),
             ("the escape when the only match has no label", "solo-self", "solo-noself", True), ("namespaces list", "ns-listed", "ns-default", True),
             ("anti-affinity key zone / hostname", "anti-db-zone", "anti-db-host", True),
             ("anti-affinity namespaces list", "anti-queue-listed", "anti-queue-default", True),
             ("symmetry rule by namespace", "intruder", "intruder-other", True), ("symmetry rule", "intruder", "plain", True),
             ("symmetry rule on hostname", "hintruder", "plain", True), ("one term / two terms", "aff-db-zone", "aff-two", True),
             ("self-match with / without a match elsewhere", "aff-db-self", "escape-self", True)]
    meta = {"population": "interpod", "zone_of": zone_of, "has_host": has_host, "at": at, "hguards": hguards, "pairs": pairs,
            "same": [("ns-listed", "ns-both"), ("aff-db-host", "aff-two-keys"), ("escape-self", "solo-self"), ("aff-db-zone", "aff-db-self")],
            "degenerate": ["aff-two", "escape-noself", "solo-noself", "ns-default", "anti-queue-default", "plain", "nobody"],
            "both_fail": "both"}
    return {"nodes": nodes, "pods": asks}, meta


POPULATIONS = {"skew_ladder": skew_ladder, "policies": policies, "hostname": hostname, "interpod": interpod}


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _selector_matches(sel, labels):
    """metav1.LabelSelector: nil matches nothing, {} matches everything; matchLabels and matchExpressions are ANDed."""
    if sel is None:
        return False
    for k, v in (sel.get("matchLabels") or {}).items():
        if labels.get(k) != v:
            return False
    for r in sel.get("matchExpressions") or []:
        has, op = r["key"] in labels, r["operator"]
        if op == "In" and not (has and labels[r["key"]] in r.get("values", [])):
            return False
        if op == "NotIn" and has and labels[r["key"]] in r.get("values", []):
            return False
        if op == "Exists" and not has:
            return False
        if op == "DoesNotExist" and has:
            return False
    return True


def _selector_empty(sel):
    return sel is not None and not (sel.get("matchLabels") or {}) and not (sel.get("matchExpressions") or [])


def _tolerates(tol, taint):
    """SURVEY.md §A.4."""
    if tol.get("effect", "") not in ("", taint["effect"]):
        return False
    if tol.get("key", "") not in ("", taint["key"]):
        return False
    op = tol.get("operator", "")
    return op == "Exists" or (op in ("Equal", "") and tol.get("value", "") == taint.get("value", ""))


def _masks(plugins):
    """plugins: a list of names (PreFilter list = Filter list; "*" = all) or a pair (PreFilter list, Filter list)."""
    if len(plugins) == 2 and not isinstance(plugins[0], str):
        pre, filt = plugins
    else:
        pre = filt = plugins
    full = lambda names: set(PLUGINS) if "*" in names else set(names)   # noqa: E731
    return full(pre), full(filt)


class _Cluster:
    def __init__(self, snapshot):
        self.nodes = snapshot["nodes"]
        self.n = len(self.nodes)
        self.labels = [n["metadata"].get("labels") or {} for n in self.nodes]
        self.names = [n["metadata"]["name"] for n in self.nodes]
        self.pods = []   # (node, namespace, labels, replicas, terminating, required anti-affinity terms)
        self.pod_count = np.zeros(self.n, dtype=np.int64)
        for i, n in enumerate(self.nodes):
            for p in n.get("pods") or []:
                reps = p.get("replicas", 1)
                anti = (((p["spec"].get("affinity") or {}).get("podAntiAffinity") or {}).get("requiredDuringSchedulingIgnoredDuringExecution")) or []
                self.pods.append((i, p["metadata"].get("namespace", "default"), p["metadata"].get("labels") or {}, reps,
                                  "deletionTimestamp" in p["metadata"], anti))
                self.pod_count[i] += reps
        self.allowed = np.array([int(n["status"]["allocatable"]["pods"]) for n in self.nodes], dtype=np.int64)
        self.unschedulable = np.array([bool(n["spec"].get("unschedulable")) for n in self.nodes])
        self._dom, self._vec, self._sel, self._tol = {}, {}, {}, {}

    def domain(self, key):
        """(domain id per node, -1 = no label; number of values)."""
        if key not in self._dom:
            ids = {}
            d = np.array([ids.setdefault(l[key], len(ids)) if key in l else -1 for l in self.labels], dtype=np.int64)
            self._dom[key] = (d, len(ids))
        return self._dom[key]

    def count(self, key, pred, skip_terminating):
        """Per node: the existing pods (replicas expanded) that satisfy pred(namespace, labels, anti terms) → how many times."""
        if key not in self._vec:
            v = np.zeros(self.n, dtype=np.int64)
            for node, ns, labels, reps, terminating, anti in self.pods:
                if terminating and skip_terminating:
                    continue
                v[node] += reps * int(pred(ns, labels, anti))
            self._vec[key] = v
        return self._vec[key]

    def selected(self, node_selector):
        key = json.dumps(node_selector, sort_keys=True)
        if key not in self._sel:
            self._sel[key] = np.array([all(l.get(k) == v for k, v in node_selector.items()) for l in self.labels])
        return self._sel[key]

    def tolerated(self, tolerations):
        """No taint with effect NoSchedule / NoExecute that no toleration tolerates."""
        key = json.dumps(tolerations, sort_keys=True)
        if key not in self._tol:
            self._tol[key] = np.array([all(any(_tolerates(t, taint) for t in tolerations) for taint in (n["spec"].get("taints") or [])
                                           if taint["effect"] in ("NoSchedule", "NoExecute")) for n in self.nodes])
        return self._tol[key]


def _term_matches(t, owner_ns, ns, labels):
    """framework.AffinityTerm.Matches: the namespaces list (default: the owner's namespace) holds the pod's, the selector its labels."""
    spaces = t.get("namespaces") or [owner_ns]
    return ns in spaces and _selector_matches(t.get("labelSelector"), labels)


def model(snapshot, meta, plugins):
    """→ {"fit": uint8[P][N], "code": uint8[P][N] first failing plugin (0 where the ask fits), "missing": bool[P][N] the
    PodTopologySpread failure is the missing-label one, "sums": (sum of all count cells, sum of all present cells) over the distinct
    topology signatures, "detail": per ask the (domains, minimum after the minDomains rule) of its hard constraints}.
    A Filter plugin that reads PreFilter state fails every node (an Error status) when its PreFilter is not in the list.
    meta is not read: the verdicts come from the snapshot alone (the argument keeps the call sites of the populations uniform)."""
    pre, filt = _masks(plugins)
    cl = _Cluster(snapshot)
    N, asks = cl.n, snapshot["pods"]
    fit = np.ones((len(asks), N), dtype=np.uint8)
    code = np.zeros((len(asks), N), dtype=np.uint8)
    missing = np.zeros((len(asks), N), dtype=bool)
    detail, signatures, histograms = [], {}, {}
    unsched_taint = {"key": "node.kubernetes.io/unschedulable", "value": "", "effect": "NoSchedule"}
    for p, pod in enumerate(asks):
        spec, labels, ns = pod["spec"], pod["metadata"].get("labels") or {}, pod["metadata"].get("namespace", "default")
        assert not any(c["resources"]["requests"] for c in spec["containers"]) and not any(c.get("ports") for c in spec["containers"])
        tolerations, node_selector = spec.get("tolerations") or [], spec.get("nodeSelector") or {}
        affinity = spec.get("affinity") or {}
        assert "nodeAffinity" not in affinity, "the designed asks select nodes by nodeSelector only"
        failed = np.zeros(N, dtype=np.uint8)

        def fail(mask, plugin):
            np.copyto(failed, np.uint8(CODE[plugin]), where=mask & (failed == 0))

        if "NodeUnschedulable" in filt and not any(_tolerates(t, unsched_taint) for t in tolerations):
            fail(cl.unschedulable, "NodeUnschedulable")
        if "NodeName" in filt and spec.get("nodeName"):
            fail(np.array([name != spec["nodeName"] for name in cl.names]), "NodeName")
        if "TaintToleration" in filt:
            fail(~cl.tolerated(tolerations), "TaintToleration")
        if "NodeAffinity" in filt and node_selector:   # (no selector: PreFilter Skip, or a Filter that passes)
            fail(~cl.selected(node_selector), "NodeAffinity")
        if "NodePorts" in filt and "NodePorts" not in pre:
            fail(np.ones(N, dtype=bool), "NodePorts")
        if "NodeResourcesFit" in filt:
            fail(np.ones(N, dtype=bool) if "NodeResourcesFit" not in pre else cl.pod_count + 1 > cl.allowed, "NodeResourcesFit")
        # ---- PodTopologySpread
        hard = [c for c in spec.get("topologySpreadConstraints") or [] if c["whenUnsatisfiable"] == "DoNotSchedule"]
        info, sig, cells = [], [ns], [0, 0]
        if hard:
            has_all = np.ones(N, dtype=bool)
            for c in hard:
                has_all &= cl.domain(c["topologyKey"])[0] >= 0
            honor_aff = honor_taints = False
            for c in hard:
                sel = c.get("labelSelector")
                if sel is not None:   # matchLabelKeys: the incoming pod's value of every listed key it carries is ANDed on
                    extra = {k: labels[k] for k in c.get("matchLabelKeys") or [] if k in labels}
                    if extra:
                        sel = dict(sel, matchLabels=dict(sel.get("matchLabels") or {}, **extra))
                selkey = json.dumps(sel, sort_keys=True)
                eligible = has_all.copy()
                if c.get("nodeAffinityPolicy", "Honor") == "Honor":
                    honor_aff = True
                    eligible &= cl.selected(node_selector)
                if c.get("nodeTaintsPolicy", "Ignore") == "Honor":
                    honor_taints = True
                    eligible &= cl.tolerated(tolerations)
                d, nd = cl.domain(c["topologyKey"])
                # (templates that ask the same of the same nodes share the arrays: the ladder's thousands differ in maxSkew only)
                hkey = (tuple(x["topologyKey"] for x in hard), c["topologyKey"], ns, selkey, c.get("minDomains", 1),
                        json.dumps(node_selector, sort_keys=True) if c.get("nodeAffinityPolicy", "Honor") == "Honor" else None,
                        json.dumps(tolerations, sort_keys=True) if c.get("nodeTaintsPolicy", "Ignore") == "Honor" else None)
                if hkey not in histograms:
                    if _selector_empty(sel):   # countPodsMatchSelector: an empty selector counts nothing
                        per_node = np.zeros(N, dtype=np.int64)
                    else:
                        per_node = cl.count(("spread", ns, selkey), lambda pns, pl, _a, sel=sel: pns == ns and _selector_matches(sel, pl), True)
                    cnt = np.bincount(d[eligible], weights=per_node[eligible], minlength=max(nd, 1)).astype(np.int64)
                    present = np.bincount(d[eligible], minlength=max(nd, 1)) > 0
                    domains = int(present.sum())
                    minimum = int(cnt[present].min()) if domains else 0
                    if domains < c.get("minDomains", 1):
                        minimum = 0
                    histograms[hkey] = (cnt, present, domains, minimum, np.where((d >= 0) & present[np.maximum(d, 0)], cnt[np.maximum(d, 0)], 0))
                cnt, present, domains, minimum, here = histograms[hkey]
                self_match = int(_selector_matches(sel, labels))
                info.append({"domains": domains, "min": minimum, "count": cnt, "present": present, "self": self_match})
                sig.append(("spread", c["topologyKey"], selkey, c["maxSkew"], c.get("minDomains", 1), self_match,
                            c.get("nodeAffinityPolicy", "Honor"), c.get("nodeTaintsPolicy", "Ignore")))
                cells[0] += int(cnt.sum())
                cells[1] += domains
                if "PodTopologySpread" in filt and "PodTopologySpread" in pre:
                    no_label = (d < 0) & (failed == 0)
                    missing[p] |= no_label
                    fail((d < 0) | (here + self_match - minimum > c["maxSkew"]), "PodTopologySpread")
            sig.append((json.dumps(node_selector, sort_keys=True) if honor_aff else None,
                        tuple(bool(x) for x in cl.tolerated(tolerations)) if honor_taints else None))
        if "PodTopologySpread" in filt and "PodTopologySpread" not in pre:
            fail(np.ones(N, dtype=bool), "PodTopologySpread")
        # ---- InterPodAffinity
        aff = ((affinity.get("podAffinity") or {}).get("requiredDuringSchedulingIgnoredDuringExecution")) or []
        anti = ((affinity.get("podAntiAffinity") or {}).get("requiredDuringSchedulingIgnoredDuringExecution")) or []
        lkey = json.dumps(labels, sort_keys=True)
        # existing pods' required anti-affinity terms that match the incoming pod, by topology key (the symmetry rule)
        existing_keys = sorted({t["topologyKey"] for _n, pns, _l, _r, _t, terms in cl.pods for t in terms if _term_matches(t, pns, ns, labels)})
        ipa_fail = np.zeros(N, dtype=bool)
        if aff:
            akey = json.dumps(aff, sort_keys=True)
            all_terms = cl.count(("aff", ns, akey), lambda pns, pl, _a: all(_term_matches(t, ns, pns, pl) for t in aff), False)
            self_match = all(_term_matches(t, ns, ns, labels) for t in aff)
            pods_exist, any_match = np.ones(N, dtype=bool), False
            for t in aff:
                d, nd = cl.domain(t["topologyKey"])
                cnt = np.bincount(d[d >= 0], weights=all_terms[d >= 0], minlength=max(nd, 1)).astype(np.int64)
                any_match |= bool((cnt > 0).any())
                ipa_fail |= d < 0   # every topology label of the terms must be on the node
                pods_exist &= np.where(d >= 0, cnt[np.maximum(d, 0)], 0) > 0
                cells[0] += int(cnt.sum())
            ipa_fail |= ~pods_exist & (not (not any_match and self_match))
            sig.append(("affinity", akey, self_match))
        for t in anti:
            tkey = json.dumps(t, sort_keys=True)
            d, nd = cl.domain(t["topologyKey"])
            per_node = cl.count(("anti", ns, tkey), lambda pns, pl, _a, t=t: _term_matches(t, ns, pns, pl), False)
            cnt = np.bincount(d[d >= 0], weights=per_node[d >= 0], minlength=max(nd, 1)).astype(np.int64)
            ipa_fail |= (d >= 0) & (cnt[np.maximum(d, 0)] > 0)
            cells[0] += int(cnt.sum())
            sig.append(("anti", tkey))
        for key in existing_keys:
            d, nd = cl.domain(key)
            per_node = cl.count(("existing", ns, lkey, key),
                                lambda pns, _pl, terms, key=key: sum(1 for t in terms if t["topologyKey"] == key and _term_matches(t, pns, ns, labels)), False)
            cnt = np.bincount(d[d >= 0], weights=per_node[d >= 0], minlength=max(nd, 1)).astype(np.int64)
            ipa_fail |= (d >= 0) & (cnt[np.maximum(d, 0)] > 0)
            cells[0] += int(cnt.sum())
            sig.append(("existing", lkey, key))
        if "InterPodAffinity" in filt and (aff or anti or existing_keys or "InterPodAffinity" not in pre):
            fail(np.ones(N, dtype=bool) if "InterPodAffinity" not in pre else ipa_fail, "InterPodAffinity")
        code[p] = failed
        fit[p] = failed == 0
        missing[p] &= failed == SPREAD
        detail.append(info)
        if len(sig) > 1:
            signatures[json.dumps(sig, sort_keys=True, default=str)] = cells
    sums = (sum(c[0] for c in signatures.values()), sum(c[1] for c in signatures.values()))
    return {"fit": fit, "code": code, "missing": missing, "sums": sums, "signatures": len(signatures), "detail": detail}
