"""Designed clusters for the headroom of asks with ONE hard topology spread constraint, with a model over Python ints.

Pure Python, no randomness. The nodes are tests/_headgen.py's (_node: free values at the quotient boundaries, a tainted word of nodes, an
unschedulable node), the asks are built with its _ask and carry a constraint of their own; a case may label the nodes with a further
key, leave some of them without it, and SEED nodes with resident pods that match the constraint's selector (they request nothing, and
the node's pod allowance is raised by as many: free values and free slots stay what _headgen designed).

case(...) → dict: snapshot (nodes + the case's asks), meta (what _headgen's model reads), ask (index of the ask under test), labels (per
node the value of the constraint's key, None = not labelled), matching (per node the resident pods the selector matches), and the
constraint's max_skew / min_domains / self_match. model(case) → (rows, cells): rows[d] = [cnt, cap, nodes, copies] per domain id (the
rank of the bytewise-sorted label values), cells = the 16 summary cells, from the rule alone:
    cap[d] = Σ replicas over the counting nodes of d (replicas: _headgen's, without the spread constraint)
    self_match: M = min over present d of cnt + cap; floor = 0 if present < min_domains else M; copies = clamp(floor + skew − cnt, 0, cap)
    else:       floor = minv (min over present d of cnt, 0 under the minDomains rule); copies = cap if cnt − minv <= skew else 0
status_cluster() → one cluster with the asks that must NOT come out at status 0 under some plugin lists.
"""
import copy

import _headgen as hg

CELLS, ROW = 16, 4
ZONE, HOST = "zone", "kubernetes.io/hostname"


def _constraint(key, max_skew=1, min_domains=None, app="ask"):
    c = {"maxSkew": max_skew, "topologyKey": key, "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": {"app": app}}}
    if min_domains is not None:
        c["minDomains"] = min_domains
    return c


def _spread_ask(uid, req, constraints, **kw):
    pod, info = hg._ask(uid, req, **kw)
    pod["spec"]["topologySpreadConstraints"] = constraints
    return pod, info


def case(name, n_nodes=hg.PERIOD, req=None, max_skew=1, min_domains=None, key=ZONE, app="ask", tolerate=False, zone=None, label=None,
         seeded=None, extra_asks=0):
    """label: i → value of `key` for node i (None = unlabelled), for a key of the case's own; seeded: i → matching resident pods."""
    built = [hg._node(i) for i in range(n_nodes)]
    nodes, infos = [copy.deepcopy(b[0]) for b in built], [b[1] for b in built]
    labels, matching = [], []
    for i, node in enumerate(nodes):
        if label is not None:
            value = label(i)
            if value is not None:
                node["metadata"]["labels"][key] = value
        labels.append(node["metadata"]["labels"].get(key))
        count = seeded(i) if seeded else 0
        for c in range(count):
            uid = f"seed-{i}-{c}"
            node["pods"].append({"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": {"app": "ask"}},
                                 "spec": {"containers": [{"name": "c", "resources": {}}]}})
        node["status"]["allocatable"]["pods"] = str(int(node["status"]["allocatable"]["pods"]) + count)
        matching.append(count if app == "ask" else 1)  # (app == "res": the one resident pod of every node)
    req = {"cpu": 250} if req is None else req
    asks = [_spread_ask("s-" + name, req, [_constraint(key, max_skew, min_domains, app)], tolerate=tolerate, zone=zone)]
    for c in range(extra_asks):  # distinct tasks of the same shape: other requests, other skews
        asks.append(_spread_ask(f"s-{name}-x{c}", {"cpu": 60 + 37 * c}, [_constraint(key, 1 + c % 5, min_domains, app)], tolerate=c % 3 == 0))
    return {"name": name, "snapshot": {"nodes": nodes, "pods": [a[0] for a in asks]},
            "meta": {"nodes": infos, "templates": [a[1] for a in asks]}, "ask": 0, "labels": labels, "matching": matching, "key": key,
            "max_skew": max_skew, "min_domains": 1 if min_domains is None else min_domains, "self_match": 1 if app == "ask" else 0,
            "skews": [max_skew] + [1 + c % 5 for c in range(extra_asks)]}


def _q7(i):
    return None if i % 17 == 0 else f"q{(i * 5) % 7}"


def _r14(i):
    return f"r{i % 14:02d}"


def designed_cases():
    """The 16 cases at which the rule was checked against the clone loop, plus an ask with a node selector (only its zone counts)."""
    return [
        case("skew1"),                                                    # the tainted zone z1 is present with cap 0: it pins the floor at 0
        case("skew3", max_skew=3),
        case("seed-z0", seeded=lambda i: 2 if i in (3, 9) else 0),         # cnt above floor + skew in z0: shut
        case("seed-z2", max_skew=2, seeded=lambda i: 1 if i in (130, 140, 150) else 0),
        case("seed-min4", min_domains=4, max_skew=2, seeded=lambda i: 1 if i in (7, 131) else 0),  # 3 present < 4: floor 0
        case("min3", min_domains=3),
        case("tol-30", req={"cpu": 1900}, tolerate=True),                  # every zone takes copies: the minimum rises to 30 (in z2) ...
        case("tol-32", req={"cpu": 1800}, tolerate=True, max_skew=2),      # ... and to 32 (in z1)
        case("q7", key="q", label=_q7, tolerate=True, req={"cpu": 2000}, seeded=lambda i: 1 if i % 14 == 3 else 0),
        case("q7-min9", key="q", label=_q7, tolerate=True, req={"cpu": 2000}, min_domains=9, max_skew=4, seeded=lambda i: 1 if i % 14 == 3 else 0),
        case("r14", key="r", label=_r14, tolerate=True, req={"cpu": 1500}, max_skew=2, seeded=lambda i: i % 3 == 0 and 1 or 0),
        case("host2", key=HOST, max_skew=2, tolerate=True),                # 200 domains: ids on both sides of 63 / 64
        case("host1", key=HOST, max_skew=1, tolerate=True, seeded=lambda i: 1 if i in (62, 63, 64, 65) else 0),
        case("res1", app="res", max_skew=1, tolerate=True, req={"cpu": 1500}),                # the selector matches the residents, not the ask itself
        case("res7", app="res", max_skew=7, tolerate=True, req={"cpu": 1500}),
        case("res8", app="res", max_skew=8, tolerate=True, req={"cpu": 1500}),                # z0 (72 nodes against 64) opens at 8
        case("sel-z2", zone="z2", max_skew=5),                             # nodeAffinityPolicy Honor: only z2 counts, one present domain
    ]


def counts(node, tmpl):
    """Does a node that carries the key count for the constraint (nodeAffinityPolicy Honor, nodeTaintsPolicy Ignore)?"""
    return not tmpl["zone"] or tmpl["zone"] == node["zone"]


def domain_values(c):
    return sorted({v for v in c["labels"] if v is not None})


def model(c, ask=None):
    ask = c["ask"] if ask is None else ask
    tmpl, skew = c["meta"]["templates"][ask], c["skews"][ask]
    values = domain_values(c)
    D = len(values)
    index = {v: d for d, v in enumerate(values)}
    cnt, cap, nodes, present = [0] * D, [0] * D, [0] * D, [0] * D
    for i, node in enumerate(c["meta"]["nodes"]):
        if c["labels"][i] is None or not counts(node, tmpl):
            continue
        d = index[c["labels"][i]]
        present[d] = 1
        cnt[d] += c["matching"][i]
        k, _ = hg.replicas(node, tmpl)
        cap[d] += k
        nodes[d] += 1 if k >= 1 else 0
    here = [d for d in range(D) if present[d]]
    under = len(here) < c["min_domains"]
    pin = -1
    if c["self_match"]:
        if here and not under:
            M = min(cnt[d] + cap[d] for d in here)
            pin = min(d for d in here if cnt[d] + cap[d] == M)
            floor = M
        else:
            floor = 0
        copies = [min(max(floor + skew - cnt[d], 0), cap[d]) for d in range(D)]
    else:
        floor = 0 if under or not here else min(cnt[d] for d in here)
        copies = [cap[d] if cnt[d] - floor <= skew else 0 for d in range(D)]
    rows = [[cnt[d], cap[d], nodes[d], copies[d]] for d in range(D)]
    most = max(copies + [0])
    cells = [sum(copies), sum(1 for x in copies if x >= 1), most, 0, sum(cap), len(here), floor, pin,
             sum(1 for d in range(D) if cap[d] >= 1 and copies[d] == cap[d]), sum(1 for d in range(D) if 0 < copies[d] < cap[d]),
             sum(1 for d in range(D) if cap[d] >= 1 and copies[d] == 0), copies.index(most) if most >= 1 else -1, None, skew, sum(nodes), 0]
    return rows, cells


def domain_of_nodes(c):
    index = {v: d for d, v in enumerate(domain_values(c))}
    return [index[v] if v is not None else -1 for v in c["labels"]]


_LOOPS = {}


def clone_loop(c):
    """→ (copies per domain, unplaced): the oracle's sequential allocation loop over model total + 3 clones of the case's ask."""
    import numpy as np

    import _oracle as orc
    if c["name"] not in _LOOPS:
        total = model(c)[1][0]
        placed = orc.Oracle(hg.clones(c["snapshot"], c["ask"], total + 3)).allocate_sequential()
        dom = np.array(domain_of_nodes(c))
        where = dom[placed[placed >= 0]]
        assert (where >= 0).all()
        _LOOPS[c["name"]] = (np.bincount(where, minlength=len(domain_values(c))).astype(np.int64), int((placed < 0).sum()))
    return _LOOPS[c["name"]]


def status_cluster():
    """One cluster with the asks whose status is NOT 0 under some plugin lists → (snapshot, {uid: index})."""
    nodes = [hg._node(i)[0] for i in range(hg.PERIOD)]
    anti = _spread_ask("s-anti", {"cpu": 250}, [_constraint(ZONE, 2)])
    anti[0]["metadata"]["labels"]["role"] = "anti"  # (its term matches itself alone: no other ask gains an existing-anti-affinity constraint)
    anti[0]["spec"]["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": {"role": "anti"}}, "topologyKey": HOST}]}}
    asks = [
        _spread_ask("s-one", {"cpu": 250}, [_constraint(ZONE, 2)]),
        _spread_ask("s-selector", {"cpu": 250}, [_constraint(ZONE, 2)], zone="z2"),
        _spread_ask("s-two", {"cpu": 250}, [_constraint(ZONE, 2), _constraint(HOST, 3)]),
        anti,
        hg._ask("s-routed", hg.MAIN_REQ, pvc=True),
        hg._ask("s-plain", hg.MAIN_REQ),
    ]
    return {"nodes": nodes, "pods": [a[0] for a in asks]}, {a[1]["uid"]: i for i, a in enumerate(asks)}
