"""Designed clusters for the headroom of asks with required pod (anti-)affinity, with a model over Python ints.

Pure Python, no randomness. The nodes are tests/_headgen.py's (_node: free values at the quotient boundaries, a tainted word of nodes, an
unschedulable node, labels "zone" and "kubernetes.io/hostname"); a case may take the hostname label away from some nodes and put RESIDENT
pods with labels and anti-affinity terms of their own on others (they request nothing, and the node's pod allowance is raised by as
many: free values and free slots stay what _headgen designed). The ask is built with _headgen._ask (labels app=ask) and carries required
podAffinity / podAntiAffinity terms.

case(...) → dict with the snapshot, the meta _headgen's model reads, the ask's terms and the residents. model(case) → (status, key, mode,
rows, cells): rows[d] = [cnt, cap, nodes, copies] per domain id of the key (the rank of the bytewise-sorted label values) with the
OUTSIDE row — the nodes without the key — last, cells = the 16 summary cells, from the rule alone:
    verdict(n)  the static InterPodAffinity Filter against the residents: every affinity key on the node and a pod matching ALL affinity
                terms in the node's domain of every term's key (or no such pod anywhere while the ask matches its own terms: bootstrap);
                no pod matching an anti term in the node's domain of its key; no resident whose anti term matches the ask there
    cap(d)      Σ _headgen.replicas over the nodes of d that pass the verdict
    mode 0      no anti row the ask itself adds to: copies = cap        mode 1: all of them on one key: copies = min(cap, 1)
    status 4    bootstrap with one affinity term and mode 0; status 2: anti rows the ask adds to on two keys, any other bootstrap
clone_loop(case) → where the oracle's sequential loop (the reference's node loop + AssumePod) put model total + 3 clones.
"""
import copy

import _headgen as hg

CELLS, ROW = 16, 4
ZONE, HOST = "zone", "kubernetes.io/hostname"
ASK_LABELS = {"app": "ask"}


def term(key, **labels):
    return {"labelSelector": {"matchLabels": dict(labels)}, "topologyKey": key}


def _matches(t, labels):
    return all(labels.get(k) == v for k, v in t["labelSelector"]["matchLabels"].items())


def _affinity(aff, anti):
    out = {}
    if aff:
        out["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": list(aff)}
    if anti:
        out["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": list(anti)}
    return out


def case(name, n_nodes=hg.PERIOD, req=None, tolerate=True, aff=(), anti=(), residents=None, unlabel=None, extra_asks=0, ask_labels=None,
         label=None):
    """residents: i → list of (labels, anti terms) of further pods on node i; unlabel: i → True to take the hostname label away;
    label: (key, i → value or None) labels the nodes with a further key."""
    built = [hg._node(i) for i in range(n_nodes)]
    nodes, infos = [copy.deepcopy(b[0]) for b in built], [b[1] for b in built]
    on_node = []
    for i, node in enumerate(nodes):
        if unlabel and unlabel(i):
            del node["metadata"]["labels"][HOST]
        if label is not None and label[1](i) is not None:
            node["metadata"]["labels"][label[0]] = label[1](i)
        here = list(residents(i)) if residents else []
        for c, (labels, terms) in enumerate(here):
            uid = f"aff-res-{i}-{c}"
            pod = {"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": dict(labels)},
                   "spec": {"containers": [{"name": "c", "resources": {}}]}}
            if terms:
                pod["spec"]["affinity"] = _affinity((), terms)
            node["pods"].append(pod)
        node["status"]["allocatable"]["pods"] = str(int(node["status"]["allocatable"]["pods"]) + len(here))
        on_node.append([({"app": "res"}, [])] + [(dict(labels), list(terms)) for labels, terms in here])
    req = {"cpu": 250} if req is None else req
    asks = []
    for c in range(1 + extra_asks):  # distinct tasks of the same shape: other requests
        pod, info = hg._ask(f"a-{name}" if c == 0 else f"a-{name}-x{c}", req if c == 0 else {"cpu": 60 + 37 * c}, tolerate=tolerate if c == 0 else c % 3 != 1)
        if ask_labels:
            pod["metadata"]["labels"].update(ask_labels)
        if aff or anti:
            pod["spec"]["affinity"] = _affinity(aff, anti)
        asks.append((pod, info))
    return {"name": name, "snapshot": {"nodes": nodes, "pods": [a[0] for a in asks]},
            "meta": {"nodes": infos, "templates": [a[1] for a in asks]}, "ask": 0, "aff": list(aff), "anti": list(anti),
            "labels": [dict(n["metadata"]["labels"]) for n in nodes], "pods_on": on_node,
            "ask_labels": dict(ASK_LABELS, **(ask_labels or {}))}


def _no_host(i):
    return i % 17 == 0


BLOCKER = ({"app": "ask"}, [])                       # a resident the ask's own anti term matches
OTHER = ({"role": "blk"}, [])
SVC = ({"role": "svc"}, [])
SELF_HOST, SELF_ZONE = term(HOST, app="ask"), term(ZONE, app="ask")


def designed_cases():
    """The cases of the rule's pin table, every status-0 one checked against the clone loop."""
    return [
        case("host-self", anti=[SELF_HOST]),                                                  # one executor per host
        case("zone-self", anti=[SELF_ZONE]),
        case("zone-self-res", anti=[SELF_ZONE], residents=lambda i: [BLOCKER] if i == 3 else []),   # z0 shut by a resident
        case("host-self-1500", req={"cpu": 1500}, anti=[SELF_HOST], unlabel=_no_host,
             residents=lambda i: [BLOCKER] if i in (62, 63, 64, 65) else []),                  # blocked hosts on both sides of 63 / 64, copies outside
        case("host-self-main", req=hg.MAIN_REQ, anti=[SELF_HOST], unlabel=_no_host, residents=lambda i: [BLOCKER] if i % 9 == 2 else []),
        case("host-other", req={"cpu": 1500}, anti=[term(HOST, role="blk")],                   # the term does not match the ask: static
             residents=lambda i: [OTHER] if i in (62, 63, 64, 65) else []),
        case("zone-existing", req={"cpu": 1500}, residents=lambda i: [({"role": "solo"}, [SELF_ZONE])] if i == 3 else []),  # a resident's term matches the ask
        case("aff-svc-host-self", aff=[term(ZONE, role="svc")], anti=[SELF_HOST], residents=lambda i: [SVC] if i in (70, 130) else []),
        case("aff-res", req={"cpu": 1500}, aff=[term(ZONE, role="svc")], residents=lambda i: [SVC] if i == 130 else []),
        case("aff-res-self", req={"cpu": 1500}, aff=[term(ZONE, role="svc")], ask_labels={"role": "svc"},
             residents=lambda i: [SVC] if i == 130 else []),                                   # self-matching, but a match exists: no bootstrap
        case("boot", req={"cpu": 1500}, aff=[term(ZONE, role="svc")], ask_labels={"role": "svc"}),    # no match anywhere: status 4
        case("two-keys", anti=[SELF_HOST, SELF_ZONE]),                                         # status 2
    ]


def _domain_values(c, key):
    return sorted({lab[key] for lab in c["labels"] if key in lab})


def domain_values(c, key=None):
    return _domain_values(c, model(c)[1] if key is None else key)


def _existing_keys(c):
    """Topology keys on which some resident's anti term matches the ask (sorted: the order of the signature's rows)."""
    return sorted({t["topologyKey"] for pods in c["pods_on"] for _, terms in pods for t in terms if _matches(t, c["ask_labels"])})


def verdict(c):
    """→ per node whether the static InterPodAffinity Filter passes the ask there, and whether the ask is in bootstrap."""
    if "_verdict" in c:  # (the asks of a case share labels and terms: one verdict per case)
        return c["_verdict"]
    N = len(c["labels"])
    me = c["ask_labels"]
    self_aff = bool(c["aff"]) and all(_matches(t, me) for t in c["aff"])
    aff_nodes = [i for i in range(N) for labels, _ in c["pods_on"][i] if c["aff"] and all(_matches(t, labels) for t in c["aff"])]
    boot = bool(c["aff"]) and self_aff and not any(t["topologyKey"] in c["labels"][i] for i in aff_nodes for t in c["aff"])
    ok = []
    for n in range(N):
        lab = c["labels"][n]
        good = True
        if c["aff"]:
            if not all(t["topologyKey"] in lab for t in c["aff"]):
                good = False
            elif not all(any(c["labels"][i].get(t["topologyKey"]) == lab[t["topologyKey"]] for i in aff_nodes) for t in c["aff"]):
                good = boot
        for t in c["anti"]:
            k = t["topologyKey"]
            if k in lab and any(c["labels"][i].get(k) == lab[k] and _matches(t, labels) for i in range(N) for labels, _ in c["pods_on"][i]):
                good = False
        for i in range(N):
            for _, terms in c["pods_on"][i]:
                for t in terms:
                    k = t["topologyKey"]
                    if _matches(t, me) and k in lab and c["labels"][i].get(k) == lab[k]:
                        good = False
        ok.append(good)
    c["_verdict"] = (ok, boot)
    return ok, boot


def with_resident(c, node, labels, terms=()):
    """The case after a pod with these labels and anti terms came to stand on node `node` (what AssumePod of a copy does), for the
    model alone: the snapshot is not touched, and neither are the node's free values."""
    out = dict(c, pods_on=[list(p) for p in c["pods_on"]])
    out.pop("_verdict", None)
    out["pods_on"][node].append((dict(labels), list(terms)))
    return out


def model(c, ask=None, one_key=None):
    """→ (status, key, mode, rows, cells). one_key: apply the one-key rule on that key whatever the qualification says (the two-key case)."""
    ask = c["ask"] if ask is None else ask
    tmpl = c["meta"]["templates"][ask]
    me = c["ask_labels"]
    star = sorted({t["topologyKey"] for t in c["anti"] if _matches(t, me)})
    live = [t["topologyKey"] for t in c["aff"]] + [t["topologyKey"] for t in c["anti"]] + _existing_keys(c)
    ok, boot = verdict(c)
    if not live:
        return 3, None, 0, [], [0, 0, 0, 3] + [0] * 12
    coupled = [-1, 0, -1, 2] + [0] * 12
    if one_key is None and len(star) > 1:
        return 2, None, 0, [], coupled
    mode = 1 if star else 0
    key = one_key or (star[0] if star else live[0])
    status = 0
    if boot:
        if len(c["aff"]) == 1 and not star:
            status, mode = 4, 2
        else:
            return 2, None, 0, [], coupled
    values = _domain_values(c, key)
    index = {v: d for d, v in enumerate(values)}
    D = len(values)
    cnt, cap, nodes = [0] * (D + 1), [0] * (D + 1), [0] * (D + 1)
    for i, node in enumerate(c["meta"]["nodes"]):
        d = index.get(c["labels"][i].get(key), D)
        if d < D:
            for labels, terms in c["pods_on"][i]:
                cnt[d] += sum(1 for t in c["anti"] if t["topologyKey"] == key and _matches(t, labels))
                cnt[d] += sum(1 for t in terms if t["topologyKey"] == key and _matches(t, me))  # (pod, term) pairs that match the ask
        k = hg.replicas(node, tmpl)[0] if ok[i] else 0
        cap[d] += k
        nodes[d] += 1 if k >= 1 else 0
    copies = [min(x, 1) if mode == 1 else x for x in cap[:D]] + [cap[D]]
    rows = [[cnt[d], cap[d], nodes[d], copies[d]] for d in range(D + 1)]
    inside = copies[:D]
    most = max(inside + [0])
    cells = [-1 if status == 4 else sum(copies), sum(1 for x in inside if x >= 1), most, status, sum(cap[:D]), sum(1 for x in cnt[:D] if x > 0),
             cap[D], nodes[D], sum(1 for d in range(D) if cap[d] >= 1 and copies[d] == cap[d]), sum(1 for d in range(D) if 0 < copies[d] < cap[d]),
             0, inside.index(most) if most >= 1 else -1, None, mode, sum(nodes), 0]
    return status, key, mode, rows, cells


def domain_of_nodes(c, key):
    index = {v: d for d, v in enumerate(_domain_values(c, key))}
    return [index.get(lab.get(key), len(index)) for lab in c["labels"]]


_LOOPS = {}


def clone_loop(c, count=None, key=None):
    """→ (copies per domain of `key` with the outside row last, unplaced, the node of the first copy): the oracle's sequential allocation
    loop over `count` clones of the case's ask (default: the model's total + 3)."""
    import numpy as np

    import _oracle as orc
    status, mkey, _, rows, cells = model(c)
    key = key or mkey
    count = cells[0] + 3 if count is None else count
    memo = (c["name"], count, key)
    if memo not in _LOOPS:
        placed = orc.Oracle(hg.clones(c["snapshot"], c["ask"], count)).allocate_sequential()
        dom = np.array(domain_of_nodes(c, key))
        where = dom[placed[placed >= 0]]
        first = int(placed[0]) if len(placed) else -1
        _LOOPS[memo] = (np.bincount(where, minlength=len(_domain_values(c, key)) + 1).astype(np.int64), int((placed < 0).sum()), first)
    return _LOOPS[memo]
