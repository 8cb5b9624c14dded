"""Designed clusters (Kubernetes-JSON snapshots), PreemptionPredicates queries and a plain model of the call.

Independent of the product's generators and of `_gen.py`: pure Python, `random.Random(seed)` only. Where the random queries of
tests/test_gpu_parity.py hardly ever find an index, the populations here put every query ON a rule of predicate_manager.go:141-179:

  resource_edges(...)   the ask's request equals free + the victims removed so far exactly, and that sum +- 1, per dimension (R = 8),
                        victim lists of 1 / 2 / 7 / 300, sums beside 2^53 and ending at 2^63 - 1
  slot_edges(...)       nodes full by pod count; nil, foreign, unknown and repeated victims must not free a slot
  start_rules(...)      every start in 0..len + 2 against one list, the empty list, lists of nil victims only
  incurable(...)        a PreFilter that fails, or a Filter no removal changes, next to a sibling ask that does get an index
  ports(...)            the holder of the wanted host port at every position, wildcard IPs, two holders, two dictionary words
  topology_frozen(...)  PodTopologySpread / InterPodAffinity state is computed BEFORE the victims go
  batch_geometry(...)   1001 queries whose neighbours differ in answer and in victim count (a prefix of any length keeps that)

Each returns (snapshot, queries, meta). queries: [(ask uid, node name, victim uids with None for a nil victim, start)].
meta["intended"][q] is the answer the generator meant, meta["rule"][q] the rule the query sits on, meta["rules"] every rule name of
the population, meta["claims"] the answers the population claims to produce.

Model(snapshot).answer(query, frozen, plugins) restates the call over Python ints: free_r = allocatable_r - requested_r, victims
leave in order, pod slots are len(pods) + 1 <= allowed, host ports are a SET of (ip, protocol, port) with upstream's conflict rule.
`frozen` is the verdict of the plugins no removal can influence (everything but NodeResourcesFit and NodePorts; the PreFilter
state of the two topology plugins is written before the first victim leaves), one boolean per query, which the caller takes from
the oracle's eval_grid with those plugins alone. The model reads quantities itself (plain integers, "<n>m" for cpu) and imports
nothing from the package or the oracle."""
import random

I64_MAX = (1 << 63) - 1
P53 = 1 << 53
HOST = "kubernetes.io/hostname"
PLUGINS = ("NodeUnschedulable", "NodeName", "TaintToleration", "NodeAffinity", "NodePorts", "NodeResourcesFit", "PodTopologySpread",
           "InterPodAffinity")
REMOVAL = ("NodePorts", "NodeResourcesFit")   # the plugins whose Filter reads what RemovePod changes
FROZEN = tuple(p for p in PLUGINS if p not in REMOVAL)
DIMS = ("cpu", "memory", "ephemeral-storage") + tuple(f"example.com/s{j}" for j in range(5))   # R = 8, the engine's most
MAGNITUDES = ("small", "across-2^53", "above-2^53", "ends-at-int64-max")
TAINT = {"key": "dedicated", "value": "x", "effect": "NoSchedule"}
TOLERATION = {"key": "dedicated", "operator": "Equal", "value": "x", "effect": "NoSchedule"}
TOLERATE_UNSCHEDULABLE = {"key": "node.kubernetes.io/unschedulable", "operator": "Exists", "effect": "NoSchedule"}


# ---- snapshot pieces ---------------------------------------------------------------------------------------------------------
def quantity(dim, value):
    return f"{value}m" if dim == "cpu" else str(value)


def make_node(name, alloc, pods, labels=None, taints=(), unschedulable=False, allowed=1000):
    labels = dict(labels or {})
    labels.setdefault(HOST, name)
    allocatable = {d: quantity(d, v) for d, v in alloc.items()}
    allocatable["pods"] = str(allowed)
    return {"metadata": {"name": name, "labels": labels}, "spec": {"taints": list(taints), "unschedulable": unschedulable},
            "status": {"allocatable": allocatable}, "pods": list(pods)}


def _container(req, ports):
    c = {"name": "c", "resources": {"requests": {d: quantity(d, v) for d, v in (req or {}).items()}}}
    if ports:
        c["ports"] = [dict({"hostPort": port, "containerPort": 8000}, **({"hostIP": ip} if ip else {}), **({"protocol": proto} if proto else {}))
                      for ip, proto, port in ports]
    return c


def resident(uid, req=None, ports=None, labels=None):
    """ports: (hostIP or None, protocol or None, hostPort) — None leaves the field out (0.0.0.0 / TCP by HostPortInfo.sanitize)."""
    return {"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": dict(labels or {"app": "res"})},
            "spec": {"containers": [_container(req, ports)]}}


def make_ask(uid, req=None, ports=None, labels=None, **spec):
    out = resident(uid, req, ports, labels or {"app": "ask"})
    out["spec"].update(spec)
    return out


def node_affinity(*terms):
    """Required node affinity. Every argument is one term (the terms are ORed): a list of node names, each of which becomes a
    metadata.name In [name] field requirement of the term (ANDed; a field requirement takes exactly one value)."""
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
        {"matchFields": [{"key": "metadata.name", "operator": "In", "values": [name]} for name in term]} for term in terms]}}}


class _Population:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.nodes, self.asks, self.queries, self.intended, self.rule, self.detail = [], [], [], [], [], []

    def query(self, ask, node, victims, start, intended, rule, **detail):
        """ask: an ask object (added to the snapshot) or the uid of one that is already there."""
        if not isinstance(ask, str):
            self.asks.append(ask)
            ask = ask["metadata"]["uid"]
        self.queries.append((ask, node, list(victims), start))
        self.intended.append(intended)
        self.rule.append(rule)
        self.detail.append(detail)

    def finish(self, claims, **more):
        """Asks and queries are shuffled separately: a query's index says nothing about its ask's index."""
        self.rng.shuffle(self.asks)
        order = list(range(len(self.queries)))
        if more.pop("shuffle_queries", True):
            self.rng.shuffle(order)
        pick = lambda xs: [xs[i] for i in order]   # noqa: E731
        meta = dict(intended=pick(self.intended), rule=pick(self.rule), detail=pick(self.detail), rules=sorted(set(self.rule)),
                    claims=sorted(claims), **more)
        return {"nodes": self.nodes, "pods": self.asks}, pick(self.queries), meta


# ---- (a) resource edges --------------------------------------------------------------------------------------------------------
def _edge_positions(length):
    return sorted({0, length // 2, length - 1})


def _edge_node(rng, name, length, rotation):
    """`length` residents that request every dimension; the one at an edge position requests exactly 1 of each, so that the sums
    S_k - 1 and S_{k-1} coincide there. Dimension d has the magnitude MAGNITUDES[(d + rotation) % 4]: the node's free amount F_d is
    chosen so that, along the victim order, S_mid = 2^53 exactly (across), F = 2^53 + 1 (above), S_last + 1 = 2^63 - 1 (ends)."""
    uids = [f"{name}-r{i}" for i in range(length)]
    order = list(range(length))
    rng.shuffle(order)   # the victim order is not the order of the node's pod list
    edges = _edge_positions(length)
    sizes = {d: [1 if pos in edges else rng.randrange(2, 10) for pos in range(length)] for d in DIMS}   # by position in the victim list
    free, mags = {}, {}
    for j, d in enumerate(DIMS):
        mags[d] = MAGNITUDES[(j + rotation) % 4]
        total, upto_mid = sum(sizes[d]), sum(sizes[d][:length // 2 + 1])
        free[d] = {"small": rng.randrange(0, 50), "across-2^53": P53 - upto_mid, "above-2^53": P53 + 1, "ends-at-int64-max": I64_MAX - 1 - total}[mags[d]]
    pods = [None] * length
    for pos, i in enumerate(order):
        pods[i] = resident(uids[i], {d: sizes[d][pos] for d in DIMS})
    alloc = {d: free[d] + sum(sizes[d]) for d in DIMS}
    assert all(0 <= v <= I64_MAX for v in alloc.values())
    return make_node(name, alloc, pods), [uids[i] for i in order], sizes, free, mags


def resource_edges(seed, long_list=300):
    """One blocking dimension at a time. For the victim list of a node and k at its first, a middle and its last position, three asks
    request S_k - 1, S_k and S_k + 1 of the blocking dimension d (S_k = free_d + the first k + 1 victims' requests) and, of every other
    dimension with even odds, exactly the node's free amount (free == request must pass). Intended: S_k -> k; S_k + 1 -> k + 1, or
    -1 behind the last victim; S_k - 1 = S_{k-1} -> k - 1, or 0 at k = 0, where nothing smaller than 0 can be answered for a list
    that is not empty — the one place where two of the three share an answer, and the rule itself is the reason.
    Then: a dimension the ask does not request on a node over-committed in it; an all-zero request on a node full by pod count."""
    pop = _Population(seed)
    rng = pop.rng
    shapes = [(length, rot) for length in (1, 2, 7) for rot in range(4)] + [(long_list, 1)]
    for length, rot in shapes:
        name = f"edge-{length}-{rot}"
        node, victims, sizes, free, mags = _edge_node(rng, name, length, rot)
        pop.nodes.append(node)
        for d in DIMS:
            for k in _edge_positions(length):
                s_k = free[d] + sum(sizes[d][:k + 1])
                for delta in (-1, 0, 1):
                    req = {o: free[o] for o in DIMS if o != d and free[o] > 0 and rng.random() < 0.5}
                    req[d] = s_k + delta
                    want = k if delta == 0 else ((k + 1 if k + 1 < length else -1) if delta > 0 else max(k - 1, 0))
                    pop.query(make_ask(f"a-{name}-{DIMS.index(d)}-{k}-{delta + 1}", req), name, victims, 0, want,
                              ("one below", "exact", "one above")[delta + 1], dim=d, k=k, length=length, magnitude=mags[d], delta=delta)
    # over-committed in ephemeral-storage (free -25): an ask that does not request it is decided by cpu alone; its sibling that
    # requests 1 byte waits until every resident has gone (free 5)
    over = [resident(f"over-r{i}", {"cpu": 100, "ephemeral-storage": 10}) for i in range(3)]
    pop.nodes.append(make_node("over", {"cpu": 300, "memory": 1 << 30, "ephemeral-storage": 5}, over))
    uids = [p["metadata"]["uid"] for p in over]
    for k in range(3):
        pop.query(make_ask(f"a-over-{k}", {"cpu": 100 * (k + 1)}), "over", uids, 0, k, "unrequested dimension over-committed", k=k)
        pop.query(make_ask(f"a-over-eph-{k}", {"cpu": 100 * (k + 1), "ephemeral-storage": 1}), "over", uids, 0, 2, "requested dimension over-committed", k=k)
    pop.query(make_ask("a-over-eph-6", {"ephemeral-storage": 6}), "over", uids, 0, -1, "requested dimension over-committed", k=3)
    # full by pod count only, and every resource used up: an ask that requests nothing needs one slot
    full = [resident(f"full-r{i}", {"cpu": 250, "memory": 1 << 20}) for i in range(4)]
    pop.nodes.append(make_node("full", {"cpu": 1000, "memory": 4 << 20}, full, allowed=4))
    uids = [p["metadata"]["uid"] for p in full]
    pop.query(make_ask("a-zero-none", {}), "full", uids, 0, 0, "all-zero request, full by pod count")
    pop.query(make_ask("a-zero-explicit", {"cpu": 0, "memory": 0}), "full", uids[::-1], 2, 2, "all-zero request, full by pod count")
    pop.query(make_ask("a-zero-one-milli", {"cpu": 1}), "full", uids, 0, 0, "all-zero request, full by pod count")
    return pop.finish(claims={-1, 0, 1, 2, 3, 4, 6, long_list // 2 - 1, long_list // 2, long_list // 2 + 1, long_list - 2, long_list - 1})


# ---- (b) slot edges ------------------------------------------------------------------------------------------------------------
SLOT_PATTERNS = ("P", "NP", "FP", "UP", "PP", "PRP", "NFUPRNP", "NN", "FU", "PR", "PNRFP", "UUPNPP", "PFRRP", "NPUPFP", "")


def slot_edges(seed):
    """Nodes whose resources are plentiful and whose pod count is allowed - 1, allowed and allowed + 1: the ask needs 0, 1 and 2
    removals. A victim list is written as a pattern: P a resident of the node not yet named, R the resident named last once more,
    N a nil entry, F a pod of another node, U a uid nobody has. Intended: the position of the n-th P at or after which start is
    reached — R, N, F and U free nothing."""
    pop = _Population(seed)
    rng = pop.rng
    foreign = [resident(f"elsewhere-r{i}", {"cpu": 10}) for i in range(4)]
    pop.nodes.append(make_node("elsewhere", {"cpu": 64000, "memory": 1 << 40}, foreign, allowed=110))
    patterns = list(SLOT_PATTERNS) + ["".join(rng.choice("PPPNFUR") for _ in range(rng.randrange(1, 9))) for _ in range(30)]
    serial = 0
    for allowed in (3, 6):
        for need in (0, 1, 2):
            name = f"slots-{allowed}-{need}"
            pods = [resident(f"{name}-r{i}", {"cpu": 10}) for i in range(allowed - 1 + need)]
            pop.nodes.append(make_node(name, {"cpu": 64000, "memory": 1 << 40}, pods, allowed=allowed))
            for pattern in patterns:
                fresh, last, victims, leaves = [p["metadata"]["uid"] for p in pods], None, [], []
                rng.shuffle(fresh)
                for ch in pattern:
                    if ch == "P" and fresh:
                        last = fresh.pop()
                        victims.append(last)
                        leaves.append(True)
                        continue
                    victims.append({"N": None, "F": rng.choice(foreign)["metadata"]["uid"], "U": f"nobody-{rng.randrange(99)}"}.get(ch, last))
                    leaves.append(False)   # (P with no resident left and R before any P are nil entries)
                for start in sorted({0, rng.randrange(0, len(victims) + 2)}):
                    gone, want = 0, -1
                    for i, left in enumerate(leaves):
                        gone += left
                        if i >= start and gone >= need:
                            want = i
                            break
                    serial += 1
                    req = {} if serial % 3 else {"cpu": 10}
                    pop.query(make_ask(f"a-slot-{serial}", req), name, victims, start, want,
                              ("a slot is free", "one removal", "two removals")[need] + ("" if start == 0 else ", start > 0"), pattern=pattern, need=need)
    return pop.finish(claims=set(range(-1, 7)))


# ---- (c) the start rule --------------------------------------------------------------------------------------------------------
def start_rules(seed):
    """One node per cause of the first fit (cpu, a pod slot, a host port), a list of 6 victims whose first fit is at k = 3, every
    start in 0..8: start <= 3 -> 3, 4 and 5 -> start (the fit exists before start), from len on -> -1. Then an ask that fits with
    nothing removed: [] -> -1, [v] -> 0 from start 0 and -1 from start 1; lists of nil victims only -> start while start < len."""
    pop = _Population(seed)
    k, length = 3, 6
    for cause in ("cpu", "slot", "port"):
        name = f"start-{cause}"
        pods = [resident(f"{name}-r{i}", {"cpu": 100}, ports=[(None, None, 7000 + i)]) for i in range(length)]
        # cpu: free 0, the ask needs 400. slot: allowed = count - 3. port: the ask wants the port of the victim at k
        alloc = {"cpu": 600 if cause == "cpu" else 64000, "memory": 1 << 40}
        pop.nodes.append(make_node(name, alloc, pods, allowed=length - k if cause == "slot" else 110))
        victims = [p["metadata"]["uid"] for p in pods][::-1]
        ask = make_ask(f"a-start-{cause}", {"cpu": 400} if cause == "cpu" else {"cpu": 1},
                       ports=[(None, None, 7000 + length - 1 - k)] if cause == "port" else None)
        for start in range(length + 3):
            want = k if start <= k else (start if start < length else -1)
            rule = "start before the first fit" if start <= k else ("start behind the first fit" if start < length else "start from len on")
            pop.query(ask if start == 0 else ask["metadata"]["uid"], name, victims, start, want, f"{rule} ({cause})", cause=cause)
    pods = [resident(f"roomy-r{i}", {"cpu": 100}) for i in range(3)]
    pop.nodes.append(make_node("roomy", {"cpu": 64000, "memory": 1 << 40}, pods))
    v = pods[0]["metadata"]["uid"]
    fits = make_ask("a-fits-already", {"cpu": 100})
    never = make_ask("a-fits-never", {"cpu": 64001})
    pop.query(fits, "roomy", [], 0, -1, "empty list")
    pop.query("a-fits-already", "roomy", [v], 0, 0, "fits already, one victim")
    pop.query("a-fits-already", "roomy", [v], 1, -1, "fits already, one victim")
    for start in range(5):
        pop.query("a-fits-already", "roomy", [None, None, None], start, start if start < 3 else -1, "nil victims only")
    pop.query(never, "roomy", [None, None, None], 0, -1, "nil victims only")
    pop.query("a-fits-never", "roomy", [], 2, -1, "empty list")
    for start in (0, 2):   # a nil entry in front shifts every position by one
        pop.query("a-fits-already", "roomy", [None, v, pods[1]["metadata"]["uid"]], start, start, "nil victims only")
    return pop.finish(claims={-1, 0, 1, 2, 3, 4, 5})


# ---- (d) what no removal cures -------------------------------------------------------------------------------------------------
def incurable(seed):
    """Every node is short of cpu by what its residents hold, so that the sibling ask gets the index of the last resident it needs
    gone; the incurable ask differs from its sibling in ONE attribute and gets -1 whatever the victims are."""
    pop = _Population(seed)
    kinds = {"plain": {}, "tainted": {"taints": [TAINT]}, "cordoned": {"unschedulable": True}, "zoned": {"labels": {"zone": "a"}}}
    victims_of = {}
    for kind, more in kinds.items():
        pods = [resident(f"{kind}-r{i}", {"cpu": 100}) for i in range(5)]
        pop.nodes.append(make_node(kind, {"cpu": 500, "memory": 1 << 40}, pods, **more))
        victims_of[kind] = [p["metadata"]["uid"] for p in pods]
    cases = [   # (rule, node, what the incurable ask carries, what its sibling carries instead)
        ("PreFilter: conflicting metadata.name terms", "plain", {"affinity": node_affinity(["plain", "zoned"])}, {"affinity": node_affinity(["plain"])}),
        ("PreFilter: node outside the node-name set", "plain", {"affinity": node_affinity(["zoned"], ["tainted"])}, {"affinity": node_affinity(["zoned"], ["plain"])}),
        ("Filter: untolerated taint", "tainted", {}, {"tolerations": [TOLERATION]}),
        ("Filter: unschedulable node", "cordoned", {}, {"tolerations": [TOLERATE_UNSCHEDULABLE]}),
        ("Filter: foreign nodeName", "plain", {"nodeName": "zoned"}, {"nodeName": "plain"}),
        ("Filter: selector mismatch", "zoned", {"nodeSelector": {"zone": "b"}}, {"nodeSelector": {"zone": "a"}}),
    ]
    for c, (rule, node, bad, good) in enumerate(cases):
        for k in range(5):
            lists = [victims_of[node], victims_of[node][::-1], [None] + victims_of[node]]
            victims = lists[k % 3]
            shift = 1 if k % 3 == 2 else 0
            start = (0, 0, 1, k, 4)[k]
            want = max(k + shift, start)
            pop.query(make_ask(f"a-bad-{c}-{k}", {"cpu": 100 * (k + 1)}, **bad), node, victims, start, -1, rule, sibling=f"a-good-{c}-{k}")
            pop.query(make_ask(f"a-good-{c}-{k}", {"cpu": 100 * (k + 1)}, **good), node, victims, start, want, "sibling of: " + rule, sibling=f"a-bad-{c}-{k}")
    return pop.finish(claims={-1, 0, 1, 3, 4})


# ---- (e) host ports ------------------------------------------------------------------------------------------------------------
def ports(seed, dictionary_ports=70):
    """Nodes with plenty of everything but host ports. T = ("10.0.0.1", "TCP", 80) is what most asks want."""
    pop = _Population(seed)
    rng = pop.rng
    serial = [0]

    def scene(holders, want_ports, lists, rule, req=None, cpu=None):
        """holders: the ports of the node's residents in pod-list order. lists: (victim positions or None, start, intended)."""
        serial[0] += 1
        name = f"ports-{serial[0]}"
        pods = [resident(f"{name}-r{i}", {"cpu": 100}, ports=p) for i, p in enumerate(holders)]
        pop.nodes.append(make_node(name, {"cpu": cpu if cpu is not None else 64000, "memory": 1 << 40}, pods))
        ask = make_ask(f"a-{name}", req or {"cpu": 1}, ports=want_ports)
        for j, (positions, start, want) in enumerate(lists):
            victims = [None if i is None else pods[i]["metadata"]["uid"] for i in positions]
            pop.query(ask if j == 0 else ask["metadata"]["uid"], name, victims, start, want, rule)

    T = ("10.0.0.1", "TCP", 80)
    other = lambda i: [("10.0.0.1", "TCP", 3000 + i)]   # noqa: E731
    for at in (0, 2, 4):   # the holder first, in the middle, last
        holders = [[T] if i == at else other(i) for i in range(5)]
        scene(holders, [T], [([0, 1, 2, 3, 4], 0, at), ([4, 3, 2, 1, 0], 0, 4 - at), ([i for i in range(5) if i != at], 0, -1)], "holder position")
    scene([other(0), [(None, "TCP", 80)], other(2)], [T], [([0, 1, 2], 0, 1), ([1], 0, 0)], "wildcard holder")
    scene([other(0), other(1), [T]], [("0.0.0.0", None, 80)], [([0, 1, 2], 0, 2), ([2, 1], 1, 1)], "wildcard ask")
    # the same port on another protocol, on a disjoint IP: no holders at all
    scene([[("10.0.0.1", "UDP", 80)], [("10.0.0.2", "TCP", 80)], [T], [("10.0.0.1", "SCTP", 80)]], [T],
          [([0, 1, 2, 3], 0, 2), ([0, 1, 3], 0, -1), ([2], 0, 0)], "same port, other protocol or IP")
    scene([[("10.0.0.1", "UDP", 80)], [("10.0.0.2", "TCP", 80)], other(2)], [T], [([0, 1, 2], 0, 0), ([0, 1, 2], 2, 2)], "same port, other protocol or IP")
    # two holders of overlapping but different triples: both must go, in either order
    scene([[("0.0.0.0", "TCP", 80)], other(1), [T], other(3)], [T], [([0, 1, 2, 3], 0, 2), ([2, 3, 1, 0], 0, 3), ([0, 1, 3], 0, -1), ([2, 0], 0, 1)],
          "two holders, different triples")
    # two holders of the IDENTICAL triple: NodeInfo.UsedPorts is a set, the first removal frees the port
    scene([[T], other(1), [T], other(3)], [T], [([1, 0, 2, 3], 0, 1), ([3, 2, 1, 0], 0, 1), ([0, 2], 1, 1), ([1, 3], 0, -1)], "two holders, identical triple")
    scene([other(0), [T], other(2)], [T], [([1, None, None], 0, 0), ([1, None, None], 2, 2), ([None, 1, None, None], 3, 3), ([None, None], 0, -1)],
          "nil victims behind the holder")
    # the port is free from position 1 on, cpu (free 0, 300 wanted) from position 2 on, and the other way round
    scene([other(0), [T], other(2), other(3)], [T], [([0, 1, 2, 3], 0, 2), ([1, 0, 2, 3], 0, 2), ([0, 2, 3, 1], 0, 3), ([2, 3, 0, 1], 1, 3)],
          "port and cpu cured at different positions", req={"cpu": 300}, cpu=400)
    # more wanted ports than one dictionary word holds: every ask wants a port of its own, each held by one resident
    name, count = "ports-dictionary", dictionary_ports
    pods = [resident(f"{name}-r{i}", {"cpu": 10}, ports=[(None, "TCP", 9000 + i)]) for i in range(count)]
    pop.nodes.append(make_node(name, {"cpu": 64000, "memory": 1 << 40}, pods))
    order = list(range(count))
    rng.shuffle(order)
    victims = [pods[i]["metadata"]["uid"] for i in order]
    for at, i in enumerate(order):
        pop.query(make_ask(f"a-dict-{i}", {"cpu": 1}, ports=[("10.0.0.9", "TCP", 9000 + i)]), name, victims, 0, at, "a dictionary port of its own", port=9000 + i)
    pop.query(make_ask("a-dict-two", {"cpu": 1}, ports=[(None, "TCP", 9000 + order[3]), (None, "TCP", 9000 + order[count - 2])]), name, victims, 0, count - 2,
              "a dictionary port of its own")
    return pop.finish(claims=set(range(-1, count)), identical_triple="two holders, identical triple", dictionary_ports=count + 4)


# ---- (f) topology state is frozen ----------------------------------------------------------------------------------------------
def topology_frozen(seed):
    """Nodes s0-x0, s0-z0 (first half) and s1-y0, s1-w0 (second half: the other shard of a two-way split), x0 .. w0 for short; x0 and
    y0 are zone za, z0 and w0 zone zb. x0, the queried node, is short of cpu by what its five residents hold (100m each); three of them are app=victim.
    y0 holds three app=web pods, nobody else holds any: the zone histogram of selector app=web reads za 3, zb 0 — and what decides
    the verdict ON x0 sits on y0."""
    pop = _Population(seed)
    X, Y = "s0-x0", "s1-y0"   # (node-sharded engines take ranges of the name-sorted node list)
    labels = [{"app": "victim"}, {"app": "other"}, {"app": "victim"}, {"app": "other"}, {"app": "victim"}]
    xs = [resident(f"x0-r{i}", {"cpu": 100}, labels=labels[i]) for i in range(5)]
    web = [resident(f"y0-web{i}", {"cpu": 100}, labels={"app": "web"}) for i in range(3)]
    big = {"cpu": 64000, "memory": 1 << 40}
    pop.nodes += [make_node(X, {"cpu": 500, "memory": 1 << 40}, xs, labels={"zone": "za"}), make_node("s0-z0", big, [], labels={"zone": "zb"}),
                  make_node(Y, big, web, labels={"zone": "za"}), make_node("s1-w0", big, [resident("w0-r0", {"cpu": 100})], labels={"zone": "zb"})]
    victims = [p["metadata"]["uid"] for p in xs]
    matching_first = [victims[i] for i in (0, 2, 4, 1, 3)]   # every app=victim pod has gone before position 3

    def term(app, key=HOST):
        return {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": key}

    def spread(app, key, skew):
        return [{"maxSkew": skew, "topologyKey": key, "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": {"app": app}}}]

    anti = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [term("victim")]}}
    aff = {"podAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [term("victim")]}}
    for k in range(5):
        cpu = {"cpu": 100 * (k + 1)}
        lists = (victims, matching_first)
        pop.query(make_ask(f"a-anti-{k}", cpu, affinity=anti), X, lists[k % 2], 0, -1, "anti-affinity against the victims is not cured", k=k)
        pop.query(make_ask(f"a-plain-{k}", cpu), X, lists[k % 2], 0, k, "sibling without a topology term", k=k)
        pop.query(make_ask(f"a-hostspread-{k}", cpu, topologySpreadConstraints=spread("victim", HOST, 1)), X, lists[k % 2], 0, -1,
                  "hostname skew exceeded by the victims is not cured", k=k)
        pop.query(make_ask(f"a-hostspread-wide-{k}", cpu, topologySpreadConstraints=spread("victim", HOST, 3)), X, lists[k % 2], 0, k,
                  "spread passes, cpu decides", k=k)
        pop.query(make_ask(f"a-aff-{k}", cpu, affinity=aff), X, matching_first, 0, k, "affinity towards a victim survives its removal", k=k)
        pop.query(make_ask(f"a-aff-late-{k}", cpu, affinity=aff), X, matching_first, min(k + 1, 4), min(k + 1, 4),
                  "affinity towards a victim survives its removal", k=k)
        # zone histogram of app=web: za 3 (all on y0), zb 0. maxSkew 2 fails on x0, maxSkew 3 passes
        pop.query(make_ask(f"a-zone-2-{k}", cpu, topologySpreadConstraints=spread("web", "zone", 2)), X, victims, 0, -1, "zone skew exceeded by another node's pods", k=k)
        pop.query(make_ask(f"a-zone-3-{k}", cpu, topologySpreadConstraints=spread("web", "zone", 3)), X, victims, 0, k, "zone skew just met, cpu decides", k=k)
    return pop.finish(claims={-1, 0, 1, 2, 3, 4}, queried=X, remote=Y, remote_web=[p["metadata"]["uid"] for p in web],
                      flips=[f"a-zone-2-{k}" for k in range(5)], shards=([X, "s0-z0"], [Y, "s1-w0"]))


# ---- (g) the shape of a batch --------------------------------------------------------------------------------------------------
GEOMETRY_COUNTS = (1, 63, 64, 65, 129, 1001)
VICTIM_CYCLE = (0, 1, 300, 2)   # "0, 1, 300, 2 and 0 again": an empty list between every two long ones


def batch_geometry(seed, n_queries=1001, long_list=300):
    """Query q has VICTIM_CYCLE[q % 4] victims, so neighbours never share a victim count and an empty list (always -1) sits between
    the long ones. Within a block of 64 the 16 queries of 300 victims get 16 different answers (the ask requests S_k of cpu for a k
    of its own; the first and the last position come up in every block), those of 2 victims alternate 0, 1 and -1, those of one
    victim 0, 0 and -1. The queries are NOT shuffled: every prefix of the list is a batch with the same properties — GEOMETRY_COUNTS
    are the lengths the tests launch. Asks are shuffled, and node q % n is never the node of query q."""
    pop = _Population(seed)
    rng = pop.rng
    sizes = [rng.randrange(1, 10) for _ in range(long_list)]
    pods = [resident(f"long-r{i}", {"cpu": sizes[i]}) for i in range(long_list)]
    small = []
    for j in range(11):
        small.append(make_node(f"pair-{j}", {"cpu": 200, "memory": 1 << 40}, [resident(f"pair-{j}-r{i}", {"cpu": 100}) for i in range(2)]))
    pop.nodes = small[:5] + [make_node("long", {"cpu": sum(sizes), "memory": 1 << 40}, pods)] + small[5:]
    order = list(range(long_list))
    rng.shuffle(order)
    long_victims = [pods[i]["metadata"]["uid"] for i in order]
    prefix = [0]
    for i in order:
        prefix.append(prefix[-1] + sizes[i])
    names = [n["metadata"]["name"] for n in pop.nodes]
    for q in range(n_queries):
        count, turn = VICTIM_CYCLE[q % 4], q // 4
        if count == long_list:
            k = (0, long_list - 1)[turn % 16] if turn % 16 < 2 else 1 + (turn * 37 + 11) % (long_list - 2)
            pop.query(make_ask(f"a-geo-{q}", {"cpu": prefix[k + 1]}), "long", long_victims, 0, k, "long list", k=k)
            continue
        j = next(j for j in range(turn, turn + 11) if small[j % 11]["metadata"]["name"] != names[q % len(names)]) % 11
        uids = [p["metadata"]["uid"] for p in small[j]["pods"]]
        if turn % 2:
            uids = uids[::-1]
        want = (-1, (0, 0, -1)[turn % 3], None, (0, 1, -1)[turn % 3])[q % 4]
        cpu = 300 if want == -1 else 100 * (want + 1)
        pop.query(make_ask(f"a-geo-{q}", {"cpu": cpu}), f"pair-{j}", uids[:count], 0, want, ("empty list", "one victim", None, "two victims")[q % 4])
    snapshot, queries, meta = pop.finish(claims={-1, 0, 1, long_list - 1}, shuffle_queries=False, counts=GEOMETRY_COUNTS)
    asks = snapshot["pods"]
    for q in range(len(queries)):   # the shuffle may leave an ask at the index of its own query: move it on
        if asks[q]["metadata"]["uid"] == queries[q][0]:
            other = (q + 1) % len(asks)
            asks[q], asks[other] = asks[other], asks[q]
    return snapshot, queries, meta


POPULATIONS = {"resource_edges": resource_edges, "slot_edges": slot_edges, "start_rules": start_rules, "incurable": incurable, "ports": ports,
               "topology_frozen": topology_frozen, "batch_geometry": batch_geometry}


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _masks(plugins):
    """plugins: a list of names (PreFilter list = Filter list; "*" = all) or a pair (PreFilter list, Filter list)."""
    pre, filt = plugins if len(plugins) == 2 and not isinstance(plugins[0], str) else (plugins, plugins)
    full = lambda names: set(PLUGINS) if "*" in names else set(names)   # noqa: E731
    return full(pre), full(filt)


def _amount(dim, text):
    return (int(text[:-1]) if text.endswith("m") else 1000 * int(text)) if dim == "cpu" else int(text)


def _requests(pod):
    out = {}
    for c in pod["spec"]["containers"]:
        for dim, text in c["resources"]["requests"].items():
            out[dim] = out.get(dim, 0) + _amount(dim, text)
    return out


def _host_ports(pod):
    """HostPortInfo.sanitize: no hostIP is 0.0.0.0, no protocol is TCP."""
    return [(p.get("hostIP") or "0.0.0.0", p.get("protocol") or "TCP", p["hostPort"]) for c in pod["spec"]["containers"] for p in c.get("ports", [])
            if p.get("hostPort", 0) > 0]


def _conflict(want, used):
    """HostPortInfo.CheckConflict: same protocol and port, and one of the two IPs is the wildcard or they are equal."""
    return any(u[1] == want[1] and u[2] == want[2] and ("0.0.0.0" in (want[0], u[0]) or u[0] == want[0]) for u in used)


class Model:
    def __init__(self, snapshot):
        self.asks = {p["metadata"]["uid"]: (_requests(p), _host_ports(p)) for p in snapshot["pods"]}
        self.nodes = {}
        for n in snapshot["nodes"]:
            alloc = {d: _amount(d, t) for d, t in n["status"]["allocatable"].items() if d != "pods"}
            pods = {p["metadata"]["uid"]: (_requests(p), _host_ports(p)) for p in n["pods"]}
            self.nodes[n["metadata"]["name"]] = (alloc, int(n["status"]["allocatable"]["pods"]), pods)

    def answer(self, query, frozen, plugins=("*",)):
        uid, node, victims, start = query
        pre, filt = _masks(plugins)
        fit_on, ports_on = "NodeResourcesFit" in filt, "NodePorts" in filt
        if not frozen or (fit_on and "NodeResourcesFit" not in pre) or (ports_on and "NodePorts" not in pre):
            return -1   # a PreFilter failed, a Filter no removal changes fails, or a Filter misses its PreFilter state (an Error status)
        request, wanted = self.asks[uid]
        alloc, allowed, pods = self.nodes[node]
        pods = dict(pods)
        free = {d: alloc.get(d, 0) - sum(req.get(d, 0) for req, _ in pods.values()) for d in request}
        used = {t for _, held in pods.values() for t in held}   # NodeInfo.UsedPorts: a set
        for i, v in enumerate(victims):
            if v is not None and v in pods:   # RemovePod; a nil pod and a pod that is not on the node change nothing (:181-192)
                req, held = pods.pop(v)
                for d in free:
                    free[d] += req.get(d, 0)
                used -= set(held)
            if i < start:
                continue
            fits = not fit_on or (len(pods) + 1 <= allowed and all(q <= free[d] for d, q in request.items() if q > 0))
            if fits and not (ports_on and any(_conflict(w, used) for w in wanted)):
                return i
        return -1
