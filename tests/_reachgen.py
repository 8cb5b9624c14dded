"""Designed clusters for preemption reach (ykpred_preempt_reach): snapshots whose resident pods carry priorities, priority bounds that
cut them into tiers, and a plain model of the level of every (ask, node) pair.

Pure Python, `random.Random(seed)` only; the snapshot pieces come from tests/_preemptgen.py. Every population puts designed (ask, node)
pairs ON a rule of the level definition and records the level it meant in meta["intended"][(ask uid, node name)] (NEVER = -1):

  resource_boundaries  free + the requests of tiers < L equal to the ask's request exactly, and that sum +- 1, per dimension (R = 8),
                       free amounts beside 2^53 and sums ending at 2^63 - 1; allocatable = free + every resident <= 2^63 - 1
  slots                nodes full by pod count, cured by tiers of zero-request pods: the slots freed by tiers < L below / on / above the need
  ports                the holder of the wanted host port in a tier, two holders of one triple in different tiers, a holder in no tier
  shut                 unschedulable flag, taint, selector, NodeName, hard spread constraint, required anti-affinity — each beside plenty
                       of reclaimable resources, each next to a sibling ask that does get a level
  empty_and_opted_out  tiers that are empty on a node; an opted-out pod holding what would cure the node
  limits               one node at level 3 for an ask of limit 3 and never for its sibling of limit 2; preemptionPolicy: Never
  one_tier             T = 1: the rules above with a single bound
  best_ties            two nodes with equal (level, victim pods), one strictly better on pods, one better on level

Each returns (snapshot, bounds, meta). Every population also holds a LADDER — node j of it is at level j for the ladder ask, one node is
never — so that every level 0..T and never occurs whatever else the population is about.

ReachModel(snapshot, bounds) restates the definition over Python ints: the tier of a resident, the limit of an ask, the reclaim planes
(per tier: summed requests, pod count, the SET of used ports once tiers 0..t are gone) and level(ask, node, frozen) — `frozen` is the
verdict of the plugins no removal moves, which the caller takes from the oracle, exactly as _preemptgen.Model does."""
import random

from _preemptgen import (DIMS, HOST, I64_MAX, P53, REMOVAL, TAINT, TOLERATE_UNSCHEDULABLE, TOLERATION, _conflict, _host_ports, _requests, make_ask,
                         make_node, node_affinity, resident)

NEVER = -1
OPT_OUT = "yunikorn.apache.org/allow-preemption"
BOUNDS = {1: (10,), 3: (100, 200, 300), 8: (-50, 0, 1, 10, 100, 1000, 10 ** 6, 2 * 10 ** 9)}
BIG = {"cpu": 64000, "memory": 1 << 40}
T80 = ("10.0.0.1", "TCP", 80)


# ---- pieces --------------------------------------------------------------------------------------------------------------------------
def tier_priority(bounds, t, rng=None):
    """A priority of tier t: below bounds[t] and, for t > 0, at or above bounds[t - 1]. t == len(bounds): in no tier."""
    if t == len(bounds):
        return bounds[-1] + (rng.randrange(0, 3) if rng else 0)
    low = bounds[t - 1] if t > 0 else bounds[0] - 5
    return rng.randrange(low, bounds[t]) if rng else low


def victim(uid, bounds, t, req=None, ports=None, labels=None, opt_out=False, rng=None):
    """A resident of tier t. A priority of 0 is left out of the document half of the time: a missing spec.priority counts as 0."""
    pod = resident(uid, req, ports, labels)
    prio = tier_priority(bounds, t, rng)
    if prio != 0 or (rng and rng.random() < 0.5):
        pod["spec"]["priority"] = prio
    if opt_out:
        pod["metadata"]["annotations"] = {OPT_OUT: "false", "note": "a \"quoted\" value"}
    return pod


def asker(uid, bounds, limit, req=None, ports=None, never=False, **spec):
    """An ask whose priority gives it `limit` tiers below it."""
    ask = make_ask(uid, req, ports, **spec)
    ask["spec"]["priority"] = bounds[limit - 1] if limit > 0 else bounds[0] - 1
    if never:
        ask["spec"]["preemptionPolicy"] = "Never"
    elif limit % 2:
        ask["spec"]["preemptionPolicy"] = "PreemptLowerPriority"
    return ask


class _Population:
    def __init__(self, seed, T):
        self.rng = random.Random(seed)
        self.T, self.bounds = T, BOUNDS[T]
        self.nodes, self.asks, self.intended, self.rule = [], [], {}, {}

    def pair(self, ask, node, level, rule):
        if not isinstance(ask, str):
            self.asks.append(ask)
            ask = ask["metadata"]["uid"]
        self.intended[(ask, node)] = level
        self.rule[(ask, node)] = rule

    def ladder(self):
        """Node lad-j (j = 0..T) has 100m x (T - j) free and one 100m resident per tier: the ladder ask (100m x T, limit T) is at
        level j there; lad-never has nothing free and nobody to remove. The askers of lower limits stop at their limit."""
        T, b = self.T, self.bounds
        for j in range(T + 1):
            pods = [victim(f"lad-{j}-t{t}", b, t, {"cpu": 100}, rng=self.rng) for t in range(T)]
            self.rng.shuffle(pods)
            self.nodes.append(make_node(f"lad-{j}", {"cpu": 100 * (T - j) + 100 * T, "memory": 1 << 40}, pods))
        self.nodes.append(make_node("lad-never", {"cpu": 100 * T - 1, "memory": 1 << 40}, []))
        for limit in sorted({T, T // 2, 0}):
            ask = asker(f"a-lad-{limit}", b, limit, {"cpu": 100 * T})
            for j in range(T + 1):
                self.pair(ask if j == 0 else ask["metadata"]["uid"], f"lad-{j}", j if j <= limit else NEVER, "ladder")
            self.pair(ask["metadata"]["uid"], "lad-never", NEVER, "ladder")

    def finish(self, roomy=None, **more):
        """Adds the ladder and `roomy` nodes that take almost any ask as they stand (so that never stays the minority), shuffles the
        nodes, and arranges the asks so that neighbours differ in (level counts, limit): greedily from the largest group left."""
        self.ladder()
        for i in range(len(self.nodes) // 2 + 2 if roomy is None else roomy):
            self.nodes.append(make_node(f"room-{i}", {d: I64_MAX for d in DIMS}, [victim(f"room-{i}-r", self.bounds, 0, {"cpu": 10}, rng=self.rng)],
                                        labels={"zone": "zb"}))
        self.rng.shuffle(self.nodes)
        self.rng.shuffle(self.asks)
        snapshot = {"nodes": self.nodes, "pods": self.asks}
        model = ReachModel(snapshot, self.bounds)
        names = [n["metadata"]["name"] for n in self.nodes]
        groups = {}
        for ask in self.asks:   # (the key: the level counts the model gives the ask when no frozen plugin shuts a node, and its limit)
            uid = ask["metadata"]["uid"]
            levels = sorted(model.level(uid, n, True) for n in names)
            groups.setdefault((tuple(levels), model.asks[uid][2]), []).append(ask)
        arranged, last = [], None
        while groups:
            key = max((k for k in groups if k != last), key=lambda k: len(groups[k]), default=last)
            arranged.append(groups[key].pop())
            if not groups[key]:
                del groups[key]
            last = key
        meta = dict(intended=self.intended, rule=self.rule, rules=sorted(set(self.rule.values())), T=self.T, **more)
        return {"nodes": self.nodes, "pods": arranged}, list(self.bounds), meta


# ---- (1) resource boundaries -----------------------------------------------------------------------------------------------------------
def resource_boundaries(seed, T=3):
    """Node rb-<d>-<L>: one resident per tier requesting 2..9 of every dimension; dimension j has the magnitude MAGS[j % 4] on every node — a
    small free amount, S_L = 2^53 exactly, free = 2^53 + 1, or the sum over every tier ending one below 2^63 - 1 — so that an ask sits
    beside a boundary on the nodes it was not designed for as well. Three asks of limit T request
    S_L - 1, S_L and S_L + 1 of the blocking dimension d (S_L = free_d + the requests of tiers < L) and of every other dimension, with
    even odds, exactly the node's free amount. Intended: the smallest L' with S_L' >= the request, never past S_T."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    levels = sorted({1, (T + 1) // 2, T})
    for j, d in enumerate(DIMS):
        for L in levels:
            name = f"rb-{j}-{L}"
            sizes = {o: [rng.randrange(2, 10) for _ in range(T)] for o in DIMS}
            free = {}
            for i, o in enumerate(DIMS):
                mag = ("small", "across", "above", "ends")[i % 4]
                free[o] = {"small": rng.randrange(20, 30), "across": P53 - sum(sizes[o][:L]), "above": P53 + 1, "ends": I64_MAX - 1 - sum(sizes[o])}[mag]
            pods = [victim(f"{name}-t{t}", b, t, {o: sizes[o][t] for o in DIMS}, rng=rng) for t in range(T)]
            rng.shuffle(pods)
            alloc = {o: free[o] + sum(sizes[o]) for o in DIMS}
            assert all(0 <= v <= I64_MAX for v in alloc.values())
            pop.nodes.append(make_node(name, alloc, pods))
            S = [free[d] + sum(sizes[d][:k]) for k in range(T + 1)]
            for delta in (-1, 0, 1):
                req = {o: free[o] for o in DIMS if o != d and free[o] > 0 and rng.random() < 0.5}
                req[d] = S[L] + delta
                want = next((k for k in range(T + 1) if S[k] >= req[d]), NEVER)
                pop.pair(asker(f"a-{name}-{delta + 1}", b, T, req), name, want, ("one below", "exact", "one above")[delta + 1])
    return pop.finish()


# ---- (2) pod slots ---------------------------------------------------------------------------------------------------------------------
def slots(seed, T=3):
    """Nodes with plenty of everything and too many pods. Tier t holds c_t zero-request pods; allowed = count + 1 - need, so the ask needs
    `need` of them gone: need = (the pods of tiers < L) - 1, that number, and one more. An ask that requests nothing needs a slot too."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    asks = [asker("a-slot-nothing", b, T, {}), asker("a-slot-milli", b, T, {"cpu": 1}), asker("a-slot-half", b, max(T // 2, 1), {})]
    for a in asks:
        pop.asks.append(a)
    for L in range(1, T + 1):
        for delta in (-1, 0, 1):
            name = f"sl-{L}-{delta + 1}"
            counts = [rng.randrange(2, 4) for _ in range(T)]
            pods = [victim(f"{name}-t{t}-{i}", b, t, {}, rng=rng) for t in range(T) for i in range(counts[t])]
            keep = [victim(f"{name}-keep", b, T, {"cpu": 10})]
            rng.shuffle(pods)
            need = sum(counts[:L]) + delta
            total = len(pods) + 1
            pop.nodes.append(make_node(name, BIG, pods + keep, allowed=total + 1 - need))
            cum = [sum(counts[:k]) for k in range(T + 1)]
            for a in asks:
                limit = T if a is not asks[2] else max(T // 2, 1)
                want = next((k for k in range(limit + 1) if cum[k] >= need), NEVER)
                pop.pair(a["metadata"]["uid"], name, want, ("slots below the need", "slots on the need", "slots above the need")[delta + 1])
    pop.nodes.append(make_node("sl-roomy", BIG, [victim("sl-roomy-r", b, 0, {})], allowed=2))
    for a in asks:
        pop.pair(a["metadata"]["uid"], "sl-roomy", 0, "a slot is free")
    return pop.finish()


# ---- (3) host ports --------------------------------------------------------------------------------------------------------------------
def ports(seed, T=3):
    """Nodes short of nothing but the host port the ask wants. po-one-<t>: one holder, in tier t. po-two-<t>-<u>: two holders of the
    IDENTICAL triple in tiers t < u — NodeInfo.UsedPorts is a set, the triple goes with the first of them. po-kept: the holder has a
    priority in no tier; po-out: it opted out. The sibling ask wants a port nobody holds."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    other = lambda i: [("10.0.0.1", "TCP", 3000 + i)]   # noqa: E731
    want = asker("a-port", b, T, {"cpu": 1}, ports=[T80])
    half = asker("a-port-half", b, max(T - 1, 1), {"cpu": 1}, ports=[("0.0.0.0", None, 80)])
    free = asker("a-port-free", b, T, {"cpu": 1}, ports=[("10.0.0.1", "TCP", 81)])
    pop.asks += [want, half, free]

    def scene(name, holders, level):
        """holders: tier -> ports of that tier's resident (a tier without an entry holds a pod with a port of its own)."""
        pods = [victim(f"{name}-t{t}", b, t, {"cpu": 10}, ports=holders.get(t, other(t)), rng=rng) for t in range(T + 1)]
        rng.shuffle(pods)
        pop.nodes.append(make_node(name, BIG, pods))
        pop.pair("a-port", name, level, name.rsplit("-", 1)[0] if name[-1].isdigit() else name)
        pop.pair("a-port-half", name, level if 0 <= level <= max(T - 1, 1) else NEVER, "lower limit")
        pop.pair("a-port-free", name, 0, "a port nobody holds")

    for t in range(T):
        scene(f"po-one-{t}", {t: [T80]}, t + 1)
    for t in range(T - 1):
        scene(f"po-two-{t}-{T - 1}", {t: [T80], T - 1: [T80]}, t + 1)
    scene("po-wild-0", {0: [(None, "TCP", 80)]}, 1)
    scene("po-kept", {T: [T80]}, NEVER)
    pods = [victim("po-out-t0", b, 0, {"cpu": 10}, ports=[T80], opt_out=True), victim("po-out-t1", b, min(1, T - 1), {"cpu": 10}, ports=other(1))]
    pop.nodes.append(make_node("po-out", BIG, pods))
    pop.pair("a-port", "po-out", NEVER, "holder opted out")
    return pop.finish()


# ---- (4) what no removal cures ---------------------------------------------------------------------------------------------------------
def shut(seed, T=3):
    """Every node is short of cpu by what its residents hold — one 100m resident per tier, nothing free — so the sibling ask (100m x L) is
    at level L; the shut ask differs from it in ONE attribute and is never."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    kinds = {"plain": {}, "tainted": {"taints": [TAINT]}, "cordoned": {"unschedulable": True}, "zoned": {"labels": {"zone": "a"}},
             "crowded": {"labels": {"zone": "za"}}}
    for kind, more in kinds.items():
        labels = {"app": "victim"} if kind == "crowded" else None
        pods = [victim(f"sh-{kind}-t{t}", b, t, {"cpu": 100}, labels=labels, rng=rng) for t in range(T)]
        pop.nodes.append(make_node(f"sh-{kind}", {"cpu": 100 * T, "memory": 1 << 40}, pods, **more))
    web = [resident(f"sh-web{i}", {"cpu": 100}, labels={"app": "web"}) for i in range(3)]
    pop.nodes.append(make_node("sh-far", BIG, web, labels={"zone": "za"}))
    pop.nodes.append(make_node("sh-empty", BIG, [], labels={"zone": "zb"}))
    term = {"labelSelector": {"matchLabels": {"app": "victim"}}, "topologyKey": HOST}
    anti = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [term]}}
    spread = lambda skew: [{"maxSkew": skew, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule",   # noqa: E731
                            "labelSelector": {"matchLabels": {"app": "web"}}}]
    cases = [   # (rule, node, what the shut ask carries, what its sibling carries instead)
        ("unschedulable node", "sh-cordoned", {}, {"tolerations": [TOLERATE_UNSCHEDULABLE]}),
        ("untolerated taint", "sh-tainted", {}, {"tolerations": [TOLERATION]}),
        ("selector mismatch", "sh-zoned", {"nodeSelector": {"zone": "b"}}, {"nodeSelector": {"zone": "a"}}),
        ("foreign nodeName", "sh-plain", {"nodeName": "sh-zoned"}, {"nodeName": "sh-plain"}),
        ("PreFilter: node outside the node-name set", "sh-plain", {"affinity": node_affinity(["sh-zoned"])}, {"affinity": node_affinity(["sh-plain"])}),
        ("anti-affinity against the victims", "sh-crowded", {"affinity": anti}, {}),
        # zone histogram of app=web: za 3 (all on sh-far), zb 0: maxSkew 2 fails on the za node sh-crowded, maxSkew 3 passes
        ("zone skew exceeded by another node's pods", "sh-crowded", {"topologySpreadConstraints": spread(2)}, {"topologySpreadConstraints": spread(3)}),
    ]
    for c, (rule, node, bad, good) in enumerate(cases):
        for L in sorted({1, T}):
            pop.pair(asker(f"a-shut-{c}-{L}", b, T, {"cpu": 100 * L}, **bad), node, NEVER, rule)
            pop.pair(asker(f"a-open-{c}-{L}", b, T, {"cpu": 100 * L}, **good), node, L, "sibling of: " + rule)
    return pop.finish(roomy=20)


# ---- (5) empty tiers, opted-out pods ---------------------------------------------------------------------------------------------------
def empty_and_opted_out(seed, T=8):
    """em-<k>: nothing free, tiers 0..k-1 hold nobody, tier k holds the one 100m resident -> level k + 1. oo-<k>: the same resident opted
    out, a 50m resident one tier up (where there is one) -> never for 100m. Its sibling asks 50m and gets the tier above."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    full = asker("a-em-100", b, T, {"cpu": 100})
    part = asker("a-em-50", b, T, {"cpu": 50})
    pop.asks += [full, part]
    for k in range(T):
        keep = victim(f"em-{k}-keep", b, T, {"cpu": 500}, rng=rng)
        pop.nodes.append(make_node(f"em-{k}", {"cpu": 600, "memory": 1 << 40}, [victim(f"em-{k}-r", b, k, {"cpu": 100}, rng=rng), keep]))
        pop.pair("a-em-100", f"em-{k}", k + 1, "empty tiers below the cure")
        pop.pair("a-em-50", f"em-{k}", k + 1, "empty tiers below the cure")
        pods = [victim(f"oo-{k}-r", b, k, {"cpu": 100}, opt_out=True, rng=rng)]
        if k + 1 < T:
            pods.append(victim(f"oo-{k}-up", b, k + 1, {"cpu": 50}, rng=rng))
        pop.nodes.append(make_node(f"oo-{k}", {"cpu": 100 + 50 * (len(pods) - 1), "memory": 1 << 40}, pods))
        pop.pair("a-em-100", f"oo-{k}", NEVER, "the cure opted out")
        pop.pair("a-em-50", f"oo-{k}", k + 2 if k + 1 < T else NEVER, "the cure opted out")
    return pop.finish()


# ---- (6) limits ------------------------------------------------------------------------------------------------------------------------
def limits(seed, T=3):
    """li-<L>: nothing free, one 100m resident per tier. Asks of every limit request 100m x L: at level L when the limit reaches it,
    never below. An ask with preemptionPolicy: Never has limit 0 whatever its priority."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    pods = [victim(f"li-t{t}", b, t, {"cpu": 100}, rng=rng) for t in range(T)]
    rng.shuffle(pods)
    pop.nodes.append(make_node("li", {"cpu": 100 * T, "memory": 1 << 40}, pods))
    pop.nodes.append(make_node("li-free", {"cpu": 100 * T, "memory": 1 << 40}, []))
    for L in range(1, T + 1):
        for limit in range(T + 1):
            ask = asker(f"a-li-{L}-{limit}", b, limit, {"cpu": 100 * L})
            pop.pair(ask, "li", L if limit >= L else NEVER, f"level {L}, limit {limit}")
            pop.pair(ask["metadata"]["uid"], "li-free", 0, "fits as it stands")
        ask = asker(f"a-li-{L}-policy", b, T, {"cpu": 100 * L}, never=True)
        pop.pair(ask, "li", NEVER, "preemptionPolicy: Never")
        pop.pair(ask["metadata"]["uid"], "li-free", 0, "fits as it stands")
    return pop.finish()


# ---- (7) one tier ----------------------------------------------------------------------------------------------------------------------
def one_tier(seed, T=1):
    """T = 1: every resident below the bound is a victim of every ask at or above it. Exact / +-1 on cpu, a slot, a port, an opted-out pod."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    pods = [victim(f"ot-r{i}", b, 0, {"cpu": 100}, ports=[("10.0.0.1", "TCP", 80 + i)], rng=rng) for i in range(3)]
    pop.nodes.append(make_node("ot", {"cpu": 350, "memory": 1 << 40}, pods + [victim("ot-keep", b, 1, {"cpu": 40})], allowed=4))
    for cpu, want in ((10, 1), (11, 1), (310, 1), (311, NEVER), (0, 1)):
        pop.pair(asker(f"a-ot-{cpu}", b, 1, {"cpu": cpu} if cpu else {}), "ot", want, "one tier")
        pop.pair(asker(f"a-ot-low-{cpu}", b, 0, {"cpu": cpu} if cpu else {}), "ot", NEVER, "one tier, limit 0")
    pop.pair(asker("a-ot-port", b, 1, {"cpu": 1}, ports=[("10.0.0.1", "TCP", 81)]), "ot", 1, "one tier")
    return pop.finish()


# ---- (8) the best node -----------------------------------------------------------------------------------------------------------------
def best_ties(seed, T=3):
    """All nodes have nothing free in cpu. bt-a and bt-b are alike: tier 0 and tier 1 hold 100m in 2 + 1 pods. bt-c frees the same in
    1 + 1 pods; bt-d frees 200m in tier 0 alone, in 5 pods. Memory tells the asks apart: "a-bt-tie" fits bt-a and bt-b only (equal level 2,
    equal 3 victims: the lower INDEX wins, whatever the names), "a-bt-pods" also bt-c (2 victims beat 3), "a-bt-level" also bt-d (level 1
    beats level 2 in spite of 5 victims)."""
    pop = _Population(seed, T)
    b = pop.bounds

    def node(name, per_tier, memory):
        pods = [victim(f"{name}-t{t}-{i}", b, t, {"cpu": cpu}) for t, cpus in enumerate(per_tier) for i, cpu in enumerate(cpus)]
        pop.nodes.append(make_node(name, {"cpu": sum(sum(c) for c in per_tier), "memory": memory, DIMS[3]: 1}, pods))

    node("bt-a", [[50, 50], [100]], 8 << 30)
    node("bt-b", [[50, 50], [100]], 8 << 30)
    node("bt-c", [[100], [100]], 4 << 30)
    node("bt-d", [[40, 40, 40, 40, 40]], 2 << 30)
    for uid, memory, levels, best in (("a-bt-tie", 8 << 30, {"bt-a": 2, "bt-b": 2, "bt-c": NEVER, "bt-d": NEVER}, ("bt-a", "bt-b")),
                                      ("a-bt-pods", 4 << 30, {"bt-a": 2, "bt-b": 2, "bt-c": 2, "bt-d": NEVER}, ("bt-c",)),
                                      ("a-bt-level", 2 << 30, {"bt-a": 2, "bt-b": 2, "bt-c": 2, "bt-d": 1}, ("bt-d",))):
        ask = asker(uid, b, T, {"cpu": 200, "memory": memory, DIMS[3]: 1})   # (a scalar the ladder nodes do not have)
        pop.asks.append(ask)
        for name, level in levels.items():
            pop.pair(uid, name, level, "best node")
    return pop.finish(roomy=10, best={"a-bt-tie": ("bt-a", "bt-b"), "a-bt-pods": ("bt-c",), "a-bt-level": ("bt-d",)})


POPULATIONS = {"resource_boundaries": (resource_boundaries, 3), "resource_boundaries_8": (resource_boundaries, 8), "slots": (slots, 3),
               "ports": (ports, 3), "shut": (shut, 3), "empty_and_opted_out": (empty_and_opted_out, 8), "limits": (limits, 3),
               "one_tier": (one_tier, 1), "best_ties": (best_ties, 3)}


def population(name, seed):
    fn, T = POPULATIONS[name]
    return fn(seed, T)


def geometry(seed, n_nodes, n_asks=70, T=3):
    """The shape of a launch: n_nodes nodes (off the wave width, across the 256-node block) with random free cpu and random tiers, and
    n_asks asks that are n_asks DISTINCT (request, limit) tasks — three chunks of 32 at 70. No intended levels: the model decides."""
    rng = random.Random(seed * 1000 + n_nodes)
    b = BOUNDS[T]
    nodes = []
    for n in range(n_nodes):
        pods = [victim(f"g{n}-t{t}-{i}", b, t, {"cpu": rng.randrange(1, 40)}, rng=rng) for t in range(T + 1) for i in range(rng.randrange(0, 3))]
        used = sum(_requests(p).get("cpu", 0) for p in pods)
        nodes.append(make_node(f"g{n:04d}", {"cpu": used + rng.randrange(0, 60), "memory": 1 << 40}, pods, allowed=rng.choice((2, 4, 110))))
    asks = [asker(f"a-g{i}", b, i % (T + 1), {"cpu": 1 + i}) for i in range(n_asks)]
    rng.shuffle(asks)
    return {"nodes": nodes, "pods": asks}, list(b), {"T": T}


# ---- the model -------------------------------------------------------------------------------------------------------------------------
class ReachModel:
    def __init__(self, snapshot, bounds):
        self.bounds = list(bounds)
        self.asks = {p["metadata"]["uid"]: (_requests(p), _host_ports(p), self.limit(p)) for p in snapshot["pods"]}
        self.nodes = {}
        for n in snapshot["nodes"]:
            alloc = {d: _amount(d, t) for d, t in n["status"]["allocatable"].items() if d != "pods"}
            pods = [(_requests(p), _host_ports(p), self.tier(p)) for p in n["pods"]]
            self.nodes[n["metadata"]["name"]] = (alloc, int(n["status"]["allocatable"]["pods"]), pods)

    def tier(self, pod):
        """The smallest t with priority < bounds[t]; -1 (never a victim) at or above the last bound or when the pod opted out."""
        if (pod["metadata"].get("annotations") or {}).get(OPT_OUT) == "false":
            return -1
        prio = pod["spec"].get("priority") or 0
        return next((t for t, bound in enumerate(self.bounds) if prio < bound), -1)

    def limit(self, pod):
        if pod["spec"].get("preemptionPolicy") == "Never":
            return 0
        return sum(1 for bound in self.bounds if bound <= (pod["spec"].get("priority") or 0))

    def level(self, uid, node, frozen, plugins=("*",)):
        """frozen: the verdict of every plugin but NodeResourcesFit and NodePorts on the pair (PreFilter rejections included)."""
        fit_on, ports_on = ("*" in plugins or "NodeResourcesFit" in plugins), ("*" in plugins or "NodePorts" in plugins)
        request, wanted, limit = self.asks[uid]
        alloc, allowed, pods = self.nodes[node]
        if not frozen:
            return NEVER
        for L in range(limit + 1):
            left = [p for p in pods if not 0 <= p[2] < L]
            free = {d: alloc.get(d, 0) - sum(req.get(d, 0) for req, _, _ in left) for d in request}
            used = {t for _, held, _ in pods for t in held} - {t for _, held, tier in pods if 0 <= tier < L for t in held}   # a SET
            fits = not fit_on or (len(left) + 1 <= allowed and all(q <= free[d] for d, q in request.items() if q > 0))
            if fits and not (ports_on and any(_conflict(w, used) for w in wanted)):
                return L
        return NEVER

    def victims_below(self, node, L):
        return sum(1 for p in self.nodes[node][2] if 0 <= p[2] < L)

    def planes(self, node_names, dims):
        """The reclaim planes in the given node and dimension order: requests[t][r][n], pods[t][n] as nested lists, and
        used_after[t][n] = the set of (ip, protocol, port) the node still uses once tiers 0..t are gone."""
        T = len(self.bounds)
        req = [[[sum(p[0].get(d, 0) for p in self.nodes[n][2] if p[2] == t) for n in node_names] for d in dims] for t in range(T)]
        cnt = [[sum(1 for p in self.nodes[n][2] if p[2] == t) for n in node_names] for t in range(T)]
        used = [[{x for _, held, _ in self.nodes[n][2] for x in held} - {x for _, held, tier in self.nodes[n][2] if 0 <= tier <= t for x in held}
                 for n in node_names] for t in range(T)]
        return req, cnt, used


def _amount(dim, text):
    return (int(text[:-1]) if text.endswith("m") else 1000 * int(text)) if dim == "cpu" else int(text)


def cells(levels, victims, limit, T=8):
    """The 16 cells of one ask from its per-node levels (NEVER = -1) and per-node victim pods at that level, nodes in index order."""
    out = [0] * 16
    for lv in levels:
        out[9 if lv == NEVER else lv] += 1
    out[11] = limit
    out[13] = -1
    reached = [(lv, victims[n], n) for n, lv in enumerate(levels) if lv >= 1]
    if reached:
        out[12], out[14], out[13] = min(reached)
    return out


__all__ = ["NEVER", "OPT_OUT", "BOUNDS", "POPULATIONS", "population", "geometry", "ReachModel", "cells", "REMOVAL"]
