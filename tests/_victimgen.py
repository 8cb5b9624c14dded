"""Designed clusters for preemption victims (ykpred_preempt_victims): snapshots whose resident pods carry priorities and uids that fix
order(n) — the node's pods in a tier by (priority ascending, uid ascending bytewise) — and a plain model of need(ask, node): 0 when the
ask fits as the node stands, k >= 1 when it fits once the first k pods of order(n) in tiers < limit are gone and not before, NEVER else.

Pure Python, `random.Random(seed)` only; the pieces and the tier rules come from tests/_reachgen.py and tests/_preemptgen.py. Every
population records the need it meant in meta["intended"][(ask uid, node name)]:

  lengths              victim lists of length 0, 1, 2, 3, 4, 5, 7, 8, 9: every answer 1..len and never on each; lists of 63, 64 and 65:
                       the answers 1, len and both sides of the first two bisection midpoints; prefixes that end mid-tier
  resource_exact       free + the prefix sum of the first k victims equal to the request exactly, and that sum +- 1, in each of the eight
                       dimensions, free amounts beside 2^53 and sums ending at 2^63 - 1
  slots                nodes full by pod count and short of nothing else, cured by zero-request pods: need = the slots missing
  ports                a port triple with two holders in one tier and in two tiers (the first holder frees it), a holder behind two
                       others, a holder of equal priority where the uid decides who goes first
  order                two pods of equal priority whose uid order decides the need; opted-out pods and pods at or above the last bound
                       beside them, in no list; the best node by the exact count where the whole-tier count names another
  limits               two victims per tier, asks of every limit 0..T and every need 1..2T
  gaps                 a node with no victims between two full ones, in that order (nothing is shuffled)
  shut                 _reachgen.shut: pairs shut by a taint, a selector, NodeName or a frozen topology verdict beside siblings that
                       open — one resident per tier there, so the level it records IS the need

Each returns (snapshot, bounds, meta). Every population but `gaps` also holds _reachgen's LADDER (one resident per tier: need == level)
and roomy nodes, so that every outcome occurs and never stays the minority."""
import random

import _reachgen
from _preemptgen import DIMS, I64_MAX, P53, _conflict, make_node, resident
from _reachgen import BIG, BOUNDS, NEVER, OPT_OUT, T80, ReachModel, asker, tier_priority

LONG = (63, 64, 65)
SHORT = (0, 1, 2, 3, 4, 5, 7, 8, 9)


def midpoints(length):
    """The first bisection midpoint over (0, length] and the two second ones: lo + (hi - lo) // 2 from (0, len), (0, m), (m, len)."""
    m = length // 2
    return m, m // 2, m + (length - m) // 2


def placed(uid, prio, req=None, ports=None, opt_out=False):
    """A resident with an explicit priority (0 is left out of the document: a missing spec.priority counts as 0)."""
    pod = resident(uid, req, ports)
    if prio != 0:
        pod["spec"]["priority"] = prio
    if opt_out:
        pod["metadata"]["annotations"] = {OPT_OUT: "false"}
    return pod


def spread_tiers(bounds, count, rng):
    """count priorities in tiers 0..T-1, non-decreasing tier by position, every tier used when count allows; shuffled order of equal
    ones is left to the uids."""
    T = len(bounds)
    tiers = sorted(rng.randrange(T) for _ in range(count))
    for t in range(min(T, count)):
        tiers[(count * t) // min(T, count)] = t
    tiers.sort()
    return [tier_priority(bounds, t, rng) for t in tiers]


class _Population(_reachgen._Population):
    def finish(self, roomy=None, shuffle=True, ladder=True, **more):
        if ladder:
            self.ladder()   # (one resident per tier: the level it records is the need)
            for i in range(len(self.nodes) // 2 + 2 if roomy is None else roomy):
                self.nodes.append(make_node(f"room-{i}", {d: I64_MAX for d in DIMS}, [placed(f"room-{i}-r", self.bounds[0] - 1, {"cpu": 10})],
                                            labels={"zone": "zb"}))
        if shuffle:
            self.rng.shuffle(self.nodes)
            self.rng.shuffle(self.asks)
        return arrange({"nodes": self.nodes, "pods": self.asks}, list(self.bounds),
                       dict(intended=self.intended, rule=self.rule, rules=sorted(set(self.rule.values())), T=self.T, **more))


def arrange(snapshot, bounds, meta):
    """Orders the asks so that neighbours differ in (need counts, limit): greedily from the largest group left."""
    model = VictimModel(snapshot, bounds)
    names = [n["metadata"]["name"] for n in snapshot["nodes"]]
    groups = {}
    for ask in snapshot["pods"]:
        uid = ask["metadata"]["uid"]
        needs = [model.need(uid, n, True) for n in names]
        groups.setdefault((tuple(sorted(needs)), model.asks[uid][2]), []).append(ask)
    arranged, last = [], None
    while groups:
        key = max((k for k in groups if k != last), key=lambda k: len(groups[k]), default=last)
        arranged.append(groups[key].pop())
        if not groups[key]:
            del groups[key]
        last = key
    return {"nodes": snapshot["nodes"], "pods": arranged}, bounds, meta


# ---- (1) lengths -------------------------------------------------------------------------------------------------------------------------
def lengths(seed, T=3):
    """ln-<len>: nothing free, `len` residents of 100m over the tiers, a kept pod above the last bound. Ask a-ln-<k> wants 100m x k: need k
    where k <= len, never beyond. lg-<len> (63 / 64 / 65): residents of 10m; the asks want 10m x k for k = 1, len and both sides of the
    first two midpoints of every long length — on each long node need k or never."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    for length in SHORT:
        prios = spread_tiers(b, length, rng)
        pods = [placed(f"ln-{length}-v{i:02d}", p, {"cpu": 100}) for i, p in enumerate(prios)] + [placed(f"ln-{length}-keep", b[-1], {"cpu": 50})]
        rng.shuffle(pods)
        pop.nodes.append(make_node(f"ln-{length}", {"cpu": 100 * length + 50, "memory": 1 << 40}, pods))
    for k in range(1, 11):
        ask = asker(f"a-ln-{k}", b, T, {"cpu": 100 * k, "memory": 1 << 20})
        pop.asks.append(ask)
        for length in SHORT:
            pop.pair(ask["metadata"]["uid"], f"ln-{length}", k if k <= length else NEVER, f"length {length}")
    ks = set()
    for length in LONG:
        prios = spread_tiers(b, length, rng)
        pods = [placed(f"lg-{length}-v{i:02d}", p, {"cpu": 10}) for i, p in enumerate(prios)]
        rng.shuffle(pods)
        pop.nodes.append(make_node(f"lg-{length}", {"cpu": 10 * length, "memory": 1 << 19}, pods))
        ks |= {1, length} | {m + s for m in midpoints(length) for s in (0, 1)}
    for k in sorted(ks):
        ask = asker(f"a-lg-{k}", b, T, {"cpu": 10 * k, "memory": 1 << 19})   # (memory keeps them off the ln- nodes' free 50m ... and on lg-)
        pop.asks.append(ask)
        for length in LONG:
            pop.pair(ask["metadata"]["uid"], f"lg-{length}", k if k <= length else NEVER, f"length {length}")
    return pop.finish(long=LONG, short=SHORT)


# ---- (2) resources at the prefix sum ----------------------------------------------------------------------------------------------------
def resource_exact(seed, T=3):
    """Node rx-<j>-<k>: five residents in tiers 0, 0, 1, 1, 2 (T = 1: all in tier 0) requesting 2..9 of every dimension; dimension i has the
    magnitude of _reachgen.resource_boundaries. Three asks request S_k - 1, S_k and S_k + 1 of dimension j — S_k = free_j + the requests of
    the first k residents in order — for k = 1, 3 (prefixes that end MID-TIER) and 5. Intended: the smallest k' with S_k' >= the request."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    tiers = [min(t, T - 1) for t in (0, 0, 1, 1, 2)]
    for j, d in enumerate(DIMS):
        for k in (1, 3, 5):
            name = f"rx-{j}-{k}"
            prios = sorted(tier_priority(b, t, rng) for t in tiers)
            sizes = {o: [rng.randrange(2, 10) for _ in prios] for o in DIMS}
            free = {}
            for i, o in enumerate(DIMS):
                mag = ("small", "across", "above", "ends")[i % 4]
                free[o] = {"small": rng.randrange(20, 30), "across": P53 - sum(sizes[o][:k]), "above": P53 + 1, "ends": I64_MAX - 1 - sum(sizes[o])}[mag]
            pods = [placed(f"{name}-v{i}", p, {o: sizes[o][i] for o in DIMS}) for i, p in enumerate(prios)]   # (uid order == position)
            rng.shuffle(pods)
            alloc = {o: free[o] + sum(sizes[o]) for o in DIMS}
            assert all(0 <= v <= I64_MAX for v in alloc.values())
            pop.nodes.append(make_node(name, alloc, pods))
            S = [free[d] + sum(sizes[d][:i]) for i in range(len(prios) + 1)]
            for delta in (-1, 0, 1):
                req = {o: free[o] for o in DIMS if o != d and free[o] > 0 and rng.random() < 0.5}
                req[d] = S[k] + delta
                want = next((i for i in range(len(S)) if S[i] >= req[d]), NEVER)
                pop.pair(asker(f"a-{name}-{delta + 1}", b, T, req), name, want, ("one below", "exact", "one above")[delta + 1])
    return pop.finish()


# ---- (3) pod slots as the only binder ------------------------------------------------------------------------------------------------------
def slots(seed, T=3):
    """sl-<k>: plenty of everything, six zero-request residents over the tiers and one kept pod; allowed = count + 1 - k, so exactly k of
    them must go. The half ask (limit 1) sees only tier 0's."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    asks = [asker("a-slot-nothing", b, T, {}), asker("a-slot-milli", b, T, {"cpu": 1}), asker("a-slot-half", b, 1, {})]
    pop.asks += asks
    for k in range(1, 8):
        name = f"sl-{k}"
        prios = spread_tiers(b, 6, rng)
        pods = [placed(f"{name}-v{i}", p, {}) for i, p in enumerate(prios)] + [placed(f"{name}-keep", b[-1] + 1, {"cpu": 10})]
        rng.shuffle(pods)
        pop.nodes.append(make_node(name, BIG, pods, allowed=len(pods) + 1 - k))
        tier0 = sum(1 for p in prios if p < b[0])
        for a in asks:
            length = tier0 if a is asks[2] else 6
            pop.pair(a["metadata"]["uid"], name, k if k <= length else NEVER, f"{k} slots missing")
    pop.nodes.append(make_node("sl-roomy", BIG, [placed("sl-roomy-r", b[0] - 1, {})], allowed=2))
    for a in asks:
        pop.pair(a["metadata"]["uid"], "sl-roomy", 0, "a slot is free")
    return pop.finish()


# ---- (4) host ports: the first holder frees the triple -----------------------------------------------------------------------------------
def ports(seed, T=3):
    """Nodes short of nothing but the host port the ask wants; every resident holds a port of its own unless named a holder of T80."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    own = lambda i: [("10.0.0.1", "TCP", 3000 + i)]   # noqa: E731
    want = asker("a-port", b, T, {"cpu": 1}, ports=[T80])
    half = asker("a-port-half", b, 1, {"cpu": 1}, ports=[("0.0.0.0", None, 80)])
    free = asker("a-port-free", b, T, {"cpu": 1}, ports=[("10.0.0.1", "TCP", 81)])
    pop.asks += [want, half, free]
    lo, mid, top = tier_priority(b, 0), tier_priority(b, min(1, T - 1)), tier_priority(b, T - 1)

    def scene(name, residents, need, need_half):
        """residents: (uid suffix, priority, holds T80) in any order."""
        pods = [placed(f"{name}-{s}", p, {"cpu": 10}, ports=[T80] if holds else own(i)) for i, (s, p, holds) in enumerate(residents)]
        rng.shuffle(pods)
        pop.nodes.append(make_node(name, BIG, pods))
        pop.pair("a-port", name, need, name)
        pop.pair("a-port-half", name, need_half, "lower limit: " + name)
        pop.pair("a-port-free", name, 0, "a port nobody holds")

    in_tier0 = lambda p: p < b[0]   # noqa: E731
    # two holders in ONE tier, at one priority, behind a pod of lower priority: the first of them by uid frees the triple
    scene("pp-same", [("x", lo - 1, False), ("h-b", lo, True), ("h-a", lo, True)], 2, 2)
    # two holders in TWO tiers (T == 1: two priorities of the one tier): the lower one frees it
    scene("pp-two", [("h0", lo, True), ("m", mid, False), ("h2", top, True)], 1, 1)
    # the holder behind two others
    scene("pp-last", [("x0", lo - 2, False), ("x1", lo - 1, False), ("h", top, True)], 3, 3 if in_tier0(top) else NEVER)
    # equal priority: the holder's uid sorts behind its neighbour's / in front of it
    scene("pp-uid-late", [("b-holder", lo, True), ("a-other", lo, False)], 2, 2)
    scene("pp-uid-early", [("a-holder", lo, True), ("b-other", lo, False)], 1, 1)
    # the holder is in no tier / opted out
    scene("pp-kept", [("x", lo, False), ("h", b[-1], True)], NEVER, NEVER)
    pods = [placed("pp-out-h", lo, {"cpu": 10}, ports=[T80], opt_out=True), placed("pp-out-x", lo, {"cpu": 10}, ports=own(9))]
    pop.nodes.append(make_node("pp-out", BIG, pods))
    pop.pair("a-port", "pp-out", NEVER, "holder opted out")
    return pop.finish()


# ---- (5) the order itself ------------------------------------------------------------------------------------------------------------------
def order(seed, T=3):
    """eq: two residents of ONE priority — eq-b (300m) is listed first, eq-a (100m) sorts first: an ask of 300m needs both, by uid order;
    listed order would need one. Beside them an opted-out pod of the lowest priority and a pod at the last bound: in no list. bn-a / bn-b:
    the best node by the exact count (bn-a: 2 of its 5) where the whole-tier count (5 against 3) names bn-b."""
    pop = _Population(seed, T)
    b = pop.bounds
    lo = tier_priority(b, 0)
    pods = [placed("eq-b", lo, {"cpu": 300}), placed("eq-a", lo, {"cpu": 100}), placed("eq-out", lo - 3, {"cpu": 400}, opt_out=True),
            placed("eq-top", b[-1], {"cpu": 400})]
    pop.nodes.append(make_node("eq", {"cpu": 1200, "memory": 4 << 30, DIMS[3]: 1}, pods))
    for cpu, need in ((100, 1), (101, 2), (300, 2), (400, 2), (401, NEVER)):
        pop.pair(asker(f"a-eq-{cpu}", b, T, {"cpu": cpu, "memory": 4 << 30, DIMS[3]: 1}), "eq", need, "uid order decides" if cpu in (101, 300) else "order")
    # the best node: memory keeps the ask off everything else, a scalar off the ladder and the roomy nodes
    pods = [placed(f"bn-a-v{i}", lo, {"cpu": 40}) for i in range(5)]
    pop.nodes.append(make_node("bn-a", {"cpu": 200, "memory": 2 << 30, DIMS[4]: 1}, pods))
    pods = [placed("bn-b-v0", lo, {"cpu": 20}), placed("bn-b-v1", lo, {"cpu": 20}), placed("bn-b-v2", lo, {"cpu": 100})]
    pop.nodes.append(make_node("bn-b", {"cpu": 140, "memory": 2 << 30, DIMS[4]: 1}, pods))
    ask = asker("a-bn", b, T, {"cpu": 80, "memory": 2 << 30, DIMS[4]: 1})
    pop.pair(ask, "bn-a", 2, "best node")
    pop.pair("a-bn", "bn-b", 3, "best node")
    return pop.finish(roomy=6, best={"a-bn": ("bn-a", 1, 2)}, absent=("eq-out", "eq-top"))


# ---- (6) limits -----------------------------------------------------------------------------------------------------------------------------
def limits(seed, T=3):
    """li: nothing free, two 100m residents per tier. Asks of every limit 0..T request 100m x k, k = 1..2T: need k when 2 x limit reaches it."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    pods = [placed(f"li-t{t}-{i}", tier_priority(b, t, rng), {"cpu": 100}) for t in range(T) for i in range(2)]
    rng.shuffle(pods)
    pop.nodes.append(make_node("li", {"cpu": 200 * T, "memory": 1 << 40}, pods))
    pop.nodes.append(make_node("li-free", {"cpu": 200 * T, "memory": 1 << 40}, []))
    for k in range(1, 2 * T + 1):
        for limit in range(T + 1):
            ask = asker(f"a-li-{k}-{limit}", b, limit, {"cpu": 100 * k})
            pop.pair(ask, "li", k if k <= 2 * limit else NEVER, f"need {k}, limit {limit}")
            pop.pair(ask["metadata"]["uid"], "li-free", 0, "fits as it stands")
    ask = asker("a-li-policy", b, T, {"cpu": 100}, never=True)
    pop.pair(ask, "li", NEVER, "preemptionPolicy: Never")
    return pop.finish()


# ---- (7) a node with no victims between two full ones -------------------------------------------------------------------------------------
def gaps(seed, T=3):
    """gp-0 and gp-2 hold four 100m residents and nothing free; gp-1 between them holds one pod in no tier; gp-3 is free. In this order:
    the segment of gp-1 is empty and its neighbours' rows touch."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    for n in (0, 2):
        pods = [placed(f"gp-{n}-v{i}", p, {"cpu": 100}) for i, p in enumerate(spread_tiers(b, 4, rng))]
        pop.nodes.append(make_node(f"gp-{n}", {"cpu": 400, "memory": 1 << 40}, pods))
    pop.nodes.insert(1, make_node("gp-1", {"cpu": 400, "memory": 1 << 40}, [placed("gp-1-keep", b[-1], {"cpu": 400})]))
    pop.nodes.append(make_node("gp-3", {"cpu": 400, "memory": 1 << 40}, []))
    for k in range(1, 6):
        ask = asker(f"a-gp-{k}", b, T, {"cpu": 100 * k})
        pop.asks.append(ask)
        for n in (0, 2):
            pop.pair(ask["metadata"]["uid"], f"gp-{n}", k if k <= 4 else NEVER, "full node")
        pop.pair(ask["metadata"]["uid"], "gp-1", NEVER, "no victims")
        pop.pair(ask["metadata"]["uid"], "gp-3", 0 if k <= 4 else NEVER, "free node")
    return pop.finish(shuffle=False, ladder=False)


def shut(seed, T=3):
    snapshot, bounds, meta = _reachgen.shut(seed, T)
    return arrange(snapshot, bounds, meta)


POPULATIONS = {"lengths": (lengths, 3), "lengths_1": (lengths, 1), "lengths_8": (lengths, 8), "resource_exact": (resource_exact, 3),
               "resource_exact_8": (resource_exact, 8), "slots": (slots, 3), "ports": (ports, 3), "ports_1": (ports, 1), "order": (order, 3),
               "limits": (limits, 3), "limits_8": (limits, 8), "limits_1": (limits, 1), "gaps": (gaps, 3), "shut": (shut, 3)}


def population(name, seed):
    fn, T = POPULATIONS[name]
    return fn(seed, T)


def geometry(seed, n_nodes, n_asks=70, T=3, most=6):
    """The shape of a launch: n_nodes nodes with random free cpu and 0..most residents of random priorities (so: random segment lengths,
    some empty), and n_asks asks that are n_asks DISTINCT (request, limit) tasks. No intended needs: the model decides."""
    rng = random.Random(seed * 1000 + n_nodes)
    b = BOUNDS[T]
    nodes = []
    for n in range(n_nodes):
        count = rng.randrange(0, most + 1)
        pods = [placed(f"g{n}-v{rng.randrange(10 ** 6):06d}-{i}", rng.randrange(b[0] - 5, b[-1] + 3), {"cpu": rng.randrange(1, 40)}) for i in range(count)]
        used = sum(int(p["spec"]["containers"][0]["resources"]["requests"]["cpu"][:-1]) for p in pods)
        nodes.append(make_node(f"g{n:04d}", {"cpu": used + rng.randrange(0, 60), "memory": 1 << 40}, pods, allowed=rng.choice((2, 4, 110))))
    asks = [asker(f"a-g{i}", b, i % (T + 1), {"cpu": 1 + 2 * i}) for i in range(n_asks)]
    rng.shuffle(asks)
    return {"nodes": nodes, "pods": asks}, list(b), {"T": T}


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
class VictimModel(ReachModel):
    """ReachModel with the victim order: self.orders[node] = positions in the node's pod list of its pods in a tier, by (priority, uid)."""

    def __init__(self, snapshot, bounds):
        super().__init__(snapshot, bounds)
        self.orders, self.uids = {}, {}
        for n in snapshot["nodes"]:
            keyed = sorted((p["spec"].get("priority") or 0, p["metadata"]["uid"].encode(), i) for i, p in enumerate(n["pods"]) if self.tier(p) >= 0)
            self.orders[n["metadata"]["name"]] = [i for _, _, i in keyed]
            self.uids[n["metadata"]["name"]] = [p["metadata"]["uid"] for p in n["pods"]]

    def victims(self, node, limit):
        """order(node) cut at the limit: positions in the node's pod list."""
        pods = self.nodes[node][2]
        return [i for i in self.orders[node] if pods[i][2] < limit]

    def victim_uids(self, node, limit):
        return [self.uids[node][i] for i in self.victims(node, limit)]

    def need(self, uid, node, frozen, plugins=("*",)):
        """frozen: the verdict of every plugin but NodeResourcesFit and NodePorts on the pair (PreFilter rejections included)."""
        fit_on, ports_on = ("*" in plugins or "NodeResourcesFit" in plugins), ("*" in plugins or "NodePorts" in plugins)
        request, wanted, limit = self.asks[uid]
        alloc, allowed, pods = self.nodes[node]
        if not frozen:
            return NEVER
        victims = self.victims(node, limit)
        for k in range(len(victims) + 1):
            gone = set(victims[:k])
            left = [p for i, p in enumerate(pods) if i not in gone]
            free = {d: alloc.get(d, 0) - sum(req.get(d, 0) for req, _, _ in left) for d in request}
            used = {t for _, held, _ in pods for t in held} - {t for i in gone for t in pods[i][1]}   # a SET: the first holder frees it
            fits = not fit_on or (len(left) + 1 <= allowed and all(q <= free[d] for d, q in request.items() if q > 0))
            if fits and not (ports_on and any(_conflict(w, used) for w in wanted)):
                return k
        return NEVER

    def level_of(self, node, limit, need):
        """The reach level of a need >= 1: the tier of the last victim of the prefix, plus one."""
        return self.nodes[node][2][self.victims(node, limit)[need - 1]][2] + 1

    def table(self, node_names, dims):
        """Per node, in the given node and dimension order: (uids of order(n), tier_end[T], prefix sums [count][R], used_after [count] =
        the set of (ip, protocol, port) the node still uses once victims 0..i are gone)."""
        out = []
        T = len(self.bounds)
        for n in node_names:
            pods = self.nodes[n][2]
            order = self.victims(n, T)
            tier_end = [sum(1 for i in order if pods[i][2] <= t) for t in range(T)]
            cum = [[sum(pods[i][0].get(d, 0) for i in order[:k + 1]) for d in dims] for k in range(len(order))]
            held = {x for _, ports, _ in pods for x in ports}
            used = [held - {x for i in order[:k + 1] for x in pods[i][1]} for k in range(len(order))]
            out.append(([self.uids[n][i] for i in order], tier_end, cum, used))
        return out


def cells(needs, levels, limit):
    """The 16 cells of one ask from its per-node needs (NEVER = -1) and the levels of the needs >= 1, nodes in index order."""
    out = [0] * 16
    out[0] = sum(1 for k in needs if k == 0)
    out[1] = sum(1 for k in needs if k >= 1)
    out[2] = sum(1 for k in needs if k == NEVER)
    out[4] = limit
    out[6] = -1
    opened = [(levels[n], k, n) for n, k in enumerate(needs) if k >= 1]
    if opened:
        out[5], out[7], out[6] = min(opened)
        out[8] = sum(k for _, k, _ in opened)
    return out


__all__ = ["NEVER", "LONG", "SHORT", "POPULATIONS", "population", "geometry", "VictimModel", "cells", "midpoints"]
