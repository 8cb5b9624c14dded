"""Designed clusters for preemption explain (ykpred_preempt_explain): the pieces of tests/_reachgen.py / tests/_preemptgen.py put
together so that designed (ask, node) pairs sit ON the rules of the final verdict V — the verdict of the node with every pod of the
tiers below the ask's limit gone — and a plain model of (level, V, elig, class) for every pair.

Pure Python, `random.Random(seed)` only. designed(seed, T) builds ONE population per tier count T (1, 3, 8) that holds every rule and
records what it meant in meta["verdicts"][(ask uid, node name)] = (class, code of V, reasons of V) and meta["rule"]:

  two short resources     removal cures cpu but not memory: the insufficient bits of V differ from those as the node stands; free + every
                          eligible request == request - 1 exactly, beside 2^53; and on an R = 8 node every dimension one short, the
                          scalar sums ending at 2^63 - 1
  ports into resources    the first failure moves 5 -> 6 once the port holder's tier is gone; it stays 5 when the holder opted out or
                          sits at or above the limit
  slots stay full         nodes full by pod count stay full after the removal (reason bit 0 in V)
  wrong tiers             elig == 0 because the only pods sit in tiers >= the limit, next to a sibling ask of a higher limit for which
                          the same node has a level, and one for which it is not enough
  unresolvable            unschedulable flag, taint, selector, NodeName, PreFilter rejection, PreFilter node set, hard spread, required
                          anti-affinity — each beside plenty of reclaimable resources
  frozen behind           removal cures cpu and a frozen plugin behind NodeResourcesFit then fails (spread: missing label)
  empty tiers             the victims of the designed nodes sit in the first and the last tier below the limit: the tiers between are
                          empty on the node and stepped over
Each population also holds _reachgen's ladder (every level 0..T) and roomy nodes.

The victims carry the label app=res and every selector of an ask aims at app=web / app=blocker pods that are in no tier, so deleting
the victims from the snapshot leaves the oracle's topology PreFilter state as the engine froze it.

ExplainModel(snapshot, bounds) is ReachModel plus the final verdict, over Python ints."""
import _reachgen
from _preemptgen import DIMS, HOST, I64_MAX, P53, TAINT, _conflict, make_node, node_affinity
from _reachgen import BOUNDS, NEVER, ReachModel, asker, victim

UNRESOLVABLE, NO_VICTIMS, NOT_ENOUGH = "unresolvable", "no victims", "not enough"
TOO_MANY = "Too many pods"
NOT_ELIGIBLE, REJECTED, MISSING_LABEL = "node not eligible", "prefilter rejected", "missing required label"
BIG = {"cpu": 64000, "memory": 1 << 40}
T80 = ("10.0.0.1", "TCP", 80)
CELLS = 32


def keeper(uid, bounds, req=None, ports=None, labels=None):
    """A resident at or above the last bound: in no tier."""
    return victim(uid, bounds, len(bounds), req, ports, labels)


def designed(seed, T):
    pop = _reachgen._Population(seed, T)
    b, rng = pop.bounds, pop.rng
    verdicts = {}
    last = T - 1   # the last tier: with tier 0 the two ends of the walk, the tiers between stay empty on the designed nodes

    def pair(ask, node, level, rule, cls=None, code=None, reasons=()):
        pop.pair(ask, node, level, rule)
        uid = ask if isinstance(ask, str) else ask["metadata"]["uid"]
        if cls:
            verdicts[(uid, node)] = (cls, code, frozenset(reasons))

    # ---- two short resources: cpu cured, memory one short, beside 2^53
    mem_free = P53 - 10
    pods = [victim("ts-t0", b, 0, {"cpu": 60, "memory": 4}, rng=rng), victim("ts-tl", b, last, {"cpu": 40, "memory": 5}, rng=rng),
            keeper("ts-keep", b, {"cpu": 500})]
    pop.nodes.append(make_node("ts", {"cpu": 600, "memory": mem_free + 9}, pods))
    pair(asker("a-ts", b, T, {"cpu": 100, "memory": mem_free + 10}), "ts", NEVER, "two short resources", NOT_ENOUGH, 6, {"Insufficient memory"})
    pair(asker("a-ts-exact", b, T, {"cpu": 100, "memory": mem_free + 9}), "ts", T, "two short resources: exact")
    # ---- R = 8: every dimension one short once everybody eligible is gone; the scalars end at 2^63 - 1
    held = {d: rng.randrange(2, 9) for d in DIMS}
    kept = {d: rng.randrange(2, 9) for d in DIMS}
    alloc = {d: (I64_MAX if i >= 3 else P53 + 1 + i) for i, d in enumerate(DIMS)}
    pods = [victim("r8-t0", b, 0, {d: held[d] - 1 for d in DIMS}, rng=rng), victim("r8-tl", b, last, {d: 1 for d in DIMS}, rng=rng),
            keeper("r8-keep", b, kept)]
    pop.nodes.append(make_node("r8", alloc, pods))
    pair(asker("a-r8", b, T, {d: alloc[d] - kept[d] + 1 for d in DIMS}), "r8", NEVER, "R = 8, every dimension one short", NOT_ENOUGH, 6,
         {"Insufficient " + d for d in DIMS})
    pair(asker("a-r8-cpu", b, T, dict({d: alloc[d] - kept[d] for d in DIMS}, cpu=alloc["cpu"] - kept["cpu"] + 1)), "r8", NEVER,
         "R = 8, cpu alone one short", NOT_ENOUGH, 6, {"Insufficient cpu"})
    pair(asker("a-r8-fits", b, T, {d: alloc[d] - kept[d] for d in DIMS}), "r8", T, "R = 8, exact")
    # ---- ports into resources
    want = asker("a-pr", b, T, {"cpu": 50}, ports=[T80])
    pop.asks.append(want)
    pods = [victim("pr-t0", b, 0, {"cpu": 10}, ports=[T80], rng=rng), keeper("pr-keep", b, {"cpu": 90})]
    pop.nodes.append(make_node("pr", {"cpu": 100, "memory": 1 << 40}, pods))
    pair("a-pr", "pr", NEVER, "ports into resources", NOT_ENOUGH, 6, {"Insufficient cpu"})
    pods = [victim("pr-out-h", b, 0, {"cpu": 10}, ports=[T80], opt_out=True), victim("pr-out-t0", b, 0, {"cpu": 60}, rng=rng)]
    pop.nodes.append(make_node("pr-out", {"cpu": 70, "memory": 1 << 40}, pods))
    pair("a-pr", "pr-out", NEVER, "the port holder opted out", NOT_ENOUGH, 5)
    pods = [keeper("pr-kept-h", b, {"cpu": 10}, ports=[T80]), victim("pr-kept-tl", b, last, {"cpu": 60}, rng=rng)]
    pop.nodes.append(make_node("pr-kept", {"cpu": 70, "memory": 1 << 40}, pods))
    pair("a-pr", "pr-kept", NEVER, "the port holder is in no tier", NOT_ENOUGH, 5)
    pods = [victim("pr-hi-h", b, last, {"cpu": 60}, ports=[T80], rng=rng)]
    pop.nodes.append(make_node("pr-hi", {"cpu": 60, "memory": 1 << 40}, pods))
    pair("a-pr", "pr-hi", T, "the port holder is below the limit")
    low = asker("a-pr-low", b, T - 1, {"cpu": 50}, ports=[T80])
    pair(low, "pr-hi", NEVER, "the port holder is at the limit", NO_VICTIMS, 5)
    if T == 1:
        pair("a-pr-low", "pr", NEVER, "ports into resources, limit 0", NO_VICTIMS, 5)
    else:
        pair("a-pr-low", "pr", NEVER, "ports into resources, lower limit", NOT_ENOUGH, 6, {"Insufficient cpu"})
    # ---- slots stay full
    pods = [victim(f"sf-t0-{i}", b, 0, {}, rng=rng) for i in range(2)] + [victim("sf-tl", b, last, {}, rng=rng)] + [
        keeper(f"sf-keep-{i}", b, {"cpu": 1}) for i in range(3)]
    pop.nodes.append(make_node("sf", BIG, pods, allowed=3))
    pair(asker("a-sf", b, T, {"cpu": 1}), "sf", NEVER, "slots stay full", NOT_ENOUGH, 6, {TOO_MANY})
    pop.nodes.append(make_node("sf-cpu", {"cpu": 4, "memory": 1 << 40}, [victim("sfc-t0", b, 0, {"cpu": 1}, rng=rng)] + [
        keeper(f"sfc-keep-{i}", b, {"cpu": 1}) for i in range(3)], allowed=3))
    pair(asker("a-sf-both", b, T, {"cpu": 1}), "sf-cpu", NEVER, "slots stay full, cpu cured", NOT_ENOUGH, 6, {TOO_MANY})
    # ---- victims in the wrong tiers
    pods = [victim("wt-tl-a", b, last, {"cpu": 100}, rng=rng), victim("wt-tl-b", b, last, {"cpu": 100}, rng=rng)]
    pop.nodes.append(make_node("wt", {"cpu": 200, "memory": 1 << 40}, pods))
    pair(asker("a-wt-low", b, T - 1, {"cpu": 150}), "wt", NEVER, "victims in the wrong tiers", NO_VICTIMS, 6, {"Insufficient cpu"})
    pair(asker("a-wt-high", b, T, {"cpu": 150}), "wt", T, "sibling of a higher limit: a level")
    pair(asker("a-wt-more", b, T, {"cpu": 201}), "wt", NEVER, "sibling of a higher limit: not enough", NOT_ENOUGH, 6, {"Insufficient cpu"})
    pop.nodes.append(make_node("wt-bare", {"cpu": 10, "memory": 1 << 40}, []))
    pair("a-wt-high", "wt-bare", NEVER, "nobody on the node", NO_VICTIMS, 6, {"Insufficient cpu"})
    # ---- unresolvable beside plenty of reclaimable resources
    kinds = {"plain": {}, "tainted": {"taints": [TAINT]}, "cordoned": {"unschedulable": True}, "zoned": {"labels": {"zone": "a"}}}
    for kind, more in kinds.items():
        pods = [victim(f"un-{kind}-t0", b, 0, {"cpu": 100}, rng=rng), victim(f"un-{kind}-tl", b, last, {"cpu": 100}, rng=rng)]
        pop.nodes.append(make_node(f"un-{kind}", {"cpu": 200, "memory": 1 << 40}, pods, **more))
    web = [keeper(f"un-web{i}", b, {"cpu": 100}, labels={"app": "web"}) for i in range(3)]
    pop.nodes.append(make_node("un-far", BIG, web, labels={"zone": "za"}))
    pop.nodes.append(make_node("un-near", BIG, [victim("un-near-t0", b, 0, {"cpu": 100}, rng=rng)], labels={"zone": "zb"}))
    blocked = [keeper("un-blocker", b, {"cpu": 100}, labels={"app": "blocker"}), victim("un-crowded-t0", b, 0, {"cpu": 1000}, rng=rng)]
    pop.nodes.append(make_node("un-crowded", BIG, blocked, labels={"zone": "za"}))
    term = {"labelSelector": {"matchLabels": {"app": "blocker"}}, "topologyKey": HOST}
    anti = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [term]}}
    spread = [{"maxSkew": 2, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": {"app": "web"}}}]
    cases = [("unschedulable node", "un-cordoned", {}, 1, ()), ("untolerated taint", "un-tainted", {}, 3, ()),
             ("selector mismatch", "un-zoned", {"nodeSelector": {"zone": "b"}}, 4, ()),
             ("foreign nodeName", "un-plain", {"nodeName": "un-zoned"}, 2, ()),
             ("PreFilter: node outside the node-name set", "un-plain", {"affinity": node_affinity(["un-zoned"])}, 4, {NOT_ELIGIBLE}),
             ("PreFilter: no node can match", "un-plain", {"affinity": node_affinity(["un-zoned", "un-plain"])}, 0, {REJECTED}),
             ("anti-affinity against a pod in no tier", "un-crowded", {"affinity": anti}, 8, ()),
             ("zone skew exceeded by another node's pods", "un-crowded", {"topologySpreadConstraints": spread}, 7, ())]
    for c, (rule, node, bad, code, reasons) in enumerate(cases):
        pair(asker(f"a-un-{c}", b, T, {"cpu": 100}, **bad), node, NEVER, rule, UNRESOLVABLE, code, reasons)
    # ---- a frozen plugin behind NodeResourcesFit fails once cpu is cured: the node lacks the topology key
    pop.nodes.append(make_node("fb", {"cpu": 100, "memory": 1 << 40}, [victim("fb-t0", b, 0, {"cpu": 100}, rng=rng)]))
    pair(asker("a-fb", b, T, {"cpu": 100}, topologySpreadConstraints=spread), "fb", NEVER, "frozen behind: missing label", NOT_ENOUGH, 7,
         {MISSING_LABEL})
    snapshot, bounds, meta = pop.finish(roomy=30)
    meta["verdicts"] = verdicts
    return snapshot, bounds, meta


POPULATIONS = {"designed_1": 1, "designed_3": 3, "designed_8": 8}


def population(name, seed):
    return designed(seed, POPULATIONS[name])


def geometry(seed, n_nodes, n_asks=70, T=3):
    """_reachgen.geometry with host ports and slot pressure mixed in: 70 distinct tasks on n_nodes random nodes."""
    return _reachgen.geometry(seed, n_nodes, n_asks, T)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
class ExplainModel(ReachModel):
    def elig(self, node, limit):
        return self.victims_below(node, limit)

    def state(self, uid, node, L, plugins):
        """(NodePorts fails, the NodeResourcesFit reasons) of the ask on the node with every pod of tiers < L gone."""
        fit_on, ports_on = ("*" in plugins or "NodeResourcesFit" in plugins), ("*" in plugins or "NodePorts" in plugins)
        request, wanted, _ = self.asks[uid]
        alloc, allowed, pods = self.nodes[node]
        left = [p for p in pods if not 0 <= p[2] < L]
        used = {t for _, held, _ in pods for t in held} - {t for _, held, tier in pods if 0 <= tier < L for t in held}   # a SET
        reasons = set()
        if fit_on:
            if len(left) + 1 > allowed:
                reasons.add(TOO_MANY)
            for d, q in request.items():
                if q > 0 and q > alloc.get(d, 0) - sum(req.get(d, 0) for req, _, _ in left):
                    reasons.add("Insufficient " + d)
        return ports_on and any(_conflict(w, used) for w in wanted), reasons

    def first(self, uid, node, L, frozen, plugins):
        """(fits, code, reasons) at level L. frozen = (code, reasons) of the first failing plugin among those no removal moves, or None —
        taken from the oracle. Order: PreFilter (0, 4), 1, 2, 3, 4, NodePorts 5, NodeResourcesFit 6, 7, 8."""
        if frozen and frozen[0] < 5:
            return False, frozen[0], frozenset(frozen[1])
        ports, reasons = self.state(uid, node, L, plugins)
        if ports:
            return False, 5, frozenset()
        if reasons:
            return False, 6, frozenset(reasons)
        if frozen:
            return False, frozen[0], frozenset(frozen[1])
        return True, 0, frozenset()

    def verdict(self, uid, node, frozen, plugins=("*",)):
        """→ (level, (fits, code, reasons) of the state the verdict comes from, elig, class or None)."""
        limit = self.asks[uid][2]
        elig = self.elig(node, limit)
        stands = self.first(uid, node, 0, frozen, plugins)
        if stands[0]:
            return 0, stands, elig, None
        if stands[1] not in (5, 6):
            return NEVER, stands, elig, UNRESOLVABLE
        v = stands
        for L in range(1, limit + 1):
            v = self.first(uid, node, L, frozen, plugins)
            if v[0]:
                return L, v, elig, None
        return NEVER, v, elig, NO_VICTIMS if elig == 0 else NOT_ENOUGH


def reason_bits(reasons, dims=DIMS):
    """The reason word of ykpred_query for a set of reason texts: bits 0..3 the flags, bit 8 + r "insufficient resource r"."""
    word = 0
    for text in reasons:
        if text == TOO_MANY:
            word |= 1
        elif text == NOT_ELIGIBLE:
            word |= 2
        elif text == REJECTED:
            word |= 4
        elif text == MISSING_LABEL:
            word |= 8
        else:
            word |= 1 << (8 + dims.index(text[len("Insufficient "):]))
    return word


def node_word(level, v, elig, dims=DIMS):
    """The per-node word of ykpred_preempt_explain_pod."""
    fits, code, reasons = v
    r = reason_bits(reasons, dims)
    return (code & 0xff) | (0x100 if fits else 0) | ((r & 15) << 9) | ((r >> 8) << 13) | ((15 if level == NEVER else level) << 24) | ((1 << 28) if elig > 0 else 0)


def cells(verdicts, limit, dims=DIMS):
    """The 32 cells of one ask from its per-node (level, v, elig, class)."""
    out = [0] * CELLS
    for level, (fits, code, reasons), elig, cls in verdicts:
        if level == 0:
            out[9] += 1
        elif level != NEVER:
            out[11] += 1
        else:
            out[code] += 1
            out[{NO_VICTIMS: 24, UNRESOLVABLE: 25, NOT_ENOUGH: 26}[cls]] += 1
            if cls == NOT_ENOUGH:
                r = reason_bits(reasons, dims)
                for bit in range(4):
                    out[12 + bit] += (r >> bit) & 1
                for d in range(8):
                    out[16 + d] += (r >> (8 + d)) & 1
                out[27] += code == 5
                out[28] += elig
    out[29] = limit
    return out


__all__ = ["POPULATIONS", "population", "designed", "geometry", "ExplainModel", "cells", "node_word", "reason_bits", "NEVER", "BOUNDS",
           "UNRESOLVABLE", "NO_VICTIMS", "NOT_ENOUGH"]
