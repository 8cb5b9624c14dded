"""Designed clusters for preemption headroom (ykpred_preempt_headroom): how many copies of an ask every node takes once all pods of the
priority tiers below level L are gone, with a model over Python ints.

Pure Python, `random.Random(seed)` only; the pieces come from tests/_reachgen.py and tests/_preemptgen.py by import. Every population
records the copies it MEANT in meta["intended"][(ask uid, node name)] = [rep_0, ..., rep_limit]:

  quotient_edges   free + the requests of tiers < L equal to k x req, k x req - 1 and k x req + 1 for k in 1, 2, 7, one blocking dimension
                   at a time (R = 8), the designed level rotating through 1..T; amounts beside 2^53 and sums ending at 2^63 - 1
  slots_bind       tiers of zero-request pods: the slots freed by tiers < L below / on / above the resource quotient, so that the bound
                   switches between levels; an ask that requests nothing is bounded by the slots alone
  ports            the ask wants a host port whose holder sits in tier 1: 0, 0, 1, 1, while its sibling without the port gets the whole
                   quotient; two holders of one triple in different tiers (the triple leaves the SET with the first of them)
  flat_tiers       a tier that is empty on the node; a tier that frees less than one request (no rise, not charged in victims) followed
                   by one that does; an opted-out pod holding what would add copies
  limits           asks of every limit on one node (flat above the limit); preemptionPolicy: Never (every level equals headroom)
  shut             statically rejected pairs beside plenty to reclaim: 0 at every level, each next to a sibling that rises
  coupled          a hard-spread ask and a required anti-affinity ask (status 2) beside plain siblings
  one_tier, eight_tiers   the limit, slot and port scenes with T = 1 and T = 8

Each returns (snapshot, bounds, meta); every population also holds a LADDER (node lad-j takes the ladder ask's first copy at level j),
so that every level occurs. meta["set_pairs"] names the (ask, node, L) at which the model follows NodeInfo.RemovePod — a host-port
triple is gone once its FIRST holder is — where a snapshot with those residents deleted still shows the second holder.

GangModel(snapshot, bounds) sits on ReachModel.planes: rep(ask, node, L, frozen) restates rep_L, gone(node, L) the victim pods;
expected_cells(...) the 32 cells of one ask; wants_for(...) designs the wants so that every outcome of cell [30] occurs."""
import random

import _reachgen
from _preemptgen import DIMS, I64_MAX, P53, TAINT, TOLERATE_UNSCHEDULABLE, TOLERATION, HOST, _conflict, make_node, node_affinity
from _reachgen import BOUNDS, T80, ReachModel, asker, victim

CELLS = 32
COPIES, NODES, VICTIMS, STATUS, LIMIT, WANT, LEVEL = 0, 9, 18, 27, 28, 29, 30
MEM = 1 << 40


class _Population:
    def __init__(self, seed, T):
        self.rng = random.Random(seed)
        self.T, self.bounds = T, BOUNDS[T]
        self.nodes, self.asks, self.intended, self.set_pairs, self.coupled = [], [], {}, set(), set()

    def ask(self, ask):
        self.asks.append(ask)
        return ask["metadata"]["uid"]

    def pair(self, uid, node, reps):
        self.intended[(uid, node)] = list(reps)

    def ladder(self):
        """Node lad-j (j = 0..T) has 100m x (T - j) free and one 100m resident per tier; the ladder ask requests 100m x T: its copies
        there at level L are (T - j + L) // T — the first at level j, a second one on lad-0 at level T. lad-never has nobody to remove."""
        T, b = self.T, self.bounds
        for j in range(T + 1):
            pods = [victim(f"lad-{j}-t{t}", b, t, {"cpu": 100}, rng=self.rng) for t in range(T)]
            self.rng.shuffle(pods)
            self.nodes.append(make_node(f"lad-{j}", {"cpu": 100 * (T - j) + 100 * T, "memory": MEM}, pods))
        self.nodes.append(make_node("lad-never", {"cpu": 100 * T - 1, "memory": MEM}, []))
        for limit in sorted({T, T // 2, 0}):
            uid = self.ask(asker(f"a-lad-{limit}", b, limit, {"cpu": 100 * T}))
            for j in range(T + 1):
                self.pair(uid, f"lad-{j}", [(T - j + L) // T for L in range(limit + 1)])
            self.pair(uid, "lad-never", [0] * (limit + 1))

    def finish(self, roomy=2):
        """Adds the ladder and a few roomy nodes (five free slots, one tier-0 resident), shuffles the nodes, and arranges the asks so
        that neighbours differ in (copies per level, limit) as the model sees them with no frozen rejection."""
        self.ladder()
        for i in range(roomy):
            pods = [victim(f"room-{i}-r", self.bounds, 0, {"cpu": 10}, rng=self.rng)]
            self.nodes.append(make_node(f"room-{i}", {d: I64_MAX for d in DIMS}, pods, labels={"zone": "zb"}, allowed=6))
        self.rng.shuffle(self.nodes)
        self.rng.shuffle(self.asks)
        model = GangModel({"nodes": self.nodes, "pods": self.asks}, self.bounds)
        groups = {}
        for ask in self.asks:
            uid = ask["metadata"]["uid"]
            limit = model.asks[uid][2]
            key = (tuple(sum(model.rep(uid, n, L, True) for n in model.names) for L in range(limit + 1)), limit)
            groups.setdefault(key, []).append(ask)
        arranged, last = [], None
        while groups:
            key = max((k for k in groups if k != last), key=lambda k: len(groups[k]), default=last)
            arranged.append(groups[key].pop())
            if not groups[key]:
                del groups[key]
            last = key
        meta = dict(intended=self.intended, T=self.T, set_pairs=self.set_pairs, coupled=self.coupled)
        return {"nodes": self.nodes, "pods": arranged}, list(self.bounds), meta


# ---- (1) quotient edges ------------------------------------------------------------------------------------------------------------------
def quotient_edges(seed, T=3):
    """Node qe-<j>-<k>-<delta>: one resident per tier requesting 2..9 of the blocking dimension j, whose free amount is chosen so that
    free + the requests of tiers < L == k x req + delta at the designed level L = 1 + (j + k) % T. The request has the magnitude
    MAGS[j % 4]: small, k x req beside 2^53 from below and from above, or k x req + what the tiers at and above L hold ending one below
    2^63 - 1. One ask per (j, k) requests that dimension alone, so its copies on the three nodes are the quotient of that dimension:
    k - 1, k, k at level L."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    for j, d in enumerate(DIMS):
        for k in (1, 2, 7):
            L = 1 + (j + k) % T
            mag = ("small", "across", "above", "ends")[j % 4]
            req = {"small": rng.randrange(20, 30), "across": P53 // k, "above": (P53 + 1) // k + 1, "ends": (I64_MAX - 2 - 9 * T) // k}[mag]
            uid = pop.ask(asker(f"a-qe-{j}-{k}", b, T, {d: req}))
            for delta in (-1, 0, 1):
                name = f"qe-{j}-{k}-{delta + 1}"
                sizes = [rng.randrange(2, 10) for _ in range(T)]
                free = k * req + delta - sum(sizes[:L])
                pods = [victim(f"{name}-t{t}", b, t, {d: sizes[t]}, rng=rng) for t in range(T)]
                rng.shuffle(pods)
                alloc = {"cpu": 25, "memory": MEM}
                alloc[d] = free + sum(sizes)
                assert 0 <= free and alloc[d] <= I64_MAX
                pop.nodes.append(make_node(name, alloc, pods, allowed=T + 9))
                pop.pair(uid, name, [(free + sum(sizes[:l])) // req for l in range(T + 1)])
    return pop.finish()


# ---- (2) pod slots against the quotient ----------------------------------------------------------------------------------------------------
def slots_bind(seed, T=3):
    """Node sb-<q>-<s>: cpu for exactly q copies of the 100m ask, s free slots, and tier t holds c_t zero-request pods: the slots at
    level L are s + c_0 + ... + c_{L-1} — below q, on q and above q along the levels. a-sb-zero requests nothing: the slots alone."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    cpu = pop.ask(asker("a-sb-cpu", b, T, {"cpu": 100}))
    zero = pop.ask(asker("a-sb-zero", b, T, {}))
    half = pop.ask(asker("a-sb-half", b, max(T // 2, 1), {"cpu": 100}))
    for q in (3, 5, 6):
        for s in (0, 1, 4):
            name = f"sb-{q}-{s}"
            counts = [rng.randrange(1, 4) for _ in range(T)]
            pods = [victim(f"{name}-t{t}-{i}", b, t, {}, rng=rng) for t in range(T) for i in range(counts[t])]
            rng.shuffle(pods)
            pods.append(victim(f"{name}-keep", b, T, {"cpu": 10}))
            pop.nodes.append(make_node(name, {"cpu": 100 * q + 10 + 50, "memory": MEM}, pods, allowed=len(pods) + s))
            slots = [s + sum(counts[:L]) for L in range(T + 1)]
            pop.pair(cpu, name, [min(x, q) for x in slots])
            pop.pair(zero, name, slots)
            pop.pair(half, name, [min(x, q) for x in slots[:max(T // 2, 1) + 1]])
    return pop.finish()


# ---- (3) host ports ------------------------------------------------------------------------------------------------------------------------
def ports(seed, T=3):
    """Nodes with 250m free and one 100m resident per tier — the sibling without the port gets 2, 3, 4, ... copies. po-one-<t>: the holder
    of the wanted triple sits in tier t: 0 up to level t, then ONE copy (a pod conflicts with its own host port). po-two-<t>-<u>: two
    holders of the IDENTICAL triple: the triple goes with the first. po-kept: the holder is in no tier."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    other = lambda i: [("10.0.0.1", "TCP", 3000 + i)]   # noqa: E731
    want = pop.ask(asker("a-port", b, T, {"cpu": 100}, ports=[T80]))
    half = pop.ask(asker("a-port-half", b, max(T - 1, 1), {"cpu": 100}, ports=[("0.0.0.0", None, 80)]))
    plain = pop.ask(asker("a-port-none", b, T, {"cpu": 100}))
    free = pop.ask(asker("a-port-free", b, T, {"cpu": 100}, ports=[("10.0.0.1", "TCP", 81)]))

    def scene(name, holders):
        pods = [victim(f"{name}-t{t}", b, t, {"cpu": 100}, ports=holders.get(t, other(t)), rng=rng) for t in range(T + 1)]
        rng.shuffle(pods)
        pop.nodes.append(make_node(name, {"cpu": 250 + 100 * (T + 1), "memory": MEM}, pods))
        tiered = sorted(t for t in holders if t < T)   # (a holder in no tier never leaves)
        open_at = 0 if not holders else tiered[0] + 1 if len(tiered) == len(holders) else T + 1
        pop.pair(want, name, [1 if L >= open_at else 0 for L in range(T + 1)])
        pop.pair(half, name, [1 if L >= open_at else 0 for L in range(max(T - 1, 1) + 1)])
        pop.pair(plain, name, [2 + L for L in range(T + 1)])
        pop.pair(free, name, [1] * (T + 1))
        if len(tiered) > 1:   # between the first holder and the last one, a snapshot with the residents deleted still holds the triple
            for L in range(tiered[0] + 1, tiered[-1] + 1):
                for uid in (want, half):
                    pop.set_pairs.add((uid, name, L))

    for t in range(T):
        scene(f"po-one-{t}", {t: [T80]})
    if T >= 2:
        scene(f"po-two-0-{T - 1}", {0: [T80], T - 1: [T80]})
    scene("po-kept", {T: [T80]})
    scene("po-none", {})
    return pop.finish()


# ---- (4) flat tiers ------------------------------------------------------------------------------------------------------------------------
def flat_tiers(seed, T=3):
    """ft-short: 100m free, tier 0 frees 50m (no copy of the 100m ask: not charged), tier 1 frees 100m (a copy: both tiers are charged),
    tier 2 is empty. ft-late: nothing free, tier 0 empty, two 30m pods in tier 1 (nothing), one 40m pod in tier 2 (a copy, three pods).
    ft-out: 100m free, an opted-out 100m pod of tier-0 priority, a 100m pod in tier 1."""
    pop = _Population(seed, T)
    b = pop.bounds
    assert T >= 3
    pop.nodes.append(make_node("ft-short", {"cpu": 250, "memory": MEM}, [victim("ft-short-t0", b, 0, {"cpu": 50}), victim("ft-short-t1", b, 1, {"cpu": 100})]))
    pop.nodes.append(make_node("ft-late", {"cpu": 100, "memory": MEM}, [victim("ft-late-t1a", b, 1, {"cpu": 30}), victim("ft-late-t1b", b, 1, {"cpu": 30}),
                                                                       victim("ft-late-t2", b, 2, {"cpu": 40})]))
    pop.nodes.append(make_node("ft-out", {"cpu": 300, "memory": MEM}, [victim("ft-out-t0", b, 0, {"cpu": 100}, opt_out=True), victim("ft-out-t1", b, 1, {"cpu": 100})]))
    flat = [0] * (T - 3)   # (tiers above 2 hold nobody)
    for uid, limit, rows in (("a-ft-100", T, {"ft-short": [1, 1, 2, 2], "ft-late": [0, 0, 0, 1], "ft-out": [1, 1, 2, 2]}),
                             ("a-ft-50", T, {"ft-short": [2, 3, 5, 5], "ft-late": [0, 0, 1, 2], "ft-out": [2, 2, 4, 4]}),
                             ("a-ft-100-1", 1, {"ft-short": [1, 1], "ft-late": [0, 0], "ft-out": [1, 1]}),
                             ("a-ft-50-2", 2, {"ft-short": [2, 3, 5], "ft-late": [0, 0, 1], "ft-out": [2, 2, 4]})):
        pop.ask(asker(uid, b, limit, {"cpu": int(uid.split("-")[2])}))
        for node, reps in rows.items():
            pop.pair(uid, node, reps + [reps[-1] for _ in flat] if limit == T else reps)
    return pop.finish()


# ---- (5) limits ----------------------------------------------------------------------------------------------------------------------------
def limits(seed, T=3):
    """li: nothing free, one 100m resident per tier: the 100m ask of limit l takes L copies at level L <= l and stays there above;
    li-free takes T copies at every level. preemptionPolicy: Never is limit 0 whatever the priority."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    pods = [victim(f"li-t{t}", b, t, {"cpu": 100}, rng=rng) for t in range(T)]
    rng.shuffle(pods)
    pop.nodes.append(make_node("li", {"cpu": 100 * T, "memory": MEM}, pods))
    pop.nodes.append(make_node("li-free", {"cpu": 100 * T, "memory": MEM}, []))
    for cpu in (100, 50):
        for limit in range(T + 1):
            uid = pop.ask(asker(f"a-li-{cpu}-{limit}", b, limit, {"cpu": cpu}))
            pop.pair(uid, "li", [100 * L // cpu for L in range(limit + 1)])
            pop.pair(uid, "li-free", [100 * T // cpu] * (limit + 1))
        uid = pop.ask(asker(f"a-li-{cpu}-policy", b, T, {"cpu": cpu}, never=True))
        pop.pair(uid, "li", [0])
        pop.pair(uid, "li-free", [100 * T // cpu])
    return pop.finish()


# ---- (6) what no removal opens -------------------------------------------------------------------------------------------------------------
def shut(seed, T=3):
    """Every node: nothing free, one 100m resident per tier. The shut ask differs from its sibling in ONE attribute that no removal
    changes: 0 at every level beside 100m x L // request copies for the sibling."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    kinds = {"plain": {}, "tainted": {"taints": [TAINT]}, "cordoned": {"unschedulable": True}, "zoned": {"labels": {"zone": "a"}}}
    for kind, more in kinds.items():
        pods = [victim(f"sh-{kind}-t{t}", b, t, {"cpu": 100}, rng=rng) for t in range(T)]
        pop.nodes.append(make_node(f"sh-{kind}", {"cpu": 100 * T, "memory": MEM}, pods, **more))
    cases = [("sh-cordoned", {}, {"tolerations": [TOLERATE_UNSCHEDULABLE]}),
             ("sh-tainted", {}, {"tolerations": [TOLERATION]}),
             ("sh-zoned", {"nodeSelector": {"zone": "b"}}, {"nodeSelector": {"zone": "a"}}),
             ("sh-plain", {"nodeName": "sh-zoned"}, {"nodeName": "sh-plain"}),
             ("sh-plain", {"affinity": node_affinity(["sh-zoned"])}, {"affinity": node_affinity(["sh-plain"])})]
    for c, (node, bad, good) in enumerate(cases):
        cpu = 100 // (c + 1)   # (a request of its own per case: the siblings' cells differ)
        uid = pop.ask(asker(f"a-shut-{c}", b, T, {"cpu": cpu}, **bad))
        pop.pair(uid, node, [0] * (T + 1))
        uid = pop.ask(asker(f"a-open-{c}", b, T, {"cpu": cpu}, **good))
        pop.pair(uid, node, [100 * L // cpu for L in range(T + 1)])
    return pop.finish()


# ---- (7) coupled asks ----------------------------------------------------------------------------------------------------------------------
def coupled(seed, T=3):
    """A hard-spread ask and a required anti-affinity ask: their copies change each other's verdicts, status 2. Their plain siblings
    are computed. The nodes carry zones and app=web / app=victim pods so that the frozen verdicts differ between nodes."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    for z, zone in enumerate(("za", "za", "zb")):
        labels = {"app": "victim"} if z == 0 else {"app": "web"}
        pods = [victim(f"co-{z}-t{t}", b, t, {"cpu": 100}, labels=labels, rng=rng) for t in range(T)]
        pop.nodes.append(make_node(f"co-{z}", {"cpu": 100 * T + 50 * z, "memory": MEM}, pods, labels={"zone": zone}))
    term = {"labelSelector": {"matchLabels": {"app": "victim"}}, "topologyKey": HOST}
    anti = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [term]}}
    spread = [{"maxSkew": 3, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": {"app": "web"}}}]
    for cpu in (100, 50):
        pop.coupled.add(pop.ask(asker(f"a-co-anti-{cpu}", b, T, {"cpu": cpu}, affinity=anti)))
        pop.coupled.add(pop.ask(asker(f"a-co-spread-{cpu}", b, T - 1, {"cpu": cpu}, topologySpreadConstraints=spread)))
        uid = pop.ask(asker(f"a-co-plain-{cpu}", b, T, {"cpu": cpu}))
        for z in range(3):
            pop.pair(uid, f"co-{z}", [(50 * z + 100 * L) // cpu for L in range(T + 1)])
    return pop.finish()


# ---- (8) other tier counts -----------------------------------------------------------------------------------------------------------------
def tier_mix(seed, T):
    """The limit scene, a slot scene and a port scene with T tiers (T = 1 and T = 8)."""
    pop = _Population(seed, T)
    rng, b = pop.rng, pop.bounds
    pods = [victim(f"tm-li-t{t}", b, t, {"cpu": 100}, rng=rng) for t in range(T)]
    pop.nodes.append(make_node("tm-li", {"cpu": 100 * T + 30, "memory": MEM}, pods))
    pods = [victim(f"tm-sl-t{t}", b, t, {}, rng=rng) for t in range(T)] + [victim("tm-sl-keep", b, T, {"cpu": 10})]
    pop.nodes.append(make_node("tm-sl", {"cpu": 310, "memory": MEM}, pods, allowed=len(pods) + 1))
    holder = T // 2
    pods = [victim(f"tm-po-t{t}", b, t, {"cpu": 100}, ports=[T80] if t == holder else None, rng=rng) for t in range(T)]
    pop.nodes.append(make_node("tm-po", {"cpu": 100 * T + 100, "memory": MEM}, pods))
    for limit in sorted({T, T // 2, 0, 1}):
        for cpu in (100, 30):
            uid = pop.ask(asker(f"a-tm-{cpu}-{limit}", b, limit, {"cpu": cpu}))
            pop.pair(uid, "tm-li", [(30 + 100 * L) // cpu for L in range(limit + 1)])
            pop.pair(uid, "tm-sl", [min(1 + L, 300 // cpu) for L in range(limit + 1)])
            pop.pair(uid, "tm-po", [(100 + 100 * L) // cpu for L in range(limit + 1)])
    uid = pop.ask(asker("a-tm-port", b, T, {"cpu": 100}, ports=[T80]))
    pop.pair(uid, "tm-po", [1 if L > holder else 0 for L in range(T + 1)])
    pop.pair(uid, "tm-li", [1 if L >= 1 else 0 for L in range(T + 1)])
    return pop.finish()


POPULATIONS = {"quotient_edges": (quotient_edges, 3), "slots_bind": (slots_bind, 3), "ports": (ports, 3), "flat_tiers": (flat_tiers, 3),
               "limits": (limits, 3), "shut": (shut, 3), "coupled": (coupled, 3), "one_tier": (tier_mix, 1), "eight_tiers": (tier_mix, 8)}


def population(name, seed):
    fn, T = POPULATIONS[name]
    return fn(seed, T)


def geometry(seed, n_nodes, n_asks=70, T=3):
    """The shape of a launch, as _reachgen.geometry: n_nodes nodes off the wave width and across the 256-node block with random free cpu,
    random tiers and few pod slots, and n_asks DISTINCT (request, limit) tasks — three chunks of 32 at 70. The model decides."""
    snapshot, bounds, meta = _reachgen.geometry(seed, n_nodes, n_asks, T)
    return snapshot, bounds, dict(meta, intended={}, set_pairs=set(), coupled=set())


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
class GangModel(ReachModel):
    """rep_L over Python ints, from the reclaim planes of ReachModel.planes: the node's free amounts grow by the planes' request sums of
    tiers < L, its pod count drops by their pod counts, its used ports are the planes' set after tier L - 1."""

    def __init__(self, snapshot, bounds):
        super().__init__(snapshot, bounds)
        self.names = [n["metadata"]["name"] for n in snapshot["nodes"]]
        self.at = {name: i for i, name in enumerate(self.names)}
        self.dims = sorted({d for alloc, _, _ in self.nodes.values() for d in alloc} | {d for req, _, _ in self.asks.values() for d in req})
        self.req, self.cnt, self.used_after = self.planes(self.names, self.dims)

    def gone(self, node, L):
        return sum(self.cnt[t][self.at[node]] for t in range(L))

    def rep(self, uid, node, L, frozen, plugins=("*",)):
        """frozen: the verdict of every plugin but NodeResourcesFit and NodePorts on the pair (PreFilter rejections included).
        L above the ask's limit counts as the limit."""
        ports_on = "*" in plugins or "NodePorts" in plugins
        request, wanted, limit = self.asks[uid]
        alloc, allowed, pods = self.nodes[node]
        L, n = min(L, limit), self.at[node]
        if not frozen:
            return 0
        slots = allowed - len(pods) + self.gone(node, L)
        k = slots
        for d, q in request.items():
            if q > 0:
                free = alloc.get(d, 0) - sum(p[0].get(d, 0) for p in pods) + sum(self.req[t][self.dims.index(d)][n] for t in range(L))
                k = min(k, free // q if free >= 0 else 0)
        if k < 1:
            return 0
        if ports_on and wanted:
            used = self.used_after[L - 1][n] if L >= 1 else {x for _, held, _ in pods for x in held}
            if any(_conflict(w, used) for w in wanted):
                return 0
            k = 1
        return k

    def rows(self, uid, frozen_row, plugins=("*",)):
        """[limit + 1][N] copies of one ask; frozen_row[n] as for rep."""
        limit = self.asks[uid][2]
        return [[self.rep(uid, node, L, bool(frozen_row[n]), plugins) for n, node in enumerate(self.names)] for L in range(limit + 1)]


def expected_cells(rows, gone, limit, want, status=0, fit_rows=None):
    """The 32 cells of one ask. rows[L][n] = rep_L for L = 0..limit; gone[L][n] = the pods of node n in tiers < L. status 2 (coupled):
    fit_rows[L][n] = whether one copy fits at level L (rows is ignored); status 1: routed."""
    out = [0] * CELLS
    out[STATUS], out[LIMIT], out[WANT] = status, limit, want
    if status == 1:
        return out
    out[LEVEL] = -1
    for L in range(9):
        m = min(L, limit)
        if status == 2:
            out[COPIES + L] = out[VICTIMS + L] = -1
            out[NODES + L] = sum(1 for x in fit_rows[m] if x)
            continue
        out[COPIES + L] = sum(rows[m])
        out[NODES + L] = sum(1 for x in rows[m] if x >= 1)
        for n, x in enumerate(rows[m]):
            first = next(l for l in range(m + 1) if rows[l][n] == x)   # the fewest whole tiers that give the node its level-L copies
            out[VICTIMS + L] += gone[first][n]
    if status == 0:
        out[LEVEL] = next((L for L in range(limit + 1) if out[COPIES + L] >= want), -1)
    return out


def wants_for(copies, limits):
    """One want per ask from its copies per level (copies[i][L], L = 0..limit): ask i aims at level (i mod (limit + 2)) - 1 — the want
    is that level's copies when the level adds some (cell [30] is then that level), and one more than the limit's copies otherwise or
    when it aims at -1 (cell [30] is -1). Always >= 1."""
    out = []
    for i, (row, limit) in enumerate(zip(copies, limits)):
        aim = i % (limit + 2) - 1
        if aim >= 0 and row[aim] >= 1 and (aim == 0 or row[aim] > row[aim - 1]):
            out.append(row[aim])
        else:
            out.append(max(row[limit], 0) + 1)
    return out


__all__ = ["CELLS", "POPULATIONS", "population", "geometry", "GangModel", "expected_cells", "wants_for"]
