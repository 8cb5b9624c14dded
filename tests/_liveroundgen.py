"""Designed rounds for the preemption round with LIVE topology histograms (ykpred_preempt_round_live), and a model over Python ints.

Rounds of at most 40 turns on 70 and 130 nodes, T = 1 and 3 tiers. Three zones (label "zone"); the hostname key gives one domain per
node, i.e. more than 64 domains. Every node that is not part of a scene is a FILLER: full, its one resident in no tier, labelled with a
zone in turn — it counts for the histograms and takes nothing. Each turn is listed with what it is meant to do (meta["intended"]: the
outcome, node, from and extra, or None where the round states a count instead):

  victim_min      a victim that matches a spread selector is claimed by an uncoupled ask: its zone's count and the global minimum
                  drop, so the next spread ask gets into that (full) zone by a victim while the free nodes of the crowded zones are
                  never; the last domain at the minimum leaves it (at_min 1 -> 0) and the minimum rises; an unsupported ask mid-list;
                  chosen nodes at indices 63, 64 and N - 1
  zone_gang_*     a zone-spread gang (maxSkew 1) of copies - 1, copies and copies + 2, most copies by two victims
  host_gang_*     a "one per host" self anti-affinity gang of the same three sizes; one host holds a matching pod that an uncoupled ask
                  claims first: the host opens for the gang, not for the claimer's own turn
  affinity        a victim that was the only match of a later ask's anti-affinity term in its zone; a victim CARRYING a required
                  anti-affinity term against a later ask's labels; the only match of a required-affinity term claimed (the later ask
                  goes nowhere, a self-matching one bootstraps: the count of domains with a match fell to zero); the bootstrap — first copy by self-match, second bound to its domain, third nowhere beside a free node
  policy          a placement on a node that does not count for a constraint (nodeAffinityPolicy Honor: the zone of the pool is all the
                  template sees — zone c is absent for it); minDomains above the present domains; a spec that adds to 12 constraints;
                  uncoupled asks whose labels match a later ask's selector

LiveModel is _preemptroundgen.RoundModel (resources, slots, ports, the taken prefixes) with the verdicts of NodeName, NodeAffinity,
PodTopologySpread and InterPodAffinity computed from the pods as they stand at the START of the turn: the residents minus the claimed
victims plus the pods the round placed. live=False freezes them at the start of the round — what a round without the feature sees."""
import copy
import json
import random

from _preemptgen import HOST, make_node, resident
from _preemptroundgen import MAX_ASKS, PVC, RoundModel
from _reachgen import BOUNDS, asker, tier_priority

ZONE = "zone"
ZONES = ("z-a", "z-b", "z-c")
MEM = {"memory": 1 << 30}


def spread(app, key=ZONE, skew=1, **more):
    return dict({"maxSkew": skew, "topologyKey": key, "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": app if isinstance(app, dict) else {"app": app}}}, **more)


def term(app, key=ZONE):
    return {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": key}


def affinity(aff=(), anti=()):
    out = {}
    if aff:
        out["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": list(aff)}
    if anti:
        out["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": list(anti)}
    return out


class _Round:
    def __init__(self, seed, T, N):
        self.rng = random.Random(seed)
        self.T, self.bounds, self.N = T, BOUNDS[T], N
        self.nodes, self.pool, self.turns, self.intended, self.at = [], {}, [], [], {}
        self.keep = self.bounds[-1]   # a priority in no tier

    def tier(self, t):
        return tier_priority(self.bounds, min(t, self.T - 1))

    def pod(self, uid, prio, cpu, app="res", anti=()):
        p = resident(uid, {"cpu": cpu} if cpu else {}, None, {"app": app})
        if prio != 0:
            p["spec"]["priority"] = prio
        if anti:
            p["spec"]["affinity"] = affinity(anti=anti)
        return p

    def node(self, name, zone, free, pods, index=None, **labels):
        used = sum(int(p["spec"]["containers"][0]["resources"]["requests"].get("cpu", "0m")[:-1]) for p in pods)
        labels = dict({"scene": name}, **labels)
        if zone is not None:
            labels[ZONE] = zone
        n = make_node(name, dict({"cpu": used + free}, **MEM), pods, labels=labels)
        if index is None:
            self.nodes.append(n)
        else:
            self.at[index] = n
        return name

    def ask(self, uid, limit, cpu, app="ask", selector=None, labels=None, **spec):
        if selector is not None:
            spec["nodeSelector"] = selector
        self.pool[uid] = asker(uid, self.bounds, min(limit, self.T), {"cpu": cpu}, None, **spec)
        self.pool[uid]["metadata"]["labels"] = dict(labels or {"app": app})
        return uid

    def copy_of(self, uid, new):
        """Another pod of the same template: the same spec row on the device."""
        self.pool[new] = copy.deepcopy(self.pool[uid])
        self.pool[new]["metadata"]["uid"] = self.pool[new]["metadata"]["name"] = new
        return new

    def turn(self, uid, *intent):
        """A uid that already took a turn comes back as ANOTHER pod of the same template (uid.2, uid.3 ...): the same spec row on the device,
        and a pod of its own for the host loop the round is compared with."""
        if uid in self.turns:
            uid = self.copy_of(uid, f"{uid}.{sum(1 for t in self.turns if t.split('.')[0] == uid) + 1}")
        self.turns.append(uid)
        self.intended.append(tuple(intent) if intent else None)

    def finish(self, **more):
        fill = self.N - len(self.nodes) - len(self.at)
        assert fill >= 0 and len(self.turns) <= MAX_ASKS, (fill, len(self.turns))
        fillers = [make_node(f"fill-{i}", {"cpu": 5, "memory": 1 << 20}, [self.pod(f"fill-{i}-r", self.keep, 5)], labels={ZONE: ZONES[i % 3]}, allowed=1)
                   for i in range(fill)]
        for f in fillers:
            f["pods"][0]["spec"]["containers"][0]["resources"]["requests"]["memory"] = str(1 << 20)
        free = [i for i in range(self.N) if i not in self.at]
        mine = set(self.rng.sample(free, len(self.nodes)))   # (the scene nodes keep their relative order: ties go by index)
        scene, nodes = iter(self.nodes), []
        for i in range(self.N):
            nodes.append(self.at[i] if i in self.at else next(scene) if i in mine else fillers.pop())
        snapshot = {"nodes": nodes, "pods": list(self.pool.values())}
        intended = [None if t is None else (t + (None,) * (2 - len(t)) + (0, 0))[:4] for t in self.intended]
        return snapshot, list(self.bounds), dict(turns=list(self.turns), intended=intended, T=self.T, **more)


# ---- (1) a claimed victim moves the minimum ----------------------------------------------------------------------------------------
def victim_min(seed, T=3, N=70):
    r = _Round(seed, T, N)
    lo, mid = r.tier(0), r.tier(1)
    r.node("vm-a0", "z-a", 400, [r.pod("vm-a0-web", lo, 600, "web")])
    r.node("vm-a1", "z-a", 0, [r.pod("vm-a1-v", lo, 500), r.pod("vm-a1-k", r.keep, 500)], index=63)
    r.node("vm-a2", "z-a", 0, [r.pod("vm-a2-v", mid, 300), r.pod("vm-a2-k", r.keep, 700)])
    r.node("vm-b", "z-b", 900, [r.pod("vm-b-web", r.keep, 100, "web")], index=64)
    r.node("vm-c", "z-c", 900, [r.pod("vm-c-web", r.keep, 100, "web")], index=N - 1)
    r.ask("claim", 2, 900, "batch", selector={"scene": "vm-a0"})
    web = r.ask("web-1", 2, 300, "web", topologySpreadConstraints=[spread("web")])
    r.ask("routed", 2, 100, "batch", volumes=PVC)
    r.turn("claim", 1, "vm-a0", 0, 1)             # web: a 1 -> 0, the minimum 1 -> 0, one domain at the minimum
    r.turn(web, 1, "vm-a1", 0, 1)                 # zone a is full: in by a victim; vm-b and vm-c are free and never. a = 1, three at the minimum
    r.turn("routed", 3)
    r.turn(r.copy_of(web, "web-2"), 0, "vm-b")    # b = 2
    r.turn(r.copy_of(web, "web-3"), 0, "vm-c")    # b is over the skew, a has no room at level 0; c = 2: ONE domain left at the minimum
    r.turn(r.copy_of(web, "web-4"), 1, "vm-a2", 0, 1)   # only zone a: by the tier-1 victim; a = 2: the last domain at the minimum leaves it, the minimum is 2
    r.turn(r.copy_of(web, "web-5"), 0, "vm-b")    # (a minimum that stayed 1 would send it nowhere)
    r.turn(r.copy_of(web, "web-6"), 0, "vm-c")
    r.turn(r.copy_of(web, "web-7"), 2)            # a = 2 without room, b = c = 3
    return r.finish()


# ---- (2) a zone-spread gang ---------------------------------------------------------------------------------------------------------
def zone_gang(seed, T=3, N=70, beyond=0):
    """Zones a and b: four nodes each, zone c: three; one copy per node, the first node of a zone free, the others by two victims.
    maxSkew 1 and three nodes in zone c: copies == 3 + 4 + 4."""
    r = _Round(seed, T, N)
    lo = r.tier(0)
    for z, count in (("z-a", 4), ("z-b", 4), ("z-c", 3)):
        for i in range(count):
            name = f"zg-{z[-1]}{i}"
            pods = [] if i == 0 else [r.pod(f"{name}-v{j}", lo, 200) for j in range(2)] + [r.pod(f"{name}-k", r.keep, 100)]
            r.node(name, z, 450 if i == 0 else 0, pods, pool="zg")
    r.ask("gang", T, 400, "zg", selector={"pool": "zg"}, topologySpreadConstraints=[spread("zg", nodeAffinityPolicy="Ignore")])
    copies = 11
    for i in range(copies + beyond):
        r.turn("gang")
    return r.finish(copies=copies, gang="gang")


# ---- (3) one per host -----------------------------------------------------------------------------------------------------------------
def host_gang(seed, T=3, N=130, beyond=0):
    """Eight hosts — the even ones with room for two copies by resources, the odd ones full with one victim — and the rule allows one each. hg-x holds a matching pod in tier 0: `opener` claims it
    first, and the host takes a copy of the gang. copies == 9."""
    r = _Round(seed, T, N)
    lo = r.tier(0)
    at = {0: 63, 1: 64, 2: N - 1}
    for i in range(8):
        pods = [r.pod(f"hg-{i}-v", lo, 100)] if i % 2 else []
        r.node(f"hg-{i}", ZONES[i % 3], 0 if i % 2 else 250, pods, index=at.get(i), pool="hg")
    r.node("hg-x", "z-a", 0, [r.pod("hg-x-old", lo, 300, "hg")], pool="hg", own="x")
    r.ask("opener", T, 150, "batch", selector={"own": "x"})
    r.ask("gang", T, 100, "hg", selector={"pool": "hg"}, affinity=affinity(anti=[term("hg", HOST)]))
    r.turn("opener", 1, "hg-x", 0, 1)
    copies = 9
    for i in range(copies + beyond):
        r.turn("gang")
    return r.finish(copies=copies, gang="gang")


# ---- (4) victims and the affinity terms -------------------------------------------------------------------------------------------------
def affinity_round(seed, T=3, N=130):
    r = _Round(seed, T, N)
    lo = r.tier(0)
    # the only db pod of zone c is a victim; zone a keeps its db pod
    r.node("af-a", "z-a", 500, [r.pod("af-a-db", r.keep, 100, "db")], pool="af")
    r.node("af-c", "z-c", 0, [r.pod("af-c-db", lo, 400, "db")], pool="af", own="af-c")
    r.ask("af-claim", T, 300, "batch", selector={"own": "af-c"})
    r.ask("nodb", T, 100, "nodb", selector={"pool": "af"}, affinity=affinity(anti=[term("db")]))
    r.turn("nodb", 2)                                 # both zones of its pool hold a db pod
    r.turn("af-claim", 1, "af-c", 0, 1)
    r.turn(r.copy_of("nodb", "nodb-2"), 0, "af-c", 1)   # zone c has opened; 100 of the 400 are left
    # a victim that carries an anti-affinity term against app=shy
    r.node("ax-1", "z-b", 0, [r.pod("ax-1-hater", lo, 400, "hater", anti=[term("shy")])], pool="ax", own="ax-1")
    r.node("ax-2", "z-b", 500, [], pool="ax")
    r.ask("ax-claim", T, 100, "batch", selector={"own": "ax-1"})
    r.ask("shy", T, 100, "shy", selector={"pool": "ax"})
    r.turn("shy", 2)                                  # the whole zone is shut by the existing pod's term
    r.turn("ax-claim", 1, "ax-1", 0, 1)
    r.turn(r.copy_of("shy", "shy-2"), 0, "ax-1", 1)    # both nodes are open now: the lower index
    # the only match of a required-affinity term
    r.node("rq", "z-a", 200, [r.pod("rq-drv", lo, 300, "drv")], pool="rq")
    r.ask("wrk", T, 100, "wrk", selector={"pool": "rq"}, affinity=affinity(aff=[term("drv", HOST)]))
    r.ask("rq-claim", T, 350, "batch", selector={"pool": "rq"})
    r.turn("wrk", 0, "rq")
    r.turn("rq-claim", 1, "rq", 0, 1)                 # 100 free: the driver goes
    r.turn(r.copy_of("wrk", "wrk-2"), 2)              # no driver anywhere, and a worker does not match its own term
    r.ask("drv-2", T, 50, "drv", selector={"pool": "rq"}, affinity=affinity(aff=[term("drv", HOST)]))
    r.turn("drv-2", 0, "rq", 1)                       # ... while a second driver matches its own: no domain holds a match any more, the bootstrap
    # the bootstrap
    r.node("bt-a", "z-a", 100, [], pool="bt")
    r.node("bt-b", "z-b", 300, [], pool="bt")
    r.node("bt-a2", "z-a", 100, [], pool="bt")
    r.ask("boot", T, 100, "boot", selector={"pool": "bt"}, affinity=affinity(aff=[term("boot")]))
    r.turn("boot", 0, "bt-a")                         # no match anywhere and it matches itself
    r.turn("boot", 0, "bt-a2")                        # bound to zone a; bt-a is full
    r.turn("boot", 2)                                 # zone a is full, bt-b is free and never
    return r.finish()


# ---- (5) inclusion policies, minDomains, twelve constraints -----------------------------------------------------------------------------
def policy(seed, T=1, N=70):
    r = _Round(seed, T, N)
    # the pool has nodes in zones a and b only: zone c is absent for the template (Honor); `out` is in zone a and outside the pool
    r.node("p-a", "z-a", 300, [], pool="p1")
    r.node("p-b", "z-b", 300, [], pool="p1")
    r.node("out", "z-a", 300, [], own="out")
    r.ask("stray", T, 100, "pol", selector={"own": "out"})   # uncoupled, and its labels match pol's selector
    r.ask("pol", T, 100, "pol", selector={"pool": "p1"}, topologySpreadConstraints=[spread("pol", minDomains=3)])
    r.turn("stray", 0, "out")       # `out` does not count for pol's constraint: no cell moves
    r.turn("pol", 0, "p-a")         # (a counted stray would send it to p-b)
    r.turn("pol", 0, "p-b")
    r.turn("pol", 2)                # two domains under minDomains 3: the minimum counts as 0
    # a spec whose pods add to twelve constraints: six selectors, each spread over the zone and the host
    keys = {f"k{i}": "v" for i in range(6)}
    r.node("tw-1", "z-a", 1000, [], pool="tw")
    r.node("tw-2", "z-b", 1000, [], pool="tw")
    r.ask("multi", T, 100, labels=dict({"app": "multi"}, **keys), selector={"scene": "tw-1"})
    r.turn("multi", 0, "tw-1")
    r.turn("multi", 0, "tw-1")
    for i in range(6):
        uid = r.ask(f"s{i}", T, 50, f"s{i}", selector={"pool": "tw"},
                    topologySpreadConstraints=[spread({f"k{i}": "v"}, ZONE), spread({f"k{i}": "v"}, HOST)])
        r.turn(uid, 0, "tw-2")      # two matches on tw-1 and none on tw-2: over the skew there
    return r.finish()


ROUNDS = {"victim_min": lambda s: victim_min(s, 3, 70), "victim_min_130": lambda s: victim_min(s, 3, 130),
          "zone_gang_m1": lambda s: zone_gang(s, 3, 70, -1), "zone_gang_eq": lambda s: zone_gang(s, 1, 130, 0), "zone_gang_p2": lambda s: zone_gang(s, 3, 70, 2),
          "host_gang_m1": lambda s: host_gang(s, 1, 130, -1), "host_gang_eq": lambda s: host_gang(s, 3, 130, 0), "host_gang_p2": lambda s: host_gang(s, 3, 70, 2),
          "affinity": lambda s: affinity_round(s, 3, 130), "policy": lambda s: policy(s, 1, 70)}


def round_(name, seed):
    return ROUNDS[name](seed)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _matches(selector, labels):
    return selector is not None and all(labels.get(k) == v for k, v in (selector.get("matchLabels") or {}).items())


def _anti_terms(spec):
    return (((spec.get("affinity") or {}).get("podAntiAffinity") or {}).get("requiredDuringSchedulingIgnoredDuringExecution")) or []


def _aff_terms(spec):
    return (((spec.get("affinity") or {}).get("podAffinity") or {}).get("requiredDuringSchedulingIgnoredDuringExecution")) or []


class LiveModel(RoundModel):
    """RoundModel whose frozen verdicts are computed per turn from the pods as they stand. Every pod is in namespace default, selectors
    are matchLabels, nodes are selected by nodeSelector or nodeName, no taints: what the designed rounds use (asserted)."""

    def __init__(self, snapshot, bounds, live=True):
        self.live = live
        self.node_labels = [n["metadata"]["labels"] for n in snapshot["nodes"]]
        self.residents = [[(p["metadata"].get("labels") or {}, _anti_terms(p["spec"])) for p in n["pods"]] for n in snapshot["nodes"]]
        self.ask_labels = {p["metadata"]["uid"]: p["metadata"].get("labels") or {} for p in snapshot["pods"]}
        assert all(not (n["spec"].get("taints")) and not n["spec"].get("unschedulable") for n in snapshot["nodes"])
        super().__init__(snapshot, bounds)
        self.steps = 0

    def start(self):
        super().start()
        self.placed_pods = [[] for _ in self.node_labels]   # (labels, anti terms) of what the round placed
        self.steps = 0

    def settled(self, uid, plugins=("*",)):
        return 3 if super().settled(uid, plugins) == 3 else 0

    def pods_now(self, live):
        """Per node the (labels, anti terms) of its pods: the residents minus the claimed prefix, plus the placed pods."""
        out = []
        for n, name in enumerate(self.names):
            gone = set(self.victims(name, len(self.bounds))[:self.taken[name]]) if live else set()
            out.append([p for i, p in enumerate(self.residents[n]) if i not in gone] + (self.placed_pods[n] if live else []))
        return out

    def frozen_row(self, uid, plugins=("*",)):
        """The verdicts of NodeName, NodeAffinity, PodTopologySpread and InterPodAffinity of one ask on every node, from the pods as they
        stand (live) or as they stood at the start of the round."""
        on = lambda p: "*" in plugins or p in plugins   # noqa: E731
        spec, labels = self.specs[uid], self.ask_labels[uid]
        pods = self.pods_now(self.live)
        N = len(self.names)
        selector = spec.get("nodeSelector") or {}
        selected = [all(self.node_labels[n].get(k) == v for k, v in selector.items()) for n in range(N)]
        ok = [True] * N
        if on("NodeName") and spec.get("nodeName"):
            ok = [ok[n] and self.names[n] == spec["nodeName"] for n in range(N)]
        if on("NodeAffinity"):
            ok = [ok[n] and selected[n] for n in range(N)]
        hard = [c for c in spec.get("topologySpreadConstraints") or [] if c["whenUnsatisfiable"] == "DoNotSchedule"]
        if hard and on("PodTopologySpread"):
            has_all = [all(c["topologyKey"] in self.node_labels[n] for c in hard) for n in range(N)]
            for c in hard:
                key, sel = c["topologyKey"], c.get("labelSelector")
                counts = {}
                for n in range(N):
                    if not has_all[n] or (c.get("nodeAffinityPolicy", "Honor") == "Honor" and not selected[n]):
                        continue
                    d = self.node_labels[n][key]
                    counts[d] = counts.get(d, 0) + sum(1 for pl, _ in pods[n] if _matches(sel, pl))
                minimum = min(counts.values()) if counts else 0
                if len(counts) < c.get("minDomains", 1):
                    minimum = 0
                own = 1 if _matches(sel, labels) else 0
                for n in range(N):
                    if key not in self.node_labels[n]:
                        ok[n] = False
                    elif counts.get(self.node_labels[n][key], 0) + own - minimum > c["maxSkew"]:
                        ok[n] = False
        if on("InterPodAffinity"):
            aff, anti = _aff_terms(spec), _anti_terms(spec)
            # existing pods' terms against the incoming pod
            shut = set()
            for n in range(N):
                for _, terms in pods[n]:
                    for t in terms:
                        if _matches(t.get("labelSelector"), labels) and t["topologyKey"] in self.node_labels[n]:
                            shut.add((t["topologyKey"], self.node_labels[n][t["topologyKey"]]))
            anti_at, aff_at = set(), set()
            for n in range(N):
                for pl, _ in pods[n]:
                    for t in anti:
                        if _matches(t.get("labelSelector"), pl) and t["topologyKey"] in self.node_labels[n]:
                            anti_at.add((t["topologyKey"], self.node_labels[n][t["topologyKey"]]))
                    if aff and all(_matches(t.get("labelSelector"), pl) for t in aff):
                        for t in aff:
                            if t["topologyKey"] in self.node_labels[n]:
                                aff_at.add((t["topologyKey"], self.node_labels[n][t["topologyKey"]]))
            own = bool(aff) and all(_matches(t.get("labelSelector"), labels) for t in aff)
            for n in range(N):
                nl = self.node_labels[n]
                if any((k, nl.get(k)) in shut for k, _ in shut) or any((t["topologyKey"], nl.get(t["topologyKey"])) in anti_at for t in anti):
                    ok[n] = False
                if aff:
                    if any(t["topologyKey"] not in nl for t in aff):
                        ok[n] = False
                    elif not all((t["topologyKey"], nl[t["topologyKey"]]) in aff_at for t in aff) and not (not aff_at and own):
                        ok[n] = False
        return ok

    # ---- the histograms: one ROW per constraint of every distinct topology signature among the asks' templates ------------------------
    def hist_rows(self):
        """→ the rows, as the engine keeps them: per template its hard spread constraints, one row per required affinity term (the pods that
        match ALL terms), one per required anti-affinity term, and one per topology key on which some anti-affinity term of ANY template
        (residents' and asks' alike) matches the template's labels. Templates with equal rows and equal eligibility share them."""
        if hasattr(self, "_rows"):
            return self._rows
        carriers = [terms for pods in self.residents for _, terms in pods if terms] + [_anti_terms(s) for s in self.specs.values() if _anti_terms(s)]
        rows, seen = [], set()
        for uid, spec in self.specs.items():
            labels, selector = self.ask_labels[uid], spec.get("nodeSelector") or {}
            hard = [c for c in spec.get("topologySpreadConstraints") or [] if c["whenUnsatisfiable"] == "DoNotSchedule"]
            keys = [c["topologyKey"] for c in hard]
            mine = []
            for c in hard:
                honor = c.get("nodeAffinityPolicy", "Honor") == "Honor"
                mine.append(("spread", c["topologyKey"], json.dumps(c.get("labelSelector"), sort_keys=True), c["maxSkew"], c.get("minDomains", 1),
                             int(_matches(c.get("labelSelector"), labels)), json.dumps(selector, sort_keys=True) if honor else None, tuple(keys)))
            aff, anti = _aff_terms(spec), _anti_terms(spec)
            for t in aff:
                mine.append(("aff", t["topologyKey"], json.dumps(aff, sort_keys=True), int(all(_matches(x.get("labelSelector"), labels) for x in aff))))
            for t in anti:
                mine.append(("anti", t["topologyKey"], json.dumps(t, sort_keys=True)))
            for key in sorted({t["topologyKey"] for terms in carriers for t in terms if _matches(t.get("labelSelector"), labels)}):
                mine.append(("existing", key, json.dumps(labels, sort_keys=True)))
            if mine and json.dumps(mine) not in seen:
                seen.add(json.dumps(mine))
                rows.extend(mine)
        self._rows = rows
        return rows

    def histograms(self, pods):
        """→ (counts, minima): per row {domain value: matches} over the nodes that count for it, and the row's minimum cell — a spread row's
        minimum over the present domains (0 under the minDomains rule), any other row's number of domains with a match."""
        counts, minima = [], []
        N = len(self.names)
        for row in self.hist_rows():
            kind, key = row[0], row[1]
            cnt, present = {}, set()
            for n in range(N):
                nl = self.node_labels[n]
                if key not in nl:
                    continue
                if kind == "spread":
                    selector = json.loads(row[6]) if row[6] is not None else {}
                    if any(k not in nl for k in row[7]) or any(nl.get(k) != v for k, v in selector.items()):
                        continue
                    sel = json.loads(row[2])
                    v = sum(1 for pl, _ in pods[n] if _matches(sel, pl))
                elif kind == "aff":
                    terms = json.loads(row[2])
                    v = sum(1 for pl, _ in pods[n] if all(_matches(t.get("labelSelector"), pl) for t in terms))
                elif kind == "anti":
                    v = sum(1 for pl, _ in pods[n] if _matches(json.loads(row[2]).get("labelSelector"), pl))
                else:
                    labels = json.loads(row[2])
                    v = sum(1 for _, terms in pods[n] for t in terms if t["topologyKey"] == key and _matches(t.get("labelSelector"), labels))
                present.add(nl[key])
                cnt[nl[key]] = cnt.get(nl[key], 0) + v
            counts.append(cnt)
            if kind == "spread":
                minima.append(0 if len(present) < row[4] or not present else min(cnt[d] for d in present))
            else:
                minima.append(sum(1 for v in cnt.values() if v > 0))
        return counts, minima

    def turn(self, uid, frozen_row=None, plugins=("*",), offset=0):
        before = self.histograms(self.pods_now(True))[0]
        row = super().turn(uid, self.frozen_row(uid, plugins), plugins, offset)
        if row[1] >= 0:
            self.placed_pods[row[1] - offset].append((self.ask_labels[uid], _anti_terms(self.specs[uid])))
            self.steps += sum(1 for a, b in zip(before, self.histograms(self.pods_now(True))[0]) if a != b)
        return row

    def run(self, turns, plugins=("*",)):
        """→ (cells, summary); summary[7] = the (turn, row) pairs whose cell moved. self.hist_start / hist_end: histograms() before the first
        and after the last turn — the round-local histograms move whatever the plugin lists hold."""
        self.start()
        self.hist_start = self.histograms(self.pods_now(True))
        cells = [self.turn(uid, None, plugins) for uid in turns]
        self.hist_end = self.histograms(self.pods_now(True))
        self.hist_placed = self.histograms([list(p) for p in self.placed_pods])
        summary = [sum(1 for c in cells if c[0] == o) for o in range(5)] + [sum(c[3] for c in cells), len({c[1] for c in cells if c[1] >= 0}),
                                                                             self.steps if self.live else 0]
        return cells, summary


def nonzero(values):
    return sorted(int(v) for v in values if v)


def flat(counts):
    """Every cell of a list of rows, as (row, domain) → value."""
    return {(r, d): v for r, row in enumerate(counts) for d, v in row.items()}


def text(snapshot):
    return json.dumps(snapshot)


__all__ = ["ROUNDS", "round_", "LiveModel", "MAX_ASKS"]
