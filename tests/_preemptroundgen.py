"""Designed ROUNDS for ykpred_preempt_round: a snapshot, tier bounds, the list of asks in the order they take their turn (a repeat is one
more copy), what the generator meant to happen to each of them, and a plain model of the round over Python ints.

Pure Python, `random.Random(seed)` only; built on the pieces of tests/_victimgen.py. A round is made of SCENES: a few nodes labelled
scene=<name> and asks whose nodeSelector keeps them there (NodeAffinity is a frozen plugin: on every other node the pair is shut, which is
one of the answers). The scene nodes keep their relative order and some sit at designed indices: ties go by index. N is 70 or 130 — off the wave width — by filler nodes that
are full and carry no scene label. meta["intended"][i] = (outcome, node name or None, from, extra) of turn i under the default lists.

  conflicts   two asks whose independent best node coincides: the second takes further victims there (from > 0) / goes elsewhere; a
              victim whose surplus lets the next ask in at extra 0 on a node that did not fit at round start; a lower-limit ask after a
              higher-limit one took past its tier_end (taken > len), once fitting and once nowhere; pod slots as the only binder, the
              placed pod taking the slot back; a host port: the second copy shut out of the node, a triple with two holders; an
              unsupported and a coupled ask mid-list; a NodeName-pinned ask; limit-0 asks
  exact_lo /  per dimension three nodes: an opener takes the first victim and places free + size0 - 1 (beside 2^53, up to 2^63 - 1); the
  exact_hi    probe then requests free + cum[1] - placed exactly, one below (both: one further victim) and one above (two)
  bisect      segments of 63 / 64 / 65: an opener takes 5, the probes land on both sides of the first two midpoints of (taken, hi]
  places      best nodes at indices 63, 64 and N - 1; an exact key tie that goes to the lower index, across a wave boundary too
  gang_m1 /   copies(limit) - 1, copies(limit) and copies(limit) + 2 turns of one ask (the two beyond separated by another ask: two
  gang_eq /   neighbouring turns never share all their cells)
  gang_p2

One corner is left out on purpose: an ask that wants a port triple which a pod PLACED by the round holds while a later victim of the node
holds it too. The round keeps placed ports (port words | placed_ports); NodeInfo.RemovePod drops the triple with any holder."""
import copy
import random

from _preemptgen import DIMS, I64_MAX, P53, _conflict, _requests, make_node
from _reachgen import BOUNDS, NEVER, T80, asker, tier_priority
from _victimgen import VictimModel, placed, spread_tiers

MAX_ASKS = 40
SPREAD = [{"maxSkew": 1, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": {"app": "web"}}}]
PVC = [{"name": "data", "persistentVolumeClaim": {"claimName": "pvc-1"}}]
T81 = ("10.0.0.1", "TCP", 81)


def mids(taken, hi):
    """The first bisection midpoint over (taken, hi] and the two second ones."""
    m = taken + (hi - taken) // 2
    return m, taken + (m - taken) // 2, m + (hi - m) // 2


class _Round:
    def __init__(self, seed, T, N):
        self.rng = random.Random(seed)
        self.T, self.bounds, self.N = T, BOUNDS[T], N
        self.nodes, self.pool, self.turns, self.intended, self.at = [], {}, [], [], {}

    def tier(self, t):
        return tier_priority(self.bounds, min(t, self.T - 1))

    def node(self, name, scene, alloc, pods, index=None, **more):
        n = make_node(name, alloc, pods, labels={"scene": scene}, **more)
        if index is None:
            self.nodes.append(n)
        else:
            self.at[index] = n

    def ask(self, uid, scene, limit, req=None, ports=None, **spec):
        if scene is not None:
            spec["nodeSelector"] = {"scene": scene}
        self.pool[uid] = asker(uid, self.bounds, min(limit, self.T), req, ports, **spec)
        return uid

    def turn(self, uid, outcome, node=None, start=0, extra=0):
        self.turns.append(uid)
        self.intended.append((outcome, node, start, extra))

    def finish(self, **more):
        """Fillers: full nodes without a scene label whose one resident is in no tier. Designed indices first, the rest in order."""
        fill = self.N - len(self.nodes) - len(self.at)
        assert fill >= 0 and len(self.turns) <= MAX_ASKS, (fill, len(self.turns))
        fillers = [make_node(f"fill-{i}", {"cpu": 5, "memory": 1 << 20}, [placed(f"fill-{i}-r", self.bounds[-1], {"cpu": 5, "memory": 1 << 20})],
                             allowed=1) for i in range(fill)]
        free = [i for i in range(self.N) if i not in self.at]
        mine = set(self.rng.sample(free, len(self.nodes)))   # (the scene nodes keep their relative order: ties go by index)
        scene, nodes = iter(self.nodes), []
        for i in range(self.N):
            nodes.append(self.at[i] if i in self.at else next(scene) if i in mine else fillers.pop())
        snapshot = {"nodes": nodes, "pods": list(self.pool.values())}
        return snapshot, list(self.bounds), dict(turns=list(self.turns), intended=list(self.intended), T=self.T, **more)


# ---- (1) conflicts ---------------------------------------------------------------------------------------------------------------------
def conflicts(seed, T=3, N=70):
    r = _Round(seed, T, N)
    lo, mid, top = r.tier(0), r.tier(1), r.tier(2)
    mem = {"memory": 1 << 30}
    # cs: the best node of both asks is cs-a (tier 0); the second takes a further victim there — cs-b would cost a higher tier
    r.node("cs-a", "cs", {"cpu": 400, **mem}, [placed(f"cs-a-v{i}", lo, {"cpu": 100}) for i in range(4)])
    r.node("cs-b", "cs", {"cpu": 300, **mem}, [placed(f"cs-b-v{i}", mid, {"cpu": 100}) for i in range(3)])
    # ca: the second ask goes elsewhere — the next victim of ca-a sits two tiers up
    r.node("ca-a", "ca", {"cpu": 200, **mem}, [placed("ca-a-v0", lo, {"cpu": 100}), placed("ca-a-v1", top, {"cpu": 100})])
    r.node("ca-b", "ca", {"cpu": 100, **mem}, [placed("ca-b-v0", mid, {"cpu": 100})])
    # su: one victim of 300m; the next two asks live off its surplus
    r.node("su", "su", {"cpu": 300, **mem}, [placed("su-v0", lo, {"cpu": 300})])
    # ll: the high ask takes both victims, past the low ask's tier_end
    r.node("ll", "ll", {"cpu": 200, **mem}, [placed("ll-v0", lo, {"cpu": 100}), placed("ll-v1", mid if T > 1 else lo, {"cpu": 100})])
    # sl: full by pod count alone; two zero-request victims
    r.node("sl", "sl", {"cpu": 64000, **mem}, [placed("sl-v0", lo, {}), placed("sl-v1", lo, {}), placed("sl-keep", r.bounds[-1], {"cpu": 10})], allowed=3)
    # po: one holder of the port; pt: two holders of another triple — the first frees it
    r.node("po", "po", {"cpu": 64000, **mem}, [placed("po-h", lo, {"cpu": 10}, ports=[T80])])
    r.node("pt", "pt", {"cpu": 64000, **mem}, [placed("pt-h0", lo, {"cpu": 10}, ports=[T81]), placed("pt-h1", lo, {"cpu": 10}, ports=[T81])])
    r.node("l0", "l0", {"cpu": 100, **mem}, [placed("l0-v0", lo, {"cpu": 100})])
    a = r.ask
    r.turn(a("cs-1", "cs", 3, {"cpu": 100}), 1, "cs-a", 0, 1)
    r.turn(a("cs-2", "cs", 3, {"cpu": 100}), 1, "cs-a", 1, 1)
    r.turn(a("ca-1", "ca", 3, {"cpu": 100}), 1, "ca-a", 0, 1)
    r.turn(a("routed", "cs", 3, {"cpu": 100}, volumes=PVC), 3)
    r.turn(a("ca-2", "ca", 3, {"cpu": 100}), 1, "ca-b" if T > 1 else "ca-a", 0 if T > 1 else 1, 1)
    r.turn(a("su-1", "su", 3, {"cpu": 100}), 1, "su", 0, 1)
    r.turn(a("coupled", "su", 3, {"cpu": 100}, topologySpreadConstraints=SPREAD), 4)
    r.turn(a("su-2", "su", 3, {"cpu": 150}), 0, "su", 1, 0)
    r.turn(a("su-0", "su", 0, {"cpu": 50}), 0, "su", 1, 0)          # limit 0: only what is free, and the surplus is
    r.turn(a("su-3", "su", 3, {"cpu": 1}), 2)
    r.turn(a("ll-hi", "ll", 3, {"cpu": 150}), 1, "ll", 0, 2)
    r.turn(a("ll-lo", "ll", 1, {"cpu": 50}), 0, "ll", 2, 0)          # taken == 2 > tier_end[0] == 1
    r.turn(a("ll-lo2", "ll", 1, {"cpu": 50}), 2)
    r.turn(a("sl-1", "sl", 3, {}), 1, "sl", 0, 1)
    r.turn(a("sl-2", "sl", 3, {"cpu": 1}), 1, "sl", 1, 1)            # the placed pod took the slot back
    r.turn(a("sl-3", "sl", 3, {}), 2)
    r.turn(a("po-1", "po", 3, {"cpu": 1}, ports=[T80]), 1, "po", 0, 1)
    r.turn("cs-1", 1, "cs-a", 2, 1)                                   # (a repeat: one more copy)
    r.turn(a("po-2", "po", 3, {"cpu": 1}, ports=[T80]), 2)            # the first copy holds the port now
    r.turn(a("pt-1", "pt", 3, {"cpu": 1}, ports=[T81]), 1, "pt", 0, 1)
    r.turn(a("pt-2", "pt", 3, {"cpu": 2}), 0, "pt", 1, 0)
    r.turn(a("pin", None, 3, {"cpu": 100}, nodeName="cs-b"), 1, "cs-b", 0, 1)
    r.turn(a("l0-0", "l0", 0, {"cpu": 100}), 2)                       # limit 0 on a full node
    r.turn(a("l0-1", "l0", 1, {"cpu": 100}), 1, "l0", 0, 1)
    return r.finish()


# ---- (2) requests at free + cum - placed -------------------------------------------------------------------------------------------------
def exact(seed, T=8, N=130, dims=range(4)):
    r = _Round(seed, T, N)
    rng = r.rng
    for j in dims:
        d = DIMS[j]
        for delta in (-1, 0, 1):
            name = f"rx-{j}-{delta + 1}"
            sizes = {o: [rng.randrange(2, 10) for _ in range(3)] for o in DIMS}
            free = {}
            for i, o in enumerate(DIMS):
                mag = ("small", "across", "above", "ends")[(i + j) % 4]
                free[o] = {"small": rng.randrange(20, 30), "across": P53 - sizes[o][0], "above": P53 + 1, "ends": I64_MAX - 1 - sum(sizes[o])}[mag]
            prios = sorted(tier_priority(r.bounds, min(t, T - 1), rng) for t in (0, 1, 2))
            pods = [placed(f"{name}-v{i}", p, {o: sizes[o][i] for o in DIMS}) for i, p in enumerate(prios)]
            rng.shuffle(pods)
            alloc = {o: free[o] + sum(sizes[o]) for o in DIMS}
            assert all(0 <= v <= I64_MAX for v in alloc.values())
            r.node(name, name, alloc, pods)
            opener = {o: free[o] for o in DIMS if o != d}
            opener[d] = free[d] + sizes[d][0] - 1            # needs the first victim, leaves 1 of dimension d
            r.turn(r.ask(f"a-{name}-open", name, T, opener), 1, name, 0, 1)
            probe = {d: free[d] + sizes[d][0] + sizes[d][1] - opener[d] + delta}
            r.turn(r.ask(f"a-{name}-probe", name, T, probe), 1, name, 1, 1 if delta <= 0 else 2)
    return r.finish()


def exact_hi(seed, T=8, N=130):
    return exact(seed + 1, T, N, dims=range(4, 8))


# ---- (3) the bisection from a taken prefix -----------------------------------------------------------------------------------------------
def bisect(seed, T=3, N=130, taken=5):
    r = _Round(seed, T, N)
    rng = r.rng
    for length in (63, 64, 65):
        m, m_lo, m_hi = mids(taken, length)
        for k in (m, m + 1, m_lo + 1, m_hi):
            name = f"lg-{length}-{k}"
            pods = [placed(f"{name}-v{i:02d}", p, {"cpu": 10}) for i, p in enumerate(spread_tiers(r.bounds, length, rng))]
            rng.shuffle(pods)
            r.node(name, name, {"cpu": 10 * length, "memory": 1 << 30}, pods)
            r.turn(r.ask(f"a-{name}-open", name, T, {"cpu": 10 * taken}), 1, name, 0, taken)
            r.turn(r.ask(f"a-{name}-probe", name, T, {"cpu": 10 * (k - taken)}), 1, name, taken, k - taken)
    return r.finish(taken=taken)


# ---- (4) where the best node sits ---------------------------------------------------------------------------------------------------------
def places(seed, T=3, N=130):
    r = _Round(seed, T, N)
    lo = r.tier(0)
    one = lambda name, cpu=100: [placed(f"{name}-v{i}", lo, {"cpu": cpu}) for i in range(2)]   # noqa: E731
    for index in (63, 64, N - 1):
        r.node(f"at-{index}", f"at-{index}", {"cpu": 200, "memory": 1 << 30}, one(f"at-{index}"), index=index)
    r.node("tie-a", "tie", {"cpu": 200, "memory": 1 << 30}, one("tie-a"), index=10)
    r.node("tie-b", "tie", {"cpu": 200, "memory": 1 << 30}, one("tie-b"), index=20)
    r.node("wv-a", "wv", {"cpu": 200, "memory": 1 << 30}, one("wv-a"), index=127)   # a tie across the wave boundary 127 | 128
    r.node("wv-b", "wv", {"cpu": 200, "memory": 1 << 30}, one("wv-b"), index=128)
    for index in (63, 64, N - 1):
        r.turn(r.ask(f"a-at-{index}", f"at-{index}", T, {"cpu": 100}), 1, f"at-{index}", 0, 1)
    for scene, first, second in (("tie", "tie-a", "tie-b"), ("wv", "wv-a", "wv-b")):
        r.turn(r.ask(f"a-{scene}-1", scene, T, {"cpu": 100}), 1, first, 0, 1)
        r.turn(r.ask(f"a-{scene}-2", scene, T, {"cpu": 100}), 1, first, 1, 1)    # the tie again: extra 1 on both
        r.turn(r.ask(f"a-{scene}-3", scene, T, {"cpu": 100}), 1, second, 0, 1)
        r.turn(r.ask(f"a-{scene}-4", scene, T, {"cpu": 300}), 2)
    return r.finish()


# ---- (5) gangs -----------------------------------------------------------------------------------------------------------------------------
def gang(seed, T=3, N=70, beyond=0):
    """g-a: 100m free, three 100m victims below the gang's limit and one above; g-b: two victims. copies(limit) == 1 + 3 + 2 == 6."""
    r = _Round(seed, T, N)
    limit = max(1, T - 1)
    below, above = tier_priority(r.bounds, limit - 1), tier_priority(r.bounds, limit)
    r.node("g-a", "g", {"cpu": 500, "memory": 1 << 30}, [placed(f"g-a-v{i}", below, {"cpu": 100}) for i in range(3)] + [placed("g-a-top", above, {"cpu": 100})])
    r.node("g-b", "g", {"cpu": 200, "memory": 1 << 30}, [placed(f"g-b-v{i}", below, {"cpu": 100}) for i in range(2)])
    r.ask("gang", "g", limit, {"cpu": 100})
    r.ask("other", "g", 0, {"cpu": 1000})
    copies = 6
    plan = [(0, "g-a", 0, 0), (1, "g-a", 0, 1), (1, "g-a", 1, 1), (1, "g-a", 2, 1), (1, "g-b", 0, 1), (1, "g-b", 1, 1)]
    for i in range(min(copies + beyond, copies)):
        r.turn("gang", *plan[i])
    for i in range(max(beyond, 0)):
        r.turn("gang", 2)
        r.turn("other", 2)
    return r.finish(copies=copies, gang="gang", limit=limit)


def geometry(seed, n_nodes, n_asks=70, T=3, most=12):
    """The shape of a large launch: n_nodes nodes with 0..9 cpu free and 0..most residents of 20..60 cpu over random priorities, and
    n_asks asks that are n_asks DISTINCT (request, limit) tasks of 10 cpu and more, in non-increasing limit order: most need a victim or
    two, and the lowest-index node with cheap victims is taken again and again. No intent: the model, or the host loop, decides."""
    rng = random.Random(seed * 1000 + n_nodes)
    b = BOUNDS[T]
    nodes = []
    for n in range(n_nodes):
        count = rng.randrange(0, most + 1)
        pods = [placed(f"g{n}-v{rng.randrange(10 ** 6):06d}-{i}", rng.randrange(b[0] - 5, b[-1] + 3), {"cpu": rng.randrange(20, 61)}) for i in range(count)]
        used = sum(_requests(p).get("cpu", 0) for p in pods)
        nodes.append(make_node(f"g{n:04d}", {"cpu": used + rng.randrange(0, 10), "memory": 1 << 40}, pods, allowed=rng.choice((count + 1, 110))))
    asks = [asker(f"a-g{i:02d}", b, i % (T + 1), {"cpu": 10 + i}) for i in range(n_asks)]
    asks.sort(key=lambda p: (-i_limit(p, b), p["metadata"]["uid"]))
    return {"nodes": nodes, "pods": asks}, list(b), {"T": T, "turns": [p["metadata"]["uid"] for p in asks]}


def i_limit(pod, bounds):
    return sum(1 for bound in bounds if bound <= (pod["spec"].get("priority") or 0))


ROUNDS = {"conflicts": lambda s: conflicts(s, 3, 70), "conflicts_1": lambda s: conflicts(s, 1, 130), "conflicts_8": lambda s: conflicts(s, 8, 70),
          "exact_lo": lambda s: exact(s), "exact_hi": lambda s: exact_hi(s), "bisect": lambda s: bisect(s, 3), "bisect_8": lambda s: bisect(s, 8, 70),
          "places": lambda s: places(s), "gang_m1": lambda s: gang(s, 3, 70, -1), "gang_eq": lambda s: gang(s, 8, 130, 0),
          "gang_p2": lambda s: gang(s, 1, 70, 2)}


def round_(name, seed):
    return ROUNDS[name](seed)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
class RoundModel(VictimModel):
    """VictimModel with the round's state: taken[node] and the (request, wanted ports) of the asks placed on each node."""

    def __init__(self, snapshot, bounds):
        super().__init__(snapshot, bounds)
        self.names = [n["metadata"]["name"] for n in snapshot["nodes"]]
        self.specs = {p["metadata"]["uid"]: p["spec"] for p in snapshot["pods"]}
        self.start()

    def start(self):
        self.taken = {n: 0 for n in self.names}
        self.placed_on = {n: [] for n in self.names}

    def settled(self, uid, plugins=("*",)):
        """3 for an ask the engine does not evaluate, 4 for a coupled one under these lists, else 0."""
        spec = self.specs[uid]
        if any("persistentVolumeClaim" in v for v in spec.get("volumes") or []):
            return 3
        # (ykpred_headroom's rule: the spec carries a topology signature and either topology plugin is in the lists)
        if spec.get("topologySpreadConstraints") and ("*" in plugins or "PodTopologySpread" in plugins or "InterPodAffinity" in plugins):
            return 4
        return 0

    def need_more(self, uid, node, frozen, plugins=("*",)):
        """→ (extra, level): the further victims beyond taken[node], NEVER when no k in [taken, hi] passes."""
        fit_on, ports_on = ("*" in plugins or "NodeResourcesFit" in plugins), ("*" in plugins or "NodePorts" in plugins)
        request, wanted, limit = self.asks[uid]
        alloc, allowed, pods = self.nodes[node]
        if not frozen:
            return NEVER, 0
        order = self.victims(node, len(self.bounds))
        taken = self.taken[node]
        hi = max(taken, len(self.victims(node, limit)))
        mine = self.placed_on[node]
        for k in range(taken, hi + 1):
            gone = set(order[:k])
            left = [p for i, p in enumerate(pods) if i not in gone]
            free = {d: alloc.get(d, 0) - sum(req.get(d, 0) for req, _, _ in left) - sum(req.get(d, 0) for req, _ in mine) for d in request}
            used = ({t for _, held, _ in pods for t in held} - {t for i in gone for t in pods[i][1]}) | {t for _, held in mine for t in held}
            fits = not fit_on or (len(left) + len(mine) + 1 <= allowed and all(q <= free[d] for d, q in request.items() if q > 0))
            if fits and not (ports_on and any(_conflict(w, used) for w in wanted)):
                return k - taken, (0 if k == taken else pods[order[k - 1]][2] + 1)
        return NEVER, 0

    def turn(self, uid, frozen_row, plugins=("*",), offset=0):
        """One ask takes its turn: → its 8 cells; the state moves. frozen_row[n]: the frozen verdict of the pair (uid, node n)."""
        limit = self.asks[uid][2]
        settled = self.settled(uid, plugins)
        if settled:
            return [settled, -1, 0, 0, 0, limit, 0, 0]
        needs = [self.need_more(uid, node, bool(frozen_row[n]), plugins) for n, node in enumerate(self.names)]
        keys = [(level, min(extra, (1 << 28) - 1), n) for n, (extra, level) in enumerate(needs) if extra >= 0]
        if not keys:
            return [2, -1, 0, 0, 0, limit, 0, 0]
        level, extra, n = min(keys)
        node = self.names[n]
        start = self.taken[node]
        self.taken[node] += extra
        self.placed_on[node].append((self.asks[uid][0], self.asks[uid][1]))
        return [1 if extra else 0, n + offset, start, extra, level, limit, len(keys), sum(e for _, e, _ in keys)]

    def run(self, turns, frozen, ask_index, plugins=("*",)):
        """The whole round from zero state: → (cells [turns][8], summary [8]). frozen[a][n] by ask index."""
        self.start()
        cells = [self.turn(uid, frozen[ask_index[uid]], plugins) for uid in turns]
        summary = [sum(1 for c in cells if c[0] == o) for o in range(5)] + [sum(c[3] for c in cells), len({c[1] for c in cells if c[1] >= 0}), 0]
        return cells, summary

    def victims_of(self, cells_row):
        node = self.names[cells_row[1]]
        order = self.victims(node, len(self.bounds))
        return [self.uids[node][i] for i in order[cells_row[2]:cells_row[2] + cells_row[3]]]


def edited(snapshot, model, uid, cells_row, copy_no):
    """The snapshot after a turn: the victims deleted from the node, the placed pod — a copy of the ask under a uid of its own — added."""
    node = snapshot["nodes"][cells_row[1]]
    gone = set(model.victims_of(cells_row))
    node["pods"] = [p for p in node["pods"] if p["metadata"]["uid"] not in gone]
    pod = copy.deepcopy(next(p for p in snapshot["pods"] if p["metadata"]["uid"] == uid))
    pod["metadata"]["uid"] = pod["metadata"]["name"] = f"{uid}.placed{copy_no}"
    pod["spec"]["nodeName"] = node["metadata"]["name"]
    pod["spec"].pop("nodeSelector", None)
    pod["status"] = {"phase": "Running"}
    node["pods"].append(pod)
    return gone


__all__ = ["ROUNDS", "round_", "RoundModel", "edited", "mids", "MAX_ASKS", "NEVER"]
