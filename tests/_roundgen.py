"""Designed clusters for the conflict-resolved allocation rounds (k_allocate_round, the batched form and its host replay): every
population sits ON a limit the round's code branches on, and says so. Each generator returns (snapshot, meta); meta["expect"] is the
node the generator INTENDS for every ask, derived from how the cluster is laid out (never from running anything), next to the
claims the population makes about itself (run lengths and header offsets, binding dimensions, moved winners, slot numbers ...).
tests/test_round_inputs.py holds the oracle's sequential loop against all of it on the CPU; tests/test_gpu_rounds_designed.py
holds the device against the oracle. Pure Python, tests only.

What the intentions rest on (oracle/ykoracle.cpp, binpack_score): nodes are tried in ascending (score, NodeID), score = 1 - mean
utilisation of cpu and memory — a node that holds something stands before every empty one, empty nodes stand in name order, and a
pod that requests neither cpu nor memory does not move its node."""

I64_MAX = 2 ** 63 - 1
RES8 = ["cpu", "memory", "ephemeral-storage"] + [f"example.com/r{r}" for r in range(3, 8)]
WINDOW = 64            # asks whose headers one load round of k_allocate_round holds (kWave)
SLOTS_PER_LOAD = 64 * 512  # moved-node slots one load round of the bitsets covers (64 steps x kRoundThreads)


def _q(res, v):
    return f"{v}m" if res == "cpu" else str(v)


def _node(name, alloc, pods, labels=None, taints=(), resident=()):
    a = {k: _q(k, v) for k, v in alloc.items()}
    a["pods"] = str(pods)
    return {"metadata": {"name": name, "labels": dict(labels or {})}, "spec": {"taints": [dict(t) for t in taints]},
            "status": {"allocatable": a}, "pods": list(resident)}


def _pod(uid, req, labels=None, ports=(), **spec):
    c = {"name": "c", "resources": {"requests": {k: _q(k, v) for k, v in req.items()}}}
    if ports:
        c["ports"] = [{"hostPort": p, "containerPort": p} for p in ports]
    return {"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": dict(labels or {})}, "spec": dict({"containers": [c]}, **spec)}


class _Stream:
    """An ask list under construction: every ask with the node it is meant for; `run` records a run the generator intends."""

    def __init__(self):
        self.nodes, self.pods, self.expect, self.spec_of, self.runs = [], [], [], [], []

    def node(self, *a, **kw):
        self.nodes.append(_node(*a, **kw))
        return self.nodes[-1]["metadata"]["name"]

    def ask(self, spec_name, req, node, **kw):
        self.pods.append(_pod(f"ask-{len(self.pods):06d}", req, **kw))
        self.expect.append(node)
        self.spec_of.append(spec_name)

    def run(self, spec_name, req, node, n, **kw):
        if n > 1:
            self.runs.append({"start": len(self.pods), "length": n, "node": node, "spec": spec_name, "offset": len(self.pods) % WINDOW})
        for _ in range(n):
            self.ask(spec_name, req, node, **kw)

    def finish(self, **meta):
        index = {n["metadata"]["name"]: i for i, n in enumerate(self.nodes)}
        meta.update(expect=[-1 if e is None else index[e] for e in self.expect], spec_of=self.spec_of, runs=self.runs)
        return {"nodes": self.nodes, "pods": self.pods}, meta


# ---------------------------------------------------------------------------------------------------------------------------
# 1. runs: run lengths decided by arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def runs():
    """R = 8, 56 nodes, 572 asks (the padding between the header offsets is most of them). Every spec is bound to its own group of
    nodes by a nodeSelector (one requirement per spec: no topology, W = 1), so what a spec's asks do is closed form inside the group: they pile onto the group's current node
    while it holds one more copy, then take the next empty node in name order.
      dim<d>: free = 3 req, 3 req - 1, 3 req + 1 in dimension d and ample elsewhere -> runs of 3, 2, 3, d = 0..7
      slots:  the smallest quotient is 4; pod slots 3, 4, 5 -> runs of 3 (dead), 4 (dead), 4 (one slot left: a one-slot ask of another
              spec must still land there); then 6 slots and a quotient of 4 with a resident pod -> `allowed - count` = 5
      zero:   no request at all: only the slots bound the run (5, then 2)
      big:    memory request 2^53 + 1 on nodes of 2^63 - 1 bytes whose residents leave 1 and 2 copies; a fourth ask fits nothing
      win:    runs of one spec starting at header offsets 0, 1, 62, 63; one of 4 that ends with its window while the node holds 10
              (the next window starts with another spec); 130 on one node across two window edges; runs cut by a pin of the same
              spec to another node, by a nodeName that names no node, by one ask of another spec with 0 and with 1 copies left
      port:   six asks of a spec with a host port: twins conflict, one node each
      the list ends inside a run the node could continue."""
    s = _Stream()
    ample = {"cpu": 64000, "memory": 1 << 40, "ephemeral-storage": 1 << 40}
    ample.update({r: 10 ** 6 for r in RES8[3:]})
    fillers = {}

    def filler(k=None):
        """One ask of a spec no neighbour shares (two filler specs alternate): 110 per node, node after node."""
        k = len(s.pods) % 2 if k is None else k
        st = fillers.setdefault(k, {"n": 0})
        if st["n"] % 110 == 0:
            st["node"] = s.node(f"fill{k}-{st['n'] // 110:02d}", ample, 110, labels={"grp": f"fill{k}"})
        st["n"] += 1
        s.ask(f"fill{k}", {"cpu": 10, "memory": 1 << 20}, st["node"], nodeSelector={"grp": f"fill{k}"})

    def pad_to(offset):
        filler()  # (at least one: the run behind it does not continue the one in front)
        while len(s.pods) % WINDOW != offset:
            filler()

    binding = []
    req8 = {"cpu": 300, "memory": 3 << 20, "ephemeral-storage": 5 << 20, RES8[3]: 3, RES8[4]: 7, RES8[5]: 2, RES8[6]: 11, RES8[7]: 13}
    for d, res in enumerate(RES8):
        sel = {"grp": f"dim{d}"}
        for j, (extra, k) in enumerate(((0, 3), (-1, 2), (1, 3))):
            alloc = dict(ample)
            alloc[res] = 3 * req8[res] + extra
            name = s.node(f"dim{d}-{j}", alloc, 110, labels=sel)
            binding.append({"start": len(s.pods), "dimension": d, "resource": res, "free": alloc[res], "request": req8[res], "copies": k})
            s.run(f"dim{d}", req8, name, k, nodeSelector=sel)
        filler()
    # pod slots one below, on and one above the smallest quotient (cpu: 4 copies)
    sel, rq = {"grp": "slots"}, {"cpu": 1000, "memory": 1 << 20}
    slots = []
    for j, (allowed, k) in enumerate(((3, 3), (4, 4), (5, 4))):
        name = s.node(f"slots-{j}", dict(ample, cpu=4000), allowed, labels=sel)
        slots.append({"start": len(s.pods), "allowed": allowed, "quotient": 4, "copies": k})
        s.run("slots", rq, name, k, nodeSelector=sel)
    last_slot = {"ask": len(s.pods), "node": "slots-2"}
    s.ask("slots-one", {"memory": 1 << 20}, "slots-2", nodeSelector=sel)  # the fifth slot of slots-2: the node is not dead
    resident = _pod("slots-resident", {}, nodeName="slots-3")  # (no requests: the node stays as empty as its neighbours)
    name = s.node("slots-3", dict(ample, cpu=4000), 6, labels=sel, resident=[resident])
    slots.append({"start": len(s.pods), "allowed": 6, "quotient": 4, "copies": 4})
    s.run("slots", rq, name, 4, nodeSelector=sel)
    s.ask("slots-one", {"memory": 1 << 20}, "slots-3", nodeSelector=sel)
    filler()
    # no positive request: the quotient is INT64_MAX in every lane
    sel = {"grp": "zero"}
    zero = []
    for j, allowed in enumerate((5, 2)):
        name = s.node(f"zero-{j}", ample, allowed, labels=sel)
        zero.append({"start": len(s.pods), "copies": allowed})
        s.run("zero", {}, name, allowed, nodeSelector=sel)
    filler()
    # requests beside 2^53 on nodes of 2^63 - 1
    sel, rq = {"grp": "big"}, {"cpu": 100, "memory": 2 ** 53 + 1}
    big = []
    for j, (copies, left) in enumerate(((1, (2 ** 53 + 1) + 2 ** 52), (2, 2 * (2 ** 53 + 1) + 7))):
        res_pod = _pod(f"big-resident-{j}", {"memory": I64_MAX - left}, nodeName=f"big-{j}")
        name = s.node(f"big-{j}", dict(ample, memory=I64_MAX), 110, labels=sel, resident=[res_pod])
        big.append({"start": len(s.pods), "free": left, "request": rq["memory"], "copies": copies})
        s.run("big", rq, name, copies, nodeSelector=sel)
    s.ask("big", rq, None, nodeSelector=sel)
    # the header window
    sel, rq = {"grp": "win"}, {"cpu": 100}
    wn = [0]

    def wnode(copies, allowed=200):
        wn[0] += 1
        return s.node(f"win-{wn[0]:02d}", dict(ample, cpu=100 * copies), allowed, labels=sel)

    offsets = []
    for off in (0, 1, 62, 63):
        pad_to(off)
        offsets.append(len(s.pods))
        s.run("win", rq, wnode(5), 5, nodeSelector=sel)
    pad_to(60)
    window_end = {"start": len(s.pods), "length": 4, "node_holds": 10}
    a = wnode(10)
    s.run("win", rq, a, 4, nodeSelector=sel)  # 60..63, then another spec opens the next window
    filler()
    filler()
    s.run("win", rq, a, 6, nodeSelector=sel)  # (the node is emptied of copies: later runs start on empty nodes)
    pad_to(10)
    long_run = {"start": len(s.pods), "length": 130}
    s.run("win", rq, wnode(130), 130, nodeSelector=sel)
    # a pin of the same spec to another node inside the run (that node holds exactly the pinned copy)
    filler()
    a, pinned_to = wnode(6), s.node("win-pin", dict(ample, cpu=100), 200, labels=sel)
    pin_cut = {"start": len(s.pods), "pinned": len(s.pods) + 3}
    s.run("win", rq, a, 3, nodeSelector=sel)
    s.ask("win", rq, pinned_to, nodeSelector=sel, nodeName=pinned_to)
    s.run("win", rq, a, 3, nodeSelector=sel)
    filler()
    a = wnode(6)
    no_node_cut = {"start": len(s.pods), "pinned": len(s.pods) + 3}
    s.run("win", rq, a, 3, nodeSelector=sel)
    s.ask("win", rq, None, nodeSelector=sel, nodeName="no-such-node")
    s.run("win", rq, a, 3, nodeSelector=sel)
    # one ask of another spec inside the run; the node has exactly 0 / exactly 1 copy left when the spec resumes
    filler()
    resumes = []
    a, b = wnode(4), wnode(3)
    s.run("win", rq, a, 4, nodeSelector=sel)
    filler(0)
    resumes.append({"ask": len(s.pods), "left": 0})
    s.run("win", rq, b, 3, nodeSelector=sel)
    filler()
    a, b = wnode(4), wnode(2)
    s.run("win", rq, a, 3, nodeSelector=sel)
    filler(0)
    resumes.append({"ask": len(s.pods), "left": 1})
    s.ask("win", rq, a, nodeSelector=sel)
    s.run("win", rq, b, 2, nodeSelector=sel)
    # a host port: no run
    filler()
    sel_p = {"grp": "port"}
    port = {"start": len(s.pods), "length": 6}
    for j in range(6):
        name = s.node(f"port-{j}", ample, 110, labels=sel_p)
        s.ask("port", {"cpu": 100}, name, nodeSelector=sel_p, ports=(8080,))
    filler()
    # the end of the list cuts a run the node could continue
    tail = {"start": len(s.pods), "length": 7, "node_holds": 20}
    s.run("win", rq, wnode(20), 7, nodeSelector=sel)
    return s.finish(binding=binding, slots=slots, last_slot=last_slot, zero=zero, big=big, offsets=offsets, window_end=window_end,
                    long_run=long_run, pin_cut=pin_cut, no_node_cut=no_node_cut, resumes=resumes, port=port, tail=tail,
                    split=long_run["start"] + 40)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. wide: the limits of the flat form of the scan over the moved nodes
# ---------------------------------------------------------------------------------------------------------------------------
WIDE = ["r4", "r5", "kt1", "kt2", "w4", "w5", "w8", "w9", "kp1", "kp2", "terms64", "terms68", "names64", "names68"]
WIDE_DIMS = {  # variant: (the table dimension it sets, its value, whether every spec still takes the flat form of the scan)
    "r4": ("R", 4, True), "r5": ("R", 5, False), "kt1": ("KT", 1, True), "kt2": ("KT", 2, False),
    "w4": ("W", 4, True), "w5": ("W", 5, False), "w8": ("W", 8, False), "w9": ("W", 9, False),
    "kp1": ("KP", 1, True), "kp2": ("KP", 2, False),
    "terms64": ("W", 4, True), "terms68": ("W", 4, False), "names64": ("W", 4, True), "names68": ("W", 4, False),
}


def _never(n, tag):
    """n label requirements no node satisfies, as the matchExpressions of ONE term."""
    return [{"key": f"never-{tag}-{k}", "operator": "In", "values": ["x"]} for k in range(n)]


def _affinity(terms):
    return {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": terms}}}


def wide(variant):
    """About 60 nodes of 5 cores, about 300 asks of one core (names64 / names68: 16 / 17 pairs of nodes, one per PreFilter name row,
    so 32 / 34 nodes and 164 / 174 asks). Nodes alternate by name: `plain` (even) and `good` (odd). Spec X fits
    every node, spec Y fits the good ones only — and what keeps Y off a plain node is ONE bit or value in the LAST word / dimension
    of the table the variant widens (the last resource, the last taint of the dictionary, the last label requirement, the last
    host port, the last term row). X and Y alternate, so pair p of nodes is filled by asks 10p .. 10p + 9: X onto the plain node, Y
    onto the good one. From its second ask on, every ask wins a node that already took a pod this round; and every Y but the last
    of a pair passes a moved plain node that stands FIRST in the order (as full as Y's node, earlier name), has room, and is turned
    down by that one bit alone. kp1 / kp2 differ (a host port is taken once per node): see _wide_ports."""
    if variant in ("kp1", "kp2"):
        return _wide_ports(variant)
    s = _Stream()
    pairs = {"names64": 16, "names68": 17}.get(variant, 30)
    alloc = {"cpu": 5000, "memory": 8 << 30, "ephemeral-storage": 1 << 40}
    x_req, y_req = {"cpu": 1000, "memory": 1 << 20}, {"cpu": 1000, "memory": 1 << 20}
    x_spec, y_spec, plain_kw, good_kw, pre = {}, {}, {}, {}, []
    good_names = [f"n{2 * p + 1:03d}" for p in range(pairs)]
    if variant in ("r4", "r5"):
        last = RES8[3] if variant == "r4" else RES8[4]
        y_req[last] = 1
        good_kw["extra"] = {last: 5}
        plain_kw["extra"] = {last: 0}
        if variant == "r5":  # (dimension 3 exists and is requested by everybody: the deciding one is dimension 4)
            x_req[RES8[3]] = y_req[RES8[3]] = 1
            good_kw["extra"][RES8[3]] = plain_kw["extra"][RES8[3]] = 100
    elif variant in ("kt1", "kt2"):
        n_common = 63 if variant == "kt1" else 64
        common = [{"key": f"t{k:02d}", "value": "v", "effect": "NoSchedule"} for k in range(n_common)]
        deciding = {"key": "zz-deciding", "value": "v", "effect": "NoSchedule"}
        good_kw["taints"], plain_kw["taints"] = common, common + [deciding]  # (the deciding taint enters the dictionary last)
        x_spec["tolerations"] = [{"operator": "Exists"}]
        # (taints that the same toleration lists tolerate share a bit: seven asks that fit nothing tolerate the common taints by
        # the binary digits of their number, so that every taint has a bit of its own)
        for b in range(7):
            tol = [{"key": t["key"], "operator": "Equal", "value": "v", "effect": "NoSchedule"} for k, t in enumerate(common) if (k + 1) >> b & 1]
            pre.append(("digit", {"cpu": 1000}, {"tolerations": tol}))
        y_spec["tolerations"] = [{"key": t["key"], "operator": "Equal", "value": "v", "effect": "NoSchedule"} for t in common]
    elif variant in ("w4", "w5", "w8", "w9"):
        total = {"w4": 224, "w5": 257, "w8": 480, "w9": 513}[variant]  # (the dictionary keeps 32 spare bits: W = (total + 32 + 63) // 64)
        left, k = total - 1, 0
        while left > 0:  # asks that fit nothing and come first: their requirements fill the dictionary in front of Y's
            n = min(left, 64)
            pre.append(("never", {"cpu": 1000}, {"affinity": _affinity([{"matchExpressions": _never(n, f"z{k}")}])}))
            left, k = left - n, k + 1
        good_kw["labels"] = {"want": "yes"}
        y_spec["nodeSelector"] = {"want": "yes"}
    elif variant in ("terms64", "terms68"):
        n_terms = 16 if variant == "terms64" else 17
        terms = [{"matchExpressions": _never(30 - n_terms, f"t{k}")} for k in range(n_terms - 1)]  # 211 / 209 requirements: W = 4
        terms.append({"matchExpressions": [{"key": "want", "operator": "In", "values": ["yes"]}]})  # the LAST term row is the one that matches
        good_kw["labels"] = {"want": "yes"}
        y_spec["affinity"] = _affinity(terms)
    elif variant in ("names64", "names68"):
        n_names = len(good_names)  # one PreFilter name row (and one Filter term row) per good node
        fill = 224 - 2 * n_names   # (every name is a metadata.name field requirement and a PreFilter name: two dictionary entries)
        k = 0
        while fill > 0:
            n = min(fill, 64)
            pre.append(("never", {"cpu": 1000}, {"affinity": _affinity([{"matchExpressions": _never(n, f"z{k}")}])}))
            fill, k = fill - n, k + 1
        y_spec["affinity"] = _affinity([{"matchFields": [{"key": "metadata.name", "operator": "In", "values": [nm]}]} for nm in good_names])
    for p in range(pairs):
        for kind, kw in (("plain", plain_kw), ("good", good_kw)):
            name = f"n{2 * p + (kind == 'good'):03d}"
            s.node(name, dict(alloc, **kw.get("extra", {})), 110, labels=dict({"kind": kind}, **kw.get("labels", {})), taints=kw.get("taints", ()))
    for tag, rq, extra in pre:
        s.ask(f"{tag}-{len(s.pods)}", rq, None, **extra)
    first = len(s.pods)
    for p in range(pairs):
        for k in range(5):
            s.ask("x", x_req, f"n{2 * p:03d}", **x_spec)
            s.ask("y", y_req, f"n{2 * p + 1:03d}", **y_spec)
    n = len(s.pods)
    return s.finish(variant=variant, dims=WIDE_DIMS[variant], first=first, deciding_spec="y",
                    moved_winner_share=(pairs * 8) / n, moved_rejected_share=(pairs * 4) / n)


def _wide_ports(variant):
    """64 / 65 distinct host ports. Y wants the LAST port of the dictionary and so takes it: one Y per node. X and X2 (two specs, so
    that no neighbours share one) are bound to 20 `plain` nodes of 10 cores, whose resident pod (no requests) holds that port; Y goes
    to 45 `good` nodes of one core in name order. The list is Y X X2 Y X X2 ...: every Y passes moved plain nodes with room that
    stand in front of every empty node and are turned down by the port bit alone — four Ys in five: the fifth finds the plain
    node in use just filled — (and the good nodes that took a Y, by the same bit); the 46th Y onwards fits nothing."""
    s = _Stream()
    n_ports = 64 if variant == "kp1" else 65
    ports = [20000 + k for k in range(n_ports)]
    last = ports[-1]
    s.ask("all-ports", {"cpu": 1000}, None, ports=tuple(ports[:-1]), nodeSelector={"kind": "none"})  # (fills the dictionary, fits nothing)
    for j in range(20):
        s.node(f"p{j:02d}", {"cpu": 10000, "memory": 8 << 30}, 110, labels={"kind": "plain"},
               resident=[_pod(f"holder-{j}", {}, ports=(last,), nodeName=f"p{j:02d}")])
    for j in range(45):
        s.node(f"g{j:02d}", {"cpu": 1000, "memory": 8 << 30}, 110, labels={"kind": "good"})
    first = len(s.pods)
    ys = xs = rejected = 0
    for k in range(300):
        if k % 3 == 0:
            rejected += xs % 10 != 0  # (the plain node in use has room: it is turned down by the port bit alone)
            s.ask("y", {"cpu": 1000, "memory": 1 << 20}, f"g{ys:02d}" if ys < 45 else None, ports=(last,))
            ys += 1
        else:
            s.ask("x" if k % 3 == 1 else "x2", {"cpu": 1000, "memory": (1 << 20) + k % 3}, f"p{xs // 10:02d}", nodeSelector={"kind": "plain"})
            xs += 1
    n = len(s.pods)
    return s.finish(variant=variant, dims=WIDE_DIMS[variant], first=first, deciding_spec="y", deciding_port=last,
                    moved_winner_share=(xs - 20) / n, moved_rejected_share=rejected / n)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. many_moved: more moved nodes than one load round of the bitsets covers
# ---------------------------------------------------------------------------------------------------------------------------
def many_moved(n_nodes=SLOTS_PER_LOAD + 192, n_b=300, hot=96):
    """n_nodes nodes of 4 cores, name order = index order. Phase A: one ask of 3 cores per node — ask i takes node i (every node that
    took one cannot take another; the empty ones tie and stand in name order), so node i holds SLOT i and class A has failed on
    every slot. Then n_b asks of B (1 core, fits every moved node exactly once) with one C after every fourth B (1 core, bound to
    the LAST 64 nodes by a label).
    B takes the fullest node: A also asks for 1 GiB, and 2 * hot nodes have less memory than the rest (4 GiB + rank MiB against
    8 GiB) — hot rank r even: node n_nodes - 160 + r / 2 (its slot is >= 32 768 at full size), r odd: node 200 + r / 2 (< 512).
    The B asks behind them tie on the other nodes and take them in name order. Nodes 5, 300, n_nodes - 180 and n_nodes - 170 have
    ONE pod slot (dead after A: B skips them), hot ranks 0 .. 3 have two (dead after B). C k takes node n_nodes - 64 + k; 64 fit."""
    assert n_nodes >= 600 and 2 * hot + 8 <= n_b
    hot_of = {}
    for r in range(2 * hot):
        hot_of[(n_nodes - 160 + r // 2) if r % 2 == 0 else (200 + r // 2)] = r
    one_slot = {5, 300, n_nodes - 180, n_nodes - 170}
    rank_node = {r: n for n, r in hot_of.items()}
    two_slots = {rank_node[r] for r in range(4)}
    width = len(str(n_nodes - 1))
    nodes = []
    for i in range(n_nodes):
        mem = (4 << 30) + (hot_of[i] << 20) if i in hot_of else 8 << 30
        labels = {"tail": "yes"} if i >= n_nodes - 64 else {}
        nodes.append(_node(f"m{i:0{width}d}", {"cpu": 4000, "memory": mem}, 1 if i in one_slot else 2 if i in two_slots else 110, labels=labels))
    pods, expect, spec_of = [], [], []

    def ask(spec, req, node, **kw):
        pods.append(_pod(f"ask-{len(pods):06d}", req, **kw))
        expect.append(node)
        spec_of.append(spec)

    for i in range(n_nodes):
        ask("a", {"cpu": 3000, "memory": 1 << 30}, i)
    cold = (i for i in range(n_nodes) if i not in hot_of and i not in one_slot)
    n_c = 0
    for k in range(n_b):
        ask("b", {"cpu": 1000}, rank_node[k] if k < 2 * hot else next(cold))
        if k % 4 == 3:
            ask("c", {"cpu": 1000}, n_nodes - 64 + n_c if n_c < 64 else -1, nodeSelector={"tail": "yes"})
            n_c += 1
    assert n_c > 64 and max(e for e, sp in zip(expect, spec_of) if sp == "b" and e not in hot_of) < n_nodes - 64
    meta = dict(expect=expect, spec_of=spec_of, n_nodes=n_nodes, first_bc=n_nodes, one_slot=sorted(one_slot), two_slots=sorted(two_slots),
                hot=hot_of)
    return {"nodes": nodes, "pods": pods}, meta


# ---------------------------------------------------------------------------------------------------------------------------
# 4. batched_cut: where the replay of a batch has to stop
# ---------------------------------------------------------------------------------------------------------------------------
PROP_K = 8           # candidates per ask and shard (kPropK)
BATCH_MAX = 256      # asks per batch (kShardBatchMax)


def batched_cut():
    """12 nodes of 2 cores, 14 asks of 2 cores and 14 DISTINCT specs (a byte of memory apart: no run applies). Every ask fills its
    node, all rank the same candidates (empty nodes in name order): ask j takes node j, asks 12 and 13 fit nothing. Proposed
    together, every ask lists nodes 0 .. 7: from ask 8 on all PROP_K entries are accepted and full and the lists were cut."""
    s = _Stream()
    for j in range(12):
        s.node(f"c{j:02d}", {"cpu": 2000, "memory": 8 << 30}, 110)
    for j in range(14):
        s.ask(f"s{j}", {"cpu": 2000, "memory": (1 << 20) + j}, f"c{j:02d}" if j < 12 else None)
    return s.finish(full_in_front=[min(j, 12) for j in range(14)])


def batched_lists(n_asks):
    """40 nodes of 2 cores, asks of 100 m: 20 per node, node after node, whatever the spec (two specs a byte of memory apart
    alternate). Asks 250 .. 262 are a run of a third spec across position BATCH_MAX; ask 110 wants a host port and stands directly
    behind accepted pods on the node it takes."""
    s = _Stream()
    for j in range(40):
        s.node(f"b{j:02d}", {"cpu": 2000, "memory": 8 << 30}, 110)
    for i in range(n_asks):
        node = f"b{i // 20:02d}"
        if i == 110:
            s.ask("port", {"cpu": 100, "memory": (1 << 20) + 3}, node, ports=(8080,))
        elif 250 <= i <= 262:
            s.ask("run", {"cpu": 100, "memory": (1 << 20) + 2}, node)
        else:
            s.ask(f"alt{i % 2}", {"cpu": 100, "memory": (1 << 20) + i % 2}, node)
    return s.finish(run=(250, min(263, n_asks)), port_ask=110)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. delta_limit: histogram cells one assumed pod moves
# ---------------------------------------------------------------------------------------------------------------------------
DELTA_MAX = 10   # cells per delta record of a sharded round (kDeltaMax)
DELTA_NODES = 192  # the cluster of the two-rank case: shards are cut at multiples of 64 nodes (128 + 64), 30 nodes would leave rank 1 empty


def many_constraints(n_constraints, n_nodes=30, n_asks=150, extra_label=None):
    """n_constraints templates spread over three zones by the SAME selector (app = shared) with n_constraints different maxSkew
    values: an assumed pod with that label adds to one cell of every one of them, and their minima rise in the same assume.
    extra_label: one further template whose constraint selects (app = shared, extra = yes) — pods carrying both labels add to
    n_constraints + 1 cells; they come LAST in the list (meta["extra_from"]), and asks without the app label behind them
    (meta["plain_from"]) add to none."""
    nodes = [_node(f"z{i:03d}", {"cpu": 8000, "memory": 16 << 30}, 12, labels={"zone": "abc"[i % 3], "kubernetes.io/hostname": f"z{i:03d}"})
             for i in range(n_nodes)]

    def spread(skew, sel):
        return [{"maxSkew": skew, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule", "labelSelector": {"matchLabels": sel}}]

    pods = []
    for k in range(n_asks):
        t = k % n_constraints
        pods.append(_pod(f"ask-{k:04d}", {"cpu": 250, "memory": 256 << 20}, labels={"app": "shared", "tier": f"x{t}"},
                         topologySpreadConstraints=spread(1 + t, {"app": "shared"})))
    meta = {"cells": n_constraints, "extra_from": len(pods), "plain_from": len(pods)}
    if extra_label:
        for k in range(12):
            pods.append(_pod(f"extra-{k:02d}", {"cpu": 250, "memory": 256 << 20}, labels={"app": "shared", "extra": "yes"},
                             topologySpreadConstraints=spread(n_constraints + 1, {"app": "shared", "extra": "yes"})))
        meta["plain_from"] = len(pods)
        for k in range(40):
            # (no constraint of their own: the engine keeps a constraint row per spec that carries one, and a row that counted
            # app = shared would be an eleventh cell for every pod of the first group)
            pods.append(_pod(f"plain-{k:02d}", {"cpu": 250, "memory": (256 << 20) + k % 2}, labels={"app": "other"}))
    return {"nodes": nodes, "pods": pods}, meta
