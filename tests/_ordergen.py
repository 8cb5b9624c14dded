"""Designed clusters (Kubernetes-JSON snapshots) for the bin-pack ORDER: whole permutations, not first feasible nodes.

Pure Python, `random.Random(seed)` only, used only by tests, in the style of `_advgen.py`. Every quantity is a plain integer
("<n>m" of cpu, bytes of memory) so that meta["usage"][i] = (total_cpu, total_mem, used_cpu, used_mem) of node i is exact and a
test can restate the score in Python floats. Populations (each a list of such tuples, laid out by `cluster`):

  ties       most nodes idle and identical (score 1.0: the clamped last bucket), a group of identical half-used nodes
  dense      >= 1100 pairwise distinct scores inside ONE rank bucket (total 2^30, used 2^29 + i), plus a block of idle nodes
  edges      scores exactly on a bucket boundary (totals 1024, used u) and 2^-40 on either side (totals 2^40)
  signs      overcommitted nodes (negative scores, two of them tied), score 0.0, allocatable cpu / memory / both 0
  int64      memory totals 2^62 and 2^63 - 1 with used 2^53 and 2^53 +- 1: distinct integers, one double
  mixed      all of them in one cluster, shuffled

Node names are ASCII and follow neither index order nor its reverse (`node_names`). `cluster` returns (snapshot, meta).
"""
import random

I64_MAX = (1 << 63) - 1
IDLE = (16000, 1 << 34, 0, 0)
HALF = (16000, 1 << 34, 8000, 1 << 33)
POOLS = ("a", "a", "a", "a", "b", "b", "c")   # the label that splits the nodes unevenly
TOL_X = {"key": "dedicated", "operator": "Equal", "value": "x", "effect": "NoSchedule"}
TOL_ALL = {"operator": "Exists"}


def node_names(n):
    """n distinct names, unpadded numbers (node-9 / node-10) and prefix pairs (n1, n10, n1-a). Node i gets the name of rank
    r(i) in byte order, r = the reverse of the index order with the middle two of every four swapped: of the pairs (i, i + 1)
    three in four are inverted, and the order is neither the index order nor its reverse."""
    pool = sorted((("node-%d", "n%d", "n%d-a")[k % 3] % (k // 3 + 1)).encode() for k in range(n))
    out = []
    for i in range(n):
        j = i ^ 3 if i % 4 in (1, 2) and (i | 3) < n else i
        out.append(pool[n - 1 - j].decode())
    return out


# ---- populations: lists of (total_cpu, total_mem, used_cpu, used_mem) ------------------------------------------------
def ties(rng, n):
    out = []
    for k in range(n):
        r = k % 20
        if r < 17:
            out.append(IDLE)
        elif r < 19:
            out.append(HALF)
        else:
            out.append((16000, 1 << 34, rng.randrange(1, 16000), rng.randrange(1, 1 << 34)))
    return out


def dense(rng, n, distinct=None):
    """`distinct` nodes (default: half of n >= 2200) with pairwise distinct scores 0.5 - i / 2^30 (i >= 1: all in bucket 511), the
    rest idle."""
    if distinct is None:
        if n < 2200:
            raise ValueError("the dense population needs 2200 nodes: 1100 distinct keys and a multi-tile block of idle nodes")
        distinct = n // 2
    steps = rng.sample(range(1, 1 << 20), distinct)   # distinct, not consecutive: 0.5 - i / 2^30 is exact for every one of them
    return [(1 << 30, 1 << 30, (1 << 29) + i, (1 << 29) + i) for i in steps] + [IDLE] * (n - distinct)


def edges(rng, n):
    out = [(1024, 1024, 0, 0), (1024, 1024, 1024, 1024)]
    k = 0
    while len(out) < n:
        if k % 2 == 0:
            u = (k * 37 + 5) % 1025
            out.append((1024, 1024, u, u))
        else:
            j = 1 + (k * 13) % 1022
            u = (j << 30) + (k // 2) % 3 - 1
            out.append((1 << 40, 1 << 40, u, u))
        k += 1
    return out[:n]


SIGNS = [
    (1000, 1 << 30, 1500, (1 << 30) + (1 << 29)),     # -0.5
    (1000, 1 << 30, 3000, 1 << 31),                   # -1.5
    (4000, 1 << 32, 4100, (1 << 32) + 12345),         # a little below zero
    (2000, 1 << 31, 2500, (1 << 31) + (1 << 29)),     # -0.25 ...
    (2000, 1 << 31, 2500, (1 << 31) + (1 << 29)),     # ... twice: a negative tie
    (1000, 1 << 30, 1000, 1 << 30),                   # exactly 0.0
    (0, 1 << 30, 0, 1 << 28),                         # cpu: "0", memory in use: scored from memory alone
    (0, 1 << 30, 500, 1 << 29),                       # ... with a resident cpu request on top
    (4000, 0, 1000, 0),                               # memory 0, cpu in use
    (4000, 0, 1000, 1 << 20),
    (0, 0, 0, 0),                                     # both 0: score 1.0
    (0, 0, 100, 100),
    (1000, 1 << 30, 2000, 0),                         # cpu overcommitted, memory idle: 0.0 again, by another route
    (1000, 1 << 30, 3000, 0),                         # -0.5 again: ties with the first node on different usage
    (1000, 1 << 30, 0, 1 << 31),
]


def signs(rng, n):
    if n < len(SIGNS) + 8:
        raise ValueError("too few nodes for the signs-and-zeros population")
    out = list(SIGNS)
    while len(out) < n:   # ordinary nodes on a coarse grid (they tie among themselves), a few idle
        q = rng.randrange(9)
        out.append((8000, 1 << 33, 1000 * q, (1 << 30) * rng.randrange(9)) if q else IDLE)
    return out


def int64(rng, n):
    combos = [(t, u) for t in (1 << 62, I64_MAX) for u in ((1 << 53) - 1, 1 << 53, (1 << 53) + 1)]
    combos += [(1 << 54, (1 << 53) - 1), (1 << 54, 1 << 53), (1 << 54, (1 << 53) + 1), ((1 << 53) + 1, 1), ((1 << 53) + 2, 2)]
    cpus = [(1000, 0), (0, 0), (1000, 500), (1000, 0)]
    return [(cpus[(k // len(combos)) % 4][0], combos[k % len(combos)][0], cpus[(k // len(combos)) % 4][1], combos[k % len(combos)][1])
            for k in range(n)]


def mixed(rng, n):
    """All populations in one cluster: a quarter of the nodes are the dense part (1100 from 2500 nodes on), the rest of the room
    goes to the ties."""
    if n < 200:
        raise ValueError("too few nodes for the mixed population")
    out = signs(rng, len(SIGNS) + 8) + int64(rng, 24) + edges(rng, min(n // 10, 130))
    assert len(out) == pairs_at(n)
    out += PAIRS
    d = 1100 if n >= 2500 else n // 4
    out += dense(rng, d, distinct=d)
    return out + ties(rng, n - len(out))


# designed pairs of the node-change sequence (mixed only): an ask of MOVE_EQ units moves PAIRS[0] exactly onto the score of
# PAIRS[1]; an ask of MOVE_BUCKET units moves PAIRS[2] from 2^-40 above a bucket boundary to 2^-40 below it. Their totals
# (2048, 2^41) are no other population's, so no other node has their usage; `cluster` finds them by position all the same.
MOVE_EQ, MOVE_BUCKET = 4, 2
PAIRS = [(2048, 2048, 602, 602), (2048, 2048, 606, 606), (1 << 41, 1 << 41, (417 << 31) - 1, (417 << 31) - 1)]


def pairs_at(n):
    """Index of PAIRS[0] in mixed(rng, n), before `cluster` shuffles the nodes."""
    return len(SIGNS) + 8 + 24 + min(n // 10, 130)


POPULATIONS = {"ties": ties, "dense": dense, "edges": edges, "signs": signs, "int64": int64, "mixed": mixed}


# ---- snapshot ----------------------------------------------------------------------------------------------------------
def make_node(name, usage, pool="a", zone="z0", tainted=False, disk=False, slots=110):
    tc, tm, uc, um = usage
    labels = {"pool": pool, "zone": zone, "kubernetes.io/hostname": name}
    if disk:
        labels["disk"] = "ssd"
    if tainted:
        labels["ded"] = "x"
    node = {"metadata": {"name": name, "labels": labels},
            "spec": {"taints": [{"key": "dedicated", "value": "x", "effect": "NoSchedule"}] if tainted else []},
            "status": {"allocatable": {"cpu": f"{tc}m" if tc else "0", "memory": str(tm), "pods": str(slots)}}, "pods": []}
    if uc or um:
        req = {}
        if uc:
            req["cpu"] = f"{uc}m"
        if um:
            req["memory"] = str(um)
        node["pods"].append({"metadata": {"name": f"res-{name}", "uid": f"res-{name}", "namespace": "default", "labels": {"app": "res"}},
                             "spec": {"containers": [{"name": "c", "resources": {"requests": req}}]}})
    return node


def make_ask(uid, cpu=None, mem=None, selector=None, tolerations=None, pin=None, labels=None, containers=True, spread=None):
    req = {}
    if cpu is not None:
        req["cpu"] = f"{cpu}m" if cpu else "0"
    if mem is not None:
        req["memory"] = str(mem)
    spec = {"containers": [{"name": "main", "resources": {"requests": req}}] if containers else []}
    if selector:
        spec["nodeSelector"] = selector
    if tolerations:
        spec["tolerations"] = tolerations
    if pin is not None:
        spec["nodeName"] = pin
    if spread:
        spec["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule",
                                              "labelSelector": {"matchLabels": {"app": spread}}}]
    return {"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": labels or {"app": "ask"}}, "spec": spec}


def _cuts(free, count):
    """`count` request values that cut the nodes by free capacity: order statistics of the positive free values, alternately
    exact (free == request fits) and one above (misses by one)."""
    pos = sorted({f for f in free if f > 0})
    if not pos:
        return [1] * count
    out = []
    for k in range(count):
        v = pos[min(len(pos) - 1, (k * len(pos)) // count)]
        out.append(min(v + k % 2, I64_MAX))
    return out


def make_asks(rng, names, usage, topology=False):
    """About 40 asks. meta keys of note: fits_all, infeasible, pinned (uids)."""
    free_cpu = [u[0] - u[2] for u in usage]
    free_mem = [u[1] - u[3] for u in usage]
    mover = {"app": "mover"} if topology else None
    asks = [make_ask("fits-all", tolerations=[TOL_ALL], containers=False),
            make_ask("nowhere", cpu=1, selector={"pool": "nowhere"}),
            make_ask("pinned", pin=names[len(names) // 2], tolerations=[TOL_ALL]),
            make_ask("move-eq", cpu=MOVE_EQ, mem=MOVE_EQ, labels=mover),
            make_ask("move-bucket", cpu=MOVE_BUCKET, mem=MOVE_BUCKET, labels=mover)]
    for pool in ("a", "b", "c"):
        asks.append(make_ask(f"pool-{pool}", selector={"pool": pool}))
        asks.append(make_ask(f"pool-{pool}-tol", cpu=1, selector={"pool": pool}, tolerations=[TOL_X]))
    asks.append(make_ask("ssd", selector={"disk": "ssd"}, tolerations=[TOL_ALL]))
    for k in range(3):
        asks.append(make_ask(f"ded-{k}", cpu=k or None, selector={"ded": "x"}, tolerations=[TOL_X]))
    asks.append(make_ask("ded-untolerated", selector={"ded": "x"}))
    cpus, mems = _cuts(free_cpu, 8), _cuts(free_mem, 8)
    for k in range(8):
        asks.append(make_ask(f"cpu-{k}", cpu=cpus[k], tolerations=[TOL_ALL]))
        asks.append(make_ask(f"mem-{k}", cpu=0, mem=mems[k], tolerations=[TOL_ALL]))   # zero cpu, some memory
        if k % 2:
            asks.append(make_ask(f"both-{k}", cpu=cpus[(k * 3) % 8], mem=mems[k], selector={"pool": "a"}))
    if topology:
        asks.append(make_ask("spread-0", cpu=1, labels={"app": "mover"}, spread="mover"))
        asks.append(make_ask("spread-1", mem=1, labels={"app": "mover"}, spread="mover", tolerations=[TOL_ALL]))
    rng.shuffle(asks)
    return asks


def cluster(population, seed, n, topology=False):
    """(snapshot, meta). meta: usage[i], names[i], designed[i] (True: neither IDLE nor HALF), pairs (indices of the PAIRS nodes,
    mixed only). One node in seven is tainted, designed ones too (a taint does not change a score), so that the toleration-gated
    asks (ded-*, pool-*-tol) have nodes on every population; only the PAIRS nodes are not: their asks carry no toleration."""
    rng = random.Random(f"{population}-{seed}-{n}")
    usage = POPULATIONS[population](rng, n)
    assert len(usage) == n
    designed = [u not in (IDLE, HALF) for u in usage]
    order = list(range(n))
    rng.shuffle(order)
    usage = [usage[k] for k in order]
    designed = [designed[k] for k in order]
    names = node_names(n)
    pairs = [order.index(pairs_at(n) + k) for k in range(len(PAIRS))] if population == "mixed" else []
    nodes = []
    for i in range(n):
        tainted = i not in pairs and rng.random() < 1 / 7
        nodes.append(make_node(names[i], usage[i], pool=POOLS[rng.randrange(len(POOLS))], zone=f"z{rng.randrange(3)}", tainted=tainted,
                               disk=rng.random() < 0.1))
    meta = {"usage": usage, "names": names, "designed": designed, "population": population}
    if population == "mixed":
        meta["pairs"] = pairs
        assert [usage[i] for i in pairs] == PAIRS
    return {"nodes": nodes, "pods": make_asks(rng, names, usage, topology)}, meta


# ---- rounds ------------------------------------------------------------------------------------------------------------
def round_ties(seed, n_nodes=200, n_asks=500):
    """Round cluster (i): totals 1024 / 1024, asks of 1 / 1, 2 / 2 and 4 / 4 units, staggered initial usage a few units below
    full, 3 to 6 pod slots. A node that cannot take a 4-unit ask waits unmoved while a moved node is filled up to exactly its
    usage: the next smaller ask finds the minimal key shared by a moved and an unmoved node. meta: usage, names, slots."""
    rng = random.Random(f"round-ties-{seed}")
    names = node_names(n_nodes)
    usage, slots, nodes = [], [], []
    for i in range(n_nodes):
        u = 1024 - rng.choice([1, 2, 3, 3, 5, 6, 7, 7, 9, 10, 11, 13])
        s = rng.choice([3, 4, 5, 6])
        usage.append((1024, 1024, u, u))
        slots.append(s)
        nodes.append(make_node(names[i], usage[i], slots=s))
    sizes = [rng.choice([1, 1, 2, 2, 4]) for _ in range(n_asks)]
    pods = [make_ask(f"ask-{k}", cpu=v, mem=v) for k, v in enumerate(sizes)]
    return {"nodes": nodes, "pods": pods}, {"usage": usage, "names": names, "slots": slots, "sizes": sizes}


def round_signs(seed, n_nodes=200, n_asks=500):
    """Round cluster (ii): the signs-and-zeros nodes among ordinary ones, 2 to 5 pod slots; asks that request zero cpu and some
    memory, asks that request nothing, and a few ordinary ones: overcommitted and zero-allocatable nodes take pods."""
    rng = random.Random(f"round-signs-{seed}")
    names = node_names(n_nodes)
    usage = signs(rng, n_nodes)
    rng.shuffle(usage)
    slots = [rng.choice([2, 3, 4, 5]) for _ in range(n_nodes)]
    nodes = [make_node(names[i], usage[i], slots=slots[i]) for i in range(n_nodes)]
    pods = []
    for k in range(n_asks):
        r = k % 5
        if r < 2:
            pods.append(make_ask(f"ask-{k}"))
        elif r < 4:
            pods.append(make_ask(f"ask-{k}", cpu=0, mem=rng.choice([1 << 20, 1 << 28, 1 << 30])))
        else:
            pods.append(make_ask(f"ask-{k}", cpu=rng.choice([100, 500]), mem=1 << 28))
    return {"nodes": nodes, "pods": pods}, {"usage": usage, "names": names, "slots": slots}


# ---- the score contract, restated ------------------------------------------------------------------------------------------
RANK_BUCKETS = 1024


def score(usage):
    """The bin-pack score in plain Python floats, in the operation order of the contract: per dimension with total > 0,
    share = 1 - float(total - used) / float(total); score = 1 - (sum of shares) / (number of such dimensions); 1.0 without one."""
    tc, tm, uc, um = usage
    total, count = 0.0, 0.0
    for t, u in ((tc, uc), (tm, um)):
        if t <= 0:
            continue
        share = 1.0 - float(t - u) / float(t)
        total = total + share
        count = count + 1.0
    if count == 0.0:
        return 1.0
    return 1.0 - total / count


def bucket(s):
    """The rank bucket of a score: 1024 equal bins of [0, 1], clamped at both ends."""
    x = s * float(RANK_BUCKETS)
    if x >= float(RANK_BUCKETS - 1):
        return RANK_BUCKETS - 1
    return int(x) if x > 0.0 else 0


def replay_round(meta):
    """Round cluster (i) replayed in plain Python: feasible = free >= request and a pod slot left, winner = minimum (score, name).
    → (node per ask, steps whose minimal key a moved and an unmoved feasible node share, how often the moved / the unmoved one
    won by its name)."""
    n = len(meta["usage"])
    used = [u[2] for u in meta["usage"]]
    left = [s - 1 for s in meta["slots"]]   # every node starts with one resident pod
    names = [x.encode() for x in meta["names"]]
    moved = [False] * n
    out, shared, moved_won, unmoved_won = [], 0, 0, 0
    for size in meta["sizes"]:
        best, tie = None, []
        for i in range(n):
            if 1024 - used[i] < size or left[i] <= 0:
                continue
            s = score((1024, 1024, used[i], used[i]))
            if best is None or s < best:
                best, tie = s, [i]
            elif s == best:
                tie.append(i)
        if best is None:
            out.append(-1)
            continue
        w = min(tie, key=lambda i: names[i])
        if any(moved[i] for i in tie) and not all(moved[i] for i in tie):
            shared += 1
            moved_won += moved[w]
            unmoved_won += not moved[w]
        out.append(w)
        used[w] += size
        left[w] -= 1
        moved[w] = True
    return out, shared, moved_won, unmoved_won
