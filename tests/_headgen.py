"""Designed clusters for the headroom question — how many copies of an ask a node still takes — with a model over Python ints.

Pure Python, no randomness: every node's free value in every dimension is CONSTRUCTED from the main template's request so that the
integer quotient sits at its boundaries (free = k·req exactly, k·req − 1, k·req + 1), the pod slots lie below every quotient, on the
smallest one (the resource is then the binder), at 0 or far above, and a few nodes carry free memory beside 2^53 and up to 2^63 − 1
(where a float64 quotient is off by one and only the slots bind small requests).

designed() → (snapshot, meta): the snapshot is what load_snapshot and the oracle are both given; meta["nodes"][i] and
meta["templates"][j] say what the generator intended in exact integers, model(meta, j) → per-node (replicas, binder cell) from them
alone, expected_cells(meta, j) → the 16 cells. clones(snapshot, j, count) → the same nodes with `count` copies of ask j as the only
pending pods: the reference's own sequential loop over them fills every node until nothing fits.
"""
import copy

RES = ["cpu", "memory", "ephemeral-storage", "example.com/foo"]  # dimension r of the engine: the three base resources, then scalars
MAIN_REQ = {"cpu": 250, "memory": 1 << 30, "ephemeral-storage": 3_000_000_000, "example.com/foo": 2}  # cpu in milli, the rest in units
RESIDENT = {"cpu": 500, "memory": 1 << 28, "ephemeral-storage": 1000, "example.com/foo": 1}
CELLS = 16
SLOTS, PORT, RES0 = 4, 5, 8
N_DESIGNED = 192
PERIOD = N_DESIGNED + 8
BIG = 1 << 53
EDGE = (1 << 60) + 1
# free memory of the last eight nodes: both sides of 2^53, multiples of 2^53 + 1 and of 2^60 + 1 and one below them, 2^63 − 1
HUGE_MEM = [BIG - 1, BIG, BIG + 1, 5 * (BIG + 1) - 1, 5 * (BIG + 1), (1 << 63) - 1, 7 * EDGE, 7 * EDGE - 1]
HUGE_SLOTS = [9, 16, 3, 12, 4, 20, 6, 11]
TAINT_A = {"key": "dedicated", "value": "a", "effect": "NoSchedule"}
TOL_A = {"key": "dedicated", "operator": "Equal", "value": "a", "effect": "NoSchedule"}


def _qty(res, v):
    return f"{v}m" if res == "cpu" else str(v)


def _node(i):
    """→ (node JSON, what it means: free per resource, free slots, zone, tainted, unschedulable, port 8080 taken)."""
    name = f"hn{i:04d}"
    index, i = i, i % PERIOD  # (clusters past PERIOD nodes repeat the design under new names)
    zone = f"z{(i // 64) % 3}" if i < N_DESIGNED else "z0"
    tainted = 64 <= i < 128  # one whole word of nodes
    info = {"name": name, "zone": zone, "tainted": tainted, "unsched": i == 5, "port_busy": i % 10 == 7}
    resident = dict(RESIDENT)
    if i < N_DESIGNED:
        k, d, delta = (i * 7) % 13, i % 4, (0, -1, 1)[(i // 4) % 3]
        free = {}
        for e, res in enumerate(RES):
            q = MAIN_REQ[res]
            free[res] = k * q + delta if e == d else (k + 2 + i % 3) * q + i % 7
        quotients = [free[res] // MAIN_REQ[res] if free[res] >= 0 else -1 for res in RES]
        qmin = max(min(quotients), 0)
        slots = (20, 20, max(qmin - 1, 0), qmin, 0)[(i // 12) % 5]  # far above | below every quotient | on the smallest one | none
    else:
        h = i - N_DESIGNED
        free = {"cpu": 1_000_000 + h, "memory": HUGE_MEM[h], "ephemeral-storage": (1 << 62) + h, "example.com/foo": 40}
        resident.pop("memory")  # (allocatable = free: nothing can be added to 2^63 − 1)
        slots = HUGE_SLOTS[h]
    info["free"], info["slots"] = free, slots
    alloc = {res: _qty(res, free[res] + resident.get(res, 0)) for res in RES}
    alloc["pods"] = str(slots + 1)  # (the resident pod holds one)
    container = {"name": "c", "resources": {"requests": {res: _qty(res, v) for res, v in resident.items()}}}
    if info["port_busy"]:
        container["ports"] = [{"hostPort": 8080, "containerPort": 8080, "protocol": "TCP"}]
    node = {"metadata": {"name": name, "labels": {"zone": zone, "kubernetes.io/hostname": name}},
            "spec": {"taints": [TAINT_A] if tainted else [], "unschedulable": info["unsched"]},
            "status": {"allocatable": alloc},
            "pods": [{"metadata": {"name": f"res-{index}", "uid": f"res-{index}", "namespace": "default", "labels": {"app": "res"}},
                      "spec": {"containers": [container]}}]}
    return node, info


def _ask(uid, req, tolerate=False, zone=None, pin=None, port=False, pvc=False, spread=False):
    """→ (pod JSON, what it means)."""
    container = {"name": "main", "resources": {"requests": {res: _qty(res, v) for res, v in req.items()}}}
    if port:
        container["ports"] = [{"hostPort": 8080, "containerPort": 8080, "protocol": "TCP"}]
    spec = {"containers": [container]}
    if tolerate:
        spec["tolerations"] = [TOL_A]
    if zone:
        spec["nodeSelector"] = {"zone": zone}
    if pin:
        spec["nodeName"] = pin
    if pvc:
        spec["volumes"] = [{"name": "data", "persistentVolumeClaim": {"claimName": "pvc-1"}}]
    if spread:
        spec["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": "zone", "whenUnsatisfiable": "DoNotSchedule",
                                              "labelSelector": {"matchLabels": {"app": "ask"}}}]
    pod = {"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": {"app": "ask"}}, "spec": spec}
    info = {"uid": uid, "req": dict(req), "tolerate": tolerate, "zone": zone, "pin": pin, "port": port,
            "status": 1 if pvc else 2 if spread else 0}
    return pod, info


def designed(n_nodes=PERIOD, extra=0):
    """`extra` further asks with request vectors of their own (distinct tasks for the kernel's task chunks)."""
    built = [_node(i) for i in range(n_nodes)]
    asks = [
        _ask("t-main", MAIN_REQ),
        _ask("t-zero", {}),                                              # all-zero requests: only the slots bound it
        _ask("t-port", {"cpu": 300, "memory": 1 << 29}, port=True),      # k0 > 1 on most nodes, cut to 1 by its own host port
        _ask("t-pin", {"cpu": 200}, pin=built[min(9, n_nodes - 1)][1]["name"]),
        _ask("t-z2", {"cpu": 400, "memory": 3 << 29}, zone="z2"),        # a selector that excludes whole words of nodes
        _ask("t-tol-z1", MAIN_REQ, tolerate=True, zone="z1"),            # ... and the tainted word alone
        _ask("t-big", {"cpu": 1, "memory": BIG + 1}),                    # quotients of values a float64 cannot hold
        _ask("t-edge", {"memory": EDGE}),
        _ask("t-tiny", {"cpu": 1, "memory": 1}),                         # quotients up to 2^63 − 1: the slots bind
        _ask("t-cpu", {"cpu": 400}, tolerate=True),
        _ask("t-foo", {"example.com/foo": 1}),
        _ask("t-eph", {"ephemeral-storage": 7_000_000_001, "cpu": 50}),
        _ask("t-routed", MAIN_REQ, pvc=True),                            # not evaluated by the engine
        _ask("t-spread", {"cpu": 250}, spread=True),                     # a hard spread constraint: copies interact across nodes
    ]
    for c in range(extra):
        req = {"cpu": 60 + 37 * c}
        if c % 2:
            req["memory"] = (3 + c) << 27
        if c % 5 == 0:
            req["example.com/foo"] = 1 + c % 3
        asks.append(_ask(f"t-x{c}", req, tolerate=c % 3 == 0, zone=(None, None, "z0", "z1")[c % 4], port=c % 11 == 10))
    snapshot = {"nodes": [b[0] for b in built], "pods": [a[0] for a in asks]}
    return snapshot, {"nodes": [b[1] for b in built], "templates": [a[1] for a in asks]}


def replicas(node, tmpl):
    """The rule in Python ints → (replicas, binder cell or None)."""
    if node["unsched"] or (node["tainted"] and not tmpl["tolerate"]) or (tmpl["zone"] and tmpl["zone"] != node["zone"]):
        return 0, None
    if tmpl["pin"] and tmpl["pin"] != node["name"]:
        return 0, None
    if tmpl["port"] and node["port_busy"]:
        return 0, None
    if node["slots"] < 1:
        return 0, None
    k0, binder = node["slots"], SLOTS
    quotients = []
    for r, res in enumerate(RES):
        q = tmpl["req"].get(res, 0)
        if q > 0:
            if node["free"][res] < q:
                return 0, None
            quotients.append((node["free"][res] // q, r))
    if quotients and min(quotients)[0] <= k0:
        k0, binder = min(quotients)[0], RES0 + min(quotients)[1]  # (the lowest r among equal quotients: tuples compare r next)
    if tmpl["port"] and k0 > 1:
        return 1, PORT
    return k0, binder


def model(meta, j):
    return [replicas(node, meta["templates"][j]) for node in meta["nodes"]]


def expected_cells(meta, j):
    tmpl = meta["templates"][j]
    cells = [0] * CELLS
    cells[3] = tmpl["status"]
    if tmpl["status"]:
        return cells  # (a coupled ask's [0], [1], [2] are not the model's to say)
    per_node = model(meta, j)
    cells[0] = sum(k for k, _ in per_node)
    cells[1] = sum(1 for k, _ in per_node if k >= 1)
    cells[2] = max([k for k, _ in per_node] + [0])
    for k, binder in per_node:
        if k >= 1:
            cells[binder] += 1
    return cells


def clones(snapshot, j, count):
    """The same nodes, and `count` copies of ask j — distinct name and uid — as the only pending pods."""
    pods = []
    for c in range(count):
        pod = copy.deepcopy(snapshot["pods"][j])
        pod["metadata"]["name"] = pod["metadata"]["uid"] = f"{snapshot['pods'][j]['metadata']['uid']}-copy-{c}"
        pods.append(pod)
    return {"nodes": snapshot["nodes"], "pods": pods}


_CLONE_LOOPS = {}


def clone_loop(n_nodes=PERIOD):
    """→ {template index: np.int64[n_nodes]}: per node how many of Σ model + 3 copies the oracle's sequential allocation loop (the
    reference's node loop + AssumePod) put there, for every template of designed(n_nodes) the engine computes (status 0). The loop
    fills a node until nothing fits and never gets past the model's total: exactly 3 copies stay unplaced. Computed once per process."""
    import numpy as np

    import _oracle as orc
    if n_nodes not in _CLONE_LOOPS:
        snapshot, meta = designed(n_nodes)
        out = {}
        for j, tmpl in enumerate(meta["templates"]):
            if tmpl["status"]:
                continue
            total = sum(k for k, _ in model(meta, j))
            placed = orc.Oracle(clones(snapshot, j, total + 3)).allocate_sequential()
            assert int((placed < 0).sum()) == 3, (tmpl["uid"], total, int((placed < 0).sum()))
            out[j] = np.bincount(placed[placed >= 0], minlength=n_nodes).astype(np.int64)
        _CLONE_LOOPS[n_nodes] = out
    return _CLONE_LOOPS[n_nodes]
