"""Structured, seeded clusters (Kubernetes-JSON snapshots) built to meet the row writers where they special-case.

Independent of the product's KWOK generator and of `_gen.py`'s palettes: pure Python, `random.Random(seed)` only, used only by
tests. Where `_gen` draws everything at random at sizes of a few hundred asks, the populations here are DESIGNED at the sizes
where the writers differ (rows of several word groups, runs of hundreds of rows, several bands):

  sweep(...)           one walked dimension (cpu), free values constructed per 64-node word
  two_dims(...)        cpu and memory walked, a third many-valued dimension on ballot planes, values at the int64 edges
  own_templates(...)   no walked dimension: a few signatures with thousands of asks, hundreds with a selector of their own
  uneven_classes(...)  templates with very uneven member counts (the band layout of zone A)

Each returns (snapshot, meta): the snapshot is what `load_snapshot` and the oracle are both given; meta says what the generator
intended (word kinds, the run / template of every ask) so that a test can assert the property and name a failing bit's origin.
"""
import random

I64_MAX = (1 << 63) - 1
GI = 1 << 30
WORD_KINDS = ("tied", "consecutive", "uniform", "extremes", "off-by-one", "isolated-mid", "isolated-low")
# the kinds by word, cycling: the kinds whose nodes all differ come up more often, so that most request values meet a node
WORD_CYCLE = ("tied", "consecutive", "uniform", "extremes", "off-by-one", "isolated-mid", "consecutive", "off-by-one", "uniform",
              "consecutive", "off-by-one", "isolated-low")

# (tolerations, nodeSelector, node-affinity terms) of the signature families; "all" tolerates everything and selects nothing
_TOL_A = {"key": "dedicated", "operator": "Equal", "value": "a", "effect": "NoSchedule"}
_TOL_B = {"key": "dedicated", "operator": "Equal", "value": "b", "effect": "NoSchedule"}
_TOL_DED = {"key": "dedicated", "operator": "Exists"}
_TOL_ALL = {"operator": "Exists"}


def _aff(op, values):
    return [{"matchExpressions": [{"key": "zone", "operator": op, "values": list(values)}]}]


FAMILIES = {
    "plain": ([], None, None),
    "all": ([_TOL_ALL], None, None),
    "a-z1": ([_TOL_A], {"zone": "z1"}, None),
    "ab-z02": ([_TOL_A, _TOL_B], None, _aff("In", ["z0", "z2"])),
    "ded-notiso": ([_TOL_DED], None, _aff("NotIn", ["zs", "zt"])),
    "ab": ([_TOL_A, _TOL_B], None, None),
    "b-z3": ([_TOL_B], {"zone": "z3"}, None),
    "z012": ([], None, _aff("In", ["z0", "z1", "z2"])),
    "a-notz0": ([_TOL_A], None, _aff("NotIn", ["z0"])),
    "b": ([_TOL_B], None, None),
    # the two that live on the isolated words (taint dedicated=iso): "iso-mid" sees nodes whose free values lie inside the
    # request grid (first rows = its eligibility mask, last rows empty), "iso-low" nodes below the smallest request (every
    # row of its run is empty: the run starts above the largest free value)
    "iso-mid": ([_TOL_ALL], {"zone": "zs"}, None),
    "iso-low": ([_TOL_DED], None, _aff("In", ["zt"])),
}
GENERAL = ["plain", "all", "a-z1", "ab-z02", "ded-notiso", "ab", "b-z3", "z012", "a-notz0", "b"]


def node_name(i):
    """Unpadded and padded names mixed: the string order of the NodeIDs (the decision tie-break) is not the index order."""
    return f"n{i}" if i % 3 else f"n{i:07d}"


def irregular_grid(rng, count, start, steps):
    """`count` distinct ascending values on an irregular grid."""
    out, v = [], start
    for _ in range(count):
        out.append(v)
        v += rng.choice(steps)
    return out


def design_word(rng, kind, values, occurrence=0):
    """64 free values of one word of nodes. values: the ascending request values of the dimension."""
    vmin, vmax = values[0], values[-1]
    n = len(values)
    if kind == "tied":          # one step clears the whole word; free == request fits
        return [values[rng.randrange(n)]] * 64
    if kind == "consecutive":   # every row of a run over these values clears exactly one bit of the word
        s = rng.randrange(max(n - 64, 1))
        out = [values[(s + k) % n] for k in range(64)]
        rng.shuffle(out)
        return out
    if kind == "uniform":
        return [rng.randint(0, vmax + vmax // 8 + 2) for _ in range(64)]
    if kind == "extremes":
        pool = [-rng.randint(1, 5000), -1, 0, 1, vmin - 1, vmin, vmax - 1, vmax, vmax + 1, 4 * vmax + 7]
        return [pool[(k + occurrence) % len(pool)] for k in range(64)]
    if kind == "off-by-one":
        return [values[rng.randrange(n)] + (-1, 0, 1)[k % 3] for k in range(64)]
    raise ValueError(kind)


def _resident(i, req):
    return {"metadata": {"name": f"res-{i}", "uid": f"res-{i}", "namespace": "default", "labels": {"app": "res"}},
            "spec": {"containers": [{"name": "c", "resources": {"requests": req}}]}}


def _pod(uid, family, req, node_name_pin=None):
    tol, sel, aff = FAMILIES[family]
    spec = {"containers": [{"name": "main", "resources": {"requests": req}}]}
    if tol:
        spec["tolerations"] = tol
    if sel:
        spec["nodeSelector"] = sel
    if aff:
        spec["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": aff}}}
    if node_name_pin is not None:
        spec["nodeName"] = node_name_pin
    return {"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": {"app": "ask"}}, "spec": spec}


def _cpu(m):
    return f"{m}m"


def _build_nodes(rng, n_nodes, free_cpu, free_mem, kinds, extra_alloc=None):
    """Nodes whose free cpu (milli) / memory (bytes) are the given values: allocatable − one resident pod's request.
    free_mem[i] may be a (allocatable, resident) pair of exact integers instead (the int64-edge slice)."""
    nodes = []
    for i in range(n_nodes):
        kind = kinds[i // 64]
        if kind.startswith("isolated"):
            taints = [{"key": "dedicated", "value": "iso", "effect": "NoSchedule"}]
            zone = "zs" if kind == "isolated-mid" else "zt"
        else:
            r = rng.random()
            taints = [] if r < 0.7 else [{"key": "dedicated", "value": "a" if r < 0.88 else "b", "effect": "NoSchedule"}]
            zone = f"z{rng.randrange(4)}"
        fc = free_cpu[i]
        res_cpu = rng.randint(100, 4000) if fc >= 0 else 1000 - fc
        alloc_cpu = fc + res_cpu
        fm = free_mem[i]
        if isinstance(fm, tuple):
            alloc_mem, res_mem = fm
        else:
            res_mem = rng.choice([GI, 3 * GI + 1]) if fm >= 0 else GI - fm
            alloc_mem = fm + res_mem
        alloc = {"cpu": _cpu(alloc_cpu), "memory": str(alloc_mem), "pods": "110"}
        if extra_alloc is not None:
            alloc.update(extra_alloc(rng, i))
        name = node_name(i)
        nodes.append({"metadata": {"name": name, "labels": {"zone": zone, "rack": f"r{i // 16}", "kubernetes.io/hostname": name}},
                      "spec": {"taints": taints, "unschedulable": rng.random() < 0.01},
                      "status": {"allocatable": alloc},
                      "pods": [_resident(i, {"cpu": _cpu(res_cpu), "memory": str(res_mem)})]})
    return nodes


def _word_kinds(n_nodes, with_isolated=True):
    kinds = [k for k in WORD_CYCLE if with_isolated or not k.startswith("isolated")]
    return [kinds[w % len(kinds)] for w in range((n_nodes + 63) // 64)]


def _designed_free(rng, n_nodes, kinds, values, iso_mid, shift=0):
    """Free values of every node: by word kind; of the isolated words, "mid" (zone zs) has values inside the grid and "low"
    (zone zt) values below the smallest request. `shift` rotates the kinds (a second dimension gets another phase)."""
    free, seen = [], {}
    plain = [k for k in WORD_KINDS if not k.startswith("isolated")]
    for w, kind in enumerate(kinds):
        if kind == "isolated-mid":
            word = [rng.randint(iso_mid[0], iso_mid[1]) for _ in range(64)]
        elif kind == "isolated-low":
            word = [rng.randint(values[0] - 40, values[0] - 1) for _ in range(64)]
        else:
            k = plain[(plain.index(kind) + shift * (1 + w // len(WORD_CYCLE))) % len(plain)] if shift else kind
            seen[k] = seen.get(k, 0) + 1
            word = design_word(rng, k, values, seen[k])
        free.extend(word)
    return free[:n_nodes]


def _blocks(rng, count, runs, weights, first=None, last=None):
    """Assigns value positions 0..count-1 to runs one position at a time or in contiguous blocks of 2..8 positions (so that a run
    also has stretches of consecutive values); `first` / `last`: the run that gets the lowest / highest block."""
    out = []
    while len(out) < count:
        r = rng.choices(runs, weights)[0]
        if not out and first is not None:
            r = first
        out.extend([r] * (1 if rng.random() < 0.85 else rng.randint(2, 8)))
    out = out[:count]
    if last is not None:
        for k in range(1, min(12, count) + 1):
            out[-k] = last
    return out


MEM_PALETTE = [None, GI, 15 * GI + 1, 100 * GI]   # node free memory is one of MEM_FREE: 1Gi fits exactly, or misses by one byte
MEM_FREE = [GI - 1, GI, 15 * GI, 127 * GI, 1000 * GI]


def _family_list(families):
    general = GENERAL[:max(families - 2, 1)]
    return general + ["iso-mid", "iso-low"]


def sweep(seed, nodes, asks, families=6):
    """Population (a): `asks` asks, nearly all with a cpu request of their own on an irregular grid; runs = (family, memory
    palette entry). meta: values (ascending cpu grid), word_kind[w], run_of[uid] = (family, mem index), cpu_of[uid]."""
    rng = random.Random(seed)
    fams = _family_list(families)
    n_extra = 6
    n_sweep = asks - 4 * n_extra
    values = irregular_grid(rng, n_sweep, 37, [1, 1, 2, 3, 5, 8, 13, 40])
    kinds = _word_kinds(nodes)
    free_cpu = _designed_free(rng, nodes, kinds, values, (values[n_sweep // 4], values[3 * n_sweep // 4]))
    free_mem = [rng.choice(MEM_FREE) for _ in range(nodes)]
    node_list = _build_nodes(rng, nodes, free_cpu, free_mem, kinds)
    runs = [(f, m) for f in fams for m in range(len(MEM_PALETTE))]
    weights = [(0.1 if f.startswith("iso") else 1.0) * (2.0 if m == 0 else 1.0) for f, m in runs]
    owner = _blocks(rng, n_sweep, runs, weights, first=("iso-mid", 0), last=("iso-mid", 0))
    pods, run_of, cpu_of = [], {}, {}

    def ask(uid, family, mem, cpu, pin=None):
        req = {}
        if cpu is not None:
            req["cpu"] = _cpu(cpu)
        if MEM_PALETTE[mem] is not None:
            req["memory"] = str(MEM_PALETTE[mem])
        pods.append(_pod(uid, family, req, pin))
        run_of[uid] = (family, mem)
        cpu_of[uid] = cpu

    for k, v in enumerate(values):
        ask(f"a-{k}", owner[k][0], owner[k][1], v)
    general = [f for f in fams if not f.startswith("iso")]
    for k in range(n_extra):
        src = pods[rng.randrange(n_sweep)]   # an exact duplicate: a class of two inside a would-be run
        uid = f"dup-{k}"
        pods.append({"metadata": dict(src["metadata"], name=uid, uid=uid), "spec": src["spec"]})
        run_of[uid], cpu_of[uid] = run_of[src["metadata"]["uid"]], cpu_of[src["metadata"]["uid"]]
        pin = "ghost" if k == 0 else node_name(rng.randrange(nodes))
        ask(f"pin-{k}", rng.choice(general), rng.randrange(len(MEM_PALETTE)), values[rng.randrange(n_sweep)] + 1, pin)
        ask(f"nocpu-{k}", rng.choice(general), k % len(MEM_PALETTE), None)
        ask(f"cpu0-{k}", rng.choice(general), k % len(MEM_PALETTE), 0)
    rng.shuffle(pods)
    meta = {"values": values, "word_kind": kinds, "run_of": run_of, "cpu_of": cpu_of, "families": fams, "free_cpu": free_cpu,
            "serial": 0, "rng": rng}
    return {"nodes": node_list, "pods": pods}, meta


def sweep_more(meta, count):
    """`count` new asks of the same families with cpu values that no ask has yet (the incremental case)."""
    rng, used = meta["rng"], set(meta["values"])
    fams = [f for f in meta["families"]]
    out = []
    while len(out) < count:
        v = rng.randint(meta["values"][0], meta["values"][-1])
        if v in used:
            continue
        used.add(v)
        meta["serial"] += 1
        mem = rng.randrange(len(MEM_PALETTE))
        req = {"cpu": _cpu(v)}
        if MEM_PALETTE[mem] is not None:
            req["memory"] = str(MEM_PALETTE[mem])
        out.append(_pod(f"new-{meta['serial']}", rng.choice(fams), req))
    return out


# ---- (b) ------------------------------------------------------------------------------------------------------------
EDGES = [(1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 2, 1 << 62, I64_MAX - 1, I64_MAX]
# (allocatable, resident request) of the int64-edge nodes: no per-node sum leaves int64; free values on both sides of 2^53
EDGE_NODES = [((1 << 53) + 1, 1), ((1 << 53) + 1, 2), ((1 << 53) - 1, 1), ((1 << 53) + 2, 1), (1 << 53, 0), (1 << 62, 1),
              (I64_MAX, 0), ("8Ei", 1), (I64_MAX, (1 << 53) + 1), (I64_MAX - 1, 1 << 62), ((1 << 62) + 1, 1), ("8Ei", I64_MAX - (1 << 53))]
TWO_DIM_FAMILIES = ["plain", "all", "a-z1", "ab-z02"]
CPU_PALETTE = [250, 1000, 4000]
EPH_VALUES = 300


def two_dims(seed, nodes, asks):
    """Population (b): group "cpu" = a cpu value of their own × (nothing | memory palette | ephemeral-storage), group "mem" = a
    memory value of their own × (no cpu | cpu palette | ephemeral-storage), group "both" = both their own (two index rows).
    ephemeral-storage has EPH_VALUES distinct values (more than walk_rows: it must stay on ballot planes). The words with
    w % 7 == 3 are the int64-edge slice. meta: group_of[uid], edge_nodes (indices), edge_asks (uids), mem_values, cpu_values."""
    rng = random.Random(seed)
    n_both = asks // 10
    n_cpu = (asks - n_both) // 2
    n_mem = asks - n_both - n_cpu
    cpu_values = irregular_grid(rng, n_cpu + n_both, 41, [1, 2, 3, 5, 8, 13, 40])
    n_edge_asks = 2 * len(EDGES) + 1
    mem_plain = irregular_grid(rng, n_mem + n_both - n_edge_asks, (1 << 20) + 17, [1, 3, 4097, 1 << 20, (1 << 21) + 5, (3 << 22) + 1, 1 << 27])
    eph_values = irregular_grid(rng, EPH_VALUES, GI, [1 << 20, 1 << 28, GI + 1])
    kinds = _word_kinds(nodes, with_isolated=False)
    free_cpu = _designed_free(rng, nodes, kinds, cpu_values, None)
    free_mem = _designed_free(rng, nodes, kinds, mem_plain, None, shift=1)
    edge_nodes = []
    for i in range(nodes):
        if (i // 64) % 7 == 3:
            free_mem[i] = EDGE_NODES[(i + i // 64) % len(EDGE_NODES)]
            edge_nodes.append(i)

    def eph_alloc(r, i):
        k = r.random()
        return {} if k < 0.2 else {"ephemeral-storage": str(eph_values[r.randrange(EPH_VALUES)] + r.choice([-1, 0, 1]))}

    node_list = _build_nodes(rng, nodes, free_cpu, free_mem, kinds, extra_alloc=eph_alloc)
    for i in edge_nodes:   # the edge nodes are open to every family, so that the edge asks reach them
        node_list[i]["spec"]["taints"] = []
        node_list[i]["spec"]["unschedulable"] = False
    fams = TWO_DIM_FAMILIES
    pods, group_of, edge_asks = [], {}, []
    eph_order = list(eph_values)
    rng.shuffle(eph_order)
    eph_used = [0]

    def next_eph():   # every value in turn: all EPH_VALUES occur from that many asks on
        eph_used[0] += 1
        return eph_order[eph_used[0] % EPH_VALUES]

    def ask(uid, group, family, cpu, mem, eph):
        req = {}
        if cpu is not None:
            req["cpu"] = _cpu(cpu)
        if mem is not None:
            req["memory"] = mem if isinstance(mem, str) else str(mem)
        if eph is not None:
            req["ephemeral-storage"] = str(eph)
        pods.append(_pod(uid, family, req))
        group_of[uid] = group

    cpu_own = list(cpu_values)
    rng.shuffle(cpu_own)
    for k in range(n_cpu):
        r = rng.random()
        mem = None if r < 0.35 else (rng.choice(MEM_PALETTE[1:]) if r < 0.7 else None)
        eph = next_eph() if r >= 0.7 else None
        ask(f"c-{k}", "cpu", rng.choice(fams), cpu_own[k], mem, eph)
    # memory values of their own: the plain grid, then the int64 edges (twice, in two families: the same value row in two
    # runs) and "8Ei", which the quantity readers saturate to 2^63 - 1
    mem_own = list(mem_plain)
    rng.shuffle(mem_own)
    for j, e in enumerate(EDGES + EDGES + ["8Ei"]):
        uid = f"e-{j}"
        ask(uid, "mem", "plain" if j < len(EDGES) else "all", None, e, None)
        edge_asks.append(uid)
    for k in range(n_mem - n_edge_asks):
        r = rng.random()
        cpu = None if r < 0.5 else (rng.choice(CPU_PALETTE) if r < 0.7 else None)
        eph = next_eph() if r >= 0.7 else None
        ask(f"m-{k}", "mem", rng.choice(fams), cpu, mem_own[k], eph)
    for k in range(n_both):
        ask(f"b-{k}", "both", rng.choice(fams), cpu_own[n_cpu + k], mem_own[n_mem - n_edge_asks + k], None)
    rng.shuffle(pods)
    meta = {"group_of": group_of, "edge_nodes": edge_nodes, "edge_asks": edge_asks, "cpu_values": cpu_values, "mem_values": mem_plain,
            "word_kind": kinds, "groups": {"cpu": n_cpu, "mem": n_mem, "both": n_both}}
    return {"nodes": node_list, "pods": pods}, meta


# ---- (c) ------------------------------------------------------------------------------------------------------------
def _palettes(rng, big):
    if big:   # 40 x 30 values: more request-value rows than the writers stage in LDS
        cpu = irregular_grid(rng, 40, 90, [10, 25, 60, 125, 300])
        mem = irregular_grid(rng, 30, 1 << 28, [1 << 26, (1 << 28) + 1, 1 << 30])
    else:     # 7 + 6 rows
        cpu = [100, 250, 500, 1000, 2000, 3500, 8000]
        mem = [1 << 27, GI, 4 * GI, 4 * GI + 1, 16 * GI, 64 * GI]
    return cpu, mem


def own_templates(seed, nodes, asks, big_palette=False):
    """Population (c): request vectors from palettes (no dimension walked); three signatures take three quarters of the asks
    (thousands each, in classes of a few dozen rows at most: too small for the band layout at these widths), the rest are groups
    of 1-7 asks with a selector of their own. big_palette: 40 x 30 values, of which the head (8 + 8 values, used by most asks and
    first in ask order) is what the writers stage. meta: sig_of[uid]."""
    rng = random.Random(seed)
    cpu_pal, mem_pal = _palettes(rng, big_palette)
    kinds = _word_kinds(nodes, with_isolated=False)
    free_cpu = _designed_free(rng, nodes, kinds, cpu_pal, None)
    free_mem = _designed_free(rng, nodes, kinds, mem_pal, None, shift=1)

    def more_alloc(r, i):
        out = {"ephemeral-storage": "100Gi"} if r.random() < 0.7 else {}
        if r.random() < 0.5:
            out["example.com/gpu"] = r.choice(["1", "2", "4"])
        if r.random() < 0.5:
            out["example.com/nic"] = r.choice(["1", "2"])
        return out

    node_list = _build_nodes(rng, nodes, free_cpu, free_mem, kinds, extra_alloc=more_alloc)
    head_c, head_m = (cpu_pal[:8], mem_pal[:8]) if big_palette else (cpu_pal, mem_pal)

    def vector(head):
        c = rng.choice((head_c if head else cpu_pal) + [None])
        m = rng.choice((head_m if head else mem_pal) + [None])
        req = {}
        if c is not None:
            req["cpu"] = _cpu(c)
        if m is not None:
            req["memory"] = str(m)
        return req

    cover = []   # the head rows first in ask order: the first request-value rows the engine sees are the ones it stages
    for k in range(max(len(head_c), len(head_m))):
        cover.append(_pod(f"h-{k}", "plain", {"cpu": _cpu(head_c[k % len(head_c)]), "memory": str(head_m[k % len(head_m)])}))
    sig_of = {p["metadata"]["uid"]: "plain" for p in cover}
    pods = []
    n_small = asks // 4
    n_wide = max(asks // 100, 8)   # five request dimensions: more value rows than a run class holds, left to the row-by-row writers
    n_big = asks - n_small - n_wide - len(cover)
    popular = ["plain", "all", "ab-z02"]
    for k in range(n_big):
        f = rng.choices(popular, [5, 3, 2])[0]
        pods.append(_pod(f"t-{k}", f, vector(not big_palette or rng.random() < 0.75)))
        sig_of[f"t-{k}"] = f
    for k in range(n_wide):
        req = dict(vector(True), **{"ephemeral-storage": "10Gi", "example.com/gpu": "2", "example.com/nic": "1"})
        req.setdefault("cpu", _cpu(head_c[0]))
        req.setdefault("memory", str(head_m[0]))
        pods.append(_pod(f"w-{k}", "ab-z02", req))
        sig_of[f"w-{k}"] = "ab-z02"
    racks = (nodes + 15) // 16
    seen, k, g = set(), 0, 0
    while k < n_small:
        while True:
            sel = tuple(sorted(rng.sample(range(racks), rng.choice([1, 2, 3, 4]))))
            if sel not in seen:
                seen.add(sel)
                break
        terms = [{"matchExpressions": [{"key": "rack", "operator": "In", "values": [f"r{r}" for r in sel]}]}]
        tol = rng.choice([[], [_TOL_A], [_TOL_ALL]])
        for _ in range(min(rng.randint(1, 7), n_small - k)):
            spec = {"containers": [{"name": "main", "resources": {"requests": vector(True)}}],
                    "affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": terms}}}}
            if tol:
                spec["tolerations"] = tol
            uid = f"s-{k}"
            pods.append({"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": {"app": "ask"}}, "spec": spec})
            sig_of[uid] = f"own-{g}"
            k += 1
        g += 1
    rng.shuffle(pods)
    meta = {"sig_of": sig_of, "cpu_palette": cpu_pal, "mem_palette": mem_pal, "word_kind": kinds, "own_selectors": g}
    return {"nodes": node_list, "pods": cover + pods}, meta


# ---- (d) ------------------------------------------------------------------------------------------------------------
def class_sizes(asks, singletons=None):
    """The member counts of population (d): every size 1..64 once, a ladder above 64 whose steps are at most 8 % (up to about
    a third of the asks in all), `singletons` classes of one, and what is left in a few classes of tens of thousands."""
    sizes = list(range(1, 65))
    ladder, s = [], 64
    while True:
        s = max(s + 1, int(s * 1.08))
        if sum(ladder) + s > asks // 3:
            break
        ladder.append(s)
    singletons = min(asks // 20, 1500) if singletons is None else singletons
    left = asks - sum(sizes) - sum(ladder) - singletons
    if left < 3 * (ladder[-1] + 1):
        raise ValueError("too few asks for the size ladder")
    big = [left // 2, left // 3, left - left // 2 - left // 3]
    return sizes + ladder + big + [1] * singletons, ladder[-1]


def uneven_classes(seed, nodes, asks):
    """Population (d): templates = distinct (family, cpu, memory) triples from palettes below walk_rows values per dimension;
    member counts from class_sizes(), members interleaved in ask order. meta: template_of[ask position], templates
    [(family, cpu milli, memory bytes)], sizes, ladder_top, free_cpu, free_mem (per node, for the model of equal rows)."""
    rng = random.Random(seed)
    sizes, ladder_top = class_sizes(asks)
    cpu_pal = irregular_grid(rng, 200, 50, [5, 10, 25, 60, 125])
    mem_pal = irregular_grid(rng, 120, 1 << 26, [1 << 24, (1 << 26) + 1, 1 << 28, 1 << 29])
    kinds = _word_kinds(nodes, with_isolated=False)
    free_cpu = _designed_free(rng, nodes, kinds, cpu_pal, None)
    free_mem = _designed_free(rng, nodes, kinds, mem_pal, None, shift=1)
    node_list = _build_nodes(rng, nodes, free_cpu, free_mem, kinds)
    fams = GENERAL[:6]
    seen, templates = set(), []
    while len(templates) < len(sizes):
        t = (rng.choice(fams), rng.choice(cpu_pal), rng.choice(mem_pal))
        if t not in seen:
            seen.add(t)
            templates.append(t)
    rng.shuffle(templates)
    specs = [_pod("", f, {"cpu": _cpu(c), "memory": str(m)})["spec"] for f, c, m in templates]
    template_of = [t for t, n in enumerate(sizes) for _ in range(n)]
    rng.shuffle(template_of)
    pods = [{"metadata": {"name": f"u-{k}", "uid": f"u-{k}", "namespace": "default", "labels": {"app": "ask"}}, "spec": specs[t]}
            for k, t in enumerate(template_of)]
    meta = {"template_of": template_of, "templates": templates, "specs": specs, "sizes": sizes, "ladder_top": ladder_top,
            "free_cpu": free_cpu, "free_mem": free_mem, "word_kind": kinds, "serial": 0, "rng": rng}
    return {"nodes": node_list, "pods": pods}, meta


def uneven_more(meta, count):
    """`count` new members of existing templates → (pods, their templates)."""
    rng = meta["rng"]
    pods, tmpl = [], []
    for _ in range(count):
        t = rng.randrange(len(meta["templates"]))
        meta["serial"] += 1
        uid = f"new-{meta['serial']}"
        pods.append({"metadata": {"name": uid, "uid": uid, "namespace": "default", "labels": {"app": "ask"}}, "spec": meta["specs"][t]})
        tmpl.append(t)
    return pods, tmpl


def model_rows(snapshot, meta):
    """Population (d) through a model of its own (no oracle): the set of nodes each template fits, as a frozenset — eligibility
    by the family's tolerations and zone selector, free cpu / memory >= the request. Templates with equal sets are "equal by
    construction"."""
    nodes = snapshot["nodes"]
    elig = {}
    for f in {t[0] for t in meta["templates"]}:
        tol, sel, aff = FAMILIES[f]
        ok = []
        for i, n in enumerate(nodes):
            zone = n["metadata"]["labels"]["zone"]
            good = True
            taints = list(n["spec"]["taints"])
            if n["spec"]["unschedulable"]:
                taints.append({"key": "node.kubernetes.io/unschedulable", "value": "", "effect": "NoSchedule"})
            for t in taints:
                good &= any(("key" not in o or o["key"] == t["key"]) and (o["operator"] == "Exists" or o.get("value") == t["value"])
                            and (not o.get("effect") or o["effect"] == t["effect"]) for o in tol)
            if sel:
                good &= zone == sel["zone"]
            if aff:
                e = aff[0]["matchExpressions"][0]
                good &= (zone in e["values"]) == (e["operator"] == "In")
            if good:
                ok.append(i)
        elig[f] = ok
    fc, fm = meta["free_cpu"], meta["free_mem"]
    return [frozenset(i for i in elig[f] if fc[i] >= c and fm[i] >= m) for f, c, m in meta["templates"]]
