"""Group columns over the designed clusters of tests/_headgen.py for the per-domain headroom question — which zone, rack or host still
takes `want` copies of an ask, and which is the tightest fit — with a model over Python ints.

Every grouping is built BY CONSTRUCTION on hg.designed() and hg.model, never from what the device answers:
  zone(n)        (a) the `zone` label: G = 3 (fewer on clusters too small to reach every zone)
  zone_holes(n)  (b) the zone label removed from the nodes i % 17 == 3: ungrouped nodes (and a snapshot and meta of their own: a node
                     without the label no longer matches a zone selector)
  hostname(n)    (c) one group per node: G = N
  tie()          (d) a partition built from the model so that for t-main two groups tie on the most copies with different node counts:
                     the lowest id wins for the group with the most copies and for the tightest one alike
  empty_group(n) (e) the zones on ids 0, 2, 3 of G = 4: group 1 has no node
  modulo(n, G)   (f) n % G, for G on either side of the LDS-form limit
Each returns a dict: snapshot, meta, column (list of ids in [-1, G)), G, label_key (None when only the explicit column describes it).
rows(meta, j, column, G) → the (G + 1) x [copies, nodes] table of template j, summary(...) → the 8 summary cells, wants(...) → the
want values at which a summary cell changes.
"""
import copy

import _headgen as hg

LDS_LIMIT = 63  # YKPRED_GROUP_LDS_MAX_GROUPS: up to this many groups a workgroup accumulates in LDS
CELLS, SUMMARY = 2, 8
TIE_KEY = "domain"


def _grouping(snapshot, meta, column, G, label_key=None):
    assert len(column) == len(meta["nodes"]) and all(-1 <= g < G for g in column)
    return {"snapshot": snapshot, "meta": meta, "column": list(column), "G": G, "label_key": label_key}


def zone(n_nodes=hg.PERIOD, extra=0):
    snapshot, meta = hg.designed(n_nodes, extra)
    present = sorted({node["zone"] for node in meta["nodes"]})  # (z0 alone up to 64 nodes, all three from 129 on)
    return _grouping(snapshot, meta, [present.index(node["zone"]) for node in meta["nodes"]], len(present), "zone")


def zone_holes(n_nodes=hg.PERIOD):
    snapshot, meta = hg.designed(n_nodes)
    snapshot, meta = copy.deepcopy(snapshot), copy.deepcopy(meta)
    column = []
    present = sorted({info["zone"] for i, info in enumerate(meta["nodes"]) if i % 17 != 3})
    for i, (node, info) in enumerate(zip(snapshot["nodes"], meta["nodes"])):
        if i % 17 == 3:
            del node["metadata"]["labels"]["zone"]
            info["zone"] = None
            column.append(-1)
        else:
            column.append(present.index(info["zone"]))
    return _grouping(snapshot, meta, column, len(present), "zone")


def hostname(n_nodes=hg.PERIOD, extra=0):
    snapshot, meta = hg.designed(n_nodes, extra)
    names = sorted(node["name"] for node in meta["nodes"])
    assert names == [node["name"] for node in meta["nodes"]]  # (zero-padded: the bytewise order is the index order)
    return _grouping(snapshot, meta, list(range(n_nodes)), n_nodes, "kubernetes.io/hostname")


def tie():
    """G = 5 for t-main (template 0): group 1 = two nodes and group 3 = one node with the SAME total, the largest of all groups; group 0
    and group 2 one node each with fewer copies; group 4 three nodes that take none; every other node ungrouped. The nodes carry the
    label TIE_KEY = d0 .. d4 (a label no ask selects on: no verdict changes)."""
    snapshot, meta = hg.designed()
    snapshot = copy.deepcopy(snapshot)
    reps = [k for k, _ in hg.model(meta, 0)]
    top = max(reps)
    single = reps.index(top)
    pair = next((p, q) for p in range(len(reps)) for q in range(p + 1, len(reps))
                if single not in (p, q) and reps[p] > 0 and reps[q] > 0 and reps[p] + reps[q] == top)
    used = {single, *pair}
    lower = [n for n, k in enumerate(reps) if 0 < k < top and n not in used]
    none = [n for n, k in enumerate(reps) if k == 0][:3]
    column = [-1] * len(reps)
    column[lower[0]], column[lower[-1]], column[single] = 0, 2, 3
    for n in pair:
        column[n] = 1
    for n in none:
        column[n] = 4
    for n, g in enumerate(column):
        if g >= 0:
            snapshot["nodes"][n]["metadata"]["labels"][TIE_KEY] = f"d{g}"
    return _grouping(snapshot, meta, column, 5, TIE_KEY)


def empty_group(n_nodes=hg.PERIOD):
    snapshot, meta = hg.designed(n_nodes)
    return _grouping(snapshot, meta, [(0, 2, 3)[int(node["zone"][1:])] for node in meta["nodes"]], 4)


def modulo(n_nodes, G, extra=0):
    snapshot, meta = hg.designed(n_nodes, extra)
    return _grouping(snapshot, meta, [n % G for n in range(n_nodes)], G)


def rows(meta, j, column, G):
    """→ [[copies, nodes]] * (G + 1) of template j in Python ints; row G = the ungrouped nodes. Status 1: zeros. Status 2: None (the
    copies are -1 and the nodes the single-copy fits, which the model of an uncoupled ask does not describe)."""
    status = meta["templates"][j]["status"]
    if status == 2:
        return None
    table = [[0, 0] for _ in range(G + 1)]
    if status == 0:
        for g, (k, _) in zip(column, hg.model(meta, j)):
            table[g if g >= 0 else G][0] += k
            table[g if g >= 0 else G][1] += 1 if k >= 1 else 0
    return table


def summary_of(table, status, G, want):
    """The 8 summary cells from a table of rows() (None for a coupled template)."""
    if status == 1:
        return [1, 0, 0, 0, 0, 0, 0, 0]
    if status == 2:
        return [2, 0, 0, -1, 0, -1, 0, -1]
    copies = [r[0] for r in table[:G]]
    some = [g for g in range(G) if copies[g] >= 1]
    enough = [g for g in range(G) if copies[g] >= want]
    most = max(some, key=lambda g: (copies[g], -g)) if some else -1
    tight = min(enough, key=lambda g: (copies[g], g)) if enough else -1
    return [0, len(some), len(enough), most, copies[most] if some else 0, tight, copies[tight] if enough else 0, table[G][0]]


def summary(meta, j, column, G, want):
    return summary_of(rows(meta, j, column, G), meta["templates"][j]["status"], G, want)


def wants_of(table, G):
    totals = sorted({r[0] for r in table[:G]}) if table else [0]
    out = {1, totals[-1] + 1}
    for c in totals:
        out.update((c - 1, c, c + 1))
    return sorted(w for w in out if w >= 1)


def wants(meta, j, column, G):
    """1, c − 1, c, c + 1 for every distinct group total c, and max + 1: every value at which a cell of the summary changes."""
    return wants_of(rows(meta, j, column, G), G)
