"""The group columns of tests/_domaingen.py held to what they claim, without a device; their model against the reference's own clone loop
counted per group; and the boundary the feature adds: exported symbols, header constants, the Go binding."""
import ctypes
import importlib
import os
import re

import numpy as np

import _domaingen as dg
import _headgen as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = 0


def _groupings():
    return {"zone": dg.zone(), "holes": dg.zone_holes(), "hostname": dg.hostname(), "tie": dg.tie(), "empty": dg.empty_group(),
            "whole": dg.modulo(hg.PERIOD, 1), "below": dg.modulo(hg.PERIOD, dg.LDS_LIMIT - 1), "limit": dg.modulo(hg.PERIOD, dg.LDS_LIMIT),
            "above": dg.modulo(hg.PERIOD, dg.LDS_LIMIT + 1)}


def test_the_groupings_are_what_they_claim():
    gs = _groupings()
    assert [gs[k]["G"] for k in ("zone", "holes", "hostname", "tie", "empty", "below", "limit", "above")] == [3, 3, 200, 5, 4, 62, 63, 64]
    # (d) the tie: groups 1 and 3 hold the same, the largest, number of t-main copies on different node counts — the lowest id wins
    # both as the group with the most copies and, for every want above the other groups' totals, as the tightest
    t = gs["tie"]
    table = dg.rows(t["meta"], MAIN, t["column"], t["G"])
    assert table[1][0] == table[3][0] > max(table[0][0], table[2][0]) > 0 and table[1][1] == 2 and table[3][1] == 1
    assert table[4] == [0, 0] and t["column"].count(4) == 3 and table[5][0] > 0
    top = table[1][0]
    assert dg.summary(t["meta"], MAIN, t["column"], 5, top)[1:7] == [4, 2, 1, top, 1, top]
    assert dg.summary(t["meta"], MAIN, t["column"], 5, 1)[3:7] == [1, top, min((0, 2), key=lambda g: (table[g][0], g)), min(table[0][0], table[2][0])]
    assert top in dg.wants(t["meta"], MAIN, t["column"], 5) and top + 1 in dg.wants(t["meta"], MAIN, t["column"], 5)
    assert all(node["metadata"]["labels"].get(dg.TIE_KEY) == (f"d{g}" if g >= 0 else None) for node, g in zip(t["snapshot"]["nodes"], t["column"]))
    # (e) the empty group is empty, (b) ungrouped nodes exist, some of them take copies, and they no longer match a zone selector
    e = gs["empty"]
    assert e["column"].count(1) == 0 and all(e["column"].count(g) > 0 for g in (0, 2, 3))
    h = gs["holes"]
    holes = [n for n, g in enumerate(h["column"]) if g < 0]
    assert holes == [n for n in range(hg.PERIOD) if n % 17 == 3] and all("zone" not in h["snapshot"]["nodes"][n]["metadata"]["labels"] for n in holes)
    assert dg.rows(h["meta"], MAIN, h["column"], 3)[3][0] > 0 and dg.rows(h["meta"], MAIN, h["column"], 3)[3][1] > 0
    z2 = [t["uid"] for t in h["meta"]["templates"]].index("t-z2")
    assert dg.rows(h["meta"], z2, h["column"], 3)[3] == [0, 0] and dg.rows(h["meta"], z2, h["column"], 3)[2][0] > 0
    assert dg.rows(h["meta"], z2, h["column"], 3)[2][0] < dg.rows(gs["zone"]["meta"], z2, gs["zone"]["column"], 3)[2][0]


def test_the_wants_reach_both_ends_of_the_summary():
    """In EVERY grouping the largest want (max + 1) leaves no group that holds it, for every computed template. [2] == G needs a copy in
    every group, which a pinned or zone-selecting template cannot have for G > 1: every computed template reaches it where the whole
    cluster is one group, and t-cpu (it tolerates the tainted zone) also with the three zones as groups."""
    for name, g in _groupings().items():
        meta, column, G = g["meta"], g["column"], g["G"]
        for j, tmpl in enumerate(meta["templates"]):
            if tmpl["status"]:
                assert dg.summary(meta, j, column, G, 1)[0] == tmpl["status"]
                continue
            seen = [dg.summary(meta, j, column, G, w) for w in dg.wants(meta, j, column, G)]
            assert any(s[2] == 0 and s[5] == -1 and s[6] == 0 for s in seen), (name, tmpl["uid"])
            assert all(s[1] >= s[2] and (s[2] == 0) == (s[5] < 0) and (s[1] == 0) == (s[3] < 0) and s[6] <= s[4] for s in seen)
            if name == "whole" or (name == "zone" and tmpl["uid"] == "t-cpu"):
                assert any(s[2] == G for s in seen), (name, tmpl["uid"])
            if name == "whole":
                assert seen[0][4] == hg.expected_cells(meta, j)[0] > 0 and seen[0][7] == 0
            table = dg.rows(meta, j, column, G)
            assert sum(r[0] for r in table) == hg.expected_cells(meta, j)[0] and sum(r[1] for r in table) == hg.expected_cells(meta, j)[1]


def test_model_equals_the_clone_loop_counted_by_group():
    """The reference's sequential loop over Σ model + 3 clones of a template (hg.clone_loop, once per process), its per-node counts
    bincounted by group: every row of the model, for every computed template and every grouping over the unchanged designed cluster."""
    loops = hg.clone_loop()
    gs = _groupings()
    gs["holes"] = dict(gs["zone"], column=gs["holes"]["column"])  # (the column of (b) over the cluster the loop ran on)
    for name, g in gs.items():
        meta, G = g["meta"], g["G"]
        ids = np.array([c if c >= 0 else G for c in g["column"]])
        for j, tmpl in enumerate(meta["templates"]):
            if tmpl["status"]:
                continue
            copies = [0] * (G + 1)
            for n, k in enumerate(loops[j]):
                copies[ids[n]] += int(k)
            nodes = np.bincount(ids[loops[j] >= 1], minlength=G + 1)
            assert [[int(c), int(k)] for c, k in zip(copies, nodes)] == dg.rows(meta, j, g["column"], G), (name, tmpl["uid"])


def test_libraries_header_and_go_file_carry_the_per_domain_calls():
    pkg = importlib.import_module("yunikorn-k8shim_amd")
    pred_path, host_path = pkg.build_all()
    pred = ctypes.CDLL(pred_path, mode=ctypes.RTLD_GLOBAL)
    host = ctypes.CDLL(host_path)
    assert hasattr(pred, "ykpred_headroom_groups")
    for fn in ("ykhost_headroom_domains", "ykhost_domain_values", "ykhost_headroom_domain_by_key"):
        assert hasattr(host, fn), fn
    header = open(os.path.join(ROOT, "include", "ykpred.h")).read()
    assert re.search(r"#define\s+YKPRED_GROUP_CELLS\s+2\b", header) and re.search(r"#define\s+YKPRED_GROUP_SUMMARY\s+8\b", header)
    assert re.search(rf"#define\s+YKPRED_GROUP_LDS_MAX_GROUPS\s+{dg.LDS_LIMIT}\b", header)
    assert (pkg.GROUP_CELLS, pkg.GROUP_SUMMARY, pkg.GROUP_LDS_MAX_GROUPS) == (dg.CELLS, dg.SUMMARY, dg.LDS_LIMIT)
    pred.ykpred_abi_version.restype = ctypes.c_int32
    assert pred.ykpred_abi_version() == 4
    go = open(os.path.join(ROOT, "integration", "gpu_predicate_manager.go")).read()
    assert "C.ykhost_headroom_domain_by_key(" in go and "func (m *gpuPredicateManager) DomainHeadroom(pod *v1.Pod, labelKey string, want int64)" in go
