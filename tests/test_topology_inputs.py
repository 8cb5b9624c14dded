"""The designed clusters of tests/_topogen.py are what they claim, and its model of PodTopologySpread / InterPodAffinity is the
oracle's — no device.

tests/test_gpu_topology.py compares the engine with the oracle AND with the model on these populations. That only discriminates if
the inputs put counts at the thresholds of the rules (sibling templates whose rows really differ, a domain that is absent for one
template, more than 4096 topology signatures, a minimum in the last partial stride of a histogram's cells), and the model is only
worth comparing against if it is right: both are asserted here. The model is written from SURVEY.md §A.6 and states each rule once
per template; the oracle restates the reference path plugin by plugin. Whole grids are compared through the oracle's prefilter_once
form, the per-pair form (the reference's own shape: the PreFilter pass again for every pair) on a sample of asks and, on the
clusters of more than 400 nodes, of nodes."""
import functools
import json
import os

import numpy as np
import pytest

import _oracle as orc
import _topogen

THREADS = min(16, os.cpu_count() or 8)
SEED = 20261
TOPOLOGY = ("PodTopologySpread", "InterPodAffinity")
# plugin lists by name: (PreFilter list, Filter list); the last two are the Filter-without-PreFilter forms
LISTS = {"all": (("*",), ("*",)), "spread": (TOPOLOGY[:1], TOPOLOGY[:1]), "interpod": (TOPOLOGY[1:], TOPOLOGY[1:]), "topology": (TOPOLOGY, TOPOLOGY),
         "reservation": _topogen.RESERVE, "spread-filter-only": ((), TOPOLOGY[:1]), "interpod-filter-only": ((), TOPOLOGY[1:])}
CASES = ("skew_ladder", "policies", "hostname", "interpod", "skew_ladder+ninth")


class Case:
    """One population: the snapshot, the JSON text both sides load, the oracle on it, and the two references per plugin list."""

    def __init__(self, name, snapshot=None, meta=None):
        if snapshot is None:
            base, _, ninth = name.partition("+")
            snapshot, meta = _topogen.POPULATIONS[base](SEED, **({"ninth_zone": True} if ninth else {}))
        self.name, self.snap, self.meta = name, snapshot, meta
        self.text = json.dumps(snapshot)
        self.oracle = orc.Oracle(self.text)
        self.uids = [p["metadata"]["uid"] for p in snapshot["pods"]]
        self.at = {u: k for k, u in enumerate(self.uids)}
        self.names = [n["metadata"]["name"] for n in snapshot["nodes"]]
        self.n = len(snapshot["nodes"])
        self._model, self._grid = {}, {}

    def model(self, which):
        if which not in self._model:
            self._model[which] = _topogen.model(self.snap, self.meta, LISTS[which])
        return self._model[which]

    def grid(self, which):
        """(fit, first failing plugin) of the oracle, the PreFilter pass once per ask."""
        if which not in self._grid:
            pre, filt = (orc.mask_of(_topogen._masks(LISTS[which])[k]) for k in (0, 1))
            self._grid[which] = self.oracle.eval_grid(pre_mask=pre, filt_mask=filt, threads=THREADS, want_plugin=True, prefilter_once=True)
        return self._grid[which]

    def row(self, which, uid):
        return self.model(which)["fit"][self.at[uid]]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def assert_model_is_oracle(c, which):
    m, (fit, code) = c.model(which), c.grid(which)
    bad = np.argwhere(m["fit"] != fit)
    assert bad.size == 0, (f"{c.name} [{which}]: {len(bad)} verdicts differ, first ask {c.uids[bad[0][0]]} node {bad[0][1]}: "
                           f"model {m['fit'][tuple(bad[0])]} oracle {fit[tuple(bad[0])]}")
    bad = np.argwhere(m["code"] != code)
    assert bad.size == 0, (f"{c.name} [{which}]: {len(bad)} failing plugins differ, first ask {c.uids[bad[0][0]]} node {bad[0][1]}: "
                           f"model {m['code'][tuple(bad[0])]} oracle {code[tuple(bad[0])]}")


def test_generators_are_deterministic():
    for name, fn in _topogen.POPULATIONS.items():
        small = {"skew_ladder": {"n_nodes": 90, "n_asks": 40}, "hostname": {"n_nodes": 300}}.get(name, {})
        a = json.dumps(fn(5, **small), sort_keys=True, default=str)
        assert a == json.dumps(fn(5, **small), sort_keys=True, default=str), name
        assert a != json.dumps(fn(6, **small), sort_keys=True, default=str), name


@pytest.mark.parametrize("which", list(LISTS))
@pytest.mark.parametrize("name", CASES)
def test_model_equals_oracle_on_the_whole_grid(name, which):
    assert_model_is_oracle(case(name), which)


@pytest.mark.parametrize("name", CASES[:4])
def test_model_equals_the_per_pair_form_on_a_sample(name):
    """The reference's own shape — every PreFilter plugin again for every (ask, node) pair — on at most 50 asks; on the clusters of
    more than 400 nodes against 64 nodes (the first, the last, the designed ones, the rest spaced evenly)."""
    c = case(name)
    designed = [c.at[u] for pair in c.meta["pairs"] for u in pair[1:3]] + [c.at[u] for u in c.meta["degenerate"]]
    asks = sorted(set(designed[:30] + list(range(0, len(c.uids), max(len(c.uids) // 20, 1)))[:20]))
    assert len(asks) <= 50
    nodes = np.arange(c.n)
    if c.n > 400:
        special = [0, c.n - 1] + list(c.meta.get("minima", {}).values()) + list(c.meta.get("nolabel", [])) + list(c.meta.get("at", {}).values())
        nodes = np.array(sorted(set(special) | set(range(3, c.n, c.n // 40))))
        assert len(nodes) <= 64   # (no slice: it would drop designed nodes without a word)
    for which in ("all", "topology"):
        pre, filt = (orc.mask_of(_topogen._masks(LISTS[which])[k]) for k in (0, 1))
        fit, code = c.oracle.eval_grid(pods=asks, nodes=nodes, pre_mask=pre, filt_mask=filt, threads=THREADS, want_plugin=True)
        m = c.model(which)
        assert np.array_equal(fit, m["fit"][np.ix_(asks, nodes)]), f"{name} [{which}]: per-pair verdicts"
        assert np.array_equal(code, m["code"][np.ix_(asks, nodes)]), f"{name} [{which}]: per-pair failing plugins"


@pytest.mark.parametrize("name", CASES)
def test_sibling_templates_differ_where_the_design_says(name):
    """Every named pair differs in at least one node under the topology plugins alone and, where meta says so, under the full
    list; the templates meta calls equal are equal; no row is constant but the ones that are so by design; fit shares inside (0, 1)."""
    c = case(name)
    for rule, a, b, visible in c.meta["pairs"]:
        assert (c.row("topology", a) != c.row("topology", b)).any(), f"{name}: `{rule}` — {a} and {b} have equal rows under the topology plugins"
        if visible:
            assert (c.row("all", a) != c.row("all", b)).any(), f"{name}: `{rule}` — {a} and {b} have equal rows under the full list"
    for a, b in c.meta["same"]:
        assert np.array_equal(c.row("topology", a), c.row("topology", b)), f"{name}: {a} and {b} were designed to share their verdicts"
    fit = c.model("topology")["fit"]
    constant = {u for u in c.uids if fit[c.at[u]].min() == fit[c.at[u]].max()}
    twins = {u + "-twin" for u in c.meta["degenerate"]}
    assert constant <= set(c.meta["degenerate"]) | twins, f"{name}: constant rows nobody designed: {sorted(constant - set(c.meta['degenerate']) - twins)[:5]}"
    assert constant >= set(c.meta["degenerate"]), f"{name}: rows designed constant that are not: {sorted(set(c.meta['degenerate']) - constant)}"
    for which in ("all", "topology"):
        share = c.model(which)["fit"].mean()
        print(f"TOPO-INPUT {name} [{which}]: {len(c.uids)} asks x {c.n} nodes, fit share {share:.3f}, {c.model(which)['signatures']} topology signatures")
        assert 0 < share < 1


@pytest.mark.parametrize("name", ["skew_ladder", "skew_ladder+ninth"])
def test_skew_ladder_is_its_closed_form_and_crosses_the_signature_threshold(name):
    c = case(name)
    meta = c.meta
    rows = [c.at[u] for u, _, _ in meta["ladder"]]
    closed = _topogen.ladder_closed_form(meta)
    for which in ("topology", "all"):   # (no taints, selectors or requests in this population: the full list decides the same)
        assert np.array_equal(c.model(which)["fit"][rows], closed), which
        assert np.array_equal(c.grid(which)[0][rows], closed), which
    combos = {(json.dumps(p["spec"]["topologySpreadConstraints"], sort_keys=True), s) for p, (_, _, s) in
              zip((c.snap["pods"][k] for k in rows), meta["ladder"])}
    assert len(combos) > 4096 and c.model("topology")["signatures"] > 4096   # kManySigs of kernels.hip.h
    assert 0.65 < closed.mean() < 0.75
    zone = np.array([z or "" for z in meta["zone_of"]])
    assert (zone == "").sum() >= 8 and not closed[:, zone == ""].any()
    for z, off in meta["offsets"].items():
        col = closed[:, zone == z]
        assert (col == col[:, :1]).all()   # a zone's nodes share their verdicts
        if off == 0:
            assert col.all()               # the minimum zone: 0 + self ≤ maxSkew for every maxSkew ≥ 1
            continue
        assert col[:, 0].any() and not col[:, 0].all(), f"zone {z}: only one side of its threshold occurs"
        for self_match in (0, 1):          # the last failing and the first fitting maxSkew, for either self-match
            at = {s: col[k, 0] for k, (_, s, m) in enumerate(meta["ladder"]) if m == self_match}
            assert not any(v for s, v in at.items() if s < off + self_match) and all(v for s, v in at.items() if s >= off + self_match)
    # the pieces of a zone's pods lie in different 256-node blocks (k_spread_count adds them from different workgroups)
    split = [z for z, parts in meta["pieces"].items() if len({i // 256 for i, _ in parts}) > 1]
    assert len(split) >= 2, split
    det = c.model("topology")["detail"][rows[0]][0]
    assert det["min"] == meta["base"] and det["domains"] == len(meta["offsets"])
    assert sorted(det["count"].tolist()) == sorted(meta["base"] + off for off in meta["offsets"].values())
    if name.endswith("ninth"):
        assert len(meta["zone_nodes"]["z8"]) == 1
        assert c.row("topology", "md-9").any() and not c.row("topology", "md-10").any()


def test_policies_population_has_an_absent_domain_and_the_designed_minima():
    c = case("policies")
    meta = c.meta
    zone = np.array([a["zone"] for a in meta["attr"]])
    for uid, want in meta["minimum"].items():
        assert c.model("topology")["detail"][c.at[uid]][0]["min"] == want, uid
    assert c.model("topology")["detail"][c.at["skew-6"]][0]["domains"] == meta["domains"]
    counts = c.model("topology")["detail"][c.at["skew-6"]][0]["count"]
    assert sorted(counts.tolist()) == sorted(_topogen.POLICY_TOTALS.values())
    # the zones outside the selection are no domains for the Honor template: their nodes fit it (count 0 against minimum 5) and fail
    # its Ignore sibling — and no other plugin has a say under the topology list
    honor, zones, ignore = meta["absent_domain"]
    det = c.model("topology")["detail"][c.at[honor]][0]
    assert det["domains"] == meta["domains"] - len(zones) and det["min"] > 0
    there = np.isin(zone, zones)
    assert there.sum() >= 100 and c.row("topology", honor)[there].all()
    assert not c.row("topology", ignore)[zone == zones[0]].any()   # (zm is the sibling's minimum zone: its nodes fit that one too)
    hidden = c.model("all")["code"][c.at[honor]][there]   # under the full list TaintToleration or NodeAffinity answers first there
    assert np.isin(hidden, [_topogen.CODE["TaintToleration"], _topogen.CODE["NodeAffinity"]]).all()
    # pods on nodes without the rack label do not count for the zone constraint of a template that also constrains rack
    one, two, z = meta["rackless_zone"]
    racked = np.array([a["rack"] is not None for a in meta["attr"]])
    assert not c.row("topology", one)[zone == z].any() and c.row("topology", two)[(zone == z) & racked].all()
    m = c.model("topology")
    # a rack-less node fails the template either way: by the zone constraint's skew where that fails first, else by the missing label
    miss = m["missing"][c.at[two]]
    assert not miss[racked].any() and miss[~racked].any() and not miss[~racked].all()
    assert np.array_equal(miss[~racked], np.isin(zone[~racked], sorted(set(zone[racked & (c.row("topology", two) == 1)]))))
    assert (m["code"][c.at[two]][~racked] == _topogen.SPREAD).all()


def test_hostname_population_has_its_minimum_where_claimed():
    c = case("hostname")
    assert c.n % 64 and c.n % 256
    for key, node in c.meta["minima"].items():
        det = c.model("topology")["detail"][c.at[f"{key}-1-0"]][0]
        assert det["min"] == 1 and det["domains"] == c.n - len(c.meta["nolabel"])
        assert (det["count"] == 1).sum() == 1   # ONE domain holds the minimum
        assert np.flatnonzero(c.row("topology", f"{key}-1-0")).tolist() == [node], key
        row = c.row("topology", f"{key}-0-0")
        assert row[node] and 0.7 < row.mean() < 0.9
    # in node order (one thread per node): the first, the last, and two wavefronts of the last, partial 256-node block
    at = c.meta["minima"]
    assert (at["first"], at["last"], at["left"], at["right"]) == (0, c.n - 1, 8255, 8256)
    assert at["left"] // 64 + 1 == at["right"] // 64 and at["right"] // 256 == (c.n - 1) // 256
    # in the order of the histogram's cells (a 64-lane walk over the domains): a key's domains are numbered by the byte order of their
    # values — computed here from the names, not taken from meta
    labelled = sorted(c.names[i].encode() for i in range(c.n) if i not in c.meta["nolabel"])
    domains = len(labelled)
    cell = {key: labelled.index(c.names[node].encode()) for key, node in at.items()}
    assert cell == c.meta["cells"] and len(set(cell.values())) == len(cell)
    assert domains % 64 and domains % 256
    assert cell["cell-left"] // 64 + 1 == cell["cell-right"] // 64 and cell["cell-right"] == domains // 64 * 64   # last full / partial stride
    assert {0, domains - 1} <= set(cell.values())   # the first and the last cell
    flat = c.model("topology")["detail"][c.at["flat-1-0"]][0]
    assert flat["min"] == 2 and set(flat["count"][flat["present"]].tolist()) == {2}
    m = c.model("topology")
    assert m["missing"][c.at["flat-0-0"]].sum() == len(c.meta["nolabel"]) == 3 == (1 - c.row("topology", "flat-0-0")).sum()


def test_interpod_population_states_the_rules_it_names():
    c = case("interpod")
    meta, m = c.meta, c.model("topology")
    zone = np.array([z or "" for z in meta["zone_of"]])
    row = functools.partial(c.row, "topology")
    assert np.array_equal(row("aff-db-zone"), np.isin(zone, ["z1", "z3"]).astype(np.uint8))
    assert np.array_equal(row("aff-db-self"), np.isin(zone, ["z1", "z3"]).astype(np.uint8))   # self-match alone opens no escape
    assert sorted(np.flatnonzero(row("aff-db-host")).tolist()) == sorted([meta["at"]["db-z1"], meta["at"]["db-z3"]])
    assert np.array_equal(row("escape-self"), (zone != "").astype(np.uint8))   # the escape; nodes without the key still fail
    assert np.array_equal(row("solo-self"), (zone != "").astype(np.uint8))
    assert np.array_equal(row("ns-listed"), (zone == "z4").astype(np.uint8))
    assert np.array_equal(row("anti-db-zone"), (~np.isin(zone, ["z1", "z3"])).astype(np.uint8)) and row("anti-db-zone")[zone == ""].all()
    assert np.array_equal(row("intruder"), (zone != "z5").astype(np.uint8))
    assert np.array_equal(row("intruder-other"), (zone != "z0").astype(np.uint8))
    assert sorted(np.flatnonzero(1 - row("hintruder")).tolist()) == sorted(meta["hguards"])
    both = m["code"][c.at[meta["both_fail"]]]
    assert ((both == _topogen.SPREAD) == np.isin(zone, ["z1", "z3", ""])).all()      # PodTopologySpread answers first
    assert ((both == _topogen.INTERPOD) == np.isin(zone, ["z0", "z4", "z5"])).all()
    alone = c.model("interpod")["code"][c.at[meta["both_fail"]]]
    assert (alone[np.isin(zone, ["z1", "z3", ""])] == _topogen.INTERPOD).all()      # ... on nodes that InterPodAffinity fails as well
    assert m["missing"][c.at[meta["both_fail"]]].sum() == (zone == "").sum() > 0


# ---- the incremental steps of tests/test_gpu_topology.py ---------------------------------------------------------------------------
class Edited:
    """The Python snapshot of a case under node and pod changes; with a manager every edit is applied to both."""

    def __init__(self, c, m=None):
        self.m, self.meta = m, c.meta
        self.snap = json.loads(c.text)
        self.names = list(c.names)
        self.where = {}

    def assume(self, uid, node):
        """AssumePod: the ask leaves the pending list and joins the node's pods."""
        pod = next(p for p in self.snap["pods"] if p["metadata"]["uid"] == uid)
        self.snap["pods"] = [p for p in self.snap["pods"] if p["metadata"]["uid"] != uid]
        self.snap["nodes"][node]["pods"].append(dict(pod, spec=dict(pod["spec"], nodeName=self.names[node])))
        self.where[uid] = node
        if self.m:
            self.m.assume_pod(uid, self.names[node])

    def remove(self, uid):
        """RemovePod of an assumed pod: it leaves its node (and the ask table)."""
        pods = self.snap["nodes"][self.where.pop(uid)]["pods"]
        pods[:] = [p for p in pods if p["metadata"]["uid"] != uid]
        if self.m:
            self.m.remove_pod(uid)

    def forget(self, uid):
        """ForgetPod: the pod stays accounted on its node; its ask is pending again, pinned to that node by spec.nodeName."""
        self.snap["pods"].append(next(p for p in self.snap["nodes"][self.where[uid]]["pods"] if p["metadata"]["uid"] == uid))
        if self.m:
            self.m.forget_pod(uid)

    def drop_label(self, node, key):
        del self.snap["nodes"][node]["metadata"]["labels"][key]
        if self.m:
            self.m.update_node({k: v for k, v in self.snap["nodes"][node].items() if k != "pods"})

    def case(self, name):
        return Case(name, self.snap, self.meta)


def ladder_steps(c):
    """The ladder with a ninth zone of one node and the minDomains siblings. None of the steps adds a dictionary entry (no new label
    value, selector or topology key): a manager patches every one of them."""
    zn = c.meta["zone_nodes"]
    return [("z2 from offset 63 to 64", lambda ed: ed.assume("ladder-100", zn["z2"][3])),
            ("the minimum zone gains a pod", lambda ed: ed.assume("ladder-200", zn["z0"][5])),
            ("a pod nobody selects", lambda ed: ed.assume("idle-1", zn["z4"][2])),
            ("remove_pod", lambda ed: ed.remove("ladder-100")),
            ("forget_pod", lambda ed: ed.forget("ladder-200")),
            ("the ninth zone loses its node", lambda ed: ed.drop_label(zn["z8"][0], "zone"))]


def ladder_steps_hold(c, after):
    """What the steps of ladder_steps were designed to do, on the model of the snapshot after each."""
    base = c.meta["base"]

    def hist(x):
        d = x.model("all")["detail"][x.at["ladder-7"]][0]
        return sorted(d["count"][d["present"]].tolist()), d["min"], d["domains"]

    assert hist(c)[1:] == (base, 9) and base + 63 in hist(c)[0]
    h = [hist(x) for x in after]
    assert base + 64 in h[0][0] and base + 63 not in h[0][0] and h[0][1] == base          # every rung's histogram moves, the minimum stays
    assert h[1][1] == base + 1 and h[1][0].count(base + 1) == 2                           # z0 joined z1: the global minimum rose
    assert h[2] == h[1] and np.array_equal(after[2].model("all")["fit"], np.delete(after[1].model("all")["fit"], after[1].at["idle-1"], axis=0))
    assert base + 63 in h[3][0] and h[3][1] == base + 1
    assert h[4] == h[3] and after[4].uids[-1] == "ladder-200" and after[4].row("all", "ladder-200").sum() == 1   # back, pinned by spec.nodeName
    assert (h[4][2], h[5][2]) == (9, 8)                                                    # nine domains → eight
    assert after[4].row("all", "md-9").any() and not after[5].row("all", "md-9").any() and after[5].row("all", "md-8").any()


def interpod_steps(c):
    """No step brings a new anti-affinity term, label value or topology key: a manager patches every one of them."""
    zone = np.array([z or "" for z in c.meta["zone_of"]])
    return [("fresh into z0", lambda ed: ed.assume("fresh-0", int(np.flatnonzero(zone == "z0")[40]))),
            ("a pod nobody selects", lambda ed: ed.assume("nobody", int(np.flatnonzero(zone == "z3")[9]))),
            ("remove_pod", lambda ed: ed.remove("fresh-0")),
            ("fresh onto a node without the label", lambda ed: ed.assume("fresh-1", int(np.flatnonzero(zone == "")[3]))),
            ("forget_pod", lambda ed: ed.forget("fresh-1"))]


def interpod_steps_hold(c, after):
    zone = np.array([z or "" for z in c.meta["zone_of"]])
    labelled = (zone != "").astype(np.uint8)
    assert np.array_equal(c.row("all", "escape-self"), labelled) and not c.row("all", "escape-noself").any()
    # a match exists now: the "no match anywhere" escape is over, with or without self-match the term wants z0
    assert np.array_equal(after[0].row("all", "escape-self"), (zone == "z0").astype(np.uint8))
    assert np.array_equal(after[0].row("all", "escape-noself"), (zone == "z0").astype(np.uint8))
    assert np.array_equal(after[1].model("all")["fit"], np.delete(after[0].model("all")["fit"], after[0].at["nobody"], axis=0))
    assert np.array_equal(after[2].row("all", "escape-self"), labelled)
    # the only match sits on a node without the zone label — in no domain: the escape still holds
    assert np.array_equal(after[3].row("all", "escape-self"), labelled) and not after[3].row("all", "escape-noself").any()
    assert after[4].uids[-1] == "fresh-1" and not after[4].row("all", "fresh-1").any()   # pinned to a node that lacks the key of its own term


@pytest.mark.parametrize("name,steps,hold", [("skew_ladder+ninth", ladder_steps, ladder_steps_hold), ("interpod", interpod_steps, interpod_steps_hold)])
def test_incremental_steps_do_what_they_were_designed_for(name, steps, hold):
    c = case(name)
    ed, after = Edited(c), []
    for k, (label, edit) in enumerate(steps(c)):
        edit(ed)
        after.append(ed.case(f"{name}, step {k + 1} ({label})"))
        assert_model_is_oracle(after[-1], "all")
    hold(c, after)
