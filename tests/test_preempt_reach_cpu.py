"""The host side of preemption reach without a device: the mirror parses spec.priority, spec.preemptionPolicy and the allow-preemption
annotation in both ingest paths and keeps them through a dump, and the reclaim table it would upload (ykhost_reclaim_table on a
mirror-only handle) equals the planes of tests/_reachgen.py's model — after load and after every kind of change."""
import copy
import importlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import _preemptgen
import _reachgen
from _reachgen import OPT_OUT, victim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
SEED = 20263
FIXED = ("cpu", "memory", "ephemeral-storage")


@pytest.fixture()
def mirror():
    pm = pkg.GpuPredicateManager(device=-1)
    yield pm
    pm.close()


def dims_of(pm):
    """The engine's dimension order by name, read off the one call that prints them: "Insufficient <resource r>" of explain_format."""
    names = []
    for r in range(pm.encoded_tables()["R"]):
        bins = np.zeros(pkg.EXPLAIN_BINS, dtype=np.int32)
        bins[6] = bins[pkg.EXPLAIN_RESOURCE0 + r] = 1
        names.append(pm.explain_format(bins).split("Insufficient ")[1].rstrip("."))
    assert names[:3] == list(FIXED)
    return names


def check_table(pm, snapshot, bounds):
    """reclaim_table() against the model, every cell of the three planes: requests and pod counts as they are; the port words against an
    encoding of the model's used-after sets — the dictionary bit of a triple is read off the wanted words of the ask that wants it (every
    ask of these populations wants at most one port), and bit k of ports_after[t][:, n] is set exactly when dictionary port k conflicts
    with what node n still uses once tiers 0..t are gone."""
    model = _reachgen.ReachModel(snapshot, bounds)
    names = [n["metadata"]["name"] for n in snapshot["nodes"]]
    order = [names[i] for i in np.argsort([pm.node_index(n) for n in names])]
    assert sorted(pm.node_index(n) for n in names) == list(range(len(names)))
    req, cnt, ports = pm.reclaim_table()
    dims = dims_of(pm)
    want_req, want_cnt, used = model.planes(order, dims)
    assert req.shape == (len(bounds), len(dims), len(order)) and cnt.shape == (len(bounds), len(order))
    assert req.tolist() == want_req
    assert cnt.tolist() == want_cnt
    tables = pm.encoded_tables()
    KP = tables["KP"]
    assert ports.shape == (len(bounds), KP, len(order))
    triple_of, dictionary = {}, [0] * KP
    for ask in snapshot["pods"]:
        wanted = _preemptgen._host_ports(ask)
        row = pm.pod_index(ask["metadata"]["uid"])
        if not wanted or row < 0:
            continue
        assert len(wanted) == 1
        words = tables["wanted_ports"][tables["pod_spec"][row] * KP:(tables["pod_spec"][row] + 1) * KP]
        bits = [(k, b) for k in range(KP) for b in range(64) if words[k] >> b & 1]
        assert len(bits) == 1, (ask["metadata"]["uid"], words)
        assert triple_of.setdefault(bits[0], wanted[0]) == wanted[0]
    for s in range(len(tables["wanted_ports"]) // KP if KP else 0):
        dictionary = [d | w for d, w in zip(dictionary, tables["wanted_ports"][s * KP:(s + 1) * KP])]
    assert dictionary == [sum(1 << b for (k, b) in triple_of if k == word) for word in range(KP)]   # every dictionary bit is accounted for
    want_ports = [[[sum(1 << b for (k, b), triple in triple_of.items() if k == word and _preemptgen._conflict(triple, used[t][n]))
                    for n in range(len(order))] for word in range(KP)] for t in range(len(bounds))]
    assert ports.tolist() == want_ports
    return len(triple_of)


@pytest.mark.parametrize("name", ("resource_boundaries", "slots", "ports", "empty_and_opted_out", "one_tier", "best_ties"))
def test_reclaim_table_equals_the_model_after_load(mirror, name):
    snapshot, bounds, _ = _reachgen.population(name, SEED)
    mirror.load_snapshot(snapshot)
    mirror.set_preemption_tiers(bounds)
    ports = check_table(mirror, snapshot, bounds)
    assert ports > 0 or name not in ("ports", "one_tier")


def running(pod, node):
    doc = copy.deepcopy(pod)
    doc["spec"]["nodeName"] = node
    doc["status"] = {"phase": "Running"}
    return doc


def test_reclaim_table_follows_every_change(mirror):
    """add, remove, update (a priority change, an opt-out), assume, forget, new bounds, a node removal: the table stays the model's."""
    snapshot, bounds, _ = _reachgen.population("ports", SEED)
    snap = copy.deepcopy(snapshot)
    mirror.load_snapshot(snapshot)
    mirror.set_preemption_tiers(bounds)
    node = {n["metadata"]["name"]: n for n in snap["nodes"]}
    check_table(mirror, snap, bounds)
    # add: a tier-1 pod holding the port on po-kept
    new = victim("added", bounds, 1, {"cpu": 30, "memory": 5}, ports=[_reachgen.T80])
    mirror.update_pod(running(new, "po-kept"))
    node["po-kept"]["pods"].append(new)
    check_table(mirror, snap, bounds)
    # remove: the tier-0 holder of po-one-0
    gone = next(p for p in node["po-one-0"]["pods"] if p["metadata"]["uid"] == "po-one-0-t0")
    assert mirror.remove_pod("po-one-0-t0")
    node["po-one-0"]["pods"].remove(gone)
    check_table(mirror, snap, bounds)
    # update: a priority change moves a pod from tier 1 to tier 2; an annotation takes another out of every tier
    moved = next(p for p in node["po-one-1"]["pods"] if p["metadata"]["uid"] == "po-one-1-t1")
    moved["spec"]["priority"] = bounds[1]
    mirror.update_pod(running(moved, "po-one-1"))
    check_table(mirror, snap, bounds)
    out = next(p for p in node["po-one-2"]["pods"] if p["metadata"]["uid"] == "po-one-2-t2")
    out["metadata"]["annotations"] = {OPT_OUT: "false"}
    mirror.update_pod(running(out, "po-one-2"))
    check_table(mirror, snap, bounds)
    # ... and a version that changes nothing but the priority back is not taken for a resync
    moved["spec"]["priority"] = bounds[0]
    mirror.update_pod(running(moved, "po-one-1"))
    check_table(mirror, snap, bounds)
    # assume: an ask becomes a resident of its node (its own priority decides its tier); forget keeps it there
    ask = next(p for p in snap["pods"] if p["metadata"]["uid"] == "a-port-half")
    mirror.assume_pod("a-port-half", "po-wild-0")   # (the ask keeps its row and its dictionary port; the node holds a copy of it)
    node["po-wild-0"]["pods"].append(copy.deepcopy(ask))
    check_table(mirror, snap, bounds)
    mirror.forget_pod("a-port-half")
    check_table(mirror, snap, bounds)
    # new bounds: another tier count, other cuts
    bounds = [50, 150, 250, 1000]
    mirror.set_preemption_tiers(bounds)
    check_table(mirror, snap, bounds)
    # a node removal shifts the columns
    mirror.remove_node("po-one-1")
    snap["nodes"].remove(node["po-one-1"])
    check_table(mirror, snap, bounds)
    mirror.set_preemption_tiers([])
    with pytest.raises(RuntimeError, match="no preemption tiers"):
        mirror.reclaim_table()


def preemption_fields(snapshot):
    """uid -> (priority, policy is Never, opted out) of every pod of a snapshot document"""
    out = {}
    for p in snapshot["pods"] + [q for n in snapshot["nodes"] for q in n["pods"]]:
        out[p["metadata"]["uid"]] = (p["spec"].get("priority") or 0, p["spec"].get("preemptionPolicy") == "Never",
                                     (p["metadata"].get("annotations") or {}).get(OPT_OUT) == "false")
    return out


@pytest.mark.parametrize("name", ("limits", "empty_and_opted_out"))
def test_fields_survive_dump_and_load(mirror, name):
    snapshot, bounds, _ = _reachgen.population(name, SEED)
    mirror.load_snapshot(snapshot)
    dumped = json.loads(mirror.dump_snapshot())
    assert preemption_fields(dumped) == preemption_fields(snapshot)
    assert any(never for _, never, _ in preemption_fields(dumped).values()) or name != "limits"
    again = pkg.GpuPredicateManager(device=-1)
    try:
        again.load_snapshot(dumped)
        again.set_preemption_tiers(bounds)
        mirror.set_preemption_tiers(bounds)
        for a, b in zip(again.reclaim_table(), mirror.reclaim_table()):
            assert np.array_equal(a, b)
        compact = json.loads(again.dump_snapshot(compact=True))
        assert sum(p.get("replicas", 1) for n in compact["nodes"] for p in n["pods"]) == sum(len(n["pods"]) for n in snapshot["nodes"])
    finally:
        again.close()


def documents(snapshot):
    nodes = [dict(n, pods=[]) for n in snapshot["nodes"]]
    pods = [running(p, n["metadata"]["name"]) for n in snapshot["nodes"] for p in n["pods"]] + [dict(p, status={"phase": "Pending"}) for p in snapshot["pods"]]
    return nodes, pods


@pytest.mark.parametrize("threads", ("1", "4"))
def test_both_ingest_paths_and_parallel_ingest_agree(monkeypatch, threads):
    """The same cluster through load_snapshot (the tree parser), update_pod one by one (the scanner) and update_pods_batch (a batch this
    small stays on the caller's thread whatever the thread count: the scanning threads are test_parallel_ingest_equals_one_thread's):
    the same fields on every pod (seen through the dump) and the same reclaim table."""
    monkeypatch.setenv("YKHOST_INGEST_THREADS", threads)
    snapshot, bounds, _ = _reachgen.population("empty_and_opted_out", SEED)
    extra = victim("odd", bounds, 3, {"cpu": 1})
    extra["spec"]["priority"] = None            # an explicit null counts as missing
    extra["spec"]["preemptionPolicy"] = None
    extra["metadata"]["annotations"] = {"kubectl.kubernetes.io/last-applied-configuration": "{\"a\":\"b\\n\"}", OPT_OUT: "true"}
    snapshot["nodes"][0]["pods"].append(extra)
    nodes, pods = documents(snapshot)
    tables = []
    for how in ("snapshot", "one by one", "batch"):
        pm = pkg.GpuPredicateManager(device=-1)
        try:
            if how == "snapshot":
                pm.load_snapshot(snapshot)
            else:
                pm.update_nodes_batch(nodes)
                if how == "batch":
                    assert pm.update_pods_batch(pods) == len(pods)
                else:
                    for p in pods:
                        pm.update_pod(p)
            assert preemption_fields(json.loads(pm.dump_snapshot())) == preemption_fields(snapshot), how
            pm.set_preemption_tiers(bounds)
            check_table(pm, snapshot, bounds)
            tables.append(pm.reclaim_table())
        finally:
            pm.close()
    for other in tables[1:]:
        for a, b in zip(tables[0], other):
            assert np.array_equal(a, b)


def big_cluster():
    """40 nodes, 3 000 residents and 400 asks with mixed priorities, policies, opt-outs and host ports — 1.3 MB of pod documents, well
    over the size from which a batch is cut into pieces for the scanning threads — and a second delivery of every third resident in
    which priorities move across tiers, opt-outs flip and some documents change nothing."""
    b = [100, 200, 300]
    rng = random.Random(5)
    nodes = [_preemptgen.make_node(f"big-{i:03d}", {"cpu": 10 ** 9, "memory": 1 << 50}, [], allowed=100000) for i in range(40)]
    for i in range(3000):
        ports = [("10.0.0.1", "TCP", 8000 + i % 7)] if i % 5 == 0 else None
        nodes[i % 40]["pods"].append(victim(f"big-r{i}", b, rng.randrange(4), {"cpu": rng.randrange(1, 500), "memory": rng.randrange(1, 99)}, ports=ports,
                                            opt_out=i % 11 == 0, rng=rng))
    asks = [_reachgen.asker(f"big-a{i}", b, i % 4, {"cpu": 1 + i % 50}, never=i % 7 == 0, ports=[("10.0.0.1", "TCP", 8000 + i % 7)] if i % 3 == 0 else None)
            for i in range(400)]
    first = {"nodes": nodes, "pods": asks}
    second = copy.deepcopy(first)
    again = []
    for n in second["nodes"]:
        for p in n["pods"]:
            i = int(p["metadata"]["uid"][5:])
            if i % 3:
                continue
            if i % 9 == 0:
                p["spec"]["priority"] = _reachgen.tier_priority(b, rng.randrange(4), rng)
            elif i % 9 == 3:
                if p["metadata"].pop("annotations", None) is None:
                    p["metadata"]["annotations"] = {OPT_OUT: "false"}
            again.append(running(p, n["metadata"]["name"]))
    return b, first, second, again


def test_parallel_ingest_equals_one_thread(monkeypatch):
    """Pod batches large enough for the scanning threads (the handle's parallel_batches counter says that they ran): the bulk cache pass
    of a start-up replay, then the ordered pass of a second delivery of cached uids. On 4 threads and on 1: the priority, policy and
    opt-out of every pod (seen through the dump) and the reclaim table are the expected ones — and so equal each other."""
    bounds, first, second, again = big_cluster()
    nodes, pods = documents(first)
    pods = [json.dumps(p).encode() for p in pods]
    again = [json.dumps(p).encode() for p in again]
    assert sum(map(len, pods)) > 8 * 65536 and sum(map(len, again)) > 4 * 65536
    assert preemption_fields(first) != preemption_fields(second)
    tables = {}
    for threads in ("4", "1"):
        monkeypatch.setenv("YKHOST_INGEST_THREADS", threads)
        pm = pkg.GpuPredicateManager(device=-1)
        try:
            pm.update_nodes_batch(nodes)
            assert pm.update_pods_batch(pods) == len(pods)
            timing = pm.ingest_timing()
            assert (timing["parallel_batches"], timing["bulk_batches"]) == ((1, 1) if threads == "4" else (0, 0)), timing
            assert preemption_fields(json.loads(pm.dump_snapshot())) == preemption_fields(first)
            pm.set_preemption_tiers(bounds)
            assert check_table(pm, first, bounds) == 7
            assert pm.update_pods_batch(again) == len(again)
            timing = pm.ingest_timing()
            assert (timing["parallel_batches"], timing["bulk_batches"]) == ((2, 1) if threads == "4" else (0, 0)), timing
            assert preemption_fields(json.loads(pm.dump_snapshot())) == preemption_fields(second)
            check_table(pm, second, bounds)
            tables[threads] = pm.reclaim_table()
        finally:
            pm.close()
    for a, b in zip(tables["4"], tables["1"]):
        assert np.array_equal(a, b)


def test_scanner_hands_odd_documents_to_the_full_parser(mirror):
    """A priority written as a string or with an exponent, an escaped annotation key: the tree parser's reading counts."""
    mirror.update_node({"metadata": {"name": "n0"}, "status": {"allocatable": {"cpu": "4", "memory": "1Gi", "pods": "10"}}})
    pod = running(victim("p", (10,), 0, {"cpu": 100}), "n0")
    for i, (priority, annotations, want) in enumerate((("7", None, (7, False)), (3, {"yunikorn.apache.org\\/allow-preemption": "false"}, (3, False)),
                                                       (-2147483648, {OPT_OUT: "false"}, (-2147483648, True)), (2147483647, {OPT_OUT: "False"}, (2147483647, False)))):
        doc = copy.deepcopy(pod)
        doc["metadata"]["uid"] = doc["metadata"]["name"] = f"p{i}"
        doc["spec"]["priority"] = priority
        if annotations:
            doc["metadata"]["annotations"] = annotations
        mirror.update_pod(doc)
        got = preemption_fields(json.loads(mirror.dump_snapshot()))[f"p{i}"]
        assert (got[0], got[2]) == want, (i, got)
    text = json.dumps(dict(pod, metadata=dict(pod["metadata"], uid="esc", name="esc"))).replace('"annotations"', '"x"')
    text = text.replace('"labels"', '"annotations": {"yunikorn.apache.org\\/allow-preemption": "false"}, "labels"')
    mirror.update_pods_batch([text.encode()])
    assert preemption_fields(json.loads(mirror.dump_snapshot()))["esc"][2] is True


def test_tiers_are_validated(mirror):
    for bad in ([3, 3], [5, 1], list(range(9))):
        with pytest.raises(RuntimeError, match="set_preemption_tiers"):
            mirror.set_preemption_tiers(bad)
    mirror.set_preemption_tiers([1, 2, 3, 4, 5, 6, 7, 8])
    with pytest.raises(RuntimeError, match="mirror-only"):
        mirror.preempt_reach()
    with pytest.raises(RuntimeError, match="mirror-only"):
        mirror.preempt_reach_nodes(0)


def test_reclaim_table_program_under_the_sanitizers(tmp_path):
    """tests/c/reclaim_table_host.c built together with the host library's SOURCES under AddressSanitizer + UBSan, run directly."""
    lib = os.path.join(ROOT, "yunikorn-k8shim_amd", "lib")
    pkg.build_all()
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    obj, exe = str(tmp_path / "reclaim.o"), str(tmp_path / "reclaim")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra"] + san + ["-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "c", "reclaim_table_host.c"), "-o", obj])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "yunikorn-k8shim_amd", "csrc", "host", "host.cpp"), obj, "-o", exe, "-L" + lib, "-lykpred",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert out.returncode == 0 and "reclaim table ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
