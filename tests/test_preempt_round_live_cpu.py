"""The live preemption round without a device: the new symbols are exported by the libraries and bound — header <-> library, header <->
Python, header <-> Go; the mirror's victim-effects plane on a mirror-only handle — derived at the first request, its prefix sums against
the pods' labels, its column sums against selector_count, patched when pods leave and arrive, derived anew when the selector classes
move; and tests/c/victim_effects_host.c — a stand-alone program built with libykhost's sources under AddressSanitizer + UBSan and run
directly."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import _liveroundgen as gen
from test_live_round_inputs import SEED
from test_preempt_round_cpu import params, read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
ffi = importlib.import_module("yunikorn-k8shim_amd._ffi")
ENGINE = ("ykpred_preempt_round_live", "ykpred_set_victim_effects", "ykpred_update_victim_effects_node", "ykpred_histogram_dims")
HOST = ("ykhost_preempt_round_live", "ykhost_preempt_round_live_by_keys", "ykhost_preempt_gang_live_by_key", "ykhost_victim_effects")


def test_header_library_python_and_go_name_the_same_calls():
    pkg.build_all()
    pred_h, host_h = read("include", "ykpred.h"), read("include", "ykhost.h")
    assert re.search(r"#define\s+YKPRED_ABI_VERSION\s+4\b", pred_h) and 'dlsym("ykpred_preempt_round_live")' in pred_h   # arrived within version 4
    pred, host = ffi.load_ykpred(), ffi.load_ykhost()
    for lib, header, names in ((pred, pred_h, ENGINE), (host, host_h, HOST)):
        for name in names:
            fn = getattr(lib, name)   # exported: ctypes resolves the symbol here
            assert fn.argtypes is not None and len(fn.argtypes) == params(header, name), name
    fields = re.search(r"typedef struct ykpred_victim_effects \{(.*?)\} ykpred_victim_effects_t;", re.sub(r"/\*.*?\*/", "", pred_h, flags=re.S), flags=re.S)
    assert fields and len([f for f in fields.group(1).split(";") if f.strip()]) == len(ffi.YkpredVictimEffects._fields_)
    for method in ("preempt_round_live", "preempt_round_live_by_keys", "preempt_gang_live", "victim_effects"):
        assert callable(getattr(pkg.GpuPredicateManager, method))
    go = read("integration", "gpu_predicate_manager.go")
    assert "func (m *gpuPredicateManager) PreemptionRoundLive(" in go
    call = re.search(r"C\.ykhost_preempt_round_live_by_keys\((.*?)\)\n", go, flags=re.S)
    assert call and len(call.group(1).split(",")) == params(host_h, "ykhost_preempt_round_live_by_keys")
    engine = read("yunikorn-k8shim_amd", "csrc", "engine", "engine.hip")
    assert "PreemptionRoundLive" in read("INTEGRATION.md") and "ykpred:preempt_round_live" in engine
    for kernel in ("k_preempt_round_effects", "k_preempt_round_topo"):
        assert kernel in engine and kernel in read("yunikorn-k8shim_amd", "csrc", "engine", "kernels.hip.h")


@pytest.mark.parametrize("name", ("victim_min", "affinity", "host_gang_eq"))
def test_the_mirrors_plane_on_a_mirror_only_handle(name):
    snapshot, bounds, meta = gen.round_(name, SEED)
    pm = pkg.GpuPredicateManager(device=-1)
    try:
        pm.load_snapshot(snapshot)
        pm.set_preemption_tiers(bounds)
        t = pm.victim_table()
        assert t["derived"] == 1
        fx = pm.victim_effects()
        assert fx["derived"] == 1 and fx["patches"] == 0 and pm.victim_table()["derived"] == 1   # (asking for the plane derives no table)
        tables = pm.encoded_tables()
        N, KS = len(snapshot["nodes"]), len(fx["class_col"])
        selcount = np.array(tables["selector_count"], dtype=np.int64).reshape(KS, N) if KS else np.zeros((0, N), dtype=np.int64)
        T = len(bounds)
        count = t["tier_end"][T - 1]
        KA = fx["cum"].shape[0]
        assert sorted(c for c in fx["class_col"] if c >= 0) == list(range(KA)) and fx["cum"].shape[1] == t["cum"].shape[1]
        seen = 0
        for n in range(N):
            base, k = int(t["seg_base"][n]), int(count[n])
            every = len(snapshot["nodes"][n]["pods"])
            for s in range(KS):
                col = fx["class_col"][s]
                row = fx["cum"][col, base:base + k] if col >= 0 else np.zeros(k, dtype=np.int32)
                assert (np.diff(row, prepend=0) >= 0).all()          # prefix sums of contributions >= 0
                total = int(row[-1]) if k else 0
                assert total <= selcount[s, n]                        # the victims are some of the node's pods
                if k == every:
                    assert total == selcount[s, n], (n, s)            # every pod of the node is a victim: the column sum
                seen += total
        assert seen > 0 and KA >= 1
        # a class with no column has no contributing victim anywhere; a class with one has some
        for s in range(KS):
            if fx["class_col"][s] >= 0:
                assert fx["cum"][fx["class_col"][s]].max() > 0
        # pods leave: segments are patched, nothing is derived anew, and the plane equals a fresh handle's
        victims = [(n, pm.victim_list(n, T)) for n in range(N) if count[n] > 0][:3]
        for n, uids in victims:
            assert pm.remove_pod(uids[0])
        fx2 = pm.victim_effects()
        if name == "affinity":   # (a removed pod carried an anti-affinity term or was a class's only match: the classes moved)
            assert fx2["derived"] == 2
        else:
            assert fx2["derived"] == 1 and fx2["patches"] == len(victims)
        fresh = pkg.GpuPredicateManager(device=-1)
        try:
            fresh.load_snapshot(pm.dump_snapshot())
            fresh.set_preemption_tiers(bounds)
            t3, fx3 = fresh.victim_table(), fresh.victim_effects()
        finally:
            fresh.close()
        t2 = pm.victim_table()
        assert len(fx2["class_col"]) == len(fx3["class_col"])
        KS = len(fx2["class_col"])
        for n in range(N):
            k = int(t2["tier_end"][T - 1][n])
            assert k == int(t3["tier_end"][T - 1][n])
            for s in range(KS):
                a, b = fx2["class_col"][s], fx3["class_col"][s]
                mine = fx2["cum"][a, int(t2["seg_base"][n]):int(t2["seg_base"][n]) + k] if a >= 0 else np.zeros(k, dtype=np.int32)
                theirs = fx3["cum"][b, int(t3["seg_base"][n]):int(t3["seg_base"][n]) + k] if b >= 0 else np.zeros(k, dtype=np.int32)
                assert np.array_equal(mine, theirs), (n, s)
        with pytest.raises(RuntimeError, match="mirror-only"):
            pm.preempt_round_live([0])
        with pytest.raises(RuntimeError, match="mirror-only"):
            pm.preempt_round_live_by_keys([meta["turns"][0]])
        with pytest.raises(RuntimeError, match="mirror-only"):
            pm.preempt_gang_live(meta["turns"][0], 3)
    finally:
        pm.close()


def test_the_plane_is_derived_anew_when_the_selector_classes_move():
    snapshot, bounds, meta = gen.round_("victim_min", SEED)
    pm = pkg.GpuPredicateManager(device=-1)
    try:
        pm.load_snapshot(snapshot)
        pm.set_preemption_tiers(bounds)
        fx = pm.victim_effects()
        assert fx["derived"] == 1 and fx["cum"].shape[0] == 1
        # an ask with a selector of its own that the tier-0 residents match: one more class, with contributing victims
        ask = {"metadata": {"name": "late", "uid": "late", "namespace": "default", "labels": {"app": "late"}},
               "spec": {"containers": [{"name": "c", "resources": {"requests": {"cpu": "10m"}}}],
                        "topologySpreadConstraints": [gen.spread("res")]}}
        pm.update_pod(ask)
        fx2 = pm.victim_effects()
        assert fx2["derived"] == 2 and len(fx2["class_col"]) == len(fx["class_col"]) + 1 and fx2["cum"].shape[0] == 2
    finally:
        pm.close()


def test_effects_host_program_under_the_sanitizers(tmp_path):
    """tests/c/victim_effects_host.c built together with the host library's SOURCES under AddressSanitizer + UBSan, run directly."""
    lib = os.path.join(ROOT, "yunikorn-k8shim_amd", "lib")
    pkg.build_all()
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    obj, exe = str(tmp_path / "effects.o"), str(tmp_path / "effects")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-D_POSIX_C_SOURCE=200809L"] + san + ["-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "c", "victim_effects_host.c"), "-o", obj])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "yunikorn-k8shim_amd", "csrc", "host", "host.cpp"), obj, "-o", exe, "-L" + lib, "-lykpred",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert out.returncode == 0 and "victim effects host ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
