"""The headroom calls (ykpred_headroom / ykpred_headroom_pod / ykhost_headroom*) as far as they go without a device: the ABI declares
and exports them within version 4, the Python prototypes carry the headers' parameter counts, a mirror-only handle refuses the call
like every other evaluation, and the Go manager binds the one-crossing form."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
PRED = {"ykpred_headroom": 6, "ykpred_headroom_pod": 5}
HOST = {"ykhost_headroom": 4, "ykhost_headroom_nodes": 3, "ykhost_headroom_by_key": 3}


def test_headers_declare_the_calls_and_both_libraries_export_them():
    text = open(os.path.join(ROOT, "include", "ykpred.h")).read()
    assert re.search(r"#define\s+YKPRED_HEADROOM_CELLS\s+16\b", text)
    assert re.search(r"#define\s+YKPRED_ABI_VERSION\s+4\b", text)  # arrived within version 4: detected by the symbol
    for fn in PRED:
        assert re.search(r"\bint32_t\s+" + fn + r"\s*\(", text), fn
    host_text = open(os.path.join(ROOT, "include", "ykhost.h")).read()
    for fn in HOST:
        assert re.search(r"\bint32_t\s+" + fn + r"\s*\(", host_text), fn
    pred_path, host_path = pkg.build_all()
    pred = ctypes.CDLL(pred_path, mode=ctypes.RTLD_GLOBAL)
    host = ctypes.CDLL(host_path)
    for fn in PRED:
        assert hasattr(pred, fn), fn
    for fn in HOST:
        assert hasattr(host, fn), fn
    assert (pkg.HEADROOM_CELLS, pkg.HEADROOM_TOTAL, pkg.HEADROOM_NODES, pkg.HEADROOM_MAX, pkg.HEADROOM_STATUS, pkg.HEADROOM_BY_SLOTS,
            pkg.HEADROOM_BY_PORT, pkg.HEADROOM_BY_RESOURCE0) == (16, 0, 1, 2, 3, 4, 5, 8)


def test_python_prototypes_carry_the_headers_parameter_counts():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_go_bindings as cg
    headers = ""
    for h in ("ykpred.h", "ykhost.h"):
        headers += cg.strip_comments(open(os.path.join(ROOT, "include", h)).read()) + "\n"
    ffi = importlib.import_module("yunikorn-k8shim_amd._ffi")
    for lib, table in ((ffi.load_ykpred(), PRED), (ffi.load_ykhost(), HOST)):
        for name, want in table.items():
            m = re.search(r"\b" + name + r"\s*\(", headers)
            assert m, name
            assert len(cg.split_args(cg.call_args(headers, m.end() - 1))) == want, name
            assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == want, name


def test_headroom_needs_a_device():
    """There is no CPU evaluation path: on a mirror-only handle the reduction fails like every other evaluation."""
    mirror = pkg.GpuPredicateManager(device=-1)
    try:
        mirror.load_snapshot({"nodes": [{"metadata": {"name": "n0"}, "status": {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": "10"}}}],
                              "pods": [{"metadata": {"name": "p0", "uid": "p0"}, "spec": {"containers": [{"name": "c"}]}}]})
        out = np.zeros((1, 16), dtype=np.int64)
        per_node = np.zeros(1, dtype=np.int32)
        assert mirror._L.ykhost_headroom(mirror._h, 1, None, out.ctypes.data) < 0
        assert mirror._L.ykhost_headroom_nodes(mirror._h, 0, per_node.ctypes.data) < 0
        assert mirror._L.ykhost_headroom_by_key(mirror._h, b"p0", out.ctypes.data) < 0
        assert mirror._L.ykhost_headroom_by_key(mirror._h, b"no-such-pod", out.ctypes.data) == -10  # YKHOST_E_POD_NOT_FOUND
        with pytest.raises(RuntimeError, match="mirror-only"):
            mirror.headroom()
        with pytest.raises(RuntimeError, match="mirror-only"):
            mirror.headroom_nodes(0)
    finally:
        mirror.close()


def test_go_manager_binds_the_one_crossing_form():
    go = open(os.path.join(ROOT, "integration", "gpu_predicate_manager.go")).read()
    body = re.search(r"func \(m \*gpuPredicateManager\) Headroom\(pod \*v1\.Pod\).*?\n}\n", go, flags=re.S)
    assert body, "no Headroom(pod) method"
    calls = [c for c in re.findall(r"\bC\.(ykhost_\w+)\(", body.group(0)) if c != "ykhost_last_error"]  # (the error text: failure path only)
    assert calls == ["ykhost_headroom_by_key"], calls
