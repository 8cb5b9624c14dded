"""The shared routines behind libykhost's headroom calls, as far as a handle without an engine reaches them, under AddressSanitizer +
UBSan: tests/c/headroom_host_helpers.c built together with the host library's SOURCES into one stand-alone program."""
import importlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_headroom_host_helpers_on_a_mirror_only_handle_under_the_sanitizers(tmp_path):
    lib = os.path.join(ROOT, "yunikorn-k8shim_amd", "lib")
    importlib.import_module("yunikorn-k8shim_amd").build_all()
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    obj, exe = str(tmp_path / "helpers.o"), str(tmp_path / "helpers")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra"] + san + ["-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "c", "headroom_host_helpers.c"), "-o", obj])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "yunikorn-k8shim_amd", "csrc", "host", "host.cpp"), obj, "-o", exe, "-L" + lib, "-lykpred",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert out.returncode == 0 and "headroom helpers ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
