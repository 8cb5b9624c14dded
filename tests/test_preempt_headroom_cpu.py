"""Preemption headroom without a device: the finish step (csrc/engine/preempt_headroom_finish.h — per-level deltas to the 32 cells of one
ask, plain C++) on hand-made delta tables against a Python restatement, run by tests/c/preempt_headroom_finish.cpp — a stand-alone
program built with libykhost's sources under AddressSanitizer + UBSan and run directly — and the argument errors of the host calls on a
mirror-only handle."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import _gangreachgen as gg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("yunikorn-k8shim_amd")
T = 8


def finish_model(deltas, limit, want, coupled):
    """The contract of include/ykpred.h over Python ints."""
    out = [0] * 32
    out[27], out[28], out[29] = (1 if deltas[27] else 2 if coupled else 0), limit, want
    if deltas[27]:
        return out
    for row in range(3):
        for L in range(9):
            out[9 * row + L] = sum(deltas[9 * row:9 * row + L + 1])
    out[30] = -1
    if coupled:
        out[0:9] = out[18:27] = [-1] * 9
        return out
    out[30] = next((L for L in range(limit + 1) if out[L] >= want), -1)
    return out


def table(limit, copies, nodes, victims, routed=0):
    """Deltas of one task: the three rows hold something at the levels 0..limit only, as the kernel leaves them."""
    row = [0] * 32
    for L in range(limit + 1):
        row[L], row[9 + L], row[18 + L] = copies[L], nodes[L], victims[L]
    row[27] = routed
    return row


def cases():
    out = []
    steep = ([5, 0, 7, 1, 0, 0, 2, 40, 1], [2, 0, 3, 1, 0, 0, 1, 9, 1], [0, 0, 6, 2, 0, 0, 3, 50, 4])
    for limit in (0, 1, 4, T):
        d = table(limit, *steep)
        sums = np.cumsum(d[:9]).tolist()
        wants = {1, sums[limit] + 1, 2 ** 40}
        for s in set(sums):   # on, one above and one below every prefix sum
            wants |= {w for w in (s - 1, s, s + 1) if w >= 1}
        for want in sorted(wants):
            out.append((limit, want, 0, d))
        out.append((limit, 3, 1, d))                              # coupled
        out.append((limit, 3, 0, table(limit, *steep, routed=1)))  # routed, by one shard ...
        out.append((limit, 3, 1, table(limit, *steep, routed=2)))  # ... by both, and coupled beside it: routed wins
    for limit in (0, 3, T):   # N == 0: nothing arrived
        out.append((limit, 1, 0, [0] * 32))
        out.append((limit, 1, 1, [0] * 32))
    big = table(T, [2 ** 37] * 9, [2 ** 20] * 9, [0] + [2 ** 36] * 8)   # sums past 2^32
    out += [(T, 2 ** 40, 0, big), (T, 2 ** 40 + 1, 0, big), (3, 2 ** 39 + 1, 0, table(3, [2 ** 37] * 9, [1] * 9, [0] * 9))]
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/c/preempt_headroom_finish.cpp + the host library's SOURCES in one binary under the sanitizers; the engine library as built."""
    lib = os.path.join(ROOT, "yunikorn-k8shim_amd", "lib")
    pkg.build_all()
    exe = str(tmp_path_factory.mktemp("preempt_headroom") / "finish")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter"] + san + ["-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "preempt_headroom_finish.cpp"),
                           os.path.join(ROOT, "yunikorn-k8shim_amd", "csrc", "host", "host.cpp"), "-o", exe, "-L" + lib, "-lykpred", "-Wl,-rpath," + lib])
    return exe


def test_finish_on_hand_made_delta_tables_under_the_sanitizers(program, tmp_path):
    listed = cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(str(x) for x in [limit, want, coupled] + d) + "\n" for limit, want, coupled, d in listed))
    out = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert out.returncode == 0 and out.stdout.endswith("preempt headroom ok\n"), (out.stdout[-500:], out.stderr[-3000:])
    lines = out.stdout.splitlines()[:-1]
    assert len(lines) == len(listed) > 50
    levels = set()
    for line, (limit, want, coupled, d) in zip(lines, listed):
        got = [int(x) for x in line.split()]
        assert got == finish_model(d, limit, want, coupled), (limit, want, coupled, d, got)
        levels.add(got[30])
        if got[27] == 0:   # the invariants of the contract
            assert got[0:9] == sorted(got[0:9]) and got[9:18] == sorted(got[9:18]) and got[18:27] == sorted(got[18:27])
            assert got[limit:9] == [got[limit]] * (9 - limit)
    assert levels >= {-1, 0, 2, 3, 6, 7, 8}


def test_finish_model_is_the_generators_expected_cells():
    """The restatement above and tests/_gangreachgen.expected_cells — which starts from per-node copies — agree on a small table."""
    rows = [[0, 1, 2, 0], [0, 1, 3, 0], [1, 1, 3, 0], [1, 4, 3, 0]]   # [level][node]
    gone = [[0, 0, 0, 0], [2, 1, 1, 5], [3, 1, 2, 6], [3, 4, 2, 7]]
    deltas = [0] * 32
    for n in range(4):
        prev = paid = 0
        for L in range(4):
            if rows[L][n] > prev:
                deltas[L] += rows[L][n] - prev
                deltas[9 + L] += prev == 0
                deltas[18 + L] += gone[L][n] - paid
                prev, paid = rows[L][n], gone[L][n]
    for limit in (0, 2, 3):
        for want in (1, 3, 4, 5, 8, 9):
            d = deltas[:]
            for row in range(3):
                for L in range(limit + 1, 9):
                    d[9 * row + L] = 0
            assert finish_model(d, limit, want, False) == gg.expected_cells(rows, gone, limit, want), (limit, want)


@pytest.fixture()
def mirror():
    pm = pkg.GpuPredicateManager(device=-1)
    yield pm
    pm.close()


def test_host_argument_errors_need_no_device(mirror):
    mirror.load_snapshot({"nodes": [], "pods": [{"metadata": {"name": "p", "uid": "p", "namespace": "d"}, "spec": {"containers": [{"name": "c"}]}}]})
    with pytest.raises(RuntimeError, match="want below 1"):
        mirror.preempt_headroom([0], wants=[0])
    with pytest.raises(ValueError, match="one want per listed ask"):
        mirror.preempt_headroom([0], wants=[1, 2])
    with pytest.raises(RuntimeError, match="want below 1"):
        mirror.preempt_headroom_by_key("p", 0)
    with pytest.raises(KeyError):
        mirror.preempt_headroom_by_key("no-such-pod", 1)
    for call in (lambda: mirror.preempt_headroom(), lambda: mirror.preempt_headroom_nodes(0), lambda: mirror.preempt_headroom_by_key("p", 2)):
        with pytest.raises(RuntimeError, match="mirror-only"):
            call()
    assert pkg.PREEMPT_HEADROOM_CELLS == gg.CELLS == 32
    assert (pkg.PREEMPT_HEADROOM_COPIES, pkg.PREEMPT_HEADROOM_NODES, pkg.PREEMPT_HEADROOM_VICTIMS) == (gg.COPIES, gg.NODES, gg.VICTIMS)
    assert (pkg.PREEMPT_HEADROOM_STATUS, pkg.PREEMPT_HEADROOM_LIMIT, pkg.PREEMPT_HEADROOM_WANT, pkg.PREEMPT_HEADROOM_LEVEL) == (27, 28, 29, 30)
