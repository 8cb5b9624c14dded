"""The host side the per-ask queries of the engine share, without a device (csrc/engine/ask_tasks.h, plain C++): the partition of a list
of asks into tasks, the two words a node-sharded engine's ranks compare, and the fix-up of a packed best key — on hand-made tables
against a Python restatement, run by tests/c/ask_tasks.cpp, a stand-alone program built under AddressSanitizer + UBSan and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_PIN = -1
SEED, PRIME, M64 = 0x9e3779b97f4a7c15, 0x100000001b3, (1 << 64) - 1
PODS_MAX = (1 << 28) - 1   # kReachPodsMax
NO_NODE = 0x7f7f7f7f7f7f7f7f   # what the best-key column is seeded with


def partition_model(spec, pin, asks, extra, sharded, by_ask):
    """Tasks by first appearance: keyed by (spec, pin); by ask index for a pinned ask of a sharded engine and throughout under by_ask;
    and by the extra value beside either."""
    index, task_of, t_spec, t_pin, extra_of = {}, [], [], [], []
    for i, a in enumerate(asks):
        key = ("ask", a) if by_ask or (sharded and pin[a] != NO_PIN) else (spec[a], pin[a])
        key += (extra[i] & 15,) if extra is not None else ()
        if key not in index:
            index[key] = len(t_spec)
            t_spec.append(spec[a])
            t_pin.append(pin[a])
            extra_of += [extra[i]] if extra is not None else []
        task_of.append(index[key])
    return task_of, t_spec, t_pin, extra_of


def fnv(values):
    h = SEED
    for v in values:
        h = ((h ^ (v & 0xffffffff)) * PRIME) & M64
    return h


def fixup_model(row, at, key, limit):
    row, level = list(row), key >> 59
    if row[at] != 0:
        row = [0] * len(row)
        row[at], row[at + 3] = 1, -1
    elif 1 <= level <= 8:
        row[at + 2], row[at + 3], row[at + 4] = level, key & 0x7fffffff, (key >> 31) & PODS_MAX
    else:
        row[at + 3] = -1
    row[at + 1] = limit
    return row


#        pod  0       1       2       3  4       5  6  7       8
SPEC = [0, 0, 1, 1, 2, 2, 2, 3, 1]
PIN = [NO_PIN, NO_PIN, NO_PIN, 4, NO_PIN, 7, 9, NO_PIN, 4]
OTHER_SPEC = [0, 1, 1, 1, 2, 2, 2, 3, 1]   # another rank's spec table: pod 1 merged with pod 2 instead of pod 0

PARTITIONS = {   # name: (spec table, asks, extra, sharded, by_ask)
    "repeats": (SPEC, [0, 1, 0, 2, 2, 0, 7, 1], None, False, False),
    "one spec, three pins": (SPEC, [4, 5, 6, 5], None, False, False),
    "two pods, one spec and pin": (SPEC, [3, 8, 3], None, False, False),
    "limits 0..8": (SPEC, [0] * 9 + [1] * 9 + [2], list(range(9)) + list(range(8, -1, -1)) + [4], False, False),
    "sharded: pinned asks alone, siblings merge": (SPEC, [2, 3, 8, 3, 0, 5, 1, 4, 6, 2], None, True, False),
    "sharded, limits": (SPEC, [3, 3, 0, 1, 0], [2, 5, 1, 1, 7], True, False),
    "by ask": (SPEC, [0, 1, 0, 2, 1], None, False, True),
    "by ask, sharded, limits": (SPEC, [0, 0, 1, 3, 3], [3, 8, 3, 0, 0], True, True),
    "empty": (SPEC, [], None, False, False),
    "empty, limits": (SPEC, [], [], True, False),
    "a, b, c": (SPEC, [0, 1, 2], None, False, False),
    "a, c, b": (SPEC, [0, 2, 1], None, False, False),
    "a, b, c on the other table": (OTHER_SPEC, [0, 1, 2], None, False, False),
}
KEYS = {   # name: (key, status cell as it arrives)
    "no node": (NO_NODE, 0),
    "level 1": ((1 << 59) | (PODS_MAX << 31) | 0x7fffffff, 0),
    "level 8": ((8 << 59) | (PODS_MAX << 31) | 0x7fffffff, 0),
    "level 3, node 0, no pods": (3 << 59, 0),
    "unsupported on two shards": (NO_NODE, 2),
    "unsupported on one, a key from the other": ((2 << 59) | (5 << 31) | 17, 1),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ask_tasks") / "ask_tasks")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + san + [os.path.join(ROOT, "tests", "c", "ask_tasks.cpp"), "-o", exe])
    return exe


def run(program, tmp_path, lines):
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(str(x) for x in line) + "\n" for line in lines))
    out = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert out.returncode == 0 and out.stdout.endswith("ask tasks ok\n"), (out.stdout[-500:], out.stderr[-3000:])
    got = [[int(x) for x in line.split()] for line in out.stdout.splitlines()[:-1]]
    assert len(got) == len(lines)
    return got


def test_partition_and_agreement_words_under_the_sanitizers(program, tmp_path):
    names = list(PARTITIONS)
    lines = [["P", int(sharded), int(by_ask), int(extra is not None), len(spec)] + spec + PIN + [len(asks)] + asks + (extra or [])
             for spec, asks, extra, sharded, by_ask in PARTITIONS.values()]
    got = dict(zip(names, run(program, tmp_path, lines)))
    tasks, words = {}, {}
    for name, (spec, asks, extra, sharded, by_ask) in PARTITIONS.items():
        task_of, t_spec, t_pin, extra_of = partition_model(spec, PIN, asks, extra, sharded, by_ask)
        want = [len(t_spec)] + task_of + t_spec + t_pin + [len(extra_of)] + extra_of + [fnv(asks), fnv(task_of)]
        assert got[name] == want, (name, got[name], want)
        tasks[name], words[name] = len(t_spec), tuple(want[-2:])
    # the shapes the cases were made for, stated once more by hand
    assert tasks["repeats"] == 3 and tasks["one spec, three pins"] == 3 and tasks["two pods, one spec and pin"] == 1 and tasks["limits 0..8"] == 10
    assert partition_model(*PARTITIONS["limits 0..8"][:1], PIN, *PARTITIONS["limits 0..8"][1:])[3] == list(range(9)) + [4]
    assert got["sharded: pinned asks alone, siblings merge"][1:11] == [0, 1, 2, 1, 3, 4, 3, 5, 6, 0]   # (3 and 8 apart, 0 and 1 together)
    assert tasks["by ask"] == 3 and tasks["by ask, sharded, limits"] == 4 and tasks["empty"] == tasks["empty, limits"] == 0
    assert words["empty"] == (SEED, SEED)
    # two asks swap: both words move; one ask moves to another task: the list word stays, the partition word moves
    assert words["a, b, c"][0] != words["a, c, b"][0] and words["a, b, c"][1] != words["a, c, b"][1]
    assert words["a, b, c"][0] == words["a, b, c on the other table"][0] and words["a, b, c"][1] != words["a, b, c on the other table"][1]


def test_best_key_fixup_under_the_sanitizers(program, tmp_path):
    cells = 16
    listed = [(name, at, limit) for name in KEYS for at, limit in ((10, 8), (3, 0))]   # (the cells of ykpred_preempt_reach, of _victims)
    rows = {name: [100 + c for c in range(cells)] for name in KEYS}
    lines = []
    for name, at, limit in listed:
        row = list(rows[name])
        row[at:at + 5] = [KEYS[name][1], 0, 0, 0, 0]   # (the kernel leaves the five cells to the host; [at] counts the refusing shards)
        lines.append(["K", cells, at, KEYS[name][0], limit] + row)
    for (name, at, limit), line, got in zip(listed, lines, run(program, tmp_path, lines)):
        assert got == fixup_model(line[5:], at, KEYS[name][0], limit), (name, at, got)
        best = got[at + 2:at + 5]
        if name in ("level 1", "level 8"):
            assert best == [int(name[-1]), 0x7fffffff, PODS_MAX] and got[:at] == line[5:5 + at]
        elif name == "no node":
            assert best == [0, -1, 0] and got[at] == 0 and got[:at] == line[5:5 + at]
        elif name.startswith("unsupported"):
            assert got == [0] * at + [1, limit, 0, -1, 0] + [0] * (cells - at - 5)
