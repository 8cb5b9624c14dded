#!/usr/bin/env python3
"""Writes tests/golden/go_patch_preimages.json: for every file that integration/patches/*.diff edits, its line count in the
reference (apache/yunikorn-k8shim at the version the patches target) and the SHA-256 of the lines each hunk replaces, read
from the reference at the hunk's own position. No source text is stored, only what
tests/test_abi_symbols.py::test_go_patches_apply_to_the_reference needs to show that every hunk meets exactly these lines.

Usage: python tests/golden/make_go_patch_preimages.py <reference checkout>
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATCHES = os.path.join(ROOT, "integration", "patches")
OUT = os.path.join(HERE, "go_patch_preimages.json")
HUNK = re.compile(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@")


def digest(lines):
    return hashlib.sha256("".join(line + "\n" for line in lines).encode()).hexdigest()


def hunks(diff_text):
    """(target path, [(old_start, old_len, new_start, new_len, pre-image lines, post-image lines)]) of a one-file unified diff."""
    target, out, cur = None, [], None
    for line in diff_text.split("\n"):
        if line.startswith("--- a/"):
            target = line[len("--- a/"):]
            continue
        if line.startswith("+++ "):
            continue
        m = HUNK.match(line)
        if m:
            cur = [int(m.group(1)), int(m.group(2) or 1), int(m.group(3)), int(m.group(4) or 1), [], []]
            out.append(cur)
        elif cur is not None and line[:1] in (" ", "-", "+"):
            if line[0] != "+":
                cur[4].append(line[1:])
            if line[0] != "-":
                cur[5].append(line[1:])
    return target, [tuple(h) for h in out]


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    ref = sys.argv[1]
    files = {}
    for name in sorted(n for n in os.listdir(PATCHES) if n.endswith(".diff")):
        target, hs = hunks(open(os.path.join(PATCHES, name)).read())
        text = open(os.path.join(ref, target)).read().split("\n")
        if text and text[-1] == "":
            text.pop()
        files[name] = {"target": target, "lines": len(text),
                       "hunks": [{"old_start": s, "old_len": n, "sha256": digest(text[s - 1:s - 1 + n])} for s, n, *_ in hs]}
    with open(OUT, "w") as f:
        json.dump(files, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
