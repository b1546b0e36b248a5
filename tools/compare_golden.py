#!/usr/bin/env python3
"""
Compare the fixtures of two trees:  python tools/compare_golden.py DIR_A DIR_B  (two tests/golden directories).

Every *.npz must hold the same keys and, per key, the same dtype, shape and bytes (the archives themselves differ in
their members' timestamps); every *.json must be the same text.  Reads data only.  Exit status 1 on any difference.
"""

from __future__ import annotations

import glob
import os
import sys

import numpy as np


def names(directory, pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(directory, pattern)))


def compare(dir_a, dir_b):
    bad, arrays = [], 0
    for pattern in ("*.npz", "*.json"):
        if names(dir_a, pattern) != names(dir_b, pattern):
            bad.append(f"{pattern}: {names(dir_a, pattern)} != {names(dir_b, pattern)}")
    for name in names(dir_a, "*.npz"):
        if not os.path.exists(os.path.join(dir_b, name)):
            continue
        a, b = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        if sorted(a.files) != sorted(b.files):
            bad.append(f"{name}: keys differ ({len(a.files)} and {len(b.files)})")
            continue
        for key in a.files:
            x, y = a[key], b[key]
            arrays += 1
            if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                bad.append(f"{name}[{key}]: {x.dtype}{x.shape} and {y.dtype}{y.shape} differ")
    for name in names(dir_a, "*.json"):
        if not os.path.exists(os.path.join(dir_b, name)):
            continue
        with open(os.path.join(dir_a, name)) as fa, open(os.path.join(dir_b, name)) as fb:
            if fa.read() != fb.read():
                bad.append(f"{name}: text differs")
    print(f"{len(names(dir_a, '*.npz'))} npz files ({arrays} arrays), {len(names(dir_a, '*.json'))} json files: "
          + ("identical" if not bad else f"{len(bad)} differences"))
    for line in bad:
        print("  " + line)
    return not bad


if __name__ == "__main__":
    sys.exit(0 if compare(sys.argv[1], sys.argv[2]) else 1)
