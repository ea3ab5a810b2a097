#!/usr/bin/env python3
"""Search the reference noise stream (tests/_philox_ref.py) for counters that hit the Box-Muller transform's edge
inputs: the table EDGES of that module, which tests/test_philox_ref_host.py verifies and tests/test_gpu_philox.py
aims the kernel at. CPU only, about 15 s for the default range.

    python tools/philox_edges.py [--seed 0] [--cands 4194304] [--flat 64]

Prints (kind, candidate, quad, word, raw word) for slice 0:
  u0_one  word 0 / 2 >= 2^32 - 128: float32(r) = 2^32, u0 = 1.0, radius sqrt(-0)
  u1_one  word 1 / 3 >= 2^32 - 128: u1 = 1.0, the angle is fp32 2 pi
  u0_below_one  word 0 / 2 in [2^32 - 384, 2^32 - 128): u0 = 1 - 2^-24, the largest below 1 (the smallest radius:
          a logarithm with a positive last-bit error there would make the radius NaN)
  u0_min  the smallest word 0 and the smallest word 2 found (the largest radii)
  u1_min  the smallest non-zero word 1 and word 3 found (the angles next to 0)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _philox_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0)
    ap.add_argument("--cands", type=int, default=1 << 22)
    ap.add_argument("--flat", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    a = ap.parse_args()
    ones, lo = [], {}
    for c0 in range(0, a.cands, a.chunk):
        n = min(a.chunk, a.cands - c0)
        w = R.raw_words(a.seed, c0, n, 1, a.flat)[0]  # [n][quads][4]
        for b, q, k in zip(*np.nonzero(w >= 2 ** 32 - 128)):
            ones.append(("u0_one" if k in (0, 2) else "u1_one", c0 + int(b), int(q), int(k), int(w[b, q, k])))
        # float32(r) = 2^32 - 256 for r in [2^32 - 384, 2^32 - 128), and + 1 rounds back to it: u0 = 1 - 2^-24
        for b, q, k in zip(*np.nonzero((w >= 2 ** 32 - 384) & (w < 2 ** 32 - 128) & (np.arange(4) % 2 == 0))):
            ones.append(("u0_below_one", c0 + int(b), int(q), int(k), int(w[b, q, k])))
        # per word: u0 and u2 (likewise u1 and u3) are formed by separate statements in the kernels
        for kind, k, floor in (("u0_min", 0, 0), ("u0_min", 2, 0), ("u1_min", 1, 1), ("u1_min", 3, 1)):
            v = np.where(w[:, :, k] >= floor, w[:, :, k], np.uint32(0xffffffff))
            b, q = np.unravel_index(np.argmin(v), v.shape)
            hit = (kind, c0 + int(b), int(q), k, int(v[b, q]))
            if (kind, k) not in lo or hit[4] < lo[kind, k][4]:
                lo[kind, k] = hit
    for row in sorted(ones) + [lo[key] for key in sorted(lo)]:
        print(row)


if __name__ == "__main__":
    main()
