#!/usr/bin/env python3
"""Measure the in-kernel noise transform against the fp64 reference (tests/_philox_ref.py): max |z_gpu - z_ref| of
mpcd_philox_noise over the cases of tests/test_gpu_philox.py (a) and (b), where it occurs, and how it grows with the
radius. profiles/philox_reference.txt is this tool's output; the tests' bar BAR is 4 x the maximum it prints,
rounded up to one significant digit. Needs a GPU.

    python tools/philox_error.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpc_via_diffusion_model_amd.planner import philox_noise  # noqa: E402
from tests import _philox_ref as R  # noqa: E402

CASES = ((12345, 0, 4096, 4, 64), (0, 0, 1, 1, 4), (7, 100, 5, 3, 28), (0xDEADBEEF00000001, 2 ** 32 - 3, 8, 2, 32),
         (2 ** 64 - 1, 2 ** 40 + 5, 3, 2, 16), (1, 0, 1, 1002, 4))
CASES += tuple((0, cand, 1, 1, 64) for _, cand, _, _ in R.EDGES)


def main():
    print(f"torch {torch.__version__}, HIP {torch.version.hip}, {torch.cuda.get_device_name(0)}")
    worst = 0.0
    for case in CASES:
        seed, goff, n, k, flat = case
        got = philox_noise(n, k, flat, seed=seed, global_offset=goff)
        torch.cuda.synchronize()
        got = got.cpu().double().numpy()
        ref = R.ref_noise(*case)
        err = np.abs(got - ref)
        at = np.unravel_index(np.argmax(err), err.shape)
        words = R.raw_words(*case)
        u = [float(v[at[0], at[1], at[2] // 4]) for v in R.uniforms(words)]
        print(f"seed={seed:#x} offset={goff:#x} {n} cand x {k} slices x {flat}: finite={bool(np.isfinite(got).all())} "
              f"max|z|={np.abs(got).max():.6f} max err={err.max():.4e} rms err={np.sqrt((err ** 2).mean()):.3e}\n"
              f"    at [slice, cand, elem]={tuple(int(i) for i in at)} gpu={float(got[at])!r} ref={float(ref[at])!r} "
              f"words={[int(x) for x in words[at[0], at[1], at[2] // 4]]} u={u}")
        worst = max(worst, float(err.max()))
        if got.size > 100000:  # where the error comes from: the angle's fp32 rounding scales with the radius
            r = np.hypot(ref[..., 0::2], ref[..., 1::2])
            e2 = np.maximum(err[..., 0::2], err[..., 1::2])
            for lo, hi in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 7)):
                m = (r >= lo) & (r < hi)
                print(f"    radius [{lo}, {hi}): {int(m.sum())} pairs, max err {e2[m].max() if m.any() else 0:.3e}")
            ur = np.abs(np.hypot(got[..., 0::2], got[..., 1::2]) - r)
            print(f"    error of the radius alone: max {ur.max():.3e}, relative {np.max(ur / np.maximum(r, 1e-30)):.3e}")
    print(f"maximum over all cases: {worst:.4e}; x 4 = {4 * worst:.3e}")


if __name__ == "__main__":
    main()
