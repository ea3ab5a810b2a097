"""An independent reference of the samplers' noise stream (include/mpcd.h: "Philox4x32-10 keyed by seed, global
candidate index, slice, element quad"), in plain numpy.

philox4x32_10 is written from Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11),
section 3.2 / the Random123 reference: a round multiplies counter words 0 and 2 by two fixed 32-bit constants,
keeps the 64-bit products' halves, and mixes the high halves with counter words 1 and 3 and the key; the key is
bumped by two Weyl constants after every round. tests/test_philox_ref_host.py holds it to Random123's known answers.

ref_noise is the project's use of it: the counter and key layout, the uint32 -> (0, 1] / [0, 1] uniforms formed in
fp32 exactly as the kernels form them (they are inputs of the transform, and fp32 rounding decides edge cases such
as u0 == 1), then the Box-Muller transform in fp64: the high-precision reference of what the kernels compute with
fp32 angles and fast intrinsics.
"""
import functools
import math

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85  # Weyl key increments (golden ratio, sqrt(3) - 1)
_MASK = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)

# |z| <= sqrt(-2 ln 2^-32): the smallest u0 is 2^-32
Z_MAX = math.sqrt(64.0 * math.log(2.0))


def philox4x32_10(counter_words, key_words, rounds=10):
    """counter_words: four, key_words: two uint64 arrays (or ints) of 32-bit values, broadcast against each other.
    Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(w, dtype=np.uint64) & _MASK for w in counter_words)
    k0, k1 = (np.asarray(w, dtype=np.uint64) & _MASK for w in key_words)
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _SH, p0 & _MASK, p1 >> _SH, p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _MASK, (k1 + np.uint64(PHILOX_W1)) & _MASK
    return c0, c1, c2, c3


def raw_words(seed, global_offset, n_cand, n_slices, flat):
    """uint32 [n_slices][n_cand][flat / 4][4]: the four Philox words of every (slice, candidate, element quad).
    counter = (quad, cand & 0xffffffff, cand >> 32, slice), key = (seed & 0xffffffff, seed >> 32), cand =
    global_offset + the candidate's index in the call."""
    assert flat >= 4 and flat % 4 == 0 and n_cand >= 1 and n_slices >= 1
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cand = np.uint64(int(global_offset)) + np.arange(n_cand, dtype=np.uint64)
    sl = np.arange(n_slices, dtype=np.uint64)[:, None, None]
    quad = np.arange(flat // 4, dtype=np.uint64)[None, None, :]
    cand = cand[None, :, None]
    words = philox4x32_10((quad, cand & _MASK, cand >> _SH, sl), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(np.broadcast_arrays(*words), axis=-1).astype(np.uint32)


def uniforms(words):
    """fp32 (u0, u1, u2, u3) of raw words [..., 4]: u0, u2 in (0, 1] ((r + 1) 2^-32), u1, u3 in [0, 1] (r 2^-32),
    each conversion, add and product rounded to fp32 (numpy's uint32 -> float32 rounds to nearest even)."""
    f = words.astype(np.float32)
    s, one = np.float32(2.0 ** -32), np.float32(1.0)
    return (f[..., 0] + one) * s, f[..., 1] * s, (f[..., 2] + one) * s, f[..., 3] * s


def ref_noise(seed, global_offset, n_cand, n_slices, flat):
    """float64 [n_slices][n_cand][flat]: elements 4q .. 4q + 3 of a row are sqrt(-2 ln u0) (cos, sin)(2 pi u1),
    sqrt(-2 ln u2) (cos, sin)(2 pi u3) of quad q's words, in fp64 from the fp32 uniforms."""
    u0, u1, u2, u3 = (u.astype(np.float64) for u in uniforms(raw_words(seed, global_offset, n_cand, n_slices, flat)))
    ra, rb = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    ta, tb = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=-1)
    return z.reshape(n_slices, n_cand, flat)


@functools.lru_cache(maxsize=16)
def shared_ref_noise(seed, global_offset, n_cand, n_slices, flat):
    """ref_noise computed once per case and shared between the tests that need it (read-only)"""
    z = ref_noise(seed, global_offset, n_cand, n_slices, flat)
    z.setflags(write=False)
    return z


def _lag1(a, axis):
    """Pearson correlation of neighbours along axis, times sqrt(number of pairs): ~ N(0, 1) for independent values"""
    n = a.shape[axis]
    x, y = np.take(a, np.arange(n - 1), axis=axis).ravel(), np.take(a, np.arange(1, n), axis=axis).ravel()
    x, y = x - x.mean(), y - y.mean()
    return float((x * y).sum() / math.sqrt((x * x).sum() * (y * y).sum()) * math.sqrt(x.size))


_ndtr = np.frompyfunc(lambda v: 0.5 * math.erfc(-v / math.sqrt(2.0)), 1, 1)


def moments_and_lags(z):
    """Standardised statistics of z [n_slices][n_cand][flat] under the hypothesis "independent N(0, 1)": each of
    mean, var, skew, kurt and the lag-1 correlations lag_{z,z2}_{elem,cand,slice} is ~ N(0, 1); "ks" is the
    Kolmogorov-Smirnov distance to the normal distribution times sqrt(n) (asymptotic 0.1 % point: 1.95)."""
    z = np.asarray(z, dtype=np.float64)
    assert z.ndim == 3
    n = z.size
    v = z.ravel()
    d = v - v.mean()
    m2, m3, m4 = (d ** 2).mean(), (d ** 3).mean(), (d ** 4).mean()
    out = {"mean": float(v.mean() * math.sqrt(n)), "var": float((m2 - 1.0) * math.sqrt(n / 2.0)),
           "skew": float(m3 / m2 ** 1.5 * math.sqrt(n / 6.0)), "kurt": float((m4 / m2 ** 2 - 3.0) * math.sqrt(n / 24.0))}
    for name, axis in (("elem", 2), ("cand", 1), ("slice", 0)):
        if z.shape[axis] > 1:
            out[f"lag_z_{name}"] = _lag1(z, axis)
            out[f"lag_z2_{name}"] = _lag1(z * z, axis)
    cdf = _ndtr(np.sort(v)).astype(np.float64)
    i = np.arange(n, dtype=np.float64)
    out["ks"] = float(max((cdf - i / n).max(), ((i + 1.0) / n - cdf).max()) * math.sqrt(n))
    return out


# the bounds of the statistics above (conditions, not measurements): a two-sided normal tail of 7e-6 per
# standardised moment or correlation, the asymptotic 0.1 % point of sqrt(n) D
STAT_BOUND, KS_BOUND = 4.5, 1.95


def assert_stats(z, what):
    st = moments_and_lags(z)
    print(what, {k: round(v, 3) for k, v in st.items()})
    bad = {k: v for k, v in st.items() if (v > KS_BOUND if k == "ks" else abs(v) > STAT_BOUND)}
    assert not bad, f"{what}: statistics outside their bounds (|.| <= {STAT_BOUND}, ks <= {KS_BOUND}): {bad}"
    return st


# Edge inputs of the transform at seed 0, slice 0, flat = 64 (quads 0 .. 15), found by tools/philox_edges.py over
# candidates 0 .. 2^22: (kind, candidate, quad, word). "u0_one": word 0 / 2 >= 2^32 - 128, so float32(r) = 2^32 and
# u0 = 1.0 (radius sqrt(-0)); "u1_one": word 1 / 3 likewise, the angle is fp32 2 pi; "u0_min": the smallest u0
# found (r = 1: radius 6.5555); "u1_min": the angle next to 0 (r = 29); "u0_below_one": word 0 / 2 in
# [2^32 - 384, 2^32 - 128), u0 = 1 - 2^-24, the largest below 1 and the smallest non-zero radius (3.45e-4): a fast
# logarithm with a positive last-bit error there would make the radius NaN.
EDGES = (("u0_one", 58585, 12, 0), ("u0_one", 1260597, 6, 0), ("u0_one", 3570461, 8, 2),
         ("u1_one", 507113, 13, 3), ("u1_one", 2662490, 3, 3), ("u1_one", 3052028, 9, 1), ("u1_one", 3207180, 14, 1),
         ("u0_min", 3441155, 14, 2), ("u1_min", 2317303, 5, 1),
         # the smallest word 0 (r = 16: radius 6.2205) and word 3 (r = 144): u0 and u2, u1 and u3 are formed by
         # separate statements in the kernels, so each word position has its own small-value edge
         ("u0_min", 3474781, 1, 0), ("u1_min", 2664212, 0, 3),
         ("u0_below_one", 67566, 3, 0), ("u0_below_one", 921823, 0, 2))
EDGE_RAW = {58585: 4294967267, 3441155: 1, 2317303: 29, 3474781: 16, 2664212: 144}  # the raw word, where recorded
