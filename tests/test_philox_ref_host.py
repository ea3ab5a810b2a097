"""CPU: the Philox reference of tests/_philox_ref.py checks itself, so that tests/test_gpu_philox.py compares the
kernels with something known to be right: Random123's known answers for Philox4x32-10, the edge counters the GPU
test aims at (their raw words really are what the record says), and the distribution of the reference stream under
the project's counter layout (moments, lag-1 correlations along every axis, Kolmogorov-Smirnov)."""
import numpy as np
import pytest

from . import _philox_ref as R

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key, output
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


@pytest.mark.parametrize("ctr,key,want", KAT, ids=("zeros", "ones", "pi"))
def test_random123_known_answers(ctr, key, want):
    got = tuple(int(w) for w in R.philox4x32_10(ctr, key))
    assert got == want, [hex(w) for w in got]


def test_known_answers_vectorised():
    """the same three through one broadcast call: array inputs are what ref_noise uses"""
    ctr = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = np.stack(R.philox4x32_10(ctr, key), axis=-1)
    assert got.dtype == np.uint64 and (got == np.array([k[2] for k in KAT], dtype=np.uint64)).all()


def test_counter_and_key_layout():
    """raw_words places (quad, cand lo, cand hi, slice) and (seed lo, seed hi) where include/mpcd.h says"""
    seed, goff = 0xDEADBEEF00000001, 2 ** 32 - 3
    w = R.raw_words(seed, goff, 8, 3, 32)
    assert w.shape == (3, 8, 8, 4) and w.dtype == np.uint32
    for k, b, q in ((0, 0, 0), (2, 2, 7), (1, 3, 5), (2, 7, 1)):  # candidates below, at and above the carry
        cand = goff + b
        want = R.philox4x32_10((q, cand & 0xffffffff, cand >> 32, k), (seed & 0xffffffff, seed >> 32))
        assert tuple(int(x) for x in want) == tuple(int(x) for x in w[k, b, q]), (k, b, q)
    # the high words matter: another high candidate word or high seed word is another stream
    assert not (R.raw_words(seed, 2 ** 32, 1, 1, 4) == R.raw_words(seed, 0, 1, 1, 4)).any()
    assert not (R.raw_words(seed, 5, 1, 1, 4) == R.raw_words(seed & 0xffffffff, 5, 1, 1, 4)).any()
    # slice and quad are different counter words
    assert not (R.raw_words(1, 0, 1, 2, 8)[1, 0, 0] == R.raw_words(1, 0, 1, 2, 8)[0, 0, 1]).all()


def test_uniform_mapping():
    w = np.array([[0, 0, 2 ** 32 - 1, 2 ** 32 - 1], [2 ** 32 - 129, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 128],
                  [1, 29, 2 ** 31, 2 ** 31]], dtype=np.uint32)
    u0, u1, u2, u3 = R.uniforms(w)
    assert all(u.dtype == np.float32 for u in (u0, u1, u2, u3))
    assert u0[0] == np.float32(2.0 ** -32) and u1[0] == 0.0 and u2[0] == 1.0 and u3[0] == 1.0
    # float32(2^32 - 129) = 2^32 - 256 (and + 1 rounds back to it); 2^32 - 128 is the tie that rounds to 2^32
    assert u0[1] == np.float32(1 - 2.0 ** -24) and u1[1] == np.float32(1 - 2.0 ** -24) and u2[1] == 1.0 and u3[1] == 1.0
    assert u0[2] == np.float32(2.0 ** -31) and u1[2] == np.float32(29 * 2.0 ** -32) and u3[2] == 0.5
    assert u2[2] == np.float32(0.5)  # 2^31 + 1 is not an fp32 number
    z = R.ref_noise(0, 0, 2, 2, 8)
    assert z.shape == (2, 2, 8) and z.dtype == np.float64 and np.isfinite(z).all()


@pytest.mark.parametrize("kind,cand,quad,word", R.EDGES, ids=lambda v: str(v))
def test_edge_counters_are_edges(kind, cand, quad, word):
    """the GPU test calls these candidates to hit the transform's edge inputs: they must really be there"""
    w = R.raw_words(0, cand, 1, 1, 64)[0, 0]
    r = int(w[quad, word])
    u = R.uniforms(w)[word][quad]
    if cand in R.EDGE_RAW:
        assert r == R.EDGE_RAW[cand]
    z = R.ref_noise(0, cand, 1, 1, 64)[0, 0]
    assert np.isfinite(z).all()
    pair = z[4 * quad + (word & 2):4 * quad + (word & 2) + 2]
    if kind == "u0_one":
        assert word in (0, 2) and r >= 2 ** 32 - 128 and u == 1.0
        assert (pair == 0.0).all(), "radius sqrt(-2 ln 1) = 0: both outputs of the pair are zero"
    elif kind == "u1_one":
        assert word in (1, 3) and r >= 2 ** 32 - 128 and u == 1.0
    elif kind == "u0_min":
        assert word in (0, 2) and r in (1, 16) and u == np.float32((r + 1) * 2.0 ** -32)
        assert abs(np.hypot(*pair) - {1: 6.5555, 16: 6.2205}[r]) < 1e-4  # sqrt(2 (32 ln 2 - ln(r + 1)))
    elif kind == "u0_below_one":
        assert word in (0, 2) and 2 ** 32 - 384 <= r < 2 ** 32 - 128 and u == np.float32(1 - 2.0 ** -24)
        assert abs(np.hypot(*pair) - np.sqrt(-2 * np.log1p(-2.0 ** -24))) < 1e-12 and np.hypot(*pair) > 3.4e-4
    else:
        assert kind == "u1_min" and word in (1, 3) and r in (29, 144) and u == np.float32(r * 2.0 ** -32)


SEEDS = (12345, 0xDEADBEEF00000001)


def _bulk(seed):
    return R.shared_ref_noise(seed, 0, 4096, 4, 64)


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_reference_stream_is_standard_normal(seed):
    """n = 2^20 values: every standardised moment and lag-1 correlation within 4.5, sqrt(n) D within 1.95"""
    z = _bulk(seed)
    assert z.shape == (4, 4096, 64) and np.isfinite(z).all() and np.abs(z).max() <= R.Z_MAX
    st = R.assert_stats(z, f"reference, seed {seed:#x}")
    assert set(st) == {"mean", "var", "skew", "kurt", "ks"} | {f"lag_{a}_{b}" for a in ("z", "z2")
                                                                 for b in ("elem", "cand", "slice")}


def test_statistics_reject_broken_streams():
    """moments_and_lags is the GPU test's guard: it must flag what it is there for"""
    z = _bulk(SEEDS[0])

    def rejected(bad):
        st = R.moments_and_lags(bad)
        return [k for k, v in st.items() if (v > R.KS_BOUND if k == "ks" else abs(v) > R.STAT_BOUND)]

    rep = z.copy()
    rep[1] = rep[0]  # a slice repeated
    assert "lag_z_slice" in rejected(rep)
    rep = z.copy()
    rep[:, 1::2] = rep[:, 0::2]  # candidates repeated in pairs
    assert "lag_z_cand" in rejected(rep)
    assert "var" in rejected(z * 1.01) and "ks" in rejected(z + 0.01)
    assert "kurt" in rejected(np.clip(z, -3.0, 3.0))  # a cut tail
    with pytest.raises(AssertionError):
        R.assert_stats(z * 1.01, "scaled")
