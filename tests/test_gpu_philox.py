"""GPU: the in-kernel noise stream against an independent reference (tests/_philox_ref.py, checked on the CPU by
tests/test_philox_ref_host.py).

a. mpcd_philox_noise against the fp64 reference, elementwise, at shapes that catch index arithmetic, 64-bit candidate
   indices (a carry into the high counter word inside one call), high seed words and large slice numbers;
b. the Box-Muller transform's edge inputs (u0 == 1, u1 == 1, u0 = 1 - 2^-24, the smallest u0 and the angle next to
   0 in either word position) hit on purpose;
c. every in-kernel draw site equals that materialised stream bit for bit: a seeded cold run is its injected replay,
   with candidates that straddle 2^32 and a seed with a high word, for every kernel family and forced layout;
d. one call across the carry equals the two calls split at 2^32;
e. the distribution of the GPU stream (moments, lag-1 correlations, Kolmogorov-Smirnov);
f. mpcd_philox_noise's argument refusals.

The elementwise bar BAR: the transform runs in fp32 with the fast intrinsics (__logf, __cosf, __sinf), so it differs
from the fp64 reference by the fp32 rounding of the angle (up to 2 pi: 2.4e-7 per rounded product) times a radius of
up to 6.66, plus the intrinsics' own error: a few 1e-6 expected. Measured on an MI355X over the cases of (a) and (b):
profiles/philox_reference.txt; BAR is 4 times that maximum, rounded up to one significant digit (another ROCm's
intrinsics, inputs the sample missed), and may not exceed the project's elementwise parity bar ABS_ELEM = 1e-4. A
structural error (a wrong word, multiplier or round count) moves values by O(1).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec
from mpc_via_diffusion_model_amd import _native as nat
from mpc_via_diffusion_model_amd.planner import force_mlp_layout, force_unet_path, philox_noise

from . import _philox_ref as R
from ._util import ABS_ELEM, make_mlp, make_unet
from .test_gpu_warm_start import _inputs, _run, _same

pytestmark = pytest.mark.gpu

# measured maximum 1.7518e-06 (bulk case, slice 1, candidate 4023, element 60: radius 4.14); x 4 = 7.01e-06
BAR = 8e-6
assert BAR <= ABS_ELEM, "a transform that needs more than the project's parity bar is a defect of the transform"

# (seed, global_offset, n_cand, n_slices, flat)
BULK = (12345, 0, 4096, 4, 64)
CASES = (BULK,
         (0, 0, 1, 1, 4),                              # one quad
         (7, 100, 5, 3, 28),                           # seven quads per row: the output index arithmetic
         (0xDEADBEEF00000001, 2 ** 32 - 3, 8, 2, 32),  # a carry into the high candidate word, a high seed word
         (2 ** 64 - 1, 2 ** 40 + 5, 3, 2, 16),
         (1, 0, 1, 1002, 4))                           # slice numbers beyond any real chain
SEED, GOFF = 0xDEADBEEF00000001, 2 ** 32 - 3  # (c): candidates GOFF .. GOFF + 20 straddle the carry


@functools.lru_cache(maxsize=None)
def _gpu_noise(seed, goff, n_cand, n_slices, flat):
    z = philox_noise(n_cand, n_slices, flat, seed=seed, global_offset=goff)
    torch.cuda.synchronize()
    assert z.shape == (n_slices, n_cand, flat) and z.dtype == torch.float32
    z = z.cpu().double().numpy()
    z.setflags(write=False)
    return z


def _worst(got, ref):
    err = np.abs(got - ref)
    at = np.unravel_index(np.argmax(err), err.shape)
    return float(err[at]), tuple(int(i) for i in at)


# ------------------------------------------------------------------- a. the stream against the reference
@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%x_off%x_%dx%dx%d" % c)
def test_noise_matches_reference(case):
    got, ref = _gpu_noise(*case), R.shared_ref_noise(*case)
    assert np.isfinite(got).all(), "non-finite noise"
    assert np.abs(got).max() <= R.Z_MAX + BAR, f"|z| = {np.abs(got).max()} is outside the transform's range"
    err, at = _worst(got, ref)
    print(f"max |z_gpu - z_ref| = {err:.3e} at [slice, candidate, element] {at}: gpu {got[at]!r}, ref {ref[at]!r}")
    assert err <= BAR, f"differs from the reference by {err:.3e} at [slice, candidate, element] {at}"


# ---------------------------------------------------------------------- b. the transform's edge inputs
@pytest.mark.parametrize("kind,cand,quad,word", R.EDGES, ids=lambda v: str(v))
def test_transform_edges(kind, cand, quad, word):
    got, ref = _gpu_noise(0, cand, 1, 1, 64)[0, 0], R.shared_ref_noise(0, cand, 1, 1, 64)[0, 0]
    lo = 4 * quad + (word & 2)  # the two outputs this word feeds
    print(f"{kind} at candidate {cand}, quad {quad}, word {word}: gpu {got[lo:lo + 2]}, ref {ref[lo:lo + 2]}, "
          f"row max err {np.abs(got - ref).max():.3e}")
    assert np.isfinite(got).all(), f"non-finite output in the row of a {kind} input"
    if kind == "u0_one":
        # radius sqrt(-2 ln 1) = sqrt(-0) = -0: a zero of either sign, never NaN
        assert (got[lo:lo + 2] == 0.0).all(), f"u0 == 1.0 must give exact zeros, got {got[lo:lo + 2]}"
    if kind == "u0_below_one":
        # ln(1 - 2^-24) = -5.96e-8 must survive the fast logarithm: radius 3.45e-4, where BAR alone is 2 % of the
        # value. A logarithm flushed to zero or of the wrong sign is off by 100 %; one good to a few fp32 ulps (6e-8
        # each) gives the radius to half of that, so 1e-3 relative separates the two with three decades on each side
        rg, rr = np.hypot(*got[lo:lo + 2]), np.hypot(*ref[lo:lo + 2])
        print(f"radius gpu {rg!r}, ref {rr!r}, relative difference {abs(rg - rr) / rr:.3e}")
        assert abs(rg - rr) <= 1e-3 * rr, f"radius {rg} for u0 = 1 - 2^-24, reference {rr}"
    err, at = _worst(got, ref)
    assert err <= BAR, f"row of a {kind} input differs from the reference by {err:.3e} at element {at}"
    assert np.abs(got).max() <= R.Z_MAX + BAR


# ------------------------------------------------------------------------- e. statistics of the GPU stream
def test_gpu_stream_is_standard_normal():
    R.assert_stats(_gpu_noise(*BULK), "mpcd_philox_noise, bulk case")


# --------------------------------------------------- c. every draw site is the materialised stream, cold
C, N = 4, 25  # 25 denoise steps: the fewest at which the exponential schedule's fp32 tables are finite
MLP_LAYOUTS = ("32x8", "16x8", "16x4", "rw32", "rw16", "rw32x8")
# H * d = 32: the final layer is one n-tile per wave (NZT == 1 in mlp_rw.hip / mlp_h2.hip, so STAGED_NOISE), and the
# 4-wave resident-weight kernels (rw32, rw16) and the two-term fp16 kernel draw step 0 with fetch_noise and every later
# step with the staged ph_init / ph_step copy of the generator. H * d = 128: two n-tiles per wave (NZT == 2), every
# step's draw is fetch_noise; an f16x2 net is outside its fp16 kernel there (H * d 32 / 64 only) and runs the
# split-bf16 kernel of its batch's layout. The exact-f32 and streaming split-bf16 kernels (mlp_sampler.hip,
# mlp_x3.hip) and the 8-wave rw32x8 (waves 4-7 draw for waves 0-3) call fetch_noise for every step at both shapes.
MLP_SHAPES = ((16, 2), (64, 2))
# (kind, H, d): the layered U-Net at test_gpu_warm_start.py's small shape, the whole-network launch at H = 32
UNET_SMALL, UNET_FUSED = (8, 2), (32, 1)


@functools.lru_cache(maxsize=None)
def _plan(kind, dtype, H, d):
    net = make_unet(d, C, seed=7) if kind == "unet" else make_mlp(d, H, C, seed=21)
    return DiffusionMPC(NetSpec(kind, d, H, C, dtype=dtype), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=N)


def _assert_seeded_is_replay(plan, B, H, d, group=None, layout="auto", unet_path="auto", what="", **kw):
    """a seeded run == the run with noise = philox_noise(the same seed and offset) injected: chain, sample, maxima"""
    S = plan.n_denoise_steps(kw.get("sample_fn", "ddpm_cfg"), kw.get("n_wo_noise", 0), kw.get("ddim_steps"))
    ctx = _inputs(B, H, d, group, 1, 1)[0]
    nz = philox_noise(B, S + 1, H * d, seed=SEED, global_offset=GOFF).view(S + 1, B, H, d)
    try:
        force_mlp_layout(layout)
        force_unet_path(unet_path)
        got = _run(plan, ctx, B, H, d, group, seed=SEED, global_offset=GOFF, **kw)
        want = _run(plan, ctx, B, H, d, group, noise=nz, **kw)
    finally:
        force_mlp_layout("auto")
        force_unet_path("auto")
    assert got[0].shape == (S + 1, B, H, d) and torch.isfinite(got[0]).all(), what
    assert _same(got[0][0], nz[0]), f"chain[0] is not slice 0 of the stream ({what})"
    for a, b, name in zip(got, want, ("chain", "final sample", "chain maxima")):
        if not _same(a, b):
            first = int((a.view(torch.int32) != b.view(torch.int32)).flatten().nonzero()[0])
            raise AssertionError(f"{name}: the seeded run is not its injected replay ({what}); first difference at flat "
                                 f"index {first} of shape {tuple(a.shape)}")


@pytest.mark.parametrize("nwo", (0, 2))
@pytest.mark.parametrize("H,d", MLP_SHAPES)
# f16x2: its fp16 kernel takes 16-row workgroups under "auto" at this batch (and "rw16"), 32-row ones under "rw32"
@pytest.mark.parametrize("dtype,layout", (("f32", "auto"), ("f16x2", "auto"), ("f16x2", "rw32"))
                         + tuple(("f32x3", lay) for lay in MLP_LAYOUTS))
def test_mlp_draw_sites_replay(dtype, layout, H, d, nwo):
    plan = _plan("mlp", dtype, H, d)
    want = {"f32": "f32", "f32x3": "x3", "f16x2": "h2" if H * d <= 64 else "x3"}[dtype]
    assert plan.mlp_form(21)["kernel"] == want, "this case is meant for another kernel"
    _assert_seeded_is_replay(plan, 21, H, d, layout=layout, n_wo_noise=nwo,
                             what=f"MLP {dtype}, layout {layout}, H*d = {H * d}, n_wo_noise = {nwo}")


@pytest.mark.parametrize("nwo", (0, 2))
@pytest.mark.parametrize("dtype", ("f32", "f32x3", "f16"))
def test_unet_layered_draw_sites_replay(dtype, nwo):
    H, d = UNET_SMALL
    _assert_seeded_is_replay(_plan("unet", dtype, H, d), 21, H, d, unet_path="layered", n_wo_noise=nwo,
                             what=f"layered U-Net {dtype}, n_wo_noise = {nwo}")


@pytest.mark.parametrize("nwo", (0, 2))
def test_unet_fused_draw_site_replays(nwo):
    H, d = UNET_FUSED
    plan = _plan("unet", "f32x3", H, d)
    assert plan.unet_form()["fused"], "this case is meant to take the fused U-Net path"
    _assert_seeded_is_replay(plan, 21, H, d, n_wo_noise=nwo, what=f"fused U-Net, n_wo_noise = {nwo}")


# CFG-DDIM draws x_T only; once per kernel family (the fp16 MLP kernel has no DDIM form)
@pytest.mark.parametrize("kind,dtype,layout,shape", (("mlp", "f32", "auto", (16, 2)), ("mlp", "f32x3", "32x8", (16, 2)),
                                                     ("mlp", "f32x3", "rw32", (64, 2)), ("mlp", "f32x3", "rw32x8", (16, 2)),
                                                     ("unet", "f32", "auto", UNET_SMALL), ("unet", "f32x3", "auto", UNET_FUSED)),
                         ids=lambda v: str(v))
def test_ddim_cfg_draw_sites_replay(kind, dtype, layout, shape):
    H, d = shape
    _assert_seeded_is_replay(_plan(kind, dtype, H, d), 21, H, d, layout=layout, sample_fn="ddim_cfg", ddim_steps=5,
                             what=f"ddim_cfg, {kind} {dtype}, layout {layout}, H*d = {H * d}")


@pytest.mark.parametrize("kind,dtype,shape", (("mlp", "f32x3", (16, 2)), ("mlp", "f32", (16, 2)), ("unet", "f32", UNET_SMALL)),
                         ids=lambda v: str(v))
def test_grouped_candidate_index_stays_global(kind, dtype, shape):
    """context_group: 3 groups of 5 candidates; the counter's candidate index is the call's, not the group's"""
    H, d = shape
    _assert_seeded_is_replay(_plan(kind, dtype, H, d), 15, H, d, group=5, n_wo_noise=2,
                             what=f"grouped (3, 5), {kind} {dtype}")


# ------------------------------------------------------------------------------ d. a shard split at 2^32
def test_noise_shards_across_the_carry():
    one = philox_noise(16, 3, 28, seed=SEED, global_offset=2 ** 32 - 8)
    parts = [philox_noise(8, 3, 28, seed=SEED, global_offset=off) for off in (2 ** 32 - 8, 2 ** 32)]
    assert _same(one, torch.cat(parts, dim=1))
    ref = R.ref_noise(SEED, 2 ** 32 - 8, 16, 3, 28)
    assert np.abs(one.cpu().double().numpy() - ref).max() <= BAR


@pytest.mark.parametrize("kind,dtype,shape", (("mlp", "f32x3", (16, 2)), ("mlp", "f16x2", (16, 2)), ("unet", "f32", UNET_SMALL)),
                         ids=lambda v: str(v))
def test_samplers_shard_across_the_carry(kind, dtype, shape):
    H, d = shape
    plan = _plan(kind, dtype, H, d)
    ctx = _inputs(16, H, d, None, 1, 1)[0]
    one = _run(plan, ctx, 16, H, d, seed=SEED, global_offset=2 ** 32 - 8, n_wo_noise=2)
    parts = [_run(plan, ctx, 8, H, d, seed=SEED, global_offset=off, n_wo_noise=2) for off in (2 ** 32 - 8, 2 ** 32)]
    assert _same(one[0], torch.cat([p[0] for p in parts], dim=1)), "the chain depends on the split at 2^32"
    assert _same(one[1], torch.cat([p[1] for p in parts])) and _same(one[2], torch.cat([p[2] for p in parts]))
    # and the candidates past the carry are not the ones 2^32 below them
    low = _run(plan, ctx, 8, H, d, seed=SEED, global_offset=0, n_wo_noise=2)
    assert not _same(low[0], parts[1][0]), "the high candidate word is ignored"


# ---------------------------------------------------------------------------------------- f. refusals
@pytest.mark.parametrize("what,kw", (("out = NULL", dict(out=None)), ("n_cand < 1", dict(n_cand=0)),
                                     ("n_cand < 0", dict(n_cand=-4)), ("n_slices < 1", dict(n_slices=0)),
                                     ("flat < 4", dict(flat=0)), ("flat = 3", dict(flat=3)),
                                     ("flat % 4 != 0", dict(flat=6)), ("global_offset < 0", dict(global_offset=-1))),
                         ids=lambda v: v if isinstance(v, str) else "")
def test_philox_noise_refusals(what, kw):
    out = torch.full((2, 4, 8), 7.0, device="cuda")  # room for the valid call below
    a = dict(seed=3, global_offset=0, n_cand=4, n_slices=2, flat=8, out=out)
    a.update(kw)
    ptr = ctypes.c_void_p(a["out"].data_ptr()) if a["out"] is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = nat.lib()
    rc = L.mpcd_philox_noise(a["seed"], a["global_offset"], a["n_cand"], a["n_slices"], a["flat"], ptr, stream)
    torch.cuda.synchronize()
    assert rc == -1 and nat._STATUS[rc] == "EINVAL", (what, rc)
    assert L.mpcd_last_error(), what
    assert (out == 7.0).all(), f"{what}: a refused call wrote to out"
    # the same call with valid arguments is taken
    rc = L.mpcd_philox_noise(3, 0, 4, 2, 8, ctypes.c_void_p(out.data_ptr()), stream)
    torch.cuda.synchronize()
    assert rc == 0 and (out != 7.0).all()
