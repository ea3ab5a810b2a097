"""GPU: grouped contexts (mpcd_sample_grouped, sample_trajectories(context_group=g), closed_loop(grouped=True)): one
context row per group of g consecutive candidates, so that a closed-loop batch of M plant states keeps the
split-bf16 MLP kernels. Group m of a grouped call must be bit for bit the shared-context call of g candidates with
row m and global_offset m * g (the exact-f32 kernel's bits differ, so a fall-back to it cannot pass), nothing may be
written past a group's or the batch's end, and the results must hold the project's oracle bar. Small shapes: what
can go wrong is the workgroup-to-group mapping (a group smaller than, equal to, ragged against and larger than a
workgroup at 8, 16 and 32 candidates per workgroup), not the size."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
from mpc_via_diffusion_model_amd import _native as nat
from mpc_via_diffusion_model_amd.planner import force_mlp_layout
from oracle import normalizer as onorm
from oracle import sampler as osam
from oracle import schedule as osch
from oracle import systems as osys

from ._util import assert_traj_close, make_mlp, make_unet

pytestmark = pytest.mark.gpu

# 25 denoise steps: the fewest at which the exponential schedule's fp32 tables are finite (below that its last beta
# rounds above 1, alphas_cumprod turns negative and every sample is a NaN, which would compare nothing)
C, N = 4, 25
LAYOUTS = ("auto", "32x8", "16x8", "16x4", "rw32", "rw16", "rw32x8")
# (M groups, group): a single candidate; smaller than any workgroup; one 16-candidate workgroup exactly; ragged at
# both 8 and 16 candidates per workgroup; several workgroups per group
SHAPES = ((3, 1), (3, 5), (2, 16), (3, 20), (2, 40))


@functools.lru_cache(maxsize=None)
def _net(H, d, seed=21):
    return make_mlp(d, H, C, seed=seed)


@functools.lru_cache(maxsize=None)
def _plan(H, d, dtype, cfg=True, n_steps=N):
    spec = NetSpec("mlp", state_dim=d, horizon=H, context_dim=C, cfg=cfg, dtype=dtype)
    return DiffusionMPC(spec, _net(H, d).state_dict(), variance_schedule="exponential", n_diffusion_steps=n_steps)


def _ctx(M, seed=3):
    return torch.rand(M, C, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """torch.equal on the bit patterns: what torch.equal asks, and a NaN equals the same NaN"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run(plan, ctx, B, H, d, group=None, **kw):
    """(chain, final sample, chain maxima) of one sample call"""
    x = torch.full((B, H, d), 7.0, device="cuda")
    am = torch.full((B,), -1.0, device="cuda")
    chain = plan.sample_trajectories(ctx, B, H, return_chain=True, out=x, absmax_out=am, context_group=group, **kw)
    torch.cuda.synchronize()
    return chain, x, am


def _assert_groups_equal_shared_calls(plan, M, g, H, d, layout, sample_fn="ddpm_cfg", nwo=0, injected=False, seed=7):
    B = M * g
    ctx = _ctx(M)
    steps = plan.n_denoise_steps(sample_fn, nwo)
    noise = torch.randn(steps + 1, B, H, d, generator=torch.Generator().manual_seed(11)).cuda() if injected else None
    kw = dict(sample_fn=sample_fn, n_wo_noise=nwo, seed=seed, w=0.01)
    try:
        force_mlp_layout(layout)
        chain, x, am = _run(plan, ctx, B, H, d, group=g, noise=noise, **kw)
        parts = [_run(plan, ctx[m:m + 1], g, H, d, global_offset=m * g,
                      noise=None if noise is None else noise[:, m * g:(m + 1) * g], **kw) for m in range(M)]
    finally:
        force_mlp_layout("auto")
    what = f"layout {layout}, {M} x {g}, H*d = {H * d}, {sample_fn}"
    assert chain.shape == (steps + 1, B, H, d)
    if sample_fn == "ddpm_cfg":  # clamped: bounded (the unclamped DDIM chains need not be)
        assert torch.isfinite(chain).all(), what
    assert _same(chain, torch.cat([p[0] for p in parts], dim=1)), f"chain differs ({what})"
    assert _same(x, torch.cat([p[1] for p in parts])), f"final sample differs ({what})"
    assert _same(am, torch.cat([p[2] for p in parts])), f"chain maxima differ ({what})"
    assert _same(x, chain[-1]), what


@pytest.mark.parametrize("M,g", SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_groups_bit_identical_to_shared_context_calls(layout, M, g):
    H, d = 16, 2
    _assert_groups_equal_shared_calls(_plan(H, d, "f32x3"), M, g, H, d, layout)


@pytest.mark.parametrize("layout", ("auto", "rw32x8"))
@pytest.mark.parametrize("case", ("hd64", "hd128", "nwo2", "injected", "ddim_cfg", "ddim"))
def test_groups_bit_identical_other_paths(case, layout):
    M, g = 3, 20
    H, d = {"hd64": (32, 2), "hd128": (64, 2)}.get(case, (16, 2))
    plan = _plan(H, d, "f32x3", cfg=case != "ddim")
    _assert_groups_equal_shared_calls(plan, M, g, H, d, layout, nwo=2 if case == "nwo2" else 0, injected=case == "injected",
                                      sample_fn=case if case in ("ddim_cfg", "ddim") else "ddpm_cfg")


def test_form_of_a_grouped_call():
    H, d = 16, 2
    for M, g in SHAPES:
        form = _plan(H, d, "f32x3").mlp_form_grouped(M, g)
        assert form["kernel"] == "x3" and form["layout"] in LAYOUTS and form["rows_per_workgroup"] in (16, 32), form
        f32 = _plan(H, d, "f32").mlp_form_grouped(M, g)
        assert f32["kernel"] == "f32" and f32["layout"] is None, f32
    assert _plan(H, d, "f16x2").mlp_form_grouped(3, 5)["kernel"] == "x3"  # never the fp16 kernel
    try:
        force_mlp_layout("16x4")
        assert _plan(H, d, "f32x3").mlp_form_grouped(64, 64)["layout"] == "16x4", "a forced layout wins"
    finally:
        force_mlp_layout("auto")


@pytest.mark.parametrize("M,g", ((3, 5), (3, 20)))
@pytest.mark.parametrize("layout", ("auto", "32x8", "16x4", "rw16", "rw32x8"))
def test_no_write_past_the_batch(layout, M, g):
    H, d, B, pad = 16, 2, M * g, 40
    plan = _plan(H, d, "f32x3")
    big = torch.full((B + pad, H, d), 1234.5, device="cuda")
    big_am = torch.full((B + pad,), -5.0, device="cuda")
    try:
        force_mlp_layout(layout)
        plan.sample_trajectories(_ctx(M), B, H, seed=2, out=big[:B], absmax_out=big_am[:B], context_group=g)
        torch.cuda.synchronize()
    finally:
        force_mlp_layout("auto")
    assert (big[B:] == 1234.5).all(), "samples written past the batch"
    assert (big_am[B:] == -5.0).all(), "chain maxima written past the batch"
    assert torch.isfinite(big[:B]).all() and (big[:B] != 1234.5).any(dim=(1, 2)).all(), "a candidate left unwritten"
    assert (big_am[:B] >= 0).all(), "a chain maximum left unwritten"


@pytest.mark.parametrize("dtype", ("f32", "f32x3", "f16x2"))
def test_grouped_mlp_matches_oracle(dtype):
    M, g, H, d = 3, 5, 16, 2
    B = M * g
    ctx = _ctx(M, seed=5)
    noise = torch.randn(N + 1, B, H, d, generator=torch.Generator().manual_seed(13))
    ref = osam.ddpm_cfg(_net(H, d), osch.buffers("exponential", N), ctx.repeat_interleave(g, 0), 0.01, B, H, noise=noise,
                        return_chain=True)
    got = _plan(H, d, dtype).sample_trajectories(ctx, B, H, w=0.01, noise=noise, return_chain=True, context_group=g)
    assert_traj_close(got, ref, what=f"grouped ddpm chain, {dtype}, {M} x {g}")


def test_grouped_unet_matches_oracle():
    """the U-Net path: the rows' projections replicated per candidate in front of the per-candidate kernels"""
    M, g, H, d = 2, 3, 8, 2
    B = M * g
    net = make_unet(d, C, seed=7)
    plan = DiffusionMPC(NetSpec("unet", d, H, C), net.state_dict(), variance_schedule="exponential", n_diffusion_steps=N)
    ctx = _ctx(M, seed=6)
    noise = torch.randn(N + 1, B, H, d, generator=torch.Generator().manual_seed(14))
    ref = osam.ddpm_cfg(net, osch.buffers("exponential", N), ctx.repeat_interleave(g, 0), 0.01, B, H, noise=noise,
                        return_chain=True)
    got = plan.sample_trajectories(ctx, B, H, w=0.01, noise=noise, return_chain=True, context_group=g)
    assert_traj_close(got, ref, what=f"grouped U-Net ddpm chain, {M} x {g}")
    per_cand = plan.sample_trajectories(ctx.repeat_interleave(g, 0), B, H, w=0.01, noise=noise, return_chain=True)
    assert _same(got, per_cand), "the replicated rows are the per-candidate call's"


# ---------------------------------------------------------------------------------------------- closed loop
CL_LIMITS = dict(cmin=-2 * np.ones(C, np.float32), cmax=2 * np.ones(C, np.float32), amin=-np.ones(2, np.float32),
                 amax=np.ones(2, np.float32))
# (x0 seed, noise seed) per n_samples, picked on the CPU so that the oracle's best and second-best costs are more than
# MIN_GAP apart (relative) at every (state, step): a last-bit difference of the samples then cannot flip an index
CL_SEEDS = {16: (3, 17), 3: (3, 18)}  # smallest gaps: 7.9e-3 and 9.7e-3
MIN_GAP = 1e-3


def _oracle_closed_loop(net, bufs, x0, sysname, T, n, H, d, w, noise, select, cmin, cmax, amin, amax):
    """tests/test_gpu_closed_loop.py's oracle loop, which also returns the smallest relative gap between the best and
    the second-best candidate cost over every (state, step)"""
    x = np.array(x0, dtype=np.float64)
    M = x.shape[0]
    xs, us, idx, gap = [x.copy()], [], [], np.inf
    for it in range(T):
        ctx = onorm.normalize(torch.from_numpy(x), torch.from_numpy(cmin), torch.from_numpy(cmax)).float()
        chain = osam.ddpm_cfg(net, bufs, ctx.repeat_interleave(n, 0), w, M * n, H, noise=noise(it), return_chain=True)
        u_it, i_it = [], []
        for m in range(M):
            u = onorm.unnormalize(chain[:, m * n:(m + 1) * n], torch.from_numpy(amin), torch.from_numpy(amax))[-1]
            cost = np.asarray(osys.rollout_cost(sysname, x[m], u.double().numpy()), dtype=np.float64)
            best2 = np.sort(cost)[:2]
            gap = min(gap, (best2[1] - best2[0]) / max(abs(best2[0]), 1e-300))
            i = 0 if select == "first" else int(osys.argmin(cost))
            u0 = np.array([round(float(v), 4) for v in u[i, 0]], dtype=np.float64)
            x[m] = osys.step(sysname, x[m], u0)
            u_it.append(u0)
            i_it.append(m * n + i)
        xs.append(x.copy())
        us.append(np.stack(u_it))
        idx.append(i_it)
    return np.stack(xs, 1), np.stack(us, 1), np.array(idx).T, gap


def closed_loop_case(n, select):
    """the inputs and the oracle's run of one closed-loop case (CPU only)"""
    M, T, H, d = 5, 4, 16, 2
    xseed, nseed = CL_SEEDS[n]
    x0 = np.random.default_rng(xseed).uniform(-1.5, 1.5, (M, 4))
    g = torch.Generator().manual_seed(nseed)
    noises = [torch.randn(N + 1, M * n, H, d, generator=g) for _ in range(T)]
    ref = _oracle_closed_loop(_net(H, d), osch.buffers("exponential", N), x0, "double_int2d", T, n, H, d, 0.01,
                              lambda it: noises[it], select, **CL_LIMITS)
    return x0, noises, ref


@pytest.mark.parametrize("select", ("argmin", "first"))
@pytest.mark.parametrize("n", (16, 3))
def test_grouped_closed_loop_matches_oracle(n, select):
    M, T, H, d = 5, 4, 16, 2
    x0, noises, (xr, ur, ir, gap) = closed_loop_case(n, select)
    assert gap > MIN_GAP, f"the oracle's two best costs are within {gap:.2e}: pick other seeds"
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), _net(H, d).state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=N, context_limits=(CL_LIMITS["cmin"].astype(np.float64), CL_LIMITS["cmax"].astype(np.float64)),
                        action_limits=(-np.ones(d), np.ones(d)))
    assert plan.mlp_form_grouped(M, n)["kernel"] == "x3" and plan.grouped_pays(M, n), "the grouped call is not taken"
    res = plan.closed_loop(x0, systems.get("double_int2d"), T, n_samples=n, w=0.01, select=select,
                           noise=lambda it: noises[it], grouped=True)
    assert res.x.shape == (M, T + 1, 4) and res.u.shape == (M, T, d) and res.index.shape == (M, T)
    np.testing.assert_array_equal(res.index, ir)
    # u0 is rounded to 4 decimals: a sampler difference within the 1e-4 parity bar can move it by 1e-4
    assert np.abs(res.u - ur).max() <= 1.01e-4
    assert np.abs(res.x - xr).max() <= 1e-4 * max(1.0, np.abs(xr).max())


def test_grouped_falls_back_where_it_was_measured_to_lose():
    """closed_loop(grouped=True) keeps per-candidate rows where part-empty workgroups cost more than the exact-f32
    kernel: the splits of profiles/grouped_ab.txt (an MI355X has 256 CUs), each on the side it was measured on"""
    plan = _plan(16, 2, "f32x3")
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        for M, n, pays in ((64, 64, True), (128, 32, True), (256, 16, True), (512, 8, True), (320, 12, False),
                           (640, 6, False), (1024, 4, False), (1280, 3, False), (2048, 2, False), (4096, 1, False)):
            assert plan.grouped_pays(M, n) is pays, (M, n)
    assert plan.grouped_pays(5, 16) and plan.grouped_pays(5, 3)  # less than one round of workgroups either way
    assert _plan(16, 2, "f32").grouped_pays(4096, 1)  # the same kernel either way


# ------------------------------------------------------------------------------------------------ arguments
def _grouped_rc(plan, B, H, d, ctx, group, sampler="ddpm_cfg"):
    x = torch.empty(B, H, d, device="cuda")
    a = nat.SampleArgs()
    a.context = ctx.data_ptr() if ctx is not None else None
    a.sampler = plan._sampler_id(sampler)
    a.batch = B
    a.w = 0.01
    a.x_out = x.data_ptr()
    rc = plan._lib.mpcd_sample_grouped(plan._ctx, ctypes.byref(a), group, plan._stream())
    torch.cuda.synchronize()
    return rc, plan._lib.mpcd_last_error().decode(errors="replace")


def test_grouped_argument_errors():
    H, d = 16, 2
    plan = _plan(H, d, "f32x3")
    ctx = _ctx(4).cuda()
    einval = -1
    assert nat._STATUS[einval] == "EINVAL"
    for what, args in (("group < 1", (12, ctx, 0)), ("negative group", (12, ctx, -3)),
                       ("batch % group != 0", (10, ctx, 3)), ("no context pointer", (12, None, 3))):
        rc, msg = _grouped_rc(plan, args[0], H, d, args[1], args[2])
        assert rc == einval and msg, (what, rc, msg)
    rc, msg = _grouped_rc(plan, 12, H, d, ctx, 3)
    assert rc == 0, msg
    # a net without a context
    unet = make_unet(1, 0, seed=5, cfg=False)
    bare = DiffusionMPC(NetSpec("unet", 1, 32, 0, cfg=False), unet.state_dict(), n_diffusion_steps=N)
    rc, msg = _grouped_rc(bare, 6, 32, 1, ctx, 3, sampler="ddim")
    assert rc == einval and "context" in msg, (rc, msg)


def test_context_group_needs_one_row_per_group():
    H, d = 16, 2
    plan = _plan(H, d, "f32x3")
    for rows in (1, 2, 12):  # 12 candidates in groups of 3: four rows, nothing else
        with pytest.raises(ValueError):
            plan.sample_trajectories(_ctx(rows), 12, H, context_group=3)
    with pytest.raises(ValueError):
        plan.sample_trajectories(_ctx(4), 12, H, context_group=5)
    with pytest.raises(ValueError):
        plan.sample_trajectories(None, 12, H, context_group=3)
    assert plan.sample_trajectories(_ctx(4), 12, H, context_group=3).shape == (12, H, d)
