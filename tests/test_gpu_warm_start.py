"""GPU: warm-started sampling (mpcd_sample_warm, sample_trajectories(x_init=, t_start=K), mpcd_shift_plans,
mpcd_mpc_step_warm, closed_loop(warm_start=K)): the chain starts at a prior plan noised to diffusion level K (the
reference's q_sample at t = K - 1) and runs the last K steps of the CFG-DDPM chain only.

What is checked: slice 0 of the chain is torch's fp32 q_sample bit for bit with the right prior row per candidate
(shared, per candidate, per group); the rest of the chain is bit for bit what the existing kernels compute from that
slice 0 on a schedule cut to its first K rows (so the warm call adds nothing but the start); the whole chain holds the
project's oracle bar against the oracle on the cut tables; Philox numbering, sharding, bounds, arguments; the one-call
control step against the same step composed by hand; the closed loop against an oracle loop. Small shapes: what can
go wrong is the row mapping and the slice numbering, not the size."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
from mpc_via_diffusion_model_amd import _native as nat
from mpc_via_diffusion_model_amd import distributed as D
from mpc_via_diffusion_model_amd.planner import force_mlp_layout, philox_noise
from oracle import normalizer as onorm
from oracle import sampler as osam
from oracle import schedule as osch
from oracle import systems as osys

from ._util import assert_traj_close, make_mlp, make_unet
from .test_gpu_comm import _key, _run_ranks

pytestmark = pytest.mark.gpu

# 25 denoise steps: the fewest at which the exponential schedule's fp32 tables are finite (test_gpu_grouped_context.py)
C, N, K = 4, 25, 20
LAYOUTS = ("auto", "32x8", "16x8", "16x4", "rw32", "rw16", "rw32x8")
NETS = ("f32", "f32x3", "f16x2", "unet")
# prior rows: one for all, one per candidate (a ragged batch), one per group of a grouped call (M, g)
PRIORS = ("shared", "per_cand", (3, 5), (2, 16), (3, 20))
EINVAL, EUNSUP = -1, -5


@functools.lru_cache(maxsize=None)
def _net(kind, H, d):
    return make_unet(d, C, seed=7) if kind.startswith("unet") else make_mlp(d, H, C, seed=21)


def _shape(kind, H=None, d=None):
    # "unet": layer by layer (H = 8); "unet_fused": the whole-network launch (H = 32, split-bf16), the other x staging
    return {"unet": (8, 2), "unet_fused": (32, 1)}.get(kind) or (H or 16, d or 2)


@functools.lru_cache(maxsize=None)
def _plan(kind, H=None, d=None, k_rows=None):
    """kind: an MLP dtype or "unet"; k_rows: the schedule cut to its first k_rows rows (the replay's planner)"""
    H, d = _shape(kind, H, d)
    spec = {"unet": NetSpec("unet", d, H, C), "unet_fused": NetSpec("unet", d, H, C, dtype="f32x3")}.get(kind) \
        or NetSpec("mlp", d, H, C, dtype=kind)
    full = DiffusionMPC(spec, _net(kind, H, d).state_dict(), variance_schedule="exponential", n_diffusion_steps=N)
    if k_rows is None:
        return full
    return DiffusionMPC(spec, _net(kind, H, d).state_dict(), tables={k: v[:k_rows].clone() for k, v in full.tables.items()})


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _layout_of(prior):
    """(batch, group or None, prior rows) of a prior kind"""
    if prior == "shared":
        return 21, None, 1
    if prior == "per_cand":
        return 21, None, 21
    M, g = prior
    return M * g, g, M


def _expand(x_init, B, group):
    """the prior row of every candidate: row(b) of mpcd_warm_start"""
    if x_init.shape[0] == 1:
        return x_init.expand(B, -1, -1)
    return x_init if x_init.shape[0] == B else x_init.repeat_interleave(group, 0)


def _q_sample(plan, k, x_rows, z0):
    """torch fp32, on the CPU: two rounded products and one add"""
    sa = plan.tables["sqrt_alphas_cumprod"][k - 1].float()
    sb = plan.tables["sqrt_one_minus_alphas_cumprod"][k - 1].float()
    return sa * x_rows.float().cpu() + sb * z0.float().cpu()


def _inputs(B, H, d, group, rows, slices, seed=11):
    g = torch.Generator().manual_seed(seed)
    ctx = torch.rand(B // group if group else 1, C, generator=g) * 2 - 1
    x_init = torch.rand(rows, H, d, generator=g) * 1.6 - 0.8
    noise = torch.randn(slices, B, H, d, generator=g)
    return ctx, x_init, noise


def _run(plan, ctx, B, H, d, group=None, **kw):
    """(chain, final sample, chain maxima) of one sample call"""
    x = torch.full((B, H, d), 7.0, device="cuda")
    am = torch.full((B,), -1.0, device="cuda")
    chain = plan.sample_trajectories(ctx, B, H, w=0.01, return_chain=True, out=x, absmax_out=am, context_group=group, **kw)
    torch.cuda.synchronize()
    return chain, x, am


@functools.lru_cache(maxsize=None)
def _warm_case(kind, prior, k=K, nwo=0, H=None, d=None, layout="auto"):
    """one warm injected-noise call and its inputs, shared by the slice-0, replay and oracle tests"""
    H, d = _shape(kind, H, d)
    B, group, rows = _layout_of(prior)
    plan = _plan(kind, H, d)
    S = plan.n_denoise_steps(n_wo_noise=nwo, t_start=k)
    assert S == k + nwo
    ctx, x_init, noise = _inputs(B, H, d, group, rows, S + 1)
    try:
        force_mlp_layout(layout)
        chain, x, am = _run(plan, ctx, B, H, d, group, noise=noise, n_wo_noise=nwo, x_init=x_init, t_start=k)
    finally:
        force_mlp_layout("auto")
    assert chain.shape == (S + 1, B, H, d) and _same(x, chain[-1])
    return dict(plan=plan, ctx=ctx, x_init=x_init, noise=noise, chain=chain, x=x, am=am, B=B, group=group, H=H, d=d, S=S)


# ------------------------------------------------------------------------------- 1. slice 0 is q_sample
@pytest.mark.parametrize("prior", PRIORS, ids=str)
@pytest.mark.parametrize("kind", NETS)
def test_slice0_is_q_sample_bitwise(kind, prior):
    c = _warm_case(kind, prior)
    want = _q_sample(c["plan"], K, _expand(c["x_init"], c["B"], c["group"]), c["noise"][0])
    assert _same(c["chain"][0].cpu(), want), f"chain[0] is not torch's q_sample ({kind}, prior {prior})"


# ------------------------------------------------------------------ 2. the rest is the existing kernel's
def _assert_replay(kind, prior, k=K, nwo=0, H=None, d=None, layout="auto"):
    c = _warm_case(kind, prior, k, nwo, H, d, layout)
    cold = _plan(kind, c["H"], c["d"], k_rows=k)
    assert cold.n_steps == k and cold.n_denoise_steps(n_wo_noise=nwo) == c["S"]
    noise = c["noise"].cuda().clone()
    noise[0] = c["chain"][0]
    try:
        force_mlp_layout(layout)
        chain, x, am = _run(cold, c["ctx"], c["B"], c["H"], c["d"], c["group"], noise=noise, n_wo_noise=nwo)
    finally:
        force_mlp_layout("auto")
    what = f"{kind}, prior {prior}, K = {k}, n_wo_noise = {nwo}, H*d = {c['H'] * c['d']}, layout {layout}"
    assert torch.isfinite(c["chain"]).all(), what
    assert _same(c["chain"], chain), f"chain differs from the cold call on the cut schedule ({what})"
    assert _same(c["x"], x), f"final sample differs ({what})"
    assert _same(c["am"], am), f"chain maxima differ ({what})"
    # the maxima cover the chain's slices and nothing else (not the noise z0 the start was built from)
    assert _same(c["am"], c["chain"].abs().amax(dim=(0, 2, 3))), f"chain maxima are not the chain's ({what})"


@pytest.mark.parametrize("prior", ("shared", "per_cand", (3, 20)), ids=str)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_replay_f32x3_every_layout(layout, prior):
    _assert_replay("f32x3", prior, layout=layout)


@pytest.mark.parametrize("prior", ("shared", "per_cand", (3, 5)), ids=str)
@pytest.mark.parametrize("kind", ("f32", "f16x2", "unet"))
def test_replay_other_nets(kind, prior):
    _assert_replay(kind, prior)


@pytest.mark.parametrize("prior", ("shared", "per_cand", (3, 5)), ids=str)
def test_fused_unet_start_and_replay(prior):
    assert _plan("unet_fused").unet_form()["fused"], "this case is meant to take the fused U-Net path"
    c = _warm_case("unet_fused", prior)
    want = _q_sample(c["plan"], K, _expand(c["x_init"], c["B"], c["group"]), c["noise"][0])
    assert _same(c["chain"][0].cpu(), want), f"chain[0] is not torch's q_sample (fused U-Net, prior {prior})"
    _assert_replay("unet_fused", prior)


@pytest.mark.parametrize("layout", ("auto", "rw32x8"))
@pytest.mark.parametrize("H", (32, 64))
@pytest.mark.parametrize("prior", ("shared", (3, 20)), ids=str)
def test_replay_wider_nets(prior, H, layout):
    _assert_replay("f32x3", prior, H=H, d=2, layout=layout)


@pytest.mark.parametrize("nwo", (0, 2))
@pytest.mark.parametrize("k", (1, 20, 25))
@pytest.mark.parametrize("kind", ("f32x3", "f16x2"))
def test_replay_start_levels(kind, k, nwo):
    _assert_replay(kind, "shared", k=k, nwo=nwo)
    _assert_replay(kind, (3, 5), k=k, nwo=nwo)


# ------------------------------------------------------------------------------------ 3. oracle parity
@pytest.mark.parametrize("prior", ("shared", "per_cand", (3, 5)), ids=str)
@pytest.mark.parametrize("kind", NETS)
def test_warm_chain_matches_oracle(kind, prior):
    c = _warm_case(kind, prior)
    B, group, H = c["B"], c["group"], c["H"]
    nz = c["noise"].clone()
    nz[0] = _q_sample(c["plan"], K, _expand(c["x_init"], B, group), c["noise"][0])
    ctx = c["ctx"].repeat_interleave(group, 0) if group else c["ctx"].expand(B, C)
    bufs = {k: v[:K] for k, v in osch.buffers("exponential", N).items()}
    ref = osam.ddpm_cfg(_net(kind, H, c["d"]), bufs, ctx, 0.01, B, H, noise=nz, return_chain=True)
    assert ref.shape == c["chain"].shape and torch.isfinite(ref).all()
    assert_traj_close(c["chain"], ref, what=f"warm ddpm chain, {kind}, prior {prior}")


# --------------------------------------------------------------------------------------------- 4. Philox
@pytest.mark.parametrize("prior", ("shared", "per_cand", (3, 5)), ids=str)
@pytest.mark.parametrize("kind", NETS)
def test_philox_slices_are_the_executed_steps(kind, prior):
    H, d = _shape(kind)
    B, group, rows = _layout_of(prior)
    plan = _plan(kind, H, d)
    ctx, x_init, _ = _inputs(B, H, d, group, rows, 1)
    kw = dict(n_wo_noise=2, x_init=x_init, t_start=K)
    S = K + 2
    got = _run(plan, ctx, B, H, d, group, seed=5, global_offset=100, **kw)
    nz = philox_noise(B, S + 1, H * d, seed=5, global_offset=100).view(S + 1, B, H, d)
    want = _run(plan, ctx, B, H, d, group, noise=nz, **kw)
    for a, b, name in zip(got, want, ("chain", "final sample", "chain maxima")):
        assert _same(a, b), f"{name}: the seeded warm call is not its injected replay ({kind}, prior {prior})"


@pytest.mark.parametrize("prior", ("shared", "per_cand"))
@pytest.mark.parametrize("kind", NETS)
def test_sharding_invariance(kind, prior):
    H, d = _shape(kind)
    B, rows = 21, 1 if prior == "shared" else 21
    plan = _plan(kind, H, d)
    ctx, x_init, _ = _inputs(B, H, d, None, rows, 1)
    one = _run(plan, ctx, B, H, d, seed=9, global_offset=40, x_init=x_init, t_start=K)
    parts = [_run(plan, ctx, n, H, d, seed=9, global_offset=40 + lo, t_start=K,
                  x_init=x_init if rows == 1 else x_init[lo:lo + n]) for lo, n in ((0, 13), (13, 8))]
    assert _same(one[0], torch.cat([p[0] for p in parts], dim=1)), "chain depends on the split"
    assert _same(one[1], torch.cat([p[1] for p in parts])) and _same(one[2], torch.cat([p[2] for p in parts]))


# --------------------------------------------------------------------------------------------- 5. bounds
@pytest.mark.parametrize("layout", ("auto", "32x8", "16x4", "rw16", "rw32x8"))
@pytest.mark.parametrize("prior", ("shared", "per_cand", (3, 7)), ids=str)
def test_no_write_past_the_batch(prior, layout):
    H, d, pad = 16, 2, 40
    B, group, rows = _layout_of(prior)
    plan = _plan("f32x3", H, d)
    ctx, x_init, _ = _inputs(B, H, d, group, rows, 1)
    big = torch.full((B + pad, H, d), 1234.5, device="cuda")
    big_am = torch.full((B + pad,), -5.0, device="cuda")
    try:
        force_mlp_layout(layout)
        plan.sample_trajectories(ctx, B, H, seed=2, out=big[:B], absmax_out=big_am[:B], context_group=group,
                                 x_init=x_init, t_start=K)
        torch.cuda.synchronize()
    finally:
        force_mlp_layout("auto")
    assert (big[B:] == 1234.5).all(), "samples written past the batch"
    assert (big_am[B:] == -5.0).all(), "chain maxima written past the batch"
    assert torch.isfinite(big[:B]).all() and (big[:B] != 1234.5).any(dim=(1, 2)).all(), "a candidate left unwritten"
    assert (big_am[:B] >= 0).all(), "a chain maximum left unwritten"


@pytest.mark.parametrize("where", ("end", "middle"))
@pytest.mark.parametrize("prior", PRIORS, ids=str)
@pytest.mark.parametrize("kind", NETS)
def test_no_read_past_the_prior(kind, prior, where):
    """a prior of exactly `rows` rows is enough: it sits in a tensor that is NaN everywhere else"""
    H, d = _shape(kind)
    B, group, rows = _layout_of(prior)
    plan = _plan(kind, H, d)
    ctx, x_init, _ = _inputs(B, H, d, group, rows, 1)
    big = torch.full((rows + 64, H, d), float("nan"), device="cuda")
    lo = 64 if where == "end" else 32
    big[lo:lo + rows] = x_init.cuda()
    chain, x, am = _run(plan, ctx, B, H, d, group, seed=4, x_init=big[lo:lo + rows], t_start=K)
    assert torch.isfinite(chain).all() and torch.isfinite(x).all() and torch.isfinite(am).all()


# ------------------------------------------------------------------------------ 6. t_start = 0, arguments
def _sample_args(plan, B, H, d, ctx, noise=None, seed=3, sampler="ddpm_cfg", nwo=0):
    x = torch.full((B, H, d), 7.0, device="cuda")
    a = nat.SampleArgs()
    a.context = ctx.data_ptr() if ctx is not None else None
    a.context_shared = 1 if ctx is not None and ctx.shape[0] == 1 else 0
    a.sampler = plan._sampler_id(sampler)
    a.batch, a.w, a.seed, a.n_wo_noise = B, 0.01, seed, nwo
    a.noise = noise.data_ptr() if noise is not None else None
    a.x_out = x.data_ptr()
    return a, x


def _warm_rc(plan, a, group, warm):
    rc = plan._lib.mpcd_sample_warm(plan._ctx, ctypes.byref(a), group, ctypes.byref(warm) if warm is not None else None,
                                    plan._stream())
    torch.cuda.synchronize()
    return rc, plan._lib.mpcd_last_error().decode(errors="replace")


@pytest.mark.parametrize("kind", NETS)
def test_t_start_zero_is_the_cold_call(kind):
    H, d = _shape(kind)
    plan = _plan(kind, H, d)
    nan_prior = torch.full((1, H, d), float("nan"), device="cuda")  # ignored
    for group, B in ((None, 21), (5, 15)):
        ctx, _, _ = _inputs(B, H, d, group, 1, 1)
        cold = _run(plan, ctx, B, H, d, group, seed=6)
        warm0 = _run(plan, ctx, B, H, d, group, seed=6, x_init=nan_prior, t_start=0)
        for a, b in zip(cold, warm0):
            assert _same(a, b), f"t_start = 0 differs from the cold call ({kind}, group {group})"
        assert cold[0].shape[0] == N + 1
    # the entry point itself, with a null prior
    ctx = _inputs(12, H, d, None, 1, 1)[0].cuda()
    a, x = _sample_args(plan, 12, H, d, ctx)
    assert plan._lib.mpcd_sample(plan._ctx, ctypes.byref(a), plan._stream()) == 0
    torch.cuda.synchronize()
    want = x.clone()
    x.fill_(7.0)
    w = nat.WarmStart()
    rc, msg = _warm_rc(plan, a, 0, w)
    assert rc == 0, msg
    assert _same(x, want)


def test_steps_of_a_warm_call():
    plan = _plan("f32x3")
    for k, nwo in ((1, 0), (20, 0), (20, 2), (25, 3)):
        assert plan.n_denoise_steps(n_wo_noise=nwo, t_start=k) == k + nwo
    assert plan.n_denoise_steps(n_wo_noise=2, t_start=0) == N + 2 == plan.n_denoise_steps(n_wo_noise=2)
    a = nat.SampleArgs()
    a.sampler = nat.MPCD_DDIM_CFG
    w = nat.WarmStart()
    w.t_start = 5
    n = ctypes.c_int32()
    assert plan._lib.mpcd_sample_steps_warm(plan._ctx, ctypes.byref(a), ctypes.byref(w), ctypes.byref(n)) == EUNSUP
    a.sampler = nat.MPCD_DDPM_CFG
    w.t_start = N + 1
    assert plan._lib.mpcd_sample_steps_warm(plan._ctx, ctypes.byref(a), ctypes.byref(w), ctypes.byref(n)) == EINVAL
    assert plan._lib.mpcd_sample_steps_warm(plan._ctx, ctypes.byref(a), None, ctypes.byref(n)) == EINVAL


def test_warm_argument_errors():
    H, d = 16, 2
    plan = _plan("f32x3")
    assert nat._STATUS[EINVAL] == "EINVAL" and nat._STATUS[EUNSUP] == "EUNSUP"
    ctx1, ctx4 = (_inputs(12, H, d, g, 1, 1)[0].cuda() for g in (None, 3))
    prior = torch.zeros(12, H, d, device="cuda")

    def warm(t_start, rows, ptr=prior):
        w = nat.WarmStart()
        w.t_start, w.rows, w.x_init = t_start, rows, ptr.data_ptr() if ptr is not None else None
        return w

    a1, _ = _sample_args(plan, 12, H, d, ctx1)
    a4, _ = _sample_args(plan, 12, H, d, ctx4)
    for what, a, group, w in (("null warm", a1, 0, None), ("t_start < 0", a1, 0, warm(-1, 1)),
                              ("t_start > n_steps", a1, 0, warm(N + 1, 1)), ("null x_init", a1, 0, warm(K, 1, None)),
                              ("rows 0", a1, 0, warm(K, 0)), ("rows 5", a1, 0, warm(K, 5)),
                              ("rows batch / group without a group", a1, 0, warm(K, 4)),
                              ("rows 5 grouped", a4, 3, warm(K, 5)), ("group does not divide", a4, 5, warm(K, 1)),
                              ("group does not divide, cold", a4, 5, warm(0, 1)), ("negative group", a4, -3, warm(K, 1))):
        rc, msg = _warm_rc(plan, a, group, w)
        assert rc == EINVAL and msg, (what, rc, msg)
    for what, a, group, w in (("shared", a1, 0, warm(K, 1)), ("per candidate", a1, 0, warm(K, 12)),
                              ("per group", a4, 3, warm(K, 4)), ("grouped, shared", a4, 3, warm(K, 1)),
                              ("grouped, per candidate", a4, 3, warm(K, 12)), ("t_start = n_steps", a1, 0, warm(N, 1))):
        rc, msg = _warm_rc(plan, a, group, w)
        assert rc == 0, (what, rc, msg)
    # DDIM: not implemented with a warm start, fine cold
    ddim = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), _net("f32x3", H, d).state_dict(),
                        variance_schedule="exponential", n_diffusion_steps=N)
    ad, _ = _sample_args(ddim, 12, H, d, ctx1, sampler="ddim_cfg")
    ad.ddim_steps = 5
    rc, msg = _warm_rc(ddim, ad, 0, warm(K, 1))
    assert rc == EUNSUP and "DDPM" in msg, (rc, msg)
    rc, msg = _warm_rc(ddim, ad, 0, warm(0, 1))
    assert rc == 0, msg
    # the control step: one prior for every candidate, and not the buffer the next one is written to
    st = nat.StepArgs()
    best = nat.Best()
    assert plan._lib.mpcd_mpc_step_warm(plan._ctx, ctypes.byref(st), None, None, ctypes.byref(best), None, None) == EINVAL
    w = warm(K, 12)
    assert plan._lib.mpcd_mpc_step_warm(plan._ctx, ctypes.byref(st), ctypes.byref(w), None, ctypes.byref(best), None,
                                        None) == EINVAL
    assert b"rows" in plan._lib.mpcd_last_error()
    w = warm(K, 1)
    assert plan._lib.mpcd_mpc_step_warm(plan._ctx, ctypes.byref(st), ctypes.byref(w), ctypes.c_void_p(prior.data_ptr()),
                                        ctypes.byref(best), None, None) == EINVAL
    assert b"alias" in plan._lib.mpcd_last_error()
    # mpcd_shift_plans
    out = torch.empty(1, H, d, device="cuda")
    L, p = plan._lib, lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.mpcd_shift_plans(plan._ctx, None, 12, H, None, 0, 1, p(out), None) == EINVAL
    assert L.mpcd_shift_plans(plan._ctx, p(prior), 12, H + 1, None, 0, 1, p(out), None) == EINVAL
    assert L.mpcd_shift_plans(plan._ctx, p(prior), 12, H, None, 0, 0, p(out), None) == EINVAL


def test_python_argument_errors():
    H, d = 16, 2
    plan = _plan("f32x3")
    ctx4 = _inputs(12, H, d, 3, 1, 1)[0]
    ok = torch.zeros(1, H, d)
    for kw in (dict(t_start=K), dict(t_start=K, x_init=torch.zeros(5, H, d)), dict(t_start=K, x_init=torch.zeros(1, H, d + 1)),
               dict(t_start=K, x_init=torch.zeros(4, H, d)), dict(t_start=N + 1, x_init=ok), dict(t_start=-1, x_init=ok),
               dict(t_start=K, x_init=ok, noise=torch.zeros(N + 1, 12, H, d))):
        with pytest.raises(ValueError):
            plan.sample_trajectories(ctx4[:1], 12, H, **kw)
    with pytest.raises(ValueError):
        plan.sample_trajectories(ctx4, 12, H, context_group=3, t_start=K, x_init=torch.zeros(3, H, d))
    assert plan.sample_trajectories(ctx4, 12, H, context_group=3, t_start=K, x_init=torch.zeros(4, H, d)).shape == (12, H, d)
    assert plan.sample_trajectories(ctx4[:1], 12, H, t_start=K, x_init=torch.zeros(H, d),
                                    noise=torch.zeros(K + 1, 12, H, d)).shape == (12, H, d)
    sysm, x0 = systems.double_int2d(), np.zeros(4)
    for kw in (dict(warm_start=K, native=False), dict(warm_start=0), dict(warm_start=N + 1),
               dict(warm_start=K, sample_fn="ddim_cfg"), dict(prior=ok)):
        with pytest.raises(ValueError):
            plan.mpc_step(x0, sysm, 12, **kw)
    for kw in (dict(warm_start=0), dict(warm_start=N + 1), dict(warm_start=K, sample_fn="ddim_cfg")):
        with pytest.raises(ValueError):
            plan.closed_loop(np.zeros((2, 4)), sysm, 2, n_samples=3, **kw)


# ------------------------------------------------------------------------------------ shift_plan_kernel
@pytest.mark.parametrize("H,d", ((16, 2), (8, 1), (8, 4), (8, 3)))
def test_shift_plans_gathers_and_shifts(H, d):
    """every vector width of the kernel (d = 4, 2, odd): the entry point takes the net's H and d, so a net per shape"""
    mp = _plan("f32x3") if (H, d) == (16, 2) else DiffusionMPC(NetSpec("unet", d, H, C), make_unet(d, C, seed=2).state_dict(),
                                                               n_diffusion_steps=N)
    B, off = 9, 100
    u = torch.randn(B + 2, H, d, generator=torch.Generator().manual_seed(1)).cuda()
    idx = torch.tensor([off + 4, off + 0, off + 8, off + 9, off - 1], dtype=torch.int64, device="cuda")
    out = torch.full((len(idx) + 1, H, d), 55.0, device="cuda")
    got = mp.shift_plans(u[:B], idx, off, out=out[:len(idx)])
    torch.cuda.synchronize()
    want = torch.cat([u[:, 1:], u[:, -1:]], dim=1)
    for m, i in enumerate((4, 0, 8)):
        assert _same(got[m], want[i]), f"state {m}"
    assert (out[3:] == 55.0).all(), "an index outside the batch must write nothing (nor may anything land past the states)"
    every = mp.shift_plans(u[:B])
    assert _same(every, want[:B])


# --------------------------------------------------------------------------------- 7. mpcd_mpc_step_warm
STEP_X0 = (np.array([0.3, -0.2, 0.1, 0.05]), np.array([0.25, -0.1, 0.12, 0.0]), np.array([0.2, -0.05, 0.1, -0.02]))


def _step_plan(dtype):
    H, d = 16, 2
    return DiffusionMPC(NetSpec("mlp", d, H, C, dtype=dtype), _net(dtype, H, d).state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=N, context_limits=(-2 * np.ones(C), 2 * np.ones(C)),
                        action_limits=(-np.ones(d), np.ones(d)))


def _composed_steps(plan, B, nwo=0):
    """cold, warm, warm by hand: sample_trajectories -> clip flag -> rollout_cost -> argmin -> a torch shift"""
    sysm, H = systems.double_int2d(), 16
    prior, out = None, []
    for s, x0 in enumerate(STEP_X0):
        ctx = torch.from_numpy(plan.normalize_condition(x0)[None])
        am = torch.empty(B, dtype=torch.float32, device="cuda")
        u_norm = plan.sample_trajectories(ctx, B, H, w=0.01, seed=20 + s, absmax_out=am, n_wo_noise=nwo, x_init=prior,
                                          t_start=None if prior is None else K)
        flag = plan.clip_flag(am)
        cost = plan.rollout_cost(sysm, x0, u_norm, flag)
        idx, best = plan.argmin(cost)
        u_best = plan.unnormalize_states(u_norm[idx][None], flag)[0].cpu().numpy()
        prior = torch.cat([u_norm[idx, 1:], u_norm[idx, -1:]])[None].clone()
        out.append(dict(index=idx, cost=best, u_best=u_best, costs=cost.clone(), u_norm=u_norm.clone(), prior=prior[0]))
    return out


@pytest.mark.parametrize("dtype", ("f32x3", "f32", "f16x2"))
def test_mpc_step_warm_equals_the_composed_steps(dtype):
    B = 48
    sysm = systems.double_int2d()
    want = _composed_steps(_step_plan(dtype), B)
    plan = _step_plan(dtype)
    assert plan.warm_prior() is None
    for s, (x0, w) in enumerate(zip(STEP_X0, want)):
        r = plan.mpc_step(x0, sysm, B, w=0.01, seed=20 + s, warm_start=K)
        torch.cuda.synchronize()
        assert (r.best_index, r.best_cost) == (w["index"], w["cost"]), f"step {s}"
        np.testing.assert_array_equal(r.u_best, w["u_best"])
        assert torch.equal(r.costs, w["costs"]) and _same(r.u_norm, w["u_norm"]), f"step {s}"
        assert _same(plan.warm_prior(), w["prior"]), f"step {s}: the next prior is not the shifted winner"
    # a dropped prior: the next step is the cold one again; an overriding prior: the step that started from it
    plan.reset_warm_start()
    r = plan.mpc_step(STEP_X0[0], sysm, B, w=0.01, seed=20, warm_start=K)
    assert _same(r.u_norm, want[0]["u_norm"])
    r = plan.mpc_step(STEP_X0[2], sysm, B, w=0.01, seed=22, warm_start=K, prior=want[1]["prior"])
    assert _same(r.u_norm, want[2]["u_norm"]) and r.best_index == want[2]["index"]


def test_mpc_step_warm_takes_the_plan_reuse_branch_and_leaves_the_cold_step_alone():
    """a loop of warm steps reuses the cached K-step plan (same results as fresh planners give), and mpc_step without
    warm_start on the same planner is the cold step whatever ran before"""
    B, sysm = 48, systems.double_int2d()
    plan = _step_plan("f32x3")
    cold = plan.mpc_step(STEP_X0[0], sysm, B, seed=20)
    plan.mpc_step(STEP_X0[0], sysm, B, seed=20, warm_start=K)
    a = plan.mpc_step(STEP_X0[1], sysm, B, seed=21, warm_start=K)
    prior = plan._prior_spare.clone()  # what step a started from
    b = plan.mpc_step(STEP_X0[1], sysm, B, seed=21, warm_start=K, prior=prior[0])
    assert _same(a.u_norm, b.u_norm) and a.best_cost == b.best_cost
    again = plan.mpc_step(STEP_X0[0], sysm, B, seed=20)
    assert _same(again.u_norm, cold.u_norm) and again.best_cost == cold.best_cost


def test_mpc_step_warm_loopback_ranks_equal_one_rank():
    nranks, b_local, sysm = 2, 24, systems.double_int2d()
    want = _composed_steps(_step_plan("f32x3"), nranks * b_local)
    plans = [_step_plan("f32x3") for _ in range(nranks)]
    key = _key()
    comms = [D.NativeComm(plans[r], loopback=(nranks, r, key)) for r in range(nranks)]

    def body(r):
        out = []
        for s, x0 in enumerate(STEP_X0):
            res = plans[r].mpc_step(x0, sysm, b_local, w=0.01, seed=20 + s, comm=comms[r], warm_start=K)
            torch.cuda.current_stream().synchronize()
            out.append((res, plans[r].warm_prior().clone()))
        return out

    for r, steps in enumerate(_run_ranks(nranks, body)):
        for s, ((res, prior), w) in enumerate(zip(steps, want)):
            assert (res.best_index, res.best_cost) == (w["index"], w["cost"]), (r, s)
            np.testing.assert_array_equal(res.u_best, w["u_best"])
            assert _same(res.u_norm, w["u_norm"][r * b_local:(r + 1) * b_local]), (r, s)
            assert _same(prior, w["prior"]), f"rank {r}, step {s}: the ranks' priors differ from one rank's"


# --------------------------------------------------------------------- 8. closed loop against the oracle
CL_LIMITS = dict(cmin=-2 * np.ones(C, np.float32), cmax=2 * np.ones(C, np.float32), amin=-np.ones(2, np.float32),
                 amax=np.ones(2, np.float32))
CL_XSEED, CL_NSEED = 3, 17  # the oracle's smallest relative gap of the two best costs: 5.3e-3 (n = 16), 1.0e-2 (n = 3)
MIN_GAP = 1e-3


@functools.lru_cache(maxsize=None)
def _closed_loop_case(n):
    """inputs and the oracle's warm closed loop (CPU): test_gpu_grouped_context.py's loop, iteration 0 cold with N + 1
    noise slices, later ones warm with K + 1 (slice 0 the q_sample draw) from the winner's shifted final row"""
    M, T, H, d = 5, 4, 16, 2
    net, bufs = _net("f32x3", H, d), osch.buffers("exponential", N)
    cut = {k: v[:K] for k, v in bufs.items()}
    sa, sb = bufs["sqrt_alphas_cumprod"][K - 1], bufs["sqrt_one_minus_alphas_cumprod"][K - 1]
    x = np.random.default_rng(CL_XSEED).uniform(-1.5, 1.5, (M, 4))
    x0 = x.copy()
    g = torch.Generator().manual_seed(CL_NSEED)
    lim = {k: torch.from_numpy(v) for k, v in CL_LIMITS.items()}
    noises, xs, us, idx, gap, prior = [], [x.copy()], [], [], np.inf, None
    for it in range(T):
        S = N if it == 0 else K
        noise = torch.randn(S + 1, M * n, H, d, generator=g)
        noises.append(noise)
        ctx = onorm.normalize(torch.from_numpy(x), lim["cmin"], lim["cmax"]).float().repeat_interleave(n, 0)
        if it == 0:
            chain = osam.ddpm_cfg(net, bufs, ctx, 0.01, M * n, H, noise=noise, return_chain=True)
        else:
            nz = noise.clone()
            nz[0] = sa * prior.repeat_interleave(n, 0) + sb * noise[0]
            chain = osam.ddpm_cfg(net, cut, ctx, 0.01, M * n, H, noise=nz, return_chain=True)
        u_it, i_it, rows = [], [], []
        for m in range(M):
            u = onorm.unnormalize(chain[:, m * n:(m + 1) * n], lim["amin"], lim["amax"])[-1]
            cost = np.asarray(osys.rollout_cost("double_int2d", x[m], u.double().numpy()), dtype=np.float64)
            best2 = np.sort(cost)[:2]
            gap = min(gap, (best2[1] - best2[0]) / max(abs(best2[0]), 1e-300))
            i = int(osys.argmin(cost))
            u0 = np.array([round(float(v), 4) for v in u[i, 0]], dtype=np.float64)
            x[m] = osys.step("double_int2d", x[m], u0)
            u_it.append(u0)
            i_it.append(m * n + i)
            row = chain[-1, m * n + i]
            rows.append(torch.cat([row[1:], row[-1:]]))
        prior = torch.stack(rows)
        xs.append(x.copy())
        us.append(np.stack(u_it))
        idx.append(i_it)
    return x0, noises, np.stack(xs, 1), np.stack(us, 1), np.array(idx).T, gap


@pytest.mark.parametrize("grouped", (True, False))
@pytest.mark.parametrize("n", (16, 3))
def test_warm_closed_loop_matches_oracle(n, grouped):
    M, T, H, d = 5, 4, 16, 2
    x0, noises, xr, ur, ir, gap = _closed_loop_case(n)
    assert gap > MIN_GAP, f"the oracle's two best costs are within {gap:.2e}: pick other seeds"
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), _net("f32x3", H, d).state_dict(),
                        variance_schedule="exponential", n_diffusion_steps=N,
                        context_limits=(CL_LIMITS["cmin"].astype(np.float64), CL_LIMITS["cmax"].astype(np.float64)),
                        action_limits=(-np.ones(d), np.ones(d)))
    if grouped:
        assert plan.mlp_form_grouped(M, n)["kernel"] == "x3" and plan.grouped_pays(M, n), "the grouped call is not taken"
    res = plan.closed_loop(x0, systems.get("double_int2d"), T, n_samples=n, w=0.01, select="argmin",
                           noise=lambda it: noises[it], grouped=grouped, warm_start=K)
    assert res.x.shape == (M, T + 1, 4) and res.u.shape == (M, T, d) and res.index.shape == (M, T)
    np.testing.assert_array_equal(res.index, ir)
    # u0 is rounded to 4 decimals: a sampler difference within the 1e-4 parity bar can move it by 1e-4
    assert np.abs(res.u - ur).max() <= 1.01e-4
    assert (np.abs(res.x - xr) <= 1e-4 * np.maximum(1.0, np.abs(xr))).all()
