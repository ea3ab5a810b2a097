"""GPU: closed_loop(native=True) - one mpcd_closed_loop call, per iteration the sampler and one fused control-tail
launch (closed_loop_tail_kernel) - against closed_loop(native=False), the composed calls. Both run the same sampler
kernels and the same fp64 operations in the same order per candidate, so every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
from mpc_via_diffusion_model_amd.planner import force_unet_path
from oracle import schedule as osch

from ._systems_ref import TAIL_DESCRIPTORS
from ._util import make_mlp, make_unet
from .test_gpu_closed_loop import _oracle_closed_loop

pytestmark = pytest.mark.gpu

H, D, C, NSTEPS, T = 16, 2, 4, 25, 4
LIMITS = (-2 * np.ones(C), 2 * np.ones(C))


@functools.lru_cache(maxsize=None)
def _plan(dtype="f32"):
    net = make_mlp(D, H, C, seed=31)
    return DiffusionMPC(NetSpec("mlp", D, H, C, dtype=dtype), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=LIMITS)


def _x0(M, nx=4):
    return np.random.default_rng(3).uniform(-1.5, 1.5, (M, nx))


def _noises(M, n, slices, seed=17, H=H):
    """slices[it] noise slices for iteration it, from one seeded generator"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, M * n, H, D, generator=g) for s in slices]


def _equal(a, b):
    for f in ("x", "u", "cost", "index"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)  # NaNs compare equal in place


def _both(plan, M, n, noises, iterations=T, x0=None, **kw):
    """(composed, native) results of one closed-loop call, asserted equal"""
    x0 = _x0(M) if x0 is None else x0
    noise = None if noises is None else (lambda it: noises[it])
    sysm = systems.get("double_int2d")
    ref = plan.closed_loop(x0, sysm, iterations, n_samples=n, noise=noise, native=False, **kw)
    got = plan.closed_loop(x0, sysm, iterations, n_samples=n, noise=noise, native=True, **kw)
    assert got.x.shape == (M, iterations + 1, 4) and got.index.shape == (M, iterations)
    _equal(got, ref)
    return ref, got


# a partial wave; two waves with a 16-lane tail; a single lane; three waves in one state
@pytest.mark.parametrize("clip_rule", ["chain", "final"])
@pytest.mark.parametrize("select", ["argmin", "first"])
@pytest.mark.parametrize("M,n", [(5, 16), (3, 80), (4, 1), (1, 130)])
def test_workgroup_split_shapes(M, n, select, clip_rule):
    _, got = _both(_plan(), M, n, _noises(M, n, [NSTEPS + 1] * T), select=select, clip_rule=clip_rule)
    assert ((got.index // n) == np.arange(M)[:, None]).all()
    if select == "first":
        assert (got.index == (np.arange(M) * n)[:, None]).all()


def test_ties_across_workgroups_go_to_the_lowest_index():
    M, n = 2, 130
    g = torch.Generator().manual_seed(5)
    noises = [torch.randn(NSTEPS + 1, M, 1, H, D, generator=g).expand(-1, -1, n, -1, -1).reshape(NSTEPS + 1, M * n, H, D)
              for _ in range(T)]
    ref, got = _both(_plan(), M, n, noises)
    for r in (ref, got):
        np.testing.assert_array_equal(r.index, np.repeat((np.arange(M) * n)[:, None], T, 1))


def test_nan_candidate_ranks_as_inf():
    M, n, state, cand = 3, 80, 1, 70
    clean = _noises(M, n, [NSTEPS + 1] * T)
    dirty = [z.clone() for z in clean]
    for z in dirty:
        z[0, state * n + cand, 3, 1] = float("nan")  # a NaN in arithmetic: this candidate's chain, samples and cost
    _, got = _both(_plan(), M, n, dirty)
    assert (got.index[state] != state * n + cand).all()
    assert np.isfinite(got.cost).all() and np.isfinite(got.x).all()
    plain = _plan().closed_loop(_x0(M), systems.get("double_int2d"), T, n_samples=n, noise=lambda it: clean[it],
                                native=True)
    for f in ("x", "u", "cost", "index"):
        for m in (0, 2):
            np.testing.assert_array_equal(getattr(got, f)[m], getattr(plain, f)[m], err_msg=f"{f}[{m}]")


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("M,n", [(3, 20), (2, 40)])
def test_split_bf16_grouped_and_per_candidate(M, n, grouped):
    plan = _plan("f32x3")
    # one round of workgroups for either kernel on >= 9 CUs, at a round cost of 0.45 or 0.65 against 1.0
    assert plan.grouped_pays(M, n)
    _both(plan, M, n, _noises(M, n, [NSTEPS + 1] * T), grouped=grouped)


@pytest.mark.parametrize("dtype,grouped", [("f32x3", True), ("f32x3", False), ("f32", True), ("f32", False)])
def test_warm_start_injected_noise(dtype, grouped):
    M, n, K = 3, 20, 5
    _both(_plan(dtype), M, n, _noises(M, n, [NSTEPS + 1] + [K + 1] * (T - 1)), grouped=grouped, warm_start=K)


@pytest.mark.parametrize("grouped", [True, False])
def test_warm_start_philox(grouped):
    _both(_plan("f32x3"), 3, 20, None, iterations=6, seed=5, grouped=grouped, warm_start=5)


def test_warm_start_with_steps_without_noise():
    M, n, K = 3, 80, 5
    _both(_plan(), M, n, _noises(M, n, [NSTEPS + 3] + [K + 3] * (T - 1)), warm_start=K, n_wo_noise=2)


def test_ddim_cfg_cold():
    M, n = 3, 80
    S = _plan().n_denoise_steps("ddim_cfg")
    _both(_plan(), M, n, _noises(M, n, [S + 1] * T), sample_fn="ddim_cfg")


def test_small_unet_layered():
    M, n, Nu, Tu = 2, 8, 10, 2
    net = make_unet(D, C, seed=7)
    # the exponential schedule is not finite at N = 10
    plan = DiffusionMPC(NetSpec("unet", D, H, C), net.state_dict(), variance_schedule="cosine",
                        n_diffusion_steps=Nu, context_limits=LIMITS)
    force_unet_path("layered")
    try:
        assert not plan.unet_form()["fused"]
        _both(plan, M, n, _noises(M, n, [Nu + 1] * Tu), iterations=Tu)
    finally:
        force_unet_path("auto")


def test_workspace_reuse_and_counter_reset():
    net = make_mlp(D, H, C, seed=31)
    plan = DiffusionMPC(NetSpec("mlp", D, H, C), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=LIMITS)
    small, large = _noises(5, 16, [NSTEPS + 1] * T), _noises(3, 80, [NSTEPS + 1] * T)
    _, first = _both(plan, 5, 16, small)
    _both(plan, 3, 80, large)
    _, third = _both(plan, 5, 16, small)
    _equal(first, third)


@pytest.mark.parametrize("select", ["argmin", "first"])
def test_native_matches_oracle(select):
    M, n = 5, 16
    net = make_mlp(D, H, C, seed=31)
    plan = DiffusionMPC(NetSpec("mlp", D, H, C), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=LIMITS, action_limits=(-np.ones(D), np.ones(D)))
    x0 = _x0(M)
    noises = _noises(M, n, [NSTEPS + 1] * T)
    res = plan.closed_loop(x0, systems.get("double_int2d"), T, n_samples=n, w=0.01, select=select,
                           noise=lambda it: noises[it], native=True)
    xr, ur, ir = _oracle_closed_loop(net, osch.buffers("exponential", NSTEPS), x0, "double_int2d", T, n, H, D, 0.01,
                                     lambda it: noises[it], -2 * np.ones(C, np.float32), 2 * np.ones(C, np.float32),
                                     -np.ones(D, np.float32), np.ones(D, np.float32), select)
    np.testing.assert_array_equal(res.index, ir)
    assert np.abs(res.u - ur).max() <= 1.01e-4
    assert np.abs(res.x - xr).max() <= 1e-4 * max(1.0, np.abs(xr).max())


@pytest.mark.parametrize("name", ["cartpole_lin5", "cartpole_nl5", "cartpole_zoh4", "pendulum", "quadrotor12"])
def test_every_system_and_cost_kind(name):
    """the tail's other five instantiations (cartpole_lin5 costs with calMPCCost): a net of the system's sizes, Philox
    noise, two waves with a tail per state, a warm loop so that context rows and priors are the tail's"""
    _system_case(systems.get(name))


@pytest.mark.parametrize("which", sorted(TAIL_DESCRIPTORS))
def test_non_default_descriptor(which):
    """the same comparison at a descriptor that is not the registry's (tests/_systems_ref.py: every constant distinct
    and non-zero, a set-point that is non-zero everywhere; the nonlinear cart-pole under calMPCCost)"""
    _system_case(TAIL_DESCRIPTORS[which]())


def _system_case(sysm):
    d, Cx, Hs, M, n = sysm.n_u, sysm.n_x, 32 // min(sysm.n_u, 2), 3, 80
    net = make_mlp(d, Hs, Cx, seed=9)
    plan = DiffusionMPC(NetSpec("mlp", d, Hs, Cx), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=(-2 * np.ones(Cx), 2 * np.ones(Cx)))
    x0 = np.random.default_rng(4).uniform(-0.3, 0.3, (M, Cx))
    ref = plan.closed_loop(x0, sysm, 3, n_samples=n, seed=2, warm_start=5, native=False)
    got = plan.closed_loop(x0, sysm, 3, n_samples=n, seed=2, warm_start=5, native=True)
    _equal(got, ref)
    assert np.isfinite(got.cost).all()


def test_last_samples_are_returned():
    """args.u_norm: the last iteration's samples = a sampler call with that iteration's contexts and seed"""
    M, n, iters, seed = 3, 20, 3, 11
    plan = _plan()
    res = plan.closed_loop(_x0(M), systems.get("double_int2d"), iters, n_samples=n, seed=seed, native=True)
    ctx = torch.from_numpy(plan.normalize_condition(res.x[:, iters - 1])).repeat_interleave(n, dim=0)
    want = plan.sample_trajectories(ctx, M * n, seed=seed + iters - 1)
    assert res.u_norm.shape == (M * n, H, D)
    assert torch.equal(res.u_norm, want)


def test_c_abi_refusals():
    import ctypes

    from mpc_via_diffusion_model_amd import _native as N

    def args(plan, sysm):
        a = N.ClosedLoopArgs()
        desc = sysm.desc()
        buf = torch.zeros(64, dtype=torch.float64, device=plan.device)
        a.sys = ctypes.pointer(desc)
        a.ctx_min, a.ctx_max = plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data
        a.act_min, a.act_max = plan.act_min.ctypes.data, plan.act_max.ctypes.data
        a.sample.sampler = N.MPCD_DDPM_CFG
        a.n_states, a.group, a.iterations, a.decimals = 2, 4, 1, 4
        a.x_dev = a.x_hist = a.u_hist = a.cost_hist = a.index_hist = buf.data_ptr()
        return a, (desc, buf)

    def call(plan, a):
        return plan._lib.mpcd_closed_loop(plan._ctx, ctypes.byref(a), None)

    plan, di = _plan(), systems.get("double_int2d")
    for field, value in (("clip_rule", N.MPCD_CLIP_NONE), ("iterations", 0), ("group", 0), ("n_states", 0),
                         ("x_hist", None), ("warm_t_start", NSTEPS + 1)):
        a, keep = args(plan, di)
        setattr(a, field, value)
        assert call(plan, a) == -1, field  # MPCD_EINVAL
    a, keep = args(plan, systems.get("pendulum"))  # n_u = 1, n_x = 2 against the net's 2 and 4
    assert call(plan, a) == -1
    a, keep = args(plan, di)
    a.sample.sampler, a.warm_t_start = N.MPCD_DDIM_CFG, 5
    assert call(plan, a) == -5  # MPCD_EUNSUP
    a, keep = args(_plan("f16x2"), di)
    assert call(_plan("f16x2"), a) == -5
    assert b"F16X2" in plan._lib.mpcd_last_error()


def test_refusals():
    sysm = systems.get("double_int2d")
    with pytest.raises(ValueError, match="f16x2"):
        _plan("f16x2").closed_loop(_x0(2), sysm, 2, n_samples=8, native=True)
    with pytest.raises(ValueError, match="warm_start"):
        _plan().closed_loop(_x0(2), sysm, 2, n_samples=8, sample_fn="ddim_cfg", warm_start=5, native=True)
