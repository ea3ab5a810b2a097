"""GPU: mpc_step_batch - one mpcd_mpc_step_batch call per control step for M plant states that arrive from outside
(one state upload, the sampler, one batch_step_tail_kernel launch, one result download) - against the closed loop fed
its own states, the composed entry points and the oracle. The step and the loop run the same sampler kernels and the
same fp64 operations in the same order per candidate, so every comparison between them is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
from mpc_via_diffusion_model_amd import _native as N
from mpc_via_diffusion_model_amd.planner import force_unet_path
from oracle import normalizer as onorm
from oracle import sampler as osam
from oracle import schedule as osch
from oracle import systems as osys

from ._systems_ref import TAIL_DESCRIPTORS
from ._util import assert_traj_close, make_mlp, make_unet

pytestmark = pytest.mark.gpu

H, D, C, NSTEPS, T, K = 16, 2, 4, 25, 3, 10
LIMITS = (-2 * np.ones(C), 2 * np.ones(C))
SHAPES = [(5, 16), (3, 80), (4, 1), (1, 130)]  # a partial wave; two waves with a tail; single lanes; three workgroups
CLIPPED, NAN_SAMPLES, NONFINITE = N.MPCD_STEP_CLIPPED, N.MPCD_STEP_NAN_SAMPLES, N.MPCD_STEP_NONFINITE_WINNER


def _new_plan(dtype="f32", **kw):
    net = make_mlp(D, H, C, seed=31)
    return DiffusionMPC(NetSpec("mlp", D, H, C, dtype=dtype), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=LIMITS, **kw)


@functools.lru_cache(maxsize=None)
def _plan(dtype="f32"):
    return _new_plan(dtype)


def _di():
    return systems.get("double_int2d")


def _x0(M, nx=4):
    return np.random.default_rng(3).uniform(-1.5, 1.5, (M, nx))


def _noises(M, n, slices, seed=17, H=H):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, M * n, H, D, generator=g) for s in slices]


def _same(r, ref, it, what=""):
    for f in ("u", "cost", "index"):
        np.testing.assert_array_equal(getattr(r, f), getattr(ref, f)[:, it], err_msg=f"{what} {f}[{it}]")


def _steps_vs_loop(plan, M, n, noises, sysm=None, x0=None, seed=0, iterations=T, check=None, **kw):
    """closed_loop(native=False) once, then one mpc_step_batch per iteration on the loop's recorded states"""
    sysm = sysm or _di()
    x0 = _x0(M) if x0 is None else x0
    noise = None if noises is None else (lambda it: noises[it])
    ref = plan.closed_loop(x0, sysm, iterations, n_samples=n, noise=noise, seed=seed, native=False, **kw)
    plan.reset_warm_start()
    out = []
    for it in range(iterations):
        r = plan.mpc_step_batch(ref.x[:, it], sysm, n, seed=seed + it, noise=None if noises is None else noises[it],
                                return_samples=check is not None, **kw)
        assert r.u.shape == (M, sysm.n_u) and r.plan.shape[0] == M and r.flags.shape == (M,)
        _same(r, ref, it)
        assert ((r.index // n) == np.arange(M)).all()
        if check is not None:
            check(plan, r)
        out.append(r)
    return ref, out


# ---- 1. equals the closed loop, fed its states

@pytest.mark.parametrize("clip_rule", ["chain", "final"])
@pytest.mark.parametrize("select", ["argmin", "first"])
@pytest.mark.parametrize("M,n", SHAPES)
def test_equals_closed_loop_shapes(M, n, select, clip_rule):
    _, out = _steps_vs_loop(_plan(), M, n, _noises(M, n, [NSTEPS + 1] * T), select=select, clip_rule=clip_rule)
    if select == "first":
        for r in out:
            np.testing.assert_array_equal(r.index, np.arange(M) * n)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("M,n", [(3, 20), (2, 40)])
def test_equals_closed_loop_split_bf16(M, n, grouped):
    plan = _plan("f32x3")
    assert plan.grouped_pays(M, n)
    _steps_vs_loop(plan, M, n, _noises(M, n, [NSTEPS + 1] * T), grouped=grouped)


def test_equals_closed_loop_philox():
    _steps_vs_loop(_plan(), 3, 80, None, seed=5)


def test_equals_closed_loop_ddim_cfg_cold():
    M, n = 3, 80
    S = _plan().n_denoise_steps("ddim_cfg")
    _steps_vs_loop(_plan(), M, n, _noises(M, n, [S + 1] * T), sample_fn="ddim_cfg")


def test_equals_closed_loop_small_unet_layered():
    M, n, Nu, Tu = 2, 8, 10, 2
    net = make_unet(D, C, seed=7)
    plan = DiffusionMPC(NetSpec("unet", D, H, C), net.state_dict(), variance_schedule="cosine",
                        n_diffusion_steps=Nu, context_limits=LIMITS)
    force_unet_path("layered")
    try:
        assert not plan.unet_form()["fused"]
        _steps_vs_loop(plan, M, n, _noises(M, n, [Nu + 1] * Tu), iterations=Tu)
    finally:
        force_unet_path("auto")


@pytest.mark.parametrize("name", ["cartpole_lin5", "cartpole_nl5", "cartpole_zoh4", "pendulum", "quadrotor12"])
def test_every_system_and_cost_kind(name):
    """the tail's other five instantiations (cartpole_lin5 costs with calMPCCost): a net of the system's sizes, Philox
    noise, two waves with a tail per state, a warm sequence so that the priors are the tail's"""
    _system_case(systems.get(name))


def _system_case(sysm):
    d, Cx, Hs, M, n = sysm.n_u, sysm.n_x, 32 // min(sysm.n_u, 2), 3, 80
    net = make_mlp(d, Hs, Cx, seed=9)
    plan = DiffusionMPC(NetSpec("mlp", d, Hs, Cx), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=(-2 * np.ones(Cx), 2 * np.ones(Cx)))
    x0 = np.random.default_rng(4).uniform(-0.3, 0.3, (M, Cx))
    ref, out = _steps_vs_loop(plan, M, n, None, sysm=sysm, x0=x0, seed=2, warm_start=5, check=_check_plan)
    assert np.isfinite(ref.cost).all()


@pytest.mark.parametrize("which", sorted(TAIL_DESCRIPTORS))
def test_non_default_descriptor(which):
    """the same harness at a descriptor that is not the registry's (tests/_systems_ref.py: every constant distinct and
    non-zero, a set-point that is non-zero everywhere; the nonlinear cart-pole under calMPCCost): the tail and the
    composed calls take the descriptor through different arguments, and here a slip in either shows"""
    _system_case(TAIL_DESCRIPTORS[which]())


# ---- 2. warm start

def _check_priors(plan, r):
    want = plan.shift_plans(r.u_norm, torch.from_numpy(r.index).to(plan.device))
    assert torch.equal(plan.batch_priors(), want)


@pytest.mark.parametrize("n_wo", [0, 2])
@pytest.mark.parametrize("dtype,grouped", [("f32x3", True), ("f32x3", False), ("f32", False)])
def test_warm_start_injected_noise(dtype, grouped, n_wo):
    M, n = 3, 20
    plan = _plan(dtype)
    noises = _noises(M, n, [NSTEPS + n_wo + 1] + [K + n_wo + 1] * (T - 1))
    _steps_vs_loop(plan, M, n, noises, grouped=grouped, warm_start=K, n_wo_noise=n_wo, check=_check_priors)
    assert plan.warm_prior() is None  # mpc_step's single prior is a separate one
    plan.reset_warm_start()
    assert plan.batch_priors() is None


@pytest.mark.parametrize("grouped", [True, False])
def test_warm_start_philox(grouped):
    _steps_vs_loop(_plan("f32x3"), 3, 20, None, seed=5, grouped=grouped, warm_start=K, check=_check_priors)


def test_warm_start_restarts_cold_when_the_state_count_changes():
    plan = _new_plan()
    di = _di()
    cold = plan.mpc_step_batch(_x0(3), di, 20, seed=4)
    plan.mpc_step_batch(_x0(5), di, 20, seed=3, warm_start=K)
    r = plan.mpc_step_batch(_x0(3), di, 20, seed=4, warm_start=K)  # 5 priors kept, 3 states: cold
    np.testing.assert_array_equal(r.cost, cold.cost)
    assert plan.batch_priors().shape == (3, H, D)


# ---- 3. plan output

def _check_plan(plan, r):
    row = r.u_norm.shape[1] * r.u_norm.shape[2]
    for m in range(r.index.shape[0]):
        flag = torch.tensor([1 if r.flags[m] & CLIPPED else 0], dtype=torch.int32, device=plan.device)
        want = plan.unnormalize_states(r.u_norm[int(r.index[m])][None], flag)[0].cpu().numpy()
        assert r.plan[m].tobytes() == want.tobytes(), m
        assert want.size == row
        np.testing.assert_array_equal(r.u[m], np.rint(want[0].astype(np.float64) * 1e4) / 1e4)


@pytest.mark.parametrize("clip_rule", ["chain", "final"])
@pytest.mark.parametrize("M,n", SHAPES)
def test_plan_output(M, n, clip_rule):
    plan = _plan()
    seen = set()
    for it, z in enumerate(_noises(M, n, [NSTEPS + 1] * 2, seed=23)):
        r = plan.mpc_step_batch(_x0(M) * (1 - 0.5 * it), _di(), n, noise=z, clip_rule=clip_rule, return_samples=True)
        _check_plan(plan, r)
        seen |= set(int(f) & CLIPPED for f in r.flags)
        assert not (r.flags & ~CLIPPED).any()
    if clip_rule == "chain" and n > 1:
        assert CLIPPED in seen  # x_T ~ N(0, 1) is inside the tested chain


# ---- 4. an external plant, against the oracle

def test_external_plant_matches_oracle():
    """The states come from a host-side plant no built-in system produces (the model's step plus a disturbance).
    Bars: the suite's parity bars - samples 1e-4 (assert_traj_close), costs rtol 1e-4, u0 1.01e-4 (rounded to 4
    places: a sampler difference within 1e-4 can move it by 1e-4, tests/test_gpu_closed_loop.py), the selected index
    equal wherever the oracle's two best costs differ by more than the cost bar."""
    M, n = 5, 16
    net = make_mlp(D, H, C, seed=31)
    plan = _new_plan(action_limits=(-np.ones(D), np.ones(D)))
    bufs = osch.buffers("exponential", NSTEPS)
    cmin, cmax = -2 * np.ones(C, np.float32), 2 * np.ones(C, np.float32)
    amin, amax = -np.ones(D, np.float32), np.ones(D, np.float32)
    noises = _noises(M, n, [NSTEPS + 1] * T)
    rng = np.random.default_rng(11)
    x = _x0(M)
    for it in range(T):
        r = plan.mpc_step_batch(x, _di(), n, w=0.01, noise=noises[it], return_samples=True)
        ctx = onorm.normalize(torch.from_numpy(x), torch.from_numpy(cmin), torch.from_numpy(cmax)).float()
        chain = osam.ddpm_cfg(net, bufs, ctx.repeat_interleave(n, 0), 0.01, M * n, H, noise=noises[it],
                              return_chain=True)
        assert_traj_close(r.u_norm, chain[-1], what=f"step {it}")
        for m in range(M):
            g = chain[:, m * n:(m + 1) * n]
            u = onorm.unnormalize(g, torch.from_numpy(amin), torch.from_numpy(amax))[-1]
            cost = np.asarray(osys.rollout_cost("double_int2d", x[m], u.double().numpy()), dtype=np.float64)
            j = int(r.index[m]) - m * n
            assert 0 <= j < n
            np.testing.assert_allclose(r.cost[m], cost[j], rtol=1e-4)
            best = int(osys.argmin(cost))
            second = np.partition(cost, 1)[1] if n > 1 else np.inf
            if second - cost[best] > 1e-4 * abs(cost[best]):
                assert j == best, (it, m)
            if j == best:
                u0 = np.array([round(float(v), 4) for v in u[best, 0]])
                assert np.abs(r.u[m] - u0).max() <= 1.01e-4
        # the external plant: the model's step under the applied action, then a disturbance
        x = np.stack([osys.step("double_int2d", x[m], r.u[m]) for m in range(M)]) + rng.normal(0, 0.05, x.shape)


# ---- 5. ties and NaNs

def test_ties_across_workgroups_go_to_the_lowest_index():
    M, n = 2, 130
    g = torch.Generator().manual_seed(5)
    z = torch.randn(NSTEPS + 1, M, 1, H, D, generator=g).expand(-1, -1, n, -1, -1).reshape(NSTEPS + 1, M * n, H, D)
    r = _plan().mpc_step_batch(_x0(M), _di(), n, noise=z)
    np.testing.assert_array_equal(r.index, np.arange(M) * n)


def _assert_states_equal(a, b, states):
    for f in ("u", "plan", "cost", "index", "flags"):
        for m in states:
            np.testing.assert_array_equal(getattr(a, f)[m], getattr(b, f)[m], err_msg=f"{f}[{m}]")


def test_nan_candidate_never_wins():
    M, n, state, cand = 3, 80, 1, 70
    clean = _noises(M, n, [NSTEPS + 1])[0]
    dirty = clean.clone()
    dirty[0, state * n + cand, 3, 1] = float("nan")  # this candidate's chain, samples and cost
    plan = _plan()
    want = plan.mpc_step_batch(_x0(M), _di(), n, noise=clean)
    got = plan.mpc_step_batch(_x0(M), _di(), n, noise=dirty)
    assert got.index[state] != state * n + cand and np.isfinite(got.cost).all()
    assert got.flags[state] & NAN_SAMPLES and not got.flags[state] & NONFINITE
    _assert_states_equal(got, want, (0, 2))


def _all_nan_noise(M, n, state):
    clean = _noises(M, n, [NSTEPS + 1])[0]
    dirty = clean.clone()
    dirty[0, state * n:(state + 1) * n, 3, 1] = float("nan")
    return clean, dirty


def _c_args(plan, sysm, M, n, keep):
    """a valid cold argument block of mpcd_mpc_step_batch (Philox) with its host outputs in `keep`"""
    a = N.BatchStepArgs()
    desc = sysm.desc()
    a.sys = ctypes.pointer(desc)
    a.ctx_min, a.ctx_max = plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data
    a.act_min, a.act_max = plan.act_min.ctypes.data, plan.act_max.ctypes.data
    a.sample.sampler, a.sample.w = N.MPCD_DDPM_CFG, 0.01
    a.n_states, a.group, a.decimals = M, n, 4
    keep["desc"] = desc
    keep["x"] = np.ascontiguousarray(_x0(M, sysm.n_x))
    keep["rec"] = np.zeros((M, 3), dtype=np.int64)  # mpcd_state_result: 24 bytes
    keep["u"] = np.zeros((M, sysm.n_u))
    a.x_host, a.result_host, a.u_host = keep["x"].ctypes.data, keep["rec"].ctypes.data, keep["u"].ctypes.data
    return a


def test_all_nan_state_is_reported_and_the_others_stand():
    M, n, state = 3, 80, 1
    clean, dirty = _all_nan_noise(M, n, state)
    plan = _new_plan()
    want = plan.mpc_step_batch(_x0(M), _di(), n, noise=clean, warm_start=K)
    assert plan.batch_priors() is not None
    warm_dirty = clean[:K + 1].clone()  # the second warm-enabled step samples K steps from the priors
    warm_dirty[0, state * n:(state + 1) * n, 3, 1] = float("nan")
    with pytest.raises(N.MpcdError) as err:
        plan.mpc_step_batch(_x0(M), _di(), n, noise=warm_dirty, warm_start=K)
    assert err.value.status == N.MPCD_ENONFINITE
    assert plan.batch_priors() is None
    # the C call: MPCD_ENONFINITE, every output written
    keep = {}
    a = _c_args(plan, _di(), M, n, keep)
    z = dirty.to(plan.device)
    a.sample.noise = z.data_ptr()
    torch.cuda.synchronize()
    assert plan._lib.mpcd_mpc_step_batch(plan._ctx, ctypes.byref(a), None) == N.MPCD_ENONFINITE
    assert b"finite" in plan._lib.mpcd_last_error()
    got = plan.mpc_step_batch(_x0(M), _di(), n, noise=dirty, warm_start=K, allow_nonfinite=True)
    assert got.flags[state] & NONFINITE and got.flags[state] & NAN_SAMPLES and not np.isfinite(got.cost[state])
    assert got.index[state] == state * n
    assert not (got.flags[[0, 2]] & (NONFINITE | NAN_SAMPLES)).any()
    _assert_states_equal(got, want, (0, 2))
    rec = keep["rec"].view(np.dtype([("cost", "<f8"), ("index", "<i8"), ("flags", "<i4"), ("reserved", "<i4")]))[:, 0]
    np.testing.assert_array_equal(rec["cost"], got.cost)
    np.testing.assert_array_equal(rec["index"], got.index)
    np.testing.assert_array_equal(rec["flags"], got.flags)
    assert not rec["reserved"].any()
    np.testing.assert_array_equal(keep["u"], got.u)
    # the kept priors were dropped: the next warm-enabled step is cold (and clean: the counters were left reset)
    assert plan.batch_priors() is None
    again = plan.mpc_step_batch(_x0(M), _di(), n, noise=clean, warm_start=K)
    _assert_states_equal(again, want, range(M))


# ---- 6. reset mask

def test_reset_mask_splits_cold_and_warm():
    M, n = 5, 16
    plan = _new_plan()
    di = _di()
    mask = np.array([False, True, False, False, True])
    ic, iw = np.flatnonzero(mask), np.flatnonzero(~mask)
    z0 = _noises(M, n, [NSTEPS + 1], seed=1)[0]
    zc = _noises(len(ic), n, [NSTEPS + 1], seed=2)[0]
    zw = _noises(len(iw), n, [K + 1], seed=3)[0]
    x0, x1 = _x0(M), _x0(M) * 0.7
    plan.mpc_step_batch(x0, di, n, noise=z0, warm_start=K)
    before = plan.batch_priors().clone()
    got = plan.mpc_step_batch(x1, di, n, noise=(zc, zw), warm_start=K, reset=mask, return_samples=True)
    after = plan.batch_priors().clone()
    # the masked states alone, cold
    plan.reset_warm_start()
    cold = plan.mpc_step_batch(x1[ic], di, n, noise=zc, warm_start=K, return_samples=True)
    cold_priors = plan.batch_priors().clone()
    # the others alone, warm from their priors
    plan.set_batch_priors(before[torch.from_numpy(iw).to(plan.device)])
    warm = plan.mpc_step_batch(x1[iw], di, n, noise=zw, warm_start=K, return_samples=True)
    warm_priors = plan.batch_priors().clone()
    for idx, sub, pri in ((ic, cold, cold_priors), (iw, warm, warm_priors)):
        for f in ("u", "plan", "cost", "flags"):
            np.testing.assert_array_equal(getattr(got, f)[idx], getattr(sub, f), err_msg=f)
        np.testing.assert_array_equal(got.index[idx] - idx * n, sub.index - np.arange(len(idx)) * n)
        t = torch.from_numpy(idx).to(plan.device)
        assert torch.equal(after[t], pri)
        assert torch.equal(got.u_norm.view(M, n, H, D)[t], sub.u_norm.view(len(idx), n, H, D))
    _check_priors_of(plan, got, after)
    with pytest.raises(ValueError, match="pair"):
        plan.set_batch_priors(before)
        plan.mpc_step_batch(x1, di, n, noise=zc, warm_start=K, reset=mask)
    with pytest.raises(ValueError, match="reset"):
        plan.mpc_step_batch(x1, di, n, warm_start=K, reset=np.zeros(M + 1, dtype=bool))


def _check_priors_of(plan, r, priors):
    assert torch.equal(priors, plan.shift_plans(r.u_norm, torch.from_numpy(r.index).to(plan.device)))


# ---- 7. workspace reuse

def test_workspace_reuse():
    plan = _new_plan()
    small, large = _noises(5, 16, [NSTEPS + 1])[0], _noises(3, 80, [NSTEPS + 1])[0]
    first = plan.mpc_step_batch(_x0(5), _di(), 16, noise=small)
    plan.mpc_step_batch(_x0(3), _di(), 80, noise=large)
    third = plan.mpc_step_batch(_x0(5), _di(), 16, noise=small)
    _assert_states_equal(first, third, range(5))


# ---- 8. the C ABI's argument checks and refusals

def _call(plan, a):
    return plan._lib.mpcd_mpc_step_batch(plan._ctx, ctypes.byref(a), None)


@pytest.mark.parametrize("field,value,word", [
    ("sys", None, b"null"), ("ctx_min", None, b"null"), ("ctx_max", None, b"null"), ("act_min", None, b"null"),
    ("act_max", None, b"null"), ("x_host", None, b"null"), ("result_host", None, b"null"), ("u_host", None, b"null"),
    ("n_states", 0, b"n_states"), ("group", 0, b"group"), ("clip_rule", N.MPCD_CLIP_NONE, b"clip_rule"),
    ("clip_rule", 7, b"clip_rule"), ("decimals", 16, b"decimals"), ("warm_t_start", -1, b"warm_t_start"),
    ("warm_t_start", NSTEPS + 1, b"warm_t_start"), ("warm_t_start", 5, b"priors")])
def test_c_abi_einval(field, value, word):
    plan, keep = _plan(), {}
    a = _c_args(plan, _di(), 2, 4, keep)
    if field == "sys":
        a.sys = ctypes.POINTER(N.SystemDesc)()
    else:
        setattr(a, field, value)
    assert _call(plan, a) == -1
    assert word in plan._lib.mpcd_last_error()


def test_c_abi_einval_null_and_mismatch():
    plan, keep = _plan(), {}
    assert plan._lib.mpcd_mpc_step_batch(plan._ctx, None, None) == -1
    assert plan._lib.mpcd_mpc_step_batch(None, ctypes.byref(_c_args(plan, _di(), 2, 4, keep)), None) == -1
    a = _c_args(plan, systems.get("pendulum"), 2, 4, keep)  # n_u = 1, n_x = 2 against the net's 2 and 4
    assert _call(plan, a) == -1
    assert b"n_u" in plan._lib.mpcd_last_error()
    zoh = systems.get("cartpole_zoh4")  # n_x = 4 as the net's context, n_u = 1
    net = make_mlp(1, 32, 5, seed=1)
    p5 = DiffusionMPC(NetSpec("mlp", 1, 32, 5), net.state_dict(), variance_schedule="exponential",
                      n_diffusion_steps=NSTEPS)
    assert _call(p5, _c_args(p5, zoh, 2, 4, keep)) == -1  # n_u matches, n_x 4 != context_dim 5
    assert b"n_x" in p5._lib.mpcd_last_error()


def test_c_abi_eunsup():
    keep = {}
    plan, di = _plan(), _di()
    a = _c_args(plan, di, 2, 4, keep)
    pri = torch.zeros(2, H, D, device=plan.device)
    a.sample.sampler, a.warm_t_start, a.priors = N.MPCD_DDIM_CFG, 5, pri.data_ptr()
    assert _call(plan, a) == -5
    assert b"CFG-DDPM" in plan._lib.mpcd_last_error()
    h2 = _plan("f16x2")
    assert _call(h2, _c_args(h2, di, 2, 4, keep)) == -5
    assert b"F16X2" in h2._lib.mpcd_last_error()
    lb = _new_plan()
    N.check(lb._lib.mpcd_comm_init_loopback(lb._ctx, 1, 0, 0x5eed), "mpcd_comm_init_loopback")
    assert _call(lb, _c_args(lb, di, 2, 4, keep)) == -5
    assert b"communicator" in lb._lib.mpcd_last_error()
    # H * n_u = 256 floats per candidate: 64 rows of 257 floats exceed the tail's 64 KiB of LDS
    pend = systems.get("pendulum")
    net = make_unet(1, 2, seed=3)
    big = DiffusionMPC(NetSpec("unet", 1, 256, 2), net.state_dict(), variance_schedule="cosine", n_diffusion_steps=10)
    assert _call(big, _c_args(big, pend, 2, 4, keep)) == -5
    assert b"too large" in big._lib.mpcd_last_error()


def test_python_refusals():
    di = _di()
    with pytest.raises(ValueError, match="f16x2"):
        _plan("f16x2").mpc_step_batch(_x0(2), di, 8)
    with pytest.raises(ValueError, match="warm_start"):
        _plan().mpc_step_batch(_x0(2), di, 8, sample_fn="ddim_cfg", warm_start=5)
    with pytest.raises(ValueError, match="select"):
        _plan().mpc_step_batch(_x0(2), di, 8, select="best")
    with pytest.raises(ValueError, match="clip_rule"):
        _plan().mpc_step_batch(_x0(2), di, 8, clip_rule="none")
    with pytest.raises(ValueError, match="columns"):
        _plan().mpc_step_batch(_x0(2, 3), di, 8)
    with pytest.raises(ValueError, match="noise"):
        _plan().mpc_step_batch(_x0(2), di, 8, noise=torch.zeros(NSTEPS, 16, H, D))
