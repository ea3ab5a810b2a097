"""GPU: mpc_step_batch(warm_start=K, elites=k) - one mpcd_mpc_step_batch_elite call per control step: the batched
external step whose fused tail (batch_step_elite_tail_kernel) also ranks each state's k best candidates, followed by one
mpcd_elite_priors launch for the per-candidate priors - against the composed closed loop with elites fed its own
states, mpcd_topk over mpcd_rollout_cost_grouped's costs and mpcd_elite_priors. The step and its references run the
same kernels and the same fp64 operations per candidate, so every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
from mpc_via_diffusion_model_amd import _native as N

from ._systems_ref import TAIL_DESCRIPTORS
from ._util import make_mlp, make_unet

pytestmark = pytest.mark.gpu

H, D, C, NSTEPS, T, K = 16, 2, 4, 25, 3, 10
LIMITS = (-2 * np.ones(C), 2 * np.ones(C))
CLIPPED, NAN_SAMPLES, NONFINITE = N.MPCD_STEP_CLIPPED, N.MPCD_STEP_NAN_SAMPLES, N.MPCD_STEP_NONFINITE_WINNER
# a partial wave; single lanes; every candidate of a full wave an elite; two workgroups with a tail; k above the second
# workgroup's 16 candidates (a partial list shorter than k); three workgroups, the last with 2 candidates, k =
# MPCD_MAX_ELITES; 65 workgroups (a lane owns two lists)
SHAPES = [(5, 16, 3), (4, 1, 1), (2, 64, 64), (3, 80, 8), (3, 80, 20), (1, 130, 64), (1, 4160, 8)]


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


def _noises(M, n, slices, seed=17):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, M * n, H, D, generator=g) for s in slices]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _cost_ref(plan, sysm, x, n, r, clip_rule="chain", grouped=False, prior=None, **skw):
    """mpcd_clip_flags + mpcd_rollout_cost_grouped on the step's samples r.u_norm: fp64 [M * n] on the device. The
    chain rule's clip test reads the chain maxima, which the step does not return: the step's sampler call is run
    again for them (its samples must be the step's)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    M, nx = x.shape
    B, dev, st = M * n, plan.device, plan._stream()
    Hs, d = plan.spec.horizon, plan.spec.state_dim
    flags = torch.empty(M, dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    xd = torch.from_numpy(x).to(dev)
    if clip_rule == "chain":
        ctx = torch.empty((M, nx), dtype=torch.float32, device=dev)
        N.check(plan._lib.mpcd_normalize_states(plan._ctx, _ptr(xd), M, nx, plan.ctx_min.ctypes.data,
                                                plan.ctx_max.ctypes.data, _ptr(ctx), st), "mpcd_normalize_states")
        grouped = bool(grouped) and plan.grouped_pays(M, n)
        absmax = torch.empty(B, dtype=torch.float32, device=dev)
        warm = {} if prior is None else dict(x_init=prior.reshape(B, Hs, d), t_start=skw.pop("t_start"))
        skw.pop("t_start", None)
        u = plan.sample_trajectories(ctx if grouped else ctx.repeat_interleave(n, dim=0), B, Hs, absmax_out=absmax,
                                     context_group=n if grouped else None, **warm, **skw)
        assert torch.equal(u.view(torch.int32), r.u_norm.view(torch.int32))
        N.check(plan._lib.mpcd_clip_flags(plan._ctx, _ptr(absmax), M, n, _ptr(flags), st), "mpcd_clip_flags")
    else:
        N.check(plan._lib.mpcd_clip_flags(plan._ctx, _ptr(r.u_norm), M, n * Hs * d, _ptr(flags), st), "mpcd_clip_flags")
    desc = sysm.desc()
    N.check(plan._lib.mpcd_rollout_cost_grouped(plan._ctx, ctypes.byref(desc), _ptr(xd), n, _ptr(r.u_norm),
                                                plan.act_min.ctypes.data, plan.act_max.ctypes.data, B, Hs, _ptr(flags),
                                                _ptr(cost), st), "mpcd_rollout_cost_grouped")
    return cost


def _check_elites(plan, r, cost_ref, M, n, k):
    want_c, want_i = plan.topk(cost_ref, k, n_groups=M)
    assert r.elite_index.shape == (M, k) and r.elite_index.dtype == np.int64 and r.elite_cost.dtype == np.float64
    np.testing.assert_array_equal(r.elite_index, want_i.cpu().numpy())
    np.testing.assert_array_equal(r.elite_cost.view(np.int64), want_c.cpu().numpy().view(np.int64))
    np.testing.assert_array_equal(r.elite_index[:, 0], r.index)
    pri = plan.batch_priors()
    Hs, d = plan.spec.horizon, plan.spec.state_dim
    assert tuple(pri.shape) == (M, n, Hs, d)
    want_p = plan.elite_priors(r.u_norm, want_i, n)
    assert torch.equal(pri.view(M * n, Hs, d).view(torch.int32), want_p.view(torch.int32))


def _steps_vs_loop(plan, M, n, k, noises, sysm=None, x0=None, seed=0, n_wo_noise=0, **kw):
    """closed_loop(native=False, elites=k) once, then one mpc_step_batch(elites=k) per iteration on its states"""
    sysm = sysm or _di()
    x0 = _x0(M) if x0 is None else x0
    noise = None if noises is None else (lambda it: noises[it])
    ref = plan.closed_loop(x0, sysm, T, n_samples=n, noise=noise, seed=seed, native=False, warm_start=K, elites=k,
                           n_wo_noise=n_wo_noise, **kw)
    plan.reset_warm_start()
    out = []
    for it in range(T):
        z = None if noises is None else noises[it]
        before = plan.batch_priors()
        before = None if before is None else before.clone()
        r = plan.mpc_step_batch(ref.x[:, it], sysm, n, seed=seed + it, noise=z, warm_start=K, elites=k,
                                return_samples=True, n_wo_noise=n_wo_noise, **kw)
        assert (before is None) == (it == 0)
        for f in ("u", "cost", "index"):
            np.testing.assert_array_equal(getattr(r, f), getattr(ref, f)[:, it], err_msg=f"{f}[{it}]")
        cost_ref = _cost_ref(plan, sysm, ref.x[:, it], n, r, kw.get("clip_rule", "chain"), kw.get("grouped", False), before,
                             seed=seed + it, noise=z, n_wo_noise=n_wo_noise, t_start=K)
        _check_elites(plan, r, cost_ref, M, n, k)
        out.append(r)
    return ref, out


# ---- 1. equals the composed closed loop with elites, fed its states

@pytest.mark.parametrize("M,n,k", SHAPES)
def test_equals_closed_loop_shapes(M, n, k):
    _steps_vs_loop(_plan(), M, n, k, _noises(M, n, [NSTEPS + 1] + [K + 1] * (T - 1)))


@pytest.mark.parametrize("clip_rule", ["chain", "final"])
def test_equals_closed_loop_clip_rules(clip_rule):
    M, n, k = 3, 80, 8
    _, out = _steps_vs_loop(_plan(), M, n, k, _noises(M, n, [NSTEPS + 1] + [K + 1] * (T - 1), seed=23),
                            clip_rule=clip_rule)
    if clip_rule == "chain":
        assert any((r.flags & CLIPPED).any() for r in out)  # x_T ~ N(0, 1) is inside the tested chain


def test_equals_closed_loop_philox():
    _steps_vs_loop(_plan(), 3, 80, 8, None, seed=5)


@pytest.mark.parametrize("grouped", [True, False])
def test_equals_closed_loop_split_bf16(grouped):
    M, n, k = 3, 20, 4
    plan = _plan("f32x3")
    assert plan.grouped_pays(M, n)
    _steps_vs_loop(plan, M, n, k, _noises(M, n, [NSTEPS + 1] + [K + 1] * (T - 1)), grouped=grouped)


def test_equals_closed_loop_n_wo_noise():
    M, n, k = 3, 20, 4
    _steps_vs_loop(_plan(), M, n, k, _noises(M, n, [NSTEPS + 3] + [K + 3] * (T - 1)), n_wo_noise=2)


# ---- 2. one elite is the warm start

def test_one_elite_equals_warm_start_alone():
    M, n = 3, 80
    a, b = _new_plan(), _new_plan()
    noises = _noises(M, n, [NSTEPS + 1] + [K + 1] * (T - 1))
    for it in range(T):
        x = _x0(M) * (1 - 0.2 * it)
        ra = a.mpc_step_batch(x, _di(), n, noise=noises[it], warm_start=K)
        rb = b.mpc_step_batch(x, _di(), n, noise=noises[it], warm_start=K, elites=1)
        for f in ("u", "plan", "cost", "index", "flags"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f"{f}[{it}]")
        assert ra.elite_index is None and ra.elite_cost is None
        np.testing.assert_array_equal(rb.elite_index[:, 0], ra.index)
        pa, pb = a.batch_priors(), b.batch_priors()
        assert tuple(pa.shape) == (M, H, D) and tuple(pb.shape) == (M, n, H, D)
        assert torch.equal(pb.view(torch.int32), pa[:, None].expand(M, n, H, D).contiguous().view(torch.int32))


# ---- 3. every system

@pytest.mark.parametrize("name", ["cartpole_lin5", "cartpole_nl5", "cartpole_zoh4", "pendulum", "quadrotor12"])
def test_every_system_and_cost_kind(name):
    """the elite tail's other five instantiations: a net of the system's sizes, Philox noise, two workgroups with a
    tail per state, a warm sequence"""
    _system_case(systems.get(name))


def _system_case(sysm):
    d, Cx, Hs, M, n, k = sysm.n_u, sysm.n_x, 32 // min(sysm.n_u, 2), 3, 80, 4
    net = make_mlp(d, Hs, Cx, seed=9)
    plan = DiffusionMPC(NetSpec("mlp", d, Hs, Cx), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=(-2 * np.ones(Cx), 2 * np.ones(Cx)))
    x0 = np.random.default_rng(4).uniform(-0.3, 0.3, (M, Cx))
    ref, _ = _steps_vs_loop(plan, M, n, k, None, sysm=sysm, x0=x0, seed=2)
    assert np.isfinite(ref.cost).all()


@pytest.mark.parametrize("which", sorted(TAIL_DESCRIPTORS))
def test_non_default_descriptor(which):
    """the same harness at a descriptor that is not the registry's (tests/_systems_ref.py: every constant distinct and
    non-zero, a set-point that is non-zero everywhere; the nonlinear cart-pole under calMPCCost)"""
    _system_case(TAIL_DESCRIPTORS[which]())


# ---- 4. ties across workgroups

def test_ties_across_workgroups_go_to_the_lower_index():
    M, n, k = 2, 130, 16
    g = torch.Generator().manual_seed(5)
    z7 = torch.randn(NSTEPS + 1, M, 7, H, D, generator=g)
    z = z7[:, :, torch.arange(n) % 7].reshape(NSTEPS + 1, M * n, H, D).contiguous()  # candidate j copies j mod 7
    plan = _new_plan()
    r = plan.mpc_step_batch(_x0(M), _di(), n, noise=z, warm_start=K, elites=k, return_samples=True)
    cost = _cost_ref(plan, _di(), _x0(M), n, r, noise=z).cpu().view(M, n)
    for m in range(M):
        assert len(np.unique(cost[m].numpy())) <= 7  # the input does contain duplicates
    assert torch.isfinite(cost).all()
    v, i = torch.sort(cost, dim=1, stable=True)  # by (cost, index)
    np.testing.assert_array_equal(r.elite_index, (i[:, :k] + torch.arange(M)[:, None] * n).numpy())
    np.testing.assert_array_equal(r.elite_cost, v[:, :k].numpy())
    assert (np.diff(r.elite_index[:, :3], axis=1) == 7).all()  # the best plan's copies: j, j + 7, j + 14


# ---- 5. NaNs

def _assert_states_equal(a, b, states, fields=("u", "plan", "cost", "index", "flags", "elite_index", "elite_cost")):
    for f in fields:
        for m in states:
            np.testing.assert_array_equal(getattr(a, f)[m], getattr(b, f)[m], err_msg=f"{f}[{m}]")


def test_nan_candidate_is_in_no_elite_list():
    M, n, k, state, cand = 3, 80, 8, 1, 70
    clean = _noises(M, n, [NSTEPS + 1])[0]
    dirty = clean.clone()
    dirty[0, state * n + cand, 3, 1] = float("nan")  # this candidate's chain, samples and cost
    plan = _new_plan()
    want = plan.mpc_step_batch(_x0(M), _di(), n, noise=clean, warm_start=K, elites=k)
    plan.reset_warm_start()
    got = plan.mpc_step_batch(_x0(M), _di(), n, noise=dirty, warm_start=K, elites=k)
    assert state * n + cand not in got.elite_index and np.isfinite(got.elite_cost).all() and np.isfinite(got.cost).all()
    assert got.flags[state] & NAN_SAMPLES and not got.flags[state] & NONFINITE
    _assert_states_equal(got, want, (0, 2))


def test_all_nan_state_is_reported_and_the_others_stand():
    M, n, k, state = 3, 80, 8, 1
    clean = _noises(M, n, [NSTEPS + 1])[0]
    dirty = clean.clone()
    dirty[0, state * n:(state + 1) * n, 3, 1] = float("nan")
    plan = _new_plan()
    want = plan.mpc_step_batch(_x0(M), _di(), n, noise=clean, warm_start=K, elites=k)
    assert plan.batch_priors() is not None
    warm_dirty = clean[:K + 1].clone()
    warm_dirty[0, state * n:(state + 1) * n, 3, 1] = float("nan")
    with pytest.raises(N.MpcdError) as err:
        plan.mpc_step_batch(_x0(M), _di(), n, noise=warm_dirty, warm_start=K, elites=k)
    assert err.value.status == N.MPCD_ENONFINITE
    assert plan.batch_priors() is None  # the kept priors are dropped
    got = plan.mpc_step_batch(_x0(M), _di(), n, noise=dirty, warm_start=K, elites=k, allow_nonfinite=True)
    assert plan.batch_priors() is None
    assert got.flags[state] & NONFINITE and got.flags[state] & NAN_SAMPLES and not np.isfinite(got.cost[state])
    assert not (got.flags[[0, 2]] & (NONFINITE | NAN_SAMPLES)).any()
    np.testing.assert_array_equal(got.elite_index[state], state * n + np.arange(k))
    assert np.isposinf(got.elite_cost[state]).all()
    _assert_states_equal(got, want, (0, 2))
    again = plan.mpc_step_batch(_x0(M), _di(), n, noise=clean, warm_start=K, elites=k)  # cold, counters left reset
    _assert_states_equal(again, want, range(M))


# ---- 6. reset mask

def test_reset_mask_with_elites():
    M, n, k = 5, 16, 3
    plan = _new_plan()
    di = _di()
    mask = np.array([False, True, False, False, True])
    ic, iw = np.flatnonzero(mask), np.flatnonzero(~mask)
    z0 = _noises(M, n, [NSTEPS + 1], seed=1)[0]
    zc = _noises(len(ic), n, [NSTEPS + 1], seed=2)[0]
    zw = _noises(len(iw), n, [K + 1], seed=3)[0]
    x0, x1 = _x0(M), _x0(M) * 0.7
    kw = dict(warm_start=K, elites=k, return_samples=True)
    plan.mpc_step_batch(x0, di, n, noise=z0, **kw)
    before = plan.batch_priors().clone()
    got = plan.mpc_step_batch(x1, di, n, noise=(zc, zw), reset=mask, **kw)
    after = plan.batch_priors().clone()
    assert tuple(after.shape) == (M, n, H, D)
    plan.reset_warm_start()
    cold = plan.mpc_step_batch(x1[ic], di, n, noise=zc, **kw)
    cold_priors = plan.batch_priors().clone()
    plan.set_batch_priors(before[torch.from_numpy(iw).to(plan.device)])
    warm = plan.mpc_step_batch(x1[iw], di, n, noise=zw, **kw)
    warm_priors = plan.batch_priors().clone()
    for idx, sub, pri in ((ic, cold, cold_priors), (iw, warm, warm_priors)):
        for f in ("u", "plan", "cost", "flags", "elite_cost"):
            np.testing.assert_array_equal(getattr(got, f)[idx], getattr(sub, f), err_msg=f)
        local = np.arange(len(idx)) * n
        np.testing.assert_array_equal(got.index[idx] - idx * n, sub.index - local)
        np.testing.assert_array_equal(got.elite_index[idx] - (idx * n)[:, None], sub.elite_index - local[:, None])
        t = torch.from_numpy(idx).to(plan.device)
        assert torch.equal(after[t], pri)
        assert torch.equal(got.u_norm.view(M, n, H, D)[t], sub.u_norm.view(len(idx), n, H, D))
    assert ((got.elite_index // n) == np.arange(M)[:, None]).all()
    want = plan.elite_priors(got.u_norm, torch.from_numpy(got.elite_index).to(plan.device), n)
    assert torch.equal(after.view(M * n, H, D), want)


# ---- 7. transitions between the two kinds of prior set

def test_transitions():
    M, n, k = 3, 20, 4
    di, x = _di(), _x0(M)
    z0, z1 = _noises(M, n, [NSTEPS + 1, K + 1])
    dev = _plan().device
    # a stored [M, H, d] set, then an elite call: every candidate of a state starts from the state's one prior
    a, b = _new_plan(), _new_plan()
    a.mpc_step_batch(x, di, n, noise=z0, warm_start=K)
    one = a.batch_priors().clone()
    assert tuple(one.shape) == (M, H, D)
    ra = a.mpc_step_batch(x, di, n, noise=z1, warm_start=K, elites=k)
    assert tuple(a.batch_priors().shape) == (M, n, H, D)
    b.set_batch_priors(one[:, None].expand(M, n, H, D))  # rank 4
    assert tuple(b.batch_priors().shape) == (M, n, H, D)
    rb = b.mpc_step_batch(x, di, n, noise=z1, warm_start=K, elites=k)
    _assert_states_equal(ra, rb, range(M))
    assert torch.equal(a.batch_priors(), b.batch_priors())
    rw = _new_plan()
    rw.set_batch_priors(one)  # rank 3
    rc = rw.mpc_step_batch(x, di, n, noise=z1, warm_start=K)  # the same samples: the same winner and cost
    _assert_states_equal(ra, rc, range(M), ("u", "plan", "cost", "index", "flags"))
    # an elite set, then a plain call: row 0 of each state, the winner's
    four = a.batch_priors().clone()
    r1 = a.mpc_step_batch(x, di, n, noise=z1, warm_start=K)
    assert r1.elite_index is None and tuple(a.batch_priors().shape) == (M, H, D)
    b.set_batch_priors(four[:, 0])
    r2 = b.mpc_step_batch(x, di, n, noise=z1, warm_start=K)
    _assert_states_equal(r1, r2, range(M), ("u", "plan", "cost", "index", "flags"))
    assert torch.equal(a.batch_priors(), b.batch_priors())
    # M or n changed: a cold step
    cold = _new_plan()
    for M2, n2 in ((M, n + 4), (M + 1, n)):
        zc = _noises(M2, n2, [NSTEPS + 1], seed=9)[0]
        a.set_batch_priors(four)
        got = a.mpc_step_batch(_x0(M2), di, n2, noise=zc, warm_start=K, elites=k)
        cold.reset_warm_start()
        want = cold.mpc_step_batch(_x0(M2), di, n2, noise=zc, warm_start=K, elites=k)
        _assert_states_equal(got, want, range(M2))
        assert tuple(a.batch_priors().shape) == (M2, n2, H, D)
    with pytest.raises(ValueError, match="priors"):
        a.set_batch_priors(torch.zeros(M, H + 1, D, device=dev))
    with pytest.raises(ValueError, match="priors"):
        a.set_batch_priors(torch.zeros(H, D))
    a.set_batch_priors(None)
    assert a.batch_priors() is None


# ---- 8. workspace reuse

def test_workspace_reuse():
    plan = _new_plan()
    di = _di()
    small, large = _noises(5, 16, [NSTEPS + 1])[0], _noises(3, 200, [NSTEPS + 1])[0]

    def step(M, n, k, z):
        plan.reset_warm_start()
        return plan.mpc_step_batch(_x0(M), di, n, noise=z, warm_start=K, elites=k)

    big = step(3, 200, 64, large)
    first = step(5, 16, 3, small)
    second = step(5, 16, 3, small)
    _assert_states_equal(first, second, range(5))
    _assert_states_equal(step(3, 200, 64, large), big, range(3))
    fresh = _new_plan().mpc_step_batch(_x0(5), di, 16, noise=small, warm_start=K, elites=3)
    _assert_states_equal(first, fresh, range(5))
    plain = plan.mpc_step_batch(_x0(5), di, 16, noise=small)  # the plain call on the same workspace
    _assert_states_equal(plain, first, range(5), ("u", "plan", "cost", "index", "flags"))


# ---- 9. refusals

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


def _e_args(k=2):
    e = N.BatchEliteArgs()
    e.k = k
    return e


def _call(plan, a, e):
    return plan._lib.mpcd_mpc_step_batch_elite(plan._ctx, ctypes.byref(a), None if e is None else ctypes.byref(e), None)


@pytest.mark.parametrize("field,value,word", [
    ("sys", None, b"null"), ("ctx_min", None, b"null"), ("act_max", None, b"null"), ("x_host", None, b"null"),
    ("result_host", None, b"null"), ("u_host", None, b"null"), ("n_states", 0, b"n_states"), ("group", 0, b"group"),
    ("clip_rule", N.MPCD_CLIP_NONE, b"clip_rule"), ("decimals", 16, b"decimals"), ("warm_t_start", -1, b"warm_t_start"),
    ("warm_t_start", NSTEPS + 1, b"warm_t_start"), ("warm_t_start", 5, b"priors"), ("select_first", 1, b"select_first"),
    ("priors", 256, b"args->priors")])
def test_c_abi_einval_batch_fields(field, value, word):
    plan, keep = _plan(), {}
    a = _c_args(plan, _di(), 2, 4, keep)
    if field == "sys":
        a.sys = ctypes.POINTER(N.SystemDesc)()
    else:
        setattr(a, field, value)
    assert _call(plan, a, _e_args()) == -1
    assert word in plan._lib.mpcd_last_error()
    assert b"mpcd_mpc_step_batch_elite" in plan._lib.mpcd_last_error() or field in ("decimals", "warm_t_start")


@pytest.mark.parametrize("k", [0, -1, 5, 65])
def test_c_abi_einval_k(k):
    plan, keep = _plan(), {}
    n = 4 if k <= 5 else 80
    assert _call(plan, _c_args(plan, _di(), 2, n, keep), _e_args(k)) == -1
    assert b"k %d outside" % k in plan._lib.mpcd_last_error()


def test_c_abi_einval_elite_struct():
    plan, keep = _plan(), {}
    a = _c_args(plan, _di(), 2, 4, keep)
    assert _call(plan, a, None) == -1
    assert b"elite" in plan._lib.mpcd_last_error()
    e = _e_args()
    e.reserved = 1
    assert _call(plan, a, e) == -1
    assert b"reserved" in plan._lib.mpcd_last_error()
    assert plan._lib.mpcd_mpc_step_batch_elite(plan._ctx, None, ctypes.byref(_e_args()), None) == -1


def test_c_abi_eunsup():
    keep = {}
    plan, di = _plan(), _di()
    a = _c_args(plan, di, 2, 4, keep)
    pri = torch.zeros(8, H, D, device=plan.device)
    e = _e_args()
    e.priors = pri.data_ptr()
    a.sample.sampler, a.warm_t_start = N.MPCD_DDIM_CFG, 5
    assert _call(plan, a, e) == -5
    assert b"CFG-DDPM" in plan._lib.mpcd_last_error()
    h2 = _plan("f16x2")
    assert _call(h2, _c_args(h2, di, 2, 4, keep), _e_args()) == -5
    assert b"F16X2" in h2._lib.mpcd_last_error()
    lb = _new_plan()
    N.check(lb._lib.mpcd_comm_init_loopback(lb._ctx, 1, 0, 0x5eed), "mpcd_comm_init_loopback")
    assert _call(lb, _c_args(lb, di, 2, 4, keep), _e_args()) == -5
    assert b"communicator" in lb._lib.mpcd_last_error()
    pend = systems.get("pendulum")  # H * n_u = 256 floats per candidate exceed the tail's 64 KiB of LDS
    net = make_unet(1, 2, seed=3)
    big = DiffusionMPC(NetSpec("unet", 1, 256, 2), net.state_dict(), variance_schedule="cosine", n_diffusion_steps=10)
    assert _call(big, _c_args(big, pend, 2, 4, keep), _e_args()) == -5
    assert b"too large" in big._lib.mpcd_last_error()


def test_c_call_and_the_plain_call_unchanged():
    """the C entry point end to end (cold, Philox) against the Python wrapper, and mpcd_mpc_step_batch with its own
    struct on the same context"""
    M, n, k = 3, 80, 8
    plan, keep = _new_plan(), {}
    a = _c_args(plan, _di(), M, n, keep)
    e = _e_args(k)
    best = np.zeros((M, k, 2), dtype=np.int64)
    e.elites_host = best.ctypes.data
    torch.cuda.synchronize()
    assert _call(plan, a, e) == 0, plan._lib.mpcd_last_error()
    want = plan.mpc_step_batch(_x0(M), _di(), n, warm_start=K, elites=k)
    rec = keep["rec"].view(np.dtype([("cost", "<f8"), ("index", "<i8"), ("flags", "<i4"), ("reserved", "<i4")]))[:, 0]
    np.testing.assert_array_equal(rec["cost"], want.cost)
    np.testing.assert_array_equal(rec["index"], want.index)
    np.testing.assert_array_equal(keep["u"], want.u)
    np.testing.assert_array_equal(best[..., 1], want.elite_index)
    np.testing.assert_array_equal(best[..., 0], want.elite_cost.view(np.int64))
    keep2 = {}
    a2 = _c_args(plan, _di(), M, n, keep2)
    assert plan._lib.mpcd_mpc_step_batch(plan._ctx, ctypes.byref(a2), None) == 0, plan._lib.mpcd_last_error()
    np.testing.assert_array_equal(keep2["rec"], keep["rec"])
    np.testing.assert_array_equal(keep2["u"], keep["u"])


def test_python_refusals():
    di, plan = _di(), _plan()
    with pytest.raises(ValueError, match="warm_start"):
        plan.mpc_step_batch(_x0(2), di, 8, elites=2)
    with pytest.raises(ValueError, match="select"):
        plan.mpc_step_batch(_x0(2), di, 8, warm_start=K, elites=2, select="first")
    for k in (0, 9, 65):
        with pytest.raises(ValueError, match="elites"):
            plan.mpc_step_batch(_x0(2), di, 8 if k < 65 else 80, warm_start=K, elites=k)
