"""GPU: elite sets (mpcd_topk, mpcd_elite_priors, mpcd_mpc_step_elite; DiffusionMPC.topk / elite_priors,
mpc_step(warm_start=K, elites=k), closed_loop(warm_start=K, elites=k)).

What is checked: the ranked top-k against torch's stable sort on the host (NaN = +inf), exactly, with entry 0 the
device argmin's winner and nothing written past [M][k]; the prior writer against a torch gather bit for bit at every
vector width; the one-call step with one elite against the warm step of a twin planner, and with k elites against the
same step composed from the public calls with torch-built priors; the closed loop likewise; every refusal. Nothing here
has a tolerance: selection and copying do not round, and the sampler calls compared are the same kernels on the same
inputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
from mpc_via_diffusion_model_amd import _native as nat
from mpc_via_diffusion_model_amd import distributed as D
from mpc_via_diffusion_model_amd.planner import _STEP_CONTEXT

from ._util import make_mlp, make_unet
from .test_gpu_comm import _key

pytestmark = pytest.mark.gpu

# 25 denoise steps: the fewest at which the exponential schedule's fp32 tables are finite
C, N, K = 4, 25, 20
EINVAL, EUNSUP = -1, -5
STEP_X0 = (np.array([0.3, -0.2, 0.1, 0.05]), np.array([0.25, -0.1, 0.12, 0.0]), np.array([0.2, -0.05, 0.1, -0.02]))
SENTINEL = -(2 ** 62) + 12345  # as int64; its fp64 reading is a finite, very negative number


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _net(kind, H, d):
    return make_unet(d, C, seed=7) if kind == "unet" else make_mlp(d, H, C, seed=21)


def _step_plan(kind):
    """the warm-start tests' step planners: an MLP (H = 16, d = 2) of the given dtype, or their layer-by-layer U-Net
    (H = 8, d = 2)"""
    H, d = (8, 2) if kind == "unet" else (16, 2)
    spec = NetSpec("unet", d, H, C) if kind == "unet" else NetSpec("mlp", d, H, C, dtype=kind)
    return DiffusionMPC(spec, _net(kind, H, d).state_dict(), variance_schedule="exponential", n_diffusion_steps=N,
                        context_limits=(-2 * np.ones(C), 2 * np.ones(C)), action_limits=(-np.ones(d), np.ones(d)))


@functools.lru_cache(maxsize=None)
def _plan():
    return _step_plan("f32x3")


@functools.lru_cache(maxsize=None)
def _shape_plan(H, d):
    """mpcd_elite_priors takes the net's H and d: a net per shape"""
    return DiffusionMPC(NetSpec("unet", d, H, C), make_unet(d, C, seed=2).state_dict(), n_diffusion_steps=N)


def _shift(rows, shift=True):
    return torch.cat([rows[:, 1:], rows[:, -1:]], dim=1) if shift else rows


def _ref_topk(cost, M, k, off=0):
    """torch's stable sort of each group on the host, NaN as +inf: (cost [M, k], global index [M, k])"""
    c = cost.detach().cpu().view(M, -1)
    c = torch.where(torch.isnan(c), torch.full_like(c, float("inf")), c)
    v, i = torch.sort(c, dim=1, stable=True)
    base = off + torch.arange(M, dtype=torch.int64)[:, None] * c.shape[1]
    return v[:, :k].contiguous(), (i[:, :k] + base).contiguous()


# ------------------------------------------------------------------------------------------- 1. mpcd_topk
def _costs(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "duplicates":
        return torch.randint(0, 4, (n,), generator=g).double()
    if kind == "all_nan":
        return torch.full((n,), float("nan"), dtype=torch.float64)
    c = torch.randn(n, generator=g, dtype=torch.float64)
    if kind == "nan_inf":
        what = torch.randint(0, 8, (n,), generator=g)
        c[what == 0] = float("nan")
        c[what == 1] = float("inf")
        c[what == 2] = float("-inf")
    return c


@pytest.mark.parametrize("kind", ("random", "duplicates", "nan_inf", "all_nan", "offset"))
@pytest.mark.parametrize("M,group", ((3, 5), (2, 16), (1, 48), (2, 300), (1, 4096)))
def test_topk_is_the_stable_sort(M, group, kind):
    plan = _plan()
    off = 1000 if kind == "offset" else 0
    host = _costs(kind, M * group, seed=group + M)
    cost = host.cuda()
    for k in sorted({1, 3, min(group, 64), 64} & set(range(1, group + 1))):
        want_c, want_i = _ref_topk(host, M, k, off)
        got_c, got_i = plan.topk(cost, k, n_groups=M, index_offset=off)
        assert got_c.shape == (M, k) and got_c.dtype == torch.float64 and got_i.dtype == torch.int64 and got_c.is_cuda
        assert torch.equal(got_i.cpu(), want_i), f"indices, k = {k}"
        assert torch.equal(got_c.cpu().view(torch.int64), want_c.view(torch.int64)), f"costs, k = {k}"
        if kind == "all_nan":
            assert torch.isinf(got_c).all() and (got_c > 0).all()
            assert torch.equal(got_i.cpu(), torch.arange(M)[:, None] * group + torch.arange(k)[None])
        # the entry point itself, into the middle of a sentinel-filled buffer
        pad = 4
        raw = torch.full((M * k + 2 * pad, 2), SENTINEL, dtype=torch.int64, device="cuda")
        rc = plan._lib.mpcd_topk(plan._ctx, _ptr(cost), M, group, k, off, _ptr(raw[pad:]), plan._stream())
        torch.cuda.synchronize()
        assert rc == 0, plan._lib.mpcd_last_error()
        assert (raw[:pad] == SENTINEL).all() and (raw[pad + M * k:] == SENTINEL).all(), "written outside [M][k]"
        body = raw[pad:pad + M * k].view(M, k, 2).cpu()
        assert torch.equal(body[..., 1], want_i) and torch.equal(body[..., 0], want_c.view(torch.int64))
    for m in range(M):  # entry 0 is mpcd_argmin's winner on the same slice
        idx, best = plan.argmin(cost[m * group:(m + 1) * group], index_offset=off + m * group)
        got_c, got_i = plan.topk(cost, 1, n_groups=M, index_offset=off)
        assert int(got_i[m, 0]) == idx
        assert np.float64(best).view(np.int64) == np.float64(float(got_c[m, 0])).view(np.int64)


# ----------------------------------------------------------------------------------- 2. mpcd_elite_priors
@pytest.mark.parametrize("shift", (True, False))
@pytest.mark.parametrize("M,group,k", ((3, 5, 3), (1, 300, 8), (2, 16, 16)))
@pytest.mark.parametrize("H,d", ((8, 1), (8, 2), (8, 4), (16, 1), (16, 2), (16, 4)))
def test_elite_priors_is_the_gather(H, d, M, group, k, shift):
    plan = _shape_plan(H, d)
    B, off, pad = M * group, 100, 2
    g = torch.Generator().manual_seed(H * d + B)
    u = torch.randn(B, H, d, generator=g).cuda()
    idx = torch.stack([m * group + torch.randint(0, group, (k,), generator=g) for m in range(M)])  # rows of u
    big = torch.full((B + pad, H, d), 55.0, device="cuda")
    got = plan.elite_priors(u, (idx + off).cuda(), group, shift=shift, index_offset=off, out=big[:B])
    torch.cuda.synchronize()
    j = torch.arange(B) % group % k
    rows = idx[torch.arange(B) // group, j]
    assert _same(got, _shift(u, shift)[rows.cuda()]), "not the gather of the elites' plans"
    assert (big[B:] == 55.0).all(), "written past the batch"
    if shift:  # one elite: every candidate of the state gets shift_plans' row
        one = plan.elite_priors(u, (idx[:, :1] + off).cuda(), group, index_offset=off)
        want = plan.shift_plans(u, (idx[:, 0] + off).cuda(), off).repeat_interleave(group, 0)
        assert _same(one, want)


def test_elite_priors_skips_indices_outside_the_batch():
    H, d, M, group, k, off = 16, 2, 3, 5, 3, 100
    plan, B = _plan(), 15
    u = torch.randn(B, H, d, generator=torch.Generator().manual_seed(3)).cuda()
    idx = torch.tensor([[0, 1, 2], [7, -1, 5], [B, 12, 14]], dtype=torch.int64) + off  # two outside [off, off + B)
    out = torch.full((B + 1, H, d), 55.0, device="cuda")
    plan.elite_priors(u, idx.cuda(), group, index_offset=off, out=out[:B])
    torch.cuda.synchronize()
    sh = _shift(u)
    for b in range(B):
        e = int(idx[b // group, b % group % k]) - off
        if 0 <= e < B:
            assert _same(out[b], sh[e]), b
        else:
            assert (out[b] == 55.0).all(), f"candidate {b}: an elite outside the batch must leave its rows untouched"
    assert (out[B:] == 55.0).all()


# -------------------------------------------------------------- 3. one elite is the shared prior's chain
@pytest.mark.parametrize("kind", ("f32x3", "f32", "f16x2", "unet"))
def test_one_elite_equals_the_warm_step(kind):
    B, sysm = 48, systems.double_int2d()
    twin, plan = _step_plan(kind), _step_plan(kind)
    for s, x0 in enumerate(STEP_X0):
        w = twin.mpc_step(x0, sysm, B, w=0.01, seed=20 + s, warm_start=K)
        r = plan.mpc_step(x0, sysm, B, w=0.01, seed=20 + s, warm_start=K, elites=1)
        torch.cuda.synchronize()
        assert (r.best_index, r.best_cost, r.flags) == (w.best_index, w.best_cost, w.flags), f"step {s}"
        np.testing.assert_array_equal(r.u_best, w.u_best)
        np.testing.assert_array_equal(r.u0, w.u0)
        assert _same(r.u_norm, w.u_norm) and torch.equal(r.costs, w.costs), f"step {s}"
        assert r.elite_index.shape == (1,) and int(r.elite_index[0]) == r.best_index and r.elite_cost[0] == r.best_cost
        assert w.elite_index is None and w.elite_cost is None
        assert _same(plan.warm_prior(), twin.warm_prior()), f"step {s}: row 0 is not the shifted winner"
        assert plan._prior.shape == (B, 16 if kind != "unet" else 8, 2)
        assert _same(plan._prior, twin._prior.expand(B, -1, -1)), f"step {s}: the priors are not B copies of it"


# ------------------------------------------------------------------ 4. k elites against the composed step
@pytest.mark.parametrize("k", (3, 8))
def test_elite_step_equals_the_composed_step(k):
    B, H, d, nwo, sysm = 48, 16, 2, 2, systems.double_int2d()
    ref, plan = _step_plan("f32x3"), _step_plan("f32x3")
    g = torch.Generator().manual_seed(5)
    priors = None
    for s, x0 in enumerate(STEP_X0):
        S = (N if s == 0 else K) + nwo
        assert ref.n_denoise_steps(n_wo_noise=nwo, t_start=None if s == 0 else K) == S
        noise = torch.randn(S + 1, B, H, d, generator=g)  # after step 0: K + n_wo_noise + 1 slices
        # composed: the public calls, the priors built in torch from the previous step's costs
        ctx = torch.from_numpy(ref.normalize_condition(x0)[None])
        am = torch.empty(B, dtype=torch.float32, device="cuda")
        u_norm = ref.sample_trajectories(ctx, B, H, w=0.01, noise=noise, absmax_out=am, n_wo_noise=nwo, x_init=priors,
                                         t_start=None if s == 0 else K)
        flag = ref.clip_flag(am)
        cost = ref.rollout_cost(sysm, x0, u_norm, flag)
        idx, best = ref.argmin(cost)
        u_best = ref.unnormalize_states(u_norm[idx][None], flag)[0].cpu().numpy()
        want_c, want_i = _ref_topk(cost, 1, k)
        priors = _shift(u_norm)[want_i[0].cuda()[torch.arange(B, device="cuda") % k]].clone()
        # the one call
        r = plan.mpc_step(x0, sysm, B, w=0.01, noise=noise, n_wo_noise=nwo, warm_start=K, elites=k)
        torch.cuda.synchronize()
        assert (r.best_index, r.best_cost) == (idx, best), f"step {s}"
        np.testing.assert_array_equal(r.u_best, u_best)
        assert _same(r.u_norm, u_norm) and torch.equal(r.costs, cost), f"step {s}"
        assert int(r.elite_index[0]) == r.best_index and r.elite_index.dtype == np.int64
        assert (np.diff(r.elite_cost) >= 0).all(), "elite costs must not decrease"
        np.testing.assert_array_equal(r.elite_index, want_i[0].numpy())
        np.testing.assert_array_equal(r.elite_cost, want_c[0].numpy())
        assert _same(plan._prior, priors), f"step {s}: the next priors are not the shifted elites"
        assert _same(plan.warm_prior(), priors[0])
        if s > 0:
            with pytest.raises(ValueError):  # a cold step's slice count is refused once the priors exist
                plan.mpc_step(x0, sysm, B, noise=torch.zeros(N + nwo + 1, B, H, d), n_wo_noise=nwo, warm_start=K, elites=k)


# ---------------------------------------------------------------------------------------- 5. closed loop
def _loop_plan():
    return _step_plan("f32x3")


def _composed_loop(plan, x0, sysm, T, n, k, grouped, seed):
    """closed_loop's composition from the library's public calls, the elite priors built in torch"""
    M, nx = x0.shape
    H, d, B, dev, L, st = plan.spec.horizon, plan.spec.state_dim, M * n, plan.device, plan._lib, plan._stream()
    desc = sysm.desc()
    x = torch.from_numpy(x0.copy()).to(dev)
    xs, us, cs, ix = [x0.copy()], [], [], []
    ctx = torch.empty((M, nx), dtype=torch.float32, device=dev)
    flags = torch.empty(M, dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    absmax = torch.empty(B, dtype=torch.float32, device=dev)
    u_it = torch.empty((M, d), dtype=torch.float64, device=dev)
    c_it = torch.empty(M, dtype=torch.float64, device=dev)
    i_it = torch.empty(M, dtype=torch.int64, device=dev)
    grouped = grouped and plan.grouped_pays(M, n)
    priors = None
    for it in range(T):
        nat.check(L.mpcd_normalize_states(plan._ctx, _ptr(x), M, nx, plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data,
                                          _ptr(ctx), st), "mpcd_normalize_states")
        u_norm = plan.sample_trajectories(ctx if grouped else ctx.repeat_interleave(n, 0), B, H, w=0.01, seed=seed + it,
                                          absmax_out=absmax, context_group=n if grouped else None, x_init=priors,
                                          t_start=None if priors is None else K)
        nat.check(L.mpcd_clip_flags(plan._ctx, _ptr(absmax), M, n, _ptr(flags), st), "mpcd_clip_flags")
        nat.check(L.mpcd_rollout_cost_grouped(plan._ctx, ctypes.byref(desc), _ptr(x), n, _ptr(u_norm),
                                              plan.act_min.ctypes.data, plan.act_max.ctypes.data, B, H, _ptr(flags),
                                              _ptr(cost), st), "mpcd_rollout_cost_grouped")
        nat.check(L.mpcd_control_step(plan._ctx, ctypes.byref(desc), _ptr(x), M, n, _ptr(u_norm), H, _ptr(cost),
                                      plan.act_min.ctypes.data, plan.act_max.ctypes.data, _ptr(flags), 0, 4, _ptr(u_it),
                                      _ptr(i_it), _ptr(c_it), st), "mpcd_control_step")
        _, el = _ref_topk(cost, M, k)
        b = torch.arange(B)
        priors = _shift(u_norm)[el[b // n, b % n % k].cuda()].clone()
        xs.append(x.cpu().numpy())
        us.append(u_it.cpu().numpy())
        cs.append(c_it.cpu().numpy())
        ix.append(i_it.cpu().numpy())
    return np.stack(xs, 1), np.stack(us, 1), np.stack(cs, 1), np.stack(ix, 1)


@pytest.mark.parametrize("grouped", (True, False))
@pytest.mark.parametrize("M,n", ((3, 5), (2, 16)))
def test_closed_loop_elites(M, n, grouped):
    T, sysm, plan = 3, systems.double_int2d(), _loop_plan()
    x0 = np.random.default_rng(3).uniform(-1.5, 1.5, (M, 4))
    kw = dict(n_samples=n, w=0.01, seed=7, grouped=grouped, warm_start=K)
    warm = plan.closed_loop(x0, sysm, T, **kw)
    one = plan.closed_loop(x0, sysm, T, elites=1, **kw)
    for f in ("x", "u", "cost", "index"):
        np.testing.assert_array_equal(getattr(one, f), getattr(warm, f), err_msg=f"elites=1: {f}")
    got = plan.closed_loop(x0, sysm, T, elites=3, **kw)
    want = _composed_loop(plan, x0, sysm, T, n, 3, grouped, seed=7)
    for f, w in zip(("x", "u", "cost", "index"), want):
        np.testing.assert_array_equal(getattr(got, f), w, err_msg=f"elites=3: {f}")
    assert got.x.shape == (M, T + 1, 4) and got.index.shape == (M, T)


# ------------------------------------------------------------------------------------------ 6. refusals
def _step_args(plan, B, x0, sysm, u_norm, cost, sampler="ddpm_cfg"):
    desc = sysm.desc()
    a = nat.StepArgs()
    a.sys = ctypes.pointer(desc)
    a.x0 = x0.ctypes.data
    a.ctx_min, a.ctx_max = plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data
    a.act_min, a.act_max = plan.act_min.ctypes.data, plan.act_max.ctypes.data
    a.sample = plan._args(plan._sampler_id(sampler), B, _STEP_CONTEXT, 0.01, 0, 5 if sampler != "ddpm_cfg" else None, False,
                          1, 0, None, u_norm, None)
    a.clip_rule = nat.MPCD_CLIP_CHAIN
    a.cost_local = a.costs_all = cost.data_ptr()
    return a, desc


def test_c_refusals():
    plan, L = _step_plan("f32x3"), nat.lib()
    B, H, d, sysm = 12, 16, 2, systems.double_int2d()
    cost = torch.zeros(B, dtype=torch.float64, device="cuda")
    u = torch.zeros(B, H, d, device="cuda")
    out = torch.zeros(B, H, d, device="cuda")
    raw = torch.zeros((B, 2), dtype=torch.int64, device="cuda")
    err = lambda: L.mpcd_last_error().decode(errors="replace")  # noqa: E731
    # mpcd_topk
    for what, args in (("null cost", (None, 1, B, 1, 0, _ptr(raw))), ("null out", (_ptr(cost), 1, B, 1, 0, None)),
                       ("k 0", (_ptr(cost), 1, B, 0, 0, _ptr(raw))), ("k > group", (_ptr(cost), 2, 6, 7, 0, _ptr(raw))),
                       ("k > 64", (_ptr(cost), 1, B, 65, 0, _ptr(raw))), ("group 0", (_ptr(cost), 1, 0, 1, 0, _ptr(raw))),
                       ("n_groups 0", (_ptr(cost), 0, B, 1, 0, _ptr(raw)))):
        assert L.mpcd_topk(plan._ctx, *args, None) == EINVAL and err(), what
    big = torch.zeros(100, dtype=torch.float64, device="cuda")
    raw65 = torch.zeros((65, 2), dtype=torch.int64, device="cuda")
    assert L.mpcd_topk(plan._ctx, _ptr(big), 1, 100, 65, 0, _ptr(raw65), None) == EINVAL and "k 65" in err()
    # mpcd_elite_priors
    ok = (_ptr(u), 1, B, H, _ptr(raw), 3, 0, 1, _ptr(out))

    def with_(i, v):
        return ok[:i] + (v,) + ok[i + 1:]

    assert L.mpcd_elite_priors(plan._ctx, *ok, None) == 0, err()
    for what, args in (("null u_norm", with_(0, None)), ("null elites", with_(4, None)), ("null out", with_(8, None)),
                       ("k 0", with_(5, 0)), ("k > group", with_(5, B + 1)), ("k > 64", with_(5, 65)),
                       ("shift 2", with_(7, 2)), ("shift -1", with_(7, -1)), ("horizon", with_(3, H + 1)),
                       ("group 0", with_(2, 0)), ("out is u_norm", with_(8, _ptr(u))), ("out overlaps u_norm", with_(8, _ptr(u[1:])))):
        assert L.mpcd_elite_priors(plan._ctx, *args, None) == EINVAL and err(), what
    assert L.mpcd_elite_priors(plan._ctx, *with_(7, 2), None) == EINVAL and "shift" in err()
    torch.cuda.synchronize()
    # mpcd_mpc_step_elite
    x0 = np.ascontiguousarray(STEP_X0[0])
    a, desc = _step_args(plan, B, x0, sysm, u, cost)
    best, ub = nat.Best(), np.empty((H, d), dtype=np.float32)
    prior = torch.zeros(B, H, d, device="cuda")

    def warm(t_start, rows, ptr=prior):
        w = nat.WarmStart()
        w.t_start, w.rows, w.x_init = t_start, rows, ptr.data_ptr() if ptr is not None else None
        return w

    def step(pl, a, w, k, nxt=out, best=best, ub=ub):
        rc = L.mpcd_mpc_step_elite(pl._ctx, ctypes.byref(a) if a is not None else None,
                                   ctypes.byref(w) if w is not None else None, k, _ptr(nxt) if nxt is not None else None,
                                   None, ctypes.byref(best) if best is not None else None,
                                   ub.ctypes.data if ub is not None else None, pl._stream())
        torch.cuda.synchronize()
        return rc

    assert step(plan, a, warm(0, 0), 3) == 0, err()  # a cold step that fills the priors
    assert step(plan, a, warm(K, B), 3) == 0, err()
    assert step(plan, a, warm(K, 1), 3, nxt=None) == 0, err()
    for what, args in (("null args", (None, warm(K, 1), 3)), ("null warm", (a, None, 3)), ("k 0", (a, warm(K, 1), 0)),
                       ("k > batch", (a, warm(K, 1), B + 1)), ("k > 64", (a, warm(K, 1), 65)),
                       ("rows 5", (a, warm(K, 5), 3)), ("rows 0", (a, warm(K, 0), 3)),
                       ("t_start > n_steps", (a, warm(N + 1, 1), 3)), ("null x_init", (a, warm(K, 1, None), 3))):
        assert step(plan, *args) == EINVAL and err(), what
    assert step(plan, a, warm(K, 5), 3) == EINVAL and "rows" in err()
    assert step(plan, a, warm(K, 1), 3, best=None) == EINVAL
    assert step(plan, a, warm(K, 1), 3, ub=None) == EINVAL
    assert step(plan, a, warm(K, B), 3, nxt=prior) == EINVAL and "alias" in err()
    assert step(plan, a, warm(K, 1), 3, nxt=prior) == EINVAL and "alias" in err()
    assert step(plan, a, warm(0, B), 3, nxt=prior) == 0, err()  # a cold step does not read the priors
    assert step(plan, a, warm(K, 1), 3, nxt=u) == EINVAL and "x_out" in err()
    bad, _ = _step_args(plan, B, x0, sysm, u, cost)
    bad.clip_rule = 7
    assert step(plan, bad, warm(K, 1), 3) == EINVAL  # the existing step checks
    ddim, _ = _step_args(plan, B, x0, sysm, u, cost, sampler="ddim_cfg")
    assert step(plan, ddim, warm(K, 1), 3) == EUNSUP and "DDPM" in err()
    # a context with a communicator
    ranked = _step_plan("f32x3")
    D.NativeComm(ranked, loopback=(1, 0, _key()))
    ar, _ = _step_args(ranked, B, x0, sysm, u, cost)
    assert step(ranked, ar, warm(K, 1), 3) == EUNSUP and "rank" in err()


def test_python_refusals():
    plan, sysm, x0 = _step_plan("f32x3"), systems.double_int2d(), np.zeros(4)
    B = 12
    for kw in (dict(elites=3), dict(warm_start=K, elites=3, native=False), dict(warm_start=K, elites=0),
               dict(warm_start=K, elites=B + 1), dict(warm_start=K, elites=65)):
        with pytest.raises(ValueError):
            plan.mpc_step(x0, sysm, 100 if kw.get("elites") == 65 else B, **kw)
    ranked = _step_plan("f32x3")
    comm = D.NativeComm(ranked, loopback=(1, 0, _key()))
    with pytest.raises(ValueError):
        ranked.mpc_step(x0, sysm, B, warm_start=K, elites=3, comm=comm)
    # stored priors of another batch size
    plan.mpc_step(x0, sysm, B, warm_start=K, elites=3)
    with pytest.raises(ValueError, match="reset_warm_start"):
        plan.mpc_step(x0, sysm, B + 4, warm_start=K, elites=3)
    plan.reset_warm_start()
    r = plan.mpc_step(x0, sysm, B + 4, warm_start=K, elites=3)
    assert r.elite_index.shape == (3,) and plan._prior.shape[0] == B + 4
    # a single stored prior (from a step without elites) seeds every candidate
    plan.reset_warm_start()
    plan.mpc_step(x0, sysm, B, warm_start=K)
    assert plan.mpc_step(x0, sysm, B, warm_start=K, elites=3).elite_index.shape == (3,)
    # closed loop
    xs = np.zeros((2, 4))
    for kw in (dict(elites=2), dict(warm_start=K, elites=2, native=True), dict(warm_start=K, elites=4),
               dict(warm_start=K, elites=0), dict(warm_start=K, elites=2, select="first")):
        with pytest.raises(ValueError):
            plan.closed_loop(xs, sysm, 2, n_samples=3, **kw)
    # topk / elite_priors
    cost = torch.zeros(12, dtype=torch.float64, device="cuda")
    for args in ((cost, 0), (cost, 13), (cost.float(), 2), (cost.cpu(), 2)):
        with pytest.raises(ValueError):
            plan.topk(*args)
    with pytest.raises(ValueError):
        plan.topk(cost, 2, n_groups=5)
    u = torch.zeros(12, 16, 2, device="cuda")
    idx = torch.zeros((3, 2), dtype=torch.int64, device="cuda")
    assert plan.elite_priors(u, idx, 4).shape == (12, 16, 2)
    for args in ((u, idx, 5), (u, idx.int(), 4), (u, idx.cpu(), 4), (u, torch.zeros((3, 5), dtype=torch.int64, device="cuda"), 4)):
        with pytest.raises(ValueError):
            plan.elite_priors(*args)
    with pytest.raises(ValueError):
        plan.elite_priors(u, idx, 4, out=torch.zeros(11, 16, 2, device="cuda"))
