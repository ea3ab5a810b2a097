"""GPU: mpc_step_batch_box - one mpcd_mpc_step_batch_box call per control step: the batched external step whose fused
tail (batch_step_box_tail_kernel) also reports every candidate's violation of a state box and selects and ranks in the
feasibility-first order.

The reference is tests/test_gpu_state_box.py's and never the code under test: an fp64 rollout through
oracle.systems.step gives the visited states, numpy their box violation and numpy.lexsort on (index, cost, g) the order.
The costs it ranks come from the unchanged mpcd_rollout_cost_grouped on the step's returned samples
(test_gpu_mpc_step_batch_elites.py's _cost_ref). double_int2d has no sin / cos: its states, hence V, are exact, and
ranking and copying do not round, so every comparison is on bit patterns."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
from mpc_via_diffusion_model_amd import _native as N

from ._systems_ref import TAIL_DESCRIPTORS
from ._util import make_mlp
from .test_gpu_mpc_step_batch_elites import (D, H, K, NSTEPS, T, _c_args, _cost_ref, _di, _e_args, _new_plan, _noises,
                                              _plan, _ptr, _x0)
from .test_gpu_state_box import BOX_COMPONENTS, _box, _rank, _violation, _visited

pytestmark = pytest.mark.gpu

CLIPPED, NAN_SAMPLES, NONFINITE, INFEASIBLE = (N.MPCD_STEP_CLIPPED, N.MPCD_STEP_NAN_SAMPLES, N.MPCD_STEP_NONFINITE_WINNER,
                                               N.MPCD_STEP_INFEASIBLE)
# test_gpu_mpc_step_batch_elites.py's reasons: a partial wave; single lanes; every candidate of a full wave an elite; a
# partial list shorter than k; three workgroups with MPCD_MAX_ELITES; 65 workgroups (a lane owns two lists)
SHAPES = [(5, 16, 3), (4, 1, 1), (2, 64, 64), (3, 80, 20), (1, 130, 64), (1, 4160, 8)]
VEL = (2, 3)  # the bounded components: the velocities, which the cheapest plans (fastest towards the origin) push up
FIELDS = ("u", "plan", "cost", "index", "flags", "violation", "n_feasible")
ELITE_FIELDS = ("elite_index", "elite_cost", "elite_violation")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _eq(a, b, msg=""):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{msg}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _assert_states_equal(a, b, states, fields):
    for f in fields:
        for m in states:
            _eq(np.asarray(getattr(a, f)[m]), np.asarray(getattr(b, f)[m]), f"{f}[{m}]")


def _unnormalize(u_norm, clipped, mn, mx):
    """fp32 LimitsNormalizer.unnormalize of one state's candidates under that state's clip decision"""
    x = np.asarray(u_norm, dtype=np.float32)
    if clipped:
        x = np.clip(x, np.float32(-1), np.float32(1))
    h = (x + np.float32(1)) / np.float32(2)
    return h * (mx - mn) + mn


def _reference(plan, sysm, x, n, r0, cost_dev):
    """What the host reference needs of one step, from the UNCONSTRAINED step r0 (return_samples=True) on the states x:
    each state's clip decision (r0's flags), the unnormalised plans, the visited states xs [M, n, ., n_x] through
    oracle.systems.step and the costs [M, n] of mpcd_rollout_cost_grouped. Computed once per case and left unchanged."""
    M = len(x)
    un = r0.u_norm.cpu().numpy().reshape(M, n, *r0.u_norm.shape[1:])
    clipped = (r0.flags & CLIPPED) != 0
    u = np.stack([_unnormalize(un[m], clipped[m], plan.act_min, plan.act_max) for m in range(M)])
    xs = np.stack([_visited(sysm.name, x[m], u[m].astype(np.float64)) for m in range(M)])
    ref = types.SimpleNamespace(M=M, n=n, x=np.ascontiguousarray(x, dtype=np.float64), r0=r0, u=u, xs=xs,
                                cost=cost_dev.cpu().numpy().reshape(M, n), sysm=sysm,
                                codes=np.where(r0.flags & NAN_SAMPLES, 2, np.where(clipped, 1, 0)).astype(np.int32))
    for a in (ref.u, ref.xs, ref.cost, ref.codes):
        a.setflags(write=False)
    return ref


def _reach(ref, m, comps=VEL):
    """[n, len(comps)]: the largest magnitude each candidate of state m reaches on each bounded component"""
    return np.abs(ref.xs[m][:, :, list(comps)]).max(axis=1)


def _median_bounds(reach):
    """per component the median over the candidates: the midpoint of the two middle distinct values, so that no state
    lies on a bound and about half the candidates stay inside"""
    out = []
    for c in range(reach.shape[1]):
        v = np.unique(reach[:, c])
        out.append(float(v[0]) if len(v) == 1 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))
    return out


def _sym_box(n_x, comps, bounds):
    return _box(n_x, {i: (-b, b) for i, b in zip(comps, bounds)})


def _viol_ref(ref, lo, hi):
    return np.stack([_violation(ref.xs[m], lo, hi) for m in range(ref.M)])


def _check(plan, ref, r, box_arrays, tol, k, elites, what=""):
    """the constrained step r against the host reference: selection, violation, count, flags, action, plan, ranked
    lists and the kept priors"""
    lo, hi = box_arrays
    M, n, sysm = ref.M, ref.n, ref.sysm
    V = _viol_ref(ref, lo, hi)
    wi, wc, wv, wn = _rank(ref.cost, V, M, k, tol)
    assert torch.equal(r.u_norm.view(torch.int32), ref.r0.u_norm.view(torch.int32)), "the samples differ"
    _eq(r.index, wi[:, 0], f"{what} index")
    _eq(r.cost, ref.cost.reshape(-1)[wi[:, 0]], f"{what} cost as computed")
    _eq(r.violation, wv[:, 0], f"{what} violation")
    _eq(r.n_feasible, wn, f"{what} n_feasible")
    _eq(r.flags, (ref.r0.flags & (CLIPPED | NAN_SAMPLES)) | np.where(np.isfinite(r.cost), 0, NONFINITE).astype(np.int32)
        | np.where(wn == 0, INFEASIBLE, 0).astype(np.int32), f"{what} flags")
    pick = ref.u.reshape(M * n, *ref.u.shape[2:])[wi[:, 0]]
    _eq(r.plan, pick, f"{what} plan")
    dev = plan.device
    xd = torch.from_numpy(ref.x.copy()).to(dev)
    u_dev, i_dev, _ = plan.control_step_picked(sysm, xd, r.u_norm, torch.from_numpy(wi[:, 0].copy()).to(dev),
                                               torch.from_numpy(wc[:, 0].copy()).to(dev),
                                               torch.from_numpy(ref.codes.copy()).to(dev))
    _eq(r.u, u_dev.cpu().numpy(), f"{what} u")
    pri = plan.batch_priors()
    Hs, d = plan.spec.horizon, plan.spec.state_dim
    if elites:
        _eq(r.elite_index, wi, f"{what} elite_index")
        _eq(r.elite_cost, wc, f"{what} elite_cost")
        _eq(r.elite_violation, wv, f"{what} elite_violation")
        if pri is not None:
            assert tuple(pri.shape) == (M, n, Hs, d)
            want = plan.elite_priors(r.u_norm, torch.from_numpy(wi.copy()).to(dev), n)
            assert torch.equal(pri.view(M * n, Hs, d).view(torch.int32), want.view(torch.int32)), f"{what} priors"
    else:
        assert r.elite_index is None and r.elite_cost is None and r.elite_violation is None
        if pri is not None:
            assert tuple(pri.shape) == (M, Hs, d)
            want = plan.shift_plans(r.u_norm, torch.from_numpy(wi[:, 0].copy()).to(dev))
            assert torch.equal(pri.view(torch.int32), want.view(torch.int32)), f"{what} priors"
    return V, (wi, wc, wv, wn)


@functools.lru_cache(maxsize=None)
def _case(M, n, seed=17, x_key=None):
    """the unconstrained cold step with injected noise on M states x n candidates and its reference"""
    plan, di = _plan(), _di()
    x = _x0(M) if x_key is None else np.array(x_key, dtype=np.float64)
    z = _noises(M, n, [NSTEPS + 1], seed=seed)[0]
    plan.reset_warm_start()
    r0 = plan.mpc_step_batch(x, di, n, noise=z, return_samples=True)
    return z, _reference(plan, di, x, n, r0, _cost_ref(plan, di, x, n, r0, noise=z))


def _box_step(plan, ref, z, box, tol=0.0, elites=None, **kw):
    plan.reset_warm_start()
    return plan.mpc_step_batch_box(ref.x, ref.sysm, ref.n, box, tol, noise=z, warm_start=K, elites=elites,
                                   return_samples=True, **kw)


# ---- 1. against the host reference, shapes

@pytest.mark.parametrize("elites", [True, False], ids=["elites", "winner_only"])
@pytest.mark.parametrize("M,n,k", SHAPES)
def test_against_the_host_reference(M, n, k, elites):
    """One constrained call per state's own box (its candidates' median excursions on the two velocities: about half of
    THAT state's candidates stay inside, by construction), every call compared for all M states: under another state's
    box a state may be all inside or all outside, which are cases too."""
    z, ref = _case(M, n)
    plan = _plan()
    k = k if elites else 1
    both = moved = 0
    for s in range(M):
        reach = _reach(ref, s)
        bounds = _median_bounds(reach)
        if (M, n) == (3, 80) and s == 0:  # the state whose last candidate must be feasible: 48 lanes past the group
            bounds = [max(b, float(e)) for b, e in zip(bounds, reach[-1])]
        box, lo, hi = _sym_box(4, VEL, bounds)
        V = _viol_ref(ref, lo, hi)
        if (M, n) == (3, 80) and s == 0:
            assert V[0, -1] == 0.0, "the last candidate of the two-workgroup state must be feasible"
        both += int(((V[s] == 0).any() and (V[s] > 0).any()))
        moved += int((_rank(ref.cost, V, M, 1, 0.0)[0][:, 0] != ref.r0.index).sum())
        assert n == 1 or ((V[s] == 0).any() and (V[s] > 0).any()), "a median of distinct excursions splits the state"
        r = _box_step(plan, ref, z, box, elites=k if elites else None)
        _check(plan, ref, r, (lo, hi), 0.0, k, elites, f"box of state {s}")
    print(f"\n({M}, {n}, {k}): calls with both classes in their state {both} of {M}; winners moved by the box {moved}")
    if n > 1:  # one candidate per state is one class and one winner whatever the box
        assert both >= 1, "no state holds both classes"
        assert moved >= 1, "the constrained winner is the unconstrained one in every state"


# ---- 2. no admissible plan

@pytest.mark.parametrize("elites", [8, None])
def test_no_admissible_plan(elites):
    """state 1 starts at v_x = 2: one step of |a_x| <= 1 leaves every candidate above 1.8, the others start slowly. A
    v_x bound between the two has no admissible plan in state 1 alone; tol at the median violation of state 1 turns
    about half its candidates feasible."""
    x = ((.2, -.1, .3, -.2), (.2, -.1, 2.0, 0.), (-.4, .3, -.2, .1))
    M, n, s = 3, 80, 1
    z, ref = _case(M, n, 19, x)
    plan = _plan()
    least = np.array([_reach(ref, m, (2,)).min() for m in range(M)])
    assert least[s] > 1.8 and np.delete(least, s).max() < 1.5, "the states were not reproduced"
    bound = 0.5 * (np.delete(least, s).max() + least[s])
    box, lo, hi = _sym_box(4, (2,), [bound])
    V = _viol_ref(ref, lo, hi)
    assert (V[s] > 0).all() and all((V[m] == 0).any() for m in (0, 2))
    vs = np.unique(V[s])
    for tol in (0.0, float(0.5 * (vs[len(vs) // 2 - 1] + vs[len(vs) // 2]))):
        r = _box_step(plan, ref, z, box, tol, elites=elites)
        _, (wi, wc, wv, wn) = _check(plan, ref, r, (lo, hi), tol, elites or 1, elites is not None, f"tol {tol}")
        if tol == 0.0:
            assert r.n_feasible[s] == 0 and (r.flags & INFEASIBLE).tolist() == [0, INFEASIBLE, 0]
            order = np.lexsort((np.arange(n), np.where(np.isnan(ref.cost[s]), np.inf, ref.cost[s]), V[s]))
            assert r.index[s] == s * n + order[0] and r.violation[s] == V[s].min() > 0
        else:
            assert 0 < r.n_feasible[s] < n and not (r.flags & INFEASIBLE).any()
            assert r.violation[s] <= tol and r.violation[s] > 0  # feasible within the tolerance, V as computed


# ---- 3. ties across workgroups

def test_ties_across_workgroups_go_to_the_lower_index():
    M, n, k = 2, 130, 64
    g = torch.Generator().manual_seed(5)
    z7 = torch.randn(NSTEPS + 1, M, 7, H, D, generator=g)
    z = z7[:, :, torch.arange(n) % 7].reshape(NSTEPS + 1, M * n, H, D).contiguous()  # candidate j copies j mod 7
    plan, di, x = _new_plan(), _di(), _x0(M)
    r0 = plan.mpc_step_batch(x, di, n, noise=z, return_samples=True)
    ref = _reference(plan, di, x, n, r0, _cost_ref(plan, di, x, n, r0, noise=z))
    # one bounded component: of state 0's 7 distinct plans the 3 with the smallest excursion are feasible
    box, lo, hi = _sym_box(4, (2,), _median_bounds(_reach(ref, 0, (2,))))
    V = _viol_ref(ref, lo, hi)
    for m in range(M):
        assert len(np.unique(ref.cost[m])) <= 7 and len(np.unique(V[m])) <= 7  # the input does contain duplicates
    assert (V[0] == 0).any() and (V[0] > 0).any() and (V[0] == 0).sum() < k  # the list spans both classes
    r = _box_step(plan, ref, z, box, elites=k)
    _check(plan, ref, r, (lo, hi), 0.0, k, True)
    assert (np.diff(r.elite_index[:, :3], axis=1) == 7).all()  # the best plan's copies: j, j + 7, j + 14
    nf = int(r.n_feasible[0])
    assert (np.diff(r.elite_index[0, nf:nf + 3]) == 7).all()  # and the least violating plan's


# ---- 4. NaN

def _nan_setup(M, n):
    z, ref = _case(M, n, 17)
    box, lo, hi = _sym_box(4, VEL, _median_bounds(np.concatenate([_reach(ref, m) for m in range(M)])))
    return z, ref, box, (lo, hi)


def test_nan_candidate_is_last_and_reported_as_inf():
    M, n, k, state, cand = 3, 40, 40, 1, 30
    clean, ref, box, arrays = _nan_setup(M, n)
    dirty = clean.clone()
    dirty[0, state * n + cand, 3, 1] = float("nan")  # this candidate's chain, samples, cost (NaN) and states (V = +inf)
    plan = _plan()
    want = _box_step(plan, ref, clean, box, elites=k)
    _check(plan, ref, want, arrays, 0.0, k, True)
    plan.reset_warm_start()
    got = plan.mpc_step_batch_box(ref.x, _di(), n, box, noise=dirty, warm_start=K, elites=k)
    assert got.elite_index[state, -1] == state * n + cand
    assert np.isposinf(got.elite_cost[state, -1]) and np.isposinf(got.elite_violation[state, -1])
    assert np.isfinite(got.elite_cost[state, :-1]).all() and np.isfinite(got.elite_violation[state, :-1]).all()
    assert got.flags[state] & NAN_SAMPLES and not got.flags[state] & NONFINITE
    _assert_states_equal(got, want, (0, 2), FIELDS + ELITE_FIELDS)


def test_all_nan_state_is_reported_and_the_others_stand():
    M, n, k, state = 3, 40, 8, 1
    clean, ref, box, arrays = _nan_setup(M, n)
    dirty = clean.clone()
    dirty[0, state * n:(state + 1) * n, 3, 1] = float("nan")
    plan = _new_plan()
    want = _box_step(plan, ref, clean, box, elites=k)
    assert plan.batch_priors() is not None
    plan.reset_warm_start()
    with pytest.raises(N.MpcdError) as err:
        plan.mpc_step_batch_box(ref.x, _di(), n, box, noise=dirty, warm_start=K, elites=k)
    assert err.value.status == N.MPCD_ENONFINITE
    assert plan.batch_priors() is None  # the kept priors are dropped
    got = plan.mpc_step_batch_box(ref.x, _di(), n, box, noise=dirty, warm_start=K, elites=k, allow_nonfinite=True)
    assert got.flags[state] & NONFINITE and got.flags[state] & INFEASIBLE and got.flags[state] & NAN_SAMPLES
    assert got.n_feasible[state] == 0 and np.isposinf(got.violation[state]) and np.isnan(got.cost[state])
    assert not (got.flags[[0, 2]] & (NONFINITE | NAN_SAMPLES)).any()
    np.testing.assert_array_equal(got.elite_index[state], state * n + np.arange(k))
    assert np.isposinf(got.elite_cost[state]).all() and np.isposinf(got.elite_violation[state]).all()
    _assert_states_equal(got, want, (0, 2), FIELDS + ELITE_FIELDS)
    again = _box_step(plan, ref, clean, box, elites=k)  # the counters were left reset
    _assert_states_equal(again, want, range(M), FIELDS + ELITE_FIELDS)


# ---- 5. an all-infinite box is today's step

@pytest.mark.parametrize("M,n,k", [(3, 80, 8), (1, 4160, 8), (5, 16, 3)])
def test_infinite_box_equals_the_unconstrained_step(M, n, k):
    a, b = _new_plan(), _new_plan()
    di = _di()
    noises = _noises(M, n, [NSTEPS + 1, K + 1, K + 1], seed=29)
    inf_box = ([-np.inf] * 4, [np.inf] * 4)
    common = ("u", "plan", "cost", "index", "flags")
    for elites in (None, k):
        a.reset_warm_start()
        b.reset_warm_start()
        cold_a = a.mpc_step_batch(_x0(M), di, n, noise=noises[0])  # cold, no warm start kept
        cold_b = b.mpc_step_batch_box(_x0(M), di, n, inf_box, noise=noises[0])
        _assert_states_equal(cold_a, cold_b, range(M), common)
        assert cold_a.violation is None and cold_a.n_feasible is None and cold_a.elite_violation is None
        for it in range(3):  # cold, then warm twice
            x = _x0(M) * (1 - 0.2 * it)
            ra = a.mpc_step_batch(x, di, n, noise=noises[it], warm_start=K, elites=elites)
            rb = b.mpc_step_batch_box(x, di, n, inf_box, 0.0, noise=noises[it], warm_start=K, elites=elites)
            _assert_states_equal(ra, rb, range(M), common + (("elite_index", "elite_cost") if elites else ()))
            assert (rb.violation == 0).all() and (rb.n_feasible == n).all() and not (rb.flags & INFEASIBLE).any()
            assert elites is None or (rb.elite_violation == 0).all()
            assert torch.equal(a.batch_priors().view(torch.int32), b.batch_priors().view(torch.int32))


# ---- 6. equals the composed closed loop

@pytest.mark.parametrize("clip_rule", ["chain", "final"])
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("warm,elites", [(None, None), (K, None), (K, 4)], ids=["cold", "warm", "warm_elites"])
def test_equals_the_composed_closed_loop(warm, elites, grouped, clip_rule):
    M, n = 3, 20
    plan = _plan("f32x3" if grouped else "f32")
    assert not grouped or plan.grouped_pays(M, n)
    di, x0 = _di(), _x0(M)
    noises = _noises(M, n, [NSTEPS + 1] + [(K if warm else NSTEPS) + 1] * (T - 1), seed=23)
    box, tol = _box(4, {2: (-1.0, 1.0), 3: (-1.2, 1.2)})[0], 0.05
    kw = dict(warm_start=warm, elites=elites, grouped=grouped, clip_rule=clip_rule)
    ref = plan.closed_loop(x0, di, T, n_samples=n, noise=lambda it: noises[it], native=False, state_box=box, viol_tol=tol,
                           **kw)
    plan.reset_warm_start()
    for it in range(T):
        r = plan.mpc_step_batch_box(ref.x[:, it], di, n, box, tol, seed=it, noise=noises[it], **kw)
        for f in ("u", "cost", "index", "violation", "n_feasible"):
            _eq(getattr(r, f), np.ascontiguousarray(getattr(ref, f)[:, it]), f"{f}[{it}]")
        assert ((r.flags & INFEASIBLE) != 0).tolist() == (ref.n_feasible[:, it] == 0).tolist()
    assert np.isfinite(ref.cost).all()


# ---- 7. every system and cost kind

@pytest.mark.parametrize("name", sorted(systems.REGISTRY))
def test_every_system_and_cost_kind(name):
    """the tail's six instantiations against the composed device path on the returned samples: rollout_cost_box +
    topk_feasible + control_step_picked, pinned to the host reference by their own tests (calMPCCost's visited-state set
    with them). The bounds are the medians of the excursions that path itself reports (V under a box of width 0)."""
    _system_case(systems.get(name))


@pytest.mark.parametrize("which", sorted(TAIL_DESCRIPTORS))
def test_non_default_descriptor(which):
    """the same harness at a descriptor that is not the registry's (tests/_systems_ref.py: every constant distinct and
    non-zero, a set-point that is non-zero everywhere; the nonlinear cart-pole under calMPCCost, whose visited states
    are x_1 .. x_{H-2})"""
    _system_case(TAIL_DESCRIPTORS[which]())


def _system_case(sysm):
    name = sysm.name
    d, Cx, Hs, M, n, k = sysm.n_u, sysm.n_x, 32 // min(sysm.n_u, 2), 3, 35, 4
    net = make_mlp(d, Hs, Cx, seed=9)
    plan = DiffusionMPC(NetSpec("mlp", d, Hs, Cx), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NSTEPS, context_limits=(-2 * np.ones(Cx), 2 * np.ones(Cx)))
    x = np.random.default_rng(4).uniform(-0.3, 0.3, (M, Cx))
    kw = dict(seed=2, clip_rule="final", warm_start=K)
    r0 = plan.mpc_step_batch(x, sysm, n, return_samples=True, **kw)
    dev, st = plan.device, plan._stream()
    flags = torch.empty(M, dtype=torch.int32, device=dev)
    N.check(plan._lib.mpcd_clip_flags(plan._ctx, _ptr(r0.u_norm), M, n * Hs * d, _ptr(flags), st), "mpcd_clip_flags")
    comps = BOX_COMPONENTS[name]
    bounds = []
    for i in comps:
        reach = plan.rollout_cost_box(sysm, x, r0.u_norm, _box(Cx, {i: (0.0, 0.0)})[0], group=n, clip_flags=flags)[1]
        v = np.unique(reach.cpu().numpy())
        bounds.append(0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))
    box = _sym_box(Cx, comps, bounds)[0]
    cost, viol = plan.rollout_cost_box(sysm, x, r0.u_norm, box, group=n, clip_flags=flags)
    assert (viol == 0).any() and (viol > 0).any() and torch.isfinite(cost).all()
    for elites in (k, None):
        kk = elites or 1
        wi, wc, wv, wn = (t.cpu().numpy() for t in plan.topk_feasible(cost, viol, kk, n_groups=M))
        plan.reset_warm_start()
        r = plan.mpc_step_batch_box(x, sysm, n, box, elites=elites, return_samples=True, **kw)
        assert torch.equal(r.u_norm.view(torch.int32), r0.u_norm.view(torch.int32))
        _eq(r.index, np.ascontiguousarray(wi[:, 0]), "index")
        _eq(r.cost, np.ascontiguousarray(wc[:, 0]), "cost")
        _eq(r.violation, np.ascontiguousarray(wv[:, 0]), "violation")
        _eq(r.n_feasible, wn, "n_feasible")
        xd = torch.from_numpy(x.copy()).to(dev)
        pick = plan.topk_feasible(cost, viol, 1, n_groups=M)
        u_dev, _, _ = plan.control_step_picked(sysm, xd, r0.u_norm, pick[0][:, 0].contiguous(), pick[1][:, 0].contiguous(),
                                               flags)
        _eq(r.u, u_dev.cpu().numpy(), "u")
        if elites:
            _eq(r.elite_index, wi, "elite_index")
            _eq(r.elite_cost, wc, "elite_cost")
            _eq(r.elite_violation, wv, "elite_violation")


# ---- 8. the reset mask; workspace reuse

@pytest.mark.parametrize("k", [3, None], ids=["elites", "winner_only"])
def test_reset_mask_with_a_box(k):
    M, n = 5, 16
    plan = _new_plan()
    di = _di()
    box, tol = _box(4, {2: (-0.5, 0.5), 3: (-0.6, 0.6)})[0], 0.0
    mask = np.array([False, True, False, False, True])
    ic, iw = np.flatnonzero(mask), np.flatnonzero(~mask)
    z0 = _noises(M, n, [NSTEPS + 1], seed=1)[0]
    zc = _noises(len(ic), n, [NSTEPS + 1], seed=2)[0]
    zw = _noises(len(iw), n, [K + 1], seed=3)[0]
    x0, x1 = _x0(M), _x0(M) * 0.7
    kw = dict(warm_start=K, elites=k, return_samples=True)
    plan.mpc_step_batch_box(x0, di, n, box, tol, noise=z0, **kw)
    before = plan.batch_priors().clone()
    got = plan.mpc_step_batch_box(x1, di, n, box, tol, noise=(zc, zw), reset=mask, **kw)
    after = plan.batch_priors().clone()
    assert tuple(after.shape) == ((M, n, H, D) if k else (M, H, D))
    plan.reset_warm_start()
    cold = plan.mpc_step_batch_box(x1[ic], di, n, box, tol, noise=zc, **kw)
    cold_priors = plan.batch_priors().clone()
    plan.set_batch_priors(before[torch.from_numpy(iw).to(plan.device)])
    warm = plan.mpc_step_batch_box(x1[iw], di, n, box, tol, noise=zw, **kw)
    warm_priors = plan.batch_priors().clone()
    # the box is live in this step: states 0, 1 and 3 start more than dt * |a|_max = 0.1 outside it on one velocity
    assert (np.abs(x1[[0, 1, 3], 2:]) - 0.1 > [0.5, 0.6]).any(axis=1).all()
    assert (got.flags[[0, 1, 3]] & INFEASIBLE).all() and (got.violation[[0, 1, 3]] > 0).all()
    for idx, sub, pri in ((ic, cold, cold_priors), (iw, warm, warm_priors)):
        for f in ("u", "plan", "cost", "flags", "violation", "n_feasible") + (("elite_cost", "elite_violation") if k else ()):
            _eq(getattr(got, f)[idx], getattr(sub, f), f)
        local = np.arange(len(idx)) * n
        np.testing.assert_array_equal(got.index[idx] - idx * n, sub.index - local)
        if k:
            np.testing.assert_array_equal(got.elite_index[idx] - (idx * n)[:, None], sub.elite_index - local[:, None])
            np.testing.assert_array_equal(got.elite_index[:, 0], got.index)
        else:
            assert got.elite_index is None and got.elite_violation is None
        t = torch.from_numpy(idx).to(plan.device)
        assert torch.equal(after[t], pri)
        assert torch.equal(got.u_norm.view(M, n, H, D)[t], sub.u_norm.view(len(idx), n, H, D))


def test_workspace_reuse():
    """calls that change M, n and k on one context, interleaved with the plain and the elite call: every result is a
    fresh context's (the partial lists, counts and the self-resetting counters carry nothing over)"""
    plan, di = _new_plan(), _di()
    box = _box(4, {2: (-1.0, 1.0), 3: (-1.2, 1.2)})[0]
    noise = {(M, n): _noises(M, n, [NSTEPS + 1])[0] for M, n in ((5, 16), (3, 200), (2, 4160))}

    def step(p, kind, M, n, k):
        p.reset_warm_start()
        z = noise[(M, n)]
        if kind == "box":
            return p.mpc_step_batch_box(_x0(M), di, n, box, noise=z, warm_start=K, elites=k)
        return p.mpc_step_batch(_x0(M), di, n, noise=z, warm_start=K, elites=k)

    seq = [("box", 3, 200, 64), ("box", 5, 16, 3), ("plain", 5, 16, None), ("box", 5, 16, None), ("box", 2, 4160, 8),
           ("plain", 3, 200, 64), ("box", 5, 16, 3), ("box", 3, 200, 64), ("plain", 2, 4160, 8), ("box", 3, 200, None)]
    fresh = {}
    for kind, M, n, k in seq:
        got = step(plan, kind, M, n, k)
        if (kind, M, n, k) not in fresh:
            fresh[(kind, M, n, k)] = step(_new_plan(), kind, M, n, k)
        fields = ("u", "plan", "cost", "index", "flags") + (("violation", "n_feasible") if kind == "box" else ())
        fields += (("elite_index", "elite_cost") if k else ()) + (("elite_violation",) if k and kind == "box" else ())
        _assert_states_equal(got, fresh[(kind, M, n, k)], range(M), fields)


# ---- 9. refusals

def _b_args(keep, M, k=None, box=None, tol=0.0):
    b = N.BatchBoxArgs()
    keep["box"] = box if box is not None else DiffusionMPC._state_box(([None] * 4, [None] * 4), 4)
    keep["viol"], keep["nfeas"] = np.zeros(M), np.zeros(M, dtype=np.int64)
    b.box, b.tol = ctypes.pointer(keep["box"]), tol
    b.viol_host, b.n_feasible_host = keep["viol"].ctypes.data, keep["nfeas"].ctypes.data
    if k:
        keep["eviol"] = np.zeros((M, k))
        b.elite_viol_host = keep["eviol"].ctypes.data
    return b


def _call(plan, a, e, b):
    return plan._lib.mpcd_mpc_step_batch_box(plan._ctx, ctypes.byref(a), None if e is None else ctypes.byref(e),
                                             None if b is None else ctypes.byref(b), None)


def _bad_box(lo=None, hi=None):
    box = DiffusionMPC._state_box(([None] * 4, [None] * 4), 4)
    for side, v in ((box.lo, lo), (box.hi, hi)):
        if v is not None:
            side[v[0]] = v[1]
    return box


@pytest.mark.parametrize("what,word", [
    ("no_box_args", b"null"), ("no_box", b"null"), ("no_viol", b"null"), ("no_nfeas", b"null"), ("nan_bound", b"NaN"),
    ("nan_bound_past_nx", b"NaN"), ("lo_above_hi", b"lo[1]"), ("tol_negative", b"tol"), ("tol_nan", b"tol"),
    ("reserved", b"reserved"), ("reserved2", b"reserved"), ("select_first", b"select_first"),
    ("elite_viol_without_elite", b"elite_viol_host"), ("n_states", b"n_states"), ("clip_rule", b"clip_rule"),
    ("warm_without_priors", b"priors"), ("k", b"k 5 outside"), ("elite_reserved", b"reserved"),
    ("state_priors_with_elite", b"args->priors")])
def test_c_abi_einval(what, word):
    plan, keep = _plan(), {}
    M, n = 2, 4
    a = _c_args(plan, _di(), M, n, keep)
    e = _e_args() if what in ("k", "elite_reserved", "state_priors_with_elite", "select_first") else None
    b = _b_args(keep, M)
    if what == "no_box_args":
        b = None
    elif what == "no_box":
        b.box = ctypes.POINTER(N.StateBox)()
    elif what == "no_viol":
        b.viol_host = None
    elif what == "no_nfeas":
        b.n_feasible_host = None
    elif what == "nan_bound":
        b = _b_args(keep, M, box=_bad_box(hi=(2, float("nan"))))
    elif what == "nan_bound_past_nx":
        b = _b_args(keep, M, box=_bad_box(lo=(7, float("nan"))))
    elif what == "lo_above_hi":
        b = _b_args(keep, M, box=_bad_box(lo=(1, 1.0), hi=(1, 0.5)))
    elif what == "tol_negative":
        b.tol = -1e-9
    elif what == "tol_nan":
        b.tol = float("nan")
    elif what in ("reserved", "reserved2"):
        setattr(b, what, 1)
    elif what == "select_first":
        a.select_first = 1
        assert _call(plan, a, None, b) == -1 and b"select_first" in plan._lib.mpcd_last_error()  # without elites too
    elif what == "elite_viol_without_elite":
        keep["ev"] = np.zeros((M, 1))
        b.elite_viol_host = keep["ev"].ctypes.data
    elif what == "n_states":
        a.n_states = 0
    elif what == "clip_rule":
        a.clip_rule = N.MPCD_CLIP_NONE
    elif what == "warm_without_priors":
        a.warm_t_start = 5
    elif what == "k":
        e.k = 5
    elif what == "elite_reserved":
        e.reserved = 1
    elif what == "state_priors_with_elite":
        a.priors = 256
    assert _call(plan, a, e, b) == -1
    assert word in plan._lib.mpcd_last_error(), plan._lib.mpcd_last_error()
    assert b"mpcd_mpc_step_batch_box" in plan._lib.mpcd_last_error()
    assert plan._lib.mpcd_mpc_step_batch_box(plan._ctx, None, None, ctypes.byref(_b_args(keep, M)), None) == -1


def test_c_abi_eunsup():
    keep, di = {}, _di()
    h2 = _plan("f16x2")
    assert _call(h2, _c_args(h2, di, 2, 4, keep), None, _b_args(keep, 2)) == -5
    assert b"F16X2" in h2._lib.mpcd_last_error()
    lb = _new_plan()
    N.check(lb._lib.mpcd_comm_init_loopback(lb._ctx, 1, 0, 0x5eed), "mpcd_comm_init_loopback")
    assert _call(lb, _c_args(lb, di, 2, 4, keep), _e_args(), _b_args(keep, 2, 2)) == -5
    assert b"communicator" in lb._lib.mpcd_last_error()
    plan = _plan()
    a = _c_args(plan, di, 2, 4, keep)
    pri = torch.zeros(2, H, D, device=plan.device)
    a.priors, a.sample.sampler, a.warm_t_start = pri.data_ptr(), N.MPCD_DDIM_CFG, 5
    assert _call(plan, a, None, _b_args(keep, 2)) == -5
    assert b"CFG-DDPM" in plan._lib.mpcd_last_error()


def test_c_call_and_the_other_two_calls_unchanged():
    """the C entry point end to end (cold, Philox) against the Python wrapper; mpcd_mpc_step_batch and
    mpcd_mpc_step_batch_elite return byte-identical results before and after box calls on the same context"""
    M, n, k = 3, 80, 8
    plan, di = _new_plan(), _di()
    L = plan._lib

    def plain():
        keep = {}
        a = _c_args(plan, di, M, n, keep)
        assert L.mpcd_mpc_step_batch(plan._ctx, ctypes.byref(a), None) == 0, L.mpcd_last_error()
        return keep["rec"].tobytes() + keep["u"].tobytes()

    def elite():
        keep = {}
        a, e = _c_args(plan, di, M, n, keep), _e_args(k)
        best = np.zeros((M, k, 2), dtype=np.int64)
        e.elites_host = best.ctypes.data
        assert L.mpcd_mpc_step_batch_elite(plan._ctx, ctypes.byref(a), ctypes.byref(e), None) == 0, L.mpcd_last_error()
        return keep["rec"].tobytes() + keep["u"].tobytes() + best.tobytes()

    before = plain(), elite()
    box = DiffusionMPC._state_box(_box(4, {2: (-1.0, 1.0), 3: (-1.2, 1.2)})[0], 4)
    for with_elites in (True, False):
        keep = {}
        a = _c_args(plan, di, M, n, keep)
        e = _e_args(k) if with_elites else None
        b = _b_args(keep, M, k if with_elites else None, box=box, tol=0.05)
        best = np.zeros((M, k, 2), dtype=np.int64)
        if with_elites:
            e.elites_host = best.ctypes.data
        torch.cuda.synchronize()
        assert _call(plan, a, e, b) == 0, L.mpcd_last_error()
        plan.reset_warm_start()
        want = plan.mpc_step_batch_box(_x0(M), di, n, _box(4, {2: (-1.0, 1.0), 3: (-1.2, 1.2)})[0], 0.05, warm_start=K,
                                       elites=k if with_elites else None)
        rec = keep["rec"].view(np.dtype([("cost", "<f8"), ("index", "<i8"), ("flags", "<i4"), ("reserved", "<i4")]))[:, 0]
        _eq(rec["cost"].copy(), want.cost, "cost")
        _eq(rec["index"].copy(), want.index, "index")
        _eq(rec["flags"].copy(), want.flags, "flags")
        assert (rec["reserved"] == 0).all()
        _eq(keep["u"], want.u, "u")
        _eq(keep["viol"], want.violation, "violation")
        _eq(keep["nfeas"], want.n_feasible, "n_feasible")
        assert (want.violation > 0).any() or (want.n_feasible < n).any()  # the box is live
        if with_elites:
            _eq(np.ascontiguousarray(best[..., 1]), want.elite_index, "elite_index")
            _eq(np.ascontiguousarray(best[..., 0]), want.elite_cost.view(np.int64), "elite_cost")
            _eq(keep["eviol"], want.elite_violation, "elite_violation")
        assert (plain(), elite()) == before


def test_python_refusals():
    di, plan = _di(), _plan()
    box = _box(4, {2: (-1.0, 1.0)})[0]
    with pytest.raises(ValueError, match="follow-up") as err:
        plan.mpc_step_batch(_x0(2), di, 8, state_box=box)
    assert "mpc_step_batch_box" in str(err.value)
    with pytest.raises(ValueError, match="state_box ranks candidates feasibility-first: it needs select='argmin'"):
        plan.mpc_step_batch_box(_x0(2), di, 8, box, select="first")
    with pytest.raises(ValueError, match="warm_start"):
        plan.mpc_step_batch_box(_x0(2), di, 8, box, elites=2)
    for k in (0, 9, 65):
        with pytest.raises(ValueError, match="elites"):
            plan.mpc_step_batch_box(_x0(2), di, 8 if k < 65 else 80, box, warm_start=K, elites=k)
    with pytest.raises(ValueError, match="viol_tol"):
        plan.mpc_step_batch_box(_x0(2), di, 8, box, -0.1)
    with pytest.raises(ValueError, match="viol_tol"):
        plan.mpc_step_batch_box(_x0(2), di, 8, box, float("nan"))
    with pytest.raises(ValueError, match="state_box"):
        plan.mpc_step_batch_box(_x0(2), di, 8, None)
    with pytest.raises(ValueError, match="n_x"):
        plan.mpc_step_batch_box(_x0(2), di, 8, ([0.0] * 3, [1.0] * 3))
    with pytest.raises(ValueError, match="not an interval"):
        plan.mpc_step_batch_box(_x0(2), di, 8, ([1.0, None, None, None], [0.0, None, None, None]))
    with pytest.raises(TypeError):
        plan.mpc_step_batch_box(_x0(2), di, 8, box, 0.0, state_box=box)
    with pytest.raises(ValueError, match="f16x2"):
        _plan("f16x2").mpc_step_batch_box(_x0(2), di, 8, box)
