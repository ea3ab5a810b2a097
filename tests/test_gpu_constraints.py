"""GPU: the constraint set - linear rows and input-rate bounds beside the state box (mpcd_rollout_cost_constr;
DiffusionMPC.rollout_cost_constr, mpc_step(constraints=), closed_loop(constraints=)).

The reference is written here and never is the code under test. It is tests/test_gpu_state_box.py's: an fp64 rollout
through oracle.systems.step gives the visited states, the row sums are an explicit Python loop over the components in
the contract's order (numpy rounds every product and every sum on its own), numpy.lexsort gives the order. The inputs u
are fp32 values promoted to fp64, hence exact; ranking and copying do not round. The one tolerance is the violation of
the three systems with sin / cos: the existing state bar 1e-9 max(1, max |x|) carried through a row sum, that is times
max(1, max_r sum_i |A[r][i]|)."""
import ctypes

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import Constraints, systems
from mpc_via_diffusion_model_amd import _native as nat
from mpc_via_diffusion_model_amd import distributed as D
from mpc_via_diffusion_model_amd.constraints import Feasibility

from ._util import unnormalize_np
from .test_gpu_comm import _key
from .test_gpu_rollout import EXACT, _limits, _planner, _x0
from .test_gpu_state_box import (BOX_COMPONENTS, EINVAL, INF, LOOP_K, LOOP_N, STATE_BAR, _loop_plan, _ptr, _rank, _same,
                                 _step_plan, _violation, _visited)

pytestmark = pytest.mark.gpu
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the reference
def _row_sums(xs, us, a, c):
    """s [B, n] of one row over the visited pairs (xs [B, n, n_x], us [B, n, n_u]): the contract's order, one rounding
    per product and per sum"""
    s = a[0] * xs[:, :, 0]
    for i in range(1, xs.shape[2]):
        s = s + a[i] * xs[:, :, i]
    for j in range(us.shape[2]):
        s = s + c[j] * us[:, :, j]
    return s


def _excess_max(e):
    """per plan the largest of the excesses e [B, ...], a NaN excess counting as +inf"""
    e = np.where(np.isnan(e), np.inf, e).reshape(len(e), -1)
    return e.max(axis=1) if e.shape[1] else np.full(len(e), -np.inf)


def _rows_violation(xs, us, rows):
    """max(0, the largest row excess) per plan; rows: [(a [n_x], c [n_u], b)]"""
    V = np.zeros(len(xs))
    with np.errstate(invalid="ignore"):
        for a, c, b in rows:
            V = np.maximum(V, _excess_max(_row_sums(xs, us, a, c) - b))
    return V


def _rate_steps(us, u_prev):
    """|u_k - u_{k-1}| [B, n, n_u] over the visited inputs; k = 0 against u_prev [B, n_u], where a row with a NaN (or
    u_prev None) has no predecessor: its entries are -inf, below every bound"""
    B, n, nu = us.shape
    prev = np.full((B, nu), np.nan) if u_prev is None else np.broadcast_to(np.asarray(u_prev, dtype=np.float64), (B, nu))
    none = np.isnan(prev).any(axis=1)
    with np.errstate(invalid="ignore"):
        first = np.where(none[:, None], -np.inf, np.abs(us[:, 0] - prev))
        return np.concatenate([first[:, None], np.abs(us[:, 1:] - us[:, :-1])], axis=1)


def _rate_violation(us, u_prev, du):
    with np.errstate(invalid="ignore"):  # no predecessor: -inf - du is no excess
        return np.maximum(0.0, _excess_max(_rate_steps(us, u_prev) - np.asarray(du, dtype=np.float64)))


def _set_violation(xs, us, lo, hi, rows, du, u_prev):
    """(box, rows, rate) violations per plan; the set's V is their elementwise maximum"""
    return _violation(xs, lo, hi), _rows_violation(xs, us, rows), _rate_violation(us, u_prev, du)


def _median(values):
    """the midpoint of the two middle distinct values (clipped plans tie), so both classes are present"""
    v = np.unique(values)
    assert len(v) >= 2, "the quantity does not separate the plans"
    return 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _median_box(xs, comps):
    """(lo, hi) lists with None = unbounded: +- the median of the largest magnitude the plans reach, on those of comps
    whose magnitude separates the plans (a component whose largest magnitude is x_1's does not depend on the plan)"""
    nx = xs.shape[2]
    reach = {c: np.unique(np.abs(xs[:, :, c]).max(axis=1)) for c in comps}
    reach = {c: _median(v) for c, v in reach.items() if len(v) >= 2}
    assert reach, "no component separates the plans"
    return (_full(nx, None, {c: -b for c, b in reach.items()}), _full(nx, None, {c: b for c, b in reach.items()})), reach


def _full(n, fill, entries):
    out = [fill] * n
    for i, v in entries.items():
        out[i] = v
    return out


def _inputs(name, spread, B=70, H=7, seed=5):
    """test_gpu_state_box.py's inputs: (system, planner, x0, u_norm, u [B, H, n_u] fp64, xs [B, n, n_x], us [B, n, n_u])"""
    sysd = systems.get(name)
    d = sysd.n_u
    rng = np.random.default_rng(seed)
    lo_u, hi_u = _limits(name)
    plan = _planner(d=d, C=2, lo=lo_u, hi=hi_u)
    x0 = _x0(name, rng)
    u_norm = rng.uniform(-spread, spread, (B, H, d)).astype(np.float32)
    u = unnormalize_np(u_norm, np.full(d, lo_u), np.full(d, hi_u)).astype(np.float64)
    xs = _visited(name, x0, u)
    return sysd, plan, x0, u_norm, u, xs, u[:, :xs.shape[1]]


def _median_set(name, xs, us, u_prev):
    """the issue's set on BOX_COMPONENTS' pair (i, j): x_i + 0.5 x_j <= b0, -x_i + 0.25 u_0 <= b1, du_max on input 0;
    each bound the median over the plans of the largest value the plan reaches"""
    nx, nu = xs.shape[2], us.shape[2]
    i, j = BOX_COMPONENTS[name]
    a0, a1 = np.array(_full(nx, 0.0, {i: 1.0, j: 0.5})), np.array(_full(nx, 0.0, {i: -1.0}))
    c0, c1 = np.zeros(nu), np.array(_full(nu, 0.0, {0: 0.25}))
    s0, s1 = _row_sums(xs, us, a0, c0), _row_sums(xs, us, a1, c1)
    rows = [(a0, c0, _median(s0.max(axis=1))), (a1, c1, _median(s1.max(axis=1)))]
    steps = _rate_steps(us, u_prev)[:, :, 0]
    du = _full(nu, INF, {0: _median(steps.max(axis=1))})
    margin = min(np.abs(s0 - rows[0][2]).min(), np.abs(s1 - rows[1][2]).min())
    return rows, du, margin, max(np.abs(a0).sum(), np.abs(a1).sum()), np.abs(steps - du[0]).min()


def _cons(rows=(), du=None, box=None):
    return Constraints(state_box=box, rows=[(list(a), list(c), float(b)) for a, c, b in rows],
                       du_max=None if du is None else [None if v == INF else v for v in du])


# ------------------------------------------------------------------------- 1. violation and cost, all six systems
@pytest.mark.parametrize("name", sorted(systems.REGISTRY))
@pytest.mark.parametrize("spread", [0.9, 1.3])  # 1.3: the clip rule is live
def test_violation_and_cost(name, spread):
    """B = 70, H = 7: one full one-wave workgroup and one of 6. Two rows, a rate bound on input 0 and a u_prev row; every
    bound at the median of the reference's per-plan maxima of its quantity, so feasible and infeasible plans are present
    for each part by construction."""
    sysd, plan, x0, u_norm, u, xs, us = _inputs(name, spread)
    B = len(u)
    u_prev = 0.5 * (u[0, 0] + u[1, 0])  # a previous action inside the limits
    rows, du, row_margin, asum, rate_margin = _median_set(name, xs, us, u_prev)
    scale = max(1.0, np.abs(xs).max())
    bar = STATE_BAR * scale * max(1.0, asum)
    assert row_margin > bar and rate_margin > 0, "the reference puts a value on a bound: move the bound"
    Vb, Vr, Vd = _set_violation(xs, us, np.full(sysd.n_x, -INF), np.full(sysd.n_x, INF), rows, du, u_prev)
    for r in range(2):
        vr = _rows_violation(xs, us, rows[r:r + 1])
        assert (vr > 0).any() and (vr == 0).any(), f"row {r} must hold both classes"
    assert (Vd > 0).any() and (Vd == 0).any(), "the rate bound must hold both classes"
    want = np.maximum(Vr, Vd)
    u_dev = torch.from_numpy(u_norm).cuda()
    free = plan.rollout_cost(sysd, x0, u_dev)
    cost, viol = plan.rollout_cost_constr(sysd, x0, u_dev, _cons(rows, du), u_prev=u_prev)
    assert cost.shape == viol.shape == (B,) and viol.dtype == torch.float64
    assert _same(cost, free), "the cost is not the unconstrained rollout's, bit for bit"
    got = viol.cpu().numpy()
    err = np.abs(got - want)
    print(f"\n{name} spread {spread}: {(want > 0).sum()} of {B} violate (rows {(Vr > 0).sum()}, rate {(Vd > 0).sum()}), "
          f"max |V - V_ref| = {err.max():.3e}, bar {bar:.3e}")
    if name in EXACT:
        np.testing.assert_array_equal(got, want)
    else:
        assert (err <= bar).all(), f"worst violation error {err.max():.3e} against {bar:.3e}"
    assert ((got == 0) == (want == 0)).all(), "feasibility differs from the reference"


# ------------------------------------------------------------------------ 2. each part alone, and their maximum
@pytest.mark.parametrize("name", sorted(systems.REGISTRY))
def test_parts_alone_and_their_maximum(name):
    sysd, plan, x0, u_norm, u, xs, us = _inputs(name, 1.3, seed=8)
    u_prev = 0.5 * (u[2, 0] + u[3, 0])
    rows, du, _, asum, _ = _median_set(name, xs, us, u_prev)
    box, reach = _median_box(xs, BOX_COMPONENTS[name])
    lo = np.array([-INF if v is None else v for v in box[0]])
    hi = np.array([INF if v is None else v for v in box[1]])
    Vb, Vr, Vd = _set_violation(xs, us, lo, hi, rows, du, u_prev)
    u_dev = torch.from_numpy(u_norm).cuda()
    bar = STATE_BAR * max(1.0, np.abs(xs).max()) * max(1.0, asum)
    got = {}
    for what, con, want, kw in (("box", _cons(box=box), Vb, {}), ("rows", _cons(rows), Vr, {}),
                                ("rate", _cons(du=du), Vd, dict(u_prev=u_prev)),
                                ("all", _cons(rows, du, box), np.maximum(np.maximum(Vb, Vr), Vd), dict(u_prev=u_prev))):
        assert (want > 0).any() and (want == 0).any(), what
        got[what] = plan.rollout_cost_constr(sysd, x0, u_dev, con, **kw)[1].cpu().numpy()
        if name in EXACT:
            np.testing.assert_array_equal(got[what], want, err_msg=what)
        else:
            assert (np.abs(got[what] - want) <= bar).all(), what
    np.testing.assert_array_equal(got["all"], np.maximum(np.maximum(got["box"], got["rows"]), got["rate"]))
    assert not (got["all"] == got["box"]).all() and not (got["all"] == got["rows"]).all() \
        and not (got["all"] == got["rate"]).all(), "one part decides every plan: the maximum is not tested"


# ----------------------------------------------------------------------- 3. identities against the parent's code
@pytest.mark.parametrize("name", sorted(systems.REGISTRY))
def test_identities(name):
    sysd, plan, x0, u_norm, u, xs, us = _inputs(name, 1.3, seed=9)
    nx = sysd.n_x
    box, reach = _median_box(xs, BOX_COMPONENTS[name])
    u_dev = torch.from_numpy(u_norm).cuda()
    cb, vb = plan.rollout_cost_box(sysd, x0, u_dev, box)
    assert (vb > 0).any() and (vb == 0).any()
    cc, vc = plan.rollout_cost_constr(sysd, x0, u_dev, Constraints(state_box=box))
    assert _same(cc, cb) and _same(vc, vb), "a set that is only a box is not rollout_cost_box, bit for bit"
    c0, v0 = plan.rollout_cost_constr(sysd, x0, u_dev, Constraints(), u_prev=u[0, 0])
    assert _same(c0, cb) and (v0 == 0).all() and not torch.signbit(v0).any(), "an all-infinite set must give V = 0"
    # the box as rows +-e_i: a sum of zeros and x_i is exact, so the excess x_i - hi_i (or lo_i - x_i) is the box's
    rows = []
    for c, b in reach.items():
        rows += [(_full(nx, 0.0, {c: 1.0}), None, b), (_full(nx, 0.0, {c: -1.0}), None, b)]
    cr, vr = plan.rollout_cost_constr(sysd, x0, u_dev, Constraints(rows=rows))
    assert _same(cr, cb) and _same(vr, vb), "the box rewritten as rows differs from the box"


# -------------------------------------------------------------------------------------------- 4. rate edge cases
@pytest.mark.parametrize("H", [3, 4])
def test_rate_edge_cases_calmpccost(H):
    """cartpole_lin5 costs with calMPCCost, which visits (x_1, u_0) .. (x_{H-2}, u_{H-3}): at H = 3 one pair, so the only
    rate term is u_0 against u_prev; at H = 4 the in-plan term |u_1 - u_0| exists as well."""
    sysd, plan, x0, u_norm, u, xs, us = _inputs("cartpole_lin5", 0.9, B=70, H=H)
    assert us.shape[1] == H - 2
    B = len(u)
    u_dev = torch.from_numpy(u_norm).cuda()
    u_prev = np.array([0.25])
    first = np.abs(u[:, 0, 0] - u_prev[0])
    du = [_median(first)]
    none = plan.rollout_cost_constr(sysd, x0, u_dev, _cons(du=du))[1].cpu().numpy()
    given = plan.rollout_cost_constr(sysd, x0, u_dev, _cons(du=du), u_prev=u_prev)[1].cpu().numpy()
    nanrow = plan.rollout_cost_constr(sysd, x0, u_dev, _cons(du=du), u_prev=[NAN])[1].cpu().numpy()
    inplan = np.maximum(0.0, np.abs(u[:, 1, 0] - u[:, 0, 0]) - du[0]) if H == 4 else np.zeros(B)
    np.testing.assert_array_equal(none, inplan)
    np.testing.assert_array_equal(nanrow, none)
    np.testing.assert_array_equal(given, np.maximum(inplan, np.maximum(0.0, first - du[0])))
    np.testing.assert_array_equal(given, _rate_violation(us, u_prev, du))
    assert (given > none).any() and (given == none).any(), "u_prev must decide some plans and not others"
    if H == 3:
        assert (none == 0).all(), "one visited pair: no in-plan rate term"
    else:
        assert (none > 0).any()


@pytest.mark.parametrize("name", ["double_int2d", "cartpole_lin5"])
def test_rate_with_a_u_prev_row_per_state(name):
    """M = 3 states of g = 5 candidates: one workgroup's lanes belong to three states with a finite row, a NaN-sentinel
    row (one NaN entry is enough) and another finite row"""
    sysd = systems.get(name)
    M, g, H, d = 3, 5, 4, sysd.n_u
    rng = np.random.default_rng(3)
    lo_u, hi_u = _limits(name)
    plan = _planner(d=d, C=2, lo=lo_u, hi=hi_u)
    x0 = np.stack([_x0(name, rng) for _ in range(M)])
    u_norm = rng.uniform(-0.9, 0.9, (M * g, H, d)).astype(np.float32)
    u = unnormalize_np(u_norm, np.full(d, lo_u), np.full(d, hi_u)).astype(np.float64)
    u_prev = rng.uniform(lo_u, hi_u, (M, d))
    u_prev[1, d - 1] = NAN
    per_plan = np.repeat(u_prev, g, axis=0)
    xs = np.concatenate([_visited(name, x0[m], u[m * g:(m + 1) * g]) for m in range(M)])
    us = u[:, :xs.shape[1]]
    du = [_median(_rate_steps(us, per_plan)[:, :, j].max(axis=1)) for j in range(d)]
    want = _rate_violation(us, per_plan, du)
    assert (want > 0).any() and (want == 0).any()
    got = plan.rollout_cost_constr(sysd, x0, torch.from_numpy(u_norm).cuda(), _cons(du=du), group=g, u_prev=u_prev)[1]
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    other = _rate_violation(us, np.repeat(u_prev[::-1], g, axis=0), du)
    assert (other != want).any(), "the rows must matter per state"
    dev_prev = torch.from_numpy(u_prev).cuda()  # a device tensor is taken as it is
    again = plan.rollout_cost_constr(sysd, x0, torch.from_numpy(u_norm).cuda(), _cons(du=du), group=g, u_prev=dev_prev)[1]
    assert _same(again, got)


# ------------------------------------------------------------------------------------------- 5. NaN and infinity
def test_nan_and_infinity():
    sysd, plan, x0, u_norm, u, xs, us = _inputs("double_int2d", 0.9, B=70, H=7)
    u_norm = u_norm.copy()
    u_norm[7, 3, 1] = NAN  # a NaN makes the clip code 2: no clipping, as for the reference's inputs (spread 0.9)
    con = _cons([(np.array([1.0, 0, 0, 0]), np.zeros(2), 1e6)], [1e6, 1e6])
    cost, viol = plan.rollout_cost_constr(sysd, x0, torch.from_numpy(u_norm).cuda(), con, u_prev=[0.0, 0.0])
    cost, viol = cost.cpu().numpy(), viol.cpu().numpy()
    assert np.isnan(cost[7]) and viol[7] == INF
    keep = np.arange(70) != 7
    assert np.isfinite(cost[keep]).all() and (viol[keep] == 0).all()
    # a NaN input alone: the rate test of a set without rows sees it (the box's states are NaN as well)
    v2 = plan.rollout_cost_constr(sysd, x0, torch.from_numpy(u_norm).cuda(), _cons(du=[1e6, 1e6]))[1].cpu().numpy()
    assert v2[7] == INF and (v2[keep] == 0).all()
    # a zero coefficient on a component driven to infinity: 0 * inf is NaN, the excess is NaN, V = +inf
    xinf = x0.copy()
    xinf[1] = INF
    u_dev = torch.from_numpy(_inputs("double_int2d", 0.9)[3]).cuda()
    row_x0 = _cons([(np.array([1.0, 0.0, 0, 0]), np.zeros(2), 1e6)])
    v3 = plan.rollout_cost_constr(sysd, xinf, u_dev, row_x0)[1].cpu().numpy()
    assert (v3 == INF).all(), "0 * inf must not be dropped"
    v4 = plan.rollout_cost_constr(sysd, x0, u_dev, row_x0)[1].cpu().numpy()
    assert (v4 == 0).all()
    # b = +inf switches a row off even where the sum is large
    off = _cons([(np.array([1e9, 0.0, 0, 0]), np.zeros(2), INF)])
    assert (plan.rollout_cost_constr(sysd, x0, u_dev, off)[1] == 0).all()


# --------------------------------------------------------------------------------- 6. mpc_step(constraints=)
def _di_set(xs, us, u_prev):
    """double_int2d: a row on the velocities, a mixed row and a rate bound on input 0, each at its median"""
    a0, c0 = np.array([0.0, 0.0, 1.0, 0.5]), np.zeros(2)
    a1, c1 = np.array([0.0, 0.0, -1.0, 0.0]), np.array([0.25, 0.0])
    rows = [(a0, c0, _median(_row_sums(xs, us, a0, c0).max(axis=1))), (a1, c1, _median(_row_sums(xs, us, a1, c1).max(axis=1)))]
    return rows, [_median(_rate_steps(us, u_prev)[:, :, 0].max(axis=1)), INF]


def test_mpc_step_constraints():
    plan, sysm, B = _step_plan(), systems.double_int2d(), 100
    x0 = np.array([0.4, -0.3, 0.2, -0.1])
    kw = dict(seed=7, clip_rule="final")
    free = plan.mpc_step(x0, sysm, B, native=False, **kw)
    u = unnormalize_np(free.u_norm.cpu().numpy(), plan.act_min, plan.act_max).astype(np.float64)
    xs = _visited("double_int2d", x0, u)
    costs = free.costs.cpu().numpy()
    u_prev = np.array([0.3, -0.1])
    rows, du = _di_set(xs, u, u_prev)
    lo, hi = np.full(4, -INF), np.full(4, INF)
    hi[3] = _median(np.abs(xs[:, :, 3]).max(axis=1))
    lo[3] = -hi[3]
    box = ([None, None, None, lo[3]], [None, None, None, hi[3]])
    moved = 0
    for what, con, up in (("rows", _cons(rows), None), ("rate", _cons(du=du), u_prev), ("rate, no u_prev", _cons(du=du), None),
                          ("all", _cons(rows, du, box), u_prev)):
        parts = _set_violation(xs, u, lo if what == "all" else np.full(4, -INF), hi if what == "all" else np.full(4, INF),
                               rows if what in ("rows", "all") else [], du if what != "rows" else [INF, INF], up)
        ref_v = np.maximum(np.maximum(parts[0], parts[1]), parts[2])
        for tol in (0.0, 0.01):
            res = plan.mpc_step(x0, sysm, B, constraints=con, u_prev=up, viol_tol=tol, **kw)
            assert _same(res.u_norm, free.u_norm) and _same(res.costs, free.costs)
            wi, wc, wv, wn = _rank(costs, ref_v, 1, 1, tol)
            print(f"\n{what} tol {tol}: n_feasible {res.n_feasible}, winner {res.best_index}, V {res.violation:.4g}")
            assert (res.best_index, res.best_cost, res.violation, res.n_feasible) == (wi[0, 0], wc[0, 0], wv[0, 0], wn[0])
            np.testing.assert_array_equal(res.u_best, u[res.best_index].astype(np.float32))
            assert res.n_feasible < B and (what == "all" or res.n_feasible > 0)
            moved += res.best_index != free.best_index
    assert moved, "no set moved the winner"
    loose = plan.mpc_step(x0, sysm, B, constraints=Constraints(), **kw)
    assert (loose.best_index, loose.best_cost, loose.violation, loose.n_feasible) == (free.best_index, free.best_cost, 0.0, B)


# ------------------------------------------------------------------------------- 7. closed_loop(constraints=)
def _public_loop(plan, x0, sysm, T, n, con, tol, u_prev, noise, K, k):
    """closed_loop(constraints=)'s iteration from the public methods (and the two library calls closed_loop makes for the
    context rows and the clip flags); also returns every iteration's (samples, clip codes, V of every candidate, u_prev)"""
    M, nx = x0.shape
    H, B, L, st = plan.spec.horizon, M * n, plan._lib, plan._stream()
    x = torch.from_numpy(x0.copy()).cuda()
    ctx = torch.empty((M, nx), dtype=torch.float32, device="cuda")
    flags = torch.empty(M, dtype=torch.int32, device="cuda")
    absmax = torch.empty(B, dtype=torch.float32, device="cuda")
    out = dict(x=[x0.copy()], u=[], cost=[], index=[], violation=[], n_feasible=[])
    its, priors = [], None
    up = None if u_prev is None else torch.from_numpy(np.asarray(u_prev, dtype=np.float64)).cuda()
    for it in range(T):
        nat.check(L.mpcd_normalize_states(plan._ctx, _ptr(x), M, nx, plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data,
                                          _ptr(ctx), st), "mpcd_normalize_states")
        warm = {} if priors is None else dict(x_init=priors, t_start=K)
        u_norm = plan.sample_trajectories(ctx.repeat_interleave(n, 0), B, H, w=0.01, noise=noise(it), absmax_out=absmax,
                                          **warm)
        nat.check(L.mpcd_clip_flags(plan._ctx, _ptr(absmax), M, n, _ptr(flags), st), "mpcd_clip_flags")
        x_before = x.cpu().numpy().copy()
        cost, viol = plan.rollout_cost_constr(sysm, x, u_norm, con, group=n, clip_flags=flags, u_prev=up)
        idx, c, v, nf = plan.topk_feasible(cost, viol, k or 1, n_groups=M, tol=tol)
        u_it, i_it, c_it = plan.control_step_picked(sysm, x, u_norm, idx[:, 0].contiguous(), c[:, 0].contiguous(), flags)
        its.append((x_before, u_norm.cpu().numpy().copy(), flags.cpu().numpy().copy(), viol.cpu().numpy().copy(),
                    None if up is None else up.cpu().numpy().copy()))
        up = u_it
        if k is not None:
            priors = plan.elite_priors(u_norm, idx, n)
        elif K is not None:
            priors = plan.shift_plans(u_norm, i_it).repeat_interleave(n, 0)
        for f, t in zip(("x", "u", "cost", "index", "violation", "n_feasible"), (x, u_it, c_it, i_it, v[:, 0], nf)):
            out[f].append(t.cpu().numpy().copy())
    return {f: np.stack(a, 1) for f, a in out.items()}, its


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm_start_5_elites_4"])
@pytest.mark.parametrize("first", ["u_prev", "none"])
def test_closed_loop_constraints(warm, first):
    """M = 3 states, 16 candidates, 4 iterations, the rate bound the only one: V of every candidate of every iteration
    against the host reference with the action applied one iteration earlier as u_prev; a reference with any other
    predecessor gives another V."""
    plan, sysm = _loop_plan(), systems.double_int2d()
    T, M, n, H, d = 4, 3, 16, 16, 2
    x0 = np.array([[0.3, -0.2, 0.1, 0.05], [0.25, -0.1, -0.12, 0.0], [-0.2, 0.3, 0.05, -0.1]])
    K, k = (LOOP_K, 4) if warm else (None, None)
    g = torch.Generator().manual_seed(4)
    draws = [torch.randn((LOOP_N if it == 0 or not warm else LOOP_K) + 1, M * n, H, d, generator=g) for it in range(T)]
    u_prev = np.array([[0.5, -0.5], [NAN, 0.0], [-0.25, 0.75]]) if first == "u_prev" else None
    # the bounds: per input the median over the last iteration's plans of an unconstrained native loop (which returns
    # them) of the largest step inside the plan; only the choice of the bounds rests on that loop. Warm plans are
    # smoother than cold ones: under their median the cold iteration 0 has few feasible plans, or none, a case too
    u0 = plan.closed_loop(x0, sysm, T, n_samples=n, w=0.01, noise=lambda it: draws[it], warm_start=K,
                          native=True).u_norm.cpu().numpy()
    inplan = np.abs(np.diff(np.clip(u0, -1, 1).astype(np.float64), axis=1)).max(axis=1)
    du, tol = [float(_median(inplan[:, j])) for j in range(d)], 0.01
    con = Constraints(du_max=du)
    passed, raw = [], Feasibility.rollout  # what the loop hands the rollout as u_prev, iteration by iteration

    def spy(feas, pl, desc, x_dev, group, u_norm, flags, cost, viol, up=None):
        passed.append(None if up is None else up.cpu().numpy().copy())
        return raw(feas, pl, desc, x_dev, group, u_norm, flags, cost, viol, up)

    Feasibility.rollout = spy
    try:
        got = plan.closed_loop(x0, sysm, T, n_samples=n, w=0.01, noise=lambda it: draws[it], warm_start=K, elites=k,
                               constraints=con, u_prev=u_prev, viol_tol=tol)
    finally:
        Feasibility.rollout = raw
    assert len(passed) == T and (passed[0] is None if u_prev is None else np.array_equal(passed[0], u_prev, equal_nan=True))
    for it in range(1, T):
        np.testing.assert_array_equal(passed[it], got.u[:, it - 1], err_msg="u_prev is not the action applied last")
    want, its = _public_loop(plan, x0, sysm, T, n, con, tol, u_prev, lambda it: draws[it], K, k)
    print(f"\nn_feasible\n{got.n_feasible}\nviolation\n{got.violation}")
    for f in ("x", "u", "cost", "index", "violation", "n_feasible"):
        a, b = np.ascontiguousarray(getattr(got, f)), want[f]
        assert a.shape == b.shape and a.dtype == b.dtype, f
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64), err_msg=f)
    assert ((0 < got.n_feasible) & (got.n_feasible < n)).any(), "the bound must separate candidates"
    differs = 0
    for it, (x_it, u_norm, codes, viol, up) in enumerate(its):
        np.testing.assert_array_equal(x_it, got.x[:, it])
        if it > 0:
            np.testing.assert_array_equal(up, got.u[:, it - 1], err_msg="u_prev is not the action applied last")
        for m in range(M):
            un = u_norm[m * n:(m + 1) * n]
            x32 = np.clip(un, np.float32(-1), np.float32(1)) if codes[m] == 1 else un
            u = ((x32 + np.float32(1)) / np.float32(2) * (plan.act_max - plan.act_min) + plan.act_min).astype(np.float64)
            ref = _rate_violation(u, None if up is None else up[m], du)
            np.testing.assert_array_equal(viol[m * n:(m + 1) * n], ref, err_msg=f"iteration {it} state {m}")
            assert (ref <= tol).sum() == got.n_feasible[m, it]
            if it > 0:  # the predecessor decides a candidate's class: without it, n_feasible would be another
                differs += int(((_rate_violation(u, None, du) <= tol) != (ref <= tol)).any())
    print(f"later (state, iteration) pairs in which the applied action decides a candidate's class: {differs}")
    # cold plans are rough enough for the first step to decide; warm ones (seeded from the shifted elites) are not at
    # these bounds, where the check above on what the loop passes stands alone
    assert differs >= 1 or warm, "the predecessor of u_0 never binds"


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_python_refusals():
    plan, sysm, x0 = _loop_plan(), systems.double_int2d(), np.zeros(4)
    con = Constraints(du_max=[0.5, None])
    box = ([None, None, -1.0, -1.0], [None, None, 1.0, 1.0])
    for kw in (dict(native=True), dict(warm_start=LOOP_K), dict(warm_start=LOOP_K, elites=2), dict(prior=torch.zeros(16, 2))):
        with pytest.raises(ValueError, match="constraint"):
            plan.mpc_step(x0, sysm, 12, constraints=con, **kw)
    ranked = _loop_plan()
    comm = D.NativeComm(ranked, loopback=(1, 0, _key()))
    with pytest.raises(ValueError, match="single-rank"):
        ranked.mpc_step(x0, sysm, 12, constraints=con, comm=comm)
    xs = np.zeros((2, 4))
    with pytest.raises(ValueError, match="put the box into the set"):
        plan.mpc_step(x0, sysm, 12, constraints=con, state_box=box)
    with pytest.raises(ValueError, match="put the box into the set"):
        plan.closed_loop(xs, sysm, 2, n_samples=4, constraints=con, state_box=box)
    with pytest.raises(ValueError, match="native=True"):
        plan.closed_loop(xs, sysm, 2, n_samples=4, constraints=con, native=True)
    with pytest.raises(ValueError, match="argmin"):
        plan.closed_loop(xs, sysm, 2, n_samples=4, constraints=con, select="first")
    with pytest.raises(ValueError, match="u_prev"):
        plan.closed_loop(xs, sysm, 2, n_samples=4, u_prev=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="u_prev"):
        plan.mpc_step(x0, sysm, 12, u_prev=np.zeros(2))
    with pytest.raises(ValueError, match=r"u_prev must be \[2, 2\]"):
        plan.closed_loop(xs, sysm, 2, n_samples=4, constraints=con, u_prev=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="Constraints"):
        plan.mpc_step(x0, sysm, 12, constraints=box)
    for tol in (-0.1, NAN):
        with pytest.raises(ValueError):
            plan.mpc_step(x0, sysm, 12, constraints=con, viol_tol=tol)
    u = torch.zeros(12, 16, 2, device="cuda")
    for bad in (Constraints(rows=[([1.0] * 3, None, 0.0)]), Constraints(rows=[([1.0] * 4, [NAN, 0.0], 0.0)]),
                Constraints(rows=[([1.0] * 4, None, 0.0)] * 9), Constraints(du_max=[-1.0, 0.0]),
                Constraints(du_max=[1.0]), Constraints(state_box=([1.0, 0, 0, 0], [0.0, 1, 1, 1]))):
        with pytest.raises(ValueError):
            plan.rollout_cost_constr(sysm, np.zeros((2, 4)), u, bad)
    with pytest.raises(ValueError):
        plan.rollout_cost_constr(sysm, np.zeros((5, 4)), u, con)  # 12 candidates are not 5 groups
    with pytest.raises(ValueError, match="u_prev"):
        plan.rollout_cost_constr(sysm, np.zeros((2, 4)), u, con, u_prev=np.zeros((2, 3)))


def test_c_refusals():
    plan, L, sysm = _loop_plan(), nat.lib(), systems.double_int2d()
    B, H, d, M = 12, 16, 2, 2
    desc = sysm.desc()
    u = torch.zeros(B, H, d, device="cuda")
    x = torch.zeros(M, 4, dtype=torch.float64, device="cuda")
    up = torch.zeros(M, d, dtype=torch.float64, device="cuda")
    flags = torch.zeros(M, dtype=torch.int32, device="cuda")
    cost = torch.zeros(B, dtype=torch.float64, device="cuda")
    viol = torch.zeros(B, dtype=torch.float64, device="cuda")
    err = lambda: L.mpcd_last_error().decode(errors="replace")  # noqa: E731

    def con(**edit):
        c = Constraints(rows=[([1.0, 0, 0, 0], [0.5, 0], 2.0), ([0, 1.0, 0, 0], None, 3.0)], du_max=[1.0, None]).native(4, 2)
        for f, v in edit.items():
            if f in ("n_rows", "reserved"):
                setattr(c, f, v)
            elif f in ("lo", "hi"):
                getattr(c.box, f)[v[0]] = v[1]
            elif f in ("A", "C"):
                getattr(c, f)[v[0]][v[1]] = v[2]
            else:
                getattr(c, f)[v[0]] = v[1]
        return c

    umin, umax = plan.act_min.ctypes.data, plan.act_max.ctypes.data
    ok = (ctypes.byref(desc), _ptr(x), B // M, _ptr(u), umin, umax, B, H, _ptr(flags), ctypes.byref(con()), _ptr(up),
          _ptr(cost), _ptr(viol))

    def with_(args, i, v):
        return args[:i] + (v,) + args[i + 1:]

    def with_con(**edit):
        return with_(ok, 9, ctypes.byref(con(**edit)))

    assert L.mpcd_rollout_cost_constr(plan._ctx, *ok, None) == 0, err()
    assert L.mpcd_rollout_cost_constr(plan._ctx, *with_(ok, 10, None), None) == 0, "u_prev may be NULL"
    bad = [("null con", with_(ok, 9, None)), ("null viol", with_(ok, 12, None)), ("null cost", with_(ok, 11, None)),
           ("null x0", with_(ok, 1, None)), ("group 5", with_(ok, 2, 5)), ("group 0", with_(ok, 2, 0)),
           ("batch 0", with_(ok, 6, 0)), ("horizon 1", with_(ok, 7, 1)),
           ("NaN bound", with_con(lo=(0, NAN))), ("NaN bound past n_x", with_con(hi=(7, NAN))),
           ("lo > hi", with_con(lo=(3, 1.0), hi=(3, 0.5))),
           ("n_rows -1", with_con(n_rows=-1)), ("n_rows 9", with_con(n_rows=9)), ("reserved", with_con(reserved=1)),
           ("A NaN", with_con(A=(1, 3, NAN))), ("A inf", with_con(A=(0, 0, INF))), ("C -inf", with_con(C=(1, 1, -INF))),
           ("C NaN", with_con(C=(0, 0, NAN))), ("b NaN", with_con(b=(1, NAN))), ("b -inf", with_con(b=(0, -INF))),
           ("du NaN", with_con(du_max=(0, NAN))), ("du negative", with_con(du_max=(1, -1e-9)))]
    for what, args in bad:
        assert L.mpcd_rollout_cost_constr(plan._ctx, *args, None) == EINVAL and err(), what
    assert L.mpcd_rollout_cost_constr(plan._ctx, *with_con(A=(1, 3, NAN)), None) == EINVAL and "A[1][3]" in err()
    assert L.mpcd_rollout_cost_constr(plan._ctx, *with_con(du_max=(1, -1.0)), None) == EINVAL and "du_max[1]" in err()
    # what the contract ignores or allows: entries past n_x / n_u / n_rows, b = +inf, du_max = 0 and +inf
    for what, args in (("A past n_x", with_con(A=(0, 4, NAN))), ("C past n_u", with_con(C=(0, 2, INF))),
                       ("row past n_rows", with_con(A=(2, 0, NAN), b=(2, NAN))), ("du past n_u", with_con(du_max=(2, -1.0))),
                       ("b +inf", with_con(b=(0, INF))), ("du 0", with_con(du_max=(0, 0.0))), ("n_rows 0", with_con(n_rows=0)),
                       ("n_rows 8", with_con(n_rows=8))):
        assert L.mpcd_rollout_cost_constr(plan._ctx, *args, None) == 0, f"{what}: {err()}"
    torch.cuda.synchronize()
