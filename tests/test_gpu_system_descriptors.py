"""GPU: the rollout, cost, box violation and plant step at descriptors that are NOT the registry's.

mpcd_system_desc is a public input, and every rollout kernel computes through dyn_step / candidate_cost with whatever it
holds; the C oracle has the registry's constants compiled in, and those are degenerate exactly where an operand or index
slip would hide (equal inertias, m = 1, P == Q, Q[2] == 0, a zero set-point, equal weights). Here the reference is
tests/_systems_ref.py - plain Python fp64 on the packed descriptor, equal to the C oracle bit for bit at the registry
(tests/test_systems_ref_host.py) - and the descriptors are its perturbed() ones: every constant distinct and non-zero,
a set-point that is non-zero everywhere, plus the cost-kind pairings check_system accepts and the registry never makes,
and the factories' dt arguments.

Shapes: B = 70 candidates (one full 64-candidate workgroup and one of 6), grouped as two plant states of 35 with their
own start states and clip flags (off, on); H = 2 (canonical only), 3 (calMPCCost's loop body runs once), 7 and 32.
Bars: bit equality for the systems without sin / cos; tests/test_gpu_rollout.py's rtol 1e-9 for the others, whose
condition (one ulp of sin / cos moves these very costs by < 1e-10) the host test asserts on the same draws."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec
from mpc_via_diffusion_model_amd import _native as N

from . import _systems_ref as R
from ._util import make_mlp
from .test_gpu_rollout import RTOL, _limits, _planner
from .test_gpu_state_box import BOX_COMPONENTS, STATE_BAR, _box

pytestmark = pytest.mark.gpu

ALL_CASES = sorted(R.CASES)
M, GROUP = R.M_GROUPS, R.B // R.M_GROUPS


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _log(line):
    """the figures of a run, appended to the file $MPCD_DESCRIPTOR_LOG names (profiles/system_descriptors.txt is made
    from one such run)"""
    path = os.environ.get("MPCD_DESCRIPTOR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def _plan(d, lo, hi):
    return _planner(d=d, C=2, lo=lo, hi=hi)  # the cost calls take H from the samples


def _exact(sysd):
    return sysd.name not in R.TRANSCENDENTAL


@functools.lru_cache(maxsize=None)
def _reference(case, H):
    """The case's inputs and everything the reference says about them, computed once, shared and left unchanged:
    single[spread] = costs [B] of all B candidates from x0[0] under the global clip rule; J [M, GROUP] and visited
    (the states each grouped plan's cost evaluation produces) of the grouped layout."""
    lo, hi = _limits(R.CASES[case]().name)
    sysd, x0, u_norm, parts, single, grouped = R.case_plans(case, H, lo, hi)
    ref = types.SimpleNamespace(sysd=sysd, x0=x0, u_norm=u_norm, parts=np.stack(parts), lo=lo, hi=hi,
                                single={s: np.array(R.costs(sysd, x, u)[0]) for s, (x, u) in single.items()},
                                u=np.stack([u for _, u in grouped]))
    out = [R.costs(sysd, x, u) for x, u in grouped]
    ref.J = np.array([o[0] for o in out])
    ref.visited = [o[1] for o in out]  # [M][GROUP][n_visited][n_x]
    for a in (ref.x0, ref.parts, ref.u, ref.J, *ref.single.values(), *ref.u_norm.values()):
        a.setflags(write=False)
    assert np.isfinite(ref.J).all() and all(np.isfinite(j).all() for j in ref.single.values())
    return ref


def _assert_cost(sysd, got, want, what):
    err = float((np.abs(got - want) / np.abs(want)).max())
    equal = bool((got.view(np.int64) == want.view(np.int64)).all())
    print(f"\n{what}: worst relative cost error {err:.3e}{' (bit-equal)' if equal else ''}")
    _log(f"cost\t{sysd.name}\t{sysd.cost_kind}\t{what}\t{err:.3e}\t{int(equal)}")
    if _exact(sysd):
        np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64), err_msg=what)
    else:
        np.testing.assert_allclose(got, want, rtol=RTOL[sysd.name], atol=0, err_msg=what)


def _grouped_on_device(plan, desc, ref, H):
    """mpcd_clip_flags + mpcd_rollout_cost_grouped on the grouped layout: (u_dev, x_dev, flags, cost), device tensors"""
    d = ref.sysd.n_u
    u_dev = torch.from_numpy(ref.parts.reshape(M * GROUP, H, d).copy()).cuda()
    x_dev = torch.from_numpy(ref.x0.copy()).cuda()
    flags = torch.empty(M, dtype=torch.int32, device="cuda")
    cost = torch.empty(M * GROUP, dtype=torch.float64, device="cuda")
    N.check(plan._lib.mpcd_clip_flags(plan._ctx, _ptr(u_dev), M, GROUP * H * d, _ptr(flags), plan._stream()),
            "mpcd_clip_flags")
    N.check(plan._lib.mpcd_rollout_cost_grouped(plan._ctx, ctypes.byref(desc), _ptr(x_dev), GROUP, _ptr(u_dev),
                                                plan.act_min.ctypes.data, plan.act_max.ctypes.data, M * GROUP, H,
                                                _ptr(flags), _ptr(cost), plan._stream()), "mpcd_rollout_cost_grouped")
    return u_dev, x_dev, flags, cost


def _control_step(plan, desc, x_dev, u_dev, H, cost, flags, select_first, decimals):
    """mpcd_control_step on a copy of x_dev: (x_next [M, n_x], u_applied [M, n_u], best_index [M], best_cost [M])"""
    x = x_dev.clone()
    u_out = torch.empty((M, desc.n_u), dtype=torch.float64, device="cuda")
    i_out = torch.empty(M, dtype=torch.int64, device="cuda")
    c_out = torch.empty(M, dtype=torch.float64, device="cuda")
    N.check(plan._lib.mpcd_control_step(plan._ctx, ctypes.byref(desc), _ptr(x), M, GROUP, _ptr(u_dev), H, _ptr(cost),
                                        plan.act_min.ctypes.data, plan.act_max.ctypes.data, _ptr(flags), select_first,
                                        decimals, _ptr(u_out), _ptr(i_out), _ptr(c_out), plan._stream()),
            "mpcd_control_step")
    return x, u_out, i_out, c_out


# ---- 1. rollout cost: host start state, and grouped

@pytest.mark.parametrize("case", ALL_CASES)
def test_rollout_cost_matches_the_descriptor_reference(case):
    sysd = R.CASES[case]()
    plan = _plan(sysd.n_u, *_limits(sysd.name))
    for H in R.horizons(sysd):
        ref = _reference(case, H)
        for spread in R.SPREADS:  # mpcd_rollout_cost: x0 on the host, the global clip rule computed by the call
            got = plan.rollout_cost(sysd, ref.x0[0], torch.from_numpy(ref.u_norm[spread].copy()).cuda()).cpu().numpy()
            _assert_cost(sysd, got, ref.single[spread], f"{case} H {H} spread {spread} host x0")
        _, _, flags, cost = _grouped_on_device(plan, sysd.desc(), ref, H)
        assert flags.cpu().tolist() == [0, 1]
        _assert_cost(sysd, cost.cpu().numpy(), ref.J.reshape(-1), f"{case} H {H} grouped")


# ---- 2. the box rollout: the grouped cost's bits, V against the reference's visited states

def _cut_box(case, H):
    """A box that cuts through the case's reference trajectories: symmetric bounds on two components at the median,
    over the 70 plans, of the largest magnitude each plan reaches there (the midpoint of two neighbouring distinct
    values, so no reference state lies on a bound). Where the two components' excursions are opposed and no plan stays
    inside both medians, the bounds move up a decile at a time until one does. Returns (box, V_ref [70], the state
    scale max(1, max |x|) per plan); both classes, V > 0 and V == 0, are present."""
    ref = _reference(case, H)
    n_x = ref.sysd.n_x
    xs = np.array(ref.visited).reshape(M * GROUP, -1, n_x)
    reach = {i: np.unique(np.abs(xs[:, :, i]).max(axis=1)) for i in BOX_COMPONENTS[ref.sysd.name]}
    for tenths in range(5, 11):
        bounds = {}
        for i, v in reach.items():
            r = min(len(v) - 1, max(1, len(v) * tenths // 10))
            bounds[i] = 0.5 * (v[r - 1] + v[r])
        box, lo, hi = _box(n_x, {i: (-b, b) for i, b in bounds.items()})
        want = np.array([R.violation(v, lo.tolist(), hi.tolist()) for vm in ref.visited for v in vm])
        if (want == 0).any():
            break
    scale = np.maximum(1.0, np.abs(xs).reshape(M * GROUP, -1).max(axis=1))
    with np.errstate(invalid="ignore"):
        margin = np.minimum(np.abs(xs - lo), np.abs(xs - hi))
    assert np.nanmin(np.where(np.isfinite(margin), margin, np.nan)) > STATE_BAR * scale.max(), \
        "the reference puts a state on a bound: move the bound"
    assert (want > 0).any() and (want == 0).any(), "the case must hold both classes"
    return box, want, scale


@pytest.mark.parametrize("case", ALL_CASES)
def test_box_rollout_matches_the_descriptor_reference(case):
    sysd = R.CASES[case]()
    plan = _plan(sysd.n_u, *_limits(sysd.name))
    for H in R.horizons(sysd):
        ref = _reference(case, H)
        box, want, scale = _cut_box(case, H)
        u_dev, x_dev, flags, free = _grouped_on_device(plan, sysd.desc(), ref, H)
        cost, viol = plan.rollout_cost_box(sysd, x_dev, u_dev, box, group=GROUP, clip_flags=flags)
        assert _bytes(cost) == _bytes(free), "the cost is not the grouped rollout's, bit for bit"
        got = viol.cpu().numpy()
        err = np.abs(got - want) / scale
        equal = bool((got.view(np.int64) == want.view(np.int64)).all())
        print(f"\n{case} H {H}: {(want > 0).sum()} of {M * GROUP} violate, max |V - V_ref| / max(1, |x|) = {err.max():.3e}"
              f"{' (bit-equal)' if equal else ''}")
        _log(f"viol\t{sysd.name}\t{sysd.cost_kind}\t{case} H {H}\t{err.max():.3e}\t{int(equal)}")
        if _exact(sysd):
            np.testing.assert_array_equal(got, want)
        else:
            assert (err <= STATE_BAR).all(), f"worst violation error {err.max():.3e} of the state scale"
        assert ((got == 0) == (want == 0)).all(), "feasibility differs from the reference"


# ---- 3. the control step: selection, the applied action, the plant step

@pytest.mark.parametrize("case", ALL_CASES)
def test_control_step_matches_the_descriptor_reference(case):
    """u_applied is the fp32 unnormalise of the pick's first action under its state's clip decision, promoted to fp64
    and rounded rint(o * 10^d) / 10^d (d < 0: as it is): no transcendental, so it is compared on bits for every system.
    x_dev is the reference's step() on that action from the state: bits, or rtol 1e-9 with sin / cos."""
    sysd = R.CASES[case]()
    plan = _plan(sysd.n_u, *_limits(sysd.name))
    desc = sysd.desc()
    for H in R.horizons(sysd):
        ref = _reference(case, H)
        u_dev, x_dev, flags, cost = _grouped_on_device(plan, desc, ref, H)
        c = cost.cpu().numpy().reshape(M, GROUP)
        for select_first in (0, 1):
            for decimals in (-1, 4):
                x, u_app, idx, best = (t.cpu().numpy() for t in _control_step(plan, desc, x_dev, u_dev, H, cost, flags,
                                                                              select_first, decimals))
                what = f"{case} H {H} select_first {select_first} decimals {decimals}"
                pick = np.zeros(M, dtype=np.int64) if select_first else c.argmin(axis=1)  # the lowest index on ties
                np.testing.assert_array_equal(idx, np.arange(M) * GROUP + pick, err_msg=what)
                np.testing.assert_array_equal(best.view(np.int64), c[np.arange(M), pick].view(np.int64), err_msg=what)
                o = ref.u[np.arange(M), pick, 0]  # [M, n_u]: fp32 unnormalised, exactly promoted
                if decimals >= 0:
                    sc = 10.0 ** decimals
                    o = np.rint(o * sc) / sc
                np.testing.assert_array_equal(u_app.view(np.int64), o.view(np.int64), err_msg=f"{what}: u_applied")
                want = np.array([R.step(sysd.system, sysd.params, ref.x0[m].tolist(), o[m].tolist()) for m in range(M)])
                err = float((np.abs(x - want) / np.abs(want)).max())
                equal = bool((x.view(np.int64) == want.view(np.int64)).all())
                _log(f"step\t{sysd.name}\t{sysd.cost_kind}\t{what}\t{err:.3e}\t{int(equal)}")
                if _exact(sysd):
                    np.testing.assert_array_equal(x.view(np.int64), want.view(np.int64), err_msg=f"{what}: x_dev")
                else:
                    np.testing.assert_allclose(x, want, rtol=RTOL[sysd.name], atol=0, err_msg=f"{what}: x_dev")


# ---- 4. the fields mpcd.h says are ignored

def _every_output(plan, desc, ref, H, box):
    """the output bytes of every rollout entry point under one descriptor"""
    raw = types.SimpleNamespace(name=ref.sysd.name, n_x=ref.sysd.n_x, n_u=ref.sysd.n_u, desc=lambda: desc)
    out = [_bytes(plan.rollout_cost(raw, ref.x0[0], torch.from_numpy(ref.u_norm[s].copy()).cuda())) for s in R.SPREADS]
    u_dev, x_dev, flags, cost = _grouped_on_device(plan, desc, ref, H)
    out.append(_bytes(cost))
    out += [_bytes(t) for t in plan.rollout_cost_box(raw, x_dev, u_dev, box, group=GROUP, clip_flags=flags)]
    for select_first in (0, 1):
        out += [_bytes(t) for t in _control_step(plan, desc, x_dev, u_dev, H, cost, flags, select_first, 4)]
    return out


@pytest.mark.parametrize("case", ALL_CASES)
def test_ignored_descriptor_fields_change_no_output_byte(case):
    """mpcd.h on mpcd_system_desc: entries of Q, P, x_ref at index >= n_x and of R at index >= n_u are never read, and
    MPCD_COST_CALMPC never reads x_ref. Each rule: two calls of every entry point, their output bytes compared; the
    ignored entries are set to NaN, which no arithmetic would hide. And the converse, so that the comparison is known
    to reach the kernels: under the canonical cost x_ref[n_x - 1] does change the costs."""
    sysd = R.CASES[case]()
    plan = _plan(sysd.n_u, *_limits(sysd.name))
    H = 7
    ref = _reference(case, H)
    bound = float(np.median(np.abs(np.array(ref.visited)[..., 0])))
    box = _box(sysd.n_x, {0: (-bound, bound)})[0]
    base = _every_output(plan, sysd.desc(), ref, H, box)
    padded = sysd.desc()
    for i in range(sysd.n_x, 12):
        padded.Q[i] = padded.P[i] = padded.x_ref[i] = float("nan")
    for i in range(sysd.n_u, 4):
        padded.R[i] = float("nan")
    assert _every_output(plan, padded, ref, H, box) == base, "an entry past n_x / n_u is read"
    moved = sysd.desc()
    for i in range(sysd.n_x):
        moved.x_ref[i] = sysd.x_ref[i] + 0.5 if sysd.x_ref else 0.5
    other = _every_output(plan, moved, ref, H, box)
    if sysd.cost_kind == R.CALMPC:
        assert other == base, "calMPCCost read x_ref"
    else:
        last = sysd.desc()
        last.x_ref[sysd.n_x - 1] += 0.5
        assert _every_output(plan, last, ref, H, box)[2] != base[2], "x_ref[n_x - 1] does not reach the canonical cost"
        assert other[2] != base[2]


# ---- 5. one planner, three descriptors in turn

def test_planner_reuse_across_descriptors():
    """DiffusionMPC._system_desc keeps the packed descriptor of the last system and rebuilds it when a field changes.
    One planner is called with A, with B (A but for x_ref[n_x - 1]) and with C (A but for R[n_u - 1]), through both
    callers of the cache (the one-call step and the batched external step): each result is its own descriptor's."""
    d, H, C, n = 2, 32, 4, 100
    net = make_mlp(d, H, C, seed=5)
    lo, hi = np.array([-2.0, -0.5]), np.array([2.0, 0.5])
    plan = DiffusionMPC(NetSpec("mlp", d, H, C), net.state_dict(), n_diffusion_steps=25, action_limits=(lo, hi))
    A = R.perturbed("double_int2d", 1)
    B_ = R.perturbed("double_int2d", 1)
    B_.x_ref[-1] += 0.25
    C_ = R.perturbed("double_int2d", 1)
    C_.R[-1] *= 1.5
    x0 = np.array([0.4, -0.3, 0.2, -0.1])
    seen = []
    for sysd in (A, B_, C_, A):
        r = plan.mpc_step(x0, sysd, n, seed=7, native=True)
        u = R.unnormalize(r.u_norm.cpu().numpy(), lo, hi, bool(r.flags & N.MPCD_STEP_CLIPPED))
        want = np.array(R.costs(sysd, x0, u)[0])
        np.testing.assert_array_equal(r.costs.cpu().numpy().view(np.int64), want.view(np.int64))
        assert (r.best_index, r.best_cost) == (int(want.argmin()), float(want.min()))
        rb = plan.mpc_step_batch(x0[None], sysd, n, seed=7, return_samples=True)
        ub = R.unnormalize(rb.u_norm.cpu().numpy(), lo, hi, bool(rb.flags[0] & N.MPCD_STEP_CLIPPED))
        wb = np.array(R.costs(sysd, x0, ub)[0])
        assert (int(rb.index[0]), float(rb.cost[0])) == (int(wb.argmin()), float(wb.min()))
        seen.append(want)
    assert (seen[0] != seen[1]).all() and (seen[0] != seen[2]).all(), "the three descriptors must cost differently"
    np.testing.assert_array_equal(seen[0], seen[3])
