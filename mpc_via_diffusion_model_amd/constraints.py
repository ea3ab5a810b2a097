"""Feasibility-first selection, the Python side: the public Constraints, the state-box builder, and
Feasibility - the one object a planner call carries for "who produces the violation V": a state box (the
mpcd_*_box entry points) or a constraint set (the mpcd_*_constr ones)."""
import copy
import ctypes

import numpy as np
import torch

from . import _native as N

# refusal texts shared by the callers of feasibility(), by producer
NEEDS_ARGMIN = {"state_box": "state_box ranks candidates feasibility-first: it needs select='argmin'",
                "constraints": "constraints rank candidates feasibility-first: they need select='argmin'"}


def _p(t):
    """the device (or host) address of a tensor as a ctypes pointer argument; None stays None (NULL)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def state_box_of(box, n_x):
    """(lo, hi) with None = unbounded (the whole side, or single entries) -> the mpcd_state_box of an n_x system"""
    try:
        lo, hi = box
    except (TypeError, ValueError):
        raise ValueError("state_box must be a pair (lo, hi) of per-component bounds, None = unbounded") from None
    out = N.StateBox()
    for side, fill, dst in ((lo, -np.inf, out.lo), (hi, np.inf, out.hi)):
        vals = [None] * n_x if side is None else list(side)
        if len(vals) != n_x:
            raise ValueError(f"state_box bounds must have n_x = {n_x} entries each, got {len(vals)}")
        for i in range(12):
            dst[i] = fill if i >= n_x or vals[i] is None else float(vals[i])
    for i in range(n_x):
        if np.isnan(out.lo[i]) or np.isnan(out.hi[i]) or out.lo[i] > out.hi[i]:
            raise ValueError(f"state_box component {i}: [{out.lo[i]}, {out.hi[i]}] is not an interval")
    return out


def _viol_tol(viol_tol):
    tol = float(viol_tol)
    if not tol >= 0.0:
        raise ValueError(f"viol_tol = {viol_tol} must be >= 0")
    return tol


class Constraints:
    """A constraint set (mpcd.h "Constraint set"): a state box, up to 8 linear rows and per-input rate bounds.

    state_box: (lo, hi) as everywhere (None = unbounded: the whole box, a side, or single entries).
    rows: a sequence of (a, c, b) meaning sum_i a[i] x[i] + sum_j c[j] u[j] <= b on every visited pair (x_{k+1}, u_k):
    a has n_x entries, c has n_u entries or is None (zeros), b is a float (+inf switches the row off).
    du_max: n_u entries bounding |u_k[j] - u_{k-1}[j]| (None, or None entries = unbounded).
    The set is checked against a system when a call takes it; a ValueError names the entry."""

    def __init__(self, state_box=None, rows=(), du_max=None):
        self.state_box, self.rows, self.du_max = state_box, tuple(rows), du_max

    def native(self, n_x, n_u):
        """the mpcd_constraints of a system with n_x states and n_u inputs (checked)"""
        con = N.ConstraintSet()
        con.box = state_box_of((None, None) if self.state_box is None else self.state_box, n_x)
        if len(self.rows) > N.MPCD_MAX_CON_ROWS:
            raise ValueError(f"constraints: {len(self.rows)} rows, at most {N.MPCD_MAX_CON_ROWS}")
        con.n_rows = len(self.rows)
        for r in range(N.MPCD_MAX_CON_ROWS):
            con.b[r] = np.inf
        for r, row in enumerate(self.rows):
            try:
                a, c, b = row
                a = [float(v) for v in a]
                c = [0.0] * n_u if c is None else [float(v) for v in c]
                b = float(b)
            except (TypeError, ValueError):
                raise ValueError(f"constraints row {r}: must be (a [n_x], c [n_u] or None, b)") from None
            if len(a) != n_x or len(c) != n_u:
                raise ValueError(f"constraints row {r}: a has {len(a)} entries (n_x = {n_x}), c has {len(c)} (n_u = {n_u})")
            for what, vals, dst in (("a", a, con.A[r]), ("c", c, con.C[r])):
                for i, v in enumerate(vals):
                    if not np.isfinite(v):
                        raise ValueError(f"constraints row {r}: {what}[{i}] = {v} is not finite")
                    dst[i] = v
            if np.isnan(b) or b == -np.inf:
                raise ValueError(f"constraints row {r}: b = {b} (use +inf to switch a row off)")
            con.b[r] = b
        du = [None] * n_u if self.du_max is None else list(self.du_max)
        if len(du) != n_u:
            raise ValueError(f"constraints du_max must have n_u = {n_u} entries, got {len(du)}")
        for j in range(4):
            v = np.inf if j >= n_u or du[j] is None else float(du[j])
            if not v >= 0.0:
                raise ValueError(f"constraints du_max[{j}] = {v} must be >= 0 (None = unbounded)")
            con.du_max[j] = v
        return con


class Feasibility:
    """What a feasibility-first call carries (internal; built by feasibility()): kind "state_box" (native: an
    mpcd_state_box, the box kernels) or "constraints" (native: an mpcd_constraints, the set kernels), the tolerance,
    and the u_prev rows as the caller gave them or, where it asked for host rows, as a checked float64 array."""

    def __init__(self, kind, native, tol, u_prev=None):
        self.kind, self.native, self.tol, self.u_prev = kind, native, tol, u_prev

    def rollout(self, plan, desc, x, group, u_norm, flags, cost, viol, u_prev=None):
        """mpcd_rollout_cost_box / _constr on device buffers: cost and violation [B] of u_norm [B, H, d] from the states
        x [B / group, n_x] with their clip codes; u_prev: device float64 [B / group, n_u] or None (a set's rate test)"""
        B, H, _ = u_norm.shape
        head = (plan._ctx, ctypes.byref(desc), _p(x), group, _p(u_norm), plan.act_min.ctypes.data,
                plan.act_max.ctypes.data, B, H, _p(flags), ctypes.byref(self.native))
        if self.kind == "constraints":
            N.check(plan._lib.mpcd_rollout_cost_constr(*head, _p(u_prev), _p(cost), _p(viol), plan._stream()),
                    "mpcd_rollout_cost_constr")
        else:
            N.check(plan._lib.mpcd_rollout_cost_box(*head, _p(cost), _p(viol), plan._stream()), "mpcd_rollout_cost_box")

    def batch_block(self, M, elites):
        """The extra block of the batched one-call step: (entry point name, BatchBoxArgs / BatchConstrArgs, violation
        [M], n_feasible [M], elite violations [M, elites] or None) - the host arrays the block points to."""
        if self.kind == "constraints":
            name, bx = "mpcd_mpc_step_batch_constr", N.BatchConstrArgs()
            bx.con = ctypes.pointer(self.native)
            bx.u_prev_host = None if self.u_prev is None else self.u_prev.ctypes.data
        else:
            name, bx = "mpcd_mpc_step_batch_box", N.BatchBoxArgs()
            bx.box = ctypes.pointer(self.native)
        bx.tol = self.tol
        viol, nfeas = np.empty(M, dtype=np.float64), np.empty(M, dtype=np.int64)
        bx.viol_host, bx.n_feasible_host = viol.ctypes.data, nfeas.ctypes.data
        eviol = None if elites is None else np.empty((M, elites), dtype=np.float64)
        if eviol is not None:
            bx.elite_viol_host = eviol.ctypes.data
        return name, bx, viol, nfeas, eviol

    def restrict(self, idx):
        """the same spec for the states idx of a batch (the `reset` split): their u_prev rows"""
        if self.u_prev is None:
            return self
        sub = copy.copy(self)
        sub.u_prev = np.ascontiguousarray(self.u_prev[idx])
        return sub


def feasibility(system, state_box=None, constraints=None, viol_tol=0.0, u_prev=None, kind=None, refuse=(),
                u_prev_shape=None):
    """The Feasibility of a call that takes state_box= / constraints= / viol_tol= / u_prev=, or None when it takes
    neither. kind: None (by what is given) or the producer the calling method names, whose argument is then required.
    refuse: the caller's own refusals, (condition, {kind: text}) pairs raised in order before the spec is built.
    u_prev_shape: (n_u,) or (M, n_u) where the call hands u_prev to the library from the host - it is then checked and
    kept as a contiguous float64 array; None keeps what the caller gave."""
    if kind is None:
        if constraints is not None:
            if state_box is not None:
                raise ValueError("state_box together with constraints: put the box into the set, "
                                 "Constraints(state_box=...)")
            kind = "constraints"
        elif u_prev is not None:
            raise ValueError("u_prev serves the rate bounds of constraints=")
        elif state_box is None:
            return None
        else:
            kind = "state_box"
    for cond, texts in refuse:
        if cond:
            raise ValueError(texts[kind])
    if kind == "constraints":
        if not isinstance(constraints, Constraints):
            raise ValueError("constraints must be a Constraints(state_box=, rows=, du_max=)")
        native = constraints.native(system.n_x, system.n_u)
    else:
        native = state_box_of(state_box, system.n_x)
    tol = _viol_tol(viol_tol)
    if u_prev is not None and u_prev_shape is not None:
        up = u_prev.detach().cpu().numpy() if torch.is_tensor(u_prev) else u_prev
        up = np.ascontiguousarray(up, dtype=np.float64)
        u_prev = np.atleast_2d(up) if len(u_prev_shape) == 2 else up
        if u_prev.shape != tuple(u_prev_shape):
            raise ValueError(f"u_prev must be {list(u_prev_shape)}, got {u_prev.shape}")
    return Feasibility(kind, native, tol, u_prev)
