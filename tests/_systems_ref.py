"""A reference of the rollout arithmetic that takes the DESCRIPTOR: the six dynamics, both cost kinds and the state-box
violation in plain Python floats (fp64), written from the packed layout documented in
mpc_via_diffusion_model_amd/systems.py and the dyn_step comments of csrc/rollout.hip - never from physical constants.

The C oracle (oracle/c/mpc_oracle.c) has the registry's constants compiled in, so it can check the kernels at
systems.get(name) only. This module restates the same expressions with the same association (Python evaluates left to
right in fp64 and never contracts), reading every constant from the descriptor: at the registry's descriptors it equals
the C oracle bit for bit (tests/test_systems_ref_host.py), and away from them it is the only reference there is.

No numpy in the arithmetic: numpy only draws the perturbed descriptors. sin / cos are arguments so that a test can move
every result by one ulp and measure what that does to a cost."""
import math
import zlib

import numpy as np

from mpc_via_diffusion_model_amd import _native as N
from mpc_via_diffusion_model_amd import systems

LIN5, NL5, ZOH4, DI2D, PEND, QUAD = (systems.CARTPOLE_LIN5, systems.CARTPOLE_NL5, systems.CARTPOLE_ZOH4,
                                     systems.DOUBLE_INT2D, systems.PENDULUM, systems.QUADROTOR12)
CANONICAL, CALMPC = N.MPCD_COST_CANONICAL, N.MPCD_COST_CALMPC

# The wrong variants of cost() the sensitivity test switches on, one at a time (tests/test_systems_ref_host.py). They
# exist to show that a perturbed descriptor sees a slip that the registry's constants hide; nothing else passes them.
WRONG = ("P_on_a_stage", "Q0_in_calmpc_stage_sum", "x_ref_dropped_on_last_component", "R0_for_every_input")


def step(system, params, x, u, sin=math.sin, cos=math.cos):
    """x_{k+1} = f(x_k, u_k): lists of floats in, a new list out. params is the packed descriptor array."""
    p = params
    if system == LIN5:
        # p: dt, -k*v2, (lm^2)*G*v2/il, lm*c*v2/il, v2, -l*m*k*v1/(M+m), lm*G*v1, c*v1, lm*v1/(M+m), 2/pi, pi
        xd = [x[1],
              p[1] * x[1] + p[2] * x[2] - p[3] * x[3] + p[4] * u[0],
              x[3],
              p[5] * x[1] + p[6] * x[2] - p[7] * x[3] + p[8] * u[0],
              -p[9] * (x[2] - p[10]) * x[3]]
        return [x[i] + xd[i] * p[0] for i in range(5)]
    if system == NL5:
        # p: dt, MPLP, MPG, M_TOTAL, M_POLE, MTG, MTLP, 2/pi, pi
        s, c = sin(x[2]), cos(x[2])
        dd = p[3] - p[4] * c
        xd = [x[1],
              (p[1] * -s * (x[3] * x[3]) + p[2] * s * c + u[0]) / (dd * dd),
              x[3],
              (-p[1] * s * c * (x[3] * x[3]) - p[5] * s - c * u[0]) / (p[6] - p[1] * (c * c)),
              -p[7] * (x[2] - p[8]) * x[3]]
        return [x[i] + xd[i] * p[0] for i in range(5)]
    if system == ZOH4:
        # p: A_d row-major [16], B_d [4]
        return [p[4 * i] * x[0] + p[4 * i + 1] * x[1] + p[4 * i + 2] * x[2] + p[4 * i + 3] * x[3] + p[16 + i] * u[0]
                for i in range(4)]
    if system == DI2D:
        # p: dt, 0.5*dt*dt
        return [x[0] + p[0] * x[2] + p[1] * u[0],
                x[1] + p[0] * x[3] + p[1] * u[1],
                x[2] + p[0] * u[0],
                x[3] + p[0] * u[1]]
    if system == PEND:
        # p: dt, g/l, damping, 1/(m l^2)
        return [x[0] + p[0] * x[1],
                x[1] + p[0] * (-p[1] * sin(x[0]) - p[2] * x[1] + p[3] * u[0])]
    if system == QUAD:
        # p: dt, m, g, Ix, Iy, Iz
        sph, cph, sth, cth = sin(x[3]), cos(x[3]), sin(x[4]), cos(x[4])
        sps, cps = sin(x[5]), cos(x[5])
        f_m = (p[1] * p[2] + u[0]) / p[1]
        xd = [x[6], x[7], x[8],
              x[9] + (x[10] * sph + x[11] * cph) * (sth / cth),
              x[10] * cph - x[11] * sph,
              (x[10] * sph + x[11] * cph) / cth,
              f_m * (cph * sth * cps + sph * sps),
              f_m * (cph * sth * sps - sph * cps),
              f_m * (cph * cth) - p[2],
              ((p[4] - p[5]) * x[10] * x[11] + u[1]) / p[3],
              ((p[5] - p[3]) * x[9] * x[11] + u[2]) / p[4],
              ((p[3] - p[4]) * x[9] * x[10] + u[3]) / p[5]]
        return [x[i] + p[0] * xd[i] for i in range(12)]
    raise ValueError(f"system {system}")


def _quad(w, x, ref, n):
    s = 0.0
    for j in range(n):
        e = x[j] - ref[j]
        s = s + w[j] * (e * e)
    return s


def unpack(desc):
    """(system, cost_kind, n_x, n_u, params, Q, R, P, x_ref) as plain Python values from a systems.System or from the
    mpcd_system_desc it packs (ctypes): only entries below n_x / n_u of the weights and the set-point are read."""
    nx, nu = int(desc.n_x), int(desc.n_u)
    x_ref = list(desc.x_ref) if len(desc.x_ref) else [0.0] * nx
    f = lambda a, n: [float(a[i]) for i in range(n)]  # noqa: E731
    return (int(desc.system), int(desc.cost_kind), nx, nu, [float(v) for v in desc.params], f(desc.Q, nx), f(desc.R, nu),
            f(desc.P, nx), f(x_ref, nx))


def cost(desc, x0, u, sin=math.sin, cos=math.cos, wrong=None):
    """(J, visited_states) of one plan u [H][n_u] (unnormalised floats) from x0 [n_x]. visited_states lists every state
    step() produces inside the evaluation: canonical x_1 .. x_H; calMPCCost x_1 .. x_{H-2} (its loop applies u_0 ..
    u_{H-3}), and calMPCCost ignores x_ref. wrong: one of WRONG, the sensitivity test's deliberate slips."""
    assert wrong is None or wrong in WRONG
    system, kind, nx, nu, p, Q, R, P, ref = unpack(desc)
    H = len(u)
    x = [float(v) for v in x0]
    visited = []
    if kind == CALMPC:
        assert nu == 1 and H >= 3
        stage_w = P if wrong == "P_on_a_stage" else Q
        first = 0 if wrong == "Q0_in_calmpc_stage_sum" else 1
        J = 0.0
        for i in range(nx):
            J = J + Q[i] * (x[i] * x[i])
        J = J + R[0] * (u[0][0] * u[0][0])
        xn = list(x)
        ucur = u[0][0]
        for i in range(1, H - 1):
            xn = step(system, p, x, [ucur], sin, cos)
            visited.append(xn)
            un = u[i][0]
            for j in range(first, nx):
                J = J + stage_w[j] * (xn[j] * xn[j])
            J = J + R[0] * (un * un)
            ucur = un
            x = xn
        for i in range(nx):
            J = J + P[i] * (xn[i] * xn[i])
        return J, visited
    assert H >= 2
    if wrong == "x_ref_dropped_on_last_component":
        ref = ref[:-1] + [0.0]
    Rw = [R[0]] * nu if wrong == "R0_for_every_input" else R
    zero = [0.0] * nu
    J = _quad(Q, x, ref, nx)
    for k in range(H):
        uk = [float(v) for v in u[k]]
        xn = step(system, p, x, uk, sin, cos)
        visited.append(xn)
        sx = _quad(P if (k == H - 1 or wrong == "P_on_a_stage") else Q, xn, ref, nx)
        su = _quad(Rw, uk, zero, nu)
        J = J + (sx + su)
        x = xn
    return J, visited


def violation(visited, lo, hi):
    """mpcd.h's V of one plan: max(0, max over the visited states x and i < n_x of max(lo[i] - x[i], x[i] - hi[i])); an
    excess with a NaN difference makes V +inf."""
    V = 0.0
    for x in visited:
        for i in range(len(x)):
            a, b = lo[i] - x[i], x[i] - hi[i]
            if a != a or b != b:
                return math.inf
            V = max(V, a, b)
    return V


def costs(desc, x0, U, sin=math.sin, cos=math.cos, wrong=None):
    """cost() over the plans U [B][H][n_u] (anything .tolist() or nested lists): ([J] * B, [visited] * B)"""
    U = U.tolist() if hasattr(U, "tolist") else U
    x0 = x0.tolist() if hasattr(x0, "tolist") else x0
    out = [cost(desc, x0, u, sin, cos, wrong) for u in U]
    return [o[0] for o in out], [o[1] for o in out]


def ulp_shifted(fn, direction):
    """fn with every result moved one ulp towards direction (+-inf): the sensitivity probe of the 1e-9 bar"""
    return lambda v: math.nextafter(fn(v), direction)


def _rebuilt(base, **kw):
    f = dict(name=base.name, system=base.system, cost_kind=base.cost_kind, n_x=base.n_x, n_u=base.n_u,
             params=list(base.params), Q=list(base.Q), R=list(base.R), P=list(base.P), x_ref=list(base.x_ref or []),
             reference=base.reference)
    f.update(kw)
    return systems.System(**f)


def with_cost_kind(base, cost_kind):
    return _rebuilt(base, cost_kind=int(cost_kind))


def with_params_swapped(base, i, j):
    p = list(base.params)
    p[i], p[j] = p[j], p[i]
    return _rebuilt(base, params=p)


def perturbed(name, seed, cost_kind=None):
    """A seeded non-degenerate descriptor of system `name` (a systems.System): every params entry is its default times
    an independent factor in [0.7, 1.3] (cartpole_zoh4: each A_d / B_d entry plus a uniform draw in +-0.01, which also
    fills its structural zeros), every Q, R, P entry a distinct non-zero value (a non-zero default times such a factor, a
    zero default drawn from [0.5, 1.5]), every x_ref component its default plus a draw of magnitude in [0.05, 0.25]. So
    equal defaults become distinct, the three quadrotor inertias are pairwise distinct (all three gyroscopic terms
    live), no weight multiplies a term away and the set-point is non-zero everywhere. cost_kind overrides the
    registry's pairing."""
    base = systems.get(name)
    rng = np.random.default_rng([base.system, int(seed), 20240])
    factor = lambda: float(rng.uniform(0.7, 1.3))  # noqa: E731
    if name == "cartpole_zoh4":
        params = [v + float(rng.uniform(-0.01, 0.01)) for v in base.params]
    else:
        params = [v * factor() for v in base.params]
    weight = lambda v: v * factor() if v != 0.0 else float(rng.uniform(0.5, 1.5))  # noqa: E731
    Q = [weight(v) for v in base.Q]
    R = [weight(v) for v in base.R]
    P = [weight(v) for v in base.P]
    ref0 = base.x_ref or [0.0] * base.n_x
    x_ref = [v + float(rng.choice((-1.0, 1.0)) * rng.uniform(0.05, 0.25)) for v in ref0]
    every = Q + R + P
    assert len(set(every)) == len(every) and all(v != 0.0 for v in every), "weights must be distinct and non-zero"
    assert all(v != 0.0 for v in x_ref) and all(v != 0.0 for v in params)
    if name == "quadrotor12":
        assert len({params[3], params[4], params[5]}) == 3
    return systems.System(base.name, base.system, base.cost_kind if cost_kind is None else int(cost_kind), base.n_x,
                          base.n_u, params, Q, R, P, x_ref=x_ref, reference=f"perturbed({name!r}, {seed})")


# ---- The descriptors, shapes and inputs the descriptor tests share (tests/test_gpu_system_descriptors.py runs them on
# the GPU, tests/test_systems_ref_host.py checks the one-ulp condition of the 1e-9 bar on exactly these draws).
SEEDS = (1, 2, 3)
TRANSCENDENTAL = ("cartpole_nl5", "pendulum", "quadrotor12")  # sin / cos: rtol 1e-9; the others: bit equality
SPREADS = (0.9, 1.3)  # 1.3: the global clip rule is live
B, M_GROUPS = 70, 2   # one full 64-candidate workgroup and one of 6; grouped: two states of 35 candidates

CASES = {f"{name}-s{seed}": (lambda name=name, seed=seed: perturbed(name, seed))
         for name in sorted(systems.REGISTRY) for seed in SEEDS}
# the pairings check_system accepts and the registry never makes
CASES.update({f"{name}-calmpc": (lambda name=name: perturbed(name, 1, cost_kind=CALMPC))
              for name in ("cartpole_nl5", "cartpole_zoh4", "pendulum")})
CASES["cartpole_lin5-canonical"] = lambda: perturbed("cartpole_lin5", 1, cost_kind=CANONICAL)
# the factories' arguments, which no other test passes
CASES["double_int2d-dt0.07"] = lambda: systems.double_int2d(dt=0.07)
CASES["pendulum-dt0.03"] = lambda: systems.pendulum(dt=0.03)
CASES["quadrotor12-dt0.013"] = lambda: systems.quadrotor12(dt=0.013)


# the two descriptors the one-call tails' tests run beside the registry's: every gyroscopic term live under the
# canonical cost with a set-point, and the nonlinear cart-pole under the cost kind the registry never pairs it with
TAIL_DESCRIPTORS = {"quadrotor12": lambda: perturbed("quadrotor12", 1),
                    "cartpole_nl5_calmpc": lambda: perturbed("cartpole_nl5", 1, cost_kind=CALMPC)}


def horizons(sysd):
    """the smallest horizon each cost kind accepts (calMPCCost: its loop body runs once), odd rows, the usual one"""
    return (3, 7, 32) if sysd.cost_kind == CALMPC else (2, 3, 7, 32)


def start_state(name, n_x, rng):
    """tests/test_gpu_rollout.py's start states: the 5-state cart-poles near upright with a consistent fifth state"""
    x = rng.uniform(-1, 1, n_x)
    if name.startswith("cartpole") and n_x == 5:
        x[2] = 0.9 * np.pi + 0.1 * x[2]
        x[4] = (x[2] - np.pi) ** 2 / -np.pi + np.pi
    return x


# The quadrotor's Euler-angle kinematics divide by cos(theta), and at H = 32 these plans spin it past theta = pi / 2:
# a draw in which some step lands within ~1e-3 of the singularity amplifies one ulp of a cos by 1 / cos^2 and fails the
# one-ulp condition of the 1e-9 bar (test_systems_ref_host.py asserts it; the two first draws replaced here moved their
# costs by 8.6e-9 and 5.3e-4). Such a draw is replaced by the next one, never the bar widened: (case, H) -> which draw
# is used, 0 where not listed.
REDRAW = {("quadrotor12-s2", 32): 1, ("quadrotor12-s3", 32): 1}


def case_inputs(case, H):
    """(sysd, x0 [2, n_x] fp64, {spread: u_norm [B, H, n_u] fp32}): seeded by the case's name and H"""
    sysd = CASES[case]()
    rng = np.random.default_rng([zlib.crc32(case.encode()), H, REDRAW.get((case, H), 0)])
    x0 = np.stack([start_state(sysd.name, sysd.n_x, rng) for _ in range(M_GROUPS)])
    u_norm = {s: rng.uniform(-s, s, (B, H, sysd.n_u)).astype(np.float32) for s in SPREADS}
    return sysd, x0, u_norm


def unnormalize(u_norm, lo, hi, clip):
    """fp32 LimitsNormalizer.unnormalize under a given clip decision, promoted exactly to fp64 (numpy fp32: the
    kernel's unnorm1 is the same three fp32 operations)"""
    x = np.asarray(u_norm, dtype=np.float32)
    if clip:
        x = np.clip(x, np.float32(-1), np.float32(1))
    h = (x + np.float32(1)) / np.float32(2)
    return (h * (np.float32(hi) - np.float32(lo)) + np.float32(lo)).astype(np.float64)


def clips(u_norm):
    """LimitsNormalizer's global test over these values (no NaN among them)"""
    return bool(u_norm.max() > np.float32(1 + 1e-4) or u_norm.min() < np.float32(-1 - 1e-4))


def case_plans(case, H, lo, hi):
    """The unnormalised plans of a case, as the calls under test see them:
    single[spread] = (x0[0], u [B, H, n_u]) - one start state, the global clip rule over all B candidates;
    grouped = [(x0[0], u of the first 35 candidates at spread 0.9), (x0[1], u of the last 35 at spread 1.3)] - each
    state with its own clip decision (off, on)."""
    sysd, x0, u_norm = case_inputs(case, H)
    n = B // M_GROUPS
    single = {s: (x0[0], unnormalize(u_norm[s], lo, hi, clips(u_norm[s]))) for s in SPREADS}
    parts = (u_norm[SPREADS[0]][:n], u_norm[SPREADS[1]][n:])
    assert [clips(p) for p in parts] == [False, True], "the grouped case needs one state in range and one clipped"
    grouped = [(x0[m], unnormalize(parts[m], lo, hi, clips(parts[m]))) for m in range(M_GROUPS)]
    return sysd, x0, u_norm, parts, single, grouped
