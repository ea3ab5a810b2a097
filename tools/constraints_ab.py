#!/usr/bin/env python3
"""What the constraint set costs, and that the paths beside it are the parent's: double_int2d, H = 32, an f32x3 MLP at
the cfg2 net shape (d = 2, C = 4, N = 100), one GPU, at 1 state x 4,096 candidates and 64 x 64.

Both builds (this one and, with --parent-lib, a libmpcd.so of the parent commit loaded through MPCD_LIB) run, in the
same sequence, the paths this change leaves alone: mpcd_rollout_cost_grouped and mpcd_rollout_cost_box on fixed samples
(us per launch: --launches launches between two HIP events), and the warm control step of mpc_step_batch,
mpc_step_batch(elites=k) and mpc_step_batch_box (ms per step, host clock from the host states to the host results,
tools/batch_box_ab.py's loop), at both shapes. A digest of every output must be the same for both builds. This build's
process then goes on to what only it has, with the box sibling timed again inside that block ("again": the figure the
differences are taken against):

  constr r{0,2,8}[+rate]   mpcd_rollout_cost_constr with the box of rollout_cost_box, 0, 2 or 8 rows (none ever binding:
                           the work is what is measured) and, +rate, finite rate bounds with a u_prev row per state
  step constr / +rows+rate mpc_step_batch_constr with the box alone, and with 2 rows, rate bounds and u_prev
  step composed            the same step composed by hand from the public calls (upload, mpcd_normalize_states, the
                           sampler, mpcd_clip_flags, mpcd_rollout_cost_constr, mpcd_topk_feasible,
                           mpcd_control_step_picked, mpcd_shift_plans, the downloads), checked to return the one call's
                           u, cost, index, V and n_feasible before any timing

Every round starts one fresh process per build; the build order flips from round to round. Reported: the median over the
rounds with their min / max.

    python tools/constraints_ab.py [--rounds 5] [--steps 20] [--launches 200] [--parent-lib FILE] [--json FILE]"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "CONSTRAINTS_AB "
NEW = ("mpcd_rollout_cost_constr", "mpcd_mpc_step_batch_constr")


def worker(a):
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import _native as N
    if a.worker == "parent":  # the parent's library has no such entry points to bind
        for name in NEW:
            N.EXPORTS.pop(name, None)
    from mpc_via_diffusion_model_amd import Constraints, DiffusionMPC, NetSpec, systems
    from mpc_via_diffusion_model_amd.constraints import Feasibility
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    H, d, C, NS, T, k, K = 32, 2, 4, 100, a.steps, 8, 10
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NS, context_limits=(-2 * np.ones(C), 2 * np.ones(C)))
    sysm = systems.double_int2d()
    desc = sysm.desc()
    dev, L, ctx = plan.device, plan._lib, plan._ctx
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    box_py = ([None, None, -0.6, -0.6], [None, None, 0.6, 0.6])
    tol = 0.0
    box_f = Feasibility("state_box", plan._state_box(box_py, 4), tol)
    this = a.worker == "this"
    digest = hashlib.sha256()
    res = {}

    def rows(n):  # rows that never bind: their cost is the arithmetic
        return [([0.1 * (r + 1), -0.2, 0.3, 0.05 * r], [0.25, -0.125], 1e6) for r in range(n)]

    # ---- the rollout kernels on fixed samples
    def rollout_case(M, n):
        g = torch.Generator().manual_seed(M)
        u_norm = (torch.rand(M * n, H, d, generator=g) * 2.2 - 1.1).to(dev)
        x = torch.from_numpy(np.random.default_rng(M).uniform(-1, 1, (M, 4))).to(dev)
        up = torch.from_numpy(np.random.default_rng(M + 1).uniform(-1, 1, (M, d))).to(dev)
        flags = torch.empty(M, dtype=torch.int32, device=dev)
        N.check(L.mpcd_clip_flags(ctx, ptr(u_norm), M, n * H * d, ptr(flags), plan._stream()), "mpcd_clip_flags")
        cost = torch.empty(M * n, dtype=torch.float64, device=dev)
        viol = torch.empty(M * n, dtype=torch.float64, device=dev)
        st = plan._stream()

        def grouped():
            N.check(L.mpcd_rollout_cost_grouped(ctx, ctypes.byref(desc), ptr(x), n, ptr(u_norm), plan.act_min.ctypes.data,
                                                plan.act_max.ctypes.data, M * n, H, ptr(flags), ptr(cost), st), "grouped")
        calls = {"rollout_cost_grouped": grouped,
                 "rollout_cost_box": lambda: box_f.rollout(plan, desc, x, n, u_norm, flags, cost, viol)}
        if this:
            for nr in (0, 2, 8):
                for rate in (False, True):
                    con = Constraints(box_py, rows(nr), [1.6, 1.7] if rate else None).native(4, 2)
                    con = Feasibility("constraints", con, tol)
                    calls[f"constr r{nr}" + ("+rate" if rate else "")] = (
                        lambda con=con, rate=rate: con.rollout(plan, desc, x, n, u_norm, flags, cost, viol,
                                                               up if rate else None))
        return calls, cost, viol

    def time_launches(fn):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.launches  # us

    # ---- the control steps
    def states(M):
        return np.random.default_rng(0).uniform(-1.0, 1.0, (T + 1, M, 4))

    def timed_loop(n_steps, step):
        t0 = 0.0
        for it in range(n_steps):
            if it == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            step(it)
        return (time.perf_counter() - t0) * 1e3 / (n_steps - 1)  # ms

    full = None
    if this:
        full = Constraints(box_py, rows(2), [1.6, 1.7])

    def run_batch(M, n, xs, kind):
        plan.reset_warm_start()
        out, prev = [], [None]

        def step(it):
            kw = dict(w=0.01, seed=1 + it, grouped=True, warm_start=K)
            if kind == "plain":
                r = plan.mpc_step_batch(xs[it], sysm, n, **kw)
            elif kind == "elite":
                r = plan.mpc_step_batch(xs[it], sysm, n, elites=k, **kw)
            elif kind == "box":
                r = plan.mpc_step_batch_box(xs[it], sysm, n, box_py, tol, **kw)
            elif kind == "constr":
                r = plan.mpc_step_batch_constr(xs[it], sysm, n, Constraints(box_py), tol, **kw)
            else:
                r = plan.mpc_step_batch_constr(xs[it], sysm, n, full, tol, prev[0], **kw)
                prev[0] = r.u
            out.append(r)
        return out, timed_loop(len(xs), step)

    def run_composed(M, n, xs):
        B, st = M * n, plan._stream()
        grouped = plan.grouped_pays(M, n)
        con = Feasibility("constraints", full.native(4, 2), tol)
        c = torch.empty((M, C), dtype=torch.float32, device=dev)
        flags = torch.empty(M, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        viol = torch.empty(B, dtype=torch.float64, device=dev)
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        absmax = torch.empty(B, dtype=torch.float32, device=dev)
        us = torch.empty((M, d), dtype=torch.float64, device=dev)
        cs = torch.empty(M, dtype=torch.float64, device=dev)
        ix = torch.empty(M, dtype=torch.int64, device=dev)
        priors = torch.empty((M, H, d), dtype=torch.float32, device=dev)
        out, prev = [], [None]

        def step(it):
            x = torch.from_numpy(xs[it]).to(dev)
            up = None if prev[0] is None else torch.from_numpy(prev[0]).to(dev)
            warm = {}
            if it > 0:
                warm = dict(x_init=priors if grouped else priors.repeat_interleave(n, dim=0), t_start=K)
            N.check(L.mpcd_normalize_states(ctx, ptr(x), M, C, plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data,
                                            ptr(c), st), "mpcd_normalize_states")
            plan.sample_trajectories(c if grouped else c.repeat_interleave(n, dim=0), B, H, 0.01, "ddpm_cfg", 0, None,
                                     False, 1 + it, 0, None, False, out=u_norm, absmax_out=absmax,
                                     context_group=n if grouped else None, **warm)
            N.check(L.mpcd_clip_flags(ctx, ptr(absmax), M, n, ptr(flags), st), "mpcd_clip_flags")
            con.rollout(plan, desc, x, n, u_norm, flags, cost, viol, up)
            raw, vk, nf = plan._topk_feasible_raw(cost, viol, 1, M, tol)
            plan._control_step_picked_raw(desc, x, u_norm, raw, 0, flags, 4, us, ix, cs)
            plan.shift_plans(u_norm, ix, 0, out=priors)
            prev[0] = us.cpu().numpy()
            out.append((prev[0], cs.cpu().numpy(), ix.cpu().numpy(), vk.cpu().numpy(), nf.cpu().numpy()))
        return out, timed_loop(len(xs), step)

    # both builds' processes run the same sequence first - the unchanged paths' outputs and their timing at every
    # shape - and this build's then goes on to what only it has; within a block the order flips from round to round
    shapes = [(1, 4096), (64, 64)]
    common_calls = ("rollout_cost_grouped", "rollout_cost_box")
    common_kinds = ["plain", "elite", "box"]
    flip = (lambda seq: list(seq)[::-1]) if a.reverse else list
    cases = {}
    for M, n in shapes:
        cfg = f"{M} x {n}"
        calls, cost, viol = cases[cfg] = rollout_case(M, n)
        for name in common_calls:
            calls[name]()
            torch.cuda.synchronize()
            digest.update(cost.cpu().numpy().tobytes())
            if name.endswith("box"):
                digest.update(viol.cpu().numpy().tobytes())
        for name in flip(common_calls):
            res[f"{cfg}|us|{name}"] = time_launches(calls[name])
        xs = states(M)
        for kind in common_kinds:  # the outputs first (this also warms the variants)
            for r in run_batch(M, n, xs, kind)[0]:
                fields = (r.u, r.plan, r.cost, r.index, r.flags)
                fields += (r.elite_index, r.elite_cost) if kind == "elite" else ()
                fields += (r.violation, r.n_feasible) if kind == "box" else ()
                for f in fields:
                    digest.update(np.ascontiguousarray(f).tobytes())
        for kind in flip(common_kinds):
            res[f"{cfg}|ms|step {kind}"] = run_batch(M, n, xs, kind)[1]
    for M, n in shapes if this else ():
        cfg = f"{M} x {n}"
        calls = cases[cfg][0]
        extra = [name for name in calls if name not in common_calls]
        for name in extra:
            calls[name]()
        for name in flip(extra + ["rollout_cost_box"]):  # the box sibling again, inside this block
            res[f"{cfg}|us|{name if name != 'rollout_cost_box' else 'rollout_cost_box (again)'}"] = time_launches(calls[name])
        xs = states(M)
        got, ref = run_batch(M, n, xs, "constr+rows+rate")[0], run_composed(M, n, xs)[0]
        for it, (g, r) in enumerate(zip(got, ref)):
            for f, w in zip(("u", "cost", "index", "violation", "n_feasible"), (r[0], r[1], r[2], r[3][:, 0], r[4])):
                np.testing.assert_array_equal(getattr(g, f), w, err_msg=f"{cfg} step {it}: {f}")
        res[f"{cfg}|live"] = float(np.mean([g.n_feasible.mean() / n for g in got]))
        for kind in flip(["box (again)", "constr", "constr+rows+rate"]):
            res[f"{cfg}|ms|step {kind}"] = run_batch(M, n, xs, kind.split(" ")[0])[1]
        res[f"{cfg}|ms|step composed"] = run_composed(M, n, xs)[1]
    print(TAG + json.dumps({"res": res, "digest": digest.hexdigest(), "device": torch.cuda.get_device_name(0)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed warm control steps per round")
    ap.add_argument("--launches", type=int, default=200, help="timed launches per rollout call and round")
    ap.add_argument("--parent-lib", default=None, help="libmpcd.so built from the parent commit")
    ap.add_argument("--reverse", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", default=None, choices=("this", "parent"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.worker:
        return worker(a)
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")

    def child(which, flip):
        env = dict(os.environ)
        if which == "parent":
            env["MPCD_LIB"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("MPCD_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--steps", str(a.steps), "--launches",
               str(a.launches)] + (["--reverse"] if flip else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"{which} worker failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(lines[-1][len(TAG):])

    builds = ["this"] + (["parent"] if a.parent_lib else [])
    times, digests, device, live = {}, {}, None, {}
    for rnd in range(a.rounds):
        flip = (rnd % 2 == 1) != a.reverse
        for which in (builds[::-1] if flip else builds):
            r = child(which, flip)
            device = r["device"]
            digests.setdefault(which, set()).add(r["digest"])
            for key, v in r["res"].items():
                cfg, unit, name = key.split("|") if key.count("|") == 2 else (key.split("|")[0], "live", "")
                if unit == "live":
                    live[cfg] = v
                else:
                    times.setdefault((cfg, unit), {}).setdefault(f"{which}: {name}", []).append(v)
    if any(len(dg) != 1 for dg in digests.values()) or len(set.union(*digests.values())) != 1:
        raise RuntimeError(f"the unchanged paths' outputs differ between runs or builds: {digests}")
    print(f"device {device}; {a.rounds} rounds, one fresh process per build and round; us: per launch over {a.launches} "
          f"launches between HIP events; ms: per warm control step (K = 10) over {a.steps} steps, host clock")
    print("rollout_cost_grouped, rollout_cost_box, mpc_step_batch, mpc_step_batch(elites=8) and mpc_step_batch_box outputs "
          + ("byte-identical on both builds" if a.parent_lib else "identical in every round")
          + f" (sha256 {next(iter(digests['this']))[:16]}...); step constr+rows+rate == step composed (u, cost, index, V, "
          "n_feasible) at every shape in every round")
    for cfg, frac in live.items():
        print(f"{cfg}: {100 * frac:.0f}% of the candidates feasible under the full set on average")
    out = {}
    for (cfg, unit), rows_ in times.items():
        print(f"\n[{cfg}, {unit}]\n{'build: path':34s} {'median':>10s} {'min':>10s} {'max':>10s}")
        st = {}
        for name, t in rows_.items():
            st[name] = {"median": statistics.median(t), "min": min(t), "max": max(t), "rounds": t}
        for name in sorted(st, key=lambda s: (s.split(": ")[1], s)):
            print(f"{name:34s} {st[name]['median']:10.3f} {st[name]['min']:10.3f} {st[name]['max']:10.3f}")
        out[f"{cfg} {unit}"] = st
        if a.parent_lib:
            for name in sorted(st):
                if name.startswith("parent: "):
                    p, q = st[name], st["this: " + name[8:]]
                    inside = p["min"] <= q["median"] <= p["max"]
                    print(f"{name[8:]}: this build's median {'inside' if inside else 'OUTSIDE'} the parent's min-max")
        ref = st.get("this: rollout_cost_box (again)") if unit == "us" else st.get("this: step box (again)")
        for name in sorted(st):
            if name.startswith("this: constr") or name.startswith("this: step constr") or name == "this: step composed":
                print(f"{name[6:]} - {'rollout_cost_box' if unit == 'us' else 'step box'} (again): "
                      f"{st[name]['median'] - ref['median']:+.3f} {unit} (medians)")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
