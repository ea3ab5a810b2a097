#!/usr/bin/env python3
"""Time per warm control step of M externally supplied plant states with and without a state box, for an f32x3 MLP at
the cfg2 net shape (H = 32, d = 2, C = 4, N = 100, double_int2d), one GPU. Every variant starts from the [M, n_x] fp64
states on the host and ends with its results on the host:

  plain           mpc_step_batch(x, ..., grouped=True, warm_start=K)             (mpcd_mpc_step_batch)
  elite           mpc_step_batch(x, ..., grouped=True, warm_start=K, elites=k)   (mpcd_mpc_step_batch_elite)
  box             mpc_step_batch_box(x, ..., box, warm_start=K)                  (mpcd_mpc_step_batch_box, winner only)
  box-elite       mpc_step_batch_box(x, ..., box, warm_start=K, elites=k)        (mpcd_mpc_step_batch_box with elites)
  composed-box / composed-box-elite
                  the constrained step a user composes from the public calls that exist without the box call: upload,
                  mpcd_normalize_states, the sampler, mpcd_clip_flags, mpcd_rollout_cost_box, mpcd_topk_feasible (k = 1
                  or k), mpcd_control_step_picked on a scratch copy of the states, mpcd_shift_plans or
                  mpcd_elite_priors, and the downloads (u, cost, index, V, n_feasible, the ranked list). It does not
                  fetch the selected plan, which the one call returns as well.

at 1 state x 4,096 candidates and 64 x 64, K = --level (default 10), k = --elites (default 8), the box +- --bound on
both velocities (states uniform in [-1, 1]: some candidates stay inside, some leave). Every round starts one fresh
process per build: this build and, with --parent-lib, a build of the parent commit (a libmpcd.so without
mpcd_mpc_step_batch_box, loaded through MPCD_LIB). Both processes first run the same sequence - the outputs of plain and
elite, then their timing at every shape - and this build's then goes on to the four constrained variants; within a
block the order of the variants flips from round to round (--reverse flips it again). Per round, variant and shape:
one untimed cold step, then --steps consecutive warm steps (fresh states each step, the same for every variant) between
two HIP events and inside a host clock; both divided by the steps. Reported: the median over the rounds with their min
/ max. Before any timing a process checks that box / box-elite and their composed forms return identical u, cost,
index, V, n_feasible and ranked lists; each build also reports a digest of the outputs of plain and elite (every field
of every step), which must be the same for both builds.

    python tools/batch_box_ab.py [--rounds 5] [--steps 20] [--level 10] [--elites 8] [--bound 0.6] [--parent-lib FILE]
                                 [--reverse] [--json FILE]"""
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
TAG = "BATCH_BOX_AB "


def worker(a):
    """one round in this process, with whichever library MPCD_LIB names: a JSON line"""
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import _native as N
    if a.worker == "parent":  # the parent's library has no such entry point to bind
        N.EXPORTS.pop("mpcd_mpc_step_batch_box", None)
    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
    from mpc_via_diffusion_model_amd.constraints import Feasibility
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    H, d, C, NS, T, k, K = 32, 2, 4, 100, a.steps, a.elites, a.level
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NS, context_limits=(-2 * np.ones(C), 2 * np.ones(C)))
    sysm = systems.double_int2d()
    desc = sysm.desc()
    dev, L, ctx = plan.device, plan._lib, plan._ctx
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    box_py = ([None, None, -a.bound, -a.bound], [None, None, a.bound, a.bound])
    tol = 0.0
    box_f = Feasibility("state_box", plan._state_box(box_py, 4), tol)

    def states(M):
        return np.random.default_rng(0).uniform(-1.0, 1.0, (T + 1, M, 4))

    def timed_loop(n_steps, step):
        """step(0) cold and untimed, then steps 1 .. between two events and inside a host clock: (ms, ms) per step"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = 0.0
        for it in range(n_steps):
            if it == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
            step(it)
        wall = (time.perf_counter() - t0) * 1e3 / (n_steps - 1)
        e1.record()
        torch.cuda.synchronize()
        return wall, e0.elapsed_time(e1) / (n_steps - 1)

    def run_batch(M, n, xs, elites, box):
        plan.reset_warm_start()
        out = []

        def step(it):
            kw = dict(w=0.01, seed=1 + it, grouped=True, warm_start=K, elites=elites)
            if box:
                out.append(plan.mpc_step_batch_box(xs[it], sysm, n, box_py, tol, **kw))
            else:
                out.append(plan.mpc_step_batch(xs[it], sysm, n, **kw))
        return out, timed_loop(len(xs), step)

    def run_composed(M, n, xs, elites):
        B, st, kk = M * n, plan._stream(), elites or 1
        grouped = plan.grouped_pays(M, n)
        c = torch.empty((M, C), dtype=torch.float32, device=dev)
        flags = torch.empty(M, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        viol = torch.empty(B, dtype=torch.float64, device=dev)
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        absmax = torch.empty(B, dtype=torch.float32, device=dev)
        us = torch.empty((M, d), dtype=torch.float64, device=dev)
        cs = torch.empty(M, dtype=torch.float64, device=dev)
        ix = torch.empty(M, dtype=torch.int64, device=dev)
        priors = torch.empty((B if elites else M, H, d), dtype=torch.float32, device=dev)
        out = []

        def step(it):
            x = torch.from_numpy(xs[it]).to(dev)
            warm = {}
            if it > 0:
                warm = dict(x_init=priors if elites or grouped else priors.repeat_interleave(n, dim=0), t_start=K)
            N.check(L.mpcd_normalize_states(ctx, ptr(x), M, C, plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data,
                                            ptr(c), st), "mpcd_normalize_states")
            plan.sample_trajectories(c if grouped else c.repeat_interleave(n, dim=0), B, H, 0.01, "ddpm_cfg", 0, None,
                                     False, 1 + it, 0, None, False, out=u_norm, absmax_out=absmax,
                                     context_group=n if grouped else None, **warm)
            N.check(L.mpcd_clip_flags(ctx, ptr(absmax), M, n, ptr(flags), st), "mpcd_clip_flags")
            box_f.rollout(plan, desc, x, n, u_norm, flags, cost, viol)
            raw, vk, nf = plan._topk_feasible_raw(cost, viol, kk, M, tol)
            # x is this step's own upload: the plant step lands in a buffer nobody reads again
            plan._control_step_picked_raw(desc, x, u_norm, raw, 0, flags, 4, us, ix, cs)
            if elites:
                plan._elite_priors_raw(u_norm, raw, n, True, 0, priors)
            else:
                plan.shift_plans(u_norm, ix, 0, out=priors)
            out.append((us.cpu().numpy(), cs.cpu().numpy(), ix.cpu().numpy(), vk.cpu().numpy(), nf.cpu().numpy(),
                        raw.cpu().numpy()))
        return out, timed_loop(len(xs), step)

    # the two unconstrained variants first, outputs and timing, in exactly the sequence both builds' processes run;
    # the constrained ones, which only this build has, after them
    this = a.worker == "this"
    free = [("plain", lambda M, n, xs: run_batch(M, n, xs, None, False)),
            ("elite", lambda M, n, xs: run_batch(M, n, xs, k, False))]
    boxed = [("box", lambda M, n, xs: run_batch(M, n, xs, None, True)),
             ("box-elite", lambda M, n, xs: run_batch(M, n, xs, k, True)),
             ("composed-box", lambda M, n, xs: run_composed(M, n, xs, None)),
             ("composed-box-elite", lambda M, n, xs: run_composed(M, n, xs, k))]
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    digest = hashlib.sha256()
    live, wall, evt = {}, {}, {}

    def time_all(variants):
        torch.cuda.synchronize()
        for M, n in shapes:
            xs = states(M)
            for v, fn in (variants[::-1] if a.reverse else variants):
                wall[f"{M} x {n}|{v}"], evt[f"{M} x {n}|{v}"] = fn(M, n, xs)[1]

    for M, n in shapes:  # the outputs first (this also warms the variants at every shape)
        xs = states(M)
        for el in (None, k):
            for r in run_batch(M, n, xs, el, False)[0]:
                for f in (r.u, r.plan, r.cost, r.index, r.flags) + ((r.elite_index, r.elite_cost) if el else ()):
                    digest.update(np.ascontiguousarray(f).tobytes())
    time_all(free)
    for M, n in shapes:
        xs = states(M)
        for el in (None, k):
            if this:
                got, ref = run_batch(M, n, xs, el, True)[0], run_composed(M, n, xs, el)[0]
                for it, (g, r) in enumerate(zip(got, ref)):
                    what = f"{M} x {n} elites={el} step {it}: "
                    np.testing.assert_array_equal(g.u, r[0], err_msg=what + "u")
                    np.testing.assert_array_equal(g.cost, r[1], err_msg=what + "cost")
                    np.testing.assert_array_equal(g.index, r[2], err_msg=what + "index")
                    np.testing.assert_array_equal(g.violation, r[3][:, 0], err_msg=what + "violation")
                    np.testing.assert_array_equal(g.n_feasible, r[4], err_msg=what + "n_feasible")
                    if el:
                        np.testing.assert_array_equal(g.elite_index, r[5][..., 1], err_msg=what + "elite index")
                        np.testing.assert_array_equal(g.elite_cost.view(np.int64), r[5][..., 0], err_msg=what + "elite cost")
                        np.testing.assert_array_equal(g.elite_violation, r[3], err_msg=what + "elite violation")
                    live[f"{M} x {n}"] = [float(np.mean([g.n_feasible.mean() / n for g in got])),
                                          float(np.mean([(g.n_feasible == 0).mean() for g in got]))]
    if this:
        time_all(boxed)
    print(TAG + json.dumps({"wall": wall, "event": evt, "digest": digest.hexdigest(), "live": live,
                            "device": torch.cuda.get_device_name(0)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed warm control steps per round")
    ap.add_argument("--level", type=int, default=10, help="warm-start level K")
    ap.add_argument("--shapes", default="1x4096,64x64", help="states x candidates, comma separated")
    ap.add_argument("--elites", type=int, default=8)
    ap.add_argument("--bound", type=float, default=0.6, help="the box: |v_x|, |v_y| <= bound")
    ap.add_argument("--parent-lib", default=None, help="libmpcd.so built from the parent commit")
    ap.add_argument("--reverse", action="store_true", help="start with the other build / variant order")
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
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--steps", str(a.steps), "--level", str(a.level),
               "--shapes", a.shapes, "--elites", str(a.elites), "--bound", str(a.bound)]
        if flip:
            cmd.append("--reverse")
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"{which} worker failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(lines[-1][len(TAG):])

    builds = ["this"] + (["parent"] if a.parent_lib else [])
    times, digests, device, live = {"wall": {}, "event": {}}, {}, None, {}
    for rnd in range(a.rounds):
        flip = (rnd % 2 == 1) != a.reverse
        for which in (builds[::-1] if flip else builds):
            r = child(which, flip)
            device = r["device"]
            live = r["live"] or live
            digests.setdefault(which, set()).add(r["digest"])
            for clock in ("wall", "event"):
                for key, v in r[clock].items():
                    cfg, var = key.split("|")
                    times[clock].setdefault(cfg, {}).setdefault(f"{which}: {var}", []).append(v)
    if any(len(dg) != 1 for dg in digests.values()) or len(set.union(*digests.values())) != 1:
        raise RuntimeError(f"plain / elite outputs differ between runs or builds: {digests}")
    print(f"device {device}; ms per warm control step (K = {a.level}) over {a.steps} steps; wall: host clock from the host "
          f"states to the host results; event: HIP events around the same steps; {a.rounds} rounds, one fresh process per "
          f"build and round; k = {a.elites}; box |v| <= {a.bound}, tol 0")
    print("box == composed-box and box-elite == composed-box-elite (u, cost, index, V, n_feasible, ranked lists) at every "
          "shape in every round; plain and elite outputs "
          + ("byte-identical on both builds" if a.parent_lib else "identical in every round")
          + f" (sha256 {next(iter(digests['this']))[:16]}...)")
    for cfg, (frac, none) in live.items():
        print(f"{cfg}: {100 * frac:.0f}% of the candidates feasible on average; {100 * none:.0f}% of the states without an "
              "admissible plan")
    res = {"H": 32, "d": 2, "C": 4, "n_diffusion_steps": 100, "steps": a.steps, "rounds": a.rounds, "elites": a.elites,
           "level": a.level, "bound": a.bound, "device": device, "wall": {}, "event": {}}
    order = ["plain", "elite", "box", "box-elite", "composed-box", "composed-box-elite"]
    for clock in ("wall", "event"):
        print(f"\n[{clock}]")
        print(f"{'states x cand':14s} {'build: variant':28s} {'median':>9s} {'min':>9s} {'max':>9s}")
        for cfg, rows in times[clock].items():
            res[clock][cfg] = {}
            for name in sorted(rows, key=lambda s: (order.index(s.split(": ")[1]), s)):
                t = rows[name]
                res[clock][cfg][name] = {"median": statistics.median(t), "min": min(t), "max": max(t), "rounds": t}
                print(f"{cfg:14s} {name:28s} {statistics.median(t):9.4f} {min(t):9.4f} {max(t):9.4f}")
            st = res[clock][cfg]
            if a.parent_lib:
                for v in ("plain", "elite"):
                    p, q = st[f"parent: {v}"], st[f"this: {v}"]
                    inside = p["min"] <= q["median"] <= p["max"]
                    print(f"{cfg:14s} {v}: this build's median {'inside' if inside else 'OUTSIDE'} the parent's min-max")
            for one, comp in (("box", "composed-box"), ("box-elite", "composed-box-elite")):
                p, q = st[f"this: {one}"], st[f"this: {comp}"]
                gap = q["median"] - p["median"]
                spread = max(p["max"] - p["min"], q["max"] - q["min"])
                verdict = "faster" if gap > spread else "slower" if -gap > spread else "not separated"
                print(f"{cfg:14s} {one} vs {comp}: {1e3 * gap:+.1f} us (medians), larger min-max spread "
                      f"{1e3 * spread:.1f} us: the one call is {verdict}")
            for one, free in (("box", "plain"), ("box-elite", "elite")):
                print(f"{cfg:14s} {one} - {free}: {1e3 * (st[f'this: {one}']['median'] - st[f'this: {free}']['median']):+.1f} "
                      "us (medians): the cost of the constraint")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
