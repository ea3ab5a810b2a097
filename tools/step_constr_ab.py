#!/usr/bin/env python3
"""What the constraint set costs in the one-call control step, and that mpc_step beside it is the parent's: double_int2d,
H = 32, an f32x3 MLP at the cfg2 net shape (d = 2, C = 4, N = 100), one GPU, one state x 4,096 candidates.

Both builds (this one and, with --parent-lib, a libmpcd.so of the parent commit loaded through MPCD_LIB) run, in the same
sequence, what this change leaves alone: the native unconstrained mpc_step, cold, warm (K = 10) and warm with elites = 8,
and the composed constrained step mpc_step(constraints=) (cold: it takes no warm start). A digest of every output must be
the same for both builds. This build's process, and the parent's if its library has the entry point (then a second
digest, of these outputs, must be the same too), goes on to mpc_step_constr:

  constr box               the box alone, cold
  constr full              the box, 2 rows, the rate bounds and u_prev, cold
  constr full warm         the same with warm_start = 10
  constr full warm elites  the same with warm_start = 10, elites = 8

Before any timing each process of this build checks that the composed step and the one call return the same index,
cost, V and n_feasible. ms per control step: the host clock around the call (which ends synchronised), and beside it the
time between two HIP events recorded around the call. Every round starts one fresh process per build; the build order
flips from round to round. Reported: the median over the rounds with their min / max.

    python tools/step_constr_ab.py [--rounds 5] [--steps 20] [--parent-lib FILE] [--json FILE]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "STEP_CONSTR_AB "
NEW = ("mpcd_mpc_step_constr",)


def worker(a):
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import _native as N
    this = a.worker == "this"
    if not this:  # a parent from before mpc_step_constr has no such entry point to bind; a later one runs those paths too
        import ctypes
        this = all(hasattr(ctypes.CDLL(os.environ["MPCD_LIB"]), name) for name in NEW)
        if not this:
            for name in NEW:
                N.EXPORTS.pop(name, None)
    from mpc_via_diffusion_model_amd import Constraints, DiffusionMPC, NetSpec, systems
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    H, d, C, NS, T, B, k, K = 32, 2, 4, 100, a.steps, 4096, 8, 10
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NS, context_limits=(-2 * np.ones(C), 2 * np.ones(C)))
    sysm = systems.double_int2d()
    box_py = ([None, None, -0.6, -0.6], [None, None, 0.6, 0.6])
    rows = [([0.1 * (r + 1), -0.2, 0.3, 0.05 * r], [0.25, -0.125], 1e6) for r in range(2)]
    box, full, tol = Constraints(box_py), Constraints(box_py, rows, [1.9, 1.95]), 0.0
    xs = np.random.default_rng(0).uniform(-1.0, 1.0, (T + 1, 4))
    digest, digest_constr = hashlib.sha256(), hashlib.sha256()
    res, live = {}, {}

    def add(dg, r):
        fields = [r.u_best, np.float64(r.best_cost), np.int64(r.best_index), r.costs.cpu().numpy(), r.u_norm.cpu().numpy()]
        fields += [np.asarray(f) for f in (r.violation, r.n_feasible, r.elite_index, r.elite_cost, r.elite_violation)
                   if f is not None]
        for f in fields:
            dg.update(np.ascontiguousarray(f).tobytes())

    def run(kind):
        """T + 1 control steps (the first one untimed): (results, ms per step by the host clock, by HIP events)"""
        plan.reset_warm_start()
        out, prev, host, evs = [], [np.array([0.0, 0.0])], [], []
        for it in range(T + 1):
            kw = dict(w=0.01, seed=1 + it)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            if kind == "step":
                r = plan.mpc_step(xs[it], sysm, B, **kw)
            elif kind == "step warm":
                r = plan.mpc_step(xs[it], sysm, B, warm_start=K, **kw)
            elif kind == "step warm elites":
                r = plan.mpc_step(xs[it], sysm, B, warm_start=K, elites=k, **kw)
            elif kind == "composed full":
                r = plan.mpc_step(xs[it], sysm, B, constraints=full, u_prev=prev[0], viol_tol=tol, **kw)
            elif kind == "constr box":
                r = plan.mpc_step_constr(xs[it], sysm, B, box, tol, **kw)
            elif kind == "constr full":
                r = plan.mpc_step_constr(xs[it], sysm, B, full, tol, prev[0], **kw)
            elif kind == "constr full warm":
                r = plan.mpc_step_constr(xs[it], sysm, B, full, tol, prev[0], warm_start=K, **kw)
            else:
                r = plan.mpc_step_constr(xs[it], sysm, B, full, tol, prev[0], warm_start=K, elites=k, **kw)
            t1 = time.perf_counter()  # the call ended synchronised: its results are on the host
            e1.record()
            torch.cuda.synchronize()
            prev[0] = r.u0.astype(np.float64)
            out.append(r)
            if it > 0:
                host.append((t1 - t0) * 1e3)
                evs.append(e0.elapsed_time(e1))
        return out, statistics.mean(host), statistics.mean(evs)

    common = ["step", "step warm", "step warm elites", "composed full"]
    flip = (lambda seq: list(seq)[::-1]) if a.reverse else list
    for kind in common:  # the outputs first (this also warms every variant)
        for r in run(kind)[0]:
            add(digest, r)
    for kind in flip(common):
        _, res[f"host|{kind}"], res[f"event|{kind}"] = run(kind)
    if this:
        own = ["constr box", "constr full", "constr full warm", "constr full warm elites"]
        ref, got = run("composed full")[0], run("constr full")[0]
        for it, (g, r) in enumerate(zip(got, ref)):
            assert (g.best_index, g.best_cost, g.violation, g.n_feasible) == \
                (r.best_index, r.best_cost, r.violation, r.n_feasible), f"step {it}: the one call is not the composed step"
            np.testing.assert_array_equal(g.u_best, r.u_best)
        for kind in own:
            out = run(kind)[0]
            live[kind] = float(np.mean([r.n_feasible for r in out[1:]]))
            for r in out:
                add(digest_constr, r)
        for kind in flip(own + ["composed full"]):
            name = kind if kind != "composed full" else "composed full (again)"
            _, res[f"host|{name}"], res[f"event|{name}"] = run(kind)
    print(TAG + json.dumps({"res": res, "live": live, "digest": digest.hexdigest(), "device": torch.cuda.get_device_name(0),
                            "digest_constr": digest_constr.hexdigest() if this else None}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed control steps per path and round")
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
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--steps", str(a.steps)] + \
            (["--reverse"] if flip else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"{which} worker failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(lines[-1][len(TAG):])

    builds = ["this"] + (["parent"] if a.parent_lib else [])
    times, digests, device, live, constr, constr_builds = {}, {}, None, {}, set(), set()
    for rnd in range(a.rounds):
        flip = (rnd % 2 == 1) != a.reverse
        for which in (builds[::-1] if flip else builds):
            r = child(which, flip)
            device = r["device"]
            digests.setdefault(which, set()).add(r["digest"])
            if r.get("digest_constr"):
                constr.add(r["digest_constr"])
                constr_builds.add(which)
            live.update(r["live"])
            for key, v in r["res"].items():
                clock, name = key.split("|")
                times.setdefault(clock, {}).setdefault(f"{which}: {name}", []).append(v)
    if any(len(dg) != 1 for dg in digests.values()) or len(set.union(*digests.values())) != 1:
        raise RuntimeError(f"the unchanged paths' outputs differ between runs or builds: {digests}")
    if len(constr) != 1:
        raise RuntimeError(f"mpc_step_constr's outputs differ between runs or builds: {constr}")
    print(f"device {device}; {a.rounds} rounds, one fresh process per build and round; ms per control step over {a.steps} "
          "steps of one state x 4,096 candidates; host: the host clock around the call; event: between two HIP events "
          "recorded around it")
    print("mpc_step (cold, warm K = 10, with elites = 8) and the composed mpc_step(constraints=) outputs "
          + ("byte-identical on both builds" if a.parent_lib else "identical in every round")
          + f" (sha256 {next(iter(digests['this']))[:16]}...); mpc_step_constr == the composed step (index, cost, V, "
          "n_feasible, plan) at every step in every round; its four forms' outputs "
          + ("byte-identical on both builds" if len(constr_builds) == 2 else "identical in every round")
          + f" (sha256 {next(iter(constr))[:16]}...)")
    for kind, n in live.items():
        print(f"{kind}: {n:.0f} of 4096 candidates feasible on average over the timed steps")
    out = {}
    for clock, rows_ in times.items():
        print(f"\n[{clock}, ms per step]\n{'build: path':40s} {'median':>10s} {'min':>10s} {'max':>10s}")
        st = {name: {"median": statistics.median(t), "min": min(t), "max": max(t), "rounds": t} for name, t in rows_.items()}
        for name in sorted(st, key=lambda s: (s.split(": ")[1], s)):
            print(f"{name:40s} {st[name]['median']:10.3f} {st[name]['min']:10.3f} {st[name]['max']:10.3f}")
        out[clock] = st
        spread = lambda s: s["max"] - s["min"]  # noqa: E731
        one = st.get("this: constr full")
        for base in ("parent: composed full", "this: composed full (again)", "parent: step", "this: step"):
            if one and base in st:
                print(f"constr full - {base}: {one['median'] - st[base]['median']:+.3f} ms (medians); the larger min-max "
                      f"spread of the two: {max(spread(one), spread(st[base])):.3f} ms")
        if a.parent_lib:
            for name in sorted(st):
                if name.startswith("parent: "):
                    p, q = st[name], st["this: " + name[8:]]
                    inside = p["min"] <= q["median"] <= p["max"]
                    print(f"{name[8:]}: this build's median {'inside' if inside else 'OUTSIDE'} the parent's min-max")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
