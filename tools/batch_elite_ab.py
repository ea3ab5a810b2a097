#!/usr/bin/env python3
"""Wall-clock time per warm control step of M externally supplied plant states with and without elite sets, for an
f32x3 MLP at the cfg2 net shape (H = 32, d = 2, C = 4, N = 100, double_int2d), grouped contexts, one GPU. Every variant
starts from the [M, n_x] fp64 states on the host and ends with its results on the host:

  warm            mpc_step_batch(x, ..., grouped=True, warm_start=K)            one prior per state
                                                                                (mpcd_mpc_step_batch)
  elite           mpc_step_batch(x, ..., grouped=True, warm_start=K, elites=k)  one prior per candidate from the k best
                  plans: mpcd_mpc_step_batch_elite = the sampler, batch_step_elite_tail_kernel, one mpcd_elite_priors
                  launch, one download
  composed-elite  the same step from the existing entry points: upload, mpcd_normalize_states, the sampler with
                  per-candidate priors, mpcd_clip_flags, mpcd_rollout_cost_grouped, mpcd_control_step on a scratch copy
                  of the states, mpcd_topk, mpcd_elite_priors, four downloads

at 64 states x 64 candidates and 256 x 16, K in --levels (default 10, 20), k = --elites (default 8). Every round starts
one fresh process per build: this build, which times the three variants one after the other at every configuration, in
an order that flips from round to round (--reverse flips it again), and, with --parent-lib, a build of the parent commit
(a libmpcd.so without mpcd_mpc_step_batch_elite, loaded through MPCD_LIB), which times `warm` alone. Per round, variant
and configuration: one untimed cold step, then a host clock around --steps consecutive warm steps (fresh states each
step, the same for every variant), divided by the steps. Reported: the median over the rounds with their min / max.
Before any timing a process checks that elite and composed-elite return identical u, cost, index and elites at the
timed size; each build also reports a digest of `warm`'s outputs (u, plan, cost, index, flags of every step), which must
be the same for both builds.

    python tools/batch_elite_ab.py [--rounds 7] [--steps 20] [--levels 10,20] [--elites 8] [--parent-lib FILE]
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
TAG = "BATCH_ELITE_AB "


def worker(a):
    """one round in this process, with whichever library MPCD_LIB names: a JSON line"""
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import _native as N
    if a.worker == "parent":  # the parent's library has no such entry point to bind
        N.EXPORTS.pop("mpcd_mpc_step_batch_elite", None)
    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    H, d, C, NS, T, k = 32, 2, 4, 100, a.steps, a.elites
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NS, context_limits=(-2 * np.ones(C), 2 * np.ones(C)))
    sysm = systems.double_int2d()
    desc = sysm.desc()
    dev, L, ctx = plan.device, plan._lib, plan._ctx
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def states(M):
        return np.random.default_rng(0).uniform(-1.0, 1.0, (T + 1, M, 4))

    def run_batch(M, n, K, xs, elites, timed):
        """step 0 cold and untimed, then the timed warm steps: (results, ms per warm step)"""
        plan.reset_warm_start()
        out, t0 = [], 0.0
        for it in range(len(xs)):
            if it == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            r = plan.mpc_step_batch(xs[it], sysm, n, w=0.01, seed=1 + it, grouped=True, warm_start=K, elites=elites)
            if not timed:
                out.append(r)
        return out, (time.perf_counter() - t0) * 1e3 / (len(xs) - 1)

    def run_composed(M, n, K, xs, timed):
        B, st = M * n, plan._stream()
        c = torch.empty((M, C), dtype=torch.float32, device=dev)
        flags = torch.empty(M, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        absmax = torch.empty(B, dtype=torch.float32, device=dev)
        us = torch.empty((M, d), dtype=torch.float64, device=dev)
        cs = torch.empty(M, dtype=torch.float64, device=dev)
        ix = torch.empty(M, dtype=torch.int64, device=dev)
        raw = torch.empty((M, k, 2), dtype=torch.int64, device=dev)
        priors = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        out, t0 = [], 0.0
        for it in range(len(xs)):
            if it == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            x = torch.from_numpy(xs[it]).to(dev)
            warm = dict(x_init=priors, t_start=K) if it > 0 else {}
            N.check(L.mpcd_normalize_states(ctx, ptr(x), M, C, plan.ctx_min.ctypes.data, plan.ctx_max.ctypes.data,
                                            ptr(c), st), "mpcd_normalize_states")
            plan.sample_trajectories(c, B, H, 0.01, "ddpm_cfg", 0, None, False, 1 + it, 0, None, False, out=u_norm,
                                     absmax_out=absmax, context_group=n, **warm)
            N.check(L.mpcd_clip_flags(ctx, ptr(absmax), M, n, ptr(flags), st), "mpcd_clip_flags")
            N.check(L.mpcd_rollout_cost_grouped(ctx, ctypes.byref(desc), ptr(x), n, ptr(u_norm),
                                                plan.act_min.ctypes.data, plan.act_max.ctypes.data, B, H, ptr(flags),
                                                ptr(cost), st), "mpcd_rollout_cost_grouped")
            # x is this step's own upload: mpcd_control_step's plant step lands in a buffer nobody reads again
            N.check(L.mpcd_control_step(ctx, ctypes.byref(desc), ptr(x), M, n, ptr(u_norm), H, ptr(cost),
                                        plan.act_min.ctypes.data, plan.act_max.ctypes.data, ptr(flags), 0, 4, ptr(us),
                                        ptr(ix), ptr(cs), st), "mpcd_control_step")
            N.check(L.mpcd_topk(ctx, ptr(cost), M, n, k, 0, ptr(raw), st), "mpcd_topk")
            N.check(L.mpcd_elite_priors(ctx, ptr(u_norm), M, n, H, ptr(raw), k, 0, 1, ptr(priors), st),
                    "mpcd_elite_priors")
            res = (us.cpu().numpy(), cs.cpu().numpy(), ix.cpu().numpy(), raw.cpu().numpy())
            if not timed:
                out.append(res)
        return out, (time.perf_counter() - t0) * 1e3 / (len(xs) - 1)

    this = a.worker == "this"
    variants = [("warm", lambda M, n, K, xs, timed: run_batch(M, n, K, xs, None, timed))]
    if this:
        variants += [("elite", lambda M, n, K, xs, timed: run_batch(M, n, K, xs, k, timed)), ("composed-elite", run_composed)]
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    configs = [(M, n, int(K)) for M, n in shapes for K in a.levels.split(",") if K]
    digest = hashlib.sha256()
    for M, n, K in configs:  # the outputs first (this also warms every variant at every configuration)
        assert plan.grouped_pays(M, n), f"{M} x {n}: the grouped call is expected to pay"
        xs = states(M)
        for r in run_batch(M, n, K, xs, None, False)[0]:
            for f in (r.u, r.plan, r.cost, r.index, r.flags):
                digest.update(np.ascontiguousarray(f).tobytes())
        if this:
            got, ref = run_batch(M, n, K, xs, k, False)[0], run_composed(M, n, K, xs, False)[0]
            for it, (g, r) in enumerate(zip(got, ref)):
                what = f"{M} x {n} K={K} step {it}: "
                np.testing.assert_array_equal(g.u, r[0], err_msg=what + "u")
                np.testing.assert_array_equal(g.cost, r[1], err_msg=what + "cost")
                np.testing.assert_array_equal(g.index, r[2], err_msg=what + "index")
                np.testing.assert_array_equal(g.elite_index, r[3][..., 1], err_msg=what + "elite index")
                np.testing.assert_array_equal(g.elite_cost.view(np.int64), r[3][..., 0], err_msg=what + "elite cost")
    torch.cuda.synchronize()
    order = variants[::-1] if a.reverse else variants
    ms = {}
    for M, n, K in configs:
        xs = states(M)
        for v, fn in order:
            ms[f"{M} x {n} K={K}|{v}"] = fn(M, n, K, xs, True)[1]
    print(TAG + json.dumps({"ms": ms, "warm_digest": digest.hexdigest(), "device": torch.cuda.get_device_name(0),
                            "agree": this}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="timed warm control steps per round")
    ap.add_argument("--levels", default="10,20", help="warm-start levels K, comma separated")
    ap.add_argument("--shapes", default="64x64,256x16", help="states x candidates, comma separated")
    ap.add_argument("--elites", type=int, default=8)
    ap.add_argument("--parent-lib", default=None, help="libmpcd.so built from the parent commit")
    ap.add_argument("--reverse", action="store_true", help="start with the other build / variant order")
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", default=None, choices=("this", "parent"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.worker:
        return worker(a)
    if a.rounds < 7:
        ap.error("--rounds must be at least 7")

    def child(which, flip):
        env = dict(os.environ)
        if which == "parent":
            env["MPCD_LIB"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("MPCD_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--steps", str(a.steps), "--levels", a.levels,
               "--shapes", a.shapes, "--elites", str(a.elites)]
        if flip:
            cmd.append("--reverse")
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"{which} worker failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(lines[-1][len(TAG):])

    builds = ["this"] + (["parent"] if a.parent_lib else [])
    ms, digests, device = {}, {}, None
    for rnd in range(a.rounds):
        flip = (rnd % 2 == 1) != a.reverse
        for which in (builds[::-1] if flip else builds):
            r = child(which, flip)
            device = r["device"]
            digests.setdefault(which, set()).add(r["warm_digest"])
            for key, v in r["ms"].items():
                cfg, var = key.split("|")
                ms.setdefault(cfg, {}).setdefault(f"{which}: {var}", []).append(v)
    if any(len(d) != 1 for d in digests.values()) or len(set.union(*digests.values())) != 1:
        raise RuntimeError(f"`warm` outputs differ between runs or builds: {digests}")
    print(f"device {device}; ms per warm control step over {a.steps} steps, wall clock from the host states to the host "
          f"results; {a.rounds} rounds, one fresh process per build and round; k = {a.elites}")
    print("elite == composed-elite (u, cost, index, elites) at every configuration in every round; `warm` outputs "
          + ("byte-identical on both builds" if a.parent_lib else "identical in every round")
          + f" (sha256 {next(iter(digests['this']))[:16]}...)")
    print(f"{'states x cand, level':22s} {'build: variant':22s} {'median':>9s} {'min':>9s} {'max':>9s}")
    res = {"H": 32, "d": 2, "C": 4, "n_diffusion_steps": 100, "steps": a.steps, "rounds": a.rounds, "elites": a.elites,
           "device": device, "configs": {}}
    for cfg, rows in ms.items():
        res["configs"][cfg] = {}
        for name in sorted(rows, key=lambda s: (s.split(": ")[1] != "warm", s.split(": ")[1], s)):
            t = rows[name]
            res["configs"][cfg][name] = {"median": statistics.median(t), "min": min(t), "max": max(t), "rounds": t}
            print(f"{cfg:22s} {name:22s} {statistics.median(t):9.4f} {min(t):9.4f} {max(t):9.4f}")
        med = {name: statistics.median(t) for name, t in rows.items()}
        print(f"{cfg:22s} elite - warm {1e3 * (med['this: elite'] - med['this: warm']):+.1f} us; elite - composed-elite "
              f"{1e3 * (med['this: elite'] - med['this: composed-elite']):+.1f} us (medians)")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
