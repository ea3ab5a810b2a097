#!/usr/bin/env python3
"""Control-step time of the elite-seeded warm start against the plain warm start, for an f32x3 MLP at the cfg2 net shape
(H = 32, d = 2, N = 100), B = 4,096 candidates, one GPU:

  warm K          mpc_step(..., warm_start=K)             one shared prior (mpcd_mpc_step_warm)
  elite K k=8     mpc_step(..., warm_start=K, elites=8)   one prior per candidate from the 8 best plans
                                                          (mpcd_mpc_step_elite: + the top-k and the prior-writer launch)

for K in --levels (default 10, 20). Every round starts one fresh process per build: this build, which times both
variants alternately, and, with --parent-lib, a build of the parent commit (a libmpcd.so without the elite entry points,
loaded through MPCD_LIB), which times `warm K` alone: the reference the added launches are judged against. The two
processes of a round alternate in order from round to round (--reverse flips it). Per round and variant: wall-clock ms
per control step over --calls steps (the call returns when the result is on the host) and mpcd_sample_ms_mean over the
same steps. Reported: the median over the rounds with their min / max (the run-to-run spread).
This build's process also times the two added launches alone with HIP events at the same size: one event pair around
each launch (median of --reps), and one pair around --reps back-to-back launches divided by their number.

    python tools/elite_ab.py [--rounds 7] [--calls 20] [--levels 10,20] [--elites 8] [--parent-lib FILE] [--reverse]
                             [--json FILE] [--quality]

--quality: instead of the timing, the closed-loop cost (sum over 20 steps of the stage cost of the realised states and
actions, mean over 8 start states, 64 candidates) of the trained CartPole-LMPC checkpoint tests/golden/
lmpc_2406400_1000000 (U-Net, N = 25, linear ZOH cart-pole): cold, warm_start = 5, and warm_start = 5 with elites 4 and
8. It says something about that model at that K and nothing about another."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quality(a):
    import numpy as np
    from safetensors.torch import load_file

    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems

    sd = load_file(os.path.join(ROOT, "tests", "golden", "lmpc_2406400_1000000_ema.safetensors"))
    cmin = np.array([-2, -3, -0.5, -3], dtype=np.float32)
    cmax = np.array([2, 3, 0.5, 3], dtype=np.float32)
    plan = DiffusionMPC.from_state_dict(sd, NetSpec("unet", state_dim=1, horizon=32, context_dim=4, dtype="f32x3"),
                                        action_limits=(np.array([-10.0]), np.array([10.0])), context_limits=(cmin, cmax))
    sysm = systems.get("cartpole_zoh4")
    M, T, n, K = 8, 20, 64, plan.n_steps // 5
    x0 = np.random.default_rng(0).uniform(-0.5, 0.5, (M, 4)) * np.array([1.0, 1.0, 0.3, 1.0])
    Q, R = np.asarray(sysm.Q[:sysm.n_x]), np.asarray(sysm.R[:sysm.n_u])
    xref = np.asarray((sysm.x_ref or [0.0] * 12)[:sysm.n_x])
    res = {"model": "lmpc_2406400_1000000", "n_diffusion_steps": plan.n_steps, "states": M, "steps": T, "n_samples": n}
    variants = [("cold", {}), (f"warm_start={K}", dict(warm_start=K))]
    variants += [(f"warm_start={K} elites={k}", dict(warm_start=K, elites=k)) for k in (4, 8)]
    for name, kw in variants:
        r = plan.closed_loop(x0, sysm, T, n_samples=n, w=0.01, n_wo_noise=5, seed=1, **kw)
        cost = (((r.x[:, 1:] - xref) ** 2) * Q).sum(-1) + ((r.u ** 2) * R).sum(-1)  # [M, T]
        res[name] = {"closed_loop_cost_mean": float(cost.sum(1).mean()), "per_state": cost.sum(1).tolist()}
        print(f"{name:24s} closed-loop cost over {T} steps, mean of {M} states: {res[name]['closed_loop_cost_mean']:.6g}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


def worker(a):
    """one round in this process, with whichever library MPCD_LIB names: a JSON line {variant: [step ms, sample ms]}"""
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import _native as nat
    if a.worker == "parent":  # the parent's library has no elite entry points to bind
        for name in ("mpcd_topk", "mpcd_elite_priors", "mpcd_mpc_step_elite"):
            nat.EXPORTS.pop(name, None)
    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
    from oracle import nets

    H, d, C, N, B = 32, 2, 4, 100, a.batch
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=N)
    sysm = systems.double_int2d()
    x0 = np.array([0.3, -0.2, 0.1, 0.05])
    has_elite = hasattr(plan._lib, "mpcd_mpc_step_elite") and a.worker == "this"
    step = [0]

    def call(**kw):
        step[0] += 1
        return plan.mpc_step(x0, sysm, B, w=0.01, seed=step[0], **kw)

    variants = {}
    for k in (int(s) for s in a.levels.split(",")):
        variants[f"warm K={k}"] = dict(warm_start=k)
        if has_elite:
            variants[f"elite K={k} k={a.elites}"] = dict(warm_start=k, elites=a.elites)
    out = {}
    order = list(variants)[::-1] if a.reverse else list(variants)
    for name in order:
        kw = variants[name]
        plan.reset_warm_start()
        for _ in range(20):  # code objects, buffers, the priors, the K-step plan
            call(**kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call(**kw)
        out[name] = [(time.perf_counter() - t0) * 1e3 / a.calls, plan.sample_ms_mean(a.calls)]
    res = {"variants": out, "device": torch.cuda.get_device_name(0)}
    if has_elite:  # the two added launches alone, HIP events
        cost = torch.randn(B, dtype=torch.float64, device="cuda")
        u = torch.randn(B, H, d, device="cuda")
        pri = torch.empty_like(u)
        raw = plan._topk_raw(cost, a.elites, 1)
        launches = {"topk": lambda: plan._topk_raw(cost, a.elites, 1),
                    "elite_priors": lambda: plan._elite_priors_raw(u, raw, B, True, 0, pri)}
        res["launch_us"] = {}
        for name, fn in launches.items():
            for _ in range(10):
                fn()
            single = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                single.append(e0.elapsed_time(e1) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            res["launch_us"][name] = {"single_median": statistics.median(single), "single_min": min(single),
                                      "back_to_back": e0.elapsed_time(e1) * 1e3 / a.reps}
    print("ELITE_AB " + json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--levels", default="10,20", help="warm-start levels K, comma separated")
    ap.add_argument("--elites", type=int, default=8)
    ap.add_argument("--reps", type=int, default=100, help="launches per event timing")
    ap.add_argument("--parent-lib", default=None, help="libmpcd.so built from the parent commit")
    ap.add_argument("--reverse", action="store_true", help="start with the other build / variant")
    ap.add_argument("--json", default=None)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--worker", default=None, choices=("this", "parent"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.quality:
        return quality(a)
    if a.worker:
        return worker(a)

    def child(which, flip):
        env = dict(os.environ)
        if which == "parent":
            env["MPCD_LIB"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("MPCD_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--calls", str(a.calls), "--batch",
               str(a.batch), "--levels", a.levels, "--elites", str(a.elites), "--reps", str(a.reps)]
        if flip:
            cmd.append("--reverse")
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ELITE_AB ")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"{which} worker failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(lines[-1][len("ELITE_AB "):])

    builds = ["this"] + (["parent"] if a.parent_lib else [])
    ms, launch, device = {}, {}, None
    for rnd in range(a.rounds):
        flip = (rnd % 2 == 1) != a.reverse
        for which in (builds[::-1] if flip else builds):
            r = child(which, flip)
            device = r["device"]
            for name, v in r["variants"].items():
                ms.setdefault(f"{which}: {name}", []).append(v)
            for name, v in r.get("launch_us", {}).items():
                for f, x in v.items():
                    launch.setdefault(name, {}).setdefault(f, []).append(x)
    res = {"batch": a.batch, "H": 32, "d": 2, "n_diffusion_steps": 100, "rounds": a.rounds, "calls_per_round": a.calls,
           "device": device, "variants": {}, "launch_us": {}}
    print(f"device {device}; B = {a.batch}; {a.rounds} rounds, one fresh process per build and round, {a.calls} steps each")
    print(f"{'build: variant':28s} {'step ms median':>15s} {'min':>8s} {'max':>8s} {'sample_ms_mean median':>22s} {'min':>8s} {'max':>8s}")
    for k in sorted(ms, key=lambda s: (s.split("K=")[1].split()[0], s)):
        w, s = [x[0] for x in ms[k]], [x[1] for x in ms[k]]
        res["variants"][k] = {"step_ms_median": statistics.median(w), "step_ms_min": min(w), "step_ms_max": max(w),
                              "sample_ms_mean_median": statistics.median(s), "rounds": ms[k]}
        print(f"{k:28s} {statistics.median(w):15.4f} {min(w):8.4f} {max(w):8.4f} {statistics.median(s):22.4f} "
              f"{min(s):8.4f} {max(s):8.4f}")
    if launch:
        print(f"\nthe added launches alone, HIP events, microseconds (median over the rounds; k = {a.elites}, one state x "
              f"{a.batch} candidates, H = 32, d = 2)")
        print(f"{'launch':14s} {'one launch per event pair':>26s} {'its minimum':>12s} {'back to back, per launch':>25s}")
        for name, v in launch.items():
            res["launch_us"][name] = {f: statistics.median(x) for f, x in v.items()}
            print(f"{name:14s} {statistics.median(v['single_median']):26.2f} {statistics.median(v['single_min']):12.2f} "
                  f"{statistics.median(v['back_to_back']):25.2f}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
