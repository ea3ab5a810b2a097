#!/usr/bin/env python3
"""Control-step time of warm-started sampling against the cold step, for an f32x3 MLP at the cfg2 net shape (H = 32,
d = 2, N = 100), B = 4,096 candidates, one GPU:

  cold      mpc_step(...)                  the full chain, N denoise steps (mpcd_mpc_step)
  warm K    mpc_step(..., warm_start=K)    K denoise steps from the previous winner's shifted plan (mpcd_mpc_step_warm)

for K in --levels (default 100, 50, 20, 10). The variants alternate in one process, round after round; per round and
variant: wall-clock ms per control step over --calls steps (the call returns when the result is on the host) and
mpcd_sample_ms_mean (HIP events around the sampler launch) over the same steps. Reported: the median over the rounds
with their min / max (the run-to-run spread inside the process).

    python tools/warm_ab.py [--rounds 7] [--calls 20] [--levels 100,50,20,10] [--reverse] [--json FILE] [--quality]

--quality: instead of the timing, one control-quality figure: the closed-loop cost (sum over 20 steps of the stage
cost of the realised states and actions, mean over 8 start states) of the trained CartPole-LMPC checkpoint
tests/golden/lmpc_2406400_1000000 (U-Net, N = 25, linear ZOH cart-pole), cold against warm_start = N / 5. It says
something about that model at that K and nothing about another."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quality(a):
    import numpy as np
    import torch
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
    for name, kw in (("cold", {}), (f"warm_start={K}", dict(warm_start=K))):
        r = plan.closed_loop(x0, sysm, T, n_samples=n, w=0.01, n_wo_noise=5, seed=1, **kw)
        cost = (((r.x[:, 1:] - xref) ** 2) * Q).sum(-1) + ((r.u ** 2) * R).sum(-1)  # [M, T]
        res[name] = {"closed_loop_cost_mean": float(cost.sum(1).mean()), "per_state": cost.sum(1).tolist()}
        print(f"{name:16s} closed-loop cost over {T} steps, mean of {M} states: {res[name]['closed_loop_cost_mean']:.6g}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--levels", default="100,50,20,10", help="warm-start levels K, comma separated")
    ap.add_argument("--reverse", action="store_true", help="run the variants of a round in the opposite order")
    ap.add_argument("--json", default=None)
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    if a.quality:
        return quality(a)
    H, d, C, N, B = 32, 2, 4, 100, a.batch
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=N)
    sysm = systems.double_int2d()
    x0 = np.array([0.3, -0.2, 0.1, 0.05])
    step = [0]

    def call(**kw):
        step[0] += 1
        return plan.mpc_step(x0, sysm, B, w=0.01, seed=step[0], **kw)

    variants = {"cold": {}}
    for k in (int(s) for s in a.levels.split(",")):
        variants[f"warm K={k}"] = dict(warm_start=k)

    def timed(kw):
        call(**kw)  # a change of K rebuilds the step plan and its time projections once: not part of a step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            call(**kw)
        wall = (time.perf_counter() - t0) * 1e3 / a.calls
        return wall, plan.sample_ms_mean(a.calls)

    for kw in variants.values():  # warm every shape: code objects, buffers, the prior
        for _ in range(20):
            call(**kw)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    order = list(variants)[::-1] if a.reverse else list(variants)
    for _ in range(a.rounds):
        for k in order:
            ms[k].append(timed(variants[k]))
    f = plan.mlp_form(B)
    res = {"batch": B, "H": H, "d": d, "n_diffusion_steps": N, "rounds": a.rounds, "calls_per_round": a.calls,
           "device": torch.cuda.get_device_name(0), "kernel": f"{f['kernel']} {f['layout']}", "variants": {}}
    print(f"{'variant':12s} {'step ms median':>15s} {'min':>8s} {'max':>8s} {'sample_ms_mean median':>22s} {'min':>8s} {'max':>8s}")
    for k, v in ms.items():
        w, s = [x[0] for x in v], [x[1] for x in v]
        r = {"step_ms_median": statistics.median(w), "step_ms_min": min(w), "step_ms_max": max(w),
             "sample_ms_mean_median": statistics.median(s), "sample_ms_min": min(s), "sample_ms_max": max(s), "rounds": v}
        res["variants"][k] = r
        print(f"{k:12s} {r['step_ms_median']:15.4f} {min(w):8.4f} {max(w):8.4f} {r['sample_ms_mean_median']:22.4f} "
              f"{min(s):8.4f} {max(s):8.4f}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
