#!/usr/bin/env python3
"""Wall-clock time per iteration of the many-state closed loop, composed calls against the one-call native loop, for
an f32x3 MLP at the cfg2 net shape (H = 32, d = 2, C = 4, N = 100, double_int2d), one GPU:

  composed  closed_loop(..., grouped=True, native=False)   per iteration: mpcd_normalize_states, the sampler,
                                                            mpcd_clip_flags, mpcd_rollout_cost_grouped,
                                                            mpcd_control_step, (mpcd_shift_plans), two history copies
  native    closed_loop(..., grouped=True, native=True)    one mpcd_closed_loop call: per iteration the sampler and one
                                                            closed_loop_tail_kernel launch

at 64 states x 64 candidates and 256 x 16, cold and with warm_start in --levels (default 20, 10). The two variants
alternate in one process, round after round, after both were warmed at every configuration. Per round and variant: a
host clock around the whole call (it ends in the device-to-host copies of the histories), divided by the T = --iters
iterations. Reported: the median over the rounds with their min / max. Before any timing, both variants must return
identical arrays at the timed size.

    python tools/closed_loop_ab.py [--rounds 7] [--iters 20] [--levels 20,10] [--reverse] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="closed-loop iterations T per call")
    ap.add_argument("--levels", default="20,10", help="warm-start levels K, comma separated")
    ap.add_argument("--shapes", default="64x64,256x16", help="states x candidates, comma separated")
    ap.add_argument("--reverse", action="store_true", help="run the variants of a round in the opposite order")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds must be at least 7")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    H, d, C, N, T = 32, 2, 4, 100, a.iters
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=N, context_limits=(-2 * np.ones(C), 2 * np.ones(C)))
    sysm = systems.double_int2d()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    levels = [("cold", None)] + [(f"warm K={int(k)}", int(k)) for k in a.levels.split(",") if k]
    variants = (("composed", False), ("native", True))

    def call(M, n, K, native):
        x0 = np.random.default_rng(0).uniform(-1.0, 1.0, (M, 4))
        return plan.closed_loop(x0, sysm, T, n_samples=n, w=0.01, seed=1, grouped=True, warm_start=K, native=native)

    configs = [(M, n, name, K) for M, n in shapes for name, K in levels]
    for M, n, name, K in configs:  # identical results first (this also warms both variants at every configuration)
        assert plan.grouped_pays(M, n), f"{M} x {n}: the grouped call is expected to pay"
        ref, got = call(M, n, K, False), call(M, n, K, True)
        for f in ("x", "u", "cost", "index"):
            np.testing.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f"{M} x {n} {name}: {f}")
        for _ in range(2):
            for _, native in variants:
                call(M, n, K, native)
    print(f"native == composed (x, u, cost, index) at all {len(configs)} configurations, T = {T}")
    torch.cuda.synchronize()

    order = variants[::-1] if a.reverse else variants
    ms = {(cfg, v): [] for cfg in configs for v, _ in variants}
    for _ in range(a.rounds):
        for cfg in configs:
            M, n, _, K = cfg
            for v, native in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(M, n, K, native)
                ms[(cfg, v)].append((time.perf_counter() - t0) * 1e3 / T)
    res = {"H": H, "d": d, "C": C, "n_diffusion_steps": N, "iterations": T, "rounds": a.rounds,
           "order": [v for v, _ in order], "device": torch.cuda.get_device_name(0), "configs": []}
    print(f"device {res['device']}; ms per iteration over T = {T}, wall clock around the whole call; {a.rounds} rounds; "
          f"order in a round: {', '.join(res['order'])}")
    print(f"{'states x cand':>13s} {'level':10s} {'composed median':>15s} {'min':>8s} {'max':>8s} "
          f"{'native median':>14s} {'min':>8s} {'max':>8s}  native median < composed min")
    for cfg in configs:
        M, n, name, K = cfg
        c, g = ms[(cfg, "composed")], ms[(cfg, "native")]
        wins = statistics.median(g) < min(c)
        res["configs"].append({"states": M, "candidates": n, "level": name, "composed_ms": c, "native_ms": g,
                               "composed_median": statistics.median(c), "native_median": statistics.median(g),
                               "native_median_below_composed_min": wins})
        print(f"{f'{M} x {n}':>13s} {name:10s} {statistics.median(c):15.4f} {min(c):8.4f} {max(c):8.4f} "
              f"{statistics.median(g):14.4f} {min(g):8.4f} {max(g):8.4f}  {'yes' if wins else 'no'}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
