#!/usr/bin/env python3
"""Wall-clock time per control step of M externally supplied plant states, for an f32x3 MLP at the cfg2 net shape
(H = 32, d = 2, C = 4, N = 100, double_int2d), grouped contexts, one GPU. Every variant starts from the [M, n_x] fp64
states on the host and ends with u, cost and index of every state on the host:

  batch     mpc_step_batch(x, ..., grouped=True)     one mpcd_mpc_step_batch call: one upload, the sampler, one
                                                      batch_step_tail_kernel launch, one download
  composed  the same step from the existing entry points: upload, mpcd_normalize_states, sample_trajectories(
            context_group=n), mpcd_clip_flags, mpcd_rollout_cost_grouped, mpcd_control_step on a scratch copy of the
            states (its plant step is not wanted), (mpcd_shift_plans), three downloads
  seq       M sequential mpc_step calls (warm: one prior per state, handed in with prior= and read back)

at 64 states x 64 candidates and 256 x 16, cold and with warm_start in --levels (default 20). The variants alternate in
one process, round after round, after all were warmed at every configuration. Per round and variant: a host clock
around --steps consecutive control steps (fresh states each step, the same for every variant), divided by the steps.
Reported: the median over the rounds with their min / max. Before any timing, batch and composed must return identical
u, cost and index at the timed size.

    python tools/batch_step_ab.py [--rounds 7] [--steps 20] [--levels 20] [--reverse] [--no-seq] [--json FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="control steps per timed round")
    ap.add_argument("--levels", default="20", help="warm-start levels K, comma separated")
    ap.add_argument("--shapes", default="64x64,256x16", help="states x candidates, comma separated")
    ap.add_argument("--reverse", action="store_true", help="run the variants of a round in the opposite order")
    ap.add_argument("--no-seq", action="store_true", help="leave the M sequential mpc_step calls out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds must be at least 7")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
    from mpc_via_diffusion_model_amd import _native as N
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    H, d, C, NS, T = 32, 2, 4, 100, a.steps
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=NS, context_limits=(-2 * np.ones(C), 2 * np.ones(C)))
    sysm = systems.double_int2d()
    desc = sysm.desc()
    dev, L, ctx = plan.device, plan._lib, plan._ctx
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def states(M):
        return np.random.default_rng(0).uniform(-1.0, 1.0, (T, M, 4))

    def run_batch(M, n, K, xs):
        plan.reset_warm_start()
        out = []
        for it in range(len(xs)):
            r = plan.mpc_step_batch(xs[it], sysm, n, w=0.01, seed=1 + it, grouped=True, warm_start=K)
            out.append((r.u, r.cost, r.index))
        return out

    def run_composed(M, n, K, xs):
        B, st = M * n, plan._stream()
        c = torch.empty((M, C), dtype=torch.float32, device=dev)
        flags = torch.empty(M, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        absmax = torch.empty(B, dtype=torch.float32, device=dev)
        us = torch.empty((M, d), dtype=torch.float64, device=dev)
        cs = torch.empty(M, dtype=torch.float64, device=dev)
        ix = torch.empty(M, dtype=torch.int64, device=dev)
        priors = torch.empty((M, H, d), dtype=torch.float32, device=dev) if K else None
        out = []
        for it in range(len(xs)):
            x = torch.from_numpy(xs[it]).to(dev)
            warm = dict(x_init=priors, t_start=K) if K and it > 0 else {}
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
            if K:
                plan.shift_plans(u_norm, ix, 0, out=priors)
            out.append((us.cpu().numpy(), cs.cpu().numpy(), ix.cpu().numpy()))
        return out

    def run_seq(M, n, K, xs):
        priors = [None] * M
        out = []
        for it in range(len(xs)):
            u, cst = np.empty((M, d)), np.empty(M)
            for m in range(M):
                if K:
                    plan.reset_warm_start()
                    r = plan.mpc_step(xs[it, m], sysm, n, w=0.01, seed=1 + it, warm_start=K, prior=priors[m])
                    priors[m] = plan.warm_prior()
                else:
                    r = plan.mpc_step(xs[it, m], sysm, n, w=0.01, seed=1 + it)
                u[m], cst[m] = np.round(r.u0.astype(np.float64), 4), r.best_cost
            out.append((u, cst, None))
        return out

    variants = [("batch", run_batch), ("composed", run_composed)] + ([] if a.no_seq else [("seq", run_seq)])
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    levels = [("cold", None)] + [(f"warm K={int(k)}", int(k)) for k in a.levels.split(",") if k]
    configs = [(M, n, name, K) for M, n in shapes for name, K in levels]
    for M, n, name, K in configs:  # identical results first (this also warms every variant at every configuration)
        assert plan.grouped_pays(M, n), f"{M} x {n}: the grouped call is expected to pay"
        xs = states(M)
        got, ref = run_batch(M, n, K, xs), run_composed(M, n, K, xs)
        for it in range(T):
            for f, g, r in zip(("u", "cost", "index"), got[it], ref[it]):
                np.testing.assert_array_equal(g, r, err_msg=f"{M} x {n} {name}: {f}[{it}]")
        for _, fn in variants[2:]:
            fn(M, n, K, xs[:2])
    print(f"batch == composed (u, cost, index) at all {len(configs)} configurations over {T} steps")
    torch.cuda.synchronize()

    order = variants[::-1] if a.reverse else variants
    ms = {(cfg, v): [] for cfg in configs for v, _ in variants}
    for _ in range(a.rounds):
        for cfg in configs:
            M, n, _, K = cfg
            xs = states(M)
            for v, fn in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(M, n, K, xs)
                ms[(cfg, v)].append((time.perf_counter() - t0) * 1e3 / T)
    res = {"H": H, "d": d, "C": C, "n_diffusion_steps": NS, "steps": T, "rounds": a.rounds,
           "order": [v for v, _ in order], "device": torch.cuda.get_device_name(0), "configs": []}
    print(f"device {res['device']}; ms per control step over {T} steps, wall clock from the host states to the host "
          f"results; {a.rounds} rounds; order in a round: {', '.join(res['order'])}")
    print(f"{'states x cand':>13s} {'level':10s} " + " ".join(f"{v + ' median':>15s} {'min':>8s} {'max':>8s}"
                                                               for v, _ in variants))
    for cfg in configs:
        M, n, name, K = cfg
        row = {"states": M, "candidates": n, "level": name}
        cells = []
        for v, _ in variants:
            t = ms[(cfg, v)]
            row[v + "_ms"], row[v + "_median"] = t, statistics.median(t)
            cells.append(f"{statistics.median(t):15.4f} {min(t):8.4f} {max(t):8.4f}")
        res["configs"].append(row)
        print(f"{f'{M} x {n}':>13s} {name:10s} " + " ".join(cells))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
