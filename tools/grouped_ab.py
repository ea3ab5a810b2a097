#!/usr/bin/env python3
"""Sampler-kernel time of a closed-loop batch three ways, for an f32x3 MLP at the cfg2 net shape (H = 32, d = 2,
N = 100): B = 4,096 candidates as 64 states x 64, 256 x 16 and 4,096 x 1, each with

  grouped        one context row per state (mpcd_sample_grouped: split-bf16 kernels, workgroups aligned to the states)
  per_candidate  the state's row repeated per candidate (what closed_loop(grouped=False) hands over: exact-f32 kernel)

next to the shared-context call of the same B (one row for all: the ceiling). The variants alternate in one process,
round after round; each figure is mpcd_sample_ms_mean (HIP events around the sampler launch) over the calls of a round,
reported as the median over the rounds with their min / max (the run-to-run spread inside the process).

    python tools/grouped_ab.py [--rounds 7] [--calls 20] [--splits 64,16,1] [--reverse] [--tree DIR] [--json FILE]

--tree DIR: time the package of another checkout (built there) instead, e.g. the parent commit's; a tree without
mpcd_sample_grouped reports the shared and per-candidate variants only. Alternate `--tree` runs of two builds in
one session to compare them."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default=None)
    ap.add_argument("--splits", default="64,16,1", help="candidates per state, comma separated (each divides --batch)")
    ap.add_argument("--reverse", action="store_true", help="run the variants of a round in the opposite order")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec
    from oracle import nets

    assert torch.cuda.is_available(), "a timing needs the GPU"
    H, d, C, N, B = 32, 2, 4, 100, a.batch
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), variance_schedule="exponential",
                        n_diffusion_steps=N)
    has_grouped = hasattr(plan, "mlp_form_grouped")
    out = torch.empty(B, H, d, device="cuda")
    g = torch.Generator().manual_seed(1)
    variants = {}  # name -> (call, kernel description)
    shared = (torch.rand(1, C, generator=g) * 2 - 1).cuda()
    f = plan.mlp_form(B)
    variants["shared"] = (lambda: plan.sample_trajectories(shared, B, H, seed=3, out=out), f"{f['kernel']} {f['layout']}")
    for n in (int(s) for s in a.splits.split(",")):
        assert B % n == 0, f"{n} does not divide {B}"
        M = B // n
        rows = (torch.rand(M, C, generator=g) * 2 - 1).cuda()
        rep = rows.repeat_interleave(n, 0).contiguous()
        if has_grouped:
            f = plan.mlp_form_grouped(M, n)
            variants[f"{M}x{n} grouped"] = (lambda rows=rows, n=n: plan.sample_trajectories(rows, B, H, seed=3, out=out, context_group=n),
                                            f"{f['kernel']} {f['layout']}")
        variants[f"{M}x{n} per_candidate"] = (lambda rep=rep: plan.sample_trajectories(rep, B, H, seed=3, out=out), "f32")

    def timed(call):
        for _ in range(a.calls):
            call()
        return plan.sample_ms_mean(a.calls)  # blocks until the last call has finished

    for call, _ in variants.values():  # warm every shape: code objects, buffers
        call()
        call()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    order = list(variants)[::-1] if a.reverse else list(variants)
    for _ in range(a.rounds):
        for k in order:
            ms[k].append(timed(variants[k][0]))
    res = {"batch": B, "H": H, "d": d, "n_diffusion_steps": N, "rounds": a.rounds, "calls_per_round": a.calls,
           "device": torch.cuda.get_device_name(0), "tree": os.path.abspath(a.tree), "variants": {}}
    print(f"{'variant':26s} {'kernel':12s} {'median ms':>10s} {'min':>8s} {'max':>8s}")
    for k, v in ms.items():
        r = {"kernel": variants[k][1], "sample_ms_mean_median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}
        res["variants"][k] = r
        print(f"{k:26s} {r['kernel']:12s} {r['sample_ms_mean_median']:10.4f} {r['min']:8.4f} {r['max']:8.4f}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
