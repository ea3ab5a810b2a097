#!/usr/bin/env python3
"""What the state-constraint entry points cost, against the calls they stand beside, and that the existing path is
untouched. One GPU. Three parts, every round of each in a fresh process per build, the builds alternating in order from
round to round; reported: the median over the rounds with their min - max (the run-to-run spread).

  launches   mpcd_rollout_cost_grouped on the parent build against mpcd_rollout_cost_box on this build, and mpcd_topk
             against mpcd_topk_feasible at k = 1 and 8, for double_int2d, H = 32, at 1 x 4,096 and 64 x 64 (states x
             candidates). This build's process times its own mpcd_rollout_cost_grouped / mpcd_topk too (the same kernels
             as the parent's: how far two builds of one kernel lie apart). HIP events: --reps back-to-back launches
             between one event pair, per launch (what a stream of dependent launches pays), and the median of --reps
             single launches each between its own pair. A launch this short is bounded below by the host's issue rate,
             the same on both sides.
  step       the composed control step of closed_loop per iteration after the sampler, on this build: rollout_cost_grouped +
             control_step against rollout_cost_box + topk_feasible + control_step_picked, back to back as above: the cost
             of constraints per control step.
  bench      `bench.py --gpus 1 --workload cfg2 --dump-outputs` in the parent's tree and in this one, alternating: the
             JSON line's value per round, and whether every dumped array is byte-identical between the two builds. Read
             the difference of the medians against the parent's own min - max.

The parent build is a checkout of the parent commit with its library built (--parent-tree); its libmpcd.so has none of
the new entry points, so the launches worker drops their bindings before loading it (MPCD_LIB).

    python tools/state_box_ab.py --parent-tree DIR [--rounds 5] [--reps 200] [--steps 50] [--warmup 20] [--json FILE]
"""
import argparse
import ctypes
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpcd_rollout_cost_box", "mpcd_topk_feasible", "mpcd_control_step_picked")
SHAPES = ((1, 4096), (64, 64))


def worker(a):
    """one round in this process, with whichever library MPCD_LIB names: a JSON line {name: [back-to-back us, single us]}"""
    import numpy as np
    import torch

    from mpc_via_diffusion_model_amd import _native as nat
    this = a.worker == "this"
    if not this:
        for name in NEW:
            nat.EXPORTS.pop(name, None)
    from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, systems
    from oracle import nets

    H, d, C = 32, 2, 4
    torch.manual_seed(0)
    net = nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C).eval()
    plan = DiffusionMPC(NetSpec("mlp", d, H, C, dtype="f32x3"), net.state_dict(), n_diffusion_steps=25,
                        action_limits=(np.full(d, -3.0), np.full(d, 2.0)))
    sysm, L, ctx, st = systems.double_int2d(), plan._lib, plan._ctx, plan._stream()
    desc = sysm.desc()
    umin, umax = plan.act_min.ctypes.data, plan.act_max.ctypes.data
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rng = np.random.default_rng(0)
    out = {}

    def timed(name, fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
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
        out[name] = [e0.elapsed_time(e1) * 1e3 / a.reps, statistics.median(single)]

    for M, n in SHAPES:
        B, tag = M * n, f"{M} x {n}"
        u = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, H, d)).astype(np.float32)).cuda()
        x = torch.from_numpy(rng.uniform(-0.5, 0.5, (M, 4))).cuda()
        x_step = x.clone()
        flags = torch.zeros(M, dtype=torch.int32, device="cuda")
        cost = torch.empty(B, dtype=torch.float64, device="cuda")
        viol = torch.zeros(B, dtype=torch.float64, device="cuda")
        raw = torch.empty((M, 8, 2), dtype=torch.int64, device="cuda")
        vk = torch.empty((M, 8), dtype=torch.float64, device="cuda")
        nf = torch.empty(M, dtype=torch.int64, device="cuda")
        ua = torch.empty((M, d), dtype=torch.float64, device="cuda")
        ia = torch.empty(M, dtype=torch.int64, device="cuda")
        ca = torch.empty(M, dtype=torch.float64, device="cuda")

        def grouped():
            L.mpcd_rollout_cost_grouped(ctx, ctypes.byref(desc), p(x), n, p(u), umin, umax, B, H, p(flags), p(cost), st)

        timed(f"rollout_cost_grouped {tag}", grouped)
        if this:
            box = plan._state_box(([None, None, -0.6, -0.6], [None, None, 0.6, 0.6]), 4)

            def boxed():
                L.mpcd_rollout_cost_box(ctx, ctypes.byref(desc), p(x), n, p(u), umin, umax, B, H, p(flags), ctypes.byref(box),
                                        p(cost), p(viol), st)

            timed(f"rollout_cost_box {tag}", boxed)
        for k in (1, 8):
            timed(f"topk k={k} {tag}", lambda k=k: L.mpcd_topk(ctx, p(cost), M, n, k, 0, p(raw), st))
            if this:
                timed(f"topk_feasible k={k} {tag}",
                      lambda k=k: L.mpcd_topk_feasible(ctx, p(cost), p(viol), M, n, k, 0.0, 0, p(raw), p(vk), p(nf), st))
        if this:  # the composed control step after the sampler, per iteration (the plant state is put back each time)
            def step_today():
                x_step.copy_(x)
                grouped()
                L.mpcd_control_step(ctx, ctypes.byref(desc), p(x_step), M, n, p(u), H, p(cost), umin, umax, p(flags), 0, 4,
                                    p(ua), p(ia), p(ca), st)

            def step_box():
                x_step.copy_(x)
                boxed()
                L.mpcd_topk_feasible(ctx, p(cost), p(viol), M, n, 1, 0.0, 0, p(raw), p(vk), p(nf), st)
                L.mpcd_control_step_picked(ctx, ctypes.byref(desc), p(x_step), M, p(u), B, H, p(raw), 1, 0, umin, umax,
                                           p(flags), 4, p(ua), p(ia), p(ca), st)

            timed(f"step: grouped + control_step {tag}", step_today)
            timed(f"step: box + topk_feasible + picked {tag}", step_box)
    print("STATE_BOX_AB " + json.dumps({"us": out, "device": torch.cuda.get_device_name(0)}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libmpcd.so built")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="launches per event timing")
    ap.add_argument("--steps", type=int, default=50, help="bench.py --steps")
    ap.add_argument("--warmup", type=int, default=20, help="bench.py --warmup")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", default=None, choices=("this", "parent"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.worker:
        return worker(a)
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    parent_lib = os.path.join(parent, "mpc_via_diffusion_model_amd", "libmpcd.so") if parent else None
    if parent and not os.path.exists(parent_lib):
        raise SystemExit(f"{parent_lib} is missing: build the parent's library first")
    builds = ["this"] + (["parent"] if parent else [])

    def launches(which):
        env = dict(os.environ)
        env.pop("MPCD_LIB", None)
        if which == "parent":
            env["MPCD_LIB"] = parent_lib
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--reps", str(a.reps)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STATE_BOX_AB ")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"{which} worker failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(lines[-1][len("STATE_BOX_AB "):])

    def bench(which, dump):
        tree = parent if which == "parent" else ROOT
        env = dict(os.environ)
        env.pop("MPCD_LIB", None)
        cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--workload", "cfg2", "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--dump-outputs", dump]
        r = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"{which} bench.py failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        return json.loads(lines[-1])

    us, values, device, unit, identical = {}, {}, None, None, None
    work = tempfile.mkdtemp(prefix="state_box_ab_")
    try:
        for rnd in range(a.rounds):
            order = builds[::-1] if rnd % 2 else builds
            for which in order:
                r = launches(which)
                device = r["device"]
                for name, v in r["us"].items():
                    us.setdefault(f"{which}: {name}", []).append(v)
            if a.no_bench:
                continue
            for which in order:
                dump = os.path.join(work, f"{which}_{rnd}")
                line = bench(which, dump)
                unit = line.get("unit")
                values.setdefault(which, []).append(line["value"])
            if parent:
                da, db = os.path.join(work, f"this_{rnd}"), os.path.join(work, f"parent_{rnd}")
                names = sorted(os.listdir(da))
                same = names == sorted(os.listdir(db)) and len(names) > 0 and all(
                    filecmp.cmp(os.path.join(da, f), os.path.join(db, f), shallow=False) for f in names)
                identical = same if identical is None else (identical and same)
                if not same:
                    print(f"round {rnd}: bench.py outputs DIFFER between the builds ({names})")
    finally:
        shutil.rmtree(work, ignore_errors=True)

    print(f"device {device}; {a.rounds} rounds, one fresh process per build and round; double_int2d, H = 32, d = 2")
    print(f"\nmicroseconds per launch (or per composed step), HIP events, {a.reps} launches per timing")
    print(f"{'build: call, states x candidates':58s} {'back to back median':>20s} {'min':>8s} {'max':>8s} "
          f"{'single median':>14s} {'min':>8s} {'max':>8s}")
    res = {"device": device, "rounds": a.rounds, "reps": a.reps, "us": {}, "bench": {}}
    for k in sorted(us, key=lambda s: (s.split(": ", 1)[1].rsplit(" ", 3)[-3:], s.split(": ", 1)[1], s)):
        b2b, single = [v[0] for v in us[k]], [v[1] for v in us[k]]
        res["us"][k] = {"back_to_back": b2b, "single": single}
        print(f"{k:58s} {statistics.median(b2b):20.2f} {min(b2b):8.2f} {max(b2b):8.2f} {statistics.median(single):14.2f} "
              f"{min(single):8.2f} {max(single):8.2f}")
    if values:
        print(f"\nbench.py --gpus 1 --workload cfg2 --steps {a.steps} --warmup {a.warmup}: value ({unit}) per round")
        for which in builds:
            v = values[which]
            res["bench"][which] = v
            print(f"{which:8s} median {statistics.median(v):14.1f}  min {min(v):14.1f}  max {max(v):14.1f}  "
                  f"spread {100 * (max(v) - min(v)) / statistics.median(v):5.2f} %  rounds {' '.join(f'{x:.1f}' for x in v)}")
        if parent:
            dm = statistics.median(values["this"]) / statistics.median(values["parent"]) - 1
            res["bench"]["outputs_identical"] = identical
            print(f"this / parent - 1 = {100 * dm:+.2f} % of the medians; dumped outputs byte-identical in every round: "
                  f"{identical}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0 if identical in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
