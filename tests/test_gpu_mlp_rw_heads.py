"""The resident-weight MLP sampler with its layer heads moved (csrc/mlp_rw.hip: accumulator-init reads, the next
step's plan and cond tables, and several weight-fragment loads are issued before the barrier that opens their layer,
or in another layer's MFMA slots): the 8-wave form rw32x8 against the 4-wave rw32, bit for bit, on the paths where a
moved read or load can go wrong and that tests/test_gpu_mlp_rw8.py does not reach - the control step with the context
row projected in the kernel, one, two and three denoise steps (no next step to prefetch for; the loop wrapping once
and twice), a warm start, a context group with idle columns, H*d = 128 and 32, CFG-DDIM, and the 16-row rw16 kernel
(the same hidden_ilv) against the streaming 32x8. Small shapes: one full workgroup plus one candidate."""
import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import systems
from mpc_via_diffusion_model_amd.planner import force_mlp_layout

from ._util import make_mlp
from .test_gpu_mlp import _ctx, _planner

pytestmark = pytest.mark.gpu
C = 4


def _under(layouts, run):
    outs = {}
    try:
        for lay in layouts:
            force_mlp_layout(lay)
            outs[lay] = run()
            torch.cuda.synchronize()
    finally:
        force_mlp_layout("auto")
    return outs


def _same(outs, a, b, what):
    xs, ys = outs[a], outs[b]
    if torch.is_tensor(xs):
        xs, ys = [xs], [ys]
    assert len(xs) == len(ys)
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert torch.isfinite(x).all(), f"{what}: {a} result {i} is not finite"
        assert torch.equal(x, y), f"{what}: {a} differs from {b} in result {i}: max |d| {float((x - y).abs().max()):.3e}"


def _step_plan(n_steps, H=32, d=2, seed=5):
    # cosine: the exponential schedule is not finite at 2, 3 or 20 steps
    return _planner(make_mlp(d, H, C, seed=seed), d, H, C, n_steps, kind="cosine", dtype="f32x3")


@pytest.mark.parametrize("n_steps", [1, 2, 3])
def test_mpc_step_fused_context_few_steps(n_steps):
    """mpc_step projects the context row in the sampler (ctx_fused). N = 1: no next step, the plan and table prefetches
    stay inside the plan; N = 2, 3: step s + 1's tables and plan are read one step after they are written."""
    B = 17
    plan = _step_plan(n_steps)
    sysm = systems.get("double_int2d")
    x0 = np.random.default_rng(1).uniform(-1, 1, C)
    outs = _under(("rw32", "rw32x8"), lambda: plan.mpc_step(x0, sysm, B, w=0.01, seed=2).u_norm.clone())
    _same(outs, "rw32x8", "rw32", f"mpc_step, B={B}, N={n_steps}")


def test_mpc_step_warm_started_at_two_steps():
    B, K = 17, 2
    plan = _step_plan(20)
    sysm = systems.get("double_int2d")
    x0 = np.random.default_rng(1).uniform(-1, 1, C)

    def run():
        plan.reset_warm_start()
        cold = plan.mpc_step(x0, sysm, B, w=0.01, seed=2, warm_start=K).u_norm.clone()  # fills the prior
        warm = plan.mpc_step(x0, sysm, B, w=0.01, seed=3, warm_start=K).u_norm.clone()  # K steps from it
        return [cold, warm]

    try:
        outs = _under(("rw32", "rw32x8"), run)
    finally:
        plan.reset_warm_start()
    _same(outs, "rw32x8", "rw32", f"mpc_step warm_start={K}, B={B}")
    assert not torch.equal(outs["rw32x8"][0], outs["rw32x8"][1])


def test_grouped_context_with_idle_columns():
    B, g, H, d = 24, 12, 32, 2
    plan = _step_plan(3)
    ctx = _ctx(B // g, C, False)
    outs = _under(("rw32", "rw32x8"), lambda: plan.sample_trajectories(ctx, B, H, seed=3, return_chain=True, context_group=g))
    _same(outs, "rw32x8", "rw32", f"context_group={g}, B={B}")


@pytest.mark.parametrize("H,what", [(64, "H*d = 128: Linear 0's fragments issued after the update, two update quads per lane"),
                                    (16, "H*d = 32: two n-tiles in the final layer, waves 2-3 idle there")])
def test_other_widths_three_steps(H, what):
    B, d = 17, 2
    plan = _step_plan(3, H=H)
    ctx = _ctx(B, C, True)
    outs = _under(("rw32", "rw32x8"), lambda: plan.sample_trajectories(ctx, B, H, seed=3, return_chain=True))
    _same(outs, "rw32x8", "rw32", what)


def test_cfg_ddim_three_steps():
    B, H, d = 33, 32, 2
    plan = _step_plan(3)
    ctx = _ctx(B, C, True)
    outs = _under(("rw32", "rw32x8"), lambda: plan.sample_trajectories(ctx, B, H, seed=3, sample_fn="ddim_cfg"))
    _same(outs, "rw32x8", "rw32", f"ddim_cfg, B={B}, N=3")


def test_rw16_against_streaming_kernel():
    B, H, d = 8, 32, 2
    plan = _step_plan(3)
    ctx = _ctx(B, C, True)
    outs = _under(("32x8", "rw16"), lambda: plan.sample_trajectories(ctx, B, H, seed=3, return_chain=True))
    _same(outs, "rw16", "32x8", f"rw16, B={B}, H={H}")
