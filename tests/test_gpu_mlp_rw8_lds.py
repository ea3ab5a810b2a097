"""The 8-wave resident-weight MLP sampler (layout "rw32x8") with its own LDS layout (csrc/mlp_rw.hip, Lds8): the x
planes share storage with the 256-wide concat buffer, the fp32 x_T with the first activation buffer, and the trailing
k-chunks of Linear 8's weights are staged in LDS once per launch and read from there in every step. No sum and no order
of products changes, so every result is compared bit for bit with the 4-wave rw32 and the streaming 32x8 kernels. What
can go wrong: the aliased buffers (x carried across steps), the staging (stale, or from another planner's pack) and the
instantiations with another amount of LDS room; none of it needs a large batch."""
import pytest
import torch

from oracle import sampler as osam
from oracle import schedule as osch

from ._util import assert_traj_close, make_mlp
from .test_gpu_mlp import _ctx, _planner

C, N = 4, 20
LAYOUTS = ("32x8", "rw32", "rw32x8")


def _under(layouts, run):
    from mpc_via_diffusion_model_amd.planner import force_mlp_layout
    outs = {}
    try:
        for lay in layouts:
            force_mlp_layout(lay)
            outs[lay] = run()
            torch.cuda.synchronize()
    finally:
        force_mlp_layout("auto")
    return outs


def _assert_same(outs, what):
    new = outs["rw32x8"]
    assert torch.isfinite(new).all(), what
    for lay in outs:
        if lay != "rw32x8":
            assert torch.equal(new, outs[lay]), f"rw32x8 differs from {lay} ({what}): max |d| {float((new - outs[lay]).abs().max()):.3e}"


# B = 17: one full workgroup plus one candidate; the chain shows x after every step, carried in the aliased S1.
# ddim (3-arg net): one branch, 32 candidates per workgroup, the fp32 x kept in LDS; at H = 32 no k-chunk is resident, at
# H = 16 three are. H = 64: H*d = 128, none resident. H = 16: H*d = 32.
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,mode", [(17, 32, "ddpm_nwo_chain"), (33, 32, "ddim_cfg"), (48, 32, "ddim"), (40, 64, "ddpm"),
                                      (100, 16, "ddpm"), (17, 32, "ddpm_noise"), (48, 16, "ddim")])
def test_bit_identical_to_rw32_and_32x8(B, H, mode):
    d = 2
    net = make_mlp(d, H, C, seed=5)
    plan = _planner(net, d, H, C, N, kind="cosine", cfg=mode != "ddim", dtype="f32x3")
    ctx = _ctx(B, C, True)
    noise = torch.randn(N + 1, B, H, d, generator=torch.Generator().manual_seed(11))

    def run():
        if mode == "ddpm_nwo_chain":
            return plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, return_chain=True,
                                n_diffusion_steps_without_noise=5, seed=3)
        if mode == "ddpm":
            return plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, seed=3)
        if mode == "ddpm_noise":
            return plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, return_chain=True, noise=noise)
        return plan.sample_trajectories(ctx, B, H, seed=3, sample_fn=mode)

    _assert_same(_under(LAYOUTS, run), f"{mode}, B={B}, H={H}")


@pytest.mark.gpu
def test_eps_both_branches_bit_identical():
    """One evaluation: the staging followed by a single pass."""
    B, H, d = 40, 32, 2
    plan = _planner(make_mlp(d, H, C, seed=12), d, H, C, N, kind="cosine", dtype="f32x3")
    x = torch.randn(B, H, d, generator=torch.Generator().manual_seed(1))
    ctx = _ctx(B, C, True)
    outs = _under(LAYOUTS, lambda: torch.stack(plan.eps(x, 7, ctx)))
    _assert_same(outs, "plan.eps, both branches")
    assert not torch.equal(outs["rw32x8"][0], outs["rw32x8"][1])


@pytest.mark.gpu
def test_grouped_three_ragged_groups_bit_identical():
    """Groups of 5, 16 and 23 candidates: less than, exactly and more than a workgroup's 16."""
    H, d = 32, 2
    plan = _planner(make_mlp(d, H, C, seed=8), d, H, C, N, kind="cosine", dtype="f32x3")
    for g in (5, 16, 23):
        ctx = _ctx(3, C, False, seed=g)
        outs = _under(LAYOUTS, lambda: plan.sample_trajectories(ctx, 3 * g, H, seed=3, context_group=g, n_wo_noise=2))
        _assert_same(outs, f"sample_grouped, 3 groups of {g}")


@pytest.mark.gpu
def test_warm_start_bit_identical():
    B, H, d, K = 21, 32, 2, 8
    plan = _planner(make_mlp(d, H, C, seed=9), d, H, C, N, kind="cosine", dtype="f32x3")
    ctx = _ctx(B, C, True)
    prior = torch.rand(1, H, d, generator=torch.Generator().manual_seed(2)) * 2 - 1
    outs = _under(LAYOUTS, lambda: plan.sample_trajectories(ctx, B, H, seed=4, n_wo_noise=1, x_init=prior, t_start=K,
                                                            return_chain=True))
    assert outs["rw32x8"].shape[0] == K + 1 + 1
    _assert_same(outs, f"warm start, t_start={K}")


@pytest.mark.gpu
def test_consecutive_calls_and_two_planners():
    """Two calls on one planner with different seeds, and two planners with different weights sampled alternately:
    each call's staged weights are its own pack's."""
    B, H, d = 19, 32, 2
    ctx = _ctx(B, C, True)
    plans = [_planner(make_mlp(d, H, C, seed=s), d, H, C, N, kind="cosine", dtype="f32x3") for s in (5, 6)]

    def run():
        a = [plans[0].sample_trajectories(ctx, B, H, seed=s) for s in (1, 2)]
        b = [plans[i % 2].sample_trajectories(ctx, B, H, seed=7) for i in range(4)]
        return torch.stack(a + b)

    outs = _under(("rw32", "rw32x8"), run)
    _assert_same(outs, "two seeds, then two planners alternately")
    new = outs["rw32x8"]
    assert not torch.equal(new[0], new[1]), "two seeds"
    assert not torch.equal(new[2], new[3]), "two nets"
    assert torch.equal(new[2], new[4]) and torch.equal(new[3], new[5]), "a planner's result does not depend on the call before it"


@pytest.mark.gpu
def test_matches_oracle_at_the_cfg1_shape():
    B, H, d, n = 64, 16, 2, 50
    net = make_mlp(d, H, C)
    plan = _planner(net, d, H, C, n, dtype="f32x3")
    ctx = _ctx(B, C, True)
    noise = torch.randn(n + 1, B, H, d, generator=torch.Generator().manual_seed(11))
    ref = osam.ddpm_cfg(net, osch.buffers("exponential", n), ctx.expand(B, C), 0.01, B, H, 0, noise=noise, return_chain=True)
    got = _under(("rw32x8",), lambda: plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, return_chain=True,
                                                    n_diffusion_steps_without_noise=0, noise=noise))["rw32x8"]
    assert_traj_close(got, ref, what="ddpm chain, layout rw32x8 (Lds8), B=64")
