"""GPU parity of every U-Net inference path at weights default initialisation never reaches (tests/_unet_draw.py):
a drawn GroupNorm affine (signed gamma, nonzero beta), per-conv power-of-two weight magnitudes (the two-term fp16
fused program's per-layer scales) and GroupNorm groups whose mean lies far from zero (the three ways the kernels
take the statistics: fp64 sums in csrc/unet.hip, shifted fp64 sums in csrc/unet_mx.hip, fp32 two-pass in
csrc/unet_fused.hip).

Reference: the oracle net with every Linear / Conv / ConvTranspose / GroupNorm in fp64 (_util.oracle_fp64_layers).
Bars, unchanged from tests/test_gpu_unet.py and tests/test_gpu_unet_fused.py: eps error <= 2e-5 of max(|eps| max, 1)
for f32, f32x3 and f16x2, 2e-2 for f16. tests/test_unet_draw_host.py shows on the CPU that each slip of the affine
moves eps by 0.37 .. 1.6 at these draws, and that the fp32 oracle sits within 2.0e-6 (1/10 of the bar) of the
reference at every case below.

The offsets-10 case has no fixed bar: at group offsets of amplitude 10 the fp32 oracle's own distance s from the
fp64-layer oracle comes near the bar (measured on the CPU per evaluation at d1 H32: 5.7e-6 .. 7.2e-6), so the bar
is max(2e-5, SPREAD_X s), s taken per evaluation from the reference pair, never from the kernel."""
import functools

import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, force_unet_path
from oracle import sampler as osam
from oracle import schedule as osch

from . import _unet_draw as D
from ._util import SPREAD_X, assert_traj_close, oracle_fp64_layers, oracle_sensitivity

pytestmark = pytest.mark.gpu

PLANES = {"f32": 0, "f32x3": 3, "f16": 1, "f16x2": 3}        # layered: an f16x2 net runs the split-bf16 kernels
FUSED_PLANES = {"f32x3": 3, "f16": 1, "f16x2": 2}
# rows per fused workgroup (csrc/unet_fused.hip kCfgs): B = 3 at H = 32 leaves a workgroup part empty, d4 H64 runs
# two rows and d7 H128 one row per workgroup in the fp32-accurate forms, ops spanning several waves per row
FUSED_ROWS = {("f16", 32): 8, ("f16", 64): 2, ("f16", 128): 2, ("f32x3", 32): 4, ("f32x3", 64): 2, ("f32x3", 128): 1,
              ("f16x2", 32): 4, ("f16x2", 64): 2, ("f16x2", 128): 1}


@pytest.fixture(autouse=True)
def _auto_path_afterwards():
    yield
    force_unet_path("auto")


@functools.lru_cache(maxsize=None)
def _reference(case, draw):
    """per evaluation: (label, x, t, ctx, fp64-layer eps, fp32 oracle's distance s from it), computed once per case"""
    net = D.case_net(case, draw)
    out = []
    for lab, x, t, ctx in D.case_evals(case):
        own = D.oracle_eps(net, case, x, t, ctx)
        with oracle_fp64_layers():
            ref = D.oracle_eps(net, case, x, t, ctx)
        out.append((lab, x, t, ctx, ref, tuple(D.eps_err(o, r) for o, r in zip(own, ref))))
    return net, out


def _planner(net, case, dtype):
    cfg, d, H, C, B, mults, _ = D.FWD_CASES[case]
    spec = NetSpec("unet", state_dim=d, horizon=H, context_dim=C, cfg=cfg, dim_mults=mults, dtype=dtype)
    return DiffusionMPC(spec, net.state_dict(), variance_schedule="exponential", n_diffusion_steps=D.case_steps(case))


def _force(plan, path, dtype, H):
    """force the path and confirm through unet_form() that it is the one an eps call takes"""
    force_unet_path(path)
    form = plan.unet_form()
    if path == "fused":
        assert form["fused"] and form["planes"] == FUSED_PLANES[dtype], form
        assert form["rows_per_workgroup"] == FUSED_ROWS[(dtype, H)], form
    else:
        assert not form["fused"] and form["planes"] == PLANES[dtype], form


def _run(plan, case, evals, what, bar_of):
    """eps of every evaluation; asserts each branch against its bar; returns ([eps...], worst error, worst err / s)"""
    outs, worst, ratio = [], 0.0, 0.0
    for lab, x, t, ctx, ref, s in evals:
        got = [e for e in plan.eps(x, t, ctx) if e is not None]
        assert len(got) == len(ref)
        for g, r, s_, br in zip(got, ref, s, ("cond", "uncond")):
            assert torch.isfinite(g).all(), (what, lab, br)
            e = D.eps_err(g, r)
            worst, ratio = max(worst, e), max(ratio, e / max(s_, 1e-30))
            assert e <= bar_of(s_), f"{what} {lab} {br}: eps err {e:.3e} (bar {bar_of(s_):.1e}, oracle's own {s_:.1e})"
        outs += got
    return outs, worst, ratio


def _params():
    out = []
    for case, (cfg, d, H, C, B, mults, fused) in D.FWD_CASES.items():
        kinds = ["f32", "f32x3"] if not cfg else ["f32", "f32x3", "f16"] + (["f16x2"] if fused else [])
        out += [(case, draw, k) for draw in D.FIXED_BAR_DRAWS for k in kinds]
    return out


@pytest.mark.parametrize("case,draw,dtype", _params(), ids=lambda v: str(v))
def test_eps_at_drawn_weights(case, draw, dtype):
    """Both CFG branches, a shared and a per-candidate context, t = 0 and t = N - 1, through the layered kernels of
    the dtype and, where the fused program covers the net, through it too; the two agree within the same bar."""
    cfg, d, H, C, B, mults, covered = D.FWD_CASES[case]
    net, evals = _reference(case, draw)
    bar = D.EPS_BAR_F16 if dtype == "f16" else D.EPS_BAR
    plan = _planner(net, case, dtype)
    res = {}
    paths = ["layered"] + (["fused"] if covered and dtype != "f32" else [])
    for path in paths:
        _force(plan, path, dtype, H)
        res[path] = _run(plan, case, evals, f"{case} {draw} {dtype} {path}", lambda s: bar)
        print(f"{case} {draw} {dtype} {path}: worst eps err {res[path][1]:.3e} (bar {bar:g})")
    if len(res) == 2:
        agree = max(D.eps_err(a, b.cpu()) for a, b in zip(res["fused"][0], res["layered"][0]))
        print(f"{case} {draw} {dtype}: fused against layered {agree:.3e}")
        assert agree <= bar, (case, draw, dtype, agree)
    plan.close()


@pytest.mark.parametrize("dtype,path", [("f32", "layered"), ("f32x3", "layered"), ("f32x3", "fused"), ("f16x2", "fused")])
def test_eps_at_group_offsets_of_ten(dtype, path):
    """affine + offsets 10 at d1 H32: |group mean| up to 10 standard deviations of the conv's own output. Bar per
    evaluation max(2e-5, SPREAD_X s), s = the fp32 oracle's distance from the fp64-layer oracle there (CPU:
    5.7e-6 .. 7.2e-6 at this seed: SPREAD_X s is 1.7e-5 .. 2.2e-5, the bar 2.0e-5 .. 2.2e-5). Measured on the
    MI355X: error / s 0.34 (f32), 1.48 (layered f32x3), 0.33 (fused f32x3), 0.30 (fused f16x2)."""
    case, draw = D.OFFSET10_CASE, "affine+offsets10"
    H = D.FWD_CASES[case][2]
    net, evals = _reference(case, draw)
    plan = _planner(net, case, dtype)
    _force(plan, path, dtype, H)
    _, worst, ratio = _run(plan, case, evals, f"{case} {draw} {dtype} {path}", lambda s: max(D.EPS_BAR, SPREAD_X * s))
    smin, smax = min(min(e[5]) for e in evals), max(max(e[5]) for e in evals)
    print(f"{case} {draw} {dtype} {path}: worst eps err {worst:.3e}, worst err / s {ratio:.3f} "
          f"(s {smin:.2e} .. {smax:.2e})")
    plan.close()


@functools.lru_cache(maxsize=None)
def _chain_reference():
    case, draw = "d1H32C5-B3", "affine+scales"
    d, H, C = D.FWD_CASES[case][1:4]
    B, N, nwo = 4, 25, 5
    net = D.case_net(case, draw)
    g = torch.Generator().manual_seed(77)
    ctx = torch.rand(1, C, generator=g) * 2 - 1
    noise = torch.randn(N + nwo + 1, B, H, d, generator=g)
    ref, spread = oracle_sensitivity(lambda: osam.ddpm_cfg(net, osch.buffers("exponential", N), ctx.expand(B, C), 0.01,
                                                           B, H, n_wo_noise=nwo, noise=noise, return_chain=True))
    return net, ctx, noise, ref, spread


@pytest.mark.parametrize("dtype,path", [("f32", "layered"), ("f32x3", "fused"), ("f16x2", "fused")])
def test_cfg_ddpm_chain_at_scaled_weights(dtype, path):
    """The per-conv 2^k magnitudes through the sampler's own launch path (the per-step fused launches, the layered
    step loop), not mpcd_eps only: CFG-DDPM, N = 25 and 5 noise-free steps, B = 4, injected noise, the whole chain at
    the 1e-4 trajectory bar and max(1e-4, SPREAD_X x the oracle's own spread) elementwise, as the Panda test has it
    (the spread is 8.4e-7 .. 1.0e-6 on the CPU: the 1e-4 term governs)."""
    B, N, nwo, H = 4, 25, 5, 32
    net, ctx, noise, ref, spread = _chain_reference()
    plan = DiffusionMPC(NetSpec("unet", state_dim=1, horizon=H, context_dim=5, dtype=dtype), net.state_dict(),
                        variance_schedule="exponential", n_diffusion_steps=N)
    _force(plan, path, dtype, H)
    got = plan.run_CFG(ctx, None, 0.01, n_samples=B, horizon=H, return_chain=True, noise=noise,
                       n_diffusion_steps_without_noise=nwo)
    assert tuple(got.shape) == (N + nwo + 1, B, H, 1)
    tr, el = assert_traj_close(got, ref, spread=spread, what=f"scaled-weights chain {dtype} {path}")
    print(f"scaled-weights chain {dtype} {path}: trajectory {tr:.3e}, element {el:.3e}, oracle's own spread "
          f"{float(spread):.3e}")
    plan.close()
