"""The training step's loss and every gradient tensor where gemm_mfma_kernel's guards matter: M, N and K that are
no multiple of the 64-wide tile or the 16-deep k-step, a single row, one row past a tile, split-K slices that end
inside a k-step (with the bias-gradient row sums taken from those same tiles), the 4-level U-Net trunk (GroupNorm,
the stride-2 conv and the k=4 transposed conv at L = 2), N = 1000 diffusion steps, and one trainer re-used across
batch sizes (Trainer::reserve's free-and-reallocate path and its reuse for a smaller batch).

Reference: the oracle's autograd with every Linear / Conv / ConvTranspose / GroupNorm computing in fp64
(_util.oracle_fp64_layers, the perturbation oracle_sensitivity applies). Bars: loss 1e-5 relative; per gradient
tensor ||got - ref|| <= 1e-4 ||ref|| and max|got - ref| <= ABS_ELEM max|ref|; a tensor whose reference gradient
is exactly zero must be exactly zero. The fp32 oracle itself sits 2e-7 .. 3.5e-6 (norm) and 4e-7 .. 4e-6
(elementwise) from this reference at these shapes, measured on the CPU."""
import math

import pytest
import torch

from mpc_via_diffusion_model_amd import NetSpec
from mpc_via_diffusion_model_amd.training import DiffusionTrainer
from oracle import layers as olayers
from oracle import nets
from oracle import schedule as osch

from ._train_util import REL_GRAD, REL_LOSS, _assert_grads, _errors, _inputs, _oracle_grads
from ._util import ABS_ELEM, SPREAD_X

pytestmark = pytest.mark.gpu


def _net(kind, d, H, C, base, mults, seed=0):
    torch.manual_seed(seed)
    if kind == "mlp":
        return nets.ConditionedMLPNet(state_dim=d, horizon=H, context_dim=C, dim=base, dim_mults=mults).train()
    return nets.ConditionedTemporalUnet(state_dim=d, context_dim=C, unet_input_dim=base, dim_mults=mults).train()


CASES = [
    ("mlp", 3, 10, 3, 37, 24, (1, 2, 4)),    # flat 30, widths 24 / 48 / 96: every M, N, K ragged
    ("mlp", 2, 32, 4, 1, 32, (1, 2, 4)),     # a single row
    ("mlp", 2, 32, 4, 65, 32, (1, 2, 4)),    # one row in the second row tile
    ("mlp", 2, 32, 4, 513, 32, (1, 2, 4)),   # split K: two slices, the last ends inside a k-step
    ("mlp", 2, 32, 4, 1000, 32, (1, 2, 4)),  # split K with K % 16 = 8
    ("unet", 1, 32, 5, 1, 32, (1, 2, 4)),    # a single row through the U-Net tape
    ("unet", 1, 32, 5, 65, 32, (1, 2, 4)),   # deepest convs: K = 65 * 8 = 520, split K with a ragged last slice
    ("unet", 2, 16, 4, 5, 32, (1, 2, 4, 8)),  # four levels, L down to 2
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-d{c[1]}H{c[2]}C{c[3]}-B{c[4]}-base{c[5]}x{len(c[6])}")
def test_loss_and_grads_at_ragged_shapes(case):
    kind, d, H, C, B, base, mults = case
    net = _net(kind, d, H, C, base, mults)
    tables = osch.buffers("exponential", 100)
    batch = _inputs(d, H, C, B, 100, seed=31)
    ref_loss, ref = _oracle_grads(net, tables, batch)
    tr = DiffusionTrainer(NetSpec(kind, d, H, C, base_dim=base, dim_mults=mults), net.state_dict(), tables=tables)
    got = tr.loss(*batch)
    assert abs(got - ref_loss) <= REL_LOSS * abs(ref_loss), (got, ref_loss)
    got = tr.train_step(*batch)
    assert abs(got - ref_loss) <= REL_LOSS * abs(ref_loss), (got, ref_loss)
    print(f"{case}: loss rel err {abs(got - ref_loss) / abs(ref_loss):.3e}")
    _assert_grads(tr.state_dict("grads"), ref, str(case))


def _sinemb_one_ulp(self, t):
    """SinusoidalPosEmb.forward with every frequency moved one fp32 ulp up"""
    half = self.dim // 2
    step = math.log(10000) / (half - 1)
    freqs = torch.exp(torch.arange(half, device=t.device) * -step)
    freqs = torch.nextafter(freqs, torch.full_like(freqs, float("inf")))
    arg = t[:, None] * freqs[None, :]
    return torch.cat((arg.sin(), arg.cos()), dim=-1)


@pytest.mark.parametrize("kind,shape", [("mlp", (2, 32, 4, 64)), ("unet", (1, 32, 5, 16))])
def test_n1000_timestep_embedding(kind, shape):
    """N = 1000 (the ordinary DDPM length), t from the top tenth and at 0, 1, 500, 998, 999: sinf / cosf of
    arguments up to 999, where one ulp of a frequency is 999 ulps of the argument. Bar per tensor:
    max(1e-4, SPREAD_X s), s = the fp32 oracle's own norm-relative change of that tensor when the embedding's
    frequencies move one fp32 ulp (at most 3.5e-5 for the MLP and 2.1e-5 for the U-Net, so the 1e-4 term governs)."""
    d, H, C, B = shape
    net = _net(kind, d, H, C, 32, (1, 2, 4))
    tables = osch.buffers("exponential", 1000)
    x0, ctx, t, noise, mask = _inputs(d, H, C, B, 1000, seed=32, top_tenth=True)
    t[:5] = torch.tensor([0, 1, 500, 998, 999])
    batch = (x0, ctx, t, noise, mask)
    ref_loss, ref = _oracle_grads(net, tables, batch)
    _, g0 = _oracle_grads(net, tables, batch, fp64=False)
    saved = olayers.SinusoidalPosEmb.forward
    olayers.SinusoidalPosEmb.forward = _sinemb_one_ulp
    try:
        _, g1 = _oracle_grads(net, tables, batch, fp64=False)
    finally:
        olayers.SinusoidalPosEmb.forward = saved
    s = {n: float((g1[n].double() - g0[n].double()).norm() / g0[n].double().norm().clamp_min(1e-300)) for n in g0}
    bars = {n: (max(REL_GRAD, SPREAD_X * s[n]), max(ABS_ELEM, SPREAD_X * s[n])) for n in s}
    tr = DiffusionTrainer(NetSpec(kind, d, H, C), net.state_dict(), tables=tables)
    got = tr.train_step(*batch)
    assert abs(got - ref_loss) <= REL_LOSS * abs(ref_loss), (got, ref_loss)
    grads = tr.state_dict("grads")
    errs = _errors(grads, ref)
    ratio = max(e[0] / max(s[n], 1e-30) for n, e in errs.items())
    print(f"N=1000 {kind}: s (one-ulp frequency spread of the fp32 oracle) max {max(s.values()):.3e}, "
          f"device worst error / s {ratio:.3f}, loss rel err {abs(got - ref_loss) / abs(ref_loss):.3e}")
    _assert_grads(grads, ref, f"N=1000 {kind}", bars=bars)


@pytest.mark.parametrize("kind,shape", [("mlp", (2, 32, 4)), ("unet", (1, 32, 5))])
def test_one_trainer_across_batch_sizes(kind, shape):
    """One trainer (lr = 0: Adam must leave every weight bit-identical) stepped at B = 96, 192, 8, 192: growth frees
    and reallocates every activation buffer, the smaller batch runs in the larger buffers, and the split-K
    workspace grows with the batch. Each step's gradients == a fresh trainer's first step at that B on the same
    inputs, bit for bit; the first step's also meet the oracle bars."""
    d, H, C = shape
    net = _net(kind, d, H, C, 32, (1, 2, 4))
    tables = osch.buffers("exponential", 100)
    spec = NetSpec(kind, d, H, C)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    tr = DiffusionTrainer(spec, sd, tables=tables, lr=0.0)
    p0 = tr.state_dict("params")
    for i, B in enumerate((96, 192, 8, 192)):
        batch = _inputs(d, H, C, B, 100, seed=40 + i)
        loss = tr.train_step(*batch)
        grads = tr.state_dict("grads")
        fresh = DiffusionTrainer(spec, sd, tables=tables, lr=0.0)
        assert fresh.train_step(*batch) == loss, (i, B)
        fg = fresh.state_dict("grads")
        fresh.close()
        for n in fg:
            assert torch.equal(grads[n], fg[n]), (i, B, n)
        params = tr.state_dict("params")
        for n in p0:
            assert torch.equal(params[n], p0[n]), (i, B, n)
        if i == 0:
            ref_loss, ref = _oracle_grads(net, tables, batch)
            assert abs(loss - ref_loss) <= REL_LOSS * abs(ref_loss), (loss, ref_loss)
            _assert_grads(grads, ref, f"re-used trainer {kind}, first step B={B}")
