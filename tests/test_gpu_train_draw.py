"""The U-Net training step at a drawn GroupNorm affine (tests/_unet_draw.py). Every other U-Net training test starts
from torch's initialisation, gamma = 1 and beta = 0, where gn_bwd_kernel's d = dy[e] * w[c] (csrc/train.hip) could
lose or misplace gamma and every gradient would still sit 2e-6 from the reference; at the drawn affine the same slip
puts 144 of 148 gradient tensors over the bar while the loss moves by 1e-7 (tests/test_unet_draw_host.py).

Reference, helpers and bars are those of tests/test_gpu_train_shapes.py: the oracle's autograd with fp64 layers; loss
1e-5 relative; per gradient tensor ||got - ref|| <= 1e-4 ||ref|| and max|got - ref| <= ABS_ELEM max|ref|; a tensor
whose reference gradient is exactly zero must be exactly zero. The fp32 oracle itself sits within 3.9e-6 (norm) and
6.1e-6 (elementwise) of the reference at these cases (CPU, test_training_cases_are_well_conditioned)."""
import pytest
import torch

from mpc_via_diffusion_model_amd import DiffusionMPC, NetSpec, force_unet_path
from mpc_via_diffusion_model_amd.training import DiffusionTrainer
from oracle import schedule as osch
from oracle.layers import Conv1dBlock

from . import _unet_draw as D
from ._train_util import REL_LOSS, _assert_grads, _errors, _inputs, _oracle_grads
from ._util import oracle_fp64_layers

pytestmark = pytest.mark.gpu


def _named_worst(grads, ref, what):
    """the worst GroupNorm weight / bias gradients and the worst gradient upstream of a GroupNorm (its conv's)"""
    errs = _errors(grads, ref)
    for label, key in (("GroupNorm weight", ".block.2.weight"), ("GroupNorm bias", ".block.2.bias"),
                       ("conv weight upstream of a GroupNorm", ".block.0.weight"),
                       ("conv bias upstream of a GroupNorm", ".block.0.bias")):
        sel = [(e[0], n) for n, e in errs.items() if n.endswith(key)]
        assert sel, key
        w = max(sel)
        print(f"{what}: worst {label} gradient norm-rel {w[0]:.3e} ({w[1]}) of {len(sel)}")


@pytest.mark.parametrize("draw", D.TRAIN_DRAWS)
@pytest.mark.parametrize("case", sorted(D.TRAIN_CASES))
def test_loss_and_grads_at_drawn_affine(case, draw):
    d, H, C, B, mults = D.TRAIN_CASES[case]
    net = D.train_net(case, draw)
    tables = osch.buffers("exponential", 100)
    batch = _inputs(d, H, C, B, 100, seed=D.TRAIN_INPUT_SEED)
    assert 0 < float(batch[4].sum()) < B  # a drawn context mask: some rows keep their context, some lose it
    ref_loss, ref = _oracle_grads(net, tables, batch)
    tr = DiffusionTrainer(NetSpec("unet", d, H, C, base_dim=32, dim_mults=mults), net.state_dict(), tables=tables)
    got = tr.loss(*batch)
    assert abs(got - ref_loss) <= REL_LOSS * abs(ref_loss), (got, ref_loss)
    got = tr.train_step(*batch)
    assert abs(got - ref_loss) <= REL_LOSS * abs(ref_loss), (got, ref_loss)
    what = f"{case} {draw}"
    print(f"{what}: loss rel err {abs(got - ref_loss) / abs(ref_loss):.3e}")
    grads = tr.state_dict("grads")
    tr.close()
    _named_worst(grads, ref, what)
    _assert_grads(grads, ref, what)


def test_three_steps_then_the_ema_weights_through_the_sampler():
    """Three Adam steps (lr = 1e-3; EMA blending from the first step on) at d1 H32. Each step's gradients against the
    oracle's at the device's own current parameters (downloaded and loaded into the oracle net, so the steps do not
    compound). Then the trainer's EMA weights - gamma and beta that went through adam_kernel and ema_kernel - into
    a DiffusionMPC: one eps forward per inference kernel family against the oracle with those weights, 2e-5."""
    case, draw = "d1H32C5-B5", "affine"
    d, H, C, B, mults = D.TRAIN_CASES[case]
    net = D.train_net(case, draw)
    start = {k: v.clone() for k, v in net.state_dict().items()}
    tables = osch.buffers("exponential", 100)
    tr = DiffusionTrainer(NetSpec("unet", d, H, C, base_dim=32, dim_mults=mults), start, tables=tables, lr=1e-3,
                          ema_decay=0.9, step_start_ema=1, update_ema_every=1)
    for step in range(3):
        net.load_state_dict(tr.state_dict("params"), strict=True)
        batch = _inputs(d, H, C, B, 100, seed=D.TRAIN_INPUT_SEED + 10 * (step + 1))
        ref_loss, ref = _oracle_grads(net, tables, batch)
        got = tr.train_step(*batch)
        assert abs(got - ref_loss) <= REL_LOSS * abs(ref_loss), (step, got, ref_loss)
        grads = tr.state_dict("grads")
        _named_worst(grads, ref, f"step {step + 1}")
        _assert_grads(grads, ref, f"three steps at the drawn affine, step {step + 1}")
    ema, params = tr.state_dict("ema"), tr.state_dict("params")
    tr.close()
    gn = [k for k in ema if k.endswith(".block.2.weight") or k.endswith(".block.2.bias")]
    assert len(gn) == 2 * sum(isinstance(m, Conv1dBlock) for m in net.modules())
    for k in gn:  # Adam moved every gamma and beta, and the EMA is a blend, not a copy of either end
        assert bool((ema[k] != start[k]).all()) and not torch.equal(ema[k], params[k]), k
    net.load_state_dict(ema, strict=True)
    net.eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, H, d, generator=g)
    ctx = torch.rand(3, C, generator=g) * 2 - 1
    t = 17
    tt = torch.full((3,), t, dtype=torch.long)
    with oracle_fp64_layers(), torch.no_grad():
        refs = net(x, tt, ctx, torch.zeros(3, 1)), net(x, tt, ctx, torch.ones(3, 1))
    try:
        for dtype, path in (("f32", "layered"), ("f32x3", "layered"), ("f32x3", "fused"), ("f16x2", "fused")):
            plan = DiffusionMPC(NetSpec("unet", d, H, C, dtype=dtype), ema, variance_schedule="exponential",
                                n_diffusion_steps=50)
            force_unet_path(path)
            assert plan.unet_form()["fused"] == (path == "fused")
            errs = [D.eps_err(e, r) for e, r in zip(plan.eps(x, t, ctx), refs)]
            print(f"EMA weights after three steps, {dtype} {path}: eps err {max(errs):.3e}")
            assert max(errs) <= D.EPS_BAR, (dtype, path, errs)
            plan.close()
    finally:
        force_unet_path("auto")
