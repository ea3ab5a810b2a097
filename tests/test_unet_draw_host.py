"""CPU side of the U-Net weight draws (tests/_unet_draw.py): the draw itself, what it makes visible, and the
condition of the unchanged parity bars at the cases the GPU tests run.

The project applies the GroupNorm affine in five separately written places (csrc/unet.hip, two in csrc/unet_mx.hip,
csrc/unet_fused.hip, gn_fwd_kernel / gn_bwd_kernel of csrc/train.hip). The slips below restate on the oracle, by
patching nn.GroupNorm.forward, what a wrong operand or index at one of those sites computes. At torch's default
initialisation (gamma = 1, beta = 0) each of them is invisible; at the `affine` draw each moves the result by at
least 100 times the bar the GPU tests hold the kernels to."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import schedule as osch
from oracle.layers import Conv1dBlock, ResidualTemporalBlock

from . import _unet_draw as D
from ._train_util import REL_GRAD, _errors, _inputs, _oracle_grads
from ._util import ABS_ELEM, make_unet, oracle_fp64_layers

SMALLEST = ("d1H32C5-B3", "d2H16C4-B5-x4")  # the smallest 3-level and 4-level shapes of the GPU tests


# ------------------------------------------------------------------------------------------------ the draw itself
@pytest.mark.parametrize("cfg,mults", [(True, (1, 2, 4)), (False, (1, 2, 4, 8))])
def test_draw_is_deterministic_and_touches_only_the_conv_blocks(cfg, mults):
    base = make_unet(2, 3, mults=mults, seed=5, cfg=cfg)
    ref = {k: v.clone() for k, v in base.state_dict().items()}
    again = make_unet(2, 3, mults=mults, seed=5, cfg=cfg)
    for k, v in again.state_dict().items():
        assert torch.equal(v, ref[k]), k  # make_unet's default output: unchanged by this module
    for name, kw in D.DRAWS.items():
        a = D.draw_unet_weights(make_unet(2, 3, mults=mults, seed=5, cfg=cfg), 9, **kw)
        state = torch.get_rng_state()
        b = D.draw_unet_weights(make_unet(2, 3, mults=mults, seed=5, cfg=cfg), 9, **kw)
        assert torch.equal(torch.get_rng_state(), state), "the draw has its own generator"
        c = D.draw_unet_weights(make_unet(2, 3, mults=mults, seed=5, cfg=cfg), 10, **kw)
        sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
        assert list(sa) == list(ref) and all(sa[k].shape == ref[k].shape for k in ref), name
        assert all(torch.equal(sa[k], sb[k]) for k in ref), name
        blocks = {n for n, m in a.named_modules() if isinstance(m, Conv1dBlock)}
        assert blocks
        n_gn = 0
        for k in ref:
            owner = k.rsplit(".block.", 1)[0] if ".block." in k else None
            if owner not in blocks:
                assert torch.equal(sa[k], ref[k]), f"{name}: {k} is outside every Conv1dBlock"
                continue
            if ".block.2." in k:  # the GroupNorm
                n_gn += 1
                assert not torch.equal(sa[k], sc[k]), (name, k)
                if k.endswith("weight"):
                    assert bool((sa[k] != 1).all()) and bool(((sa[k].abs() >= 0.5) & (sa[k].abs() <= 1.5)).all()), k
                else:
                    assert bool((sa[k] != 0).all()) and bool((sa[k].abs() <= 1).all()), k
            elif not (kw.get("scales") or kw.get("offsets")):
                assert torch.equal(sa[k], ref[k]), f"{name}: conv {k} moved without scales / offsets"
        assert n_gn == 2 * len(blocks)
        gammas = torch.cat([sa[k] for k in ref if k.endswith(".block.2.weight")])
        assert 0.3 < float((gammas < 0).float().mean()) < 0.7, "a fair sign per channel"


def test_scales_and_offsets_act_on_the_conv_as_stated():
    """scales: weight and bias of a conv times one 2^k, k in [-6, 6], not all alike; offsets: one value per group on
    the conv bias, |value| <= A, scaled with the bias (the offset is applied first)."""
    base = make_unet(2, 3, seed=5)
    sd0 = base.state_dict()
    s = D.draw_unet_weights(make_unet(2, 3, seed=5), 3, affine=False, scales=True).state_dict()
    ks = set()
    for n, m in base.named_modules():
        if isinstance(m, Conv1dBlock):
            r = s[n + ".block.0.weight"] / sd0[n + ".block.0.weight"]
            k = math.log2(float(r.flatten()[0]))
            assert k == int(k) and -6 <= k <= 6 and bool((r == 2.0 ** k).all()), n
            assert torch.equal(s[n + ".block.0.bias"], sd0[n + ".block.0.bias"] * 2.0 ** k), n
            ks.add(int(k))
    assert len(ks) >= 5
    o = D.draw_unet_weights(make_unet(2, 3, seed=5), 3, affine=False, offsets=3.0).state_dict()
    both = D.draw_unet_weights(make_unet(2, 3, seed=5), 3, affine=False, offsets=3.0, scales=True).state_dict()
    for n, m in base.named_modules():
        if isinstance(m, Conv1dBlock):
            gn = m.block[2]
            off = (o[n + ".block.0.bias"] - sd0[n + ".block.0.bias"]).reshape(gn.num_groups, -1)
            assert float(off.abs().max()) <= 3.0 + 1e-6 and float(off.abs().max()) > 0.1, n
            assert float((off - off[:, :1]).abs().max()) <= 1e-6, f"{n}: one offset per group"
            assert torch.equal(o[n + ".block.0.weight"], sd0[n + ".block.0.weight"])
            r = both[n + ".block.0.weight"].flatten()[0] / sd0[n + ".block.0.weight"].flatten()[0]
            # with both, the offsets are other draws of the same stream: still one per group, inside the scale
            off = (both[n + ".block.0.bias"] / r - sd0[n + ".block.0.bias"]).reshape(gn.num_groups, -1)
            assert float(off.abs().max()) <= 3.0 + 1e-6 and float((off - off[:, :1]).abs().max()) <= 1e-6, n


# ------------------------------------------------------------------------- slips of the GroupNorm affine, restated
def _xhat(self, x):
    return F.group_norm(x, self.num_groups, None, None, self.eps)


def _per_channel(v, x):
    return v.reshape(1, -1, *([1] * (x.dim() - 2)))


def _by_group(self, v):
    cpg = self.num_channels // self.num_groups
    return v[torch.arange(self.num_channels) // cpg]


def _by_index(self, v, mod):
    return v[torch.arange(self.num_channels) % mod]


def _affine(self, x, gamma, beta):
    return _xhat(self, x) * _per_channel(gamma, x) + _per_channel(beta, x)


def _scale_shift(self, x, gamma_in_shift=True):
    """unet.hip's form, y = x scale + shift with scale = rstd gamma, shift = -mean rstd gamma + beta; gamma_in_shift
    False leaves gamma out of the shift's mean term"""
    n, c, cpg = x.shape[0], self.num_channels, self.num_channels // self.num_groups
    xg = x.reshape(n, self.num_groups, -1)
    mean = xg.mean(dim=2, keepdim=True)
    rstd = (xg.var(dim=2, unbiased=False, keepdim=True) + self.eps).rsqrt()
    tail = [1] * (x.dim() - 2)
    scale = rstd.expand(n, self.num_groups, cpg).reshape(n, c, *tail) * _per_channel(self.weight, x)
    mrs = (mean * rstd).expand(n, self.num_groups, cpg).reshape(n, c, *tail)
    if gamma_in_shift:
        mrs = mrs * _per_channel(self.weight, x)
    return x * scale - mrs + _per_channel(self.bias, x)


def _right(s, x):
    """the restatement without a slip: what every _affine slip is compared with bit for bit at initialisation"""
    return _affine(s, x, s.weight, s.bias)


FORWARD_SLIPS = {
    # the issue's four, as each site could commit them
    "gamma dropped": lambda s, x: _affine(s, x, torch.ones_like(s.weight), s.bias),
    "beta dropped": lambda s, x: _affine(s, x, s.weight, torch.zeros_like(s.bias)),  # unet.hip: shift = -scale mean
    "gamma by group": lambda s, x: _affine(s, x, _by_group(s, s.weight), s.bias),
    "gamma, beta by c % channels_per_group": lambda s, x: _affine(
        s, x, _by_index(s, s.weight, s.num_channels // s.num_groups), _by_index(s, s.bias, s.num_channels // s.num_groups)),
    # "gamma and beta swapped": see _sibling_swap below (the literal swap is visible at any weights)
    # further ones, from reading the five sites
    "gamma by c % 4": lambda s, x: _affine(s, x, _by_index(s, s.weight, 4), s.bias),  # unet_fused.hip: gnw[e] of a quad
    "gamma, beta by c % 4": lambda s, x: _affine(s, x, _by_index(s, s.weight, 4), _by_index(s, s.bias, 4)),
    "beta by group": lambda s, x: _affine(s, x, s.weight, _by_group(s, s.bias)),
    "beta in the wrong unit": lambda s, x: _affine(s, x, s.weight, s.bias * math.log2(math.e)),  # the log2-unit FMAs
    "|gamma|": lambda s, x: _affine(s, x, s.weight.abs(), s.bias),
}
# a slip in another arithmetic form is compared with that form done right
SLIP_TWINS = {"gamma missing from the shift": (_scale_shift, lambda s, x: _scale_shift(s, x, gamma_in_shift=False))}


class _patched:
    """nn.GroupNorm.forward replaced inside the context, restored in finally"""

    def __init__(self, fwd):
        self.fwd = fwd

    def __enter__(self):
        self.saved = nn.GroupNorm.forward
        nn.GroupNorm.forward = self.fwd

    def __exit__(self, *exc):
        nn.GroupNorm.forward = self.saved


def _sibling_swap(net):
    """"gamma and beta swapped", the reading default initialisation hides: each GroupNorm of a ResidualTemporalBlock
    takes the weight and bias of the block's other GroupNorm (the packed layouts keep both side by side). The literal
    swap, y = xhat beta + gamma, is constant 1 at initialisation: every test sees that one already (asserted below)."""
    other = {}
    for m in net.modules():
        if isinstance(m, ResidualTemporalBlock):
            a, b = m.blocks[0].block[2], m.blocks[1].block[2]
            other[a], other[b] = b, a
    return lambda s, x: _affine(s, x, other.get(s, s).weight, other.get(s, s).bias)


def _all_eps(net, case):
    out = []
    for _lab, x, t, ctx in D.case_evals(case):
        out += list(D.oracle_eps(net, case, x, t, ctx))
    return out


def _moved(a, b):
    return max(D.eps_err(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("case", SMALLEST)
def test_forward_slips_hide_at_default_init_and_show_at_the_affine_draw(case):
    """Every slip, at the smallest 3-level and 4-level shapes of the GPU tests: at the default initialisation eps is
    bit-identical to the same arithmetic without the slip (xhat gamma + beta on F.group_norm's xhat, which itself
    sits within 1/5 of the bar of nn.GroupNorm's own kernel); at the affine draw eps moves by >= 100 x 2e-5 of
    max(|eps| max, 1) from the oracle."""
    init, drawn = D.case_net(case, None), D.case_net(case, "affine")
    oracle = {init: _all_eps(init, case), drawn: _all_eps(drawn, case)}
    pairs = {name: (_right, fwd) for name, fwd in FORWARD_SLIPS.items()}
    pairs.update(SLIP_TWINS)
    for name, (right, slipped) in pairs.items():
        for net in (init, drawn):
            with _patched(right):
                ref = _all_eps(net, case)
            assert _moved(ref, oracle[net]) <= D.EPS_BAR / 5, (case, name, "the restatement")
            with _patched(slipped):
                got = _all_eps(net, case)
            if net is init:
                assert all(torch.equal(g, r) for g, r in zip(got, ref)), f"{case} {name}: visible at initialisation"
            else:
                moved = _moved(got, oracle[net])
                print(f"{case} {name}: eps moves by {moved:.3e} of max(|eps| max, 1) at the affine draw")
                assert moved >= 100 * D.EPS_BAR, (case, name, moved)
    name = "gamma and beta swapped with the block's other GroupNorm"
    with _patched(_right):
        ref = _all_eps(init, case)
    with _patched(_sibling_swap(init)):
        assert all(torch.equal(g, r) for g, r in zip(_all_eps(init, case), ref)), f"{case} {name}"
    with _patched(_sibling_swap(drawn)):
        moved = _moved(_all_eps(drawn, case), oracle[drawn])
    print(f"{case} {name}: eps moves by {moved:.3e} of max(|eps| max, 1) at the affine draw")
    assert moved >= 100 * D.EPS_BAR, (case, name, moved)
    with _patched(lambda s, x: _affine(s, x, s.bias, s.weight)):  # the literal swap is not a hidden one
        assert _moved(_all_eps(init, case), oracle[init]) >= 100 * D.EPS_BAR


class _ScaleBackwardWithout(torch.autograd.Function):
    """y = xhat gamma, backward as gn_bwd_kernel would be with d = dy[e] (or gamma taken by group): the affine
    partials stay right, the gradient handed upstream loses (or misplaces) gamma."""

    @staticmethod
    def forward(ctx, xhat, gamma, wrong):
        ctx.save_for_backward(xhat, gamma, wrong)
        return xhat * _per_channel(gamma, xhat)

    @staticmethod
    def backward(ctx, dy):
        xhat, gamma, wrong = ctx.saved_tensors
        dims = [0] + list(range(2, dy.dim()))
        return dy * _per_channel(wrong, dy), (dy * xhat).sum(dim=dims), None


BACKWARD_SLIPS = {
    "dx without gamma": lambda s: torch.ones_like(s.weight),
    "dx with gamma by group": lambda s: _by_group(s, s.weight.detach()),
}


def _slipped_grads(net, tables, batch, wrong_of):
    def fwd(s, x):
        return _ScaleBackwardWithout.apply(_xhat(s, x), s.weight, wrong_of(s)) + _per_channel(s.bias, x)
    with _patched(fwd):
        return _oracle_grads(net, tables, batch, fp64=False)


@pytest.mark.parametrize("case", ["d1H32C5-B5", "d2H16C4-B5-x4"])
def test_backward_slips_hide_at_default_init_and_show_at_the_affine_draw(case):
    """A backward pass whose dx omits (or misplaces) gamma. At initialisation loss and every gradient tensor stay as
    close to the fp64-layer reference as the fp32 oracle itself is (within 1/5 of the bars): no test from
    initialisation can see it. At the affine draw at least one tensor moves by >= 100 x REL_GRAD while the loss
    stays within its bar, so the loss check alone does not see it either."""
    d, H, C, B, mults = D.TRAIN_CASES[case]
    tables = osch.buffers("exponential", 100)
    batch = _inputs(d, H, C, B, 100, seed=D.TRAIN_INPUT_SEED)
    for name, wrong_of in BACKWARD_SLIPS.items():
        net = D.train_net(case, None)
        ref_loss, ref = _oracle_grads(net, tables, batch)
        _, own = _oracle_grads(net, tables, batch, fp64=False)
        loss, got = _slipped_grads(net, tables, batch, wrong_of)
        e_own, e_slip = _errors(own, ref), _errors(got, ref)
        w_own = max(max(e) for e in e_own.values())
        w_slip = max(max(e) for e in e_slip.values())
        print(f"{case} {name} at initialisation: slipped worst {w_slip:.3e}, fp32 oracle's own {w_own:.3e}, "
              f"over {len(e_slip)} tensors")
        assert w_slip <= 2 * w_own, "no further from the reference than the fp32 oracle's own rounding puts it"
        assert w_slip <= REL_GRAD / 5 and abs(loss - ref_loss) <= 1e-5 / 5 * abs(ref_loss)
        net = D.train_net(case, "affine")
        ref_loss, ref = _oracle_grads(net, tables, batch)
        loss, got = _slipped_grads(net, tables, batch, wrong_of)
        e_slip = _errors(got, ref)
        over = [n for n, e in e_slip.items() if e[0] > REL_GRAD]
        worst = max((e[0], n) for n, e in e_slip.items())
        print(f"{case} {name} at the affine draw: {len(over)}/{len(e_slip)} tensors over the bar, worst "
              f"{worst[0]:.3e} ({worst[1]}), loss moves {abs(loss - ref_loss) / abs(ref_loss):.1e}")
        assert worst[0] >= 100 * REL_GRAD, (case, name, worst)
        assert len(over) >= len(e_slip) // 2


# ---------------------------------------------------------------------------------- condition of the unchanged bars
@pytest.mark.parametrize("draw", D.FIXED_BAR_DRAWS)
@pytest.mark.parametrize("case", sorted(D.FWD_CASES))
def test_forward_cases_are_well_conditioned(case, draw):
    """Every (shape, draw, context form, t, branch) of tests/test_gpu_unet_draw.py: the fp32 oracle sits within 1/5 of
    the 2e-5 bar of the oracle with fp64 layers. A case that misses gets its seed redrawn (_unet_draw.REDRAWN_SEEDS
    names those), never its bar moved."""
    net = D.case_net(case, draw)
    worst = 0.0
    for lab, x, t, ctx in D.case_evals(case):
        own = D.oracle_eps(net, case, x, t, ctx)
        with oracle_fp64_layers():
            ref = D.oracle_eps(net, case, x, t, ctx)
        for o, r in zip(own, ref):
            assert float(r.abs().max()) > 1e-2, "a reference that is all but zero checks nothing"
            e = D.eps_err(o, r)
            worst = max(worst, e)
            assert e <= D.EPS_BAR / 5, (case, draw, lab, e)
    print(f"{case} {draw}: fp32 oracle within {worst:.2e} of the fp64-layer oracle (bar {D.EPS_BAR:g})")


@pytest.mark.parametrize("draw", D.TRAIN_DRAWS)
@pytest.mark.parametrize("case", sorted(D.TRAIN_CASES))
def test_training_cases_are_well_conditioned(case, draw):
    """Every case of tests/test_gpu_train_draw.py: the fp32 oracle's loss and every gradient tensor within 1/5 of
    REL_LOSS / REL_GRAD / ABS_ELEM of the fp64-layer reference."""
    d, H, C, B, mults = D.TRAIN_CASES[case]
    net = D.train_net(case, draw)
    tables = osch.buffers("exponential", 100)
    batch = _inputs(d, H, C, B, 100, seed=D.TRAIN_INPUT_SEED)
    assert 0 < float(batch[4].sum()) < B, "the drawn context mask keeps some rows and drops some"
    ref_loss, ref = _oracle_grads(net, tables, batch)
    loss, own = _oracle_grads(net, tables, batch, fp64=False)
    errs = _errors(own, ref)
    wn, we = max(e[0] for e in errs.values()), max(e[1] for e in errs.values())
    print(f"{case} {draw}: fp32 oracle's gradients within {wn:.2e} (norm) / {we:.2e} (element) of the reference, "
          f"loss {abs(loss - ref_loss) / abs(ref_loss):.1e}")
    assert abs(loss - ref_loss) <= 1e-5 / 5 * abs(ref_loss)
    assert wn <= REL_GRAD / 5 and we <= ABS_ELEM / 5


def test_offsets10_spread_is_what_the_gpu_test_states():
    """The one forward case without a fixed bar (test_gpu_unet_draw.test_eps_at_group_offsets_of_ten): s, the fp32
    oracle's distance from the fp64-layer oracle per evaluation, is printed here; SPREAD_X s stays below 100 x the
    fixed bar, so the case still separates every slip above (they move eps by >= 0.37)."""
    case = D.OFFSET10_CASE
    net = D.case_net(case, "affine+offsets10")
    ss = []
    for lab, x, t, ctx in D.case_evals(case):
        own = D.oracle_eps(net, case, x, t, ctx)
        with oracle_fp64_layers():
            ref = D.oracle_eps(net, case, x, t, ctx)
        ss += [D.eps_err(o, r) for o, r in zip(own, ref)]
    print(f"{case} affine+offsets10: s per evaluation {min(ss):.2e} .. {max(ss):.2e}")
    assert 0 < min(ss) and 3 * max(ss) <= 100 * D.EPS_BAR
