"""Shared helpers of the training-step parity tests: the drawn batch, the oracle's loss and gradients (with the
layers in fp64 by default: _util.oracle_fp64_layers) and the per-tensor gradient bars."""
import torch

from oracle.train import OracleTrainer

from ._util import ABS_ELEM, oracle_fp64_layers

REL_LOSS = 1e-5
REL_GRAD = 1e-4


def _inputs(d, H, C, B, n_steps, seed, top_tenth=False):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, H, d, generator=g) * 2 - 1
    ctx = torch.rand(B, C, generator=g) * 2 - 1
    lo = n_steps - n_steps // 10 if top_tenth else 0
    t = torch.randint(lo, n_steps, (B,), generator=g).long()
    noise = torch.randn(B, H, d, generator=g)
    mask = torch.bernoulli(torch.full((B, 1), 0.25), generator=g)
    return x0, ctx, t, noise, mask


def _oracle_grads(net, tables, batch, fp64=True):
    """(loss, {name: gradient}) of the oracle on the CPU; fp64: with the layers computing in fp64"""
    orc = OracleTrainer(net, tables)
    net.zero_grad(set_to_none=True)
    if fp64:
        with oracle_fp64_layers():
            loss = orc.loss(*batch)
            loss.backward()
    else:
        loss = orc.loss(*batch)
        loss.backward()
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def _errors(grads, ref):
    """per tensor (norm-relative, elementwise relative to max|ref|) errors; exact zeros checked here"""
    out = {}
    for n, r in ref.items():
        got = grads[n]
        assert torch.isfinite(got).all(), n
        if float(r.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, n
            continue
        dlt = (got.double() - r.double())
        out[n] = (float(dlt.norm() / r.double().norm()), float(dlt.abs().max() / r.double().abs().max()))
    return out


def _assert_grads(grads, ref, what, bars=None):
    errs = _errors(grads, ref)
    wn = max((e[0], n) for n, e in errs.items())
    we = max((e[1], n) for n, e in errs.items())
    print(f"{what}: worst gradient tensor norm-rel {wn[0]:.3e} ({wn[1]}), elementwise {we[0]:.3e} ({we[1]})")
    for n, (en, ee) in errs.items():
        bn, be = (REL_GRAD, ABS_ELEM) if bars is None else bars[n]
        assert en <= bn, (what, n, en, bn)
        assert ee <= be, (what, n, ee, be)
    return wn[0], we[0]
