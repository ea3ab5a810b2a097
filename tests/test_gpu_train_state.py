"""The trainer's optimiser state, one step at a time: adam_kernel / ema_kernel (csrc/train.hip, through
mpcd_trainer_step and state_dict) against the fp64 transition of tests/_adam_ref.py computed from the device's own
state before the step and the device's own gradient. That takes the backward pass out of the comparison (the
gradients have their own tests) and with it the sign flips of unresolved Adam steps that force 1e-2 bars on a
multi-step comparison with the oracle: every element of exp_avg, exp_avg_sq, the parameters and the EMA model is
held to a roundoff bound (tests/_adam_ref.py states and derives them; tests/test_adam_ref_host.py shows that an
eps on the wrong side of sqrt(bc2), a bias correction one step off, swapped betas or a wrong EMA branch leave
them)."""
import numpy as np
import pytest
import torch

from mpc_via_diffusion_model_amd import NetSpec
from mpc_via_diffusion_model_amd.training import DiffusionTrainer
from oracle import schedule as osch

from . import _adam_ref as R
from ._util import make_mlp, make_unet

pytestmark = pytest.mark.gpu

STATE = ("params", "ema", "exp_avg", "exp_avg_sq")
NETS = [("mlp", 2, 16, 4, 48), ("unet", 1, 16, 3, 6)]


def _flat(tr, which):
    sd = tr.state_dict(which)
    return torch.cat([sd[n].reshape(-1) for n, _ in tr.param_spec]).numpy()


def _trainer(kind, d, H, C, hp, seed=0):
    net = (make_mlp(d, H, C, seed=seed) if kind == "mlp" else make_unet(d, C, seed=seed)).train()
    return DiffusionTrainer(NetSpec(kind, d, H, C), net.state_dict(), tables=osch.buffers("exponential", 100), **hp)


def _batch(tr, d, H, C, B, g, all_dropped=False):
    x0 = torch.rand(B, H, d, generator=g) * 2 - 1
    ctx = torch.rand(B, C, generator=g) * 2 - 1
    t, noise, mask = tr.draw(B, (B, H, d), generator=g)
    return x0, ctx, t, noise, torch.ones_like(mask) if all_dropped else mask


def _checked_step(tr, hp, step, batch, what):
    """train_step number `step` (from 1) with every state vector read before and after; asserts the transition and
    returns (worst bound ratios, how many elements had g == 0 and m == 0)."""
    before = {k: _flat(tr, k) for k in STATE}
    loss = tr.train_step(*batch)
    assert np.isfinite(loss), (what, step)
    g = _flat(tr, "grads")
    after = {k: _flat(tr, k) for k in STATE}
    for k in STATE:
        assert np.isfinite(after[k]).all(), (what, step, k)
    r = R.transition_ratios(before, after, g, step, hp)
    for k in ("exp_avg", "exp_avg_sq", "params"):
        assert r[k] <= 1.0, (what, step, k, r[k])
    if r["ema"] is None:  # the schedule skips this step
        assert np.array_equal(after["ema"], before["ema"]), (what, step, "EMA moved on a skipped step")
    else:
        assert r["ema"] <= 1.0, (what, step, "ema", r["ema"])
    still = (g == 0) & (before["exp_avg"] == 0)  # nothing to do there: not one bit may change
    for k in ("exp_avg", "exp_avg_sq", "params"):
        assert np.array_equal(after[k][still], before[k][still]), (what, step, k)
    return r, int(still.sum()), int((g == 0).sum())


@pytest.mark.parametrize("hp_name", sorted(R.HYPERS))
@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_eight_steps_state_transition(net, hp_name):
    """8 steps; under the non-default set (ema_decay 0.9, step_start_ema 3, update_ema_every 2) they cross EMA
    resets (s0 = 0, 2), blends (4, 6) and skipped steps; under the defaults one reset and seven skips. The first
    and fifth steps drop every context: the context columns of the cond layers get exactly zero gradients, first
    onto zero moments (nothing may change), then onto moments that only decay."""
    kind, d, H, C, B = net
    hp = R.HYPERS[hp_name]
    tr = _trainer(kind, d, H, C, hp)
    g = torch.Generator().manual_seed(21)
    worst = {k: 0.0 for k in STATE}
    ema_steps = []
    for step in range(1, 9):
        dropped = step in (1, 5)
        r, n_still, n_zero = _checked_step(tr, hp, step, _batch(tr, d, H, C, B, g, all_dropped=dropped),
                                           (kind, hp_name))
        if dropped:
            assert n_zero > 0, "an all-dropped step leaves the context columns without gradient"
            # step 1 meets zero moments; by step 5 the context columns' moments are nonzero and decay
            assert n_still > 0 if step == 1 else n_zero > n_still, (step, n_still, n_zero)
        for k in STATE:
            if r[k] is not None:
                worst[k] = max(worst[k], r[k])
        if r["ema"] is not None:
            ema_steps.append(step - 1)
    assert ema_steps == [s for s in range(8) if s % hp["update_ema_every"] == 0]
    print(f"state transition {kind} {hp_name}: worst bound ratios over 8 steps " +
          ", ".join(f"{k} {worst[k]:.3f}" for k in STATE))


@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_loss_leaves_the_state_alone(net):
    """loss() (update = 0) between two steps: parameters, EMA, gradients and both moments bit-identical, and the
    step after it is Adam's second (its bias corrections at step 2), not its third or its first."""
    kind, d, H, C, B = net
    hp = R.HYPER_OTHER
    tr = _trainer(kind, d, H, C, hp)
    g = torch.Generator().manual_seed(22)
    _checked_step(tr, hp, 1, _batch(tr, d, H, C, B, g), (kind, "before loss()"))
    five = STATE + ("grads",)
    before = {k: _flat(tr, k) for k in five}
    assert np.isfinite(tr.loss(*_batch(tr, d, H, C, B, g)))
    for k in five:
        assert np.array_equal(_flat(tr, k), before[k]), (kind, k)
    _checked_step(tr, hp, 2, _batch(tr, d, H, C, B, g), (kind, "after loss()"))


def test_hyperparameters_reach_the_kernel():
    """Two trainers from the same weights on the same two batches, one per hyperparameter set: each follows its
    own reference, and they end at different parameters, moments and EMA models."""
    kind, d, H, C, B = NETS[0]
    trs = {name: _trainer(kind, d, H, C, hp) for name, hp in R.HYPERS.items()}
    for step in (1, 2):
        g = torch.Generator().manual_seed(23 + step)
        batch = None
        for name, tr in trs.items():
            batch = batch or _batch(tr, d, H, C, B, g)
            _checked_step(tr, R.HYPERS[name], step, batch, (name, "two sets"))
    a, b = trs["default"], trs["other"]
    for k in STATE:
        va, vb = _flat(a, k), _flat(b, k)
        assert (va != vb).mean() > 0.9, k
