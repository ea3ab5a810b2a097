"""CPU: the optimiser-state reference of tests/_adam_ref.py checks itself, so that tests/test_gpu_train_state.py
compares adam_kernel / ema_kernel with something known to be right: adam_ref against torch.optim.Adam on float64
tensors, ema_ref against OracleTrainer's EMA bookkeeping, the op-by-op fp32 emulation of the kernels inside every
bound (with and without fused multiply-adds), and nine wrong updates each outside a bound."""
import numpy as np
import pytest
import torch

from oracle import schedule as osch
from oracle.train import OracleTrainer

from . import _adam_ref as R
from ._util import make_mlp

SETS = sorted(R.HYPERS)


@pytest.mark.parametrize("hp_name", SETS)
def test_adam_ref_matches_torch_float64(hp_name):
    """20 steps of random gradients: m, v and p of adam_ref == torch.optim.Adam on float64 CPU tensors given the
    same fp32-rounded hyperparameters, every element to 1e-12 relative."""
    hp = R.HYPERS[hp_name]
    lr, (b1, b2), eps = hp["lr"], hp["betas"], hp["eps"]
    rng = np.random.default_rng(11)
    n = 4096
    p = rng.standard_normal(n) * 0.3
    m, v = np.zeros(n), np.zeros(n)
    tp = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.Adam([tp], lr=R.f32(lr), betas=(R.f32(b1), R.f32(b2)), eps=R.f32(eps))
    for step in range(1, 21):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)
        m0, p0 = m, p
        m, v, delta = R.adam_ref(p, m, v, g, step, lr, b1, b2, eps)
        p = p - delta
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        st = opt.state[tp]
        # relative to what each sum is made of (m' and p' cancel: a moment or a weight that crosses zero has no
        # relative accuracy of its own in either implementation), i.e. the bounds' own scales with 1e-12 for u
        for name, got, want, scale in (("exp_avg", m, st["exp_avg"], np.abs(m0) + np.abs(g)),
                                       ("exp_avg_sq", v, st["exp_avg_sq"], v),
                                       ("params", p, tp, np.abs(p0) + np.abs(delta))):
            rel = np.abs(got - want.detach().numpy()) / scale
            assert rel.max() <= 1e-12, (hp_name, step, name, rel.max())


@pytest.mark.parametrize("decay,start,every", [(0.995, 1000, 10), (0.9, 3, 2)])
def test_ema_ref_matches_oracle_trainer(decay, start, every):
    """12 steps of the oracle trainer on a small net; ema_ref is driven with the parameters the oracle held after
    each step and must reproduce the oracle's EMA model: within the fp32 EMA bound on the steps that update it,
    bit for bit on the steps the schedule skips. (The oracle blends in fp32, so the bound is the comparison's
    resolution; the reset, blend and skip branches differ by the whole Adam step, ~1e-2 here.)"""
    d, H, C, B = 2, 8, 3, 16
    net = make_mlp(d, H, C, seed=5).train()
    orc = OracleTrainer(net, osch.buffers("exponential", 50), lr=1e-2, ema_decay=decay, step_start_ema=start,
                        update_ema_every=every)

    def flat(mod):
        return torch.cat([q.detach().reshape(-1) for q in mod.parameters()]).numpy().copy()

    g = torch.Generator().manual_seed(6)
    ema = flat(orc.ema).astype(np.float64)
    acted = []
    for s0 in range(12):
        x0 = torch.rand(B, H, d, generator=g) * 2 - 1
        ctx = torch.rand(B, C, generator=g) * 2 - 1
        t = torch.randint(0, 50, (B,), generator=g)
        noise = torch.randn(B, H, d, generator=g)
        mask = torch.bernoulli(torch.full((B, 1), 0.25), generator=g)
        before = flat(orc.ema)
        orc.train_step(x0, ctx, t, noise, mask)
        p_new, got = flat(orc.net), flat(orc.ema)
        ref = R.ema_ref(before, p_new, s0, decay, start, every)
        if R.ema_acts(s0, every):
            acted.append(s0)
            old = R.ema_old(before, p_new, s0, start)
            assert (np.abs(got - ref) <= R.bound_ema(old, p_new)).all(), s0
            # the other branch is far outside the bound: the comparison tells reset from blend
            other = R.ema_ref(before, p_new, s0, decay, 0 if s0 < start else 10 ** 9, every)
            if s0 > 0:
                assert (np.abs(got - other) > R.bound_ema(old, p_new)).mean() > 0.5, s0
        else:
            assert np.array_equal(got, before) and np.array_equal(ref, before.astype(np.float64)), s0
        # and the chain of references alone tracks the oracle over all 12 steps
        ema = R.ema_ref(ema, p_new, s0, decay, start, every)
        assert np.abs(ema - got).max() <= 16 * R.U * max(np.abs(got).max(), 1.0), s0
    assert acted == [s for s in range(12) if s % every == 0]


def _emulation_inputs(n, steps, seed=3):
    """parameters of a net's scale (a spread of binades, some just above a power of two), gradients spanning
    1e-12 .. 1 with both signs, a tenth of them exactly zero on every step"""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.3 * 2.0 ** rng.integers(-6, 2, n)).astype(np.float32)
    gs = []
    for _ in range(steps):
        g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 0, n)
        g[: n // 10] = 0.0
        gs.append(g.astype(np.float32))
    z = np.zeros(n, dtype=np.float32)
    return {"params": p, "ema": p.copy(), "exp_avg": z, "exp_avg_sq": z.copy()}, gs


def _run_emulation(hp, n, steps, fma=False, mutation=None, p_ulps=2):
    """-> per step: the worst bound ratios, and whether the EMA moved on a step that must skip it"""
    state, gs = _emulation_inputs(n, steps)
    out = []
    for step in range(1, steps + 1):
        new = R.emulate_step(state, gs[step - 1], step, hp, fma=fma, mutation=mutation)
        r = R.transition_ratios(state, new, gs[step - 1], step, hp, p_ulps=p_ulps)
        moved = r["ema"] is None and not np.array_equal(new["ema"], state["ema"])
        out.append((r, moved))
        state = new
    return out


@pytest.mark.parametrize("fma", [False, True], ids=["separate_roundings", "fused_multiply_adds"])
def test_emulation_stays_inside_bounds(fma):
    """10 steps, 200k elements, both hyperparameter sets: the emulation of the kernels' own operation order is
    inside every bound. Printed: the worst ratio per state vector, and the parameter ratio against
    u |p'| + 16u |delta| (the bound before its first term was doubled), which reaches 1.00."""
    for hp_name in SETS:
        hp = R.HYPERS[hp_name]
        worst = {}
        for p_ulps in (2, 1):
            runs = _run_emulation(hp, 200_000, 10, fma=fma, p_ulps=p_ulps)
            assert not any(moved for _, moved in runs)
            for k in ("exp_avg", "exp_avg_sq", "params", "ema"):
                vals = [r[k] for r, _ in runs if r[k] is not None]
                assert vals, (hp_name, k)
                worst[k if p_ulps == 2 or k != "params" else "params_1u"] = max(vals)
        print(f"adam/ema emulation, fma={fma}, {hp_name}: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))
        for k in ("exp_avg", "exp_avg_sq", "params", "ema"):
            assert worst[k] <= 1.0, (hp_name, k, worst[k])
        # the measurement behind the params bound's 2u |p'|: with u |p'| the emulation sits at the bound itself
        assert 0.9 <= worst["params_1u"] <= 1.05, worst["params_1u"]
        # the bounds are roundoff-sized, not loose: the emulation uses a good part of each (the EMA's only where
        # it blends: a fused reset p decay + (1 - decay) p returns p almost exactly)
        assert worst["exp_avg"] >= 0.1 and worst["exp_avg_sq"] >= 0.3, worst
        assert worst["ema"] >= 0.1 or hp_name == "default", worst


# the step at which each wrong update must have left a bound. Every Adam mutation and the two EMA mutations the
# first step can tell apart: step 2 at the latest. An EMA that resets where it should blend cannot differ before
# the first blend, which under (start 3, every 2) is s0 = 4, the fifth step.
BREAKS_BY = {m: 2 for m in R.MUTATIONS}
BREAKS_BY["ema_resets_instead_of_blend"] = 5


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_bounds_reject_wrong_updates(mutation):
    hp = R.HYPER_OTHER
    runs = _run_emulation(hp, 20_000, BREAKS_BY[mutation], mutation=mutation)
    broke = [i + 1 for i, (r, moved) in enumerate(runs)
             if moved or any(v is not None and not v <= 1.0 for v in r.values())]
    print(f"{mutation}: outside a bound at steps {broke}; first step's ratios {runs[0][0]}")
    assert broke and broke[0] <= BREAKS_BY[mutation], (mutation, broke)
    # and the same run without the mutation is inside every bound at every one of those steps
    clean = _run_emulation(hp, 20_000, BREAKS_BY[mutation])
    assert all(not moved and all(v is None or v <= 1.0 for v in r.values()) for r, moved in clean)
