"""U-Net weights away from torch's default initialisation, for the parity tests.

nn.GroupNorm initialises to weight = 1, bias = 0, every conv of a fresh net has nearly the same magnitude, and a
conv's output has a group mean near zero. At those weights a GroupNorm affine that is dropped, swapped or indexed by
the wrong channel changes nothing, the per-layer power-of-two weight scales of the two-term fp16 fused program are
all alike, and no GroupNorm statistic cancels. draw_unet_weights redraws what reaches those regimes and nothing else
(tests/test_unet_draw_host.py shows on the oracle what each draw makes visible)."""
import torch

from oracle.layers import Conv1dBlock


def draw_unet_weights(net, seed, affine=True, scales=False, offsets=0.0):
    """In place, deterministic from seed (its own torch.Generator; torch's global stream is not touched). Visits the
    net's Conv1dBlock modules in net.modules() order; block[0] is the conv, block[2] the GroupNorm.

    affine:  GroupNorm weight = +-U(0.5, 1.5) with a fair sign per channel, bias = U(-1, 1).
    offsets: A > 0 draws one offset per GroupNorm group, U(-A, A), and adds it to the conv bias of every channel of
             that group: the group's mean moves away from zero while its spread stays.
    scales:  one integer k in [-6, 6] per conv; the conv's weight and bias (the offset included) times 2^k. The
             GroupNorm behind the conv undoes the scale up to its eps, so activations stay O(1).
    Every other parameter stays as it was; state_dict() keys and shapes do not change. Returns net."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if not isinstance(m, Conv1dBlock):
                continue
            conv, gn = m.block[0], m.block[2]
            ch = gn.num_channels
            if affine:
                mag = torch.rand(ch, generator=g) + 0.5
                sign = torch.randint(0, 2, (ch,), generator=g).to(mag.dtype) * 2 - 1
                gn.weight.copy_(sign * mag)
                gn.bias.copy_(torch.rand(ch, generator=g) * 2 - 1)
            if offsets:
                off = (torch.rand(gn.num_groups, generator=g) * 2 - 1) * float(offsets)
                conv.bias.add_(off.repeat_interleave(ch // gn.num_groups))
            if scales:
                k = int(torch.randint(-6, 7, (1,), generator=g))
                conv.weight.mul_(2.0 ** k)
                conv.bias.mul_(2.0 ** k)
    return net


DRAWS = {
    "affine": dict(affine=True),
    "affine+scales": dict(affine=True, scales=True),
    "affine+offsets3": dict(affine=True, offsets=3.0),
    "affine+offsets10": dict(affine=True, offsets=10.0),
}
FIXED_BAR_DRAWS = ("affine", "affine+scales", "affine+offsets3")

# ---------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_unet_draw.py and tests/test_gpu_train_draw.py, stated once: the GPU tests run them and
# tests/test_unet_draw_host.py checks on the CPU that the fp32 oracle sits within 1/5 of each case's bar of the
# reference (the oracle with fp64 layers), so that a miss on the GPU is the kernel's.

EPS_BAR = 2e-5        # f32, f32x3, f16x2: of max(|eps| max, 1)
EPS_BAR_F16 = 2e-2    # fp16 operands

# name: (cfg net, d, H, C, B, mults, fused program covers it). N = 50 (CFG nets) / 100 (TemporalUnet); t = 0, N - 1.
FWD_CASES = {
    "d1H32C5-B3": (True, 1, 32, 5, 3, (1, 2, 4), True),           # fewer candidates than a fused workgroup's rows
    "d2H16C4-B5-x4": (True, 2, 16, 4, 5, (1, 2, 4, 8), False),    # 256 channels, 32 per group, L down to 2
    "d4H64C12-B5": (True, 4, 64, 12, 5, (1, 2, 4), True),         # f32x3: two rows per workgroup, rows over 2+ waves
    "d7H128C20-B3": (True, 7, 128, 20, 3, (1, 2, 4), True),       # f32x3: one row per workgroup
    "d1H32C2-B37": (True, 1, 32, 2, 37, (1, 2, 4), True),         # several workgroups, a ragged last one
    "plain-d2H32C0-B4": (False, 2, 32, 0, 4, (1, 2, 4), False),   # TemporalUnet, c_emb = t_emb
    "plain-d2H64C3-B4-x4": (False, 2, 64, 3, 4, (1, 2, 4, 8), False),
}
OFFSET10_CASE = "d1H32C5-B3"
# seed of the net and of its draw per (case, draw); none had to be redrawn for conditioning (test_unet_draw_host)
REDRAWN_SEEDS = {}


def case_seed(case, draw):
    return REDRAWN_SEEDS.get((case, draw), 100 + 7 * sorted(FWD_CASES).index(case) + sorted(DRAWS).index(draw))


def case_net(case, draw):
    """the oracle net of a forward case, in eval mode, at the named draw (None: default initialisation)"""
    from ._util import make_unet
    cfg, d, H, C, B, mults, _ = FWD_CASES[case]
    seed = case_seed(case, draw or "affine")
    net = make_unet(d, C, mults=mults, seed=seed, cfg=cfg)
    if draw is not None:
        draw_unet_weights(net, seed, **DRAWS[draw])
    return net


def case_steps(case):
    return 50 if FWD_CASES[case][0] else 100


def case_evals(case):
    """[(label, x, t, ctx or None)]: a shared [1, C] and a per-candidate [B, C] context at t = 0 and t = N - 1"""
    cfg, d, H, C, B, mults, _ = FWD_CASES[case]
    g = torch.Generator().manual_seed(1000 + sorted(FWD_CASES).index(case))
    x = torch.randn(B, H, d, generator=g)
    if not C:
        return [(f"t={t}", x, t, None) for t in (0, case_steps(case) - 1)]
    ctxs = [("shared", torch.rand(1, C, generator=g) * 2 - 1), ("per-candidate", torch.rand(B, C, generator=g) * 2 - 1)]
    if not cfg:  # the 3-argument forward takes a [B, C] context only
        ctxs = ctxs[1:]
    return [(f"{lab} t={t}", x, t, ctx) for lab, ctx in ctxs for t in (0, case_steps(case) - 1)]


def oracle_eps(net, case, x, t, ctx):
    """the oracle's forward(s) under whatever layer precision is in force: (cond, uncond) or (eps,)"""
    cfg, d, H, C, B, mults, _ = FWD_CASES[case]
    tt = torch.full((B,), t, dtype=torch.long)
    with torch.no_grad():
        if cfg:
            c = ctx.expand(B, C)
            return net(x, tt, c, torch.zeros(B, 1)), net(x, tt, c, torch.ones(B, 1))
        return (net(x, tt, ctx),)


def eps_err(got, ref):
    return float((got.detach().cpu().double() - ref.double()).abs().max()) / max(float(ref.abs().max()), 1.0)


# training cases: (d, H, C, B, mults), N = 100, inputs from _train_util.inputs(seed=TRAIN_INPUT_SEED)
TRAIN_CASES = {
    "d1H32C5-B5": (1, 32, 5, 5, (1, 2, 4)),
    "d2H16C4-B5-x4": (2, 16, 4, 5, (1, 2, 4, 8)),
    "d4H64C12-B3": (4, 64, 12, 3, (1, 2, 4)),
}
TRAIN_DRAWS = ("affine", "affine+offsets3")
TRAIN_INPUT_SEED = 54  # the first seed from 51 whose drawn context mask keeps some rows and drops some at all three
TRAIN_REDRAWN_SEEDS = {}


def train_net(case, draw):
    """the oracle net of a training case, in train mode, at the named draw (None: default initialisation)"""
    d, H, C, B, mults = TRAIN_CASES[case]
    seed = TRAIN_REDRAWN_SEEDS.get((case, draw), 200 + 7 * sorted(TRAIN_CASES).index(case) + sorted(DRAWS).index(draw or "affine"))
    torch.manual_seed(seed)
    from oracle import nets
    net = nets.ConditionedTemporalUnet(state_dim=d, context_dim=C, unet_input_dim=32, dim_mults=mults).train()
    if draw is not None:
        draw_unet_weights(net, seed, **DRAWS[draw])
    return net
