"""Independent reference of the trainer's optimiser state (TEST INFRASTRUCTURE ONLY): torch's single-tensor Adam
(no weight decay, no amsgrad) and the trainer's EMA schedule, restated in plain numpy fp64. Nothing here comes from
torch.optim or from csrc/train.hip; tests/test_adam_ref_host.py checks it against both restatements the tree
already has (torch.optim.Adam on float64 tensors, oracle.train.OracleTrainer's EMA bookkeeping).

Hyperparameters enter as the C ABI carries them: mpcd_train_cfg holds floats, so lr, the betas, eps and the EMA
decay are rounded to fp32 first, and 1 - beta / 1 - decay are formed in fp32 as the kernels form them (exact for
0.5 <= beta <= 1, so this matters only below 0.5). Everything else is fp64.

  m'    = m + (1 - b1) (g - m)
  v'    = b2 v + (1 - b2) g^2
  delta = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),   bc_i = 1 - b_i^step,   p' = p - delta
  EMA   : only when s0 % update_ema_every == 0 (s0 = steps taken before this one):
          old = p' if s0 < step_start_ema else ema;   ema' = old decay + (1 - decay) p'

Per-element roundoff bounds of an fp32 implementation (u = 2^-24), each against the reference transition from the
implementation's own state before the step:

  exp_avg      4u (|m| + |g|)          one subtraction, one product, one sum, all of terms bounded by |m| + |g|
  exp_avg_sq   4u v' + 2^-126          four roundings of positive terms; g^2 may underflow or flush in fp32
  params       2u |p'| + 16u |delta|   delta from the m', v' the implementation reports, so only the step's own
                                       roundings are left: sqrtf, two divisions (<= 2.5 ulp each), two sums and a
                                       product, <= 7 ulp of delta, and the final sum's half ulp of p' (which is
                                       u |p'| just above a power of two: the op-by-op emulation below reaches
                                       1.00 of u |p'| + 16u |delta|, hence 2u)
  EMA          4u (|old| + |p'|)       two products and a sum

emulate_step is the op-by-op fp32 emulation of adam_kernel / ema_kernel those bounds were measured on (with and
without fused multiply-adds where a compiler may contract them), and the wrong variants the host test shows the
bounds to reject."""
import numpy as np

U = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126

HYPER_DEFAULT = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, ema_decay=0.995, step_start_ema=1000, update_ema_every=10)
HYPER_OTHER = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-3, ema_decay=0.9, step_start_ema=3, update_ema_every=2)
HYPERS = {"default": HYPER_DEFAULT, "other": HYPER_OTHER}


def f32(x):
    """a hyperparameter as mpcd_train_cfg carries it"""
    return float(np.float32(x))


def one_minus_f32(b):
    """1 - b as the kernels form it: both operands and the difference in fp32"""
    return float(np.float32(1) - np.float32(b))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def adam_delta(m_new, v_new, step, lr, b1, b2, eps):
    """the parameter decrement of the step-th Adam step from the updated moments"""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return (lr / bc1) * _f64(m_new) / (np.sqrt(_f64(v_new)) / np.sqrt(bc2) + eps)


def adam_ref(p, m, v, g, step, lr, b1, b2, eps):
    """-> (m', v', delta) of the step-th step (step counts from 1); p' = p - delta"""
    m, v, g = _f64(m), _f64(v), _f64(g)
    m_new = m + one_minus_f32(b1) * (g - m)
    v_new = f32(b2) * v + one_minus_f32(b2) * (g * g)
    return m_new, v_new, adam_delta(m_new, v_new, step, lr, b1, b2, eps)


def ema_acts(s0, update_ema_every):
    return update_ema_every > 0 and s0 % update_ema_every == 0


def ema_old(ema, p_new, s0, step_start_ema):
    return _f64(p_new) if s0 < step_start_ema else _f64(ema)


def ema_ref(ema, p_new, s0, decay, step_start_ema, update_ema_every):
    """the EMA model after a step that began with s0 steps taken and ended with parameters p_new"""
    if not ema_acts(s0, update_ema_every):
        return _f64(ema).copy()
    return ema_old(ema, p_new, s0, step_start_ema) * f32(decay) + one_minus_f32(decay) * _f64(p_new)


# ---- bounds
def bound_exp_avg(m, g):
    return 4 * U * (np.abs(_f64(m)) + np.abs(_f64(g)))


def bound_exp_avg_sq(v_new_ref):
    return 4 * U * _f64(v_new_ref) + F32_MIN_NORMAL


def bound_params(p_new_ref, delta, p_ulps=2):
    return p_ulps * U * np.abs(_f64(p_new_ref)) + 16 * U * np.abs(_f64(delta))


def bound_ema(old, p_new):
    return 4 * U * (np.abs(_f64(old)) + np.abs(_f64(p_new)))


def transition_ratios(before, after, g, step, hp, p_ulps=2):
    """Worst |implementation - reference| / bound per state vector for one step of an fp32 implementation.
    before / after: dicts of the flat "params", "ema", "exp_avg", "exp_avg_sq" vectors around the step-th step
    (step counts from 1), g: the gradient it used. A ratio <= 1 is inside the bound; a non-finite value in the
    implementation's state gives inf. The EMA entry is None on the steps whose schedule skips it (the caller
    asserts bit-identity there)."""
    lr, (b1, b2), eps = hp["lr"], hp["betas"], hp["eps"]
    p, m, v = before["params"], before["exp_avg"], before["exp_avg_sq"]
    m_ref, v_ref, _ = adam_ref(p, m, v, g, step, lr, b1, b2, eps)
    delta = adam_delta(after["exp_avg"], after["exp_avg_sq"], step, lr, b1, b2, eps)
    p_ref = _f64(p) - delta

    def worst(got, ref, bound):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(_f64(got) - ref) / bound
        r = np.where(np.isfinite(r), r, np.where((_f64(got) == ref) & np.isfinite(ref), 0.0, np.inf))
        return float(r.max())

    out = {"exp_avg": worst(after["exp_avg"], m_ref, bound_exp_avg(m, g)),
           "exp_avg_sq": worst(after["exp_avg_sq"], v_ref, bound_exp_avg_sq(v_ref)),
           "params": worst(after["params"], p_ref, bound_params(p_ref, delta, p_ulps)),
           "ema": None}
    s0 = step - 1
    if ema_acts(s0, hp["update_ema_every"]):
        e_ref = ema_ref(before["ema"], after["params"], s0, hp["ema_decay"], hp["step_start_ema"], hp["update_ema_every"])
        old = ema_old(before["ema"], after["params"], s0, hp["step_start_ema"])
        out["ema"] = worst(after["ema"], e_ref, bound_ema(old, after["params"]))
    return out


# ---- op-by-op fp32 emulation of adam_kernel / ema_kernel and of the host code that launches them
MUTATIONS = ("eps_before_bc2_division", "eps_inside_sqrt", "bias_correction_step_minus_1", "bias_correction_step_plus_1",
             "bc1_dropped", "betas_swapped", "ema_blends_instead_of_reset", "ema_resets_instead_of_blend",
             "ema_on_step_not_s0")


def _fma(a, b, c):
    """fp32 a * b + c with one rounding: the product of two fp32 numbers is exact in fp64; the fp64 sum is rounded
    once more on the way to fp32 (a double rounding only on exact fp64 ties, immaterial for a bound measurement)"""
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def emulate_step(state, g, step, hp, fma=False, mutation=None):
    """One step of the emulation: state = dict of fp32 "params", "ema", "exp_avg", "exp_avg_sq"; -> the new dict.
    fma: contract m + w (g - m), v b2 + (1 - b2) g^2, p + (-step_size) q and old decay + (1 - decay) p into fused
    multiply-adds. mutation: one of MUTATIONS, a wrong update the bounds must reject."""
    assert mutation is None or mutation in MUTATIONS, mutation
    F = np.float32
    b1, b2 = F(hp["betas"][0]), F(hp["betas"][1])
    if mutation == "betas_swapped":
        b1, b2 = b2, b1
    lr, eps, decay = F(hp["lr"]), F(hp["eps"]), F(hp["ema_decay"])
    bstep = step + {"bias_correction_step_minus_1": -1, "bias_correction_step_plus_1": 1}.get(mutation, 0)
    bc1, bc2 = 1.0 - float(b1) ** bstep, 1.0 - float(b2) ** bstep  # the host forms these in fp64
    with np.errstate(divide="ignore", invalid="ignore"):
        step_size = F(float(lr) if mutation == "bc1_dropped" else np.float64(lr) / np.float64(bc1))
        bc2_sqrt = F(np.sqrt(bc2))
        p, m, v = (state[k].astype(F) for k in ("params", "exp_avg", "exp_avg_sq"))
        g = np.asarray(g, dtype=F)
        w1, w2 = F(1) - b1, F(1) - b2
        m = _fma(g - m, w1, m) if fma else m + w1 * (g - m)
        t = w2 * (g * g)
        v = _fma(v, b2, t) if fma else v * b2 + t
        if mutation == "eps_before_bc2_division":
            denom = (np.sqrt(v) + eps) / bc2_sqrt
        elif mutation == "eps_inside_sqrt":
            denom = np.sqrt(v + eps) / bc2_sqrt
        else:
            denom = np.sqrt(v) / bc2_sqrt + eps
        q = m / denom
        p = _fma(q, -step_size, p) if fma else p + (-step_size) * q
    ema = state["ema"].astype(F)
    s0 = step - 1
    every, start = hp["update_ema_every"], hp["step_start_ema"]
    acts = (step if mutation == "ema_on_step_not_s0" else s0) % every == 0
    if acts:
        reset = s0 < start
        if mutation == "ema_blends_instead_of_reset":
            reset = False
        elif mutation == "ema_resets_instead_of_blend":
            reset = True
        old = p if reset else ema
        wd = F(1) - decay
        t = wd * p
        ema = _fma(old, decay, t) if fma else old * decay + t
    return {"params": p, "ema": ema, "exp_avg": m, "exp_avg_sq": v}
