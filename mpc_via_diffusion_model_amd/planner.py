"""Diffusion-MPC planner: the reference's operator API over the MI355X HIP kernels.

Drop-in for the control-loop body of scripts/inference/Diffusion_MPC_Inference.py:191-289 and
Cart_Diffusion_inference.py:405-512:

  reference                                             here
  GaussianDiffusionModel(model=..., ...) + load_state_dict  DiffusionMPC.from_state_dict(sd, spec)
  dataset.normalize_condition(x0)                        DiffusionMPC.normalize_condition(x0)
  model.run_CFG(context, hard_conds, w, n_samples, horizon, return_chain, sample_fn, n_wo)
                                                         DiffusionMPC.run_CFG(...)   (same signature)
  dataset.unnormalize_states(chain)                      DiffusionMPC.unnormalize_states(x)
  calMPCCost / MPC objective per sample, argmin          DiffusionMPC.mpc_step(x0, system, n_samples)
  (no reference name)                                    DiffusionMPC.sample_trajectories(...)

All compute runs in libmpcd.so (HIP, gfx950); torch supplies device memory, the current stream and
torch.distributed. There is no CPU fallback: a missing library or a failing call raises.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N
from . import distributed as D
from . import schedule as S
from .constraints import Constraints  # noqa: F401 (re-exported)
from .constraints import NEEDS_ARGMIN, _p, _viol_tol, feasibility, state_box_of
from .systems import System

_STEP_CONTEXT = object()  # _args placeholder: mpcd_mpc_step normalises x0 into the context itself
_CLIP_RULES = {"chain": N.MPCD_CLIP_CHAIN, "final": N.MPCD_CLIP_FINAL}
_SAMPLERS = {"ddpm_cfg": N.MPCD_DDPM_CFG, "ddpm_cart_pole_sample_fn": N.MPCD_DDPM_CFG,
             "ddim_cfg": N.MPCD_DDIM_CFG, "ddim": N.MPCD_DDIM, "ddim_sample": N.MPCD_DDIM}
_ELITES_NEED_WARM = "elites needs warm_start=K: the elite set seeds the warm-start priors"
_BAD_CLIP_RULE = f"clip_rule must be one of {sorted(_CLIP_RULES)}"
# closed_loop(native=True) and the native mpc_step take neither producer of V: their refusals, by producer
_NO_NATIVE_LOOP = {
    "state_box": "state_box is not available with native=True: folding the constraint into mpcd_closed_loop's fused "
                 "tail is the follow-up; use native=False",
    "constraints": "constraints are not available with native=True: mpcd_closed_loop's fused tail takes no constraint "
                   "set; use native=False"}
_NO_NATIVE_STEP = {
    "state_box": "state_box is not available with native=True: the fused step (mpcd_mpc_step) takes no box; its "
                 "follow-up mpc_step_constr does (Constraints(state_box=...)), or leave native unset",
    "constraints": "constraints are not available with native=True: the fused step (mpcd_mpc_step) takes no constraint "
                   "set; leave native unset or False"}
_NO_WARM_STEP = {
    "state_box": "state_box with warm_start / prior / elites needs the native step, which takes no box: use its "
                 "follow-up mpc_step_constr, or closed_loop(native=False)",
    "constraints": "constraints with warm_start / prior / elites need the native step, which takes no constraint set; "
                   "closed_loop(native=False) combines them"}
_SINGLE_RANK_STEP = {
    "state_box": "state_box is single-rank here: the multi-rank feasibility-first selection is the follow-up "
                 "mpc_step_constr's",
    "constraints": "constraints are single-rank: there is no multi-rank feasibility-first selection"}


def _rows_dev(rows, device, name, M, cols):
    """rows [M, cols] (or [cols] for one state; host values or a device tensor) as a contiguous device float64 tensor,
    checked (M None: any number of rows); None stays None"""
    if rows is None:
        return None
    if torch.is_tensor(rows):
        t = rows.to(device, torch.float64)
    else:
        t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)).to(device)
    t = (t[None] if t.dim() == 1 else t).contiguous()
    if t.dim() != 2 or t.shape[1] != cols or (M is not None and t.shape[0] != M):
        raise ValueError(f"{name} must be [{'M' if M is None else M}, {cols}], got {tuple(t.shape)}")
    return t


def _check_clip_flags(clip_flags, M, device):
    if clip_flags.dtype != torch.int32 or clip_flags.device != device or clip_flags.numel() != M:
        raise ValueError(f"clip_flags must be {M} int32 codes on {device}")


def _group_split(B, M, group, noun):
    """the candidates per state of B rows over M states (default B // M), checked"""
    group = B // M if group is None else int(group)
    if group < 1 or M * group != B:
        raise ValueError(f"u_norm has {B} {noun}: not {M} states x group={group}")
    return group


def _check_inputs(system, d):
    if d != system.n_u:
        raise ValueError(f"system {system.name} has {system.n_u} inputs, samples have {d}")


def _history(T, M, nx, d, dev):
    """closed_loop's device history: states [T + 1, M, n_x], actions [T, M, d], costs and indices [T, M]"""
    f64 = dict(dtype=torch.float64, device=dev)
    return (torch.empty((T + 1, M, nx), **f64), torch.empty((T, M, d), **f64), torch.empty((T, M), **f64),
            torch.empty((T, M), dtype=torch.int64, device=dev))


def _loop_result(xs, us, cs, ix, **more):
    """the history on the host, state-major (the copies wait for the stream)"""
    return ClosedLoopResult(x=xs.transpose(0, 1).cpu().numpy(), u=us.transpose(0, 1).cpu().numpy(),
                            cost=cs.t().cpu().numpy(), index=ix.t().cpu().numpy(), **more)


def philox_noise(n_cand, n_slices, flat, seed=0, global_offset=0, device=None):
    """The samplers' in-kernel noise for candidates [global_offset, global_offset + n_cand) as a device
    tensor [n_slices, n_cand, flat] (slice 0 = x_T, slice k = denoise step k's draw): feeding it back as
    `noise` replays a Philox run in injected-noise mode (mpcd_philox_noise)."""
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    out = torch.empty((int(n_slices), int(n_cand), int(flat)), dtype=torch.float32, device=dev)
    N.check(N.lib().mpcd_philox_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(global_offset), int(n_cand), int(n_slices),
                                      int(flat), _p(out), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
            "mpcd_philox_noise")
    return out


def force_unet_tiling(conv=-1, block=-1):
    """Process-wide U-Net tiling override (mpcd_unet_force_tiling): conv = candidate index for every conv
    (-1: measured), block = fused-block candidate (-1: measured, -2: never fuse)."""
    N.check(N.lib().mpcd_unet_force_tiling(int(conv), int(block)), "mpcd_unet_force_tiling")


UNET_PATHS = {"auto": 0, "layered": 1, "fused": 2}


def force_unet_path(path="auto"):
    """Process-wide U-Net execution form (mpcd_unet_force_path): "auto" (the whole-network fused launch where
    it applies), "layered" (one launch per conv) or "fused" (error where it does not apply)."""
    N.check(N.lib().mpcd_unet_force_path(UNET_PATHS[path]), "mpcd_unet_force_path")


MLP_LAYOUTS = {"auto": -1, "32x8": 0, "16x8": 1, "16x4": 2, "rw32": 3, "rw16": 4, "rw32x8": 5}


def force_mlp_layout(layout="auto"):
    """Process-wide MLP sampler workgroup layout (mpcd_mlp_force_layout): "auto" (by batch size), "32x8",
    "16x8" or "16x4" (rows x waves per workgroup), "rw32" / "rw16" (4 waves, resident 128-wide weights), "rw32x8"
    (the resident-weight kernel on 8 waves, 32 rows)."""
    N.check(N.lib().mpcd_mlp_force_layout(MLP_LAYOUTS[layout]), "mpcd_mlp_force_layout")


@dataclass
class NetSpec:
    """Architecture of the noise-net (temporal_unet.py constructor arguments)."""
    kind: str                 # "mlp" (build-defined CFG MLP) or "unet" (ConditionedTemporalUnet / TemporalUnet)
    state_dim: int            # d
    horizon: int              # H
    context_dim: int          # C (0: TemporalUnet with conditioning None)
    base_dim: int = 32        # unet_input_dim
    dim_mults: tuple = (1, 2, 4)
    time_emb_dim: int = 32
    cfg: bool = True          # 4-arg net with the CFG context mask
    # GEMM numerics (include/mpcd.h mpcd_dtype): "f32" exact fp32 MFMA; "f32x3" fp32-accurate split-bf16
    # MFMA (MLP: shared, grouped (context_group) or no context; UNet: any); "f16" fp16 operands / fp32 accumulate (UNet, cfg 5); "f16x2"
    # two-term fp16 MFMA - NOT fp32 arithmetic: 22-bit operands in the fp16 range (MLP: the CFG-DDPM sampler / eps
    # forward at H*d 32 or 64 with a shared context; U-Net: the fused CFG-DDPM program; the other cases of such a
    # net run its f32x3 kernels). A call that leaves the fp16 range (NaN in the chain) is re-run in f32x3.
    dtype: str = "f32"

    def desc(self):
        d = N.NetDesc()
        d.kind = N.MPCD_NET_MLP if self.kind == "mlp" else N.MPCD_NET_UNET
        d.state_dim, d.horizon, d.context_dim = self.state_dim, self.horizon, self.context_dim
        d.base_dim, d.n_mults = self.base_dim, len(self.dim_mults)
        for i, m in enumerate(self.dim_mults):
            d.mults[i] = m
        d.time_emb_dim = self.time_emb_dim
        d.cfg_masked = 1 if self.cfg else 0
        dtypes = {"f32": N.MPCD_F32, "f16": N.MPCD_F16, "f32x3": N.MPCD_F32X3, "f16x2": N.MPCD_F16X2}
        if self.dtype not in dtypes:
            raise ValueError(f"dtype {self.dtype!r}: use one of {sorted(dtypes)}")
        d.dtype = dtypes[self.dtype]
        return d


@dataclass
class MPCResult:
    u0: np.ndarray          # [d] applied action, unnormalised
    u_best: np.ndarray      # [H, d] winning trajectory, unnormalised
    best_cost: float
    best_index: int         # global candidate index
    costs: torch.Tensor     # [B_total] fp64 on device (all ranks' candidates)
    u_norm: torch.Tensor    # [B_local, H, d] this rank's normalised samples
    flags: int = 0          # mpcd_last_step_flags bits (native step): 1 clipped, 2 NaN in the samples
    elite_index: np.ndarray = None  # [k] int64 global indices of the k best candidates, best first (elites=k)
    elite_cost: np.ndarray = None   # [k] fp64 their costs, nondecreasing (a NaN cost is reported as +inf)
    violation: float = None  # state_box= / constraints=: the selected candidate's violation V (0.0 = admissible)
    n_feasible: int = None   # state_box=: how many candidates have V <= viol_tol (0: the least violating was selected)
    elite_violation: np.ndarray = None  # [k] fp64 mpc_step_constr(elites=k): V of each ranked candidate


@dataclass
class ClosedLoopResult:
    x: np.ndarray           # [M, T+1, n_x] plant states (fp64), x[:, 0] = the initial states
    u: np.ndarray           # [M, T, n_u] applied actions (unnormalised, rounded as requested)
    cost: np.ndarray        # [M, T] cost of the selected candidate at each step
    index: np.ndarray       # [M, T] global index of the selected candidate in that step's batch
    u_norm: torch.Tensor = None  # [M * n, H, d] the last iteration's normalised samples (native=True only)
    violation: np.ndarray = None   # [M, T] state_box=: the selected candidate's box violation V at each step
    n_feasible: np.ndarray = None  # [M, T] state_box=: the state's candidates with V <= viol_tol at each step


@dataclass
class BatchStepResult:
    u: np.ndarray           # [M, n_u] fp64 applied actions (unnormalised, rounded as requested)
    plan: np.ndarray        # [M, H, d] fp32 selected plans, unnormalised with each state's clip flag
    cost: np.ndarray        # [M] cost of the selected candidate as computed (a NaN stays one)
    index: np.ndarray       # [M] global index m * n + j of the selected candidate in this step's batch
    flags: np.ndarray       # [M] int32 MPCD_STEP_CLIPPED | MPCD_STEP_NAN_SAMPLES | MPCD_STEP_NONFINITE_WINNER
    u_norm: torch.Tensor = None  # [M * n, H, d] this step's normalised samples (return_samples=True)
    elite_index: np.ndarray = None  # [M, k] int64 global indices of each state's k best, best first (elites=k)
    elite_cost: np.ndarray = None   # [M, k] fp64 their costs, nondecreasing (a NaN cost is reported as +inf)
    violation: np.ndarray = None    # [M] mpc_step_batch_box / _constr: the selected candidate's violation V (0.0 = admissible)
    n_feasible: np.ndarray = None   # [M] int64 mpc_step_batch_box / _constr: the state's candidates with V <= viol_tol (0: the
                                    # least violating one was selected; the state carries MPCD_STEP_INFEASIBLE)
    elite_violation: np.ndarray = None  # [M, k] mpc_step_batch_box / _constr with elites: V of each ranked candidate


_STATE_RESULT = np.dtype([("cost", "<f8"), ("index", "<i8"), ("flags", "<i4"), ("reserved", "<i4")])
_BEST = np.dtype([("cost", "<f8"), ("index", "<i8")])  # mpcd_best


class DiffusionMPC:
    def __init__(self, spec, params, tables=None, variance_schedule="exponential", n_diffusion_steps=100,
                 device=None, context_limits=None, action_limits=None):
        """params: dict name -> tensor (module state_dict keys, no "model." prefix) in any order.
        tables: dict of the 12 diffusion buffers (e.g. from a checkpoint) or None to compute them."""
        self.spec = spec
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.n_steps = n_diffusion_steps if tables is None else int(tables["betas"].numel())
        self.tables = tables if tables is not None else S.tables(variance_schedule, n_diffusion_steps)
        if not S.is_finite(self.tables):
            raise ValueError(f"{variance_schedule} schedule with N={self.n_steps} is not finite "
                             "(the reference would produce NaN; use 'cosine' or another N)")
        c_lo, c_hi = context_limits if context_limits is not None else (-np.ones(spec.context_dim),
                                                                        np.ones(spec.context_dim))
        a_lo, a_hi = action_limits if action_limits is not None else (-np.ones(spec.state_dim),
                                                                      np.ones(spec.state_dim))
        self.ctx_min = np.ascontiguousarray(c_lo, dtype=np.float32)
        self.ctx_max = np.ascontiguousarray(c_hi, dtype=np.float32)
        self.act_min = np.ascontiguousarray(a_lo, dtype=np.float32)
        self.act_max = np.ascontiguousarray(a_hi, dtype=np.float32)
        self._lib = N.lib()
        self._ctx = ctypes.c_void_p()
        N.check(self._lib.mpcd_create(self.device.index, ctypes.byref(self._ctx)), "mpcd_create")
        self._desc = spec.desc()
        self.param_spec = N.param_spec(self._desc)
        blob = torch.cat([params[n].detach().to("cpu", torch.float32).reshape(-1) for n, _ in self.param_spec])
        for n, shp in self.param_spec:
            if tuple(params[n].shape) != shp:
                raise ValueError(f"{n}: shape {tuple(params[n].shape)} != {shp}")
        blob = blob.contiguous()
        N.check(self._lib.mpcd_load_net(self._ctx, ctypes.byref(self._desc), _p(blob), blob.numel()), "mpcd_load_net")
        tab = S.pack(self.tables)
        std = S.posterior_std(self.tables).contiguous()
        N.check(self._lib.mpcd_set_schedule(self._ctx, _p(tab), self.n_steps, _p(std)), "mpcd_set_schedule")
        # DDPM with clip_denoised ends with x = coef1[0]*clamp(x0) + coef2[0]*x: if coef2[0] == 0 and
        # |coef1[0]| <= 1 + 1e-4 the clip flag over the FINAL samples is provably 0 (clip_rule="final";
        # the reference's chain-wide rule still sees x_T and is computed).
        c1, c2 = float(self.tables["posterior_mean_coef1"][0]), float(self.tables["posterior_mean_coef2"][0])
        self.ddpm_final_in_range = c2 == 0.0 and abs(c1) <= np.float32(1 + 1e-4)
        self._flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._best = torch.zeros(2, dtype=torch.float64, device=self.device)  # mpcd_best {double, int64}

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def from_state_dict(cls, state_dict, spec, **kw):
        """Reference checkpoint layout: "model.<param>" + the 12 schedule buffers (weights-only load)."""
        has_prefix = any(k.startswith("model.") for k in state_dict)
        params = {k[6:] if has_prefix and k.startswith("model.") else k: v for k, v in state_dict.items()}
        tables = None
        if all(k in state_dict for k in S.TABLE_ORDER):
            tables = {k: state_dict[k].detach().cpu().to(torch.float32) for k in S.TABLE_ORDER}
        return cls(spec, params, tables=tables, **kw)

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.mpcd_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ normalisation (A12)
    def normalize_condition(self, x0):
        """LimitsNormalizer.normalize of the fp64 state (normalization.py:149-154), cast to fp32 as the
        net's c_emb.float() does (temporal_unet.py:314). Host-side: C values per control step."""
        x = np.asarray(x0, dtype=np.float64)
        mn = self.ctx_min.astype(np.float64)
        den = (self.ctx_max - self.ctx_min).astype(np.float64)  # fp32 subtraction, then promoted
        return (2 * ((x - mn) / den) - 1).astype(np.float32)

    def unnormalize_states(self, x, clip_flag=None):
        """LimitsNormalizer.unnormalize on device (normalization.py:156-167), global clip rule."""
        x = x.contiguous()
        out = torch.empty_like(x)
        d = x.shape[-1]
        N.check(self._lib.mpcd_unnormalize(self._ctx, _p(x), x.numel() // d, d, self.act_min.ctypes.data,
                                           self.act_max.ctypes.data, _p(clip_flag), _p(out), self._stream()),
                "mpcd_unnormalize")
        return out

    # ------------------------------------------------------------------ sampling (A2-A11)
    def _system_desc(self, system):
        """system.desc() (a ctypes struct), rebuilt only when the system's fields change: a control loop calls
        mpc_step with the same system every step."""
        key = (system.system, system.cost_kind, system.n_x, system.n_u, tuple(system.params), tuple(system.Q),
               tuple(system.R), tuple(system.P), tuple(system.x_ref or ()))
        c = getattr(self, "_desc_cache", None)
        if c is None or c[0] != key:
            c = self._desc_cache = (key, system.desc())
        return c[1]

    def _stream(self):
        # the raw handle of the device's current stream (torch.cuda.current_stream(device).cuda_stream without
        # building a Stream object: this runs once per control step on the host path)
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if raw is not None:
            return ctypes.c_void_p(raw(self.device.index))
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _sampler_id(self, sample_fn):
        name = sample_fn if isinstance(sample_fn, str) else getattr(sample_fn, "__name__", str(sample_fn))
        if name not in _SAMPLERS:
            raise ValueError(f"unsupported sample_fn {name!r}; use one of {sorted(_SAMPLERS)}")
        return _SAMPLERS[name]

    def _ddim_times(self, a):
        """the reference's DDIM time list of a SampleArgs (a DDIM sampler's) with ddim_steps set; self._times keeps it alive"""
        times = S.ddim_times(self.n_steps, a.ddim_steps or None)
        self._times = (ctypes.c_int32 * len(times))(*times)
        a.ddim_times = ctypes.cast(self._times, ctypes.POINTER(ctypes.c_int32))
        a.n_ddim_times = len(times)

    def _plant_block(self, a, desc):
        """sys and the normaliser limits: the head of the step, closed-loop and batched-step argument blocks"""
        a.sys = ctypes.pointer(desc)
        a.ctx_min, a.ctx_max = self.ctx_min.ctypes.data, self.ctx_max.ctypes.data
        a.act_min, a.act_max = self.act_min.ctypes.data, self.act_max.ctypes.data
        return a

    def _noise(self, noise, B, steps):
        """Injected noise on the device, checked to be [steps + 1, B, H, d]: one slice per denoise step of the call
        (fewer after a warm start) and one more. steps: the count, or n_denoise_steps' arguments."""
        H, d = self.spec.horizon, self.spec.state_dim
        if not isinstance(steps, int):
            steps = self.n_denoise_steps(*steps)
        noise = noise.to(self.device, torch.float32).contiguous()
        if tuple(noise.shape) != (steps + 1, B, H, d):
            raise ValueError(f"noise must be [{steps + 1}, {B}, {H}, {d}], got {tuple(noise.shape)}")
        return noise

    def _args(self, sampler, batch, context, w, n_wo_noise, ddim_steps, clamp_x0, seed, global_offset, noise,
              x_out, chain, absmax=None, group=None):
        a = N.SampleArgs()
        if group is not None:  # mpcd_sample_grouped: one context row per `group` consecutive candidates
            if self.spec.context_dim == 0:
                raise ValueError("context_group needs a net with a context")
            if group < 1 or batch % group != 0:
                raise ValueError(f"context_group={group} must be >= 1 and divide n_samples={batch}")
            if context is None or context is _STEP_CONTEXT or context.shape[0] != batch // group:
                rows = None if context is None or context is _STEP_CONTEXT else context.shape[0]
                raise ValueError(f"context rows {rows} must be n_samples / context_group = {batch // group}")
            a.context = context.data_ptr()
        elif self.spec.context_dim > 0 and context is not _STEP_CONTEXT:
            if context is None:
                raise ValueError("this net needs a context")
            a.context = context.data_ptr()
            a.context_shared = 1 if context.shape[0] == 1 else 0
            if not a.context_shared and context.shape[0] != batch:
                raise ValueError(f"context rows {context.shape[0]} must be 1 or n_samples={batch}")
        a.sampler = sampler
        a.batch = batch
        a.w = float(w)
        a.n_wo_noise = int(n_wo_noise)
        a.ddim_steps = int(ddim_steps or 0)
        a.clamp_x0 = 1 if clamp_x0 else 0
        if sampler != N.MPCD_DDPM_CFG:
            self._ddim_times(a)
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        a.global_offset = int(global_offset)
        a.noise = noise.data_ptr() if noise is not None else None
        a.x_out = x_out.data_ptr()
        a.chain_out = chain.data_ptr() if chain is not None else None
        a.chain_absmax = absmax.data_ptr() if absmax is not None else None
        return a

    def _warm(self, x_init, t_start, batch, group=None):
        """(mpcd_warm_start, the prior tensor it points to) of a sample call, checked; t_start 0: a cold start."""
        K = int(t_start)
        if K < 0 or K > self.n_steps:
            raise ValueError(f"t_start={K} must be in [0, {self.n_steps}]")
        w = N.WarmStart()
        w.t_start = K
        if K == 0:
            return w, None
        if x_init is None:
            raise ValueError("t_start > 0 needs x_init (the normalised prior plan)")
        H, d = self.spec.horizon, self.spec.state_dim
        x_init = torch.as_tensor(x_init, dtype=torch.float32)
        if x_init.dim() == 2:
            x_init = x_init[None]
        allowed = [1, batch] + ([batch // group] if group else [])
        if x_init.dim() != 3 or tuple(x_init.shape[1:]) != (H, d) or x_init.shape[0] not in allowed:
            raise ValueError(f"x_init must be [rows, {H}, {d}] with rows one of {sorted(set(allowed))} "
                             f"(1, n_samples{', n_samples / context_group' if group else ''}), got {tuple(x_init.shape)}")
        x_init = x_init.to(self.device).contiguous()
        w.x_init = x_init.data_ptr()
        w.rows = x_init.shape[0]
        return w, x_init

    def shift_plans(self, u_norm, index=None, index_offset=0, out=None):
        """The next warm-start priors (mpcd_shift_plans): out[m, h] = u_norm[index[m] - index_offset, min(h + 1, H - 1)],
        each chosen candidate's normalised plan moved one horizon point ahead with its last point repeated.
        u_norm [B, H, d] device fp32; index: device int64 [M] global candidate indices (closed_loop's / mpc_step's
        winners), None = every row of u_norm. Returns out [M, H, d]."""
        B, H, d = u_norm.shape
        u_norm = u_norm.contiguous()
        M = B if index is None else int(index.numel())
        if index is not None and (index.dtype != torch.int64 or index.device != self.device or not index.is_contiguous()):
            raise ValueError(f"index must be a contiguous int64 tensor on {self.device}")
        if out is None:
            out = torch.empty((M, H, d), dtype=torch.float32, device=self.device)
        N.check(self._lib.mpcd_shift_plans(self._ctx, _p(u_norm), B, H, _p(index), int(index_offset), M, _p(out),
                                           self._stream()), "mpcd_shift_plans")
        return out

    def n_denoise_steps(self, sample_fn="ddpm_cfg", n_wo_noise=0, ddim_steps=None, t_start=None):
        """Denoise steps S of a sample call; t_start=K (warm start, CFG-DDPM): K + n_wo_noise."""
        a = N.SampleArgs()
        a.sampler = self._sampler_id(sample_fn)
        a.n_wo_noise = n_wo_noise
        a.ddim_steps = int(ddim_steps or 0)
        if a.sampler != N.MPCD_DDPM_CFG:
            self._ddim_times(a)
        n = ctypes.c_int32()
        if t_start is None:
            N.check(self._lib.mpcd_sample_steps(self._ctx, ctypes.byref(a), ctypes.byref(n)), "mpcd_sample_steps")
        else:
            if int(t_start) < 0 or int(t_start) > self.n_steps:
                raise ValueError(f"t_start={int(t_start)} must be in [0, {self.n_steps}]")
            w = N.WarmStart()
            w.t_start = int(t_start)
            N.check(self._lib.mpcd_sample_steps_warm(self._ctx, ctypes.byref(a), ctypes.byref(w), ctypes.byref(n)),
                    "mpcd_sample_steps_warm")
        return n.value

    def sample_trajectories(self, context=None, n_samples=1, horizon=None, w=0.01, sample_fn="ddpm_cfg",
                            n_wo_noise=0, ddim_steps=None, clamp_x0=False, seed=0, global_offset=0, noise=None,
                            return_chain=False, out=None, absmax_out=None, context_group=None, x_init=None,
                            t_start=None):
        """Normalised candidate trajectories [B, H, d] (or the chain [S+1, B, H, d]).
        context: [1, C] (shared) or [B, C] normalised fp32; noise: optional injected [S+1, B, H, d].
        context_group=g: context is [B / g, C], candidate b uses row b // g (mpcd_sample_grouped: a closed-loop
        batch of B / g plant states with g candidates each; an f32x3 MLP keeps its split-bf16 kernels, where a
        [B, C] context runs the exact-f32 one). Anything but B / g rows raises ValueError.
        absmax_out: optional fp32 [B] device tensor <- per candidate max |x| over the whole chain
        (x_T .. x_0; NaN if any NaN): the input of the reference's chain-wide clip test without
        materialising the chain.
        t_start=K with x_init (warm start, CFG-DDPM only; mpcd_sample_warm): the chain starts at the prior plan
        x_init noised to level K, x = sqrt_alphas_cumprod[K-1] x_init + sqrt_one_minus_alphas_cumprod[K-1] z0 (the
        reference's q_sample at t = K - 1, z0 = noise slice 0), and runs the last K steps only: S = K + n_wo_noise,
        noise / chain are [S+1, B, H, d] with chain[0] the noised prior. x_init: normalised [1, H, d] (or [H, d]; one
        prior for all), [B, H, d] (one per candidate) or, with context_group=g, [B / g, H, d] (one per context row);
        other shapes raise ValueError. t_start=0 is a cold start through the same entry point; None (default) is
        today's call."""
        H = horizon or self.spec.horizon
        if H != self.spec.horizon:
            raise ValueError(f"net was built for horizon {self.spec.horizon}")
        sampler = self._sampler_id(sample_fn)
        B = int(n_samples)
        d = self.spec.state_dim
        if context is not None:
            context = torch.as_tensor(context, dtype=torch.float32)
            if context.dim() == 1:
                context = context[None]
            context = context.to(self.device).contiguous()
        steps = self.n_denoise_steps(sample_fn, n_wo_noise, ddim_steps, t_start if t_start else None)
        if noise is not None:
            noise = self._noise(noise, B, steps)
        x = out if out is not None else torch.empty((B, H, d), dtype=torch.float32, device=self.device)
        chain = torch.empty((steps + 1, B, H, d), dtype=torch.float32, device=self.device) if return_chain else None
        if absmax_out is not None and (absmax_out.dtype != torch.float32 or absmax_out.numel() != B
                                       or absmax_out.device != self.device or not absmax_out.is_contiguous()):
            raise ValueError(f"absmax_out must be a contiguous fp32 [{B}] tensor on {self.device}")
        # f16x2 numerics compute in the fp16 range: ask for the chain maxima (a NaN there = a value left the range),
        # check them (one synchronisation) and re-run the call with the net's split-bf16 programs if so
        guard = self.spec.dtype == "f16x2"
        amax = absmax_out
        if guard and amax is None:
            amax = torch.empty(B, dtype=torch.float32, device=self.device)
        group = None if context_group is None else int(context_group)
        a = self._args(sampler, B, context, w, n_wo_noise, ddim_steps, clamp_x0, seed, global_offset, noise, x, chain,
                       amax, group)
        warm = None if t_start is None else self._warm(x_init, t_start, B, group)

        def run(what):
            if warm is not None:
                N.check(self._lib.mpcd_sample_warm(self._ctx, ctypes.byref(a), group or 0, ctypes.byref(warm[0]),
                                                   self._stream()), what.replace("mpcd_sample", "mpcd_sample_warm"))
            elif group is None:
                N.check(self._lib.mpcd_sample(self._ctx, ctypes.byref(a), self._stream()), what)
            else:
                N.check(self._lib.mpcd_sample_grouped(self._ctx, ctypes.byref(a), group, self._stream()),
                        what.replace("mpcd_sample", "mpcd_sample_grouped"))

        run("mpcd_sample")
        self.last_f32x3_rerun = False
        if guard and bool(torch.isnan(amax).any()):
            N.check(self._lib.mpcd_force_f32x3(self._ctx, 1), "mpcd_force_f32x3")
            try:
                run("mpcd_sample (f32x3 re-run)")
            finally:
                N.check(self._lib.mpcd_force_f32x3(self._ctx, 0), "mpcd_force_f32x3")
            self.last_f32x3_rerun = True
        return chain if return_chain else x

    def run_CFG(self, context=None, hard_conds=None, context_weight=0.1, n_samples=1, horizon=8,
                return_chain=False, sample_fn="ddpm_cart_pole_sample_fn", n_diffusion_steps_without_noise=0,
                noise=None, seed=0, **_unused):
        """GaussianDiffusionModel.run_CFG (diffusion_model_base.py:394-418): chain [S+1, B, H, d] or
        the final [B, H, d], normalised. hard_conds is ignored as in the reference (commented out there)."""
        return self.sample_trajectories(context, n_samples, horizon, context_weight, sample_fn,
                                        n_diffusion_steps_without_noise, noise=noise, seed=seed,
                                        return_chain=return_chain)

    def eps(self, x, t, context=None):
        """Noise-net forward(s) at time t: (eps_cond, eps_uncond) for a CFG net, (eps, None) otherwise."""
        x = x.to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        if context is not None:
            context = torch.as_tensor(context, dtype=torch.float32).to(self.device).contiguous()
            if context.dim() == 1:
                context = context[None]
        ec = torch.empty_like(x)
        eu = torch.empty_like(x) if self.spec.cfg else None
        N.check(self._lib.mpcd_eps(self._ctx, _p(x), int(t), _p(context),
                                   1 if context is not None and context.shape[0] == 1 else 0, B, _p(ec), _p(eu),
                                   self._stream()), "mpcd_eps")
        return ec, eu

    def unet_form(self, sample_fn="ddpm_cfg"):
        """The U-Net execution form an mpc_step / sample call with this sampler takes (mpcd_unet_form):
        {"fused": bool, "planes": 0 | 1 | 3, "rows_per_workgroup": R, "waves_per_workgroup": W} - the kernel
        bench.py names."""
        out = (ctypes.c_int32 * 4)()
        N.check(self._lib.mpcd_unet_form(self._ctx, self._sampler_id(sample_fn), out), "mpcd_unet_form")
        return {"fused": bool(out[0]), "planes": int(out[1]), "rows_per_workgroup": int(out[2]),
                "waves_per_workgroup": int(out[3])}

    def mlp_layout(self, n_samples):
        """The MLP sampler layout ("32x8", "16x8", "16x4", "rw32", "rw16", "rw32x8") a sample call of n_samples runs."""
        out = ctypes.c_int32()
        with torch.cuda.device(self.device):  # the library decides on the current device's CU count
            N.check(self._lib.mpcd_mlp_layout(int(n_samples), int(self.spec.cfg), ctypes.byref(out)), "mpcd_mlp_layout")
        return {v: k for k, v in MLP_LAYOUTS.items()}[out.value]

    def mlp_form(self, n_samples, sample_fn="ddpm_cfg"):
        """The MLP kernel a shared-context sample call of n_samples runs (mpcd_mlp_form): {"kernel": "f32" | "x3" |
        "h2", "layout": the bf16x3 layout name or None, "rows_per_workgroup": 32 | 16}."""
        out = (ctypes.c_int32 * 3)()
        N.check(self._lib.mpcd_mlp_form(self._ctx, self._sampler_id(sample_fn), int(n_samples), out), "mpcd_mlp_form")
        lay = {v: k for k, v in MLP_LAYOUTS.items()}.get(out[1]) if out[1] >= 0 else None
        return {"kernel": ("f32", "x3", "h2")[out[0]], "layout": lay, "rows_per_workgroup": int(out[2])}

    def mlp_form_grouped(self, n_groups, group, sample_fn="ddpm_cfg"):
        """mlp_form for a sample call with context_group=group over n_groups context rows (mpcd_mlp_form_grouped):
        the kernel is "x3" for an f32x3 / f16x2 net and "f32" for an f32 one, never "h2"."""
        out = (ctypes.c_int32 * 3)()
        N.check(self._lib.mpcd_mlp_form_grouped(self._ctx, self._sampler_id(sample_fn), int(n_groups), int(group), out),
                "mpcd_mlp_form_grouped")
        lay = {v: k for k, v in MLP_LAYOUTS.items()}.get(out[1]) if out[1] >= 0 else None
        return {"kernel": ("f32", "x3", "h2")[out[0]], "layout": lay, "rows_per_workgroup": int(out[2])}

    # Sampler-kernel time of one round of workgroups (one per CU) relative to the exact-f32 kernel's, measured at the
    # cfg2 net shape on an MI355X (profiles/grouped_ab.txt): rw32x8 1.09 ms, rw16 0.757 ms, exact f32 1.68 ms
    _ROUND_COST = {32: 0.65, 16: 0.45}

    def grouped_pays(self, n_groups, group, sample_fn="ddpm_cfg"):
        """Whether a grouped sample call of n_groups x group candidates is expected to beat the same call with one
        context row per candidate. Only an MLP on the split-bf16 kernels can lose: its workgroups hold candidates of
        one group only, so small groups leave them part empty (one candidate per group: 12.0 against 1.68 ms at 4,096
        candidates). Both kernels take (rounds of workgroups over the CUs) x (the time of one round), which is what
        is compared, with the measured round times."""
        if self.spec.kind != "mlp" or self.mlp_form_grouped(n_groups, group, sample_fn)["kernel"] != "x3":
            return True  # the same kernel either way, and no repeated rows to build
        rows = self.mlp_form_grouped(n_groups, group, sample_fn)["rows_per_workgroup"]
        n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        nb = 2 if self.spec.cfg else 1
        wgs = n_groups * -(-group * nb // rows)
        wgs_f32 = -(-n_groups * group * nb // 32)
        return -(-wgs // n_cu) * self._ROUND_COST[rows] < -(-wgs_f32 // n_cu) * 1.0

    def last_sample_ms(self):
        ms = ctypes.c_float()
        N.check(self._lib.mpcd_last_sample_ms(self._ctx, ctypes.byref(ms)), "mpcd_last_sample_ms")
        return ms.value

    def sample_ms_mean(self, n):
        """Mean sampler-kernel time (HIP events) over the last n sample calls (n <= 256), read once after a loop."""
        ms = ctypes.c_float()
        N.check(self._lib.mpcd_sample_ms_mean(self._ctx, int(n), ctypes.byref(ms)), "mpcd_sample_ms_mean")
        return ms.value

    # ------------------------------------------------------------------ rollout / cost / selection (A13-A15)
    def rollout_cost(self, system: System, x0, u_norm, clip_flag=None):
        """fp64 cost per candidate [B] on device."""
        B, H, d = u_norm.shape
        _check_inputs(system, d)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        cost = torch.empty(B, dtype=torch.float64, device=self.device)
        desc = system.desc()
        N.check(self._lib.mpcd_rollout_cost(self._ctx, ctypes.byref(desc), x0.ctypes.data, _p(u_norm.contiguous()),
                                            self.act_min.ctypes.data, self.act_max.ctypes.data, B, H, _p(clip_flag),
                                            _p(cost), self._stream()), "mpcd_rollout_cost")
        return cost

    def clip_flag(self, x):
        flag = torch.empty(1, dtype=torch.int32, device=self.device)
        N.check(self._lib.mpcd_clip_flag(self._ctx, _p(x), x.numel(), _p(flag), self._stream()), "mpcd_clip_flag")
        return flag

    def argmin(self, cost, index_offset=0):
        """Device argmin (NaN = +inf, lowest index on ties) -> (index, cost); syncs the stream."""
        N.check(self._lib.mpcd_argmin(self._ctx, _p(cost), cost.numel(), index_offset, _p(self._best), self._stream()),
                "mpcd_argmin")
        host = self._best.cpu()
        return int(host.view(torch.int64)[1]), float(host[0])

    def _check_elites(self, k, group):
        k = int(k)
        if k < 1 or k > group or k > N.MPCD_MAX_ELITES:
            raise ValueError(f"elites / k = {k} must be in [1, min({group} candidates, {N.MPCD_MAX_ELITES})]")
        return k

    def _topk_raw(self, cost, k, n_groups, index_offset=0):
        """mpcd_topk into a fresh device buffer of mpcd_best records, viewed as int64 [n_groups, k, 2] (cost bits, index)."""
        if cost.dtype != torch.float64 or cost.device != self.device or not cost.is_contiguous():
            raise ValueError(f"cost must be a contiguous float64 tensor on {self.device}")
        M = int(n_groups)
        if M < 1 or cost.numel() < 1 or cost.numel() % M != 0:
            raise ValueError(f"cost has {cost.numel()} entries: not n_groups={M} groups of equal size")
        group = cost.numel() // M
        k = self._check_elites(k, group)
        raw = torch.empty((M, k, 2), dtype=torch.int64, device=self.device)
        N.check(self._lib.mpcd_topk(self._ctx, _p(cost), M, group, k, int(index_offset), _p(raw), self._stream()),
                "mpcd_topk")
        return raw

    def topk(self, cost, k, n_groups=1, index_offset=0):
        """The k best candidates of each of n_groups equal groups of consecutive costs, ranked on the device (mpcd_topk):
        (cost [M, k] float64, index [M, k] int64) device tensors, best first, in argmin()'s order (NaN = +inf and
        reported as +inf, lower cost, then lower index). index = index_offset + the position in `cost`, so [:, 0] is each
        group's argmin / closed_loop's selected index. cost: device float64 [M * group]; 1 <= k <= min(group, 64)."""
        raw = self._topk_raw(cost, k, n_groups, index_offset)
        return raw[..., 0].contiguous().view(torch.float64), raw[..., 1].contiguous()

    def elite_priors(self, u_norm, elite_index, group, shift=True, index_offset=0, out=None):
        """Per-candidate warm-start priors seeded from elite sets (mpcd_elite_priors): for candidate b = m * group + j,
        out[b, h] = u_norm[elite_index[m, j % k] - index_offset, min(h + shift, H - 1)]. shift=True moves each plan one
        horizon point ahead (shift_plans' rule, for the next control step); shift=False copies it (re-sampling within
        one step). u_norm [M * group, H, d] device fp32; elite_index [M, k] device int64 (topk's index). An index outside
        [index_offset, index_offset + M * group) leaves its candidates' rows of `out` as they are. Returns out
        [M * group, H, d], which must not overlap u_norm; hand it to sample_trajectories(x_init=out, t_start=K)."""
        B, H, d = u_norm.shape
        u_norm = u_norm.contiguous()
        group = int(group)
        if elite_index.dim() == 1:
            elite_index = elite_index[None]
        if elite_index.dtype != torch.int64 or elite_index.device != self.device or elite_index.dim() != 2:
            raise ValueError(f"elite_index must be an int64 [M, k] tensor on {self.device}")
        M, k = elite_index.shape
        group = _group_split(B, M, group, "rows")
        self._check_elites(k, group)
        raw = torch.zeros((M, k, 2), dtype=torch.int64, device=self.device)
        raw[..., 1] = elite_index
        return self._elite_priors_raw(u_norm, raw, group, shift, index_offset, out)

    def _elite_priors_raw(self, u_norm, raw, group, shift, index_offset, out):
        B, H, d = u_norm.shape
        if out is None:
            out = torch.empty((B, H, d), dtype=torch.float32, device=self.device)
        elif (tuple(out.shape) != (B, H, d) or out.dtype != torch.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous fp32 [{B}, {H}, {d}] tensor on {self.device}")
        N.check(self._lib.mpcd_elite_priors(self._ctx, _p(u_norm), raw.shape[0], group, H, _p(raw), raw.shape[1],
                                            int(index_offset), 1 if shift else 0, _p(out), self._stream()),
                "mpcd_elite_priors")
        return out

    # ------------------------------------------------------------------ state constraints
    _state_box = staticmethod(state_box_of)

    def _clip_flags(self, src, M, per_state, flags):
        """mpcd_clip_flags: flags[m] <- LimitsNormalizer's clip code over state m's per_state consecutive values of src"""
        N.check(self._lib.mpcd_clip_flags(self._ctx, _p(src), M, per_state, _p(flags), self._stream()), "mpcd_clip_flags")

    def _rollout_feasible(self, system, x0_states, u_norm, group, clip_flags, feas=None, **spec):
        """rollout_cost_box / rollout_cost_constr: one body. feas: the call's Feasibility, or None to build it from
        **spec (feasibility()'s arguments) once the shapes are checked."""
        B, H, d = u_norm.shape
        _check_inputs(system, d)
        x = _rows_dev(x0_states, self.device, "x0_states", None, system.n_x)
        M = x.shape[0]
        group = _group_split(B, M, group, "candidates")
        if feas is None:
            feas = feasibility(system, **spec)
        up = _rows_dev(feas.u_prev, self.device, "u_prev", M, d)
        u_norm = u_norm.contiguous()
        if clip_flags is None:
            clip_flags = torch.empty(M, dtype=torch.int32, device=self.device)
            self._clip_flags(u_norm, M, group * H * d, clip_flags)
        else:
            _check_clip_flags(clip_flags, M, self.device)
        cost = torch.empty(B, dtype=torch.float64, device=self.device)
        viol = torch.empty(B, dtype=torch.float64, device=self.device)
        feas.rollout(self, system.desc(), x, group, u_norm, clip_flags, cost, viol, up)
        return cost, viol

    def rollout_cost_box(self, system: System, x0_states, u_norm, state_box, group=None, clip_flags=None):
        """rollout_cost for M start states with a state box (mpcd_rollout_cost_box): (cost [B], violation [B]) device
        float64 tensors. Candidate b of u_norm [B, H, d] starts from x0_states[b // group] ([M, n_x], or [n_x] for one
        state; host values or a device float64 tensor); group defaults to B // M. cost is bit for bit what the rollout
        without a box computes. violation[b] = max(0, the largest excess of any component of any state the candidate's
        cost evaluation visits over state_box = (lo, hi)), None entries = unbounded; the start state is not tested; +inf
        where an excess is NaN. clip_flags: device int32 [M] clip codes (one per state); default: LimitsNormalizer's
        rule over each state's own candidates of u_norm."""
        return self._rollout_feasible(system, x0_states, u_norm, group, clip_flags, kind="state_box", state_box=state_box)

    def rollout_cost_constr(self, system: System, x0_states, u_norm, constraints, group=None, clip_flags=None, u_prev=None):
        """rollout_cost_box with a constraint set (mpcd_rollout_cost_constr): (cost [B], violation [B]) device float64
        tensors. constraints: a Constraints; violation[b] = max(0, every excess of the box, the rows and the rate bounds
        over the pairs (x_{k+1}, u_k) the candidate's cost evaluation visits), +inf where an excess is NaN. u_prev
        [M, n_u] (host values or a device float64 tensor; [n_u] for one state): each state's previous applied action,
        the predecessor of u_0 in the rate test; None, or a row with a NaN: that state's rate test starts at u_1.
        x0_states, group, clip_flags: rollout_cost_box's. cost is bit for bit the unconstrained rollout's."""
        return self._rollout_feasible(system, x0_states, u_norm, group, clip_flags, kind="constraints",
                                      constraints=constraints, u_prev=u_prev)

    def _topk_feasible_raw(self, cost, viol, k, n_groups, tol, index_offset=0):
        """mpcd_topk_feasible: (mpcd_best records as int64 [M, k, 2] (cost bits, index), violation [M, k], n_feasible [M])"""
        for name, t in (("cost", cost), ("violation", viol)):
            if t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float64 tensor on {self.device}")
        M = int(n_groups)
        if M < 1 or cost.numel() < 1 or cost.numel() % M != 0 or viol.numel() != cost.numel():
            raise ValueError(f"cost / violation have {cost.numel()} / {viol.numel()} entries: not n_groups={M} groups of "
                             "equal size each")
        group = cost.numel() // M
        k = self._check_elites(k, group)
        raw = torch.empty((M, k, 2), dtype=torch.int64, device=self.device)
        vk = torch.empty((M, k), dtype=torch.float64, device=self.device)
        nf = torch.empty(M, dtype=torch.int64, device=self.device)
        N.check(self._lib.mpcd_topk_feasible(self._ctx, _p(cost), _p(viol), M, group, k, _viol_tol(tol), int(index_offset),
                                             _p(raw), _p(vk), _p(nf), self._stream()), "mpcd_topk_feasible")
        return raw, vk, nf

    def topk_feasible(self, cost, violation, k, n_groups=1, tol=0.0, index_offset=0):
        """topk in the feasibility-first order (mpcd_topk_feasible): (index [M, k] int64, cost [M, k], violation [M, k],
        n_feasible [M] int64) device tensors. A candidate is feasible iff violation <= tol; every feasible candidate
        ranks before every infeasible one; feasible ones by (cost, index), infeasible ones by (violation, cost, index);
        NaN costs and violations rank and are reported as +inf. n_feasible counts the feasible candidates of the whole
        group: where it is 0 there is no admissible plan and entry 0 is the least violating one."""
        raw, vk, nf = self._topk_feasible_raw(cost, violation, k, n_groups, tol, index_offset)
        return raw[..., 1].contiguous(), raw[..., 0].contiguous().view(torch.float64), vk, nf

    def _control_step_picked_raw(self, desc, x, u_norm, raw, index_offset, flags, decimals, u_out, i_out, c_out):
        B, H, _ = u_norm.shape
        N.check(self._lib.mpcd_control_step_picked(
            self._ctx, ctypes.byref(desc), _p(x), raw.shape[0], _p(u_norm), B, H, _p(raw), raw.shape[1], int(index_offset),
            self.act_min.ctypes.data, self.act_max.ctypes.data, _p(flags), -1 if decimals is None else int(decimals),
            _p(u_out), _p(i_out), _p(c_out), self._stream()), "mpcd_control_step_picked")

    def control_step_picked(self, system: System, x_states, u_norm, index, cost, clip_flags, decimals=4, index_offset=0):
        """One control step with the selection supplied (mpcd_control_step_picked): state m applies candidate index[m] -
        index_offset of u_norm [B, H, d] - its first action unnormalised with clip_flags[m] and rounded to `decimals`
        places (None: not rounded) - and x_states (device float64 [M, n_x]) is stepped IN PLACE. index [M] int64 and
        cost [M] float64 are device tensors, e.g. column 0 of topk_feasible. Returns (u_applied [M, n_u], best_index [M],
        best_cost [M]) device tensors. An index outside the batch leaves its state alone: u_applied NaN, best_index -1,
        best_cost +inf."""
        B, H, d = u_norm.shape
        if (not torch.is_tensor(x_states) or x_states.dtype != torch.float64 or x_states.device != self.device
                or x_states.dim() != 2 or x_states.shape[1] != system.n_x or not x_states.is_contiguous()):
            raise ValueError(f"x_states must be a contiguous float64 [M, {system.n_x}] tensor on {self.device}")
        M = x_states.shape[0]
        _check_inputs(system, d)
        if index.dtype != torch.int64 or index.device != self.device or index.numel() != M:
            raise ValueError(f"index must be {M} int64 entries on {self.device}")
        if cost.dtype != torch.float64 or cost.device != self.device or cost.numel() != M:
            raise ValueError(f"cost must be {M} float64 entries on {self.device}")
        _check_clip_flags(clip_flags, M, self.device)
        raw = torch.empty((M, 1, 2), dtype=torch.int64, device=self.device)
        raw[:, 0, 0] = cost.reshape(M).view(torch.int64)
        raw[:, 0, 1] = index.reshape(M)
        u_out = torch.empty((M, d), dtype=torch.float64, device=self.device)
        i_out = torch.empty(M, dtype=torch.int64, device=self.device)
        c_out = torch.empty(M, dtype=torch.float64, device=self.device)
        self._control_step_picked_raw(system.desc(), x_states, u_norm.contiguous(), raw, index_offset, clip_flags, decimals,
                                      u_out, i_out, c_out)
        return u_out, i_out, c_out

    def _check_modes(self, K, sample_fn, select, clip_rule, elites, n, native=False):
        """closed_loop's and the batched step's refusals over warm_start=K, select, clip_rule and elites; n: the
        candidates per state the elite count is checked against (None: not yet). Returns the checked elite count."""
        if elites is not None:
            if K is None:
                raise ValueError(_ELITES_NEED_WARM)
            if native:
                raise ValueError("elites is not available with native=True: mpcd_closed_loop's fused tail writes one "
                                 "prior per state; use native=False")
            if select != "argmin":
                raise ValueError("elites ranks candidates by cost: it needs select='argmin'")
            if n is not None:
                elites = self._check_elites(elites, n)
        if K is not None and (K < 1 or K > self.n_steps or self._sampler_id(sample_fn) != N.MPCD_DDPM_CFG):
            raise ValueError(f"warm_start={K} needs 1 <= K <= {self.n_steps} and the CFG-DDPM sampler")
        if select not in ("argmin", "first"):
            raise ValueError("select must be 'argmin' or 'first'")
        if clip_rule not in _CLIP_RULES:
            raise ValueError(_BAD_CLIP_RULE)
        return elites

    def _check_plant(self, system, nx, what):
        """a call that conditions on the plant state (`what`, for the text): states of nx columns against the planning
        model and the net"""
        if nx != system.n_x or system.n_u != self.spec.state_dim:
            raise ValueError(f"system {system.name}: n_x={system.n_x}, n_u={system.n_u}; states have {nx} columns, "
                             f"the net samples {self.spec.state_dim} actions")
        if self.spec.context_dim != nx:
            raise ValueError(f"{what} conditions on the plant state: context_dim {self.spec.context_dim} != n_x {nx}")

    def closed_loop(self, x0_states, system: System, iterations, n_samples=1, w=0.01, sample_fn="ddpm_cfg",
                    n_wo_noise=0, ddim_steps=None, clamp_x0=False, select="argmin", decimals=4, seed=0, noise=None,
                    clip_rule="chain", grouped=False, warm_start=None, native=False, elites=None, state_box=None,
                    viol_tol=0.0, constraints=None, u_prev=None):
        """Closed-loop diffusion MPC for M plant states at once, resident on the device.
        The reference runs one initial state at a time on the host (Cart_Diffusion_inference.py:405-512:
        normalize_condition -> run_CFG -> unnormalize -> u0 = round(u[0], 4) -> x = f(x, u0), repeated
        ITERATIONS times per initial state). Here every iteration is: per-state contexts
        (mpcd_normalize_states), n_samples candidates per state in one sampler launch, per-state clip flags,
        rollout + cost from each state's own x, and mpcd_control_step (per-state selection, u0, plant step);
        nothing returns to the host until the end. select: "argmin" (lowest cost) or "first" (candidate 0 of
        each group: the reference scripts with n_samples = 1). grouped=False (the default) hands the sampler one
        context row per candidate (each state's row repeated n_samples times): an MLP then runs the exact-f32
        kernel whatever spec.dtype says. grouped=True hands it the [M, C] rows with context_group=n_samples
        (mpcd_sample_grouped): an f32x3 or f16x2 MLP runs the split-bf16 kernels with workgroups aligned to the
        states, each state's samples bit-identical to a shared-context call for that state; an f32 MLP and a
        U-Net compute what grouped=False computes. Measured at 4,096 candidates (profiles/grouped_ab.txt): 64 x 64
        and 256 x 16 take the shared-context time, 1.07 - 1.10 ms against 1.68 ms per candidate, but the part-empty
        workgroups of small groups lose (4,096 x 1: 12.0 ms), so grouped=True falls back to per-candidate rows
        where grouped_pays() says so. noise: optional callable it -> injected sampler
        noise [S+1, M*n_samples, H, d] (parity tests); default in-kernel Philox keyed by (seed + it).
        clip_rule: "chain" (the reference: run_CFG(return_chain=True) then unnormalize_states of the whole
        chain, so each state's clip test also sees its x_T) or "final" (the final samples only).
        warm_start=K (CFG-DDPM, 1 <= K <= N): iteration 0 samples cold; after every control step each state's
        selected plan, moved one horizon point ahead (mpcd_shift_plans on the step's winners), becomes its prior, and
        the later iterations sample from it with t_start=K (see sample_trajectories): K + n_wo_noise denoise steps
        instead of N + n_wo_noise. grouped=True where grouped_pays(): the [M, H, d] priors go in as they are; else
        they are repeated per candidate like the contexts. noise(it) must then return K + n_wo_noise + 1 slices for
        it >= 1. Under clip_rule="chain" a warm iteration's clip test sees the noised prior, not x_T.
        native=True: the whole loop is ONE library call (mpcd_closed_loop) - per iteration the sampler and one fused
        launch for the clip code, rollout, cost, selection, plant step, history rows and the next context row / prior -
        with results bit for bit those of native=False (the default, the composed calls above). noise(it) is then
        evaluated for every iteration up front, and the result's u_norm holds the last iteration's samples. An f16x2
        spec raises ValueError: its range guard reads the chain maxima on the host in every iteration, the round trip
        the native loop removes.
        elites=k (with warm_start, select="argmin", native=False; 1 <= k <= min(n_samples, 64)): after every control
        step each state's k best plans are ranked on the device (mpcd_topk) and candidate j of the state is seeded from
        elite j % k, moved one horizon point ahead (mpcd_elite_priors): the next iteration samples from [M * n, H, d]
        priors, one per candidate, instead of one per state. elites=1 computes what warm_start alone computes. The
        fused tail of native=True writes one prior per state: elites there raises ValueError.
        state_box=(lo, hi) (None entries = unbounded; native=False, select="argmin"), viol_tol >= 0: feasibility-first
        selection. Per iteration, after the sampler and the clip flags: mpcd_rollout_cost_box (cost and box
        violation of every candidate), mpcd_topk_feasible with k = elites or 1, mpcd_control_step_picked on entry 0, and
        the next priors from the same ranked list (shift_plans on entry 0's index, or elite_priors: the elites are
        feasibility-first too). The result carries violation / n_feasible [M, T]: where n_feasible is 0 no candidate
        stayed in the box and the least violating one was applied. The fused tail of native=True takes no box: it
        raises ValueError, as does select="first".
        constraints=Constraints(...) (instead of state_box, which goes into the set): the same loop with
        mpcd_rollout_cost_constr as the producer of V - the box, linear rows over (x_{k+1}, u_k) and input-rate bounds.
        u_prev [M, n_u] or None is each state's previous applied action for iteration 0 (a NaN row: none); every later
        iteration's is the previous iteration's applied (rounded) action, read on the device. Same refusals."""
        K = None if warm_start is None else int(warm_start)
        feas = feasibility(system, state_box, constraints, viol_tol, u_prev,
                           refuse=((native, _NO_NATIVE_LOOP), (select != "argmin", NEEDS_ARGMIN)))
        elites = self._check_modes(K, sample_fn, select, clip_rule, elites, int(n_samples), native)
        x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(x0_states, dtype=np.float64)))
        M, nx = x0.shape
        self._check_plant(system, nx, "closed loop")
        T, n, H, d = int(iterations), int(n_samples), self.spec.horizon, self.spec.state_dim
        B, dev, st = M * n, self.device, self._stream()
        if native:
            return self._closed_loop_native(x0, system, T, n, w, sample_fn, n_wo_noise, ddim_steps, clamp_x0, select,
                                            decimals, seed, noise, clip_rule, grouped, K)
        desc = system.desc()
        x = torch.from_numpy(x0).to(dev)
        xs, us, cs, ix = _history(T, M, nx, d, dev)
        ctx = torch.empty((M, nx), dtype=torch.float32, device=dev)
        flags = torch.empty(M, dtype=torch.int32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        absmax = torch.empty(B, dtype=torch.float32, device=dev) if clip_rule == "chain" else None
        grouped = bool(grouped) and self.grouped_pays(M, n, sample_fn)
        priors = None
        if K is not None:  # one prior per state, or (elites) one per candidate
            priors = torch.empty((M if elites is None else B, H, d), dtype=torch.float32, device=dev)
        if feas is not None:
            viol = torch.empty(B, dtype=torch.float64, device=dev)
            vs = torch.empty((T, M), dtype=torch.float64, device=dev)
            nfs = torch.empty((T, M), dtype=torch.int64, device=dev)
            up = _rows_dev(feas.u_prev, dev, "u_prev", M, d)
        xs[0] = x
        for it in range(T):
            warm = {}
            if K is not None and it > 0:
                per_row = elites is not None or grouped  # the sampler takes the priors as they are
                warm = dict(x_init=priors if per_row else priors.repeat_interleave(n, dim=0), t_start=K)
            N.check(self._lib.mpcd_normalize_states(self._ctx, _p(x), M, nx, self.ctx_min.ctypes.data,
                                                    self.ctx_max.ctypes.data, _p(ctx), st), "mpcd_normalize_states")
            self.sample_trajectories(ctx if grouped else ctx.repeat_interleave(n, dim=0), B, H, w, sample_fn, n_wo_noise,
                                     ddim_steps, clamp_x0, seed + it, 0, None if noise is None else noise(it), False,
                                     out=u_norm, absmax_out=absmax, context_group=n if grouped else None, **warm)
            if absmax is not None:  # each state's flag over its candidates' chains
                self._clip_flags(absmax, M, n, flags)
            else:
                self._clip_flags(u_norm, M, n * H * d, flags)
            if feas is None:
                N.check(self._lib.mpcd_rollout_cost_grouped(self._ctx, ctypes.byref(desc), _p(x), n, _p(u_norm),
                                                            self.act_min.ctypes.data, self.act_max.ctypes.data, B, H,
                                                            _p(flags), _p(cost), st), "mpcd_rollout_cost_grouped")
                N.check(self._lib.mpcd_control_step(self._ctx, ctypes.byref(desc), _p(x), M, n, _p(u_norm), H, _p(cost),
                                                    self.act_min.ctypes.data, self.act_max.ctypes.data, _p(flags),
                                                    1 if select == "first" else 0, -1 if decimals is None else int(decimals),
                                                    _p(us[it]), _p(ix[it]), _p(cs[it]), st), "mpcd_control_step")
                raw = None if elites is None else self._topk_raw(cost, elites, M)
            else:  # feasibility-first: one ranked list serves the selection and the next priors
                # the predecessor of u_0 in a set's rate test: the action the plant received last
                feas.rollout(self, desc, x, n, u_norm, flags, cost, viol, up if it == 0 else us[it - 1])
                raw, vk, nf = self._topk_feasible_raw(cost, viol, elites or 1, M, feas.tol)
                self._control_step_picked_raw(desc, x, u_norm, raw, 0, flags, decimals, us[it], ix[it], cs[it])
                vs[it], nfs[it] = vk[:, 0], nf
            if elites is not None:
                self._elite_priors_raw(u_norm, raw, n, True, 0, priors)
            elif K is not None:
                self.shift_plans(u_norm, ix[it], 0, out=priors)
            xs[it + 1] = x
        more = {} if feas is None else dict(violation=vs.t().cpu().numpy(), n_feasible=nfs.t().cpu().numpy())
        return _loop_result(xs, us, cs, ix, **more)

    def _closed_loop_native(self, x0, system, T, n, w, sample_fn, n_wo_noise, ddim_steps, clamp_x0, select, decimals,
                            seed, noise, clip_rule, grouped, K):
        """closed_loop(native=True): one mpcd_closed_loop call; the arguments are closed_loop's, already checked."""
        if self.spec.dtype == "f16x2":
            raise ValueError("closed_loop(native=True) does not take an f16x2 spec: its range guard reads the chain "
                             "maxima on the host in every iteration, the round trip the native loop removes")
        M, nx = x0.shape
        H, d, B, dev = self.spec.horizon, self.spec.state_dim, M * n, self.device
        noises = None
        if noise is not None:  # evaluated up front and kept alive until the results are on the host
            cold = self.n_denoise_steps(sample_fn, n_wo_noise, ddim_steps)
            later = cold if K is None else self.n_denoise_steps(sample_fn, n_wo_noise, ddim_steps, K)
            noises = [self._noise(noise(it), B, cold if it == 0 else later) for it in range(T)]
        grouped = bool(grouped) and self.grouped_pays(M, n, sample_fn)
        x = torch.from_numpy(x0).to(dev)
        xs, us, cs, ix = _history(T, M, nx, d, dev)
        desc = system.desc()
        a = self._plant_block(N.ClosedLoopArgs(), desc)
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        a.sample = self._args(self._sampler_id(sample_fn), B, _STEP_CONTEXT, w, n_wo_noise, ddim_steps, clamp_x0, seed, 0,
                              None, u_norm, None)
        a.sample.x_out = None  # ignored by the call: it samples into its workspace and copies the last iteration out
        a.u_norm = u_norm.data_ptr()
        a.n_states, a.group, a.iterations = M, n, T
        a.group_contexts = 1 if grouped else 0
        if noises is not None:
            ptrs = (ctypes.c_void_p * T)(*[z.data_ptr() for z in noises])
            a.noise_iters = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        a.clip_rule = _CLIP_RULES[clip_rule]
        a.select_first = 1 if select == "first" else 0
        a.decimals = -1 if decimals is None else int(decimals)
        a.warm_t_start = 0 if K is None else K
        a.x_dev, a.x_hist, a.u_hist = x.data_ptr(), xs.data_ptr(), us.data_ptr()
        a.cost_hist, a.index_hist = cs.data_ptr(), ix.data_ptr()
        N.check(self._lib.mpcd_closed_loop(self._ctx, ctypes.byref(a), self._stream()), "mpcd_closed_loop")
        res = _loop_result(xs, us, cs, ix, u_norm=u_norm)
        del noises  # the copies above waited for the loop: its inputs may go now
        return res

    def mpc_step_batch(self, x_states, system: System, n_samples, w=0.01, sample_fn="ddpm_cfg", n_wo_noise=0,
                       ddim_steps=None, clamp_x0=False, seed=0, noise=None, select="argmin", decimals=4,
                       clip_rule="chain", grouped=False, warm_start=None, reset=None, return_samples=False,
                       allow_nonfinite=False, elites=None, state_box=None):
        """One control step for M plant states that arrive from OUTSIDE (a vectorised simulator, a plant with model
        mismatch, a fleet of devices): ONE library call (mpcd_mpc_step_batch) - one upload of the [M, n_x] fp64
        states, the sampler over M * n_samples candidates, one fused launch (batch_step_tail_kernel) for each state's
        clip code, rollout, cost, selection, u0, selected plan and next prior, and one download of the packed
        results. `system` is the PLANNING model; no plant step is taken. Given a closed_loop iteration's states and
        its seed (seed + it) the step returns that iteration's u, cost and index bit for bit.
        select, decimals, clip_rule, noise ([S + 1, M * n_samples, H, d], this step's): closed_loop's.
        grouped=True: mpcd_sample_grouped on the [M, C] context rows where grouped_pays() (closed_loop's rule).
        warm_start=K (CFG-DDPM, 1 <= K <= N): the planner keeps one normalised prior per state on the device,
        [M, H, d], separate from mpc_step's single prior. The first such call, and any call after M changed, samples
        cold and fills the set; later calls sample with t_start=K from it and refresh it with each state's selected
        plan moved one horizon point ahead (mpcd_shift_plans' rule). batch_priors() returns the set,
        set_batch_priors() replaces it, reset_warm_start() drops it.
        reset: bool [M], the states whose episode restarted (the normal case in a vectorised simulator). Those are
        sampled cold in a library call of their own and the others warm in theirs; priors are gathered for the two
        calls and scattered back, results merged in state order (index and u_norm as of one M * n_samples batch).
        Philox numbering then follows each sub-call's own batch (candidate j of the k-th reset state draws what
        candidate k * n_samples + j of a cold call of the reset states alone draws), and injected noise is a pair
        (noise of the cold call, noise of the warm call).
        A state without a finite cost carries MPCD_STEP_NONFINITE_WINNER and the call raises MpcdError
        (MPCD_ENONFINITE) unless allow_nonfinite=True, which returns the result with its flags (the other states'
        entries are valid); either way the kept priors are dropped, so the next step is cold.
        elites=k (with warm_start and select="argmin"; 1 <= k <= min(n_samples, 64)): the same single call
        (mpcd_mpc_step_batch_elite) also ranks each state's k best candidates inside the fused launch and keeps one prior
        per candidate, [M, n_samples, H, d]: candidate j of a state is seeded from the state's elite j % k, moved one
        horizon point ahead (one mpcd_elite_priors launch after the tail). The result carries elite_index / elite_cost
        [M, k] (topk()'s order and cost reporting; column 0 is `index`). The first such call, and any after M or
        n_samples changed, samples cold. A stored [M, H, d] set seeds every candidate of a state from its one prior; a
        call without elites after one with them starts from row 0 of each state, the winner's (as warm_prior() does).
        elites=1 computes what warm_start alone computes.
        state_box: raises ValueError. This method selects by cost alone; mpc_step_batch_box is the same step with a
        state box."""
        if state_box is not None:
            raise ValueError("mpc_step_batch takes no state_box: the constrained one-call step that was the follow-up "
                             "is mpc_step_batch_box(x_states, system, n_samples, state_box, viol_tol)")
        return self._mpc_step_batch(x_states, system, n_samples, w, sample_fn, n_wo_noise, ddim_steps, clamp_x0, seed,
                                    noise, select, decimals, clip_rule, grouped, warm_start, reset, return_samples,
                                    allow_nonfinite, elites)

    def mpc_step_batch_box(self, x_states, system: System, n_samples, state_box, viol_tol=0.0, **kw):
        """mpc_step_batch with a state box: still ONE library call (mpcd_mpc_step_batch_box) - one upload, the sampler,
        one fused launch (batch_step_box_tail_kernel), with elites the one mpcd_elite_priors launch, one download.
        Inside the fused launch every candidate's rollout also reports its violation V of state_box = (lo, hi) (None
        entries = unbounded; rollout_cost_box's definition), and the selection and the elite ranking follow
        topk_feasible's feasibility-first order with tol = viol_tol: every candidate with V <= viol_tol before every
        other one, those by (cost, index), the others by (V, cost, index). index, cost, violation, n_feasible and the
        elite lists are bit for bit what rollout_cost_box + topk_feasible give on the step's samples, u and the plan
        what control_step_picked applies for that pick, the kept priors shift_plans / elite_priors on that ranking.
        **kw: mpc_step_batch's own keywords (w, sample_fn, n_wo_noise, ddim_steps, clamp_x0, seed, noise, decimals,
        clip_rule, grouped, warm_start, elites, reset, return_samples, allow_nonfinite), with the same meaning and the
        same kept prior set (batch_priors(), set_batch_priors(), reset_warm_start()): a fleet may switch between the
        two methods. select="first" raises ValueError.
        The result carries violation [M], n_feasible [M] and, with elites, elite_violation [M, k]. Where n_feasible is
        0 no candidate stayed in the box: the least violating plan is returned and the state's flags carry
        MPCD_STEP_INFEASIBLE - not an error; the caller decides whether to apply it. An all-infinite box with
        viol_tol=0 returns mpc_step_batch's results bit for bit."""
        feas = feasibility(system, state_box, viol_tol=viol_tol, kind="state_box",
                           refuse=((kw.get("select", "argmin") != "argmin", NEEDS_ARGMIN),))
        return self._mpc_step_batch(x_states, system, n_samples, feas=feas, **kw)

    def mpc_step_batch_constr(self, x_states, system: System, n_samples, constraints, viol_tol=0.0, u_prev=None, **kw):
        """mpc_step_batch_box with a constraint set in place of the box: still ONE library call
        (mpcd_mpc_step_batch_constr; the fused launch is batch_step_box_tail_kernel<SYS, ConTolK>). constraints: a Constraints (box,
        linear rows over (x_{k+1}, u_k), input-rate bounds); V and everything ranked by it are bit for bit
        rollout_cost_constr + topk_feasible on the step's samples. u_prev [M, n_u] or None: each state's previous
        applied action (the predecessor of u_0 in the rate test; a NaN row: none), uploaded with the states in the one
        copy. A state named by `reset` whose row the caller left out (u_prev=None) has none. **kw, the kept prior set,
        the `reset` split and the result fields: mpc_step_batch_box's."""
        x = np.asarray(x_states, dtype=np.float64)
        feas = feasibility(system, None, constraints, viol_tol, u_prev, kind="constraints",
                           refuse=((kw.get("select", "argmin") != "argmin", NEEDS_ARGMIN),),
                           u_prev_shape=(1 if x.ndim == 1 else x.shape[0], system.n_u))
        return self._mpc_step_batch(x_states, system, n_samples, feas=feas, **kw)

    def _mpc_step_batch(self, x_states, system, n_samples, w=0.01, sample_fn="ddpm_cfg", n_wo_noise=0, ddim_steps=None,
                        clamp_x0=False, seed=0, noise=None, select="argmin", decimals=4, clip_rule="chain", grouped=False,
                        warm_start=None, reset=None, return_samples=False, allow_nonfinite=False, elites=None, feas=None):
        """mpc_step_batch, mpc_step_batch_box and mpc_step_batch_constr (feas: their Feasibility, with host u_prev rows):
        one body, one kept prior set"""
        K, n = None if warm_start is None else int(warm_start), int(n_samples)
        elites = self._check_modes(K, sample_fn, select, clip_rule, elites, n if n >= 1 else None)  # (n < 1: refused below)
        if self.spec.dtype == "f16x2":
            raise ValueError("mpc_step_batch does not take an f16x2 spec: its range guard reads the chain maxima on "
                             "the host and re-runs the sampler, a second round trip inside the step")
        x = np.asarray(x_states, dtype=np.float64)
        if x.ndim == 1:
            x = x[None]
        if x.ndim != 2 or x.shape[0] < 1:
            raise ValueError(f"x_states must be [M, n_x], got {x.shape}")
        x = np.ascontiguousarray(x)
        M, nx = x.shape
        self._check_plant(system, nx, "the step")
        if n < 1:
            raise ValueError(f"n_samples={n} must be >= 1")
        mask = None
        if reset is not None:
            mask = np.asarray(reset)
            if mask.dtype != np.bool_ or mask.shape != (M,):
                raise ValueError(f"reset must be a bool mask [{M}], got {mask.dtype} {mask.shape}")
        H, d = self.spec.horizon, self.spec.state_dim
        kw = dict(system=system, n=n, w=w, sample_fn=sample_fn, n_wo_noise=n_wo_noise, ddim_steps=ddim_steps,
                  clamp_x0=clamp_x0, seed=seed, select=select, decimals=decimals, clip_rule=clip_rule, grouped=grouped,
                  return_samples=return_samples, elites=elites)
        priors = getattr(self, "_batch_priors", None) if K is not None else None
        if priors is not None and priors.shape[0] != M:
            priors = None  # the fleet changed size: a cold start
        if priors is not None and elites is None and priors.dim() == 4:
            priors = priors[:, 0].contiguous()  # an elite set: each state's winner
        elif priors is not None and elites is not None:
            if priors.dim() == 3:  # one prior per state seeds all its candidates
                priors = priors[:, None].expand(M, n, H, d).contiguous()
            elif priors.shape[1] != n:
                priors = None  # another candidate count: a cold start
        pshape = (H, d) if elites is None else (n, H, d)
        split = K is not None and priors is not None and mask is not None and mask.any() and not mask.all()
        if isinstance(noise, (tuple, list)) != split:
            raise ValueError("noise is a pair (cold call's, warm call's) exactly when `reset` names some but not all "
                             "states of a warm step")
        if not split:
            warm = K is not None and priors is not None and not (mask is not None and mask.all())
            if K is not None and not warm:
                priors = torch.empty((M,) + pshape, dtype=torch.float32, device=self.device)
            res, bad = self._batch_step_call(x, K if warm else 0, priors, noise, feas=feas, **kw)
        else:
            ic, iw = np.flatnonzero(mask), np.flatnonzero(~mask)
            tc, tw = torch.from_numpy(ic).to(self.device), torch.from_numpy(iw).to(self.device)
            pc = torch.empty((len(ic),) + pshape, dtype=torch.float32, device=self.device)
            pw = priors.index_select(0, tw)
            fc, fw = (None, None) if feas is None else (feas.restrict(ic), feas.restrict(iw))  # their u_prev rows
            rc_, bad_c = self._batch_step_call(x[ic], 0, pc, noise[0], feas=fc, **kw)
            rw_, bad_w = self._batch_step_call(x[iw], K, pw, noise[1], feas=fw, **kw)
            priors.index_copy_(0, tc, pc)
            priors.index_copy_(0, tw, pw)
            bad = bad_c or bad_w
            # every host field a sub-call returned, scattered to its states' rows (index and elite_index renumbered
            # from the sub-call's batch to the whole one's)
            res = BatchStepResult(**{f: np.empty((M,) + v.shape[1:], dtype=v.dtype) for f, v in vars(rc_).items()
                                     if isinstance(v, np.ndarray)})
            if return_samples:
                res.u_norm = torch.empty((M * n, H, d), dtype=torch.float32, device=self.device)
            for idx, tidx, sub in ((ic, tc, rc_), (iw, tw, rw_)):
                first = (idx - np.arange(len(idx))) * n
                for f, v in vars(sub).items():
                    if isinstance(v, np.ndarray):
                        renumber = f in ("index", "elite_index")
                        getattr(res, f)[idx] = v + first.reshape((-1,) + (1,) * (v.ndim - 1)) if renumber else v
                if return_samples:
                    res.u_norm.view(M, n, H, d).index_copy_(0, tidx, sub.u_norm.view(len(idx), n, H, d))
        if K is not None:
            self._batch_priors = None if bad else priors
        if bad and not allow_nonfinite:
            N.check(N.MPCD_ENONFINITE, "mpcd_mpc_step_batch")
        return res

    def batch_priors(self):
        """The normalised priors the next mpc_step_batch(warm_start=K) starts from (device), as stored: [M, H, d], or
        [M, n, H, d] after a call with elites; or None."""
        return getattr(self, "_batch_priors", None)

    def set_batch_priors(self, priors):
        """Replace mpc_step_batch's prior set: normalised plans [M, H, d], or one per candidate [M, n, H, d] (copied to
        the device), or None."""
        if priors is not None:
            H, d = self.spec.horizon, self.spec.state_dim
            priors = torch.as_tensor(priors, dtype=torch.float32)
            if priors.dim() not in (3, 4) or tuple(priors.shape[-2:]) != (H, d) or 0 in priors.shape:
                raise ValueError(f"priors must be [M, {H}, {d}] or [M, n, {H}, {d}], got {tuple(priors.shape)}")
            priors = priors.to(self.device).contiguous().clone()
        self._batch_priors = priors

    def _batch_step_call(self, x, t_start, priors, noise, system, n, w, sample_fn, n_wo_noise, ddim_steps, clamp_x0,
                         seed, select, decimals, clip_rule, grouped, return_samples, elites=None, feas=None):
        """One mpcd_mpc_step_batch call on the states x [M, n_x] (checked by mpc_step_batch): (BatchStepResult, whether
        the call returned MPCD_ENONFINITE). priors: device [M, H, d] read when t_start > 0 and refreshed, or None.
        elites=k: mpcd_mpc_step_batch_elite, priors [M, n, H, d]. feas: a Feasibility for these states, with or without
        elites - mpcd_mpc_step_batch_box or mpcd_mpc_step_batch_constr, as it says."""
        x = np.ascontiguousarray(x)
        M = x.shape[0]
        H, d, B, dev = self.spec.horizon, self.spec.state_dim, M * n, self.device
        sampler = self._sampler_id(sample_fn)
        if noise is not None:
            noise = self._noise(noise, B, (sample_fn, n_wo_noise, ddim_steps, t_start or None))
        a = self._plant_block(N.BatchStepArgs(), self._system_desc(system))
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev) if return_samples else None
        a.sample = self._args(sampler, B, _STEP_CONTEXT, w, n_wo_noise, ddim_steps, clamp_x0, seed, 0, noise,
                              self._flag, None)
        a.sample.x_out = None  # ignored by the call: it samples into its workspace
        a.n_states, a.group = M, n
        a.group_contexts = 1 if bool(grouped) and self.grouped_pays(M, n, sample_fn) else 0
        a.clip_rule = _CLIP_RULES[clip_rule]
        a.select_first = 1 if select == "first" else 0
        a.decimals = -1 if decimals is None else int(decimals)
        a.warm_t_start = int(t_start)
        rec = np.empty(M, dtype=_STATE_RESULT)
        u = np.empty((M, d), dtype=np.float64)
        plan = np.empty((M, H, d), dtype=np.float32)
        a.x_host = x.ctypes.data
        a.result_host, a.u_host, a.plan_host = rec.ctypes.data, u.ctypes.data, plan.ctypes.data
        a.u_norm = u_norm.data_ptr() if u_norm is not None else None
        e = None
        if elites is None:
            a.priors = priors.data_ptr() if priors is not None else None
        else:
            e = N.BatchEliteArgs()
            e.k = elites
            e.priors = priors.data_ptr() if priors is not None else None
            best = np.empty((M, elites), dtype=_BEST)
            e.elites_host = best.ctypes.data
        if feas is not None:
            name, bx, viol, nfeas, eviol = feas.batch_block(M, elites)
            rc = getattr(self._lib, name)(self._ctx, ctypes.byref(a), None if e is None else ctypes.byref(e),
                                          ctypes.byref(bx), self._stream())
        elif e is None:
            rc = self._lib.mpcd_mpc_step_batch(self._ctx, ctypes.byref(a), self._stream())
        else:
            rc = self._lib.mpcd_mpc_step_batch_elite(self._ctx, ctypes.byref(a), ctypes.byref(e), self._stream())
        if rc != N.MPCD_ENONFINITE:
            N.check(rc, "mpcd_mpc_step_batch")
        res = BatchStepResult(u=u, plan=plan, cost=rec["cost"].copy(), index=rec["index"].copy(),
                              flags=rec["flags"].copy(), u_norm=u_norm)
        if elites is not None:
            res.elite_index, res.elite_cost = best["index"].copy(), best["cost"].copy()
        if feas is not None:
            res.violation, res.n_feasible, res.elite_violation = viol, nfeas, eviol
        return res, rc == N.MPCD_ENONFINITE

    def mpc_step(self, x0, system: System, n_samples, w=0.01, sample_fn="ddpm_cfg", n_wo_noise=0, ddim_steps=None,
                 clamp_x0=False, seed=0, noise=None, group=None, comm=None, native=None, clip_rule="chain",
                 warm_start=None, prior=None, elites=None, state_box=None, viol_tol=0.0, constraints=None, u_prev=None):
        """One control step: sample n_samples candidates on this rank (weak scaling: every rank adds
        n_samples), roll out + cost them, all-gather costs, pick the global argmin, broadcast it.
        comm: a distributed.NativeComm (the exchange inside libmpcd.so over RCCL) or None
        (torch.distributed collectives on `group`).
        native: run the whole step as one mpcd_mpc_step call (default whenever the library can do the
        exchange itself: a NativeComm, or a single rank); False = the step composed from the separate
        entry points (sample, clip flag, rollout, select), kept as the reference composition.
        clip_rule: which tensor LimitsNormalizer's global clip test runs over. "chain" (default) = the
        reference scripts, which call run_CFG(return_chain=True) and unnormalise the whole chain
        (Cart_Diffusion_inference.py:450-463, Diffusion_MPC_Inference.py:232-247), so x_T ~ N(0, 1) is in
        the test; "final" = the final samples only (proven 0 for DDPM when the last posterior mean cannot
        leave [-1, 1], then no reduction is run).
        warm_start=K (native step, CFG-DDPM, 1 <= K <= N; mpcd_mpc_step_warm): receding-horizon warm start. The
        planner keeps the winner's normalised plan, moved one horizon point ahead, on the device as the next call's
        prior: the first warm-enabled call (no prior yet) runs the full chain and fills it, later calls denoise only
        K steps from the prior noised to level K (noise then has K + n_wo_noise + 1 slices) and refresh it.
        reset_warm_start() drops the prior (a new episode); prior= (normalised [H, d]) overrides it for this call.
        Under clip_rule="chain" a warm step's test sees the noised prior instead of x_T, so the clip is no longer
        practically certain. What K costs in control quality depends on the model: measure it.
        elites=k (with warm_start=K, the native single-rank step; 1 <= k <= min(n_samples, 64); mpcd_mpc_step_elite):
        the planner keeps one prior per candidate, [n_samples, H, d]: after the selection the k best plans are ranked on
        the device and candidate j's next prior is elite j % k's plan moved one horizon point ahead, so a small K keeps
        k modes instead of one. The result carries elite_index / elite_cost (host arrays, best first; entry 0 is the
        winner) and warm_prior() returns row 0, the best plan shifted. A stored prior of one row (from a call without
        elites) seeds every candidate; prior= may be [H, d] or [n_samples, H, d]. elites=1 computes what warm_start
        alone computes. ValueError: elites without warm_start, with native=False or on several ranks, or stored priors
        whose row count is neither 1 nor n_samples (call reset_warm_start() after changing n_samples).
        state_box=(lo, hi) (None entries = unbounded), viol_tol >= 0: feasibility-first selection on the
        composed step, single rank (native then defaults to False): mpcd_rollout_cost_box gives every candidate's cost
        and box violation, and the winner is entry 0 of mpcd_topk_feasible - the cheapest candidate whose predicted
        states stay in the box, or, when none does, the least violating one. The result carries violation and
        n_feasible. ValueError with native=True, warm_start / prior / elites, a comm or several ranks: those are
        mpc_step_constr's, the one-call step with a set (a plain box is Constraints(state_box=...)).
        constraints=Constraints(...), u_prev [n_u] or None: the same composed step with mpcd_rollout_cost_constr as the
        producer of V (the box goes into the set: state_box= together with constraints= raises ValueError); u_prev is the
        previous applied action, the predecessor of u_0 in the rate test. Same result fields, same refusals."""
        if clip_rule not in _CLIP_RULES:
            raise ValueError(_BAD_CLIP_RULE)
        if comm is not None:
            rank, size = comm.rank, comm.size
        else:
            rank, size = D.world(group)
        feas = None
        if state_box is not None or constraints is not None or u_prev is not None:  # (the plain step pays one test)
            feas = feasibility(system, state_box, constraints, viol_tol, u_prev, refuse=(
                (native, _NO_NATIVE_STEP),
                (warm_start is not None or prior is not None or elites is not None, _NO_WARM_STEP),
                (comm is not None or size > 1, _SINGLE_RANK_STEP)))
            native = False
        if native is None:
            native = comm is not None or size == 1
        if elites is not None:
            if warm_start is None:
                raise ValueError(_ELITES_NEED_WARM)
            if not native:
                raise ValueError("elites needs the native step (native=True)")
            if comm is not None or size > 1:
                raise ValueError("elites is single-rank: the elite rows live on other ranks (no comm / process group)")
        if native:
            if size > 1 and comm is None:
                raise ValueError("native mpc_step on several ranks needs a NativeComm")
            return self._mpc_step_native(x0, system, n_samples, w, sample_fn, n_wo_noise, ddim_steps, clamp_x0, seed,
                                         noise, comm, clip_rule, warm_start, prior, elites)
        if warm_start is not None or prior is not None:
            raise ValueError("warm_start / prior need the native step (native=True)")
        offset = rank * n_samples
        ctx = torch.from_numpy(self.normalize_condition(x0)[None]) if self.spec.context_dim > 0 else None
        absmax = torch.empty(n_samples, dtype=torch.float32, device=self.device) if clip_rule == "chain" else None
        u_norm = self.sample_trajectories(ctx, n_samples, self.spec.horizon, w, sample_fn, n_wo_noise, ddim_steps,
                                          clamp_x0, seed, offset, noise, absmax_out=absmax)
        # LimitsNormalizer's clip flag is global over the whole batch: this rank's own code, the max over
        # ranks (mpcd_clip_flag codes: 1 = clip, 2 = NaN seen), or provably zero (final-samples rule,
        # DDPM whose last posterior mean stays in range) -> no exchange
        sampler = self._sampler_id(sample_fn)
        if clip_rule == "final" and sampler == N.MPCD_DDPM_CFG and self.ddpm_final_in_range:
            flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        else:
            flag = self.clip_flag(absmax if absmax is not None else u_norm)
            if size > 1:
                flag = comm.any_flag(flag) if comm else D.any_flag(flag, group)
        if feas is not None:
            cost_local, viol = self._rollout_feasible(system, x0, u_norm, None, flag, feas)
            raw, vk, nf = self._topk_feasible_raw(cost_local, viol, 1, 1, feas.tol)
            idx, best = int(raw[0, 0, 1]), float(raw[0, 0, 0:1].view(torch.float64))
            u_host = self.unnormalize_states(u_norm[idx][None], flag)[0].cpu().numpy()
            return MPCResult(u0=u_host[0].copy(), u_best=u_host, best_cost=best, best_index=idx, costs=cost_local,
                             u_norm=u_norm, violation=float(vk[0, 0]), n_feasible=int(nf[0]))
        cost_local = self.rollout_cost(system, x0, u_norm, flag)
        if comm is not None:
            idx, best, row, costs = comm.select(cost_local, u_norm)
        else:
            idx, best, row, costs = D.select(cost_local, u_norm, self.argmin, group)
        u_best = self.unnormalize_states(row[None], flag)[0]
        u_host = u_best.cpu().numpy()
        return MPCResult(u0=u_host[0].copy(), u_best=u_host, best_cost=best, best_index=idx, costs=costs,
                         u_norm=u_norm)

    def mpc_step_constr(self, x0, system: System, n_samples, constraints, viol_tol=0.0, u_prev=None, w=0.01,
                        sample_fn="ddpm_cfg", n_wo_noise=0, ddim_steps=None, clamp_x0=False, seed=0, noise=None, comm=None,
                        clip_rule="chain", warm_start=None, prior=None, elites=None):
        """mpc_step's native step with a constraint set and the feasibility-first selection (mpcd_mpc_step_constr;
        DESIGN §4 "Constraint set in the one-call step"): one library call, on one rank or over a NativeComm's ranks,
        cold, warm-started (warm_start=K, prior=) or with an elite set (elites=k, single rank), exactly as in mpc_step.
        constraints: a Constraints (a plain box is Constraints(state_box=...)); viol_tol >= 0; u_prev [n_u] or None: the
        action applied last, the predecessor of u_0 in the rate test (a NaN entry: none). The winner is the cheapest
        candidate of all ranks whose violation V is <= viol_tol or, when there is none, the least violating one (flags
        then carries MPCD_STEP_INFEASIBLE). The kept prior (reset_warm_start(), warm_prior()) is mpc_step's: a loop may
        alternate the two methods. Returns an MPCResult with violation, n_feasible (over all ranks), flags and costs
        (all ranks' gathered costs); with elites also elite_index, elite_cost and elite_violation.
        ValueError: constraints that is no Constraints, a bad viol_tol, a u_prev that is not [n_u], elites without
        warm_start or with a comm, several torch.distributed ranks without a NativeComm."""
        if clip_rule not in _CLIP_RULES:
            raise ValueError(_BAD_CLIP_RULE)
        feas = feasibility(system, None, constraints, viol_tol, u_prev, kind="constraints", u_prev_shape=(system.n_u,))
        if elites is not None:
            if warm_start is None:
                raise ValueError(_ELITES_NEED_WARM)
            if comm is not None:
                raise ValueError("elites is single-rank: the elite rows live on other ranks (no comm)")
        if comm is None and D.world(None)[1] > 1:
            raise ValueError("mpc_step_constr on several ranks needs a NativeComm")
        return self._mpc_step_native(x0, system, n_samples, w, sample_fn, n_wo_noise, ddim_steps, clamp_x0, seed, noise,
                                     comm, clip_rule, warm_start, prior, elites, feas)

    def reset_warm_start(self):
        """Drop the prior plan mpc_step(warm_start=K) keeps and the prior set mpc_step_batch(warm_start=K) keeps: the
        next warm-enabled call of either starts cold."""
        self._prior = self._prior_spare = None
        self._batch_priors = None

    def warm_prior(self):
        """The normalised prior plan [H, d] the next mpc_step(warm_start=K) starts from (device), or None."""
        p = getattr(self, "_prior", None)
        return None if p is None else p[0]

    def _step_warm(self, sampler, B, warm_start, prior, elites):
        """The warm start of a native single-state step (mpc_step, mpc_step_constr): (warm, prior, nxt, elites) - the
        WarmStart block (None without warm_start / prior: the cold call), the prior it reads, the buffer the call
        writes the next priors into and the checked elite count."""
        if warm_start is None and prior is None:
            return None, None, None, elites
        H, d = self.spec.horizon, self.spec.state_dim
        K = int(warm_start) if warm_start is not None else 0
        if K < 1 or K > self.n_steps or sampler != N.MPCD_DDPM_CFG:
            raise ValueError(f"warm_start={warm_start} needs 1 <= K <= {self.n_steps} and the CFG-DDPM sampler")
        if elites is not None:
            elites = self._check_elites(elites, B)
        if prior is None:
            prior = getattr(self, "_prior", None)
            if elites is not None and prior is not None and prior.shape[0] not in (1, B):
                raise ValueError(f"the stored priors have {prior.shape[0]} rows, neither 1 nor n_samples={B}: call "
                                 "reset_warm_start() after changing n_samples")
        # no prior yet: a cold step (t_start 0) that fills it
        warm, prior = self._warm(prior, K if prior is not None else 0, B)
        if elites is None and prior is not None and prior.shape[0] != 1:
            raise ValueError(f"prior must be one plan [{H}, {d}], got {tuple(prior.shape)}")
        rows = 1 if elites is None else B  # the next priors: the winner's plan, or one per candidate
        nxt = getattr(self, "_prior_spare", None)
        if nxt is None or nxt.shape[0] != rows or (prior is not None and nxt.data_ptr() == prior.data_ptr()):
            nxt = torch.empty((rows, H, d), dtype=torch.float32, device=self.device)
        return warm, prior, nxt, elites

    def _step_args(self, desc, sampler, B, w, n_wo_noise, ddim_steps, clamp_x0, seed, offset, noise, u_norm, clip_rule):
        """The StepArgs block of a native single-state step, all but x0 and the cost pointers."""
        a = self._plant_block(N.StepArgs(), desc)
        a.sample = self._args(sampler, B, _STEP_CONTEXT, w, n_wo_noise, ddim_steps, clamp_x0, seed, offset, noise, u_norm,
                              None)
        a.clip_rule = _CLIP_RULES[clip_rule]
        if clip_rule == "final" and sampler == N.MPCD_DDPM_CFG and self.ddpm_final_in_range:
            a.clip_rule = N.MPCD_CLIP_NONE
        return a

    def _swap_prior(self, nxt):
        """After a step that wrote the next priors into nxt: they become the next call's prior, and this call's prior
        buffer the next call's output."""
        if nxt is not None:
            self._prior, self._prior_spare = nxt, getattr(self, "_prior", None)

    def _mpc_step_native(self, x0, system, n_samples, w, sample_fn, n_wo_noise, ddim_steps, clamp_x0, seed, noise,
                         comm, clip_rule="chain", warm_start=None, prior=None, elites=None, feas=None):
        """mpc_step and mpc_step_constr (feas: its Feasibility, u_prev a host [n_u] row) as one libmpcd call
        (mpcd_mpc_step, _warm, _elite or _constr): the context row by value in the sampler launch, the kernels, the
        result block {best, u_best} written to pinned host memory by the selecting workgroup (one rank) or one D2H copy +
        stream synchronisation (with a communicator)."""
        size, rank = (comm.size, comm.rank) if comm is not None else (1, 0)
        B, H, d, dev = int(n_samples), self.spec.horizon, self.spec.state_dim, self.device
        _check_inputs(system, d)
        sampler = self._sampler_id(sample_fn)
        warm, prior, nxt, elites = self._step_warm(sampler, B, warm_start, prior, elites)
        if noise is not None:
            noise = self._noise(noise, B, (sample_fn, n_wo_noise, ddim_steps, warm.t_start or None if warm else None))
        u_norm = torch.empty((B, H, d), dtype=torch.float32, device=dev)
        cost = torch.empty(B, dtype=torch.float64, device=dev)
        costs = torch.empty(size * B, dtype=torch.float64, device=dev) if size > 1 else cost
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        desc = self._system_desc(system)
        # the argument block of a control loop's repeated call is built once and patched per step (x0, seed, noise, the
        # output pointers): the host path between two sampler launches is part of every control step's latency. The key
        # is everything else the block holds: rank * B is its global_offset, clip_rule with the sampler its clip code
        key = (id(desc), B, sampler, float(w), int(n_wo_noise), ddim_steps, bool(clamp_x0), clip_rule, size, rank,
               noise is None)
        cache = getattr(self, "_step_args_cache", None)
        if cache is None or cache[0] != key:
            a = self._step_args(desc, sampler, B, w, n_wo_noise, ddim_steps, clamp_x0, seed, rank * B, noise, u_norm,
                                clip_rule)
            # (+ the DDIM time list a.sample points into, kept alive with the block)
            cache = self._step_args_cache = (key, a, ctypes.byref(a), desc, N.Best(), ctypes.c_int32(),
                                             getattr(self, "_times", None))
        _, a, a_ref, _, best, fl, _ = cache
        sa = a.sample
        sa.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        sa.x_out = u_norm.data_ptr()
        sa.noise = noise.data_ptr() if noise is not None else None
        a.x0 = x0.__array_interface__["data"][0]
        a.cost_local = cost.data_ptr()
        a.costs_all = costs.data_ptr()
        u_best = np.empty((H, d), dtype=np.float32)
        ub, st = u_best.__array_interface__["data"][0], self._stream()
        el = None if elites is None else np.empty(elites, dtype=_BEST)
        more = {}
        # MPCD_ENONFINITE (no candidate with a finite cost: NaN / Inf samples) raises MpcdError here
        if feas is not None:  # the set, its outputs and the warm / elite outputs travel in one block, built per call
            viol = torch.empty(B, dtype=torch.float64, device=dev)
            viols = torch.empty(size * B, dtype=torch.float64, device=dev) if size > 1 else viol
            e = N.StepConstrArgs()
            e.con, e.tol = ctypes.pointer(feas.native), feas.tol
            e.u_prev_host = feas.u_prev.ctypes.data if feas.u_prev is not None else None
            e.viol_local, e.viols_all = viol.data_ptr(), viols.data_ptr()
            e.k = elites or 0
            e.next_priors_out = nxt.data_ptr() if nxt is not None else None
            ev = None
            if el is not None:
                ev = np.empty(elites, dtype=np.float64)
                e.elites_host, e.elite_viol_host = el.ctypes.data, ev.ctypes.data
            v_host, nf_host = ctypes.c_double(), ctypes.c_int64()
            e.viol_host, e.n_feasible_host = ctypes.pointer(v_host), ctypes.pointer(nf_host)
            N.check(self._lib.mpcd_mpc_step_constr(self._ctx, a_ref, ctypes.byref(warm) if warm is not None else None,
                                                   ctypes.byref(e), ctypes.byref(best), ub, st), "mpcd_mpc_step_constr")
            more = dict(violation=v_host.value, n_feasible=nf_host.value, elite_violation=ev)
        elif warm is None:
            N.check(self._lib.mpcd_mpc_step(self._ctx, a_ref, ctypes.byref(best), ub, st), "mpcd_mpc_step")
        elif el is not None:
            N.check(self._lib.mpcd_mpc_step_elite(self._ctx, a_ref, ctypes.byref(warm), elites, _p(nxt), el.ctypes.data,
                                                  ctypes.byref(best), ub, st), "mpcd_mpc_step_elite")
        else:
            N.check(self._lib.mpcd_mpc_step_warm(self._ctx, a_ref, ctypes.byref(warm), _p(nxt), ctypes.byref(best), ub, st),
                    "mpcd_mpc_step_warm")
        self._swap_prior(nxt)
        N.check(self._lib.mpcd_last_step_flags(self._ctx, ctypes.byref(fl)), "mpcd_last_step_flags")
        return MPCResult(u0=u_best[0].copy(), u_best=u_best, best_cost=best.cost, best_index=best.index, costs=costs,
                         u_norm=u_norm, flags=fl.value, elite_index=None if el is None else el["index"].copy(),
                         elite_cost=None if el is None else el["cost"].copy(), **more)
