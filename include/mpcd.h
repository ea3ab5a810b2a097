/*
 * mpcd.h — C ABI of libmpcd.so, the MI355X (gfx950) diffusion-MPC hot path.
 *
 * The reference (XuehuaOvO/MPC_via_Diffusion_Model) is pure Python/PyTorch; its seam for this
 * path is a Python call, not an FFI. Each entry point below replaces one reference interface
 * (cited file:line, paths relative to the reference root); the Python package
 * mpc_via_diffusion_model_amd binds them with ctypes.
 *
 * Conventions
 *  - Every function returns 0 (MPCD_OK) or a negative mpcd_status; nothing throws across the ABI.
 *    mpcd_last_error() gives a thread-local message for the last failure on this thread.
 *  - "dev" pointers are device (HBM) pointers owned by the caller; "host" pointers are read
 *    during the call only. Weights, schedule, plan and workspace belong to the context.
 *  - Work is enqueued on the caller's HIP stream (void* hip_stream; NULL = legacy default stream)
 *    and is asynchronous unless stated otherwise. One context per device; not thread-safe.
 *  - A context owns workspace (plan, projections, U-Net activations, reduction counters) that
 *    consecutive calls reuse: issue a context's calls on ONE stream, or order the streams yourself
 *    (hipStreamWaitEvent) before switching. The cached step plan / time projections are the exception:
 *    a call on another stream waits for them by itself.
 *  - All trajectory tensors are fp32 row-major [B][H][d] (candidate, horizon, action dim), the
 *    layout of the reference's x in cart_pole_sample_loop (diffusion_model_base.py:188-189).
 */
#ifndef MPCD_H
#define MPCD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpcd_ctx mpcd_ctx;

enum mpcd_status {
    MPCD_OK = 0,
    MPCD_EINVAL = -1,   /* bad argument / shape */
    MPCD_EHIP = -2,     /* HIP runtime error */
    MPCD_ESTATE = -3,   /* missing net / schedule, or call out of order */
    MPCD_ENOMEM = -4,
    MPCD_EUNSUP = -5,   /* configuration the kernels do not implement */
    MPCD_ENONFINITE = -6, /* mpcd_mpc_step: no candidate has a finite cost (NaN / Inf samples or rollout) -
                             the result block is still written; see mpcd_last_step_flags */
};

enum mpcd_net_kind {
    MPCD_NET_MLP = 1,   /* build-defined CFG MLP noise-net: PointUnet stack on [B, H*d] (temporal_unet.py:451-550) */
    MPCD_NET_UNET = 2,  /* ConditionedTemporalUnet (temporal_unet.py:189-358) or TemporalUnet (:28-187) */
};

/* GEMM numerics of the noise-net.
 * MPCD_F32:   exact fp32 MFMA (v_mfma_f32_16x16x4_f32: one rounding per product, an fmaf chain).
 * MPCD_F16:   fp16 GEMM operands with fp32 accumulation on v_mfma_f32_16x16x32_f16 (SURVEY cfg 5,
 *             "fp16 hidden with MFMA GEMM"); U-Net only (an MLP net returns MPCD_EUNSUP).
 * MPCD_F32X3: fp32-accurate split-bf16 MFMA (MLP and U-Net): each fp32 operand = three bf16 terms, the six
 *             partial products >= 2^-16 of the leading one accumulated in fp32 (error at the level of
 *             the fp32 MFMA's). MLP: needs one context row per workgroup, i.e. a context shared by all
 *             candidates, none, or one row per group of consecutive candidates (mpcd_sample_grouped); a
 *             per-candidate context (mpcd_sample with context_shared = 0) runs the MPCD_F32 kernel.
 * MPCD_F16X2: two-term fp16 MFMA (MLP: csrc/mlp_h2.hip; U-Net: the fused P = 2 program) - NOT fp32 arithmetic:
 *             each operand = hi + lo (two fp16, the weights scaled per layer by an exact power of two, the
 *             activations unscaled), three products per 32-k chunk accumulated in fp32. 22 significant bits per
 *             operand (fp32: 24) and the fp16 range: an activation above 65504 becomes a NaN sample (mpcd_mpc_step
 *             then re-runs the step in MPCD_F32X3, see mpcd_force_f32x3), activations below 2^-14 keep an
 *             absolute, not relative, precision of 2^-25. Used for the CFG-DDPM sampler and the eps forward (MLP at
 *             H*d = 32 / 64 with a shared context); every other case (unclamped DDIM, whose unbounded x leaves
 *             the fp16 range; per-candidate and grouped contexts; H*d = 128) runs the MPCD_F32X3 kernels of the same net. */
enum mpcd_dtype { MPCD_F32 = 0, MPCD_F16 = 1, MPCD_F32X3 = 2, MPCD_F16X2 = 3 };

typedef struct {
    int32_t kind;          /* mpcd_net_kind */
    int32_t state_dim;     /* d: channels of the denoised trajectory (actions per horizon point) */
    int32_t horizon;       /* H (MLP: input width H*d; UNet: H % 4 == 0) */
    int32_t context_dim;   /* C: conditioning width (0 = TemporalUnet with conditioning None) */
    int32_t base_dim;      /* unet_input_dim / dim, 32 */
    int32_t n_mults;       /* len(dim_mults), 3 for UNET_DIM_MULTS[0] = (1, 2, 4) */
    int32_t mults[4];
    int32_t time_emb_dim;  /* 32 */
    int32_t cfg_masked;    /* 1: 4-arg net with the CFG context mask (ConditionedTemporalUnet :296-300);
                              0: 3-arg TemporalUnet (context concatenated unmasked when C > 0) */
    int32_t dtype;         /* mpcd_dtype of the hidden activations/GEMM operands */
} mpcd_net_desc;

/* Parameter blob = every parameter of the torch module, flattened row-major, concatenated in the
 * order mpcd_net_param_info() enumerates (= the module's state_dict() order, which is the
 * reference's for the U-Nets, e.g. "time_mlp.encoder.1.weight", "downs.0.0.blocks.0.block.0.weight").
 * Replaces GaussianDiffusionModel(model=...) + load_state_dict (Diffusion_MPC_Inference.py:211-222). */
int mpcd_net_param_count(const mpcd_net_desc *desc, int32_t *n_tensors, int64_t *n_floats);
int mpcd_net_param_info(const mpcd_net_desc *desc, int32_t i, char *name, size_t name_cap,
                        int32_t *ndim, int64_t shape[4]);

int mpcd_create(int device, mpcd_ctx **out);
void mpcd_destroy(mpcd_ctx *ctx);
const char *mpcd_last_error(void);

/* Upload and repack weights into the kernels' layouts (blocking). */
int mpcd_load_net(mpcd_ctx *ctx, const mpcd_net_desc *desc, const float *blob_host, size_t n_floats);

/* The 12 diffusion buffers, fp32, each [n_steps], in GaussianDiffusionModel's registration order
 * (diffusion_model_base.py:87-109): betas, alphas_cumprod, alphas_cumprod_prev, sqrt_alphas_cumprod,
 * sqrt_one_minus_alphas_cumprod, log_one_minus_alphas_cumprod, sqrt_recip_alphas_cumprod,
 * sqrt_recipm1_alphas_cumprod, posterior_variance, posterior_log_variance_clipped,
 * posterior_mean_coef1, posterior_mean_coef2.
 * posterior_std_host: optional [n_steps] = sqrt(exp(posterior_log_variance_clipped)) as the caller's
 * fp32 math computes it (sample_functions.py:35-37); NULL = computed here with expf/sqrtf. */
int mpcd_set_schedule(mpcd_ctx *ctx, const float *tables_host, int32_t n_steps, const float *posterior_std_host);

enum mpcd_sampler {
    MPCD_DDPM_CFG = 0,  /* run_CFG + ddpm_cart_pole_sample_fn (diffusion_model_base.py:394-418, sample_functions.py:17-44) */
    MPCD_DDIM_CFG = 1,  /* build-defined CFG-DDIM */
    MPCD_DDIM = 2,      /* ddim_sample with a 3-arg net (diffusion_model_base.py:239-314), eta = 0 */
};

typedef struct {
    const float *context;      /* dev [B][C] normalised context, or [1][C] if context_shared; NULL if C == 0 */
    int32_t context_shared;    /* 1: one context row for every candidate (one x0 per control step) */
    int32_t sampler;           /* mpcd_sampler */
    int64_t batch;             /* B candidates handled by this call (this rank's shard) */
    double w;                  /* CFG weight (context_weight of run_CFG) */
    int32_t n_wo_noise;        /* n_diffusion_steps_without_noise (DDPM) */
    int32_t ddim_steps;        /* DDIM sampling_timesteps; 0 = reference n_steps // 5 (:252) */
    int32_t clamp_x0;          /* DDIM only; DDPM always clamps (clip_denoised, :172-173) */
    int32_t n_ddim_times;      /* length of ddim_times, 0 = derive the grid here */
    const int32_t *ddim_times; /* host, optional: the reference's time list [T-1, ..., 0, -1] (:255-258) */
    uint64_t seed;             /* Philox4x32-10 key (throughput mode) */
    int64_t global_offset;     /* global index of candidate 0 (Philox counter; sharding-invariant) */
    const float *noise;        /* dev [S+1][B][H][d] injected noise (parity mode) or NULL -> Philox;
                                  slice 0 = x_T, slice k = the draw of denoise step k */
    float *x_out;              /* dev [B][H][d] final normalised sample */
    float *chain_out;          /* dev [S+1][B][H][d] or NULL (run_CFG return_chain, :403-415) */
    float *chain_absmax;       /* dev [B] or NULL: per candidate, max |x| over every chain slice x_T .. x_0
                                  (NaN if any element is NaN) - what LimitsNormalizer's global clip test
                                  sees when the caller unnormalises the whole chain (see mpcd_clip_rule) */
} mpcd_sample_args;

/* The sampler's in-kernel noise stream (Philox4x32-10 keyed by seed, global candidate index, slice,
 * element quad) for candidates [global_offset, global_offset + n_cand): out dev [n_slices][n_cand][flat]
 * fp32, slice 0 = x_T, slice k = the draw of denoise step k (what `noise` would have to hold to replay
 * a Philox run in injected-noise mode). flat = H*d, a multiple of 4.
 *
 * The stream, for replaying it elsewhere (tests/_philox_ref.py is a numpy implementation, held to Random123's known
 * answers; tests/test_gpu_philox.py holds every kernel to it): elements 4q .. 4q + 3 of candidate c (global index:
 * global_offset + its index in the call) in slice k are made from the four 32-bit words r0 .. r3 of
 *   Philox4x32-10(counter = (q, c & 0xffffffff, c >> 32, k), key = (seed & 0xffffffff, seed >> 32))
 * (counter and key words in Random123's order, ten rounds). Uniforms, in fp32: u0 = ((float)r0 + 1) * 2^-32 and
 * u2 = ((float)r2 + 1) * 2^-32 in (0, 1] (the + 1 keeps the logarithm finite), u1 = (float)r1 * 2^-32 and
 * u3 = (float)r3 * 2^-32 in [0, 1] (no + 1), each conversion rounding to nearest even. Box-Muller:
 *   z[4q + 0] = sqrt(-2 ln u0) cos(2 pi u1), z[4q + 1] = sqrt(-2 ln u0) sin(2 pi u1),
 *   z[4q + 2] = sqrt(-2 ln u2) cos(2 pi u3), z[4q + 3] = sqrt(-2 ln u2) sin(2 pi u3),
 * evaluated in fp32 with the fast logarithm, sine and cosine: within 1.8e-6 of the same transform in fp64
 * (profiles/philox_reference.txt), |z| <= sqrt(64 ln 2) = 6.66, u0 == 1 gives zeros.
 * MPCD_EINVAL (nothing written): out NULL, n_cand < 1, n_slices < 1, flat < 4 or not a multiple of 4,
 * global_offset < 0. */
int mpcd_philox_noise(uint64_t seed, int64_t global_offset, int64_t n_cand, int32_t n_slices, int32_t flat,
                      float *out, void *hip_stream);

/* Number of denoise steps S a call makes (DDPM: N + n_wo_noise; DDIM: grid pairs). */
int mpcd_sample_steps(mpcd_ctx *ctx, const mpcd_sample_args *args, int32_t *n_steps);
int mpcd_sample(mpcd_ctx *ctx, const mpcd_sample_args *args, void *hip_stream);
/* mpcd_sample with one context row per GROUP of `group` consecutive candidates: args->context is dev
 * [batch / group][C] (context_shared is ignored), batch % group == 0, group >= 1. Candidate b uses row b / group.
 * Everything else (Philox keyed by global_offset + b, noise / chain / chain_absmax layouts) is mpcd_sample's.
 * This is a closed-loop batch (M plant states x n candidates each) without M x n context rows: an MPCD_F32X3 MLP
 * runs its split-bf16 kernels with the workgroups aligned to the groups, and group m's results are bit for bit
 * those of a shared-context mpcd_sample of `group` candidates with row m and global_offset + m * group. An MPCD_F32
 * MLP indexes its per-candidate table by b / group; an MPCD_F16X2 MLP runs its MPCD_F32X3 programs; a U-Net gets the
 * rows' projections replicated per candidate. MPCD_EINVAL: group < 1, batch % group != 0, no context pointer, a
 * net with context_dim == 0. */
int mpcd_sample_grouped(mpcd_ctx *ctx, const mpcd_sample_args *args, int64_t group, void *hip_stream);

/* ---- Warm start: denoise from a noised prior plan instead of from x_T ~ N(0, 1) (CFG-DDPM only).
 * Receding-horizon use: the previous control step's winning plan, shifted by one horizon point (mpcd_shift_plans),
 * is noised to diffusion level K = t_start <= N and only the K last steps of the chain run:
 *     x = fp32(sa * x_init[row(b)]) + fp32(sb * z0[b]),   sa = sqrt_alphas_cumprod[K - 1],
 *                                                         sb = sqrt_one_minus_alphas_cumprod[K - 1]
 * which is GaussianDiffusionModel.q_sample at t = K - 1 (diffusion_model_base.py q_sample; two separately rounded
 * products, one add), then the steps t = K - 1 ... 0 and the n_wo_noise extra steps at t = 0 exactly as the cold
 * chain runs them: S = K + n_wo_noise. z0 is noise slice 0 (noise[0] when injected, else Philox slice 0 under the
 * cold call's key); slice k >= 1 is the draw of the call's k-th executed step; noise / chain_out are [S + 1][B][H][d]
 * with chain_out slice 0 = the noised x above, and chain_absmax covers exactly those slices (x_T is not in it).
 * row(b): 0 when rows == 1 (one prior for every candidate), b when rows == batch (an elite set), b / group when
 * rows == batch / group in a grouped call (one prior per plant state). Sharding invariance holds as for the cold
 * call (global_offset keys Philox; the prior rows are the shard's own).
 * t_start == 0 is the cold start: x_init is ignored and the call is bit for bit mpcd_sample / mpcd_sample_grouped.
 * The DDIM samplers with t_start > 0 return MPCD_EUNSUP: their time grids and the unclamped chain's conditioning
 * under a truncated start are not implemented. How good a warm plan is depends on the model and on K, not on this
 * code: K = N keeps every step and only replaces x_T by a fully noised prior; a small K trusts the prior. */
typedef struct {
    const float *x_init;  /* dev, normalised [rows][H][d]; ignored when t_start == 0 */
    int64_t rows;         /* 1 | batch | batch / group (grouped call) */
    int32_t t_start;      /* K: 0 = cold start; else 1 <= K <= n_steps, the chain starts at t = K - 1 */
} mpcd_warm_start;

/* mpcd_sample (group == 0) or mpcd_sample_grouped (group >= 1) with a warm start. MPCD_EINVAL: warm == NULL,
 * t_start outside [0, n_steps], t_start > 0 with x_init == NULL or rows not one of the values above, a group that
 * does not divide the batch (and mpcd_sample_grouped's other conditions). */
int mpcd_sample_warm(mpcd_ctx *ctx, const mpcd_sample_args *args, int64_t group /* 0: as mpcd_sample */,
                     const mpcd_warm_start *warm, void *hip_stream);
/* mpcd_sample_steps of such a call: t_start + n_wo_noise (t_start == 0: mpcd_sample_steps) */
int mpcd_sample_steps_warm(mpcd_ctx *ctx, const mpcd_sample_args *args, const mpcd_warm_start *warm, int32_t *n_steps);
/* The next priors from finished plans: for m < n_states, out[m][h] = u_norm[index_dev[m] - index_offset][min(h + 1,
 * H - 1)] - the candidate's normalised plan moved one horizon point ahead, its last point repeated. u_norm dev
 * [batch][H][d] (d = the net's state_dim), index_dev dev int64 [n_states] of GLOBAL candidate indices (mpcd_control_step's
 * best_index, or &best->index of a device mpcd_best); NULL = row m. A state whose index falls outside
 * [index_offset, index_offset + batch) keeps its out[m] (a shard that does not own the winner). out must not
 * overlap u_norm. One launch for any n_states. */
int mpcd_shift_plans(mpcd_ctx *ctx, const float *u_norm, int64_t batch, int32_t horizon, const int64_t *index_dev,
                     int64_t index_offset, int64_t n_states, float *out /* dev [n_states][H][d] */, void *hip_stream);

/* One noise-net forward at diffusion time t (the model(x, t, context, mask) calls of
 * p_mean_variance_CFG, diffusion_model_base.py:166-168): x dev [B][H][d]; eps_cond dev [B][H][d] =
 * net(x, t, ctx, mask = 0); eps_uncond dev [B][H][d] = net(x, t, ctx, mask = 1) for a cfg_masked net
 * (NULL for a 3-arg net, whose single output goes to eps_cond). */
int mpcd_eps(mpcd_ctx *ctx, const float *x, int32_t t, const float *context, int32_t context_shared, int64_t batch,
             float *eps_cond, float *eps_uncond, void *hip_stream);

/* --- rollout / cost / selection --- */
enum mpcd_system {
    MPCD_SYS_CARTPOLE_LIN5 = 0,  /* EulerForwardCartpole_virtual, Cart_Diffusion_inference.py:168-197 */
    MPCD_SYS_CARTPOLE_NL5 = 1,   /* nonlinear Euler, nmpc_multi_process_collect_data.py:121-137 */
    MPCD_SYS_CARTPOLE_ZOH4 = 2,  /* linear ZOH, Diffusion_MPC_Inference.py:39-84 */
    MPCD_SYS_DOUBLE_INT2D = 3,   /* build-defined */
    MPCD_SYS_PENDULUM = 4,       /* build-defined */
    MPCD_SYS_QUADROTOR12 = 5,    /* build-defined */
};
enum mpcd_cost_kind {
    MPCD_COST_CANONICAL = 0,     /* J = q(x0) + sum_k [q(x_{k+1}) + r(u_k)], terminal P (nmpc...py:158-172) */
    MPCD_COST_CALMPC = 1,        /* calMPCCost quirks (Cart_Diffusion_inference.py:247-283) */
};

/* The system a rollout call computes with. No constant of a system is compiled in: the dynamics read params, the cost
 * reads the weights and the set-point, as given on that call. Two rules say what is NOT read:
 *  - entries of Q, P and x_ref at index >= n_x and entries of R at index >= n_u are ignored, whatever they hold;
 *  - MPCD_COST_CALMPC ignores x_ref altogether (calMPCCost costs the state itself, x^T Q x), while MPCD_COST_CANONICAL
 *    costs e = x - x_ref in every stage and in the terminal term. The dynamics never read x_ref. */
typedef struct {
    int32_t system;      /* mpcd_system */
    int32_t cost_kind;   /* mpcd_cost_kind */
    int32_t n_x, n_u;    /* n_u must equal the net's state_dim */
    double params[24];   /* dynamics constants, layout per system (mpc_via_diffusion_model_amd/systems.py) */
    double Q[12], R[4], P[12], x_ref[12];   /* diagonal weights and set-point, fp64 */
} mpcd_system_desc;

/* Global clip flag of LimitsNormalizer.unnormalize (normalization.py:160-162): *flag_dev = 1 iff
 * x.max() > 1+1e-4 or x.min() < -1-1e-4 over the n values, with torch's NaN semantics (a NaN anywhere
 * makes max/min NaN and both tests false: flag 0). Also valid over mpcd_sample's chain_absmax values.
 * Sharded callers max-reduce the per-rank flags (a NaN on any rank is reported as flag value 2, which
 * a max-reduction keeps: only 1 means clip). */
int mpcd_clip_flag(mpcd_ctx *ctx, const float *x, int64_t n, int32_t *flag_dev, void *hip_stream);

/* Unnormalise (LimitsNormalizer.unnormalize, normalization.py:156-167; clip iff the GLOBAL max/min of
 * u_norm leaves [-1-1e-4, 1+1e-4]) then roll out and cost every candidate in fp64, one thread each.
 * x0_host [n_x] fp64; u_norm dev [B][H][n_u]; umin/umax host [n_u] fp32 (dataset limits);
 * clip_flag_dev: dev int32 from mpcd_clip_flag (e.g. OR-reduced over ranks), or NULL = computed here
 * from u_norm; cost_out dev [B] fp64. Replaces calMPCCost / the MPC objective evaluated per sample. */
int mpcd_rollout_cost(mpcd_ctx *ctx, const mpcd_system_desc *sys, const double *x0_host, const float *u_norm,
                      const float *umin_host, const float *umax_host, int64_t batch, int32_t horizon,
                      const int32_t *clip_flag_dev, double *cost_out, void *hip_stream);

/* Unnormalise only: out = ((x+1)/2)*(max-min)+min in fp32 over [n_rows][dim], with the global clip
 * rule (clip_flag_dev as above; NULL = computed from x). dim <= 16. */
int mpcd_unnormalize(mpcd_ctx *ctx, const float *x, int64_t n_rows, int32_t dim, const float *min_host,
                     const float *max_host, const int32_t *clip_flag_dev, float *out, void *hip_stream);

typedef struct {
    double cost;         /* +inf if every cost is NaN */
    int64_t index;       /* index_offset + position; lowest index on ties; NaN costs rank as +inf */
} mpcd_best;

/* Device argmin over cost[n] (torch.argmin(cost_all), inference_(mpd).py:335-338). best_dev is a
 * device pointer to one mpcd_best. */
int mpcd_argmin(mpcd_ctx *ctx, const double *cost, int64_t n, int64_t index_offset, mpcd_best *best_dev,
                void *hip_stream);

/* ---- Elite sets: the k best plans of each plant state, ranked on the device, and the per-candidate warm-start priors
 * seeded from them (mpcd_warm_start.rows == batch). One shared prior collapses a warm-started candidate set onto one
 * mode at a small t_start; seeding candidate j from elite j mod k keeps k modes alive. The ranked list also serves a
 * caller that wants fallback plans, or the first plan that passes a safety filter, without downloading every cost. */
#define MPCD_MAX_ELITES 64
/* Ranked top-k per group: for m < n_groups, out_dev[m][0..k) = the k best of cost[m * group, (m + 1) * group), best
 * first, in mpcd_argmin's order: NaN ranks (and is reported) as +inf, lower cost wins, then lower index. index =
 * index_offset + the entry's position in cost[] (m * group + j: mpcd_control_step's global candidate index), so with
 * n_groups == 1 entry 0 is bit for bit mpcd_argmin's winner, and entry 0 of group m mpcd_control_step's. One launch, one
 * workgroup per group; every cost is read from memory once. cost dev fp64 [n_groups * group]; out_dev dev
 * [n_groups][k]. MPCD_EINVAL: a null pointer, n_groups / group < 1, k < 1, k > group or k > MPCD_MAX_ELITES. */
int mpcd_topk(mpcd_ctx *ctx, const double *cost, int64_t n_groups, int64_t group, int32_t k, int64_t index_offset,
              mpcd_best *out_dev /* [n_groups][k], best first */, void *hip_stream);
/* The priors an elite set seeds: with batch = n_groups * group, for candidate b = m * group + j
 *     out[b][h] = u_norm[elites_dev[m][j mod k].index - index_offset][min(h + shift, H - 1)]
 * shift == 1: mpcd_shift_plans' rule (the plan moved one horizon point ahead, its last point repeated), for the next
 * control step; shift == 0: the plan as it is, for re-sampling within one control step. u_norm and out dev
 * [batch][H][d] (d = the net's state_dim), elites_dev dev [n_groups][k] as mpcd_topk writes it (only .index is read).
 * An elite whose index falls outside [index_offset, index_offset + batch) leaves its candidates' rows of out as they
 * are (mpcd_shift_plans' rule). One launch, spread over the whole of out. MPCD_EINVAL: a null pointer, n_groups / group
 * < 1, k < 1, k > group or k > MPCD_MAX_ELITES, shift not 0 or 1, horizon != the net's, out overlapping u_norm. */
int mpcd_elite_priors(mpcd_ctx *ctx, const float *u_norm, int64_t n_groups, int64_t group, int32_t horizon,
                      const mpcd_best *elites_dev, int32_t k, int64_t index_offset, int32_t shift,
                      float *out /* dev [n_groups*group][H][d] */, void *hip_stream);

/* ---- Closed loop on the device: M plant states advanced together, each with its
 * own group of `group` consecutive candidates, no host round trip inside the loop
 * (Cart_Diffusion_inference.py:405-512 runs one state at a time on the host). */

/* Per-group clip flags: flags_dev[g] = mpcd_clip_flag's code over x[g*group_elems, (g+1)*group_elems)
 * (LimitsNormalizer's rule applied to each state's own candidate batch, or to its candidates'
 * chain_absmax values: 1 = clip). */
int mpcd_clip_flags(mpcd_ctx *ctx, const float *x, int64_t n_groups, int64_t group_elems, int32_t *flags_dev,
                    void *hip_stream);

/* normalize_condition of n_states device fp64 states [n_states][dim] (normalization.py:149-154 in fp64,
 * then the net's .float()): ctx_out dev fp32 [n_states][dim]. min/max host fp32 [dim], dim <= 16. */
int mpcd_normalize_states(mpcd_ctx *ctx, const double *x_dev, int64_t n_states, int32_t dim, const float *min_host,
                          const float *max_host, float *ctx_out, void *hip_stream);

/* mpcd_rollout_cost with one start state per group: candidate b starts from x0_dev[b / group] (dev fp64
 * [batch/group][n_x]) and uses flags_dev[b / group]. batch % group == 0. */
int mpcd_rollout_cost_grouped(mpcd_ctx *ctx, const mpcd_system_desc *sys, const double *x0_dev, int64_t group,
                              const float *u_norm, const float *umin_host, const float *umax_host, int64_t batch,
                              int32_t horizon, const int32_t *flags_dev, double *cost_out, void *hip_stream);

/* One control step for n_states plant states (A15 + the plant step): for state m pick the candidate of
 * [m*group, (m+1)*group) with the lowest cost (NaN = +inf, lowest index on ties) or, select_first != 0,
 * the group's first one (the reference scripts' n_samples = 1 use); unnormalise its u[0] with
 * flags_dev[m]; round it to `decimals` places (the reference's round(u, 4); < 0 = no rounding); then
 * x_dev[m] <- f(x_dev[m], u0) in fp64 with the system's dynamics (in place). Outputs (device):
 * u_applied [n_states][n_u] fp64, best_index [n_states] int64 (global candidate index), best_cost fp64. */
int mpcd_control_step(mpcd_ctx *ctx, const mpcd_system_desc *sys, double *x_dev, int64_t n_states, int64_t group,
                      const float *u_norm, int32_t horizon, const double *cost, const float *umin_host,
                      const float *umax_host, const int32_t *flags_dev, int32_t select_first, int32_t decimals,
                      double *u_applied, int64_t *best_index, double *best_cost, void *hip_stream);

/* ---- State constraints: rollout violation and feasibility-first ranking (single rank). Every selection above ranks
 * by cost alone; these three entry points let a caller keep the plant inside a box of admissible states. They compose
 * with the calls above (mpcd_elite_priors and mpcd_shift_plans consume the ranked list unchanged). Of the one-call
 * tails the batched external step takes a box (mpcd_mpc_step_batch_box below: the same violation and the same order,
 * computed inside its one tail launch) and the single-state step takes one as a constraint set that is only a box
 * (mpcd_mpc_step_constr below, on one rank or many); mpcd_mpc_step / _warm / _elite themselves and mpcd_closed_loop do
 * not.
 *
 * State box: component i < n_x of a state is admissible in [lo[i], hi[i]]; -inf / +inf mean unbounded; entries >= n_x
 * are ignored.
 *
 * Violation of a candidate, in fp64:
 *     V = max(0, max over the visited states x and i < n_x of max(lo[i] - x[i], x[i] - hi[i]))
 * The visited states are exactly the states the dynamics step produces inside that candidate's cost evaluation:
 * MPCD_COST_CANONICAL x_1 .. x_H; MPCD_COST_CALMPC x_1 .. x_{H-2} (calMPCCost's loop applies u_0 .. u_{H-3}: the quirk
 * is kept, so the cost and the violation speak of the same trajectory). The start state is not tested: the caller
 * knows it. An excess that is NaN (either difference is: a NaN state, inf - inf) makes V = +inf. A maximum does not
 * depend on the order of its operands, so V is reproducible bit for bit where the states are.
 *
 * Feasibility-first order with tolerance tol >= 0: a candidate is feasible iff V <= tol; every feasible candidate ranks
 * before every infeasible one; feasible candidates are ordered by (cost, index), infeasible ones by (V, cost, index);
 * a NaN cost ranks and is reported as +inf, as in mpcd_topk. This is ONE strict lexicographic order on (g, cost, index)
 * with g = V <= tol ? 0 : V. */
typedef struct { double lo[12], hi[12]; } mpcd_state_box;

/* mpcd_rollout_cost_grouped plus the box: cost_out [batch] is bit for bit what mpcd_rollout_cost_grouped writes (the
 * same cost function, visited by the bounds test), viol_out [batch] each candidate's V. MPCD_EINVAL:
 * mpcd_rollout_cost_grouped's cases; box or viol_out NULL; a NaN bound; lo[i] > hi[i] for some i < n_x. */
int mpcd_rollout_cost_box(mpcd_ctx *ctx, const mpcd_system_desc *sys, const double *x0_dev, int64_t group,
                          const float *u_norm, const float *umin_host, const float *umax_host, int64_t batch,
                          int32_t horizon, const int32_t *flags_dev, const mpcd_state_box *box, double *cost_out,
                          double *viol_out, void *hip_stream);

/* mpcd_topk in the feasibility-first order: for m < n_groups, out_dev[m][0..k) = the k first of group m's candidates,
 * {cost (NaN -> +inf), index_offset + position}; viol_out_dev[m][r] (or NULL) = that entry's V as computed (NaN -> +inf;
 * not g); n_feasible_dev[m] (or NULL) = the number of candidates of the WHOLE group with V <= tol: 0 means "no
 * admissible plan; entry 0 is the least violating one". One launch, one workgroup per group; every cost and violation
 * is read from memory once. cost, viol dev fp64 [n_groups * group]. MPCD_EINVAL: mpcd_topk's cases; viol NULL; tol
 * negative or NaN. */
int mpcd_topk_feasible(mpcd_ctx *ctx, const double *cost, const double *viol, int64_t n_groups, int64_t group, int32_t k,
                       double tol, int64_t index_offset, mpcd_best *out_dev /* [n_groups][k] */,
                       double *viol_out_dev /* [n_groups][k] or NULL */, int64_t *n_feasible_dev /* [n_groups] or NULL */,
                       void *hip_stream);

/* mpcd_control_step with the selection supplied: state m applies candidate picks_dev[m * pick_stride].index -
 * index_offset of u_norm [batch][H][n_u] (pick_stride = k walks entry 0 of a ranked [n_states][k] list): its u[0]
 * unnormalised with flags_dev[m] and rounded to `decimals` places, then x_dev[m] <- f(x_dev[m], u0) in place;
 * best_index[m] = the pick's index as given, best_cost[m] = the pick's cost (mpcd_topk's reporting: NaN -> +inf). A pick
 * outside [0, batch) touches no memory through it: x_dev[m] stays, u_applied[m] = NaN, best_index[m] = -1,
 * best_cost[m] = +inf. MPCD_EINVAL: a NULL pointer, n_states / batch / horizon / pick_stride < 1, decimals > 15, a bad
 * system descriptor. */
int mpcd_control_step_picked(mpcd_ctx *ctx, const mpcd_system_desc *sys, double *x_dev, int64_t n_states,
                             const float *u_norm, int64_t batch, int32_t horizon, const mpcd_best *picks_dev,
                             int64_t pick_stride, int64_t index_offset, const float *umin_host, const float *umax_host,
                             const int32_t *flags_dev, int32_t decimals, double *u_applied, int64_t *best_index,
                             double *best_cost, void *hip_stream);

/* ---- Constraint set: linear rows and input-rate bounds beside the state box. The violation V above is the box's; a
 * constraint set generalises its producer and nothing else: the feasibility-first order, tol, n_feasible and every
 * consumer of V (mpcd_topk_feasible, mpcd_control_step_picked, mpcd_shift_plans / mpcd_elite_priors on the ranked list,
 * MPCD_STEP_INFEASIBLE) are unchanged. Of the one-call steps mpcd_mpc_step_batch_constr (many external states) and
 * mpcd_mpc_step_constr (one state: cold, warm-started, with elites, or over a communicator's ranks) take a set;
 * mpcd_closed_loop does not.
 *
 * The tests run where the box is tested: each time the dynamics step produces a state inside the candidate's cost
 * evaluation, on the pair (x_{k+1}, u_k) of the new state and the input that produced it: MPCD_COST_CANONICAL k = 0 ..
 * H-1; MPCD_COST_CALMPC k = 0 .. H-3 (the quirk above). u is the unnormalised, clipped input in fp64 (exact from fp32).
 * Excesses, all fp64, no contraction:
 *   box       as above.
 *   row r < n_rows   s = A[r][0]*x[0]; s = s + A[r][i]*x[i] for i = 1 .. n_x-1 in that order; s = s + C[r][j]*u[j] for
 *             j = 0 .. n_u-1 in that order; the excess is s - b[r]. The order is part of the contract (it makes V
 *             reproducible bit for bit). Entries at i >= n_x and j >= n_u are ignored. b[r] = +inf switches a row off.
 *   rate, input j < n_u   fabs(u_k[j] - u_{k-1}[j]) - du_max[j] for every visited k that has a predecessor; +inf =
 *             unbounded. For k = 0 the predecessor is the caller's previous applied action u_prev of that plant state, if
 *             one is given; a u_prev row with a NaN in any entry means "no previous input" (a restarted episode in a
 *             batch): that state's rate test starts at k = 1.
 * V = max(0, every excess above); an excess that is NaN (a NaN state or input, inf - inf, 0 * inf) makes V = +inf. A
 * maximum has no order, so for the systems without sin / cos V is exact. */
#define MPCD_MAX_CON_ROWS 8
typedef struct {
    mpcd_state_box box;                 /* rules unchanged; all-infinite = no box */
    int32_t n_rows;                     /* 0 .. MPCD_MAX_CON_ROWS */
    int32_t reserved;                   /* 0 */
    double A[MPCD_MAX_CON_ROWS][12];    /* row r: sum_i A[r][i] x[i] + sum_j C[r][j] u[j] <= b[r] */
    double C[MPCD_MAX_CON_ROWS][4];
    double b[MPCD_MAX_CON_ROWS];        /* +inf switches a row off */
    double du_max[4];                   /* |u_k[j] - u_{k-1}[j]| <= du_max[j]; +inf = unbounded */
} mpcd_constraints;

/* mpcd_rollout_cost_box with the set (rollout_cost_constr_kernel, csrc/rollout.hip): cost_out [batch] stays bit for
 * bit mpcd_rollout_cost_grouped's, viol_out [batch] is each candidate's V over the set. u_prev_dev: dev fp64
 * [batch / group][n_u], each plant state's previous applied action, or NULL (no state has one). With n_rows = 0 and an
 * infinite du_max the call writes mpcd_rollout_cost_box's bits. MPCD_EINVAL: mpcd_rollout_cost_box's cases (the box's
 * included); con NULL; n_rows outside [0, MPCD_MAX_CON_ROWS]; reserved != 0; a NaN or infinite coefficient in a used
 * row's A[r][i < n_x] / C[r][j < n_u]; a NaN or -inf in a used b[r]; a NaN or negative du_max[j < n_u]. */
int mpcd_rollout_cost_constr(mpcd_ctx *ctx, const mpcd_system_desc *sys, const double *x0_dev, int64_t group,
                             const float *u_norm, const float *umin_host, const float *umax_host, int64_t batch,
                             int32_t horizon, const int32_t *flags_dev, const mpcd_constraints *con,
                             const double *u_prev_dev, double *cost_out, double *viol_out, void *hip_stream);

/* ---- The whole closed loop in one call. mpcd_closed_loop enqueues, on hip_stream and without a host synchronisation,
 * what DiffusionMPC.closed_loop composes from the entry points above: one mpcd_normalize_states launch for iteration
 * 0, then per iteration the sampler and ONE launch (closed_loop_tail_kernel, csrc/rollout.hip) for everything else:
 * each state's clip code, the fp64 rollout and cost of its candidates, the selection (NaN = +inf, lowest index on
 * ties, or the group's first candidate), u0 unnormalised and rounded, the plant step, the history rows, the next
 * iteration's context row and, with a warm start, its next prior. The results are bit for bit those of the composed
 * calls (same fp64 operations in the same order per candidate).
 * MPCD_EINVAL: a NULL required pointer, iterations / group / n_states < 1, sys->n_u != the net's state_dim,
 * sys->n_x != its context_dim, clip_rule == MPCD_CLIP_NONE (or unknown), warm_t_start outside [0, n_steps].
 * MPCD_EUNSUP: an MPCD_F16X2 net - its range guard needs a look at the chain maxima on the host in every iteration
 * (the re-run with the split-bf16 programs), which is exactly the round trip this call removes; a context with a
 * communicator (the loop is single-rank); warm_t_start > 0 with a sampler other than MPCD_DDPM_CFG. */
typedef struct {
    const mpcd_system_desc *sys;    /* n_u == the net's state_dim, n_x == its context_dim */
    const float *ctx_min, *ctx_max; /* host [n_x] condition limits (mpcd_normalize_states) */
    const float *act_min, *act_max; /* host [n_u] action limits */
    mpcd_sample_args sample;        /* the sampler, w, n_wo_noise, the DDIM fields and clamp_x0; seed = iteration 0's
                                       seed (iteration it: seed + it, global_offset 0). batch, context,
                                       context_shared, global_offset, noise, x_out, chain_out and chain_absmax are
                                       ignored: batch = n_states * group */
    int64_t n_states;               /* M plant states */
    int64_t group;                  /* n candidates per state */
    int32_t iterations;             /* T */
    int32_t group_contexts;         /* 1: the sampler runs as mpcd_sample_grouped on the [M][C] rows and [M][H][d] priors;
                                       0: one row (and prior) per candidate, each state's repeated n times - an MLP
                                       then runs the exact-f32 kernel, as with mpcd_sample and a [B][C] context */
    const float *const *noise_iters; /* host [iterations] device pointers, entry it = that iteration's injected noise
                                       [S_it + 1][B][H][d] (S_0 = the cold step count; S_it = warm_t_start + n_wo_noise
                                       for it >= 1 of a warm loop); NULL = Philox */
    int32_t clip_rule;              /* MPCD_CLIP_CHAIN or MPCD_CLIP_FINAL, per state over its own candidates */
    int32_t select_first;           /* mpcd_control_step's */
    int32_t decimals;               /* mpcd_control_step's (< 0: no rounding) */
    int32_t warm_t_start;           /* 0: every iteration samples cold; K >= 1: iteration 0 cold, the later ones
                                       t_start = K from the shifted winners (mpcd_shift_plans' rule) */
    double *x_dev;                  /* dev [M][n_x] fp64 plant states, in and out */
    double *x_hist;                 /* dev [T + 1][M][n_x]; slice 0 = the initial states (written by the call) */
    double *u_hist;                 /* dev [T][M][n_u] applied actions */
    double *cost_hist;              /* dev [T][M] cost of the selected candidate */
    int64_t *index_hist;            /* dev [T][M] global index of the selected candidate in that iteration's batch */
    float *u_norm;                  /* dev [B][H][d] or NULL: the last iteration's normalised samples */
} mpcd_closed_loop_args;
/* The context owns the loop's workspace (context rows, per-state counters, partials, samples, chain maxima, priors),
 * reused and grown across calls: like every context workspace it is ordered on ONE stream. */
int mpcd_closed_loop(mpcd_ctx *ctx, const mpcd_closed_loop_args *args, void *hip_stream);

/* ---- One control step for many plant states that arrive from OUTSIDE (a vectorised simulator, a plant with model
 * mismatch or disturbances, a fleet of devices). mpcd_closed_loop owns its plant; mpcd_mpc_step takes one state per
 * call. mpcd_mpc_step_batch takes n_states fp64 states from the host and returns every state's applied action,
 * selected plan, cost, index and flags to the host in ONE call: one host-to-device copy of the states through pinned
 * staging, mpcd_normalize_states, the sampler over n_states * group candidates (grouped, or each state's row repeated
 * per candidate), ONE launch (batch_step_tail_kernel, csrc/rollout.hip) for each state's clip code, the fp64 rollout
 * and cost of its candidates, the selection (NaN = +inf, lowest index on ties, or the group's first candidate), u0
 * unnormalised and rounded, the selected plan unnormalised and the next prior, then one device-to-host copy of the
 * packed result block into pinned memory of the context and one stream synchronisation. The host outputs are complete
 * when the call returns.
 * Given states equal to a closed-loop iteration's x_dev (and that iteration's seed, noise and warm start) the call
 * computes bit for bit what that iteration of mpcd_closed_loop computes up to and including the selection and u0, and
 * the same next prior. It takes no plant step and writes no history rows and no next context row.
 * Flags per state: MPCD_STEP_CLIPPED / MPCD_STEP_NAN_SAMPLES from the state's clip code (1 / 2) and
 * MPCD_STEP_NONFINITE_WINNER when the selected cost is not finite.
 * Returns MPCD_ENONFINITE when any state carries MPCD_STEP_NONFINITE_WINNER: all outputs are still written and the
 * other states' results are valid.
 * MPCD_EINVAL: a NULL required pointer, n_states / group < 1, sys->n_u != the net's state_dim, sys->n_x != its
 * context_dim, clip_rule == MPCD_CLIP_NONE (or unknown), decimals > 15, warm_t_start outside [0, n_steps],
 * warm_t_start > 0 without priors.
 * MPCD_EUNSUP: an MPCD_F16X2 net (its range guard reads the chain maxima on the host and re-runs the sampler: a
 * second round trip inside the step); a context with a communicator (the step is single-rank); warm_t_start > 0 with
 * a sampler other than MPCD_DDPM_CFG; H * n_u too large for the tail's LDS. */
typedef struct {
    double cost;      /* the selected candidate's cost as computed (a NaN stays one) */
    int64_t index;    /* its global index in this call's batch: m * group + j */
    int32_t flags;    /* per state: MPCD_STEP_CLIPPED | MPCD_STEP_NAN_SAMPLES | MPCD_STEP_NONFINITE_WINNER
                         (| MPCD_STEP_INFEASIBLE from mpcd_mpc_step_batch_box) */
    int32_t reserved; /* 0 */
} mpcd_state_result;

typedef struct {
    const mpcd_system_desc *sys;    /* the PLANNING model: n_u == the net's state_dim, n_x == its context_dim */
    const float *ctx_min, *ctx_max; /* host [n_x] condition limits (mpcd_normalize_states) */
    const float *act_min, *act_max; /* host [n_u] action limits */
    mpcd_sample_args sample;        /* as in mpcd_closed_loop_args: the sampler, w, n_wo_noise, the DDIM fields and
                                       clamp_x0; seed and noise are THIS step's (noise: injected [S + 1][B][H][d], S =
                                       warm_t_start + n_wo_noise for a warm step, or NULL = Philox). batch, context,
                                       context_shared, global_offset, x_out, chain_out and chain_absmax are ignored:
                                       batch = n_states * group, global_offset 0 */
    int64_t n_states;               /* M plant states */
    int64_t group;                  /* n candidates per state */
    int32_t group_contexts;         /* mpcd_closed_loop_args' meaning */
    int32_t clip_rule;              /* MPCD_CLIP_CHAIN or MPCD_CLIP_FINAL, per state over its own candidates */
    int32_t select_first;           /* mpcd_control_step's */
    int32_t decimals;               /* mpcd_control_step's (< 0: no rounding) */
    int32_t warm_t_start;           /* 0: a cold step; K >= 1: sample from `priors` with t_start = K (CFG-DDPM only) */
    const double *x_host;           /* host [M][n_x] fp64 plant states, read during the call */
    float *priors;                  /* dev [M][H][d] or NULL. Read when warm_t_start > 0 (then required); when non-NULL
                                       it is overwritten, after the sampler has read it, with the NEXT priors: each
                                       state's selected plan under mpcd_shift_plans' rule */
    mpcd_state_result *result_host; /* host [M] */
    double *u_host;                 /* host [M][n_u]: the applied action (unnormalised with the state's clip flag,
                                       rounded to `decimals`) */
    float *plan_host;               /* host [M][H][d] or NULL: the selected plan, unnormalised the same way */
    float *u_norm;                  /* dev [B][H][d] or NULL: all normalised samples of this step */
} mpcd_batch_step_args;
/* The context owns the step's workspace (state and context rows, per-state counters, partials, samples, chain maxima,
 * repeated priors, the packed result block) and its pinned host staging, reused and grown across calls like the closed
 * loop's; the per-state counters reset themselves. Like every context workspace it is ordered on ONE stream. */
int mpcd_mpc_step_batch(mpcd_ctx *ctx, const mpcd_batch_step_args *args, void *hip_stream);

/* mpcd_mpc_step_batch with elite sets: the same call - one state upload, the sampler, ONE tail launch
 * (batch_step_elite_tail_kernel), one download, one synchronisation - that also ranks each state's k best candidates
 * inside the tail (no cost array, no mpcd_topk launch) and keeps one warm-start prior per CANDIDATE: one
 * mpcd_elite_priors(shift = 1) launch after the tail seeds candidate j of state m from the state's elite j mod k.
 * Everything mpcd_mpc_step_batch returns is returned, computed the same way; elites_host[m][0..k) is bit for bit
 * mpcd_topk over mpcd_rollout_cost_grouped's costs of this step's samples (NaN reported as +inf, ties to the lower
 * index, global indices m * group + j), so elites_host[m][0].index == result_host[m].index, while result_host[m].cost
 * stays the cost as computed. A state without a finite cost gets k elites of cost +inf in index order and carries
 * MPCD_STEP_NONFINITE_WINNER (the call returns MPCD_ENONFINITE as mpcd_mpc_step_batch does). With
 * args->group_contexts == 0 the priors are not repeated: they are per candidate already.
 * MPCD_EINVAL: mpcd_mpc_step_batch's cases; elite == NULL; k outside [1, min(args->group, MPCD_MAX_ELITES)];
 * reserved != 0; args->select_first != 0 (ranking needs costs); args->priors != NULL (the per-state prior buffer has
 * no meaning here); warm_t_start > 0 with elite->priors == NULL. MPCD_EUNSUP: mpcd_mpc_step_batch's cases. */
typedef struct {
    int32_t k;              /* elites per state: 1 <= k <= min(args->group, MPCD_MAX_ELITES) */
    int32_t reserved;       /* 0 */
    float *priors;          /* dev [M*group][H][d] or NULL: one prior per CANDIDATE (mpcd_warm_start.rows == batch, grouped or
                               not). Read when warm_t_start > 0 (then required); when non-NULL overwritten, after the sampler
                               has read it, with mpcd_elite_priors(shift = 1) of this step's samples and elites */
    mpcd_best *elites_host; /* host [M][k] or NULL: each state's k best, best first, mpcd_topk's order and cost reporting */
} mpcd_batch_elite_args;
/* The partial ranked lists and the larger result block belong to the same context workspace as mpcd_mpc_step_batch's;
 * the per-state counters are the same self-resetting ones. */
int mpcd_mpc_step_batch_elite(mpcd_ctx *ctx, const mpcd_batch_step_args *args, const mpcd_batch_elite_args *elite,
                              void *hip_stream);

/* mpcd_mpc_step_batch / mpcd_mpc_step_batch_elite with a state box ("State constraints" above): the same call - one
 * state upload, the sampler, ONE tail launch (batch_step_box_tail_kernel, csrc/rollout.hip), with elites the one
 * mpcd_elite_priors launch, one download, one synchronisation. Inside the tail every candidate's rollout also reports
 * its violation V of the box, and the selection and the elite ranking follow the feasibility-first order with `tol`;
 * no cost array and no violation array goes through memory.
 * The call returns everything mpcd_mpc_step_batch returns (elite == NULL) or mpcd_mpc_step_batch_elite returns (elite
 * given), computed the same way; the one difference is the order. result_host[m].cost stays the selected candidate's
 * cost as computed; elite costs are reported as mpcd_topk_feasible reports them (NaN -> +inf) and
 * elites_host[m][0].index == result_host[m].index. For the same samples, states, clip flags and box, the index, cost, V
 * and n_feasible of every state, elite_viol_host and the ranked lists are bit for bit entry 0 (entries 0..k) of
 * mpcd_rollout_cost_box followed by mpcd_topk_feasible(k, tol); u0 and the plan are what mpcd_control_step_picked
 * applies for that pick; the next priors are mpcd_shift_plans on entry 0 (elite == NULL, args->priors) or
 * mpcd_elite_priors(shift = 1) on the ranked list (elite->priors).
 * An all-infinite box with tol = 0 gives mpcd_mpc_step_batch's / _elite's results bit for bit: V = 0 then, except that
 * a NaN state gives V = +inf, and such a candidate's cost is +inf in the order already, so the ranking does not move.
 * Flags: MPCD_STEP_CLIPPED, MPCD_STEP_NAN_SAMPLES and MPCD_STEP_NONFINITE_WINNER as above (MPCD_ENONFINITE is returned
 * as above); MPCD_STEP_INFEASIBLE is set exactly when n_feasible_host[m] == 0: no candidate of the state has V <= tol
 * and the selected plan is the least violating one. It is a per-state flag, not an error return: the caller decides
 * whether to apply that plan.
 * MPCD_EINVAL: the underlying call's cases; box, box->box, viol_host or n_feasible_host NULL; a NaN bound or lo[i] >
 * hi[i] for some i < n_x (mpcd_rollout_cost_box's rules); tol negative or NaN; a non-zero reserved field;
 * args->select_first != 0 (ranking needs costs); elite_viol_host without elite. MPCD_EUNSUP: the underlying call's. */
enum { MPCD_STEP_INFEASIBLE = 16 };
typedef struct {
    const mpcd_state_box *box;   /* host; mpcd_rollout_cost_box's rules */
    double tol;                  /* mpcd_topk_feasible's tol: a candidate is feasible iff V <= tol */
    double *viol_host;           /* host [M]: the selected candidate's V as computed (NaN -> +inf) */
    int64_t *n_feasible_host;    /* host [M]: candidates of the whole group with V <= tol */
    double *elite_viol_host;     /* host [M][k] or NULL: V of each elite (with elite != NULL) */
    int32_t reserved, reserved2; /* 0 */
} mpcd_batch_box_args;
/* The partial lists, their violations and counts and the larger result block belong to the same context workspace as
 * mpcd_mpc_step_batch's (which does not grow for the two calls above); the per-state counters are the same
 * self-resetting ones, so the three calls may alternate on one context. */
int mpcd_mpc_step_batch_box(mpcd_ctx *ctx, const mpcd_batch_step_args *args,
                            const mpcd_batch_elite_args *elite /* NULL: winner only */, const mpcd_batch_box_args *box,
                            void *hip_stream);

/* mpcd_mpc_step_batch_box with a constraint set ("Constraint set" above) in place of the box: the same shape of call -
 * one state upload, the sampler, ONE tail launch (batch_step_box_tail_kernel<SYS, ConTolK>, csrc/rollout.hip), with elites the one
 * mpcd_elite_priors launch, one download, one synchronisation. u_prev_host rides the pinned staging block and the single
 * host-to-device copy of the states: [M][n_x], then [M][n_u].
 * Everything mpcd_mpc_step_batch_box promises holds with mpcd_rollout_cost_constr in place of mpcd_rollout_cost_box:
 * for the same samples, states, clip flags, set and u_prev, the index, cost, V and n_feasible of every state, the ranked
 * lists and their V are bit for bit entries 0..k of mpcd_rollout_cost_constr followed by mpcd_topk_feasible(k, tol); u0
 * and the plan are mpcd_control_step_picked's; the next priors mpcd_shift_plans' / mpcd_elite_priors(shift = 1)'s;
 * MPCD_STEP_INFEASIBLE is set exactly when n_feasible_host[m] == 0. A set that is only a box gives
 * mpcd_mpc_step_batch_box's results, an all-infinite set mpcd_mpc_step_batch's / _elite's, bit for bit.
 * MPCD_EINVAL / MPCD_EUNSUP: mpcd_mpc_step_batch_box's cases (con and con->con for box and box->box), plus
 * mpcd_rollout_cost_constr's for the set. */
typedef struct {
    const mpcd_constraints *con;  /* host */
    double tol;                   /* mpcd_topk_feasible's tol */
    const double *u_prev_host;    /* host [M][n_u] or NULL: each state's previous applied action (NaN row: none) */
    double *viol_host;            /* host [M] */
    int64_t *n_feasible_host;     /* host [M] */
    double *elite_viol_host;      /* host [M][k] or NULL (with elite != NULL) */
    int32_t reserved, reserved2;  /* 0 */
} mpcd_batch_constr_args;
/* The workspace is mpcd_mpc_step_batch's (which does not grow for this call either); the counters are the same
 * self-resetting ones, so the four calls may alternate on one context. */
int mpcd_mpc_step_batch_constr(mpcd_ctx *ctx, const mpcd_batch_step_args *args,
                               const mpcd_batch_elite_args *elite /* NULL: winner only */,
                               const mpcd_batch_constr_args *con, void *hip_stream);

/* ---- Candidate-batch data parallelism over RCCL / xGMI. One process per GPU, one
 * communicator per context; rank r owns global candidates [r*B_local, (r+1)*B_local). The reference has
 * no distributed code: these entry points are new design, not replacements. */
#define MPCD_COMM_ID_BYTES 128
/* Rank 0 creates the id (ncclGetUniqueId) and ships its 128 bytes to every rank out of band. */
int mpcd_comm_unique_id(void *id_out);
int mpcd_comm_init(mpcd_ctx *ctx, int32_t nranks, int32_t rank, const void *id);
/* Loopback communicator: `nranks` VIRTUAL ranks = nranks contexts on the same device in one process,
 * each context driven by its own host thread, joined by a caller-chosen group_key. The collectives are
 * device copies ordered by HIP events plus a host rendezvous of the member threads (120 s timeout), so
 * mpcd_select / mpcd_mpc_step run their N-rank code (rank offsets, gathered-cost order, owner-row sum,
 * flag max-reduction) on one GPU: the single-GPU rehearsal and test of the RCCL path. */
int mpcd_comm_init_loopback(mpcd_ctx *ctx, int32_t nranks, int32_t rank, uint64_t group_key);

/* ---- native training step: GaussianDiffusionModel.loss / p_losses with CFG context
 * dropout (diffusion_model_base.py:434-467), WeightedL2 (helpers.py:71-99), backward, torch.optim.Adam
 * (trainer.py:152) and the EMA model (trainer.py:70-88, 302-308), on the device in fp32. The CFG MLP net and
 * ConditionedTemporalUnet (MPCD_NET_UNET with cfg_masked; training always runs in fp32 whatever desc->dtype). The random draws of p_losses (t ~ randint, noise ~ randn_like, context_mask ~
 * bernoulli(drop_prob)) are inputs, so a caller reproduces the reference's RNG stream exactly. */
typedef struct mpcd_trainer mpcd_trainer;
typedef struct {
    float lr, beta1, beta2, eps; /* Adam (torch defaults: 0.9, 0.999, 1e-8) */
    float ema_decay;             /* EMA beta (trainer default 0.995) */
    int32_t step_start_ema;      /* before this step the EMA model is reset to the model (trainer: 1000) */
    int32_t update_ema_every;    /* EMA update period in steps (trainer: 10) */
} mpcd_train_cfg;
/* params: the net's parameters in mpcd_net_param_info() order; the schedule's sqrt(abar) and
 * sqrt(1 - abar) [n_steps] (q_sample). The EMA model starts as a copy of params. */
int mpcd_trainer_create(const mpcd_net_desc *desc, const float *params, size_t n_floats, const mpcd_train_cfg *cfg,
                        const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod, int32_t n_steps,
                        mpcd_trainer **out);
/* One batch (device pointers): x0 [B][H*d] normalised trajectories, context [B][C], t [B] (int64, < n_steps),
 * noise [B][H*d], context_mask [B] (1 = context dropped); t outside [0, n_steps) is clamped on the device (the
 * Python wrapper rejects it). update = 0: the loss only (p_losses forward);
 * 1: loss, backward, Adam step, EMA update. Blocks until done; *loss = mean((eps_pred - noise)^2). */
int mpcd_trainer_step(mpcd_trainer *tr, const float *x0, const float *context, const int64_t *t, const float *noise,
                      const float *context_mask, int64_t batch, int32_t update, double *loss, void *hip_stream);
/* which: 0 parameters, 1 EMA parameters, 2 last gradients, 3 Adam exp_avg, 4 Adam exp_avg_sq (host copy) */
int mpcd_trainer_params(mpcd_trainer *tr, int32_t which, float *host_out, size_t n_floats);
/* Data-parallel training: each rank steps on its own rows; the flat gradient is sum-all-reduced over the
 * communicator and divided by nranks before Adam (DistributedDataParallel's averaging), so all ranks keep
 * identical parameters and EMA. RCCL (one process per GPU; id from mpcd_comm_unique_id) or an in-process
 * loopback group of nranks trainers on one GPU, each stepped from its own host thread. */
int mpcd_trainer_comm_init(mpcd_trainer *tr, int32_t nranks, int32_t rank, const void *unique_id);
int mpcd_trainer_comm_init_loopback(mpcd_trainer *tr, int32_t nranks, int32_t rank, uint64_t group_key);
void mpcd_trainer_destroy(mpcd_trainer *tr);
int mpcd_comm_info(mpcd_ctx *ctx, int32_t *nranks, int32_t *rank);  /* 1, 0 without mpcd_comm_init */
/* recv [nranks * count_per_rank] (rank order); without a communicator: a device copy. */
int mpcd_allgather_f32(mpcd_ctx *ctx, const float *send, float *recv, size_t count_per_rank, void *hip_stream);
int mpcd_allgather_f64(mpcd_ctx *ctx, const double *send, double *recv, size_t count_per_rank, void *hip_stream);
int mpcd_broadcast_f32(mpcd_ctx *ctx, float *buf, size_t count, int32_t root, void *hip_stream);
int mpcd_allreduce_max_i32(mpcd_ctx *ctx, int32_t *buf, size_t count, void *hip_stream);  /* OR of clip flags */
/* The per-control-step exchange, device-resident end to end (no host round trip): all-gather the fp64
 * costs into costs_all [nranks * n_local], global argmin (torch.argmin(cost_all), inference_(mpd).py:335-338;
 * NaN = +inf, lowest global index on ties) into *best_dev, and the winner's row [row_len] (its normalised
 * [H][d] trajectory) into row_out on every rank (owner writes it, the others zeros, sum all-reduce). */
int mpcd_select(mpcd_ctx *ctx, const double *cost_local, int64_t n_local, const float *rows_local, int32_t row_len,
                double *costs_all, mpcd_best *best_dev, float *row_out, void *hip_stream);

/* ---- One control step in one call: the whole per-step path of Diffusion_MPC_Inference.py:229-262 /
 * Cart_Diffusion_inference.py:439-470 (normalize_condition -> run_CFG -> unnormalize_states -> cost of
 * every candidate -> argmin -> applied action) for this rank's shard, plus the exchange of mpcd_select
 * when the context has a communicator. Everything stays on the device until the result block leaves it: on one
 * rank the selecting rollout workgroup writes it to mapped pinned host memory followed by a completion word the
 * call spins on (no copy launch, no stream-synchronisation wake-up; every kernel's device writes precede that
 * word); with a communicator one D2H copy and a stream synchronisation. best_host / u_best_host are valid on
 * return either way. */
/* The reference scripts call run_CFG(..., return_chain=True) and unnormalise the WHOLE chain
 * (Cart_Diffusion_inference.py:450-463, Diffusion_MPC_Inference.py:232-247), so the clip test sees x_T
 * ~ N(0, 1) as well and practically always clips. MPCD_CLIP_CHAIN reproduces that (the default);
 * MPCD_CLIP_FINAL tests the final samples only (a caller that unnormalises just x_0); MPCD_CLIP_NONE: the
 * caller has proven the final-only flag 0 (DDPM whose last posterior mean cannot leave [-1, 1]). */
enum mpcd_clip_rule { MPCD_CLIP_CHAIN = 0, MPCD_CLIP_FINAL = 1, MPCD_CLIP_NONE = 2 };

typedef struct {
    const mpcd_system_desc *sys;   /* n_u == the net's state_dim */
    const double *x0;              /* host [n_x] fp64 plant state */
    const float *ctx_min, *ctx_max; /* host [C] condition limits: ctx = fp32(2*((x0-min)/fp32(max-min)) - 1) in fp64
                                      (LimitsNormalizer.normalize, normalization.py:149-154) */
    const float *act_min, *act_max; /* host [d] action limits (LimitsNormalizer.unnormalize, :156-167) */
    mpcd_sample_args sample;       /* .context / .context_shared are ignored (the normalised x0 is the shared
                                      context); .batch = B_local; .global_offset = rank * B_local; .x_out required;
                                      .chain_absmax is set by the call itself under MPCD_CLIP_CHAIN */
    int32_t clip_rule;             /* mpcd_clip_rule: which tensor LimitsNormalizer's global clip test runs over */
    double *cost_local;            /* dev [batch] fp64 costs of this rank's candidates (out) */
    double *costs_all;             /* dev [nranks * batch] all costs (out), needed with a communicator, else unused */
} mpcd_step_args;

/* Ordering: best_host / u_best_host are complete when the call returns (one rank: the call spins on a completion word
 * the selecting workgroup writes to mapped host memory after the result block; with a communicator: a stream
 * synchronisation). The DEVICE outputs (sample.x_out, cost_local, costs_all) are ordered only on hip_stream: read them
 * from another stream or from the host after a stream synchronisation or an event.
 * best_host: global winner (index over all ranks); u_best_host: host [H*d] fp32, the winner's
 * UNnormalised trajectory (u_best[0] is the applied action before the reference's rounding).
 * Returns MPCD_ENONFINITE (outputs written) when the winning cost is not finite, i.e. every candidate of
 * every rank is NaN / Inf - garbage is never returned as a normal result. */
int mpcd_mpc_step(mpcd_ctx *ctx, const mpcd_step_args *args, mpcd_best *best_host, float *u_best_host,
                  void *hip_stream);
/* mpcd_mpc_step whose sampler call is mpcd_sample_warm with one prior for every candidate (warm->rows == 1; t_start
 * == 0: a cold step), plus the next step's prior: when next_init_out != NULL (dev [H][d]) one mpcd_shift_plans launch
 * on the winner's normalised plan follows the selection on hip_stream (one rank: row best.index - global_offset of
 * sample.x_out; with a communicator: the all-reduced winner row, so every rank holds the same prior). It is a DEVICE
 * output, ordered on hip_stream like sample.x_out, and may alias nothing the step reads - in particular not
 * warm->x_init: keep two buffers and swap them. The MPCD_F16X2 re-run rule is mpcd_mpc_step's. mpcd_mpc_step itself
 * is unchanged (no launch, no branch added).
 * Clip rule: under MPCD_CLIP_CHAIN the tested chain of a warm step starts at the noised prior, not at x_T ~ N(0, 1),
 * so the flag is no longer "practically always 1": it is 1 only if some chain value really leaves [-1 - 1e-4,
 * 1 + 1e-4] (likely at K near N, where sb ~ 1; rare at a small K with a prior inside [-1, 1]). That is what the
 * reference's whole-chain unnormalise would see for such a chain; a caller who wants the cold step's (clipping)
 * behaviour at every K has no rule for it here. */
int mpcd_mpc_step_warm(mpcd_ctx *ctx, const mpcd_step_args *args, const mpcd_warm_start *warm /* rows == 1 */,
                       float *next_init_out /* dev [H][d] or NULL */, mpcd_best *best_host, float *u_best_host,
                       void *hip_stream);
/* mpcd_mpc_step_warm with an elite set (single rank). Differences:
 *  - warm->rows is 1 (one prior for every candidate) or sample.batch (one per candidate: the priors a previous call
 *    wrote); t_start == 0 is a cold step that still fills the priors.
 *  - after the selection, mpcd_topk over cost_local (one group of `batch`, index_offset = sample.global_offset) and,
 *    next_priors_out non-null, mpcd_elite_priors(shift = 1) of sample.x_out into next_priors_out follow on hip_stream:
 *    candidate j's next prior is elite j mod k's plan moved one horizon point ahead, so row 0 is the winner's.
 *    next_priors_out is a DEVICE output ordered on hip_stream, like next_init_out.
 *  - elites_host non-null: the k elites {cost, global index}, best first, complete when the call returns like
 *    best_host (the top-k launch writes them to mapped host memory and the call waits for its completion word);
 *    elites_host[0] equals *best_host.
 * The MPCD_F16X2 re-run rule is mpcd_mpc_step's: next_priors_out may not overlap warm->x_init (keep two buffers and swap
 * them), nor sample.x_out.
 * MPCD_EINVAL: mpcd_mpc_step_warm's cases; k < 1, k > sample.batch or k > MPCD_MAX_ELITES; t_start > 0 with rows
 * neither 1 nor batch; next_priors_out overlapping warm->x_init. MPCD_EUNSUP: a context with a communicator (the elite
 * rows live on other ranks; exchanging them is separate work); t_start > 0 with a DDIM sampler. */
int mpcd_mpc_step_elite(mpcd_ctx *ctx, const mpcd_step_args *args, const mpcd_warm_start *warm /* rows == 1 or batch */,
                        int32_t k, float *next_priors_out /* dev [batch][H][d] or NULL */,
                        mpcd_best *elites_host /* [k] or NULL */, mpcd_best *best_host, float *u_best_host,
                        void *hip_stream);

/* Failure-detection flags of the last mpcd_mpc_step on this context (read after it returned):
 * bit 0 (MPCD_STEP_CLIPPED): LimitsNormalizer's global clip was applied; bit 1 (MPCD_STEP_NAN_SAMPLES): some
 * candidate's tested tensor (its chain under MPCD_CLIP_CHAIN, its final sample under MPCD_CLIP_FINAL) holds a
 * NaN on some rank - the reference's torch max()/min() are then NaN and nothing is clipped; bit 2
 * (MPCD_STEP_NONFINITE_WINNER): no finite cost (the call returned MPCD_ENONFINITE); bit 3 (MPCD_STEP_F32X3_RERUN): an
 * MPCD_F16X2 net's step left the fp16 range (NaN samples or no finite cost, one rank) and was re-run with the net's
 * split-bf16 programs - the other bits and the outputs are the re-run's. */
enum { MPCD_STEP_CLIPPED = 1, MPCD_STEP_NAN_SAMPLES = 2, MPCD_STEP_NONFINITE_WINNER = 4, MPCD_STEP_F32X3_RERUN = 8 };
int mpcd_last_step_flags(mpcd_ctx *ctx, int32_t *flags);

/* mpcd_mpc_step / _warm / _elite with a constraint set ("Constraint set" above) and the feasibility-first order, on
 * one rank or over a communicator. warm NULL: a cold step; else mpcd_mpc_step_warm's (k == 0) or mpcd_mpc_step_elite's
 * (k >= 1) warm start. All results below are for the same samples, x0, global clip flag, set and u_prev:
 *  - cost_local / viol_local are bit for bit what mpcd_rollout_cost_constr writes with group = batch, the one start
 *    state x0 and the step's global clip flag.
 *  - *best_host, *viol_host and *n_feasible_host are bit for bit entry 0, its V and the count of
 *    mpcd_topk_feasible(k = 1, tol, index_offset = 0) over the gathered arrays of all ranks, in rank order: indices are
 *    global, a NaN cost is reported as +inf. (One rank: index_offset = sample.global_offset, as in mpcd_mpc_step.)
 *  - u_best_host is the winner's row unnormalised with the global clip flag, as mpcd_mpc_step does.
 *  - k == 0: next_priors_out (dev [H][d] or NULL) is mpcd_shift_plans on the winner; with a communicator it is taken
 *    from the all-reduced winner row, identical on every rank, as in mpcd_mpc_step_warm.
 *  - k >= 1 (single rank): elites_host / elite_viol_host are entries 0..k of mpcd_topk_feasible(k, tol) over
 *    cost_local / viol_local, elites_host[0] equals *best_host, and next_priors_out (dev [batch][H][d] or NULL) is
 *    mpcd_elite_priors(shift = 1) on that list.
 *  - A set that is only a box gives the box's V. An all-infinite set with tol = 0 and no u_prev gives bit for bit the
 *    results of mpcd_mpc_step / _warm / _elite (V = 0 then, except that a candidate with a NaN state has V = +inf and
 *    ranks after every candidate without one: mpcd_mpc_step_batch_box's caveat).
 * Flags (mpcd_last_step_flags): the bits above keep their meaning; MPCD_STEP_INFEASIBLE (16) is set exactly when
 * *n_feasible_host == 0 - a flag, not an error: the return code stays MPCD_OK. MPCD_ENONFINITE is returned, with all
 * outputs written, when the selected cost is not finite. The MPCD_F16X2 re-run rule is mpcd_mpc_step's (single rank);
 * next_priors_out may not alias warm->x_init or sample.x_out. A refused call leaves the flags as they were.
 * One rank: the sampler, then ONE launch (rollout_constr_select_kernel, csrc/rollout.hip: rollout, cost, V, the
 * selection, the winner's row); with elites the mpcd_topk_feasible and mpcd_elite_priors launches follow. The result
 * returns through mapped host memory and a completion word, V and n_feasible included. With a communicator: the
 * clip-flag launch and its max-reduce, the producer launch, all-gathers of the costs and of the violations,
 * mpcd_topk_feasible over the gathered arrays (one group, k = 1), the owner-row sum all-reduce, one device-to-host copy
 * and one stream synchronisation.
 * MPCD_EINVAL: mpcd_mpc_step_warm's / _elite's cases; con or con->con NULL; mpcd_rollout_cost_constr's cases for the
 * set; tol negative or NaN; viol_local, viol_host or n_feasible_host NULL; viols_all NULL with a communicator;
 * reserved != 0; k < 0, k > sample.batch or k > MPCD_MAX_ELITES; warm->t_start > 0 with warm->rows not 1 (k == 0), or
 * neither 1 nor batch (k >= 1); elites_host or elite_viol_host given with k == 0. MPCD_EUNSUP: k >= 1 with a
 * communicator (multi-rank elites stay out); t_start > 0 with a DDIM sampler. */
typedef struct {
    const mpcd_constraints *con;  /* host; mpcd_rollout_cost_constr's rules and refusals */
    double tol;                   /* mpcd_topk_feasible's tol */
    const double *u_prev_host;    /* host [n_u] or NULL: the action applied last; a NaN entry: none */
    double *viol_local;           /* dev [batch] out: V of this rank's candidates (required) */
    double *viols_all;            /* dev [nranks * batch] out; required with a communicator, else unused */
    int32_t k;                    /* 0: winner only; 1 .. min(batch, MPCD_MAX_ELITES): elites (single rank) */
    int32_t reserved;             /* 0 */
    float *next_priors_out;       /* dev or NULL. k == 0: [H][d], mpcd_mpc_step_warm's next_init_out;
                                     k >= 1: [batch][H][d], mpcd_mpc_step_elite's next_priors_out */
    mpcd_best *elites_host;       /* host [k] or NULL */
    double *elite_viol_host;      /* host [k] or NULL (k >= 1) */
    double *viol_host;            /* host [1]: the selected candidate's V (required) */
    int64_t *n_feasible_host;     /* host [1]: candidates of ALL ranks with V <= tol (required) */
} mpcd_step_constr_args;
int mpcd_mpc_step_constr(mpcd_ctx *ctx, const mpcd_step_args *args, const mpcd_warm_start *warm /* NULL: cold */,
                         const mpcd_step_constr_args *con, mpcd_best *best_host, float *u_best_host, void *hip_stream);

/* U-Net conv tilings (MPCD_F32X3 / MPCD_F16). Each conv launch picks rows-per-workgroup x register tile
 * x persistent-or-not among candidates by timing them once per layer shape and batch, and each
 * ResidualTemporalBlock picks fused-or-not the same way. This process-wide override makes the choice
 * deterministic, so a caller can run EVERY candidate on its own batch (they are bit-identical: the
 * K order and the GroupNorm summation order do not depend on the tiling):
 *   conv_pick  -1 = measured (default); i >= 0 = candidate (i mod count) for every conv, blocks unfused
 *              unless block_pick says otherwise;
 *   block_pick -1 = measured; -2 = never fuse; i >= 0 = fused candidate (i mod count) for every block. */
int mpcd_unet_force_tiling(int32_t conv_pick, int32_t block_pick);
/* MLP split-bf16 sampler workgroup layout (rows x waves), process-wide: -1 = by batch size (default: rw32x8, or
 * rw16 when 32-row workgroups would leave CUs idle); 0 = 32x8; 1 = 16x8; 2 = 16x4 (two 4-wave workgroups per
 * CU where their LDS fits, else 16x8); 3 / 4 = rw32 / rw16 (csrc/mlp_rw.hip: 32 / 16 rows on 4 waves, the
 * 128-wide layers' weights resident in registers for the whole launch); 5 = rw32x8 (the same kernel on 8 waves,
 * two per SIMD, 32 rows: Linear 5, 6 and half of Linear 7 resident). All layouts compute the same sums in the
 * same order (bit-identical results). */
int mpcd_mlp_force_layout(int32_t layout);
/* The layout (0..5 as above) an MPCD_F32X3 MLP sample call of `batch` candidates runs on the current device
 * (cfg_masked: CFG net, two rows per candidate). */
int mpcd_mlp_layout(int64_t batch, int32_t cfg_masked, int32_t *layout_out);
/* Which kernel an mpcd_sample / mpcd_mpc_step call with this sampler and `batch` candidates (shared context) runs
 * on this context's MLP, on its device: out[0] = 0 exact fp32 (mlp_sample_kernel), 1 split bf16 (mlp_x3_kernel /
 * mlp_rw_kernel), 2 two-term fp16 (mlp_h2_kernel); out[1] = the bf16x3 layout (as mpcd_mlp_layout) or -1;
 * out[2] = rows per workgroup (32 or 16). MPCD_EUNSUP on a U-Net context. */
int mpcd_mlp_form(mpcd_ctx *ctx, int32_t sampler, int64_t batch, int32_t out[3]);
/* The same for an mpcd_sample_grouped call of n_groups x group candidates: out[0] is 0 or 1 (never 2: the fp16
 * kernel takes no grouped call); the layout is chosen for the workgroups such a call launches,
 * n_groups * ceil(group / candidates per workgroup), with 16 rows where a group fills at most half of a 32-row
 * workgroup. mpcd_mlp_force_layout wins here too. */
int mpcd_mlp_form_grouped(mpcd_ctx *ctx, int32_t sampler, int64_t n_groups, int64_t group, int32_t out[3]);
/* on != 0: an MPCD_F16X2 net runs its split-bf16 (MPCD_F32X3) programs for every call on this context until turned
 * off again (mpcd_mpc_step does this by itself for one re-run when an MPCD_F16X2 step's samples come back with a NaN
 * or without a finite cost: the fp16 range was left; MPCD_STEP_F32X3_RERUN flags it). */
int mpcd_force_f32x3(mpcd_ctx *ctx, int32_t on);
/* U-Net execution form, process-wide. The whole-network form (csrc/unet_fused.hip: every conv of one denoise
 * step in ONE launch, a workgroup per few candidates, activations in LDS) covers the CFG samplers and the
 * two-branch eps of ConditionedTemporalUnet(base 32, dim_mults (1, 2, 4)) at H = 32 / 64 with the MPCD_F32X3
 * or MPCD_F16 numerics; everything else runs layer by layer (one launch per conv). 0 = automatic (the fused
 * form where it applies; env MPCD_UNET_FUSED=0 turns it off), 1 = layer by layer, 2 = fused (a sample / eps
 * call it does not cover returns MPCD_EUNSUP). */
int mpcd_unet_force_path(int32_t path);
/* Which form an mpcd_sample call with this sampler (mpcd_sampler) takes on this context's U-Net under the
 * current mpcd_unet_force_path / MPCD_UNET_FUSED settings: out[0] = 1 whole-network fused launch per denoise
 * step / 0 layer by layer, out[1] = GEMM operand planes (0 exact fp32, 1 fp16, 3 split bf16), out[2] = rows
 * (candidate x CFG branch) and out[3] = waves per workgroup of the fused launch. MPCD_EUNSUP on an MLP
 * context. */
int mpcd_unet_form(mpcd_ctx *ctx, int32_t sampler, int32_t out[4]);
#define MPCD_UNET_MAX_CONV_TILINGS 12   /* 6 rows-per-workgroup values x {tiled, persistent} */
#define MPCD_UNET_MAX_BLOCK_TILINGS 6

/* Timing of the last mpcd_sample's main kernel (HIP events on the call's stream), milliseconds.
 * Blocks until that kernel has finished. */
int mpcd_last_sample_ms(mpcd_ctx *ctx, float *ms);
/* Mean of that timing over the last n sample calls (1 <= n <= 256 and <= the calls made): a timed control loop reads
 * it once afterwards instead of one mpcd_last_sample_ms per step. Blocks until the last of them has finished. */
int mpcd_sample_ms_mean(mpcd_ctx *ctx, int32_t n, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* MPCD_H */
