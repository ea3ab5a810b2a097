// Internal (non-ABI) declarations shared by the libmpcd.so translation units.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/mpcd.h"
#include "common.h"

// One conditioning Linear (cond_mlp.1 of a residual / MLP block): out width `width`, weight
// [width][cond_dim] row-major, written at column `off` of the per-step / per-candidate tables.
struct CondLayer {
    const float *W;
    const float *b;
    int32_t width;
    int32_t off;
};

// Time-embedding prologue: tproj[s][off_j + n] = cond_mlp_j.W[n, :T] . Mish(t_emb(t_s)) + b_j[n]
void launch_time_prologue(const StepPlan *plan, int n_steps, const float *time_w1, const float *time_b1,
                          const float *time_w2, const float *time_b2, const CondLayer *layers_dev, int n_layers,
                          int cond_dim, int cond_total, float *tproj, hipStream_t stream);

// Context prologue: cproj[b][off_j + n] = cond_mlp_j.W[n, T:] . Mish(ctx_b)   (no bias)
void launch_ctx_prologue(const float *ctx, int64_t n_rows, int ctx_dim, const CondLayer *layers_dev, int n_layers,
                         int cond_dim, int cond_total, float *cproj, hipStream_t stream);
// dst[b][:] = src[b / group][:] for b < batch (rows of cond_total floats): a grouped call's projections as the
// per-candidate table of the U-Net kernels
void launch_ctx_replicate(const float *src, int64_t batch, int64_t group, int cond_total, float *dst, hipStream_t stream);
// one shared context row passed by value (mpcd_mpc_step: no host-to-device copy before the sampler)
constexpr int kCtxRowMax = 64;
struct CtxRowArg {
    float v[kCtxRowMax];
};
constexpr int kCondTdim = 32;  // time_emb_dim: the cond Linears' first input columns (cond_prologue.hip TDIM)
// Column col of one shared context row's projection, cond_mlp_j.W[n, T:] . Mish(ctx) in fp64: the body of
// ctx_prologue_row_kernel, and of the fp16 MLP kernel's in-launch form (mpcd_mpc_step), so both give the same bits
MPCD_DEV float ctx_proj_col(const CtxRowArg &row, int ctx_dim, const CondLayer *layers, int n_layers, int cond_dim,
                            int col)
{
    int l = 0;
    while (l + 1 < n_layers && layers[l + 1].off <= col) ++l;
    const CondLayer L = layers[l];
    const int n = col - L.off;
    double acc = 0.0;
    for (int k = 0; k < ctx_dim; ++k)
        acc += (double)L.W[(size_t)n * cond_dim + kCondTdim + k] * (double)mish_precise(row.v[k]);
    return (float)acc;
}
void launch_ctx_prologue_row(const CtxRowArg &row, int ctx_dim, const CondLayer *layers_dev, int n_layers,
                             int cond_dim, int cond_total, float *cproj, hipStream_t stream);

// The samplers' Philox noise stream for candidates [goff, goff + n): out [n_slices][n][flat] (mpcd_philox_noise)
hipError_t launch_philox_noise(uint64_t seed, int64_t goff, int64_t n, int n_slices, int flat, float *out,
                               hipStream_t stream);

// Thread-safe launch state (several host threads may launch, e.g. the loopback communicator's ranks):
// allow_max_lds<&kernel>() raises the kernel's dynamic-LDS cap to 160 KiB exactly once per kernel and
// device (the attribute belongs to the current device's copy of the function; a std::call_once per
// device, whichever thread gets there first, the others wait for it); device_cu_count() is the
// compute-unit count of the CURRENT device, cached per device.
constexpr int kMaxDevices = 64;
template <auto Kernel>
inline hipError_t allow_max_lds()
{
    static std::once_flag once[kMaxDevices];
    static hipError_t err[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    std::call_once(once[dev], [dev] {
        err[dev] = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    });
    return err[dev];
}
int device_cu_count();

// The sample call's timing events handed to the MLP sampler's one launch: hipExtLaunchKernel records them as part of
// that dispatch, so no hipEventRecord call sits on the host path in front of the launch (sample_impl sets them for the
// launch and clears them after; null otherwise)
struct LaunchEvents {
    hipEvent_t start, stop;
};
extern thread_local LaunchEvents g_launch_ev;
template <typename K, typename A>
inline hipError_t launch_sampler_kernel(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A &args)
{
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, g_launch_ev.start, g_launch_ev.stop, 0u, args);
    return hipGetLastError();
}

struct MlpSampleArgs {
    const float *wpack;      // packed linear layers (see mlp_sampler.hip)
    const StepPlan *plan;    // [S]
    const float *tproj;      // [S][448]
    const float *cproj;      // [B or 1][448], [B / group][448] if grouped, or null (no context / NB == 1 unconditioned)
    int64_t cproj_stride;    // 448 or 0 (shared context); 448 for a grouped call
    const float *noise;      // [S+1][B][D0] or null
    float *x_out;            // [B][D0]
    float *chain;            // [S+1][B][D0] or null
    float *chain_absmax;     // [B] or null: max |x| over the chain per candidate (bits of a NaN if any)
    int64_t batch;
    int64_t global_offset;
    uint64_t seed;
    int32_t n_steps;
    int32_t mode;            // MODE_*
    int32_t clamp_x0;
    float wp1, wf;           // fp32(1 + w), fp32(w)
    float *dbg;              // debug: block 0 dumps every layer output [14][32][256] (null in production)
    // mpcd_mpc_step with the fp16 kernel: the shared context row's projection computed in the launch (cps staging)
    // instead of read from cproj (no ctx prologue launch); cproj still non-null (selects the ctx instantiation)
    int32_t ctx_fused;
    int32_t ctx_dim, n_cond, cond_dim;
    const CondLayer *cond_layers;
    CtxRowArg ctx_row;
    // mpcd_sample_grouped: candidate b uses context row b / group (cproj [batch / group][448]); 0 = not grouped
    // (cproj_stride says shared or per candidate). group_wgs = ceil(group / candidates per workgroup): set by the
    // split-bf16 launchers for their own layout (their workgroups never straddle a group), 0 elsewhere
    int64_t group;
    int32_t group_wgs;
    // warm start (mpcd_sample_warm): x_init [rows][D0] or null = start from noise slice 0 as it is; else the chain
    // starts at q_sample4(x_sa, x_sb, x_init[row], slice 0) with row by x_init_kind (XINIT_*; per group: b / group)
    int32_t x_init_kind;
    const float *x_init;
    float x_sa, x_sb;
};

int mlp_packed_floats(int d0);
void mlp_pack_weights(int d0, const float *const *lin_w, const float *const *lin_b, float *out);
hipError_t launch_mlp_sampler(int d0, int nb, const MlpSampleArgs &a, hipStream_t stream);
// fp32-accurate split-bf16 variant (mlp_x3.hip); shared, grouped (MlpSampleArgs::group) or no context
int mlp_packed_floats_x3(int d0);
void mlp_x3_force_layout(int layout);  // mpcd_mlp_force_layout
int mlp_x3_layout_of(int64_t batch, int nb);  // mpcd_mlp_layout: the layout a call of this batch runs
int mlp_x3_layout_grouped(int64_t n_groups, int64_t group, int nb);  // ... and a grouped call of n_groups x group
void mlp_pack_weights_x3(int d0, const float *const *lin_w, const float *const *lin_b, float *out);
hipError_t launch_mlp_x3(int d0, int nb, const MlpSampleArgs &a, hipStream_t stream);
// resident-weight variant (mlp_rw.hip), selected by mlp_x3's layout choice: rows = 32 or 16 per workgroup
hipError_t launch_mlp_rw(int d0, int rows, int waves, const MlpSampleArgs &a, hipStream_t stream);
// two-term fp16 variant (mlp_h2.hip, MPCD_F16X2): CFG-DDPM / eps at H*d 32 / 64, shared context; rows 32 or 16
bool mlp_h2_supports(int d0, int mode);
int mlp_packed_floats_h2(int d0);
void mlp_pack_weights_h2(int d0, const float *const *lin_w, const float *const *lin_b, float *out);
hipError_t launch_mlp_h2(int d0, int rows, const MlpSampleArgs &a, hipStream_t stream);

// Fused selection for launch_rollout_cost (single rank): see rollout.hip SelectK
constexpr int64_t kFuseClipMax = 16384;  // clip inputs up to this many floats are tested inside the selecting launch
struct RolloutSelect {
    mpcd_best *best;
    float *row_out;
    double *part_cost;
    int64_t *part_idx;
    unsigned *counter;    // zero-initialised, reset by the kernel
    int64_t n_part;       // capacity of part_* (>= ceil(batch / 64))
    int64_t offset;
    int32_t *code_out;    // optional: the clip code flags[0], written with the winner (mpcd_mpc_step's result block)
    // optional: the clip code is computed in this launch, by every workgroup, over clip_src[0, clip_n) (the
    // clip_flag_kernel test; a small batch's per-candidate chain maxima) instead of read from flag_dev
    const float *clip_src;
    int64_t clip_n;
    // optional: the result block {best, winner row, clip code} (step_out's layout) also written by the selecting
    // workgroup to mapped host memory, then *host_flag = host_seq after a system-scope fence: mpcd_mpc_step spins
    // on that word instead of a device-to-host copy and a stream synchronisation
    char *host_out;
    uint32_t *host_flag;
    uint32_t host_seq;
};
constexpr int kRolloutBlock = 64;  // candidates per rollout workgroup

// The two control tails (rollout.hip) do everything after the sampler in one launch of n_states * ceil(group /
// kRolloutBlock) workgroups. What both take to select each state's candidate; device pointers.
struct TailCommon {
    const float *u_norm;   // [n_states * group][H][n_u] this call's samples
    const float *clip_src; // chain rule: chain_absmax [n_states * group]; final rule: u_norm
    int64_t clip_per_state;  // floats of clip_src per state: group, or group * H * n_u
    double *x_dev;         // [n_states][n_x]; the closed loop steps it in place, the batched step only reads it
    int64_t n_states, group;
    int32_t H, select_first, decimals;
    // per-workgroup partials [n_states * ceil(group / kRolloutBlock)] and one zero-initialised, self-resetting
    // counter per state
    double *part_cost, *part_raw;
    int64_t *part_idx;
    unsigned *counters;
};
// One closed-loop iteration's control tail (rollout.hip closed_loop_tail_kernel, mpcd_closed_loop)
struct ClosedLoopTail : TailCommon {
    // this iteration's history rows
    double *x_next, *u_applied, *best_cost;  // x_hist[it + 1], u_hist[it], cost_hist[it]
    int64_t *best_idx;                       // index_hist[it]
    // the next iteration's sampler inputs: one row per state, or (repeat_rows) each state's row repeated `group`
    // times, one per candidate; prior_out null: no warm start
    float *ctx_out;
    float *prior_out;
    int32_t repeat_rows;
};
hipError_t launch_closed_loop_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                   const float *cmin_host, const float *cmax_host, const ClosedLoopTail &t,
                                   hipStream_t stream);
// One control step of externally supplied states (rollout.hip batch_step_tail_kernel, mpcd_mpc_step_batch):
// the packed result block `result` is what one device-to-host copy returns: n_states records of rec_stride bytes,
// each {mpcd_state_result, double u[n_u]}, then at plan_off the selected plans, float [n_states][H * n_u].
struct BatchStepTail : TailCommon {
    char *result;
    int64_t rec_stride, plan_off;
    float *prior_out;      // [n_states][H][n_u] the next priors, or null
};
constexpr int64_t batch_step_rec_stride(int n_u) { return (int64_t)sizeof(mpcd_state_result) + 8 * n_u; }
hipError_t launch_batch_step_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                  const BatchStepTail &t, hipStream_t stream);
// The same step that also ranks each state's k best candidates (rollout.hip batch_step_elite_tail_kernel,
// mpcd_mpc_step_batch_elite): the result block gains, at elite_off (256-byte aligned, after the plans), the elites
// mpcd_best [n_states][k], best first in launch_topk's order and cost reporting. part_elite [n_states][ceil(group /
// kRolloutBlock)][k] holds the workgroups' ranked lists. select_first must be 0; prior_out is not written: the next
// priors are a launch_elite_priors on result + elite_off.
struct BatchEliteTail : BatchStepTail {
    mpcd_best *part_elite;
    int64_t elite_off;
    int32_t k;  // 1 <= k <= min(group, MPCD_MAX_ELITES)
};
hipError_t launch_batch_elite_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                   const BatchEliteTail &t, hipStream_t stream);
// The same step with a state box (rollout.hip batch_step_box_tail_kernel, mpcd_mpc_step_batch_box): selection and
// ranking in the feasibility-first order of mpcd.h's "State constraints" with tolerance tol. k = 1 without elites
// (prior_out may then be set, as in BatchStepTail); the k ranked entries are always written. After the plans the result
// block holds, in this order, the selected candidate's V double [n_states] at viol_off, n_feasible int64 [n_states] at
// nfeas_off, the entries mpcd_best [n_states][k] at elite_off and their V double [n_states][k] at eviol_off. part_viol
// [n_states][ceil(group / kRolloutBlock)][k] rides with part_elite, part_nfeas holds one count per workgroup.
struct BatchBoxTail : BatchEliteTail {
    double *part_viol;
    int64_t *part_nfeas;
    int64_t viol_off, nfeas_off, eviol_off;
};
hipError_t launch_batch_box_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                 const mpcd_state_box &box, double tol, const BatchBoxTail &t, hipStream_t stream);
// The same step with a constraint set (rollout.hip batch_step_box_tail_kernel<SYS, ConTolK>, mpcd_mpc_step_batch_constr): the box
// tail's argument block and result block; u_prev_dev [n_states][n_u] fp64 (a NaN row: none) or null.
hipError_t launch_batch_constr_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                    const mpcd_constraints &con, double tol, const double *u_prev_dev,
                                    const BatchBoxTail &t, hipStream_t stream);
// launch_rollout_cost_box with a constraint set (mpcd.h "Constraint set"); u_prev_dev [batch / group][n_u] or null
hipError_t launch_rollout_cost_constr(const mpcd_system_desc &d, const double *x0_dev, int64_t group, const float *u_norm,
                                      const float *umin_host, const float *umax_host, const int *flags_dev, int64_t batch,
                                      int H, const mpcd_constraints &con, const double *u_prev_dev, double *cost,
                                      double *viol, hipStream_t stream);
// The constraint set in the one-call control step (rollout.hip rollout_constr_select_kernel, mpcd_mpc_step_constr):
// launch_rollout_cost of the single-state step with the set, the one start state and the previous applied action
// (u_prev_host [n_u] or null; a NaN entry: none) by value; cost / viol [batch] are launch_rollout_cost_constr's bits.
// sel null: that is all (the multi-rank producer; flag_dev[0] is the clip code). sel: the selection in the
// feasibility-first order in the same launch, RolloutSelect's protocol; the result block, on the device (block) and in
// mapped host memory (host_out), is {mpcd_best, winner row [row] fp32, clip code int32, padding to 8 bytes, V double,
// n_feasible int64}.
constexpr size_t step_constr_viol_off(int row)
{
    return (sizeof(mpcd_best) + sizeof(float) * (size_t)row + sizeof(int32_t) + 7) & ~(size_t)7;
}
constexpr size_t step_constr_out_bytes(int row) { return step_constr_viol_off(row) + sizeof(double) + sizeof(int64_t); }
struct RolloutConstrSelect {
    char *block;          // the device result block, step_constr_out_bytes(row)
    double *part;         // 4 * n_part 8-byte entries: the workgroups' partials (V, cost, index, feasible count)
    int64_t n_part;       // >= ceil(batch / kRolloutBlock)
    unsigned *counter;    // zero-initialised, reset by the kernel
    int64_t offset;
    const float *clip_src;  // optional, as in RolloutSelect
    int64_t clip_n;
    char *host_out;         // optional mapped mirror of the block, the same layout
    uint32_t *host_flag;
    uint32_t host_seq;
};
hipError_t launch_rollout_constr_select(const mpcd_system_desc &d, const double *x0_host, const float *u_norm,
                                        const float *umin_host, const float *umax_host, const int *flag_dev, int64_t batch,
                                        int H, const mpcd_constraints &con, double tol, const double *u_prev_host,
                                        double *cost, double *viol, hipStream_t stream, const RolloutConstrSelect *sel);
// Elite sets (elite.hip). launch_topk: out[m][0..k) = the k best of cost[m * group, (m + 1) * group), best first, in
// rollout.hip's better() order, index = offset + position in cost[]; 1 <= k <= min(group, MPCD_MAX_ELITES).
// mirror (n_groups == 1 only): the entries also written to mapped host memory, then *host_flag = host_seq after a
// system-scope fence, as RolloutSelect's result block is.
struct TopkMirror {
    mpcd_best *host_out;
    uint32_t *host_flag;
    uint32_t host_seq;
};
hipError_t launch_topk(const double *cost, int64_t n_groups, int64_t group, int k, int64_t offset, mpcd_best *out,
                       hipStream_t stream, const TopkMirror *mirror = nullptr);
// out[m * group + j][h] = rows[elites[m][j % k].index - offset][min(h + shift, H - 1)]; rows / out [n_groups * group][H][d]
hipError_t launch_elite_priors(const float *rows, int64_t n_groups, int64_t group, int H, int d, const mpcd_best *elites,
                               int k, int64_t offset, int shift, float *out, hipStream_t stream);
// State constraints (mpcd.h). launch_rollout_cost_box (rollout.hip): launch_rollout_cost of a grouped call that also
// writes each candidate's violation of `box`; the costs are the grouped call's bits. launch_topk_feasible (elite.hip):
// launch_topk in the feasibility-first order; viol_out [n_groups][k] and n_feasible [n_groups] may be null.
// launch_control_step_picked (rollout.hip): launch_control_step with the selection supplied, state m applying candidate
// picks[m * pick_stride].index - offset of u_norm [batch][H][n_u].
hipError_t launch_rollout_cost_box(const mpcd_system_desc &d, const double *x0_dev, int64_t group, const float *u_norm,
                                   const float *umin_host, const float *umax_host, const int *flags_dev, int64_t batch,
                                   int H, const mpcd_state_box &box, double *cost, double *viol, hipStream_t stream);
// mirror (n_groups == 1 only; mpcd_mpc_step_constr with elites): the k entries and their V also written to mapped host
// memory, then *host_flag = host_seq after a system-scope fence, as TopkMirror does for launch_topk
struct TopkFeasMirror {
    mpcd_best *host_out;
    double *host_viol;
    uint32_t *host_flag;
    uint32_t host_seq;
};
hipError_t launch_topk_feasible(const double *cost, const double *viol, int64_t n_groups, int64_t group, int k, double tol,
                                int64_t offset, mpcd_best *out, double *viol_out, int64_t *n_feasible, hipStream_t stream,
                                const TopkFeasMirror *mirror = nullptr);
hipError_t launch_control_step_picked(const mpcd_system_desc &d, double *x_dev, int64_t M, const float *u_norm,
                                      int64_t batch, int H, const mpcd_best *picks, int64_t pick_stride, int64_t offset,
                                      const float *umin_host, const float *umax_host, const int *flags_dev, int decimals,
                                      double *u_applied, int64_t *best_idx, double *best_cost, hipStream_t stream);
// out[r * n + j][:] = rows[r][:] for j < n (the per-candidate rows of iteration 0 when the loop is not grouped)
hipError_t launch_repeat_rows(const float *rows, int64_t n_rows, int64_t n, int row_len, float *out, hipStream_t stream);
