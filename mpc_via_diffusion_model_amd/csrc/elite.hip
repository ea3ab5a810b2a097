// Elite sets (SURVEY §8f warm start): ranked top-k selection over each plant state's fp64 costs and the writer of the
// per-candidate warm-start priors seeded from them (mpcd_topk, mpcd_elite_priors, mpcd_mpc_step_elite), and the same
// ranking in the feasibility-first order of the state constraints (mpcd_topk_feasible).
// Built with -ffp-contract=off like every translation unit; nothing here rounds: costs are compared, plans copied.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "../../include/mpcd.h"
#include "internal.h"

namespace {

constexpr int TK_THREADS = 256;                  // 4 waves
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_ITEMS = 16;                     // costs per thread and chunk, in registers
constexpr int TK_CHUNK = TK_THREADS * TK_ITEMS;  // 4,096 costs: the headline group is one chunk

// rollout.hip's order: (v, i) beats (bv, bi): lower cost, then lower index; i < 0 = empty. NaN is +inf on load.
__device__ __forceinline__ bool tk_better(double v, int64_t i, double bv, int64_t bi)
{
    return i >= 0 && (bi < 0 || v < bv || (v == bv && i < bi));
}
// (v, i) comes strictly after the last pick (pv, pi) in that order; pi < 0: nothing picked yet
__device__ __forceinline__ bool tk_after(double v, int64_t i, double pv, int64_t pi)
{
    return pi < 0 || v > pv || (v == pv && i > pi);
}
__device__ __forceinline__ void tk_wave_argmin(double &v, int64_t &i)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int64_t oi = __shfl_xor(i, m);
        if (tk_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// One workgroup per group m ranks cost[m * group, (m + 1) * group) and writes the k best to out[m][0..k), best first:
// {cost (NaN reported as +inf), index_offset + position in cost[]}. Each cost is read from memory once: the group is
// taken in chunks of TK_CHUNK costs held in registers (thread t owns positions base + r * TK_THREADS + t, so the loads
// coalesce and every register index is static), and the k best so far ride along as one more item of threads 0..k-1.
// Per chunk, k rounds of workgroup argmin: every thread keeps the best of its items that come after the last pick,
// a round reduces those (wave shuffles, then the TK_WAVES partials through LDS, double-buffered: one barrier per
// round), and only the pick's owner rescans its items. All positions are distinct, so the (cost, index) order is
// strict and "after the last pick" excludes exactly what was picked before.
// mirror / host_flag (mpcd_mpc_step_elite, one group): the k entries also go to mapped host memory, then *host_flag =
// host_seq after a system-scope fence (rollout_cost_kernel's completion-word protocol).
__global__ __launch_bounds__(TK_THREADS) void topk_kernel(const double *cost, int64_t group, int k, int64_t offset,
                                                          mpcd_best *out, mpcd_best *mirror, uint32_t *host_flag,
                                                          uint32_t host_seq)
{
    __shared__ double pv_s[2][TK_WAVES];
    __shared__ int64_t pi_s[2][TK_WAVES];
    __shared__ double sel_v[MPCD_MAX_ELITES];
    __shared__ int64_t sel_i[MPCD_MAX_ELITES];
    const int t = threadIdx.x, wave = t >> 6;
    const int64_t m = blockIdx.x, g0 = m * group;
    double carry_v = INFINITY;  // this thread's entry of the best k of the chunks before (threads < k)
    int64_t carry_i = -1;
    for (int64_t base = 0; base < group; base += TK_CHUNK) {
        double v[TK_ITEMS];
#pragma unroll
        for (int r = 0; r < TK_ITEMS; ++r) {
            const int64_t p = base + r * TK_THREADS + t;
            double c = p < group ? cost[g0 + p] : INFINITY;
            if (isnan(c)) c = INFINITY;
            v[r] = c;
        }
        // local best over the thread's items after (pv, pi); positions past the group are empty
        auto rescan = [&](double pv, int64_t pi, double &lv, int64_t &li) {
            lv = INFINITY;
            li = -1;
            if (carry_i >= 0 && tk_after(carry_v, carry_i, pv, pi)) { lv = carry_v; li = carry_i; }
#pragma unroll
            for (int r = 0; r < TK_ITEMS; ++r) {
                const int64_t p = base + r * TK_THREADS + t;
                const int64_t i = p < group ? g0 + p : -1;
                if (i >= 0 && tk_after(v[r], i, pv, pi) && tk_better(v[r], i, lv, li)) { lv = v[r]; li = i; }
            }
        };
        double lv;
        int64_t li;
        rescan(-INFINITY, -1, lv, li);
        for (int r = 0; r < k; ++r) {
            double wv = lv;
            int64_t wi = li;
            tk_wave_argmin(wv, wi);
            const int buf = r & 1;
            if ((t & 63) == 0) { pv_s[buf][wave] = wv; pi_s[buf][wave] = wi; }
            __syncthreads();
            double pv = pv_s[buf][0];
            int64_t pi = pi_s[buf][0];
#pragma unroll
            for (int w = 1; w < TK_WAVES; ++w)
                if (tk_better(pv_s[buf][w], pi_s[buf][w], pv, pi)) { pv = pv_s[buf][w]; pi = pi_s[buf][w]; }
            if (t == 0) { sel_v[r] = pv; sel_i[r] = pi; }
            if (pi >= 0 && li == pi) rescan(pv, pi, lv, li);
        }
        __syncthreads();  // sel_* complete; the next chunk's rounds start on buffer 0 again
        carry_v = t < k ? sel_v[t] : INFINITY;
        carry_i = t < k ? sel_i[t] : -1;
        __syncthreads();  // every thread holds its entry before the next chunk overwrites sel_*
    }
    if (t < k) {
        const mpcd_best e{carry_v, carry_i < 0 ? -1 : offset + carry_i};
        out[m * k + t] = e;
        if (mirror) mirror[t] = e;
    }
    if (mirror) {  // every lane's host stores ordered before the completion word
        __threadfence_system();
        __syncthreads();
        if (t == 0) __hip_atomic_store(host_flag, host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- Feasibility-first ranking (mpcd.h "State constraints"): topk_kernel's algorithm on two values per item. An item
// is (V, cost, index): V its constraint violation (NaN = +inf on load), cost as above. The order is lexicographic on
// (g, cost, index) with g = V <= tol ? 0 : V: every feasible item before every infeasible one, feasible ones by cost,
// infeasible ones by violation first. g is recomputed from V where it is compared, so a pick carries its V as computed.
__device__ __forceinline__ double tf_key(double V, double tol) { return V <= tol ? 0.0 : V; }
// on (key, cost, index) triples, the keys computed by the caller (once per item and pick, not once per comparison)
__device__ __forceinline__ bool tf_better(double g, double v, int64_t i, double bg, double bv, int64_t bi)
{
    return i >= 0 && (bi < 0 || g < bg || (g == bg && (v < bv || (v == bv && i < bi))));
}
// (g, v, i) comes strictly after the last pick (pg, pv, pi); pi < 0: nothing picked yet
__device__ __forceinline__ bool tf_after(double g, double v, int64_t i, double pg, double pv, int64_t pi)
{
    return pi < 0 || g > pg || (g == pg && (v > pv || (v == pv && i > pi)));
}
__device__ __forceinline__ void tf_wave_argmin(double &V, double &v, int64_t &i, double tol)
{
    double g = tf_key(V, tol);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oV = __shfl_xor(V, m);
        const double ov = __shfl_xor(v, m);
        const int64_t oi = __shfl_xor(i, m);
        const double og = tf_key(oV, tol);
        if (tf_better(og, ov, oi, g, v, i)) { V = oV; g = og; v = ov; i = oi; }
    }
}

// One workgroup per group m, as topk_kernel: the group in chunks of TK_CHUNK items, both values of an item in registers
// (each cost and each violation is read from memory once), the k best so far riding along as one more item of threads
// 0..k-1. out[m][r] = {cost, offset + position}, viol_out[m][r] = that entry's V (NaN reported as +inf; not g), and
// n_feasible[m] = how many items of the whole group have V <= tol (0: entry 0 is the least violating one).
// MIRROR (mpcd_mpc_step_constr with elites, one group): the k entries and their V also go to mapped host memory, then
// *host_flag = host_seq after a system-scope fence (topk_kernel's protocol). A compile-time parameter: <false> is the
// kernel as it was, its trailing arguments never read.
template <bool MIRROR>
__global__ __launch_bounds__(TK_THREADS) void topk_feasible_kernel(const double *cost, const double *viol, int64_t group,
                                                                   int k, double tol, int64_t offset, mpcd_best *out,
                                                                   double *viol_out, int64_t *n_feasible,
                                                                   mpcd_best *mirror, double *mirror_viol,
                                                                   uint32_t *host_flag, uint32_t host_seq)
{
    __shared__ double pV_s[2][TK_WAVES], pv_s[2][TK_WAVES];
    __shared__ int64_t pi_s[2][TK_WAVES];
    __shared__ double sel_V[MPCD_MAX_ELITES], sel_v[MPCD_MAX_ELITES];
    __shared__ int64_t sel_i[MPCD_MAX_ELITES];
    __shared__ int64_t cnt_s[TK_WAVES];
    const int t = threadIdx.x, wave = t >> 6;
    const int64_t m = blockIdx.x, g0 = m * group;
    double carry_V = INFINITY, carry_v = INFINITY;  // this thread's entry of the best k of the chunks before (threads < k)
    int64_t carry_i = -1;
    int64_t feasible = 0;
    for (int64_t base = 0; base < group; base += TK_CHUNK) {
        double v[TK_ITEMS], V[TK_ITEMS];
#pragma unroll
        for (int r = 0; r < TK_ITEMS; ++r) {
            const int64_t p = base + r * TK_THREADS + t;
            double c = p < group ? cost[g0 + p] : INFINITY;
            double w = p < group ? viol[g0 + p] : INFINITY;
            if (isnan(c)) c = INFINITY;
            if (isnan(w)) w = INFINITY;
            v[r] = c;
            V[r] = w;
            feasible += p < group && w <= tol;
        }
        // local best over the thread's items after the pick; positions past the group are empty
        auto rescan = [&](double pV, double pv, int64_t pi, double &lV, double &lv, int64_t &li) {
            const double pg = tf_key(pV, tol);
            double lg = INFINITY;
            lV = INFINITY;
            lv = INFINITY;
            li = -1;
            if (carry_i >= 0) {
                const double g = tf_key(carry_V, tol);
                if (tf_after(g, carry_v, carry_i, pg, pv, pi)) { lV = carry_V; lg = g; lv = carry_v; li = carry_i; }
            }
#pragma unroll
            for (int r = 0; r < TK_ITEMS; ++r) {
                const int64_t p = base + r * TK_THREADS + t;
                const int64_t i = p < group ? g0 + p : -1;
                const double g = tf_key(V[r], tol);
                if (i >= 0 && tf_after(g, v[r], i, pg, pv, pi) && tf_better(g, v[r], i, lg, lv, li)) {
                    lV = V[r];
                    lg = g;
                    lv = v[r];
                    li = i;
                }
            }
        };
        double lV, lv;
        int64_t li;
        rescan(0.0, -INFINITY, -1, lV, lv, li);
        for (int r = 0; r < k; ++r) {
            double wV = lV, wv = lv;
            int64_t wi = li;
            tf_wave_argmin(wV, wv, wi, tol);
            const int buf = r & 1;
            if ((t & 63) == 0) { pV_s[buf][wave] = wV; pv_s[buf][wave] = wv; pi_s[buf][wave] = wi; }
            __syncthreads();
            double pV = pV_s[buf][0], pv = pv_s[buf][0], pg = tf_key(pV, tol);
            int64_t pi = pi_s[buf][0];
#pragma unroll
            for (int w = 1; w < TK_WAVES; ++w) {
                const double wg = tf_key(pV_s[buf][w], tol);
                if (tf_better(wg, pv_s[buf][w], pi_s[buf][w], pg, pv, pi)) {
                    pV = pV_s[buf][w];
                    pg = wg;
                    pv = pv_s[buf][w];
                    pi = pi_s[buf][w];
                }
            }
            if (t == 0) { sel_V[r] = pV; sel_v[r] = pv; sel_i[r] = pi; }
            if (pi >= 0 && li == pi) rescan(pV, pv, pi, lV, lv, li);
        }
        __syncthreads();  // sel_* complete; the next chunk's rounds start on buffer 0 again
        carry_V = t < k ? sel_V[t] : INFINITY;
        carry_v = t < k ? sel_v[t] : INFINITY;
        carry_i = t < k ? sel_i[t] : -1;
        __syncthreads();  // every thread holds its entry before the next chunk overwrites sel_*
    }
    if (t < k) {
        out[m * k + t] = mpcd_best{carry_v, carry_i < 0 ? -1 : offset + carry_i};
        if (viol_out) viol_out[m * k + t] = carry_V;
    }
    if constexpr (MIRROR) {
        if (t < k) {
            mirror[t] = mpcd_best{carry_v, carry_i < 0 ? -1 : offset + carry_i};
            mirror_viol[t] = carry_V;
        }
    }
    if (n_feasible) {  // uniform: a kernel argument
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) feasible += __shfl_xor(feasible, s);
        if ((t & 63) == 0) cnt_s[wave] = feasible;
        __syncthreads();
        if (t == 0) {
            int64_t n = 0;
#pragma unroll
            for (int w = 0; w < TK_WAVES; ++w) n += cnt_s[w];
            n_feasible[m] = n;
        }
    }
    if constexpr (MIRROR) {  // every lane's host stores ordered before the completion word
        __threadfence_system();
        __syncthreads();
        if (t == 0) __hip_atomic_store(host_flag, host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The priors of an elite-seeded warm start: candidate b = m * group + j takes the plan of elite j mod k of its state,
// out[b][h] = rows[elite[m][j mod k].index - offset][min(h + shift, H - 1)] (shift 1: shift_plan_kernel's rule; 0: a
// copy). One thread per V-float vector of out (V divides d: a vector never straddles two horizon points), the grid
// over all of out: a state's `group` rows spread over group * H * d / (V * 256) workgroups. An elite index outside
// the rows leaves its candidates' rows of out as they are.
template <int V>
__global__ __launch_bounds__(256) void elite_priors_kernel(const float *rows, int64_t batch, int64_t group, int H, int d,
                                                           const mpcd_best *elites, int k, int64_t offset, int shift,
                                                           float *out)
{
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const int dv = d / V, n = H * dv;  // vectors per plan
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= batch * n) return;
    const int64_t b = g / n;
    const int i = (int)(g - b * n);
    const int64_t m = b / group, j = b - m * group;
    const int64_t idx = elites[m * k + j % k].index - offset;
    if (idx < 0 || idx >= batch) return;
    const int h = i / dv, e = i - h * dv;
    const vec_t *src = reinterpret_cast<const vec_t *>(rows + (size_t)idx * H * d);
    reinterpret_cast<vec_t *>(out)[g] = src[min(h + shift, H - 1) * dv + e];
}

}  // namespace

hipError_t launch_topk(const double *cost, int64_t n_groups, int64_t group, int k, int64_t offset, mpcd_best *out,
                       hipStream_t stream, const TopkMirror *mirror)
{
    if (n_groups < 1 || n_groups > 0x7fffffff || group < 1 || k < 1 || k > MPCD_MAX_ELITES || k > group ||
        (mirror && n_groups != 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)n_groups), dim3(TK_THREADS), 0, stream, cost, group, k, offset, out,
                       mirror ? mirror->host_out : nullptr, mirror ? mirror->host_flag : nullptr,
                       mirror ? mirror->host_seq : 0u);
    return hipGetLastError();
}

hipError_t launch_topk_feasible(const double *cost, const double *viol, int64_t n_groups, int64_t group, int k, double tol,
                                int64_t offset, mpcd_best *out, double *viol_out, int64_t *n_feasible, hipStream_t stream,
                                const TopkFeasMirror *mirror)
{
    if (n_groups < 1 || n_groups > 0x7fffffff || group < 1 || k < 1 || k > MPCD_MAX_ELITES || k > group || !(tol >= 0.0) ||
        (mirror && (n_groups != 1 || !mirror->host_out || !mirror->host_viol || !mirror->host_flag)))
        return hipErrorInvalidValue;
    if (mirror)
        hipLaunchKernelGGL(topk_feasible_kernel<true>, dim3(1), dim3(TK_THREADS), 0, stream, cost, viol, group, k, tol,
                           offset, out, viol_out, n_feasible, mirror->host_out, mirror->host_viol, mirror->host_flag,
                           mirror->host_seq);
    else
        hipLaunchKernelGGL(topk_feasible_kernel<false>, dim3((unsigned)n_groups), dim3(TK_THREADS), 0, stream, cost, viol,
                           group, k, tol, offset, out, viol_out, n_feasible, (mpcd_best *)nullptr, (double *)nullptr,
                           (uint32_t *)nullptr, 0u);
    return hipGetLastError();
}

hipError_t launch_elite_priors(const float *rows, int64_t n_groups, int64_t group, int H, int d, const mpcd_best *elites,
                               int k, int64_t offset, int shift, float *out, hipStream_t stream)
{
    const int64_t batch = n_groups * group;
    const uintptr_t al = reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out);  // a caller's sub-view
    const int V = d % 4 == 0 && al % 16 == 0 ? 4 : d % 2 == 0 && al % 8 == 0 ? 2 : 1;
    const int64_t blocks = (batch * H * (d / V) + 255) / 256;
    if (n_groups < 1 || group < 1 || k < 1 || blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    if (V == 4)
        hipLaunchKernelGGL(elite_priors_kernel<4>, grid, block, 0, stream, rows, batch, group, H, d, elites, k, offset, shift,
                           out);
    else if (V == 2)
        hipLaunchKernelGGL(elite_priors_kernel<2>, grid, block, 0, stream, rows, batch, group, H, d, elites, k, offset, shift,
                           out);
    else
        hipLaunchKernelGGL(elite_priors_kernel<1>, grid, block, 0, stream, rows, batch, group, H, d, elites, k, offset, shift,
                           out);
    return hipGetLastError();
}
