// Candidate rollout + MPC cost + selection, fp64, one thread per candidate.
//
// Per candidate: u = LimitsNormalizer.unnormalize(u_norm) in fp32 (normalization.py:156-167, with
// the GLOBAL clip rule computed by clip_flag_kernel), cast exactly to fp64, then the system's
// Euler / ZOH rollout and the MPC objective in fp64 with the reference's left-to-right operation
// order (built with -ffp-contract=off, so no contraction changes a rounding).
// Coalescing: a workgroup stages its candidates' [H][n_u] rows through LDS with contiguous
// loads; each thread then walks its own row from LDS.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "../../include/mpcd.h"
#include "internal.h"

namespace {

constexpr int RT_THREADS = 64;  // candidates per workgroup (one wave: the fused argmin is a wave reduction)
static_assert(RT_THREADS == kRolloutBlock, "RolloutSelect partial count");

struct SysK {
    int32_t system, cost_kind, nx, nu;
    double params[24];
    double Q[12], R[4], P[12], xr[12];
    double x0[12];
    float umin[4], umax[4];
};

struct MinMax {
    float mn[16], mx[16];
};

// Fused selection (single-rank control step): block argmins -> the last block reduces them, writes
// *best and the winner's unnormalised [H][n_u] row. part_* hold one entry per block; counter is zero
// between launches (the last block resets it).
struct SelectK {
    mpcd_best *best;
    float *row_out;      // [H * n_u] unnormalised winner row
    double *part_cost;   // [gridDim.x]
    int64_t *part_idx;   // [gridDim.x]
    unsigned *counter;
    int64_t offset;      // global index of candidate 0
    int32_t *code_out;   // optional: flags[0] copied next to the winner (saves the caller a device copy)
    const float *clip_src;  // optional: the clip code computed here over clip_src[0, clip_n) (RolloutSelect)
    int64_t clip_n;
    char *host_out;         // optional: the result block mirrored to mapped host memory + a completion word
    uint32_t *host_flag;
    uint32_t host_seq;
};

// (v, i) beats (bv, bi): NaN = +inf, lower cost, then lower index; i < 0 = empty
__device__ __forceinline__ bool better(double v, int64_t i, double bv, int64_t bi)
{
    return i >= 0 && (bi < 0 || v < bv || (v == bv && i < bi));
}
__device__ __forceinline__ void wave_argmin(double &v, int64_t &i)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int64_t oi = __shfl_xor(i, m);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// State / input sizes per system: compile-time, so every per-candidate array lives in registers
// (a runtime n_x indexed them dynamically and put them in scratch memory).
template <int SYS> struct SysDim;
template <> struct SysDim<MPCD_SYS_CARTPOLE_LIN5> { static constexpr int NX = 5, NU = 1; };
template <> struct SysDim<MPCD_SYS_CARTPOLE_NL5> { static constexpr int NX = 5, NU = 1; };
template <> struct SysDim<MPCD_SYS_CARTPOLE_ZOH4> { static constexpr int NX = 4, NU = 1; };
template <> struct SysDim<MPCD_SYS_DOUBLE_INT2D> { static constexpr int NX = 4, NU = 2; };
template <> struct SysDim<MPCD_SYS_PENDULUM> { static constexpr int NX = 2, NU = 1; };
template <> struct SysDim<MPCD_SYS_QUADROTOR12> { static constexpr int NX = 12, NU = 4; };

template <int N>
__device__ __forceinline__ double quadform(const double *w, const double *x, const double *ref)
{
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double e = x[j] - ref[j];
        s = s + w[j] * (e * e);
    }
    return s;
}

// x_{k+1} = f(x_k, u_k). Parameter layouts are filled by mpc_via_diffusion_model_amd/systems.py.
template <int SYS>
__device__ __forceinline__ void dyn_step(const SysK &S, const double *x, const double *u, double *xn)
{
    const double *p = S.params;
    switch (SYS) {
    case MPCD_SYS_CARTPOLE_LIN5: {
        // EulerForwardCartpole_virtual, xdot_new (Cart_Diffusion_inference.py:183-197)
        // p: dt, -k*v2, (lm^2)*G*v2/il, lm*c*v2/il, v2, -l*m*k*v1/(M+m), lm*G*v1, c*v1, lm*v1/(M+m), 2/pi, pi
        double xd[5];
        xd[0] = x[1];
        xd[1] = p[1] * x[1] + p[2] * x[2] - p[3] * x[3] + p[4] * u[0];
        xd[2] = x[3];
        xd[3] = p[5] * x[1] + p[6] * x[2] - p[7] * x[3] + p[8] * u[0];
        xd[4] = -p[9] * (x[2] - p[10]) * x[3];
        for (int i = 0; i < 5; ++i) xn[i] = x[i] + xd[i] * p[0];
        break;
    }
    case MPCD_SYS_CARTPOLE_NL5: {
        // nmpc_multi_process_collect_data.py:121-137. p: dt, MPLP, MPG, M_TOTAL, M_POLE, MTG, MTLP, 2/pi, pi
        const double s = sin(x[2]), c = cos(x[2]);
        const double dd = p[3] - p[4] * c;
        double xd[5];
        xd[0] = x[1];
        xd[1] = (p[1] * -s * (x[3] * x[3]) + p[2] * s * c + u[0]) / (dd * dd);
        xd[2] = x[3];
        xd[3] = (-p[1] * s * c * (x[3] * x[3]) - p[5] * s - c * u[0]) / (p[6] - p[1] * (c * c));
        xd[4] = -p[7] * (x[2] - p[8]) * x[3];
        for (int i = 0; i < 5; ++i) xn[i] = x[i] + xd[i] * p[0];
        break;
    }
    case MPCD_SYS_CARTPOLE_ZOH4:
        // Diffusion_MPC_Inference.py:74-82. p: A_d row-major [16], B_d [4]
        for (int i = 0; i < 4; ++i)
            xn[i] = p[4 * i] * x[0] + p[4 * i + 1] * x[1] + p[4 * i + 2] * x[2] + p[4 * i + 3] * x[3] + p[16 + i] * u[0];
        break;
    case MPCD_SYS_DOUBLE_INT2D:
        // p: dt, 0.5*dt*dt
        xn[0] = x[0] + p[0] * x[2] + p[1] * u[0];
        xn[1] = x[1] + p[0] * x[3] + p[1] * u[1];
        xn[2] = x[2] + p[0] * u[0];
        xn[3] = x[3] + p[0] * u[1];
        break;
    case MPCD_SYS_PENDULUM:
        // p: dt, g/l, damping, 1/(m l^2)
        xn[0] = x[0] + p[0] * x[1];
        xn[1] = x[1] + p[0] * (-p[1] * sin(x[0]) - p[2] * x[1] + p[3] * u[0]);
        break;
    case MPCD_SYS_QUADROTOR12: {
        // p: dt, m, g, Ix, Iy, Iz
        const double sph = sin(x[3]), cph = cos(x[3]), sth = sin(x[4]), cth = cos(x[4]);
        const double sps = sin(x[5]), cps = cos(x[5]);
        const double f_m = (p[1] * p[2] + u[0]) / p[1];
        double xd[12];
        xd[0] = x[6];
        xd[1] = x[7];
        xd[2] = x[8];
        xd[3] = x[9] + (x[10] * sph + x[11] * cph) * (sth / cth);
        xd[4] = x[10] * cph - x[11] * sph;
        xd[5] = (x[10] * sph + x[11] * cph) / cth;
        xd[6] = f_m * (cph * sth * cps + sph * sps);
        xd[7] = f_m * (cph * sth * sps - sph * cps);
        xd[8] = f_m * (cph * cth) - p[2];
        xd[9] = ((p[4] - p[5]) * x[10] * x[11] + u[1]) / p[3];
        xd[10] = ((p[5] - p[3]) * x[9] * x[11] + u[2]) / p[4];
        xd[11] = ((p[3] - p[4]) * x[9] * x[10] + u[3]) / p[5];
        for (int i = 0; i < 12; ++i) xn[i] = x[i] + p[0] * xd[i];
        break;
    }
    }
}

// LimitsNormalizer's global clip test x.max() > 1+eps or x.min() < -1-eps (normalization.py:160) with
// torch's NaN semantics: a NaN makes max() and min() NaN, both comparisons false, no clip. Result code:
// 0 = in range, 1 = clip, 2 = a NaN was seen (no clip; 2 also wins a max-reduction over ranks, as a NaN
// on any rank makes the global max NaN). Consumers clip iff the flag is exactly 1.
// One launch, no memset: blocks OR bit0 (out of range) / bit1 (NaN) into ws[0]; the last block to finish
// (ws[1] counts them) moves the result to *flag and leaves ws zeroed for the next launch on the stream.
__device__ __forceinline__ unsigned clip_bits(float v, float hi, float lo)
{
    return ((v > hi) | (v < lo)) ? 1u : (v != v ? 2u : 0u);
}
__device__ __forceinline__ int clip_code(unsigned bits) { return (bits & 2u) ? 2 : (int)(bits & 1u); }

__global__ __launch_bounds__(256) void clip_flag_kernel(const float *x, int64_t n, int *flag, unsigned *ws)
{
    const float hi = (float)(1.0 + 1e-4), lo = (float)(-1.0 - 1e-4);
    unsigned any = 0;
    const int64_t n4 = ((uintptr_t)x & 15) ? 0 : n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) any |= clip_bits(v[e], hi, lo);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        any |= clip_bits(x[i], hi, lo);
    __shared__ unsigned blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    if (any) atomicOr(&blk, any);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blk) atomicOr(ws, blk);
        __threadfence();
        if (atomicAdd(ws + 1, 1u) == gridDim.x - 1) {
            __threadfence();
            *flag = clip_code(atomicExch(ws, 0u));
            atomicExch(ws + 1, 0u);
        }
    }
}

__device__ __forceinline__ float unnorm1(float v, bool clip, float mn, float mx)
{
    if (clip) v = clamp1(v);
    const float h = (v + 1.0f) / 2.0f;
    return h * (mx - mn) + mn;
}

// One component of the applied action: unnormalised in fp32, promoted to double and rounded to `decimals` places
// (the reference's round(u, 4) on the fp32 value; < 0: none)
__device__ __forceinline__ double rounded_action(float v, bool clip, float mn, float mx, int decimals)
{
    double o = (double)unnorm1(v, clip, mn, mx);
    if (decimals >= 0) {
        const double sc = pow(10.0, (double)decimals);
        o = rint(o * sc) / sc;
    }
    return o;
}

__global__ void unnormalize_kernel(const float *x, int64_t n, int dim, const int *flag, const MinMax lim, float *out)
{
    const bool clip = *flag == 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % dim);
        out[i] = unnorm1(x[i], clip, lim.mn[c], lim.mx[c]);
    }
}

// ---- What the rollout kernel and the two control tails share: a workgroup's row staging, a candidate's cost, a
// state's clip code and the cross-workgroup argmin. Each exists once, so a candidate's cost, a clip decision and a
// tie are the same bits whichever kernel computes them.

// nvalid candidates' contiguous [row] floats at src -> su[c][row + 1]
__device__ __forceinline__ void stage_rows(const float *src, int64_t nvalid, int row, float *su)
{
    const int stride = row + 1;
    if ((row & 3) == 0) {  // 16-byte loads (a row never straddles a quad)
        // in batches of UNR loads per lane, all issued before the first LDS store: one memory latency per batch
        // (a load -> store loop waits for every load in turn: 16 latencies at H = 32, nu = 2)
        constexpr int UNR = 8;
        const int nq = (int)(nvalid * row / 4);
        for (int base = 0; base < nq; base += UNR * RT_THREADS) {
            f32x4 v[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int i = base + u * RT_THREADS + (int)threadIdx.x;
                v[u] = i < nq ? ldg4(src + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int i = base + u * RT_THREADS + (int)threadIdx.x;
                if (i < nq) {
                    const int c = 4 * i / row, k = 4 * i - c * row;
#pragma unroll
                    for (int e = 0; e < 4; ++e) su[c * stride + k + e] = v[u][e];
                }
            }
        }
    } else {
        for (int i = threadIdx.x; i < nvalid * row; i += RT_THREADS) {
            const int c = i / row, k = i - c * row;
            su[c * stride + k] = src[i];
        }
    }
}

// The MPC cost of the normalised plan ur[H][nu] from the state x (overwritten), both cost kinds. The fp64 operations
// and their order are the contract with the C oracle (-ffp-contract=off: no contraction changes a rounding).
// visit(xn, u) sees every state dyn_step produces, right after the step, with the input that produced it (canonical:
// (x_1, u_0) .. (x_H, u_{H-1}); calMPCCost: (x_1, u_0) .. (x_{H-2}, u_{H-3}), its loop applies u_0 .. u_{H-3}); the
// default sees nothing and compiles to nothing.
struct NoVisit {
    __device__ __forceinline__ void operator()(const double *, const double *) const {}
};
template <int SYS, class Visit = NoVisit>
__device__ __forceinline__ double candidate_cost(const SysK &S, const float *ur, bool clip, double *x, int H,
                                                 Visit visit = Visit{})
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    float mn[nu], mx[nu];
#pragma unroll
    for (int i = 0; i < nu; ++i) { mn[i] = S.umin[i]; mx[i] = S.umax[i]; }
    double xn[nx], u[nu];
    double J;
    if (S.cost_kind == MPCD_COST_CALMPC) {
        // calMPCCost (Cart_Diffusion_inference.py:247-283); num_u = 1 (batch axis of u_hor)
        J = 0.0;
        for (int i = 0; i < nx; ++i) J = J + S.Q[i] * (x[i] * x[i]);
        u[0] = (double)unnorm1(ur[0], clip, mn[0], mx[0]);
        J = J + S.R[0] * (u[0] * u[0]);
        for (int i = 0; i < nx; ++i) xn[i] = x[i];
        double ucur = u[0];
        for (int i = 1; i < H - 1; ++i) {
            dyn_step<SYS>(S, x, &ucur, xn);
            visit(xn, &ucur);
            const double un = (double)unnorm1(ur[i * nu], clip, mn[0], mx[0]);
            for (int j = 1; j < nx; ++j) J = J + S.Q[j] * (xn[j] * xn[j]);
            J = J + S.R[0] * (un * un);
            ucur = un;
            for (int j = 0; j < nx; ++j) x[j] = xn[j];
        }
        for (int i = 0; i < nx; ++i) J = J + S.P[i] * (xn[i] * xn[i]);
    } else {
        const double zero[4] = {0.0, 0.0, 0.0, 0.0};
        J = quadform<nx>(S.Q, x, S.xr);
        for (int k = 0; k < H; ++k) {
            for (int i = 0; i < nu; ++i) u[i] = (double)unnorm1(ur[k * nu + i], clip, mn[i], mx[i]);
            dyn_step<SYS>(S, x, u, xn);
            visit(xn, u);
            const double sx = k < H - 1 ? quadform<nx>(S.Q, xn, S.xr) : quadform<nx>(S.P, xn, S.xr);
            const double sv = quadform<nu>(S.R, u, zero);
            J = J + (sx + sv);
            for (int j = 0; j < nx; ++j) x[j] = xn[j];
        }
    }
    return J;
}

// clip_flag_kernel's test over cs[0, n) by one wave (a one-wave workgroup): the clip code of a state's slice, or of
// the whole batch
__device__ __forceinline__ int state_clip_code(const float *cs, int64_t n)
{
    const float hi = (float)(1.0 + 1e-4), lo = (float)(-1.0 - 1e-4);
    unsigned any = 0;
    const int64_t n4 = ((uintptr_t)cs & 15) ? 0 : n >> 2;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < n4; i += RT_THREADS) {  // unrolled: eight loads in flight per lane
        const f32x4 v = ldg4(cs + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) any |= clip_bits(v[e], hi, lo);
    }
    for (int64_t i = 4 * n4 + threadIdx.x; i < n; i += RT_THREADS) any |= clip_bits(cs[i], hi, lo);
    __shared__ unsigned blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    if (any) atomicOr(&blk, any);
    __syncthreads();
    return clip_code(blk);
}

// The cross-workgroup hand-off, of which there is one copy: each of `nslots` one-wave workgroups leaves its partial
// result in memory and counts itself on *counter; the last one to arrive reads them all. Lane 0 runs store0() (its
// stores), fences and counts the workgroup; the last workgroup fences, runs reload() on every lane and puts the counter
// back: *counter is zero between launches. Returns whether this workgroup is that last one.
// Why it is sound: lane 0 stores the partials, __threadfence() makes them visible device-wide, and only then does its
// atomicAdd count the workgroup. The workgroup whose add returns nslots - 1 therefore follows every other workgroup's
// stores and fence; its own __threadfence() and non-temporal reloads (which take no stale line of this CU's cache)
// then read all nslots partials as written. What the other lanes of a wave stored before the call (the elite tail's
// ranked list) is covered the same way once they have fenced too: the wave's stores and fences precede lane 0's
// atomicAdd in program order. The same order covers what a caller's partial depends on: a partial is computed from
// the state the workgroup read (the tails' x_dev[m]), so every workgroup has finished reading it before it counts
// itself, and the last workgroup may overwrite it (the closed loop's plant step).
template <class Store0, class Reload>
__device__ __forceinline__ bool last_arriver(unsigned *counter, int nslots, Store0 store0, Reload reload)
{
    __shared__ bool last;
    if (threadIdx.x == 0) {
        store0();
        __threadfence();
        last = atomicAdd(counter, 1u) == (unsigned)nslots - 1;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    reload();
    if (threadIdx.x == 0) *counter = 0u;
    return true;
}
// Cross-workgroup argmin on that hand-off: workgroup `slot` leaves its partial (v, i) - and raw, where part_raw is not
// null - in part_*[slot]; the last one reduces the nslots partials: (v, i) is then the winner in every lane (i < 0: no
// entrant).
__device__ __forceinline__ bool last_arriver_argmin(double *part_cost, int64_t *part_idx, double *part_raw,
                                                    unsigned *counter, int slot, int nslots, double &v, int64_t &i,
                                                    double raw)
{
    return last_arriver(
        counter, nslots,
        [&] {
            part_cost[slot] = v;
            part_idx[slot] = i;
            if (part_raw) part_raw[slot] = raw;
        },
        [&] {
            v = INFINITY;
            i = -1;
            for (int k = threadIdx.x; k < nslots; k += RT_THREADS) {
                const double pv = __builtin_nontemporal_load(part_cost + k);
                const int64_t pi = __builtin_nontemporal_load(part_idx + k);
                if (better(pv, pi, v, i)) { v = pv; i = pi; }
            }
            wave_argmin(v, i);
        });
}

// ---- Ranked lists (the elite tail). A list is k mpcd_best entries, best first in better()'s order, empty entries
// (index -1, cost +inf) last. (v, i) comes strictly after the last pick (pv, pi) in that order (elite.hip's tk_after); pi < 0:
// nothing picked yet
__device__ __forceinline__ bool after(double v, int64_t i, double pv, int64_t pi)
{
    return pi < 0 || v > pv || (v == pv && i > pi);
}
__device__ __forceinline__ void load_entry(const mpcd_best *e, double &v, int64_t &i)
{
    v = __builtin_nontemporal_load(&e->cost);
    i = __builtin_nontemporal_load(&e->index);
}
// The best entry after the pick (pv, pi) over this lane's lists lane, lane + 64, ... of nlists sorted lists: in each,
// the first entry after the pick. Stateless (topk_kernel's rule): no per-list position is kept, so a lane may own any
// number of lists without an array in registers.
__device__ __forceinline__ void lane_best_after(const mpcd_best *lists, int nlists, int k, double pv, int64_t pi,
                                                double &lv, int64_t &li)
{
    lv = INFINITY;
    li = -1;
    for (int w = threadIdx.x; w < nlists; w += RT_THREADS) {
        const mpcd_best *L = lists + (size_t)w * k;
        for (int e = 0; e < k; ++e) {
            double ev;
            int64_t ei;
            load_entry(L + e, ev, ei);
            if (ei < 0) break;
            if (after(ev, ei, pv, pi)) {
                if (better(ev, ei, lv, li)) { lv = ev; li = ei; }
                break;
            }
        }
    }
}
// The k best of nlists sorted lists by one wave: k rounds of wave argmin over each lane's best remaining entry; only
// the pick's owner moves on. Up to 64 lists: one per lane, its position h in a register; more: lane_best_after.
// Lane r < k leaves with entry r in (mv, mi).
__device__ __forceinline__ void merge_lists(const mpcd_best *lists, int nlists, int k, double &mv, int64_t &mi)
{
    const bool one = nlists <= RT_THREADS;
    double lv = INFINITY;
    int64_t li = -1;
    int h = 0;
    if (!one)
        lane_best_after(lists, nlists, k, -INFINITY, -1, lv, li);
    else if ((int)threadIdx.x < nlists)
        load_entry(lists + (size_t)threadIdx.x * k, lv, li);
    mv = INFINITY;
    mi = -1;
    for (int r = 0; r < k; ++r) {
        double wv = lv;
        int64_t wi = li;
        wave_argmin(wv, wi);
        if ((int)threadIdx.x == r) { mv = wv; mi = wi; }
        if (wi >= 0 && li == wi) {
            if (!one) {
                lane_best_after(lists, nlists, k, wv, wi, lv, li);
            } else if (++h < k) {
                load_entry(lists + (size_t)threadIdx.x * k + h, lv, li);
            } else {
                lv = INFINITY;
                li = -1;
            }
        }
    }
}

// ---- The same ranked lists in the feasibility-first order (mpcd.h "State constraints"; elite.hip's tf_*), for the box
// tail. An entry is (V, cost, index), V its violation as computed (NaN = +inf already); the order is lexicographic on
// (g, cost, index) with g = V <= tol ? 0 : V recomputed wherever keys are compared, so a pick carries its V. A list is
// k mpcd_best entries and, parallel to it, k violations.
__device__ __forceinline__ double box_key(double V, double tol) { return V <= tol ? 0.0 : V; }
__device__ __forceinline__ bool better3(double g, double v, int64_t i, double bg, double bv, int64_t bi)
{
    return i >= 0 && (bi < 0 || g < bg || (g == bg && (v < bv || (v == bv && i < bi))));
}
__device__ __forceinline__ bool after3(double g, double v, int64_t i, double pg, double pv, int64_t pi)
{
    return pi < 0 || g > pg || (g == pg && (v > pv || (v == pv && i > pi)));
}
__device__ __forceinline__ void wave_argmin3(double &V, double &v, int64_t &i, double tol)
{
    double g = box_key(V, tol);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oV = __shfl_xor(V, m);
        const double ov = __shfl_xor(v, m);
        const int64_t oi = __shfl_xor(i, m);
        const double og = box_key(oV, tol);
        if (better3(og, ov, oi, g, v, i)) { V = oV; g = og; v = ov; i = oi; }
    }
}
__device__ __forceinline__ void load_entry3(const mpcd_best *e, const double *eV, double &V, double &v, int64_t &i)
{
    load_entry(e, v, i);
    V = __builtin_nontemporal_load(eV);
}
// lane_best_after on the three keys: the pick is (pV, pv, pi), pi < 0: nothing picked yet
__device__ __forceinline__ void lane_best_after3(const mpcd_best *lists, const double *viols, int nlists, int k, double tol,
                                                 double pV, double pv, int64_t pi, double &lV, double &lv, int64_t &li)
{
    const double pg = box_key(pV, tol);
    double lg = INFINITY;
    lV = INFINITY;
    lv = INFINITY;
    li = -1;
    for (int w = threadIdx.x; w < nlists; w += RT_THREADS) {
        const mpcd_best *L = lists + (size_t)w * k;
        const double *LV = viols + (size_t)w * k;
        for (int e = 0; e < k; ++e) {
            double eV, ev;
            int64_t ei;
            load_entry3(L + e, LV + e, eV, ev, ei);
            if (ei < 0) break;
            const double eg = box_key(eV, tol);
            if (after3(eg, ev, ei, pg, pv, pi)) {
                if (better3(eg, ev, ei, lg, lv, li)) { lV = eV; lg = eg; lv = ev; li = ei; }
                break;
            }
        }
    }
}
// merge_lists on the three keys: lane r < k leaves with entry r in (mV, mv, mi)
__device__ __forceinline__ void merge_lists3(const mpcd_best *lists, const double *viols, int nlists, int k, double tol,
                                             double &mV, double &mv, int64_t &mi)
{
    const bool one = nlists <= RT_THREADS;
    double lV = INFINITY, lv = INFINITY;
    int64_t li = -1;
    int h = 0;
    if (!one)
        lane_best_after3(lists, viols, nlists, k, tol, 0.0, -INFINITY, -1, lV, lv, li);
    else if ((int)threadIdx.x < nlists)
        load_entry3(lists + (size_t)threadIdx.x * k, viols + (size_t)threadIdx.x * k, lV, lv, li);
    mV = INFINITY;
    mv = INFINITY;
    mi = -1;
    for (int r = 0; r < k; ++r) {
        double wV = lV, wv = lv;
        int64_t wi = li;
        wave_argmin3(wV, wv, wi, tol);
        if ((int)threadIdx.x == r) { mV = wV; mv = wv; mi = wi; }
        if (wi >= 0 && li == wi) {
            if (!one) {
                lane_best_after3(lists, viols, nlists, k, tol, wV, wv, wi, lV, lv, li);
            } else if (++h < k) {
                load_entry3(lists + (size_t)threadIdx.x * k + h, viols + (size_t)threadIdx.x * k + h, lV, lv, li);
            } else {
                lV = INFINITY;
                lv = INFINITY;
                li = -1;
            }
        }
    }
}

// x0_dev == nullptr: every candidate starts from S.x0; else candidate b starts from x0_dev[b / group]
// (closed loop: one plant state per group of candidates). flags[b / group] is that group's clip flag
// (group = batch for the single-state case: one global flag).
// SEL: also select (SelectK above) - one launch for rollout, cost, argmin and the winner's row.
template <int SYS, bool SEL>
__global__ __launch_bounds__(RT_THREADS) void rollout_cost_kernel(const SysK S, const float *u_norm, const int *flags,
                                                                  const double *x0_dev, int64_t group, int64_t batch,
                                                                  int H, double *cost, const SelectK K)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int row = H * nu, stride = row + 1;
    const int64_t c0 = (int64_t)blockIdx.x * RT_THREADS;
    stage_rows(u_norm + (size_t)c0 * row, min((int64_t)RT_THREADS, batch - c0), row, su);
    int code = 0;  // SEL with clip_src: the clip code, recomputed by every workgroup
    if constexpr (SEL) {
        if (K.clip_src) code = state_clip_code(K.clip_src, K.clip_n);
    }
    __syncthreads();
    const int64_t b = min(c0 + threadIdx.x, batch - 1);  // lanes past the batch recompute the last one
    const bool clip = (SEL && K.clip_src) ? code == 1 : flags[b / group] == 1;
    double x[nx];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = x0_dev ? x0_dev[(b / group) * nx + i] : S.x0[i];
    const double J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H);
    if (c0 + threadIdx.x < batch) cost[b] = J;
    if constexpr (SEL) {
        double v = isnan(J) ? INFINITY : J;
        int64_t i = c0 + threadIdx.x < batch ? b : -1;
        wave_argmin(v, i);  // RT_THREADS == one wave
        if (!last_arriver_argmin(K.part_cost, K.part_idx, nullptr, K.counter, (int)blockIdx.x, (int)gridDim.x, v, i, 0.0))
            return;
        const int32_t ccode = K.clip_src ? code : flags[0];
        float *hrow = K.host_out ? reinterpret_cast<float *>(K.host_out + sizeof(mpcd_best)) : nullptr;
        if (threadIdx.x == 0) {
            const mpcd_best bst{v, i < 0 ? -1 : K.offset + i};
            *K.best = bst;
            if (K.code_out) *K.code_out = ccode;
            if (hrow) {
                *reinterpret_cast<mpcd_best *>(K.host_out) = bst;
                *reinterpret_cast<int32_t *>(hrow + row) = ccode;
            }
        }
        if (i >= 0 && K.row_out) {
            const bool clip0 = K.clip_src ? code == 1 : flags[0] == 1;
            for (int k = threadIdx.x; k < row; k += RT_THREADS) {
                const float o = unnorm1(u_norm[(size_t)i * row + k], clip0, S.umin[k % nu], S.umax[k % nu]);
                K.row_out[k] = o;
                if (hrow) hrow[k] = o;
            }
        }
        if (hrow) {  // every lane's host stores ordered before the completion word
            __threadfence_system();
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_store(K.host_flag, K.host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- State constraints (mpcd.h "State constraints"): mpcd_rollout_cost_grouped that also reports each candidate's
// violation of a state box, V = max(0, max over the visited states and i < n_x of max(lo[i] - x[i], x[i] - hi[i])); an
// excess with a NaN difference (a NaN state, inf - inf) makes V = +inf. A maximum has no order, so V is reproducible
// bit for bit where the states are. The box is a kernel argument of its own (scalar registers); the bounds loop is
// over the compile-time NX, so nothing is indexed dynamically.
struct BoxK {
    double lo[12], hi[12];
};
// fmax drops a NaN operand, so the NaN excesses are collected apart (one unordered compare per component) and
// finish() turns any into +inf: five fp64 instructions per component and step.
template <int NX>
struct BoxVisit {
    const BoxK &box;
    double &V;   // starts at 0.0
    bool &bad;   // an excess was NaN
    __device__ __forceinline__ void operator()(const double *xn, const double *) const
    {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const double a = box.lo[i] - xn[i], b = xn[i] - box.hi[i];
            bad |= __builtin_isunordered(a, b);
            V = fmax(V, fmax(a, b));
        }
    }
    __device__ __forceinline__ static double finish(double V, bool bad) { return bad ? (double)INFINITY : V + 0.0; }
};
// rollout_cost_kernel<SYS, false> of a grouped call (candidate b starts from x0_dev[b / group]) with the visitor: the
// cost is the same candidate_cost, hence the same bits.
template <int SYS>
__global__ __launch_bounds__(RT_THREADS) void rollout_cost_box_kernel(const SysK S, const BoxK box, const float *u_norm,
                                                                      const int *flags, const double *x0_dev,
                                                                      int64_t group, int64_t batch, int H, double *cost,
                                                                      double *viol)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int row = H * nu, stride = row + 1;
    const int64_t c0 = (int64_t)blockIdx.x * RT_THREADS;
    stage_rows(u_norm + (size_t)c0 * row, min((int64_t)RT_THREADS, batch - c0), row, su);
    __syncthreads();
    const int64_t b = min(c0 + threadIdx.x, batch - 1);  // lanes past the batch recompute the last one
    const bool clip = flags[b / group] == 1;
    double x[nx];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = x0_dev[(b / group) * nx + i];
    double V = 0.0;
    bool bad = false;
    const double J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H, BoxVisit<nx>{box, V, bad});
    if (c0 + threadIdx.x < batch) {
        cost[b] = J;
        viol[b] = BoxVisit<nx>::finish(V, bad);
    }
}

// ---- Constraint set (mpcd.h "Constraint set"): the box, n_rows linear rows over (x_{k+1}, u_k) and per-input rate
// bounds. A kernel argument of its own, like BoxK (about 1.3 KiB; with SysK well under the 4 KiB limit). The row loop
// runs to the run-time, wave-uniform n_rows and reads its coefficients with scalar loads; the component loops are over
// the compile-time NX / NU, so nothing per-lane is indexed dynamically.
struct ConK {
    BoxK box;
    double A[MPCD_MAX_CON_ROWS][12], C[MPCD_MAX_CON_ROWS][4], b[MPCD_MAX_CON_ROWS];
    double du[4];
    int32_t n_rows, pad;
};
// BoxVisit with the rows and the rate test. up holds the previous input once has is set: the caller's u_prev before
// the first visit (has = it is a real one), then every visited u. A row's sum is taken in the contract's order, A's
// terms then C's, each product rounded on its own. NaN excesses are collected as in BoxVisit.
template <int NX, int NU>
struct ConstrVisit {
    const ConK &con;
    double &V;          // starts at 0.0
    bool &bad;          // an excess was NaN
    double (&up)[NU];
    bool &has;
    __device__ __forceinline__ void operator()(const double *xn, const double *u) const
    {
        BoxVisit<NX>{con.box, V, bad}(xn, u);
        for (int r = 0; r < con.n_rows; ++r) {
            double s = con.A[r][0] * xn[0];
#pragma unroll
            for (int i = 1; i < NX; ++i) s = s + con.A[r][i] * xn[i];
#pragma unroll
            for (int j = 0; j < NU; ++j) s = s + con.C[r][j] * u[j];
            const double e = s - con.b[r];
            bad |= e != e;
            V = fmax(V, e);
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const double e = has ? fabs(u[j] - up[j]) - con.du[j] : 0.0;
            bad |= e != e;
            V = fmax(V, e);
            up[j] = u[j];
        }
        has = true;
    }
    // the previous applied action of plant state m, or none: u_prev null, or a NaN in any entry of the row
    __device__ __forceinline__ static bool load_prev(const double *u_prev, int64_t m, double (&up)[NU])
    {
        bool has = u_prev != nullptr;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            up[j] = u_prev ? u_prev[m * NU + j] : 0.0;
            has = has && up[j] == up[j];
        }
        return has;
    }
};
// rollout_cost_box_kernel with the set (mpcd_rollout_cost_constr): the same cost, hence the same bits
template <int SYS>
__global__ __launch_bounds__(RT_THREADS) void rollout_cost_constr_kernel(const SysK S, const ConK con, const float *u_norm,
                                                                         const int *flags, const double *x0_dev,
                                                                         const double *u_prev, int64_t group,
                                                                         int64_t batch, int H, double *cost, double *viol)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int row = H * nu, stride = row + 1;
    const int64_t c0 = (int64_t)blockIdx.x * RT_THREADS;
    stage_rows(u_norm + (size_t)c0 * row, min((int64_t)RT_THREADS, batch - c0), row, su);
    __syncthreads();
    const int64_t b = min(c0 + threadIdx.x, batch - 1);  // lanes past the batch recompute the last one
    const bool clip = flags[b / group] == 1;
    double x[nx], up[nu];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = x0_dev[(b / group) * nx + i];
    bool has = ConstrVisit<nx, nu>::load_prev(u_prev, b / group, up);
    double V = 0.0;
    bool bad = false;
    const double J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H, ConstrVisit<nx, nu>{con, V, bad, up, has});
    if (c0 + threadIdx.x < batch) {
        cost[b] = J;
        viol[b] = BoxVisit<nx>::finish(V, bad);
    }
}

// ---- The constraint set in the one-call control step (mpcd_mpc_step_constr): rollout_cost_kernel<SYS, SEL> with
// ConstrVisit riding candidate_cost and the selection in the feasibility-first order. The one start state stays in
// SysK; the set, the tolerance and the previous applied action (with its "has a predecessor" bit, decided on the host
// by load_prev's rule) are a kernel argument of their own, so the step uploads nothing. cost[b] and viol[b] are the
// bits rollout_cost_constr_kernel writes for group = batch: the same candidate_cost, the same visitor, the same finish.
// SEL = false ends there (the multi-rank producer). SEL = true: wave_argmin3 over the workgroup's real lanes, its
// feasible count by ballot and popcount, the hand-off through last_arriver with partials (V, cost, index, count); the
// last workgroup reduces them in a strided loop (there may be more partials than lanes), sums the counts and writes
// {best, winner row unnormalised, clip code, V, n_feasible} to the device block and to mapped host memory, then the
// completion word (rollout_cost_kernel's system-scope fence protocol): entry 0, its V and the count of
// topk_feasible_kernel(k = 1) over the two arrays. A kernel of its own and not a shared __device__ body with
// rollout_cost_kernel, for the reason given at batch_step_box_tail_kernel.
struct ConStepK {
    ConK con;
    double tol;
    double u_prev[4];
    int32_t has_prev, pad;
};
// The selection's addresses, few on purpose (scalar registers are what this kernel runs out of): the device result block
// and its mapped host mirror share one layout, {mpcd_best, winner row [H * n_u] fp32, clip code int32, padding to 8
// bytes, V double, n_feasible int64} (step_constr_viol_off), and the four partial arrays are one block of 4 * gridDim.x
// 8-byte entries: V, cost, index, count.
struct ConSelectK {
    char *block;          // the device result block
    double *part;         // [4][gridDim.x]
    unsigned *counter;
    int64_t offset;       // global index of candidate 0
    const float *clip_src;  // optional: the clip code computed here over clip_src[0, clip_n)
    int64_t clip_n;
    char *host_out;       // optional: the block mirrored to mapped host memory + a completion word
    uint32_t *host_flag;
    uint32_t host_seq;
};
template <int SYS, bool SEL>
__global__ __launch_bounds__(RT_THREADS) void rollout_constr_select_kernel(const SysK S, const ConStepK C,
                                                                           const float *u_norm, const int *flags,
                                                                           int64_t batch, int H, double *cost,
                                                                           double *viol, const ConSelectK K)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int row = H * nu, stride = row + 1;
    const int64_t c0 = (int64_t)blockIdx.x * RT_THREADS;
    stage_rows(u_norm + (size_t)c0 * row, min((int64_t)RT_THREADS, batch - c0), row, su);
    int code = 0;  // SEL with clip_src: the clip code, recomputed by every workgroup
    if constexpr (SEL) {
        if (K.clip_src) code = state_clip_code(K.clip_src, K.clip_n);
    }
    __syncthreads();
    const int64_t b = min(c0 + threadIdx.x, batch - 1);  // lanes past the batch recompute the last one
    const bool clip = (SEL && K.clip_src) ? code == 1 : flags[0] == 1;
    double x[nx], up[nu];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = S.x0[i];
#pragma unroll
    for (int j = 0; j < nu; ++j) up[j] = C.u_prev[j];
    bool has = C.has_prev != 0;
    double Vacc = 0.0;
    bool bad = false;
    const double J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H, ConstrVisit<nx, nu>{C.con, Vacc, bad, up, has});
    const double V = BoxVisit<nx>::finish(Vacc, bad);  // never NaN: a NaN excess is +inf
    const bool real = c0 + threadIdx.x < batch;
    if (real) {
        cost[b] = J;
        viol[b] = V;
    }
    if constexpr (SEL) {
        const double tol = C.tol;
        double wV = V, wv = isnan(J) ? INFINITY : J;
        int64_t wi = real ? b : -1;  // lanes past the batch are never entrants
        int64_t nf = __popcll(__ballot(real && V <= tol));
        wave_argmin3(wV, wv, wi, tol);  // RT_THREADS == one wave; every lane holds the result
        const int slot = (int)blockIdx.x, nslots = (int)gridDim.x;
        double *part_viol = K.part, *part_cost = part_viol + nslots;
        int64_t *part_idx = reinterpret_cast<int64_t *>(part_cost + nslots), *part_nfeas = part_idx + nslots;
        if (!last_arriver(
                K.counter, nslots,
                [&] {
                    part_viol[slot] = wV;
                    part_cost[slot] = wv;
                    part_idx[slot] = wi;
                    part_nfeas[slot] = nf;
                },
                [&] {
                    double lV = INFINITY, lg = INFINITY, lv = INFINITY;
                    int64_t li = -1, s = 0;
                    for (int k = threadIdx.x; k < nslots; k += RT_THREADS) {
                        const double pV = __builtin_nontemporal_load(part_viol + k);
                        const double pv = __builtin_nontemporal_load(part_cost + k);
                        const int64_t pi = __builtin_nontemporal_load(part_idx + k);
                        const double pg = box_key(pV, tol);
                        if (better3(pg, pv, pi, lg, lv, li)) { lV = pV; lg = pg; lv = pv; li = pi; }
                        s += __builtin_nontemporal_load(part_nfeas + k);
                    }
                    wV = lV;
                    wv = lv;
                    wi = li;
                    wave_argmin3(wV, wv, wi, tol);
#pragma unroll
                    for (int q = 32; q >= 1; q >>= 1) s += __shfl_xor(s, q);
                    nf = s;
                }))
            return;
        const int32_t ccode = K.clip_src ? code : flags[0];
        const size_t viol_off = step_constr_viol_off(row);
        float *drow = reinterpret_cast<float *>(K.block + sizeof(mpcd_best));
        float *hrow = K.host_out ? reinterpret_cast<float *>(K.host_out + sizeof(mpcd_best)) : nullptr;
        if (threadIdx.x == 0) {
            const mpcd_best bst{wv, wi < 0 ? -1 : K.offset + wi};
            *reinterpret_cast<mpcd_best *>(K.block) = bst;
            *reinterpret_cast<int32_t *>(drow + row) = ccode;
            *reinterpret_cast<double *>(K.block + viol_off) = wV;
            *reinterpret_cast<int64_t *>(K.block + viol_off + sizeof(double)) = nf;
            if (hrow) {
                *reinterpret_cast<mpcd_best *>(K.host_out) = bst;
                *reinterpret_cast<int32_t *>(hrow + row) = ccode;
                *reinterpret_cast<double *>(K.host_out + viol_off) = wV;
                *reinterpret_cast<int64_t *>(K.host_out + viol_off + sizeof(double)) = nf;
            }
        }
        if (wi >= 0) {
            const bool clip0 = ccode == 1;
            for (int k = threadIdx.x; k < row; k += RT_THREADS) {
                const float o = unnorm1(u_norm[(size_t)wi * row + k], clip0, S.umin[k % nu], S.umax[k % nu]);
                drow[k] = o;
                if (hrow) hrow[k] = o;
            }
        }
        if (hrow) {  // every lane's host stores ordered before the completion word
            __threadfence_system();
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_store(K.host_flag, K.host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Per-group clip flags: flags[g] = the clip code above over x[g*group_elems, (g+1)*group_elems)
// (LimitsNormalizer's rule applied to each plant state's own candidate batch). One workgroup per group:
// every flag is written, so no memset is needed.
__global__ __launch_bounds__(256) void clip_flags_kernel(const float *x, int64_t group_elems, int *flags)
{
    const float hi = (float)(1.0 + 1e-4), lo = (float)(-1.0 - 1e-4);
    const float *g = x + (size_t)blockIdx.x * group_elems;
    unsigned any = 0;
    for (int64_t i = threadIdx.x; i < group_elems; i += blockDim.x) any |= clip_bits(g[i], hi, lo);
    __shared__ unsigned blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    if (any) atomicOr(&blk, any);
    __syncthreads();
    if (threadIdx.x == 0) flags[blockIdx.x] = clip_code(blk);
}

// normalize_condition for a batch of plant states (normalization.py:149-154 in fp64, then the net's
// .float()): ctx[m][c] = fp32(2 * ((x[m][c] - min[c]) / den[c]) - 1), den = fp32(max - min).
struct NormK {
    double mn[16], den[16];
};
__global__ void normalize_states_kernel(const double *x, int64_t M, int C, const NormK nk, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * C) return;
    const int c = (int)(i % C);
    out[i] = (float)(2.0 * ((x[i] - nk.mn[c]) / nk.den[c]) - 1.0);
}

// One closed-loop control step per plant state m (one workgroup each): the candidate of its group
// [m*group, (m+1)*group) with the lowest cost (NaN = +inf, lowest index on ties; or the group's first
// candidate, the reference scripts' n_samples = 1 convention), its u[0] unnormalised with the
// group's clip flag and rounded to `decimals` places (the reference's round(u, 4) on the fp32 value
// promoted to double; < 0: none), then the plant step x[m] <- f(x[m], u0) in fp64.
constexpr int CS_THREADS = 256;
template <int SYS>
__global__ __launch_bounds__(CS_THREADS) void control_step_kernel(const SysK S, double *x_dev, int64_t group,
                                                                  const float *u_norm, int H, const double *cost,
                                                                  const int *flags, int select_first, int decimals,
                                                                  double *u_applied, int64_t *best_idx, double *best_cost)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    __shared__ double sv[CS_THREADS];
    __shared__ int64_t si[CS_THREADS];
    const int64_t m = blockIdx.x, base = m * group;
    double bv = INFINITY;
    int64_t bi = -1;
    if (select_first) {
        if (threadIdx.x == 0) {
            bi = base;
            bv = cost[base];
        }
    } else {
        for (int64_t i = threadIdx.x; i < group; i += CS_THREADS) {
            double v = cost[base + i];
            if (isnan(v)) v = INFINITY;
            if (bi < 0 || v < bv) {
                bv = v;
                bi = base + i;
            }
        }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int w = CS_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double ov = sv[threadIdx.x + w];
            const int64_t oi = si[threadIdx.x + w];
            const double mv = sv[threadIdx.x];
            const int64_t mi = si[threadIdx.x];
            if (oi >= 0 && (mi < 0 || ov < mv || (ov == mv && oi < mi))) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const int64_t idx = si[0];
    const bool clip = flags[m] == 1;
    double x[nx], xn[nx], u[nu];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = x_dev[m * nx + i];
#pragma unroll
    for (int i = 0; i < nu; ++i)
        u[i] = rounded_action(u_norm[(size_t)idx * H * nu + i], clip, S.umin[i], S.umax[i], decimals);
    dyn_step<SYS>(S, x, u, xn);
#pragma unroll
    for (int i = 0; i < nx; ++i) x_dev[m * nx + i] = xn[i];
#pragma unroll
    for (int i = 0; i < nu; ++i) u_applied[m * nu + i] = u[i];
    best_idx[m] = idx;
    best_cost[m] = cost[idx];
}

// control_step_kernel with the selection supplied (mpcd_control_step_picked): one thread per plant state m applies
// candidate picks[m * pick_stride].index - offset: its u0 unnormalised with flags[m] and rounded, the plant step in
// place, best_idx = the pick's index as given, best_cost = the pick's cost. A pick outside [0, batch) reads nothing
// through it: x_dev[m] stays, u_applied[m] = NaN, best_idx[m] = -1, best_cost[m] = +inf. Every lane computes a step
// (an invalid one on row 0, a lane past n_states on the last state) and only the stores are conditional: the fp64 pow
// and the dynamics inside a divergent branch cost the quadrotor tail a private segment.
constexpr int CP_THREADS = 64;
template <int SYS>
__global__ __launch_bounds__(CP_THREADS) void control_step_picked_kernel(const SysK S, double *x_dev, int64_t n_states,
                                                                         const float *u_norm, int64_t batch, int H,
                                                                         const mpcd_best *picks, int64_t pick_stride,
                                                                         int64_t offset, const int *flags, int decimals,
                                                                         double *u_applied, int64_t *best_idx,
                                                                         double *best_cost)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    const int64_t t = (int64_t)blockIdx.x * CP_THREADS + threadIdx.x;
    const bool live = t < n_states;
    const int64_t m = live ? t : n_states - 1;
    const mpcd_best pick = picks[m * pick_stride];
    const int64_t idx = (int64_t)((uint64_t)pick.index - (uint64_t)offset);
    const bool ok = idx >= 0 && idx < batch;
    const int64_t r = ok ? idx : 0;
    const bool clip = flags[m] == 1;
    double x[nx], xn[nx], u[nu];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = x_dev[m * nx + i];
#pragma unroll
    for (int i = 0; i < nu; ++i)
        u[i] = rounded_action(u_norm[(size_t)r * H * nu + i], clip, S.umin[i], S.umax[i], decimals);
    dyn_step<SYS>(S, x, u, xn);
    if (!live) return;
    if (ok) {
#pragma unroll
        for (int i = 0; i < nx; ++i) x_dev[m * nx + i] = xn[i];
    }
#pragma unroll
    for (int i = 0; i < nu; ++i) u_applied[m * nu + i] = ok ? u[i] : (double)NAN;
    best_idx[m] = ok ? pick.index : -1;
    best_cost[m] = ok ? pick.cost : (double)INFINITY;
}

// Single-workgroup argmin: NaN -> +inf; ties -> lowest index.
__global__ __launch_bounds__(1024) void argmin_kernel(const double *cost, int64_t n, int64_t offset, mpcd_best *best)
{
    __shared__ double sv[1024];
    __shared__ int64_t si[1024];
    double bv = INFINITY;
    int64_t bi = -1;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        double v = cost[i];
        if (isnan(v)) v = INFINITY;
        if (bi < 0 || v < bv) { bv = v; bi = i; }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double ov = sv[threadIdx.x + w];
            const int64_t oi = si[threadIdx.x + w];
            const double mv = sv[threadIdx.x];
            const int64_t mi = si[threadIdx.x];
            const bool take = oi >= 0 && (mi < 0 || ov < mv || (ov == mv && oi < mi));
            if (take) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        best->cost = sv[0];
        best->index = si[0] < 0 ? -1 : offset + si[0];
    }
}

// The selection exchange without a host round trip: every rank writes the winner's row if it owns
// it and zeros otherwise; a sum all-reduce then hands every rank the winner's row exactly (x + 0 = x).
__global__ void winner_row_kernel(const mpcd_best *best, int64_t lo, int64_t n_local, const float *rows, int row_len,
                                  float *out)
{
    const int64_t idx = best->index - lo;
    const bool own = idx >= 0 && idx < n_local;
    for (int i = threadIdx.x; i < row_len; i += blockDim.x) out[i] = own ? rows[idx * row_len + i] : 0.f;
}

// The next warm-start priors (mpcd_shift_plans): workgroup m gathers state m's plan, row index[m] - offset of rows
// [batch][H][d] (index null: row m), and writes it moved one horizon point ahead with the last point repeated,
// out[m][h] = row[min(h + 1, H - 1)]. V floats per access (V divides d, so a vector never straddles two points and
// both sides are V-aligned). An index outside the rows writes nothing.
template <int V>
__global__ __launch_bounds__(256) void shift_plan_kernel(const float *rows, int64_t batch, int H, int d,
                                                         const int64_t *index, int64_t offset, float *out)
{
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const int64_t m = blockIdx.x;
    const int64_t idx = index ? index[m] - offset : m;
    if (idx < 0 || idx >= batch) return;
    const int dv = d / V, n = H * dv;
    const vec_t *src = reinterpret_cast<const vec_t *>(rows + (size_t)idx * H * d);
    vec_t *dst = reinterpret_cast<vec_t *>(out + (size_t)m * H * d);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int h = i / dv, e = i - h * dv;
        dst[i] = src[min(h + 1, H - 1) * dv + e];
    }
}

// ---- The control tails: per call, everything after the sampler in one launch (mpcd_closed_loop's iteration,
// mpcd_mpc_step_batch's step). Grid: n_states * wps workgroups, wps = ceil(group / RT_THREADS); workgroup (m, j) owns
// candidates [m * group + j * RT_THREADS, ...) of plant state m. Per state, every workgroup computes the state's clip
// code (state_clip_code over the state's slice of clip_src), rolls out and costs its candidates from x_dev[m]
// (stage_rows, candidate_cost) and enters its best one (select_first: the only entrant is the group's first
// candidate); the state's last workgroup to arrive (last_arriver_argmin on counters[m]) holds the winner and writes the
// state's results. The two kernels spell this front half out with the same calls in the same order: moved into one
// __device__ function it compiles to other register figures (batch_step_tail_kernel<3> from 97 to 106 SGPRs and from
// 8 to 7 waves per SIMD), so the shared pieces are the helpers it calls.

// NormK's constants before their (exact) promotion to fp64: half the kernel-argument registers
struct NormF {
    float mn[12], den[12];
};

// The closed loop's tail: the state's last workgroup takes control_step_kernel's plant step x_dev[m] <- f(x_dev[m],
// u0) and writes the history rows, the next context row (normalize_states_kernel's formula) and the next prior
// (shift_plan_kernel's rule on the winner's normalised plan), one row per state or one per candidate (repeat_rows).
template <int SYS>
__global__ __launch_bounds__(RT_THREADS) void closed_loop_tail_kernel(const SysK S, const NormF nk, const ClosedLoopTail T)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int H = T.H, row = H * nu, stride = row + 1;
    const int wps = (int)((T.group + RT_THREADS - 1) / RT_THREADS);
    const int64_t m = blockIdx.x / wps;
    const int j = (int)(blockIdx.x - m * wps);
    const int64_t base = m * T.group, end = base + T.group;
    const int64_t c0 = base + (int64_t)j * RT_THREADS;
    stage_rows(T.u_norm + (size_t)c0 * row, min((int64_t)RT_THREADS, end - c0), row, su);
    const int code = state_clip_code(T.clip_src + (size_t)m * T.clip_per_state, T.clip_per_state);
    __syncthreads();
    const bool clip = code == 1;
    const int64_t b = min(c0 + threadIdx.x, end - 1);  // lanes past the group recompute its last candidate
    double x[nx];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = T.x_dev[m * nx + i];
    const double J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H);
    double v = isnan(J) ? INFINITY : J;
    int64_t i = c0 + threadIdx.x < end && (!T.select_first || b == base) ? b : -1;
    wave_argmin(v, i);  // RT_THREADS == one wave; every lane holds the result
    const double raw = __shfl(J, i >= 0 ? (int)(i - c0) : 0);  // the entrant's cost as computed (a NaN stays one)
    const int64_t p0 = blockIdx.x - j;
    if (!last_arriver_argmin(T.part_cost + p0, T.part_idx + p0, T.part_raw + p0, T.counters + m, j, wps, v, i, raw)) return;
    __shared__ float ctx_row[16];
    if (i >= 0) {
        // every lane computes the (wave-uniform) plant step and lane 0 stores it: with the fp64 pow and the dynamics
        // inside a one-lane branch the quadrotor kernel reserved a 36-byte private segment
        double xc[nx], xn[nx], u[nu];
#pragma unroll
        for (int e = 0; e < nx; ++e) xc[e] = T.x_dev[m * nx + e];
#pragma unroll
        for (int e = 0; e < nu; ++e)
            u[e] = rounded_action(T.u_norm[(size_t)i * row + e], clip, S.umin[e], S.umax[e], T.decimals);
        dyn_step<SYS>(S, xc, u, xn);
        const double raw_best = __builtin_nontemporal_load(T.part_raw + p0 + (i - base) / RT_THREADS);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int e = 0; e < nx; ++e) {
                T.x_dev[m * nx + e] = xn[e];
                T.x_next[m * nx + e] = xn[e];
                ctx_row[e] = (float)(2.0 * ((xn[e] - (double)nk.mn[e]) / (double)nk.den[e]) - 1.0);
            }
#pragma unroll
            for (int e = 0; e < nu; ++e) T.u_applied[m * nu + e] = u[e];
            T.best_idx[m] = i;
            T.best_cost[m] = raw_best;
        }
    }
    __syncthreads();
    if (i < 0) return;
    const int64_t reps = T.repeat_rows ? T.group : 1;
    float *co = T.ctx_out + (size_t)m * reps * nx;
    for (int64_t e = threadIdx.x; e < reps * nx; e += RT_THREADS) co[e] = ctx_row[e % nx];
    if (T.prior_out) {
        const float *wr = T.u_norm + (size_t)i * row;
        float *po = T.prior_out + (size_t)m * reps * row;
        for (int64_t e = threadIdx.x; e < reps * row; e += RT_THREADS) {
            const int k = (int)(e % row), h = k / nu;
            po[e] = wr[min(h + 1, H - 1) * nu + (k - h * nu)];
        }
    }
}

// The batched external step's tail: closed_loop_tail_kernel's front half; no plant step, no history, no context row.
// The state's last workgroup writes into the packed result block the state's record {cost as computed, index, flags,
// u[n_u] fp64: control_step_kernel's unnormalise and rounding} and, cooperatively across the wave, the selected plan
// unnormalised under the state's clip flag; with prior_out, the next prior (shift_plan_kernel's rule on the winner's
// normalised plan).
template <int SYS>
__global__ __launch_bounds__(RT_THREADS) void batch_step_tail_kernel(const SysK S, const BatchStepTail T)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int H = T.H, row = H * nu, stride = row + 1;
    const int wps = (int)((T.group + RT_THREADS - 1) / RT_THREADS);
    const int64_t m = blockIdx.x / wps;
    const int j = (int)(blockIdx.x - m * wps);
    const int64_t base = m * T.group, end = base + T.group;
    const int64_t c0 = base + (int64_t)j * RT_THREADS;
    stage_rows(T.u_norm + (size_t)c0 * row, min((int64_t)RT_THREADS, end - c0), row, su);
    const int code = state_clip_code(T.clip_src + (size_t)m * T.clip_per_state, T.clip_per_state);
    __syncthreads();
    const bool clip = code == 1;
    const int64_t b = min(c0 + threadIdx.x, end - 1);  // lanes past the group recompute its last candidate
    double x[nx];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = T.x_dev[m * nx + i];
    const double J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H);
    double v = isnan(J) ? INFINITY : J;
    int64_t i = c0 + threadIdx.x < end && (!T.select_first || b == base) ? b : -1;
    wave_argmin(v, i);  // RT_THREADS == one wave; every lane holds the result
    const double raw = __shfl(J, i >= 0 ? (int)(i - c0) : 0);  // the entrant's cost as computed (a NaN stays one)
    const int64_t p0 = blockIdx.x - j;
    if (!last_arriver_argmin(T.part_cost + p0, T.part_idx + p0, T.part_raw + p0, T.counters + m, j, wps, v, i, raw)) return;
    if (i < 0) return;  // not reached: group >= 1 leaves an entrant in the state's first workgroup
    // every lane computes the (wave-uniform) action and lane 0 stores it, as in closed_loop_tail_kernel
    double u[nu];
#pragma unroll
    for (int e = 0; e < nu; ++e)
        u[e] = rounded_action(T.u_norm[(size_t)i * row + e], clip, S.umin[e], S.umax[e], T.decimals);
    const double raw_best = __builtin_nontemporal_load(T.part_raw + m * wps + (i - base) / RT_THREADS);
    if (threadIdx.x == 0) {
        char *rec = T.result + m * T.rec_stride;
        mpcd_state_result r;
        r.cost = raw_best;
        r.index = i;
        r.flags = (code == 1 ? MPCD_STEP_CLIPPED : 0) | (code == 2 ? MPCD_STEP_NAN_SAMPLES : 0) |
                  (isfinite(raw_best) ? 0 : MPCD_STEP_NONFINITE_WINNER);
        r.reserved = 0;
        *reinterpret_cast<mpcd_state_result *>(rec) = r;
        double *uo = reinterpret_cast<double *>(rec + sizeof(mpcd_state_result));
#pragma unroll
        for (int e = 0; e < nu; ++e) uo[e] = u[e];
    }
    const float *wr = T.u_norm + (size_t)i * row;
    float *plan = reinterpret_cast<float *>(T.result + T.plan_off) + (size_t)m * row;
    float *po = T.prior_out ? T.prior_out + (size_t)m * row : nullptr;
    for (int k = threadIdx.x; k < row; k += RT_THREADS) {
        const int h = k / nu, e = k - h * nu;
        float mn = S.umin[0], mx = S.umax[0];
#pragma unroll
        for (int q = 1; q < nu; ++q)
            if (e == q) { mn = S.umin[q]; mx = S.umax[q]; }
        plan[k] = unnorm1(wr[k], clip, mn, mx);
        if (po) po[k] = wr[min(h + 1, H - 1) * nu + e];
    }
}

// batch_step_tail_kernel that also ranks each state's k best candidates (mpcd_mpc_step_batch_elite): no cost array and
// no top-k launch. After candidate_cost every lane holds one (cost, index) pair; min(k, candidates of the workgroup)
// rounds of wave_argmin, the picked lane retiring itself, leave the workgroup's ranked list with entry r in lane r. It
// goes to part_elite[m][j][0..k) (empty entries: index -1), the raw cost of entry 0 to part_raw as in the tail above.
// The state's last workgroup (last_arriver) merges the wps lists (merge_lists; one workgroup per state: its own list is
// the result) into the k elites, bit for bit mpcd_topk over mpcd_rollout_cost_grouped's costs: NaN reported as +inf,
// ties to the lower index, global indices. Elite 0 is the winner; the record, u0 and the plan are written as above and
// the elites to result + elite_off [n_states][k], where the launch_elite_priors that follows reads them: a state's one
// wave does not write group * H * d floats of priors.
template <int SYS>
__global__ __launch_bounds__(RT_THREADS) void batch_step_elite_tail_kernel(const SysK S, const BatchEliteTail T)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int H = T.H, row = H * nu, stride = row + 1, k = T.k;
    const int wps = (int)((T.group + RT_THREADS - 1) / RT_THREADS);
    const int64_t m = blockIdx.x / wps;
    const int j = (int)(blockIdx.x - m * wps);
    const int64_t base = m * T.group, end = base + T.group;
    const int64_t c0 = base + (int64_t)j * RT_THREADS;
    const int nc = (int)min((int64_t)RT_THREADS, end - c0);
    stage_rows(T.u_norm + (size_t)c0 * row, nc, row, su);
    const int code = state_clip_code(T.clip_src + (size_t)m * T.clip_per_state, T.clip_per_state);
    __syncthreads();
    const bool clip = code == 1;
    const int64_t b = min(c0 + threadIdx.x, end - 1);  // lanes past the group recompute its last candidate
    double x[nx];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = T.x_dev[m * nx + i];
    const double J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H);
    double v = isnan(J) ? INFINITY : J;
    int64_t i = (int)threadIdx.x < nc ? b : -1;
    double mv = INFINITY, raw = J;  // lane r: entry r of the list
    int64_t mi = -1;
    const int rounds = min(k, nc);
    for (int r = 0; r < rounds; ++r) {
        double wv = v;
        int64_t wi = i;
        wave_argmin(wv, wi);  // RT_THREADS == one wave; every lane holds the result
        if (r == 0) raw = __shfl(J, (int)(wi - c0));  // entry 0's cost as computed (a NaN stays one)
        if ((int)threadIdx.x == r) { mv = wv; mi = wi; }
        if (i == wi) i = -1;
    }
    const size_t p0 = (size_t)m * wps;
    if (wps > 1) {
        mpcd_best *pl = T.part_elite + (p0 + j) * k;
        if ((int)threadIdx.x < k) pl[threadIdx.x] = mpcd_best{mv, mi};
        __threadfence();
    }
    if (!last_arriver(
            T.counters + m, wps, [&] { T.part_raw[p0 + j] = raw; },
            [&] {
                if (wps > 1) merge_lists(T.part_elite + p0 * k, wps, k, mv, mi);
            }))
        return;
    v = __shfl(mv, 0);
    i = __shfl(mi, 0);
    if (i < 0) return;  // not reached: group >= 1 leaves an entrant in the state's first workgroup
    // every lane computes the (wave-uniform) action and lane 0 stores it, as in closed_loop_tail_kernel
    double u[nu];
#pragma unroll
    for (int e = 0; e < nu; ++e)
        u[e] = rounded_action(T.u_norm[(size_t)i * row + e], clip, S.umin[e], S.umax[e], T.decimals);
    const double raw_best = __builtin_nontemporal_load(T.part_raw + p0 + (i - base) / RT_THREADS);
    if (threadIdx.x == 0) {
        char *rec = T.result + m * T.rec_stride;
        mpcd_state_result r;
        r.cost = raw_best;
        r.index = i;
        r.flags = (code == 1 ? MPCD_STEP_CLIPPED : 0) | (code == 2 ? MPCD_STEP_NAN_SAMPLES : 0) |
                  (isfinite(raw_best) ? 0 : MPCD_STEP_NONFINITE_WINNER);
        r.reserved = 0;
        *reinterpret_cast<mpcd_state_result *>(rec) = r;
        double *uo = reinterpret_cast<double *>(rec + sizeof(mpcd_state_result));
#pragma unroll
        for (int e = 0; e < nu; ++e) uo[e] = u[e];
    }
    if ((int)threadIdx.x < k) reinterpret_cast<mpcd_best *>(T.result + T.elite_off)[m * k + threadIdx.x] = mpcd_best{mv, mi};
    const float *wr = T.u_norm + (size_t)i * row;
    float *plan = reinterpret_cast<float *>(T.result + T.plan_off) + (size_t)m * row;
    for (int q = threadIdx.x; q < row; q += RT_THREADS) {
        const int e = q % nu;
        float mn = S.umin[0], mx = S.umax[0];
#pragma unroll
        for (int c = 1; c < nu; ++c)
            if (e == c) { mn = S.umin[c]; mx = S.umax[c]; }
        plan[q] = unnorm1(wr[q], clip, mn, mx);
    }
}

// The box and the tolerance of the box tail: a kernel argument of their own, as rollout_cost_box_kernel's box is
struct BoxTolK {
    BoxK box;
    double tol;
};
// batch_step_elite_tail_kernel with a state box (mpcd_mpc_step_batch_box): the same front half with BoxVisit riding
// candidate_cost, so a candidate's cost and violation are the bits rollout_cost_box_kernel writes; after it every lane
// holds (V, cost, index). The workgroup's ranked list (min(k, its candidates) rounds of wave_argmin3; k = 1 without
// elites) goes to part_elite[m][j][0..k) with each entry's V in part_viol[m][j][0..k), its count of real lanes with
// V <= tol (ballot and popcount: lanes past the group are neither entrants nor counted) to part_nfeas[m][j], entry 0's
// raw cost to part_raw. The state's last workgroup merges the lists on the three keys (merge_lists3), sums the counts
// and writes: the record (MPCD_STEP_INFEASIBLE iff the sum is 0), u0, the selected candidate's V and n_feasible, the k
// ranked entries with their V (bit for bit mpcd_topk_feasible over mpcd_rollout_cost_box), the plan and, with
// prior_out (no elites), the next prior by shift_plan_kernel's rule. No cost or violation array goes through memory.
// The constraint-set tail (mpcd_mpc_step_batch_constr) is the instantiation <SYS, ConTolK> of this same kernel: C is
// then the set, the tolerance and the states' previous applied actions (dev [n_states][n_u] or null), again a kernel
// argument of their own, so the SysK and tail argument blocks stay as they are, and ConstrVisit rides candidate_cost
// (the bits rollout_cost_constr_kernel writes). The lines that choose the visitor are all the two differ in. They are
// one kernel template and not two kernels around a shared __device__ body: inlined from such a body the box
// instantiations come out with another register allocation (3,905 against 3,869 lines for <3>, more SGPR spills to
// lanes), as the control tails above did; this way <SYS, BoxTolK> is the former kernel instruction for instruction.
struct ConTolK {
    ConK con;
    double tol;
    const double *u_prev;
};
template <int SYS, class ConArg = BoxTolK>
__global__ __launch_bounds__(RT_THREADS) void batch_step_box_tail_kernel(const SysK S, const ConArg C, const BatchBoxTail T)
{
    constexpr int nx = SysDim<SYS>::NX, nu = SysDim<SYS>::NU;
    extern __shared__ float su[];  // [RT_THREADS][H*nu + 1]
    const int H = T.H, row = H * nu, stride = row + 1, k = T.k;
    const int wps = (int)((T.group + RT_THREADS - 1) / RT_THREADS);
    const int64_t m = blockIdx.x / wps;
    const int j = (int)(blockIdx.x - m * wps);
    const int64_t base = m * T.group, end = base + T.group;
    const int64_t c0 = base + (int64_t)j * RT_THREADS;
    const int nc = (int)min((int64_t)RT_THREADS, end - c0);
    stage_rows(T.u_norm + (size_t)c0 * row, nc, row, su);
    const int code = state_clip_code(T.clip_src + (size_t)m * T.clip_per_state, T.clip_per_state);
    __syncthreads();
    const bool clip = code == 1;
    const int64_t b = min(c0 + threadIdx.x, end - 1);  // lanes past the group recompute its last candidate
    double x[nx];
#pragma unroll
    for (int i = 0; i < nx; ++i) x[i] = T.x_dev[m * nx + i];
    double Vacc = 0.0, J;
    bool bad = false;
    if constexpr (std::is_same<ConArg, ConTolK>::value) {
        double up[nu];
        bool has = ConstrVisit<nx, nu>::load_prev(C.u_prev, m, up);
        J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H, ConstrVisit<nx, nu>{C.con, Vacc, bad, up, has});
    } else {
        J = candidate_cost<SYS>(S, su + (b - c0) * stride, clip, x, H, BoxVisit<nx>{C.box, Vacc, bad});
    }
    const double tol = C.tol;
    const double V = BoxVisit<nx>::finish(Vacc, bad);  // never NaN: a NaN excess is +inf
    const double v = isnan(J) ? INFINITY : J;
    const bool real = (int)threadIdx.x < nc;
    int64_t i = real ? b : -1;
    int64_t nf = __popcll(__ballot(real && V <= tol));
    double mV = INFINITY, mv = INFINITY, raw = J;  // lane r: entry r of the list
    int64_t mi = -1;
    const int rounds = min(k, nc);
    for (int r = 0; r < rounds; ++r) {
        double wV = V, wv = v;
        int64_t wi = i;
        wave_argmin3(wV, wv, wi, tol);  // RT_THREADS == one wave; every lane holds the result
        if (r == 0) raw = __shfl(J, (int)(wi - c0));  // entry 0's cost as computed (a NaN stays one)
        if ((int)threadIdx.x == r) { mV = wV; mv = wv; mi = wi; }
        if (i == wi) i = -1;
    }
    const size_t p0 = (size_t)m * wps;
    if (wps > 1) {
        if ((int)threadIdx.x < k) {
            T.part_elite[(p0 + j) * k + threadIdx.x] = mpcd_best{mv, mi};
            T.part_viol[(p0 + j) * k + threadIdx.x] = mV;
        }
        __threadfence();
    }
    if (!last_arriver(
            T.counters + m, wps,
            [&] {
                T.part_raw[p0 + j] = raw;
                T.part_nfeas[p0 + j] = nf;
            },
            [&] {
                if (wps > 1) {
                    merge_lists3(T.part_elite + p0 * k, T.part_viol + p0 * k, wps, k, tol, mV, mv, mi);
                    int64_t s = 0;
                    for (int w = threadIdx.x; w < wps; w += RT_THREADS) s += __builtin_nontemporal_load(T.part_nfeas + p0 + w);
#pragma unroll
                    for (int q = 32; q >= 1; q >>= 1) s += __shfl_xor(s, q);
                    nf = s;
                }
            }))
        return;
    const double V0 = __shfl(mV, 0);
    i = __shfl(mi, 0);
    if (i < 0) return;  // not reached: group >= 1 leaves an entrant in the state's first workgroup
    // every lane computes the (wave-uniform) action and lane 0 stores it, as in closed_loop_tail_kernel
    double u[nu];
#pragma unroll
    for (int e = 0; e < nu; ++e)
        u[e] = rounded_action(T.u_norm[(size_t)i * row + e], clip, S.umin[e], S.umax[e], T.decimals);
    const double raw_best = __builtin_nontemporal_load(T.part_raw + p0 + (i - base) / RT_THREADS);
    if (threadIdx.x == 0) {
        char *rec = T.result + m * T.rec_stride;
        mpcd_state_result r;
        r.cost = raw_best;
        r.index = i;
        r.flags = (code == 1 ? MPCD_STEP_CLIPPED : 0) | (code == 2 ? MPCD_STEP_NAN_SAMPLES : 0) |
                  (isfinite(raw_best) ? 0 : MPCD_STEP_NONFINITE_WINNER) | (nf == 0 ? MPCD_STEP_INFEASIBLE : 0);
        r.reserved = 0;
        *reinterpret_cast<mpcd_state_result *>(rec) = r;
        double *uo = reinterpret_cast<double *>(rec + sizeof(mpcd_state_result));
#pragma unroll
        for (int e = 0; e < nu; ++e) uo[e] = u[e];
        reinterpret_cast<double *>(T.result + T.viol_off)[m] = V0;
        reinterpret_cast<int64_t *>(T.result + T.nfeas_off)[m] = nf;
    }
    if ((int)threadIdx.x < k) {
        reinterpret_cast<mpcd_best *>(T.result + T.elite_off)[m * k + threadIdx.x] = mpcd_best{mv, mi};
        reinterpret_cast<double *>(T.result + T.eviol_off)[m * k + threadIdx.x] = mV;
    }
    const float *wr = T.u_norm + (size_t)i * row;
    float *plan = reinterpret_cast<float *>(T.result + T.plan_off) + (size_t)m * row;
    float *po = T.prior_out ? T.prior_out + (size_t)m * row : nullptr;
    for (int q = threadIdx.x; q < row; q += RT_THREADS) {
        const int h = q / nu, e = q - h * nu;
        float mn = S.umin[0], mx = S.umax[0];
#pragma unroll
        for (int c = 1; c < nu; ++c)
            if (e == c) { mn = S.umin[c]; mx = S.umax[c]; }
        plan[q] = unnorm1(wr[q], clip, mn, mx);
        if (po) po[q] = wr[min(h + 1, H - 1) * nu + e];
    }
}
__global__ __launch_bounds__(256) void repeat_rows_kernel(const float *rows, int64_t total, int64_t n, int row_len, float *out)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / row_len;
        out[e] = rows[(r / n) * row_len + (e - r * row_len)];
    }
}

// The by-value system argument of the kernels above (x0 zero: launch_rollout_cost sets it)
SysK make_sysk(const mpcd_system_desc &d, const float *umin_host, const float *umax_host)
{
    SysK S = {};
    S.system = d.system;
    S.cost_kind = d.cost_kind;
    S.nx = d.n_x;
    S.nu = d.n_u;
    for (int i = 0; i < 24; ++i) S.params[i] = d.params[i];
    for (int i = 0; i < 12; ++i) { S.Q[i] = d.Q[i]; S.P[i] = d.P[i]; S.xr[i] = d.x_ref[i]; }
    for (int i = 0; i < 4; ++i) S.R[i] = d.R[i];
    for (int i = 0; i < d.n_u; ++i) { S.umin[i] = umin_host[i]; S.umax[i] = umax_host[i]; }
    return S;
}

// launch(std::integral_constant<int, SYS>) for the descriptor's system, refused unless its sizes are that system's
template <class Launch>
hipError_t dispatch_system(const mpcd_system_desc &d, Launch launch)
{
#define MPCD_SYSTEM(SYS_)                                                                        \
    case SYS_:                                                                                   \
        if (d.n_x != SysDim<SYS_>::NX || d.n_u != SysDim<SYS_>::NU) return hipErrorInvalidValue; \
        launch(std::integral_constant<int, SYS_>{});                                             \
        break;
    switch (d.system) {
        MPCD_SYSTEM(MPCD_SYS_CARTPOLE_LIN5)
        MPCD_SYSTEM(MPCD_SYS_CARTPOLE_NL5)
        MPCD_SYSTEM(MPCD_SYS_CARTPOLE_ZOH4)
        MPCD_SYSTEM(MPCD_SYS_DOUBLE_INT2D)
        MPCD_SYSTEM(MPCD_SYS_PENDULUM)
        MPCD_SYSTEM(MPCD_SYS_QUADROTOR12)
    default: return hipErrorInvalidValue;
    }
#undef MPCD_SYSTEM
    return hipGetLastError();
}

}  // namespace

hipError_t launch_repeat_rows(const float *rows, int64_t n_rows, int64_t n, int row_len, float *out, hipStream_t stream)
{
    const int64_t total = n_rows * n * row_len;
    const int64_t blocks = std::min<int64_t>(4096, (total + 255) / 256);
    hipLaunchKernelGGL(repeat_rows_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, stream, rows, total,
                       n, row_len, out);
    return hipGetLastError();
}

hipError_t launch_closed_loop_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                   const float *cmin_host, const float *cmax_host, const ClosedLoopTail &t,
                                   hipStream_t stream)
{
    const SysK S = make_sysk(d, umin_host, umax_host);
    NormF nk;
    for (int i = 0; i < 12; ++i) {
        nk.mn[i] = i < d.n_x ? cmin_host[i] : 0.f;
        nk.den[i] = i < d.n_x ? cmax_host[i] - cmin_host[i] : 1.f;  // fp32 subtraction; promoted in the kernel
    }
    const int64_t wgs = t.n_states * ((t.group + RT_THREADS - 1) / RT_THREADS);
    if (t.n_states < 1 || t.group < 1 || wgs > 0x7fffffff) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * RT_THREADS * (t.H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(closed_loop_tail_kernel<decltype(sys)::value>, dim3((unsigned)wgs), dim3(RT_THREADS), lds, stream,
                           S, nk, t);
    });
}

hipError_t launch_batch_step_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                  const BatchStepTail &t, hipStream_t stream)
{
    const SysK S = make_sysk(d, umin_host, umax_host);
    const int64_t wgs = t.n_states * ((t.group + RT_THREADS - 1) / RT_THREADS);
    if (t.n_states < 1 || t.group < 1 || wgs > 0x7fffffff) return hipErrorInvalidValue;
    if (t.rec_stride != batch_step_rec_stride(d.n_u) || t.plan_off < t.n_states * t.rec_stride) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * RT_THREADS * (t.H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(batch_step_tail_kernel<decltype(sys)::value>, dim3((unsigned)wgs), dim3(RT_THREADS), lds, stream,
                           S, t);
    });
}

hipError_t launch_batch_elite_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                   const BatchEliteTail &t, hipStream_t stream)
{
    const SysK S = make_sysk(d, umin_host, umax_host);
    const int64_t wgs = t.n_states * ((t.group + RT_THREADS - 1) / RT_THREADS);
    if (t.n_states < 1 || t.group < 1 || wgs > 0x7fffffff) return hipErrorInvalidValue;
    if (t.rec_stride != batch_step_rec_stride(d.n_u) || t.plan_off < t.n_states * t.rec_stride) return hipErrorInvalidValue;
    if (t.k < 1 || t.k > MPCD_MAX_ELITES || t.k > t.group || t.select_first || !t.part_elite ||
        t.elite_off < t.plan_off + (int64_t)sizeof(float) * t.n_states * t.H * d.n_u || t.elite_off % alignof(mpcd_best))
        return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * RT_THREADS * (t.H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(batch_step_elite_tail_kernel<decltype(sys)::value>, dim3((unsigned)wgs), dim3(RT_THREADS), lds,
                           stream, S, t);
    });
}

// The set as the kernels take it: entries the kernels never read (i >= n_x, j >= n_u, rows >= n_rows) are neutral
static ConK make_conk(const mpcd_system_desc &d, const mpcd_constraints &con)
{
    ConK k = {};
    for (int i = 0; i < 12; ++i) {
        k.box.lo[i] = i < d.n_x ? con.box.lo[i] : -INFINITY;
        k.box.hi[i] = i < d.n_x ? con.box.hi[i] : INFINITY;
    }
    k.n_rows = con.n_rows;
    for (int r = 0; r < MPCD_MAX_CON_ROWS; ++r) {
        const bool used = r < con.n_rows;
        for (int i = 0; i < 12; ++i) k.A[r][i] = used && i < d.n_x ? con.A[r][i] : 0.0;
        for (int j = 0; j < 4; ++j) k.C[r][j] = used && j < d.n_u ? con.C[r][j] : 0.0;
        k.b[r] = used ? con.b[r] : INFINITY;
    }
    for (int j = 0; j < 4; ++j) k.du[j] = j < d.n_u ? con.du_max[j] : INFINITY;
    return k;
}

// What the box tail and the constraint-set tail check of their common argument block
static bool viol_tail_ok(const mpcd_system_desc &d, double tol, const BatchBoxTail &t)
{
    const int64_t wgs = t.n_states * ((t.group + RT_THREADS - 1) / RT_THREADS);
    if (t.n_states < 1 || t.group < 1 || wgs > 0x7fffffff) return false;
    if (t.rec_stride != batch_step_rec_stride(d.n_u) || t.plan_off < t.n_states * t.rec_stride) return false;
    // the result block's parts in order, none overlapping the one before: plans, V, n_feasible, entries, their V
    return !(t.k < 1 || t.k > MPCD_MAX_ELITES || t.k > t.group || t.select_first || !t.part_elite || !t.part_viol ||
             !t.part_nfeas || !(tol >= 0.0) ||
             t.viol_off < t.plan_off + (int64_t)sizeof(float) * t.n_states * t.H * d.n_u || t.viol_off % alignof(double) ||
             t.nfeas_off < t.viol_off + (int64_t)sizeof(double) * t.n_states || t.nfeas_off % alignof(int64_t) ||
             t.elite_off < t.nfeas_off + (int64_t)sizeof(int64_t) * t.n_states || t.elite_off % alignof(mpcd_best) ||
             t.eviol_off < t.elite_off + (int64_t)sizeof(mpcd_best) * t.n_states * t.k || t.eviol_off % alignof(double));
}

hipError_t launch_batch_constr_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                    const mpcd_constraints &con, double tol, const double *u_prev_dev,
                                    const BatchBoxTail &t, hipStream_t stream)
{
    if (!viol_tail_ok(d, tol, t) || con.n_rows < 0 || con.n_rows > MPCD_MAX_CON_ROWS) return hipErrorInvalidValue;
    const SysK S = make_sysk(d, umin_host, umax_host);
    const int64_t wgs = t.n_states * ((t.group + RT_THREADS - 1) / RT_THREADS);
    const ConTolK C{make_conk(d, con), tol, u_prev_dev};
    const size_t lds = sizeof(float) * RT_THREADS * (t.H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL((batch_step_box_tail_kernel<decltype(sys)::value, ConTolK>), dim3((unsigned)wgs),
                           dim3(RT_THREADS), lds, stream, S, C, t);
    });
}

hipError_t launch_rollout_cost_constr(const mpcd_system_desc &d, const double *x0_dev, int64_t group, const float *u_norm,
                                      const float *umin_host, const float *umax_host, const int *flags_dev, int64_t batch,
                                      int H, const mpcd_constraints &con, const double *u_prev_dev, double *cost,
                                      double *viol, hipStream_t stream)
{
    const int64_t wgs = (batch + RT_THREADS - 1) / RT_THREADS;
    if (batch < 1 || group < 1 || wgs > 0x7fffffff || con.n_rows < 0 || con.n_rows > MPCD_MAX_CON_ROWS)
        return hipErrorInvalidValue;
    const SysK S = make_sysk(d, umin_host, umax_host);
    const ConK ck = make_conk(d, con);
    const size_t lds = sizeof(float) * RT_THREADS * (H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(rollout_cost_constr_kernel<decltype(sys)::value>, dim3((unsigned)wgs), dim3(RT_THREADS), lds,
                           stream, S, ck, u_norm, flags_dev, x0_dev, u_prev_dev, group, batch, H, cost, viol);
    });
}

hipError_t launch_rollout_constr_select(const mpcd_system_desc &d, const double *x0_host, const float *u_norm,
                                        const float *umin_host, const float *umax_host, const int *flag_dev, int64_t batch,
                                        int H, const mpcd_constraints &con, double tol, const double *u_prev_host,
                                        double *cost, double *viol, hipStream_t stream, const RolloutConstrSelect *sel)
{
    const int64_t wgs = (batch + RT_THREADS - 1) / RT_THREADS;
    if (batch < 1 || wgs > 0x7fffffff || con.n_rows < 0 || con.n_rows > MPCD_MAX_CON_ROWS || !(tol >= 0.0) || !x0_host)
        return hipErrorInvalidValue;
    SysK S = make_sysk(d, umin_host, umax_host);
    for (int i = 0; i < d.n_x; ++i) S.x0[i] = x0_host[i];
    ConStepK C = {};
    C.con = make_conk(d, con);
    C.tol = tol;
    C.has_prev = u_prev_host != nullptr;  // ConstrVisit::load_prev's rule: a NaN in any entry means "none"
    for (int j = 0; j < d.n_u && j < 4; ++j) {
        C.u_prev[j] = u_prev_host ? u_prev_host[j] : 0.0;
        if (C.u_prev[j] != C.u_prev[j]) C.has_prev = 0;
    }
    ConSelectK K = {};
    if (sel) {
        if (!sel->block || !sel->part || sel->n_part < wgs || !sel->counter || (sel->host_out && !sel->host_flag))
            return hipErrorInvalidValue;
        K = ConSelectK{sel->block,  sel->part,     sel->counter,   sel->offset,  sel->clip_src,
                       sel->clip_n, sel->host_out, sel->host_flag, sel->host_seq};
    }
    const size_t lds = sizeof(float) * RT_THREADS * (H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        constexpr int SYS = decltype(sys)::value;
        if (sel)
            hipLaunchKernelGGL((rollout_constr_select_kernel<SYS, true>), dim3((unsigned)wgs), dim3(RT_THREADS), lds, stream,
                               S, C, u_norm, flag_dev, batch, H, cost, viol, K);
        else
            hipLaunchKernelGGL((rollout_constr_select_kernel<SYS, false>), dim3((unsigned)wgs), dim3(RT_THREADS), lds, stream,
                               S, C, u_norm, flag_dev, batch, H, cost, viol, K);
    });
}

hipError_t launch_batch_box_tail(const mpcd_system_desc &d, const float *umin_host, const float *umax_host,
                                 const mpcd_state_box &box, double tol, const BatchBoxTail &t, hipStream_t stream)
{
    if (!viol_tail_ok(d, tol, t)) return hipErrorInvalidValue;
    const SysK S = make_sysk(d, umin_host, umax_host);
    const int64_t wgs = t.n_states * ((t.group + RT_THREADS - 1) / RT_THREADS);
    BoxTolK C;
    for (int i = 0; i < 12; ++i) {  // entries >= n_x are ignored: the kernel never reads them
        C.box.lo[i] = i < d.n_x ? box.lo[i] : -INFINITY;
        C.box.hi[i] = i < d.n_x ? box.hi[i] : INFINITY;
    }
    C.tol = tol;
    const size_t lds = sizeof(float) * RT_THREADS * (t.H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(batch_step_box_tail_kernel<decltype(sys)::value>, dim3((unsigned)wgs), dim3(RT_THREADS), lds,
                           stream, S, C, t);
    });
}

hipError_t launch_shift_plans(const float *rows, int64_t batch, int H, int d, const int64_t *index, int64_t offset,
                              int64_t n_states, float *out, hipStream_t stream)
{
    const dim3 grid((unsigned)n_states), block(256);
    const uintptr_t al = reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out);  // a caller's sub-view
    if (d % 4 == 0 && al % 16 == 0)
        hipLaunchKernelGGL(shift_plan_kernel<4>, grid, block, 0, stream, rows, batch, H, d, index, offset, out);
    else if (d % 2 == 0 && al % 8 == 0)
        hipLaunchKernelGGL(shift_plan_kernel<2>, grid, block, 0, stream, rows, batch, H, d, index, offset, out);
    else
        hipLaunchKernelGGL(shift_plan_kernel<1>, grid, block, 0, stream, rows, batch, H, d, index, offset, out);
    return hipGetLastError();
}

hipError_t launch_winner_row(const mpcd_best *best, int64_t lo, int64_t n_local, const float *rows, int row_len,
                             float *out, hipStream_t stream)
{
    hipLaunchKernelGGL(winner_row_kernel, dim3(1), dim3(256), 0, stream, best, lo, n_local, rows, row_len, out);
    return hipGetLastError();
}

hipError_t launch_clip_flag(const float *x, int64_t n, int *flag_dev, unsigned *ws, hipStream_t stream)
{
    const int64_t blocks = std::min<int64_t>(512, (n + 1023) / 1024);
    hipLaunchKernelGGL(clip_flag_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, stream, x, n, flag_dev,
                       ws);
    return hipGetLastError();
}

hipError_t launch_unnormalize(const float *x, int64_t n, int dim, const int *flag_dev, const float *mn_host,
                              const float *mx_host, float *out, hipStream_t stream)
{
    MinMax lim;
    for (int i = 0; i < 16; ++i) {
        lim.mn[i] = i < dim ? mn_host[i] : 0.f;
        lim.mx[i] = i < dim ? mx_host[i] : 0.f;
    }
    const int64_t blocks = std::min<int64_t>(4096, (n + 255) / 256);
    hipLaunchKernelGGL(unnormalize_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, stream, x, n,
                       dim, flag_dev, lim, out);
    return hipGetLastError();
}

hipError_t launch_rollout_cost(const mpcd_system_desc &d, const double *x0_host, const double *x0_dev, int64_t group,
                               const float *u_norm, const float *umin_host, const float *umax_host, const int *flag_dev,
                               int64_t batch, int H, double *cost, hipStream_t stream, const RolloutSelect *sel)
{
    if (group < 1) group = batch;
    SysK S = make_sysk(d, umin_host, umax_host);
    for (int i = 0; i < d.n_x; ++i) S.x0[i] = x0_host ? x0_host[i] : 0.0;
    const size_t lds = sizeof(float) * RT_THREADS * (H * d.n_u + 1);
    SelectK K = {};
    if (sel) {
        if (group != batch || sel->n_part < (batch + RT_THREADS - 1) / RT_THREADS) return hipErrorInvalidValue;
        K = SelectK{sel->best,   sel->row_out, sel->part_cost, sel->part_idx, sel->counter,   sel->offset,
                    sel->code_out, sel->clip_src, sel->clip_n,   sel->host_out, sel->host_flag, sel->host_seq};
    }
    const dim3 grid((unsigned)((batch + RT_THREADS - 1) / RT_THREADS));
    return dispatch_system(d, [&](auto sys) {
        constexpr int SYS = decltype(sys)::value;
        if (sel)
            hipLaunchKernelGGL((rollout_cost_kernel<SYS, true>), grid, dim3(RT_THREADS), lds, stream, S, u_norm, flag_dev,
                               x0_dev, group, batch, H, cost, K);
        else
            hipLaunchKernelGGL((rollout_cost_kernel<SYS, false>), grid, dim3(RT_THREADS), lds, stream, S, u_norm, flag_dev,
                               x0_dev, group, batch, H, cost, K);
    });
}

hipError_t launch_argmin(const double *cost, int64_t n, int64_t offset, mpcd_best *best, hipStream_t stream)
{
    hipLaunchKernelGGL(argmin_kernel, dim3(1), dim3(1024), 0, stream, cost, n, offset, best);
    return hipGetLastError();
}

hipError_t launch_clip_flags(const float *x, int64_t n_groups, int64_t group_elems, int *flags_dev, hipStream_t stream)
{
    if (n_groups > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_flags_kernel, dim3((unsigned)n_groups), dim3(256), 0, stream, x, group_elems, flags_dev);
    return hipGetLastError();
}

hipError_t launch_normalize_states(const double *x, int64_t M, int C, const float *mn_host, const float *mx_host,
                                   float *out, hipStream_t stream)
{
    NormK nk;
    for (int i = 0; i < 16; ++i) {
        nk.mn[i] = i < C ? (double)mn_host[i] : 0.0;
        nk.den[i] = i < C ? (double)(mx_host[i] - mn_host[i]) : 1.0;  // fp32 subtraction, then promoted
    }
    const int64_t n = M * C;
    hipLaunchKernelGGL(normalize_states_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, M, C, nk, out);
    return hipGetLastError();
}

hipError_t launch_control_step(const mpcd_system_desc &d, double *x_dev, int64_t M, int64_t group, const float *u_norm,
                               int H, const double *cost, const float *umin_host, const float *umax_host,
                               const int *flags_dev, int select_first, int decimals, double *u_applied,
                               int64_t *best_idx, double *best_cost, hipStream_t stream)
{
    const SysK S = make_sysk(d, umin_host, umax_host);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(control_step_kernel<decltype(sys)::value>, dim3((unsigned)M), dim3(CS_THREADS), 0, stream, S,
                           x_dev, group, u_norm, H, cost, flags_dev, select_first, decimals, u_applied, best_idx, best_cost);
    });
}

hipError_t launch_rollout_cost_box(const mpcd_system_desc &d, const double *x0_dev, int64_t group, const float *u_norm,
                                   const float *umin_host, const float *umax_host, const int *flags_dev, int64_t batch,
                                   int H, const mpcd_state_box &box, double *cost, double *viol, hipStream_t stream)
{
    const int64_t wgs = (batch + RT_THREADS - 1) / RT_THREADS;
    if (batch < 1 || group < 1 || wgs > 0x7fffffff) return hipErrorInvalidValue;
    const SysK S = make_sysk(d, umin_host, umax_host);
    BoxK bk;
    for (int i = 0; i < 12; ++i) {  // entries >= n_x are ignored: the kernel never reads them
        bk.lo[i] = i < d.n_x ? box.lo[i] : -INFINITY;
        bk.hi[i] = i < d.n_x ? box.hi[i] : INFINITY;
    }
    const size_t lds = sizeof(float) * RT_THREADS * (H * d.n_u + 1);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(rollout_cost_box_kernel<decltype(sys)::value>, dim3((unsigned)wgs), dim3(RT_THREADS), lds, stream,
                           S, bk, u_norm, flags_dev, x0_dev, group, batch, H, cost, viol);
    });
}

hipError_t launch_control_step_picked(const mpcd_system_desc &d, double *x_dev, int64_t M, const float *u_norm,
                                      int64_t batch, int H, const mpcd_best *picks, int64_t pick_stride, int64_t offset,
                                      const float *umin_host, const float *umax_host, const int *flags_dev, int decimals,
                                      double *u_applied, int64_t *best_idx, double *best_cost, hipStream_t stream)
{
    const int64_t wgs = (M + CP_THREADS - 1) / CP_THREADS;
    if (M < 1 || batch < 1 || pick_stride < 1 || wgs > 0x7fffffff) return hipErrorInvalidValue;
    const SysK S = make_sysk(d, umin_host, umax_host);
    return dispatch_system(d, [&](auto sys) {
        hipLaunchKernelGGL(control_step_picked_kernel<decltype(sys)::value>, dim3((unsigned)wgs), dim3(CP_THREADS), 0, stream,
                           S, x_dev, M, u_norm, batch, H, picks, pick_stride, offset, flags_dev, decimals, u_applied,
                           best_idx, best_cost);
    });
}
