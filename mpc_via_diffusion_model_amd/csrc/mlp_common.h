// Shared pieces of the two MLP sampler kernels (mlp_sampler.hip: exact-f32 MFMA; mlp_x3.hip:
// fp32-accurate 3-way bf16 split MFMA). Net = build-defined CFG MLP, SURVEY §8a A11.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"

namespace mlpc {

constexpr int NLAYER = 14;
constexpr int COND_TOTAL = 448;  // 32+64+128+128+64+32
enum { EPI_NONE = 0, EPI_MISH = 1, EPI_CMISH = 2 };
// CFG-DDPM with caller-supplied noise: its own instantiation, so the in-kernel-Philox variant has no
// global load in the step loop (a conditional noise load made the compiler drain vmcnt(0), i.e. wait
// for the next step's weight prefetch, every step).
constexpr int MODE_DDPM_XN = 16;

template <int D0>
struct Arch {
    static constexpr int K[NLAYER] = {D0, 32, 32, 64, 64, 128, 128, 128, 256, 64, 128, 32, 32, 32};
    static constexpr int N[NLAYER] = {32, 32, 64, 64, 128, 128, 128, 128, 64, 64, 32, 32, 32, D0};
    // Loop form (not recursion) so the device inliner folds every call to a constant.
    __host__ __device__ static constexpr int woff(int l) {  // f32 pack: K*N weights + N biases per layer
        int o = 0;
        for (int i = 0; i < l; ++i) o += K[i] * N[i] + N[i];
        return o;
    }
    static constexpr int total() { return woff(NLAYER); }
    __host__ __device__ static constexpr int woff3(int l) {  // bf16x3 pack, in floats: 3 K*N bf16 + N f32
        int o = 0;
        for (int i = 0; i < l; ++i) o += 3 * K[i] * N[i] / 2 + N[i];
        return o;
    }
    static constexpr int total3() { return woff3(NLAYER); }
    __host__ __device__ static constexpr int boff(int l) {  // biases staged in LDS
        int o = 0;
        for (int i = 0; i < l; ++i) o += N[i];
        return o;
    }
    static constexpr int btotal() { return boff(NLAYER); }
};

// Arch<d0>'s layer shapes for host code that has d0 at run time (the weight packers)
inline int layer_k(int d0, int l) { return l == 0 ? d0 : Arch<32>::K[l]; }
inline int layer_n(int d0, int l) { return l == NLAYER - 1 ? d0 : Arch<32>::N[l]; }

// cond block j (0..5) -> column offset in the 448-wide tables
__host__ __device__ constexpr int cond_off(int j) { return j == 0 ? 0 : j == 1 ? 32 : j == 2 ? 96 : j == 3 ? 224 : j == 4 ? 352 : 416; }

// The step plan is read through the constant address space: scalar loads (lgkmcnt), so using it
// never waits on the vector-memory queue that holds the next layers' weight prefetches.
MPCD_DEV StepPlan load_plan(const StepPlan *plan, int s)
{
    typedef const __attribute__((address_space(4))) StepPlan *cplan_t;
    const cplan_t q = (cplan_t)(uintptr_t)plan + s;
    StepPlan r;
    r.t = q->t;
    r.flags = q->flags;
    r.a = q->a;
    r.b = q->b;
    r.c1 = q->c1;
    r.c2 = q->c2;
    r.std = q->std;
    r.sqan = q->sqan;
    r.cn = q->cn;
    r.pad = 0.f;
    return r;
}

// The candidates [cand0, cand0 + n) and the context projection row of one split-bf16 workgroup (CPW candidates per
// workgroup, n <= CPW). A plain call (GRP = false): workgroup i starts at i CPW, ends with the batch and reads row 0;
// that is the code these kernels had before grouped calls existed, n is unused and the bound is candidate < batch.
// A grouped call (GRP = true, mpcd_sample_grouped; group_wgs = ceil(group / CPW) from the launcher): workgroup j of
// group m starts at m group + j CPW, ends with the group and reads row m, so that a workgroup holds candidates of one
// context row only; its columns past n are the idle rows that columns past the batch are in a plain call (zero
// input, no global write). Everything here is wave-uniform (scalar registers). GRP is a template flag and not a
// run-time branch because the 8-wave resident-weight kernels have no register to spare: a run-time form of this put
// three of their H*d = 128 instantiations into scratch (profiles/grouped_kernel_resources.txt).
struct CandSpan {
    int64_t cand0;
    int32_t n;
    const float *cproj;
    int32_t m;  // the group (0 in a plain call): the row of a per-group warm-start prior
};
template <int CPW, bool GRP>
MPCD_DEV CandSpan cand_span(const float *cproj, int64_t group, int32_t group_wgs)
{
    if constexpr (!GRP) {
        return CandSpan{(int64_t)blockIdx.x * CPW, 0, cproj, 0};
    } else {
        const uint32_t m = __builtin_amdgcn_readfirstlane(blockIdx.x / (uint32_t)group_wgs);
        const uint32_t j = blockIdx.x - m * (uint32_t)group_wgs;
        const int64_t left = group - (int64_t)j * CPW;  // >= 1: j < ceil(group / CPW)
        return CandSpan{(int64_t)m * group + (int64_t)j * CPW, left < CPW ? (int32_t)left : CPW,
                        cproj + (size_t)m * COND_TOTAL, (int32_t)m};
    }
}
// column / local candidate c of the workgroup holds a candidate of the call
template <bool GRP>
MPCD_DEV bool in_span(int64_t batch, int64_t cand0, int n, int c)
{
    if constexpr (GRP) return c < n;
    else return cand0 + c < batch;
}

// Host side of cand_span: the grid of a call and, for a grouped one (group > 0), the workgroups per group. false: a
// batch that is no whole number of groups, or a grid past the launch limit.
inline bool cand_grid(int cpw, int64_t batch, int64_t group, int64_t *blocks, int32_t *group_wgs)
{
    *group_wgs = 0;
    *blocks = (batch + cpw - 1) / cpw;
    if (group > 0) {
        if (batch % group != 0) return false;
        const int64_t wgs = (group + cpw - 1) / cpw;
        if (wgs > INT32_MAX) return false;
        *group_wgs = (int32_t)wgs;
        *blocks = batch / group * wgs;
    }
    return *blocks <= INT32_MAX;
}

// A call's run-time choices -> the template parameters of the MLP sampler kernels, once for the four families:
// f(D0, SMODE, CTX, GRP) is called with std::integral_constants (usable as template arguments) for H*d = d0, the
// sampler mode (CFG-DDPM with caller-supplied noise is MODE_DDPM_XN), context or none, grouped contexts or not.
// hipErrorInvalidValue where no kernel has the combination: an unknown d0 or mode, a grouped call without a context
// or of the eps forwards (grouped calls are the samplers': mpcd_sample_grouped). A family rejects what else it does
// not build with if constexpr, and one with no grouped form passes grouped = false.
template <class F>
hipError_t sampler_dispatch(int d0, int mode, bool noise, bool ctx, bool grouped, F f)
{
    auto with_d0 = [&](auto D0) -> hipError_t {
        auto with_mode = [&](auto SMODE) -> hipError_t {
            constexpr std::true_type yes{};
            constexpr std::false_type no{};
            if (grouped) {
                if constexpr (SMODE != MODE_EPS && SMODE != MODE_EPS1)
                    if (ctx) return f(D0, SMODE, yes, yes);
                return hipErrorInvalidValue;
            }
            return ctx ? f(D0, SMODE, yes, no) : f(D0, SMODE, no, no);
        };
        switch (mode) {
        case MODE_DDPM_CFG:
            return noise ? with_mode(std::integral_constant<int, MODE_DDPM_XN>{})
                         : with_mode(std::integral_constant<int, MODE_DDPM_CFG>{});
        case MODE_DDIM_CFG: return with_mode(std::integral_constant<int, MODE_DDIM_CFG>{});
        case MODE_DDIM: return with_mode(std::integral_constant<int, MODE_DDIM>{});
        case MODE_EPS: return with_mode(std::integral_constant<int, MODE_EPS>{});
        case MODE_EPS1: return with_mode(std::integral_constant<int, MODE_EPS1>{});
        }
        return hipErrorInvalidValue;
    };
    switch (d0) {
    case 32: return with_d0(std::integral_constant<int, 32>{});
    case 64: return with_d0(std::integral_constant<int, 64>{});
    case 128: return with_d0(std::integral_constant<int, 128>{});
    }
    return hipErrorInvalidValue;
}

// Layer profile of the MLP sampler kernels (tools/layer_prof.py, tools/mlp_prof.sh). Only a build with
// -DMPCD_PROF_LAYERS measures: per-wave shader-clock cycles of each barrier-to-barrier segment k (work, then the
// barrier wait) in tacc[2 k] / tacc[2 k + 1], dumped to MlpSampleArgs::dbg at the kernel's end. A kernel keeps
//     ProfAcc tacc = {}; const uint64_t rt0 = prof_realtime(); uint64_t tprev = prof_now(); const uint64_t ct0 = tprev;
// In the product build ProfAcc is empty, the clocks read 0, prof_barrier() is lds_barrier() and the rest does nothing:
// the kernels carry no trace of it.
#ifdef MPCD_PROF_LAYERS
typedef uint64_t ProfAcc[2 * 16];
MPCD_DEV uint64_t prof_now() { return __builtin_readcyclecounter(); }
MPCD_DEV uint64_t prof_realtime() { return __builtin_amdgcn_s_memrealtime(); }
MPCD_DEV void prof_barrier(ProfAcc &tacc, uint64_t &tprev, int k)  // ends segment k
{
    uint64_t t = __builtin_readcyclecounter();
    tacc[2 * k] += t - tprev;
    lds_barrier();
    tprev = __builtin_readcyclecounter();
    tacc[2 * k + 1] += tprev - t;
}
// cycles of a stretch inside a segment: t0 = prof_now() ... prof_mark(tacc, t0, k, dep) adds the cycles since t0 to
// tacc[k] once dep is computed, and moves t0 on
template <class T>
MPCD_DEV void prof_mark(ProfAcc &tacc, uint64_t &t0, int k, const T &dep)
{
    asm volatile("" ::"v"(dep) : "memory");
    const uint64_t t = __builtin_readcyclecounter();
    tacc[k] += t - t0;
    t0 = t;
}
MPCD_DEV void prof_mark(ProfAcc &tacc, uint64_t t0, int k)
{
    asm volatile("" ::: "memory");
    tacc[k] += __builtin_readcyclecounter() - t0;
}
// The end-of-kernel dump, in a scope with the four variables above and the MlpSampleArgs p. W waves per workgroup: the
// first 32 / W workgroups fill the 32 wave slots. A macro, not a function: as a function it changed the profile
// build's register allocation and schedule in every kernel (profiles/mlp_switch_cleanup_isa.txt).
#define MPCD_PROF_DUMP(W, wave, lane)                                                                                  \
    do {                                                                                                               \
        const uint64_t t = __builtin_readcyclecounter();                                                               \
        tacc[2 * 15] += t - tprev;                                                                                     \
        if (p.dbg && blockIdx.x < 32 / (W) && (lane) == 0)                                                             \
            for (int i = 0; i < 32; ++i) p.dbg[(blockIdx.x * (W) + (wave)) * 32 + i] = (float)tacc[i];                 \
        if (p.dbg && threadIdx.x == 0) { /* per-block loop start / end (memrealtime, low 32 bits) */                   \
            p.dbg[4096 + blockIdx.x * 2] = __builtin_bit_cast(float, (uint32_t)rt0);                                   \
            p.dbg[4096 + blockIdx.x * 2 + 1] = __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_s_memrealtime()); \
        }                                                                                                              \
        if (p.dbg && blockIdx.x < 8 && threadIdx.x == 0) { /* shader clock = d(memtime) / d(memrealtime) x 100 MHz */  \
            p.dbg[8 * 4 * 32 + blockIdx.x * 2] = (float)(t - ct0);                                                     \
            p.dbg[8 * 4 * 32 + blockIdx.x * 2 + 1] = (float)(__builtin_amdgcn_s_memrealtime() - rt0);                  \
        }                                                                                                              \
    } while (0)
#else
struct ProfAcc {};
MPCD_DEV uint64_t prof_now() { return 0; }
MPCD_DEV uint64_t prof_realtime() { return 0; }
MPCD_DEV void prof_barrier(ProfAcc &, uint64_t &, int) { lds_barrier(); }
template <class T>
MPCD_DEV void prof_mark(ProfAcc &, uint64_t &, int, const T &) {}
MPCD_DEV void prof_mark(ProfAcc &, uint64_t, int) {}
#define MPCD_PROF_DUMP(W, wave, lane) (void)0
#endif

// Warm start (MlpSampleArgs::x_init non-null): the x the chain starts from, for element quad qd of local candidate gc
// whose noise slice 0 is z. grow = the candidate's row under XINIT_PER_GROUP. Called in the staging loops before the
// step loop, for candidates of the call only (no read of the prior for an idle column).
template <int D0>
MPCD_DEV f32x4 warm_x(const float *x_init, int kind, float sa, float sb, int64_t gc, int64_t grow, int qd, const f32x4 &z)
{
    const int64_t row = kind == XINIT_SHARED ? 0 : kind == XINIT_PER_CAND ? gc : grow;
    return q_sample4(sa, sb, *reinterpret_cast<const f32x4 *>(x_init + (size_t)row * D0 + qd * 4), z);
}

// |v| as an ordered integer: max over these bits is max |v| and propagates a NaN (its magnitude bits
// exceed +inf's), which is what the chain clip test needs (mpcd_sample_args.chain_absmax).
MPCD_DEV uint32_t abs_bits(float v) { return __builtin_bit_cast(uint32_t, v) & 0x7fffffffu; }

// Per-candidate chain |x| maximum: each updating lane has folded the x it read and wrote (x_T .. x_0)
// into am[]; reduce them per candidate in LDS (amx[CPW], zeroed at kernel start) and store.
template <int CPW, int THREADS>
MPCD_DEV void store_chain_absmax(uint32_t *amx, const uint32_t (&am)[2], int cl0, int cl1, bool active, float *out,
                                 int64_t cand0, int64_t batch)
{
    if (active) {
        atomicMax(amx + cl0, am[0]);
        if (cl1 >= 0) atomicMax(amx + cl1, am[1]);
    }
    lds_barrier();
    if (threadIdx.x < CPW && cand0 + threadIdx.x < batch)
        out[cand0 + threadIdx.x] = __builtin_bit_cast(float, amx[threadIdx.x]);
}

}  // namespace mlpc
