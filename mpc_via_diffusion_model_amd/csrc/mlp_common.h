// Shared pieces of the two MLP sampler kernels (mlp_sampler.hip: exact-f32 MFMA; mlp_x3.hip:
// fp32-accurate 3-way bf16 split MFMA). Net = build-defined CFG MLP, SURVEY §8a A11.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
};
template <int CPW, bool GRP>
MPCD_DEV CandSpan cand_span(const float *cproj, int64_t group, int32_t group_wgs)
{
    if constexpr (!GRP) {
        return CandSpan{(int64_t)blockIdx.x * CPW, 0, cproj};
    } else {
        const uint32_t m = __builtin_amdgcn_readfirstlane(blockIdx.x / (uint32_t)group_wgs);
        const uint32_t j = blockIdx.x - m * (uint32_t)group_wgs;
        const int64_t left = group - (int64_t)j * CPW;  // >= 1: j < ceil(group / CPW)
        return CandSpan{(int64_t)m * group + (int64_t)j * CPW, left < CPW ? (int32_t)left : CPW,
                        cproj + (size_t)m * COND_TOTAL};
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
