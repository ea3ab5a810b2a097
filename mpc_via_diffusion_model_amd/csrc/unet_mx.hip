// U-Net convolutions on the bf16 / f16 matrix cores (MPCD_F32X3 and MPCD_F16 nets).
//
// Same fused op per launch as unet.hip's fp32 conv_kernel (one conv of ResidualTemporalBlock /
// Conv1dBlock / Downsample1d / Upsample1d, layers.py:258-355, with its bias -> GroupNorm -> Mish ->
// + cond / + residual epilogue), but the implicit GEMM runs on v_mfma_f32_16x16x32_{bf16,f16}:
//
//  * MPCD_F32X3 (P = 3 planes): every fp32 operand is split into three bf16 terms (x = x0 + x1 + x2,
//    exact to ~2^-27 relative) and each dot product accumulates the six partial products whose weight
//    is >= 2^-16 of the leading one in fp32 (as mlp_x3.hip): fp32-level GEMM error at the bf16 rate.
//  * MPCD_F16 (P = 1): fp16 operands, fp32 accumulation - BASELINE cfg 5's "fp16 hidden with MFMA GEMM".
//
// A workgroup (4 waves) owns rb whole rows (row = one candidate of one CFG branch). It stages the
// rows' input window in LDS already split into bf16 / f16 planes, channels-last
// [plane][row][position][channel] with a per-position stride whose 16-B count is odd (the 16 lanes of a
// ds_read_b128 quarter hit distinct banks). The output tile [cout] x [rb * lout columns] is cut into
// jobs of NN 16-channel n-tiles x NC 16-column c-tiles; a wave keeps the NN x NC accumulators, reads
// each weight fragment (A, packed per 32-k chunk, streamed from L2 by buffer loads, next chunk in
// flight) once for NC column tiles and each input fragment (B, LDS) once for NN channel tiles. The
// K order is k = tap * cinp + ci, so one lane's 8 k-values are 8 consecutive channels of one tap:
// the B fragment is one 16-byte LDS read. Accumulators start from the bias; the fp32 tile then goes
// through LDS (reusing the staged input when one job per wave suffices) for the GroupNorm statistics
// (fp64, shifted) and the elementwise epilogue, stored coalesced channels-last.
#include <hip/hip_runtime.h>

#include <cmath>

#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <functional>
#include <map>
#include <mutex>
#include <sstream>
#include <tuple>
#include <type_traits>
#include <vector>
#include <string>

#include "mx_common.h"
#include "unet.h"

namespace {

using namespace mx;

constexpr int MT = 256;  // threads per workgroup
// weight chunks in flight for the small f16 tiles (NN x NC <= 8): the GEMM phase of a 4-row block
// streams the whole layer's weights from L2 for 64 columns, so its A loads are latency-bound
constexpr int DA_SMALL = 4;
// 16-byte staging loads / epilogue items each thread keeps in flight
constexpr int SU = 4, EU = 4;
constexpr size_t LDS_CAP = (size_t)160 * 1024;  // dynamic LDS a workgroup may ask for (allow_max_lds): one per CU

// n / d and n % d for small non-negative n (< 2^20) via a float reciprocal + one correction step:
// a handful of VALU ops instead of the ~20-op integer division sequence.
MPCD_DEV int qdiv(int n, int d, float inv_d, int &rem)
{
    int q = (int)((float)n * inv_d);
    int r = n - q * d;
    if (r < 0) { --q; r += d; }
    if (r >= d) { ++q; r -= d; }
    rem = r;
    return q;
}

// Walks the K chunks of one lane quarter q: chunk kc covers, for this lane, 8 consecutive channels
// of one tap (cinp >= 32: 32/cinp... chunks per tap; cinp 8 / 16: 4 / 2 taps per chunk). koff() is
// the byte offset of those 8 channels in the staged window relative to the column's tap-0 position.
struct KWalk {
    int tap, ci0, cpt, tpc, cinp;
    MPCD_DEV void init(int q, int cinp_)
    {
        cinp = cinp_;
        if (cinp >= 32) {
            cpt = cinp >> 5;
            tpc = 0;
            tap = 0;
            ci0 = 8 * q;
        } else {
            cpt = 0;
            tpc = 32 / cinp;
            tap = (8 * q) / cinp;
            ci0 = (8 * q) % cinp;
        }
    }
    MPCD_DEV void next()
    {
        if (cpt) {
            ci0 += 32;
            if (ci0 >= cinp) { ci0 -= cinp; ++tap; }
        } else {
            tap += tpc;
        }
    }
    template <int KIND> MPCD_DEV int koff(int cs) const { return (KIND == UCONV_UP4 ? -tap : tap) * cs + 2 * ci0; }
};

// PERS = false: one row block per workgroup (grid = blocks). PERS = true: a resident grid walks the
// row blocks; while block b runs its GEMM / statistics / epilogue, the 16-byte loads of block b+grid's
// input window are already in flight (registers), and are converted into the (non-aliased) staging
// area once b's GEMM has finished reading it.
constexpr int SUP = 6;  // staging items per thread a persistent workgroup keeps in flight (host-checked)

// The launch's convs: one (NPH = 1), or a ResidualTemporalBlock's two 5-tap convs (NPH = 2): the
// first conv's GroupNorm / Mish / cond epilogue writes its rows straight into the second conv's
// staged planes in LDS (same values the unfused pair would store to HBM and re-stage, so the
// results are bit-identical), and only the block output goes back to HBM.
struct ConvMK2 {
    ConvMK ph[2];
};

template <int KIND, int P, int NN, int NC, bool PERS, int NPH>
__device__ __forceinline__ void conv_mx_body(const ConvMK2 &as)
{
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    static_assert(NPH == 1 || (!PERS && KIND == UCONV_SAME5), "fused pairs: 5-tap convs, one row block per workgroup");
    if constexpr (NPH == 2) {  // zero the halo positions of the second conv's staging window (rows rb)
        const ConvMK &a = as.ph[0];
        const int hp = a.nx_win - a.lout, u16 = a.nx_cs >> 4;  // halo positions per row, 16-B units per position
        const int nrowB = a.nx_win * a.nx_cs, nplaneB = a.rb * nrowB;
        const int n = P * a.rb * hp * u16;
        for (int i = tid; i < n; i += MT) {
            const int u = i % u16, t = i / u16, h = t % hp, rp = t / hp, r = rp % a.rb, pl = rp / a.rb;
            const int pos = h < a.nx_halo_l ? h : a.lout + h;
            *reinterpret_cast<u32x4 *>(sm + a.nx_off + pl * nplaneB + r * nrowB + pos * a.nx_cs + u * 16) =
                u32x4{0u, 0u, 0u, 0u};
        }
    }
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
    const ConvMK &a = as.ph[ph];
    const int win = a.lin + a.halo_l + a.halo_r;
    const int rowB = win * a.cs, planeB = a.rb * rowB;
    const int64_t nblocks = (a.rows + a.rb - 1) / a.rb;
    float *s_stat = reinterpret_cast<float *>(sm + a.stat_off);  // [rb][groups][mean, rstd]
    // [4][coutp]: gn_w, gn_b, cond of the context rows (tproj + shared cproj), cond of the masked rows (tproj)
    float *s_chan = s_stat + 2 * a.rb * 32 + 4;
    if (a.epi != UEPI_BIAS) {
        for (int c = tid; c < a.coutp; c += MT) {
            const bool ok = c < a.cout;
            s_chan[c] = ok ? a.gn_w[c] : 0.f;
            s_chan[a.coutp + c] = ok ? a.gn_b[c] : 0.f;
            float cu = 0.f, cc = 0.f;
            if (ok && a.epi == UEPI_GN_MISH_COND) {
                cu = a.tp[c];
                cc = (a.cp && !a.cp_stride) ? cu + a.cp[c] : cu;
            }
            s_chan[2 * a.coutp + c] = cc;
            s_chan[3 * a.coutp + c] = cu;
        }
    }

    // ---- staging of a row block's input window, split into P planes (zero outside [0, lin), padded
    // channels, rows past the batch)
    const int g8n = a.cinp >> 3, cin = a.ca + a.cb;
    const float inv_g8n = 1.0f / (float)g8n, inv_win = 1.0f / (float)win;
    const int n_items = a.rb * win * g8n;
    // input row of staged row r: rows >= x_rows re-read the first x_rows (CFG's branches share x)
    auto xrow = [&](int64_t r0, int r) {
        int64_t xr = r0 + r;
        while (xr >= a.x_rows) xr -= a.x_rows;
        return xr;
    };
    // one 16-byte item (8 channels of one position of one row): source pointer (or null = zeros), LDS dest
    // activations in HBM: fp32, or (in_h, f16 net only) fp16 - 8 channels = one 16-byte load that is
    // already the staged f16 plane
    const int esh = a.in_h ? 1 : 2;
    auto item = [&](int64_t r0, int nrow, int i, const char *&src, int &dst) {
        int g8, pw;
        const int rp = qdiv(i, g8n, inv_g8n, g8);
        const int r = qdiv(rp, win, inv_win, pw);
        const int p = pw - a.halo_l, ci = 8 * g8;
        dst = r * rowB + pw * a.cs + g8 * 16;
        src = nullptr;
        if (r < nrow && p >= 0 && p < a.lin && ci < cin) {
            const int64_t xr = xrow(r0, r);
            src = ci < a.ca ? reinterpret_cast<const char *>(a.xa) + ((((size_t)xr * a.lin + p) * a.ca + ci) << esh)
                            : reinterpret_cast<const char *>(a.xb) + ((((size_t)xr * a.lin + p) * a.cb + (ci - a.ca)) << esh);
        }
    };
    auto fetch = [&](const char *src, f32x4 &lo, f32x4 &hi) {  // in_h: the 8 halves' bits in lo
        const float *s = src ? reinterpret_cast<const float *>(src) : a.xa;
        lo = ldg4(s);
        hi = a.in_h ? f32x4{0.f, 0.f, 0.f, 0.f} : ldg4(s + 4);
        if (!src) lo = hi = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto put = [&](int dst, const f32x4 &lo, const f32x4 &hi) {
        if (P == 1 && a.in_h) {
            *reinterpret_cast<f32x4 *>(sm + a.in_off + dst) = lo;
            return;
        }
        u32x4 o[P];
        split8<P>(lo, hi, o);
#pragma unroll
        for (int pl = 0; pl < P; ++pl) *reinterpret_cast<u32x4 *>(sm + a.in_off + pl * planeB + dst) = o[pl];
    };
    auto stage_direct = [&](int64_t r0, int nrow) {
        if ((a.ca & 7) == 0 && (a.cb & 7) == 0) {
            // SU items per thread in flight before any conversion or LDS store
            for (int i0 = tid; i0 < n_items; i0 += SU * MT) {
                f32x4 lo[SU], hi[SU];
                int dst[SU];
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    const char *src;
                    item(r0, nrow, min(i0 + u * MT, n_items - 1), src, dst[u]);
                    fetch(src, lo[u], hi[u]);
                }
#pragma unroll
                for (int u = 0; u < SU; ++u)
                    if (i0 + u * MT < n_items) put(dst[u], lo[u], hi[u]);
            }
        } else {  // channel counts not multiples of 8 (the first layer: d channels): scalar loads
            for (int i = tid; i < n_items; i += MT) {
                int g8, pw;
                const int rp = qdiv(i, g8n, inv_g8n, g8);
                const int r = qdiv(rp, win, inv_win, pw);
                const int p = pw - a.halo_l, ci = 8 * g8;
                f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
                if (r < nrow && p >= 0 && p < a.lin) {
                    const int64_t xr = xrow(r0, r);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int c = ci + e;
                        float v = 0.f;
                        if (c < a.ca) v = a.xa[((size_t)xr * a.lin + p) * a.ca + c];
                        else if (c < cin) v = a.xb[((size_t)xr * a.lin + p) * a.cb + (c - a.ca)];
                        if (e < 4) lo[e] = v; else hi[e - 4] = v;
                    }
                }
                put(r * rowB + pw * a.cs + g8 * 16, lo, hi);
            }
        }
    };
    // persistent prefetch: issue (loads into registers) / commit (convert + LDS stores)
    f32x4 pre_lo[PERS ? SUP : 1], pre_hi[PERS ? SUP : 1];
    int pre_dst[PERS ? SUP : 1];
    auto stage_issue = [&](int64_t r0, int nrow) {
#pragma unroll
        for (int u = 0; u < (PERS ? SUP : 1); ++u) {
            const int i = tid + u * MT;
            const char *src;
            item(r0, nrow, min(i, n_items - 1), src, pre_dst[u]);
            if (i >= n_items) pre_dst[u] = -1;
            fetch(src, pre_lo[u], pre_hi[u]);
        }
    };
    auto stage_commit = [&]() {
#pragma unroll
        for (int u = 0; u < (PERS ? SUP : 1); ++u)
            if (pre_dst[u] >= 0) put(pre_dst[u], pre_lo[u], pre_hi[u]);
    };

    // ---- implicit GEMM geometry
    const int NT = a.coutp >> 4, KC = a.kc;
    const int npar = KIND == UCONV_UP4 ? 2 : 1;
    const int nval = KIND == UCONV_UP4 ? a.rb * a.lin : a.rb * a.lout;  // real columns per parity block
    const int ctp = (nval + 15) >> 4, cpar16 = ctp * 16;
    const int npj = (NT + NN - 1) / NN, ncg = (ctp + NC - 1) / NC;
    const int jobs = npj * ncg * npar;
    const int col = lane & 15, q = lane >> 4;
    // pre-norm output tile in LDS, fp32
    using tile_t = float;
    const int sout = a.coutp + 4;
    tile_t *s_out = reinterpret_cast<tile_t *>(sm + a.out_off);
    auto tile_ld4 = [&](const tile_t *p) -> f32x4 { return *reinterpret_cast<const f32x4 *>(p); };

    const uint64_t wa = (uint64_t)a.w;
    const uint32_t wlo = __builtin_amdgcn_readfirstlane((uint32_t)wa), whi = __builtin_amdgcn_readfirstlane((uint32_t)(wa >> 32));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(((uint64_t)whi << 32) | wlo), (short)0, (int)(npar * NT * KC * P * 1024), 0x00020000);
    const int lane16 = lane * 16;

    f32x4 acc[NN][NC];
    auto compute = [&](int job) {
        const int np = job % npj, rest = job / npj, cg = rest % ncg, par = rest / ncg;
        // LDS byte offset of this lane's column window (tap 0 / slot 0, channel 0) per c-tile
        int bb[NC];
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            int cl = (cg * NC + cc) * 16 + col;
            if (cl >= nval) cl = 0;  // padding column: any in-bounds window, never stored
            int r, pos0;
            if (KIND == UCONV_UP4) {
                r = cl / a.lin;
                const int m = cl - r * a.lin;
                pos0 = par == 0 ? m : m + 1;
            } else {
                r = cl / a.lout;
                const int o = cl - r * a.lout;
                pos0 = KIND == UCONV_SAME5 ? o - 2 : KIND == UCONV_DOWN3 ? 2 * o - 1 : o;
            }
            bb[cc] = r * rowB + (pos0 + a.halo_l) * a.cs;
        }
        const int nt0 = np * NN;
#pragma unroll
        for (int j = 0; j < NN; ++j) {
            const int nt = min(nt0 + j, NT - 1);
            const int n = nt * 16 + 4 * q;
            f32x4 b;
#pragma unroll
            for (int e = 0; e < 4; ++e) b[e] = n + e < a.cout ? a.bias[n + e] : 0.f;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) acc[j][cc] = b;
        }
        auto load_a = [&](u32x4 (&A)[NN][P], int kc) {
#pragma unroll
            for (int j = 0; j < NN; ++j) {
                const int nt = min(nt0 + j, NT - 1);
#pragma unroll
                for (int pl = 0; pl < P; ++pl) {
                    const int soff = __builtin_amdgcn_readfirstlane((((par * NT + nt) * KC + kc) * P + pl) * 1024);
                    A[j][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, soff, 0));
                }
            }
        };
        auto load_b = [&](u32x4 (&B)[NC][P], int koff) {
#pragma unroll
            for (int cc = 0; cc < NC; ++cc)
#pragma unroll
                for (int pl = 0; pl < P; ++pl)
                    B[cc][pl] = *reinterpret_cast<const u32x4 *>(sm + a.in_off + pl * planeB + bb[cc] + koff);
        };
        auto mmas = [&](const u32x4 (&A)[NN][P], const u32x4 (&B)[NC][P]) {
#pragma unroll
            for (int i = 0; i < NPROD(P); ++i)
#pragma unroll
                for (int j = 0; j < NN; ++j)
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc)
                        acc[j][cc] = mma<P>(A[j][PA<P>(i)], B[cc][PB<P>(i)], acc[j][cc]);
        };
        // A (weights, L2) runs DA chunks ahead in a register ring; B (LDS) one chunk ahead. The
        // prefetches are unconditional (clamped to the last chunk) so the waits before each chunk's
        // MFMAs leave the younger loads in flight.
        constexpr int DA = P == 1 ? (NN * NC >= 32 ? 2 : NN * NC >= 16 ? 4 : DA_SMALL) : 2;
        u32x4 A[DA][NN][P];
#pragma unroll
        for (int s = 0; s < DA; ++s) load_a(A[s], min(s, KC - 1));
        KWalk kw;
        kw.init(q, a.cinp);
        u32x4 Bc[NC][P], Bn[NC][P];
        load_b(Bc, kw.koff<KIND>(a.cs));
        int kc = 0;
        for (; kc + DA <= KC; kc += DA) {
#pragma unroll
            for (int s = 0; s < DA; ++s) {
                KWalk kn = kw;
                kn.next();
                const bool more = kc + s + 1 < KC;
                load_b(Bn, more ? kn.koff<KIND>(a.cs) : kw.koff<KIND>(a.cs));
                mmas(A[s], Bc);
                load_a(A[s], min(kc + s + DA, KC - 1));
#pragma unroll
                for (int cc = 0; cc < NC; ++cc)
#pragma unroll
                    for (int pl = 0; pl < P; ++pl) Bc[cc][pl] = Bn[cc][pl];
                kw = kn;
            }
        }
#pragma unroll
        for (int s = 0; s < DA - 1; ++s) {  // tail: KC % DA chunks, A[s] holds chunk kc + s
            if (kc + s < KC) {
                KWalk kn = kw;
                kn.next();
                const bool more = kc + s + 1 < KC;
                load_b(Bn, more ? kn.koff<KIND>(a.cs) : kw.koff<KIND>(a.cs));
                mmas(A[s], Bc);
#pragma unroll
                for (int cc = 0; cc < NC; ++cc)
#pragma unroll
                    for (int pl = 0; pl < P; ++pl) Bc[cc][pl] = Bn[cc][pl];
                kw = kn;
            }
        }
    };
    auto store = [&](int job) {
        const int np = job % npj, rest = job / npj, cg = rest % ncg, par = rest / ncg;
#pragma unroll
        for (int j = 0; j < NN; ++j) {
            const int nt = np * NN + j;
            if (nt >= NT) continue;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int ct = cg * NC + cc;
                if (ct >= ctp) continue;
                tile_t *dst = s_out + (size_t)(par * cpar16 + ct * 16 + col) * sout + nt * 16 + 4 * q;
                *reinterpret_cast<f32x4 *>(dst) = acc[j][cc];
            }
        }
    };
    auto colof = [&](int r, int oo) -> int {
        if (KIND == UCONV_UP4) return (oo & 1) * cpar16 + r * a.lin + (oo >> 1);
        return r * a.lout + oo;
    };
    const int epi = a.epi, gsh = a.cpg_shift;  // cpg = cout / groups = 1 << gsh (host-checked, >= 4)

    // ---- GroupNorm statistics per (row, group): fp64, shifted by the group's first value, tpp lanes each
    auto stats = [&](int nrow) {
        const int pairs = nrow * a.groups, nq = a.lout << (gsh - 2);  // channel quads per (row, group)
        // a fixed 4 lanes per (row, group), strided over its quads, then a fixed xor tree: the summation
        // order depends on the layer only, never on rows per workgroup or batch (results are
        // bit-identical however the batch is sharded)
        constexpr int TPP = 4;
        const int sub = tid & (TPP - 1);
        // fp64 sums for the fp32-accurate net; fp32 (shifted) sums for the fp16-operand net (P == 1),
        // whose GEMM operands already carry 2^-11 relative rounding
        using sum_t = typename std::conditional<P == 1, float, double>::type;
        for (int pi = tid / TPP; pi < pairs; pi += MT / TPP) {
            const int r = pi / a.groups, g = pi - r * a.groups;
            const tile_t *base = s_out + (g << gsh);
            const float ref = (float)base[(size_t)colof(r, 0) * sout];
            sum_t s1 = 0, s2 = 0;
            for (int e = sub; e < nq; e += TPP) {
                const int oo = e >> (gsh - 2), cc = (e - (oo << (gsh - 2))) * 4;
                const f32x4 v4 = tile_ld4(base + (size_t)colof(r, oo) * sout + cc);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const sum_t v = (sum_t)v4[k] - (sum_t)ref;
                    s1 += v;
                    s2 += v * v;
                }
            }
#pragma unroll
            for (int m = 1; m < TPP; m <<= 1) {  // the 4 lanes of a pair are consecutive and active together
                s1 += __shfl_xor(s1, m);
                s2 += __shfl_xor(s2, m);
            }
            if (sub == 0) {
                const double n = (double)(nq * 4), ms = (double)s1 / n;
                const double var = fmax((double)s2 / n - ms * ms, 0.0);
                s_stat[2 * pi] = (float)((double)ref + ms);
                s_stat[2 * pi + 1] = (float)(1.0 / sqrt(var + 1e-5));
            }
        }
    };

    // ---- epilogue + store: every thread keeps one channel quad (its GroupNorm affine and cond
    // operands in registers) and walks (row, position) items; one 16-byte load / store per item
    const int cq = (a.cout + 3) >> 2;
    const int q4t = tid % cq, tps = MT / cq;  // cq divides MT (cout <= 256, host-checked)
    const int co_t = 4 * q4t, g_t = co_t >> gsh;
    const float inv_lout = 1.0f / (float)a.lout;
    f32x4 gw_t = {0.f, 0.f, 0.f, 0.f}, gb_t = gw_t, cv0_t = gw_t, cv1_t = gw_t;
    auto epi_setup = [&]() {  // after s_chan is visible
        if (epi != UEPI_BIAS) {
            gw_t = *reinterpret_cast<const f32x4 *>(s_chan + co_t);
            gb_t = *reinterpret_cast<const f32x4 *>(s_chan + a.coutp + co_t);
            cv0_t = *reinterpret_cast<const f32x4 *>(s_chan + 2 * a.coutp + co_t);
            cv1_t = *reinterpret_cast<const f32x4 *>(s_chan + 3 * a.coutp + co_t);
        }
    };
    auto epilogue = [&](int64_t r0, int nrow) {
        const int n_ro = nrow * a.lout;
        // EU items per thread with their residual loads in flight together
        for (int i0 = tid < tps * cq ? tid / cq : n_ro; i0 < n_ro; i0 += EU * tps) {
            f32x4 rv[EU];
            int rr[EU], oo_[EU];
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                const int ro = min(i0 + u * tps, n_ro - 1);  // clamped: a duplicate item is recomputed, not stored
                rr[u] = qdiv(ro, a.lout, inv_lout, oo_[u]);
                if (epi == UEPI_GN_MISH_RES) {
                    const size_t e = ((size_t)(r0 + rr[u]) * a.lout + oo_[u]) * a.cout + co_t;
                    if (a.res_h) {
                        // one f16x4 load + convertvector (bit-casting the two dwords of a u32x2 load
                        // separately compiled to a single-dword load whose halves were reused)
                        const f16x4 h = *reinterpret_cast<const f16x4 *>(reinterpret_cast<const char *>(a.res) + 2 * e);
                        rv[u] = __builtin_convertvector(h, f32x4);
                    } else {
                        rv[u] = ldg4(a.res + e);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                if (i0 + u * tps >= n_ro) break;
                const int r = rr[u], oo = oo_[u];
                const f32x4 raw = tile_ld4(s_out + (size_t)colof(r, oo) * sout + co_t);
                const int64_t grow = r0 + r;
                f32x4 v = raw;
                if (epi != UEPI_BIAS) {
                    const float mean = s_stat[2 * (r * a.groups + g_t)], rstd = s_stat[2 * (r * a.groups + g_t) + 1];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float scale = rstd * gw_t[e];
                        const float shift = -scale * mean + gb_t[e];
                        // Each element's Mish in scalar VALU ops (common.h mish_scalar: packed by hipcc's SLP
                        // vectorizer, this epilogue read v_rcp_f32 results with v_pk_fma_f32 one wait state later
                        // and gave wrong conv outputs on the GPU, profiles/r3_hazard_ab.txt). ~2 % of the kernel.
                        v[e] = mish_scalar(raw[e] * scale + shift);
                    }
                    if (epi == UEPI_GN_MISH_COND) {  // row < b_cand: context branch; else the masked (CFG) branch
                        int64_t cand = grow, br = 0;  // branch = row / b_cand (0: context, 1: masked)
                        while (cand >= a.b_cand) { cand -= a.b_cand; ++br; }
                        f32x4 cv = br == 0 ? cv0_t : cv1_t;
                        if (a.cp && a.cp_stride && br == 0)
                            cv = cv + *reinterpret_cast<const f32x4 *>(a.cp + (size_t)cand * a.cp_stride + co_t);
                        v = v + cv;
                    }
                    if (epi == UEPI_GN_MISH_RES) v = v + rv[u];
                }
                if (NPH == 2 && ph == 0) {  // the second conv's staged planes (cout % 4 == 0, host-checked)
                    u32x2 o[P];
                    split4<P>(v, o);
                    const int nrowB = a.nx_win * a.nx_cs;
                    char *d = sm + a.nx_off + r * nrowB + (oo + a.nx_halo_l) * a.nx_cs + co_t * 2;
#pragma unroll
                    for (int pl = 0; pl < P; ++pl) *reinterpret_cast<u32x2 *>(d + pl * a.rb * nrowB) = o[pl];
                    continue;
                }
                if (a.out_h) {  // fp16 activation (cout % 4 == 0, host-checked)
                    *reinterpret_cast<u32x2 *>(reinterpret_cast<char *>(a.out) + 2 * (((size_t)grow * a.lout + oo) * a.cout + co_t)) =
                        u32x2{pk_f16(v.x, v.y), pk_f16(v.z, v.w)};
                    continue;
                }
                float *dst = a.out + ((size_t)grow * a.lout + oo) * a.cout + co_t;
                if ((a.cout & 3) == 0) {
                    *reinterpret_cast<f32x4 *>(dst) = v;
                } else {
                    for (int e = 0; e < 4 && co_t + e < a.cout; ++e) dst[e] = v[e];
                }
            }
        }
    };

    if constexpr (!PERS) {
        const int64_t r0 = (int64_t)blockIdx.x * a.rb;
        const int nrow = (int)min((int64_t)a.rb, a.rows - r0);
        if (ph == 0) stage_direct(r0, nrow);
        __syncthreads();
        epi_setup();
        if (a.alias) {  // one job per wave (host-checked): finish every read of the staged input first
            if (wave < jobs) compute(wave);
            __syncthreads();
            if (wave < jobs) store(wave);
        } else {
            for (int job = wave; job < jobs; job += MT / 64) {
                compute(job);
                store(job);
            }
        }
        __syncthreads();
        if (epi != UEPI_BIAS) {
            stats(nrow);
            __syncthreads();
        }
        epilogue(r0, nrow);
    } else {  // host: no alias, 16-byte staging, items per thread <= SUP
        int64_t blk = blockIdx.x;
        {
            const int64_t r0 = blk * a.rb;
            stage_issue(r0, (int)min((int64_t)a.rb, a.rows - r0));
            stage_commit();
        }
        __syncthreads();
        epi_setup();
        for (; blk < nblocks; blk += gridDim.x) {
            const int64_t r0 = blk * a.rb;
            const int nrow = (int)min((int64_t)a.rb, a.rows - r0);
            const int64_t nxt = blk + gridDim.x;
            if (nxt < nblocks) stage_issue(nxt * a.rb, (int)min((int64_t)a.rb, a.rows - nxt * a.rb));
            for (int job = wave; job < jobs; job += MT / 64) {
                compute(job);
                store(job);
            }
            __syncthreads();  // staged input fully read, fp32 tile complete
            if (nxt < nblocks) stage_commit();
            if (epi != UEPI_BIAS) stats(nrow);
            __syncthreads();
            epilogue(r0, nrow);
            __syncthreads();  // tile and statistics read before the next block overwrites them
        }
    }
    if (ph + 1 < NPH) __syncthreads();  // the second conv's planes complete; tile / statistics free
    }
}

template <int KIND, int P, int NN, int NC, bool PERS, int NPH>
__global__ __launch_bounds__(MT) void conv_mx_kernel(const ConvMK2 as)
{
    conv_mx_body<KIND, P, NN, NC, PERS, NPH>(as);
}

// ---- host side

uint16_t bf16_rne(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float bf16_f(uint16_t h)
{
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
uint16_t f16_rne(float f)
{
    const _Float16 h = (_Float16)f;  // IEEE round to nearest even
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

int cinp_of(int cin) { return cin <= 8 ? 8 : cin <= 16 ? 16 : (cin + 31) / 32 * 32; }
int ks_of(int kind) { return kind == UCONV_SAME5 ? 5 : kind == UCONV_DOWN3 ? 3 : kind == UCONV_UP4 ? 2 : 1; }

struct Tile {
    int nn, nc;
};
constexpr Tile kTiles3[] = {{2, 4}, {1, 8}, {1, 4}};
constexpr Tile kTiles1[] = {{4, 8}, {2, 8}, {2, 4}, {1, 8}, {1, 4}};

// Workgroups of a kernel that fit one CU at `lds` bytes of dynamic LDS (occupancy query, cached per
// (kernel, lds) under a mutex: launches may come from several host threads).
hipError_t resident_per_cu(const void *fn, size_t lds, int &out)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, size_t>, int> cache;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find({fn, lds});
        if (it != cache.end()) {
            out = it->second;
            return hipSuccess;
        }
    }
    int n = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, MT, lds);
    if (e != hipSuccess) return e;
    out = std::max(n, 1);
    std::lock_guard<std::mutex> g(mu);
    cache[{fn, lds}] = out;
    return hipSuccess;
}

// LDS bytes of the pre-norm output tile (rows x (coutp + pad)), as the kernel lays it out
size_t tile_bytes(size_t rows, int coutp) { return rows * (size_t)(coutp + 4) * 4; }

template <int KIND, int P, int NN, int NC, bool PERS, int NPH = 1>
hipError_t launch_one(const ConvMK2 &k2, size_t lds, hipStream_t st)
{
    const ConvMK &k = k2.ph[0];
    constexpr auto kfn = &conv_mx_kernel<KIND, P, NN, NC, PERS, NPH>;
    auto *fn = reinterpret_cast<const void *>(kfn);
    if (hipError_t e = allow_max_lds<kfn>(); e != hipSuccess) return e;
    int64_t blocks = (k.rows + k.rb - 1) / k.rb;
    if (PERS) {  // a resident grid: workgroups per CU at this kernel's registers and this launch's LDS
        int resident = 1;
        if (hipError_t e = resident_per_cu(fn, lds, resident); e != hipSuccess) return e;
        blocks = std::min<int64_t>(blocks, (int64_t)resident * device_cu_count());
    }
    hipLaunchKernelGGL(kfn, dim3((unsigned)blocks), dim3(MT), lds, st, k2);
    return hipGetLastError();
}

template <int KIND, int P>
hipError_t launch_kind(const ConvMK2 &k, Tile t, bool pers, size_t lds, hipStream_t st)
{
#define T_(A, B)                                                                          \
    if (t.nn == A && t.nc == B)                                                           \
        return pers ? launch_one<KIND, P, A, B, true>(k, lds, st) : launch_one<KIND, P, A, B, false>(k, lds, st);
    if constexpr (P == 3) {
        T_(2, 4) T_(1, 8) T_(1, 4)
    } else {
        T_(4, 8) T_(2, 8) T_(2, 4) T_(1, 8) T_(1, 4)
    }
#undef T_
    return hipErrorInvalidValue;
}

struct MxChoice {
    int rb;
    Tile t;
    int pers;   // persistent grid with the next block's staging loads in flight
    int alias;
    size_t lds;
    int stat_off;  // LDS byte offset of the GroupNorm statistics
    double model;  // issue-model cost per row (ranks the candidates)
};

struct MxKey {
    int kind, planes, ca, cb, cout, lin, lout, epi;
    int64_t rows, x_rows;
    bool operator<(const MxKey &o) const
    {
        return std::tie(kind, planes, ca, cb, cout, lin, lout, epi, rows, x_rows) <
               std::tie(o.kind, o.planes, o.ca, o.cb, o.cout, o.lin, o.lout, o.epi, o.rows, o.x_rows);
    }
};
std::mutex g_mx_mu;
std::map<MxKey, MxChoice> g_mx_cache;  // measured pick per layer shape and batch (process-wide)
// mpcd_unet_force_tiling: -1 = measured picks; conv >= 0: candidate (conv mod count) of every conv launch;
// block -2 = never fuse, >= 0: fused candidate (block mod count) of every fusable block
std::atomic<int> g_force_conv{-1}, g_force_block{-1};
// persistent picks (MPCD_UNET_TUNE_CACHE), defined with the block cache below
void tune_cache_load();
void tune_cache_append(const std::string &line);
void key_write(std::ostringstream &os, const MxKey &k);

bool autotune_on()
{
    static const bool on = [] {
        const char *e = getenv("MPCD_UNET_AUTOTUNE");
        return !(e && e[0] == '0');
    }();
    return on;
}

bool tune_log()  // MPCD_UNET_TUNE_LOG=1: print every measured candidate (stderr)
{
    static const bool on = [] {
        const char *e = getenv("MPCD_UNET_TUNE_LOG");
        return e && e[0] == '1';
    }();
    return on;
}

hipError_t launch_choice(int kind, int planes, ConvMK &k, const MxChoice &ch0, hipStream_t st)
{
    const MxChoice &ch = ch0;
    k.rb = ch.rb;
    k.alias = ch.alias;
    k.stat_off = ch.stat_off;
    k.in_off = 0;
    k.out_off = ch.alias ? 0 : planes * ch.rb * (k.lin + k.halo_l + k.halo_r) * k.cs;
    k.lds_out = 0;
    ConvMK2 k2{};
    k2.ph[0] = k;
#define K_(KD)                                                                        \
    if (kind == KD)                                                                   \
        return planes == 1 ? launch_kind<KD, 1>(k2, ch.t, ch.pers, ch.lds, st)        \
                           : launch_kind<KD, 3>(k2, ch.t, ch.pers, ch.lds, st);
    K_(UCONV_SAME5)
    K_(UCONV_DOWN3)
    K_(UCONV_UP4)
    K_(UCONV_PW1)
#undef K_
    return hipErrorInvalidValue;
}

hipError_t prep_geom(int kind, ConvMK &k, std::string *why)
{
    const int cinp = k.cinp, KC = k.kc;
    const int T = KC * 32 / cinp;  // taps / slots covered by the padded K (zero weights beyond ks)
    if (kind == UCONV_SAME5) {
        k.halo_l = 2;
        k.halo_r = std::max(2, T - 3);
    } else if (kind == UCONV_DOWN3) {
        k.halo_l = 1;
        k.halo_r = std::max(0, T - 3);
    } else if (kind == UCONV_UP4) {
        k.halo_l = std::max(1, T - 1);
        k.halo_r = 1;
    } else {
        k.halo_l = 0;
        k.halo_r = T - 1;
    }
    // per-position stride = 32 mod 64 bytes: each ds_read_b128 lane group of a B-fragment read (16 columns x
    // 4 lane quarters, unet_fused.hip cs_of) covers the 64 banks once
    int cs = (cinp * 2 + 15) / 16 * 16;
    while (cs % 64 != 32) cs += 16;
    k.cs = cs;
    if ((k.in_h || k.res_h || k.out_h) &&
        (cinp != k.cinp || (k.in_h && ((k.ca & 7) || (k.cb & 7))) || (k.out_h && (k.cout & 3)))) {
        if (why) *why = "UNet mx conv: fp16 activations need 8-channel input groups and 4-channel output groups";
        return hipErrorInvalidValue;
    }
    if (k.epi != UEPI_BIAS) {
        const int cpg = k.cout / k.groups;
        int sh = 0;
        while ((1 << sh) < cpg) ++sh;
        if ((1 << sh) != cpg || cpg < 4 || k.groups > 32) {
            if (why) *why = "UNet mx conv: GroupNorm needs a power-of-two group width >= 4 and <= 32 groups";
            return hipErrorInvalidValue;
        }
        k.cpg_shift = sh;
    }
    return hipSuccess;
}

}  // namespace

void unet_pack_mx(int kind, int cin, int cout, int planes, const float *w_host, ConvLayer &L,
                  std::vector<uint16_t> &pack)
{
    const int ks = ks_of(kind), cinp = cinp_of(cin);
    const int coutp = (cout + 15) / 16 * 16, NT = coutp / 16;
    const int KC = (ks * cinp + 31) / 32, npar = kind == UCONV_UP4 ? 2 : 1;
    L.cinp8 = cinp;
    L.kc = KC;
    // planes 2: an exact power-of-two scale with max |w scale| in (2^9, 2^10], so the lo term of every weight of
    // the conv is a normal fp16 (the fused kernel multiplies the accumulator by 1 / scale before the bias)
    float scale = 1.f;
    if (planes == 2) {
        float mx = 0.f;
        const size_t nw = (size_t)cin * cout * (kind == UCONV_UP4 ? 4 : ks);
        for (size_t i = 0; i < nw; ++i) mx = std::max(mx, std::fabs(w_host[i]));
        if (mx > 0.f && mx == mx) {
            int ex;
            std::frexp(mx, &ex);
            int e = 10 - ex;
            if (std::ldexp(mx, e) > 1024.f) --e;
            scale = std::ldexp(1.f, e);
        }
        L.inv2 = 1.f / scale;
    }
    const size_t base = pack.size();
    pack.resize(base + (size_t)npar * NT * KC * planes * 512, 0);
    for (int par = 0; par < npar; ++par)
        for (int nt = 0; nt < NT; ++nt)
            for (int kc = 0; kc < KC; ++kc)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int co = nt * 16 + (lane & 15), k = kc * 32 + 8 * (lane >> 4) + e;
                        const int tap_slot = k / cinp, ci = k - tap_slot * cinp;
                        float v = 0.f;
                        if (co < cout && ci < cin && tap_slot < ks) {
                            if (kind == UCONV_UP4) {
                                // ConvTranspose1d k4 s2 p1: even o = 2m uses taps 1 (input m), 3 (m-1); odd o
                                // uses taps 0 (m+1), 2 (m) - slot 0 / slot 1 in that order
                                const int tap = par == 0 ? (tap_slot == 0 ? 1 : 3) : (tap_slot == 0 ? 0 : 2);
                                v = w_host[((size_t)ci * cout + co) * 4 + tap];
                            } else {
                                v = w_host[((size_t)co * cin + ci) * ks + tap_slot];
                            }
                        }
                        uint16_t t[3] = {0, 0, 0};
                        if (planes == 1) {
                            t[0] = f16_rne(v);
                        } else if (planes == 2) {
                            const float vs = v * scale;
                            t[0] = f16_rne(vs);
                            _Float16 h;
                            memcpy(&h, &t[0], 2);
                            t[1] = f16_rne(vs - (float)h);
                        } else {
                            t[0] = bf16_rne(v);
                            const float r1 = v - bf16_f(t[0]);
                            t[1] = bf16_rne(r1);
                            t[2] = bf16_rne(r1 - bf16_f(t[1]));
                        }
                        for (int pl = 0; pl < planes; ++pl)
                            pack[base + (((((size_t)par * NT + nt) * KC + kc) * planes + pl) * 64 + lane) * 8 + e] =
                                t[pl];
                    }
    if (planes == 2)
        L.wmx2 = reinterpret_cast<const uint16_t *>(base);  // element offset; rebased after upload
    else
        L.wmx = reinterpret_cast<const uint16_t *>(base);
}

hipError_t unet_launch_mx(int kind, int planes, ConvMK &k, hipStream_t st, std::string *why)
{
    hipError_t ge = prep_geom(kind, k, why);
    if (ge != hipSuccess) return ge;
    const int KC = k.kc, cs = k.cs, cinp = k.cinp;
    const int win = k.lin + k.halo_l + k.halo_r;
    const int NT = k.coutp / 16, npar = kind == UCONV_UP4 ? 2 : 1;
    const int nprod = planes == 1 ? 1 : 6;
    const Tile *tiles = planes == 1 ? kTiles1 : kTiles3;
    const int ntiles = planes == 1 ? 5 : 3;
    // Candidates: for each rows-per-workgroup rb, the tile an issue model likes best (MFMA slots of
    // the busiest wave, padding included, + fragment loads + staging). The model does not see
    // occupancy - the LDS of a workgroup decides how many share a CU and hide each other's staging
    // and epilogue latency - so the final pick among the candidates is measured once per layer
    // shape and batch (autotune below), unless MPCD_UNET_AUTOTUNE=0.
    std::vector<MxChoice> cands;
    for (int rb = 32; rb >= 1; rb /= 2) {
        if (rb > 1 && (int64_t)rb > k.rows) continue;
        const int nval = kind == UCONV_UP4 ? rb * k.lin : rb * k.lout;
        const int ctp = (nval + 15) / 16;
        const size_t in_b = (size_t)planes * rb * win * cs;
        const size_t out_b = tile_bytes((size_t)npar * ctp * 16, k.coutp);
        const size_t stat_b = (size_t)(2 * rb * 32 + 4) * 4 + (size_t)4 * k.coutp * 4;
        MxChoice best{};
        for (int ti = 0; ti < ntiles; ++ti) {
            const Tile t = tiles[ti];
            const int jobs = ((NT + t.nn - 1) / t.nn) * ((ctp + t.nc - 1) / t.nc) * npar;
            const int alias = jobs <= MT / 64;
            const size_t body = alias ? std::max(in_b, out_b) : in_b + out_b;
            const size_t lds = body + stat_b;
            if (lds > LDS_CAP) continue;
            const int per_wave = (jobs + 3) / 4;
            const double cyc = (double)per_wave * KC *
                                   (t.nn * t.nc * nprod * 16.0 + t.nn * planes * 24.0 + t.nc * planes * 8.0) +
                               (double)in_b / 64.0 + 600.0;
            const double cost = cyc / rb;
            if (!best.rb || cost < best.model * 0.999) best = MxChoice{rb, t, 0, alias, lds, (int)body, cost};
        }
        if (best.rb) cands.push_back(best);
        // persistent form of the same tile: staging and fp32 tile side by side (no alias), every
        // thread's staging items fit the in-flight registers
        if (best.rb && (k.ca & 7) == 0 && (k.cb & 7) == 0 && (int64_t)rb * 4 < k.rows) {
            const int items = rb * win * (cinp / 8);
            const size_t lds = in_b + out_b + stat_b;
            if ((items + MT - 1) / MT <= SUP && lds <= LDS_CAP)
                cands.push_back(MxChoice{rb, best.t, 1, 0, lds, (int)(in_b + out_b), best.model * 1.0001});
        }
    }
    if (cands.empty()) {
        if (why) *why = "UNet mx conv: no tiling fits LDS";
        return hipErrorInvalidValue;
    }
    std::sort(cands.begin(), cands.end(), [](const MxChoice &x, const MxChoice &y) { return x.model < y.model; });

    const MxKey key{kind, planes, k.ca, k.cb, k.cout, k.lin, k.lout, k.epi, k.rows, k.x_rows};
    MxChoice pick = cands[0];
    bool have = false;
    if (int f = g_force_conv.load(); f >= 0) {  // forced candidate (tests: every tiling gives the same bits)
        const MxChoice &ch = cands[f % cands.size()];
        return launch_choice(kind, planes, k, ch, st);
    }
    {
        std::lock_guard<std::mutex> g(g_mx_mu);
        tune_cache_load();
        auto it = g_mx_cache.find(key);
        if (it != g_mx_cache.end()) {
            pick = it->second;
            have = true;
        }
    }
    // re-running a conv is idempotent unless it writes one of its inputs
    const bool in_place = k.out == k.xa || (k.xb && k.out == k.xb) || (k.res && k.out == k.res);
    hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
    if (!have && cands.size() > 1 && autotune_on() && !in_place && hipStreamIsCapturing(st, &cap_st) == hipSuccess &&
        cap_st == hipStreamCaptureStatusNone) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            float best_ms = 1e30f;
            for (const MxChoice &ch : cands) {
                ConvMK kk = k;
                if (launch_choice(kind, planes, kk, ch, st) != hipSuccess) continue;  // warm-up (weights into L2)
                (void)hipEventRecord(e0, st);
                for (int r = 0; r < 2; ++r) (void)launch_choice(kind, planes, kk, ch, st);
                (void)hipEventRecord(e1, st);
                float ms = 0.f;
                if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) continue;
                if (tune_log())
                    fprintf(stderr, "[mx tune] kind %d P%d cin %d+%d cout %d L %d->%d epi %d rows %lld: rb %d tile %dx%d %s %.1f us\n",
                            kind, planes, k.ca, k.cb, k.cout, k.lin, k.lout, k.epi, (long long)k.rows, ch.rb, ch.t.nn,
                            ch.t.nc, ch.pers ? "pers" : ch.alias ? "alias" : "tile", ms * 500.f);
                if (ms < best_ms) {
                    best_ms = ms;
                    pick = ch;
                }
            }
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipGetLastError();
        std::lock_guard<std::mutex> g(g_mx_mu);
        g_mx_cache[key] = pick;
        std::ostringstream os;
        os << "mx ";
        key_write(os, key);
        os << " : " << pick.rb << ' ' << pick.t.nn << ' ' << pick.t.nc << ' ' << pick.pers << ' ' << pick.alias << ' '
           << pick.lds << ' ' << pick.stat_off;
        tune_cache_append(os.str());
    }
    return launch_choice(kind, planes, k, pick, st);
}

// ---- fused ResidualTemporalBlock (NPH = 2)

namespace {

struct RtbChoice {
    int fused;  // 0: the two convs as separate launches (their own measured picks)
    int rb;
    Tile t;
    size_t lds;
    int x_off;     // LDS byte offset of the second conv's staged planes
    int stat_off;  // LDS byte offset of the statistics / per-channel table
    double model;
};

struct RtbKey {
    MxKey a, b;
    bool operator<(const RtbKey &o) const { return a < o.a || (!(o.a < a) && b < o.b); }
};
std::map<RtbKey, RtbChoice> g_rtb_cache;

// MPCD_UNET_TUNE_CACHE=<file>: the measured picks persist across processes (loaded on first use, every
// new pick appended), so a profiling run and the bench use the same tilings and a service skips the
// autotune on start-up. One line per pick: "mx <key> : <choice>" / "rtb <key1> <key2> : <choice>".
const char *tune_cache_path()
{
    static const char *p = [] {
        const char *e = getenv("MPCD_UNET_TUNE_CACHE");
        return e && e[0] ? e : nullptr;
    }();
    return p;
}
void key_read(std::istringstream &is, MxKey &k)
{
    long long r, xr;
    is >> k.kind >> k.planes >> k.ca >> k.cb >> k.cout >> k.lin >> k.lout >> k.epi >> r >> xr;
    k.rows = r;
    k.x_rows = xr;
}
void key_write(std::ostringstream &os, const MxKey &k)
{
    os << k.kind << ' ' << k.planes << ' ' << k.ca << ' ' << k.cb << ' ' << k.cout << ' ' << k.lin << ' ' << k.lout << ' '
       << k.epi << ' ' << (long long)k.rows << ' ' << (long long)k.x_rows;
}
void tune_cache_load()  // under g_mx_mu
{
    static bool done = false;
    if (done || !tune_cache_path()) return;
    done = true;
    std::ifstream f(tune_cache_path());
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string tag, colon;
        is >> tag;
        if (tag == "mx") {
            MxKey k{};
            MxChoice c{};
            key_read(is, k);
            size_t lds;
            is >> colon >> c.rb >> c.t.nn >> c.t.nc >> c.pers >> c.alias >> lds >> c.stat_off;
            c.lds = lds;
            if (is && colon == ":") g_mx_cache[k] = c;
        } else if (tag == "rtb") {
            RtbKey k{};
            RtbChoice c{};
            key_read(is, k.a);
            key_read(is, k.b);
            size_t lds;
            is >> colon >> c.fused >> c.rb >> c.t.nn >> c.t.nc >> lds >> c.x_off >> c.stat_off;
            c.lds = lds;
            if (is && colon == ":") g_rtb_cache[k] = c;
        }
    }
}
void tune_cache_append(const std::string &line)  // under g_mx_mu
{
    if (!tune_cache_path()) return;
    std::ofstream f(tune_cache_path(), std::ios::app);
    f << line << '\n';
}

template <int P>
hipError_t launch_fused(const ConvMK2 &k2, Tile t, size_t lds, hipStream_t st)
{
#define T_(A, B) \
    if (t.nn == A && t.nc == B) return launch_one<UCONV_SAME5, P, A, B, false, 2>(k2, lds, st);
    if constexpr (P == 3) {
        T_(2, 4) T_(1, 8) T_(1, 4)
    } else {
        T_(4, 8) T_(2, 8) T_(2, 4) T_(1, 8) T_(1, 4)
    }
#undef T_
    return hipErrorInvalidValue;
}

// LDS: [first conv's staged planes | its fp32 tile] (the second conv's fp32 tile reuses the start),
// then the second conv's staged planes at x_off, then the statistics / per-channel table.
hipError_t launch_rtb_choice(int planes, const ConvMK &k1, const ConvMK &k2, const RtbChoice &ch, hipStream_t st)
{
    ConvMK2 kk{};
    kk.ph[0] = k1;
    kk.ph[1] = k2;
    for (int i = 0; i < 2; ++i) {
        ConvMK &k = kk.ph[i];
        k.rb = ch.rb;
        k.alias = 0;
        k.stat_off = ch.stat_off;
        k.lds_out = i == 0;
    }
    kk.ph[0].in_off = 0;
    kk.ph[0].out_off = planes * ch.rb * (k1.lin + k1.halo_l + k1.halo_r) * k1.cs;
    kk.ph[0].nx_off = ch.x_off;
    kk.ph[0].nx_cs = k2.cs;
    kk.ph[0].nx_win = k2.lin + k2.halo_l + k2.halo_r;
    kk.ph[0].nx_halo_l = k2.halo_l;
    kk.ph[1].in_off = ch.x_off;
    kk.ph[1].out_off = 0;
    return planes == 1 ? launch_fused<1>(kk, ch.t, ch.lds, st) : launch_fused<3>(kk, ch.t, ch.lds, st);
}

}  // namespace

void unet_force_tiling(int conv, int block)
{
    g_force_conv.store(conv < 0 ? -1 : conv);
    g_force_block.store(block < -2 ? -1 : block);
}

hipError_t unet_launch_mx_rtb(int planes, ConvMK &k1, ConvMK &k2, hipStream_t st, std::string *why)
{
    auto unfused = [&]() -> hipError_t {
        hipError_t e = unet_launch_mx(UCONV_SAME5, planes, k1, st, why);
        return e != hipSuccess ? e : unet_launch_mx(UCONV_SAME5, planes, k2, st, why);
    };
    const char *fe = getenv("MPCD_UNET_FUSE");  // 0: never fuse, 1: fuse whenever a tiling fits, unset: measured
    const int mode = fe && fe[0] ? atoi(fe) : -1;
    const int fb = g_force_block.load();
    if (mode == 0 || fb == -2 || (fb == -1 && g_force_conv.load() >= 0)) return unfused();
    hipError_t e = prep_geom(UCONV_SAME5, k1, why);
    if (e == hipSuccess) e = prep_geom(UCONV_SAME5, k2, why);
    if (e != hipSuccess) return e;
    const bool fusable = k1.epi != UEPI_BIAS && k2.epi != UEPI_BIAS && k1.lout == k2.lin && k2.ca == k1.cout &&
                         k2.cb == 0 && k2.cinp == k1.cout && k2.cout == k1.cout && k2.coutp == k1.coutp &&
                         (k1.cout & 3) == 0 && k2.rows == k1.rows;
    if (!fusable) return unfused();

    const int win1 = k1.lin + k1.halo_l + k1.halo_r, win2 = k2.lin + k2.halo_l + k2.halo_r;
    const int NT = k1.coutp / 16, nprod = planes == 1 ? 1 : 6;
    const Tile *tiles = planes == 1 ? kTiles1 : kTiles3;
    const int ntiles = planes == 1 ? 5 : 3;
    std::vector<RtbChoice> cands;
    for (int rb = 32; rb >= 1; rb /= 2) {
        if (rb > 1 && (int64_t)rb > k1.rows) continue;
        const int ctp = (rb * k1.lout + 15) / 16;
        const size_t in1 = (size_t)planes * rb * win1 * k1.cs, in2 = (size_t)planes * rb * win2 * k2.cs;
        const size_t out_b = tile_bytes((size_t)ctp * 16, k1.coutp);
        const size_t stat_b = (size_t)(2 * rb * 32 + 4) * 4 + (size_t)4 * k1.coutp * 4;
        const size_t x_off = in1 + out_b;  // >= out_b: the second tile fits in front of x_off
        const size_t lds = x_off + in2 + stat_b;
        if (lds > LDS_CAP) continue;
        RtbChoice best{};
        for (int ti = 0; ti < ntiles; ++ti) {
            const Tile t = tiles[ti];
            const int jobs = ((NT + t.nn - 1) / t.nn) * ((ctp + t.nc - 1) / t.nc);
            const int per_wave = (jobs + 3) / 4;
            const double cyc = (double)per_wave * (k1.kc + k2.kc) *
                                   (t.nn * t.nc * nprod * 16.0 + t.nn * planes * 24.0 + t.nc * planes * 8.0) +
                               (double)in1 / 64.0 + 1200.0;
            const double cost = cyc / rb;
            if (!best.rb || cost < best.model * 0.999)
                best = RtbChoice{1, rb, t, lds, (int)x_off, (int)(x_off + in2), cost};
        }
        if (best.rb) cands.push_back(best);
    }
    if (cands.empty()) return unfused();
    std::sort(cands.begin(), cands.end(), [](const RtbChoice &x, const RtbChoice &y) { return x.model < y.model; });

    auto key_of = [&](const ConvMK &k) {
        return MxKey{UCONV_SAME5, planes, k.ca, k.cb, k.cout, k.lin, k.lout, k.epi, k.rows, k.x_rows};
    };
    const RtbKey key{key_of(k1), key_of(k2)};
    if (fb >= 0) return launch_rtb_choice(planes, k1, k2, cands[fb % cands.size()], st);
    RtbChoice pick = cands[0];
    bool have = false;
    {
        std::lock_guard<std::mutex> g(g_mx_mu);
        tune_cache_load();
        auto it = g_rtb_cache.find(key);
        if (it != g_rtb_cache.end()) {
            pick = it->second;
            have = true;
        }
    }
    const bool in_place = k2.out == k1.xa || (k1.xb && k2.out == k1.xb) || (k2.res && k2.out == k2.res) ||
                          k1.out == k1.xa || (k1.xb && k1.out == k1.xb) || (k2.res && k1.out == k2.res);
    hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
    if (!have && mode < 0 && autotune_on() && !in_place && hipStreamIsCapturing(st, &cap_st) == hipSuccess &&
        cap_st == hipStreamCaptureStatusNone) {
        // measured against the unfused pair (each conv already on its own measured pick)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            float best_ms = 1e30f;
            auto timed = [&](const std::function<hipError_t()> &run) -> float {
                if (run() != hipSuccess) return 1e30f;  // warm-up (and first-use tuning of the unfused convs)
                (void)hipEventRecord(e0, st);
                for (int r = 0; r < 2; ++r) (void)run();
                (void)hipEventRecord(e1, st);
                float ms = 0.f;
                if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return 1e30f;
                return ms;
            };
            const float ms_unf = timed(unfused);
            if (ms_unf < best_ms) {
                best_ms = ms_unf;
                pick = RtbChoice{};
            }
            if (tune_log())
                fprintf(stderr, "[rtb tune] P%d cin %d+%d cout %d L %d rows %lld: unfused %.1f us\n", planes, k1.ca, k1.cb,
                        k1.cout, k1.lin, (long long)k1.rows, ms_unf * 500.f);
            for (const RtbChoice &ch : cands) {
                const float ms = timed([&] { return launch_rtb_choice(planes, k1, k2, ch, st); });
                if (tune_log())
                    fprintf(stderr, "[rtb tune]   fused rb %d tile %dx%d %.1f us\n", ch.rb, ch.t.nn, ch.t.nc, ms * 500.f);
                if (ms < best_ms) {
                    best_ms = ms;
                    pick = ch;
                }
            }
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipGetLastError();
        std::lock_guard<std::mutex> g(g_mx_mu);
        g_rtb_cache[key] = pick;
        std::ostringstream os;
        os << "rtb ";
        key_write(os, key.a);
        os << ' ';
        key_write(os, key.b);
        os << " : " << pick.fused << ' ' << pick.rb << ' ' << pick.t.nn << ' ' << pick.t.nc << ' ' << pick.lds << ' '
           << pick.x_off << ' ' << pick.stat_off;
        tune_cache_append(os.str());
    }
    if (mode == 1 && !pick.fused) pick = cands[0];
    if (!pick.fused) return unfused();
    return launch_rtb_choice(planes, k1, k2, pick, st);
}
