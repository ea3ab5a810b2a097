// Persistent CFG-DDPM / DDIM sampler for the MLP noise-net, fp32-accurate split-bf16
// GEMMs, with the three 128x128 layers' weights RESIDENT in registers for the whole launch.
//
// Why (profiles/r3_mlp_vmem_ab.txt): the streaming kernel (mlp_x3.hip) re-reads every
// layer's three-plane weights from L2 each denoise step, 888 KB per CU per step, and that per-CU
// vector-memory stream - not L2 bandwidth, not MFMA - sets its step time. A CU's register file is
// 512 KiB (4 SIMDs x 512 registers x 64 lanes x 4 B): with one wave per SIMD (4 waves, 512 registers
// each) the 288 KiB of Linear 5/6/7 (K = N = 128; wave w owns n-tiles w and w + 4: 24 fragments of
// 16 B per lane per layer) stay in registers across all denoise steps - 63 fragments in AGPRs, read
// directly as the MFMA A operand, 9 in VGPRs. Every other layer streams once per CU per step (each
// fragment loaded by the one wave that uses it, except the N = 32 layers at 32 rows, split by column
// tile: 324 KB per CU per step instead of 888).
//
// Same pack, LDS layout, layer order, MFMA order (six partial products of each 32-k chunk, smallest
// first, k-chunks in order, accumulators initialised from the bias / cond tables), Mish, split and
// denoise update as mlp_x3_kernel, so its results are bit-identical to the streaming kernel's
// (tests/test_gpu_mlp.py checks it).
//
// The 8-wave form (layout rw32x8, W = 8: two waves per SIMD, 32 rows) splits each layer's n-tiles over twice the
// waves, keeps Linear 5, 6 and half of Linear 7 resident (120 AGPRs of a wave's 256 registers), streams the rest
// one layer ahead, and has waves 4-7, idle in the 32-wide layers, draw the noise. Bit-identical to the 4-wave form
// (tests/test_gpu_mlp_rw8.py). Measured against rw32, alternating on one box (profiles/rw8_ab.txt): kernel 1.069 vs
// 1.084 ms at cfg2 (0.986x), 4.246 vs 4.313 ms at 16,384 candidates (0.984x) - a small gain, far from the 0.90x hoped
// for: the two waves of a SIMD run each layer in lock step between the same workgroup barriers (MFMA busy 0.34 of
// the shader cycles per SIMD, as before), so the matrix pipe's idle time is mostly shared, not filled. It is the
// default wherever rw32 was. It has an LDS layout of its own (Lds8, below) that keeps the last three k-chunks of Linear
// 8's weights in LDS for the whole launch (profiles/rw8_l8_lds_ab.txt: kernel 0.980x).
#include <hip/hip_runtime.h>

#include "mlp_x3.h"

namespace {
using namespace mlpx3;
static_assert(WPL == 3, "mlp_rw streams the three-plane pack");

constexpr int RW_W = 4;           // waves per workgroup (one per SIMD, 512 registers each)
constexpr int RW_T = 64 * RW_W;   // threads
constexpr int RES_L0 = 5;         // resident layers 5, 6, 7
constexpr int RES_NL = 3;
constexpr int RES_G = RES_NL * 2 * 4;  // groups (layer, n-tile j, k-chunk) of 3 plane fragments per wave: 24
constexpr int RES_AG = 21;             // groups 0..20 resident in AGPRs (63 fragments, 252 registers); the
                                       // last three (layer 7, n-tile w + 4, k-chunks 1-3) stream each step
// The 8-wave form (rw32x8: two waves per SIMD, 256 registers each, at most 128 of them AGPRs): wave w owns n-tile
// w of the 128-wide layers, 12 groups; Linear 5, 6 and k-chunks 0-1 of Linear 7 are resident (30 fragments, 120
// AGPRs), k-chunks 2-3 of Linear 7 stream each step. Waves w and w + 4 share a SIMD.
constexpr int RES_AG8 = 10;

// Transcendental pairs for packed consumers: both issued, then 2 wait states before a packed op may read them (a
// packed read one wait state behind a v_exp / v_rcp gave wrong results on gfx950: unet_fused.hip exp2_pair,
// profiles/r3_hazard_ab.txt). The same instructions as __builtin_amdgcn_exp2f / rcpf: the same bits.
MPCD_DEV f32x2 exp2_pair(f32x2 z)
{
    float a, b;
    asm("v_exp_f32 %0, %2\n\tv_exp_f32 %1, %3\n\ts_nop 1" : "=&v"(a), "=&v"(b) : "v"(z[0]), "v"(z[1]));
    return f32x2{a, b};
}
MPCD_DEV f32x2 rcp_pair(f32x2 x)
{
    float a, b;
    asm("v_rcp_f32 %0, %2\n\tv_rcp_f32 %1, %3\n\ts_nop 1" : "=&v"(a), "=&v"(b) : "v"(x[0]), "v"(x[1]));
    return f32x2{a, b};
}
MPCD_DEV f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// partial product m of a 32-k chunk, smallest first (mlp_x3.h mfma_x3): weight plane, activation plane
constexpr int wpl(int m) { return m == 0 ? 2 : (m == 1 || m == 3) ? 1 : 0; }
constexpr int xpl(int m) { return (m == 0 || m == 3 || m == 5) ? 0 : (m == 1 || m == 4) ? 1 : 2; }

// One partial product with the weight plane in an AGPR. The compiler's hazard pass does not see an MFMA in an
// asm statement, so its waits are written here: FIRST (the chain's first product), 2 wait states for a VALU
// write of the accumulator just before; LAST (the chain's last product), 8 wait states after it, before any
// VALU op may read the result (what hipcc inserts after the builtin v_mfma_f32_16x16x32_bf16 on gfx950).
// Inside a chain the accumulator goes MFMA to MFMA (srcC forwarding, no wait). tests/test_isa.py checks both
// rules on every MFMA of the library.
template <bool FIRST, bool LAST>
MPCD_DEV f32x4 mfma_agpr1(const u32x4 &w, const u32x4 &x, f32x4 acc)
{
    if constexpr (FIRST && LAST)
        asm("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n\ts_nop 7" : "+v"(acc) : "a"(w), "v"(x));
    else if constexpr (FIRST)
        asm("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(x));
    else if constexpr (LAST)
        asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n\ts_nop 7" : "+v"(acc) : "a"(w), "v"(x));
    else
        asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(x));
    return acc;
}

// LDS layout of the 8-wave form: Lds3's buffers, strides and tables, with storage shared between live ranges that never
// meet, and the bytes that frees given to W8L, where the trailing KL k-chunks of Linear 8's weights (all N / 16 n-tiles,
// three planes, 1 KB per fragment as the pack stores it: 64 lanes x 16 B, so a ds_read_b128 of lane * 16 is
// conflict-free) stay for the whole launch. Linear 8 was the one layer whose own fragments were still being loaded from
// L2 while it ran, each of them twice per CU (waves w and w + 4 hold the same n-tile).
//  - S1 lies inside C0, behind the noise hand-over block (NZT x 4 KB). Both bases are multiples of 256 B, as in Lds3:
//    bank and swizzle of every access are unchanged. S1 is written by the update (x planes, behind the final layer's
//    barrier), Linear 1's and Linear 11's epilogues, and read by Linear 0, 2 and 12. C0 is written by Linear 5's and
//    Linear 7's epilogues and, in the hand-over block only, by waves 4-7 during Linear 10; it is read by Linear 6,
//    Linear 8 and take_noise (before the final layer's barrier). In step order: S1 [update, L0, L1, L2], C0 [L5 .. L8],
//    hand-over block [L10 .. take_noise], S1 [L11, L12, update]. Linear 2's reads end before Linear 3's barrier and
//    Linear 5's epilogue starts behind Linear 5's (two barriers between); Linear 8's reads end before Linear 9's
//    barrier and Linear 11's epilogue starts behind Linear 11's (two between); the step boundary lies inside S1's own
//    range. The hand-over block is not part of S1, so its range may overlap S1's.
//  - XB (fp32 x) where XREG holds is written and read only before the step loop (x_T -> load_xr): it lies in T1, first
//    written by Linear 0's epilogue behind the loop's first barrier, which load_xr's reads precede.
template <int D0, int NB, int ROWS>
struct Lds8 : Lds3<D0, NB, ROWS> {
    using B3 = Lds3<D0, NB, ROWS>;
    static constexpr int NZT = (D0 / 16 + 3) / 4;                            // MlpRw::NZT at W = 8
    static constexpr bool XREG = NZT * (NB == 2 ? 1 : ROWS / 16) == 1;        // MlpRw::XREG at W = 8
    static constexpr int PL = B3::PL, PL2 = B3::PL2;
    static constexpr int T1 = 0;
    static constexpr int C1 = T1 + 3 * PL;
    static constexpr int C0 = C1 + 3 * PL;
    static constexpr int S1 = C0 + NZT * 4096;
    static_assert(S1 % 256 == 0 && C0 % 256 == 0 && S1 + 3 * PL <= C0 + 3 * PL2, "S1 inside C0, behind the noise block");
    static constexpr int XB = XREG ? T1 : C0 + 3 * PL2;
    static_assert(B3::CPW * B3::SX * 4 <= 3 * PL, "the fp32 x_T fits T1");
    static constexpr int TPC = C0 + 3 * PL2 + (XREG ? 0 : B3::CPW * B3::SX * 4);
    static constexpr int TPU = TPC + COND_TOTAL * 4;
    static constexpr int BIC = TPU + COND_TOTAL * 4;
    static constexpr int CPS = BIC + COND_TOTAL * 4;
    static constexpr int BI = CPS + COND_TOTAL * 4;
    static constexpr int AMX = BI + Arch<D0>::btotal() * 4;
    static constexpr int W8L = (AMX + ROWS * 4 + 255) / 256 * 256;
    // Linear 8: k-chunks KS .. KC8 - 1 resident. All or nothing at three k-chunks: the k-chunks that stay streamed are
    // all in registers when the layer starts, and 256 registers per wave hold five of them, not six.
    static constexpr int KC8 = Arch<D0>::K[8] / 32, NT8 = Arch<D0>::N[8] / 16, CHUNK = NT8 * 3 * 1024;
    static constexpr int KL = (160 * 1024 - W8L) / CHUNK >= 3 ? 3 : 0;
    static constexpr int KS = KC8 - KL;
    static constexpr int total = W8L + KL * CHUNK;
    static_assert(total <= 160 * 1024, "LDS budget (160 KiB per CU)");

    static constexpr int in_off(int l) {
        constexpr int t[NLAYER] = {S1, T1, S1, T1, C1 + 128, T1, C0 + 256, T1, C0, T1, C1, T1, S1, T1};
        return t[l];
    }
    static constexpr int out_off(int l) {
        constexpr int t[NLAYER] = {T1, S1, T1, C1 + 128, T1, C0 + 256, T1, C0, T1, C1, T1, S1, T1, 0};
        return t[l];
    }
};

// W = 4: one wave per SIMD (rw32 / rw16). W = 8: two per SIMD, 32 rows (rw32x8), the same sums in the same
// order; only which wave computes a pass, and when, differs.
// GRP: the grouped-context form (mlp_rw_grouped_kernel; see cand_span), a CTX instantiation of its own.
template <int D0, int SMODE, bool CTX, int R, int W = RW_W, bool GRP = false>
struct MlpRw {
    static_assert(CTX || !GRP, "grouped contexts need a context");
    static constexpr int NB = (SMODE == MODE_DDIM || SMODE == MODE_EPS1) ? 1 : 2;
    static constexpr bool IS_DDPM = SMODE == MODE_DDPM_CFG || SMODE == MODE_DDPM_XN;
    static_assert(R == 32 || R == 16, "32 or 16 rows per workgroup");
    static_assert(W == 4 || (W == 8 && R == 32), "4 waves, or 8 waves at 32 rows");
    static constexpr int NTH = 64 * W;      // threads
    // k-chunks of operand fragments read ahead of the MFMAs in hidden_ilv (a ring of PF + 1). W = 4: 2. W = 8: 1, the
    // partner wave of the SIMD covers LDS latency too (2 measured 0.7 % slower at 16,384 candidates and the same at
    // 4,096, profiles/rw8_ab.txt; at H*d = 128 it spills)
    static constexpr int PF = W == 8 ? 1 : 2;
    // W = 8 at H*d = 128 (Linear 0's 12 fragments, two update quads per lane): the next step's Linear 0 fragments
    // issued after the update, or the kernel spills
    static constexpr bool W0_LATE = D0 == 128;
    static constexpr int TPL = 8 / W;       // n-tiles of a 128-wide layer per wave
    static constexpr int NRG = RES_NL * TPL * 4;          // groups (layer, n-tile j, k-chunk) per wave
    static constexpr int NAG = W == 8 ? RES_AG8 : RES_AG;  // of them resident in AGPRs
    static_assert(W == 8 || NRG == RES_G);
    static constexpr int NCT = R / 16;  // 16-row column tiles
    using A = Arch<D0>;
    // W = 8: a layout of its own (Lds8), with Linear 8's last KL k-chunks of weights resident in LDS
    using L = std::conditional_t<W == 8, Lds8<D0, NB, R>, Lds3<D0, NB, R>>;
    static constexpr int CPW = L::CPW;
    static constexpr int QUADS = D0 / 4;

    // Row swizzle of every activation plane (as mlp_h2.hip's Lds2): in rows with bit 2 set the 16-byte units are
    // swapped in pairs (byte offset b -> b ^ 16). The B-fragment reads (ds_read_b128 of whole units, lane (col, q)
    // reading unit q ^ s of its row) stay conflict-free; the epilogue's ds_write_b64 of 16 rows at one feature
    // offset (one lane group, banks mod 32) drop from 4-way to 2-way bank conflicts - 2-way is that pattern's
    // floor (16 rows on the 8 unit positions of 128 bytes). s = bit 2 of the row = bit 2 of the lane's column in
    // every layout here (rows ct * 16 + col, or the candidate col / col & 7 of the shared layer-0 input).
    static MPCD_DEV int swz(int r) { return (r >> 2) & 1; }
    // byte offset in its row of the 4 features n..n+3 (n = 16 nt + 4 q) an epilogue lane of quarter q stores
    static MPCD_DEV int st_off(int n, int q, int row) { return n * 2 - 8 * q + 8 * (q ^ (swz(row) << 1)); }

    // R = 16 with CFG: columns 0-7 are the context rows of candidates 0-7, 8-15 their masked rows
    static MPCD_DEV int cand_of(int ct, int col) { return NB == 2 ? (R == 16 ? (col & 7) : col) : ct * 16 + col; }
    static MPCD_DEV bool masked_of(int ct, int col) { return NB == 2 && (R == 16 ? col >= 8 : ct == 1); }

    // Layer l's work per wave. N = 32 at 32 rows (SPL): wave w -> n-tile w & 1, column tile w >> 1. Otherwise
    // wave w -> n-tiles w + 4j (j < T) for every column tile; a wave with no tile (N = 32 at 16 rows) loads
    // a clamped copy and computes nothing.
    //
    // W = 8, hidden layers (one pass or two per wave, T = 1): N = 128: wave w -> n-tile w, both column tiles (waves
    // 4-7 in the opposite order: a phase offset between the two waves of a SIMD, which otherwise reach MFMAs, epilogue
    // and barrier together); N = 64: n-tile w & 3, column tile w >> 2; N = 32: waves 0-3 as
    // at W = 4, waves 4-7 idle. The final layer (l = 13) keeps the 4-wave mapping on waves 0-3 (n-tiles w + 4j,
    // a candidate's two CFG rows in one lane); waves 4-7 load clamped copies and skip it.
    template <int l> static constexpr bool HID = l != NLAYER - 1;
    template <int l> static constexpr bool SPL = W == 8 ? (HID<l> && A::N[l] <= 64) : (A::N[l] == 32 && NCT == 2);
    template <int l> static constexpr int TL = (SPL<l> || (W == 8 && HID<l>)) ? 1 : (A::N[l] / 16 + 3) / 4;
    template <int l> static constexpr int CL = SPL<l> ? 1 : NCT;
    template <int l> static MPCD_DEV int nt_of(int wave, int j)
    {
        if constexpr (W == 8) return !HID<l> ? (wave & 3) + 4 * j : A::N[l] == 128 ? wave : A::N[l] == 64 ? (wave & 3) : (wave & 1);
        return SPL<l> ? (wave & 1) : wave + 4 * j;
    }
    template <int l> static MPCD_DEV int ct_of(int wave, int c)
    {
        if constexpr (W == 8) return !SPL<l> ? (HID<l> ? c ^ (wave >> 2) : c) : A::N[l] == 64 ? (wave >> 2) : ((wave >> 1) & 1);
        return SPL<l> ? (wave >> 1) : c;
    }
    // a wave with no tile in hidden layer l (it still runs the layer's side work, loads and barriers)
    template <int l> static MPCD_DEV bool idle_of(int wave) { return W == 8 && HID<l> && A::N[l] == 32 && wave >= 4; }
    // waves that run the final layer and the update, and hold x_t / the noise
    static MPCD_DEV bool upd_wave(int wave) { return W == 4 || wave < 4; }

    // ONE buffer descriptor over the whole weight pack for every streamed layer (the layer offset goes into the
    // soffset): per-layer descriptors, kept live across the step loop, cost 4 SGPRs each and pushed ~50 SGPRs into
    // VGPR lanes (a v_readlane per use)
    static MPCD_DEV __amdgpu_buffer_rsrc_t pack_rsrc(const float *__restrict__ wp)
    {
        const uint64_t a = (uint64_t)wp;
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
        return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), (short)0, (int)(woffx<D0>(NLAYER) * 4),
                                                 0x00020000);
    }

    // streamed fragments of layer l for this wave
    template <int l>
    struct WS {
        u32x4 v[TL<l>][A::K[l] / 32][3];
    };

    template <int l>
    static MPCD_DEV void load_ws(WS<l> &f, const float *__restrict__ wp, int wave, int lane16)
    {
        constexpr int K = A::K[l], N = A::N[l], KC = K / 32, NT = N / 16;
        const __amdgpu_buffer_rsrc_t rs = pack_rsrc(wp);
#pragma unroll
        for (int j = 0; j < TL<l>; ++j) {
            const int nt = min(nt_of<l>(wave, j), NT - 1);  // clamped: path-independent load count
#pragma unroll
            for (int kc = 0; kc < KC; ++kc)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    const int soff = __builtin_amdgcn_readfirstlane(woffx<D0>(l) * 4 + ((nt * KC + kc) * 3 + pl) * 1024);
                    f.v[j][kc][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, soff, 0));
                }
        }
    }

    // fragment f (= (j * KC + kc) * 3 + plane) of layer l for this wave: load_ws one piece at a time, issued in
    // the free MFMA slots of an earlier layer (hidden_ilv's side work)
    template <int l>
    static MPCD_DEV void load_ws1(WS<l> &w, const float *__restrict__ wp, int wave, int lane16, int f)
    {
        constexpr int K = A::K[l], N = A::N[l], KC = K / 32, NT = N / 16;
        const __amdgpu_buffer_rsrc_t rs = pack_rsrc(wp);
        const int j = f / (KC * 3), kc = (f / 3) % KC, pl = f % 3;
        const int nt = min(nt_of<l>(wave, j), NT - 1);
        const int soff = __builtin_amdgcn_readfirstlane(woffx<D0>(l) * 4 + ((nt * KC + kc) * 3 + pl) * 1024);
        w.v[j][kc][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, soff, 0));
    }
    template <int l>
    static constexpr int NFRAG = TL<l> * (A::K[l] / 32) * 3;

    // Resident fragments: group g = ((li * 2 + j) * 4 + kc), planes 0..2 (AGPRs); Tail: groups RES_AG.. of
    // layer 7, streamed like the other layers (VGPRs)
    struct Res {
        u32x4 a[NAG][3];
    };
    struct Tail {
        u32x4 v[NRG - NAG][3];
    };
    static MPCD_DEV void load_tail1(Tail &t, const float *__restrict__ wp, int wave, int lane16, int f)
    {
        const __amdgpu_buffer_rsrc_t rs = pack_rsrc(wp);
        const int g = NAG + f / 3, pl = f % 3, j = (g / 4) % TPL, kc = g & 3, nt = wave + 4 * j;
        const int soff = __builtin_amdgcn_readfirstlane(woffx<D0>(RES_L0 + RES_NL - 1) * 4 + ((nt * 4 + kc) * 3 + pl) * 1024);
        t.v[g - NAG][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, soff, 0));
    }
    static MPCD_DEV void load_tail(Tail &t, const float *__restrict__ wp, int wave, int lane16)
    {
        const __amdgpu_buffer_rsrc_t rs = pack_rsrc(wp);
#pragma unroll
        for (int g = NAG; g < NRG; ++g) {
            const int j = (g / 4) % TPL, kc = g & 3, nt = wave + 4 * j;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const int soff = __builtin_amdgcn_readfirstlane(woffx<D0>(RES_L0 + RES_NL - 1) * 4 + ((nt * 4 + kc) * 3 + pl) * 1024);
                t.v[g - NAG][pl] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, soff, 0));
            }
        }
    }

    static MPCD_DEV void load_res(Res &r, const float *__restrict__ wp, int wave, int lane)
    {
#pragma unroll
        for (int g = 0; g < NAG; ++g) {
            const int li = g / (4 * TPL), j = (g / 4) % TPL, kc = g & 3;
            const int nt = wave + 4 * j;
            const float *base = wp + woffx<D0>(RES_L0 + li) + (size_t)((nt * 4 + kc) * 3) * 256 + lane * 4;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                r.a[g][pl] = __builtin_bit_cast(u32x4, ldg4(base + pl * 256));
            }
        }
    }

    // accumulator init of pass p of hidden layer l: this wave's 4 values of the layer's bias / cond-table row
    template <int l>
    static MPCD_DEV f32x4 init_rd(const char *lds, int wave, int lane, int p)
    {
        constexpr int NT = A::N[l] / 16, NC = CL<l>, EPI = epi_of(l);
        const int col = lane & 15, q = lane >> 4;
        const int ct = ct_of<l>(wave, p % NC);
        const float *init = reinterpret_cast<const float *>(
            lds + (EPI == EPI_CMISH ? (masked_of(ct, col) ? L::TPU : L::TPC) + cond_off(l / 2) * 4 : L::BI + A::boff(l) * 4));
        return *reinterpret_cast<const f32x4 *>(init + min(nt_of<l>(wave, p / NC), NT - 1) * 16 + 4 * q);
    }
    // byte offset in LDS of the operand fragments of pass p, k-chunk 0, plane 0
    template <int l>
    static MPCD_DEV int x_off(int wave, int lane, int p)
    {
        const int col = lane & 15, q = lane >> 4;
        const int ct = ct_of<l>(wave, p % CL<l>);
        const int row = (l == 0 && NB == 2) ? cand_of(ct, col) : ct * 16 + col;  // CFG: both branches read the candidate's x
        return L::in_off(l) + row * L::in_rs(l) + 16 * (q ^ swz(row));
    }

    // The part of a layer's head that does not depend on the previous layer, issued BEFORE the barrier that opens the
    // layer: the accumulator-init reads of its first two passes and the LDS address of its first operand reads. Behind
    // the barrier they stood in front of the first MFMA (LDS reads complete in order: the MFMA waited for the init read
    // and every operand read the compiler had placed before it); here the barrier's own lgkmcnt(0) retires them.
    // Safe: the biases (BI) are written once, before the step loop. Step s + 1's cond tables (TPU / TPC) are written in
    // Linear 12's last slot of step s and first read here before Linear 1's barrier, i.e. behind the barriers that open
    // the final layer and Linear 0: two barriers later (step 0's are written before the loop's first barrier). Step s's
    // are read last before Linear 11's barrier, and Linear 12's write stands behind Linear 12's barrier.
    // The 8-wave form only: the 4-wave kernels stand at their 512 registers (rw32 spilled another 20 with the nine
    // registers this keeps live across the barrier); they read inits and operands behind the barrier as before.
    static constexpr bool HEAD_PRE = W == 8;
    struct Pre {
        f32x4 i0, i1;
        int xa;
    };
    template <int l>
    static MPCD_DEV Pre pre_of(const char *lds, int wave, int lane)
    {
        Pre h = {};
        if constexpr (!HEAD_PRE) return h;
        h.i0 = init_rd<l>(lds, wave, lane, 0);
        h.i1 = TL<l> * CL<l> > 1 ? init_rd<l>(lds, wave, lane, 1) : h.i0;
        h.xa = x_off<l>(wave, lane, 0);
        asm volatile("" : "+v"(h.xa));  // formed here, not behind the barrier
        return h;
    }

    // Hidden layer l as a pipeline of passes (one n-tile x one column tile: a chain of 6 KC MFMAs, k-chunks in order):
    // the previous pass's epilogue (4 Mish, the 3-way split, the LDS stores of the next layer's operand planes) is
    // issued one micro-step after each of this pass's first MFMAs (pinned with sched_barrier: a bf16 MFMA leaves the
    // SIMD's vector issue free for 8 of its 16 cycles), the next activation fragments are read PF k-chunks ahead.
    // MM1(j, kc, m, x[3], acc) -> acc: partial product m (0..5, smallest first: the mfma_x3 order) of k-chunk kc of
    // n-tile j with this wave's fragments.
    // SIDE(k), k < NS: side work, one item per MFMA slot in order; items beyond the layer's slots (and all of them
    // on a wave with no tile) run after the layer's MFMAs
    // The head (barrier to first MFMA) is on the critical path of every layer: pre (pre_of, issued before the barrier)
    // brings the accumulator inits and the first operand address; behind the barrier stand only the operand reads,
    // k-chunk 0's three planes first and in product order (pinned), so that the first three products wait on counted
    // lgkmcnt for one plane each and never for the k-chunks read ahead.
    template <int l, int NS, class MM1, class SIDE>
    static MPCD_DEV void hidden_ilv(MM1 mm1, SIDE side, const Pre &pre, char *lds, int wave, int lane)
    {
        constexpr int K = A::K[l], N = A::N[l], KC = K / 32, NT = N / 16, T = TL<l>, NC = CL<l>, EPI = epi_of(l);
        constexpr int NP = T * NC, NI = NP * KC;  // passes; (pass, k-chunk) steps
        const int col = lane & 15, q = lane >> 4;
        static_assert(T == 1 || NT % 4 == 0, "only a one-tile layer can leave a wave idle");
        if constexpr (NT < 4 && !SPL<l>)
            if (wave >= NT) {  // N = 32 at 16 rows: waves 2, 3 have no tile
#pragma unroll
                for (int k = 0; k < NS; ++k) side(k);
                return;
            }
        if constexpr (W == 8 && N == 32)
            if (idle_of<l>(wave)) {  // waves 4-7: no tile; the side work, then the layer's barrier
#pragma unroll
                for (int k = 0; k < NS; ++k) side(k);
                return;
            }
        auto jp = [](int p) { return p / NC; };
        auto cp = [](int p) { return p % NC; };
        auto init_of = [&](int p) {
            return HEAD_PRE && p == 0 ? pre.i0 : HEAD_PRE && p == 1 ? pre.i1 : init_rd<l>(lds, wave, lane, p);
        };
        auto ldx = [&](u32x4 (&x)[3], int i) {  // step i = (pass i / KC, k-chunk i % KC)
            const int p = i / KC, kc = i % KC;
            load_x3(x, lds + (HEAD_PRE && p == 0 ? pre.xa : x_off<l>(wave, lane, p)) + kc * 64, L::in_pl(l));
        };
        u32x4 xb[PF + 1][3];  // operand fragments read PF k-chunks ahead
        if constexpr (HEAD_PRE) {  // k-chunk 0: plane 0, 1, 2 in this order, ahead of every other read of the layer
            const char *x0 = lds + pre.xa;
            __builtin_amdgcn_sched_barrier(0);  // nothing of the layer's later address arithmetic ahead of the reads
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                xb[0][pl] = *reinterpret_cast<const u32x4 *>(x0 + pl * L::in_pl(l));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int i = HEAD_PRE ? 1 : 0; i < PF; ++i)
            if (i < NI) ldx(xb[i], i);
        f32x4 acc = init_of(0), nxt = acc, ev = acc;
        // The previous pass's epilogue as NSTEP micro-steps of one or two VALU instructions, one after each MFMA:
        // a bf16 MFMA leaves the SIMD's vector issue free for 8 of its 16 cycles, i.e. about two VALU ops. Stage
        // by stage over the four values (the dependent ops of one value 4 slots apart), the exact operations of
        // common.h mish() and split3(); every intermediate through an empty register fence (no SLP packing).
        float et[4];
        u32x2 ep0, ep1, ep2;
        float er0 = 0.f, er1 = 0.f, er2 = 0.f, er3 = 0.f;
        constexpr int NSTEP = (EPI != EPI_NONE ? 16 : 0) + 8;
        auto fence = [](float &x) { asm volatile("" : "+v"(x)); };
        auto epi_step = [&](int k, int p) {
            if (EPI != EPI_NONE && k < 16) {
                const int e = k & 3;
                switch (k >> 2) {
                case 0: et[e] = __builtin_amdgcn_exp2f(ev[e] * 1.44269504088896341f); fence(et[e]); break;
                case 1: et[e] = __builtin_fmaf(et[e], et[e] + 2.0f, 2.0f); fence(et[e]); break;
                case 2: et[e] = __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(et[e]), 1.0f); fence(et[e]); break;
                default: { float y = ev[e] * et[e]; fence(y); ev[e] = y; } break;
                }
                return;
            }
            const int s = EPI != EPI_NONE ? k - 16 : k;
            const int n = nt_of<l>(wave, jp(p)) * 16 + 4 * q;
            const int ro = ct_of<l>(wave, cp(p)) * 16 + col;
            char *o = lds + L::out_off(l) + ro * L::out_rs(l) + st_off(n, q, ro);
            switch (s) {  // split3 (mlp_x3.h), in pieces
            // each remainder through a fence: the compiler would otherwise pair the two subtractions of a step
            // into one v_pk_add_f32, which beside MFMAs costs more issue time than the two plain ones
            // (MI355X_MICROARCH.md, price of one filler beside MFMAs)
            case 0: ep0 = u32x2{pk_bf16(ev.x, ev.y), pk_bf16(ev.z, ev.w)}; break;
            case 1: er0 = ev.x - bf_lo(ep0.x); fence(er0); er1 = ev.y - bf_hi(ep0.x); fence(er1); break;
            case 2: er2 = ev.z - bf_lo(ep0.y); fence(er2); er3 = ev.w - bf_hi(ep0.y); fence(er3); *reinterpret_cast<u32x2 *>(o) = ep0; break;
            case 3: ep1 = u32x2{pk_bf16(er0, er1), pk_bf16(er2, er3)}; break;
            case 4: er0 = er0 - bf_lo(ep1.x); fence(er0); er1 = er1 - bf_hi(ep1.x); fence(er1); break;
            case 5: er2 = er2 - bf_lo(ep1.y); fence(er2); er3 = er3 - bf_hi(ep1.y); fence(er3); break;
            case 6: *reinterpret_cast<u32x2 *>(o + L::out_pl(l)) = ep1; ep2 = u32x2{pk_bf16(er0, er1), pk_bf16(er2, er3)}; break;
            default: *reinterpret_cast<u32x2 *>(o + 2 * L::out_pl(l)) = ep2; break;
            }
        };
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (p + 1 < NP) nxt = init_of(p + 1);
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const int i = p * KC + kc;
                if (i + PF < NI) ldx(xb[(i + PF) % (PF + 1)], i + PF);
#pragma unroll
                for (int m = 0; m < 6; ++m) {
                    acc = mm1(jp(p), kc, m, xb[i % (PF + 1)], acc);
                    const int u = kc * 6 + m;
                    if (p > 0 && u < NSTEP) epi_step(u, p - 1);
                    if (i * 6 + m < NS) side(i * 6 + m);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (p > 0)
#pragma unroll
                for (int u = KC * 6; u < NSTEP; ++u) epi_step(u, p - 1);  // passes shorter than the epilogue
            ev = acc;
            acc = nxt;
        }
        // The last pass's epilogue, exposed (nothing left to hide it under): two values per packed instruction (v_pk_mul /
        // v_pk_add / v_pk_fma_f32; epi_step's operations, the same roundings) instead of the fenced scalar micro-steps:
        // loop VALU 1,631 -> 1,459 per wave-step, kernel -0.5 % (profiles/r6_mlp_tuning_ab.txt)
        auto epi_tail = [&](int p) {
            f32x2 a = {ev[0], ev[1]}, b = {ev[2], ev[3]};
            if constexpr (EPI != EPI_NONE) {
                const f32x2 l2e = {1.44269504088896341f, 1.44269504088896341f}, two = {2.0f, 2.0f};
                const f32x2 m2 = {-2.0f, -2.0f}, one = {1.0f, 1.0f};
                f32x2 ta = exp2_pair(a * l2e), tb = exp2_pair(b * l2e);
                ta = fma2(ta, ta + two, two);
                tb = fma2(tb, tb + two, two);
                ta = fma2(m2, rcp_pair(ta), one);
                tb = fma2(m2, rcp_pair(tb), one);
                a = a * ta;
                b = b * tb;
            }
            const int n = nt_of<l>(wave, jp(p)) * 16 + 4 * q;
            const int ro = ct_of<l>(wave, cp(p)) * 16 + col;
            char *o = lds + L::out_off(l) + ro * L::out_rs(l) + st_off(n, q, ro);
            const u32x2 q0 = {pk_bf16(a[0], a[1]), pk_bf16(b[0], b[1])};
            *reinterpret_cast<u32x2 *>(o) = q0;
            a = a - f32x2{bf_lo(q0.x), bf_hi(q0.x)};
            b = b - f32x2{bf_lo(q0.y), bf_hi(q0.y)};
            const u32x2 q1 = {pk_bf16(a[0], a[1]), pk_bf16(b[0], b[1])};
            *reinterpret_cast<u32x2 *>(o + L::out_pl(l)) = q1;
            a = a - f32x2{bf_lo(q1.x), bf_hi(q1.x)};
            b = b - f32x2{bf_lo(q1.y), bf_hi(q1.y)};
            *reinterpret_cast<u32x2 *>(o + 2 * L::out_pl(l)) = u32x2{pk_bf16(a[0], a[1]), pk_bf16(b[0], b[1])};
        };
        epi_tail(NP - 1);
#pragma unroll
        for (int k = NI * 6; k < NS; ++k) side(k);
    }

    template <int l, int NS = 0, class SIDE>
    static MPCD_DEV void layer(const WS<l> &w, SIDE side, const Pre &pre, char *lds, int wave, int lane)
    {
        hidden_ilv<l, NS>(
            [&](int j, int kc, int m, const u32x4 (&x)[3], f32x4 acc) { return mfma_bf(w.v[j][kc][wpl(m)], x[xpl(m)], acc); },
            side, pre, lds, wave, lane);
    }

    template <int li, int NS = 0, class SIDE>
    static MPCD_DEV void layer_res(const Res &r, const Tail &t, SIDE side, const Pre &pre, char *lds, int wave, int lane)
    {
        hidden_ilv<RES_L0 + li, NS>(
            [&](int j, int kc, int m, const u32x4 (&x)[3], f32x4 acc) {
                const int g = (li * TPL + j) * 4 + kc;
                if (g >= NAG) return mfma_bf(t.v[g - NAG][wpl(m)], x[xpl(m)], acc);
                const bool first = kc == 0 && m == 0;
                // LAST: the pass's last product, or the one before the VGPR-tail groups (a builtin MFMA then
                // reads the result: srcC forwarding needs no wait, but the compiler may copy it between)
                const bool last = (kc == 3 || g + 1 == NAG) && m == 5;
                if (first && last) return mfma_agpr1<true, true>(r.a[g][wpl(m)], x[xpl(m)], acc);
                if (first) return mfma_agpr1<true, false>(r.a[g][wpl(m)], x[xpl(m)], acc);
                if (last) return mfma_agpr1<false, true>(r.a[g][wpl(m)], x[xpl(m)], acc);
                return mfma_agpr1<false, false>(r.a[g][wpl(m)], x[xpl(m)], acc);
            },
            side, pre, lds, wave, lane);
    }

    // x (4 features) -> fp32 row in XB and the three bf16 planes layer 0 reads
    // split3 (mlp_x3.h) with every remainder through a fence: the same values, no v_pk_add_f32
    static MPCD_DEV void split3s(const f32x4 &v, u32x2 &p0, u32x2 &p1, u32x2 &p2)
    {
        auto fence = [](float &x) { asm volatile("" : "+v"(x)); };
        const uint32_t a = pk_bf16(v.x, v.y), b = pk_bf16(v.z, v.w);
        float r0 = v.x - bf_lo(a), r1 = v.y - bf_hi(a), r2 = v.z - bf_lo(b), r3 = v.w - bf_hi(b);
        fence(r0); fence(r1); fence(r2); fence(r3);
        const uint32_t c = pk_bf16(r0, r1), d = pk_bf16(r2, r3);
        r0 = r0 - bf_lo(c); r1 = r1 - bf_hi(c); r2 = r2 - bf_lo(d); r3 = r3 - bf_hi(d);
        fence(r0); fence(r1); fence(r2); fence(r3);
        p0 = u32x2{a, b};
        p1 = u32x2{c, d};
        p2 = u32x2{pk_bf16(r0, r1), pk_bf16(r2, r3)};
    }

    template <bool FP32 = true>
    static MPCD_DEV void store_x(char *lds, int cl, int n, const f32x4 &x)
    {
        if (FP32) *reinterpret_cast<f32x4 *>(lds + L::XB + (cl * L::SX + n) * 4) = x;
        u32x2 p0, p1, p2;
        split3s(x, p0, p1, p2);
        char *o = lds + L::S1 + cl * L::RS + ((n * 2) ^ (swz(cl) << 4));
        *reinterpret_cast<u32x2 *>(o) = p0;
        *reinterpret_cast<u32x2 *>(o + L::PL) = p1;
        *reinterpret_cast<u32x2 *>(o + 2 * L::PL) = p2;
    }

    using FW = WS<13>;
    // final layer: wave w -> n-tiles w + 4j, both column tiles (a candidate's two CFG rows in one lane); at
    // D0 = 32 and 32 rows load_ws<13>'s SPL mapping (n-tile w & 1) gives waves 0, 1 the same tiles
    static constexpr int NZT = TL<13>;

    // final Linear (32 -> D0) + the denoise update (reference op order, mlp_x3.hip final_and_update)
    // x_t of the update's (n-tile j, column group g) quads, when XREG keeps it in registers
    static constexpr int XG = NB == 2 ? 1 : NCT;
    // XREG: each lane keeps its x_t quads in registers across steps (the fp32 copy in LDS goes), and the update's x-only
    // products (a x, c2 x, std z) are formed while the final layer's operand reads are in flight. With the cond tables
    // as Linear 12's side work: kernel 1.098 -> 1.090 ms at cfg2 (profiles/r6_mlp_tuning_ab.txt, 3 repeats). The
    // 8-wave form only where that is one quad per lane, else the fp32 copy in LDS (the same values: 256 registers per
    // wave do not hold 2-4 quads beside the final layer's operands)
    static constexpr bool XREG = W == 4 || (D0 / 16 + 3) / 4 * XG == 1;
    // Linear 8's k-chunks KS8 .. resident in LDS (Lds8::W8L); KL8 == 0: all eight streamed, as at W = 4
    static constexpr int KL8 = [] { if constexpr (W == 8) return L::KL; else return 0; }();
    static constexpr int KS8 = A::K[8] / 32 - KL8;
    static constexpr bool lds8_agrees() { if constexpr (W == 8) return L::NZT == NZT && L::XREG == XREG; else return true; }
    static_assert(lds8_agrees(), "Lds8 places the noise block and XB by these");
    static MPCD_DEV bool x_lane(int j, int wave, int col)
    {
        return upd_wave(wave) && (D0 / 16 % 4 == 0 || wave + 4 * j < D0 / 16) && !(R == 16 && NB == 2 && col >= 8);
    }
    static MPCD_DEV void load_xr(f32x4 (&xr)[NZT][XG], const char *lds, int wave, int lane)
    {
        const int col = lane & 15, q = lane >> 4;
#pragma unroll
        for (int j = 0; j < NZT; ++j)
#pragma unroll
            for (int g = 0; g < XG; ++g) {
                const int cl = NB == 2 ? col : g * 16 + col, n = (wave + 4 * j) * 16 + 4 * q;
                xr[j][g] = x_lane(j, wave, col) ? *reinterpret_cast<const f32x4 *>(lds + L::XB + (cl * L::SX + n) * 4)
                                                : f32x4{0.f, 0.f, 0.f, 0.f};
            }
    }

    // The final layer's head before its barrier (as pre_of): its bias reads and its first operand address
    struct FPre {
        f32x4 b[NZT];
        int xa;
    };
    static MPCD_DEV FPre final_pre(const char *lds, int wave, int lane)
    {
        constexpr int NT = D0 / 16;
        const int col = lane & 15, q = lane >> 4;
        const float *bias = reinterpret_cast<const float *>(lds + L::BI + A::boff(13) * 4);
        FPre h = {};
        if constexpr (!HEAD_PRE) return h;
#pragma unroll
        for (int j = 0; j < NZT; ++j) {
            const int nt = (NT % 4 == 0 || (wave & 3) + 4 * j < NT) ? (wave & 3) + 4 * j : 0;
            h.b[j] = *reinterpret_cast<const f32x4 *>(bias + nt * 16 + 4 * q);
        }
        h.xa = L::T1 + col * L::RS + 16 * (q ^ swz(col));
        asm volatile("" : "+v"(h.xa));
        return h;
    }

    static MPCD_DEV void final_and_update(const FW &f, const FPre &pre, char *lds, const MlpSampleArgs &p, const StepPlan &sp, int s,
                                          int64_t cand0, int n_cand, const f32x4 (&nz)[NZT][NB],
                                          uint32_t (&am)[2], f32x4 (&xr)[NZT][XG], int wave, int lane, ProfAcc &tacc)
    {
        uint64_t tmark = prof_now();
        if (!upd_wave(wave)) return;  // W = 8: waves 0-3 run the final layer (no barrier, no global load inside)
        constexpr int T = NZT, NT = D0 / 16;
        const int col = lane & 15, q = lane >> 4;
        const float *bias = reinterpret_cast<const float *>(lds + L::BI + A::boff(13) * 4);
        f32x4 acc[T][2];
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int nt = (NT % 4 == 0 || wave + 4 * j < NT) ? wave + 4 * j : 0;
            acc[j][0] = acc[j][1] = HEAD_PRE ? pre.b[j] : *reinterpret_cast<const f32x4 *>(bias + nt * 16 + 4 * q);
        }
        // both column tiles' operand reads in flight before the first MFMA: one LDS latency instead of two in a row;
        // HEAD_PRE: the first tile's planes in product order (pinned), so that the first product waits for one read
        u32x4 xf[NCT][3];
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            if constexpr (HEAD_PRE) {
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    xf[c][pl] = *reinterpret_cast<const u32x4 *>(lds + pre.xa + c * 16 * L::RS + pl * L::PL);
                    if (c == 0) __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                load_x3(xf[c], lds + L::T1 + (c * 16 + col) * L::RS + 16 * (q ^ swz(col)), L::PL);
            }
        }
        // XREG, DDPM: the x-only products of the update under the operand reads' latency (each through a
        // fence, the same values as in the update's order: a x, c2 x, std z are separate roundings there too)
        constexpr bool PRE = XREG && IS_DDPM;
        f32x4 pax[T][XG], pcx[T][XG], psz[T][XG];
        if constexpr (PRE) {
            auto fn = [](float &v) { asm volatile("" : "+v"(v)); };
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int g = 0; g < XG; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float xv = xr[j][g][r];
                        float a = sp.a * xv, c = sp.c2 * xv, z = sp.std * nz[j][0][r];
                        fn(a); fn(c); fn(z);
                        pax[j][g][r] = a;
                        pcx[j][g][r] = c;
                        psz[j][g][r] = z;
                        am[g] = max(am[g], abs_bits(xv));
                    }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int j = 0; j < T; ++j)
                if (NT % 4 == 0 || wave + 4 * j < NT) acc[j][c] = mfma_x3(f.v[j][0], xf[c], acc[j][c]);
#ifndef MPCD_PROF_L8  // that build keeps rows 28 / 29 for Linear 8's halves
        prof_mark(tacc, tmark, 28, acc[0][1]);  // profile: the final layer's operand reads and MFMAs ("-" row)
#endif
        if (R == 16 && NB == 2) {
            // column c holds candidate c & 7's context row (c < 8) or masked row (c >= 8): bring the masked
            // row's eps next to the context row's (DPP row_ror:8 swaps the two halves of each 16-lane row)
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = acc[j][0][r];  // element to a scalar first (bit_cast of a vector element)
                    acc[j][1][r] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                        0, __builtin_bit_cast(int, e), 0x128, 0xF, 0xF, false));
                }
            if (col >= 8) return;  // lanes of the masked rows: their eps went to lane col - 8
        }
        const bool last = s == p.n_steps - 1;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int nt = wave + 4 * j;
            if (NT % 4 != 0 && nt >= NT) continue;
            const int n = nt * 16 + 4 * q;
#pragma unroll
            for (int g = 0; g < (NB == 2 ? 1 : NCT); ++g) {
                const int cl = NB == 2 ? col : g * 16 + col;
                const f32x4 ec = acc[j][NB == 2 ? 0 : g];
                const f32x4 eu = acc[j][1];
                const int64_t gc = cand0 + cl;
                if (SMODE == MODE_EPS || SMODE == MODE_EPS1) {
                    if (in_span<GRP>(p.batch, cand0, n_cand, cl)) {
                        *reinterpret_cast<f32x4 *>(p.x_out + (size_t)gc * D0 + n) = ec;
                        if (SMODE == MODE_EPS) *reinterpret_cast<f32x4 *>(p.chain + (size_t)gc * D0 + n) = eu;
                    }
                    continue;
                }
                const f32x4 x = XREG ? xr[j][g] : *reinterpret_cast<const f32x4 *>(lds + L::XB + (cl * L::SX + n) * 4);
                f32x4 xn;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float xv = x[r];
                    float o;
                    if constexpr (PRE) {
                        auto fn = [](float &v) { asm volatile("" : "+v"(v)); };
                        float x0c = pax[j][g][r] - sp.b * ec[r];
                        fn(x0c);
                        float x0u = pax[j][g][r] - sp.b * eu[r];
                        fn(x0u);
                        float x0 = p.wp1 * x0c - p.wf * x0u;
                        x0 = clamp1(x0);
                        float mean = sp.c1 * x0 + pcx[j][g][r];
                        fn(mean);
                        o = (sp.flags & PLAN_NOISE) ? mean + psz[j][g][r] : mean;
                        xn[r] = o;
                        am[g] = max(am[g], abs_bits(o));
                        continue;
                    }
                    if (IS_DDPM) {
                        // every intermediate through a fence: the SLP vectorizer paired the four values' products
                        // into v_pk_mul / v_pk_add_f32, dearer than the plain ops here (same values either way)
                        auto fn = [](float &v) { asm volatile("" : "+v"(v)); };
                        float x0c = sp.a * xv - sp.b * ec[r];
                        fn(x0c);
                        float x0u = sp.a * xv - sp.b * eu[r];
                        fn(x0u);
                        float x0 = p.wp1 * x0c - p.wf * x0u;
                        x0 = clamp1(x0);
                        float mean = sp.c1 * x0 + sp.c2 * xv;
                        fn(mean);
                        o = (sp.flags & PLAN_NOISE) ? mean + sp.std * nz[j][0][r] : mean;
                    } else if (SMODE == MODE_DDIM_CFG) {
                        float x0 = p.wp1 * (sp.a * xv - sp.b * ec[r]) - p.wf * (sp.a * xv - sp.b * eu[r]);
                        if (p.clamp_x0) x0 = clamp1(x0);
                        const float e = p.wp1 * ec[r] - p.wf * eu[r];
                        o = (sp.flags & PLAN_FINAL) ? x0 : x0 * sp.sqan + sp.cn * e;
                    } else {  // MODE_DDIM, 3-arg net
                        float x0 = sp.a * xv - sp.b * ec[r];
                        if (p.clamp_x0) x0 = clamp1(x0);
                        o = (sp.flags & PLAN_FINAL) ? x0 : x0 * sp.sqan + sp.cn * ec[r];
                    }
                    xn[r] = o;
                    am[g] = max(am[g], max(abs_bits(xv), abs_bits(o)));
                }
                store_x<!XREG>(lds, cl, n, xn);
                if (XREG) xr[j][g] = xn;
                if (in_span<GRP>(p.batch, cand0, n_cand, cl)) {
                    if (p.chain) *reinterpret_cast<f32x4 *>(p.chain + ((size_t)(s + 1) * p.batch + gc) * D0 + n) = xn;
                    if (last) *reinterpret_cast<f32x4 *>(p.x_out + (size_t)gc * D0 + n) = xn;
                }
            }
        }
#ifndef MPCD_PROF_L8
        prof_mark(tacc, tmark, 29, am[0]);  // profile: the update, the stores
#endif
    }

    // noise of step s (slice s+1) for this lane's quads, fetched one step ahead of use
    static MPCD_DEV void fetch_noise(f32x4 (&nz)[NZT][NB], const MlpSampleArgs &p, const StepPlan &sp, int s,
                                     int64_t cand0, int n_cand, int wave, int lane)
    {
        constexpr int NT = D0 / 16;
#pragma unroll
        for (int j = 0; j < NZT; ++j)
#pragma unroll
            for (int g = 0; g < NB; ++g) nz[j][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!IS_DDPM || !(sp.flags & PLAN_NOISE)) return;  // DDIM: sigma = 0
        const int col = lane & 15, q = lane >> 4;
#pragma unroll
        for (int j = 0; j < NZT; ++j) {
            const int nt = wave + 4 * j;
            if (NT % 4 != 0 && nt >= NT) continue;
            const int n = nt * 16 + 4 * q;
            const int64_t gc = cand0 + col;  // DDPM-CFG: NB == 2, one candidate per column (R = 16: columns < 8)
            if (!in_span<GRP>(p.batch, cand0, n_cand, col) || (R == 16 && col >= 8)) continue;
            if (SMODE == MODE_DDPM_XN)
                nz[j][0] = *reinterpret_cast<const f32x4 *>(p.noise + ((size_t)(s + 1) * p.batch + gc) * D0 + n);
            else
                nz[j][0] = philox_normal4(p.seed, (uint64_t)(p.global_offset + gc), (uint32_t)(s + 1), (uint32_t)(n >> 2));
        }
    }

    // The next step's Philox draw (CFG-DDPM with in-kernel noise, one quad per lane) as NPH micro-steps, issued
    // as side work in Linear 8's MFMA slots instead of in the open after Linear 10 (~880 cycles per step there):
    // the exact operations of common.h philox4x32_10 / philox_normal4, one quarter-rate multiply per step,
    // every intermediate through a register fence. Bit-identical to fetch_noise.
    struct PhSt {
        uint32_t c0, c1, c2, c3, k0, k1, h;
        float u0, u1, u2, u3, ra, rb;
        float z[4];
    };
    static constexpr int NPH = 40 + 12;
    static constexpr bool STAGED_NOISE = SMODE == MODE_DDPM_CFG && NZT == 1;
    static MPCD_DEV void ph_init(PhSt &st, const MlpSampleArgs &p, int slice, int64_t cand0, int wave, int lane)
    {
        const int col = lane & 15, q = lane >> 4;
        const int n = min(wave, D0 / 16 - 1) * 16 + 4 * q;  // clamped tile: lanes past NT draw and discard
        const uint64_t cand = (uint64_t)(p.global_offset + cand0 + col);
        st.c0 = (uint32_t)(n >> 2);
        st.c1 = (uint32_t)cand;
        st.c2 = (uint32_t)(cand >> 32);
        st.c3 = (uint32_t)slice;
        st.k0 = (uint32_t)p.seed;
        st.k1 = (uint32_t)(p.seed >> 32);
    }
    static MPCD_DEV void ph_step(PhSt &st, int k)
    {
        auto fu = [](uint32_t &x) { asm volatile("" : "+v"(x)); };
        auto ff = [](float &x) { asm volatile("" : "+v"(x)); };
        constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
        if (k < 40) {  // round k / 4 of philox4x32_10
            switch (k & 3) {
            case 0: st.h = __umulhi(M0, st.c0); fu(st.h); break;                  // hi0
            case 1: st.c0 = M0 * st.c0; fu(st.c0); break;                         // lo0 (in c0 until the swap)
            case 2: { const uint32_t hi1 = __umulhi(M1, st.c2); st.c3 = st.h ^ st.c3 ^ st.k1; st.h = hi1; fu(st.h); fu(st.c3); } break;
            default: {
                const uint32_t lo1 = M1 * st.c2;
                // c' = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); c3 holds hi0 ^ c3 ^ k1, c0 holds lo0
                const uint32_t n0 = st.h ^ st.c1 ^ st.k0, n2 = st.c3, n3 = st.c0;
                st.c0 = n0; st.c1 = lo1; st.c2 = n2; st.c3 = n3;
                st.k0 += W0; st.k1 += W1;
                fu(st.c0); fu(st.c1); fu(st.c2); fu(st.c3);
            } break;
            }
            return;
        }
        const float S = 2.3283064365386963e-10f;  // 2^-32
        switch (k - 40) {  // philox_normal4's Box-Muller
        case 0: st.u0 = ((float)st.c0 + 1.0f) * S; st.u1 = (float)st.c1 * S; ff(st.u0); ff(st.u1); break;
        case 1: st.u2 = ((float)st.c2 + 1.0f) * S; st.u3 = (float)st.c3 * S; ff(st.u2); ff(st.u3); break;
        case 2: st.ra = -2.0f * __logf(st.u0); ff(st.ra); break;
        case 3: st.rb = -2.0f * __logf(st.u2); ff(st.rb); break;
        case 4: st.ra = __fsqrt_rn(st.ra); ff(st.ra); break;
        case 5: st.rb = __fsqrt_rn(st.rb); ff(st.rb); break;
        case 6: st.u1 = 6.2831853071795865f * st.u1; st.u3 = 6.2831853071795865f * st.u3; ff(st.u1); ff(st.u3); break;
        case 7: st.z[0] = __cosf(st.u1); ff(st.z[0]); break;
        case 8: st.z[1] = __sinf(st.u1); ff(st.z[1]); break;
        case 9: st.z[2] = __cosf(st.u3); ff(st.z[2]); break;
        case 10: st.z[3] = __sinf(st.u3); ff(st.z[3]); break;
        default:
            for (int e = 0; e < 4; ++e) {
                st.z[e] = (e < 2 ? st.ra : st.rb) * st.z[e];
                ff(st.z[e]);
            }
            break;
        }
    }
    // fetch_noise's result from the staged draw: zeros where fetch_noise draws none
    static MPCD_DEV void ph_take(f32x4 (&nz)[NZT][NB], const PhSt &st, const StepPlan &sp, int64_t cand0,
                                 int n_cand, const MlpSampleArgs &p, int wave, int lane)
    {
        const int col = lane & 15;
#pragma unroll
        for (int g = 0; g < NB; ++g) nz[0][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bool ok = (sp.flags & PLAN_NOISE) && (D0 / 16 % 4 == 0 || wave < D0 / 16) && in_span<GRP>(p.batch, cand0, n_cand, col) &&
                        !(R == 16 && col >= 8);
        if (ok) nz[0][0] = f32x4{st.z[0], st.z[1], st.z[2], st.z[3]};
    }

    static MPCD_DEV void run(const MlpSampleArgs &p)
    {
        extern __shared__ float lds_f[];
        char *lds = reinterpret_cast<char *>(lds_f);
        const int lane = threadIdx.x & 63;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const CandSpan span = cand_span<CPW, GRP>(p.cproj, p.group, p.group_wgs);
        const int64_t cand0 = span.cand0;
        const int n_cand = span.n;  // grouped: columns c < n_cand hold candidate cand0 + c, the others idle
        int lane16 = lane * 16;
        const float *wp = p.wpack;
        float *bi = reinterpret_cast<float *>(lds + L::BI);
        float *bic = reinterpret_cast<float *>(lds + L::BIC);
        float *cps = reinterpret_cast<float *>(lds + L::CPS);

        Res res;
        load_res(res, wp, wave, lane);
        // Linear 8's resident k-chunks, pack -> W8L, once per launch: fragment f = ((kc - KS8) NT + nt) 3 + plane, 1 KB
        // each as the pack holds it, fragment i * 8 + wave by wave `wave` (past the last one: the last one again, the
        // same bytes). Ordered before every read by the barrier below.
        if constexpr (KL8 > 0) {
            constexpr int NT = A::N[8] / 16, KC = A::K[8] / 32, NF = KL8 * NT * 3, NI = (NF + W - 1) / W;
            const __amdgpu_buffer_rsrc_t rs = pack_rsrc(wp);
            u32x4 st[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int f = min(i * W + wave, NF - 1), kc = KS8 + f / (NT * 3), nt = f / 3 % NT, pl = f % 3;
                const int soff = __builtin_amdgcn_readfirstlane(woffx<D0>(8) * 4 + ((nt * KC + kc) * 3 + pl) * 1024);
                st[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, soff, 0));
            }
#pragma unroll
            for (int i = 0; i < NI; ++i)
                *reinterpret_cast<u32x4 *>(lds + L::W8L + min(i * W + wave, NF - 1) * 1024 + lane * 16) = st[i];
        }
        for (int l = 0; l < NLAYER; ++l)
            for (int i = threadIdx.x; i < A::N[l]; i += NTH) bi[A::boff(l) + i] = wp[woffx<D0>(l) + wfl<D0>(l) + i];
        for (int j = 0; j < 6; ++j)
            for (int i = threadIdx.x; i < A::N[2 * j + 1]; i += NTH)
                bic[cond_off(j) + i] = wp[woffx<D0>(2 * j + 1) + wfl<D0>(2 * j + 1) + i];
        // mpcd_mpc_step (ctx_fused): the shared context row's projection computed here, as ctx_prologue_row_kernel
        // would (the same function: the same bits), so the control step has no prologue launch
        for (int i = threadIdx.x; i < COND_TOTAL; i += NTH)
            cps[i] = !CTX ? 0.f
                          : p.ctx_fused ? ctx_proj_col(p.ctx_row, p.ctx_dim, p.cond_layers, p.n_cond, p.cond_dim, i)
                                        : span.cproj[i];
        if (threadIdx.x < CPW) reinterpret_cast<uint32_t *>(lds + L::AMX)[threadIdx.x] = 0u;
        uint32_t am[2] = {0u, 0u};
        for (int i = threadIdx.x; i < CPW * QUADS; i += NTH) {  // x_T (fp32 + planes)
            const int c = i / QUADS, qd = i - c * QUADS;
            const int64_t gc = cand0 + c;
            f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
            if (in_span<GRP>(p.batch, cand0, n_cand, c)) {
                z = p.noise ? *reinterpret_cast<const f32x4 *>(p.noise + (size_t)gc * D0 + qd * 4)
                            : philox_normal4(p.seed, (uint64_t)(p.global_offset + gc), 0u, (uint32_t)qd);
                if (IS_DDPM && p.x_init) z = warm_x<D0>(p.x_init, p.x_init_kind, p.x_sa, p.x_sb, gc, span.m, qd, z);  // warm start
                if (p.chain && SMODE != MODE_EPS) *reinterpret_cast<f32x4 *>(p.chain + (size_t)gc * D0 + qd * 4) = z;
            }
            store_x(lds, c, qd * 4, z);
        }
        f32x4 xr[NZT][XG];
        // the staged biases, context projection and x_T: read by load_xr, and by step 0's tables below (HEAD_PRE)
        if constexpr (XREG || HEAD_PRE) lds_barrier();
        if constexpr (XREG) load_xr(xr, lds, wave, lane);

        int wofs = 0;
        WS<0> w0;
        load_ws<0>(w0, wp, wave, lane16);
        f32x4 nz[NZT][NB];
        StepPlan sp = load_plan(p.plan, 0);
        if constexpr (W == 4) fetch_noise(nz, p, sp, 0, cand0, n_cand, wave, lane);
        const int tpi = threadIdx.x < COND_TOTAL / 4 ? (int)threadIdx.x : threadIdx.x < COND_TOTAL / 2 ? (int)threadIdx.x - COND_TOTAL / 4 : 0;
        f32x4 tpre = reinterpret_cast<const f32x4 *>(p.tproj)[tpi];
        // A step's time projections + cond biases (+ shared context part) -> TPU / TPC: one f32x4 per thread. Step
        // s + 1's are written as Linear 12's side work. The first step's: HEAD_PRE here, ordered before every read by the
        // step loop's first barrier (Linear 1's init reads are issued behind it, before Linear 1's own barrier: pre_of);
        // the 4-wave kernels behind that barrier (their loop as it was, instruction for instruction)
        auto table = [&] {
            if (threadIdx.x < COND_TOTAL / 2) {
                const bool ctx_half = threadIdx.x >= COND_TOTAL / 4;
                const int k = ctx_half ? (int)threadIdx.x - COND_TOTAL / 4 : (int)threadIdx.x;
                f32x4 u = tpre + reinterpret_cast<const f32x4 *>(lds + L::BIC)[k];
                if (ctx_half) u = u + reinterpret_cast<const f32x4 *>(lds + L::CPS)[k];
                reinterpret_cast<f32x4 *>(lds + (ctx_half ? L::TPC : L::TPU))[k] = u;
            }
        };
        if constexpr (HEAD_PRE) {
            table();
            tpre = reinterpret_cast<const f32x4 *>(p.tproj + (size_t)(1 < p.n_steps ? 1 : 0) * COND_TOTAL)[tpi];
        }
        // MPCD_PROF_LAYERS build (mlp_common.h): cycles of each barrier-to-barrier segment (tools/layer_prof.py)
        ProfAcc tacc = {};
        const uint64_t rt0 = prof_realtime();
        uint64_t tprev = prof_now();
        const uint64_t ct0 = tprev;
#ifdef MPCD_PROF_LAYERS
        int bk = 0;  // the segment: 14 barriers per denoise step
        auto bar = [&] {
            if constexpr (HEAD_PRE) __builtin_amdgcn_s_waitcnt(0xC07F);  // as in the product build, below
            prof_barrier(tacc, tprev, bk);
            bk = bk == 13 ? 0 : bk + 1;
        };
#else
        // No capture here and no mark in noise_next below in the product build: the empty forms of both in the lambdas'
        // closures changed the order of two scalar copies in three rw32 kernels (profiles/mlp_switch_cleanup_isa.txt)
        // HEAD_PRE: the barrier's lgkmcnt(0) once more as the builtin (0xC07F: lgkmcnt(0) alone), which the compiler's
        // wait counting sees (the one inside lds_barrier's asm it does not): with a scalar load or an LDS operation of
        // the previous layer still outstanding in its books, every head's first wait came out as lgkmcnt(0)
        auto bar = [] {
            if constexpr (HEAD_PRE) __builtin_amdgcn_s_waitcnt(0xC07F);
            lds_barrier();
        };
#endif
        int lane_l = lane;
        for (int s = 0; s < p.n_steps; ++s) {
            // launder the weight base: stops LICM hoisting the streamed layers' loads out of the loop
            asm volatile("" : "+s"(wofs), "+v"(lane16));
            const float *ws = wp + wofs;
            // W = 8: the lane index laundered too. Hoisted out of the step loop, every layer's LDS addresses stand
            // in registers for the whole launch, which 256 registers per wave do not hold (they spilled to scratch)
            if constexpr (W == 8) asm volatile("" : "+v"(lane_l));
            const int lane = lane_l;
            auto none = [](int) {};
            // Each layer's fragments are issued one at a time in the free MFMA slots of an earlier layer
            // (hidden_ilv side work): the vector-memory issue rides under MFMAs instead of stalling a layer, and
            // the register budget (one wave per SIMD, 512 registers, 252 AGPRs of resident weights) holds: L8's
            // 96 registers are in flight from L5 on, everything else one or two layers ahead.
            WS<1> w1;
            load_ws<1>(w1, ws, wave, lane16);
            WS<2> w2;
            load_ws<2>(w2, ws, wave, lane16);
            // Every layer's pre_of / final_pre stands before the barrier that opens the layer (see pre_of)
            Pre hd = pre_of<0>(lds, wave, lane);
            bar();
            if constexpr (!HEAD_PRE)
                if (s == 0) {
                    table();
                    tpre = reinterpret_cast<const f32x4 *>(p.tproj + (size_t)(s + 1 < p.n_steps ? s + 1 : s) * COND_TOTAL)[tpi];
                }
            // W = 8 (256 registers per wave, 120 of them resident weights): every streamed layer's fragments are
            // issued one layer later than at W = 4, so that at most two layers' stand in registers at a time.
            // A layer that leaves waves 4-7 without a tile (N = 32) has two arms, and loads issued inside the arms are
            // no longer counted at the join: the next head then drains vmcnt(0), on waves 4-7 for loads issued just
            // before the barrier. So at W = 8 no fragment load stands inside such a layer: Linear 3's are issued behind
            // Linear 1 (after the join), Linear 11's in Linear 9's slots, Linear 12's and the final layer's behind
            // Linear 10.
            WS<3> w3;
            WS<4> w4;
            auto side3 = [&](int k) { load_ws1<3>(w3, ws, wave, lane16, k); };
            auto side4 = [&](int k) { load_ws1<4>(w4, ws, wave, lane16, k); };
            if constexpr (W == 8) layer<0>(w0, none, hd, lds, wave, lane);
            else layer<0, NFRAG<3>>(w0, side3, hd, lds, wave, lane);
            hd = pre_of<1>(lds, wave, lane);
            bar();
            WS<8> w8;
            Tail tail;
            WS<9> w9;
            WS<10> w10;
            WS<11> w11;
            WS<12> w12;
            WS<13> w13;
            const StepPlan cur = sp;
            PhSt ph;
            auto side9 = [&](int k) {
                if (k < NFRAG<11>) load_ws1<11>(w11, ws, wave, lane16, k);
                else if (k < NFRAG<11> + NFRAG<12>) load_ws1<12>(w12, ws, wave, lane16, k - NFRAG<11>);
                else load_ws1<13>(w13, ws, wave, lane16, k - NFRAG<11> - NFRAG<12>);
            };
            f32x4 nzc[NZT][NB];
            auto noise_next = [&] {  // this step's noise to nzc, the next step's drawn / fetched into nz
#pragma unroll
                for (int j = 0; j < NZT; ++j)
#pragma unroll
                    for (int g = 0; g < NB; ++g) nzc[j][g] = nz[j][g];
                if (STAGED_NOISE && s + 1 < p.n_steps) {
                    ph_take(nz, ph, sp, cand0, n_cand, p, wave, lane);
                } else if (s + 1 < p.n_steps) {
#ifdef MPCD_PROF_LAYERS
                    const uint64_t tn0 = prof_now();
#endif
                    fetch_noise(nz, p, sp, s + 1, cand0, n_cand, wave, lane);
#ifdef MPCD_PROF_LAYERS
                    prof_mark(tacc, tn0, 31);  // the noise draws ("tail" row, wait column)
#endif
                }
            };
            if constexpr (W == 8) {
                layer<1>(w1, none, hd, lds, wave, lane);
                load_ws<3>(w3, ws, wave, lane16);
            } else {
                layer<1, NFRAG<4>>(w1, side4, hd, lds, wave, lane);
            }
            hd = pre_of<2>(lds, wave, lane);
            bar();
            if constexpr (W == 8) layer<2, NFRAG<4>>(w2, side4, hd, lds, wave, lane);
            else layer<2>(w2, none, hd, lds, wave, lane);
            hd = pre_of<3>(lds, wave, lane);
            bar();
            layer<3>(w3, none, hd, lds, wave, lane);
            hd = pre_of<4>(lds, wave, lane);
            bar();
            layer<4>(w4, none, hd, lds, wave, lane);
            hd = pre_of<5>(lds, wave, lane);
            bar();
            // The next step's plan: a scalar load, which returns out of order and so makes any wait behind it an
            // lgkmcnt(0). Issued before Linear 8's barrier, whose own lgkmcnt(0) retires it, never at a head. The last
            // step reads its own entry again (nothing past the plan's end) and does not use it.
            if constexpr (W == 8) {
                // 256 registers per wave, 120 of them resident weights: Linear 8's 24 fragments (96 registers) never
                // stand whole. Its first W8P k-chunks are issued in the MFMA slots of Linear 7's second pass (Linear 7's
                // own streamed Tail in Linear 6's slots), k-chunk c >= W8P in the MFMA slots of k-chunk c - W8P + 1 of
                // Linear 8 itself (into registers its first chunks have left), Linear 9's in the slots of k-chunk 6.
                // KL8 > 0: k-chunks KS8 .. are resident in LDS (Lds8::W8L). The KS8 streamed ones are then all issued in
                // Linear 7's slots and waited for in front of Linear 8's barrier: no load of Linear 8's own and no
                // vector-memory wait stands inside the layer. The resident ones are read one k-chunk ahead into a ring of
                // two (r8), plane 2, 1, 0 (the order the products take them) in the first three MFMA slots of the k-chunk
                // before, behind that k-chunk's operand reads: LDS reads return in order, so each product waits on a
                // counted lgkmcnt.
                constexpr int W8P = KL8 > 0 ? KS8 : 4, KC8 = A::K[8] / 32, S9 = 6 * 6, S7 = 5 * 6;
                constexpr int W8S = KL8 > 0 ? KS8 * 3 : 12, NTL = (NRG - NAG) * 3;
                static_assert(S7 + W8S <= 8 * 6, "Linear 7's MFMA slots");
                static_assert(NFRAG<8> == KC8 * 3 && NFRAG<9> == 6 && W8P >= 2);
                layer_res<0>(res, tail, none, hd, lds, wave, lane);
                hd = pre_of<6>(lds, wave, lane);
                bar();
                layer_res<1, 6 + NTL>(res, tail, [&](int k) { if (k >= 6) load_tail1(tail, ws, wave, lane16, k - 6); }, hd, lds, wave, lane);
                hd = pre_of<7>(lds, wave, lane);
                bar();
                layer_res<2, S7 + W8S>(res, tail, [&](int k) { if (k >= S7) load_ws1<8>(w8, ws, wave, lane16, k - S7); }, hd,
                                       lds, wave, lane);
#pragma unroll
                for (int f = W8S; f < W8P * 3; ++f) load_ws1<8>(w8, ws, wave, lane16, f);
                sp = load_plan(p.plan, s + 1 < p.n_steps ? s + 1 : s);
                hd = pre_of<8>(lds, wave, lane);
                if constexpr (KL8 > 0) __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0): Linear 8's streamed k-chunks
                bar();
                u32x4 r8[2][3];
                const char *w8l = nullptr;
                if constexpr (KL8 > 0) w8l = lds + L::W8L + nt_of<8>(wave, 0) * 3 * 1024 + lane * 16;
#ifdef MPCD_PROF_L8
                uint64_t t8 = tprev;  // profile: Linear 8 from its barrier to k-chunk 3's / on to k-chunk 7's last product
#endif
                auto stream8 = [&](int k) {
                    const int kc = k / 6, m = k % 6;
#ifdef MPCD_PROF_L8
                    if (k == 4 * 6 - 1 || k == KC8 * 6 - 1) {
                        asm volatile("" ::: "memory");
                        const uint64_t t = prof_now();
                        tacc[k == KC8 * 6 - 1 ? 29 : 28] += t - t8;
                        t8 = t;
                    }
#endif
                    if constexpr (KL8 > 0) {
                        if (kc + 1 >= KS8 && kc + 1 < KC8 && m < 3)
                            r8[(kc + 1) & 1][2 - m] = *reinterpret_cast<const u32x4 *>(
                                w8l + ((kc + 1 - KS8) * (A::N[8] / 16) * 3 + 2 - m) * 1024);
                    } else {
                        if (kc >= 1 && kc + W8P - 1 < KC8 && m < 3) load_ws1<8>(w8, ws, wave, lane16, (kc + W8P - 1) * 3 + m);
                    }
                    if (k >= S9 && k < S9 + NFRAG<9>) load_ws1<9>(w9, ws, wave, lane16, k - S9);
                };
                hidden_ilv<8, KC8 * 6>(
                    [&](int j, int kc, int m, const u32x4 (&x)[3], f32x4 acc) {
                        return mfma_bf(kc < KS8 ? w8.v[j][kc][wpl(m)] : r8[kc & 1][wpl(m)], x[xpl(m)], acc);
                    },
                    stream8, hd, lds, wave, lane);
                load_ws<10>(w10, ws, wave, lane16);
                hd = pre_of<9>(lds, wave, lane);
                bar();
            } else {
                // Linear 8's streamed fragments issued half in Linear 5's MFMA slots, half in Linear 6's (all 24 in
                // Linear 6's measured slower, profiles/r6_mlp_tuning_ab.txt)
                constexpr int W8A = NFRAG<8> / 2;
                layer_res<0, W8A>(res, tail, [&](int k) { load_ws1<8>(w8, ws, wave, lane16, k); }, hd, lds, wave, lane);
                hd = pre_of<6>(lds, wave, lane);
                bar();
                layer_res<1, NFRAG<8> - W8A>(res, tail, [&](int k) { load_ws1<8>(w8, ws, wave, lane16, W8A + k); }, hd, lds, wave,
                                             lane);
                load_tail(tail, ws, wave, lane16);
                hd = pre_of<7>(lds, wave, lane);
                bar();
                layer_res<2>(res, tail, none, hd, lds, wave, lane);
                load_ws<9>(w9, ws, wave, lane16);
                hd = pre_of<8>(lds, wave, lane);
                bar();
                if (s + 1 < p.n_steps) sp = load_plan(p.plan, s + 1);
                if constexpr (STAGED_NOISE) {
                    ph_init(ph, p, s + 2, cand0, wave, lane);  // step s + 1's noise is Philox slice s + 2 (fetch_noise)
                    layer<8, NPH>(w8, [&](int k) { ph_step(ph, k); }, hd, lds, wave, lane);
                } else {
                    layer<8>(w8, none, hd, lds, wave, lane);
                }
                load_ws<10>(w10, ws, wave, lane16);  // after L8: w8's 96 registers are free again
                hd = pre_of<9>(lds, wave, lane);
                bar();
            }
            constexpr int NS9 = NFRAG<11> + NFRAG<12> + NFRAG<13>;
            if constexpr (W == 8) {
                // Linear 11's fragments behind Linear 9 (every wave has a tile there: no join; in its slots they do not
                // fit beside Linear 9's and 10's), Linear 12's and the final layer's behind Linear 10, where its own 12
                // fragments are spent
                layer<9>(w9, none, hd, lds, wave, lane);
                load_ws<11>(w11, ws, wave, lane16);
                hd = pre_of<10>(lds, wave, lane);
                bar();
                // This step's noise, drawn (or fetched) by waves 4-7, which have no tile in Linear 10-12 and the final
                // layer: lane for lane what wave - 4 would draw (fetch_noise: the same bits), handed over in the C0
                // buffer, which is dead from Linear 8's barrier to the next step's Linear 5; the final layer reads it
                // two barriers later. Waves 0-3 then carry no Philox state and no noise registers through the step.
                if constexpr (IS_DDPM)
                    if (wave >= 4) {
                        f32x4 nzh[NZT][NB];
                        fetch_noise(nzh, p, cur, s, cand0, n_cand, wave - 4, lane);
#pragma unroll
                        for (int j = 0; j < NZT; ++j)
                            *reinterpret_cast<f32x4 *>(lds + L::C0 + ((j * 4 + wave - 4) * 64 + lane) * 16) = nzh[j][0];
                    }
                layer<10>(w10, none, hd, lds, wave, lane);
                load_ws<12>(w12, ws, wave, lane16);
                load_ws<13>(w13, ws, wave, lane16);
            } else {
                layer<9, NS9>(w9, side9, hd, lds, wave, lane);
                hd = pre_of<10>(lds, wave, lane);
                bar();
                layer<10>(w10, none, hd, lds, wave, lane);
                noise_next();
                load_ws<0>(w0, ws, wave, lane16);  // next step's layer 0 (unconditional: path-independent load count)
            }
            hd = pre_of<11>(lds, wave, lane);
            bar();
            layer<11>(w11, none, hd, lds, wave, lane);
            hd = pre_of<12>(lds, wave, lane);
            // W = 8: the thread's table slot from the laundered lane, formed here in front of Linear 12's barrier (as a
            // loop invariant it stood in a register the step loop does not have: it was spilled)
            const int tid = wave * 64 + lane;
            int tpl = W == 8 ? (tid < COND_TOTAL / 4 ? tid : tid < COND_TOTAL / 2 ? tid - COND_TOTAL / 4 : 0) : tpi;
            if constexpr (W == 8) asm volatile("" : "+v"(tpl));
            bar();
            {
                // step s + 1's tables as Linear 12's side work: both reads in its first MFMA slot, the add and the
                // write in its last (Linear 11 read step s's tables last; the barrier above orders them)
                constexpr int NS12 = TL<12> * CL<12> * (A::K[12] / 32) * 6;
                const bool ctx_half = W == 8 ? tid >= COND_TOTAL / 4 : threadIdx.x >= COND_TOTAL / 4;
                const bool in_tab = W == 8 ? tid < COND_TOTAL / 2 : threadIdx.x < COND_TOTAL / 2;
                f32x4 tb0, tb1;
                layer<12, NS12>(w12, [&](int k) {
                    if (k == 0) {
                        tb0 = reinterpret_cast<const f32x4 *>(lds + L::BIC)[tpl];
                        tb1 = reinterpret_cast<const f32x4 *>(lds + L::CPS)[tpl];
                    } else if (k == NS12 - 1 && s + 1 < p.n_steps && in_tab) {
                        f32x4 u = tpre + tb0;
                        if (ctx_half) u = u + tb1;
                        reinterpret_cast<f32x4 *>(lds + (ctx_half ? L::TPC : L::TPU))[tpl] = u;
                    }
                }, hd, lds, wave, lane);
                // HEAD_PRE: unconditional (no load inside a branch ahead of the final layer's head); the last steps read
                // the last row again and do not use it
                if (HEAD_PRE || s + 1 < p.n_steps)
                    tpre = reinterpret_cast<const f32x4 *>(
                        p.tproj + (size_t)(s + 2 < p.n_steps ? s + 2 : HEAD_PRE ? p.n_steps - 1 : s + 1) * COND_TOTAL)[tpl];
            }
            if constexpr (W == 8 && !W0_LATE) load_ws<0>(w0, ws, wave, lane16);  // next step's layer 0, behind the final layer
            const FPre fhd = final_pre(lds, wave, lane);
            // W = 8: the noise waves 4-7 left in C0 behind Linear 9's barrier. One quad per lane: read here, two barriers
            // later and before the final layer's own; more quads: behind it (registers)
            auto take_noise = [&] {
#pragma unroll
                for (int j = 0; j < NZT; ++j) {
#pragma unroll
                    for (int g = 0; g < NB; ++g) nzc[j][g] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (IS_DDPM && wave < 4) nzc[j][0] = *reinterpret_cast<const f32x4 *>(lds + L::C0 + ((j * 4 + wave) * 64 + lane) * 16);
                }
            };
            if constexpr (W == 8 && NZT == 1) take_noise();
            bar();
            if constexpr (W == 8 && NZT != 1) take_noise();
            final_and_update(w13, fhd, lds, p, cur, s, cand0, n_cand, nzc, am, xr, wave, lane, tacc);
            if constexpr (W == 8 && W0_LATE) load_ws<0>(w0, ws, wave, lane16);  // H*d = 128: after the update's registers
        }
        MPCD_PROF_DUMP(W, threadIdx.x >> 6, lane);
        if (SMODE != MODE_EPS && SMODE != MODE_EPS1 && p.chain_absmax) {
            const int col = lane & 15;
            store_chain_absmax<CPW, NTH>(reinterpret_cast<uint32_t *>(lds + L::AMX), am, col,
                                          (NB == 2 || R == 16) ? -1 : 16 + col, NB == 1 || R == 32 || col < 8,
                                          p.chain_absmax, cand0, GRP ? cand0 + n_cand : p.batch);
        }
    }
};

template <int D0, int SMODE, bool CTX, int R, int W>
__global__ __launch_bounds__(64 * W, 1) void mlp_rw_kernel(const MlpSampleArgs p)
{
    MlpRw<D0, SMODE, CTX, R, W>::run(p);
}

// the grouped-context form (mpcd_sample_grouped): the same program with its workgroups aligned to the groups
template <int D0, int SMODE, int R, int W>
__global__ __launch_bounds__(64 * W, 1) void mlp_rw_grouped_kernel(const MlpSampleArgs p)
{
    MlpRw<D0, SMODE, true, R, W, true>::run(p);
}

template <int D0, int SMODE, bool CTX, int R, int W, bool GRP = false>
hipError_t launch_rw_r(const MlpSampleArgs &a, hipStream_t stream)
{
    using L = typename MlpRw<D0, SMODE, CTX, R, W>::L;
    static_assert(L::total <= 160 * 1024, "LDS budget (160 KiB per CU)");
    int64_t blocks;
    int32_t group_wgs;
    if (!cand_grid(L::CPW, a.batch, GRP ? a.group : 0, &blocks, &group_wgs)) return hipErrorInvalidValue;
    if constexpr (GRP) {
        static_assert(CTX, "grouped contexts need a context");
        if (hipError_t e = allow_max_lds<&mlp_rw_grouped_kernel<D0, SMODE, R, W>>(); e != hipSuccess) return e;
        MlpSampleArgs g = a;  // the workgroups of this layout per group
        g.group_wgs = group_wgs;
        return launch_sampler_kernel(mlp_rw_grouped_kernel<D0, SMODE, R, W>, dim3((unsigned)blocks), dim3(64 * W), (size_t)L::total, stream, g);
    } else {
        if (hipError_t e = allow_max_lds<&mlp_rw_kernel<D0, SMODE, CTX, R, W>>(); e != hipSuccess) return e;
        return launch_sampler_kernel(mlp_rw_kernel<D0, SMODE, CTX, R, W>, dim3((unsigned)blocks), dim3(64 * W), (size_t)L::total, stream, a);
    }
}

template <int D0, int SMODE, bool CTX, bool GRP = false>
hipError_t launch_rw(const MlpSampleArgs &a, int rows, int waves, hipStream_t stream)
{
    if (waves == 8) return rows == 32 ? launch_rw_r<D0, SMODE, CTX, 32, 8, GRP>(a, stream) : hipErrorInvalidValue;
    return rows == 16 ? launch_rw_r<D0, SMODE, CTX, 16, 4, GRP>(a, stream) : launch_rw_r<D0, SMODE, CTX, 32, 4, GRP>(a, stream);
}

}  // namespace

// rows: 32 or 16 per workgroup, waves: 4, or 8 at 32 rows (mlp_x3.hip picks, as for its own layouts)
hipError_t launch_mlp_rw(int d0, int rows, int waves, const MlpSampleArgs &a, hipStream_t stream)
{
    return sampler_dispatch(d0, a.mode, a.noise != nullptr, a.cproj != nullptr, a.group > 0,
                            [&](auto D0, auto SMODE, auto CTX, auto GRP) { return launch_rw<D0, SMODE, CTX, GRP>(a, rows, waves, stream); });
}
