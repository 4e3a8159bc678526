// hg_fused_bf16.h -- the bottom of an hourglass as ONE launch (hg_fused.h: same region, same op order, one workgroup per crop) with the
// arithmetic of the bf16 eval path (densereg.h, "precision"): both operands of every convolution rounded to bf16 (nearest even) as
// they enter the matrix cores, fp32 accumulation, fp32 folded BatchReNorm | ReLU | skip add.  num_fea = 64, 128, 192, 256.
//
// Multiply: v_mfma_f32_16x16x32_bf16.  Lane (r = lane & 15, g = lane >> 4) holds eight consecutive k (8 g .. 8 g + 7 of a 32-channel
// K-group) of row r for A and of column r for B; the accumulator is the one of the 16x16x4 fp32 instruction (register v = row 4 g + v,
// column r), so rows = pixels, columns = output channels and the epilogue indexing of hg_fused.h carries over.
//
// Weights: the bf16 path packs them [Kp/32][tap][Np][32], so a lane's B fragment of K-group (chunk, tap) and column n is the 16 bytes at
// ((chunk * taps + tap) * Np + n) * 32 + 8 g: one load from L2 into registers, no LDS staging.  They travel one convolution ahead
// (a 3x3 one 32-channel chunk ahead) -- with one or two waves per SIMD nothing else hides an L2 round trip.  Wave w owns the column tiles
// w, w + NW, ... and ALL row tiles; at F = 256 with four waves the first 1x1 is 8 K-groups x 2 tiles = 16 fragments = 64 VGPRs of
// prefetch, a 3x3 chunk 18 fragments, twice (this chunk and the next): 256 VGPRs + 126 AGPRs of the 512 a lane has at one wave per
// SIMD.  With eight waves (two per SIMD, 256 registers each) a wave owns half the column tiles and half the prefetch (239 VGPRs at
// F = 256) and the second wave hides LDS and L2 round trips of the first: measured 94 against 114 us per launch at F = 256, 40.6
// against 43.9 at F = 128 (profiles/hg_fused_bf16.md), so the launcher takes eight from F = 128 and four at F = 64, where there are
// no tiles for more.  A tile past the layer's last (F = 64: two half-width tiles for four waves; F = 192: six for eight) re-reads a
// live tile's weights and is never stored.
//
// LDS:
//   * the residual stream A (8x8), C (4x4), D (2x2) and the zero row are fp32 -- the skip add is an fp32 add and the result leaves to
//     HBM as fp32.  Row stride F + 8 floats (2 mod 4 sixteen-byte slots, the rule at HgShape).  Within every 32 channels the image is
//     stored as [half][g][4]: channel 8 g + 4 half + j sits at 16 half + 4 g + j, so the two ds_read_b128 of a lane's fragment (its
//     eight k, converted to bf16 in registers) each touch slot (stride r + g + const) mod 16 -- the access pattern the rule is about;
//     in channel order the lanes of a group would read slots stride r + 2 g, which no row stride keeps apart.  Pools and upsample-adds
//     work per float4 in place, whatever the order; only the first pool (from HBM) and the epilogue's column index know about it.
//   * the half-width tensors T1, T2 are read by convolutions only: the epilogue stores them as bf16 (the rounding the unfused path
//     does when it stages them), a fragment is ONE ds_read_b128 and no conversion.  Row stride F / 2 + 16 elements = F / 16 + 2
//     slots: 6, 10, 14, 18 = 2 (mod 16) for F = 64 .. 256.
//   85 (F + 8) 4 + 128 (F / 2 + 16) 2 bytes = 36 / 65 / 94 / 124 KB.
#pragma once
#include "hg_fused.h"

#if defined(DR_EMU)
// host stand-in of v_mfma_f32_16x16x32_bf16 (tests/hipemu/hip_emu.h has the 32x32x16 one): products of two bf16 are exact in fp32;
// the accumulation order inside the instruction is not architected (k order here)
static inline hipemu_f32x4 __builtin_amdgcn_mfma_f32_16x16x32_bf16(hipemu_bf16x8 a, hipemu_bf16x8 b, hipemu_f32x4 c, int, int, int) {
    hipemu::Wave& w = hipemu::my_wave();
    const int l = hipemu::lane_id();
    const unsigned bank = (hipemu::cur_fiber().coll++) & 1u;
    std::memcpy(&w.slot[bank][l][0], &a, 16);
    std::memcpy(&w.slot[bank][l][4], &b, 16);
    hipemu::sync_wave();
    auto bf = [](uint32_t word, int half) { uint32_t u = (half ? (word >> 16) : (word & 0xFFFFu)) << 16; float f; std::memcpy(&f, &u, 4); return f; };
    hipemu_f32x4 d = c;
    const int j = l & 15;
    for (int v = 0; v < 4; ++v) {
        const int i = 4 * (l >> 4) + v;
        float acc = c[v];
        for (int k = 0; k < 32; ++k) {
            const int src = 16 * (k >> 3), e = k & 7;
            acc = std::fmaf(bf(w.slot[bank][i + src][e >> 1], e & 1), bf(w.slot[bank][j + src][4 + (e >> 1)], e & 1), acc);
        }
        d[v] = acc;
    }
    return d;
}
#endif

namespace dr {

struct HgConvDesc16 { const __bf16* w; const float* scale; const float* shift; int Np; int pad_; };   // bf16 pack [Kp/32][tap][Np][32], folded BN
struct HgFusedParams16 {
    const float* x; int x_cs; int x_coff;          // [B][16][16] pixels, F channels at x_coff
    float* y; int y_cs; int y_coff;                // [B][8][8] pixels, F channels at y_coff
    int B, F;
    HgConvDesc16 conv[24];                         // residual modules 0..7 in the order of hg_fused.h, three convolutions each
};

inline bool hg_fused_bf16_supported(int F) { return F >= 64 && F % 64 == 0 && F <= 256; }
__host__ __device__ inline int hg_fused_bf16_lds_bytes(int F) { return (64 + 16 + 4 + 1) * (F + 8) * 4 + 2 * 64 * (F / 2 + 16) * 2; }

template <int F, int NW> struct Hg16Shape {
    static_assert(F % 64 == 0 && F >= 64 && F <= 256 && (NW == 4 || NW == 8), "num_fea 64, 128, 192, 256; four or eight waves");
    static constexpr int H = F / 2;
    static constexpr int sF = F + 8;               // row stride of the fp32 images, floats
    static constexpr int sH = H + 16;              // row stride of the bf16 images, elements
    static constexpr int CT1 = H / 16, CT3 = F / 16;                          // column tiles of the half-width / full-width outputs
    static constexpr int QC1 = (CT1 + NW - 1) / NW, QC3 = (CT3 + NW - 1) / NW;    // ... per wave
    static constexpr int NG1 = F / 32;             // K-groups of the first 1x1 (Cin = F)
    static constexpr int NC2 = H / 32;             // 32-channel chunks of the 3x3 (x 9 taps)
    static constexpr int NG3 = H / 32;             // K-groups of the last 1x1 (Cin = F / 2)
    static constexpr int nb_(int a, int b) { return a > b ? a : b; }
    static constexpr int NB = nb_(nb_(NG1 * QC1, 9 * QC1), NG3 * QC3);        // fragments of the largest prefetch
};

// fragments [K-group or tap][column tile of this wave], scale | shift per column tile
template <int NB> struct Hg16W { float4 b[NB]; float sc[4], sh[4]; };

// where channel n of an fp32 image sits in its row (header comment): [32-channel block][half][g][4]
__device__ __forceinline__ int hg16_pos(int n) { return (n & ~31) | ((n & 4) << 2) | ((n >> 1) & 12) | (n & 3); }

// hg_pool from HBM (16x16, channel order) into the 8x8 fp32 image (channel order of hg16_pos: a float4 moves as a whole)
__device__ __forceinline__ void hg16_pool_in(const float* src, int s_stride, float* dst, int d_stride, int C) {
    const int c4n = C >> 2, n = 64 * c4n;
    for (int i0 = threadIdx.x; i0 < n; i0 += 2 * blockDim.x) {
        float4 v[2][9];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + u * blockDim.x < n ? i0 + u * blockDim.x : i0;     // (a thread past the end re-reads its first element)
            const int c4 = i % c4n, px = i / c4n, ox = px & 7, oy = px >> 3;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ry = 2 * oy + t / 3, rx = 2 * ox + t % 3;
                const int iy = ry < 15 ? ry : 15, ix = rx < 15 ? rx : 15;
                v[u][t] = *reinterpret_cast<const float4*>(src + (long)(iy * 16 + ix) * s_stride + c4 * 4);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = i0 + u * blockDim.x;
            if (i >= n) break;
            float4 m = v[u][0];
#pragma unroll
            for (int t = 1; t < 9; ++t) {
                m.x = fmaxf(m.x, v[u][t].x); m.y = fmaxf(m.y, v[u][t].y); m.z = fmaxf(m.z, v[u][t].z); m.w = fmaxf(m.w, v[u][t].w);
            }
            *reinterpret_cast<float4*>(dst + (i / c4n) * d_stride + hg16_pos((i % c4n) * 4)) = m;
        }
    }
}

// which: 0 = first 1x1 (F -> F/2), 1 = 3x3 (F/2 -> F/2; chunk `chunk`), 2 = last 1x1 (F/2 -> F)
template <int F, int NW, int WHICH>
__device__ __forceinline__ void hg16_fetch(const HgConvDesc16& d, int chunk, Hg16W<Hg16Shape<F, NW>::NB>& w) {
    using S = Hg16Shape<F, NW>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    constexpr int CT = WHICH == 2 ? S::CT3 : S::CT1;
    constexpr int QC = WHICH == 2 ? S::QC3 : S::QC1;
    constexpr int NG = WHICH == 0 ? S::NG1 : WHICH == 1 ? 9 : S::NG3;
    const int g0 = WHICH == 1 ? chunk * 9 : 0;
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        const int ct = wave + NW * q;
        const int n = (ct < CT ? ct : (wave < CT ? wave : 0)) * 16 + r;     // (a dead tile re-reads a live one: never stored)
        const __bf16* wp = d.w + (long)n * 32 + 8 * g;
        if (WHICH != 1 || chunk == 0) { w.sc[q] = d.scale[n]; w.sh[q] = d.shift[n]; }
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) w.b[gi * QC + q] = *reinterpret_cast<const float4*>(wp + (long)(g0 + gi) * d.Np * 32);
    }
}

// Everything a module computes from the lane index alone (tap offsets, fragment and epilogue addresses: some 150 values at F = 256) is
// invariant in the kernel's loop over the modules: hoisted out of it, it lives through every convolution next to the weight prefetch
// and spills.  The lane index goes through here once per module, so it is recomputed there (a few hundred VALU per module).
#if defined(DR_EMU)
static inline int hg16_per_module(int v) { return v; }
#else
__device__ __forceinline__ int hg16_per_module(int v) { asm volatile("" : "+v"(v)); return v; }
#endif

__device__ __forceinline__ dr_f32x4 hg16_mma(const float4 a, const float4 b, const dr_f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dr_bf16x8, a), __builtin_bit_cast(dr_bf16x8, b), c, 0, 0, 0);
}

// A fragment from an fp32 image: the lane's two float4 (channels 8 g .. + 3 at p, 8 g + 4 .. + 7 at p + 16) rounded to bf16 the way
// the BF = 1 convolution kernels round when they stage (conv_igemm.h)
__device__ __forceinline__ float4 hg16_afrag(const float* p) {
    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 16);
    const dr_f32x8 f = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(float4, __builtin_convertvector(f, dr_bf16x8));
}

// Epilogues of one column tile: folded BatchReNorm + ReLU.  NRT > 1: accumulator t is row tile t; NRT == 1: the K-groups alternated
// between two accumulators (a single tile would be one dependent chain), summed here.
template <int NRT>
__device__ __forceinline__ void hg16_store_half(dr_f32x4 (&acc)[4], int g, int M, int n, float sc, float sh, __bf16* dst, int d_stride) {
    if (NRT == 1) acc[0] = acc[0] + acc[1];
#pragma unroll
    for (int t = 0; t < NRT; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int p = t * 16 + 4 * g + v;
            if (p < M) dst[p * d_stride + n] = (__bf16)fmaxf(acc[t][v] * sc + sh, 0.f);
        }
}
// ... + skip, in place on the fp32 image (column n at hg16_pos(n)); gout != null: to HBM instead
template <int NRT>
__device__ __forceinline__ void hg16_store_full(dr_f32x4 (&acc)[4], int g, int M, int n, float sc, float sh, float* X, int x_stride, float* gout, int g_stride) {
    const int xn = hg16_pos(n);
    if (NRT == 1) acc[0] = acc[0] + acc[1];
#pragma unroll
    for (int t = 0; t < NRT; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int p = t * 16 + 4 * g + v;
            if (p >= M) continue;
            const float val = fmaxf(acc[t][v] * sc + sh, 0.f) + X[p * x_stride + xn];
            if (gout) gout[(long)p * g_stride + n] = val;
            else X[p * x_stride + xn] = val;
        }
}

// One residual module in place on X (side x side pixels, M = side^2 live rows).  RT4: the 8x8 level, four row tiles; otherwise one.
// w1: the first convolution's weights (fetched by whoever ran before); nd: the NEXT module's descriptors (its first convolution is
// fetched under this module's last), null at the end.
template <int F, bool RT4, int NW>
__device__ __forceinline__ void hg16_residual(float* X, int side, int side_shift, int M, const HgConvDesc16* d, __bf16* T1, __bf16* T2, const float* zrow,
                                              float* gout, int g_stride, Hg16W<Hg16Shape<F, NW>::NB>& w1, const HgConvDesc16* nd) {
    using S = Hg16Shape<F, NW>;
    using W = Hg16W<S::NB>;
    constexpr int NRT = RT4 ? 4 : 1;
    const int lane = hg16_per_module(threadIdx.x & 63), wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const __bf16* zb = reinterpret_cast<const __bf16*>(zrow);       // (zero bits are zero in both formats)
    int pix[NRT];
    bool p_ok[NRT];
#pragma unroll
    for (int t = 0; t < NRT; ++t) { pix[t] = t * 16 + r; p_ok[t] = pix[t] < M; }
    W w2, w3;
    dr_f32x4 acc[S::QC3][4];                                        // [column tile of this wave][row tile, or K-group parity]
    static_assert(S::QC1 <= S::QC3, "the half-width layers have the fewer tiles");

    // ---- 1x1, F -> F/2:  X -> T1 ----------------------------------------------------------------------------------------------
    hg16_fetch<F, NW, 1>(d[1], 0, w2);                              // the 3x3's first chunk travels under this convolution
    if (wave < S::CT1) {
#pragma unroll
        for (int q = 0; q < S::QC1; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[q][a][v] = 0.f;
        const float* ap[NRT];
#pragma unroll
        for (int t = 0; t < NRT; ++t) ap[t] = (p_ok[t] ? X + pix[t] * S::sF : zrow) + 4 * g;
        // (the fragments of K-group gi + 1 are read before the MFMAs of group gi are issued, as in hg_fused.h)
        float4 a[2][NRT];
#pragma unroll
        for (int t = 0; t < NRT; ++t) a[0][t] = hg16_afrag(ap[t]);
#pragma unroll
        for (int gi = 0; gi < S::NG1; ++gi) {
            if (gi + 1 < S::NG1) {
#pragma unroll
                for (int t = 0; t < NRT; ++t) a[(gi + 1) & 1][t] = hg16_afrag(ap[t] + (gi + 1) * 32);
            }
#pragma unroll
            for (int q = 0; q < S::QC1; ++q)
#pragma unroll
                for (int t = 0; t < NRT; ++t) {
                    const int ai = NRT > 1 ? t : gi & 1;
                    acc[q][ai] = hg16_mma(a[gi & 1][t], w1.b[gi * S::QC1 + q], acc[q][ai]);
                }
        }
#pragma unroll
        for (int q = 0; q < S::QC1; ++q)
            if (wave + NW * q < S::CT1) hg16_store_half<NRT>(acc[q], g, M, (wave + NW * q) * 16 + r, w1.sc[q], w1.sh[q], T1, S::sH);
    }
    __syncthreads();
    // ---- 3x3, F/2 -> F/2:  T1 -> T2 -------------------------------------------------------------------------------------------
    {
        const bool live = wave < S::CT1;
        // this lane's nine taps per row tile as element offsets into T1 (a tap outside the image, or a dead row: the zero row)
        const int zoff = (int)(zb - T1);
        int tp[NRT][9];
#pragma unroll
        for (int t = 0; t < NRT; ++t) {
            const int y = pix[t] >> side_shift, x = pix[t] & (side - 1);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                const bool ok = p_ok[t] && yy >= 0 && yy < side && xx >= 0 && xx < side;
                tp[t][tap] = (ok ? ((yy << side_shift) + xx) * S::sH : zoff) + 8 * g;
            }
        }
#pragma unroll
        for (int q = 0; q < S::QC1; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[q][a][v] = 0.f;
        W wn;
        float4 a2[2][NRT];
#pragma unroll
        for (int c = 0; c < S::NC2; ++c) {
            if (c + 1 < S::NC2) hg16_fetch<F, NW, 1>(d[1], c + 1, (c & 1) ? w2 : wn);     // the next chunk's nine taps, under this one's MFMAs
            else hg16_fetch<F, NW, 2>(d[2], 0, w3);                                        // ... or the last 1x1's weights
            const W& wc = (c & 1) ? wn : w2;
            if (live) {
                if (c == 0) {
#pragma unroll
                    for (int t = 0; t < NRT; ++t) a2[0][t] = *reinterpret_cast<const float4*>(T1 + tp[t][0]);
                }
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int gi = c * 9 + tap;                    // (compile-time after unrolling: the buffer parity is static)
                    if (gi + 1 < S::NC2 * 9) {
                        const int nc = tap == 8 ? c + 1 : c, nt = tap == 8 ? 0 : tap + 1;
#pragma unroll
                        for (int t = 0; t < NRT; ++t) a2[(gi + 1) & 1][t] = *reinterpret_cast<const float4*>(T1 + tp[t][nt] + nc * 32);
                    }
#pragma unroll
                    for (int q = 0; q < S::QC1; ++q)
#pragma unroll
                        for (int t = 0; t < NRT; ++t) {
                            const int ai = NRT > 1 ? t : gi & 1;
                            acc[q][ai] = hg16_mma(a2[gi & 1][t], wc.b[tap * S::QC1 + q], acc[q][ai]);
                        }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < S::QC1; ++q)
                if (wave + NW * q < S::CT1) hg16_store_half<NRT>(acc[q], g, M, (wave + NW * q) * 16 + r, w2.sc[q], w2.sh[q], T2, S::sH);
        }
    }
    __syncthreads();
    // ---- 1x1, F/2 -> F, + skip:  T2 -> X (in place) or HBM ---------------------------------------------------------------------------
    if (nd) hg16_fetch<F, NW, 0>(nd[0], 0, w1);                     // the next module's first convolution
    if (wave < S::CT3) {
#pragma unroll
        for (int q = 0; q < S::QC3; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[q][a][v] = 0.f;
        const __bf16* ap[NRT];
#pragma unroll
        for (int t = 0; t < NRT; ++t) ap[t] = (p_ok[t] ? T2 + pix[t] * S::sH : zb) + 8 * g;
        float4 a[2][NRT];
#pragma unroll
        for (int t = 0; t < NRT; ++t) a[0][t] = *reinterpret_cast<const float4*>(ap[t]);
#pragma unroll
        for (int gi = 0; gi < S::NG3; ++gi) {
            if (gi + 1 < S::NG3) {
#pragma unroll
                for (int t = 0; t < NRT; ++t) a[(gi + 1) & 1][t] = *reinterpret_cast<const float4*>(ap[t] + (gi + 1) * 32);
            }
#pragma unroll
            for (int q = 0; q < S::QC3; ++q)
#pragma unroll
                for (int t = 0; t < NRT; ++t) {
                    const int ai = NRT > 1 ? t : gi & 1;
                    acc[q][ai] = hg16_mma(a[gi & 1][t], w3.b[gi * S::QC3 + q], acc[q][ai]);
                }
        }
#pragma unroll
        for (int q = 0; q < S::QC3; ++q)
            if (wave + NW * q < S::CT3)
                hg16_store_full<NRT>(acc[q], g, M, (wave + NW * q) * 16 + r, w3.sc[q], w3.sh[q], X, S::sF, gout, g_stride);
    }
    __syncthreads();
}

template <int F, int NW>
__global__ __launch_bounds__(NW * 64, 1) void hg_tail_eval_bf16_kernel(const HgFusedParams16 p) {
    using S = Hg16Shape<F, NW>;
    DR_DYN_SMEM(smem_raw);
    float* A = reinterpret_cast<float*>(smem_raw);
    float* C = A + 64 * S::sF;
    float* D = C + 16 * S::sF;
    float* Z = D + 4 * S::sF;
    __bf16* T1 = reinterpret_cast<__bf16*>(Z + S::sF);
    __bf16* T2 = T1 + 64 * S::sH;
    for (int i = threadIdx.x; i < S::sF; i += blockDim.x) Z[i] = 0.f;
    const int b = blockIdx.x;
    Hg16W<S::NB> w1;
    hg16_fetch<F, NW, 0>(p.conv[0], 0, w1);                        // the first weights travel while the input is pooled
    hg16_pool_in(p.x + (long)b * 256 * p.x_cs + p.x_coff, p.x_cs, A, S::sF, F);
    __syncthreads();
    // the eight residual modules of hg_fused.h; what happens in front of module r: 1 C = pool(A), 3 D = pool(C), 6 C += up(D), 7 A += up(C)
#pragma clang loop unroll(disable)
    for (int r = 0; r < 8; ++r) {
        if (r == 1) { hg_pool(A, S::sF, 8, C, S::sF, F); __syncthreads(); }
        else if (r == 3) { hg_pool(C, S::sF, 4, D, S::sF, F); __syncthreads(); }
        else if (r == 6) { hg_upadd(C, 4, D, S::sF, F); __syncthreads(); }
        else if (r == 7) { hg_upadd(A, 8, C, S::sF, F); __syncthreads(); }
        const HgConvDesc16* d = p.conv + 3 * r;
        const HgConvDesc16* nd = r < 7 ? d + 3 : nullptr;
        if (r <= 1 || r == 7) {
            hg16_residual<F, true, NW>(A, 8, 3, 64, d, T1, T2, Z, r == 7 ? p.y + (long)b * 64 * p.y_cs + p.y_coff : nullptr, p.y_cs, w1, nd);
        } else {
            const bool four = r == 2 || r == 3 || r == 6;            // 4x4 on C, else 2x2 on D
            hg16_residual<F, false, NW>(four ? C : D, four ? 4 : 2, four ? 2 : 1, four ? 16 : 4, d, T1, T2, Z, nullptr, 0, w1, nd);
        }
    }
}

}  // namespace dr
