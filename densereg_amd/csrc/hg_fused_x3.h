// hg_fused_x3.h -- the bottom of an hourglass as ONE launch (hg_fused.h: same region, same op order, in-place residual modules, one
// workgroup per crop) for fp32 handles with num_fea = 192 and 256, where hg_fused.h's fp32 MFMAs would be ~200 us of issue per crop.
//
// Arithmetic: the three-way bf16 split of conv_x3.h on v_mfma_f32_16x16x32_bf16.  a = a0 + a1 + a2 and b = b0 + b1 + b2, every level
// rounded to nearest even (activations: x3_split4; weights: x3_store_planes, read from the handle's planes as they are),
//        a b  ~=  a0 b0  +  (a0 b1 + a1 b0 + a0 b2 + a1 b1 + a2 b0)
// with the leading product in one fp32 accumulator and the five corrections in another, added once in front of the epilogue.  The
// residual stream, the folded BatchReNorm scale | shift, the ReLU and the skip add are fp32; the result leaves as fp32.
//
// Fragments: lane (r = lane & 15, g = lane >> 4) holds the eight k 8 g .. 8 g + 7 of a 32-channel K-group G, of row r for A and of
// column r for B; accumulator register v is (row 4 g + v, column r) (hg_fused_bf16.h).  The planes are packed [Kp/16][tap][Np][3][16],
// so the lane's eight k of column n, plane p are the 16 bytes at element (((2 G + (g >> 1)) taps + tap) Np + n) 48 + 16 p + 8 (g & 1):
// 16-channel chunk 2 G + (g >> 1) holds k 32 G + 16 (g >> 1) + kk, and kk = 8 (g & 1) + e gives k = 32 G + 8 g + e.
//
// 1. LDS.  The residual stream A (8x8), C (4x4), D (2x2) and the zero row are fp32, row stride F + 8 floats, channel order [half][g][4]
//    within every 32 channels (hg16_pos).  T1 and T2 are fp32 at BOTH widths, row stride F / 2 + 8 floats (26 | 34 sixteen-byte slots
//    = 10 | 2 mod 16, the rule at HgShape), same channel order: 85 (F + 8) 4 + 128 (F / 2 + 8) 4 bytes = 121 248 at F = 192 and
//    159 392 of the 163 840 at F = 256.  Planes for T1 | T2 would fit at 192 and not at 256; one storage means one set of six
//    convolution bodies, and the 8x8 levels do not need the planes (2.).  The 4x4 and 2x2 levels use one 16-row tile and leave T1 | T2
//    free: there the region holds bf16 PLANE scratch, [plane][17 rows][K + 16] per tensor (row 16 = zeros: 3x3 taps outside the image
//    and rows past the level's last; row stride K / 8 + 2 slots = 2 mod 4): PX (the module's input, K = F), PT1, PT2 (K = F / 2),
//    57 120 bytes at F = 256.
// 2. Who splits.  x3_split4 is ~38 VALU per four values, 76 per A fragment.
//    8x8 (four row tiles): wave w owns ROW TILE w & 3 and every (NW / 4)-th column tile, so one split feeds 6 MFMAs x its column
//    tiles: with eight waves 4 | 4 | 8 tiles at F = 256 (first 1x1 | 3x3 | last 1x1), 3 | 3 | 6 at F = 192 -- 3.2 | 3.2 | 1.6 and
//    4.2 | 4.2 | 2.1 VALU per MFMA where "every wave owns all rows" would be 12.7.  The price is that a weight fragment is fetched by
//    the four waves of a column group (the same lines at about the same time: L1 hits, but four times the return traffic).
//    4x4, 2x2 (one row tile): no split in the K loop at all.  The module's input is split once by all threads into PX (3 x3_split4 per
//    thread at most); the half-width epilogues split the four values a lane holds (one x3_split4 per column tile) and store PLANES, so
//    T1 and T2 never exist as fp32 there; wave w owns the column tiles w, w + NW, ... and a fragment is three ds_read_b128.
// 3. Weights.  A fragment is three planes = 12 VGPRs per (K-group, column tile).  They travel through a ring of RING fragments per
//    wave: the convolution walks its fragments in the order (K-group, column tile), multiplies from slot i % RING and at once refills
//    that slot with fragment i + RING -- past the end of a convolution with the first fragments of the NEXT one (of the next module
//    behind the last 1x1: its level is a run-time value, both address forms are compiled), so no convolution starts on an empty
//    ring.  Everything is unrolled, every slot index is static.  Dead column tiles (F = 192: six half-width tiles on eight waves)
//    re-read a live tile's weights and are never stored, as in the sibling kernels.
//    Measured (profiles/hg_fused_x3.md, B = 1, per launch): eight waves 362 us at F = 256 and 166 us at F = 192 with a ring of six,
//    374 and 161 us with four; four waves 741 and 242 us (ring four: six spills at F = 256).  Eight and six are what the launcher
//    builds.  The launch replaces 332 us of launches at F = 256 -- it is SLOWER there at B = 1 -- and 275 us at F = 192: it is bound by
//    the weight stream (the 8x8 levels fetch every fragment four times), not by the matrix cores.
// 4. Code size.  The kernel is the run-time loop over the eight modules of hg_fused.h around six convolution bodies
//    {1x1 in, 3x3, 1x1 out} x {8x8, one row tile}, all six from ONE template (hgx3_conv).
#pragma once
#include "conv_x3.h"
#include "hg_fused_bf16.h"

#if !defined(DR_HGX3_WAVES)
#define DR_HGX3_WAVES 8              // measurement builds override these two (profiles/hg_fused_x3.md); the product is the default
#endif
#if !defined(DR_HGX3_RING)
#define DR_HGX3_RING 6
#endif

namespace dr {

struct HgConvDescX3 { const __bf16* w; const float* scale; const float* shift; int Np; int pad_; };   // planes [Kp/16][tap][Np][3][16], folded BN
struct HgFusedParamsX3 {
    const float* x; int x_cs; int x_coff;          // [B][16][16] pixels, F channels at x_coff
    float* y; int y_cs; int y_coff;                // [B][8][8] pixels, F channels at y_coff
    int B, F;
    HgConvDescX3 conv[24];                         // residual modules 0..7 in the order of hg_fused.h, three convolutions each
};

inline bool hg_fused_x3_supported(int F) { return F == 192 || F == 256; }
__host__ __device__ inline int hg_fused_x3_lds_bytes(int F) { return (64 + 16 + 4 + 1) * (F + 8) * 4 + 2 * 64 * (F / 2 + 8) * 4; }

template <int F, int NW> struct HgX3Shape {
    static_assert((F == 192 || F == 256) && (NW == 4 || NW == 8), "num_fea 192, 256; four or eight waves");
    static constexpr int H = F / 2;
    static constexpr int sF = F + 8, sH = H + 8;   // row strides of the fp32 images, floats
    static constexpr int pF = F + 16, pH = H + 16; // row strides of the plane scratch, bf16 elements
    static constexpr int PR = 17;                  // rows of a plane (16 = the zero row)
    static constexpr int CT1 = H / 16, CT3 = F / 16;
    static constexpr int NCG = NW / 4;             // column groups of the 8x8 levels (a wave: row tile w & 3, group w >> 2)
    static constexpr int NG1 = F / 32, NC2 = H / 32, NG3 = H / 32;
    static constexpr int oPX = 0, oPT1 = 3 * PR * pF, oPT2 = oPT1 + 3 * PR * pH, oEnd = oPT2 + 3 * PR * pH;      // elements into T1
    static_assert(CT1 % NCG == 0 && oEnd * 2 <= 2 * 64 * sH * 4, "the plane scratch lives in T1 | T2");
};

// the fragments of convolution WHICH (0 = first 1x1 F -> F/2, 1 = 3x3, 2 = last 1x1 F/2 -> F) of a wave, on an 8x8 level (RT4) or a
// one-row-tile level, in the order they are multiplied: fragment j = (K-group j / QC, column tile slot j % QC)
template <int F, int NW, int WHICH, bool RT4> struct HgX3Seq {
    using S = HgX3Shape<F, NW>;
    static constexpr int TAPS = WHICH == 1 ? 9 : 1;
    static constexpr int CT = WHICH == 2 ? S::CT3 : S::CT1;
    static constexpr int QC = RT4 ? CT / S::NCG : (CT + NW - 1) / NW;
    static constexpr int NKG = WHICH == 0 ? S::NG1 : WHICH == 1 ? 9 * S::NC2 : S::NG3;
    static constexpr int N = NKG * QC;
    static_assert(N >= DR_HGX3_RING, "a convolution is at least one ring long");
    // column tile of slot q, and whether it is stored (a dead tile re-reads a live one)
    static __device__ __forceinline__ int tile(int wave, int q) {
        if (RT4) return (wave >> 2) + S::NCG * q;
        const int ct = wave + NW * q;
        return ct < CT ? ct : (wave < CT ? wave : 0);
    }
    static __device__ __forceinline__ bool live(int wave, int q) { return RT4 || wave + NW * q < CT; }
    static __device__ __forceinline__ void load(const HgConvDescX3& d, int j, int wave, int r, int g, float4 (&b)[3]) {
        const int kg = j / QC, G = kg / TAPS, tap = kg % TAPS;
        const int n = tile(wave, j % QC) * 16 + r;
        const __bf16* p = d.w + ((long)((2 * G + (g >> 1)) * TAPS + tap) * d.Np + n) * 48 + 8 * (g & 1);
        b[0] = *reinterpret_cast<const float4*>(p);
        b[1] = *reinterpret_cast<const float4*>(p + 16);
        b[2] = *reinterpret_cast<const float4*>(p + 32);
    }
};

struct HgX3Ring { float4 b[DR_HGX3_RING][3]; };

__device__ __forceinline__ float4 hgx3_f4(unsigned a, unsigned b, unsigned c, unsigned d) {
    return make_float4(__builtin_bit_cast(float, a), __builtin_bit_cast(float, b), __builtin_bit_cast(float, c), __builtin_bit_cast(float, d));
}
// A planes of a lane's eight fp32 k (lo: k 0..3, hi: k 4..7)
__device__ __forceinline__ void hgx3_split8(const float4 lo, const float4 hi, float4 (&a)[3]) {
    uint2 l0, l1, l2, u0, u1, u2;
    x3_split4(lo, l0, l1, l2);
    x3_split4(hi, u0, u1, u2);
    a[0] = hgx3_f4(l0.x, l0.y, u0.x, u0.y); a[1] = hgx3_f4(l1.x, l1.y, u1.x, u1.y); a[2] = hgx3_f4(l2.x, l2.y, u2.x, u2.y);
}
// the six products of one (A fragment, B fragment): leading term | corrections
__device__ __forceinline__ void hgx3_mma6(const float4 (&a)[3], const float4 (&b)[3], dr_f32x4& lead, dr_f32x4& corr) {
    lead = hg16_mma(a[0], b[0], lead);
    corr = hg16_mma(a[0], b[1], corr);
    corr = hg16_mma(a[1], b[0], corr);
    corr = hg16_mma(a[0], b[2], corr);
    corr = hg16_mma(a[1], b[1], corr);
    corr = hg16_mma(a[2], b[0], corr);
}

// channel of position `pos` of an fp32 image row (the inverse of hg16_pos on multiples of four)
__device__ __forceinline__ int hgx3_chan(int pos) { return (pos & ~31) | ((pos & 16) >> 2) | ((pos & 12) << 1); }

// one-row-tile levels: the module's input X (M live rows) -> the planes PX, and the zero rows of PX | PT1 | PT2
template <int F, int NW>
__device__ __forceinline__ void hgx3_split_in(const float* X, int M, __bf16* P) {
    using S = HgX3Shape<F, NW>;
    for (int i = threadIdx.x; i < M * (F / 4); i += blockDim.x) {
        const int row = i / (F / 4), pos = (i % (F / 4)) * 4;
        uint2 h0, h1, h2;
        x3_split4(*reinterpret_cast<const float4*>(X + row * S::sF + pos), h0, h1, h2);
        __bf16* d = P + S::oPX + row * S::pF + hgx3_chan(pos);
        *reinterpret_cast<uint2*>(d) = h0;
        *reinterpret_cast<uint2*>(d + S::PR * S::pF) = h1;
        *reinterpret_cast<uint2*>(d + 2 * S::PR * S::pF) = h2;
    }
    const uint2 z = make_uint2(0u, 0u);
    for (int i = threadIdx.x; i < 3 * (S::pF / 4); i += blockDim.x)
        *reinterpret_cast<uint2*>(P + S::oPX + ((i / (S::pF / 4)) * S::PR + 16) * S::pF + (i % (S::pF / 4)) * 4) = z;
    for (int i = threadIdx.x; i < 6 * (S::pH / 4); i += blockDim.x)     // (PT1 and PT2 are adjacent: six planes of PR rows)
        *reinterpret_cast<uint2*>(P + S::oPT1 + ((i / (S::pH / 4)) * S::PR + 16) * S::pH + (i % (S::pH / 4)) * 4) = z;
}

// One convolution.  RT4: rows = this wave's row tile of the 8x8 image, A from the fp32 image `src` (row stride ss floats), split in
// registers; otherwise A from the planes `psrc` (row stride ps elements).  Output: WHICH < 2 -> the fp32 image dst (RT4) or the planes
// pdst; WHICH == 2 -> + skip, in place on X or to HBM (gout).  ring: this convolution's first RING fragments on entry, the next one's on
// exit (nd: its descriptor, null behind the region's last; nrt4: whether it runs on an 8x8 level -- only the last 1x1 asks).
template <int F, int NW, int WHICH, bool RT4>
__device__ __forceinline__ void hgx3_conv(const HgConvDescX3& d, const HgConvDescX3* nd, bool nrt4, HgX3Ring& ring, int lane, int side, int side_shift,
                                          int M, const float* src, float* dst, const __bf16* psrc, __bf16* pdst, const float* zrow, float* X,
                                          float* gout, int g_stride) {
    using S = HgX3Shape<F, NW>;
    using Q = HgX3Seq<F, NW, WHICH, RT4>;
    constexpr int D = DR_HGX3_RING, QC = Q::QC, NKG = Q::NKG, N = Q::N;
    constexpr int K = WHICH == 0 ? F : S::H;                       // input channels
    constexpr int ss = WHICH == 0 ? S::sF : S::sH, ps = WHICH == 0 ? S::pF : S::pH;
    const int wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int pix = RT4 ? (wave & 3) * 16 + r : r;
    const bool p_ok = pix < M;
    const __bf16* zb = reinterpret_cast<const __bf16*>(zrow);
    (void)K; (void)zb;

    float sc[QC], sh[QC];
    dr_f32x4 lead[QC], corr[QC];
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        const int n = Q::tile(wave, q) * 16 + r;
        sc[q] = d.scale[n]; sh[q] = d.shift[n];
#pragma unroll
        for (int v = 0; v < 4; ++v) { lead[q][v] = 0.f; corr[q][v] = 0.f; }
    }
    // this lane's A address per tap, in elements of the source (fp32 image: floats; planes: bf16 of plane 0); a tap outside the image or a
    // row past the last reads zeros
    int tp[Q::TAPS];
#pragma unroll
    for (int tap = 0; tap < Q::TAPS; ++tap) {
        int row = pix;
        bool ok = p_ok;
        if (WHICH == 1) {
            const int yy = (pix >> side_shift) + tap / 3 - 1, xx = (pix & (side - 1)) + tap % 3 - 1;
            ok = ok && yy >= 0 && yy < side && xx >= 0 && xx < side;
            row = (yy << side_shift) + xx;
        }
        if (RT4) tp[tap] = (ok ? row * ss : (int)(zrow - src)) + 4 * g;
        else tp[tap] = (ok ? row : 16) * ps + 8 * g;
    }
    // raw A of K-group kg: RT4 two float4 of fp32, otherwise the three planes
    float4 raw[2][3];
    auto read_a = [&](int kg, float4 (&o)[3]) {
        const int G = kg / Q::TAPS, tap = kg % Q::TAPS;
        if (RT4) {
            const float* p = src + tp[tap] + G * 32;
            o[0] = *reinterpret_cast<const float4*>(p);
            o[1] = *reinterpret_cast<const float4*>(p + 16);
        } else {
            const __bf16* p = psrc + tp[tap] + G * 32;
            o[0] = *reinterpret_cast<const float4*>(p);
            o[1] = *reinterpret_cast<const float4*>(p + S::PR * ps);
            o[2] = *reinterpret_cast<const float4*>(p + 2 * S::PR * ps);
        }
    };
    read_a(0, raw[0]);
#pragma unroll
    for (int kg = 0; kg < NKG; ++kg) {
        if (kg + 1 < NKG) read_a(kg + 1, raw[(kg + 1) & 1]);     // (the next group's LDS reads are issued in front of this group's MFMAs)
        float4 a[3];
        if (RT4) hgx3_split8(raw[kg & 1][0], raw[kg & 1][1], a);
        else { a[0] = raw[kg & 1][0]; a[1] = raw[kg & 1][1]; a[2] = raw[kg & 1][2]; }
#pragma unroll
        for (int q = 0; q < QC; ++q) {
            const int i = kg * QC + q, slot = i % D;               // (static after unrolling)
            hgx3_mma6(a, ring.b[slot], lead[q], corr[q]);
            if (i + D < N) Q::load(d, i + D, wave, r, g, ring.b[slot]);
            else if (WHICH == 0) HgX3Seq<F, NW, 1, RT4>::load(*nd, slot, wave, r, g, ring.b[slot]);
            else if (WHICH == 1) HgX3Seq<F, NW, 2, RT4>::load(*nd, slot, wave, r, g, ring.b[slot]);
            else if (nd) {
                if (nrt4) HgX3Seq<F, NW, 0, true>::load(*nd, slot, wave, r, g, ring.b[slot]);
                else HgX3Seq<F, NW, 0, false>::load(*nd, slot, wave, r, g, ring.b[slot]);
            }
        }
    }
    // ---- epilogue: folded BatchReNorm + ReLU; accumulator register v is (row 4 g + v, column r) of the tile --------------------
    const int row0 = (RT4 ? (wave & 3) * 16 : 0) + 4 * g;
#pragma unroll
    for (int q = 0; q < QC; ++q) {
        if (!Q::live(wave, q)) continue;
        const int n = Q::tile(wave, q) * 16 + r;
        const dr_f32x4 s = lead[q] + corr[q];
        float val[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) val[v] = fmaxf(s[v] * sc[q] + sh[q], 0.f);
        if (WHICH == 2) {
            const int xn = hg16_pos(n);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int p = row0 + v;
                if (p >= M) continue;
                const float o = val[v] + X[p * S::sF + xn];
                if (gout) gout[(long)p * g_stride + n] = o;
                else X[p * S::sF + xn] = o;
            }
        } else if (RT4) {
            const int xn = hg16_pos(n);
#pragma unroll
            for (int v = 0; v < 4; ++v) dst[(row0 + v) * S::sH + xn] = val[v];
        } else {
            uint2 h[3];
            x3_split4(make_float4(val[0], val[1], val[2], val[3]), h[0], h[1], h[2]);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                unsigned short* o = reinterpret_cast<unsigned short*>(pdst) + (pl * S::PR + row0) * S::pH + n;
                if (row0 + 0 < M) o[0] = (unsigned short)(h[pl].x & 0xFFFFu);
                if (row0 + 1 < M) o[S::pH] = (unsigned short)(h[pl].x >> 16);
                if (row0 + 2 < M) o[2 * S::pH] = (unsigned short)(h[pl].y & 0xFFFFu);
                if (row0 + 3 < M) o[3 * S::pH] = (unsigned short)(h[pl].y >> 16);
            }
        }
    }
}

// One residual module in place on X (side x side pixels, M = side^2 live rows).  T: the T1 | T2 region.  nd: the next module's
// descriptors (null at the end), nrt4: whether it runs at 8x8.
template <int F, int NW, bool RT4>
__device__ __forceinline__ void hgx3_residual(float* X, int side, int side_shift, int M, const HgConvDescX3* d, float* T, const float* zrow, float* gout,
                                              int g_stride, HgX3Ring& ring, const HgConvDescX3* nd, bool nrt4) {
    using S = HgX3Shape<F, NW>;
    const int lane = hg16_per_module(threadIdx.x & 63);           // (hg_fused_bf16.h: lane-derived addresses are recomputed per module)
    float* T1 = T;
    float* T2 = T + 64 * S::sH;
    __bf16* P = reinterpret_cast<__bf16*>(T);
    if (!RT4) { hgx3_split_in<F, NW>(X, M, P); __syncthreads(); }
    hgx3_conv<F, NW, 0, RT4>(d[0], d + 1, RT4, ring, lane, side, side_shift, M, X, T1, P + S::oPX, P + S::oPT1, zrow, X, nullptr, 0);
    __syncthreads();
    hgx3_conv<F, NW, 1, RT4>(d[1], d + 2, RT4, ring, lane, side, side_shift, M, T1, T2, P + S::oPT1, P + S::oPT2, zrow, X, nullptr, 0);
    __syncthreads();
    hgx3_conv<F, NW, 2, RT4>(d[2], nd, nrt4, ring, lane, side, side_shift, M, T2, nullptr, P + S::oPT2, nullptr, zrow, X, gout, g_stride);
    __syncthreads();
}

template <int F, int NW>
__global__ __launch_bounds__(NW * 64, 1) void hg_tail_eval_x3_kernel(const HgFusedParamsX3 p) {
    using S = HgX3Shape<F, NW>;
    DR_DYN_SMEM(smem_raw);
    float* A = reinterpret_cast<float*>(smem_raw);
    float* C = A + 64 * S::sF;
    float* D = C + 16 * S::sF;
    float* Z = D + 4 * S::sF;
    float* T = Z + S::sF;
    for (int i = threadIdx.x; i < S::sF; i += blockDim.x) Z[i] = 0.f;
    const int b = blockIdx.x;
    HgX3Ring ring;
    {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int j = 0; j < DR_HGX3_RING; ++j)                        // the first weights travel while the input is pooled
            HgX3Seq<F, NW, 0, true>::load(p.conv[0], j, threadIdx.x >> 6, lane & 15, lane >> 4, ring.b[j]);
    }
    hg16_pool_in(p.x + (long)b * 256 * p.x_cs + p.x_coff, p.x_cs, A, S::sF, F);
    __syncthreads();
    // the eight residual modules of hg_fused.h; what happens in front of module r: 1 C = pool(A), 3 D = pool(C), 6 C += up(D), 7 A += up(C)
#pragma clang loop unroll(disable)
    for (int r = 0; r < 8; ++r) {
        if (r == 1) { hg_pool(A, S::sF, 8, C, S::sF, F); __syncthreads(); }
        else if (r == 3) { hg_pool(C, S::sF, 4, D, S::sF, F); __syncthreads(); }
        else if (r == 6) { hg_upadd(C, 4, D, S::sF, F); __syncthreads(); }
        else if (r == 7) { hg_upadd(A, 8, C, S::sF, F); __syncthreads(); }
        const HgConvDescX3* d = p.conv + 3 * r;
        const HgConvDescX3* nd = r < 7 ? d + 3 : nullptr;
        const bool nrt4 = r == 0 || r == 6;                         // module r + 1 runs at 8x8
        if (r <= 1 || r == 7) {
            hgx3_residual<F, NW, true>(A, 8, 3, 64, d, T, Z, r == 7 ? p.y + (long)b * 64 * p.y_cs + p.y_coff : nullptr, p.y_cs, ring, nd, nrt4);
        } else {
            const bool four = r == 2 || r == 3 || r == 6;            // 4x4 on C, else 2x2 on D
            hgx3_residual<F, NW, false>(four ? C : D, four ? 4 : 2, four ? 2 : 1, four ? 16 : 4, d, T, Z, nullptr, 0, ring, nd, nrt4);
        }
    }
}

}  // namespace dr
