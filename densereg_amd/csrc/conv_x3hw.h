// conv_x3hw.h -- the LDS-resident 3x3 halo kernel of conv_x3h.h for 64- and 128-pixel-wide images (the full-resolution maps of 256x256 and
// 512x512 crops), on 256-row blocks.
//
// Same operator, arithmetic and bits as conv_x3_kernel and conv_x3h_kernel: the three-plane bf16 split while staging (x3_split4), the
// pre-split weight planes by LDS-DMA (x3_dma.h), the six plane products in conv_x3_kernel's order into the leading and the correction
// accumulator, K order chunk outer / tap inner, the fused epilogue of conv_epilogue.inc, and one fp64 statistics row per 128 output rows.
// What conv_x3h.h cannot do at these widths (its 128-row block is two image rows at W = 64 and one at W = 128):
//   * LDS.  A 128-row block needs (2 + 2) x 66 = 264 halo pixels at W = 64 and 3 x 130 = 390 at W = 128; double-buffered at 112 bytes per
//     pixel, with the two weight stages of the 128-column tile (24 576 B), that is 83 712 B and 111 936 B: one eight-wave workgroup per CU,
//     two waves per SIMD, and half (two thirds) of what is staged is halo.
//   * Staging.  Its one staging register carries at most four float4 units per thread and chunk (fetched in taps 0 / 2 / 4 / 6).
//
// Tile plan: BM = 256 output rows per workgroup = R = 256 / W whole image rows, haloed tile (R + 2) x (W + 2) pixels.
//   W =  64: four image rows, halo 6 x  66 = 396 pixels, LDS 2 x 44 352 + 2 x 3 x BN x 32 = 113 280 B at BN = 128
//   W = 128: two image rows,  halo 4 x 130 = 520 pixels, LDS 2 x 58 240 + 2 x 3 x BN x 32 = 141 056 B at BN = 128
//   (BN = 96: 107 136 / 134 912 B, BN = 64: 100 992 / 128 768 B) -- all within the CU's 160 KB, one workgroup per CU.
//   128 columns: SIXTEEN waves of 64x32 (4 x 4), i.e. conv_x3h_kernel's wave and its two accumulator pairs: four waves per SIMD at <= 128
//   registers, the weight tile of a tap fetched once per 256 pixels, 6 / 4 instead of 4 / 2 staged rows per output row at W = 64.
//   64 columns: eight waves of 64x32 (4 x 2); 96 columns: eight waves of 32x96 that split the rows only (8 x 1): two waves per SIMD.
//   The wave tiles are those of conv_x3_kernel's 128-row blocks, and a workgroup writes TWO statistics rows, each the sum of the waves of
//   one 128-row half in conv_x3_kernel's order: the BatchReNorm partial rows, their count and their bits are conv_x3_kernel's.
// Halo staging: a fetch slot on EVERY tap -- unit i of the next chunk is fetched behind the MFMAs of tap i and split + stored behind those
//   of tap i + 1, through one staging register (up to eight units per thread and chunk; the plan needs 2 .. 5).  The loads return in order
//   with the weight copies, so a unit fetched in tap i has landed with the weight tile of tap i + 1 in any case: a second staging register
//   would hold a value that is already there.
// A halo pixel keeps conv_x3h.h's 112 bytes (16 consecutive pixels = every bank once for a ds_read_b128 group, whatever the tap's shift:
//   a 32-lane fragment group reads 32 consecutive pixels of ONE image row because W is a multiple of 32), and the tap shift stays the
//   immediate of the ds_read (at most (2 (W + 2) + 2) x 112 + 80 = 29 424 B at W = 128).
// Measured on MI355X against conv_x3_kernel, alternating in one process (profiles/x3h_wide.md): 1.09-1.28x per launch at 40 / 200 crops of
//   64x64 maps and 10 / 40 crops of 128x128 maps on all three tiles (64x64 128->128 at 40 crops 300 -> 269 us, 180 TFLOP/s), 1.04x at worst
//   on the smallest grids conv_use_x3 admits (1.25 rounds of one workgroup per CU), repeats within 1-4 %: every width and tile is wired
//   wherever the x3 family is selected.  No spill, 116 / 120 registers for the sixteen-wave forms.  The plan was the first one built and it
//   won everywhere, so the alternatives (128-row blocks at one workgroup per CU, a single-buffered halo, two staging registers) are
//   not measured.
#pragma once
#include "conv_p3.h"

namespace dr {

// BN columns x BM rows per workgroup on W-pixel-wide images; NW waves as WM_ x (NW / WM_).
template <int BN, int W, int BM = 256, int NW = 16, int WM_ = 4>
__global__ __launch_bounds__(NW * 64, (NW == 16 ? 4 : 2)) void conv_x3hw_kernel(const ConvParams p) {
    constexpr int NT = NW * 64, WM = WM_, WN = NW / WM_, MF = 32, ABL = 0, CK = 16;
    constexpr int kWTM = BM / WM, kWTN = BN / WN, kTM = kWTM / 32, kTN = kWTN / 32;
    static_assert(kWTM % 32 == 0 && kWTN % 32 == 0, "wave tile of whole 32x32 MFMA tiles");
    static_assert((W & (W - 1)) == 0 && W % 32 == 0 && BM % W == 0, "a 32-lane fragment group reads 32 consecutive pixels of one image row");
    constexpr int Wp = W + 2, R = BM / W, NH = (R + 2) * Wp;   // tile = R whole image rows; NH halo pixels
    constexpr int PIX = 112;                                   // bytes per halo pixel: [3 planes][16 bf16] + 16 B pad
    constexpr int AH = NH * PIX;                               // bytes per halo buffer
    constexpr int AI = (NH * 4 + NT - 1) / NT;                 // float4 staging units per thread and chunk
    constexpr int BP = BN * 32, BS = 3 * BP;                   // bytes per weight plane / per weight stage
    constexpr int kBUnits = 3 * BN * 2;
    constexpr int kBInstr = kBUnits / 64;                      // 1 KB LDS-DMA copies per weight stage: three per wave, waves 0 ..
    static_assert(AH % 16 == 0 && AI <= 8 && kBUnits % 64 == 0 && kBInstr <= 3 * NW, "halo buffer / one staging unit per tap / weight copies");
    static_assert((2 * Wp + 2) * PIX + 2 * 32 + 16 < 65536, "the tap shift is a ds_read immediate");
    static_assert(2 * AH + 2 * BS <= 160 * 1024, "LDS of one CU");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * AH + 2 * BS];

    DR_PIN_ARGS(p.x, p.x_cs, p.x_coff, p.Cin, p.B, p.H, p.w3, p.Kp, p.Np, p.zeros, p.nfast, p.gx, p.gy, p.Ng);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: LDS-DMA bases live in M0)
    const int wm = wave / WN, wn = wave % WN;
    const int H = p.H, HW = H * W;
    const int M = p.B * HW;
    const int gx = p.gx, gy = p.gy;
    int mblk = blockIdx.x, nblk = blockIdx.y;                  // the XCD-aware mapping of conv_igemm.h
    if (p.nfast && gy > 1) {
        const int L = blockIdx.y * gx + blockIdx.x, nN = gy;
        if ((gx & 7) == 0) { const int s = L >> 3; mblk = (L & 7) * (gx >> 3) + s / nN; nblk = s % nN; }
        else { mblk = L / nN; nblk = L % nN; }
    } else if ((gx & 7) == 0) {
        mblk = (blockIdx.x & 7) * (gx >> 3) + (blockIdx.x >> 3);
    }
    const int m0 = mblk * BM, n0 = nblk * BN;
    const int KT = (p.Kp + CK - 1) / CK;
    const int img = m0 / HW, y0 = (m0 - img * HW) / W;         // image and first row of the tile (launcher: H * W is a multiple of BM)

    // ---- halo staging: unit (h, q) = channels 4q .. 4q+3 of halo pixel h; same units for every chunk -----------------------------
    // (kDead in a_off: the pixel lies outside the image -- zeros are stored; in a_lds: the unit lies outside the halo -- nothing is stored)
    constexpr unsigned kDead = 0xFFFFFFFFu;
    unsigned a_off[AI], a_lds[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int u = tid + i * NT, h = u >> 2, q = u & 3;
        const bool live = h < NH;
        const int hh = live ? h : 0;
        const int hy = hh / Wp, hx = hh - hy * Wp;
        const int y = y0 + hy - 1, x = hx - 1;
        const bool ok = live && y >= 0 && y < H && x >= 0 && x < W;
        a_off[i] = ok ? (unsigned)(((long)(img * H + y) * W + x) * p.x_cs + p.x_coff + q * 4) : kDead;
        a_lds[i] = live ? (unsigned)(hh * PIX + q * 8) : kDead;
    }
    const int a_q4 = (tid & 3) * 4;                            // first channel of this thread's units within a chunk (NT % 4 == 0)
    static_assert(NT % 4 == 0, "a thread's units share their channel group");
    // weight planes by LDS-DMA exactly as conv_x3h.h: a stage is [plane][BN rows][2 slots of 16 B] = kBInstr copies of 1 KB, wave w
    // issues copies 3 w .. 3 w + 2 (those that exist); rows beyond Np offer an out-of-range offset: zeros
    const int b_n = kBInstr - wave * 3 < 0 ? 0 : (kBInstr - wave * 3 > 3 ? 3 : kBInstr - wave * 3);     // copies of this wave (uniform)
    const P3Src srcB = p3_src(p.w3, 0, (size_t)9 * KT * p.Np * 96);
    unsigned b_voff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int u = (wave * 3 + j) * 64 + lane;
        const int pl = u / (BN * 2), within = u % (BN * 2), row = within >> 1, ls = (within & 1) ^ ((row >> 3) & 1);
        b_voff[j] = (u < kBUnits && n0 + row < p.Np) ? (unsigned)(((n0 + row) * 3 + pl) * 32 + ls * 16) : kP3Oob;
    }
    const unsigned b_dst = (unsigned)(2 * AH + (b_n > 0 ? wave : 0) * 3 * 1024);
    unsigned b_soff = 0;
    const unsigned w_tile = (unsigned)p.Np * 96u;

    float4 a_reg;                                               // the staging register: unit i is fetched in tap i and stored in tap i + 1
    const bool ragged = (p.Cin & 3) != 0;
    auto load_a = [&](const int i, const int kc) __attribute__((always_inline)) {
        const bool ok = a_off[i] != kDead && kc + a_q4 < p.Cin;
        a_reg = *reinterpret_cast<const float4*>(ok ? p.x + kc + a_off[i] : p.zeros);
    };
    auto store_a = [&](const int i, unsigned char* dst, const int kc) __attribute__((always_inline)) {
        if (a_lds[i] == kDead) return;
        float4 v = a_reg;
        if (ragged && kc + CK > p.Cin) {
            const int left = p.Cin - (kc + a_q4);                           // (<= 0: the unit was loaded from the zero page)
            v.y = left > 1 ? v.y : 0.f;
            v.z = left > 2 ? v.z : 0.f;
            v.w = left > 3 ? v.w : 0.f;
        }
        uint2 h0, h1, h2;
        x3_split4(v, h0, h1, h2);
        *reinterpret_cast<uint2*>(dst + a_lds[i]) = h0;
        *reinterpret_cast<uint2*>(dst + a_lds[i] + 32) = h1;
        *reinterpret_cast<uint2*>(dst + a_lds[i] + 64) = h2;
    };
    auto dma_b = [&](const unsigned stage) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < b_n) p3_dma16(srcB, b_voff[j], b_soff, lds, b_dst + stage * BS + j * 1024);
        b_soff += w_tile;
    };

    using AccT = dr_f32x16;
    constexpr int NR = 16;
    AccT acc[kTM][kTN], lo[kTM][kTN];
#pragma unroll
    for (int i = 0; i < kTM; ++i)
#pragma unroll
        for (int j = 0; j < kTN; ++j)
#pragma unroll
            for (int r = 0; r < NR; ++r) { acc[i][j][r] = 0.f; lo[i][j][r] = 0.f; }

    const int lk = lane >> 5, li = lane & 31;
    // this lane's A rows in the halo: row r = wm * kWTM + i * 32 + li of the tile is image row r / W, column r % W, halo pixel
    // (r / W + 1) * Wp + r % W + 1 at the centre tap; the base is biased by the most negative tap shift (Wp + 1 pixels) so that every
    // tap's shift is a non-negative immediate
    unsigned a_frag[kTM];
#pragma unroll
    for (int i = 0; i < kTM; ++i) {
        const int r = wm * kWTM + i * 32 + li;
        a_frag[i] = (unsigned)(((r / W + 1) * Wp + (r & (W - 1)) + 1 - (Wp + 1)) * PIX + lk * 16);
    }
    const unsigned b_frag = (unsigned)((wn * kWTN + li) * 32 + (lk ^ ((li >> 3) & 1)) * 16);

    unsigned char* const a_buf0 = lds;
    const unsigned char* const b_buf0 = lds + 2 * AH;
#pragma unroll
    for (int i = 0; i < AI; ++i) { load_a(i, 0); store_a(i, a_buf0, 0); }
    dma_b(0u);
    P3_WAIT_VM(0);
    __builtin_amdgcn_s_barrier();
#define X3HW_MMA(c, a, b)                                                                                                        \
    _Pragma("unroll") for (int i = 0; i < kTM; ++i) _Pragma("unroll") for (int j = 0; j < kTN; ++j)                              \
        c[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(dr_bf16x8, a[i]), __builtin_bit_cast(dr_bf16x8, b[j]), c[i][j], 0, 0, 0)
    unsigned bpar = 0;                                                      // weight stage of the tile being multiplied
    for (int c = 0; c < KT; ++c) {
        const unsigned char* const ah = lds + (c & 1) * AH;
        unsigned char* const ah_next = lds + ((c & 1) ^ 1) * AH;
        const bool more_c = c + 1 < KT;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bool more = more_c || tap < 8;
            if (more) dma_b(bpar ^ 1u);                                   // (that stage was last read in the previous tap: behind its barrier)
            {   // one K-tile: the products in conv_x3_kernel's order (the same bits)
                constexpr int kCentre = Wp + 1;
                const int shift = ((tap / 3 - 1) * Wp + (tap % 3 - 1) + kCentre) * PIX;      // (a constant of the unrolled tap)
                const unsigned char* ap[kTM];
#pragma unroll
                for (int i = 0; i < kTM; ++i) ap[i] = ah + a_frag[i] + shift;
                const unsigned char* const bp = b_buf0 + bpar * BS + b_frag;
                float4 a0[kTM], b0[kTN], ax[kTM], bx[kTN];
#define X3HW_READ_A(d, pl) _Pragma("unroll") for (int i = 0; i < kTM; ++i) d[i] = *reinterpret_cast<const float4*>(ap[i] + (pl) * 32)
#define X3HW_READ_B(d, pl) _Pragma("unroll") for (int j = 0; j < kTN; ++j) d[j] = *reinterpret_cast<const float4*>(bp + (pl) * BP + j * 32 * 32)
                X3HW_READ_A(a0, 0); X3HW_READ_B(b0, 0); X3HW_READ_A(ax, 2); X3HW_READ_B(bx, 2);
                X3HW_MMA(lo, ax, b0);                                       // a2*b0
                X3HW_MMA(lo, a0, bx);                                       // a0*b2
                X3HW_READ_A(ax, 1); X3HW_READ_B(bx, 1);
                X3HW_MMA(acc, a0, b0);
                X3HW_MMA(lo, ax, b0);                                       // a1*b0
                X3HW_MMA(lo, a0, bx);                                       // a0*b1
                X3HW_MMA(lo, ax, bx);                                       // a1*b1
#undef X3HW_READ_A
#undef X3HW_READ_B
            }
            // the halo of chunk c + 1, a unit per tap through a_reg: the unit requested in the previous tap is stored, then the next one requested
            if (tap >= 1 && tap - 1 < AI && more_c) store_a(tap - 1, ah_next, (c + 1) * CK);
            const bool fetch_a = tap < AI && more_c;
            if (fetch_a) load_a(tap, (c + 1) * CK);
            bpar ^= 1;
            // the weight copy issued at the top of this tap has landed (this wave's share; the halo fetch just issued may stay in flight),
            // every LDS read and write of this wave has completed -- then everybody's
            __builtin_amdgcn_sched_barrier(0);                              // (the tap's MFMAs are issued BEFORE the wait: the copy lands under them)
            if (fetch_a) P3_WAIT_VM(1); else P3_WAIT_VM(0);
            __builtin_amdgcn_s_barrier();
        }
    }
#undef X3HW_MMA
#pragma unroll
    for (int i = 0; i < kTM; ++i)
#pragma unroll
        for (int j = 0; j < kTN; ++j) acc[i][j] += lo[i][j];

    // ---- epilogue: conv_epilogue.inc (the fp32 copy), as conv_x3_kernel ------------------------------------------------------------
    double s1[kTN], s2[kTN];
#pragma unroll
    for (int j = 0; j < kTN; ++j) s1[j] = s2[j] = 0.0;
    constexpr int EP_TM = kTM, EP_TN = kTN;
    const int ep_m0 = m0 + wm * kWTM, ep_n0 = n0 + wn * kWTN;
    const unsigned ep_rows = 0xFFFFu;
    constexpr int EP_BATCH_ROWS = NW == 16 ? 4 : 8;
    constexpr int EP_TS = MF, EP_NR = NR;
    const int ep_lg = lk, ep_lc = li;
    {
        constexpr bool EP_Y16 = false, EP_B16 = false, EP_B16_CONST = false;
#include "conv_epilogue.inc"
    }
    if (p.stat_part) {
        double* red = reinterpret_cast<double*>(lds);                      // the operand tiles are dead: the K loop ended on a barrier
        static_assert(sizeof(lds) >= sizeof(double) * 2 * WM * BN, "stat scratch");
#pragma unroll
        for (int j = 0; j < kTN; ++j) {
            double a = s1[j], b = s2[j];
            a += __shfl_xor(a, 32);
            b += __shfl_xor(b, 32);
            if (ep_lg == 0) {
                const int col = wn * kWTN + j * MF + ep_lc;
                red[(0 * WM + wm) * BN + col] = a;
                red[(1 * WM + wm) * BN + col] = b;
            }
        }
        __syncthreads();
        // one partial row per 128 pixel rows: BM / 128 rows per workgroup, each the sum of the waves of its 128-row half in wave order --
        // the rows, and the bits, of conv_x3_kernel's 128-row blocks
        constexpr int kHalves = BM / 128, kWH = WM / kHalves;
        static_assert(BM % 128 == 0 && WM % kHalves == 0, "statistics rows are 128 pixel rows");
        const int srows = M >> 7;
        for (int e = tid; e < 2 * BN * kHalves; e += NT) {
            const int half = e / (2 * BN), which = (e / BN) % 2, col = e % BN, n = n0 + col;
            double tsum = 0.0;
#pragma unroll
            for (int w = 0; w < kWH; ++w) tsum += red[(which * WM + half * kWH + w) * BN + col];
            if (n < p.Cout) p.stat_part[((long)which * p.Cout + n) * srows + mblk * kHalves + half] = tsum;
        }
    }
    (void)NW; (void)M;
}

}  // namespace dr
