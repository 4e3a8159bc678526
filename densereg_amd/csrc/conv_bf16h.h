// conv_bf16h.h -- the bf16 member of the LDS-resident 3x3 halo family (conv_x3h.h, conv_x3hw.h): conv_igemm_kernel's BF arithmetic with the
// haloed input tile kept in LDS across the nine taps.
//
// Same operator, arithmetic and bits as conv_igemm_kernel<..., BF = 1, ...> on its 64-row tiles (v_mfma_f32_32x32x16_bf16, fp32 accumulate, both
// operands rounded to bf16, tf.nn.conv2d of network/slim/ops.py:282 with the fused epilogue of conv_epilogue.inc).  That kernel treats a 3x3
// convolution as nine 1x1 ones: every K-tile (32 channels of one tap) fetches its 64 pixels again, converts them to bf16 again and writes them to
// LDS again.  Here a workgroup's 128 output pixels are whole image rows (W = 16 / 32 divides 128), so the pixels its nine taps read are ONE haloed
// tile of (128 / W + 2) x (W + 2) pixels: per 32-channel chunk it is fetched, converted (round to nearest even) and stored once, and the nine taps
// read their A fragments from it at a shifted pixel -- the shift is the immediate of the ds_read, TF's 'SAME' zero padding and the pixels of the
// neighbouring image are zeros stored in the halo.
//
//   LDS: 2 x halo [pixel][32 bf16 = 64 B + 16 B pad] (chunk c + 1 is staged while the taps of chunk c multiply) + 2 x weights [BN][64 B]
//   = 2 x 16 320 + 2 x 8 192 = 49 024 B at W = 32, BN = 128.  A halo pixel is 80 bytes = 20 dwords: the 16 lanes of a ds_read_b128 group read 16
//   CONSECUTIVE halo pixels whatever the tap's shift, and 16 consecutive multiples of 20 dwords are 16 different multiples of 4 modulo 64 --
//   every bank once, no slot swizzle.
//   Weights: a tap's tile (BN rows x 64 B) is contiguous in the bf16 pack [Kp/32][tap][Np][32] (pack_all_kernel) and goes L2 -> LDS by the
//   LDS-DMA of x3_dma.h, two stages, counted waits, no staging registers.  The LDS image of a DMA is lane-linear, so conv_igemm's slot swizzle
//   (16-byte slot s of row r at s ^ ((r >> 2) & 3)) sits on the source side.
//   Halo staging: unit (h, q) = channels 4q .. 4q+3 of halo pixel h, one unit per tap through one staging register -- unit i of the next chunk
//   is fetched behind the MFMAs of tap i and converted + stored behind those of tap i + 1 (conv_x3hw.h).  XB bit 0: the source is stored as bf16
//   (ConvParams::x_bf16, channel groups of four zero-padded by the producer): the unit's 8 bytes are copied as they are.
//
// Bits.  Per output element the products are added in conv_igemm's order: chunks outermost, taps inner, within a K-tile the 16-k groups g = 0, 1
// into accumulator g % KACC, lane half lk supplying k 8 lk .. 8 lk + 7 of a group; KACC is that of the tile replaced (the 64x128 tile has one
// accumulator chain per output tile, the 64x64 tile two, and the 64x96 tile's K halves are two chains as well) and the fold is acc[0] + acc[1].
// The BatchReNorm partial statistics keep conv_igemm's rows: one fp64 row per 64 output rows, each the sum of its two 32-row wave tiles in wave
// order -- the epilogue runs once per 32-row tile with its own partials, and a workgroup writes two rows.
#pragma once
#include "conv_igemm.h"
#include "x3_dma.h"

namespace dr {

// LW = log2(image width): 5 or 4.  BN = 128: eight waves of 64x32 (NW = 8, WM_ = 2), replaces the 64x128 tile; BN = 64: four waves of 64x32
// (NW = 4, WM_ = 2), replaces the 64x64 tile; BN = 96: four waves of 32x96 that split the rows only (NW = 4, WM_ = 4), replaces the 64x96 tile.
// XB as conv_igemm_kernel's: bit 0 the bf16-stored source, bit 1 the two extra epilogue copies for bf16-stored raw outputs and gradients.
template <int BN, int LW, int NW = 8, int WM_ = 2, int XB = 0>
__global__ __launch_bounds__(NW * 64, (NW == 8 ? 4 : 2)) void conv_bf16h_kernel(const ConvParams p) {
    constexpr int BM = 128, NT = NW * 64, WM = WM_, WN = NW / WM_, MF = 32, ABL = 0, CK = 32;
    constexpr int kWTM = BM / WM, kWTN = BN / WN, kTM = kWTM / 32, kTN = kWTN / 32;
    constexpr int KACC = BN == 128 ? 1 : 2;
    static_assert(kWTM % 32 == 0 && kWTN % 32 == 0, "wave tile of whole 32x32 MFMA tiles");
    constexpr int W = 1 << LW, Wp = W + 2, R = BM / W, NH = (R + 2) * Wp;      // tile = R whole image rows; NH halo pixels
    static_assert(W <= 32 && BM % W == 0, "a 32-lane fragment group reads whole runs of 16 consecutive pixels");
    constexpr int PIX = 80;                                    // bytes per halo pixel: 32 bf16 + 16 B pad
    constexpr int AH = NH * PIX;                               // bytes per halo buffer
    constexpr int AI = (NH * 8 + NT - 1) / NT;                 // 4-channel staging units per thread and chunk
    constexpr int BS = BN * 64;                                // bytes per weight stage
    constexpr int kBUnits = BN * 4;                            // 16-byte units per weight stage
    constexpr int kBInstr = kBUnits / 64;                      // 1 KB LDS-DMA copies per weight stage
    constexpr int CPW = (kBInstr + NW - 1) / NW;               // ... per wave (waves 0 ..)
    static_assert(AH % 16 == 0 && AI <= 8 && kBUnits % 64 == 0, "halo buffer / one staging unit per tap / weight copies");
    static_assert(NT % 8 == 0, "a thread's units share their channel group");
    constexpr bool xb16 = (XB & 1) != 0;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * AH + 2 * BS];

    DR_PIN_ARGS(p.x, p.x_cs, p.x_coff, p.Cin, p.B, p.H, p.w, p.Kp, p.Np, p.zeros, p.nfast, p.gx, p.gy, p.Ng);
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
    const int KT = p.Kp / CK;                                  // (launcher: Kp is a multiple of 32)
    const int img = m0 / HW, y0 = (m0 - img * HW) >> LW;       // image and first row of the tile (launcher: H * W is a multiple of 128)

    // ---- halo staging: unit (h, q) = channels 4q .. 4q+3 of halo pixel h; same units for every chunk -----------------------------
    // (kDead in a_off: the pixel lies outside the image -- zeros are stored; in a_lds: the unit lies outside the halo -- nothing is stored)
    constexpr unsigned kDead = 0xFFFFFFFFu;
    unsigned a_off[AI], a_lds[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int u = tid + i * NT, h = u >> 3, q = u & 7;
        const bool live = h < NH;
        const int hh = live ? h : 0;
        const int hy = hh / Wp, hx = hh - hy * Wp;
        const int y = y0 + hy - 1, x = hx - 1;
        const bool ok = live && y >= 0 && y < H && x >= 0 && x < W;
        a_off[i] = ok ? (unsigned)(((long)(img * H + y) * W + x) * p.x_cs + p.x_coff + q * 4) : kDead;
        a_lds[i] = live ? (unsigned)(hh * PIX + q * 8) : kDead;
    }
    const int a_q4 = (tid & 7) * 4;                            // first channel of this thread's units within a chunk
    // weights by LDS-DMA: a stage is [BN rows][4 slots of 16 B] = kBInstr copies of 1 KB, wave w issues copies CPW w .. (those that exist).
    // Lane L of copy q owns unit u = 64 q + L = (row, physical slot) and fetches the logical slot physical ^ ((row >> 2) & 3); rows beyond Np
    // offer an out-of-range offset: zeros.
    const int b_left = kBInstr - wave * CPW;
    const int b_n = b_left < 0 ? 0 : (b_left > CPW ? CPW : b_left);             // copies of this wave (uniform)
    const P3Src srcB = p3_src(p.w, 0, (size_t)9 * KT * p.Np * 64);
    unsigned b_voff[CPW];
#pragma unroll
    for (int j = 0; j < CPW; ++j) {
        const int u = (wave * CPW + j) * 64 + lane;
        const int row = u >> 2, ls = (u & 3) ^ ((row >> 2) & 3);
        b_voff[j] = (u < kBUnits && n0 + row < p.Np) ? (unsigned)((n0 + row) * 64 + ls * 16) : kP3Oob;
    }
    const unsigned b_dst = (unsigned)(2 * AH + (b_n > 0 ? wave : 0) * CPW * 1024);
    unsigned b_soff = 0;
    const unsigned w_tile = (unsigned)p.Np * 64u;

    float4 a_reg;                                               // the staging register: unit i is fetched in tap i and stored in tap i + 1
    uint2 a_reg16;                                              // ... of a bf16-stored source
    const bool ragged = (p.Cin & 3) != 0;
    auto load_a = [&](const int i, const int kc) __attribute__((always_inline)) {
        const bool ok = a_off[i] != kDead && kc + a_q4 < p.Cin;
        if constexpr (xb16) {
            const __bf16* sb = reinterpret_cast<const __bf16*>(p.x) + kc + a_off[i];
            a_reg16 = *reinterpret_cast<const uint2*>(ok ? reinterpret_cast<const void*>(sb) : reinterpret_cast<const void*>(p.zeros));
        } else {
            a_reg = *reinterpret_cast<const float4*>(ok ? p.x + kc + a_off[i] : p.zeros);
        }
    };
    auto store_a = [&](const int i, unsigned char* dst, const int kc) __attribute__((always_inline)) {
        if (a_lds[i] == kDead) return;
        if constexpr (xb16) {                                   // (channel groups of four are zero-padded by the producer)
            *reinterpret_cast<uint2*>(dst + a_lds[i]) = a_reg16;
        } else {
            float4 v = a_reg;
            if (ragged && kc + CK > p.Cin) {
                const int left = p.Cin - (kc + a_q4);                       // (<= 0: the unit was loaded from the zero page)
                v.y = left > 1 ? v.y : 0.f;
                v.z = left > 2 ? v.z : 0.f;
                v.w = left > 3 ? v.w : 0.f;
            }
            const dr_f32x4 f = {v.x, v.y, v.z, v.w};
            *reinterpret_cast<uint2*>(dst + a_lds[i]) = __builtin_bit_cast(uint2, __builtin_convertvector(f, dr_bf16x4));
        }
    };
    auto dma_b = [&](const unsigned stage) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < CPW; ++j)
            if (j < b_n) p3_dma16(srcB, b_voff[j], b_soff, lds, b_dst + stage * BS + j * 1024);
        b_soff += w_tile;
    };

    using AccT = dr_f32x16;
    constexpr int NR = 16;
    AccT accp[KACC][kTM][1][kTN];                               // ([1]: the epilogue runs per 32-row tile on accp[.][ih])
#pragma unroll
    for (int q = 0; q < KACC; ++q)
#pragma unroll
        for (int i = 0; i < kTM; ++i)
#pragma unroll
            for (int j = 0; j < kTN; ++j)
#pragma unroll
                for (int r = 0; r < NR; ++r) accp[q][i][0][j][r] = 0.f;

    const int lk = lane >> 5, li = lane & 31;
    // this lane's A rows in the halo: row r = wm * kWTM + i * 32 + li of the tile is image row r / W, column r % W, halo pixel
    // (r / W + 1) * Wp + r % W + 1 at the centre tap; the base is biased by the most negative tap shift (Wp + 1 pixels) so that every
    // tap's shift is a non-negative immediate.  Group g of a K-tile is channels 16 g .. 16 g + 15: bytes 32 g + 16 lk of the pixel.
    unsigned a_frag[kTM];
#pragma unroll
    for (int i = 0; i < kTM; ++i) {
        const int r = wm * kWTM + i * 32 + li;
        a_frag[i] = (unsigned)((((r >> LW) + 1) * Wp + (r & (W - 1)) + 1 - (Wp + 1)) * PIX + lk * 16);
    }
    unsigned b_frag[2];                                         // per group: logical slot 2 g + lk of row wn * kWTN + li (+ 32 j)
#pragma unroll
    for (int g = 0; g < 2; ++g) b_frag[g] = (unsigned)((wn * kWTN + li) * 64 + ((2 * g + lk) ^ ((li >> 2) & 3)) * 16);

    unsigned char* const a_buf0 = lds;
    const unsigned char* const b_buf0 = lds + 2 * AH;
#pragma unroll
    for (int i = 0; i < AI; ++i) { load_a(i, 0); store_a(i, a_buf0, 0); }
    dma_b(0u);
    P3_WAIT_VM(0);
    __builtin_amdgcn_s_barrier();
    unsigned bpar = 0;                                                      // weight stage of the tile being multiplied
    for (int c = 0; c < KT; ++c) {
        const unsigned char* const ah = lds + (c & 1) * AH;
        unsigned char* const ah_next = lds + ((c & 1) ^ 1) * AH;
        const bool more_c = c + 1 < KT;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bool more = more_c || tap < 8;
            if (more) dma_b(bpar ^ 1u);                                   // (that stage was last read in the previous tap: behind its barrier)
            {   // one K-tile: the products in conv_igemm_kernel's order (the same bits)
                constexpr int kCentre = Wp + 1;
                const int shift = ((tap / 3 - 1) * Wp + (tap % 3 - 1) + kCentre) * PIX;      // (a constant of the unrolled tap)
                const unsigned char* const bp = b_buf0 + bpar * BS;
                float4 a4[2][kTM], b4[2][kTN];
#pragma unroll
                for (int g = 0; g < 2; ++g) {
#pragma unroll
                    for (int i = 0; i < kTM; ++i) a4[g][i] = *reinterpret_cast<const float4*>(ah + a_frag[i] + shift + g * 32);
#pragma unroll
                    for (int j = 0; j < kTN; ++j) b4[g][j] = *reinterpret_cast<const float4*>(bp + b_frag[g] + j * 32 * 64);
                }
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int i = 0; i < kTM; ++i)
#pragma unroll
                        for (int j = 0; j < kTN; ++j)
                            accp[g % KACC][i][0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                __builtin_bit_cast(dr_bf16x8, a4[g][i]), __builtin_bit_cast(dr_bf16x8, b4[g][j]), accp[g % KACC][i][0][j], 0, 0, 0);
            }
            // the halo of chunk c + 1, a unit per tap through the staging register: the unit requested in the previous tap is stored, then the next one requested
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
    if constexpr (KACC > 1) {
#pragma unroll
        for (int i = 0; i < kTM; ++i)
#pragma unroll
            for (int j = 0; j < kTN; ++j) accp[0][i][0][j] += accp[1][i][0][j];
    }

    // ---- epilogue: conv_epilogue.inc, once per 32-row tile of the wave (its own statistics partials: conv_igemm's 32-row wave tiles) ------
    double s1h[kTM][kTN], s2h[kTM][kTN];
#pragma unroll
    for (int i = 0; i < kTM; ++i)
#pragma unroll
        for (int j = 0; j < kTN; ++j) s1h[i][j] = s2h[i][j] = 0.0;
    constexpr int EP_TM = 1, EP_TN = kTN;
    const int ep_n0 = n0 + wn * kWTN;
    const unsigned ep_rows = 0xFFFFu;
    constexpr int EP_BATCH_ROWS = NW == 8 ? 4 : 8;
    constexpr int EP_TS = MF, EP_NR = NR;
    const int ep_lg = lk, ep_lc = li;
    if ((XB & 2) != 0 && p.bst_raw_bf16) {                   // the XB = 2 / 3 kernels: one copy of the epilogue per storage case (conv_epilogue.inc)
        constexpr bool EP_Y16 = false, EP_B16 = true, EP_B16_CONST = true;
#pragma unroll
        for (int ih = 0; ih < kTM; ++ih) {
            auto& acc = accp[0][ih]; auto& s1 = s1h[ih]; auto& s2 = s2h[ih];
            const int ep_m0 = m0 + wm * kWTM + ih * 32;
#include "conv_epilogue.inc"
        }
    } else if ((XB & 2) != 0 && p.y_bf16) {
        constexpr bool EP_Y16 = true, EP_B16 = false, EP_B16_CONST = false;
#pragma unroll
        for (int ih = 0; ih < kTM; ++ih) {
            auto& acc = accp[0][ih]; auto& s1 = s1h[ih]; auto& s2 = s2h[ih];
            const int ep_m0 = m0 + wm * kWTM + ih * 32;
#include "conv_epilogue.inc"
        }
    } else {
        constexpr bool EP_Y16 = false, EP_B16 = false, EP_B16_CONST = false;
#pragma unroll
        for (int ih = 0; ih < kTM; ++ih) {
            auto& acc = accp[0][ih]; auto& s1 = s1h[ih]; auto& s2 = s2h[ih];
            const int ep_m0 = m0 + wm * kWTM + ih * 32;
#include "conv_epilogue.inc"
        }
    }
    if (p.stat_part) {
        double* red = reinterpret_cast<double*>(lds);                      // the operand tiles are dead: the K loop ended on a barrier
        constexpr int kG = BM / 32;                                        // 32-row tiles of the workgroup: [2][kG][BN] doubles
        static_assert(sizeof(lds) >= sizeof(double) * 2 * kG * BN, "stat scratch");
#pragma unroll
        for (int ih = 0; ih < kTM; ++ih)
#pragma unroll
            for (int j = 0; j < kTN; ++j) {
                double a = s1h[ih][j], b = s2h[ih][j];
                a += __shfl_xor(a, 32);
                b += __shfl_xor(b, 32);
                if (ep_lg == 0) {
                    const int col = wn * kWTN + j * MF + ep_lc;
                    red[(0 * kG + wm * kTM + ih) * BN + col] = a;
                    red[(1 * kG + wm * kTM + ih) * BN + col] = b;
                }
            }
        __syncthreads();
        // one partial row per 64 pixel rows, each the sum of its two 32-row tiles in order: the rows, and the bits, of conv_igemm's 64-row tiles
        const int srows = M >> 6;
        for (int e = tid; e < 4 * BN; e += NT) {
            const int half = e / (2 * BN), which = (e / BN) % 2, col = e % BN, n = n0 + col;
            double tsum = 0.0;
#pragma unroll
            for (int w = 0; w < 2; ++w) tsum += red[(which * kG + half * 2 + w) * BN + col];
            if (n < p.Cout) p.stat_part[((long)which * p.Cout + n) * srows + mblk * 2 + half] = tsum;
        }
    }
    (void)NW; (void)M;
}

}  // namespace dr
