// conv_bf16hw.h -- the LDS-resident 3x3 halo kernel of the bf16 path (conv_bf16h.h) for 64- and 128-pixel-wide images (the full-resolution maps
// of 256x256 and 512x512 crops), on 256-row blocks: to conv_bf16h.h what conv_x3hw.h is to conv_x3h.h.
//
// Same operator, arithmetic and bits as conv_igemm_kernel<..., BF = 1, ...> on its 64-row tiles and as conv_bf16h_kernel: v_mfma_f32_32x32x16_bf16
// with fp32 accumulate, both operands rounded to bf16 (round to nearest even), K order chunk outer / tap inner, within a K-tile the 16-k groups
// g = 0, 1 into accumulator g % KACC (KACC of the tile replaced: 1 for 64x128, 2 for 64x64 and 64x96), the fold acc[0] + acc[1], the fused
// epilogue of conv_epilogue.inc once per 32-row tile with its own statistics partials, and one fp64 statistics row per 64 output rows, each the
// sum of its two 32-row tiles in wave order -- a workgroup writes FOUR rows, at mblk * 4 + q.
// What conv_bf16h.h cannot do at these widths: its 128-row block is two image rows at W = 64 and one at W = 128 (half / two thirds of what it
// would stage is halo), its fragment reads are reasoned for 16-pixel runs, and its one staging register of 4-channel units carries at most
// eight units per thread and chunk (a 520-pixel halo on 512 threads needs nine).
//
// Tile plan: BM = 256 output rows per workgroup = R = 256 / W whole image rows, haloed tile (R + 2) x (W + 2) pixels.
//   W =  64: four image rows, halo 6 x  66 = 396 pixels, LDS 2 x 31 680 + 2 x BN x 64 = 79 744 B at BN = 128 (two workgroups per CU fit)
//   W = 128: two image rows,  halo 4 x 130 = 520 pixels, LDS 2 x 41 600 + 2 x BN x 64 = 99 584 B at BN = 128 (one workgroup per CU)
//   128 columns: SIXTEEN waves of 64x32 (4 x 4), four waves per SIMD at <= 128 registers; 64 columns: eight waves of 64x32 (4 x 2); 96 columns:
//   eight waves of 32x96 that split the rows only (8 x 1).  The wave tiles are conv_bf16h_kernel's, twice as many along the rows; a tap's weight
//   tile is fetched once per 256 pixels.
//   A halo pixel keeps conv_bf16h.h's 80 bytes (32 bf16 + 16 B pad): W is a multiple of 32, so a 32-lane fragment group reads 32 consecutive
//   pixels of ONE image row, and 16 consecutive 20-dword pixels are every bank once whatever the tap's shift.  The shift stays the immediate of
//   the ds_read (at most (2 x 130 + 2) x 80 + 48 = 21 008 B at W = 128).
//   Weights: as conv_bf16h.h -- a tap's tile of the bf16 pack [Kp/32][tap][Np][32] by the LDS-DMA of x3_dma.h, two stages, counted waits, the
//   slot swizzle on the source side.
// Halo staging: EIGHT-channel units (of the two fixes for "nine 4-channel units do not fit one unit per tap", the one chosen: it halves the
//   units AND the LDS stores, where sixteen waves for the 64- and 96-column forms would halve only the units per thread).  Unit (h, q) =
//   channels 8q .. 8q+7 of halo pixel h: two 16-byte loads of an fp32 source (two 8-byte loads of a bf16-stored one: its channel stride is a
//   multiple of four elements, not of eight) become ONE 16-byte ds_write.  NH x 4 units per chunk = 2 (W = 64) / 3 (W = 128) per thread on
//   1024 threads, 4 / 5 on 512.  The order is conv_bf16h.h's: unit i of the next chunk is fetched behind the MFMAs of tap i and converted +
//   stored behind those of tap i + 1, and the wait for the weight copy leaves the two loads of the fetch in flight (P3_WAIT_VM(2)).  The
//   Cin % 4 tail is masked per 4-channel half; pixels outside the image, and whole halves beyond Cin, come from the zero page -- neighbouring
//   images contribute zeros, never pixels.
// Measured on MI355X against conv_igemm's BF kernel, alternating in one process (profiles/conv_bf16_halo_wide.md, the table the launcher's
//   default rule, bf16hw_wired in densereg.cpp, is read from), repeats within 1-4 %: W = 64 1.14-1.69x on 128 columns from 256 workgroups
//   (3x3 256->256 at 40 crops 394 -> 265 us, 730 TFLOP/s; 128->128 at 40 crops 98.7 -> 78.0 us), 1.14-1.44x on 64 columns, 1.25-1.41x on 96;
//   W = 128 1.07-1.45x on 128 columns and 1.21-1.36x on 96 from 640 workgroups.  Lost and not wired: W = 128 with 64 columns (0.91-0.99x at
//   every grid) and W = 128 on 128 / 320 workgroups (0.90-1.08x).  End to end with `--precision bf16`, DR_BF16_HALOW=0 against the default,
//   three repeats: forward+vote S4 F256 in_hw 256 2263 -> 2370 crops/s (+4.7 %), S2 F256 in_hw 512 1088 -> 1132 (+4.0 %); training in_hw 256
//   520.4 -> 523.4 (+0.6 %), in_hw 512 within the spread.  No spill, 87-91 registers for the sixteen-wave forms.  The plan was the first one
//   built; sixteen waves for the 64- and 96-column forms and a single-buffered halo are not measured.
#pragma once
#include "conv_igemm.h"
#include "x3_dma.h"

namespace dr {

// BN columns x 256 rows per workgroup on W-pixel-wide images; NW waves as WM_ x (NW / WM_).  BN = 128: sixteen waves of 64x32 (NW = 16,
// WM_ = 4), replaces the 64x128 tile; BN = 64: eight waves of 64x32 (NW = 8, WM_ = 4), replaces the 64x64 tile; BN = 96: eight waves of 32x96
// (NW = 8, WM_ = 8), replaces the 64x96 tile.  XB as conv_igemm_kernel's: bit 0 the bf16-stored source, bit 1 the two extra epilogue copies
// for bf16-stored raw outputs and gradients.
template <int BN, int W, int NW = 16, int WM_ = 4, int XB = 0>
__global__ __launch_bounds__(NW * 64, (NW == 16 ? 4 : 2)) void conv_bf16hw_kernel(const ConvParams p) {
    constexpr int BM = 256, NT = NW * 64, WM = WM_, WN = NW / WM_, MF = 32, ABL = 0, CK = 32;
    constexpr int kWTM = BM / WM, kWTN = BN / WN, kTM = kWTM / 32, kTN = kWTN / 32;
    constexpr int KACC = BN == 128 ? 1 : 2;
    static_assert(kWTM % 32 == 0 && kWTN % 32 == 0, "wave tile of whole 32x32 MFMA tiles");
    static_assert((W & (W - 1)) == 0 && W % 32 == 0 && BM % W == 0, "a 32-lane fragment group reads 32 consecutive pixels of one image row");
    constexpr int Wp = W + 2, R = BM / W, NH = (R + 2) * Wp;   // tile = R whole image rows; NH halo pixels
    constexpr int PIX = 80;                                    // bytes per halo pixel: 32 bf16 + 16 B pad
    constexpr int AH = NH * PIX;                               // bytes per halo buffer
    constexpr int AI = (NH * 4 + NT - 1) / NT;                 // 8-channel staging units per thread and chunk
    constexpr int BS = BN * 64;                                // bytes per weight stage
    constexpr int kBUnits = BN * 4;                            // 16-byte units per weight stage
    constexpr int kBInstr = kBUnits / 64;                      // 1 KB LDS-DMA copies per weight stage
    constexpr int CPW = (kBInstr + NW - 1) / NW;               // ... per wave (waves 0 ..)
    static_assert(AH % 16 == 0 && AI <= 8 && kBUnits % 64 == 0, "halo buffer / one staging unit per tap / weight copies");
    static_assert(NT % 4 == 0, "a thread's units share their channel group");
    static_assert((2 * Wp + 2) * PIX + 32 + 16 + 16 < 65536, "the tap shift is a ds_read immediate");
    static_assert(2 * AH + 2 * BS <= 160 * 1024, "LDS of one CU");
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
    const int img = m0 / HW, y0 = (m0 - img * HW) / W;         // image and first row of the tile (launcher: H * W is a multiple of 256)

    // ---- halo staging: unit (h, q) = channels 8q .. 8q+7 of halo pixel h; same units for every chunk -----------------------------
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
        a_off[i] = ok ? (unsigned)(((long)(img * H + y) * W + x) * p.x_cs + p.x_coff + q * 8) : kDead;
        a_lds[i] = live ? (unsigned)(hh * PIX + q * 16) : kDead;
    }
    const int a_q8 = (tid & 3) * 8;                            // first channel of this thread's units within a chunk
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

    float4 a_reg[2];                                            // the staging register: unit i is fetched in tap i and stored in tap i + 1
    uint2 a_reg16[2];                                           // ... of a bf16-stored source
    const bool ragged = (p.Cin & 3) != 0;
    auto load_a = [&](const int i, const int kc) __attribute__((always_inline)) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {                        // the unit's two 4-channel halves: each there, or the zero page
            const bool ok = a_off[i] != kDead && kc + a_q8 + hf * 4 < p.Cin;
            if constexpr (xb16) {
                const __bf16* sb = reinterpret_cast<const __bf16*>(p.x) + kc + a_off[i] + hf * 4;
                a_reg16[hf] = *reinterpret_cast<const uint2*>(ok ? reinterpret_cast<const void*>(sb) : reinterpret_cast<const void*>(p.zeros));
            } else {
                a_reg[hf] = *reinterpret_cast<const float4*>(ok ? p.x + kc + a_off[i] + hf * 4 : p.zeros);
            }
        }
    };
    auto store_a = [&](const int i, unsigned char* dst, const int kc) __attribute__((always_inline)) {
        if (a_lds[i] == kDead) return;
        uint4 o;
        if constexpr (xb16) {                                   // (channel groups of four are zero-padded by the producer)
            o = uint4{a_reg16[0].x, a_reg16[0].y, a_reg16[1].x, a_reg16[1].y};
        } else {
            uint2 h2[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float4 v = a_reg[hf];
                if (ragged && kc + CK > p.Cin) {
                    const int left = p.Cin - (kc + a_q8 + hf * 4);          // (<= 0: the half was loaded from the zero page)
                    v.y = left > 1 ? v.y : 0.f;
                    v.z = left > 2 ? v.z : 0.f;
                    v.w = left > 3 ? v.w : 0.f;
                }
                const dr_f32x4 f = {v.x, v.y, v.z, v.w};
                h2[hf] = __builtin_bit_cast(uint2, __builtin_convertvector(f, dr_bf16x4));
            }
            o = uint4{h2[0].x, h2[0].y, h2[1].x, h2[1].y};
        }
        *reinterpret_cast<uint4*>(dst + a_lds[i]) = o;
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
        a_frag[i] = (unsigned)(((r / W + 1) * Wp + (r & (W - 1)) + 1 - (Wp + 1)) * PIX + lk * 16);
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
            // the weight copy issued at the top of this tap has landed (this wave's share; the two loads of the halo fetch just issued may
            // stay in flight), every LDS read and write of this wave has completed -- then everybody's
            __builtin_amdgcn_sched_barrier(0);                              // (the tap's MFMAs are issued BEFORE the wait: the copy lands under them)
            if (fetch_a) P3_WAIT_VM(2); else P3_WAIT_VM(0);
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
    constexpr int EP_BATCH_ROWS = NW == 16 ? 4 : 8;
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
        // one partial row per 64 pixel rows, each the sum of its two 32-row tiles in order: the rows, and the bits, of conv_igemm's 64-row
        // tiles -- four rows per workgroup
        constexpr int kQ = BM / 64;
        const int srows = M >> 6;
        for (int e = tid; e < 2 * kQ * BN; e += NT) {
            const int qr = e / (2 * BN), which = (e / BN) % 2, col = e % BN, n = n0 + col;
            double tsum = 0.0;
#pragma unroll
            for (int w = 0; w < 2; ++w) tsum += red[(which * kG + qr * 2 + w) * BN + col];
            if (n < p.Cout) p.stat_part[((long)which * p.Cout + n) * srows + mblk * kQ + qr] = tsum;
        }
    }
    (void)NW; (void)M;
}

}  // namespace dr
