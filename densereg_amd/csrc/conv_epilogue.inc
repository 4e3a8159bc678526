// conv_epilogue.inc -- the epilogue shared by the conv kernels of conv_igemm.h, included TEXTUALLY inside each kernel
// body (a forceinline function taking the accumulators by reference made hipcc spill 16 bytes per lane in the hot
// 64x128 kernel; pasted in place the code is what it was).  The including kernel provides:
//   p (ConvParams), M, lk, li, ABL, m0 (the workgroup's first output row)
//   constexpr int EP_TM, EP_TN          MFMA tiles of this wave along M / N
//   constexpr int EP_TS, EP_NR          side of an MFMA output tile (32 / 16) and accumulator registers per lane and tile (16 / 4)
//   int ep_lg, ep_lc                    this lane's row group (lane >> 5 / lane >> 4: rows 4*ep_lg + ...) and column (lane & 31 / & 15)
//   acc[EP_TM][EP_TN][EP_NR]            the wave's accumulators (dr_f32x16 / dr_f32x4 tiles)
//   int ep_m0, ep_n0                    first row / column of the wave's tile
//   unsigned ep_rows                    bit r = accumulator register r: the rows of each tile this lane handles (0xFFFF
//                                       in the tiled kernels; a quarter per wave after the split-K reduction)
//   double s1[EP_TN], s2[EP_TN]         zero-initialised; receive the per-column statistics partials
//   constexpr int EP_BATCH_ROWS         8 or 16: accumulator rows of a tile column whose residual / BatchReNorm-backward /
//                                       dropout reads are issued as one batch (16 = one round trip per column, 16 more VGPRs)
//   constexpr bool EP_Y16, EP_B16       this COPY of the epilogue stores the (plain, raw) output as bf16 (ConvParams::y_bf16) / reads the
//                                       producer's raw output as bf16 (bst_raw_bf16).  The bf16 kernels include the epilogue once per
//                                       case behind a uniform branch: as run-time flags inside one copy the two paths cost the 64x160
//                                       kernel 228 bytes of scratch per lane and the 64x128 kernel 28; the fp32 kernels include one copy
//
    // D layout (32x32): col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5);  (16x16): col = lane&15, row = r + 4*(lane>>4)
#define ep_row(r) (EP_NR == 16 ? ((r) & 3) + 8 * ((r) >> 2) : (r))                         /* row of register r within the tile, minus 4*ep_lg */
    static_assert(EP_BATCH_ROWS <= EP_NR && EP_NR % EP_BATCH_ROWS == 0, "load batches tile the accumulator registers");
    // Every global read of the epilogue (output row mask, dropout keep bytes, residual) is issued as a batch of
    // independent, unconditional loads BEFORE the first use (a masked-off lane reads element 0 and ignores it):
    // written as "if (ok) v += res[...]" per element, hipcc serialises them behind s_waitcnt vmcnt(0) -- 16
    // dependent HBM round trips per 32x32 tile, which was most of the run time of the short-K 1x1 layers.
    // Indices are 32-bit element offsets from the (uniform) tensor base, so each access is "sgpr base + vgpr
    // offset" and costs one address register; launch_conv_igemm rejects tensors of 2^32 elements or more.
    // (the bf16-output copy is a PLAIN output by contract -- launch_conv_igemm checks: everything below folds away there)
    // (... and the copy that reads a BatchReNorm producer's bf16 raw output is an input-gradient launch: no fold, no ReLU, no dropout)
    constexpr bool EP_NOACT = EP_Y16 || (EP_B16 && EP_B16_CONST);
    const bool ep_res = !EP_Y16 && p.res, ep_drop = !EP_NOACT && p.drop, ep_drop_rng = !EP_NOACT && p.drop_rng, ep_relu = !EP_NOACT && p.relu;
    const bool ep_braw = (EP_B16 && EP_B16_CONST) || (!EP_Y16 && p.bst_raw);
    const bool dropping = ep_drop || ep_drop_rng;
    // The statistics: every element joins the fp64 partials one by one, unconditionally.  Measured and dropped in round 6: an fp32 sum
    // per batch of four rows joined to the fp64 partial once (+0.2 % on the step) moved config 5's train-mode maps at B = 1 from
    // 3e-5 ... 8e-5 of the oracle's to 3e-4 ... 5.5e-4 (E[x^2] - mean^2 cancels); a uniform "only when stat_part is set" branch around the
    // two accumulates (+0.7 % in eval) made hipcc spill in the 64x160 tiles and the 160-column x3 tile (tests/test_kernel_resources.py).
    constexpr int EP_B = EP_BATCH_ROWS;                                     // rows of a tile column per batch of epilogue loads (set by the including kernel)
    // The per-column coefficients of a tile column are ONE batch of unconditional loads (clamped column, zero page for absent
    // vectors, the uniform select happens at the use): behind "ptr ? ptr[n] : 1" every vector was its own round trip to L2,
    // and the workgroups of a launch run their epilogues in lockstep -- nothing hides it.
    const bool ep_bst = ep_braw && !p.bst_act;
    // micro-batch groups: this workgroup's group of rows selects the copy of the producer's coefficients -- ONE uniform offset
    // (scale | shift copies are grp_fold floats apart, the [mean | inv_std | r | d] copies twice that: four vectors against two
    // per layer); as adjusted pointers the three vectors cost six scalar registers and the bf16 64x128 kernel spilled
    // (no division: on the vector unit it takes registers the accumulators need -- at most seven scalar compare-and-adds)
    unsigned ep_goff = 0;
    if (ep_bst && p.grp_rows)
        for (int r = p.grp_rows; r <= m0; r += p.grp_rows) ep_goff += (unsigned)p.grp_fold;

#pragma unroll
    for (int i = 0; i < EP_TM; ++i) {
        const int mb = ep_m0 + i * EP_TS + 4 * ep_lg;         // row of r = 0
        unsigned rows = 0;                                                  // bit r: this lane writes row r
#pragma unroll
        for (int r = 0; r < EP_NR; ++r)
            if (mb + ep_row(r) < M) rows |= 1u << r;
        rows &= ep_rows;
        if (!EP_Y16 && p.out_rowmask) {
            float om[EP_NR];
#pragma unroll
            for (int r = 0; r < EP_NR; ++r) om[r] = p.out_rowmask[((rows >> r) & 1u) ? (unsigned)(mb + ep_row(r)) : 0u];
#pragma unroll
            for (int r = 0; r < EP_NR; ++r)
                if (om[r] < p.out_mask_thresh) rows &= ~(1u << r);
        }
#pragma unroll
        for (int j = 0; j < EP_TN; ++j) {
            const int n = ep_n0 + j * EP_TS + ep_lc;
            const bool n_ok = n < p.Cout;
            const unsigned nc = (unsigned)(n_ok ? n : p.Cout - 1);
            const float l_s = (!EP_NOACT && p.scale) ? p.scale[nc] : p.zeros[0], l_h = (!EP_NOACT && p.shift) ? p.shift[nc] : p.zeros[0];
            const float sc = (!EP_NOACT && p.scale) ? l_s : 1.f;                          // columns >= Cout: never stored (rows_j = 0)
            const float sh = (!EP_NOACT && p.shift) ? l_h : 0.f;
            const unsigned rows_j = n_ok ? rows : 0u;
            // BatchReNorm-backward statistics mode: the four coefficients of this column, in the same batch
            const float l_sc = ep_bst ? p.bst_scale[ep_goff + nc] : p.zeros[0], l_sh = ep_bst ? p.bst_shift[ep_goff + nc] : p.zeros[0];
            const float l_mean = ep_bst ? p.bst_bnc[2 * ep_goff + nc] : p.zeros[0], l_istd = ep_bst ? p.bst_bnc[2 * ep_goff + (unsigned)p.Cout + nc] : p.zeros[0];
            const float b_sc = ep_bst ? l_sc : 1.f, b_sh = ep_bst ? l_sh : 0.f, b_mean = ep_bst ? l_mean : 0.f, b_istd = ep_bst ? l_istd : 0.f;
            const float b_fac = p.bst_act ? p.bst_factor : 1.f;           // activation mode (bias conv + ReLU / dropout)
#pragma unroll
            for (int half = 0; half < EP_NR / EP_B; ++half) {                 // EP_B rows per load batch (bounds the VGPR peak)
                float rv[EP_B];
                float braw[EP_B];
                unsigned keep = 0xFFFFu;
                if (EP_B16 && (EP_B16_CONST || p.bst_raw_bf16)) {   // the producer stored its raw output as bf16: 16-bit loads, widened in place
#pragma unroll
                    for (int q = 0; q < EP_B; ++q) {
                        const int r = half * EP_B + q;
                        const unsigned m = (unsigned)(mb + ep_row(r));
                        const unsigned bits = reinterpret_cast<const unsigned short*>(p.bst_raw)[((rows_j >> r) & 1u) ? m * (unsigned)p.bst_cs + (unsigned)n : 0u];
                        braw[q] = __builtin_bit_cast(float, bits << 16);
                    }
                } else if (ep_braw) {
#pragma unroll
                    for (int q = 0; q < EP_B; ++q) {
                        const int r = half * EP_B + q;
                        const unsigned m = (unsigned)(mb + ep_row(r));
                        braw[q] = p.bst_raw[((rows_j >> r) & 1u) ? m * (unsigned)p.bst_cs + (unsigned)n : 0u];
                    }
                }
                if (ep_res) {
#pragma unroll
                    for (int q = 0; q < EP_B; ++q) {
                        const int r = half * EP_B + q;
                        const unsigned m = (unsigned)(mb + ep_row(r));
                        rv[q] = p.res[((rows_j >> r) & 1u) ? m * (unsigned)p.res_cs + (unsigned)(p.res_coff + n) : 0u];
                    }
                }
                if (ep_drop) {
                    unsigned char dv[EP_B];
#pragma unroll
                    for (int q = 0; q < EP_B; ++q) {
                        const int r = half * EP_B + q;
                        const unsigned m = (unsigned)(mb + ep_row(r));
                        dv[q] = p.drop[((rows_j >> r) & 1u) ? m * (unsigned)p.Cout + (unsigned)n : 0u];
                    }
                    keep = 0;
#pragma unroll
                    for (int q = 0; q < EP_B; ++q) keep |= (dv[q] ? 1u : 0u) << q;
                } else if (ep_drop_rng) {
                    keep = 0;
#pragma unroll
                    for (int q = 0; q < EP_B; ++q) {
                        const int r = half * EP_B + q;
                        const unsigned long long m = (unsigned long long)(mb + ep_row(r));
                        keep |= (dropout_keep(p.drop_seed, m * p.Cout + n) ? 1u : 0u) << q;
                    }
                }
#pragma unroll
                for (int q = 0; q < EP_B; ++q) {
                    const int r = half * EP_B + q;
                    if ((ABL == 3 || ABL == 9) && acc[i][j][r] != 12345.678f) continue;
                    if ((rows_j >> r) & 1u) {
                        const unsigned m = (unsigned)(mb + ep_row(r));
                        float raw = acc[i][j][r];
                        if (EP_Y16) raw = (float)(__bf16)raw;  // stored as bf16 below: the statistics are sums over what is stored
                        float v = raw * sc + sh;
                        if (ep_relu) v = fmaxf(v, 0.f);
                        if (dropping) v = ((keep >> q) & 1u) ? v * 2.f : 0.f;
                        if (ep_res) v += rv[q];
                        if (ep_braw) {
                            // a bf16-stored dOut (below): the sums are taken over the value the producer's apply pass will read back
                            if (EP_B16 && EP_B16_CONST && p.y_bf16) v = (float)(__bf16)v;
                            float g = v;
                            if (p.bst_relu && !(bn_affine(braw[q], b_sc, b_sh) > 0.f)) g = 0.f;
                            g *= b_fac;
                            if (p.bst_act) v = g;                          // the producer reads its dRaw straight from here
                            // (the copy that reads a bf16 raw output: dOut of a tensor this launch is the ONLY writer of may be stored
                            // as bf16 too -- its one reader is the producer's backward apply pass, train_exec.inc)
                            if (EP_B16 && EP_B16_CONST && p.y_bf16) reinterpret_cast<__bf16*>(p.y)[m * (unsigned)p.y_cs + (unsigned)(p.y_coff + n)] = (__bf16)v;
                            else DR_NT_STORE(4, &p.y[m * (unsigned)p.y_cs + (unsigned)(p.y_coff + n)], v);
                            const float yh = bn_yhat(braw[q], b_mean, b_istd);
                            s1[j] += (double)g;
                            s2[j] += (double)g * (double)yh;
                        } else {
                            // (y_bf16: a plain raw output -- launch_conv_igemm checks -- so v == raw, already a bf16 value)
                            if (EP_Y16) reinterpret_cast<__bf16*>(p.y)[m * (unsigned)p.y_cs + (unsigned)(p.y_coff + n)] = (__bf16)v;
                            else DR_NT_STORE(4, &p.y[m * (unsigned)p.y_cs + (unsigned)(p.y_coff + n)], v);
                            s1[j] += (double)raw;
                            s2[j] += (double)raw * (double)raw;
                        }
                    }
                }
            }
        }
    }
#undef ep_row
