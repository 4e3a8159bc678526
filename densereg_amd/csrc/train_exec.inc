// train_exec.inc -- training executors and their C ABI entry points (included by densereg.cpp).
//
// forward_train: detect_net(is_training=True)  (um_v1.py:71-185 with ops.py:130-171 BatchReNorm)
// loss:          JointDetectionModel.loss      (hourglass_um_crop_tiny.py:323-371)
// backward:      what TF's compute_gradients derives for that graph (train_single_gpu.py:71),
//                accumulated like accum_op (:84)
// apply_adam:    clip_by_value(acc/sub_batch) + AdamOptimizer.apply_gradients (:86-89)

namespace {

struct WgradPlan { int T; int nsplit; int rows_per_split; size_t partial_elems;
                   int wg16; };   // fp32: id of the 16x16-tile kernel that takes the layer instead (conv_wgrad16.h), 0 = none
void launch_wgrad_bf16(const WgradParams& p, int T, dim3 grid, hipStream_t s);
void launch_wgrad_square(const WgradParams& p, int T, dim3 grid, hipStream_t s);
bool wgrad_use_x3();
void plan_backward(dr_handle* h);

// workgroups per regularised variable in reg_loss_kernel (8 left the 590k-element weights as a 288-deep chain of
// dependent loads: 118 us)
constexpr int kRegRows = 64;
// layers of at most 16x16 pixels and this many rows (B*H*W) compute their weight gradient in the grouped launch at the end of the
// backward sweep (conv_wgrad.h: conv_wgrad_group_kernel).  Round 1-3: 10240 rows (everything up to 16x16 at B = 40); with the
// accumulation window as one pass (200 crops) that left the 8x8 and 16x16 layers (12 800 / 51 200 rows) with launches of their own:
// 65536 -> training 2569 -> 2590 crops/s (DR_GROUP_MAXM overrides).
static const long kGroupWgradMaxM = [] { const char* e = getenv("DR_GROUP_MAXM"); const long v = e ? atol(e) : 0; return v > 0 ? v : 65536l; }();

// A layer whose weight gradient may join the grouped launch: a BatchReNorm conv (its dRaw lives in a private buffer), both
// channel counts served by the 64-channel tile, small enough that its own launch cannot fill the chip.
inline bool wgrad_groupable(const ConvLayer& c, long M) {
    return c.bn && c.k != 7 && (long)c.H * c.W <= 256 && M <= kGroupWgradMaxM && c.g_keep != nullptr;
}

WgradPlan wgrad_plan(const ConvLayer& c, int B, bool force_square = false) {
    // How many slabs to cut the pixel axis (K of this GEMM) into.  The kernel is MFMA-bound per workgroup, so
    // what matters is how many workgroups land on the busiest of the 256 CUs and how many 16-pixel steps each one
    // runs; every slab costs a write and a read of the whole HWIO tile set.  A small cost model (constants from
    // profiles/r01_train_per_layer.md) replaces "about 1024 workgroups": e.g. 1x1 128->256 at 40960 pixels has
    // 2 tiles -- 160 slabs put 320 workgroups on 256 CUs (the busiest CU runs two), 128 slabs put exactly one
    // workgroup of 20 steps on every CU and write fewer slabs.
    WgradPlan w;
    const int taps = c.k * c.k;
    // Tile = the one that wastes fewer padded channels (ties -> 128: twice the arithmetic intensity).  DR_WG_TILE_RULE=1 (round 4,
    // measured and NOT adopted): count the busiest wave's LIVE 32x32 tiles instead -- the T = 128 kernel skips MFMA tiles beyond
    // Cin / Cout, so 515 -> 512 costs 72 tile-steps on either tile and the larger one has the better operand traffic per flop.
    // Alone the layer gains (200 crops: 1419 -> 1305 us, 156 -> 256 and 131 -> 128 equal), in the training step it loses (2589 ->
    // 2577 crops/s): these launches run on the side stream beside the sweep, where the 128-channel workgroups (33 KB of LDS, three
    // per CU) take more of a CU from the main stream's kernels than the 64-channel ones do.
    static const bool live_rule = [] { const char* e = getenv("DR_WG_TILE_RULE"); return e && e[0] == '1'; }();
    auto padded = [&](int T) { return (long)dr_ceil_div(c.cin, T) * dr_ceil_div(c.cout, T) * T * T; };
    auto cost64 = [&]() { return (long)dr_ceil_div(c.cin, 64) * dr_ceil_div(c.cout, 64); };
    auto cost128 = [&]() {
        long tot = 0;
        for (int ci0 = 0; ci0 < c.cin; ci0 += 128)
            for (int co0 = 0; co0 < c.cout; co0 += 128) {
                int busiest = 0;
                for (int wm = 0; wm < 2; ++wm)
                    for (int wn = 0; wn < 2; ++wn) {
                        const int na = std::max(0, std::min(2, dr_ceil_div(c.cin - (ci0 + wm * 64), 32)));
                        const int nb = std::max(0, std::min(2, dr_ceil_div(c.cout - (co0 + wn * 64), 32)));
                        busiest = std::max(busiest, na * nb);
                    }
                tot += busiest;
            }
        return tot;
    };
    // conv_wgrad_x3.h: the 128-channel tile skips MFMA tiles beyond Cin / Cout like the fp32 one, and its 64-channel sibling gains
    // little from the bf16 matrix cores (staging-bound) -- DR_WG_X3_T128=1 lets the live-tile rule decide there (measured neutral in
    // the step, profiles/r05_experiments.md section 5: the default is the padded rule).  The switch reads the ENVIRONMENT's x3 setting
    // only, never dr_dbg_force_x3: a plan must not change between the sizing of the slab buffers and the launch.
    static const bool x3_t128 = [] {
        const char* e = getenv("DR_WG_X3_T128"); const char* w = getenv("DR_WGRAD_X3"); const char* c = getenv("DR_CONV_X3");
        return e && e[0] == '1' && !(w && atoi(w) <= 0) && !(c && atoi(c) <= 0);
    }();
    if (live_rule || (x3_t128 && !force_square)) w.T = (c.cin > 64 && c.cout > 64 && cost128() <= cost64()) ? 128 : 64;
    else w.T = (padded(128) <= padded(64) && c.cin > 32 && c.cout > 32) ? 128 : 64;
    // 3x3 with 65..96 channels on both sides: one workgroup per kernel row (conv_wgrad_row_kernel), T = 96
    const bool row_kernel = c.k == 3 && c.cin <= 96 && c.cout <= 96 && std::min(c.cin, c.cout) > 64;
    if (row_kernel) w.T = 96;
    // fp32 layers whose channel counts waste most of a 32-channel MFMA tile grid: 16x16 tiles (conv_wgrad16.h; DR_WG16=0 off, a
    // bit mask selects kernels: 1 row80, 2 row32, 4 in80, 8 out80, 16 small).  The bf16 path keeps the square tiles (T above).
    // Measured at 200 crops per launch, kernel + fold (profiles/r04_wgrad16.md): 3x3 78->78 399 -> 298 us, 65->65 390 -> 292, 3x3
    // 32->32 104 -> 84, 16->16 @64x64 355 -> 277, 1x1 156->78 105 -> 84, 131->65 99 -> 82, 78->256 139 -> 115, 65->128 78 -> 63;
    // the 64x64-block variant for 16 / 32-channel 1x1 layers LOSES to the 64-channel MFMA block everywhere (32->16 59 -> 96 us,
    // 32->64 79 -> 112: too few live row blocks for four waves) and is off by default (bit 16).
    static const int wg16_mask = [] { const char* e = getenv("DR_WG16"); return e ? atoi(e) : 15; }();
    w.wg16 = WG16_NONE;
    const int cmin = std::min(c.cin, c.cout), cmax = std::max(c.cin, c.cout);
    if (c.k == 3 && cmin > 64 && cmax <= 80) w.wg16 = WG16_ROW80;
    else if (c.k == 3 && cmax <= 32) w.wg16 = WG16_ROW32;
    else if (c.k == 1 && c.cin > 64 && c.cin <= 80 && c.cout > 64) w.wg16 = WG16_IN80;
    else if (c.k == 1 && c.cout > 64 && c.cout <= 80 && c.cin > 80) w.wg16 = WG16_OUT80;
    else if (c.k == 1 && cmin <= 32 && c.cin <= 64 && c.cout <= 128) w.wg16 = WG16_SMALL;
    if (w.wg16 && !((wg16_mask >> (w.wg16 - 1)) & 1)) w.wg16 = WG16_NONE;
    if (force_square) w.wg16 = WG16_NONE;
    const long M = (long)B * c.H * c.W;
    const size_t per = (size_t)taps * c.cin * c.cout;
    // Slab count: workgroups per slab, us of MFMA issue per 16-pixel step and workgroup, us per step of a lone workgroup (load ->
    // LDS -> MFMA chain), resident workgroups per CU.
    long tiles; double t_mfma, t_lat; int occ;
    if (w.wg16) {
        tiles = wgrad16_blocks(w.wg16, c.cin, c.cout, c.k);
        // busiest wave: tiles x 4 MFMA steps x 32 cycles at ~2.1 GHz
        const int wave_tiles = w.wg16 == WG16_ROW80 ? 20 : w.wg16 == WG16_OUT80 ? 15 : w.wg16 == WG16_IN80 ? 10 : 4;
        t_mfma = wave_tiles * 4 * 32 / 2.1e3;
        t_lat = w.wg16 == WG16_ROW80 ? 1.2 : 0.6;
        occ = (w.wg16 == WG16_ROW80 || w.wg16 == WG16_OUT80) ? 2 : 4;
    } else {
        tiles = row_kernel ? 3 : (long)dr_ceil_div(c.cin, w.T) * dr_ceil_div(c.cout, w.T) * taps;
        // (32 / 8 per wave; the row kernel: its live share of 27 tiles x 8 / 4)
        const double live = 27.0;
        t_mfma = row_kernel ? live * 8 / 4 * 64 / 2.4e3 : (w.T == 128 ? 0.85 : 0.21);
        t_lat = row_kernel ? 1.2 : 0.6;
        occ = row_kernel ? 2 : (w.T == 128 ? 4 : 8);
    }
    static const double eff[5] = {1.0, 0.65, 0.85, 0.92, 0.95};   // MFMA pipe utilisation with k waves per SIMD
    const long max_ns = std::max<long>(1, std::min<long>(M / 64, (long)((size_t)(48u << 20) / per)));   // >= 4 steps, slab cap
    double best = 1e30;
    long best_ns = 1, best_rows = dr_round_up((int)M, 16);
    for (long ns_try = 1; ns_try <= max_ns; ++ns_try) {
        const long rows = dr_round_up((int)((M + ns_try - 1) / ns_try), 16);
        const long ns = (M + rows - 1) / rows;
        if (ns != ns_try) continue;                       // same plan as a smaller ns_try
        const long steps = rows / 16, blocks = tiles * ns;
        const long k = (blocks + 255) / 256;              // workgroups on the busiest CU
        const long rounds = (k + occ - 1) / occ, kr = std::min<long>(k, occ);
        const double t_step = std::max(kr * t_mfma / eff[std::min<long>(kr, 4)], t_lat);
        double cost = rounds * (steps * t_step + 4.0) + (double)ns * per * 8.0 / 3.0e6 + 3.0;
        if (ns >= 8 && (ns & 7) != 0) cost *= 1.02;      // slabs in multiples of 8 map one slab to one XCD (conv_wgrad.h)
        if (cost < best) { best = cost; best_ns = ns; best_rows = rows; }
    }
    // (Round 4, measured and not adopted: a table of the slab counts that are best in isolation at 200 crops per launch -- 3x3
    // 256->256 28 -> 64 slabs 2375 -> 2238 us, 1x1 512->512 64 -> 48 1090 -> 1048, 256<->512 128 -> 96 598 -> 564, 3x3 128->128 112 ->
    // 128 694 -> 670, profiles/r04_wgrad16.md -- changes nothing in the training step, 2569.5 vs 2571.6 crops/s: these launches run
    // on the side stream beside the backward sweep and are not what the step waits for.)
    w.nsplit = (int)best_ns;
    w.rows_per_split = (int)best_rows;
    w.partial_elems = (size_t)best_ns * per;
    return w;
}

int alloc_training_state(dr_handle* h) {
    std::vector<RegSeg> segs;
    int maxc = 1;
    size_t maxp = 1;
    for (auto& c : h->convs) {
        if (c.wd > 0.f) segs.push_back(RegSeg{(long)c.w_off, (long)c.k * c.k * c.cin * c.cout, c.wd});
        maxc = std::max(maxc, c.cout);
        if (c.k != 7) {
            // worst case over every batch size <= max_batch: the planner never exceeds M/64 slabs or 48M floats
            const size_t per = (size_t)c.k * c.k * c.cin * c.cout;
            const size_t Mmax = (size_t)h->cfg.max_batch * c.H * c.W;
            maxp = std::max(maxp, std::max<size_t>(1, std::min<size_t>(Mmax / 64, ((size_t)48u << 20) / per)) * per);
        } else {
            maxp = std::max(maxp, (size_t)dr_ceil_div((int)((size_t)h->cfg.max_batch * c.H * c.W), 256) * c.k * c.k * c.cout);
        }
    }
    h->n_reg = (int)segs.size();
    h->reg_segs = (RegSeg*)rt::dmalloc(std::max<size_t>(1, segs.size()) * sizeof(RegSeg));
    // partial rows of the loss kernels: [3][ceil(max_batch*map^2/256)] + kRegRows per regularised variable
    h->n_loss_part = (size_t)dr_ceil_div(h->cfg.max_batch * h->map_hw * h->map_hw, 256) * (size_t)h->cfg.num_jnt;   // one row per (pixel block, joint)
    h->n_loss_acc = 3 * h->n_loss_part + kRegRows * (size_t)std::max(h->n_reg, 1) + 4;
    h->loss_acc = (double*)rt::dmalloc(h->n_loss_acc * sizeof(double));
    h->bn_coef = (float*)rt::dmalloc(3 * (size_t)maxc * kMaxGroups * sizeof(float));    // [group][3][C]
    // wg_partial = [head: the largest single user, for immediate folds][slabs of a whole sweep, folded once at its end]
    size_t sweep = 0;
    for (auto& c : h->convs)
        if (c.k != 7) sweep += std::max(wgrad_plan(c, h->cfg.max_batch).partial_elems, wgrad_plan(c, h->cfg.max_batch, true).partial_elems);
    h->fold_head = maxp;
    h->n_wg_partial = maxp + 2 * sweep;                    // 2x: smaller batches may plan more slabs for some layers
    h->wg_partial = (float*)rt::dmalloc(h->n_wg_partial * sizeof(float));
    h->fold_dev = (FoldSeg*)rt::dmalloc(std::max<size_t>(1, h->convs.size()) * sizeof(FoldSeg));
    if (!h->fold_dev) return -1;
    h->bn_flags = (int*)rt::dmalloc(std::max<size_t>(1, h->convs.size()) * 4 * sizeof(int));
    if (!h->bn_flags) return -1;
    rt::memset_async(h->bn_flags, 0, std::max<size_t>(1, h->convs.size()) * 4 * sizeof(int), nullptr);
    {   // arg-max bytes of the max-pools (forward records, backward gathers)
        auto pool_arg_bytes = [&](const Op& op) { return ((size_t)h->cfg.max_batch * op.out.t->H * op.out.t->W * op.in.C + 255) / 256 * 256; };
        size_t need = 0;
        for (auto& op : h->ops)
            if (op.kind == OP_POOL) need += pool_arg_bytes(op);
        if (need > 0) {
            h->pool_arg_arena = (unsigned char*)rt::dmalloc(need);
            if (!h->pool_arg_arena) return -1;
            size_t off = 0;
            for (auto& op : h->ops)
                if (op.kind == OP_POOL) {
                    op.pool_off = off;
                    op.pool_arg = h->pool_arg_arena + off;
                    off += pool_arg_bytes(op);
                }
            h->n_pool_arg = need;
        }
    }
    {   // private dRaw buffers of the layers that can join the grouped weight-gradient launch at ANY batch size <= max_batch:
        // a layer qualifies by its pixel count at run time, so every BatchReNorm conv up to 16x16 pixels gets one
        // (with DR_WGRAD_STREAM=1 every BatchReNorm conv gets one: the full-resolution weight gradients run later too)
        // -- matching what backward_conv can use: `grouped` (small layers; a larger layer without a buffer simply keeps its own
        // launch at small batch sizes) and `side` (the map-resolution layers); the 64x64 stem-side layers never qualify
        auto keeps = [&](const ConvLayer& c) { return c.bn && c.k != 7 && ((long)c.H * c.W <= 256 || (h->wgrad_stream && c.H == h->map_hw)); };
        size_t keep = 0;
        for (auto& c : h->convs)
            if (keeps(c)) keep += (size_t)h->cfg.max_batch * c.H * c.W * dr_round_up(c.cout, 4);
        if (keep > 0) {
            h->g_keep_arena = (float*)rt::dmalloc(keep * sizeof(float));
            h->group_dev = (WgradGroupSeg*)rt::dmalloc(h->convs.size() * sizeof(WgradGroupSeg));
            if (!h->g_keep_arena || !h->group_dev) return -1;
            h->n_keep = keep; h->n_group_dev = h->convs.size();
            size_t off = 0;
            for (auto& c : h->convs)
                if (keeps(c)) {
                    c.g_keep_off = off;
                    c.g_keep = h->g_keep_arena + off;
                    off += (size_t)h->cfg.max_batch * c.H * c.W * dr_round_up(c.cout, 4);
                }
        }
    }
    if (!h->reg_segs || !h->loss_acc || !h->bn_coef || !h->wg_partial) return -1;
    h->wg_partial_l[0] = h->wg_partial;
    h->bn_coef_l[0] = h->bn_coef;
    {   // partial-sum rows: conv epilogue writes <= ceil(M/64) rows, the backward reduce <= 1024 workgroups
        size_t need = 1;
        for (auto& c : h->convs) {
            const size_t M = (size_t)h->cfg.max_batch * c.H * c.W;
            need = std::max(need, std::max<size_t>((M + 31) / 32, 1024) * 2 * (size_t)c.cout);     // one row per 32-row tile at most
        }
        h->n_stat_part = need;
        for (int l = 0; l < h->n_lanes; ++l) {
            h->stat_part_l[l] = (double*)rt::dmalloc(need * sizeof(double));
            h->stat_part2_l[l] = (double*)rt::dmalloc(need * sizeof(double));
            if (!h->stat_part_l[l] || !h->stat_part2_l[l]) return -1;
            if (l > 0) {
                h->bn_coef_l[l] = (float*)rt::dmalloc(3 * (size_t)maxc * kMaxGroups * sizeof(float));
                if (!h->bn_coef_l[l]) return -1;
            }
        }
    }
    for (int l = 1; l < h->n_lanes; ++l) {
        h->wg_partial_l[l] = (float*)rt::dmalloc(maxp * sizeof(float));
        if (!h->wg_partial_l[l]) return -1;
    }
    if (!segs.empty()) rt::h2d(h->reg_segs, segs.data(), segs.size() * sizeof(RegSeg), nullptr);
    rt::sync_stream(nullptr);
    plan_backward(h);
    return 0;
}

inline long rows_of(const Tensor* t, int B) { return (long)B * t->H * t->W; }

// Decide, once per graph, who writes each gradient buffer first in the reverse sweep.  A first writer that
// covers the whole tensor overwrites (no zero fill, no read-modify-write); only buffers whose first writer is
// partial (a channel slice of a concat buffer) or masked are zeroed per step.
void plan_backward(dr_handle* h) {
    std::vector<char> touched(h->tensors.size() + h->convs.size() + 8, 0);
    auto first_touch = [&](const TView& v, bool full_write_possible) -> bool {
        Tensor* t = v.t;
        if (!t->needs_grad) return false;
        if (touched[t->id]) return false;
        touched[t->id] = 1;
        const bool whole = v.coff == 0 && v.C == t->C;
        if (whole && full_write_possible) return true;
        t->needs_zero = true;
        return false;
    };
    for (auto& t : h->tensors) t->needs_zero = false;
    for (Tensor* t : h->hm) touched[t->id] = 1;        // the loss kernel writes the seeds (all channels)
    for (Tensor* t : h->hm3) touched[t->id] = 1;
    for (Tensor* t : h->um) touched[t->id] = 1;
    for (auto it = h->ops.rbegin(); it != h->ops.rend(); ++it) {
        Op& op = *it;
        op.ow_in = op.ow_in2 = false;
        switch (op.kind) {
            case OP_CONV:
            case OP_STEM:
                if (op.in2.valid()) op.ow_in2 = first_touch(op.in2, true);            // dres = dout
                if (op.kind == OP_CONV) op.ow_in = first_touch(op.in, !op.masked);      // dgrad (masked rows are skipped)
                break;
            case OP_COPY: op.ow_in = first_touch(op.in, true); break;
            case OP_UPADD: op.ow_in = first_touch(op.in, true); op.ow_in2 = first_touch(op.in2, true); break;
            case OP_POOL: op.ow_in = first_touch(op.in, true); break;                  // gather over the recorded arg-max
            default: break;
        }
    }
    h->zero_nseg = -1;                                   // table of the buffers to clear: built by the first dr_loss (the
                                                         // gradient pointers are assigned after this plan is made)
    // Which leading channels of a gradient buffer anybody consumes: the backward of every op that writes into the tensor
    // reads its slice, except OP_UVD (the coordinate / depth planes appended to a concat buffer come from the input).
    for (auto& t : h->tensors) t->grad_C = 0;
    for (const Op& op : h->ops) {
        if (op.kind == OP_FORK || op.kind == OP_JOIN || op.kind == OP_UVD || !op.out.valid()) continue;
        Tensor* t = op.out.t;
        t->grad_C = std::max(t->grad_C, op.out.coff + op.out.C);
    }
    // A BatchReNorm conv whose output tensor has exactly ONE reader, a conv that reads all of it unmasked and is the
    // first writer of its gradient: that reader's dgrad produces the layer's complete dOut, so it also produces the
    // layer's backward sums (conv_igemm.h, bst_*) and the layer skips its reduce pass.
    std::vector<int> readers(h->tensors.size(), 0);
    auto count = [&](const TView& v) { if (v.valid()) readers[v.t->id] += 1; };
    for (const Op& op : h->ops) {
        if (op.kind == OP_FORK || op.kind == OP_JOIN) continue;
        count(op.in); count(op.in2);
    }
    for (Tensor* t : h->hm) readers[t->id] += 1;              // read by the loss / read_maps
    for (Tensor* t : h->hm3) readers[t->id] += 1;
    for (Tensor* t : h->um) readers[t->id] += 1;
    for (Op& op : h->ops) { op.bst_conv = -1; op.bst_last = false; }
    // A/B switches of the two extensions of the fused reductions (both default on; DR_FUSE_BN_BWD=0 disables all of it)
    const char* e_act = getenv("DR_FUSE_ACT");
    const char* e_last = getenv("DR_FUSE_LAST");
    const bool fuse_act = !(e_act && e_act[0] == '0'), fuse_last = !(e_last && e_last[0] == '0');
    for (size_t i = 0; i < h->ops.size(); ++i) {
        const Op& prod = h->ops[i];
        if (prod.kind != OP_CONV) continue;
        // a bias conv qualifies when it has a ReLU (um_full 1 / 2, with dropout): its reader's dgrad then writes the
        // gradient wrt its pre-activation and the bias column sums (conv_igemm.h, bst_act)
        if (!h->convs[prod.conv].bn && !(h->convs[prod.conv].relu && !prod.in2.valid() && fuse_act)) continue;
        const Tensor* t = prod.out.t;
        // the producer wrote the whole tensor -- or (round 4, DR_FUSE_SLICE=0 off) the LEADING channels of a concat buffer whose
        // remaining channels have no gradient consumer (comb|uvd: 512 channels of the um-head residual + the three uvd planes; its
        // reader's input gradient is computed for the first 512 columns only, which is exactly the producer's dOut)
        static const bool fuse_slice = [] { const char* e = getenv("DR_FUSE_SLICE"); return !(e && e[0] == '0'); }();
        const bool whole = prod.out.coff == 0 && prod.out.C == t->C;
        const bool leading = fuse_slice && h->convs[prod.conv].bn && prod.out.coff == 0 && prod.out.C < t->C && t->grad_C == prod.out.C;
        if (!(whole || leading) || readers[t->id] != 1 || !t->needs_grad) continue;
        for (Op& cons : h->ops) {
            if (cons.kind != OP_CONV || cons.in.t != t) continue;
            if (cons.in.coff == 0 && cons.in.C == t->C && !cons.masked && cons.ow_in && cons.lane == prod.lane &&
                h->convs[cons.conv].k != 7)
                cons.bst_conv = prod.conv;
        }
    }
    // Several readers (a residual module's output feeds the next module's first conv AND its skip path): the gradient
    // buffer is complete once its LAST writer of the reverse sweep has run, i.e. the backward of the FIRST reader in
    // forward order.  When that reader is a conv reading the whole tensor unmasked, its (accumulating) dgrad epilogue sees
    // the final dOut values -- existing + its own contribution -- and reduces the producer's BatchReNorm backward sums
    // there; the producer's reduce pass (two tensor reads and a launch) disappears.
    for (size_t i = 0; i < h->ops.size(); ++i) {
        const Op& prod = h->ops[i];
        if (prod.kind != OP_CONV || !h->convs[prod.conv].bn) continue;
        const Tensor* t = prod.out.t;
        if (!fuse_last || prod.out.coff != 0 || prod.out.C != t->C || readers[t->id] < 2 || !t->needs_grad) continue;
        bool taken = false;
        for (const Op& o : h->ops) taken = taken || o.bst_conv == prod.conv;
        if (taken) continue;
        for (size_t j = i + 1; j < h->ops.size(); ++j) {             // first reader in forward order
            Op& cons = h->ops[j];
            if (cons.kind == OP_FORK || cons.kind == OP_JOIN) continue;
            const bool reads = (cons.in.valid() && cons.in.t == t) || (cons.in2.valid() && cons.in2.t == t);
            if (!reads) continue;
            if (cons.kind == OP_CONV && cons.in.t == t && !(cons.in2.valid() && cons.in2.t == t) && cons.in.coff == 0 &&
                cons.in.C == t->C && !cons.masked && !cons.ow_in && cons.lane == prod.lane && h->convs[cons.conv].k != 7 &&
                cons.bst_conv < 0 && t->grad_C >= t->C) {
                cons.bst_conv = prod.conv;
                cons.bst_last = true;
            }
            break;
        }
    }
    // activations with a single reader that is a conv reading all of it unmasked, produced whole by a BatchReNorm conv without
    // a residual add: candidates for bf16 storage on the bf16 path (net.h, Tensor::reader_op)
    for (auto& t : h->tensors) t->reader_op = -1;
    for (size_t i = 0; i < h->ops.size(); ++i) {
        const Op& prod = h->ops[i];
        if (prod.kind != OP_CONV || !h->convs[prod.conv].bn || prod.in2.valid()) continue;
        Tensor* t = prod.out.t;
        if (prod.out.coff != 0 || prod.out.C != t->C || readers[t->id] != 1) continue;
        for (size_t j = i + 1; j < h->ops.size(); ++j) {
            const Op& cons = h->ops[j];
            if (cons.kind == OP_CONV && cons.in.t == t && cons.in.coff == 0 && cons.in.C == t->C && !cons.masked && h->convs[cons.conv].k != 7 &&
                !(cons.in2.valid() && cons.in2.t == t))
                t->reader_op = (int)j;
        }
    }
    // Projection residuals (the graph builder's residual() with num_out != cin: c1, c2, cs, c3 with c3.in2 = cs's output): both
    // BatchReNorm branches meet in c3's apply passes and the skip activation is never written or differentiated on its own
    // (train_kernels.h: bn_train_join_kernel, bn_bwd_join_kernel).  fp32 storage and finalize-launch coefficients only;
    // DR_BN_JOIN=0 keeps the two-pass path (A/B, tests).  Re-planned by dr_set_precision.
    {
        const char* e_join = getenv("DR_BN_JOIN");
        h->bn_join = !(e_join && e_join[0] == '0');
    }
    for (Op& op : h->ops) { op.join_role = 0; op.join_peer = -1; }
    if (h->bn_join && h->precision == 0 && !h->bn_lookback) {
        for (size_t j = 0; j < h->ops.size(); ++j) {
            Op& c3 = h->ops[j];
            if (c3.kind != OP_CONV || !h->convs[c3.conv].bn || !c3.in2.valid()) continue;
            const Tensor* t = c3.in2.t;
            if (c3.in2.coff != 0 || c3.in2.C != t->C || readers[t->id] != 1) continue;      // the whole tensor, read by this add only
            for (size_t i = 0; i < j; ++i) {
                Op& cs = h->ops[i];
                if (cs.kind != OP_CONV || cs.out.t != t) continue;
                const ConvLayer& ls = h->convs[cs.conv];
                const ConvLayer& l3 = h->convs[c3.conv];
                if (ls.bn && ls.relu && !cs.in2.valid() && cs.out.coff == 0 && cs.out.C == t->C && cs.lane == c3.lane && cs.join_role == 0 && c3.join_role == 0 &&
                    ls.cout == l3.cout && ls.H == l3.H && ls.W == l3.W) {
                    cs.join_role = 1; cs.join_peer = (int)j;
                    c3.join_role = 2; c3.join_peer = (int)i;
                }
            }
        }
    }
    if (getenv("DR_DEBUG_PLAN")) {
        int n_bn = 0, n_only = 0, n_last = 0, n_act = 0, n_join = 0;
        for (const Op& o : h->ops) n_join += o.join_role == 2 ? 1 : 0;
        for (auto& c : h->convs) n_bn += c.bn ? 1 : 0;
        for (const Op& o : h->ops)
            if (o.bst_conv >= 0) { if (!h->convs[o.bst_conv].bn) ++n_act; else if (o.bst_last) ++n_last; else ++n_only; }
        fprintf(stderr, "[densereg] plan_backward: %d BatchReNorm layers, sums fused into the only reader's dgrad: %d, into the last writer's: %d; bias convs fused: %d; projection residuals joined: %d\n",
                n_bn, n_only, n_last, n_act, n_join);
    }
}

// ---------------------------------------------------------------------------------------------
int run_conv_train(dr_handle* h, const Op& op, int B, hipStream_t s) {
    ConvLayer& c = h->convs[op.conv];
    const long M = (long)B * c.H * c.W;
    if (!c.bn) {
        // bias conv: same kernel as eval + dropout
        ConvParams p{};
        p.x = op.in.t->p; p.x_cs = op.in.t->cs; p.x_coff = op.in.coff; p.Cin = op.in.C;
        p.B = B; p.H = c.H; p.W = c.W; p.ksize = c.k;
        p.w = h->wp + c.wp_off; p.Kp = c.Kp; p.Np = c.Np;
        p.w3 = h->precision == 0 && h->wp3 ? h->wp3 + 3 * c.wp_off : nullptr;
        p.y = op.out.t->p; p.y_cs = op.out.t->cs; p.y_coff = op.out.coff; p.Cout = c.cout;
        p.shift = h->flat_param + c.bias_off; p.relu = c.relu; p.zeros = h->zeros;
        if (h->precision == 1) { p.bf16 = 1; p.Kp = dr_round_up(c.cin, 32); p.x_bf16 = op.in.t->is_bf16 ? 1 : 0; }
        if (op.in2.valid()) { p.res = op.in2.t->p; p.res_cs = op.in2.t->cs; p.res_coff = op.in2.coff; }
        if (op.dropout >= 0) {
            if (h->dropout_mode == DR_DROPOUT_MASK) p.drop = h->keep_mask + (size_t)op.dropout * M * c.cout;
            else if (h->dropout_mode == DR_DROPOUT_RNG) { p.drop_rng = 1; p.drop_seed = h->seed * 1000003ull + (unsigned)op.dropout; }
        }
        ProfScope ps(h, s, conv_tile_id(p), 2.0 * M * c.k * c.k * c.cin * c.cout, 4.0 * M * ((double)c.cin + c.cout));
        if (launch_conv_igemm(p, s)) DR_FAIL(h, DR_E_STATE, "conv %s: unsupported layout", c.name.c_str());
        return DR_OK;
    }
    Tensor* raw = c.raw;
    const double* part = nullptr;       // [2][C][part_rows] partial moments of the raw output, folded by the BatchReNorm finalize
    int part_rows = 1;
    // micro-batch groups (dr_set_groups): G consecutive micro-batches of Mg rows, statistics and state chain per group
    const int G = h->groups;
    const long Mg = M / G;
    if (op.kind == OP_STEM) {
        StemParams sp{};
        sp.x = h->dm_in; sp.B = B; sp.H = h->cfg.in_hw; sp.W = h->cfg.in_hw;
        sp.w = h->flat_param + c.w_off; sp.k = c.k; sp.stride = c.stride;
        const int total = std::max((c.H - 1) * c.stride + c.k - sp.H, 0);
        sp.pad_t = total / 2; sp.pad_l = total / 2; sp.Ho = c.H; sp.Wo = c.W;
        sp.y = raw->p; sp.y_cs = raw->cs; sp.scale = nullptr; sp.shift = nullptr; sp.relu = 0;
        {
            ProfScope ps(h, s, KID_STEM, 2.0 * M * c.k * c.k * c.cout, 4.0 * (B * (double)sp.H * sp.W + M * c.cout));
            DR_LAUNCH(stem_conv_kernel, dim3(dr_ceil_div((int)M, 64)), dim3(256), 0, s, sp);
        }
        ProfScope ps(h, s, KID_BN, 0.0, 4.0 * M * c.cout);
        const int rows_g = bn_moments_rows(Mg, G);          // one partial row per workgroup, folded like a conv epilogue's rows
        part_rows = rows_g * G;
        double* rows = h->stat_part_l[op.lane];
        part = rows;
        DR_LAUNCH(moments_kernel, dim3(rows_g, G), dim3(256), 0, s, (const float*)raw->p, raw->cs, 0, Mg, c.cout, rows);
    } else {
        ConvParams p{};
        p.x = op.in.t->p; p.x_cs = op.in.t->cs; p.x_coff = op.in.coff; p.Cin = op.in.C;
        p.B = B; p.H = c.H; p.W = c.W; p.ksize = c.k;
        p.w = h->wp + c.wp_off; p.Kp = c.Kp; p.Np = c.Np;
        p.w3 = h->precision == 0 && h->wp3 ? h->wp3 + 3 * c.wp_off : nullptr;
        p.y = raw->p; p.y_cs = raw->cs; p.y_coff = 0; p.Cout = c.cout;
        if (op.masked) { p.rowmask = h->tiny; p.mask_thresh = -0.9f; }
        p.stat_part = h->stat_part_l[op.lane]; p.zeros = h->zeros;
        if (h->precision == 1) { p.bf16 = 1; p.Kp = dr_round_up(c.cin, 32); p.x_bf16 = op.in.t->is_bf16 ? 1 : 0; }
        if (G > 1) p.grp_rows = (int)Mg;                    // tiles cut at the group boundaries (conv_tile_id)
        // bf16 path: the raw output of a BatchReNorm conv is stored as bf16 -- the forward apply, the backward reduce (or the
        // reader's dgrad epilogue) and the backward apply read it at half the bytes, this epilogue writes half (DR_BF16_RAW=0 off)
        raw->is_bf16 = h->bf16_raw && h->precision == 1 && !h->bn_lookback;     // (the opt-in look-back kernels read fp32 only)
        p.y_bf16 = raw->is_bf16 ? 1 : 0;
        part = p.stat_part; part_rows = conv_stat_rows(p);
        if (G > 1 && Mg % conv_tile_rows(p)) DR_FAIL(h, DR_E_STATE, "conv %s: %d-row tiles straddle the micro-batch groups of %ld rows", c.name.c_str(), conv_tile_rows(p), Mg);
        ProfScope ps(h, s, conv_tile_id(p), 2.0 * M * c.k * c.k * c.cin * c.cout, 4.0 * M * ((double)c.cin + c.cout));
        if (launch_conv_igemm(p, s)) DR_FAIL(h, DR_E_STATE, "conv %s: unsupported layout", c.name.c_str());
    }
    // tensor passes of the apply: raw in, activation out (+ the residual in); a joined projection residual (plan_backward) streams
    // nothing for its skip conv and two raw tensors in, one activation out for its last conv
    const double bn_passes = op.join_role == 1 ? 0.0 : (2.0 + (op.in2.valid() ? 1.0 : 0.0));
    ProfScope ps(h, s, KID_BN, 0.0, 4.0 * M * c.cout * bn_passes);
    BnTrainParams bp{};
    bp.raw = raw->p; bp.raw_cs = raw->cs; bp.M = M; bp.C = c.cout; bp.raw_bf16 = raw->is_bf16 ? 1 : 0;
    bp.part = part; bp.part_rows = part_rows;
    bp.beta = h->flat_param + c.beta_off; bp.gamma = h->flat_param + c.gamma_off;
    bp.mm = h->flat_state + c.mm_off; bp.mv = h->flat_state + c.mv_off;
    bp.mm_next = h->flat_state_next + c.mm_off; bp.mv_next = h->flat_state_next + c.mv_off;
    bp.shadow_mean = h->shadow + c.shadow_off; bp.shadow_var = h->shadow + c.shadow_off + c.cout;
    bp.shadow_step = c.shadow_step + 1;                      // the first group's; group g's = this + g (train_kernels.h)
    c.shadow_step += G;
    bp.r_max = c.r_max; bp.d_max = c.d_max; bp.eps = 0.001f; bp.decay = 0.99f;
    bp.groups = G; bp.Mg = Mg; bp.rows_per_group = part_rows / G; bp.fold_stride = (long)h->n_fold; bp.bnc_stride = (long)h->n_bnc;
    if (G > 1 && part_rows % G) DR_FAIL(h, DR_E_STATE, "conv %s: %d statistics rows for %d groups", c.name.c_str(), part_rows, G);
    for (int g = 0; g < G; ++g) {
        bp.r_max_g[g] = c.r_max; bp.d_max_g[g] = c.d_max;
        // schedule scalars (ops.py:141-153), all from the OLD curr_t -- once per micro-batch
        const double t = (double)c.curr_t;
        c.r_max = (float)(3.0 / (1.0 + 2.0 * std::exp(-t)));
        c.d_max = (float)(5.0 / ((1.0 + 5.0 / 1e-3 - 1.0) * std::exp(-2.0 * t)));
        c.curr_t = (float)(t + 1e-5);
    }
    bp.scale = h->fold + c.fold_off; bp.shift = h->fold + c.fold_off + c.cout;
    bp.bnc = h->bnc + c.bnc_off; bp.relu = c.relu ? 1 : 0;
    bp.res = View{nullptr, 0, 0, 0};
    if (op.in2.valid()) bp.res = op.in2.fwd();
    bp.out = op.out.fwd();
    {   // bf16 storage of an activation whose only reader is a conv on the bf16 matrix cores (not the split-K kernel: fp32 only)
        Tensor* to = op.out.t;
        bool a16 = h->bf16_act && h->precision == 1 && to->reader_op >= 0 && !op.in2.valid() && op.kind == OP_CONV;
        if (a16) {
            const Op& cons = h->ops[to->reader_op];
            const ConvLayer& cc = h->convs[cons.conv];
            ConvParams q{};
            q.B = B; q.H = cc.H; q.W = cc.W; q.ksize = cc.k; q.Np = cc.Np; q.Kp = dr_round_up(cc.cin, 32); q.bf16 = 1;
            if (G > 1) q.grp_rows = (int)((long)(B / G) * cc.H * cc.W);      // (the reader may need the 32-row kernel: conv_tile_id)
            a16 = conv_tile_id(q) != KID_CONV_SPLITK;
        }
        to->is_bf16 = a16;
        bp.out_bf16 = a16 ? 1 : 0;
    }
    if (raw->cs / 4 > 256) DR_FAIL(h, DR_E_UNSUPPORTED, "BatchReNorm layer wider than 1024 channels");
    const BnForm form = bn_form(bp.part_rows, G, op.join_role != 0, h->bn_lookback);
    if (op.join_role) {                                      // joined projection residual: always the finalize-launch form
        if (raw->is_bf16 || bp.out_bf16 || h->precision != 0 || h->bn_lookback) DR_FAIL(h, DR_E_STATE, "conv %s: joined BatchReNorm branches need the fp32 path", c.name.c_str());
        launch_bn_fwd_finalize(bp, s);
        if (op.join_role == 1) return DR_OK;                 // the skip conv: coefficients only, the peer's apply forms its activation
        const ConvLayer& cs = h->convs[h->ops[op.join_peer].conv];
        if (cs.raw->cs != raw->cs || cs.raw->is_bf16) DR_FAIL(h, DR_E_STATE, "conv %s: joined skip branch with another layout", c.name.c_str());
        BnJoinParams jp{};
        jp.b = bp; jp.b.res = View{nullptr, 0, 0, 0};
        jp.raw2 = cs.raw->p; jp.scale2 = h->fold + cs.fold_off; jp.shift2 = h->fold + cs.fold_off + cs.cout;
        launch_bn_fwd_join(jp, s);
        return DR_OK;
    }
    if (form == kBnLookback) {
        c.ep_fwd += 1;
        bp.flag = h->bn_flags + 4 * op.conv; bp.flag_target = c.ep_fwd * dr_ceil_div(c.cout, 4);
    }
    if (launch_bn_fwd_apply(bp, form, s)) DR_FAIL(h, DR_E_STATE, "conv %s: the look-back BatchReNorm apply reads fp32 only", c.name.c_str());
    return DR_OK;
}

int forward_train_impl(dr_handle* h, int B, const float* dm, hipStream_t s) {
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    if (!h->finalized) DR_FAIL(h, DR_E_STATE, "forward before dr_finalize_params");
    if (B < 1 || B > h->cfg.max_batch) DR_FAIL(h, DR_E_INVALID, "batch %d outside [1, max_batch=%d]", B, h->cfg.max_batch);
    if (h->groups > 1) {
        if (B % h->groups) DR_FAIL(h, DR_E_INVALID, "batch %d is not %d micro-batch groups of equal size", B, h->groups);
        if (h->bn_lookback) DR_FAIL(h, DR_E_UNSUPPORTED, "micro-batch groups: not with DR_BN_LOOKBACK");
        // every launch that writes per-workgroup statistics rows must cut its tiles at the group boundaries: the forward conv of
        // each BatchReNorm layer and the input-gradient launches that carry a producer's backward sums (plan_backward)
        const int Bg = B / h->groups;
        for (const Op& op : h->ops) {
            if (op.kind != OP_CONV) continue;
            const ConvLayer& c = h->convs[op.conv];
            const long Mg = (long)Bg * c.H * c.W;
            ConvParams q{};
            q.B = B; q.H = c.H; q.W = c.W; q.ksize = c.k; q.grp_rows = (int)Mg;
            int rows_f = 32, rows_b = 32;
            if (c.bn) {
                q.Np = c.Np; q.Kp = h->precision == 1 ? dr_round_up(c.cin, 32) : c.Kp; q.bf16 = h->precision == 1; q.Cout = c.cout;
                rows_f = conv_tile_rows(q);
            }
            if (op.bst_conv >= 0) {
                q.Np = c.NpT; q.Kp = h->precision == 1 ? dr_round_up(c.cout, 32) : c.KpT; q.bf16 = h->precision == 1; q.Cout = c.cin;
                const int need = std::min(c.cin, std::max(op.in.t->grad_C - op.in.coff, 0));       // (backward_conv: dgrad_need)
                if (need > 0 && need < c.cin && h->convs[op.bst_conv].cout == need) { q.Cout = need; q.Ng = dr_round_up(need, 32); }
                rows_b = conv_tile_rows(q);
                q.Ng = 0;
            }
            if (Mg % rows_f || Mg % rows_b || ((c.bn || op.bst_conv >= 0) && Mg % 32))
                DR_FAIL(h, DR_E_UNSUPPORTED, "micro-batch groups of %d crops: %ld rows per group in the %dx%d layer %s, its tiles have %d / %d rows",
                        Bg, Mg, c.H, c.W, c.name.c_str(), rows_f, rows_b);
        }
        if (((long)Bg * h->map_hw * h->map_hw) % 256) DR_FAIL(h, DR_E_UNSUPPORTED, "micro-batch groups of %d crops: the loss needs whole 256-pixel blocks per group", Bg);
    }
    DR_ENTER(h);
    h->dm_in = dm;
    h->dm_train = dm;
    h->fold_is_eval = false;
    for (auto& t : h->tensors) t->is_bf16 = false;           // set again, layer by layer, by the BatchReNorm apply passes below
    for (const Op& op : h->ops) {
        if (op.kind == OP_FORK || op.kind == OP_JOIN) { lane_edge(h, op, op.kind == OP_FORK, s); continue; }
        h->prof_tag = op.conv;
        hipStream_t ls = lane_of(h, op.lane, s);
        int rc = (op.kind == OP_CONV || op.kind == OP_STEM) ? run_conv_train(h, op, B, ls) : run_simple_op(h, op, B, ls, true);
        if (rc) return rc;
    }
    h->prof_tag = -1;
    std::swap(h->flat_state, h->flat_state_next);      // every BatchReNorm layer wrote its slice of `next`
    DR_CHECK_LAUNCH(h);
    h->last_forward_train = true;
    h->last_B = B;
    return DR_OK;
}

// ---------------------------------------------------------------------------------------------
int backward_conv(dr_handle* h, const Op& op, int B, hipStream_t s) {
    ConvLayer& c = h->convs[op.conv];
    const long M = (long)B * c.H * c.W;
    // the layer's weight gradient joins the grouped launch at the end of the sweep: dRaw goes to its private buffer
    const bool grouped = h->group_wgrad && !h->multi_stream && h->precision == 0 && !op.masked && wgrad_groupable(c, M) &&
                         std::max(c.cin, c.cout) <= 128 && h->group_dev != nullptr;
    // ... or runs later on the side stream (full-resolution layers, DR_WGRAD_STREAM=1): same need
    const bool side = h->wgrad_stream && !h->profiling && c.k != 7 && c.H == h->map_hw && !grouped &&
                      (!c.bn || c.g_keep != nullptr);
    float* const scratch = (grouped || (side && c.bn)) ? c.g_keep : h->scratch_l[op.lane];   // lanes run concurrently: private dRaw scratch and slabs
    // bf16 matrix cores: dRaw of a full-resolution BatchReNorm layer is stored as bf16 -- its two readers (dgrad A operand,
    // weight-gradient G operand) round it to bf16 while staging anyway, so the numbers do not change and the tensor is half
    // the bytes in three passes (DR_BF16_DRAW=0 keeps fp32)
    bool g16 = h->bf16_draw && h->precision == 1 && c.bn && c.k != 7 && !grouped;
    // output columns of this layer's dgrad launch: trailing input channels without a consumer (uvd planes of a concat buffer:
    // 515 -> 512, 131 -> 128 columns) are not computed; 0 = all of NpT
    const int dgrad_need = std::min(c.cin, std::max(op.in.t->grad_C - op.in.coff, 0));
    // (a dgrad that also carries its producer's BatchReNorm-backward sums may be narrowed when the producer wrote exactly the leading
    // channels that are left: comb|uvd -- plan_backward)
    const bool dgrad_narrowed = dgrad_need < c.cin && dgrad_need > 0 && (op.bst_conv < 0 || h->convs[op.bst_conv].cout == dgrad_need);
    if (g16 && op.in.t->needs_grad) {                        // the split-K kernel of the small grids stages fp32 only
        ConvParams q{};                                      // the tile the dgrad launch below will select: same grid inputs
        q.B = B; q.H = c.H; q.W = c.W; q.ksize = c.k; q.Np = c.NpT; q.Kp = dr_round_up(c.cout, 32); q.bf16 = 1;
        if (dgrad_narrowed) q.Ng = dr_round_up(dgrad_need, 32);
        if (h->groups > 1) q.grp_rows = (int)(M / h->groups);
        g16 = conv_tile_id(q) != KID_CONV_SPLITK;
    }
    float* const wg_partial = h->wg_partial_l[op.lane];
    // (a joined skip conv -- plan_backward -- has no gradient buffer of its own to read: d(skip activation) = the module's dOut)
    const View dout = op.join_role == 1 ? h->ops[op.join_peer].out.grad() : op.out.grad();
    // residual branch: out = act(...) + res  =>  dres += dout (BatchReNorm layers: inside their backward apply pass; the last conv
    // of a joined projection residual reduces the skip conv's backward sums there instead and writes no dres)
    const bool wants_dres = op.in2.valid() && op.in2.t->needs_grad && op.join_role != 2;
    const bool dres_in_bn = c.bn && wants_dres;
    if (wants_dres && !dres_in_bn) {
        ProfScope ps(h, s, KID_ELTWISE, 0.0, 12.0 * M * c.cout);
        const View dres = op.in2.grad();
        DR_LAUNCH(copy_channels_kernel, dim3(grid_for(M * c.cout)), dim3(256), 0, s, (const float*)dout.p, dout.cs, dout.coff,
                  dres.p, dres.cs, dres.coff, M, c.cout, op.ow_in2 ? 0 : 1);
    }
    // gradient wrt the raw conv output -> G (dense scratch, or dout itself for linear convs)
    const float* G = nullptr;
    int g_cs = 0, g_coff = 0;
    if (c.bn) {
        // tensor passes: the reduce reads dOut and raw, the apply reads both and writes dRaw; joined projection residual: the skip
        // conv runs the apply only, the last conv's apply reads the skip conv's raw output as well
        const double bn_passes = op.join_role == 1 ? 3.0 : op.join_role == 2 ? (c.bst_rows > 0 ? 4.0 : 6.0) : 5.0;
        ProfScope ps(h, s, KID_BN, 0.0, 4.0 * M * c.cout * bn_passes);
        const float* scale = h->fold + c.fold_off;
        const float* shift = scale + c.cout;
        const float* bnc = h->bnc + c.bnc_off;
        Tensor* raw = c.raw;
        BnBwdParams bp{};
        bp.dout = dout; bp.raw = raw->p; bp.raw_cs = raw->cs; bp.M = M; bp.C = c.cout; bp.relu = c.relu ? 1 : 0;
        bp.raw_bf16 = raw->is_bf16 ? 1 : 0;
        bp.dout_bf16 = op.out.t->g_bf16 ? 1 : 0;
        // (a bf16-stored dOut is the whole tensor, written by the launch that also reduced this layer's sums: anything else here
        // would read bf16 elements as fp32)
        if (bp.dout_bf16 && (dout.coff != 0 || dout.C != op.out.t->C || c.bst_rows <= 0 || !bp.raw_bf16 || h->bn_lookback))
            DR_FAIL(h, DR_E_STATE, "conv %s: bf16-stored output gradient without its fused backward sums", c.name.c_str());
        bp.scale = scale; bp.shift = shift; bp.bnc = bnc; bp.gamma = h->flat_param + c.gamma_off;
        bp.part = h->stat_part_l[op.lane]; bp.coef = h->bn_coef_l[op.lane];
        bp.dbeta = h->gacc + c.beta_off; bp.dgamma = h->gacc + c.gamma_off;
        bp.draw = scratch; bp.draw_bf16 = g16 ? 1 : 0;
        if (dres_in_bn) { bp.dres = op.in2.grad(); bp.dres_acc = op.ow_in2 ? 0 : 1; }
        const int G_ = h->groups;                                     // micro-batch groups: per-group sums and coefficients
        const long Mg = M / G_;
        bp.groups = G_; bp.Mg = Mg; bp.fold_stride = (long)h->n_fold; bp.bnc_stride = (long)h->n_bnc;
        if (op.join_role == 1) {                                      // the joined peer's apply pass already reduced (plan_backward)
            if (c.join_rows <= 0) DR_FAIL(h, DR_E_STATE, "conv %s: joined skip branch without its backward sums", c.name.c_str());
            bp.part_rows = c.join_rows;                               // (in stat_part: the peer's dgrad wrote stat_part2 since)
            c.join_rows = 0;
        } else if (c.bst_rows > 0) {                                  // the reader's dgrad already reduced (plan_backward)
            bp.part = h->stat_part2_l[op.lane];
            bp.part_rows = c.bst_rows;
            c.bst_rows = 0;
        } else {
            launch_bn_bwd_reduce(bp, s);
        }
        bp.rows_per_group = bp.part_rows / G_;
        if (bp.part_rows % G_) DR_FAIL(h, DR_E_STATE, "conv %s: %d backward rows for %d groups", c.name.c_str(), bp.part_rows, G_);
        const BnForm form = bn_form(bp.part_rows, G_, op.join_role != 0, h->bn_lookback);
        if (op.join_role && (bp.raw_bf16 || bp.dout_bf16 || bp.draw_bf16 || h->bn_lookback))
            DR_FAIL(h, DR_E_STATE, "conv %s: joined BatchReNorm branches need the fp32 path", c.name.c_str());
        if (form == kBnLookback) {
            c.ep_bwd += 1;
            bp.flag = h->bn_flags + 4 * op.conv + 2; bp.flag_target = c.ep_bwd * dr_ceil_div(c.cout, 4);
        }
        if (op.join_role == 2) {                                      // also reduces the skip conv's sums, for its finalize + apply
            ConvLayer& cs = h->convs[h->ops[op.join_peer].conv];
            if (cs.raw->cs != raw->cs || cs.raw->is_bf16) DR_FAIL(h, DR_E_STATE, "conv %s: joined skip branch with another layout", c.name.c_str());
            launch_bn_bwd_finalize(bp, s);
            BnBwdJoinParams jp{};
            jp.b = bp;
            jp.raw2 = cs.raw->p; jp.scale2 = h->fold + cs.fold_off; jp.shift2 = h->fold + cs.fold_off + cs.cout; jp.bnc2 = h->bnc + cs.bnc_off;
            jp.part2 = h->stat_part_l[op.lane];                       // (this layer's own rows there, if any, were folded by the finalize above)
            cs.join_rows = launch_bn_bwd_join(jp, h->n_stat_part, s);
            if (cs.join_rows <= 0) DR_FAIL(h, DR_E_STATE, "conv %s: the skip branch's partial rows go beyond the statistics buffer", c.name.c_str());
        } else if (launch_bn_bwd_apply(bp, form, s)) {
            DR_FAIL(h, DR_E_STATE, "conv %s: no BatchReNorm backward apply for this storage", c.name.c_str());
        }
        G = scratch; g_cs = raw->cs; g_coff = 0;
    } else if (c.bst_rows > 0) {
        // the reader's dgrad wrote G = dOut * factor * [out > 0] in place of dOut and the bias column sums (plan_backward)
        G = dout.p; g_cs = dout.cs; g_coff = dout.coff;
        ProfScope ps(h, s, KID_ELTWISE, 0.0, 16.0 * c.bst_rows * c.cout);
        DR_LAUNCH(bias_grad_from_rows_kernel, dim3(dr_ceil_div(c.cout, 4)), dim3(256), 0, s, (const double*)h->stat_part2_l[op.lane],
                  c.bst_rows, c.cout, h->gacc + c.bias_off);
        c.bst_rows = 0;
    } else {
        const bool dropped = op.dropout >= 0 && h->dropout_mode != DR_DROPOUT_OFF;
        if (c.relu || dropped) {
            ProfScope ps(h, s, KID_ELTWISE, 0.0, 12.0 * M * c.cout);
            const int gcs = dr_round_up(c.cout, 4);
            DR_LAUNCH(act_bwd_kernel, dim3(grid_for(M * (gcs / 4))), dim3(256), 0, s, dout, op.out.fwd(), c.relu ? 1 : 0,
                      dropped ? 2.0f : 1.0f, scratch, gcs, M, c.cout);
            G = scratch; g_cs = gcs; g_coff = 0;
        } else {
            G = dout.p; g_cs = dout.cs; g_coff = dout.coff;
        }
        ProfScope ps(h, s, KID_ELTWISE, 0.0, 4.0 * M * c.cout);
        const int rows = grid_for(M / 8, 1, 256);
        DR_LAUNCH(colsum_kernel, dim3(rows), dim3(256), 0, s, G, g_cs, g_coff, M, c.cout, wg_partial);
        DR_LAUNCH(wgrad_reduce_kernel, dim3(grid_for(c.cout, 64)), dim3(256), 0, s, (const float*)wg_partial, rows, (long)c.cout,
                  h->gacc + c.bias_off);
    }
    if (g_coff % 4 || g_cs % 4) DR_FAIL(h, DR_E_STATE, "conv %s: gradient view not 16-byte aligned", c.name.c_str());

    // ---- weight gradient ---------------------------------------------------------------------
    if (op.kind == OP_STEM) {
        ProfScope ps(h, s, KID_WGRAD, 2.0 * M * c.k * c.k * c.cout, 4.0 * M * c.cout);
        const int in_hw = h->cfg.in_hw;
        const int total = std::max((c.H - 1) * c.stride + c.k - in_hw, 0);
        if (c.k != 7 || c.stride != 2 || c.cout != 32 || c.W % 64) DR_FAIL(h, DR_E_UNSUPPORTED, "stem wgrad: not the 7x7/s2 1->32 stem of um_v1.py:86");
        const int units = B * c.H * (c.W / 64), units_per_wg = 4, rows = dr_ceil_div(units, units_per_wg);
        const long n = (long)c.k * c.k * c.cout;
        if ((size_t)rows * n > h->n_wg_partial) DR_FAIL(h, DR_E_STATE, "wgrad slab too small for the stem");
        DR_LAUNCH(stem_wgrad_kernel, dim3(rows), dim3(256), 0, s, h->dm_train, B, in_hw, in_hw, G, g_cs, total / 2, total / 2, c.H, c.W,
                  units_per_wg, wg_partial);
        DR_LAUNCH(wgrad_reduce_kernel, dim3(grid_for(n, 64)), dim3(256), 0, s, (const float*)wg_partial, rows, n, h->gacc + c.w_off);
        return DR_OK;
    }
    {
        // Cin = a multiple of 128 plus a few channels (515 = 512 + u, v, d of the heads' comb|uvd inputs; 131): the leading channels on the
        // 128-channel x3 tile, the last ones by conv_wgrad_tail_kernel, both into the same slabs (conv_wgrad.h; DR_WG_TAIL=0 off).  On its
        // own tile plan 515 -> 512 ran on nine x eight 64-channel tiles at 88-97 TFLOP/s (a 128-channel plan pads Cin to 640).
        static const bool tail_on = [] { const char* e = getenv("DR_WG_TAIL"); return !(e && e[0] == '0'); }();
        int tail = (tail_on && h->precision == 0 && wgrad_use_x3() && c.k == 1 && c.cin > 128 && c.cin % 128 <= 4 && c.cout > 32 && !grouped)
                       ? c.cin % 128 : 0;
        ConvLayer cm = c;
        cm.cin = c.cin - tail;
        WgradPlan wp = wgrad_plan(cm, B, /*force_square=*/h->precision == 1);   // (the 16x16-tile kernels are fp32)
        if (tail) {
            wp.partial_elems = (size_t)wp.nsplit * c.cin * c.cout;              // (a slab holds all Cin rows)
            if (wp.T != 128 || wp.wg16 || wp.partial_elems > h->fold_head) {     // (not the plan the split is for: the layer as one launch)
                tail = 0; cm.cin = c.cin;
                wp = wgrad_plan(c, B, h->precision == 1);
            }
        }
        if (wp.partial_elems > h->fold_head) DR_FAIL(h, DR_E_STATE, "wgrad slab too small");
        // single-stream executor: keep the slabs and fold every layer in ONE launch at the end of the sweep
        const bool defer = !h->multi_stream && h->fold_used + wp.partial_elems <= h->n_wg_partial;
        float* const slab = defer ? h->wg_partial + h->fold_used : wg_partial;
        WgradParams p{};
        p.x = op.in.t->p; p.x_cs = op.in.t->cs; p.x_coff = op.in.coff; p.Cin = cm.cin;
        p.g = G; p.g_cs = g_cs; p.g_coff = g_coff; p.Cout = c.cout;
        p.B = B; p.H = c.H; p.W = c.W; p.ksize = c.k;
        if (op.masked) { p.rowmask = h->tiny; p.mask_thresh = -0.9f; }
        p.partial = slab; p.nsplit = wp.nsplit; p.rows_per_split = wp.rows_per_split;
        WgradParams pt{};                                          // the tail launch: the last `tail` input channels, same slabs
        if (tail) {
            p.cin_total = c.cin;
            pt = p; pt.Cin = tail; pt.ci_base = cm.cin;
        }
        const int tail_grid = wp.nsplit * dr_ceil_div(c.cout, 64);
        p.g_bf16 = (g16 && G == scratch) ? 1 : 0;
        p.x_bf16 = (h->precision == 1 && op.in.t->is_bf16) ? 1 : 0;
        if ((long long)M * std::max(p.x_cs, p.g_cs) >= (1ll << 32)) DR_FAIL(h, DR_E_UNSUPPORTED, "wgrad %s: tensor beyond 32-bit offsets", c.name.c_str());
        const int taps = c.k * c.k;
        const long n = (long)taps * c.cin * c.cout;
        bool in_group = false;
        if (grouped) {
            // ~512 pixels (32 steps) per workgroup: the chip is filled by the OTHER layers of the group, so a layer needs
            // few slabs (a 16x16 layer: 20 instead of the 40-160 its own launch would cut to reach every CU)
            const int ns = (int)((M + 511) / 512);
            const int rows = dr_round_up((int)((M + ns - 1) / ns), 16);
            const int nsg = (int)((M + rows - 1) / rows);
            const size_t pe = (size_t)nsg * (size_t)n;
            if (h->fold_used + pe <= h->n_wg_partial) {
                WgradGroupSeg sg{};
                sg.p = p;
                sg.p.partial = h->wg_partial + h->fold_used; sg.p.nsplit = nsg; sg.p.rows_per_split = rows;
                sg.first_block = h->group_blocks;
                h->group_host.push_back(sg);
                h->group_blocks += dr_ceil_div(c.cin, 64) * dr_ceil_div(c.cout, 64) * taps * nsg;
                h->group_flops += 2.0 * M * taps * c.cin * c.cout;
                h->group_bytes += 4.0 * M * ((double)c.cin + c.cout);
                h->fold_host.push_back(FoldSeg{(long)c.w_off, n, (long)h->fold_used, nsg, h->fold_blocks});
                h->fold_used += pe;
                h->fold_blocks += (int)((n + 63) / 64);
                in_group = true;
            }
        }
        // side stream: G must outlive this step of the sweep -- a BatchReNorm layer's private dRaw buffer, or the output's
        // gradient buffer itself (linear bias convs, and ReLU ones whose reader's dgrad wrote G in place)
        const bool g_persists = c.bn ? (G == c.g_keep) : (G == dout.p);
        if (!in_group && side && defer && g_persists) {
            dr_handle::PendingWgrad pw{};
            pw.p = p;
            if (h->precision == 1) {                              // bf16 matrix cores: square tiles only
                const int Tb = wp.T == 64 ? 64 : 128;
                pw.kind = Tb == 128 ? 4 : 3; pw.grid = dr_ceil_div(c.cin, Tb) * dr_ceil_div(c.cout, Tb) * taps * wp.nsplit;
            } else if (wp.wg16) { pw.kind = 16 + wp.wg16; pw.grid = wgrad16_blocks(wp.wg16, c.cin, c.cout, c.k) * wp.nsplit; }
            else if (wp.T == 96) { pw.kind = 2; pw.grid = 3 * wp.nsplit; }
            else { pw.kind = wp.T == 128 ? 1 : 0; pw.grid = dr_ceil_div(cm.cin, wp.T) * dr_ceil_div(c.cout, wp.T) * taps * wp.nsplit; }
            h->wg_pending.push_back(pw);
            if (tail) { dr_handle::PendingWgrad pq{}; pq.p = pt; pq.kind = 5; pq.grid = tail_grid; h->wg_pending.push_back(pq); }
            h->fold_host.push_back(FoldSeg{(long)c.w_off, n, (long)h->fold_used, wp.nsplit, h->fold_blocks});
            h->fold_used += wp.partial_elems;
            h->fold_blocks += (int)((n + 63) / 64);
            in_group = true;                                     // = "not launched here, folded at the end"
        }
        if (!in_group) {
            const int kid = (h->precision == 1 ? (wp.T == 64 ? KID_WGRAD_64 : KID_WGRAD_128)
                                               : (wp.wg16 ? KID_WGRAD_16 : wp.T == 96 ? KID_WGRAD_ROW
                                                  : wgrad_use_x3() ? (wp.T == 128 ? KID_WGRAD_X3_128 : KID_WGRAD_X3_64) : (wp.T == 128 ? KID_WGRAD_128 : KID_WGRAD_64)));
            ProfScope ps(h, s, kid, 2.0 * M * taps * c.cin * c.cout, 4.0 * M * ((double)c.cin + c.cout));
            if (h->precision == 1) {                                  // bf16 matrix cores: square tiles only (a 65..96-wide
                const int Tb = wp.T == 64 ? 64 : 128;                // layer is one 128-tile per tap, same slab layout)
                dim3 grid(dr_ceil_div(c.cin, Tb) * dr_ceil_div(c.cout, Tb) * taps * wp.nsplit);
                launch_wgrad_bf16(p, Tb, grid, s);
            } else if (wp.wg16) {
                launch_wgrad16(wp.wg16, p, wgrad16_blocks(wp.wg16, c.cin, c.cout, c.k) * wp.nsplit, s);
            } else if (wp.T == 96) {
                DR_LAUNCH(conv_wgrad_row_kernel, dim3(3 * wp.nsplit), dim3(256), 0, s, p);
            } else {
                dim3 grid(dr_ceil_div(cm.cin, wp.T) * dr_ceil_div(c.cout, wp.T) * taps * wp.nsplit);
                launch_wgrad_square(p, wp.T, grid, s);
                if (tail) DR_LAUNCH(conv_wgrad_tail_kernel, dim3(tail_grid), dim3(256), 0, s, pt);
            }
        }
        if (in_group) {
            // folded with everybody else at the end of the sweep
        } else if (defer) {
            h->fold_host.push_back(FoldSeg{(long)c.w_off, n, (long)h->fold_used, wp.nsplit, h->fold_blocks});
            h->fold_used += wp.partial_elems;
            h->fold_blocks += (int)((n + 63) / 64);
        } else {
            ProfScope ps(h, s, KID_WGRAD_FOLD, 0.0, 4.0 * n * (wp.nsplit + 2.0));   // the slab fold: HBM-bound, its own row
            DR_LAUNCH(wgrad_reduce_kernel, dim3(grid_for(n, 64)), dim3(256), 0, s, (const float*)slab, wp.nsplit, n,
                      h->gacc + c.w_off);
        }
    }
    // ---- input gradient: dX += conv(G, W^T flipped) --------------------------------------------
    if (op.in.t->needs_grad) {
        ConvParams p{};
        p.x = G; p.x_cs = g_cs; p.x_coff = g_coff; p.Cin = c.cout;
        p.B = B; p.H = c.H; p.W = c.W; p.ksize = c.k;
        p.w = h->wpT + c.wpT_off; p.Kp = c.KpT; p.Np = c.NpT;
        p.w3 = h->precision == 0 && h->wp3T ? h->wp3T + 3 * c.wpT_off : nullptr;
        if (h->precision == 1) { p.bf16 = 1; p.Kp = dr_round_up(c.cout, 32); p.x_bf16 = (g16 && G == scratch) ? 1 : 0; }
        const View dx = op.in.grad();
        p.y = dx.p; p.y_cs = dx.cs; p.y_coff = dx.coff; p.Cout = c.cin;
        if (!op.ow_in) { p.res = dx.p; p.res_cs = dx.cs; p.res_coff = dx.coff; }      // accumulate unless first writer
        if (dgrad_narrowed) { p.Cout = dgrad_need; p.Ng = dr_round_up(dgrad_need, 32); }   // (see dgrad_need above)
        if (op.masked) { p.out_rowmask = h->tiny; p.out_mask_thresh = -0.9f; }
        p.zeros = h->zeros;
        if (op.bst_conv >= 0 && (op.ow_in || (op.bst_last && !h->multi_stream)) && h->fuse_bn_bwd) {
            ConvLayer& pl = h->convs[op.bst_conv];                    // the layer that produced this conv's input
            p.stat_part = h->stat_part2_l[op.lane];
            if (pl.bn) {
                p.bst_raw = pl.raw->p; p.bst_cs = pl.raw->cs; p.bst_relu = pl.relu ? 1 : 0;
                p.bst_raw_bf16 = pl.raw->is_bf16 ? 1 : 0;
                p.bst_scale = h->fold + pl.fold_off; p.bst_shift = h->fold + pl.fold_off + pl.cout;
                p.bst_bnc = h->bnc + pl.bnc_off;
                if (h->groups > 1) { p.grp_rows = (int)(M / h->groups); p.grp_fold = (int)h->n_fold; }
            } else {                                                  // bias conv + ReLU (+ dropout): mask on its OUTPUT
                bool dropped = false;
                for (const Op& po : h->ops)
                    if (po.kind == OP_CONV && po.conv == op.bst_conv) dropped = po.dropout >= 0 && h->dropout_mode != DR_DROPOUT_OFF;
                p.bst_raw = op.in.t->p + op.in.coff; p.bst_cs = op.in.t->cs; p.bst_relu = 1;
                p.bst_act = 1; p.bst_factor = dropped ? 2.0f : 1.0f;
            }
            // bf16 path: this launch is the ONLY writer of dX (first writer of a tensor with one reader), dX is the whole tensor,
            // whole channel groups of four, and its one reader -- the producer's BatchReNorm backward apply -- comes later in this
            // sweep: stored as bf16 (half the bytes written here and read there; DR_BF16_GACT=0 off)
            if (h->bf16_gact && p.bst_raw_bf16 && pl.bn && !op.bst_last && op.ow_in && !p.res && !dgrad_narrowed && !op.masked &&
                dx.coff == 0 && dx.C == op.in.t->C && pl.cout == op.in.t->C && c.cin % 4 == 0 && dx.cs % 4 == 0) {
                p.y_bf16 = 1;
                op.in.t->g_bf16 = true;
            }
            pl.bst_rows = conv_stat_rows(p);
            if (h->groups > 1 && (M / h->groups) % conv_tile_rows(p))
                DR_FAIL(h, DR_E_STATE, "dgrad %s: %d-row tiles straddle the micro-batch groups", c.name.c_str(), conv_tile_rows(p));
        }
        ProfScope ps(h, s, conv_tile_id(p), 2.0 * M * c.k * c.k * p.Cout * c.cout, 4.0 * M * (2.0 * p.Cout + c.cout));
        if (launch_conv_igemm(p, s)) DR_FAIL(h, DR_E_STATE, "dgrad %s: unsupported layout", c.name.c_str());
    }
    return DR_OK;
}

// fp32 square-tile weight gradient: the fp32 matrix cores, or -- conv_wgrad_x3.h -- fp32-accurate products on the bf16 ones
// (DR_WGRAD_X3=0 off; follows DR_CONV_X3 / dr_dbg_force_x3)
bool wgrad_use_x3() {
    static const int env = [] { const char* e = getenv("DR_WGRAD_X3"); return e ? atoi(e) : 1; }();
    static const int conv_env = [] { const char* e = getenv("DR_CONV_X3"); return e ? atoi(e) : 1; }();
    const int mode = g_dbg_x3 >= 0 ? g_dbg_x3 : std::min(env, conv_env);
    return mode > 0;
}
void launch_wgrad_square(const WgradParams& p, int T, dim3 grid, hipStream_t s) {
    if (wgrad_use_x3()) {
        // (an eight-wave form of the T = 128 kernel -- 64x32 wave tiles, the lower waves staging x, the upper ones g -- measured 27
        // TFLOP/s against 155: 132 bytes of scratch per lane inside its pixel loop; profiles/r05_experiments.md; not kept)
        if (T == 128) DR_LAUNCH((conv_wgrad_x3_kernel<128>), grid, dim3(256), 0, s, p);
        else DR_LAUNCH((conv_wgrad_x3_kernel<64>), grid, dim3(256), 0, s, p);
    } else {
        if (T == 128) DR_LAUNCH((conv_wgrad_kernel<128>), grid, dim3(256), 0, s, p);
        else DR_LAUNCH((conv_wgrad_kernel<64>), grid, dim3(256), 0, s, p);
    }
}

// bf16 weight-gradient kernel: tile T, and whether the G operand is stored as bf16 (a compile-time variant: a run-time
// branch around the staging loads kept hipcc from batching them -- 3.5 -> 4.3 ms of weight gradients per step)
void launch_wgrad_bf16(const WgradParams& p, int T, dim3 grid, hipStream_t s) {
    // default: the LDS-transpose-read kernel (conv_wgrad_tr.h); DR_WGRAD_TR=0 selects the register-transposing one
    static const bool tr = [] { const char* e = getenv("DR_WGRAD_TR"); return !(e && e[0] == '0'); }();
    if (tr || p.x_bf16) {                                       // (only the transpose-read kernel stages a bf16-stored x)
        if (T == 128) {
            if (p.x_bf16) {
                if (p.g_bf16) DR_LAUNCH((conv_wgrad_tr_kernel<128, 1, 1>), grid, dim3(256), 0, s, p);
                else DR_LAUNCH((conv_wgrad_tr_kernel<128, 0, 1>), grid, dim3(256), 0, s, p);
            } else if (p.g_bf16) DR_LAUNCH((conv_wgrad_tr_kernel<128, 1, 0>), grid, dim3(256), 0, s, p);
            else DR_LAUNCH((conv_wgrad_tr_kernel<128, 0, 0>), grid, dim3(256), 0, s, p);
        } else {
            if (p.x_bf16) {
                if (p.g_bf16) DR_LAUNCH((conv_wgrad_tr_kernel<64, 1, 1>), grid, dim3(256), 0, s, p);
                else DR_LAUNCH((conv_wgrad_tr_kernel<64, 0, 1>), grid, dim3(256), 0, s, p);
            } else if (p.g_bf16) DR_LAUNCH((conv_wgrad_tr_kernel<64, 1, 0>), grid, dim3(256), 0, s, p);
            else DR_LAUNCH((conv_wgrad_tr_kernel<64, 0, 0>), grid, dim3(256), 0, s, p);
        }
        return;
    }
    if (T == 128) {
        if (p.g_bf16) DR_LAUNCH((conv_wgrad_bf16_kernel<128, 1>), grid, dim3(256), 0, s, p);
        else DR_LAUNCH((conv_wgrad_bf16_kernel<128, 0>), grid, dim3(256), 0, s, p);
    } else {
        if (p.g_bf16) DR_LAUNCH((conv_wgrad_bf16_kernel<64, 1>), grid, dim3(256), 0, s, p);
        else DR_LAUNCH((conv_wgrad_bf16_kernel<64, 0>), grid, dim3(256), 0, s, p);
    }
}

// Release the queued full-resolution weight gradients to the side stream: everything they read (activations, dRaw /
// gradient buffers) was produced by launches already enqueued on the main stream.
void flush_side_wgrads(dr_handle* h, hipStream_t main_s) {
    if (h->wg_pending.empty()) return;
    rt::event_record(h->wg_ready, main_s);
    rt::stream_wait_event(h->wg_stream, h->wg_ready);
    for (auto& pw : h->wg_pending) {
        if (pw.kind == 5) DR_LAUNCH(conv_wgrad_tail_kernel, dim3(pw.grid), dim3(256), 0, h->wg_stream, pw.p);
        else if (pw.kind > 16) launch_wgrad16(pw.kind - 16, pw.p, pw.grid, h->wg_stream);
        else if (pw.kind == 4 || pw.kind == 3) launch_wgrad_bf16(pw.p, pw.kind == 4 ? 128 : 64, dim3(pw.grid), h->wg_stream);
        else if (pw.kind == 2) DR_LAUNCH(conv_wgrad_row_kernel, dim3(pw.grid), dim3(256), 0, h->wg_stream, pw.p);
        else launch_wgrad_square(pw.p, pw.kind == 1 ? 128 : 64, dim3(pw.grid), h->wg_stream);
    }
    rt::event_record(h->wg_done, h->wg_stream);
    h->wg_pending.clear();
    h->wg_side_used = true;
}

int backward_impl(dr_handle* h, int B, hipStream_t main_s) {
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    if (!h->last_forward_train || B != h->last_B) DR_FAIL(h, DR_E_STATE, "dr_backward needs dr_forward_train + dr_loss with the same B first");
    DR_ENTER(h);
    for (auto& c : h->convs) { c.bst_rows = 0; c.join_rows = 0; }
    for (auto& t : h->tensors) t->g_bf16 = false;             // set again by the input-gradient launches of this sweep
    h->fold_host.clear();
    h->fold_used = h->fold_head;
    h->fold_blocks = 0;
    h->group_host.clear();
    h->group_blocks = 0;
    h->group_flops = h->group_bytes = 0.0;
    h->wg_pending.clear();
    h->wg_side_used = false;
    for (auto it = h->ops.rbegin(); it != h->ops.rend(); ++it) {
        const Op& op = *it;
        // reverse sweep: a JOIN of the forward order forks here (parent -> child), a FORK joins
        if (op.kind == OP_FORK || op.kind == OP_JOIN) { lane_edge(h, op, op.kind == OP_JOIN, main_s); continue; }
        h->prof_tag = op.conv;
        hipStream_t s = lane_of(h, op.lane, main_s);
        // entering a region below the map resolution (the hourglass pyramid): what was queued runs beside it
        if (h->wgrad_stream && op.out.valid() && op.out.t->H < h->map_hw) flush_side_wgrads(h, main_s);
        switch (op.kind) {
            case OP_CONV:
            case OP_STEM: {
                int rc = backward_conv(h, op, B, s);
                if (rc) return rc;
                if (h->wg_flush_every > 0 && (int)h->wg_pending.size() >= h->wg_flush_every) flush_side_wgrads(h, main_s);
                break;
            }
            case OP_COPY: {
                ProfScope ps(h, s, KID_ELTWISE, 0.0, 12.0 * rows_of(op.in.t, B) * op.in.C);
                const View dsrc = op.in.grad(), ddst = op.out.grad();
                const long M = rows_of(op.in.t, B);
                DR_LAUNCH(copy_channels_kernel, dim3(grid_for(M * op.in.C)), dim3(256), 0, s, (const float*)ddst.p, ddst.cs,
                          ddst.coff, dsrc.p, dsrc.cs, dsrc.coff, M, op.in.C, op.ow_in ? 0 : 1);
                break;
            }
            case OP_UPADD: {
                const Tensor* to = op.out.t;
                ProfScope ps(h, s, KID_ELTWISE, 0.0, 4.0 * rows_of(to, B) * op.out.C * 3.5);
                DR_LAUNCH(upsample_add_bwd_kernel, dim3(grid_for((long)B * (to->H / 2) * (to->W / 2) * op.out.C)), dim3(256), 0, s,
                          op.out.grad(), op.in.grad(), op.in2.grad(), B, to->H, to->W, op.out.C, op.ow_in ? 0 : 1,
                          op.ow_in2 ? 0 : 1);
                break;
            }
            case OP_POOL: {
                const Tensor* ti = op.in.t; const Tensor* to = op.out.t;
                const int k = op.pool_k;
                const int total = std::max((to->H - 1) * 2 + k - ti->H, 0);
                ProfScope ps(h, s, KID_ELTWISE, 0.0, 4.0 * B * op.in.C * (2.0 * ti->H * ti->W + (double)to->H * to->W));
                const View dx = op.in.grad(), dy = op.out.grad();
                DR_LAUNCH(maxpool_bwd_kernel, dim3(grid_for((long)B * ti->H * ti->W * (op.in.C / 4))), dim3(256), 0, s,
                          (const unsigned char*)op.pool_arg, dx.p, dx.cs, dx.coff, B, ti->H, ti->W, op.in.C, k, total / 2, total / 2,
                          (const float*)dy.p, dy.cs, dy.coff, to->H, to->W, op.ow_in ? 0 : 1);
                break;
            }
            default: break;
        }
    }
    h->prof_tag = -1;
    if (h->wgrad_stream) {
        flush_side_wgrads(h, main_s);                          // the rest (stem side of the network)
        if (h->wg_side_used) rt::stream_wait_event(main_s, h->wg_done);   // the fold below reads their slabs
    }
    if (!h->group_host.empty()) {                              // the small layers' weight gradients, one launch
        const size_t nb = h->group_host.size() * sizeof(WgradGroupSeg);
        std::vector<WgradGroupSeg>& uploaded = h->slot[h->cur_slot].group_uploaded;     // the table names this slot's buffers
        if (uploaded.size() != h->group_host.size() || memcmp(uploaded.data(), h->group_host.data(), nb)) {
            if (rt::h2d(h->group_dev, h->group_host.data(), nb, main_s)) DR_FAIL(h, DR_E_DEVICE, "h2d of the wgrad group table failed");
            rt::sync_stream(main_s);                           // host memory that changes; only on a new plan (another B)
            uploaded = h->group_host;
        }
        ProfScope ps(h, main_s, KID_WGRAD_GROUP, h->group_flops, h->group_bytes);
        DR_LAUNCH(conv_wgrad_group_kernel, dim3(h->group_blocks), dim3(256), 0, main_s, (const WgradGroupSeg*)h->group_dev,
                  (int)h->group_host.size());
    }
    if (!h->fold_host.empty()) {                               // every layer's weight-gradient slabs, one launch
        const size_t nb = h->fold_host.size() * sizeof(FoldSeg);
        std::vector<FoldSeg>& uploaded = h->slot[h->cur_slot].fold_uploaded;
        if (uploaded.size() != h->fold_host.size() || memcmp(uploaded.data(), h->fold_host.data(), nb)) {
            if (rt::h2d(h->fold_dev, h->fold_host.data(), nb, main_s)) DR_FAIL(h, DR_E_DEVICE, "h2d of the fold table failed");
            rt::sync_stream(main_s);                           // the table is host memory that changes; only on a new plan
            uploaded = h->fold_host;
        }
        double bytes = 0;
        for (auto& f : h->fold_host) bytes += 4.0 * f.n * (f.nsplit + 2.0);
        ProfScope ps(h, main_s, KID_WGRAD_FOLD, 0.0, bytes);
        DR_LAUNCH(wgrad_fold_all_kernel, dim3(h->fold_blocks), dim3(256), 0, main_s, (const float*)h->wg_partial,
                  (const FoldSeg*)h->fold_dev, (int)h->fold_host.size(), h->gacc);
    }
    // L2 regulariser gradient: reg_loss is part of every micro-step's loss (:366-371)
    if (h->n_reg > 0) {
        ProfScope ps(h, main_s, KID_ADAM, 0.0, 12.0 * h->n_train);
        DR_LAUNCH(reg_grad_kernel, dim3(64, std::min(h->n_reg, 256)), dim3(256), 0, main_s, (const float*)h->flat_param, h->gacc,
                  (const RegSeg*)h->reg_segs, h->n_reg, (float)h->groups);
    }
    DR_CHECK_LAUNCH(h);
    return DR_OK;
}

// Adam's bias-corrected step size (beta1 = 0.5, beta2 = 0.999) as dr_apply_adam hands it to adam_kernel; dr_step_report describes
// that step and must use the same bits
float adam_lr_t(float lr, int64_t step) {
    const double b1 = 0.5, b2 = 0.999;
    return (float)((double)lr * std::sqrt(1.0 - std::pow(b2, (double)step)) / (1.0 - std::pow(b1, (double)step)));
}

}  // namespace

extern "C" {

int dr_forward_train(dr_handle* h, int B, const float* dm, int dropout_mode, const uint8_t* keep_mask, uint64_t seed,
                     dr_stream stream) {
    if (!h || !dm) return DR_E_INVALID;
    if (dropout_mode < DR_DROPOUT_OFF || dropout_mode > DR_DROPOUT_RNG) DR_FAIL(h, DR_E_INVALID, "dropout_mode %d", dropout_mode);
    if (dropout_mode == DR_DROPOUT_MASK && !keep_mask) DR_FAIL(h, DR_E_INVALID, "DR_DROPOUT_MASK needs keep_mask_dev");
    // (a rejected call leaves the handle as it was, include/densereg.h: the backward of the forward before it still reads these)
    const int prev_mode = h->dropout_mode; const uint8_t* prev_mask = h->keep_mask; const uint64_t prev_seed = h->seed;
    auto rejected = [&](int rc) { h->dropout_mode = prev_mode; h->keep_mask = prev_mask; h->seed = prev_seed; return rc; };
    h->dropout_mode = dropout_mode; h->keep_mask = keep_mask; h->seed = seed;
    hipStream_t s = (hipStream_t)stream;
    if (h->pipe_depth < 2) { const int rc = forward_train_impl(h, B, dm, s); return rc == DR_OK ? rc : rejected(rc); }
    // two micro-steps in flight (pipeline.inc): this one takes the other slot and that slot's stream
    DR_ENTER(h);
    if (B < 1 || B > h->cfg.max_batch) {                       // before any state moves
        rejected(DR_E_INVALID);
        DR_FAIL(h, DR_E_INVALID, "batch %d outside [1, max_batch=%d]", B, h->cfg.max_batch);
    }
    const int prev_cur = h->cur_slot, prev_next = h->next_slot;
    bind_slot(h, h->next_slot);
    h->next_slot ^= 1;
    StepSlot& sl = h->slot[h->cur_slot];
    StepSlot& other = h->slot[h->cur_slot ^ 1];
    // The caller's crops are COPIED, in the caller's stream order (include/densereg.h: "inputs are copied at enqueue time"): the
    // buffer may be recycled right after this call, and this micro-step's backward still reads it (stem weight gradient).  The
    // slot's previous micro-step may still be reading its copy: the caller's stream waits for it first (the slot's stream would
    // anyway: it runs the micro-steps of a slot in order).
    // (BOTH events: step_recorded stays set once a backward has run on the slot, and a later forward of this slot that was not
    // followed by a backward -- forward + loss only, a failed step -- is only covered by fwd_done; pipeline_join does the same)
    if (sl.fwd_recorded) rt::stream_wait_event(s, sl.fwd_done);
    if (sl.step_recorded) rt::stream_wait_event(s, sl.step_done);
    rt::d2d(sl.dm_copy, dm, (size_t)B * h->cfg.in_hw * h->cfg.in_hw * sizeof(float), s);
    dm = sl.dm_copy;
    s = enter_step(h, s);
    // BatchReNorm's moving statistics chain the forwards: k+1 reads what k wrote (ops.py:134-162, "read old, then update")
    if (other.fwd_recorded) rt::stream_wait_event(s, other.fwd_done);
    static const int pipe_dbg = [] { const char* e = getenv("DR_PIPE_DEBUG"); return e ? atoi(e) : 0; }();
    if ((pipe_dbg & 1) && other.step_recorded) rt::stream_wait_event(s, other.step_done);      // debug: no overlap at all
    if (pipe_dbg & 2) { rt::sync_stream(h->slot[0].stream); rt::sync_stream(h->slot[1].stream); }
    const int rc = forward_train_impl(h, B, dm, s);
    if (rc != DR_OK) {
        // rejected (argument / tile checks run before the first launch): the slot parity and the bound slot go back to where they
        // were, and no completion event is recorded for a forward that never ran
        bind_slot(h, prev_cur);
        h->next_slot = prev_next;
        return rejected(rc);
    }
    rt::event_record(sl.fwd_done, s);
    sl.fwd_recorded = true;
    return rc;
}

// the gradient buffers that must be cleared before every backward sweep, as one table for zero_segments_kernel
static int build_zero_table(dr_handle* h) {
    std::vector<ZeroSeg> zs;
    for (auto& t : h->tensors)
        if (t->needs_zero && t->g) zs.push_back(ZeroSeg{(long)(t->g - h->grad_arena), (long)t->H * t->W * t->cs});
    if (h->zero_dev) { rt::dfree(h->zero_dev); h->zero_dev = nullptr; }
    h->zero_nseg = (int)zs.size();
    if (!zs.empty()) {
        h->zero_dev = rt::dmalloc(zs.size() * sizeof(ZeroSeg));
        if (!h->zero_dev || rt::h2d(h->zero_dev, zs.data(), zs.size() * sizeof(ZeroSeg), nullptr)) return -1;
        rt::sync_stream(nullptr);
    }
    return 0;
}

int dr_loss(dr_handle* h, int B, const float* dm, const float* pose, const float* cfg, const float* com, float* losses,
            dr_stream stream) {
    if (!h || !dm || !pose || !cfg || !com) return DR_E_INVALID;
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    if (!h->last_forward_train || B != h->last_B) DR_FAIL(h, DR_E_STATE, "dr_loss needs dr_forward_train with the same B first");
    if (h->cfg.num_stack > kMaxStack) DR_FAIL(h, DR_E_UNSUPPORTED, "more than %d stacks", kMaxStack);
    DR_ENTER(h);
    if (h->pipe_depth == 2) {          // the slot's own copies of poses | camera parameters | centres of mass, made in the CALLER's stream
                                       // order (the caller may recycle its buffers after this call); a loss pass of this slot that
                                       // may still be reading the copies comes first
        StepSlot& sl = h->slot[h->cur_slot];
        hipStream_t cs = (hipStream_t)stream;
        if (sl.loss_recorded) rt::stream_wait_event(cs, sl.loss_done);
        const size_t J3 = 3 * (size_t)h->cfg.num_jnt, nb = (size_t)B;
        float* a = sl.aux_copy;
        rt::d2d(a, pose, nb * J3 * sizeof(float), cs);
        rt::d2d(a + nb * J3, cfg, nb * 6 * sizeof(float), cs);
        rt::d2d(a + nb * (J3 + 6), com, nb * 3 * sizeof(float), cs);
        pose = a; cfg = a + nb * J3; com = a + nb * (J3 + 6);
    }
    hipStream_t s = enter_step(h, (hipStream_t)stream);
    if (h->zero_nseg < 0 && build_zero_table(h)) DR_FAIL(h, DR_E_NOMEM, "gradient clear table");
    if (h->zero_nseg > 0) {              // only the buffers whose first gradient writer is partial / atomic
        DR_LAUNCH(zero_segments_kernel, dim3(64, h->zero_nseg), dim3(256), 0, s, h->grad_arena, (const ZeroSeg*)h->zero_dev, B);
    }
    LossParams lp{};
    lp.S = h->cfg.num_stack; lp.B = B; lp.h = h->map_hw; lp.w = h->map_hw; lp.J = h->cfg.num_jnt;
    stack_maps(h, lp.pred, &lp.seed);
    lp.tiny = h->tiny; lp.pose = pose; lp.cfg = cfg; lp.com = com; lp.acc = h->loss_acc;
    {
        ProfScope ps(h, s, KID_LOSS, 0.0, 4.0 * B * lp.h * lp.w * lp.S * 10.0 * lp.J);
        // one thread per (pixel, joint); a micro-batch group owns whole blocks (its pixel count is a multiple of 256: checked by
        // dr_forward_train)
        const int n_loss = (int)(((long)B * lp.h * lp.w * lp.J + 255) / 256);
        if ((size_t)n_loss > h->n_loss_part) DR_FAIL(h, DR_E_STATE, "loss partial rows");
        if (h->groups > 1 && n_loss % h->groups) DR_FAIL(h, DR_E_UNSUPPORTED, "micro-batch groups: %d loss blocks for %d groups", n_loss, h->groups);
        double* reg_part = h->loss_acc + 3 * h->n_loss_part;
        DR_LAUNCH(loss_kernel, dim3(n_loss), dim3(256), 0, s, lp);
        if (h->n_reg > 0)
            DR_LAUNCH(reg_loss_kernel, dim3(h->n_reg, kRegRows), dim3(256), 0, s, (const float*)h->flat_param,
                      (const RegSeg*)h->reg_segs, reg_part);
        if (losses)
            DR_LAUNCH(losses_out_kernel, dim3(h->groups), dim3(256), 0, s, (const double*)h->loss_acc, n_loss, (const double*)reg_part,
                      h->n_reg > 0 ? kRegRows * h->n_reg : 0, losses);
    }
    if (h->pipe_depth == 2 && s != (hipStream_t)stream) {
        // the loss terms land in the caller's buffer: the caller's stream sees them in its own order
        StepSlot& sl = h->slot[h->cur_slot];
        rt::event_record(sl.loss_done, s);
        sl.loss_recorded = true;
        if (losses) rt::stream_wait_event((hipStream_t)stream, sl.loss_done);
    }
    DR_CHECK_LAUNCH(h);
    return DR_OK;
}

int dr_backward(dr_handle* h, int B, dr_stream stream) {
    if (!h) return DR_E_INVALID;
    if (h->pipe_depth < 2) return backward_impl(h, B, (hipStream_t)stream);
    hipStream_t s = enter_step(h, (hipStream_t)stream);
    const int rc = backward_impl(h, B, s);
    StepSlot& sl = h->slot[h->cur_slot];
    rt::event_record(sl.step_done, s);
    sl.step_recorded = true;
    if (h->cur_slot == 1) sl.grads_dirty = true;
    return rc;
}

int dr_zero_grad(dr_handle* h, dr_stream stream) {
    if (!h) return DR_E_INVALID;
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    DR_ENTER(h);
    pipeline_join(h, (hipStream_t)stream);                  // no backward still adding to what is cleared here
    rt::memset_async(h->flat_grad, 0, h->n_train * sizeof(float), (hipStream_t)stream);
    if (h->pipe_depth == 2) {
        rt::memset_async(h->slot[1].gacc, 0, h->n_train * sizeof(float), (hipStream_t)stream);
        h->slot[1].grads_dirty = false;
    }
    return DR_OK;
}

// Training handles: how many micro-steps may be in flight (1 = every call runs on the caller's stream, the default; 2 = pipeline.inc).
int dr_set_pipeline(dr_handle* h, int depth) {
    if (!h) return DR_E_INVALID;
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "dr_set_pipeline: handle was created with training=0");
    if (depth != 1 && depth != 2) DR_FAIL(h, DR_E_INVALID, "dr_set_pipeline: depth %d (1 or 2)", depth);
    if (depth == 2 && h->multi_stream) DR_FAIL(h, DR_E_UNSUPPORTED, "dr_set_pipeline: not together with the executor lanes (DR_MULTI_STREAM=1)");
    DR_ENTER(h);
    if (depth == h->pipe_depth) return DR_OK;
    if (depth == 2) {
        if (!h->slot[1].owns && alloc_slot1(h)) { free_slot1(h); DR_FAIL(h, DR_E_NOMEM, "dr_set_pipeline: no device memory for a second micro-step slot"); }
        const size_t MB = (size_t)h->cfg.max_batch;
        for (int i = 0; i < 2; ++i) {
            StepSlot& s = h->slot[i];
            // Normal priority, like the caller's stream.  Measured (DR_PIPE_PRIO: 1 = both slots on highest-priority streams, 2 = only
            // slot 1): 1465 and 1256 crops/s against 2245 -- queues of different priority are not run side by side but one after
            // the other, and the low-priority weight-gradient streams starve.  The runtime multiplexes the streams of one priority
            // level onto GPU_MAX_HW_QUEUES (4) hardware queues, least used first: the two slots get queues of their own as long as
            // the process has created at most two other normal-priority streams before them (the handle creates none).
            static const int prio = [] { const char* e = getenv("DR_PIPE_PRIO"); return e ? atoi(e) : 0; }();
            s.stream = (prio == 1 || (prio == 2 && i == 1)) ? rt::stream_create_high_priority() : rt::stream_create();
            s.in_ev = rt::event_create_sync(); s.fwd_done = rt::event_create_sync();
            s.loss_done = rt::event_create_sync(); s.step_done = rt::event_create_sync();
            s.events_live = true;
            s.fwd_recorded = s.step_recorded = s.loss_recorded = false;
            s.dm_copy = (float*)rt::dmalloc(MB * h->cfg.in_hw * h->cfg.in_hw * sizeof(float));
            s.aux_copy = (float*)rt::dmalloc(MB * (3 * (size_t)h->cfg.num_jnt + 9) * sizeof(float));
            if (!s.dm_copy || !s.aux_copy) {
                release_slot_streams(h);                        // both slots' streams / events / copies created so far; depth stays 1
                DR_FAIL(h, DR_E_NOMEM, "dr_set_pipeline: input copies");
            }
        }
        rt::sync_stream(nullptr);
        h->pipe_depth = 2;
        h->next_slot = h->cur_slot ^ 1;                       // the slot bound now may hold a forward somebody still reads
        return DR_OK;
    }
    // back to one slot: finish what is in flight, fold slot 1's gradients into the flat accumulator, keep working on slot 0
    if (pipeline_drain(h)) DR_FAIL(h, DR_E_DEVICE, "dr_set_pipeline: a micro-step slot's stream did not drain");
    int rc = dr_sync_grads(h, nullptr);
    if (rc) return rc;
    rt::sync_stream(nullptr);
    release_slot_streams(h);                                  // (resets the handles: dr_destroy must not release them again)
    h->pipe_depth = 1;
    bind_slot(h, 0);
    h->next_slot = 0;
    h->last_forward_train = false;                            // the activations of the last forward may live in slot 1
    return DR_OK;
}

// The next dr_forward_train / dr_loss / dr_backward treat their B crops as `groups` consecutive micro-batches of B / groups crops:
// the reference's accumulation micro-steps (train_single_gpu.py:138-150) as one pass of launches (see include/densereg.h).
int dr_set_groups(dr_handle* h, int groups) {
    if (!h) return DR_E_INVALID;
    static_assert(kMaxGroups == 8, "include/densereg.h documents 8");
    if (h->n_bnc != 2 * h->n_fold) DR_FAIL(h, DR_E_STATE, "dr_set_groups: coefficient layouts out of step");   // conv_epilogue.inc, ep_goff
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "dr_set_groups: handle was created with training=0");
    if (groups < 1 || groups > kMaxGroups) DR_FAIL(h, DR_E_INVALID, "dr_set_groups: %d groups (1..%d)", groups, kMaxGroups);
    if (groups > 1 && h->bn_lookback) DR_FAIL(h, DR_E_UNSUPPORTED, "dr_set_groups: not with DR_BN_LOOKBACK");
    DR_ENTER(h);
    if (groups != h->groups) h->last_forward_train = false;  // a forward of the other shape cannot be continued
    h->groups = groups;
    return DR_OK;
}

// `stream` waits for every micro-step in flight; afterwards the buffer dr_flat_grad names holds the SUM of all slots' accumulated
// gradients (slot 0's + slot 1's, one addition per element) -- what an all-reduce or a reader of the flat gradient wants.
int dr_sync_grads(dr_handle* h, dr_stream stream) {
    if (!h) return DR_E_INVALID;
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    if (h->pipe_depth < 2) return DR_OK;
    DR_ENTER(h);
    hipStream_t s = (hipStream_t)stream;
    pipeline_join(h, s);
    if (h->slot[1].grads_dirty) {
        DR_LAUNCH(grad_merge_kernel, dim3(grid_for((long)h->n_train)), dim3(256), 0, s, h->flat_grad, h->slot[1].gacc, (long)h->n_train);
        h->slot[1].grads_dirty = false;
    }
    DR_CHECK_LAUNCH(h);
    return DR_OK;
}

int dr_flat_grad(dr_handle* h, float** p, size_t* n) {
    if (!h || !p || !n) return DR_E_INVALID;
    if (!h->flat_grad) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    *p = h->flat_grad; *n = h->n_train;
    return DR_OK;
}

int dr_flat_param(dr_handle* h, float** p, size_t* n) {
    if (!h || !p || !n) return DR_E_INVALID;
    *p = h->flat_param; *n = h->n_train;
    return DR_OK;
}

int dr_flat_adam(dr_handle* h, float** m, float** v, size_t* n) {
    if (!h || !m || !v || !n) return DR_E_INVALID;
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    *m = h->adam_m; *v = h->adam_v; *n = h->n_train;
    return DR_OK;
}

int dr_apply_adam(dr_handle* h, float lr, float div, float clip, int64_t step, dr_stream stream) {
    if (!h) return DR_E_INVALID;
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "handle was created with training=0");
    if (step < 1 || !(div > 0.f)) DR_FAIL(h, DR_E_INVALID, "dr_apply_adam: step must be >= 1 and div > 0");
    DR_ENTER(h);
    hipStream_t s = (hipStream_t)stream;
    {   // every micro-step in flight has finished, and the slots' gradients are one sum, before the update reads them
        const int rc = dr_sync_grads(h, stream);
        if (rc) return rc;
    }
    const float lr_t = adam_lr_t(lr, step);
    {
        ProfScope ps(h, s, KID_ADAM, 0.0, 28.0 * h->n_train);
        DR_LAUNCH(adam_kernel, dim3(grid_for((long)h->n_train)), dim3(256), 0, s, h->flat_param, (const float*)h->flat_grad, h->adam_m,
                  h->adam_v, (long)h->n_train, div, clip, lr_t, 0.5f, 0.999f, 1e-8f);
    }
    DR_CHECK_LAUNCH(h);
    return repack_weights(h, s);
}

// The step dr_apply_adam(h, lr, div, clip, step, stream) would take now, described and not taken (step_report.h).  Reads both
// slots' accumulators where dr_apply_adam would first merge them; writes nothing the handle owns but the report's workspace.
int dr_step_report(dr_handle* h, float lr, float div, float clip, int64_t step, const struct dr_step_report* report, dr_stream stream) {
    if (!h) return DR_E_INVALID;
    if (!h->cfg.training) DR_FAIL(h, DR_E_STATE, "dr_step_report: handle was created with training=0");
    if (!report) DR_FAIL(h, DR_E_INVALID, "dr_step_report: report is NULL");
    const struct dr_step_report& r = *report;
    const bool want_global = r.global_dev || r.global_counts_dev;
    if (!r.param_stats_dev && !r.grad_stats_dev && !r.raw_stats_dev && !r.update_stats_dev && !r.grad_counts_dev && !want_global &&
        !r.grad_hist_dev && !r.param_hist_dev)
        DR_FAIL(h, DR_E_INVALID, "dr_step_report: every output member of the report is NULL");
    if (step < 1 || !(div > 0.f) || !(clip > 0.f)) DR_FAIL(h, DR_E_INVALID, "dr_step_report: step must be >= 1, div > 0 and clip > 0");
    if (r.num_edges < 0 || r.num_edges > kStepMaxEdges) DR_FAIL(h, DR_E_INVALID, "dr_step_report: num_edges %d outside [0, %d]", r.num_edges, kStepMaxEdges);
    if ((r.grad_hist_dev || r.param_hist_dev) && r.num_edges == 0) DR_FAIL(h, DR_E_INVALID, "dr_step_report: a histogram needs num_edges > 0");
    if (r.num_edges > 0 && !r.hist_edges_dev) DR_FAIL(h, DR_E_INVALID, "dr_step_report: num_edges > 0 but hist_edges_dev is NULL");
    DR_ENTER(h);
    hipStream_t s = (hipStream_t)stream;
    if (!h->step_report_ws) {                                  // the chunk table: once per handle (the flat layout never changes)
        std::vector<StepChunk> chunks;
        std::vector<StepVar> vars;
        long off = 0;
        for (auto& p : h->params) {
            if (!p.trainable) continue;
            StepVar v{(long)p.count, (int)chunks.size(), 0};
            for (long b = 0; b < (long)p.count; b += kStepChunk)
                chunks.push_back(StepChunk{off + b, off + std::min<long>(b + kStepChunk, (long)p.count), (int)vars.size(), 0});
            v.nchunk = (int)chunks.size() - v.first_chunk;
            vars.push_back(v);
            off += (long)p.count;
        }
        if (off != (long)h->n_train) DR_FAIL(h, DR_E_STATE, "dr_step_report: the variables do not add up to the flat buffer");
        const size_t nb_ck = chunks.size() * sizeof(StepChunk), nb_var = vars.size() * sizeof(StepVar);
        char* ws = (char*)rt::dmalloc(nb_ck + nb_var + chunks.size() * sizeof(StepPart));
        if (!ws) DR_FAIL(h, DR_E_NOMEM, "dr_step_report: no device memory for the workspace");
        if (rt::h2d(ws, chunks.data(), nb_ck, s) || rt::h2d(ws + nb_ck, vars.data(), nb_var, s)) {
            rt::sync_stream(s);
            rt::dfree(ws);
            DR_FAIL(h, DR_E_DEVICE, "dr_step_report: h2d of the chunk table failed");
        }
        rt::sync_stream(s);                                    // the tables are host memory that goes away; only on the first call
        h->step_report_ws = ws; h->step_nchunk = (int)chunks.size(); h->step_nvar = (int)vars.size();
    }
    static_assert(sizeof(StepChunk) % 8 == 0 && sizeof(StepVar) % 8 == 0 && sizeof(StepPart) % 8 == 0, "the workspace parts stay 8-byte aligned");
    const int nck = h->step_nchunk, V = h->step_nvar, E = r.num_edges;
    char* ws = (char*)h->step_report_ws;
    const StepChunk* chunks = (const StepChunk*)ws;
    const StepVar* vars = (const StepVar*)(ws + nck * sizeof(StepChunk));
    StepPart* part = (StepPart*)(ws + nck * sizeof(StepChunk) + V * sizeof(StepVar));

    pipeline_join(h, s);                                       // as dr_sync_grads: behind every micro-step in flight
    StepReportParams sp{};
    sp.grad = h->flat_grad;
    sp.grad2 = (h->pipe_depth == 2 && h->slot[1].grads_dirty) ? h->slot[1].gacc : nullptr;   // read, neither folded nor cleared
    sp.param = h->flat_param; sp.m = h->adam_m; sp.v = h->adam_v;
    sp.chunks = chunks; sp.part = part;
    sp.edges = r.hist_edges_dev; sp.E = E; sp.grad_hist = r.grad_hist_dev; sp.param_hist = r.param_hist_dev;
    sp.div = div; sp.clip = clip; sp.lr_t = adam_lr_t(lr, step); sp.b1 = 0.5f; sp.b2 = 0.999f; sp.eps = 1e-8f;
    // which of theta / acc / (m, v) are read at all: members that are NULL cost no loads
    const int need_param = (r.param_stats_dev || r.param_hist_dev || r.global_dev) ? 1 : 0;
    const int need_upd = (r.update_stats_dev || r.global_dev) ? 1 : 0;
    const int need_grad = (r.grad_stats_dev || r.raw_stats_dev || r.grad_counts_dev || r.grad_hist_dev || want_global || need_upd) ? 1 : 0;
    const int mode = need_param * kStepParam + need_grad * kStepGrad + need_upd * kStepUpd + ((r.grad_hist_dev || r.param_hist_dev) ? kStepHist : 0);
    const size_t hist_bytes = (size_t)V * (E + 1) * sizeof(int32_t);
    const size_t smem = (r.grad_hist_dev || r.param_hist_dev)
                            ? (size_t)E * sizeof(float) + (size_t)(E + 1) * sizeof(int) * ((r.grad_hist_dev ? 1 : 0) + (r.param_hist_dev ? 1 : 0)) : 0;
    ProfScope ps(h, s, KID_STEP_REPORT, 0.0,
                 4.0 * h->n_train * (need_param + need_grad * (sp.grad2 ? 2 : 1) + 2 * need_upd));
    if (r.grad_hist_dev) rt::memset_async(r.grad_hist_dev, 0, hist_bytes, s);      // the chunks ADD their bucket counts
    if (r.param_hist_dev) rt::memset_async(r.param_hist_dev, 0, hist_bytes, s);
    switch (mode) {                                            // (an update needs the gradient: six of these never occur)
#define DR_STEP_MODE(M) case M: DR_LAUNCH(step_report_kernel<M>, dim3(nck), dim3(256), smem, s, sp); break;
        DR_STEP_MODE(1) DR_STEP_MODE(2) DR_STEP_MODE(3) DR_STEP_MODE(6) DR_STEP_MODE(7)
        DR_STEP_MODE(9) DR_STEP_MODE(10) DR_STEP_MODE(11) DR_STEP_MODE(14) DR_STEP_MODE(15)
#undef DR_STEP_MODE
        default: DR_FAIL(h, DR_E_STATE, "dr_step_report: no kernel for member mode %d", mode);
    }
    StepFoldOut fo{r.param_stats_dev, r.grad_stats_dev, r.raw_stats_dev, r.update_stats_dev, r.grad_counts_dev, r.global_dev, r.global_counts_dev};
    const int n_var_blocks = (fo.param_stats || fo.grad_stats || fo.raw_stats || fo.update_stats || fo.grad_counts) ? V : 0;
    if (n_var_blocks + (want_global ? 1 : 0) > 0)
        DR_LAUNCH(step_report_fold_kernel, dim3(n_var_blocks + (want_global ? 1 : 0)), dim3(256), 0, s, (const StepPart*)part, vars, n_var_blocks, nck, fo);
    DR_CHECK_LAUNCH(h);
    return DR_OK;
}

}  // extern "C"
