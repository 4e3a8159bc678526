// step_report.h -- the training-step report (dr_step_report): per trainable variable, statistics of the weights, of the averaged
// and clipped gradient, and of the decrement the NEXT dr_apply_adam would apply -- what the reference histograms per variable
// (model/train_single_gpu.py:91-95) -- plus the counts that make a diverging or dead layer visible before the step is taken.
//
//   step_report_kernel         one workgroup per chunk of ONE variable: per-chunk fp64 sums, fp32 min / max, int counts; histogram
//                              buckets counted in LDS and added to the (V,E+1) outputs with integer atomics
//   step_report_fold_kernel    one workgroup per variable: its chunks folded in a fixed order into the per-variable members; one
//                              more workgroup: all chunks folded in a fixed order into the global members
//
// Read-only: nothing the handle owns is written but the report's workspace.  The per-element arithmetic is adam_elem
// (train_kernels.h), the function adam_kernel applies, and, where the second micro-step slot holds gradients, grad_merge_kernel's
// one addition in front of it (tests/test_step_report.py holds it to the step dr_apply_adam takes, bit for bit).  No floating-point atomics:
// every sum is fp64 in an order fixed by the chunk table alone.
#pragma once
#include "train_kernels.h"

namespace dr {

constexpr int kStepChunk = 4096;          // elements per chunk (a multiple of 4: every chunk of a variable has the same misalignment)
constexpr int kStepMaxEdges = 2048;
constexpr int kStepRow = 264;             // LDS row of the workgroup reduction: 256 threads + padding against bank conflicts

struct StepChunk { long begin, end; int var, pad; };           // [begin, end) of the flat buffers; no chunk straddles a variable
struct StepVar { long n; int first_chunk, nchunk; };
// s: sum theta, theta^2, g, g^2, a^2 (finite a), u, u^2;  mm: min / max theta, min / max g, max |a| (finite a), min / max u;
// cnt: non-finite acc, clipped, acc == 0
struct StepPart { double s[7]; float mm[7]; int cnt[3]; };

struct StepReportParams {
    const float* grad; const float* grad2;                      // grad2: the second slot's accumulator when it is dirty, else NULL
    const float* param; const float* m; const float* v;
    const StepChunk* chunks; StepPart* part;
    const float* edges; int E;
    int* grad_hist; int* param_hist;                            // (V,E+1), zeroed before the launch; NULL = not wanted
    float div, clip, lr_t, b1, b2, eps;
};

struct StepAcc {
    double s[7]; float mm[7]; int cnt[3];
};

__device__ __forceinline__ bool step_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN and +-Inf

// numpy's searchsorted(edges, x, side='right'): the number of edges <= x; NaN sorts behind everything
__device__ __forceinline__ int step_bucket(const float* edges, int E, float x) {
    if (x != x) return E;
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// What a launch needs, as a template argument: without it every element would carry the branches around what it does not need,
// and the four elements of a 16-byte group could not be scheduled together.
enum { kStepParam = 1, kStepGrad = 2, kStepUpd = 4, kStepHist = 8 };

// One element.  Everything from `a` to `u` comes from adam_elem.
template <int MODE>
__device__ __forceinline__ void step_elem(const StepReportParams& p, StepAcc& A, float th, float acc, float mi0, float vi0,
                                          const float* edges, int* hg, int* hp) {
#pragma clang fp contract(off)
    if constexpr ((MODE & kStepParam) != 0) {
        A.s[0] += (double)th;
        A.s[1] += (double)th * (double)th;
        A.mm[0] = fminf(A.mm[0], th);
        A.mm[1] = fmaxf(A.mm[1], th);
        if constexpr ((MODE & kStepHist) != 0) { if (hp) atomicAdd(&hp[step_bucket(edges, p.E, th)], 1); }
    }
    if constexpr ((MODE & kStepGrad) != 0) {
        const AdamElem e = adam_elem(acc, mi0, vi0, p.div, p.clip, p.lr_t, p.b1, p.b2, p.eps);
        const float a = e.a, g = e.g;
        A.s[2] += (double)g;
        A.s[3] += (double)g * (double)g;
        A.mm[2] = fminf(A.mm[2], g);
        A.mm[3] = fmaxf(A.mm[3], g);
        if (step_finite(a)) {
            A.s[4] += (double)a * (double)a;
            A.mm[4] = fmaxf(A.mm[4], fabsf(a));
            A.cnt[1] += fabsf(a) > p.clip ? 1 : 0;
        }
        A.cnt[0] += step_finite(acc) ? 0 : 1;
        A.cnt[2] += acc == 0.f ? 1 : 0;
        if constexpr ((MODE & kStepHist) != 0) { if (hg) atomicAdd(&hg[step_bucket(edges, p.E, g)], 1); }
        if constexpr ((MODE & kStepUpd) != 0) {
            A.s[5] += (double)e.u;
            A.s[6] += (double)e.u * (double)e.u;
            A.mm[5] = fminf(A.mm[5], e.u);
            A.mm[6] = fmaxf(A.mm[6], e.u);
        }
    }
}

// Grid: one workgroup per chunk.  Thread t takes the scalar head element t (up to the first 16-byte boundary of the flat buffers),
// the 16-byte groups t, t + 256, ... of the body and the scalar tail element t: an order that depends on the chunk table alone.
// Dynamic LDS: the edges and one (E+1)-entry table per wanted histogram; none without histograms.
template <int MODE>
__global__ __launch_bounds__(256) void step_report_kernel(const StepReportParams p) {
#pragma clang fp contract(off)
    constexpr bool P = (MODE & kStepParam) != 0, G = (MODE & kStepGrad) != 0, U = (MODE & kStepUpd) != 0, H = (MODE & kStepHist) != 0;
    DR_DYN_SMEM(dyn);
    __shared__ double red[7 * kStepRow];
    __shared__ float fred[7 * kStepRow];
    __shared__ int ired[3 * kStepRow];
    __shared__ double red_b[7 * 8];
    __shared__ float fred_b[7 * 8];
    __shared__ int ired_b[3 * 8];
    const int t = threadIdx.x;
    const StepChunk ck = p.chunks[blockIdx.x];
    const int nb = p.E + 1;
    float* edges = nullptr; int* hg = nullptr; int* hp = nullptr;
    if constexpr (H) {
        edges = reinterpret_cast<float*>(dyn);
        int* tab = reinterpret_cast<int*>(edges + p.E);
        if (p.grad_hist) { hg = tab; tab += nb; }
        if (p.param_hist) hp = tab;
        for (int i = t; i < p.E; i += 256) edges[i] = p.edges[i];
        for (int i = t; i < nb; i += 256) { if (hg) hg[i] = 0; if (hp) hp[i] = 0; }
        __syncthreads();
    }
    const float qnan = __builtin_nanf("");
    StepAcc A;
    for (int q = 0; q < 7; ++q) { A.s[q] = 0.0; A.mm[q] = qnan; }   // fminf / fmaxf drop the NaN at the first number
    A.mm[4] = 0.f;                                               // max |a| over the finite a: 0 if there is none
    A.cnt[0] = A.cnt[1] = A.cnt[2] = 0;

    auto one = [&](long i) {
        float acc = 0.f, th = 0.f, mi = 0.f, vi = 0.f;
        if constexpr (G) { acc = p.grad[i]; if (p.grad2) acc = acc + p.grad2[i]; }
        if constexpr (P) th = p.param[i];
        if constexpr (U) { mi = p.m[i]; vi = p.v[i]; }
        step_elem<MODE>(p, A, th, acc, mi, vi, edges, hg, hp);
    };
    long a0 = (ck.begin + 3) & ~3L;
    if (a0 > ck.end) a0 = ck.end;
    const long nvec = (ck.end - a0) >> 2, a1 = a0 + 4 * nvec;
    if (ck.begin + t < a0) one(ck.begin + t);
    for (long k = t; k < nvec; k += 256) {
        const long i = a0 + 4 * k;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), th = acc, mi = acc, vi = acc;
        if constexpr (G) {
            acc = *reinterpret_cast<const float4*>(p.grad + i);
            if (p.grad2) {
                const float4 b = *reinterpret_cast<const float4*>(p.grad2 + i);
                acc.x = acc.x + b.x; acc.y = acc.y + b.y; acc.z = acc.z + b.z; acc.w = acc.w + b.w;
            }
        }
        if constexpr (P) th = *reinterpret_cast<const float4*>(p.param + i);
        if constexpr (U) { mi = *reinterpret_cast<const float4*>(p.m + i); vi = *reinterpret_cast<const float4*>(p.v + i); }
        step_elem<MODE>(p, A, th.x, acc.x, mi.x, vi.x, edges, hg, hp);
        step_elem<MODE>(p, A, th.y, acc.y, mi.y, vi.y, edges, hg, hp);
        step_elem<MODE>(p, A, th.z, acc.z, mi.z, vi.z, edges, hg, hp);
        step_elem<MODE>(p, A, th.w, acc.w, mi.w, vi.w, edges, hg, hp);
    }
    if (a1 + t < ck.end) one(a1 + t);

    // workgroup reduction through LDS in a fixed order, two barriers: 8 threads per quantity add (or min / max) every 8th of the 256
    // entries, one thread per quantity the 8 results; the sums on wave 0, the min / max on wave 1, the counts on wave 2
    StepPart* out = p.part + blockIdx.x;
    for (int q = 0; q < 7; ++q) { red[q * kStepRow + t] = A.s[q]; fred[q * kStepRow + t] = A.mm[q]; }
    for (int q = 0; q < 3; ++q) ired[q * kStepRow + t] = A.cnt[q];
    __syncthreads();
    const int w = t >> 6, l = t & 63, q8 = l >> 3, r8 = l & 7;
    if (w == 0 && l < 56) {
        double a = 0.0;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) a += red[q8 * kStepRow + r8 + 8 * k];
        red_b[l] = a;
    } else if (w == 1 && l < 56) {
        const bool is_min = q8 == 0 || q8 == 2 || q8 == 5;
        float a = fred[q8 * kStepRow + r8];
#pragma unroll 8
        for (int k = 1; k < 32; ++k) {
            const float b = fred[q8 * kStepRow + r8 + 8 * k];
            a = is_min ? fminf(a, b) : fmaxf(a, b);
        }
        fred_b[l] = a;
    } else if (w == 2 && l < 24) {
        int a = 0;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) a += ired[q8 * kStepRow + r8 + 8 * k];
        ired_b[l] = a;
    }
    __syncthreads();
    if (w == 0 && l < 7) {
        double a = 0.0;
        for (int r = 0; r < 8; ++r) a += red_b[l * 8 + r];
        out->s[l] = a;
    } else if (w == 1 && l < 7) {
        const bool is_min = l == 0 || l == 2 || l == 5;
        float a = fred_b[l * 8];
        for (int r = 1; r < 8; ++r) a = is_min ? fminf(a, fred_b[l * 8 + r]) : fmaxf(a, fred_b[l * 8 + r]);
        out->mm[l] = a;
    } else if (w == 2 && l < 3) {
        int a = 0;
        for (int r = 0; r < 8; ++r) a += ired_b[l * 8 + r];
        out->cnt[l] = a;
    }
    // the histograms of this chunk: integer adds, so the result does not depend on the order the chunks arrive in
    if constexpr (H) {
        for (int i = t; i < nb; i += 256) {
            if (hg) { const int c = hg[i]; if (c) atomicAdd(&p.grad_hist[(long)ck.var * nb + i], c); }
            if (hp) { const int c = hp[i]; if (c) atomicAdd(&p.param_hist[(long)ck.var * nb + i], c); }
        }
    }
}

struct StepFoldOut {
    float* param_stats; float* grad_stats; float* raw_stats; float* update_stats; int* grad_counts;   // per variable; any may be NULL
    float* global_out; int* counts_out;                          // (6) and (3); either may be NULL
};

// The second launch.  Workgroups [0, n_var_blocks): one variable each, on the first wave -- lane l takes the variable's chunks l,
// l + 64, ... in that order, a butterfly of wave shuffles (a fixed tree) leaves the totals in every lane; a variable of one chunk
// -- most of them -- is read by every lane and needs no tree.  The workgroup behind them (present when a global member is wanted)
// folds ALL chunks the same way on four waves, one thread per quantity then adds the waves' results in wave order:
// global_out = ||g||2, ||a||2, ||theta||2, ||u||2 as fp32 casts of the square roots of the fp64 totals, max |g|, max |u|;
// counts_out = non-finite, clipped, zero.
__global__ __launch_bounds__(256) void step_report_fold_kernel(const StepPart* part, const StepVar* vars, int n_var_blocks, int nchunk_all,
                                                               const StepFoldOut o) {
    __shared__ double ds[4][4];
    __shared__ float fs[4][2];
    __shared__ int is[4][3];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const bool global_block = (int)blockIdx.x >= n_var_blocks;
    if (!global_block && w > 0) return;                           // (no barrier on the variables' path)
    const int var = blockIdx.x;
    StepVar vr{0, 0, nchunk_all};
    if (!global_block) vr = vars[var];
    const StepPart* src = part + vr.first_chunk;
    const float qnan = __builtin_nanf("");
    double S[7]; float M[7]; int Cn[3];
    for (int q = 0; q < 7; ++q) { S[q] = 0.0; M[q] = qnan; }
    M[4] = 0.f;
    Cn[0] = Cn[1] = Cn[2] = 0;
    const bool one = !global_block && vr.nchunk == 1;
    const int stride = global_block ? 256 : 64;
    for (int c = one ? 0 : t; c < vr.nchunk; c += stride) {
        const StepPart pt = src[c];
        for (int q = 0; q < 7; ++q) S[q] += pt.s[q];
        M[0] = fminf(M[0], pt.mm[0]); M[1] = fmaxf(M[1], pt.mm[1]); M[2] = fminf(M[2], pt.mm[2]); M[3] = fmaxf(M[3], pt.mm[3]);
        M[4] = fmaxf(M[4], pt.mm[4]); M[5] = fminf(M[5], pt.mm[5]); M[6] = fmaxf(M[6], pt.mm[6]);
        for (int q = 0; q < 3; ++q) Cn[q] += pt.cnt[q];
    }
    if (!one) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            for (int q = 0; q < 7; ++q) S[q] += __shfl_xor(S[q], m);
            M[0] = fminf(M[0], __shfl_xor(M[0], m)); M[1] = fmaxf(M[1], __shfl_xor(M[1], m));
            M[2] = fminf(M[2], __shfl_xor(M[2], m)); M[3] = fmaxf(M[3], __shfl_xor(M[3], m));
            M[4] = fmaxf(M[4], __shfl_xor(M[4], m));
            M[5] = fminf(M[5], __shfl_xor(M[5], m)); M[6] = fmaxf(M[6], __shfl_xor(M[6], m));
            for (int q = 0; q < 3; ++q) Cn[q] += __shfl_xor(Cn[q], m);
        }
    }
    if (!global_block) {
        if (t == 0 && o.param_stats) { float* d = o.param_stats + 4 * var; d[0] = M[0]; d[1] = M[1]; d[2] = (float)S[0]; d[3] = (float)S[1]; }
        if (t == 1 && o.grad_stats) { float* d = o.grad_stats + 4 * var; d[0] = M[2]; d[1] = M[3]; d[2] = (float)S[2]; d[3] = (float)S[3]; }
        if (t == 2 && o.raw_stats) { float* d = o.raw_stats + 2 * var; d[0] = M[4]; d[1] = (float)S[4]; }
        if (t == 3 && o.update_stats) { float* d = o.update_stats + 4 * var; d[0] = M[5]; d[1] = M[6]; d[2] = (float)S[5]; d[3] = (float)S[6]; }
        if (t == 4 && o.grad_counts) { int* d = o.grad_counts + 4 * var; d[0] = (int)vr.n; d[1] = Cn[0]; d[2] = Cn[1]; d[3] = Cn[2]; }
        return;
    }
    if (lane == 0) {
        ds[w][0] = S[3]; ds[w][1] = S[4]; ds[w][2] = S[1]; ds[w][3] = S[6];
        fs[w][0] = fmaxf(fabsf(M[2]), fabsf(M[3])); fs[w][1] = fmaxf(fabsf(M[5]), fabsf(M[6]));
        is[w][0] = Cn[0]; is[w][1] = Cn[1]; is[w][2] = Cn[2];
    }
    __syncthreads();
    if (t < 4 && o.global_out) o.global_out[t] = (float)sqrt(((ds[0][t] + ds[1][t]) + ds[2][t]) + ds[3][t]);
    else if (t >= 4 && t < 6 && o.global_out) o.global_out[t] = fmaxf(fmaxf(fs[0][t - 4], fs[1][t - 4]), fmaxf(fs[2][t - 4], fs[3][t - 4]));
    else if (t >= 6 && t < 9 && o.counts_out) o.counts_out[t - 6] = is[0][t - 6] + is[1][t - 6] + is[2][t - 6] + is[3][t - 6];
}

}  // namespace dr
