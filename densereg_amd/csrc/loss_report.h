// loss_report.h -- the loss-side report (dr_loss_report / dr_targets): the targets of JointDetectionModel.loss / .test
// (hourglass_um_crop_tiny.py:336-346, 474-480) as maps, and the l2 losses of :353 / :357 / :363 split by stack, joint and crop.
//
//   targets_kernel        loss_report_body<false>: the three target maps, nothing read but the crop and its labels
//   loss_report_kernel    loss_report_body<true>:  the same, plus per-workgroup fp64 partial sums of every stack's loss terms
//   loss_report_crop_kernel / loss_report_out_kernel   the partials summed in a fixed order into the report's members
//
// Read-only with respect to the handle: no gradient seed, no accumulator.  The targets are pose_math.h's (map_cam, cloud_point,
// pose_targets): the functions loss_kernel (train_kernels.h) calls, so the two cannot drift apart.
#pragma once
#include "train_kernels.h"

namespace dr {

struct LossReportParams {
    StackMaps pred;                                           // predictions of the most recent forward (sums only)
    int S, B, h, w, J, in_hw;
    const float* dm; const float* pose; const float* cfg; const float* com;   // dm: the normalised crop at input resolution
    float* gt_hm; float* gt_hm3; float* gt_um;                // (B,h,w,J) (B,h,w,J) (B,h,w,3J); any may be NULL
    double* part;                                             // [B][gridDim.x][S][J][3] (sums only)
};

// One body for both entry kernels.  Grid (chunks of 256 elements per crop, B): one thread per (pixel, joint) of ONE crop, joints
// fastest -- loss_kernel's geometry, so a wave reads and writes consecutive channels of consecutive pixels and every map element is
// touched once -- and a workgroup never straddles two crops (the per-crop sums need that).  SUMS = false is targets_kernel: no
// prediction is read, no LDS, no partials.
template <bool SUMS>
__device__ __forceinline__ void loss_report_body(const LossReportParams& p) {
#pragma clang fp contract(off)
    const int npix = p.h * p.w;
    const int b = blockIdx.y;
    const int e0 = (int)blockIdx.x * 256;                     // first element of this workgroup within its crop
    const int e = e0 + (int)threadIdx.x;
    const bool live = e < npix * p.J;
    int j = 0;
    long m = 0;
    PoseTargets gt{};
    if (live) {
        j = e % p.J;
        const int px = e / p.J;
        m = (long)b * npix + px;
        // the depth at the map's stride straight from the crop (tiny_dm = [::4, ::4]): no forward's copy of it is needed
        const int ix = px % p.w, iy = px / p.w, st = p.in_hw / p.w;
        const float t = p.dm[((long)b * p.in_hw + iy * st) * p.in_hw + ix * st];
        const MapCam cam = map_cam(p.cfg + b * 6, p.w, p.h);
        const CloudPoint cloud = cloud_point(cam, p.com + b * 3, t, px, p.w);
        gt = pose_targets(cam, p.com + b * 3, p.pose + (long)b * 3 * p.J + 3 * j, cloud, px, p.w);
        if (p.gt_hm) p.gt_hm[m * p.J + j] = gt.gt_hm;
        if (p.gt_hm3) p.gt_hm3[m * p.J + j] = gt.gt_hm3;
        if (p.gt_um) { float* q = p.gt_um + m * 3 * p.J + 3 * j; q[0] = gt.ux; q[1] = gt.uy; q[2] = gt.uz; }
    }
    if constexpr (SUMS) {
        // Deterministic fp64 sums without atomics: stack by stack (a per-thread array over the stacks would live in scratch), the
        // threads park their three terms in LDS, and one thread per (joint, term) adds its joint's threads in index order.  Every
        // row of the partials is written, the joints a chunk does not reach with 0.
        __shared__ double term[3][256];
        const int rest = npix * p.J - e0;
        const int nlive = rest < 256 ? rest : 256;
        const int j0 = e0 % p.J;                              // joint of thread 0
        double* part = p.part + ((long)b * gridDim.x + blockIdx.x) * p.S * p.J * 3;
        for (int s = 0; s < p.S; ++s) {
            if (live) {
                const float e1 = p.pred.hm[s].p[m * p.pred.hm[s].cs + p.pred.hm[s].coff + j] - gt.gt_hm;
                const float e2 = p.pred.hm3[s].p[m * p.pred.hm3[s].cs + p.pred.hm3[s].coff + j] - gt.gt_hm3;
                const float* um = p.pred.um[s].p + m * p.pred.um[s].cs + p.pred.um[s].coff + 3 * j;
                const float e3 = um[0] - gt.ux, e4 = um[1] - gt.uy, e5 = um[2] - gt.uz;
                term[0][threadIdx.x] = 0.5 * (double)e1 * e1;
                term[1][threadIdx.x] = 0.5 * (double)e2 * e2;
                term[2][threadIdx.x] = 0.5 * ((double)e3 * e3 + (double)e4 * e4 + (double)e5 * e5);
            }
            __syncthreads();
            for (int q = threadIdx.x; q < 3 * p.J; q += 256) {
                const int jq = q / 3, k = q - 3 * jq;
                double a = 0.0;
#pragma unroll 4
                for (int t = (jq - j0 + p.J) % p.J; t < nlive; t += p.J) a += term[k][t];
                part[((long)s * p.J + jq) * 3 + k] = a;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void targets_kernel(const LossReportParams p) {
    loss_report_body<false>(p);
}

__global__ __launch_bounds__(256) void loss_report_kernel(const LossReportParams p) {
    loss_report_body<true>(p);
}

// One workgroup per crop: bsj[b][s][j][3] = the crop's chunks added in index order; cropd[b][s][3] = its joints added in index
// order (kept in fp64 for the stack sums, cast once into the report).  n = S * J * 3.
__global__ __launch_bounds__(256) void loss_report_crop_kernel(const double* part, int nchunk, int S, int J, double* bsj,
                                                               double* cropd, float* crop_out) {
    const int b = blockIdx.x, n = S * J * 3;
    const double* src = part + (long)b * nchunk * n;
    double* dst = bsj + (long)b * n;
    for (int q = threadIdx.x; q < n; q += 256) {
        double a = 0.0;
        // (unrolled: the loads of eight chunks in flight; the adds stay in index order)
#pragma unroll 8
        for (int c = 0; c < nchunk; ++c) a += src[(long)c * n + q];
        dst[q] = a;
    }
    __syncthreads();                                          // (this workgroup's own stores: visible to it behind the barrier)
    for (int q = threadIdx.x; q < S * 3; q += 256) {
        const int s = q / 3, k = q - 3 * s;
        double a = 0.0;
        for (int j = 0; j < J; ++j) a += dst[(s * J + j) * 3 + k];
        cropd[(long)b * S * 3 + q] = a;
        if (crop_out) crop_out[(long)b * S * 3 + q] = (float)a;
    }
}

// One workgroup: joint = sum over crops of bsj, stack = sum over crops of cropd, total = sum over stacks of stack; every sum in
// index order in fp64, cast to fp32 once at the store.
__global__ __launch_bounds__(256) void loss_report_out_kernel(const double* bsj, const double* cropd, int B, int S, int J,
                                                              float* joint_out, float* stack_out, float* total_out) {
    __shared__ double stack_sum[kMaxStack * 3];
    const int n = S * J * 3;
    if (joint_out)
        for (int q = threadIdx.x; q < n; q += 256) {
            double a = 0.0;
#pragma unroll 8
            for (int b = 0; b < B; ++b) a += bsj[(long)b * n + q];
            joint_out[q] = (float)a;
        }
    if ((int)threadIdx.x < S * 3) {
        double a = 0.0;
#pragma unroll 8
        for (int b = 0; b < B; ++b) a += cropd[(long)b * S * 3 + threadIdx.x];
        stack_sum[threadIdx.x] = a;
        if (stack_out) stack_out[threadIdx.x] = (float)a;
    }
    __syncthreads();
    if (threadIdx.x < 3 && total_out) {
        double a = 0.0;
        for (int s = 0; s < S; ++s) a += stack_sum[s * 3 + threadIdx.x];
        total_out[threadIdx.x] = (float)a;
    }
}

}  // namespace dr
