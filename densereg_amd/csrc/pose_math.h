// pose_math.h -- the crop camera, the point cloud and the training targets: ONE definition each, shared by loss_kernel
// (train_kernels.h), loss_report_body (loss_report.h), the candidate block and the uvd report of vote_body (vote.h) and the overlay
// points of render_kernel (render.h).  fp32 in the reference's op order
// with contraction off (data/preprocess.py:176-242, hourglass_um_crop_tiny.py:338-346; oracle/pose.py make_targets restates it).
// Pure: values (and pointers to a crop's few label floats) in, values out; every caller keeps its own thread geometry, map loads,
// reductions and stores.
#pragma once
#include "dr_platform.h"

namespace dr {

constexpr float kDepthRange = 300.0f;      // mm of depth around the centre of mass that a crop keeps (norm_dm_kernel)
constexpr float kPoseScale = 100.0f;       // mm per unit of a normalised coordinate
constexpr float kBackground = -0.99f;      // a normalised depth below this is background (norm_dm_kernel writes -1 there)
constexpr float kConeRadius = 4.0f;        // px: radius of the 2D heat-map cone
constexpr float kOffsetRadius = 0.8f;      // normalised units: radius of the 3D heat-map and of the unit-offset ball
constexpr float kOffsetNear = 1e-2f;       // a pixel carries unit offsets when its distance is below kOffsetRadius - kOffsetNear

struct MapCam { float fx, fy, cx, cy; };                 // the crop camera at map resolution
struct CloudPoint { float zz, X, Y, Z; };                // depth in mm; position relative to the centre of mass, normalised
struct PoseTargets { float gt_hm, gt_hm3, ux, uy, uz; };
struct Uvd { float u, v, d; };                           // a point in mm projected into an image: pixels and depth

// xyz2uvd_op with a camera cfg6 = fx, fy, cx, cy, w, h, unscaled (data/util.py:20 _pro): u = (x*fx)/z + cx, v = (y*fy)/z + cy, d = z.
// The vote report's uvd joints (vote.h) and the image report's overlay points (render.h).
__device__ __forceinline__ Uvd project_uvd(const float* cfg6, float x, float y, float z) {
#pragma clang fp contract(off)
    const float u = (x * cfg6[0]) / z + cfg6[2];
    const float v = (y * cfg6[1]) / z + cfg6[3];
    return {u, v, z};
}

// cfg6 = fx, fy, cx, cy, w, h of the crop camera; (w, h) = the map's size
__device__ __forceinline__ MapCam map_cam(const float* cfg6, int w, int h) {
#pragma clang fp contract(off)
    const float w_ratio = cfg6[4] / (float)w, h_ratio = cfg6[5] / (float)h;
    return {cfg6[0] / w_ratio, cfg6[1] / h_ratio, cfg6[2] / w_ratio, cfg6[3] / h_ratio};
}

// point cloud at map pixel px (row-major, row length w) with normalised depth t (preprocess.py:202-225)
__device__ __forceinline__ CloudPoint cloud_point(const MapCam& cam, const float* com3, float t, int px, int w) {
#pragma clang fp contract(off)
    const float cx0 = com3[0], cy0 = com3[1], cz0 = com3[2];
    const float xx = (float)(px % w), yy = (float)(px / w);
    const float min_depth = cz0 - kDepthRange * 0.5f, max_depth = cz0 + kDepthRange * 0.5f;
    const float zz = (t < kBackground) ? max_depth : (t * kDepthRange + min_depth);
    float X = (xx - cam.cx) * (zz / cam.fx);
    float Y = (yy - cam.cy) * (zz / cam.fy);
    X = (X - cx0) / kPoseScale;
    Y = (Y - cy0) / kPoseScale;
    const float Z = (zz - cz0) / kPoseScale;
    return {zz, X, Y, Z};
}

// targets of one joint (pose3 = its x, y, z in mm) at map pixel px
__device__ __forceinline__ PoseTargets pose_targets(const MapCam& cam, const float* com3, const float* pose3, const CloudPoint& cloud,
                                                    int px, int w) {
#pragma clang fp contract(off)
    const float cx0 = com3[0], cy0 = com3[1], cz0 = com3[2];
    const float xx = (float)(px % w), yy = (float)(px / w);
    // 2D cone (:225-242)
    const float u = pose3[0] * cam.fx / pose3[2] + cam.cx;
    const float v = pose3[1] * cam.fy / pose3[2] + cam.cy;
    const float du = xx - u, dv = yy - v;
    const float gt_hm = fmaxf(kConeRadius - sqrtf(du * du + dv * dv), 0.0f) / kConeRadius;
    // 3D offsets (:338-346)
    const float ox = (pose3[0] - cx0) / kPoseScale - cloud.X;
    const float oy = (pose3[1] - cy0) / kPoseScale - cloud.Y;
    const float oz = (pose3[2] - cz0) / kPoseScale - cloud.Z;
    const float dist = sqrtf((ox * ox + oy * oy) + oz * oz);
    const float gt_hm3 = fmaxf((kOffsetRadius - dist) / kOffsetRadius, 0.0f);
    const float d3 = kOffsetRadius - gt_hm3 * kOffsetRadius;
    const bool near = d3 < (kOffsetRadius - kOffsetNear);
    return {gt_hm, gt_hm3, near ? ox / d3 : 0.0f, near ? oy / d3 : 0.0f, near ? oz / d3 : 0.0f};
}

}  // namespace dr
