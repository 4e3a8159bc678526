// render.h -- the image report: float maps and joints in, RGB8 panels out, on the device.
//
// Replaces what the reference draws on the host for its image summaries (model/hourglass_um_crop_tiny.py:399-432, 487-516 through
// data/visualization.py): jet-coloured panels of a map channel (figure_heatmap), the offset-angle view _vis_um_xy (:301-311), and the
// depth crop in Greys with the joints and the hand skeleton drawn over it (figure_joint_skeleton).
//
// One launch renders all panels of all crops: grid (panel, crop), 256 threads.
//   phase 1  the workgroup parks its source channel -- a strided NHWC view, at most kRenderMaxPix pixels -- as one float per pixel
//            in LDS and reduces lo / hi over the FINITE values (wave butterfly, then across the four waves through LDS);
//   phase 2  every thread owns four consecutive output pixels of a row: nearest source pixel by integer arithmetic
//            (sy = y*src_h / out_hw, sx = x*src_w / out_hw), t = (v - lo) / (hi - lo), idx = min(255, (int)(t * 256)), colour =
//            LUT[idx]; a non-finite value is drawn white; t = 0 when no value is finite or hi == lo.  Then the overlay, and the 12
//            bytes leave as three dword stores (rows are contiguous: no byte stores).
// Every output byte is a pure function of integer and single-rounded fp32 operations (contraction off, no anti-aliasing):
// tests/render_ref.py restates them one by one in numpy and the tests compare bytes.
//
// Overlay (optional per panel).  Points are (u, v) in pixels of a pts_hw-sided image, given as uvd or as xyz in mm projected with the
// crop's camera (pose_math.h's project_uvd: the function the vote report's uvd uses).  The centre of output pixel (x, y) sits at
// ((x + 0.5) * pts_hw / out_hw - 0.5, (y + 0.5) * pts_hw / out_hw - 0.5) in point coordinates.  A pixel belongs to a disc when its
// squared distance to the point is <= r*r, and to a segment when its squared distance to the segment is <= hw*hw -- no division, no
// square root: with e = b - a, f = p - a and s = f.e, the pixel is judged by |f|^2 where s <= 0, by |p - b|^2 where s >= |e|^2 and
// by cross(f, e)^2 <= hw*hw*|e|^2 in between (a zero-length segment is a disc of radius hw).  A primitive with a non-finite
// coordinate is skipped.  Painter's order: the primitives in the order figure_joint_skeleton issues its scatter / plot calls; the
// last one that covers a pixel wins.
//
// Sizes, in OUTPUT pixels at out_hw = 128 and scaled by out_hw / 128.0f (then by pts_hw / out_hw into point coordinates).  The
// reference's markers have s = 200 / 100..80 / 70..60 points^2 and its lines 3 points on a 128-pixel crop shown about 370 screen
// pixels high at 100 dpi: radius sqrt(s)/2 points = 3.4 / 2.4..2.2 / 2.0..1.9 crop pixels, half a line 0.72.  Three classes and the line:
//     kRenderRadius = 3.5, 2.25, 1.75      kRenderHalfWidth = 0.75
// Every other point count, and DR_SKEL_NONE, gives white discs of the smallest class (figure_smp_pts' s = 60).
#pragma once
#include "dr_platform.h"
#include "pose_math.h"

namespace dr {

constexpr int kRenderMaxPix = 16384;       // LDS: 16384 px x 4 B = 64 KiB (the vote's plan), a 128x128 map
constexpr int kRenderMaxPanels = 16;
constexpr int kRenderMaxPts = 64;          // points of one overlay (their pixel positions live in LDS)
constexpr int kRenderMaxOut = 512;

// the values of include/densereg.h's enums (densereg.cpp asserts that they agree)
constexpr int kPanelJet = 0, kPanelGreys = 1, kPanelUmXy = 2;
constexpr int kPtsNone = 0, kPtsUvd = 1, kPtsXyzMm = 2;
constexpr int kSkelNone = 0, kSkelIcvl = 1, kSkelNyu = 2, kSkelMsra = 3;

struct RenderPanel {
    const float* src; int h, w, cs, ch, kind;          // (B,h,w,cs) view, channel ch (UM_XY: channels 3ch .. 3ch+2)
    const float* pts; int num_pts, space, pts_hw, skel;  // (B,num_pts,3)
    const float* cfg;                                  // (B,6), kPtsXyzMm only
};
struct RenderParams {
    RenderPanel panel[kRenderMaxPanels];
    int num_panels, out_hw;
    uint8_t* rgb;                                      // (B,num_panels,out_hw,out_hw,3)
};

// LDS: [npix] values, [8] wave partials of lo / hi, [2*kRenderMaxPts] point positions
__host__ __device__ constexpr size_t render_lds_bytes(int npix) { return ((size_t)npix + 8 + 2 * kRenderMaxPts) * sizeof(float); }

// matplotlib's jet and Greys at N = 256 (cmap(np.arange(256), bytes=True)[:, :3]), 0x00BBGGRR per entry
static const uint32_t kRenderLutHost[2][256] = {
#include "render_lut.inc"
};
__device__ const uint32_t kRenderLut[2][256] = {
#include "render_lut.inc"
};
constexpr uint32_t kRenderWhite = 0xFFFFFFu;

// overlay palette (matplotlib's single-letter colours), 0x00BBGGRR: w c m y g r b
__device__ const uint32_t kRenderInk[7] = {0xFFFFFFu, 0xBFBF00u, 0xBF00BFu, 0x00BFBFu, 0x008000u, 0x0000FFu, 0xFF0000u};
__device__ const float kRenderRadius[3] = {3.5f, 2.25f, 1.75f};
constexpr float kRenderHalfWidth = 0.75f;
constexpr int kInkW = 0, kInkR = 5, kInkB = 6;        // finger f = 0..4 uses ink 1 + f: c m y g r

// One primitive of a skeleton: a disc at joint a (size class 0..2) or the segment a - b (size class 3).
struct RenderPrim { uint8_t a, b, ink, cls; };
constexpr uint8_t kSeg = 3;
#define DR_DISC(j, ink, cls) {(uint8_t)(j), (uint8_t)(j), (uint8_t)(ink), (uint8_t)(cls)}
#define DR_SEG(a, b, ink) {(uint8_t)(a), (uint8_t)(b), (uint8_t)(ink), kSeg}
#define DR_W4(j) DR_DISC(j, kInkW, 0), DR_DISC((j) + 1, kInkW, 0), DR_DISC((j) + 2, kInkW, 0), DR_DISC((j) + 3, kInkW, 0)
// icvl, 16 joints (:109-119): every joint white and large; per finger f its three joints 3f+1..3f+3 (s = 90, 80, 60) and two bones
#define DR_ICVL_FINGER(f) DR_DISC(3 * (f) + 1, 1 + (f), 1), DR_DISC(3 * (f) + 2, 1 + (f), 1), DR_DISC(3 * (f) + 3, 1 + (f), 2), \
                          DR_SEG(3 * (f) + 1, 3 * (f) + 2, 1 + (f)), DR_SEG(3 * (f) + 2, 3 * (f) + 3, 1 + (f))
__device__ const RenderPrim kSkelIcvlPrims[16 + 5 * 5] = {
    DR_W4(0), DR_W4(4), DR_W4(8), DR_W4(12),
    DR_ICVL_FINGER(0), DR_ICVL_FINGER(1), DR_ICVL_FINGER(2), DR_ICVL_FINGER(3), DR_ICVL_FINGER(4)};
// msra, 21 joints (:95-108): every joint white and large; per finger f its four joints 4f+1..4f+4 (s = 90, 80, 70, 60), three bones
#define DR_MSRA_FINGER(f) DR_DISC(4 * (f) + 1, 1 + (f), 1), DR_DISC(4 * (f) + 2, 1 + (f), 1), DR_DISC(4 * (f) + 3, 1 + (f), 2), \
                          DR_DISC(4 * (f) + 4, 1 + (f), 2), DR_SEG(4 * (f) + 1, 4 * (f) + 2, 1 + (f)), \
                          DR_SEG(4 * (f) + 2, 4 * (f) + 3, 1 + (f)), DR_SEG(4 * (f) + 3, 4 * (f) + 4, 1 + (f))
__device__ const RenderPrim kSkelMsraPrims[21 + 5 * 7] = {
    DR_W4(0), DR_W4(4), DR_W4(8), DR_W4(12), DR_W4(16), DR_DISC(20, kInkW, 0),
    DR_MSRA_FINGER(0), DR_MSRA_FINGER(1), DR_MSRA_FINGER(2), DR_MSRA_FINGER(3), DR_MSRA_FINGER(4)};
// nyu, 14 joints (:71-93): per finger f the bone 2f - 2f+1 and its two joints (s = 60), fingers 0..3 joined to the palm centre 13;
// then the thumb's 9 - 10, the palm centre (white, s = 200), the two wrist joints 11, 12 (blue, s = 100), their bones, and 13 - 10
#define DR_NYU_FINGER(f) DR_SEG(2 * (f), 2 * (f) + 1, 1 + (f)), DR_DISC(2 * (f), 1 + (f), 2), DR_DISC(2 * (f) + 1, 1 + (f), 2)
__device__ const RenderPrim kSkelNyuPrims[5 * 3 + 4 + 7] = {
    DR_NYU_FINGER(0), DR_SEG(13, 1, 1), DR_NYU_FINGER(1), DR_SEG(13, 3, 2), DR_NYU_FINGER(2), DR_SEG(13, 5, 3),
    DR_NYU_FINGER(3), DR_SEG(13, 7, 4), DR_NYU_FINGER(4),
    DR_SEG(9, 10, kInkR), DR_DISC(13, kInkW, 0), DR_DISC(11, kInkB, 1), DR_DISC(12, kInkB, 1),
    DR_SEG(13, 11, kInkB), DR_SEG(13, 12, kInkB), DR_SEG(13, 10, kInkR)};
#undef DR_DISC
#undef DR_SEG
#undef DR_W4
#undef DR_ICVL_FINGER
#undef DR_MSRA_FINGER
#undef DR_NYU_FINGER

// joints of a skeleton (0 = no skeleton: any count)
__host__ __device__ constexpr int render_skel_joints(int skel) { return skel == kSkelIcvl ? 16 : skel == kSkelNyu ? 14 : skel == kSkelMsra ? 21 : 0; }

// sin(q) for q in [-1, 1]: the odd Taylor polynomial of degree 9, Horner in q*q (remainder below 1/11! = 2.5e-8); every step one
// correctly rounded fp32 multiply or add, no fused multiply-add: bit-reproducible by any IEEE implementation.  NaN propagates.
__device__ __forceinline__ float vis_sin(float q) {
#pragma clang fp contract(off)
    const float q2 = q * q;
    float p = 2.7557319e-6f;            //  1/9!
    p = p * q2 + -1.9841270e-4f;        // -1/7!
    p = p * q2 + 8.3333333e-3f;         //  1/5!
    p = p * q2 + -1.6666667e-1f;        // -1/3!
    p = p * q2 + 1.0f;
    return p * q;
}

// _vis_um_xy (:307-309) of one pixel's unit offset
__device__ __forceinline__ float vis_um_xy(float x, float y, float z) {
#pragma clang fp contract(off)
    const float d = sqrtf(x * x + y * y);
    if ((d * d + z * z) < 0.1f) return 1.0f;
    return vis_sin(x / d);
}

__device__ __forceinline__ bool render_finite(float v) { return fabsf(v) < INFINITY; }      // NaN fails

// does the pixel centre (px, py) belong to the disc of squared radius r2 at (ax, ay)?
__device__ __forceinline__ bool render_in_disc(float px, float py, float ax, float ay, float r2) {
#pragma clang fp contract(off)
    const float fx = px - ax, fy = py - ay;
    return (fx * fx + fy * fy) <= r2;
}

// ... to the segment a - b of squared half-width w2?
__device__ __forceinline__ bool render_in_segment(float px, float py, float ax, float ay, float bx, float by, float w2) {
#pragma clang fp contract(off)
    const float ex = bx - ax, ey = by - ay, fx = px - ax, fy = py - ay;
    const float s = fx * ex + fy * ey, e2 = ex * ex + ey * ey;
    if (s <= 0.0f) return (fx * fx + fy * fy) <= w2;
    if (s >= e2) {
        const float gx = px - bx, gy = py - by;
        return (gx * gx + gy * gy) <= w2;
    }
    const float c = fx * ey - fy * ex;
    return (c * c) <= (w2 * e2);
}

__global__ __launch_bounds__(256) void render_kernel(const RenderParams p) {
#pragma clang fp contract(off)
    DR_DYN_SMEM(smem_raw);
    const RenderPanel pn = p.panel[blockIdx.x];
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int npix = pn.h * pn.w;
    float* val = reinterpret_cast<float*>(smem_raw);      // [npix]
    float* red = val + npix;                              // [8]
    float* pts = red + 8;                                 // [2 * num_pts]

    // ---- phase 1: the source channel into LDS, lo / hi over its finite values ---------------------
    float lo = INFINITY, hi = -INFINITY;
    {
        const float* src = pn.src + (long)b * npix * pn.cs + (pn.kind == kPanelUmXy ? 3 * pn.ch : pn.ch);
        for (int px = tid; px < npix; px += 256) {
            const float* s = src + (long)px * pn.cs;
            const float v = pn.kind == kPanelUmXy ? vis_um_xy(s[0], s[1], s[2]) : s[0];
            val[px] = v;
            if (render_finite(v)) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
        }
    }
    if (pn.space != kPtsNone && tid < pn.num_pts) {
        const float* q = pn.pts + ((long)b * pn.num_pts + tid) * 3;
        float u = q[0], v = q[1];
        if (pn.space == kPtsXyzMm) {
            const Uvd uvd = project_uvd(pn.cfg + b * 6, q[0], q[1], q[2]);
            u = uvd.u; v = uvd.v;
        }
        pts[2 * tid] = u;
        pts[2 * tid + 1] = v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, m));
        hi = fmaxf(hi, __shfl_xor(hi, m));
    }
    if ((tid & 63) == 0) { red[tid >> 6] = lo; red[4 + (tid >> 6)] = hi; }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    const bool flat = !(hi > lo);                         // no finite value (lo = +inf, hi = -inf) or a constant map
    const float span = hi - lo;

    // ---- phase 2: colour, overlay, store ------------------------------------------------------------
    const int out_hw = p.out_hw, gpr = out_hw >> 2;       // groups of four pixels per row
    const uint32_t* lut = kRenderLut[pn.kind == kPanelGreys ? 1 : 0];
    const RenderPrim* prims = pn.skel == kSkelIcvl ? kSkelIcvlPrims : pn.skel == kSkelNyu ? kSkelNyuPrims : kSkelMsraPrims;
    const int nprim = pn.space == kPtsNone ? 0
                    : pn.skel == kSkelIcvl ? (int)(sizeof(kSkelIcvlPrims) / sizeof(RenderPrim))
                    : pn.skel == kSkelNyu ? (int)(sizeof(kSkelNyuPrims) / sizeof(RenderPrim))
                    : pn.skel == kSkelMsra ? (int)(sizeof(kSkelMsraPrims) / sizeof(RenderPrim)) : pn.num_pts;
    // sizes in point coordinates, squared
    const float unit = ((float)out_hw / 128.0f) * ((float)pn.pts_hw / (float)out_hw);
    float r2[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) { const float r = kRenderRadius[c] * unit; r2[c] = r * r; }
    { const float r = kRenderHalfWidth * unit; r2[3] = r * r; }
    uint32_t* out = reinterpret_cast<uint32_t*>(p.rgb + ((long)b * p.num_panels + blockIdx.x) * out_hw * out_hw * 3);

    for (int g = tid; g < gpr * out_hw; g += 256) {
        const int y = g / gpr, x0 = (g - y * gpr) * 4;
        const int sy = (y * pn.h) / out_hw;
        const float py = ((float)y + 0.5f) * (float)pn.pts_hw / (float)out_hw - 0.5f;
        uint32_t c4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + i;
            const int sx = (x * pn.w) / out_hw;
            const float v = val[sy * pn.w + sx];
            uint32_t c = kRenderWhite;
            if (render_finite(v)) {
                int idx = 0;
                if (!flat) {
                    const float t = (v - lo) / span;
                    const float s = t * 256.0f;           // min(255, (int)s); a NaN (inf / inf: a span beyond fp32) gives 0
                    idx = s >= 255.0f ? 255 : (s > 0.0f ? (int)s : 0);
                }
                c = lut[idx];
            }
            if (nprim > 0) {
                const float px = ((float)x + 0.5f) * (float)pn.pts_hw / (float)out_hw - 0.5f;
                for (int k = 0; k < nprim; ++k) {
                    RenderPrim pr;
                    if (pn.skel == kSkelNone) pr = RenderPrim{(uint8_t)k, (uint8_t)k, (uint8_t)kInkW, 2};
                    else pr = prims[k];
                    const float ax = pts[2 * pr.a], ay = pts[2 * pr.a + 1];
                    if (!(render_finite(ax) && render_finite(ay))) continue;
                    bool hit;
                    if (pr.cls == kSeg) {
                        const float bx = pts[2 * pr.b], by = pts[2 * pr.b + 1];
                        if (!(render_finite(bx) && render_finite(by))) continue;
                        hit = render_in_segment(px, py, ax, ay, bx, by, r2[3]);
                    } else {
                        hit = render_in_disc(px, py, ax, ay, r2[pr.cls]);
                    }
                    if (hit) c = kRenderInk[pr.ink];
                }
            }
            c4[i] = c;
        }
        // 4 pixels x RGB = 12 bytes = three dwords, little endian: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        uint32_t* o = out + (long)g * 3;
        o[0] = c4[0] | (c4[1] << 24);
        o[1] = (c4[1] >> 8) | (c4[2] << 16);
        o[2] = (c4[2] >> 16) | (c4[3] << 8);
    }
}

}  // namespace dr
