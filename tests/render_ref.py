"""The image report's definition, restated in numpy (tests/test_image_report.py compares the kernel's bytes with it).

Every fp32 operation of ``densereg_amd/csrc/render.h`` in the same order with ``np.float32`` arithmetic (each numpy operation on
float32 operands is one correctly rounded IEEE operation: no fused multiply-add), every index by integer arithmetic.  Imports
nothing from the product; the colour tables come in from ``tests/golden/colormaps.npz``.
"""
import numpy as np

F = np.float32
JET, GREYS, UM_XY = 0, 1, 2
PTS_NONE, PTS_UVD, PTS_XYZ_MM = 0, 1, 2
SKEL_NONE, SKEL_ICVL, SKEL_NYU, SKEL_MSRA = 0, 1, 2, 3
SKEL_JOINTS = {SKEL_ICVL: 16, SKEL_NYU: 14, SKEL_MSRA: 21}

# sizes in output pixels at out_hw = 128: three disc classes and half the line width
RADIUS = (F(3.5), F(2.25), F(1.75))
HALF_WIDTH = F(0.75)
# w c m y g r b as RGB
INK = np.array([(255, 255, 255), (0, 191, 191), (191, 0, 191), (191, 191, 0), (0, 128, 0), (255, 0, 0), (0, 0, 255)], np.uint8)
W, R, B = 0, 5, 6


def _skeleton(skel, num_pts):
    """Primitives in painter's order, as figure_joint_skeleton (data/visualization.py:58-121) issues its scatter / plot calls:
    ('d', joint, ink, size class) or ('s', joint a, joint b, ink)."""
    if skel == SKEL_NONE:
        return [('d', j, W, 2) for j in range(num_pts)]
    prims = []
    if skel == SKEL_ICVL:                       # all white s=200; per finger 3 joints (s = 90, 80, 60) and 2 bones
        prims += [('d', j, W, 0) for j in range(16)]
        for f in range(5):
            prims += [('d', 3 * f + 1, 1 + f, 1), ('d', 3 * f + 2, 1 + f, 1), ('d', 3 * f + 3, 1 + f, 2),
                      ('s', 3 * f + 1, 3 * f + 2, 1 + f), ('s', 3 * f + 2, 3 * f + 3, 1 + f)]
    elif skel == SKEL_MSRA:                     # all white s=200; per finger 4 joints (s = 90, 80, 70, 60) and 3 bones
        prims += [('d', j, W, 0) for j in range(21)]
        for f in range(5):
            prims += [('d', 4 * f + 1, 1 + f, 1), ('d', 4 * f + 2, 1 + f, 1), ('d', 4 * f + 3, 1 + f, 2), ('d', 4 * f + 4, 1 + f, 2),
                      ('s', 4 * f + 1, 4 * f + 2, 1 + f), ('s', 4 * f + 2, 4 * f + 3, 1 + f), ('s', 4 * f + 3, 4 * f + 4, 1 + f)]
    elif skel == SKEL_NYU:
        for f in range(5):
            prims += [('s', 2 * f, 2 * f + 1, 1 + f), ('d', 2 * f, 1 + f, 2), ('d', 2 * f + 1, 1 + f, 2)]
            if f < 4:
                prims += [('s', 13, 2 * f + 1, 1 + f)]
        prims += [('s', 9, 10, R), ('d', 13, W, 0), ('d', 11, B, 1), ('d', 12, B, 1), ('s', 13, 11, B), ('s', 13, 12, B),
                  ('s', 13, 10, R)]
    else:
        raise ValueError(skel)
    return prims


def vis_sin(q):
    """odd Taylor polynomial of degree 9, Horner in q*q, fp32 multiplies and adds"""
    q = np.asarray(q, F)
    q2 = q * q
    p = F(2.7557319e-6)
    p = p * q2 + F(-1.9841270e-4)
    p = p * q2 + F(8.3333333e-3)
    p = p * q2 + F(-1.6666667e-1)
    p = p * q2 + F(1.0)
    return (p * q).astype(F)


def vis_um_xy(x, y, z):
    """_vis_um_xy (hourglass_um_crop_tiny.py:307-309): 1 where d^2 + z^2 < 0.1, else sin(x / d)"""
    with np.errstate(all='ignore'):
        x, y, z = (np.asarray(a, F) for a in (x, y, z))
        d = np.sqrt(x * x + y * y)
        near = (d * d + z * z) < F(0.1)
        return np.where(near, F(1.0), vis_sin(x / d)).astype(F)


def project(cfg6, xyz):
    """xyz (N,3) in mm -> (N,2): u = (x*fx)/z + cx, v = (y*fy)/z + cy"""
    with np.errstate(all='ignore'):
        xyz, c = np.asarray(xyz, F), np.asarray(cfg6, F)
        u = (xyz[:, 0] * c[0]) / xyz[:, 2] + c[2]
        v = (xyz[:, 1] * c[1]) / xyz[:, 2] + c[3]
        return np.stack([u, v], 1).astype(F)


def colour(values, lut, out_hw):
    """values (h,w) float32 -> (out_hw,out_hw,3) uint8 through lut (256,3)"""
    values = np.asarray(values, F)
    h, w = values.shape
    fin = np.isfinite(values)
    img = np.empty((out_hw, out_hw, 3), np.uint8)
    sy = (np.arange(out_hw) * h) // out_hw
    sx = (np.arange(out_hw) * w) // out_hw
    v = values[sy[:, None], sx[None, :]]
    idx = np.zeros(v.shape, np.int64)
    if fin.any():
        lo, hi = values[fin].min(), values[fin].max()
        if hi > lo:
            with np.errstate(all='ignore'):
                s = ((v - lo) / (hi - lo)) * F(256.0)
            idx = np.where(s >= F(255.0), 255, np.where(s > F(0.0), np.trunc(np.where(np.isfinite(s), s, F(0.0))), 0)).astype(np.int64)
    img[...] = lut[idx]
    img[~np.isfinite(v)] = 255
    return img


def overlay(img, uv, pts_hw, skel):
    """draw the points uv (N,2), pixels of a pts_hw-sided image, over img (out_hw,out_hw,3) in place"""
    out_hw = img.shape[0]
    uv = np.asarray(uv, F)
    c = ((np.arange(out_hw).astype(F) + F(0.5)) * F(pts_hw)) / F(out_hw) - F(0.5)
    px, py = np.broadcast_arrays(c[None, :], c[:, None])
    unit = (F(out_hw) / F(128.0)) * (F(pts_hw) / F(out_hw))
    r2 = [(r * unit) * (r * unit) for r in RADIUS] + [(HALF_WIDTH * unit) * (HALF_WIDTH * unit)]
    with np.errstate(all='ignore'):
        for prim in _skeleton(skel, len(uv)):
            a = uv[prim[1]]
            if not np.isfinite(a).all():
                continue
            fx, fy = px - a[0], py - a[1]
            if prim[0] == 'd':
                hit = (fx * fx + fy * fy) <= r2[prim[3]]
                ink = prim[2]
            else:
                b = uv[prim[2]]
                if not np.isfinite(b).all():
                    continue
                ex, ey = b[0] - a[0], b[1] - a[1]
                s = fx * ex + fy * ey
                e2 = ex * ex + ey * ey
                gx, gy = px - b[0], py - b[1]
                cr = fx * ey - fy * ex
                hit = np.where(s <= F(0.0), (fx * fx + fy * fy) <= r2[3],
                               np.where(s >= e2, (gx * gx + gy * gy) <= r2[3], (cr * cr) <= (r2[3] * e2)))
                ink = prim[3]
            img[hit] = INK[ink]
    return img


def render_panel(src, channel, kind, luts, out_hw, pts=None, pts_space=PTS_NONE, pts_hw=0, skel=SKEL_NONE, cfg6=None):
    """One panel of one crop.  src (h,w,C) float32; luts = (jet, greys), each (256,3) uint8; pts (N,3)."""
    src = np.asarray(src, F)
    if kind == UM_XY:
        values = vis_um_xy(src[..., 3 * channel], src[..., 3 * channel + 1], src[..., 3 * channel + 2])
    else:
        values = src[..., channel]
    img = colour(values, luts[1 if kind == GREYS else 0], out_hw)
    if pts_space != PTS_NONE:
        pts = np.asarray(pts, F)
        uv = project(cfg6, pts) if pts_space == PTS_XYZ_MM else pts[:, :2]
        overlay(img, uv, pts_hw, skel)
    return img
