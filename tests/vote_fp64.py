"""The test-time pose estimate (the offset vote), stated in plain numpy / float64 (tests/test_vote_fp64.py holds the HIP vote and
``oracle/pose.py`` to it).

Written from the reference's text, ``model/hourglass_um_crop_tiny.py:596-785`` (with ``:276-299`` for the offsets, ``:451-462`` for the
call and ``data/preprocess.py:157-232`` for the point cloud and the un-normalisation), NOT from the kernel or the oracle: it imports
nothing from the product or from ``oracle``, restates its constants, widens the fp32 inputs to float64 once and never rounds to fp32
in between; the one transcendental is ``np.exp``.  It follows the mathematics, not the operation order of ``vote.h``.

The estimate is discontinuous (a top-5 selection, a truncation, a cell, an arg-max), and an fp32 evaluation may legitimately land on
the other side of a discontinuity it is close to.  So ``estimate`` also returns, per (crop, joint), how far the float64 evaluation
is from each of them; ``well_conditioned`` turns that into the joints on which an fp32 evaluation has to agree.  Conditioning is a
property of the inputs under THIS definition: nothing here sees a kernel's or the oracle's output.
"""
import numpy as np

POSE_NORM_RATIO = 100.0         # data/preprocess.py:173
D_RANGE = 300.0                 # data/preprocess.py:172
MAX_DIST_3D = 0.8               # hourglass_um_crop_tiny.py:194
BACKGROUND = -0.99              # :767 and preprocess.py:205
NUM_CANDIDATES = 5              # :770
MS_ITERATIONS = 10              # :775
MS_BANDWIDTH = 0.4              # :775
NUM_QUAN = 2.0                  # :704: cells of 1/2 over [-1, 1)^3, 4 x 4 x 4

MARGIN = 1e-4                   # three orders above fp32 rounding (6e-8) of O(1) quantities
MASS_FLOOR = 1e-30              # a kernel mass is either exactly zero (all weights zero) or above this
SENS_REL = 2.0 ** -20           # relative perturbation of the sensitivity margin ...
SENS_MM = 1e-3                  # ... under which the joint has to move by less than this
MARGIN_NAMES = ('top5_gap', 'depth', 'reproj', 'cell', 'start_gap')


def scaled_camera(cfg, w, h):
    """:649-653 (and preprocess.py:213-217): the camera of the map, fx fy cx cy divided by the crop-to-map ratios."""
    wr, hr = cfg[4] / w, cfg[5] / h
    return cfg[0] / wr, cfg[1] / hr, cfg[2] / wr, cfg[3] / hr


def point_cloud(tiny, cfg, com):
    """preprocess.py:189-232 (called at :756): (B,h,w) normalised depth -> (B,h,w,3) normalised points.  Background pixels sit at the
    far plane.  The reference's meshgrid makes u the column and v the row (it needs h == w)."""
    B, h, w = tiny.shape
    assert h == w
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((B, h, w, 3))
    for b in range(B):
        near, far = com[b, 2] - D_RANGE * 0.5, com[b, 2] + D_RANGE * 0.5
        z = np.where(tiny[b] < BACKGROUND, far, tiny[b] * D_RANGE + near)
        fx, fy, cx, cy = scaled_camera(cfg[b], w, h)
        out[b, :, :, 0] = ((u - cx) * (z / fx) - com[b, 0]) / POSE_NORM_RATIO
        out[b, :, :, 1] = ((v - cy) * (z / fy) - com[b, 1]) / POSE_NORM_RATIO
        out[b, :, :, 2] = (z - com[b, 2]) / POSE_NORM_RATIO
    return out


def top_candidates(score, k):
    """:617 tf.nn.top_k(sorted=True): the k + 1 best pixels by descending score, the lower index first among equals."""
    order = np.lexsort((np.arange(score.size), -score))
    return order[:k + 1]


def reprojection(can, com, cam, hm_j):
    """:646-663 for one candidate: its pixel on the map by trunc(u + 0.5), trunc(v + 0.5), and hm there.  The reference gathers whatever
    tf.gather_nd gives out of range; the project's documented choice is weight 0 there and where u or v is not finite.
    Returns (weight, pixel or -1, margin): the margin is the distance of u + 0.5 / v + 0.5 from the nearest integer and from the range
    bounds -1 and out_hw when the candidate is inside, and how far outside the farthest offending coordinate is when it is not."""
    h, w = hm_j.shape
    fx, fy, cx, cy = cam
    p = can * POSE_NORM_RATIO + com
    with np.errstate(all='ignore'):
        uf = p[0] * fx / p[2] + cx + 0.5
        vf = p[1] * fy / p[2] + cy + 0.5
    if not (np.isfinite(uf) and np.isfinite(vf)):
        return 0.0, -1, np.inf
    outside = [max(-1.0 - f, f - n) for f, n in ((uf, w), (vf, h)) if not (-1.0 < f < n)]
    if outside:
        return 0.0, -1, max(outside)
    margin = min(min(abs(f - np.rint(f)), f + 1.0, n - f) for f, n in ((uf, w), (vf, h)))
    uu, vv = int(uf), int(vf)                                   # tf.to_int32 truncates toward zero: (-1, 1) -> 0
    return float(hm_j[vv, uu]), vv * w + uu, margin


def start_cell(can, wt):
    """:704-712: weights scattered (duplicates add) into the 4x4x4 grid over clip((can + 1) * 2, 0, 3.9); the LAST maximum in
    row-major order (tf.where(...)[-1]); its cell centre.  Returns (centre, relative gap between the heaviest and the second-heaviest
    cell, distance of (can + 1) * 2 from the nearest cell boundary 1, 2, 3 and from the clip bounds 0 and 3.9)."""
    f = (can + 1.0) * NUM_QUAN
    hi = 2 * NUM_QUAN - 0.1
    q = np.clip(f, 0.0, hi).astype(np.int64)
    grid = np.zeros(64)
    np.add.at(grid, q[:, 0] * 16 + q[:, 1] * 4 + q[:, 2], wt)
    last = int(np.nonzero(grid == grid.max())[0][-1])
    centre = np.array([last // 16, (last // 4) % 4, last % 4], np.float64) / NUM_QUAN - 1.0 + 0.5 / NUM_QUAN
    top, second = grid[last], np.delete(grid, last).max()
    gap = (top - second) / max(abs(top), 1e-300)
    bounds = np.array([0.0, 1.0, 2.0, 3.0, hi])
    cell_margin = np.abs(f[..., None] - bounds).min()
    return centre, gap, cell_margin


def mean_shift(can, wt, centre):
    """:715-721: ten times, s_i = w_i * exp(-|can_i - c|^2 / (2 bw^2)), c = sum s_i can_i / sum s_i.  The project's guard (the
    reference divides regardless): a kernel mass that is zero or not finite ends the iteration and keeps the centre.
    Returns (centre, the masses seen)."""
    inv = -1.0 / (2 * MS_BANDWIDTH * MS_BANDWIDTH)
    c, masses = centre, []
    for _ in range(MS_ITERATIONS):
        with np.errstate(all='ignore'):
            s = wt * np.exp(inv * ((can - c) ** 2).sum(axis=1))
            mass = s.sum()
        masses.append(mass)
        if mass == 0 or not np.isfinite(mass):
            break
        c = (can * s[:, None]).sum(axis=0) / mass
    return c, masses


def kernel_mass(can, wt, c):
    """sum_i w_i exp(-3.125 |can_i - c|^2) and its terms' arguments, in float64."""
    x = (-1.0 / (2 * MS_BANDWIDTH * MS_BANDWIDTH)) * ((np.asarray(can, np.float64) - np.asarray(c, np.float64)) ** 2).sum(axis=-1)
    return (np.asarray(wt, np.float64) * np.exp(x)).sum(axis=-1), x


def estimate(hm, hm3, um, ndm, cfg, com, seed=0):
    """JointDetectionModel.test (:451-462): last-stack maps (B,h,w,J) (B,h,w,J) (B,h,w,3J), normalised depth (B,H,W,1), cameras (B,6),
    centres of mass (B,3) -> dict:

    xyz_mm (B,J,3), xyz_norm (B,J,3), can_idx (B,J,5), can_pts (B,J,5,3), can_weight (B,J,5), weight_px (B,J,5; -1 = out of range);
    margins: name -> (B,J) for MARGIN_NAMES plus 'top5_gap_distinct' (the 5th score against the best score strictly below it: what is
    left of 'top5_gap' when scores tie exactly and the tie rule decides); mass_ok (B,J) bool; sens_mm (B,J)."""
    hm, hm3, um, ndm, cfg, com = (np.asarray(a, np.float32).astype(np.float64) for a in (hm, hm3, um, ndm, cfg, com))
    B, h, w, J = hm.shape
    K = NUM_CANDIDATES
    step = ndm.shape[1] // h
    tiny = ndm[:, ::step, ::step, 0]                            # :453 nearest-neighbour resize by an integer factor
    cloud = point_cloud(tiny, cfg, com)                         # :756
    om = um.reshape(B, h, w, J, 3) * (MAX_DIST_3D - hm3 * MAX_DIST_3D)[..., None]       # :287-298
    raw = (hm + 1.0) * hm3                                      # :764
    foreground = ~(tiny < BACKGROUND)                           # :767
    refined = raw * foreground[..., None]                       # :768
    rng = np.random.default_rng(seed)
    res = {'xyz_mm': np.zeros((B, J, 3)), 'xyz_norm': np.zeros((B, J, 3)), 'can_idx': np.zeros((B, J, K), np.int64),
           'can_pts': np.zeros((B, J, K, 3)), 'can_weight': np.zeros((B, J, K)), 'weight_px': np.zeros((B, J, K), np.int64),
           'margins': {n: np.zeros((B, J)) for n in MARGIN_NAMES + ('top5_gap_distinct',)},
           'mass_ok': np.zeros((B, J), bool), 'sens_mm': np.zeros((B, J))}
    mg = res['margins']
    for b in range(B):
        cam = scaled_camera(cfg[b], w, h)
        depth = tiny[b].reshape(-1)
        for j in range(J):
            score = refined[b, :, :, j].reshape(-1)
            order = top_candidates(score, K)
            idx, fifth, sixth = order[:K], score[order[K - 1]], score[order[K]]
            mg['top5_gap'][b, j] = (fifth - sixth) / max(abs(fifth), 1e-300)
            below = score[score < fifth]
            mg['top5_gap_distinct'][b, j] = (fifth - below.max()) / max(abs(fifth), 1e-300) if below.size else np.inf
            # depth: the candidates' own pixels, and background pixels that would be candidates as foreground
            rivals = ~foreground[b].reshape(-1) & (raw[b, :, :, j].reshape(-1) >= fifth)
            mg['depth'][b, j] = min(np.abs(depth[idx] - BACKGROUND).min(),
                                    np.abs(depth[rivals] - BACKGROUND).min() if rivals.any() else np.inf)
            can = (cloud[b].reshape(-1, 3) + om[b, :, :, j].reshape(-1, 3))[idx]        # :760, :618-621
            wt, wpx, rm = zip(*[reprojection(can[i], com[b], cam, hm[b, :, :, j]) for i in range(K)])
            wt = np.array(wt)
            mg['reproj'][b, j] = min(rm)
            centre, mg['start_gap'][b, j], mg['cell'][b, j] = start_cell(can, wt)
            c, masses = mean_shift(can, wt, centre)
            res['mass_ok'][b, j] = all((m == 0 and not wt.any()) or m > MASS_FLOOR for m in masses)
            moved = 0.0
            sign = rng.choice([-1.0, 1.0], size=(K, 4))
            for sg in (sign, -sign):
                can_p, wt_p = can * (1.0 + SENS_REL * sg[:, :3]), wt * (1.0 + SENS_REL * sg[:, 3])
                c_p, _ = mean_shift(can_p, wt_p, start_cell(can_p, wt_p)[0])
                moved = max(moved, np.abs(c_p - c).max() * POSE_NORM_RATIO)
            res['sens_mm'][b, j] = moved
            res['xyz_norm'][b, j] = c
            res['xyz_mm'][b, j] = c * POSE_NORM_RATIO + com[b]                          # preprocess.py:166
            res['can_idx'][b, j], res['can_pts'][b, j], res['can_weight'][b, j], res['weight_px'][b, j] = idx, can, wt, wpx
    return res


def well_conditioned(res, instead=None):
    """(B,J) bool: every distance / relative margin above MARGIN, every kernel mass zero-by-zero-weights or above MASS_FLOOR, the
    sensitivity under SENS_MM.  ``instead`` replaces margins whose discontinuity a case decides by an exact rule on exact ties:
    {'top5_gap': 'top5_gap_distinct'} for tied scores, {'start_gap': None} for the all-zero grid."""
    instead = instead or {}
    ok = res['mass_ok'] & (res['sens_mm'] < SENS_MM)
    for n in MARGIN_NAMES:
        n = instead.get(n, n)
        if n is not None:
            ok = ok & (res['margins'][n] > MARGIN)
    return ok
