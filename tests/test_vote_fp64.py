"""The offset vote against a definition that is NOT a copy of it (``tests/vote_fp64.py``: numpy / float64, ``np.exp``, written from
the reference's text), next to the bit-exact tests against ``oracle/pose.py``.

``oracle/pose.py::exp_f32`` and ``vote.h::vote_exp`` are one fp32 sequence, stated twice; an error in a coefficient, the bandwidth,
a tie rule or a truncation that both share passes every ``assert_array_equal`` of the suite.  Here (a) the oracle's exp is held to
``np.exp``, (b) the device's exp to float64 through the report's ``mass``, (c, d) the kernel's and the oracle's joints to the float64
definition at 5e-3 mm -- the bar ``test_forward_parity.py::test_vote_seeded_random_maps`` had while its two sides differed by ulps of
exp -- on every joint the definition calls well-conditioned (``vote_fp64.well_conditioned``: decided from the inputs alone).
Measured figures: ``profiles/vote_fp64.md``.
"""
import functools

import numpy as np
import pytest

from tests import vote_fp64 as V
from tests.test_vote_report import _seeded_maps, be, vote_report  # noqa: F401

BAR_MM = 5e-3
F32 = np.float32


# ---------------------------------------------------------------------------------------------
# the definition's constants are the oracle's
# ---------------------------------------------------------------------------------------------
def test_constants_equal_the_oracles():
    from oracle import pose
    assert V.POSE_NORM_RATIO == float(pose.POSE_NORM_RATIO) and V.D_RANGE == float(pose.D_RANGE)
    assert F32(V.MAX_DIST_3D) == pose.MAX_DIST_3D
    assert (V.NUM_CANDIDATES, V.MS_ITERATIONS, V.MS_BANDWIDTH) == (pose.NUM_PT, pose.MS_ITERS, pose.MS_BANDWIDTH) == (5, 10, 0.4)
    assert -1.0 / (2 * V.MS_BANDWIDTH ** 2) == pytest.approx(-3.125, rel=1e-15)


# ---------------------------------------------------------------------------------------------
# (a) the oracle's exp against the library's
# ---------------------------------------------------------------------------------------------
def _ulp_errors(xs):
    """(error against the real exp in ulps of the correctly rounded fp32 value, distance from that value in whole ulps)"""
    from oracle import pose
    xs = np.asarray(xs, F32)
    got = np.array([pose.exp_f32(x) for x in xs], F32)
    true = np.exp(xs.astype(np.float64))
    rounded = true.astype(F32)
    ulp = np.spacing(rounded).astype(np.float64)
    return np.abs(got.astype(np.float64) - true) / ulp, np.abs(got.astype(np.float64) - rounded.astype(np.float64)) / ulp


def _neighbours(x, n):
    """n consecutive fp32 values on each side of x (the nearest fp32 to x among them)"""
    c = int(np.array(x, F32).view(np.int32))
    return np.arange(c - n, c + n + 1, dtype=np.int32).view(F32)


def test_oracle_exp_against_library_exp():
    """exp_f32 within 1 ulp of the correctly rounded np.exp on (-87, 0]: seeded points, both sides of every reduction boundary
    (k + 0.5) ln 2 (where n steps and r changes sign at its largest magnitude), the top of the range, the 64 values just above the
    cutoff.  The cutoff's cost: exp_f32(x <= -87) is exactly 0 where the true value is below 2e-38.  NaN in, NaN out."""
    from oracle import pose
    rng = np.random.default_rng(8701)
    xs = [-87.0 * rng.random(20000)]
    xs += [_neighbours((k + 0.5) * np.log(2.0), 64) for k in range(0, -126, -1)]
    xs += [[0.0, -0.0, -1e-45, -1e-8]]
    above = np.array(-87.0, F32).view(np.int32) - 1 - np.arange(64, dtype=np.int32)      # negative floats: a smaller pattern is closer to 0
    xs += [above.view(F32)]
    xs = np.concatenate([np.asarray(x, F32) for x in xs])
    xs = xs[xs <= 0]
    assert xs.min() > -87 and xs.size > 36000
    real, whole = _ulp_errors(xs)
    print('\nexp_f32 vs np.exp on %d points of (-87, 0]: worst %.3f ulp of the real value (at x = %r), worst distance from the '
          'correctly rounded value %.0f ulp' % (xs.size, real.max(), float(xs[real.argmax()]), whole.max()))
    assert whole.max() <= 1
    assert pose.exp_f32(F32(0.0)) == 1 and pose.exp_f32(F32(-0.0)) == 1
    # at and below the cutoff: exactly 0, where the library's value is below 2e-38
    for x in (F32(-87.0), np.nextafter(F32(-87.0), F32(-np.inf)), F32(-88.0), F32(-1000.0), F32(-np.inf)):
        y = pose.exp_f32(x)
        assert y == 0 and not np.signbit(y) and np.exp(np.float64(x)) < 2e-38
    assert np.isnan(pose.exp_f32(F32(np.nan)))


# ---------------------------------------------------------------------------------------------
# planted maps: the winners, their offsets and their weights are chosen, not drawn
# ---------------------------------------------------------------------------------------------
def _planted_maps(rng, B, m, J, pixels, pushed_out=None, tie=False):
    """hm is a smooth positive field (0.4 .. 0.8: every re-projection weight is positive and comparable), hm3 small noise, so the
    refined heat is below 0.2 everywhere but at ``pixels[b][j]`` (n map pixels), where hm3 = 0.9 - 0.02 k puts it above 1.1 on
    foreground depth; um there is a vector of length 0.5 .. 1.5, an offset of about 0.1 normalised units.  The first
    ``pushed_out[b][j]`` of them get hm3 = 0.5 and um = (-4, 0, 0): 160 mm to the left, off the map, weight 0.  ``tie``: the planted
    pixels share one hm and one hm3 value exactly."""
    in_hw = 4 * m
    yy, xx = np.mgrid[0:m, 0:m].astype(np.float64)
    hm = np.empty((B, m, m, J), F32)
    for b in range(B):
        for j in range(J):
            p = rng.uniform(0, 2 * np.pi, 2)
            hm[b, :, :, j] = 0.6 + 0.1 * np.sin(3 * np.pi * xx / m + p[0]) + 0.1 * np.cos(2.5 * np.pi * yy / m + p[1])
    hm += (0.005 * rng.standard_normal(hm.shape)).astype(F32)
    hm3 = np.abs(0.02 * rng.standard_normal((B, m, m, J))).astype(F32)
    um = (0.2 * rng.standard_normal((B, m, m, 3 * J))).astype(F32)
    tiny = rng.uniform(0.2, 0.8, (B, m, m)).astype(F32)
    tiny[rng.random((B, m, m)) < 0.2] = -1.0
    for b in range(B):
        for j in range(J):
            for k, px in enumerate(pixels[b][j]):
                v, u = divmod(int(px), m)
                tiny[b, v, u] = rng.uniform(0.35, 0.65)
                d = rng.standard_normal(3)
                um[b, v, u, 3 * j:3 * j + 3] = d / np.linalg.norm(d) * rng.uniform(0.5, 1.5)
                hm3[b, v, u, j] = 0.9 if tie else 0.9 - 0.02 * k
                if tie:
                    hm[b, v, u, j] = 0.7
                if pushed_out is not None and k < pushed_out[b][j]:
                    hm3[b, v, u, j] = 0.5 - 0.02 * k
                    um[b, v, u, 3 * j:3 * j + 3] = (-4.0, 0.0, 0.0)
    ndm = np.repeat(np.repeat(tiny[..., None], 4, axis=1), 4, axis=2).astype(F32)
    k = in_hw / 128.0
    cfg = np.stack([[rng.uniform(450, 650) * k, rng.uniform(450, 650) * k, in_hw / 2 + rng.normal(0, 3), in_hw / 2 + rng.normal(0, 3),
                     in_hw, in_hw] for _ in range(B)]).astype(F32)
    com = np.stack([[rng.normal(0, 20), rng.normal(0, 20), rng.uniform(400, 700)] for _ in range(B)]).astype(F32)
    return hm, hm3, um, ndm, cfg, com


def _interior_pixels(rng, B, m, J, n, border=4):
    side = m - 2 * border
    pick = lambda: [(border + q // side) * m + border + q % side for q in rng.choice(side * side, n, replace=False)]
    return [[pick() for _ in range(J)] for _ in range(B)]


# ---------------------------------------------------------------------------------------------
# (b) the device's exp, through the report's kernel mass
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mass_case():
    B, m, J = 2, 32, 4
    rng = np.random.default_rng(2718)
    pushed = [[(b + j) % 4 for j in range(J)] for b in range(B)]              # 5, 4, 3, 2 candidates keep a weight
    return _planted_maps(rng, B, m, J, _interior_pixels(rng, B, m, J, 5), pushed_out=pushed), pushed


def test_device_exp_through_the_kernel_mass(be):
    """mass = sum_i w_i vote_exp(-3.125 |can_i - c|^2) from the report, against the same sum in float64 with np.exp over the report's
    OWN can_pts, can_weight and xyz_norm.  The bound is the arithmetic's: six fp32 roundings on the way to x_i (|dx_i| <= |x_i| 2^-21),
    one ulp of exp and one rounding of the product (2^-22), four roundings of a positive five-term sum (2^-22 of the mass)."""
    from oracle.graph import NetConfig
    maps, pushed = _mass_case()
    B, J = maps[0].shape[0], maps[0].shape[3]
    h = be.handle(NetConfig(1, 8, J), B)
    _, got = vote_report(be, h, *maps, want=('xyz_norm', 'can_pts', 'can_weight', 'mass'))
    h.close()
    can, w, c, mass = (got[n][0].astype(np.float64) for n in ('can_pts', 'can_weight', 'xyz_norm', 'mass'))
    assert (w >= 0).all(), 'the planted weights are positive or zero: no cancellation in the sum'
    kept = (w > 0).sum(axis=2)
    assert (kept == 5 - np.array(pushed)).all() and kept.min() == 2 and kept.max() == 5
    assert (w[w > 0].min() > 0.3) and (w.max() < 0.9)                          # comparable
    x = -3.125 * ((can - c[:, :, None, :]) ** 2).sum(axis=3)
    terms = w * np.exp(x)
    mass64 = terms.sum(axis=2)
    bound = (terms * (np.abs(x) * 2.0 ** -21 + 2.0 ** -22)).sum(axis=2) + 2.0 ** -22 * mass64
    # what the planted cases are for: several terms per joint with an argument in [-4, 0] that carry weight in the sum
    heavy = (x >= -4) & (terms >= 1e-2 * mass64[..., None])
    assert (heavy.sum(axis=2) >= 2).all() and heavy.sum() >= 3 * B * J
    assert np.abs(x[heavy]).max() > 2 and np.abs(x[heavy]).min() < 0.1
    slack = np.abs(mass - mass64) / bound
    print('\n[%s] kernel mass vs float64: worst |mass - mass64| / bound = %.3f over %d joints, %d heavy terms, |x| in [%.3f, %.3f]'
          % (be.name, slack.max(), B * J, heavy.sum(), np.abs(x[heavy]).min(), np.abs(x[heavy]).max()))
    assert (np.abs(mass - mass64) <= bound).all(), slack


# ---------------------------------------------------------------------------------------------
# (c) joints against the definition: the seeded random maps of test_forward_parity.py::test_vote_seeded_random_maps
# ---------------------------------------------------------------------------------------------
class Case:
    """maps, the definition's result on them (computed once, shared, never written to) and the joints it calls well-conditioned"""

    def __init__(self, maps, in_hw, max_batch=None, instead=None, where=None):
        self.maps, self.in_hw = maps, in_hw
        self.B, self.J = maps[0].shape[0], maps[0].shape[3]
        self.max_batch = max_batch or self.B
        self.ref = V.estimate(*maps)
        self.well = V.well_conditioned(self.ref)
        if instead:                                             # an exact rule on an exact tie, on the joints `where` names and no others
            self.well = np.where(where(self.ref), V.well_conditioned(self.ref, instead), self.well)
        for a in list(self.ref.values()) + list(self.ref['margins'].values()) + [self.well]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def worst(self, xyz_mm):
        """largest coordinate distance in mm over the well-conditioned joints"""
        d = np.abs(np.asarray(xyz_mm, np.float64).reshape(self.B, self.J, 3) - self.ref['xyz_mm']).max(axis=2)
        return float(d[self.well].max())

    def check_discrete(self, got):
        """well-conditioned joints: the kernel chose the definition's five pixels and gathered its weights from the same pixels"""
        idx, w = got['can_idx'][0], got['can_weight'][0]
        for b, j in zip(*np.nonzero(self.well)):
            assert set(idx[b, j].tolist()) == set(self.ref['can_idx'][b, j].tolist()), (b, j)
            exp_w = dict(zip(self.ref['can_idx'][b, j].tolist(), self.ref['can_weight'][b, j].tolist()))
            assert [exp_w[p] for p in idx[b, j].tolist()] == w[b, j].astype(np.float64).tolist(), (b, j)

    def run(self, be):
        from oracle.graph import NetConfig
        h = be.handle(NetConfig(1, 8, self.J, in_hw=self.in_hw), self.max_batch)
        xyz = be.vote(h, *self.maps)
        xyz_rep, got = vote_report(be, h, *self.maps, want=('can_idx', 'can_weight'))
        h.close()
        return xyz, xyz_rep, got

    def oracle(self):
        from oracle import pose
        with np.errstate(all='ignore'):
            return pose.estimate_pose_mm(*self.maps, out_hw=self.in_hw // 4)


@functools.lru_cache(maxsize=None)
def _seeded_cases():
    rng = np.random.default_rng(314159)                         # one generator through the three repetitions, as in the bit-exact test
    return [Case(_seeded_maps(rng, 4, 32, 7, 128), 128) for _ in range(3)]


def _assert_conditions(cases, what, max_share=None):
    """what keeps the comparison from hiding a failure: few joints left out, none of the crops left out altogether"""
    well = np.concatenate([c.well.reshape(-1) for c in cases])
    share = 1.0 - well.mean()
    print('\n%s: %d of %d joints ill-conditioned (%.2f %%)' % (what, (~well).sum(), well.size, 100 * share))
    assert max_share is None or share <= max_share
    for c in cases:
        assert c.well.any(axis=1).all(), 'a crop without a well-conditioned joint'
    return share


def test_seeded_generator_stays_well_conditioned():
    """CPU, before anything goes to a device: at most 5 % of the 84 joints ill-conditioned, every crop keeps one; and the oracle is
    held to the definition on the well-conditioned ones."""
    cases = _seeded_cases()
    _assert_conditions(cases, 'seeded 32x32 maps, 3 x (B = 4, J = 7)', max_share=0.05)
    worst = max(c.worst(c.oracle()) for c in cases)
    print('oracle/pose.py vs float64 definition: worst %.3g mm' % worst)
    assert worst < BAR_MM


def test_joints_against_the_fp64_definition(be):
    """dr_vote and dr_vote_report on the three repetitions: every well-conditioned joint within 5e-3 mm of the definition, its
    candidates the definition's pixels, its weights gathered from the definition's pixels."""
    cases = _seeded_cases()
    _assert_conditions(cases, 'seeded 32x32 maps', max_share=0.05)
    worst = 0.0
    for c in cases:
        xyz, xyz_rep, got = c.run(be)
        assert np.isfinite(xyz).all()
        worst = max(worst, c.worst(xyz), c.worst(xyz_rep))
        c.check_discrete(got)
    print('[%s] dr_vote vs float64 definition: worst %.3g mm' % (be.name, worst))
    assert worst < BAR_MM


# ---------------------------------------------------------------------------------------------
# (d) edges
# ---------------------------------------------------------------------------------------------
def _tiled_pixels(rng, J, m=128, tile=4096):
    """five winners per joint in at least three of the four 4096-pixel tiles (32 map rows each)"""
    pix = [[(r + int(rng.integers(0, 12))) * m + int(rng.integers(8, m - 8)) for r in rows]
           for rows in ([10, 40, 70, 100, 50], [104, 12, 76, 80, 36])[:J]]
    assert all(len({p // tile for p in pj}) >= 3 for pj in pix)
    return [pix]


@functools.lru_cache(maxsize=None)
def _shape_case(name):
    rng = np.random.default_rng({'J1': 11, 'J21': 12, 'B3_of_4': 13, '64x64': 14, '128x128_tiled': 15}[name])
    if name == 'J1':                                            # one live wave in the only workgroup; planted: two crops, two joints in all
        return Case(_planted_maps(rng, 2, 32, 1, _interior_pixels(rng, 2, 32, 1, 5)), 128)
    if name == 'J21':                                           # six workgroups per crop, one live wave in the last
        return Case(_seeded_maps(rng, 2, 32, 21, 128), 128)
    if name == 'B3_of_4':
        return Case(_seeded_maps(rng, 3, 32, 5, 128), 128, max_batch=4)
    if name == '64x64':                                         # 4096 pixels: the single launch's limit, every bit of the `taken` mask
        return Case(_planted_maps(rng, 1, 64, 3, _interior_pixels(rng, 1, 64, 3, 5)), 256)
    return Case(_planted_maps(rng, 1, 128, 2, _tiled_pixels(rng, 2)), 512)     # scan + merge launches


@pytest.mark.parametrize('name', ['J1', 'J21', 'B3_of_4', '64x64', '128x128_tiled'])
def test_edge_shapes(be, name):
    c = _shape_case(name)
    _assert_conditions([c], name)
    if name == '128x128_tiled':
        assert all(len(set((c.ref['can_idx'][0, j] // 4096).tolist())) >= 3 for j in range(c.J))
    w_oracle = c.worst(c.oracle())
    xyz, xyz_rep, got = c.run(be)
    worst = max(c.worst(xyz), c.worst(xyz_rep))
    print('[%s] %s: kernel worst %.3g mm, oracle worst %.3g mm' % (be.name, name, worst, w_oracle))
    assert w_oracle < BAR_MM and worst < BAR_MM
    c.check_discrete(got)


@functools.lru_cache(maxsize=None)
def _rule_case(name):
    B, m, J = 2, 32, 4
    rng = np.random.default_rng({'all_background': 21, 'all_out_of_range': 22, 'tied_scores': 23}[name])
    if name == 'all_background':                                # crop 0: every refined score ties at 0, the candidates are pixels 0 .. 4
        hm, hm3, um, ndm, cfg, com = _planted_maps(rng, B, m, J, _interior_pixels(rng, B, m, J, 5))
        ndm[0] = -1.0
        return Case((hm, hm3, um, ndm, cfg, com), 128, instead={'top5_gap': 'top5_gap_distinct'},
                    where=lambda ref: np.arange(B)[:, None] == np.zeros(J, int))
    if name == 'all_out_of_range':                              # joint (b, b): all five weights 0, an all-zero grid, its LAST cell, mass 0
        pushed = [[5 if j == b else 0 for j in range(J)] for b in range(B)]
        return Case(_planted_maps(rng, B, m, J, _interior_pixels(rng, B, m, J, 5), pushed_out=pushed), 128, instead={'start_gap': None},
                    where=lambda ref: ~ref['can_weight'].any(axis=2))
    # seven pixels share the best score exactly: the five lowest indices are the candidates
    pix = _interior_pixels(rng, B, m, J, 7)
    c = Case(_planted_maps(rng, B, m, J, pix, tie=True), 128, instead={'top5_gap': 'top5_gap_distinct'},
             where=lambda ref: ref['margins']['top5_gap'] == 0)
    c.planted = np.sort(np.array(pix), axis=2)
    return c


@pytest.mark.parametrize('name', ['all_background', 'all_out_of_range', 'tied_scores'])
def test_edge_rules(be, name):
    """The definition's stated result where an exact rule decides on exact ties, compared where every OTHER margin holds."""
    c = _rule_case(name)
    ref, B, J = c.ref, c.B, c.J
    if name == 'all_background':
        assert (ref['can_idx'][0] == np.arange(5)).all() and (ref['margins']['top5_gap'][0] == 0).all()
        assert c.well[0].any(), 'no joint of the all-background crop is compared'
    elif name == 'all_out_of_range':
        for b in range(B):
            assert not ref['can_weight'][b, b].any() and c.well[b, b]
            np.testing.assert_array_equal(ref['xyz_norm'][b, b], [0.75, 0.75, 0.75])      # the centre of cell (3, 3, 3), untouched
            np.testing.assert_array_equal(ref['xyz_mm'][b, b], 75.0 + c.maps[5][b].astype(np.float64))
            assert ref['margins']['start_gap'][b, b] == 0
    else:
        assert (np.sort(ref['can_idx'], axis=2) == c.planted[:, :, :5]).all() and (ref['margins']['top5_gap'] == 0).all()
        assert c.well.any(axis=1).all()
    w_oracle = c.worst(c.oracle())
    xyz, xyz_rep, got = c.run(be)
    worst = max(c.worst(xyz), c.worst(xyz_rep))
    print('[%s] %s: %d of %d joints compared, kernel worst %.3g mm, oracle worst %.3g mm'
          % (be.name, name, c.well.sum(), c.well.size, worst, w_oracle))
    assert w_oracle < BAR_MM and worst < BAR_MM
    c.check_discrete(got)
