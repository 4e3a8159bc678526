"""Image report (``dr_render_panels`` / ``dr_colormap``, ``densereg_amd/csrc/render.h``): colour-mapped map panels and joint plots
rendered on the device, against ``tests/render_ref.py`` -- the test's own numpy restatement of every fp32 and integer operation.

Every comparison of pixels is ``assert_array_equal``: an output byte is a pure function of integer and single-rounded fp32
operations, so there is no tolerance.  Kernel tests run on the host-fiber emulator and -- ``-m gpu`` -- on an MI355X.  Every call
of ``_render`` below also checks the sentinel bytes on both sides of the output buffer.
"""
import ctypes as C
import os

import numpy as np
import pytest

from densereg_amd import _lib
from tests import render_ref as R
from tests.common import GOLDEN, e2e_case

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]
PAD = 64                      # sentinel bytes on either side of the output (a multiple of 4: the output stays aligned)
SENTINEL = 0xA5


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


@pytest.fixture(scope='module')
def luts():
    z = np.load(os.path.join(GOLDEN, 'colormaps.npz'))
    assert z['jet'].shape == (256, 3) and z['greys'].shape == (256, 3) and z['jet'].dtype == np.uint8
    return z['jet'], z['greys']


class Src:
    """A panel's source on the device: ``view`` (B,h,w,C) is what the panel shows, a channel slice [lo:lo+C] of ``base``."""

    def __init__(self, be, base, lo=0, C_=None):
        self.base = np.ascontiguousarray(base, np.float32)
        self.lo, self.C = lo, self.base.shape[3] - lo if C_ is None else C_
        self.view = self.base[..., lo:lo + self.C]
        self.dev = be.dev(self.base)
        self.ptr = be.ptr(self.dev) + 4 * lo
        self.stride = self.base.shape[3]


def _panel(src, channel, kind, pts=None, space=R.PTS_NONE, pts_hw=0, skel=R.SKEL_NONE, cfg=None):
    return dict(src=src, channel=channel, kind=kind, pts=pts, space=space, pts_hw=pts_hw, skel=skel, cfg=cfg)


def _c_panels(be, panels, keep):
    arr = (_lib.DrPanel * len(panels))()
    for c, p in zip(arr, panels):
        s = p['src']
        c.src_dev, c.src_h, c.src_w, c.src_c, c.channel, c.kind = s.ptr, s.base.shape[1], s.base.shape[2], s.stride, p['channel'], p['kind']
        c.pts_space, c.pts_hw, c.skeleton = p['space'], p['pts_hw'], p['skel']
        if p['pts'] is not None:
            d = be.dev(np.ascontiguousarray(p['pts'], np.float32))
            keep.append(d)
            c.pts_dev, c.num_pts = be.ptr(d), p['pts'].shape[1]
        if p['cfg'] is not None:
            d = be.dev(np.ascontiguousarray(p['cfg'], np.float32))
            keep.append(d)
            c.cfg_dev = be.ptr(d)
    return arr


def _render(be, panels, B, out_hw):
    """dr_render_panels into a buffer with sentinels on both sides -> (B,P,out_hw,out_hw,3) uint8"""
    keep = []
    arr = _c_panels(be, panels, keep)
    n = B * len(panels) * out_hw * out_hw * 3
    buf = be.dev(np.full(n + 2 * PAD, SENTINEL, np.uint8))
    rc = be.lib.dr_render_panels(B, arr, len(panels), out_hw, be.ptr(buf) + PAD, be.stream)
    assert rc == 0, rc
    be.sync()
    got = be.host(buf)
    assert (got[:PAD] == SENTINEL).all() and (got[PAD + n:] == SENTINEL).all(), 'the kernel wrote outside (B,P,out_hw,out_hw,3)'
    return got[PAD:PAD + n].reshape(B, len(panels), out_hw, out_hw, 3).copy()


def _expect(panels, B, out_hw, luts):
    out = np.empty((B, len(panels), out_hw, out_hw, 3), np.uint8)
    for b in range(B):
        for i, p in enumerate(panels):
            out[b, i] = R.render_panel(p['src'].view[b], p['channel'], p['kind'], luts, out_hw,
                                       None if p['pts'] is None else p['pts'][b], p['space'], p['pts_hw'], p['skel'],
                                       None if p['cfg'] is None else p['cfg'][b])
    return out


# ---------------------------------------------------------------------------------------------
# 1. colour tables
# ---------------------------------------------------------------------------------------------
def test_colormap_tables_equal_the_fixture(be, luts):
    for kind in (R.JET, R.GREYS):
        lut = np.zeros((256, 3), np.uint8)
        assert be.lib.dr_colormap(kind, lut.ctypes.data) == 0
        np.testing.assert_array_equal(lut, luts[kind])
    assert be.lib.dr_colormap(R.UM_XY, lut.ctypes.data) == -1 and be.lib.dr_colormap(R.JET, None) == -1


def test_ramp_renders_every_table_row(be, luts):
    """a 16x16 source holding 0..255 (shuffled) hits every index once: the output is the table, permuted the same way"""
    perm = np.random.default_rng(1).permutation(256)
    ramp = perm.astype(np.float32).reshape(1, 16, 16, 1)
    src = Src(be, ramp)
    got = _render(be, [_panel(src, 0, R.JET), _panel(src, 0, R.GREYS)], 1, 16)
    for kind in (R.JET, R.GREYS):
        np.testing.assert_array_equal(got[0, kind].reshape(256, 3), luts[kind][perm])
    np.testing.assert_array_equal(got, _expect([_panel(src, 0, R.JET), _panel(src, 0, R.GREYS)], 1, 16, luts))


def test_fixture_is_what_the_generator_script_produces(luts):
    """regenerates data where matplotlib imports (the product check above does not depend on it)"""
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_colormaps', os.path.join(GOLDEN, 'make_colormaps.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t = mod.tables()
    np.testing.assert_array_equal(t['jet'], luts[0])
    np.testing.assert_array_equal(t['greys'], luts[1])


# ---------------------------------------------------------------------------------------------
# 2. vis_sin
# ---------------------------------------------------------------------------------------------
def _sin_args():
    rng = np.random.default_rng(2)
    special = np.array([1.0, -1.0, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, np.nextafter(np.float32(1), np.float32(0)),
                        0.5, -0.5], np.float32)
    x = np.concatenate([special, np.linspace(-1, 1, 2048, dtype=np.float32), rng.uniform(-1, 1, 4096 - 2048 - special.size).astype(np.float32)])
    assert x.size == 4096
    return x


def test_vis_sin_bits(be):
    x = _sin_args()
    d_x, d_y = be.dev(x), be.empty((x.size,))
    assert be.dbg.dr_dbg_vis_sin(be.ptr(d_x), x.size, be.ptr(d_y), be.stream) == 0
    be.sync()
    np.testing.assert_array_equal(be.host(d_y).view(np.uint32), R.vis_sin(x).view(np.uint32))
    assert be.dbg.dr_dbg_vis_sin(None, 4, be.ptr(d_y), be.stream) == -1 and be.dbg.dr_dbg_vis_sin(be.ptr(d_x), 0, be.ptr(d_y), be.stream) == -1


def test_vis_sin_is_a_sine():
    """Taylor remainder 1/11! = 2.5e-8 on [-1, 1] plus a few fp32 roundings (6e-8 each at most): 1e-6, far below half a colour
    step (1/512)"""
    x = _sin_args()
    assert np.abs(R.vis_sin(x).astype(np.float64) - np.sin(x.astype(np.float64))).max() < 1e-6


# ---------------------------------------------------------------------------------------------
# 3. map panels
# ---------------------------------------------------------------------------------------------
SHAPES = [(8, 32), (12, 36), (32, 128), (64, 64), (128, 128), (32, 16)]


def _poison(rng, a, share=0.02):
    """NaN, +Inf and -Inf sprinkled over a copy of a"""
    a = a.copy()
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, max(3, int(share * flat.size)), replace=False)
    flat[idx[0::3]] = np.nan
    flat[idx[1::3]] = np.inf
    flat[idx[2::3]] = -np.inf
    return a


@pytest.mark.parametrize('hw,out_hw', SHAPES, ids=['%dto%d' % s for s in SHAPES])
@pytest.mark.parametrize('kind', [R.JET, R.GREYS, R.UM_XY], ids=['jet', 'greys', 'um_xy'])
def test_map_panels(be, luts, hw, out_hw, kind):
    """B = 2; strided views (the channel in the middle of 7; the 15 offset channels of J = 5 inside 17); NaN and +-Inf; a constant map
    (crop 0) and an all-NaN map (crop 1); for UM_XY pixels with x = y = 0 on both sides of the 0.1 test"""
    rng = np.random.default_rng(100 * hw + out_hw + kind)
    B = 2
    if kind == R.UM_XY:
        base = rng.standard_normal((B, hw, hw, 17)).astype(np.float32)
        um = base[..., 1:16]
        n = np.sqrt((um.reshape(B, hw, hw, 5, 3) ** 2).sum(-1, keepdims=True))
        um[...] = (um.reshape(B, hw, hw, 5, 3) / n * rng.uniform(0, 1.2, (B, hw, hw, 5, 1))).reshape(B, hw, hw, 15).astype(np.float32)
        um[:, 0, :4, 6:8] = 0.0                               # joint 2: x = y = 0 ...
        um[:, 0, :2, 8] = [0.3, -0.31]                        # ... z*z < 0.1: drawn as 1
        um[:, 0, 2:4, 8] = [0.32, -0.9]                       # ... z*z >= 0.1: 0/0, drawn white
        um[:, 1, 0, 6:9] = [0.0, 0.0, 0.0]
        base[..., 1:16] = _poison(rng, um)
        flat = np.full((B, hw, hw, 17), 0.25, np.float32)
        flat[1] = np.nan
        a, b_, ch = Src(be, base, 1, 15), Src(be, flat, 1, 15), 2
    else:
        base = _poison(rng, (rng.standard_normal((B, hw, hw, 7)) * 3).astype(np.float32))
        flat = rng.standard_normal((B, hw, hw, 7)).astype(np.float32)
        flat[0, ..., 3] = -1.5
        flat[1, ..., 3] = np.nan
        a, b_, ch = Src(be, base), Src(be, flat), 3
    panels = [_panel(a, ch, kind), _panel(b_, ch, kind)]
    got = _render(be, panels, B, out_hw)
    want = _expect(panels, B, out_hw, luts)
    np.testing.assert_array_equal(got, want)
    lut = luts[1 if kind == R.GREYS else 0]
    assert (got[0, 1] == lut[0]).all() and (got[1, 1] == 255).all()        # constant map: t = 0; all-NaN map: white
    if kind == R.UM_XY and out_hw >= hw:
        f = out_hw // hw                                                    # x = y = 0 and z*z >= 0.1: 0/0, white whatever else is poisoned
        assert (got[:, 0, 0, 2 * f] == 255).all() and (got[:, 0, 0, 3 * f] == 255).all()


# ---------------------------------------------------------------------------------------------
# 4. overlays
# ---------------------------------------------------------------------------------------------
def _hand(rng, B, J, pts_hw):
    """joints spread over the image, some on the border, outside and NaN, two coincident"""
    p = np.zeros((B, J, 3), np.float32)
    p[..., :2] = rng.uniform(0.1 * pts_hw, 0.9 * pts_hw, (B, J, 2))
    p[..., 2] = rng.uniform(300, 500, (B, J))
    p[:, 1, :2] = [0.0, pts_hw - 1.0]                          # on the border
    p[:, 2, :2] = [-2.5, -40.0]                                # outside
    p[0, 3, 0] = np.nan                                        # NaN: every primitive that uses it is skipped
    p[:, 5, :2] = p[:, 4, :2]                                  # coincident (joined by a bone in icvl 4-5, nyu 4-5, msra 5-6 ... and a disc pair)
    p[1, 6, 1] = np.inf
    return p


@pytest.mark.parametrize('skel,J', [(R.SKEL_ICVL, 16), (R.SKEL_NYU, 14), (R.SKEL_MSRA, 21), (R.SKEL_NONE, 7)], ids=['icvl', 'nyu', 'msra', 'none7'])
@pytest.mark.parametrize('pts_hw,out_hw', [(128, 128), (32, 128), (128, 64), (32, 64)])
def test_overlay_uvd(be, luts, skel, J, pts_hw, out_hw):
    rng = np.random.default_rng(7 * J + pts_hw + out_hw)
    B = 2
    src = Src(be, rng.uniform(0, 1, (B, 16, 16, 1)).astype(np.float32))
    pts = _hand(rng, B, J, pts_hw)
    if skel == R.SKEL_MSRA:
        pts[:, 6, :2] = pts[:, 5, :2]
    panels = [_panel(src, 0, R.GREYS, pts, R.PTS_UVD, pts_hw, skel)]
    got = _render(be, panels, B, out_hw)
    np.testing.assert_array_equal(got, _expect(panels, B, out_hw, luts))
    bare = _render(be, [_panel(src, 0, R.GREYS)], B, out_hw)
    assert (got != bare).any(axis=-1).sum() >= 4 * B            # something was drawn (a smallest disc alone covers 9 pixels at 64)


def test_overlay_xyz_is_the_vote_reports_projection(be, luts):
    """DR_PTS_XYZ_MM against render_ref's projection; and the projection is dr_vote_report's: for the joints the vote returns in mm,
    render_ref's (u, v) have the bits of the report's uvd, and both ways of handing them over draw the same bytes"""
    from densereg_amd.data.synthetic import make_crops
    rng = np.random.default_rng(5)
    B, J, m = 2, 14, 32
    dm, poses, cfgs, coms, _ = make_crops(B, 'nyu', seed=17)
    h = _lib.Handle(be.lib, 1, 8, J, 128, 3, B, 0, False)
    ndm = be.norm_dm(h, dm, coms)
    hm = rng.uniform(0, 1, (B, m, m, J)).astype(np.float32)
    hm3 = rng.uniform(0, 1, (B, m, m, J)).astype(np.float32)
    um = rng.standard_normal((B, m, m, 3 * J)).astype(np.float32)
    args = [be.dev(np.ascontiguousarray(a, np.float32)) for a in (hm, hm3, um, ndm, cfgs, coms)]
    xyz, uvd = be.empty((B, 3 * J)), be.empty((B, J, 3))
    rep = _lib.DrVoteReport()
    rep.uvd_dev = be.ptr(uvd)
    h.call('dr_vote_report', B, *[be.ptr(a) for a in args], be.ptr(xyz), C.byref(rep), be.stream)
    be.sync()
    xyz, uvd = be.host(xyz).reshape(B, J, 3).copy(), be.host(uvd).copy()
    h.close()
    for b in range(B):
        np.testing.assert_array_equal(R.project(cfgs[b], xyz[b]).view(np.uint32), uvd[b, :, :2].view(np.uint32))
    src = Src(be, dm.reshape(B, 128, 128, 1))
    for pts in (xyz, poses.reshape(B, J, 3)):
        panels = [_panel(src, 0, R.GREYS, pts, R.PTS_XYZ_MM, 128, R.SKEL_NYU, cfgs)]
        got = _render(be, panels, B, 128)
        np.testing.assert_array_equal(got, _expect(panels, B, 128, luts))
    by_uvd = _render(be, [_panel(src, 0, R.GREYS, uvd, R.PTS_UVD, 128, R.SKEL_NYU)], B, 128)
    by_xyz = _render(be, [_panel(src, 0, R.GREYS, xyz, R.PTS_XYZ_MM, 128, R.SKEL_NYU, cfgs)], B, 128)
    np.testing.assert_array_equal(by_uvd, by_xyz)
    zero_z = poses.reshape(B, J, 3).copy()
    zero_z[:, ::2, 2] = 0.0                                    # z = 0: a non-finite projection, skipped
    panels = [_panel(src, 0, R.GREYS, zero_z, R.PTS_XYZ_MM, 128, R.SKEL_NYU, cfgs)]
    np.testing.assert_array_equal(_render(be, panels, B, 128), _expect(panels, B, 128, luts))


# ---------------------------------------------------------------------------------------------
# 5. bounds
# ---------------------------------------------------------------------------------------------
def test_sixteen_panels_equal_sixteen_calls(be, luts):
    rng = np.random.default_rng(9)
    B = 2
    a = Src(be, _poison(rng, rng.standard_normal((B, 12, 12, 7)).astype(np.float32)))
    um = Src(be, rng.standard_normal((B, 8, 8, 17)).astype(np.float32), 1, 15)
    big = Src(be, rng.standard_normal((B, 20, 20, 1)).astype(np.float32))
    pts = _hand(rng, B, 16, 32)
    panels = []
    for i in range(16):
        if i % 4 == 0:
            panels.append(_panel(um, i // 4, R.UM_XY))
        elif i % 4 == 1:
            panels.append(_panel(big, 0, R.GREYS, pts, R.PTS_UVD, 32, R.SKEL_ICVL if i == 5 else R.SKEL_NONE))
        else:
            panels.append(_panel(a, i % 7, R.JET if i % 4 == 2 else R.GREYS))
    together = _render(be, panels, B, 24)
    np.testing.assert_array_equal(together, _expect(panels, B, 24, luts))
    for i, p in enumerate(panels):
        np.testing.assert_array_equal(_render(be, [p], B, 24)[:, 0], together[:, i], err_msg='panel %d' % i)


# ---------------------------------------------------------------------------------------------
# 6. argument checks
# ---------------------------------------------------------------------------------------------
def test_argument_checks(be):
    B = 1
    src = Src(be, np.zeros((B, 8, 8, 7), np.float32))
    big = Src(be, np.zeros((B, 130, 130, 1), np.float32))
    pts16 = np.zeros((B, 16, 3), np.float32) + 4
    cfg = np.array([[200.0, 200.0, 4.0, 4.0, 8.0, 8.0]], np.float32)
    out = be.dev(np.zeros(16 * 16 * 16 * 3 + 8, np.uint8))
    keep = []

    def rc(panels, B=1, n=None, out_hw=16, o=be.ptr(out), null_panels=False):
        arr = _c_panels(be, panels, keep)
        return be.lib.dr_render_panels(B, None if null_panels else arr, len(panels) if n is None else n, out_hw, o, be.stream)

    good = _panel(src, 3, R.JET, pts16, R.PTS_UVD, 8, R.SKEL_ICVL)
    assert rc([good]) == 0
    assert rc([good], null_panels=True) == -1 and rc([good], o=None) == -1 and rc([good], o=be.ptr(out) + 1) == -1
    assert rc([good], B=0) == -1 and rc([good], B=-1) == -1
    assert rc([good], n=0) == -1 and rc([good] * 16, n=17) == -1 and rc([good] * 16) == 0
    for bad_hw in (0, -4, 6, 18, 516):
        assert rc([good], out_hw=bad_hw) == -1, bad_hw
    assert rc([_panel(src, 7, R.JET)]) == -1 and rc([_panel(src, -1, R.JET)]) == -1 and rc([_panel(src, 6, R.GREYS)]) == 0
    assert rc([_panel(src, 2, R.UM_XY)]) == -1 and rc([_panel(src, 1, R.UM_XY)]) == 0            # 3*2 + 2 >= 7
    assert rc([_panel(src, 0, 3)]) == -1
    assert rc([_panel(src, 0, R.GREYS, pts16, R.PTS_XYZ_MM, 8, R.SKEL_ICVL)]) == -1                 # no cfg
    assert rc([_panel(src, 0, R.GREYS, pts16, R.PTS_XYZ_MM, 8, R.SKEL_ICVL, cfg)]) == 0
    assert rc([_panel(src, 0, R.GREYS, pts16, R.PTS_UVD, 8, R.SKEL_NYU)]) == -1                     # 14 joints wanted
    assert rc([_panel(src, 0, R.GREYS, pts16, R.PTS_UVD, 8, R.SKEL_MSRA)]) == -1
    assert rc([_panel(src, 0, R.GREYS, pts16, R.PTS_UVD, 8, 4)]) == -1 and rc([_panel(src, 0, R.GREYS, pts16, 3, 8)]) == -1
    assert rc([_panel(src, 0, R.GREYS, pts16, R.PTS_UVD, 0)]) == -1 and rc([_panel(src, 0, R.GREYS, pts16, R.PTS_UVD, -8)]) == -1
    assert rc([_panel(src, 0, R.GREYS, None, R.PTS_UVD, 8)]) == -1                                  # points announced, none given
    null_src = _c_panels(be, [good], keep)
    null_src[0].src_dev = None
    assert be.lib.dr_render_panels(1, null_src, 1, 16, be.ptr(out), be.stream) == -1
    for field in ('src_h', 'src_w', 'src_c'):
        neg = _c_panels(be, [good], keep)
        setattr(neg[0], field, -8)
        assert be.lib.dr_render_panels(1, neg, 1, 16, be.ptr(out), be.stream) == -1, field
    assert rc([_panel(big, 0, R.JET)]) == -2                                                        # 130 x 130 > 16384 pixels
    be.sync()


# ---------------------------------------------------------------------------------------------
# 7. model level
# ---------------------------------------------------------------------------------------------
LEVEL_TAGS = {1: {'val_pts', 'gt_pts'},
              2: {'val_pts', 'gt_pts', 'gt_hm', 'gt_hm3', 'val_hm', 'val_hm3', 'val_dm', 'val_pts_hm'},
              3: {'val_pts', 'gt_pts', 'gt_hm', 'gt_hm3', 'val_hm', 'val_hm3', 'val_dm', 'val_pts_hm', 'gt_xy', 'gt_z', 'val_xy', 'val_z'}}
TRA_TAGS = {'tra_pts', 'tra_gt_pts', 'tra_gt_hm', 'tra_gt_hm3', 'tra_hm', 'tra_hm3', 'tra_dm', 'tra_pts_hm', 'tra_gt_xy', 'tra_gt_z',
            'tra_xy', 'tra_z'}


@pytest.mark.gpu
def test_model_summary_images(gpu, luts):
    """the committed S=1 / F=64 / J=16 case: tag sets by level, val_hm against render_ref on forward_eval's maps, gt_pts against
    render_ref on the ground-truth pose; the tra_ set on a training engine"""
    import torch
    from densereg_amd import flags
    from densereg_amd.model import hourglass_um_crop_tiny as M
    from densereg_amd.network import um_v1
    cfg, params, g = e2e_case()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu.device)
    args = (t(g['dm']), t(g['pose']), t(g['cfg']), t(g['com']))
    try:
        flags.parse(['--dataset', 'icvl', '--num_stack', '1', '--fea_num', '64', '--is_train', 'False', '--batch_size', '1', '--debug_level', '2'])
        eng = um_v1.get_engine(16, 128, 1, 0, False)
        eng.load_params(params)
        np.testing.assert_array_equal(eng.colormap('jet'), luts[0])
        np.testing.assert_array_equal(eng.colormap('greys'), luts[1])
        model = M.JointDetectionModel(M.SyntheticDataset('icvl', 'testing'), um_v1.detect_net, epoch=1)
        assert model.summary_images(*args, level=0) == {}
        assert set(model.summary_images(*args)) == LEVEL_TAGS[2]                     # level defaults to --debug_level
        for level in (1, 2, 3):
            imgs = model.summary_images(*args, level=level)
            assert set(imgs) == LEVEL_TAGS[level]
            assert all(v.dtype == torch.uint8 and tuple(v.shape) == (1, 128, 128, 3) for v in imgs.values())
        hm, hm3, um = eng.forward_eval(eng.norm_dm(args[0], args[3]))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(imgs['val_hm'][0].cpu().numpy(), R.render_panel(hm[0].cpu().numpy(), 0, R.JET, luts, 128))
        np.testing.assert_array_equal(imgs['val_z'][0].cpu().numpy(), R.render_panel(um[0].cpu().numpy(), 2, R.JET, luts, 128))
        np.testing.assert_array_equal(imgs['val_xy'][0].cpu().numpy(), R.render_panel(um[0].cpu().numpy(), 0, R.UM_XY, luts, 128))
        want = R.render_panel(g['dm'][0], 0, R.GREYS, luts, 128, g['pose'].reshape(16, 3), R.PTS_XYZ_MM, 128, R.SKEL_ICVL, g['cfg'][0])
        np.testing.assert_array_equal(imgs['gt_pts'][0].cpu().numpy(), want)
        np.testing.assert_array_equal(imgs['val_dm'][0].cpu().numpy(), R.render_panel(g['dm'][0], 0, R.GREYS, luts, 128))
        assert imgs['val_pts'].shape == imgs['gt_pts'].shape and (imgs['val_pts'] != imgs['val_dm']).any()
        # Engine.render on a channel-slice view, and its checks
        from densereg_amd.engine import Panel
        view = um[..., 3:6]
        one = eng.render([Panel(view, 2), Panel(view, 0, 'um_xy')], out_hw=64)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(one[0, 0].cpu().numpy(), R.render_panel(um[0].cpu().numpy(), 5, R.JET, luts, 64))
        np.testing.assert_array_equal(one[0, 1].cpu().numpy(), R.render_panel(um[0].cpu().numpy(), 1, R.UM_XY, luts, 64))
        with pytest.raises(ValueError):
            eng.render([Panel(view, 3)])
        with pytest.raises(ValueError):
            eng.render([])
        # training: the maps of the most recent forward, tra_ tags
        flags.parse(['--dataset', 'icvl', '--num_stack', '1', '--fea_num', '64', '--is_train', 'True', '--batch_size', '1', '--sub_batch', '1'])
        teng = um_v1.get_engine(16, 128, 1, 0, True)
        teng.load_params(params)
        tmodel = M.JointDetectionModel(M.SyntheticDataset('icvl', 'training'), um_v1.detect_net, epoch=1)
        teng.forward_train(teng.norm_dm(args[0], args[3]), dropout_mode=0)
        timgs = tmodel.summary_images(*args, level=3, train=True)
        assert set(timgs) == TRA_TAGS
        thm, _, _ = teng.read_maps(1, 0)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(timgs['tra_hm'][0].cpu().numpy(), R.render_panel(thm[0].cpu().numpy(), 0, R.JET, luts, 128))
        np.testing.assert_array_equal(timgs['tra_gt_pts'][0].cpu().numpy(), want)
    finally:
        flags.parse([])


# ---------------------------------------------------------------------------------------------
# 8. driver
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_driver_image_every(gpu, tmp_path, monkeypatch):
    """run_test --image_every 1 --num_frames 4 writes <train_dir>/summary/<tag>/<step>_<crop>.png, each the bytes summary_images
    returns; --image_every 0 (the default) writes no summary directory"""
    import torch
    from densereg_amd import flags
    from densereg_amd.data.png import decode_png
    from densereg_amd.model import hourglass_um_crop_tiny as M
    from densereg_amd.network import um_v1
    monkeypatch.chdir(tmp_path)
    base = ['--dataset', 'icvl', '--num_stack', '1', '--fea_num', '32', '--is_train', 'False', '--batch_size', '4', '--num_frames', '4',
            '--debug_level', '2']
    try:
        flags.parse(base)
        eng = um_v1.get_engine(16, 128, 4, 0, False)
        eng.load_params(M._random_params(eng))
        ds, vs = M.SyntheticDataset('icvl', 'training'), M.SyntheticDataset('icvl', 'testing')
        model, _, _ = M.run_test(ds, vs)
        assert not os.path.exists(os.path.join(model.train_dir, 'summary'))
        flags.parse(base + ['--image_every', '1'])
        model, _, out = M.run_test(ds, vs)
        assert len(open(out).read().splitlines()) == 4
        dm, poses, cfgs, coms, _ = vs.batch(4, 0)
        imgs = model.summary_images(model._t(dm), model._t(poses), model._t(cfgs), model._t(coms))
        torch.cuda.synchronize()
        root = os.path.join(model.train_dir, 'summary')
        assert set(os.listdir(root)) == LEVEL_TAGS[2]
        for tag in LEVEL_TAGS[2]:
            assert sorted(os.listdir(os.path.join(root, tag))) == ['0_%d.png' % c for c in range(4)]
            for c in range(4):
                info, samples = decode_png(open(os.path.join(root, tag, '0_%d.png' % c), 'rb').read())
                assert (info.width, info.height, info.channels, info.bit_depth) == (128, 128, 3, 8)
                np.testing.assert_array_equal(samples.reshape(128, 128, 3), imgs[tag][c].cpu().numpy(), err_msg='%s %d' % (tag, c))
    finally:
        flags.parse([])
