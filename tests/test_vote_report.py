"""The vote report (``dr_vote_report`` / ``dr_infer_report``, ``vote_report_kernel``): everything the reference's test graph
exposes next to the joints -- uvd joints, the five candidates per joint, their point-cloud positions, their weights, the
heat-map-only peak -- plus the mean-shift kernel mass, all written by the vote's own launch.

Every member is held to the bar of the vote itself: BIT-EXACT against the oracle's restatement (``oracle/pose.py``) on identical
maps, on the host-fiber emulator (``[emu]``) and on the MI355X (``[gpu]``).  The expected values are computed at test time; no
new golden files.
"""
import ctypes as C

import numpy as np
import pytest

from densereg_amd import _lib
from tests.common import e2e_case, golden

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


FIELDS = tuple(_lib.VOTE_REPORT_FIELDS)           # xyz_norm uvd can_idx can_score can_pts ori_pts can_weight mass hm_peak
SENT = -777                                        # exactly representable in fp32 and int32; no member can take it on these inputs
GUARD = 24                                         # elements behind every payload that must stay untouched


def _shape(name, B, J):
    return (B, J) + tuple(_lib.VOTE_REPORT_FIELDS[name][0])


def _dtype(name):
    return np.int32 if _lib.VOTE_REPORT_FIELDS[name][1] else np.float32


class ReportBuffers:
    """All nine device buffers, pre-filled with the sentinel and over-allocated by a guard tail; ``struct(want)`` names only the
    wanted ones to the library."""

    def __init__(self, be, B, J):
        self.be, self.B, self.J = be, B, J
        self.dev = {n: be.dev(np.full(int(np.prod(_shape(n, B, J))) + GUARD, SENT, _dtype(n))) for n in FIELDS}

    def struct(self, want):
        rep = _lib.DrVoteReport()
        for n in FIELDS:
            setattr(rep, n + '_dev', self.be.ptr(self.dev[n]) if n in want else None)
        return rep

    def read(self):
        """name -> (payload in its shape, guard tail)"""
        out = {}
        for n in FIELDS:
            a = np.array(self.be.host(self.dev[n]))
            out[n] = (a[:-GUARD].reshape(_shape(n, self.B, self.J)), a[-GUARD:])
        return out


def _check_written(got, want):
    """Requested buffers fully written (no sentinel left), guard tails and non-requested buffers untouched."""
    for n in FIELDS:
        payload, tail = got[n]
        assert (tail == SENT).all(), '%s: guard tail written' % n
        if n in want:
            assert not (payload == SENT).any(), '%s: sentinel left in the payload' % n
        else:
            assert (payload == SENT).all(), '%s: written although not requested' % n


def vote_report(be, h, hm, hm3, um, ndm, cfg, com, want=FIELDS):
    B, J = ndm.shape[0], h.cfg.num_jnt
    bufs = ReportBuffers(be, B, J)
    xyz = be.dev(np.full((B, 3 * J), SENT, np.float32))
    args = [be.dev(np.ascontiguousarray(a, np.float32)) for a in (hm, hm3, um, ndm, cfg, com)]
    rep = bufs.struct(want)
    h.call('dr_vote_report', B, *[be.ptr(a) for a in args], be.ptr(xyz), C.byref(rep), be.stream)
    be.sync()
    got = bufs.read()
    _check_written(got, want)
    return np.array(be.host(xyz)), got


def infer_report(be, h, ndm, cfg, com, want=FIELDS):
    B, J = ndm.shape[0], h.cfg.num_jnt
    bufs = ReportBuffers(be, B, J)
    xyz = be.dev(np.full((B, 3 * J), SENT, np.float32))
    args = [be.dev(np.ascontiguousarray(a, np.float32)) for a in (ndm, cfg, com)]
    rep = bufs.struct(want)
    h.call('dr_infer_report', B, *[be.ptr(a) for a in args], be.ptr(xyz), C.byref(rep), be.stream)
    be.sync()
    got = bufs.read()
    _check_written(got, want)
    return np.array(be.host(xyz)), got


# ---------------------------------------------------------------------------------------------
# the oracle's side: every member from oracle/pose.py, fp32 operation by operation
# ---------------------------------------------------------------------------------------------
def expected_report(hm, hm3, um, ndm, cfg, com):
    from oracle import pose
    f32 = np.float32
    hm, hm3, um, ndm, cfg, com = (np.asarray(a, f32) for a in (hm, hm3, um, ndm, cfg, com))
    B, m, _, J = hm.shape
    s = ndm.shape[1] // m
    tiny = ndm[:, ::s, ::s, :]
    with np.errstate(all='ignore'):
        n, dbg = pose.xyz_estimation(hm, pose.resume_om(hm3, um), hm3, tiny, cfg, com, return_debug=True)
        xyz_mm = pose.unnorm_xyz_pose(n.reshape(B, -1), com)
        refined = (hm + f32(1.0)) * hm3
        refined = refined * np.where(tiny < f32(-0.99), f32(0), f32(1))
        cloud = pose.generate_xyzs(tiny, cfg, com)
        idx = dbg['idx']
        exp = {'xyz_norm': n, 'can_idx': idx.astype(np.int32), 'can_pts': dbg['can'], 'can_weight': dbg['w'],
               'can_score': np.zeros((B, J, 5), f32), 'ori_pts': np.zeros((B, J, 5, 3), f32), 'uvd': np.zeros((B, J, 3), f32),
               'mass': np.zeros((B, J), f32), 'hm_peak': np.zeros((B, J, 3), f32)}
        for b in range(B):
            exp['uvd'][b] = pose.xyz2uvd(xyz_mm[b], cfg[b, :4])
            for j in range(J):
                exp['can_score'][b, j] = refined[b].reshape(-1, J)[idx[b, j], j]
                exp['ori_pts'][b, j] = cloud[b].reshape(-1, 3)[idx[b, j]]
                c, can, w = n[b, j], dbg['can'][b, j], dbg['w'][b, j]
                ss = f32(0)
                for i in range(5):
                    d0, d1, d2 = f32(can[i, 0] - c[0]), f32(can[i, 1] - c[1]), f32(can[i, 2] - c[2])
                    sq = f32(f32(f32(d0 * d0) + f32(d1 * d1)) + f32(d2 * d2))
                    ss = f32(ss + f32(pose.exp_f32(f32(f32(-3.125) * sq)) * w[i]))
                exp['mass'][b, j] = ss
                flat = hm[b, :, :, j].reshape(-1)
                i = int(np.argmax(flat))                                    # first index of the maximum
                exp['hm_peak'][b, j] = (i % m, i // m, flat[i])
    return xyz_mm, exp


def _assert_report_equal(got, exp, what=''):
    for n in FIELDS:
        np.testing.assert_array_equal(got[n][0], exp[n], err_msg='%s %s' % (what, n))


def _seeded_maps(rng, B, m, J, in_hw):
    """The generator of test_forward_parity.py::test_vote_seeded_random_maps: smooth bumps + noise, a third of the pixels background,
    cameras and centres of mass in the range of the synthetic crops (focal lengths and principal point follow the crop side)."""
    yy, xx = np.mgrid[0:m, 0:m].astype(np.float32)
    hm = 0.05 * rng.standard_normal((B, m, m, J)).astype(np.float32)
    hm3 = np.abs(0.05 * rng.standard_normal((B, m, m, J))).astype(np.float32)
    for b in range(B):
        for j in range(J):
            for _ in range(int(rng.integers(1, 4))):
                cy, cx, a = rng.uniform(3, m - 3), rng.uniform(3, m - 3), rng.uniform(0.3, 1.0)
                bump = (a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * rng.uniform(1.0, 3.0) ** 2))).astype(np.float32)
                hm[b, :, :, j] += bump
                hm3[b, :, :, j] += bump * np.float32(rng.uniform(0.5, 1.0))
    um = (0.3 * rng.standard_normal((B, m, m, 3 * J))).astype(np.float32)
    tiny = rng.uniform(-0.4, 0.9, (B, m, m, 1)).astype(np.float32)
    tiny[rng.random((B, m, m, 1)) < 0.33] = -1.0
    ndm = np.repeat(np.repeat(tiny, 4, axis=1), 4, axis=2).astype(np.float32)
    k = in_hw / 128.0
    cfg = np.stack([[rng.uniform(380, 720) * k, rng.uniform(380, 720) * k, in_hw / 2 + rng.normal(0, 3), in_hw / 2 + rng.normal(0, 3),
                     in_hw, in_hw] for _ in range(B)]).astype(np.float32)
    com = np.stack([[rng.normal(0, 40), rng.normal(0, 40), rng.uniform(250, 900)] for _ in range(B)]).astype(np.float32)
    return hm, hm3, um, ndm, cfg, com


# ---------------------------------------------------------------------------------------------
# 1. seeded random maps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_hw,B,J', [(128, 3, 7), (256, 2, 5)], ids=['32x32_B3_J7', '64x64_B2_J5'])
def test_report_seeded_random_maps(be, in_hw, B, J):
    """32x32 maps with J = 7 (the last workgroup runs three of its four waves) and 64x64 maps = 4096 pixels (the LDS plan's
    limit: 64 pixels per lane, every bit of the `taken` mask in use): every member bit for bit, xyz_mm equal to dr_vote's."""
    from oracle.graph import NetConfig
    m = in_hw // 4
    maps = _seeded_maps(np.random.default_rng(271828 + in_hw), B, m, J, in_hw)
    hm = maps[0]
    flat = hm.reshape(B, m * m, J)
    assert ((flat == flat.max(axis=1, keepdims=True)).sum(axis=1) == 1).all()      # unique maxima: the tie rule is test 2's
    xyz_exp, exp = expected_report(*maps)
    h = be.handle(NetConfig(1, 8, J, in_hw=in_hw), B)
    xyz, got = vote_report(be, h, *maps)
    xyz_plain = be.vote(h, *maps)
    h.close()
    _assert_report_equal(got, exp)
    np.testing.assert_array_equal(xyz, xyz_plain)
    np.testing.assert_array_equal(xyz, xyz_exp)
    assert np.isfinite(got['mass'][0]).all() and np.isfinite(got['uvd'][0]).all()


# ---------------------------------------------------------------------------------------------
# 2. crafted cases
# ---------------------------------------------------------------------------------------------
def test_report_crafted_cases(be):
    """Planted peaks / exact ties / negative weights / out-of-range re-projection / all-background (tests/golden/vote_cases.npz,
    read-only): can_idx is the file's idx, xyz_mm the file's xyz, every other member the oracle's; a NaN in uvd (z = 0)
    compares equal to the oracle's NaN."""
    from oracle.graph import NetConfig
    g = golden('vote_cases.npz')
    hm, hm3, um = (g[k].astype(np.float32) for k in ('hm', 'hm3', 'um'))
    B, m, _, J = hm.shape
    ndm = np.repeat(np.repeat(g['tiny'], 4, axis=1), 4, axis=2).astype(np.float32)
    cfg, com = g['cfg'].astype(np.float32), g['com'].astype(np.float32)
    xyz_exp, exp = expected_report(hm, hm3, um, ndm, cfg, com)
    h = be.handle(NetConfig(1, 8, J), B)
    xyz, got = vote_report(be, h, hm, hm3, um, ndm, cfg, com)
    h.close()
    np.testing.assert_array_equal(got['can_idx'][0], g['idx'])
    _assert_report_equal(got, exp)
    np.testing.assert_array_equal(xyz, g['xyz'])
    np.testing.assert_array_equal(xyz, xyz_exp)
    # the samples whose raw heat maps tie (several equal maxima per joint map; in one of them every pixel): the peak is the first
    # maximum in row-major order -- pixel 0 where the whole map ties
    tied = [b for b in range(B) if all((hm[b, :, :, j] == hm[b, :, :, j].max()).sum() > 1 for j in range(J))]
    assert len(tied) >= 2 and any((hm[b] == hm[b].max(axis=(0, 1))).all() for b in tied)
    for b in tied:
        for j in range(J):
            flat = hm[b, :, :, j].reshape(-1)
            first = int(np.nonzero(flat == flat.max())[0][0])
            assert got['hm_peak'][0][b, j].tolist() == [first % m, first // m, flat[first]]
            if (flat == flat[0]).all():
                assert first == 0


# ---------------------------------------------------------------------------------------------
# 3. nullable members
# ---------------------------------------------------------------------------------------------
def test_report_nullable_members(be):
    """All members NULL (xyz = dr_vote's), one member only, all members but one: requested buffers are fully written, guard
    tails and non-requested buffers untouched (checked inside vote_report), and a requested member has the same bits in every
    combination."""
    from oracle.graph import NetConfig
    B, J, in_hw = 2, 5, 128
    maps = _seeded_maps(np.random.default_rng(1618), B, in_hw // 4, J, in_hw)
    h = be.handle(NetConfig(1, 8, J, in_hw=in_hw), B)
    xyz_plain = be.vote(h, *maps)
    xyz_all, full = vote_report(be, h, *maps)
    np.testing.assert_array_equal(xyz_all, xyz_plain)
    xyz_none, _ = vote_report(be, h, *maps, want=())
    np.testing.assert_array_equal(xyz_none, xyz_plain)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for name in FIELDS:
        for want in ((name,), tuple(n for n in FIELDS if n != name)):
            xyz, got = vote_report(be, h, *maps, want=want)
            np.testing.assert_array_equal(bits(xyz), bits(xyz_plain))
            for n in want:
                np.testing.assert_array_equal(bits(got[n][0]), bits(full[n][0]), err_msg='%s in %s' % (n, want))
    h.close()


# ---------------------------------------------------------------------------------------------
# 4. fused entry point
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def case1():
    return e2e_case()


def test_infer_report_matches_forward_plus_vote_report(be, case1):
    """dr_infer_report == dr_forward_eval + dr_vote_report in every member, bit for bit; its xyz_mm is dr_infer's."""
    cfg, params, g = case1
    h = be.handle(cfg, 1)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    dm, cfgs, coms = g['dm'], g['cfg'], g['com']
    ndm = be.norm_dm(h, dm, coms)
    hm, hm3, um = be.forward_eval(h, ndm)
    xyz_split, split = vote_report(be, h, hm, hm3, um, ndm, cfgs, coms)
    xyz_fused, fused = infer_report(be, h, ndm, cfgs, coms)
    xyz_infer = be.infer(h, ndm, cfgs, coms)
    h.close()
    for n in FIELDS:
        np.testing.assert_array_equal(fused[n][0], split[n][0], err_msg=n)
    np.testing.assert_array_equal(xyz_fused, xyz_split)
    np.testing.assert_array_equal(xyz_fused, xyz_infer)


# ---------------------------------------------------------------------------------------------
# 5. graph mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_infer_report_under_graph_mode_writes_the_named_buffers(gpu, monkeypatch):
    """DR_GRAPHS=1: dr_infer_report with report buffers A, then B, then A again (dr_infer's recorded graph replayed in between on
    the same inputs): each time the named buffers hold the direct-launch result and the others keep their sentinel."""
    from densereg_amd.data.synthetic import make_crops
    from oracle import net, pose
    from oracle.graph import NetConfig
    cfg = NetConfig(1, 32, 16)
    B, J = 2, 16
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=78)
    ndm = pose.norm_dm(dm, coms)
    params = net.make_test_params(cfg, ndm, seed=3)

    def make_handle(graphs):
        if graphs:
            monkeypatch.setenv('DR_GRAPHS', '1')
        else:
            monkeypatch.delenv('DR_GRAPHS', raising=False)
        h = gpu.handle(cfg, B)
        h.load_params(params)
        h.call('dr_finalize_params', gpu.stream)
        return h

    h = make_handle(False)
    xyz_direct, direct = infer_report(gpu, h, ndm, cfgs, coms)
    h.close()

    h = make_handle(True)
    d = [gpu.dev(np.ascontiguousarray(a, np.float32)) for a in (ndm, cfgs, coms)]
    xyz = gpu.empty((B, 3 * J))
    sets = {'A': ReportBuffers(gpu, B, J), 'B': ReportBuffers(gpu, B, J)}
    for named in ('A', 'B', 'A'):
        for s in sets.values():
            for t in s.dev.values():
                t.fill_(SENT)
        xyz.fill_(SENT)
        h.call('dr_infer', B, *[gpu.ptr(a) for a in d], gpu.ptr(xyz), gpu.stream)          # records / replays dr_infer's graph
        gpu.sync()
        np.testing.assert_array_equal(gpu.host(xyz), xyz_direct)
        xyz.fill_(SENT)
        rep = sets[named].struct(FIELDS)
        h.call('dr_infer_report', B, *[gpu.ptr(a) for a in d], gpu.ptr(xyz), C.byref(rep), gpu.stream)
        gpu.sync()
        np.testing.assert_array_equal(gpu.host(xyz), xyz_direct)
        got = sets[named].read()
        _check_written(got, FIELDS)
        for n in FIELDS:
            np.testing.assert_array_equal(got[n][0], direct[n][0], err_msg='%s in set %s' % (n, named))
        other = sets['B' if named == 'A' else 'A'].read()
        _check_written(other, ())
    h.close()


# ---------------------------------------------------------------------------------------------
# 6. arguments
# ---------------------------------------------------------------------------------------------
def test_report_argument_checking(emu):
    """NULL report, B > max_batch and NULL xyz_mm_dev are DR_E_INVALID in both entry points, as dr_vote / dr_infer report them."""
    from oracle.graph import NetConfig
    be = emu
    J, m = 2, 32
    h = be.handle(NetConfig(1, 8, J), 1)
    h.call('dr_finalize_params', be.stream)
    maps = [be.dev(np.zeros(s, np.float32)) for s in ((2, m, m, J), (2, m, m, J), (2, m, m, 3 * J), (2, 128, 128, 1), (2, 6), (2, 3))]
    p = [be.ptr(a) for a in maps]
    xyz = be.dev(np.zeros((2, 3 * J), np.float32))
    rep = ReportBuffers(be, 2, J).struct(FIELDS)
    # NULL report
    assert h.lib.dr_vote_report(h._h, 1, *p, be.ptr(xyz), None, be.stream) == -1
    assert b'report' in h.lib.dr_last_error(h._h)
    assert h.lib.dr_infer_report(h._h, 1, p[3], p[4], p[5], be.ptr(xyz), None, be.stream) == -1
    assert b'report' in h.lib.dr_last_error(h._h)
    # B > max_batch, with a message
    for fn, args in (('dr_vote_report', p), ('dr_infer_report', p[3:])):
        with pytest.raises(_lib.DenseRegError) as e:
            h.call(fn, 2, *args, be.ptr(xyz), C.byref(rep), be.stream)
        assert e.value.code == -1 and 'max_batch' in str(e.value)
    # NULL xyz_mm_dev
    assert h.lib.dr_vote_report(h._h, 1, *p, None, C.byref(rep), be.stream) == -1
    assert h.lib.dr_infer_report(h._h, 1, p[3], p[4], p[5], None, C.byref(rep), be.stream) == -1
    # and the same arguments, complete, are accepted
    h.call('dr_vote_report', 1, *p, be.ptr(xyz), C.byref(rep), be.stream)
    h.close()


# ---------------------------------------------------------------------------------------------
# 7. Python layer
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_engine_and_model_report_interface(gpu):
    """Engine.infer_report: shapes and dtypes, `fields`, hm_uvd_pts; JointDetectionModel.test(report=True) sets the reference's fetch
    interface and returns the xyz of the default path."""
    import torch
    from densereg_amd import flags
    from densereg_amd.data.synthetic import make_crops
    from densereg_amd.engine import Engine, VoteReport
    from densereg_amd.model import hourglass_um_crop_tiny as M
    from densereg_amd.network import um_v1
    B, J = 2, 16
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=79)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu.device)
    eng = Engine(1, 32, J, 128, 3, B, 0, False)
    eng.load_params(M._random_params(eng))
    ndm = eng.norm_dm(t(dm), t(coms))
    xyz, rep = eng.infer_report(ndm, t(cfgs), t(coms))
    assert isinstance(rep, VoteReport) and tuple(xyz.shape) == (B, 3 * J)
    for n in FIELDS:
        a = getattr(rep, n)
        assert tuple(a.shape) == _shape(n, B, J), n
        assert a.dtype == (torch.int32 if n == 'can_idx' else torch.float32), n
    assert torch.equal(xyz, eng.infer(ndm, t(cfgs), t(coms)))
    hu = rep.hm_uvd_pts
    assert tuple(hu.shape) == (B, 3 * J)
    hu = hu.reshape(B, J, 3)
    assert torch.equal(hu[..., :2], 4 * rep.hm_peak[..., :2]) and bool((hu[..., 2] == 1).all())
    xyz1, only = eng.infer_report(ndm, t(cfgs), t(coms), fields=('uvd',))
    assert torch.equal(only.uvd, rep.uvd) and torch.equal(xyz1, xyz)
    assert all(getattr(only, n) is None for n in FIELDS if n != 'uvd') and only.hm_uvd_pts is None
    with pytest.raises(ValueError):
        eng.infer_report(ndm, t(cfgs), t(coms), fields=('no_such_member',))
    eng.close()
    # the model class
    flags.parse(['--dataset', 'icvl', '--num_stack', '1', '--fea_num', '32', '--is_train', 'False', '--batch_size', str(B)])
    try:
        e2 = um_v1.get_engine(J, 128, B, 0, False)
        e2.load_params(M._random_params(e2))
        model = M.JointDetectionModel(M.SyntheticDataset('icvl', 'testing'), um_v1.detect_net, epoch=1)
        args = (t(dm), t(poses), t(cfgs), t(coms))
        xyz_plain = model.test(*args)
        assert not hasattr(model, 'uvd_pts')
        xyz_rep = model.test(*args, report=True)
        assert torch.equal(xyz_rep, xyz_plain)
        assert tuple(model.uvd_pts.shape) == (B, J, 3) and tuple(model.hm_uvd_pts.shape) == (B, 3 * J)
        assert tuple(model.can_pts.shape) == (B, J, 5, 3) and tuple(model.ori_pts.shape) == (B, J, 5, 3)
        torch.cuda.synchronize()
    finally:
        flags.parse([])
