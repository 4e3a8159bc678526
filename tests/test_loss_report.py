"""The loss report (``dr_targets`` / ``dr_loss_report``, ``densereg_amd/csrc/loss_report.h``): the training targets as maps, and the l2
losses of the most recent forward -- eval or train, training or inference handle -- per stack, per joint and per crop.

Bars: the targets BIT-EXACT against ``oracle.pose.make_targets`` (every op of the kernel is one correctly rounded fp32 op in the
oracle's order); the loss terms against an independent host sum at ``rtol = 2.5e-7`` (two fp32 ulps: both sides are fp32 casts of
fp64 sums of at most 1e6 non-negative terms, which agree to ~1e-10 whatever their order); ``total`` against ``dr_loss`` at the same
bar; the report read-only (a training step with reports interleaved gives the bits of one without), deterministic, and the same
bits whichever members are asked for.  ``[emu]`` on the host-fiber emulator, ``[gpu]`` on the MI355X.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from densereg_amd import _lib
from tests.common import flat_grads_by_name

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


FIELDS = tuple(_lib.LOSS_REPORT_FIELDS)            # total stack_losses joint_losses crop_losses gt_hm gt_hm3 gt_um
LOSSES, MAPS = FIELDS[:4], FIELDS[4:]
SENT = -777.0                                      # no loss (>= 0) and no target (|.| <= ~1) can take it
GUARD = 24                                         # elements behind every payload that must stay untouched
RTOL = 2.5e-7

# (num_stack, num_fea, num_jnt, in_hw), B, dataset of the synthetic crops:
#   a  two stacks, an odd joint count that straddles waves and workgroups, an odd batch
#   b  64x64 maps: more chunks per crop, the depth stride on a larger crop
#   c  the msra joint count
CASES = {'a': ((2, 8, 7, 128), 3, 'icvl'), 'b': ((1, 8, 3, 256), 2, 'nyu'), 'c': ((2, 8, 21, 128), 1, 'msra')}


@functools.lru_cache(maxsize=None)
def _case(name, B=None, net=None):
    """cfg, params, (ndm, poses, cfgs, coms), make_targets' maps -- computed once per case, never modified"""
    from densereg_amd.data.synthetic import make_crops
    from oracle import net as onet, pose
    from oracle.graph import NetConfig
    (S, F, J, in_hw), B0, dataset = CASES[name]
    if net is not None:
        S, F, J, in_hw = net
    B = B or B0
    cfg = NetConfig(S, F, J, in_hw=in_hw)
    dm, poses, cfgs, coms, _ = make_crops(B, dataset, seed=5, hw=in_hw)
    poses = np.ascontiguousarray(poses[:, :3 * J])
    ndm = pose.norm_dm(dm, coms)
    params = onet.make_test_params(cfg, ndm[:4], seed=7)
    gt = pose.make_targets(ndm, poses, cfgs, coms, out_hw=in_hw // 4)
    for a in (ndm, poses, cfgs, coms) + tuple(gt):
        a.setflags(write=False)
    return cfg, params, (ndm, poses, cfgs, coms), gt


def _shape(name, B, cfg):
    return tuple(_lib.LOSS_REPORT_FIELDS[name](B, cfg.num_stack, cfg.num_jnt, cfg.in_hw // 4))


class Buffers:
    """All seven device buffers, pre-filled with the sentinel and over-allocated by a guard tail"""

    def __init__(self, be, B, cfg):
        self.be, self.B, self.cfg = be, B, cfg
        self.dev = {n: be.dev(np.full(int(np.prod(_shape(n, B, cfg))) + GUARD, SENT, np.float32)) for n in FIELDS}

    def ptr(self, n, want):
        return self.be.ptr(self.dev[n]) if n in want else None

    def struct(self, want):
        rep = _lib.DrLossReport()
        for n in FIELDS:
            setattr(rep, n + '_dev', self.ptr(n, want))
        return rep

    def read(self, want):
        """name -> payload; requested buffers fully written, guard tails and non-requested buffers untouched"""
        out = {}
        for n in FIELDS:
            a = np.array(self.be.host(self.dev[n]))
            payload, tail = a[:-GUARD].reshape(_shape(n, self.B, self.cfg)), a[-GUARD:]
            assert (tail == SENT).all(), '%s: guard tail written' % n
            if n in want:
                assert not (payload == SENT).any(), '%s: sentinel left in the payload' % n
            else:
                assert (payload == SENT).all(), '%s: written although not requested' % n
            out[n] = payload
        return out


def _upload(be, inputs):
    return [be.dev(np.array(a, np.float32)) for a in inputs]              # (writable copies: the cached inputs are read-only)


def loss_report(be, h, cfg, d_in, want=FIELDS):
    B = d_in[0].shape[0]
    bufs = Buffers(be, B, cfg)
    rep = bufs.struct(want)
    h.call('dr_loss_report', B, *[be.ptr(a) for a in d_in], C.byref(rep), be.stream)
    be.sync()
    return bufs.read(want)


def targets(be, h, cfg, d_in, want=MAPS):
    B = d_in[0].shape[0]
    bufs = Buffers(be, B, cfg)
    h.call('dr_targets', B, *[be.ptr(a) for a in d_in], *[bufs.ptr(n, want) for n in MAPS], be.stream)
    be.sync()
    return bufs.read(want)


def read_all_maps(be, h, cfg, B):
    m, J = cfg.in_hw // 4, cfg.num_jnt
    out = []
    for s in range(cfg.num_stack):
        hm, hm3, um = be.empty((B, m, m, J)), be.empty((B, m, m, J)), be.empty((B, m, m, 3 * J))
        h.call('dr_read_maps', B, s, be.ptr(hm), be.ptr(hm3), be.ptr(um), be.stream)
        be.sync()
        out.append(tuple(np.array(be.host(a)) for a in (hm, hm3, um)))
    return out


def expected_losses(maps, gt):
    """The independent sum: e = fp32(est) - fp32(gt) in fp32, 0.5 * float64(e)**2 summed in fp64 per (b, s, j, term); crop, joint,
    stack and total derived from those sums."""
    gt_hm, gt_hm3, gt_um = gt
    B, m, _, J = gt_hm.shape
    bsj = np.zeros((B, len(maps), J, 3), np.float64)
    for s, (hm, hm3, um) in enumerate(maps):
        for k, (est, ref) in enumerate(((hm, gt_hm), (hm3, gt_hm3))):
            e = (est.astype(np.float32) - ref.astype(np.float32)).astype(np.float32)
            bsj[:, s, :, k] = (0.5 * e.astype(np.float64) ** 2).sum(axis=(1, 2))
        e = (um.astype(np.float32) - gt_um.astype(np.float32)).astype(np.float32).reshape(B, m, m, J, 3)
        bsj[:, s, :, 2] = (0.5 * e.astype(np.float64) ** 2).sum(axis=(1, 2, 4))
    stack = bsj.sum(axis=(0, 2))
    return {'total': stack.sum(axis=0), 'stack_losses': stack, 'joint_losses': bsj.sum(axis=0), 'crop_losses': bsj.sum(axis=2)}


def _assert_losses(got, exp, what=''):
    for n in LOSSES:
        rel = np.abs(got[n].astype(np.float64) - exp[n]) / np.abs(exp[n])
        print('%s %s: max relative deviation from the host sum %.3g' % (what, n, rel.max()))
        np.testing.assert_allclose(got[n], exp[n].astype(np.float32), rtol=RTOL, atol=0, err_msg='%s %s' % (what, n))


def _handle(be, cfg, params, B, training=False):
    h = be.handle(cfg, B, training=training)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    return h


def _forward_eval(be, h, d_dm):
    h.call('dr_forward_eval', d_dm.shape[0], be.ptr(d_dm), None, None, None, be.stream)


def _forward_train(be, h, d_dm):
    h.call('dr_forward_train', d_dm.shape[0], be.ptr(d_dm), 0, None, C.c_uint64(0), be.stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# A forward on the emulator costs seconds, and the report changes nothing in a handle: the tests that only READ a forward share one
# handle per (backend, case, mode), forwarded once; no test runs another forward on it.
_SHARED = {}


def _forwarded(be, case, train=False):
    key = (be.name, case, train)
    if key not in _SHARED:
        cfg, params, inputs, _ = _case(case)
        h = _handle(be, cfg, params, inputs[0].shape[0], training=train)
        d_in = _upload(be, inputs)
        (_forward_train if train else _forward_eval)(be, h, d_in[0])
        _SHARED[key] = (h, d_in)
    return _SHARED[key]


@pytest.fixture(scope='module', autouse=True)
def _close_shared_handles():
    yield
    for h, _ in _SHARED.values():
        h.close()
    _SHARED.clear()


# ---------------------------------------------------------------------------------------------
# 1. targets, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_targets_bit_exact(be, case):
    """dr_targets == oracle.pose.make_targets on all three maps -- on a handle without parameters or forward -- and the gt members
    of dr_loss_report are dr_targets' bits."""
    cfg, params, inputs, gt = _case(case)
    B = inputs[0].shape[0]
    h = be.handle(cfg, B)
    d_in = _upload(be, inputs)
    got = targets(be, h, cfg, d_in)
    h.close()
    for n, ref in zip(MAPS, gt):
        np.testing.assert_array_equal(got[n], ref, err_msg=n)
    h, d_in = _forwarded(be, case)
    rep = loss_report(be, h, cfg, d_in, want=MAPS)
    for n in MAPS:
        np.testing.assert_array_equal(_bits(rep[n]), _bits(got[n]), err_msg=n)


# ---------------------------------------------------------------------------------------------
# 2. loss terms against an independent sum
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,train', [('a', False), ('b', False), ('c', False), ('a', True)],
                         ids=['a_eval', 'b_eval', 'c_eval', 'a_train'])
def test_loss_terms_against_an_independent_sum(be, case, train):
    """dr_forward_eval on an inference handle at (a), (b), (c), dr_forward_train on a training handle at (a): every loss member
    against the host sum over the maps dr_read_maps fetches and make_targets' maps."""
    cfg, _, inputs, gt = _case(case)
    h, d_in = _forwarded(be, case, train)
    got = loss_report(be, h, cfg, d_in)
    exp = expected_losses(read_all_maps(be, h, cfg, inputs[0].shape[0]), gt)
    _assert_losses(got, exp, case)


# ---------------------------------------------------------------------------------------------
# 3. consistency with dr_loss
# ---------------------------------------------------------------------------------------------
def test_total_matches_dr_loss(be):
    """dr_forward_train -> dr_loss_report -> dr_loss: both are fp32 casts of fp64 sums over the same terms, so the restated target
    arithmetic is loss_kernel's."""
    cfg, _, inputs, _ = _case('a')
    B = inputs[0].shape[0]
    h, d_in = _forwarded(be, 'a', True)
    got = loss_report(be, h, cfg, d_in, want=('total',))
    d_lo = be.dev(np.full(4, SENT, np.float32))
    h.call('dr_loss', B, *[be.ptr(a) for a in d_in], be.ptr(d_lo), be.stream)
    be.sync()
    lo = np.array(be.host(d_lo))
    print('total %s dr_loss %s' % (got['total'], lo[:3]))
    np.testing.assert_allclose(got['total'], lo[:3], rtol=RTOL, atol=0)


# ---------------------------------------------------------------------------------------------
# 4. read-only
# ---------------------------------------------------------------------------------------------
def _train_step(be, net, B, depth, groups, with_reports, steps):
    cfg, params, inputs, _ = _case('a', B, net)
    h = _handle(be, cfg, params, B, training=True)
    if depth == 2:
        h.call('dr_set_pipeline', 2)
    if groups > 1:
        h.call('dr_set_groups', groups)
    h.call('dr_zero_grad', be.stream)
    d_in = _upload(be, inputs)
    losses, reports = [], []
    for _ in range(steps):
        d_lo = be.dev(np.full((groups, 4), SENT, np.float32))
        _forward_train(be, h, d_in[0])
        if with_reports:
            reports.append(loss_report(be, h, cfg, d_in))
        h.call('dr_loss', B, *[be.ptr(a) for a in d_in], be.ptr(d_lo), be.stream)
        if with_reports:
            reports.append(loss_report(be, h, cfg, d_in))
        h.call('dr_backward', B, be.stream)
        losses.append(d_lo)
    h.call('dr_sync_grads', be.stream)
    be.sync()
    losses = [np.array(be.host(a)) for a in losses]
    grads = flat_grads_by_name(be, h, cfg)
    h.close()
    return losses, grads, reports


def _read_only_check(be, net, B, depth, groups, steps):
    lo_plain, g_plain, _ = _train_step(be, net, B, depth, groups, False, steps)
    lo_rep, g_rep, reports = _train_step(be, net, B, depth, groups, True, steps)
    for a, b in zip(lo_plain, lo_rep):
        assert not (a == SENT).any()
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert set(g_plain) == set(g_rep)
    for n in g_plain:
        np.testing.assert_array_equal(_bits(g_plain[n]), _bits(g_rep[n]), err_msg=n)
    for before, after in zip(reports[0::2], reports[1::2]):
        for n in FIELDS:
            np.testing.assert_array_equal(_bits(before[n]), _bits(after[n]), err_msg=n)
    if groups > 1:                                           # crop_losses is the per-micro-batch view of dr_loss's rows
        per_group = reports[0]['crop_losses'].astype(np.float64).reshape(groups, B // groups, -1, 3).sum(axis=(1, 2))
        np.testing.assert_allclose(per_group, lo_plain[0].reshape(groups, 4)[:, :3], rtol=1e-6)


@pytest.mark.parametrize('depth', [1, 2])
def test_report_is_read_only(be, depth):
    """Training steps from identical state with and without dr_loss_report before and after dr_loss: the same dr_loss output and
    the same flat gradient, bit for bit -- on one slot, and on two slots (two micro-steps, one per slot); the reports before and
    after dr_loss are the same bits too (dr_loss writes nothing the report reads).  Case (a) on the GPU; on the emulator, where a
    training step of it takes half a minute, one crop through one stack (what the report may not touch is the same)."""
    net, B = ((1, 8, 3, 128), 1) if be.name == 'emu' else (None, 3)
    _read_only_check(be, net, B, depth, 1, depth)


@pytest.mark.gpu
def test_report_is_read_only_with_micro_batch_groups(gpu):
    """The same with dr_set_groups(2) and B = 16 (two micro-batches of 8 crops, the smallest the groups take), where crop_losses
    also is the per-micro-batch view of dr_loss's two rows.  GPU only: two such steps take minutes on the emulator."""
    _read_only_check(gpu, None, 16, 1, 2, 1)


# ---------------------------------------------------------------------------------------------
# 5. determinism, 6. subsets
# ---------------------------------------------------------------------------------------------
def test_report_is_deterministic_and_members_are_independent(be):
    """Two calls on the same forward: the same bits in every member.  Each member alone, total + joint_losses, and the targets only:
    the bits of the all-members call, nothing else written (checked against sentinels inside loss_report)."""
    cfg = _case('a')[0]
    h, d_in = _forwarded(be, 'a')
    full = loss_report(be, h, cfg, d_in)
    again = loss_report(be, h, cfg, d_in)
    for n in FIELDS:
        np.testing.assert_array_equal(_bits(full[n]), _bits(again[n]), err_msg=n)
    for want in [(n,) for n in FIELDS] + [('total', 'joint_losses'), MAPS]:
        got = loss_report(be, h, cfg, d_in, want=want)
        for n in want:
            np.testing.assert_array_equal(_bits(got[n]), _bits(full[n]), err_msg='%s in %s' % (n, want))
    for want in [(n,) for n in MAPS]:
        got = targets(be, h, cfg, d_in, want=want)
        np.testing.assert_array_equal(_bits(got[want[0]]), _bits(full[want[0]]), err_msg=want[0])


# ---------------------------------------------------------------------------------------------
# 7. inference handle
# ---------------------------------------------------------------------------------------------
def _report_after_infer(be, case, net, fusion):
    cfg, params, inputs, gt = _case(case, None, net)
    B = inputs[0].shape[0]
    h = _handle(be, cfg, params, B)
    h.call('dr_set_fusion', fusion)
    d_in = _upload(be, inputs)
    xyz = be.empty((B, 3 * cfg.num_jnt))
    h.call('dr_infer', B, be.ptr(d_in[0]), be.ptr(d_in[2]), be.ptr(d_in[3]), be.ptr(xyz), be.stream)
    got = loss_report(be, h, cfg, d_in)
    exp = expected_losses(read_all_maps(be, h, cfg, B), gt)
    h.close()
    _assert_losses(got, exp, 'fusion=%d' % fusion)
    for n, ref in zip(MAPS, gt):
        np.testing.assert_array_equal(got[n], ref, err_msg=n)


@pytest.mark.parametrize('fusion', [1, 0])
def test_report_after_infer_on_an_inference_handle(be, fusion):
    """training = 0: dr_infer, then dr_loss_report, with dr_set_fusion on and off -- the values of the independent sum over the
    maps dr_read_maps fetches, at (c)."""
    _report_after_infer(be, 'c', None, fusion)


@pytest.mark.gpu
@pytest.mark.parametrize('fusion', [1, 0])
def test_report_after_infer_with_the_fused_hourglass_bottoms(gpu, fusion):
    """The same at (a) with num_fea = 32, the narrowest network whose hourglass bottoms run as the fused launch (8 features are too
    few for it, and the emulator too slow for 32)."""
    _report_after_infer(gpu, 'a', (2, 32, 7, 128), fusion)


# ---------------------------------------------------------------------------------------------
# 8. the vote on the targets
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_vote_on_targets(be, case):
    """dr_vote on dr_targets' maps == the oracle's vote on make_targets' maps (the vote's own ceiling on a frame; not the ground
    truth: a joint whose cone falls on background comes back elsewhere)."""
    from oracle import pose
    cfg, _, inputs, gt = _case(case)
    ndm, _, cfgs, coms = inputs
    B = ndm.shape[0]
    h = be.handle(cfg, B)
    got = targets(be, h, cfg, _upload(be, inputs))
    xyz = be.vote(h, got['gt_hm'], got['gt_hm3'], got['gt_um'], ndm.copy(), cfgs.copy(), coms.copy())
    h.close()
    with np.errstate(all='ignore'):
        exp = pose.estimate_pose_mm(gt[0], gt[1], gt[2], ndm, cfgs, coms, out_hw=cfg.in_hw // 4)
    np.testing.assert_array_equal(np.array(xyz), exp.reshape(B, -1))


# ---------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------
def test_error_contract(be):
    from oracle.graph import NetConfig
    INVALID, UNSUPPORTED, STATE = -1, -2, -3
    cfg, params, inputs, _ = _case('a', 2, (1, 8, 3, 128))
    B = inputs[0].shape[0]
    h = _handle(be, cfg, params, B)
    d_in = _upload(be, inputs)
    p = [be.ptr(a) for a in d_in]
    bufs = Buffers(be, B, cfg)
    rep = bufs.struct(FIELDS)
    lib = h.lib
    # no forward yet
    assert lib.dr_loss_report(h._h, B, *p, C.byref(rep), be.stream) == STATE
    assert b'forward' in lib.dr_last_error(h._h)
    # dr_targets needs none
    h.call('dr_targets', B, *p, *[bufs.ptr(n, MAPS) for n in MAPS], be.stream)
    _forward_eval(be, h, d_in[0])
    good = loss_report(be, h, cfg, d_in)
    # NULL handle / required pointers
    assert lib.dr_loss_report(None, B, *p, C.byref(rep), be.stream) == INVALID
    assert lib.dr_targets(None, B, *p, *[bufs.ptr(n, MAPS) for n in MAPS], be.stream) == INVALID
    for i in range(4):
        q = list(p)
        q[i] = None
        assert lib.dr_loss_report(h._h, B, *q, C.byref(rep), be.stream) == INVALID
        assert lib.dr_targets(h._h, B, *q, *[bufs.ptr(n, MAPS) for n in MAPS], be.stream) == INVALID
    # no report / nothing wanted
    assert lib.dr_loss_report(h._h, B, *p, None, be.stream) == INVALID
    assert lib.dr_loss_report(h._h, B, *p, C.byref(bufs.struct(())), be.stream) == INVALID
    assert lib.dr_targets(h._h, B, *p, None, None, None, be.stream) == INVALID
    # B outside [1, max_batch]
    for bad in (0, -1, B + 1):
        assert lib.dr_loss_report(h._h, bad, *p, C.byref(rep), be.stream) == INVALID
        assert lib.dr_targets(h._h, bad, *p, *[bufs.ptr(n, MAPS) for n in MAPS], be.stream) == INVALID
    with pytest.raises(_lib.DenseRegError) as e:
        h.call('dr_loss_report', B + 1, *p, C.byref(rep), be.stream)
    assert e.value.code == INVALID and 'max_batch' in str(e.value)
    # B differs from the last forward's
    assert lib.dr_loss_report(h._h, B - 1, *p, C.byref(rep), be.stream) == STATE
    be.sync()
    bufs.read(MAPS)                                          # dr_targets' maps are there, no rejected call wrote a loss member
    # after all that the handle still works
    again = loss_report(be, h, cfg, d_in)
    for n in FIELDS:
        np.testing.assert_array_equal(_bits(again[n]), _bits(good[n]), err_msg=n)
    h.close()
    # more stacks than the loss kernels take
    cfg9 = NetConfig(9, 8, 2)
    h = be.handle(cfg9, 1)
    b9 = Buffers(be, 1, cfg9)
    d9 = _upload(be, [inputs[0][:1], inputs[1][:1, :6], inputs[2][:1], inputs[3][:1]])
    assert h.lib.dr_loss_report(h._h, 1, *[be.ptr(a) for a in d9], C.byref(b9.struct(FIELDS)), be.stream) == UNSUPPORTED
    h.call('dr_targets', 1, *[be.ptr(a) for a in d9], *[b9.ptr(n, MAPS) for n in MAPS], be.stream)     # the targets do not care
    be.sync()
    b9.read(MAPS)
    h.close()


# ---------------------------------------------------------------------------------------------
# 10. Python layer
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_engine_and_model_loss_report_interface(gpu):
    """Engine.loss_report / Engine.targets: shapes, None members, unknown names; JointDetectionModel.test(losses=True) against the
    Engine calls made by hand; test() with defaults returns the same xyz bits and sets nothing."""
    import torch
    from densereg_amd import flags
    from densereg_amd.data.synthetic import make_crops
    from densereg_amd.engine import Engine, LossReport
    from densereg_amd.model import hourglass_um_crop_tiny as M
    from densereg_amd.network import um_v1
    B, S, J, m = 2, 2, 16, 32
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=79)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu.device)
    eng = Engine(S, 32, J, 128, 3, B, 0, False)
    cfg = types.SimpleNamespace(num_stack=S, num_jnt=J, in_hw=128)
    ndm = eng.norm_dm(t(dm), t(coms))
    gt = eng.targets(ndm, t(poses), t(cfgs), t(coms))                       # no parameters, no forward
    assert [tuple(a.shape) for a in gt] == [(B, m, m, J), (B, m, m, J), (B, m, m, 3 * J)]
    only = eng.targets(ndm, t(poses), t(cfgs), t(coms), fields=('gt_hm3',))
    assert only[0] is None and only[2] is None and torch.equal(only[1], gt[1])
    with pytest.raises(ValueError):
        eng.targets(ndm, t(poses), t(cfgs), t(coms), fields=('total',))
    eng.load_params(M._random_params(eng))
    xyz = eng.infer(ndm, t(cfgs), t(coms))
    rep = eng.loss_report(ndm, t(poses), t(cfgs), t(coms))
    assert isinstance(rep, LossReport)
    for n in FIELDS:
        a = getattr(rep, n)
        assert tuple(a.shape) == _shape(n, B, cfg) and a.dtype == torch.float32, n
    for a, b in zip(gt, (rep.gt_hm, rep.gt_hm3, rep.gt_um)):
        assert torch.equal(a, b)
    assert torch.allclose(rep.stack_losses.sum(0), rep.total, rtol=1e-6, atol=0)
    two = eng.loss_report(ndm, t(poses), t(cfgs), t(coms), fields=('total', 'crop_losses'))
    assert torch.equal(two.total, rep.total) and torch.equal(two.crop_losses, rep.crop_losses)
    assert all(getattr(two, n) is None for n in FIELDS if n not in ('total', 'crop_losses'))
    with pytest.raises(ValueError):
        eng.loss_report(ndm, t(poses), t(cfgs), t(coms), fields=('no_such_member',))
    eng.close()
    # the model class
    flags.parse(['--dataset', 'icvl', '--num_stack', str(S), '--fea_num', '32', '--is_train', 'False', '--batch_size', str(B)])
    try:
        e2 = um_v1.get_engine(J, 128, B, 0, False)
        e2.load_params(M._random_params(e2))
        model = M.JointDetectionModel(M.SyntheticDataset('icvl', 'testing'), um_v1.detect_net, epoch=1)
        args = (t(dm), t(poses), t(cfgs), t(coms))
        xyz_plain = model.test(*args)
        assert not hasattr(model, 'val_losses') and not hasattr(model, 'gt_hms')
        assert torch.equal(xyz_plain, e2.infer(e2.norm_dm(args[0], args[3]), args[2], args[3]))
        xyz_val = model.test(*args, losses=True)
        assert torch.equal(xyz_val, xyz_plain)
        hand = e2.loss_report(e2.norm_dm(args[0], args[3]), args[1], args[2], args[3])
        assert torch.equal(model.val_losses, hand.total) and tuple(model.val_losses.shape) == (3,)
        assert torch.equal(model.val_stack_losses, hand.stack_losses) and tuple(model.val_stack_losses.shape) == (S, 3)
        assert torch.equal(model.val_joint_losses, hand.joint_losses) and tuple(model.val_joint_losses.shape) == (S, J, 3)
        assert torch.equal(model.gt_hms, hand.gt_hm) and torch.equal(model.gt_hm3s, hand.gt_hm3) and torch.equal(model.gt_ums, hand.gt_um)
        xyz_both = model.test(*args, report=True, losses=True)
        assert torch.equal(xyz_both, xyz_plain) and tuple(model.uvd_pts.shape) == (B, J, 3)
        torch.cuda.synchronize()
    finally:
        flags.parse([])
