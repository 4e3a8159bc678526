"""The bottom of every hourglass as ONE launch on an fp32 handle with num_fea 192 and 256 (``densereg_amd/csrc/hg_fused_x3.h``,
``dr_set_fusion(h, 2)``): fp32-accurate products from three bf16 planes per operand on v_mfma_f32_16x16x32_bf16, fp32 residual stream
and epilogues.  Against the oracle in plain fp32 and against the unfused fp32 executor, that it is what ran, and that it is
deterministic, per crop and feeds the vote.  ``[emu]`` on CPU fibers (minutes at these widths: skipped in the suite, F = 192 was run once
by hand, profiles/hg_fused_x3.md), ``[gpu]`` on an MI355X."""
import functools

import numpy as np
import pytest

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]
S, J = 1, 3
MAPS = ('hm_outs', 'hm3_outs', 'um_outs')


@pytest.fixture(params=BACKENDS)
def be(request):
    be = request.getfixturevalue(request.param)
    if be.name == 'emu':
        pytest.skip('F = 192 | 256 on CPU fibers is minutes; covered on the GPU')
    return be


@functools.lru_cache(maxsize=None)
def _case(F, B):
    """network, inputs, the 3x3 of lower1 at 8x8 (inside the region), the region's last layer, and the oracle in plain fp32: its head
    maps and that layer, computed once per shape"""
    from densereg_amd.data.synthetic import make_crops
    from oracle import net, pose
    from oracle.graph import NetConfig, conv_specs
    cfg = NetConfig(S, F, J)
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=31)
    ndm = pose.norm_dm(dm, coms)
    params = net.make_test_params(cfg, ndm[:2], seed=5)
    c8 = [c for c in conv_specs(cfg) if c.h_out == 8]
    assert len(c8) == 9 and c8[1].k == 3 and c8[-1].cout == F
    rec = {}
    o = net.forward_eval(cfg, params, ndm, record=rec)
    ref = [o[k][-1] for k in MAPS] + [rec[c8[-1].name + '+res']]
    return cfg, params, ndm, cfgs, coms, c8[1], c8[-1], ref


def _handle(be, F, B, fusion=None):
    cfg, params = _case(F, B)[:2]
    h = be.handle(cfg, B)
    if fusion is not None:
        h.call('dr_set_fusion', fusion)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    return h


def _close(a, b, tol=2e-5):
    return np.abs(a - b).max() <= tol * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize('F', [192, 256])
def test_fused_x3_is_as_accurate_as_the_unfused_fp32_path(be, F):
    """F = 192: three K-groups in the half-width convolutions, 6 | 12 column tiles on eight waves; F = 256: the largest LDS and register
    case.  Bars: 5e-4 of range against the oracle (test_fused_tail); at most 6x the unfused executor's error + 1e-6 of range (the factor
    the x3 kernels are granted over the fp32 MFMA kernels), and fused against unfused within that same bar.  Measured on MI355X:
    profiles/hg_fused_x3.md."""
    B = 3
    ndm, out, ref = _case(F, B)[2], _case(F, B)[6], _case(F, B)[7]
    h = _handle(be, F, B, fusion=2)
    fused = list(be.forward_eval(h, ndm)) + [be.read_activation(h, out.name, (B, 8, 8, F))]     # (the region's last layer IS in HBM)
    h.call('dr_set_fusion', 1)                                                                   # no fp32 fused kernel at these widths
    plain = list(be.forward_eval(h, ndm)) + [be.read_activation(h, out.name, (B, 8, 8, F))]
    h.close()
    for what, a, p, r in zip(MAPS + (out.name,), fused, plain, ref):
        rng = max(1.0, float(np.abs(r).max()))
        e_f, e_p, e_fp = (float(np.abs(x - y).max()) for x, y in ((a, r), (p, r), (a, p)))
        print(F, what, 'range %.3e  fused-oracle %.3e  plain-oracle %.3e  fused-plain %.3e  (2e-5 of range: %s)'
              % (rng, e_f, e_p, e_fp, e_fp <= 2e-5 * rng))
        assert e_f < 5e-4 * rng, (what, e_f, rng)
        assert e_f <= 6 * e_p + 1e-6 * rng, (what, e_f, e_p)
        assert e_fp <= 6 * e_p + 1e-6 * rng, (what, e_fp, e_p)


def test_fused_x3_is_what_ran_and_the_default_did_not_move(be):
    from densereg_amd._lib import DenseRegError
    F, B = 192, 3
    ndm, inner = _case(F, B)[2], _case(F, B)[5]
    h = _handle(be, F, B, fusion=2)
    be.forward_eval(h, ndm)
    with pytest.raises(DenseRegError):                                         # it lived in LDS
        be.read_activation(h, inner.name, (B, 8, 8, F // 2))
    h.call('dr_set_fusion', 1)                                                 # the default: every op of the region is a launch at this F
    a = be.forward_eval(h, ndm)
    assert np.isfinite(be.read_activation(h, inner.name, (B, 8, 8, F // 2))).all()
    h.close()
    h = _handle(be, F, B)                                                      # a handle that never asked for fusion 2
    for x, y in zip(a, be.forward_eval(h, ndm)):
        np.testing.assert_array_equal(x, y)
    h.close()


def test_fused_x3_is_deterministic_per_crop_and_feeds_the_vote(be):
    F, B = 192, 3
    _, _, ndm, cfgs, coms = _case(F, B)[:5]
    h = _handle(be, F, B, fusion=2)
    maps = be.forward_eval(h, ndm)
    for x, y in zip(maps, be.forward_eval(h, ndm)):
        np.testing.assert_array_equal(x, y)
    xyz = be.infer(h, ndm, cfgs, coms)
    assert xyz.shape == (B, 3 * J) and np.isfinite(xyz).all()
    np.testing.assert_array_equal(xyz, be.vote(h, *maps, ndm, cfgs, coms))      # the vote is fp32 on whatever maps it is given
    # (the layers around the region pick their tiles by batch size: closeness, not bits, as in test_fused_tail)
    for a, b in zip(be.forward_eval(h, np.ascontiguousarray(ndm[1:2])), maps):
        assert _close(a[0], b[1])
    h.close()
