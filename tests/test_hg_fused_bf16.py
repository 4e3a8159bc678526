"""The bottom of every hourglass as ONE launch under DR_PREC_BF16 (``densereg_amd/csrc/hg_fused_bf16.h``, ``dr_set_fusion(h, 2)``):
bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulation, epilogues and skip adds, num_fea 64 .. 256.  Against the oracle's
bf16-operand and fp32 evaluations with the bars of ``test_network_bf16_precision``, against the unfused bf16 executor, and that the
opt-in moved nothing else.  ``[emu]`` on CPU fibers, ``[gpu]`` on an MI355X."""
import functools

import numpy as np
import pytest

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]
S, J = 1, 3


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


@functools.lru_cache(maxsize=None)
def _case(F, B):
    from densereg_amd.data.synthetic import make_crops
    from oracle import net, pose
    from oracle.graph import NetConfig, conv_specs
    cfg = NetConfig(S, F, J)
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=31)
    ndm = pose.norm_dm(dm, coms)
    params = net.make_test_params(cfg, ndm[:2], seed=5)
    # the 8x8 convolutions in creation order: lower1 (the region's first module), upper1 of the level below, lower3 (its last)
    c8 = [c for c in conv_specs(cfg) if c.h_out == 8]
    assert len(c8) == 9 and c8[1].k == 3 and c8[-1].cout == F
    return cfg, params, ndm, cfgs, coms, c8[1], c8[-1]


@functools.lru_cache(maxsize=None)
def _oracle(F, B):
    """the oracle with bf16 conv operands and in plain fp32: head maps and the region's output layer, computed once per shape"""
    from oracle import net
    cfg, params, ndm, _, _, _, out = _case(F, B)
    res = []
    for kw in ({'conv_operands': 'bf16'}, {}):
        rec = {}
        o = net.forward_eval(cfg, params, ndm, record=rec, **kw)
        res.append([o[k][-1] for k in ('hm_outs', 'hm3_outs', 'um_outs')] + [rec[out.name + '+res']])
    return res


def _handle(be, F, B, bf16, fusion=None):
    cfg, params = _case(F, B)[:2]
    h = be.handle(cfg, B)
    if bf16:
        h.call('dr_set_precision', 1)
    if fusion is not None:
        h.call('dr_set_fusion', fusion)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    return h


def _l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / (np.linalg.norm(np.asarray(b).ravel()) + 1e-12))


@pytest.mark.parametrize('F', [64, 128, 192, 256])
def test_fused_bf16_carries_the_precisions_error_and_nothing_else(be, F):
    """F = 64: one K-group in the half-width convs, idle waves; 128: the fp32 kernel's limit; 192: six half-width tiles on four waves,
    three K-groups; 256: the largest LDS and prefetch.  Measured on MI355X, worst of the four items (fused vs oracle16 | oracle16 vs
    oracle32 | fused vs unfused | unfused vs oracle16): see profiles/hg_fused_bf16.md."""
    if be.name == 'emu' and F != 64:
        pytest.skip('F = %d on CPU fibers is minutes; covered on the GPU' % F)
    B = 2 if be.name == 'emu' else 3
    ndm, out = _case(F, B)[2], _case(F, B)[6]
    o16, o32 = _oracle(F, B)
    h = _handle(be, F, B, bf16=True, fusion=2)
    fused = list(be.forward_eval(h, ndm)) + [be.read_activation(h, out.name, (B, 8, 8, F))]     # (the region's last layer IS in HBM)
    h.call('dr_set_fusion', 1)                                                                   # unfused under bf16
    plain = list(be.forward_eval(h, ndm)) + [be.read_activation(h, out.name, (B, 8, 8, F))]
    h.close()
    for what, a, p, r16, r32 in zip(('hm', 'hm3', 'um', out.name), fused, plain, o16, o32):
        e_prec = _l2(r16, r32)
        print(F, what, 'fused-o16 %.3e  o16-o32 %.3e  fused-o32 %.3e  fused-plain %.3e  plain-o16 %.3e'
              % (_l2(a, r16), e_prec, _l2(a, r32), _l2(a, p), _l2(p, r16)))
        assert e_prec > 1e-3, (what, e_prec)                                  # the bars below are not vacuous: this is bf16
        assert _l2(a, r16) <= e_prec + 1e-5, (what, _l2(a, r16), e_prec)
        assert _l2(a, r32) <= 1.25 * e_prec + 1e-5, (what, _l2(a, r32), e_prec)
        assert _l2(a, p) <= _l2(p, r16) + 1e-5, (what, _l2(a, p), _l2(p, r16))   # summation order and rare 2^-9 rounding flips


def test_fused_bf16_is_what_ran_and_the_default_did_not_move(be):
    from densereg_amd._lib import DenseRegError
    F, B = 64, 2
    ndm, inner = _case(F, B)[2], _case(F, B)[5]                                # the 3x3 of lower1 at 8x8: inside the region
    h = _handle(be, F, B, bf16=True, fusion=2)
    be.forward_eval(h, ndm)
    with pytest.raises(DenseRegError):                                         # it lived in LDS
        be.read_activation(h, inner.name, (B, 8, 8, F // 2))
    h.close()
    h = _handle(be, F, B, bf16=True)                                           # the default: every op of a bf16 forward is a launch
    be.forward_eval(h, ndm)
    assert np.isfinite(be.read_activation(h, inner.name, (B, 8, 8, F // 2))).all()
    h.close()
    h = _handle(be, F, B, bf16=False, fusion=2)                                # on an fp32 handle 2 is 1
    a = be.forward_eval(h, ndm)
    h.call('dr_set_fusion', 1)
    for x, y in zip(a, be.forward_eval(h, ndm)):
        np.testing.assert_array_equal(x, y)
    h.close()


def test_fused_bf16_is_deterministic_and_feeds_the_vote(be):
    F, B = 64, 2
    _, _, ndm, cfgs, coms = _case(F, B)[:5]
    h = _handle(be, F, B, bf16=True, fusion=2)
    maps = be.forward_eval(h, ndm)
    for x, y in zip(maps, be.forward_eval(h, ndm)):
        np.testing.assert_array_equal(x, y)
    xyz = be.infer(h, ndm, cfgs, coms)
    assert xyz.shape == (B, 3 * J) and np.isfinite(xyz).all()
    np.testing.assert_array_equal(xyz, be.vote(h, *maps, ndm, cfgs, coms))      # the vote is fp32 on whatever maps it is given
    h.close()
