"""conv_bf16hw.h: the 3x3 halo kernel of the bf16 path on 256-row blocks for 64- and 128-pixel-wide maps -- bit for bit against the conv_igemm
BF tile it replaces (output and BatchReNorm partial sums) and against the fp64 definition on bf16-rounded operands, through the handles, and
its static resources.

dr_dbg_force_tile holds both runs on the tiled BF kernel of the case's column tile.  It is needed: at the single-launch shapes the launcher's
own rule is the split-K kernel, and in the 32-feature handles (in_hw 256 at B = 2: 8 192 rows, in_hw 512 at B = 1: 16 384 rows) every 3x3
layer has at most 32 output columns, for which the rule is the split-K kernel (fp32-stored input, at most 128 workgroups) or the 128x32 tile
-- never one of the three 64-row tiles the halo kernel replaces."""
import ctypes as C

import numpy as np
import pytest

from densereg_amd import _lib
from tests.common import bf16_round, flat_grads_by_name, ref_conv2d
from tests.test_conv_bf16_halo import T64, T96, T128, _conv

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


CASES = [
    # (B, H, W, Cin, Cout, tile, also with a bf16-stored input): a block is 256 rows = four image rows at W = 64, two at W = 128
    (1, 4, 64, 24, 128, T128, False),      # one block per image: every halo row lies outside; one partial chunk
    (2, 8, 64, 35, 256, T128, True),       # two blocks per image, two images, Cin % 4, two chunks, two column blocks
    (1, 2, 128, 40, 128, T128, False),
    (2, 4, 128, 72, 128, T128, True),      # three chunks: the double buffer wraps
    (1, 8, 64, 64, 64, T64, False),
    (1, 4, 128, 32, 64, T64, False),       # exactly one full chunk
    (1, 4, 64, 78, 78, T96, False),        # the 96-column tile
    (1, 2, 128, 65, 65, T96, False),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_wide_halo_kernel_is_the_bf_tile_bit_for_bit(be, case):
    B, H, W, Cin, Cout, tile, also_stored = case
    rng = np.random.default_rng(sum(case[:5]) + 9)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    x *= np.exp(rng.uniform(-6, 6, x.shape)).astype(np.float32)             # operands across several binades
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.standard_normal(Cout).astype(np.float32)
    res = rng.standard_normal((B, H, W, Cout)).astype(np.float32)
    try:
        assert be.dbg.dr_dbg_force_bf16(1) == 0 and be.dbg.dr_dbg_force_tile(tile) == 0
        for stored in ((0, 1) if also_stored else (0,)):
            assert be.dbg.dr_dbg_force_bf16_storage(stored) == 0
            xin = bf16_round(x) if stored else x
            outs = {}
            for on in (1, 0):
                assert be.dbg.dr_dbg_force_bf16_halo(on) == 0
                n, n_narrow = be.dbg.dr_dbg_bf16hw_launches(), be.dbg.dr_dbg_bf16h_launches()
                outs[on] = _conv(be, xin, w, scale, shift, res, stored)
                assert be.dbg.dr_dbg_bf16hw_launches() - n == on
                assert be.dbg.dr_dbg_bf16h_launches() == n_narrow
            np.testing.assert_array_equal(outs[1][0], outs[0][0])
            np.testing.assert_array_equal(outs[1][1], outs[0][1])
            yr, _ = ref_conv2d(bf16_round(x), bf16_round(w), scale, shift, True, res)
            err = float(np.abs(outs[1][0] - yr).max() / (np.abs(yr).max() + 1e-12))
            print('conv_bf16hw vs fp64 (stored=%d): %.2e' % (stored, err))
            assert err < 2e-5                                               # the bar of test_conv_bf16_matrix_core_variant
    finally:
        be.dbg.dr_dbg_force_bf16_halo(-1)
        be.dbg.dr_dbg_force_bf16_storage(0)
        be.dbg.dr_dbg_force_tile(-1)
        be.dbg.dr_dbg_force_bf16(0)


def _handle_case(be, training, in_hw, B):
    from densereg_amd.data.synthetic import make_crops
    from oracle import net, pose
    from oracle.graph import NetConfig
    cfg = NetConfig(1, 32, 4, in_hw=in_hw)
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=11, hw=in_hw)
    ndm = pose.norm_dm(dm, coms)
    params = net.make_test_params(cfg, ndm, seed=7)
    h = _lib.Handle(be.dbg, cfg.num_stack, cfg.num_fea, cfg.num_jnt, in_hw, cfg.kernel_size, B, 0, training)   # (the library the hooks speak to)
    h.call('dr_set_precision', 1)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    return cfg, h, ndm, np.ascontiguousarray(poses[:, :3 * cfg.num_jnt]), cfgs, coms


def _on_and_off(be, run):
    """run() with the kernel on and off, every conv held on the 64x128 BF tile (the module docstring says why)."""
    runs = []
    try:
        assert be.dbg.dr_dbg_force_tile(T128) == 0
        for on in (1, 0):
            assert be.dbg.dr_dbg_force_bf16_halo(on) == 0
            n = be.dbg.dr_dbg_bf16hw_launches()
            runs.append(run())
            assert (be.dbg.dr_dbg_bf16hw_launches() > n) == bool(on)
    finally:
        be.dbg.dr_dbg_force_bf16_halo(-1)
        be.dbg.dr_dbg_force_tile(-1)
    return runs


@pytest.mark.gpu
def test_eval_maps_are_bit_equal_with_and_without_the_kernel(gpu):
    """in_hw 256, B = 2.  On the GPU only: on the host-fiber emulator the same test passes too, but takes 40 s."""
    def run():
        cfg, h, ndm, *_ = _handle_case(gpu, False, 256, 2)
        maps = gpu.forward_eval(h, ndm)
        h.close()
        return [np.array(m) for m in maps]
    a, b = _on_and_off(gpu, run)
    for u, v in zip(a, b):
        assert np.isfinite(u).all() and np.abs(u).max() > 0
        np.testing.assert_array_equal(u, v)


@pytest.mark.gpu
@pytest.mark.parametrize('in_hw,B', [(256, 2), (512, 1)])
def test_training_micro_step_is_bit_equal_with_and_without_the_kernel(gpu, in_hw, B):
    """Train-mode forward (statistics rows, bf16-stored activations and raw outputs), loss and backward (the input-gradient convolutions)."""
    def run():
        cfg, h, ndm, poses, cfgs, coms = _handle_case(gpu, True, in_hw, B)
        m, J = cfg.out_hw, cfg.num_jnt
        h.call('dr_zero_grad', gpu.stream)
        d_in = [gpu.dev(a) for a in (ndm, poses, cfgs, coms)]
        d_lo = gpu.empty((4,))
        h.call('dr_forward_train', B, gpu.ptr(d_in[0]), 0, None, C.c_uint64(0), gpu.stream)
        h.call('dr_loss', B, *[gpu.ptr(a) for a in d_in], gpu.ptr(d_lo), gpu.stream)
        h.call('dr_backward', B, gpu.stream)
        maps = [gpu.empty((B, m, m, J)), gpu.empty((B, m, m, J)), gpu.empty((B, m, m, 3 * J))]
        h.call('dr_read_maps', B, 0, *[gpu.ptr(a) for a in maps], gpu.stream)
        gpu.sync()
        out = [gpu.host(a).copy() for a in maps], flat_grads_by_name(gpu, h, cfg)
        h.close()
        return out
    a, b = _on_and_off(gpu, run)
    for u, v in zip(a[0], b[0]):
        assert np.isfinite(u).all()
        np.testing.assert_array_equal(u, v)
    for n in a[1]:
        np.testing.assert_array_equal(a[1][n], b[1][n], err_msg=n)


def test_static_resources_of_every_instantiation():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import kernel_resources
    rows = [(n, r) for n, r in kernel_resources.collect() if n.startswith('dr::conv_bf16hw_kernel<')]
    assert len(rows) == 24, [n for n, _ in rows]                            # three column tiles x two widths x four storage variants
    for n, r in rows:
        want = 4 if n.startswith('dr::conv_bf16hw_kernel<128,') else 2      # sixteen-wave / eight-wave forms
        assert r['scratch'] == 0 and 0 < r['lds'] <= 160 * 1024 and r['occ'] >= want, (n, r)
