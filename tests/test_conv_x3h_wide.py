"""conv_x3hw.h: the LDS-resident 3x3 halo kernel on 256-row blocks for 64- and 128-pixel-wide images -- against the fp64 definition and,
bit for bit, against conv_x3_kernel on the same layer (output and BatchReNorm partial sums), through the training executors, and its
static resources."""
import ctypes as C

import numpy as np
import pytest

from densereg_amd import _lib
from tests.common import flat_grads_by_name, ref_conv2d

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


CASES = [
    # (B, H, W, Cin, Cout): a block is 256 rows = four image rows at W = 64, two at W = 128
    (1, 4, 64, 24, 128),       # one block per image: every halo row lies outside
    (2, 8, 64, 35, 256),       # two blocks per image, two images (halo rows from the neighbour, never from the other image), Cin % 4, two column blocks
    (1, 8, 64, 16, 128),       # one chunk only
    (1, 2, 128, 40, 128), (2, 4, 128, 20, 128),
    (1, 8, 64, 64, 64), (1, 4, 64, 78, 78), (1, 4, 128, 32, 64), (1, 2, 128, 65, 65),      # the 64- and 96-column tiles
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_halo_kernel_on_wide_images_is_conv_x3_bit_for_bit(be, case):
    B, H, W, Cin, Cout = case
    rng = np.random.default_rng(hash(case) % 2**31 + 9)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    x *= np.exp(rng.uniform(-6, 6, x.shape)).astype(np.float32)             # operands across twelve binades: every split term matters
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.standard_normal(Cout).astype(np.float32)
    res = rng.standard_normal((B, H, W, Cout)).astype(np.float32)
    outs = {}
    for mode in (2, 7):
        try:
            assert be.dbg.dr_dbg_force_x3(mode) == 0
            n_hw, n_h = be.dbg.dr_dbg_x3hw_launches(), be.dbg.dr_dbg_x3h_launches()
            outs[mode] = be.conv2d(x, w, scale, shift, True, res, want_stats=True)
            assert be.dbg.dr_dbg_x3hw_launches() - n_hw == (1 if mode == 2 else 0)
            assert be.dbg.dr_dbg_x3h_launches() == n_h
        finally:
            be.dbg.dr_dbg_force_x3(be.x3_default)
    np.testing.assert_array_equal(outs[2][0], outs[7][0])
    np.testing.assert_array_equal(outs[2][1], outs[7][1])
    yr, _ = ref_conv2d(x, w, scale, shift, True, res)
    err = float(np.abs(outs[2][0] - yr).max() / (np.abs(yr).max() + 1e-12))
    print('conv_x3hw vs fp64: %.2e' % err)
    assert err < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize('in_hw,B', [(256, 2), (512, 1)])
def test_training_micro_step_is_bit_equal_with_and_without_the_kernel(gpu, in_hw, B):
    """Forward (train-mode statistics), input gradients and weight gradients of one micro-step through the executors: the full-resolution
    3x3 layers on conv_x3hw_kernel (mode 2) and on conv_x3_kernel (mode 7)."""
    from densereg_amd.data.synthetic import make_crops
    from oracle import net, pose
    from oracle.graph import NetConfig
    cfg = NetConfig(1, 32, 4, in_hw=in_hw)
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=11, hw=in_hw)
    ndm = pose.norm_dm(dm, coms)
    params = net.make_test_params(cfg, ndm, seed=7)
    poses = np.ascontiguousarray(poses[:, :3 * cfg.num_jnt])
    m, J = cfg.out_hw, cfg.num_jnt
    runs = []
    for mode in (2, 7):
        try:
            assert gpu.dbg.dr_dbg_force_x3(mode) == 0
            n_hw = gpu.dbg.dr_dbg_x3hw_launches()
            h = _lib.Handle(gpu.dbg, cfg.num_stack, cfg.num_fea, cfg.num_jnt, in_hw, cfg.kernel_size, B, 0, True)   # (the library dr_dbg_force_x3 speaks to)
            h.load_params(params)
            h.call('dr_finalize_params', gpu.stream)
            h.call('dr_zero_grad', gpu.stream)
            d_in = [gpu.dev(a) for a in (ndm, poses, cfgs, coms)]
            d_lo = gpu.empty((4,))
            h.call('dr_forward_train', B, gpu.ptr(d_in[0]), 0, None, C.c_uint64(0), gpu.stream)
            h.call('dr_loss', B, *[gpu.ptr(a) for a in d_in], gpu.ptr(d_lo), gpu.stream)
            h.call('dr_backward', B, gpu.stream)
            maps = [gpu.empty((B, m, m, J)), gpu.empty((B, m, m, J)), gpu.empty((B, m, m, 3 * J))]
            h.call('dr_read_maps', B, 0, *[gpu.ptr(a) for a in maps], gpu.stream)
            gpu.sync()
            runs.append(([gpu.host(a).copy() for a in maps], flat_grads_by_name(gpu, h, cfg)))
            h.close()
            assert (gpu.dbg.dr_dbg_x3hw_launches() > n_hw) == (mode == 2)
        finally:
            gpu.dbg.dr_dbg_force_x3(gpu.x3_default)
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)
    for n in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][n], runs[1][1][n], err_msg=n)


def test_static_resources_of_every_instantiation():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import kernel_resources
    rows = [(n, r) for n, r in kernel_resources.collect() if n.startswith('dr::conv_x3hw_kernel<')]
    assert len(rows) == 6, [n for n, _ in rows]
    for n, r in rows:
        want = 4 if n.startswith('dr::conv_x3hw_kernel<128,') else 2
        assert r['scratch'] == 0 and 0 < r['lds'] <= 160 * 1024 and r['occ'] >= want, (n, r)
