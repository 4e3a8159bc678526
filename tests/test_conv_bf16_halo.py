"""conv_bf16h.h: the LDS-resident 3x3 halo kernel of the bf16 path -- bit for bit against the conv_igemm BF tile it replaces (output and
BatchReNorm partial sums) and against the fp64 definition on bf16-rounded operands, through the handles, and its static resources.

The small shapes here would run on the split-K kernel by the launcher's own rule (grids that cannot fill the chip), which the halo kernel never
replaces: dr_dbg_force_tile holds both runs on the tiled BF kernel of the case's column tile, as tests/test_forward_parity.py does."""
import ctypes as C

import numpy as np
import pytest

from densereg_amd import _lib
from tests.common import bf16_round, flat_grads_by_name, ref_conv2d

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]
T128, T64, T96 = 1, 3, 7                    # the 64x128, 64x64 and 64x96 tiles (ids of dr_dbg_force_tile)


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


CASES = [
    # (B, H, W, Cin, Cout, tile, also with a bf16-stored input): a block is 128 rows = four image rows at W = 32, eight at W = 16
    (1, 4, 32, 24, 128, T128, False),      # one block per image: every halo row lies outside; one partial chunk
    (2, 8, 32, 35, 256, T128, True),       # two blocks per image, two images (halo rows from the neighbour, never from the other image), Cin % 4, two chunks, two column blocks
    (1, 8, 16, 64, 64, T64, False), (2, 16, 16, 40, 128, T128, True),
    (1, 4, 32, 78, 78, T96, False),        # the 96-column tile
    (1, 4, 32, 32, 64, T64, False),        # exactly one full chunk
]


def _conv(be, x, w, scale, shift, res, stored):
    """Fused conv + statistics; stored: x handed over as bf16 elements (channel groups of four zero-padded, NaN behind the tensor)."""
    if not stored:
        return be.conv2d(x, w, scale, shift, True, res, want_stats=True)
    B, H, W, Cin = x.shape
    Cout, x_cs = w.shape[-1], -(-Cin // 4) * 4
    xp = np.zeros((B, H, W, x_cs), np.float32)
    xp[..., :Cin] = x
    bits = np.concatenate([(xp.view(np.uint32) >> 16).astype(np.uint16).reshape(-1), np.full(64, 0x7FC0, np.uint16)])
    d = [be.dev(a) for a in (bits, w, scale, shift, res, np.zeros((B, H, W, Cout), np.float32), np.zeros((2, Cout), np.float64))]
    rc = be.dbg.dr_dbg_conv2d(B, H, W, Cin, Cout, 3, be.ptr(d[0]), x_cs, be.ptr(d[1]), be.ptr(d[2]), be.ptr(d[3]), 1, be.ptr(d[4]), Cout,
                              None, 0.0, be.ptr(d[5]), Cout, be.ptr(d[6]), be.stream)
    assert rc == 0, rc
    be.sync()
    return be.host(d[5]).copy(), be.host(d[6]).copy()


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c[:5])))
def test_halo_kernel_is_the_bf_tile_bit_for_bit(be, case):
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
                n = be.dbg.dr_dbg_bf16h_launches()
                outs[on] = _conv(be, xin, w, scale, shift, res, stored)
                assert be.dbg.dr_dbg_bf16h_launches() - n == on
            np.testing.assert_array_equal(outs[1][0], outs[0][0])
            np.testing.assert_array_equal(outs[1][1], outs[0][1])
            yr, _ = ref_conv2d(bf16_round(x), bf16_round(w), scale, shift, True, res)
            err = float(np.abs(outs[1][0] - yr).max() / (np.abs(yr).max() + 1e-12))
            print('conv_bf16h vs fp64 (stored=%d): %.2e' % (stored, err))
            assert err < 2e-5                                               # the bar of test_conv_bf16_matrix_core_variant
    finally:
        be.dbg.dr_dbg_force_bf16_halo(-1)
        be.dbg.dr_dbg_force_bf16_storage(0)
        be.dbg.dr_dbg_force_tile(-1)
        be.dbg.dr_dbg_force_bf16(0)


def _handle_case(be, training):
    from densereg_amd.data.synthetic import make_crops
    from oracle import net, pose
    from oracle.graph import NetConfig
    cfg, B = NetConfig(1, 32, 4, in_hw=128), 2
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=11, hw=128)
    ndm = pose.norm_dm(dm, coms)
    params = net.make_test_params(cfg, ndm, seed=7)
    h = _lib.Handle(be.dbg, cfg.num_stack, cfg.num_fea, cfg.num_jnt, 128, cfg.kernel_size, B, 0, training)     # (the library the hooks speak to)
    h.call('dr_set_precision', 1)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    return cfg, B, h, ndm, np.ascontiguousarray(poses[:, :3 * cfg.num_jnt]), cfgs, coms


def _on_and_off(be, run):
    """run() with the kernel on and off (every conv held on the 64x128 BF tile: at B = 2 the launcher's rule is the split-K kernel)."""
    runs = []
    try:
        assert be.dbg.dr_dbg_force_tile(T128) == 0
        for on in (1, 0):
            assert be.dbg.dr_dbg_force_bf16_halo(on) == 0
            n = be.dbg.dr_dbg_bf16h_launches()
            runs.append(run())
            assert (be.dbg.dr_dbg_bf16h_launches() > n) == bool(on)
    finally:
        be.dbg.dr_dbg_force_bf16_halo(-1)
        be.dbg.dr_dbg_force_tile(-1)
    return runs


def test_eval_maps_are_bit_equal_with_and_without_the_kernel(be):
    def run():
        cfg, B, h, ndm, *_ = _handle_case(be, False)
        maps = be.forward_eval(h, ndm)
        h.close()
        return [np.array(m) for m in maps]
    a, b = _on_and_off(be, run)
    for u, v in zip(a, b):
        assert np.isfinite(u).all() and np.abs(u).max() > 0
        np.testing.assert_array_equal(u, v)


@pytest.mark.gpu
def test_training_micro_step_is_bit_equal_with_and_without_the_kernel(gpu):
    """Train-mode forward (statistics rows, bf16-stored activations and raw outputs), loss and backward (the input-gradient convolutions)."""
    def run():
        cfg, B, h, ndm, poses, cfgs, coms = _handle_case(gpu, True)
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
    rows = [(n, r) for n, r in kernel_resources.collect() if n.startswith('dr::conv_bf16h_kernel<')]
    assert len(rows) == 24, [n for n, _ in rows]                            # three column tiles x two widths x four storage variants
    for n, r in rows:
        want = 4 if n.startswith('dr::conv_bf16h_kernel<128,') else 2
        assert r['scratch'] == 0 and 0 < r['lds'] <= 80 * 1024 and r['occ'] >= want, (n, r)
