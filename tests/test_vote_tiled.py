"""The tiled vote (``vote_scan_kernel`` + ``vote_finish_kernel``, ``densereg_amd/csrc/vote.h``): 128x128 maps of 512x512
crops, four tiles of 4096 pixels whose top-5 lists are merged.  The bar is the vote's own: BIT-EXACT against the oracle
(``oracle/pose.py``) on identical maps, on the host-fiber emulator (``[emu]``) and on the MI355X (``[gpu]``)."""
import numpy as np
import pytest

from tests.test_vote_report import SENT, _assert_report_equal, _seeded_maps, be, expected_report, infer_report, vote_report  # noqa: F401

IN_HW, M, TILE = 512, 128, 4096


@pytest.mark.parametrize('B,J', [(2, 5), (1, 7)], ids=['B2_J5', 'B1_J7'])
def test_tiled_seeded_random_maps(be, B, J):
    """Every report member and xyz_mm bit for bit; J = 7 leaves the last joint quad with three live waves.  Preconditions on the
    inputs: unique maxima (ties are the crafted test's) and candidates in all four tiles (so the merge is exercised)."""
    from oracle.graph import NetConfig
    maps = _seeded_maps(np.random.default_rng(1), B, M, J, IN_HW)
    flat = maps[0].reshape(B, M * M, J)
    assert ((flat == flat.max(axis=1, keepdims=True)).sum(axis=1) == 1).all()
    xyz_exp, exp = expected_report(*maps)
    assert set(np.unique(exp['can_idx'] // TILE)) == {0, 1, 2, 3}
    h = be.handle(NetConfig(1, 8, J, in_hw=IN_HW), B)
    xyz, got = vote_report(be, h, *maps)
    xyz_plain = be.vote(h, *maps)
    h.close()
    _assert_report_equal(got, exp)
    np.testing.assert_array_equal(xyz, xyz_plain)
    np.testing.assert_array_equal(xyz, xyz_exp)


PLANTED = {                                                     # case -> (planted pixels, hm3 step per pixel, expected can_idx)
    'tile_borders': ([4095, 4096, 8191, 12288, 16383], 0.1, [4095, 4096, 8191, 12288, 16383]),
    'ties_across_tiles': ([100, 5000, 5001, 9000, 13000, 13001, 16000], 0.0, [100, 5000, 5001, 9000, 13000]),
    'all_in_last_tile': ([12293, 12358, 13188, 14288, 16383], 0.1, [12293, 12358, 13188, 14288, 16383]),
    'all_background': ([], 0.0, [0, 1, 2, 3, 4]),
}


@pytest.mark.parametrize('case', list(PLANTED))
def test_tiled_crafted_maps(be, case):
    """Planted winners: refined heat (3 + 1) * (2 - step * k) on foreground, above anything the seeded maps reach (< 3 * 2), at pixels
    that straddle the tile borders / tie across tiles (lower indices win, tf.nn.top_k order) / all sit in the last tile; and an
    all-background crop, where every refined value ties at 0 and the candidates are pixels 0..4."""
    from oracle.graph import NetConfig
    B, J = 1, 5
    pix, step, idx = PLANTED[case]
    hm, hm3, um, ndm, cfg, com = _seeded_maps(np.random.default_rng(2), B, M, J, IN_HW)
    assert ((hm + 1) * hm3).max() < 6 and np.isfinite(hm).all()
    for k, px in enumerate(pix):
        v, u = divmod(px, M)
        hm[:, v, u, :] = 3.0
        hm3[:, v, u, :] = np.float32(2.0 - step * k)
        ndm[:, 4 * v:4 * v + 4, 4 * u:4 * u + 4, :] = 0.5
    if not pix:
        ndm[:] = -1.0
    maps = (hm, hm3, um, ndm, cfg, com)
    xyz_exp, exp = expected_report(*maps)
    assert (exp['can_idx'] == np.array(idx)).all()
    h = be.handle(NetConfig(1, 8, J, in_hw=IN_HW), B)
    xyz, got = vote_report(be, h, *maps, want=('can_idx', 'can_score'))
    h.close()
    for n in ('can_idx', 'can_score'):
        np.testing.assert_array_equal(got[n][0], exp[n], err_msg=n)
    np.testing.assert_array_equal(xyz, xyz_exp)


@pytest.mark.gpu
def test_tiled_infer_end_to_end(gpu, monkeypatch):
    """512x512 crops through dr_infer (DR_GRAPHS=1: recorded, then replayed) == dr_forward_eval + dr_vote, bit for bit, and
    dr_infer_report's xyz_mm is dr_infer's."""
    from densereg_amd.data.synthetic import make_crops
    from oracle import net, pose
    from oracle.graph import NetConfig
    monkeypatch.setenv('DR_GRAPHS', '1')
    cfg, B = NetConfig(1, 8, 5, in_hw=IN_HW), 2
    dm, _, cfgs, coms, _ = make_crops(B, 'icvl', seed=81, hw=IN_HW)
    ndm = pose.norm_dm(dm, coms)
    h = gpu.handle(cfg, B)
    h.load_params(net.init_params(cfg))
    h.call('dr_finalize_params', gpu.stream)
    xyz_split = gpu.vote(h, *gpu.forward_eval(h, ndm), ndm, cfgs, coms)
    assert np.isfinite(xyz_split).all()
    d = [gpu.dev(np.ascontiguousarray(a, np.float32)) for a in (ndm, cfgs, coms)]
    xyz = gpu.empty((B, 3 * cfg.num_jnt))
    for _ in range(2):
        xyz.fill_(SENT)
        h.call('dr_infer', B, *[gpu.ptr(a) for a in d], gpu.ptr(xyz), gpu.stream)
        gpu.sync()
        np.testing.assert_array_equal(gpu.host(xyz), xyz_split)
    xyz_rep, _ = infer_report(gpu, h, ndm, cfgs, coms)
    h.close()
    np.testing.assert_array_equal(xyz_rep, xyz_split)
