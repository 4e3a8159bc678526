#!/usr/bin/env python
"""What the image report costs: one level-3 ``JointDetectionModel.summary_images`` call (infer_report + read_maps + targets + the
render launch, twelve 128x128 panels per crop) and its render launch alone, at B = 3 (what a training step draws) and B = 40 (a
validation batch), timed with device events.

    python tools/image_report_probe.py > image_report_probe.md

Shape: S=2, F=128, J=14 (nyu), 128x128 crops, 32x32 maps, random weights.  Per row: PROBE_WARMUP calls, then the median over
PROBE_CALLS (default 30) single-call readings, each between two events on the current stream.
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from densereg_amd import flags  # noqa: E402
from densereg_amd.data.synthetic import make_crops  # noqa: E402
from densereg_amd.engine import Panel  # noqa: E402
from densereg_amd.model import hourglass_um_crop_tiny as M  # noqa: E402
from densereg_amd.network import um_v1  # noqa: E402


def timed(fn, n_warm, n_meas):
    for _ in range(n_warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_meas):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    n_warm, n_meas = int(os.environ.get('PROBE_WARMUP', 5)), int(os.environ.get('PROBE_CALLS', 30))
    print('| B | what | median us | min | max |')
    print('|---|---|---|---|---|')
    for B in (3, 40):
        flags.parse(['--dataset', 'nyu', '--is_train', 'False', '--batch_size', str(B), '--debug_level', '3'])
        eng = um_v1.get_engine(14, 128, B, 0, False)
        eng.load_params(M._random_params(eng))
        model = M.JointDetectionModel(M.SyntheticDataset('nyu', 'testing'), um_v1.detect_net, epoch=1)
        dm, poses, cfgs, coms, _ = make_crops(B, 'nyu', seed=7)
        args = tuple(model._t(a) for a in (dm, poses, cfgs, coms))
        ndm = eng.norm_dm(args[0], args[3])
        _, rep = eng.infer_report(ndm, args[2], args[3], fields=('uvd', 'hm_peak'))
        hm, hm3, um = eng.read_maps(B, eng.num_stack - 1)
        gt_hm, gt_hm3, gt_um = eng.targets(ndm, args[1], args[2], args[3])
        hm_pts = rep.hm_uvd_pts

        def joints(pts, space, cfg=None):
            return Panel(args[0], 0, 'greys', pts, space, 128, 'nyu', cfg)
        panels = [joints(rep.uvd, 'uvd'), joints(args[1], 'xyz_mm', args[2]), Panel(gt_hm), Panel(gt_hm3), Panel(hm), Panel(hm3),
                  Panel(args[0], 0, 'greys'), joints(hm_pts, 'uvd'), Panel(gt_um, 0, 'um_xy'), Panel(gt_um, 2), Panel(um, 0, 'um_xy'),
                  Panel(um, 2)]
        rows = (('render launch alone, 12 panels', lambda: eng.render(panels)),
                ('summary_images(level=3), all of it', lambda: model.summary_images(*args, level=3)),
                ('infer_report alone (for scale)', lambda: eng.infer_report(ndm, args[2], args[3], fields=('uvd', 'hm_peak'))))
        for name, fn in rows:
            print('| %d | %s | %.1f | %.1f | %.1f |' % ((B, name) + timed(fn, n_warm, n_meas)))
    flags.parse([])


if __name__ == '__main__':
    main()
