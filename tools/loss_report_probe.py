#!/usr/bin/env python
"""What the loss report costs: the loss pass of dr_loss (loss_kernel + the regulariser's partial sums + losses_out_kernel: what the
library accounts under `loss`) against dr_loss_report with the four loss members only, with every member, and dr_targets --
same process, same forward, through the library's own profile hooks (HIP events around the launches; `Handle.profile` /
`profile_read`).

    python tools/loss_report_probe.py > loss_report_probe.md

Shape: the NYU training shape (S=2, J=14, B=40, 32x32 maps) on a training engine at pipeline depth 1, one dr_forward_train, then the
variants on that forward.  Per variant: PROBE_WARMUP calls, then the median over PROBE_LAUNCHES (default 30) single-call readings,
the variants interleaved call by call so that a clock or neighbour change hits all of them alike.  The loss pass of THIS run is the
yardstick.  (The report is three launches -- maps + partial sums, per-crop sums, the rest -- and the reading covers all three.)
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from densereg_amd.data.synthetic import make_crops  # noqa: E402
from densereg_amd.engine import Engine  # noqa: E402
from densereg_amd.model.hourglass_um_crop_tiny import _random_params  # noqa: E402


def loss_ms(eng):
    rows = [r for r in eng.h.profile_read() if r['name'] == 'loss']
    assert len(rows) == 1 and rows[0]['launches'] == 1, rows
    return rows[0]['total_ms']


def probe(S, F, J, B, dataset, n_warm, n_meas):
    eng = Engine(S, F, J, 128, 3, B, 0, True, pipeline=1)
    eng.load_params(_random_params(eng))
    dm, poses, cfgs, coms, _ = make_crops(B, dataset, seed=7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(eng.device)
    com = t(coms)
    ndm = eng.norm_dm(t(dm), com)
    args = (ndm, t(poses[:, :3 * J]), t(cfgs), com)
    eng.forward_train(ndm, seed=1)
    variants = (('dr_loss: loss_kernel + regulariser + losses_out_kernel', lambda: eng.loss(*args)),
                ('dr_loss_report, the four loss members', lambda: eng.loss_report(*args, fields=('total', 'stack_losses', 'joint_losses', 'crop_losses'))),
                ('dr_loss_report, total only', lambda: eng.loss_report(*args, fields=('total',))),
                ('dr_loss_report, crop_losses only (two launches)', lambda: eng.loss_report(*args, fields=('crop_losses',))),
                ('dr_loss_report, every member', lambda: eng.loss_report(*args)),
                ('dr_targets, three maps', lambda: eng.targets(*args)))
    for _ in range(n_warm):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    eng.h.profile(True)
    eng.h.profile_read()
    times = {name: [] for name, _ in variants}
    for _ in range(n_meas):
        for name, fn in variants:
            fn()
            times[name].append(loss_ms(eng) * 1e3)
    eng.h.profile(False)
    eng.close()
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    n_warm, n_meas = int(os.environ.get('PROBE_WARMUP', 10)), int(os.environ.get('PROBE_LAUNCHES', 30))
    assert n_meas >= 20
    print('| shape | call | median us | min | max | x loss pass |')
    print('|---|---|---:|---:|---:|---:|')
    for S, F, J, B, dataset in ((2, 128, 14, 40, 'nyu'),):
        res = probe(S, F, J, B, dataset, n_warm, n_meas)
        base = next(iter(res.values()))[0]
        for name, (med, lo, hi) in res.items():
            print('| S=%d J=%d B=%d 32x32 maps | %s | %.1f | %.1f | %.1f | %.2f |' % (S, J, B, name, med, lo, hi, med / base))
        sys.stdout.flush()
    print('\n%d calls per variant after %d warm-up calls, interleaved; HIP-event time of the launches accounted under `loss`.' % (n_meas, n_warm))


if __name__ == '__main__':
    main()
