#!/usr/bin/env python
"""What the step report costs: dr_step_report in three configurations -- (a) `global` + `global_counts` only, (b) every member
without the histograms, (c) every member with hist_edges() -- against the optimizer step's own adam_kernel on the same handle, same
process, through the library's own profile hooks (HIP events around the launches; `Handle.profile` / `profile_read`).

    python tools/step_report_probe.py > step_report_probe.md

Shape: the NYU training handle (S=2, F=128, J=14: 5.8 M trainable elements in 426 variables) at pipeline depth 1.  The accumulator
holds the gradient of one micro-step of B=8 synthetic crops, so that the values on both sides of the clip and the histogram buckets
are a training step's.  Per variant: PROBE_WARMUP calls, then the median over PROBE_LAUNCHES (default 30) single-call readings, the
variants interleaved call by call so that a clock or neighbour change hits all of them alike.  The report's reading covers all of
its launches (and, with histograms, the two memsets); `adam` is adam_kernel alone (the weight re-packing behind it is not under
that row).  For kernel-by-kernel times run the same script under `rocprofv3 --kernel-trace --stats`, in a run of its own.
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from densereg_amd.data.synthetic import make_crops  # noqa: E402
from densereg_amd.engine import Engine, hist_edges  # noqa: E402
from densereg_amd.model.hourglass_um_crop_tiny import _random_params  # noqa: E402


def row_ms(eng, name):
    rows = [r for r in eng.h.profile_read() if r['name'] == name]
    assert len(rows) == 1 and rows[0]['launches'] == 1, rows
    return rows[0]['total_ms']


def probe(S, F, J, B, dataset, n_warm, n_meas):
    eng = Engine(S, F, J, 128, 3, B, 0, True, pipeline=1)
    eng.load_params(_random_params(eng))
    dm, poses, cfgs, coms, _ = make_crops(B, dataset, seed=7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(eng.device)
    com = t(coms)
    ndm = eng.norm_dm(t(dm), com)
    eng.zero_grad()
    eng.forward_train(ndm, seed=1)
    eng.loss(ndm, t(poses[:, :3 * J]), t(cfgs), com)
    eng.backward(B)
    no_hist = tuple(n for n in ('param_stats', 'grad_stats', 'raw_stats', 'update_stats', 'grad_counts', 'global', 'global_counts'))
    edges = eng.step_report(1e-3, 1.0, 1, fields=('grad_hist',), edges=hist_edges()).edges      # uploaded and checked once
    step = [0]

    def adam():
        step[0] += 1
        eng.apply_adam(1e-3, 1.0, step[0])

    variants = (('dr_apply_adam: adam_kernel', 'adam', adam),
                ('(a) dr_step_report, global + global_counts', 'step_report', lambda: eng.step_report(1e-3, 1.0, step[0] + 1, fields=('global', 'global_counts'))),
                ('(b) dr_step_report, every member without histograms', 'step_report', lambda: eng.step_report(1e-3, 1.0, step[0] + 1, fields=no_hist)),
                ('(c) dr_step_report, every member with hist_edges() (%d edges)' % edges.numel(), 'step_report',
                 lambda: eng.step_report(1e-3, 1.0, step[0] + 1, edges=edges)),
                ('dr_step_report, grad_counts only (no theta, m, v)', 'step_report', lambda: eng.step_report(1e-3, 1.0, step[0] + 1, fields=('grad_counts',))))
    for _ in range(n_warm):
        for _, _, fn in variants:
            fn()
    torch.cuda.synchronize()
    eng.h.profile(True)
    eng.h.profile_read()
    times = {name: [] for name, _, _ in variants}
    for _ in range(n_meas):
        for name, row, fn in variants:
            fn()
            times[name].append(row_ms(eng, row) * 1e3)
    eng.h.profile(False)
    n_train = eng.flat_view('param').numel()
    n_var = len(eng.trainable_names())
    eng.close()
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}, n_train, n_var


def main():
    n_warm, n_meas = int(os.environ.get('PROBE_WARMUP', 10)), int(os.environ.get('PROBE_LAUNCHES', 30))
    assert n_meas >= 20
    print('| handle | call | median us | min | max | x adam_kernel |')
    print('|---|---|---:|---:|---:|---:|')
    for S, F, J, B, dataset in ((2, 128, 14, 8, 'nyu'),):
        res, n_train, n_var = probe(S, F, J, B, dataset, n_warm, n_meas)
        base = next(iter(res.values()))[0]
        for name, (med, lo, hi) in res.items():
            print('| S=%d F=%d J=%d: %d elements, %d variables | %s | %.1f | %.1f | %.1f | %.2f |' % (S, F, J, n_train, n_var, name, med, lo, hi, med / base))
        sys.stdout.flush()
    print('\n%d calls per variant after %d warm-up calls, interleaved; HIP-event time of the launches accounted under `adam` / `step_report`.' % (n_meas, n_warm))


if __name__ == '__main__':
    main()
