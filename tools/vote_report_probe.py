#!/usr/bin/env python
"""What the vote report costs: vote_kernel against vote_report_kernel with every member and with `uvd` only (plus `hm_peak` alone
and everything but it: where the time goes), same process, same maps, through the library's own profile hooks (HIP events around
the launch; `Handle.profile` / `profile_read`).

    python tools/vote_report_probe.py > vote_report_probe.md

Shapes: BASELINE config 2's vote (B=40, J=16, 32x32 maps) and 64x64 maps (B=40, J=14).  Per variant: PROBE_WARMUP launches, then
the median over PROBE_LAUNCHES (default 30) single-launch readings, the variants interleaved launch by launch so that a
clock or neighbour change hits all of them alike.  The plain kernel's time of THIS run is the yardstick.
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from densereg_amd.engine import Engine  # noqa: E402


def maps(B, m, J, in_hw, dev, seed=11):
    """Heat maps with a few bumps per joint over noise, a third of the depth background: what the vote sees after the network."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:m, 0:m].astype(np.float32)
    hm = 0.05 * rng.standard_normal((B, m, m, J)).astype(np.float32)
    for b in range(B):
        for j in range(J):
            cy, cx = rng.uniform(3, m - 3, 2)
            hm[b, :, :, j] += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8.0).astype(np.float32)
    hm3 = np.abs(hm) * np.float32(0.8)
    um = (0.3 * rng.standard_normal((B, m, m, 3 * J))).astype(np.float32)
    tiny = rng.uniform(-0.4, 0.9, (B, m, m, 1)).astype(np.float32)
    tiny[rng.random((B, m, m, 1)) < 0.33] = -1.0
    ndm = np.repeat(np.repeat(tiny, 4, axis=1), 4, axis=2)
    cfg = np.tile(np.array([[480.0 * in_hw / 128, 480.0 * in_hw / 128, in_hw / 2, in_hw / 2, in_hw, in_hw]], np.float32), (B, 1))
    com = np.tile(np.array([[0.0, 0.0, 500.0]], np.float32), (B, 1))
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (hm, hm3, um, ndm, cfg, com)]


def vote_ms(eng):
    rows = [r for r in eng.h.profile_read() if r['name'] == 'vote']
    assert len(rows) == 1 and rows[0]['launches'] == 1, rows
    return rows[0]['total_ms']


def probe(B, J, in_hw, n_warm, n_meas):
    eng = Engine(1, 8, J, in_hw, 3, B, 0, False)
    args = maps(B, in_hw // 4, J, in_hw, eng.device)
    from densereg_amd._lib import VOTE_REPORT_FIELDS
    no_peak = tuple(n for n in VOTE_REPORT_FIELDS if n != 'hm_peak')
    variants = (('vote_kernel', lambda: eng.vote(*args)),
                ('vote_report_kernel, all members', lambda: eng.vote_report(*args)),
                ('vote_report_kernel, uvd only', lambda: eng.vote_report(*args, fields=('uvd',))),
                # where the all-members time goes: the heat-map peak pass on its own, and everything but it
                ('vote_report_kernel, hm_peak only', lambda: eng.vote_report(*args, fields=('hm_peak',))),
                ('vote_report_kernel, all but hm_peak', lambda: eng.vote_report(*args, fields=no_peak)))
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
            times[name].append(vote_ms(eng) * 1e3)
    eng.h.profile(False)
    eng.close()
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    n_warm, n_meas = int(os.environ.get('PROBE_WARMUP', 10)), int(os.environ.get('PROBE_LAUNCHES', 30))
    assert n_meas >= 20
    print('| shape | kernel | median us | min | max | x plain |')
    print('|---|---|---:|---:|---:|---:|')
    for B, J, in_hw in ((40, 16, 128), (40, 14, 256)):
        res = probe(B, J, in_hw, n_warm, n_meas)
        base = res['vote_kernel'][0]
        for name, (med, lo, hi) in res.items():
            print('| B=%d J=%d %dx%d maps | %s | %.1f | %.1f | %.1f | %.2f |' % (B, J, in_hw // 4, in_hw // 4, name, med, lo, hi, med / base))
        sys.stdout.flush()
    print('\n%d launches per variant after %d warm-up launches, interleaved; HIP-event time of the vote launch alone.' % (n_meas, n_warm))


if __name__ == '__main__':
    main()
