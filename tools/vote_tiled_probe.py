#!/usr/bin/env python
"""One vote shape, launched over and over, for a kernel-trace run of its own (-> profiles/vote_tiled.md):

    rocprofv3 --kernel-trace -d out -o vote -- python tools/vote_tiled_probe.py B J in_hw
    python tools/vote_tiled_probe.py --read out/vote_results.db

in_hw = 512 runs the tiled path (vote_scan_kernel + vote_finish_kernel on 128x128 maps), in_hw = 256 the single-launch vote_kernel on
64x64 maps, the yardstick.  One shape per process, so the kernel times of the trace belong to that shape.  PROBE_WARMUP launches
(default 10) and PROBE_LAUNCHES (default 200) timed ones, all of them in the trace; prints the algorithmic bytes per launch,
(5J+1) * npix * 4 per crop, which over the kernel time is the achieved rate.  --read prints, per vote kernel of a trace database,
the median / min / max duration with the first PROBE_WARMUP records dropped.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = int(os.environ.get('PROBE_WARMUP', 10))


def read(path):
    import sqlite3
    import statistics
    times = {}
    for name, ns in sqlite3.connect(path).execute("select name, end - start from kernels where name like '%vote%' order by start"):
        times.setdefault(name.split('(')[0], []).append(ns / 1e3)
    for name, t in times.items():
        t = t[WARMUP:]
        print('%-40s %d launches: median %.1f us, min %.1f, max %.1f' % (name, len(t), statistics.median(t), min(t), max(t)))


def main():
    import torch
    from densereg_amd.engine import Engine
    from tools.vote_report_probe import maps
    B, J, in_hw = (int(a) for a in sys.argv[1:4])
    n = WARMUP + int(os.environ.get('PROBE_LAUNCHES', 200))
    eng = Engine(1, 8, J, in_hw, 3, B, 0, False)
    args = maps(B, in_hw // 4, J, in_hw, eng.device)
    for _ in range(n):
        eng.vote(*args)
    torch.cuda.synchronize()
    eng.close()
    m = in_hw // 4
    print('B=%d J=%d %dx%d maps: %d launches, %d algorithmic bytes per launch' % (B, J, m, m, n, B * (5 * J + 1) * m * m * 4))


if __name__ == '__main__':
    read(sys.argv[2]) if sys.argv[1] == '--read' else main()
