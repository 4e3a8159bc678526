#!/usr/bin/env python
"""conv_x3hw.h (the 3x3 halo kernel on 256-row blocks, 64- and 128-pixel-wide maps) against conv_x3_kernel on the same layer: time per
launch, the two kernels alternating in one process, several repeats (median and min .. max of each: the spread a difference must beat).

    python tools/x3hw_bench.py [repeats] > profiles/x3h_wide_microbench.md
"""
import ctypes as C
import os
import statistics
import sys

import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, which must be the first one loaded)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densereg_amd import _lib  # noqa: E402

# (crops, map side, Cin, Cout): the full-resolution 3x3 layers of 256x256 crops (64x64 maps) and 512x512 crops (128x128 maps)
SHAPES = [(40, 64, 128, 128), (40, 64, 64, 64), (40, 64, 78, 78), (200, 64, 128, 128),
          (10, 128, 64, 64), (10, 128, 128, 128), (40, 128, 64, 64), (40, 128, 128, 128), (10, 128, 78, 78), (40, 128, 78, 78),
          # the smallest grids conv_use_x3's rule sends to the x3 family (512 128-row blocks of 128 columns, 1024 of 64 / 96 columns), and
          # crop counts between whole rounds of one 256-row workgroup per CU
          (16, 64, 128, 128), (20, 64, 128, 128), (24, 64, 128, 128), (28, 64, 128, 128), (8, 64, 256, 256), (12, 64, 256, 256), (40, 64, 256, 256),
          (4, 128, 128, 128), (6, 128, 128, 128), (32, 64, 64, 64), (32, 64, 78, 78), (8, 128, 64, 64)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dbg = _lib.load_debug()
    ms = C.c_float()
    print('| 3x3 layer | conv_x3_kernel us (min .. max) | conv_x3hw_kernel us (min .. max) | TFLOP/s | x3 / x3hw |')
    print('|---|---:|---:|---:|---:|')
    for B, hw, cin, cout in SHAPES:
        t = {7: [], 2: []}
        for _ in range(reps):
            for mode in (7, 2):
                dbg.dr_dbg_force_x3(mode)
                n = dbg.dr_dbg_x3hw_launches()
                rc = dbg.dr_dbg_conv_bench(B, hw, hw, cin, cout, 3, -1, 0, 20, C.byref(ms))
                assert rc == 0, rc
                assert (dbg.dr_dbg_x3hw_launches() > n) == (mode == 2), 'the kernel under test is not the one that ran'
                t[mode].append(ms.value * 1e3)
        dbg.dr_dbg_force_x3(-1)
        m7, m2 = statistics.median(t[7]), statistics.median(t[2])
        fl = 2.0 * B * hw * hw * 9 * cin * cout
        print('| %dx%d %d->%d, %d crops | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.1f | %.3fx |'
              % (hw, hw, cin, cout, B, m7, min(t[7]), max(t[7]), m2, min(t[2]), max(t[2]), fl / m2 / 1e6, m7 / m2))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
