#!/usr/bin/env python
"""conv_bf16h.h (the 3x3 halo kernel of the bf16 path, 16- and 32-pixel-wide maps) against conv_igemm's BF kernel on the same layer: time per
launch, the two kernels alternating in one process, several repeats (median and min .. max of each: the spread a difference must beat).
The layer runs on the tile the launcher's rule picks; rows whose rule is not one of the 64-row tiles the halo kernel replaces say so.
With "wide": conv_bf16hw.h (the same kernel on 256-row blocks, 64- and 128-pixel-wide maps) on the layers of in_hw 256 / 512 networks.

    python tools/bf16h_bench.py [repeats]          (the table of profiles/conv_bf16_halo.md)
    python tools/bf16h_bench.py [repeats] wide     (the table of profiles/conv_bf16_halo_wide.md)
"""
import ctypes as C
import os
import statistics
import sys

import torch  # noqa: F401  (before the library: torch brings its own HIP runtime, which must be the first one loaded)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densereg_amd import _lib  # noqa: E402

# (crops, map side, Cin, Cout): the residual modules' 3x3 layers (forward and, Cin <-> Cout, the input gradient) of S2 F128 at 40 crops and at
# the 200-crop training window, of S4 F256, and the 65..96-channel layers of the heads
SHAPES = [(40, 32, 64, 64), (40, 32, 128, 128), (40, 32, 256, 256), (40, 32, 78, 78), (40, 32, 65, 65),
          (200, 32, 64, 64), (200, 32, 128, 128), (200, 32, 256, 256), (200, 32, 78, 78),
          (40, 16, 64, 64), (40, 16, 128, 128), (200, 16, 64, 64), (200, 16, 128, 128), (200, 16, 256, 256),
          (40, 32, 192, 192), (40, 32, 512, 512), (200, 16, 78, 78)]
# wide: the same layers on the 64x64 maps of 256x256 crops (configuration 5: S4 F256) and the 128x128 maps of 512x512 crops, at crop counts
# from half a round to several rounds of one 256-row workgroup per CU (64x64 maps: 16 workgroups per crop and column block; 128x128: 64)
SHAPES_WIDE = [(8, 64, 128, 128), (16, 64, 128, 128), (40, 64, 128, 128), (100, 64, 128, 128),
               (8, 64, 256, 256), (16, 64, 256, 256), (40, 64, 256, 256), (100, 64, 256, 256),
               (16, 64, 64, 64), (40, 64, 64, 64), (100, 64, 64, 64), (40, 64, 78, 78), (100, 64, 78, 78), (100, 64, 65, 65),
               (2, 128, 128, 128), (5, 128, 128, 128), (10, 128, 128, 128), (25, 128, 128, 128),
               (5, 128, 256, 256), (10, 128, 256, 256), (10, 128, 64, 64), (25, 128, 64, 64), (10, 128, 78, 78), (25, 128, 78, 78)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    wide = 'wide' in sys.argv[2:]
    dbg = _lib.load_debug()
    launches = dbg.dr_dbg_bf16hw_launches if wide else dbg.dr_dbg_bf16h_launches
    ms = C.c_float()
    dbg.dr_dbg_force_bf16(1)
    print('| 3x3 layer | conv_igemm BF us (min .. max) | conv_bf16h%s_kernel us (min .. max) | TFLOP/s | igemm / bf16h%s |' % (('w', 'w') if wide else ('', '')))
    print('|---|---:|---:|---:|---:|')
    for stored, (B, hw, cin, cout) in [(s, shape) for s in (0, 1) for shape in (SHAPES_WIDE if wide else SHAPES)]:
        dbg.dr_dbg_force_bf16_storage(stored)                # 1: the input stored as bf16 elements (timing only: arbitrary bit patterns)
        t = {0: [], 1: []}
        ran = True
        for _ in range(reps):
            for on in (0, 1):
                dbg.dr_dbg_force_bf16_halo(on)
                n = launches()
                rc = dbg.dr_dbg_conv_bench(B, hw, hw, cin, cout, 3, -1, 0, 20, C.byref(ms))
                assert rc == 0, rc
                if on:
                    ran = ran and launches() > n
                else:
                    assert launches() == n, 'the kernel under test ran with the switch off'
                t[on].append(ms.value * 1e3)
        dbg.dr_dbg_force_bf16_halo(-1)
        m0, m1 = statistics.median(t[0]), statistics.median(t[1])
        fl = 2.0 * B * hw * hw * 9 * cin * cout
        name = '%dx%d %d->%d, %d crops%s' % (hw, hw, cin, cout, B, ', bf16-stored input' if stored else '')
        if not ran:
            print('| %s | %.1f (%.1f .. %.1f) | not one of the replaced tiles | %.1f | - |' % (name, m0, min(t[0]), max(t[0]), fl / m0 / 1e6))
        else:
            print('| %s | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.1f | %.3fx |'
                  % (name, m0, min(t[0]), max(t[0]), m1, min(t[1]), max(t[1]), fl / m1 / 1e6, m0 / m1))
        sys.stdout.flush()
    dbg.dr_dbg_force_bf16_storage(0)
    dbg.dr_dbg_force_bf16(0)


if __name__ == '__main__':
    main()
