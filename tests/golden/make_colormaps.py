"""Regenerates ``tests/golden/colormaps.npz``: matplotlib's ``jet`` and ``Greys`` at N = 256 as RGB8, the two colour tables
compiled into the library (``densereg_amd/csrc/render.h``: kRenderLut, one 0x00BBGGRR word per entry).

    python tests/golden/make_colormaps.py            # rewrite the fixture
    python tests/golden/make_colormaps.py --header   # print the two tables as the C initialisers of render.h

matplotlib is needed HERE only; the product never imports it (tests/test_image_report.py compares ``dr_colormap`` with the
fixture, and the fixture with this script where matplotlib imports).
"""
import os
import sys

import numpy as np

NAMES = (('jet', 'jet'), ('greys', 'Greys'))          # fixture key -> matplotlib name; order = DR_PANEL_JET, DR_PANEL_GREYS


def tables():
    import matplotlib
    out = {}
    for key, name in NAMES:
        cmap = matplotlib.colormaps[name].resampled(256)
        out[key] = np.ascontiguousarray(cmap(np.arange(256), bytes=True)[:, :3], np.uint8)
    return out


def header(tabs):
    lines = []
    for key, _ in NAMES:
        t = tabs[key].astype(np.uint32)
        words = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        lines.append('    {   // %s' % key)
        for i in range(0, 256, 8):
            lines.append('        ' + ' '.join('0x%06Xu,' % w for w in words[i:i + 8]))
        lines.append('    },')
    return '\n'.join(lines)


if __name__ == '__main__':
    t = tables()
    if '--header' in sys.argv:
        print(header(t))
    else:
        np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'colormaps.npz'), **t)
