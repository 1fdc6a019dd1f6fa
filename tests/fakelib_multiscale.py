"""Host emulation of ``yh_resize_bilinear`` (csrc/resize.hip) on top of ``fakelib.FakeLib`` — TEST INFRASTRUCTURE ONLY.

Walks the descriptor like the kernel does: per-axis taps from the documented formula in fp32 scalars (one rounding per operation),
then one output row at a time from the two source rows at their raw host addresses.
"""
import numpy as np

import fakelib
from engine.hiplib import ResizeDesc

F = np.float32


def _taps(in_size, out_size, scale):
    out = []
    for d in range(out_size):
        s = F(F(scale * F(F(d) + F(0.5))) - F(0.5))
        s = s if s > 0 else F(0)
        i0 = min(int(s), in_size - 1)
        i1 = min(i0 + 1, in_size - 1)
        l1 = F(s - F(i0))
        out.append((i0, i1, F(F(1) - l1), l1))
    return out


class FakeLibMultiscale(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.resize_calls = []

    def yh_resize_bilinear(self, dref, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        assert isinstance(d, ResizeDesc)
        if not d.src or not d.dst or min(d.n, d.c, d.ih, d.iw, d.oh, d.ow) < 1:
            return -1
        if not (0 < d.scale_h <= 2.0 ** 24 and 0 < d.scale_w <= 2.0 ** 24):
            return -1
        self.resize_calls.append((d.n, d.c, d.ih, d.iw, d.oh, d.ow))
        planes = d.n * d.c
        src = fakelib.flat(d.src, planes * d.ih * d.iw, F).reshape(planes, d.ih, d.iw)
        dst = fakelib.flat(d.dst, planes * d.oh * d.ow, F).reshape(planes, d.oh, d.ow)
        xt = _taps(d.iw, d.ow, F(d.scale_w))
        x0 = np.array([t[0] for t in xt])
        x1 = np.array([t[1] for t in xt])
        wx0 = np.array([t[2] for t in xt], dtype=F)
        wx1 = np.array([t[3] for t in xt], dtype=F)
        for y, (y0, y1, hy0, hy1) in enumerate(_taps(d.ih, d.oh, F(d.scale_h))):
            top = wx0 * src[:, y0, x0] + wx1 * src[:, y0, x1]
            bot = wx0 * src[:, y1, x0] + wx1 * src[:, y1, x1]
            dst[:, y, :] = hy0 * top + hy1 * bot
        return 0
