"""Host emulation of the test-time-augmentation entries (csrc/tta.hip, yh_yolo_decode_candidates_tta of csrc/nms.hip) on top of
``fakelib_multiscale.FakeLibMultiscale`` — TEST INFRASTRUCTURE ONLY.

The view walks the descriptor like the kernel does: ``fakelib_multiscale``'s taps (the documented formula in fp32 scalars), the source
columns mirrored when ``flip``, the pad value outside the resized content.  The de-augmentation is numpy fp32 division (IEEE) and
``flip_w - cx``; the fused candidate pass is the decode emulation, that de-augmentation, then the shared filter.
"""
import numpy as np

import fakelib
import fakelib_multiscale
from engine.hiplib import DecodeDesc, TtaViewDesc

F = np.float32


def deaugment_rows(rows, scale, flip_w):
    """In place on an (..., >= 4) fp32 array: cx, cy, w, h / scale, then cx = flip_w - cx when flip_w >= 0."""
    rows[..., :4] = rows[..., :4] / F(scale)
    if flip_w >= 0:
        rows[..., 0] = F(flip_w) - rows[..., 0]


class FakeLibTta(fakelib_multiscale.FakeLibMultiscale):
    def __init__(self):
        super().__init__()
        self.view_calls = []

    def yh_tta_view(self, dref, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        assert isinstance(d, TtaViewDesc)
        if not d.src or not d.dst or min(d.n, d.c, d.ih, d.iw, d.oh, d.ow, d.rh, d.rw) < 1:
            return -1
        if d.rh > d.oh or d.rw > d.ow or d.flip not in (0, 1):
            return -1
        if not (0 < d.scale_h <= 2.0 ** 24 and 0 < d.scale_w <= 2.0 ** 24):
            return -1
        self.view_calls.append((d.n, d.c, d.ih, d.iw, d.oh, d.ow, d.rh, d.rw, d.flip))
        planes = d.n * d.c
        src = fakelib.flat(d.src, planes * d.ih * d.iw, F).reshape(planes, d.ih, d.iw)
        dst = fakelib.flat(d.dst, planes * d.oh * d.ow, F).reshape(planes, d.oh, d.ow)
        xt = fakelib_multiscale._taps(d.iw, d.rw, F(d.scale_w))
        x0 = np.array([t[0] for t in xt])
        x1 = np.array([t[1] for t in xt])
        if d.flip:
            x0, x1 = d.iw - 1 - x0, d.iw - 1 - x1
        wx0 = np.array([t[2] for t in xt], dtype=F)
        wx1 = np.array([t[3] for t in xt], dtype=F)
        dst[:] = F(d.pad_value)
        for y, (y0, y1, hy0, hy1) in enumerate(fakelib_multiscale._taps(d.ih, d.rh, F(d.scale_h))):
            top = wx0 * src[:, y0, x0] + wx1 * src[:, y0, x1]
            bot = wx0 * src[:, y1, x0] + wx1 * src[:, y1, x1]
            dst[:, y, :d.rw] = hy0 * top + hy1 * bot
        return 0

    def yh_tta_deaugment(self, io, n, rows_total, no, row0, nrows, scale, flip_w, stream):
        if not fakelib._addr(io) or min(n, rows_total, nrows) < 1 or no < 4 or row0 < 0 or row0 + nrows > rows_total or not scale > 0:
            return -1
        x = fakelib.flat(io, n * rows_total * no, F).reshape(n, rows_total, no)
        deaugment_rows(x[:, row0:row0 + nrows], scale, flip_w)
        self.calls.append('tta_deaugment')
        return 0

    def yh_yolo_decode_candidates_tta(self, dref, scale, flip_w, conf, ml, class_mask, cand, count, cap, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        if not scale > 0:
            return -1
        rows, nc = d.na * d.ny * d.nx, d.no - 5
        io = np.zeros((d.n, rows, d.no), F)      # the decode emulation's values for this head alone
        e = DecodeDesc.from_buffer_copy(d)
        e.io, e.raw, e.rows_total, e.row_off = io.ctypes.data, None, rows, 0
        self.yh_yolo_decode(e, stream)
        deaugment_rows(io, scale, flip_w)
        mask = fakelib.flat(class_mask, nc, np.uint8) if fakelib._addr(class_mask) else None
        for i in range(d.n):
            self._emit(cand, count, cap, i, self._rows_to_records(io[i], d.row_off, nc, conf, ml, mask))
        self.calls.append('decode_candidates_tta')
        return 0
