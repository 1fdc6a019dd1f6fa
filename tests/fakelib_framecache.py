"""Host emulation of ``yh_mosaic_affine_hsv_batch`` - TEST INFRASTRUCTURE ONLY (see tests/fakelib.py).

``FakeLib.yh_mosaic_affine_hsv`` emulates the cv2 arithmetic and leaves the Pillow arithmetic to ``engine.preprocess.mosaic_reference``;
the batch entry is Pillow only, so this subclass adds the Pillow form of the single-item entry (the descriptor is turned back into an
item whose crops are views of the frames at ``src[k]`` and rendered by ``mosaic_reference``) and the batch entry on top of it: the
library's validation rules, then one emulated ``yh_mosaic_affine_hsv`` per entry."""
import ctypes as C

import numpy as np

from engine import preprocess as pp
from fakelib import FakeLib, flat

YH_EINVAL = -1
ARITH_PILLOW, ARITH_CV2_LINEAR = 0, 1


class _Item:
    pass


def desc_valid(d):
    """csrc/augment.hip mosaic_desc_valid."""
    if not d.dst or d.c not in (1, 3):
        return False
    if d.out_h <= 0 or d.out_w <= 0 or d.canvas_h <= 0 or d.canvas_w <= 0 or not d.divisor > 0:
        return False
    for k in range(4):
        if d.x2a[k] <= d.x1a[k] or d.y2a[k] <= d.y1a[k]:
            continue
        if not d.src[k] or d.x1a[k] < 0 or d.y1a[k] < 0 or d.x2a[k] > d.canvas_w or d.y2a[k] > d.canvas_h:
            return False
        if (d.x1b[k] < 0 or d.y1b[k] < 0 or d.x1b[k] + (d.x2a[k] - d.x1a[k]) > d.src_w[k] or
                d.y1b[k] + (d.y2a[k] - d.y1a[k]) > d.src_h[k] or d.src_pitch[k] < d.src_w[k] * d.c):
            return False
    if d.arith not in (ARITH_PILLOW, ARITH_CV2_LINEAR) or (d.arith == ARITH_CV2_LINEAR and d.hsv and d.c == 3 and not d.lut):
        return False
    return d.out_dtype in (0, 1, 2)


class FakeLibFrameCache(FakeLib):
    def yh_mosaic_affine_hsv(self, dref, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        if not desc_valid(d):
            return YH_EINVAL
        if d.arith != ARITH_PILLOW:
            return super().yh_mosaic_affine_hsv(dref, stream)
        c = d.c
        it = _Item()
        it.canvas, it.out_hw, it.channels = (d.canvas_h, d.canvas_w), (d.out_h, d.out_w), c
        it.inv = np.array([float(v) for v in d.inv])
        it.hsv_gains = np.array([float(v) for v in d.hsv_gain]) if d.hsv and c == 3 else None
        it.flip = bool(d.flip_lr)
        it.parts = []
        for k in range(4):
            if d.x2a[k] <= d.x1a[k] or d.y2a[k] <= d.y1a[k]:
                it.parts.append((None, (0, 0, 0, 0), (0, 0)))
                continue
            pitch = d.src_pitch[k]
            img = np.lib.stride_tricks.as_strided(flat(d.src[k], (d.src_h[k] - 1) * pitch + d.src_w[k] * c, np.uint8),
                                                  shape=(d.src_h[k], d.src_w[k], c), strides=(pitch, c, 1))
            it.parts.append((img, (d.x1a[k], d.y1a[k], d.x2a[k], d.y2a[k]), (d.x1b[k], d.y1b[k])))
        chw = pp.mosaic_reference(it)
        n = c * d.out_h * d.out_w
        if d.out_dtype == 0:
            flat(d.dst, n, np.uint8)[:] = chw.reshape(-1)
        else:      # (OutT)((float)px / divisor)
            dt = np.float32 if d.out_dtype == 1 else np.float16
            flat(d.dst, n, dt)[:] = (chw.astype(np.float32) / np.float32(d.divisor)).astype(dt).reshape(-1)
        return 0

    def yh_mosaic_affine_hsv_batch(self, host_descs, dev_descs, n, stream):
        if not host_descs or not dev_descs or n <= 0 or n > 65535:
            return YH_EINVAL
        first = host_descs[0]
        for i in range(n):
            d = host_descs[i]
            if not desc_valid(d) or d.arith != ARITH_PILLOW:
                return YH_EINVAL
            if (d.out_h, d.out_w, d.c, d.out_dtype, d.divisor) != (first.out_h, first.out_w, first.c, first.out_dtype, first.divisor):
                return YH_EINVAL
        table = C.cast(C.c_void_p(int(dev_descs)), C.POINTER(type(first)))      # the kernel reads the "device" copy
        self.calls.append(('yh_mosaic_affine_hsv_batch', n))
        for i in range(n):
            rc = self.yh_mosaic_affine_hsv(table[i], stream)
            if rc:
                return rc
        return 0
