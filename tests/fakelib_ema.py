"""Host emulation of ``yh_ema_update`` (csrc/ema.hip) on top of ``fakelib.FakeLib`` — TEST INFRASTRUCTURE ONLY.

Reads the row table and the rows at their raw host addresses, like the kernel does on the device, validates the arguments as
include/yolo_hip.h documents them, and evaluates the documented formula with numpy, independently of torch:

    t = fl32(ema[i] * d);   ema[i] = fma(one_minus_d, src[i], t)

The fused multiply-add is evaluated as ``fp32(float64(t) + float64(a) * float64(src))``.  The product of two fp32 values is exact in
fp64; the sum is rounded to fp64 and then to fp32, and that second rounding differs from the single rounding of a real fma only when
the fp64 sum lands exactly on the midpoint of two neighbouring fp32 values WITHOUT being the exact sum (every such midpoint is an fp64
number, and rounding is monotonic, so otherwise the exact sum and its fp64 rounding lie on the same side of every midpoint; an exact
sum on a midpoint ties to even either way).  ``midpoints`` counts the
elements where that happened; the tests use fixed seeds and assert that it stays 0, so the emulation there IS the exact evaluation.

Like the kernel, a row is served through its chunks: row r owns chunks ``[chunk0[r], chunk0[r + 1])`` (the last row up to
``n_chunks``), and an element that no chunk covers is not touched - a wrong prefix sum shows as stale elements, not as a pass.
"""
import ctypes as C

import numpy as np

import fakelib
from engine.hiplib import EMA_CHUNK, EmaRow


def fused(ema, src, d, a):
    """(result, midpoint mask) of the documented formula on fp32 arrays ``ema`` / ``src`` with fp32 scalars ``d`` / ``a``."""
    with np.errstate(all='ignore'):
        t = (ema * np.float32(d)).astype(np.float32)
        s64 = t.astype(np.float64) + np.float64(np.float32(a)) * src.astype(np.float64)      # the product is exact
        out = s64.astype(np.float32)
        r64 = out.astype(np.float64)
        toward = np.where(s64 > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        nb64 = np.nextafter(out, toward).astype(np.float64)
        t64, p64 = t.astype(np.float64), np.float64(np.float32(a)) * src.astype(np.float64)
        bb = s64 - t64
        err = (t64 - (s64 - bb)) + (p64 - bb)          # TwoSum: the part of t + p that the fp64 sum lost (0: the sum is exact)
        mid = np.isfinite(s64) & np.isfinite(nb64) & (s64 != r64) & ((s64 - r64) == (nb64 - s64)) & (err != 0)
    return out, mid


def two_roundings(ema, src, d, a):
    """The other candidate, ``t + fl32(one_minus_d * src)``: what the kernel must NOT compute where the two differ."""
    with np.errstate(all='ignore'):
        t = (ema * np.float32(d)).astype(np.float32)
        return (t + (np.float32(a) * src).astype(np.float32)).astype(np.float32)


class FakeLibEma(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.ema_calls = []     # dict(table, n_rows, n_chunks, d, a, rows=[(ema, src, n, chunk0)]) of every call that would launch
        self.midpoints = 0

    def yh_ema_update(self, rows, n_rows, n_chunks, d, one_minus_d, stream):
        if n_rows < 0 or n_chunks < 0:
            return -1
        if n_rows == 0:
            return 0
        base = fakelib._addr(rows)
        if not base or n_chunks < n_rows:
            return -1
        if base & 7:
            return -2
        table = [EmaRow.from_address(base + r * C.sizeof(EmaRow)) for r in range(n_rows)]
        self.ema_calls.append(dict(table=base, n_rows=int(n_rows), n_chunks=int(n_chunks), d=d, a=one_minus_d,
                                   rows=[(r.ema, r.src, int(r.n), int(r.chunk0)) for r in table]))
        for i, row in enumerate(table):
            end = table[i + 1].chunk0 if i + 1 < n_rows else n_chunks
            covered = min(int(row.n), max(0, int(end - row.chunk0)) * EMA_CHUNK)
            if covered <= 0:
                continue
            ema = fakelib.flat(row.ema, covered, np.float32)
            src = fakelib.flat(row.src, covered, np.float32)
            out, mid = fused(ema, src, d, one_minus_d)
            self.midpoints += int(mid.sum())
            ema[:] = out
        return 0
