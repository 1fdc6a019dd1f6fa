"""Host emulation of ``yh_kd_attention`` / ``yh_kd_attention_kl`` / ``yh_kd_inject`` (csrc/kd.hip) on top of ``fakelib.FakeLib`` —
TEST INFRASTRUCTURE ONLY.

The entries read the row tables exactly as include/yolo_hip.h documents them (``yh_kd_row``: NHWC buffer, pitch, channel offset,
map offset; ``yh_kd_kl_row``: offset and length of a (feature, image) row) and evaluate

    A[q]   = sum_c |y[q, c]|                                   in fp32
    loss   = sum_rows sum_i p_t (log p_t - log p_s) * T * T / batch,   G = p_s - p_t   (softmax over the row at temperature T)
    dy[q, c] = round(float(dy[q, c]) + fl32(fl32(g * coef) * G[q]) * sign(y[q, c]))

with torch CPU ops.  Sums are taken in torch's order, not the kernels' (the GPU tier checks those against fp64); everything the
engine glue decides - which buffers, which lanes, when, with which scalar - is what the kernels see.
"""
import ctypes as C

import numpy as np
import torch

import fakelib
from fakelib import flat, pitched
from engine import hiplib
from engine.hiplib import KdRow, KdKlRow

YH_EINVAL, YH_EALIGN = -1, -2
_NP = {hiplib.YH_F16: np.float16, hiplib.YH_F32: np.float32}


def _table(ptr, n, cls):
    raw = bytes(flat(ptr, n * C.sizeof(cls), np.uint8))
    return [cls.from_buffer_copy(raw[k * C.sizeof(cls):(k + 1) * C.sizeof(cls)]) for k in range(n)]


def _check_table(rows, n_rows, n_chunks):
    if n_rows < 0 or n_chunks < 0:
        return YH_EINVAL
    if n_rows == 0:
        return 0
    if not rows or n_chunks < n_rows:
        return YH_EINVAL
    if fakelib._addr(rows) & 7:
        return YH_EALIGN
    return 1


class FakeLibKd(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.kd_calls = []

    @staticmethod
    def _rows(rows, n_rows):
        out, chunk0, = [], 0
        for r in _table(rows, n_rows, KdRow):
            assert r.chunk0 == chunk0 and r.c % 8 == 0 and r.ld % 8 == 0 and r.c_off % 8 == 0 and r.c_off + r.c <= r.ld
            chunk0 += -(-r.n * r.hw // hiplib.KD_CHUNK)
            out.append(r)
        return out, chunk0

    def yh_kd_attention(self, rows, n_rows, n_chunks, out, stream):
        rc = _check_table(rows, n_rows, n_chunks)
        if rc != 1:
            return rc
        if not out:
            return YH_EINVAL
        table, chunks = self._rows(rows, n_rows)
        assert chunks == n_chunks
        for r in table:
            dt = _NP[r.dtype]
            y = pitched(fakelib._addr(r.y) + r.c_off * np.dtype(dt).itemsize, r.n * r.hw, r.c, r.ld, dt)
            a = torch.from_numpy(np.ascontiguousarray(y)).float().abs().sum(1)
            flat(fakelib._addr(out) + 4 * r.out_off, r.n * r.hw, np.float32)[:] = a.numpy()
        self.kd_calls.append('attention')
        return 0

    def yh_kd_attention_kl(self, a_s, a_t, G, rows, n_rows, partials, loss, T, batch, stream):
        if n_rows < 0 or not T > 0 or batch <= 0 or not loss:
            return YH_EINVAL
        total = torch.zeros((), dtype=torch.float32)
        if n_rows:
            if not a_s or not a_t or not G or not rows or not partials:
                return YH_EINVAL
            part = flat(partials, n_rows, np.float32)
            for k, r in enumerate(_table(rows, n_rows, KdKlRow)):
                s = torch.from_numpy(flat(fakelib._addr(a_s) + 4 * r.off, r.len, np.float32).copy())
                t = torch.from_numpy(flat(fakelib._addr(a_t) + 4 * r.off, r.len, np.float32).copy())
                ls, lt = torch.log_softmax(s / T, 0), torch.log_softmax(t / T, 0)
                ps, pt = ls.exp(), lt.exp()
                flat(fakelib._addr(G) + 4 * r.off, r.len, np.float32)[:] = (ps - pt).numpy()
                part[k] = float(torch.where(pt > 0, pt * (lt - ls), torch.zeros_like(pt)).sum())
            total = torch.from_numpy(part.copy()).sum()
        flat(loss, 1, np.float32)[0] = float(total * np.float32(T * T) / np.float32(batch))
        self.kd_calls.append('kl')
        return 0

    def yh_kd_inject(self, rows, n_rows, n_chunks, G, g, coef, stream):
        rc = _check_table(rows, n_rows, n_chunks)
        if rc != 1:
            return rc
        if not G or not g:
            return YH_EINVAL
        table, chunks = self._rows(rows, n_rows)
        assert chunks == n_chunks
        gc = np.float32(flat(g, 1, np.float32)[0]) * np.float32(coef)
        for r in table:
            dt = _NP[r.dtype]
            es = np.dtype(dt).itemsize
            y = pitched(fakelib._addr(r.y) + r.c_off * es, r.n * r.hw, r.c, r.ld, dt)
            dy = pitched(fakelib._addr(r.dy) + r.c_off * es, r.n * r.hw, r.c, r.ld, dt)
            t = (gc * flat(fakelib._addr(G) + 4 * r.out_off, r.n * r.hw, np.float32)).astype(np.float32)
            dy[:] = (dy.astype(np.float32) + t[:, None] * np.sign(y.astype(np.float32))).astype(dt)
        self.kd_calls.append('inject')
        return 0
