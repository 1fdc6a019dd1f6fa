"""Host emulation of the ``yh_qat_*`` entry points (csrc/qat.hip) on top of ``fakelib.FakeLib`` - TEST INFRASTRUCTURE ONLY.

Reads and writes the tensors, scales, flags and counters at their raw host addresses, like the kernels do on the device, with numpy
in fp32, one rounding per operation, in the order include/yolo_hip.h documents.  It does not call the modules' torch formulas: the
tests compare the two.
"""
import numpy as np

import fakelib

F = np.float32


def _one(p):
    return fakelib.flat(p, 1, F)


def nearest_pow2(x):
    """x = m 2^e, m in [0.5, 1): 2^e if m > 0.75 else 2^(e-1); 0 -> 0, inf -> inf, NaN / negative -> NaN."""
    x = F(x)
    if np.isnan(x) or x < 0:
        return F('nan')
    if x == 0 or np.isinf(x):
        return x
    m, e = np.frexp(x)
    return F(np.ldexp(F(1), int(e) if m > F(0.75) else int(e) - 1))


def _nan_min(a, b):
    return F('nan') if np.isnan(a) or np.isnan(b) else min(a, b)


def _nan_max(a, b):
    return F('nan') if np.isnan(a) or np.isnan(b) else max(a, b)


def _round(x, s, zp):
    with np.errstate(all='ignore'):
        u = (x / s).astype(F) + zp
        return np.copysign(np.floor(np.abs(u) + F(0.5)), u).astype(F)


def _clamp(r, lo, hi):
    return np.where(np.isnan(r), r, np.minimum(np.maximum(r, lo), hi)).astype(F)


class FakeLibQat(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.qat_calls = []      # name of every call that would launch

    def yh_qat_observe_workspace(self, count):
        return 0 if count <= 0 else 3 * 4 * max(1, min(1024, -(-count // 4096)))

    def yh_qat_observe(self, t, count, ws, ws_bytes, minmax, stream):
        if not (t and ws and minmax) or count <= 0 or ws_bytes < self.yh_qat_observe_workspace(count):
            return -1
        self.qat_calls.append('observe')
        v = fakelib.flat(t, count, F)
        out = fakelib.flat(minmax, 2, F)
        out[:] = (F('nan'), F('nan')) if np.isnan(v).any() else (v.min(), v.max())
        return 0

    def yh_qat_range_update(self, minmax, min_val, max_val, first, scale, zero_point, tracker, momentum, asymmetric, is_signed, bits, stream):
        if not (minmax and min_val and max_val and first) or not 2 <= bits <= 24 or tracker not in (0, 1):
            return -1
        self.qat_calls.append('update')
        mn, mx = fakelib.flat(minmax, 2, F)
        lo_b, hi_b, first_b = _one(min_val), _one(max_val), _one(first)
        lo, hi = lo_b[0], hi_b[0]
        with np.errstate(all='ignore'):
            if first_b[0] == 0:
                first_b[0] = first_b[0] + F(1)
                lo, hi = lo + mn, hi + mx
            elif tracker == 1:
                m, om = F(momentum), F(1.0 - momentum)
                lo, hi = F(lo * om) + F(mn * m), F(hi * om) + F(mx * m)
            else:
                zl, zh = lo + (-lo), hi + (-hi)
                lo, hi = zl + _nan_min(zl, mn), zh + _nan_max(zh, mx)
            lo_b[0], hi_b[0] = lo, hi
            if not scale:
                return 0
            q_lo = F(-(1 << (bits - 1))) if is_signed else F(0)
            q_hi = F((1 << (bits - 1)) - 1) if is_signed else F((1 << bits) - 1)
            if not asymmetric:
                s = F(nearest_pow2(_nan_max(abs(lo), abs(hi))) / max(abs(q_lo), abs(q_hi)))
                _one(scale)[0] = s
                if zero_point:
                    _one(zero_point)[0] = 0
            else:
                s = F(nearest_pow2(F(hi - lo)) / F(q_hi - q_lo))
                _one(scale)[0] = s
                if zero_point:
                    _one(zero_point)[0] = np.rint(F(q_hi - F(hi / s)))
        return 0

    def yh_qat_fake_quant_fwd(self, x, y, count, scale, zero_point, lo, hi, do_clamp, snapshot, step, stream):
        if not (x and y and scale) or count <= 0 or (do_clamp and not lo < hi):
            return -1
        self.qat_calls.append('fwd')
        s = _one(scale)[0]
        zp = _one(zero_point)[0] if zero_point else F(0)
        r = _round(fakelib.flat(x, count, F), s, zp)
        if do_clamp:
            r = _clamp(r, F(lo), F(hi))
        with np.errstate(all='ignore'):
            fakelib.flat(y, count, F)[:] = ((r - zp).astype(F) * s).astype(F)
        if snapshot:
            fakelib.flat(snapshot, 2, F)[:] = (s, zp)
        if step:
            _one(step)[0] += F(1)
        return 0

    def yh_qat_fake_quant_bwd(self, x, dy, dx, count, snapshot, lo, hi, stream):
        if not (x and dy and dx and snapshot) or count <= 0 or not lo < hi:
            return -1
        self.qat_calls.append('bwd')
        s, zp = fakelib.flat(snapshot, 2, F)
        r = _round(fakelib.flat(x, count, F), s, zp)
        with np.errstate(all='ignore'):
            g = np.where((r >= F(lo)) & (r <= F(hi)), (fakelib.flat(dy, count, F) * s).astype(F), F(0))
            fakelib.flat(dx, count, F)[:] = (g / s).astype(F)
        return 0
