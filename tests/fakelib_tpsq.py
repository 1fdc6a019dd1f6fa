"""Host emulation of the ``yh_tpsq_*`` entry points (csrc/tpsq.hip) on top of ``fakelib_qat.FakeLibQat`` - TEST INFRASTRUCTURE ONLY.

Reads and writes the tensors, the scale parameter, the snapshot and the ``warmup`` flag at their raw host addresses, like the kernels
do on the device, with numpy in fp32, one rounding per operation, in the order include/yolo_hip.h documents.  It does not call the
modules' torch formulas: the tests compare the two.  The sums are taken in float64 and rounded once (the kernels' fp32 trees differ
from that within the bound the tests state).
"""
import numpy as np

import fakelib
import fakelib_qat

F = np.float32
POWERS = 9


def pow2(x):
    """The header's pow2: +-0 -> +0, +inf -> +inf, negative / NaN -> NaN, else m 2^e -> 2^e if m > 0.75 else 2^(e-1)."""
    x = F(x)
    if x == 0:
        return F(0)
    return fakelib_qat.nearest_pow2(x)


def _sign(v):
    return ((0 < v).astype(F) - (v < 0).astype(F)).astype(F)


def _chain(x, p, qmul):
    with np.errstate(all='ignore'):
        a, b = (x + p).astype(F), (x - p).astype(F)
        c = (F(0.5) * (np.abs(a) - np.abs(b)).astype(F)).astype(F)
        m = (c * qmul).astype(F)
        q = (m / p).astype(F)
        r = (_sign(q) * np.floor((np.abs(q) + F(0.5)).astype(F))).astype(F)
    return a, b, m, r


def _fake_quant(x, p, qmul, qdiv):
    with np.errstate(all='ignore'):
        return ((_chain(x, p, qmul)[3] * p).astype(F) / qdiv).astype(F)


def _q(bits):
    return F((1 << (bits - 1)) - 1), F(1 << (bits - 1))


def _blocks(count):
    return max(1, min(1024, -(-count // 4096)))


class FakeLibTpsq(fakelib_qat.FakeLibQat):
    def yh_tpsq_fake_quant_fwd(self, x, y, count, scale, bits, snapshot, stream):
        if not (x and y and scale and snapshot) or count <= 0 or not 2 <= bits <= 24:
            return -1
        self.qat_calls.append('tpsq_fwd')
        s = fakelib.flat(scale, 1, F)
        s0 = s[0]
        p = pow2(s0)
        fakelib.flat(snapshot, 2, F)[:] = (s0, p)
        s[0] = p
        fakelib.flat(y, count, F)[:] = _fake_quant(fakelib.flat(x, count, F), p, *_q(bits))
        return 0

    def yh_tpsq_grad_workspace(self, count):
        return 0 if count <= 0 else 4 * 4 * _blocks(count)

    def yh_tpsq_fake_quant_bwd(self, x, dy, dx, count, snapshot, bits, ws, ws_bytes, scale_grad, stream):
        if not (x and dy and dx and snapshot and ws and scale_grad) or count <= 0 or not 2 <= bits <= 24:
            return -1
        if ws_bytes < self.yh_tpsq_grad_workspace(count):
            return -1
        self.qat_calls.append('tpsq_bwd')
        s0, p = fakelib.flat(snapshot, 2, F)
        qmul, qdiv = _q(bits)
        a, b, m, r = _chain(fakelib.flat(x, count, F), p, qmul)
        with np.errstate(all='ignore'):
            g_n = (fakelib.flat(dy, count, F) / qdiv).astype(F)
            g_q = (g_n * p).astype(F)
            g_d = (((g_q / p).astype(F) * qmul).astype(F) * F(0.5)).astype(F)
            g_a, g_b = (g_d * _sign(a)).astype(F), ((-g_d) * _sign(b)).astype(F)
            fakelib.flat(dx, count, F)[:] = (g_a + g_b).astype(F)
            terms = [g_a, -g_b, ((-g_q) * ((m / p).astype(F) / p).astype(F)).astype(F), (g_n * r).astype(F)]
            G = [F(t.astype(np.float64).sum()) for t in terms]
            first, later = F(p / s0), F(p / p)
            total = F(F(F(later * G[3]) + F(later * G[2])) + F(later * G[1])) + F(first * G[0])
        fakelib.flat(scale_grad, 1, F)[0] = total
        return 0

    def yh_tpsq_warmup_workspace(self, count):
        return 0 if count <= 0 else 8 * (1 + 2 * POWERS) * _blocks(count)

    def yh_tpsq_warmup_search(self, x, count, step, bits, ws, ws_bytes, scale, warmup, stream):
        if not (x and step and ws and scale and warmup) or count <= 0 or not 2 <= bits <= 24:
            return -1
        if ws_bytes < self.yh_tpsq_warmup_workspace(count):
            return -1
        self.qat_calls.append('tpsq_warmup')
        v = fakelib.flat(x, count, F)
        st = fakelib.flat(step, 1, F)[0]
        qmul, qdiv = _q(bits)
        with np.errstate(all='ignore'):
            p0 = pow2(st)
            powers = [F(np.ldexp(p0, k)) for k in range(POWERS)]
            v64 = v.astype(np.float64)
            nx = max(np.sqrt((v64 * v64).sum()), 1e-8)
            cos = []
            for p in powers:
                y64 = _fake_quant(v, p, qmul, qdiv).astype(np.float64)
                cos.append(F((v64 * y64).sum() / (nx * max(np.sqrt((y64 * y64).sum()), 1e-8))))
            best, max_step = -1.0, -5
            for i in range(1, 100):
                p = pow2(F(st * F(i)))
                c = F('nan')
                for k in range(POWERS):
                    if p == powers[k]:
                        c = cos[k]
                        break
                if c > best:
                    best, max_step = c, i
            fakelib.flat(scale, 1, F)[0] = F(st * F(max_step))
        w = fakelib.flat(warmup, 1, F)
        w[0] = w[0] + F(-1)
        return 0
