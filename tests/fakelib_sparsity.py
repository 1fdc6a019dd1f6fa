"""Host emulation of ``yh_bn_l1_subgrad`` (csrc/sparsity.hip) on top of ``fakelib.FakeLib`` — TEST INFRASTRUCTURE ONLY.

Reads the row table and the rows at their raw host addresses, like the kernel does on the device, and evaluates the documented
formula with numpy in fp32: ``grad[i] = grad[i] + (s * sign(gamma[i]))`` with ``(0 < x) - (x < 0)`` as the sign.
"""
import ctypes as C

import numpy as np

import fakelib
from engine.hiplib import BnL1Row


class FakeLibSparsity(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.l1_calls = []      # (first, last, s) of every call that would launch

    def yh_bn_l1_subgrad(self, rows, first, last, s, stream):
        if first < 0 or last < first:
            return -1
        if last == first:
            return 0
        base = fakelib._addr(rows)
        if not base:
            return -1
        self.l1_calls.append((int(first), int(last), float(s)))
        s32 = np.float32(s)
        for r in range(first, last):
            row = BnL1Row.from_address(base + r * C.sizeof(BnL1Row))
            gamma = fakelib.flat(row.gamma, row.n, np.float32)
            grad = fakelib.flat(row.grad, row.n, np.float32)
            sign = (gamma > 0).astype(np.float32) - (gamma < 0).astype(np.float32)
            grad[:] = grad + s32 * sign
        return 0
