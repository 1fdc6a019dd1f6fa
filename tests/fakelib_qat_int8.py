"""Host emulation of ``yh_qadd_clamped`` (csrc/quant.hip) and of its plan op on top of ``fakelib.FakeLib`` — TEST INFRASTRUCTURE ONLY.

The arithmetic is the header's formula in torch fp32: both operands re-quantised with round-half-away AND clamped to [-128, 127],
summed in real units, the sum rounded and clamped.  ``FakeLib`` keeps its op table inside ``yh_plan_run_range``; the new op reuses
``yh_qadd_desc``, so a plan records it under ``OP_QADD`` with a ``QAddClampedDesc`` instance (the replay keeps the descriptor's Python
type) and ``yh_qadd`` here dispatches on that type.
"""
import ctypes as C

import numpy as np
import torch

import fakelib
from engine import hiplib
from engine.hiplib import QAddClampedDesc


def qadd_reference(x, a, rx, ra, scale_x, scale_a, inv_scale_sum, clamp_ops):
    """The shortcut arithmetic on int8-valued fp32 tensors (the formulas of include/yolo_hip.h), fp32 throughout."""
    f = float      # the descriptor's fields are fp32 values; a Python scalar keeps the fp32 tensor arithmetic in fp32
    xq, aq = fakelib.rnd_away(x * f(rx)), fakelib.rnd_away(a * f(ra))
    if clamp_ops:
        xq, aq = xq.clamp(-128, 127), aq.clamp(-128, 127)
    return fakelib.rnd_away((xq * f(scale_x) + aq * f(scale_a)) * f(inv_scale_sum)).clamp(-128, 127)


class FakeLibQatInt8(fakelib.FakeLib):
    def _qadd(self, d, clamp_ops):
        x = torch.from_numpy(fakelib.pitched(d.x, d.pixels, d.c, d.ldx, np.int8).astype(np.float32))
        a = torch.from_numpy(fakelib.pitched(d.a, d.pixels, d.c, d.lda, np.int8).astype(np.float32))
        y = qadd_reference(x, a, d.rx, d.ra, d.scale_x, d.scale_a, d.inv_scale_sum, clamp_ops)
        fakelib.pitched(d.y, d.pixels, d.c, d.ldy, np.int8)[:] = y.numpy().astype(np.int8)
        return 0

    def yh_qadd_clamped(self, dref, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        self.calls.append('qadd_clamped')
        return self._qadd(d, True)

    def yh_qadd(self, dref, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        if isinstance(d, QAddClampedDesc):      # a recorded YH_OP_QADD_CLAMPED (see yh_plan_add below)
            return self.yh_qadd_clamped(d, stream)
        return super().yh_qadd(d, stream)

    def yh_plan_add(self, h, kind, dref, nbytes):
        if kind != hiplib.OP_QADD_CLAMPED:
            return super().yh_plan_add(h, kind, dref, nbytes)
        d = dref._obj if hasattr(dref, '_obj') else dref
        assert nbytes == C.sizeof(QAddClampedDesc) and isinstance(d, QAddClampedDesc)
        ops = self.plans[fakelib._addr(h)]['ops']
        ops.append((hiplib.OP_QADD, QAddClampedDesc.from_buffer_copy(bytes(d)), []))
        return len(ops) - 1
