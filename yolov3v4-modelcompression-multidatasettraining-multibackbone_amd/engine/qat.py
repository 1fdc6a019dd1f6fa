"""Quantization-aware training on the device: what `utils/quantized/quantized_google.py` runs when its tensors live on a GPU.
Two services, both on libyolo_hip.so (csrc/qat.hip; a missing library raises - there is no ATen fallback):

* ``observe_update``  the min / max of a tensor (`yh_qat_observe`, one pass) followed by the tracker rule, the first-call flag and
                      the power-of-two scale / zero point (`yh_qat_range_update`, one wave) - reference
                      utils/quantized/quantized_google.py:24-32, :46-55, :70-77, :178-219;
* ``fake_quant``      quantize / round / clamp / dequantize and the call counter (:114-153) as one forward kernel and one backward
                      kernel (`yh_qat_fake_quant_fwd` / `_bwd`) behind a ``torch.autograd.Function``.

Nothing is read back to the host: scale, zero point, flags and counters are read and written in device memory.
"""
import torch

from . import hiplib
from .calib import _dense

_lib_override = None      # tests inject the host emulation of the C ABI here
_force_device = False     # tests: take the device branch for host tensors too (with _lib_override set)


def _lib():
    return _lib_override if _lib_override is not None else hiplib.load()


def eligible(t):
    """The device path covers fp32 tensors on a GPU; everything else (fp16 under autocast, host tensors) takes the torch formulas."""
    return torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() > 0 and (t.is_cuda or _force_device)


def limits(bits, sign=True):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)


def observe(t):
    """[min(t), max(t)] as a 2-element device tensor (both NaN when ``t`` holds one)."""
    lib = _lib()
    t = _dense(t)
    with hiplib.on_device(t):
        need = int(lib.yh_qat_observe_workspace(t.numel()))
        ws = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=t.device)
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        hiplib.check(lib.yh_qat_observe(hiplib.ptr(t), t.numel(), hiplib.ptr(ws), ws.numel() * 4, hiplib.ptr(out), hiplib.stream_ptr()),
                     'qat observe')
    return out


def range_update(minmax, tracker, quantizer=None):
    """One ``update_range`` of ``tracker`` (its ``min_val`` / ``max_val`` / ``first_*`` buffers, in place) with the observed
    ``minmax`` and, when ``quantizer`` is given, one ``update_params`` (its ``scale`` / ``zero_point`` buffers, in place)."""
    lib = _lib()
    averaged = hasattr(tracker, 'first_a')
    first = tracker.first_a if averaged else tracker.first_w
    scale = zp = None
    asym, sign, bits = 0, 1, 8
    if quantizer is not None:
        scale, zp = quantizer.scale, quantizer.zero_point
        asym, sign, bits = int(quantizer.asymmetric), int(bool(quantizer.sign)), int(quantizer.bits)
    with hiplib.on_device(minmax):
        hiplib.check(lib.yh_qat_range_update(hiplib.ptr(minmax), hiplib.ptr(tracker.min_val), hiplib.ptr(tracker.max_val), hiplib.ptr(first),
                                             hiplib.ptr(scale), hiplib.ptr(zp),
                                             hiplib.QAT_TRACK_AVERAGED if averaged else hiplib.QAT_TRACK_GLOBAL,
                                             float(getattr(tracker, 'momentum', 0.0)), asym, sign, bits, hiplib.stream_ptr()), 'qat range update')


def observe_update(t, tracker, quantizer=None):
    range_update(observe(t), tracker, quantizer)


class _FakeQuant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, zero_point, lo, hi, clamp, step):
        lib = _lib()
        xd = _dense(x)
        y = torch.empty_like(xd)      # preserve_format: a dense permuted view keeps its strides, so element i of x is element i of y
        snap = torch.empty(2, dtype=torch.float32, device=xd.device) if clamp else None
        with hiplib.on_device(xd):
            hiplib.check(lib.yh_qat_fake_quant_fwd(hiplib.ptr(xd), hiplib.ptr(y), xd.numel(), hiplib.ptr(scale), hiplib.ptr(zero_point),
                                                   float(lo), float(hi), 1 if clamp else 0, hiplib.ptr(snap), hiplib.ptr(step),
                                                   hiplib.stream_ptr()), 'qat fake-quant forward')
        ctx.clamp, ctx.lo, ctx.hi = clamp, float(lo), float(hi)
        if clamp:
            ctx.save_for_backward(xd, snap)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.clamp:             # the straight-through estimator without a mask: the identity, no launch
            return dy, None, None, None, None, None, None
        lib = _lib()
        x, snap = ctx.saved_tensors
        if dy.dtype != torch.float32 or dy.stride() != x.stride():
            dy = torch.empty_like(x).copy_(dy)
        dx = torch.empty_like(x)
        with hiplib.on_device(x):
            hiplib.check(lib.yh_qat_fake_quant_bwd(hiplib.ptr(x), hiplib.ptr(dy), hiplib.ptr(dx), x.numel(), hiplib.ptr(snap), ctx.lo, ctx.hi,
                                                   hiplib.stream_ptr()), 'qat fake-quant backward')
        return dx, None, None, None, None, None, None


def fake_quant(x, scale, zero_point=None, bits=8, sign=True, clamp=True, step=None):
    """Fake-quantised ``x`` on the int``bits`` grid of the one-element device tensors ``scale`` / ``zero_point`` (None: 0);
    ``step`` (a one-element device tensor or None) is advanced by one."""
    lo, hi = limits(bits, sign)
    return _FakeQuant.apply(x, scale, zero_point, lo, hi, bool(clamp), step)
