"""TPSQ (learnable power-of-two scales) on the device: what `utils/quantized/quantized_TPSQ.py` runs when its tensors live on a GPU.
Three services on libyolo_hip.so (csrc/tpsq.hip, and csrc/qat.hip for the bias quantiser; a missing library raises - there is no ATen
fallback):

* ``fake_quant``     one quantiser call after warm-up (reference utils/quantized/quantized_TPSQ.py:29-63 Search_Pow2 four times, :79-118
                     clamp / quantize / round / dequantize) as one forward kernel, which also snaps the scale parameter in place, and one
                     backward kernel plus a finishing wave (`yh_tpsq_fake_quant_fwd` / `_bwd`) behind a ``torch.autograd.Function``
                     that returns ``dx`` and the scale's gradient;
* ``warmup_search``  the 99-candidate search of a quantiser's first call (:262-282): the maximum from `yh_qat_observe`, then
                     `yh_tpsq_warmup_search`, which writes the scale and decrements the ``warmup`` buffer;
* ``bias_observe_update`` / ``bias_fake_quant``  ``Bias_Quantizer`` (:166-223) has mode 1's global tracker rule and symmetric
                     power-of-two scale over 128 and mode 1's quantize / round / clamp / dequantize, so it runs on `yh_qat_observe`,
                     `yh_qat_range_update` and `yh_qat_fake_quant_*` unchanged.

Nothing is read back to the host.
"""
import torch

from . import hiplib, qat
from .calib import _dense

_lib_override = None      # tests inject the host emulation of the C ABI here
_force_device = False     # tests: take the device branch for host tensors too (with _lib_override set)


def _lib():
    return _lib_override if _lib_override is not None else hiplib.load()


def eligible(t, scale):
    """Dense fp32 tensors on a GPU with a one-element fp32 scale next to them; everything else (fp16 under autocast, per-channel
    scales, host tensors) takes the torch formulas."""
    return (torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() > 0 and (t.is_cuda or _force_device)
            and scale.numel() == 1 and scale.dtype == torch.float32 and scale.device == t.device)


class _FakeQuant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, bits):
        lib = _lib()
        xd = _dense(x)
        y = torch.empty_like(xd)      # preserve_format: a dense permuted view keeps its strides, so element i of x is element i of y
        snap = torch.empty(2, dtype=torch.float32, device=xd.device)
        with hiplib.on_device(xd):
            hiplib.check(lib.yh_tpsq_fake_quant_fwd(hiplib.ptr(xd), hiplib.ptr(y), xd.numel(), hiplib.ptr(scale), int(bits), hiplib.ptr(snap),
                                                    hiplib.stream_ptr()), 'tpsq fake-quant forward')
        ctx.bits = int(bits)
        ctx.scale_shape = scale.shape
        ctx.save_for_backward(xd, snap)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib()
        x, snap = ctx.saved_tensors
        if dy.dtype != torch.float32 or dy.stride() != x.stride():
            dy = torch.empty_like(x).copy_(dy)
        dx = torch.empty_like(x)
        grad = torch.empty(ctx.scale_shape, dtype=torch.float32, device=x.device)
        with hiplib.on_device(x):
            need = int(lib.yh_tpsq_grad_workspace(x.numel()))
            ws = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=x.device)
            hiplib.check(lib.yh_tpsq_fake_quant_bwd(hiplib.ptr(x), hiplib.ptr(dy), hiplib.ptr(dx), x.numel(), hiplib.ptr(snap), ctx.bits,
                                                    hiplib.ptr(ws), ws.numel() * 4, hiplib.ptr(grad), hiplib.stream_ptr()),
                         'tpsq fake-quant backward')
        return dx, grad, None


def fake_quant(x, scale, bits):
    """Fake-quantised ``x`` on the int``bits`` grid of the power of two nearest to the one-element device parameter ``scale``, which
    is left in ``scale``."""
    return _FakeQuant.apply(x, scale, bits)


@torch.no_grad()
def warmup_search(x, scale, warmup, bits):
    """The first-call search: ``scale`` and ``warmup`` are written in device memory."""
    lib = _lib()
    xd = _dense(x)
    step = qat.observe(xd)[1] / 100      # (:266) a one-element torch op, so the division is the one the torch formulas' device runs
    with hiplib.on_device(xd):
        need = int(lib.yh_tpsq_warmup_workspace(xd.numel()))
        ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=xd.device)
        hiplib.check(lib.yh_tpsq_warmup_search(hiplib.ptr(xd), xd.numel(), hiplib.ptr(step), int(bits), hiplib.ptr(ws), ws.numel() * 8,
                                               hiplib.ptr(scale), hiplib.ptr(warmup), hiplib.stream_ptr()), 'tpsq warm-up search')


@torch.no_grad()
def bias_observe_update(t, quantizer):
    """``range_tracker(input)`` and ``update_params()`` of a ``Bias_Quantizer`` (:137-163, :173-186), buffers in place."""
    tracker = quantizer.range_tracker
    minmax = qat.observe(t)
    with hiplib.on_device(minmax):
        hiplib.check(qat._lib().yh_qat_range_update(hiplib.ptr(minmax), hiplib.ptr(tracker.min_val), hiplib.ptr(tracker.max_val),
                                                    hiplib.ptr(tracker.first_w), hiplib.ptr(quantizer.scale), None, hiplib.QAT_TRACK_GLOBAL,
                                                    0.0, 0, 1, int(quantizer.bits), hiplib.stream_ptr()), 'tpsq bias range update')


def bias_fake_quant(t, quantizer):
    return qat.fake_quant(t, quantizer.scale, None, quantizer.bits, True, True)
