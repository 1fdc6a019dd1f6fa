"""Model EMA on the device: ``yh_ema_update`` (csrc/ema.hip) behind ``utils.torch_utils.ModelEMA.update``.

``ModelEMA.update`` walks two state dicts and runs ``v.mul_(d).add_(src[k], alpha=1 - d)`` per floating-point tensor: two launches per
tensor (732 on YOLOv3, most of them on a few hundred bytes) and two passes over the averaged weights.  ``EmaState.update`` does the
same arithmetic, bit for bit, with ONE launch over a device table of rows (include/yolo_hip.h ``yh_ema_row``) that is built once per
``ModelEMA`` and rebuilt only when a tensor on either side moves.

A pair of tensors is a row when both are fp32, contiguous, on the same GPU, of the same element count, and the destination shares
its storage with no other destination; every other floating-point pair keeps the torch statement (a half-precision buffer, a
``ModelEMA(device='cpu')``).  Integer tensors are skipped, as before.  On a GPU a missing library or entry point raises
(engine/hiplib.py): there is no quiet fallback.

The kernel writes through raw pointers, which moves no autograd version counter, and the inference engine keys its packed weights
on ``(data_ptr, _version, shape)`` (engine/plan.py ``_current_signature``): every destination's counter is bumped after the launch,
or the evaluation of epoch 2 would run on epoch 1's packed EMA weights.
"""
import ctypes as C
import os

import torch

from . import hiplib
from .hiplib import EmaRow, EMA_CHUNK

_LIB_OVERRIDE = None   # tests inject the host emulation here
_STATS = dict(launches=0, table_builds=0, torch_tensors=0)


def _lib():
    return _LIB_OVERRIDE if _LIB_OVERRIDE is not None else hiplib.load()


def stats():
    """Counters since ``reset_stats``: kernel launches, table builds, and tensors updated with the torch statement on the device path."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def _on_device(t):
    """Whether the kernel can address ``t``: a GPU tensor (a host tensor under the host emulation of the tests)."""
    return t.is_cuda or _LIB_OVERRIDE is not None


def enabled(state):
    """The device path serves a state dict with at least one floating-point tensor on a GPU; ``YOLO_HIP_EMA=0`` keeps the torch
    loop there too, for A/B runs."""
    if os.environ.get('YOLO_HIP_EMA', '1') == '0':
        return False
    return any(v.dtype.is_floating_point and _on_device(v) for v in state.values())


def _is_row(v, s):
    return (v.dtype == torch.float32 and s.dtype == torch.float32 and _on_device(v) and _on_device(s) and v.device == s.device
            and v.numel() == s.numel() and v.numel() > 0 and v.is_contiguous() and s.is_contiguous()
            and v.layout == torch.strided and s.layout == torch.strided)


class EmaState:
    """The row table of one ``ModelEMA``: built on the first update, reused while no tensor of either state dict moves."""

    def __init__(self):
        self._key = None
        self._table = None       # device bytes of yh_ema_row[n_rows]
        self._n_rows = 0
        self._n_chunks = 0
        self._dests = []         # the destinations of the rows: their version counters move with every launch
        self._torch = []         # names of the floating-point pairs that keep the torch statement

    def _build(self, pairs):
        shared = {}
        for _, v, _ in pairs:
            p = v.untyped_storage().data_ptr()
            shared[p] = shared.get(p, 0) + 1
        device = next((v.device for _, v, s in pairs if _is_row(v, s)), None)
        rows, dests, rest, chunk0 = [], [], [], 0
        for k, v, s in pairs:
            if _is_row(v, s) and v.device == device and shared[v.untyped_storage().data_ptr()] == 1:
                n = v.numel()
                rows.append(EmaRow(ema=v.data_ptr(), src=s.data_ptr(), n=n, chunk0=chunk0))
                dests.append(v)
                chunk0 += (n + EMA_CHUNK - 1) // EMA_CHUNK
            else:
                rest.append(k)
        self._n_rows, self._n_chunks, self._dests, self._torch = len(rows), chunk0, dests, rest
        self._table = None
        if rows:
            raw = bytes((EmaRow * len(rows))(*rows))
            self._table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        _STATS['table_builds'] += 1

    def update(self, dst, src, d):
        """``v.mul_(d).add_(src[k], alpha=1 - d)`` for every floating-point ``v`` of ``dst``; ``d`` is the caller's double."""
        # one flat list, not a tuple per tensor: the key is rebuilt on every update, and hundreds of live containers per update would
        # push Python's cyclic collector over its threshold every time
        key = []
        for k, v in dst.items():
            if v.dtype.is_floating_point:
                s = src[k]
                key += (v.data_ptr(), v.numel(), v.dtype, s.data_ptr(), s.numel(), s.dtype)
        if key != self._key:
            self._build([(k, v, src[k]) for k, v in dst.items() if v.dtype.is_floating_point])
            self._key = key
        if self._n_rows:
            with hiplib.on_device(self._dests[0]):
                rc = _lib().yh_ema_update(self._table.data_ptr(), self._n_rows, self._n_chunks, C.c_float(d).value,
                                          C.c_float(1. - d).value, hiplib.stream_ptr())
            hiplib.check(rc, 'yh_ema_update')
            torch.autograd.graph.increment_version(self._dests)
            _STATS['launches'] += 1
        if self._torch:
            for k in self._torch:
                dst[k].mul_(d).add_(src[k].detach(), alpha=1. - d)
            _STATS['torch_tensors'] += len(self._torch)
