"""Feature distillation on the engines' own buffers: the attention maps of ``compute_lost_KD4`` (csrc/kd.hip).

The reference's feature term (utils/utils.py:553-563) reads every conv block's output - ``feature_out``, ~70 NCHW fp32 tensors per
model and step - only through ``A = feature.abs().sum(1)``, one fp32 number per pixel.  Both engines keep their activations NHWC
(fp16 or fp32) in buffers of their own, so with ``Darknet.hip_return_features = 'attention'`` they hand out the maps instead:

    AttentionMaps          a ``list`` of (N, H, W) fp32 views of ONE flat buffer (``.flat``, ``.offsets``), written by one
                           ``yh_kd_attention`` launch over a device row table (one row per feature)
    attention_kl(s, t, b)  sum over features of KLDivLoss(sum)(log_softmax(A_s / T), softmax(A_t / T)) * T * T / b as one
                           ``yh_kd_attention_kl`` call (one workgroup per (feature, image) row, fixed-order sums, no atomics);
                           it leaves G = p_s - p_t behind
    inject                 the training engine adds the loss's gradient, (g * T / b) * G * sign(y), to its NHWC gradient buffers
                           with one ``yh_kd_inject`` launch before the first backward range runs (engine/train.py); g, the upstream
                           gradient (GradScaler scale, batch / 64 factor), is read from device memory - no host read on this path

``YOLO_HIP_KD=0`` keeps the torch statement on the maps (A/B runs): autograd then hands the training engine an ordinary gradient of
the flat buffer, which goes through the same inject launch with g = 1.  ``stats()`` counts the launches.
"""
import ctypes as C
import os

import torch

from . import hiplib
from .hiplib import KdRow, KdKlRow, KD_CHUNK

_LIB_OVERRIDE = None   # tests inject the host emulation here
_STATS = dict(attention=0, kl=0, inject=0)
T_DEFAULT = 3.0


def _lib():
    return _LIB_OVERRIDE if _LIB_OVERRIDE is not None else hiplib.load()


def stats():
    """Launch counters since ``reset_stats``: ``attention`` (one per model and step), ``kl`` and ``inject`` (one per step)."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def enabled():
    return os.environ.get('YOLO_HIP_KD', '1') != '0'


class AttentionMaps(list):
    """``[A_0, A_1, ...]``, A_i = sum_c |feature_i| as an (N, H, W) fp32 view of ``flat`` starting at ``offsets[i]``.  ``sink`` is
    the training plan's ``KdSink`` (None for maps of the evaluation engine, which take no gradient)."""

    def __init__(self, flat, shapes, sink=None):
        offsets, off = [], 0
        for n, h, w in shapes:
            offsets.append(off)
            off += n * h * w
        if flat.numel() != off:
            raise ValueError('attention maps: the flat buffer holds %d floats, the shapes need %d' % (flat.numel(), off))
        super().__init__(flat[o:o + n * h * w].view(n, h, w) for o, (n, h, w) in zip(offsets, shapes))
        self.flat, self.offsets, self.shapes, self.sink = flat, offsets, [tuple(s) for s in shapes], sink


class KdSink:
    """What a training plan keeps for the distillation term of the step in flight: G and the row partials (pieces of the step
    arena), the device table of KL rows, and the upstream gradient the KL node leaves for the injection."""

    def __init__(self):
        self.G = self.partials = self.kl_table = None
        self.n_kl_rows = 0
        self.pending = None        # (g: device fp32 scalar, coef: float, G) set by the KL node's backward, taken by the injection
        self.lib = None            # the engine's library handle (the host emulation in the CPU tests)


def feature_rows(feats):
    """Host image of the ``yh_kd_row`` table.  ``feats``: dicts with y, dy (addresses), dtype (YH_F16 / YH_F32), n, h, w, c, ld,
    c_off.  Returns (bytes, n_rows, n_chunks, shapes)."""
    rows, chunk0, off, shapes = [], 0, 0, []
    for f in feats:
        n, hw = int(f['n']), int(f['h']) * int(f['w'])
        if (f['c'] % 8 or f['ld'] % 8 or f['c_off'] % 8 or n < 1 or hw < 1 or f['c'] < 8 or f['c_off'] < 0 or f['c_off'] + f['c'] > f['ld']
                or f['y'] % 16 or (f.get('dy') or 0) % 16):
            raise NotImplementedError('attention maps: a feature of %d channels at pitch %d, offset %d' % (f['c'], f['ld'], f['c_off']))
        if f['dtype'] not in (hiplib.YH_F16, hiplib.YH_F32):
            raise NotImplementedError('attention maps are taken from fp16 / fp32 activations')
        rows.append(KdRow(y=f['y'], dy=f.get('dy'), out_off=off, chunk0=chunk0, dtype=f['dtype'], n=n, hw=hw, c=f['c'], ld=f['ld'],
                          c_off=f['c_off']))
        chunk0 += (n * hw + KD_CHUNK - 1) // KD_CHUNK
        off += n * hw
        shapes.append((n, int(f['h']), int(f['w'])))
    return bytes((KdRow * len(rows))(*rows)), len(rows), chunk0, shapes


def kl_rows(shapes):
    """Host image of the ``yh_kd_kl_row`` table of a map layout: one row per (feature, image)."""
    rows, off = [], 0
    for n, h, w in shapes:
        for _ in range(n):
            rows.append(KdKlRow(off=off, len=h * w))
            off += h * w
    return bytes((KdKlRow * len(rows))(*rows)), len(rows)


def to_device(raw, device):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def run_attention(table, n_rows, n_chunks, out, lib=None):
    """One ``yh_kd_attention`` launch: the maps of every row of the device table into ``out``."""
    with hiplib.on_device(out):
        hiplib.check((lib or _lib()).yh_kd_attention(table.data_ptr(), n_rows, n_chunks, out.data_ptr(), hiplib.stream_ptr()), 'yh_kd_attention')
    _STATS['attention'] += 1


def run_inject(table, n_rows, n_chunks, G, g, coef, lib=None):
    """One ``yh_kd_inject`` launch over the table's gradient buffers."""
    with hiplib.on_device(G):
        hiplib.check((lib or _lib()).yh_kd_inject(table.data_ptr(), n_rows, n_chunks, G.data_ptr(), g.data_ptr(), C.c_float(coef).value,
                                         hiplib.stream_ptr()), 'yh_kd_inject')
    _STATS['inject'] += 1


def _on_device(t):
    return t.is_cuda or _LIB_OVERRIDE is not None


def _sink_lib(maps):
    return getattr(maps.sink, 'lib', None) if maps.sink is not None else None


def fusable(feature_s, feature_t):
    """Both arguments are ``AttentionMaps`` with one layout on one GPU (host tensors under the tests' emulation)."""
    if not (isinstance(feature_s, AttentionMaps) and isinstance(feature_t, AttentionMaps)) or not enabled():
        return False
    fs, ft = feature_s.flat, feature_t.flat
    return ((_on_device(fs) or _sink_lib(feature_s) is not None) and fs.device == ft.device and fs.dtype == ft.dtype == torch.float32 and fs.is_contiguous()
            and ft.is_contiguous() and feature_s.shapes == feature_t.shapes and len(feature_s) > 0)


_KL_TABLES = {}    # (device, layout) -> (device table, rows): maps that come without a sink (two evaluation engines)


class _AttentionKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat_s, flat_t, maps_s, batch_size, T):
        sink = maps_s.sink
        dev = flat_s.device
        if sink is not None and sink.kl_table is not None:
            table, n_rows, G, partials = sink.kl_table, sink.n_kl_rows, sink.G, sink.partials
        else:
            key = (str(dev), tuple(maps_s.shapes))
            if key not in _KL_TABLES:
                raw, n = kl_rows(maps_s.shapes)
                _KL_TABLES.clear()         # one layout at a time: the tables of a finished run do not pile up
                _KL_TABLES[key] = (to_device(raw, dev), n)
            table, n_rows = _KL_TABLES[key]
            G = torch.empty_like(flat_s)
            partials = torch.empty(max(n_rows, 1), device=dev, dtype=torch.float32)
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        with hiplib.on_device(flat_s):
            rc = (_sink_lib(maps_s) or _lib()).yh_kd_attention_kl(flat_s.data_ptr(), flat_t.data_ptr(), G.data_ptr(), table.data_ptr(), n_rows,
                                           partials.data_ptr(), loss.data_ptr(), C.c_float(T).value, int(batch_size), hiplib.stream_ptr())
        hiplib.check(rc, 'yh_kd_attention_kl')
        _STATS['kl'] += 1
        ctx.sink, ctx.G, ctx.coef = sink, G, T / batch_size
        ctx.keep = (flat_s, flat_t, partials)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = g.reshape(1).float().contiguous()
        if ctx.sink is not None:
            # the training engine adds (g * coef) * G * sign(y) to its own gradient buffers before its first backward range: this
            # node runs first, because the maps are an output of the LAST range's autograd node
            if ctx.sink.pending is not None:
                raise RuntimeError('attention_kl: one distillation term per training step')
            ctx.sink.pending = (g, ctx.coef, ctx.G)
            return None, None, None, None, None
        return ctx.G * (g * ctx.coef), None, None, None, None


def attention_kl(feature_s, feature_t, batch_size, T=T_DEFAULT):
    """sum_i KLDivLoss(sum)(log_softmax(A_s[i] / T, 1), softmax(A_t[i] / T, 1)) * T * T / batch_size over the flattened maps, as a
    (1,) tensor; differentiable with respect to the student's maps."""
    return _AttentionKL.apply(feature_s.flat, feature_t.flat.detach(), feature_s, int(batch_size), float(T))
