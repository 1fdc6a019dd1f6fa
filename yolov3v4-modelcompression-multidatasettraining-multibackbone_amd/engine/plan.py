"""Lowering of a ``models.Darknet`` module to a replayable launch plan on ``libyolo_hip.so``.

The reference executes the graph with a per-layer Python loop over ``nn.Module`` s
(models.py:524-545) on NCHW tensors.  Here the same cfg graph is *compiled* once per input shape:

1. **Values.**  Every block output that must exist in memory becomes a ``Value`` (NHWC, dtype fp16 or
   fp32, channel pitch ``ld``).  Blocks that only re-label data produce no value: a single-layer
   ``route`` is an alias, a ``shortcut`` following a conv is folded into that conv's epilogue as a
   residual operand, an ``upsample`` following a conv makes the conv write each pixel to its 2x2
   block, and a ``yolo`` block becomes a decode op writing straight into the concatenated output.
2. **Placement.**  A multi-input ``route`` owns one wide buffer; each input that is not already placed
   elsewhere is *produced directly into its channel slice* (zero-copy concat); consumers read slices
   through the pitch.  Channel counts that are not multiples of 8 are padded per segment and the
   consumer's packed weights get zero columns at the pad positions (``cin_map``), so pruned models
   with arbitrary widths lower the same way.
3. **Weights.**  BN is folded and weights are packed K-major by ``yh_conv_pack_weights`` on the device,
   straight from the live ``nn.Parameter`` storage.  The cache is keyed on every source tensor's
   ``(data_ptr, _version, shape)``; ``Darknet`` also drops the engine on ``load_state_dict`` /
   ``load_darknet_weights`` / ``fuse`` / ``.to()`` / ``train()``.
4. **Replay.**  ``yh_plan_run`` launches the recorded ops from native code; per-call pointers (input
   frames, output tensors) are slots patched at launch.

Nothing here computes activations with torch: torch supplies device memory and the stream.
"""
import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import hiplib
from .hiplib import (ConvDesc, StemDesc, PoolDesc, CopyDesc, AddDesc, DecodeDesc, DwDesc, SeDesc, QCopyDesc, QPoolDesc,
                     QAddDesc, QAddClampedDesc, TtaViewDesc)

SLOT_INPUT, SLOT_IO, SLOT_RAW0 = 0, 1, 2
ALIGN_C = 8  # physical channel granularity of every NHWC buffer (16 bytes of fp16)
TTA_VIEWS = ((1.0, 0), (0.83, 1), (0.67, 0))   # (ratio, flip) of the test-time augmentation passes (reference models.py:484-488)
TTA_PAD = 0.447                                # torch_utils.scale_img's border value


def _round_up(a, b):
    return (a + b - 1) // b * b


def tta_views(h, w):
    """The passes of ``model(x, augment=True)`` for an h x w frame: per view ``(ratio, flip, rh, rw, oh, ow)`` - the resized content
    ``int(h * s), int(w * s)`` inside a ``ceil(h * s / 64) * 64`` frame (``torch_utils.scale_img(..., same_shape=False)``); the
    first view is the frame itself."""
    out = [(1.0, 0, h, w, h, w)]
    for s, flip in TTA_VIEWS[1:]:
        out.append((s, flip, int(h * s), int(w * s), math.ceil(h * s / 64) * 64, math.ceil(w * s / 64) * 64))
    return out


def tta_groups(views):
    """Views of equal padded shape run as ONE forward, stacked along the batch in view order: ``[[view index, ...], ...]``."""
    groups = {}
    for k, v in enumerate(views):
        groups.setdefault(v[4:6], []).append(k)
    return list(groups.values())


class Value:
    """A tensor that exists in device memory during the forward."""

    ALIGN = ALIGN_C  # physical channel granularity; the engine raises it to 16 for int8 tensors

    def __init__(self, kind, C, H, W, block=None, **kw):
        self.kind = kind  # input | conv | pool | copy | add | concat | slice
        self.C, self.H, self.W = C, H, W
        self.block = block
        self.fp32 = False  # head convs store fp32 regardless of the engine precision
        self.segs = [(0, C)]  # (physical start relative to c_off, logical length)
        self.c_phys = _round_up(C, Value.ALIGN)
        self.scale = None  # int8 engines: real value = grid value * scale (power of two)
        self.parent = None  # concat value this one is produced into
        self.storage = None
        self.c_off = 0
        self.ld = None
        self.__dict__.update(kw)

    def channel_map(self):
        m = []
        for start, length in self.segs:
            m.extend(range(start, start + length))
        return m

    def is_dense(self):
        """Logical channel c sits at physical channel c (a concat of unpadded pieces counts)."""
        at = 0
        for start, length in self.segs:
            if start != at:
                return False
            at += length
        return at == self.C


class Head:
    def __init__(self, block, src, module):
        self.block, self.src = block, src
        self.na, self.no, self.nc = module.na, module.no, module.nc
        self.stride = float(module.stride)
        self.scale_x_y = float(getattr(module, 'scale_x_y', 1.0))      # darknet's grid sensitivity; 1.0 unless Darknet(scale_x_y=True)
        self.anchor_vec = module.anchor_vec.detach().float().cpu().numpy()  # anchors / stride, fp32 (models.py:362)


def _activation_of(block):
    """(code, slope) of a conv block's activation child, by class name like the reference's scripts."""
    for child in block.children():
        name = child.__class__.__name__
        if name == 'LeakyReLU':
            return hiplib.ACT_CODES['leaky'], float(child.negative_slope)
        if name == 'ReLU6':
            return hiplib.ACT_CODES['relu6'], 0.0
        if name == 'HardSwish':
            return hiplib.ACT_CODES['h_swish'], 0.0
        if name == 'ReLU':
            return hiplib.ACT_CODES['relu'], 0.0
        if name == 'Mish':
            return hiplib.ACT_CODES['mish'], 0.0
        if name in ('Swish', 'PReLU', 'Sigmoid'):
            raise NotImplementedError('HIP engine: activation %s is not lowered' % name)
    return hiplib.ACT_CODES['linear'], 0.0


_ACT_BY_NAME = {'leaky': 'leaky', 'relu6': 'relu6', 'h_swish': 'h_swish', 'relu': 'relu', 'mish': 'mish', 'linear': 'linear'}


# The int8 engine executes two module families with the same eval arithmetic: the calibrated COS-PTQ graph (quantized == 3,
# utils/quantized/quantized_ptq_cos.py) and the BN-folding QAT graph (quantized == 1, utils/quantized/quantized_google.py).  What
# differs between them sits in the small functions below (duck-typed by class name, like the rest of the lowering); _build_values,
# _place and _pack_qconv are shared.
_COS_CONV = 'BNFold_COSPTQuantizedConv2d_For_FPGA'
_QAT_CONV = 'BNFold_QuantizedConv2d_For_FPGA'
_COS_SHORTCUTS = ('COSPTQuantizedShortcut_min', 'COSPTQuantizedShortcut_max')
_QAT_SHORTCUTS = ('QuantizedShortcut_min', 'QuantizedShortcut_max')
_QUANT_CONCATS = ('COSPTQuantizedFeatureConcat', 'QuantizedFeatureConcat')


def _quant_conv_info(conv):
    """(act code, slope, s_w, s_a) of a calibrated BNFold_COSPTQuantizedConv2d_For_FPGA or of a BNFold_QuantizedConv2d_For_FPGA."""
    if conv.__class__.__name__ == _COS_CONV and not getattr(conv, 'quantized', False):
        raise RuntimeError('HIP int8 engine: quantised conv has not been calibrated (run the PTQ calibration first)')
    name = _ACT_BY_NAME.get(conv.activate)
    if name is None:
        raise NotImplementedError('HIP int8 engine: activation %r' % conv.activate)
    slope = 0.25 if getattr(conv, 'maxabsscaler', False) else 0.1
    return hiplib.ACT_CODES[name], slope, float(conv.weight_quantizer.scale), float(conv.activation_quantizer.scale)


def _quant_conv_grid(conv):
    """(weight, bias) of a quantised conv on their grids, in real units, fp32 on the module's device.  The COS-PTQ conv stores them
    (``q_weight`` / ``q_bias``).  The QAT conv folds BatchNorm with the running statistics and quantises on every forward
    (quantized_google.py forward, eval branch); the same is done here with the module's own pure methods - NOT the quantisers'
    ``forward``, which advances ``step`` and re-calibrates in training mode - so these are the eager path's weights by construction."""
    if hasattr(conv, 'q_weight'):
        return conv.q_weight.detach().float().contiguous(), conv.q_bias.detach().float().contiguous()
    with torch.no_grad():
        w, b = conv.BN_fuse()
        grid = lambda q, t: q.dequantize(q.clamp(q.round(q.quantize(t))))
        w = grid(conv.weight_quantizer, w)
        b = torch.zeros(conv.out_channels, device=w.device) if b is None else grid(conv.bias_quantizer, b)
    return w.detach().float().contiguous(), b.detach().float().contiguous()


def _quant_shortcut_info(module):
    """(scale_x, scale_a, scale_sum, operands clamped?) of a quantised shortcut.  COS-PTQ: three buffers, operands re-quantised
    without clamp.  QAT ``_min``: both operands go to ``input_scale`` without clamp, the sum to ``scale``.  QAT ``_max``: one ``scale``
    for all three, and every fake-quant of the module clamps - the operands too."""
    name = module.__class__.__name__
    if name in _COS_SHORTCUTS:
        return float(module.scale_x), float(module.scale_a), float(module.scale_sum), False
    if name == 'QuantizedShortcut_min':
        return float(module.input_scale), float(module.input_scale), float(module.scale), False
    if name == 'QuantizedShortcut_max':
        return float(module.scale), float(module.scale), float(module.scale), True
    raise NotImplementedError('HIP int8 engine: %s is not a quantised shortcut' % name)


def _quant_concat_scale(module):
    """The one scale every input of a quantised concat is re-quantised to (both families keep it in ``scale``)."""
    return float(module.scale)


def _quant_sources(block):
    """The tensors a quantised block's packed weights and plan constants were computed from (``_current_signature``), or None for a
    block of no quantised family.  The current objects are read on every call: ``update_params`` REBINDS the scale buffers."""
    if isinstance(block, nn.Sequential) and len(block) and hasattr(block[0], 'q_weight'):
        c = block[0]
        return [c.q_weight, c.q_bias, c.weight_quantizer.scale, c.activation_quantizer.scale]
    if isinstance(block, nn.Sequential) and len(block) and block[0].__class__.__name__ == _QAT_CONV:
        c = block[0]
        return [t for t in (c.weight, c.bias, c.gamma, c.beta, c.running_mean, c.running_var) if t is not None] + \
            [c.weight_quantizer.scale, c.bias_quantizer.scale, c.activation_quantizer.scale]
    if hasattr(block, 'scale_sum'):
        return [block.scale_x, block.scale_a, block.scale_sum]
    if hasattr(block, 'float_max_list'):
        return [block.scale]
    name = block.__class__.__name__
    if name == 'QuantizedShortcut_min':
        return [block.input_scale, block.scale]
    if name == 'QuantizedShortcut_max':
        return [block.scale]
    return None


def _is_pow2(s):
    return math.isfinite(s) and s > 0 and math.frexp(s)[0] == 0.5


def qat_int8_reason(model):
    """Why the ``quantized == 1`` graph ``model`` cannot run on the int8 engine: ``(block index, text)``, or None when it can.

    The ONE place that decides it: ``models.Darknet`` asks before it builds an engine (a graph that does not qualify stays on the
    eager modules), and ``DarknetEngine(precision='int8')`` raises ``NotImplementedError`` with the block index.  The engine's eval
    arithmetic is 8-bit signed symmetric with one power-of-two scale per tensor, so a graph qualifies when every conv has
    ``a_bits == w_bits == 8``, symmetric per-tensor quantisers with zero ``zero_point`` and finite, positive power-of-two scales
    (a fresh model has ``scale == 0``), no depthwise or squeeze-excite block, and unweighted single-source shortcuts over equal
    widths.  All buffers are read with one host transfer."""
    defs, mods = model.module_defs, model.module_list
    scales, zeros, widths = [], [], []      # (block, tensor) pairs checked after the one read

    def quantizer(i, q, what):
        if getattr(q, 'asymmetric', False) or not q.sign:
            return i, '%s quantiser is asymmetric' % what
        if q.bits != 8:
            return i, '%s quantiser has %d bits' % (what, q.bits)
        if not q._per_tensor() or q.zero_point.numel() != 1:
            return i, '%s quantiser is per channel' % what
        scales.append((i, q.scale))
        zeros.append((i, q.zero_point))
        return None

    for i, (mdef, m) in enumerate(zip(defs, mods)):
        kind, name = mdef['type'], m.__class__.__name__
        prev = widths[-1] if widths else 3
        if kind == 'convolutional':
            c = m[0] if isinstance(m, nn.Sequential) and len(m) else None
            if c.__class__.__name__ != _QAT_CONV:
                return i, 'not a BNFold_QuantizedConv2d_For_FPGA'
            if c.groups != 1:
                return i, 'grouped convolution'
            if c.a_bits != 8 or c.w_bits != 8:
                return i, 'a_bits %d, w_bits %d' % (c.a_bits, c.w_bits)
            if c.activate not in _ACT_BY_NAME:
                return i, 'activation %r' % c.activate
            for q, what in ((c.weight_quantizer, 'weight'), (c.bias_quantizer, 'bias'), (c.activation_quantizer, 'activation')):
                bad = quantizer(i, q, what)
                if bad:
                    return bad
            widths.append(c.out_channels)
        elif kind in ('depthwise', 'se'):
            return i, '%s block' % kind
        elif kind == 'shortcut':
            if name not in _QAT_SHORTCUTS:
                return i, 'shortcut module %s' % name
            if m.weight or len(m.layers) != 1:
                return i, 'weighted or multi-source shortcut'
            if m.bits != 8:
                return i, 'shortcut has %d bits' % m.bits
            j = i + m.layers[0] if m.layers[0] < 0 else m.layers[0]
            if not 0 <= j < i or widths[j] != prev:
                return i, 'shortcut over different widths'
            scales.extend((i, t) for t in _quant_sources(m))
            widths.append(prev)
        elif kind == 'route':
            if name != 'QuantizedFeatureConcat':
                return i, 'route module %s' % name
            src = [widths[i + l if l < 0 else l] for l in m.layers]
            if m.multiple:
                if m.bits != 8:
                    return i, 'concat has %d bits' % m.bits
                scales.append((i, m.scale))
                widths.append(sum(src))
            else:
                widths.append(prev // 2 if m.groups else src[0])
        elif kind in ('maxpool', 'upsample', 'yolo', 'reorg3d'):
            widths.append(prev)
        else:
            return i, 'block type %r' % kind
    if not scales:
        return 0, 'no quantised block'
    flat = torch.cat([t.detach().reshape(-1)[:1].float() for _, t in scales + zeros]).tolist()
    for (i, _), s in zip(scales, flat):
        if not _is_pow2(s):
            return i, 'scale %r is not a finite positive power of two (not calibrated?)' % s
    for (i, _), z in zip(zeros, flat[len(scales):]):
        if z != 0:
            return i, 'zero_point %r' % z
    return None


def _conv_parts(block):
    kids = list(block.children())
    conv = kids[0]
    if not isinstance(conv, nn.Conv2d):
        raise NotImplementedError('HIP engine: block starts with %s, not nn.Conv2d' % conv.__class__.__name__)
    bn = None
    for k in kids[1:]:
        if isinstance(k, nn.modules.batchnorm.BatchNorm2d):
            bn = k
    return conv, bn


class DarknetEngine:
    def __init__(self, model, precision='fp16', lib=None):
        if precision not in ('fp16', 'fp32', 'int8'):
            raise ValueError("precision must be 'fp16', 'fp32' or 'int8'")
        # ``lib`` is only ever passed by the CPU test tier (tests/fakelib.py emulates the C ABI on host
        # memory to validate this lowering); the product path always loads the real library or raises.
        self.lib = hiplib.load() if lib is None else lib
        self.model = model
        self.precision = precision
        self.code = {'fp16': hiplib.YH_F16, 'fp32': hiplib.YH_F32, 'int8': hiplib.YH_I8}[precision]
        self.dtype = {'fp16': torch.float16, 'fp32': torch.float32, 'int8': torch.int8}[precision]
        self.kstep = {'fp16': 32, 'fp32': 16, 'int8': 64}[precision]
        self.align = 16 if precision == 'int8' else ALIGN_C
        # int8: the eval graph of a quantised module family - the reference's COSPTQuantized* classes (quantized == 3) or the QAT
        # classes of quantized_google.py (quantized == 1), which must qualify (qat_int8_reason, checked whenever a plan is built)
        self.q = precision == 'int8'
        self.qat = self.q and getattr(model, 'quantized', None) == 1
        self.want_raw = True
        self.return_features = False
        self.force_tile = int(os.environ.get('YOLO_HIP_TILE', '0'))  # A/B profiling knob; 0 = library heuristic
        # batches up to this size replay through a captured hipGraph (one launch instead of ~100).  Off by default:
        # with the native plan executor the frame-at-a-time forward is GPU-bound (1.63 ms at batch 1, YOLOv3-608),
        # and the graph's staged input / cloned outputs make it ~8 % slower (profiles/r01_latency_*.txt).
        self.graph_max_batch = int(os.environ.get('YOLO_HIP_GRAPH_BATCH', '0'))
        self.max_plans = max(1, int(os.environ.get('YOLO_HIP_MAX_PLANS', '6')))   # input shapes kept resident
        self._plans = {}
        self._plans_with_features = False
        self._packed = {}  # block index -> dict(w=, b=, ...)
        self._signature = None
        self.device = None

    # ------------------------------------------------------------------------------------ graph
    def _build_values(self, N, Cin, H, W):
        model = self.model
        defs, mods, routs = model.module_defs, model.module_list, model.routs
        L = len(mods)
        if self.qat:
            reason = qat_int8_reason(model)
            if reason is not None:
                raise NotImplementedError('HIP int8 engine: QAT graph does not qualify, block %d: %s' % reason)
        Value.ALIGN = self.align
        x0 = Value('input', Cin, H, W)
        values, heads = [x0], []
        outs = [None] * L
        cur = x0
        skip = set()

        def ref(i, l):
            j = i + l if l < 0 else l
            v = outs[j]
            if v is None:
                raise NotImplementedError('HIP engine: block %d reads block %d, which has no tensor' % (i, j))
            return v

        for i, (mdef, module) in enumerate(zip(defs, mods)):
            kind = mdef['type']
            cname = module.__class__.__name__
            if i in skip:
                outs[i] = cur
                continue
            hidden = False  # True when this block's own output is fused away into its follower
            if kind in ('convolutional', 'depthwise'):
                conv, bn = _conv_parts(module)
                k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
                if conv.groups != 1:
                    if not (conv.groups == conv.in_channels == conv.out_channels == cur.C) or cur.kind == 'input':
                        raise NotImplementedError('HIP engine: grouped conv with groups != channels (block %d)' % i)
                    Ho, Wo = (cur.H + 2 * p - k) // s + 1, (cur.W + 2 * p - k) // s + 1
                    act, slope = _activation_of(module)
                    v = Value('dw', cur.C, Ho, Wo, block=i, src=cur, conv=conv, bn=bn, k=k, stride=s, pad=p, act=act,
                              slope=slope)
                    v.segs, v.c_phys = list(cur.segs), cur.c_phys
                    values.append(v)
                    cur = v
                    outs[i] = cur
                    continue
                if conv.kernel_size[0] != conv.kernel_size[1] or conv.in_channels != cur.C:
                    raise NotImplementedError('HIP engine: unsupported conv geometry at block %d' % i)
                Ho, Wo = (cur.H + 2 * p - k) // s + 1, (cur.W + 2 * p - k) // s + 1
                if self.q:
                    if conv.__class__.__name__ not in (_COS_CONV, _QAT_CONV):
                        raise NotImplementedError('HIP int8 engine: block %d is not a COS-PTQ or QAT quantised conv' % i)
                    act, slope, s_w, s_a = _quant_conv_info(conv)
                else:
                    act, slope = _activation_of(module)
                v = Value('conv', conv.out_channels, Ho, Wo, block=i, src=cur, conv=conv, bn=bn, k=k, stride=s, pad=p,
                          act=act, slope=slope, res=None, ups=1)
                if self.q:
                    v.s_w, v.scale = s_w, s_a
                nxt = defs[i + 1]['type'] if i + 1 < L else None
                keep = self.return_features   # feature_out needs every conv block's own output: no epilogue fusion
                if nxt == 'shortcut' and not routs[i] and not keep and self._fusable_shortcut(i + 1, v, outs):
                    v.res = ref(i + 1, mods[i + 1].layers[0])
                    skip.add(i + 1)
                    hidden = True
                    if self.q:   # quantised shortcut in the conv epilogue: the value leaves on the SUM grid
                        v.qadd = _quant_shortcut_info(mods[i + 1])[:3]
                        v.act_scale, v.scale = v.scale, v.qadd[2]
                elif nxt == 'upsample' and not routs[i] and not keep and int(defs[i + 1]['stride']) == 2:
                    v.ups = 2
                    v.H, v.W = 2 * Ho, 2 * Wo
                    v.Ho, v.Wo = Ho, Wo
                    skip.add(i + 1)
                    hidden = True
                elif nxt == 'yolo':
                    v.fp32 = True
                if v.ups == 1:
                    v.Ho, v.Wo = Ho, Wo
                values.append(v)
                cur = v
            elif kind == 'maxpool':
                k, s = int(mdef['size']), int(mdef['stride'])
                if k == 2 and s == 1:
                    Ho, Wo, pad_lo, edge_zero = cur.H, cur.W, 0, 1
                else:
                    pad_lo, edge_zero = (k - 1) // 2, 0
                    Ho, Wo = (cur.H + 2 * pad_lo - k) // s + 1, (cur.W + 2 * pad_lo - k) // s + 1
                v = Value('pool', cur.C, Ho, Wo, block=i, src=cur, k=k, stride=s, pad_lo=pad_lo, edge_zero=edge_zero)
                v.segs, v.c_phys, v.scale = list(cur.segs), cur.c_phys, cur.scale
                values.append(v)
                cur = v
            elif kind == 'se':
                se = module[0] if isinstance(module, nn.Sequential) else module
                fc1, fc2 = se.fc[0], se.fc[2]
                if fc1.in_features != cur.C or fc2.out_features != cur.C or fc1.bias is not None or fc2.bias is not None:
                    raise NotImplementedError('HIP engine: unsupported SE geometry at block %d' % i)
                v = Value('se', cur.C, cur.H, cur.W, block=i, src=cur, fc1=fc1, fc2=fc2)
                v.segs, v.c_phys = list(cur.segs), cur.c_phys
                values.append(v)
                cur = v
            elif kind == 'upsample':
                s = int(mdef['stride'])
                if s != 2:
                    raise NotImplementedError('HIP engine: upsample stride %d' % s)
                v = Value('copy', cur.C, cur.H * 2, cur.W * 2, block=i, src=cur, ups=2)
                v.segs, v.c_phys, v.scale = list(cur.segs), cur.c_phys, cur.scale
                values.append(v)
                cur = v
            elif kind == 'route':
                layers = module.layers
                if len(layers) > 1:
                    srcs = [ref(i, l) for l in layers]
                    if any((s.H, s.W) != (srcs[0].H, srcs[0].W) for s in srcs):
                        raise ValueError('route %d joins tensors of different spatial size' % i)
                    v = Value('concat', sum(s.C for s in srcs), srcs[0].H, srcs[0].W, block=i, srcs=srcs)
                    # physical layout is fixed here (later pool/copy/add values inherit it): every source
                    # keeps its own padded span, logical channels map through the per-source segments
                    v.segs, v.offsets, off = [], [], 0
                    for s in srcs:
                        v.offsets.append(off)
                        v.segs.extend((off + st, ln) for st, ln in s.segs)
                        off += s.c_phys
                    v.c_phys = off
                    if self.q:  # (COSPT)QuantizedFeatureConcat: every input is re-quantised to one shared scale
                        if cname not in _QUANT_CONCATS:
                            raise NotImplementedError('HIP int8 engine: route %d is a %s' % (i, cname))
                        v.scale = _quant_concat_scale(module)
                        if not v.scale > 0:
                            raise RuntimeError('HIP int8 engine: route %d has no calibrated scale' % i)
                    values.append(v)
                    cur = v
                    if self.q:
                        # ... and the reference re-quantises the CACHED outputs in place (quantized_ptq_cos.py:1531-1545:
                        # `outputs[layer] = quantize(outputs[layer])`), so whatever reads block `layer` through `outputs` after
                        # this route - a later route or shortcut - sees it on THIS concat's grid (yolov4-tiny: block 23 feeds
                        # the routes 24 and 34).  Later references resolve to the re-quantised slice of the concat buffer.
                        for l, s_, off_ in zip(layers, srcs, v.offsets):
                            if s_.scale != v.scale:
                                j = i + l if l < 0 else l
                                sl = Value('slice', s_.C, s_.H, s_.W, block=j, src=v, first=off_)
                                sl.segs, sl.c_phys, sl.scale = list(s_.segs), s_.c_phys, v.scale
                                values.append(sl)
                                outs[j] = sl
                elif getattr(module, 'groups', False):
                    half = cur.C // 2
                    if not cur.is_dense() or half % self.align or (cur.C - half) % self.align:
                        raise NotImplementedError('HIP engine: unaligned group split at block %d' % i)
                    v = Value('slice', cur.C - half, cur.H, cur.W, block=i, src=cur, first=half)
                    v.scale = cur.scale
                    values.append(v)
                    cur = v
                else:
                    cur = ref(i, layers[0])
            elif kind == 'shortcut' and self.q:
                if cname not in _COS_SHORTCUTS + _QAT_SHORTCUTS or getattr(module, 'weight', False) or len(module.layers) != 1:
                    raise NotImplementedError('HIP int8 engine: shortcut form at block %d' % i)
                other = ref(i, module.layers[0])
                if other.C != cur.C or not cur.is_dense() or not other.is_dense():
                    raise NotImplementedError('HIP int8 engine: channel-mismatched shortcut (block %d)' % i)
                if cur.scale is None or other.scale is None:
                    raise NotImplementedError('HIP int8 engine: shortcut %d reads a tensor that is not on an int8 grid' % i)
                sx, sa, ssum, clamp_ops = _quant_shortcut_info(module)
                v = Value('qadd', cur.C, cur.H, cur.W, block=i, a=cur, b=other, scale_x=sx, scale_a=sa, clamp_ops=clamp_ops)
                v.scale = ssum
                values.append(v)
                cur = v
            elif kind == 'shortcut':
                if getattr(module, 'weight', False):
                    raise NotImplementedError('HIP engine: weighted shortcut (block %d)' % i)
                for l in module.layers:
                    other = ref(i, l)
                    if (other.H, other.W) != (cur.H, cur.W) or cur.fp32 or other.fp32:
                        raise NotImplementedError('HIP engine: shortcut over mismatched maps (block %d)' % i)
                    v = Value('add', cur.C, cur.H, cur.W, block=i, a=cur, b=other)
                    if other.C != cur.C or not cur.is_dense() or not other.is_dense():
                        # operands of different width sum over the leading min(Ca, Cb) channels (layers.py:65-70);
                        # concats of padded pieces are gathered through their channel maps
                        ma, mb = cur.channel_map(), other.channel_map()
                        v.amap = ma + [-1] * (v.c_phys - len(ma))
                        v.bmap = [mb[k] if k < len(mb) else -1 for k in range(cur.C)] + [-1] * (v.c_phys - cur.C)
                    values.append(v)
                    cur = v
            elif kind == 'yolo':
                if not getattr(cur, 'fp32', False):
                    raise NotImplementedError('HIP engine: yolo block %d is not fed by a conv block' % i)
                heads.append(Head(i, cur, module))
            elif kind == 'reorg3d':
                pass
            else:
                raise NotImplementedError('HIP engine: block type %r (block %d) is not lowered' % (kind, i))
            outs[i] = None if hidden else cur
        if not heads:
            raise ValueError('cfg has no yolo block')
        return values, heads, outs

    def _fusable_shortcut(self, j, conv_value, outs):
        module = self.model.module_list[j]
        names = _COS_SHORTCUTS + _QAT_SHORTCUTS if self.q else ('Shortcut',)
        if module.__class__.__name__ not in names or getattr(module, 'weight', False) or len(module.layers) != 1:
            return False
        l = module.layers[0]
        other = outs[j + l if l < 0 else l]
        ok = (other is not None and other.C == conv_value.C and (other.H, other.W) == (conv_value.H, conv_value.W)
              and other.is_dense())
        if ok and self.q:
            # the int8 epilogue carries the shortcut for the compile-time activations only; the routed tensor must be on a grid
            ok = (conv_value.act in (hiplib.ACT_CODES['linear'], hiplib.ACT_CODES['leaky'], hiplib.ACT_CODES['mish'])
                  and other.scale is not None and conv_value.C % 16 == 0 and os.environ.get('YOLO_HIP_FUSE_QADD', '1') != '0')
        if ok and self.q:
            # the epilogue has no operand clamp.  A shortcut whose operands are clamped (QAT QuantizedShortcut_max) may ride in it only
            # when rx <= 1 and ra <= 1: an int8 operand times such a ratio stays inside [-128, 127], so the clamp cannot act.
            # Otherwise the shortcut stays a separate yh_qadd_clamped op.
            sx, sa, _, clamp_ops = _quant_shortcut_info(module)
            ok = not clamp_ops or (conv_value.scale <= sx and other.scale <= sa)
        return ok

    def _place(self, values):
        """Decide which values are produced directly into a concat buffer's channel slice."""
        for v in values:
            if v.kind != 'concat':
                continue
            seen = set()
            v.parts = []
            for s, off in zip(v.srcs, v.offsets):
                if s.kind == 'input':
                    raise NotImplementedError('HIP engine: route over the network input')
                inplace = (s.kind in ('conv', 'pool', 'copy', 'add', 'dw', 'se', 'qadd') and s.parent is None
                           and id(s) not in seen and not s.fp32 and s.storage is None
                           and (not self.q or s.scale == v.scale))  # int8: zero-copy only when no re-quantisation is due
                if inplace:
                    s.parent, s.parent_off = v, off
                seen.add(id(s))
                v.parts.append((s, off, inplace))

    # ---------------------------------------------------------------------------------- weights
    def _source_tensors(self):
        out = []
        for block in self.model.module_list:
            quant = _quant_sources(block) if self.q else None
            if quant is not None:
                out.extend(quant)
            elif isinstance(block, nn.Sequential) and len(block) and isinstance(block[0], nn.Conv2d):
                conv, bn = _conv_parts(block)
                out.extend(t for t in (conv.weight, conv.bias) if t is not None)
                if bn is not None:
                    out.extend((bn.weight, bn.bias, bn.running_mean, bn.running_var))
            elif isinstance(block, nn.Sequential) and len(block) and block[0].__class__.__name__ == 'SE':
                out.extend((block[0].fc[0].weight, block[0].fc[2].weight))
        return out

    def _current_signature(self):
        return tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in self._source_tensors())

    def _pack_conv(self, v):
        """(Re)build the packed weight image of conv value ``v``; buffers are reused when shapes allow."""
        conv, bn = v.conv, v.bn
        dev = conv.weight.device
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        if self.q:
            return self._pack_qconv(v)
        w = f32(conv.weight)
        cb = f32(conv.bias)
        g, be, mu, var = (f32(bn.weight), f32(bn.bias), f32(bn.running_mean), f32(bn.running_var)) if bn is not None \
            else (None, None, None, None)
        eps = float(bn.eps) if bn is not None else 0.0
        keep = [w, cb, g, be, mu, var]
        P = hiplib.ptr
        slot = self._packed.get(v.block)
        if v.src.kind == 'input':
            cout_pad = _round_up(v.C, 32) if v.C % 32 == 0 else _round_up(v.C, 16)
            taps = v.k * v.k
            if slot is None or slot['w'].numel() != taps * v.src.C * cout_pad:
                slot = dict(w=torch.empty(taps * v.src.C * cout_pad, device=dev, dtype=torch.float32),
                            b=torch.empty(cout_pad, device=dev, dtype=torch.float32), cout_pad=cout_pad)
            rc = self.lib.yh_stem_pack_weights(P(w), P(cb), P(g), P(be), P(mu), P(var), eps, v.C, v.src.C, v.k, v.k,
                                               cout_pad, P(slot['w']), P(slot['b']), hiplib.stream_ptr())
            hiplib.check(rc, 'yh_stem_pack_weights')
        else:
            cin_k = _round_up(v.src.c_phys, self.kstep)
            m_pad = _round_up(_round_up(v.C, ALIGN_C), 128)
            taps = v.k * v.k
            cmap = None
            if not v.src.is_dense():
                cmap = torch.tensor(v.src.channel_map(), dtype=torch.int32, device=dev)
                keep.append(cmap)
            if slot is None or slot['w'].numel() != m_pad * taps * cin_k or slot['w'].dtype != self.dtype:
                slot = dict(w=torch.empty(m_pad * taps * cin_k, device=dev, dtype=self.dtype),
                            b=torch.empty(m_pad, device=dev, dtype=torch.float32), cin_k=cin_k, m_pad=m_pad)
            rc = self.lib.yh_conv_pack_weights(self.code, P(w), P(cb), P(g), P(be), P(mu), P(var), eps, P(cmap), v.C,
                                               conv.in_channels, v.k, v.k, cin_k, m_pad, P(slot['w']), P(slot['b']),
                                               hiplib.stream_ptr())
            hiplib.check(rc, 'yh_conv_pack_weights')
        slot['keep'] = keep  # fp32 staging copies must outlive the async pack kernels
        self._packed[v.block] = slot
        return slot

    def _pack_qconv(self, v):
        """int8 image of a quantised conv: grid weights from the real-unit grid weight / s_w, bias on its grid in real units
        (``_quant_conv_grid``: stored by a COS-PTQ conv, computed here from the live parameters of a QAT conv)."""
        conv = v.conv
        qw, qb = _quant_conv_grid(conv)
        dev = qw.device
        P = hiplib.ptr
        slot = self._packed.get(v.block)
        if v.src.kind == 'input':  # float frames in: the stem kernel multiplies real-valued (de-quantised) weights
            cout_pad = v.C if v.C % 32 == 0 else _round_up(v.C, 16)
            taps = v.k * v.k
            if slot is None or slot['w'].numel() != taps * v.src.C * cout_pad:
                slot = dict(w=torch.empty(taps * v.src.C * cout_pad, device=dev, dtype=torch.float32),
                            b=torch.empty(cout_pad, device=dev, dtype=torch.float32), cout_pad=cout_pad)
            rc = self.lib.yh_stem_pack_weights(P(qw), P(qb), None, None, None, None, 0.0, v.C, v.src.C, v.k, v.k, cout_pad,
                                               P(slot['w']), P(slot['b']), hiplib.stream_ptr())
            hiplib.check(rc, 'yh_stem_pack_weights')
        else:
            cin_k = _round_up(v.src.c_phys, self.kstep)
            m_pad = _round_up(_round_up(v.C, self.align), 128)
            taps = v.k * v.k
            cmap = None
            if not v.src.is_dense():
                cmap = torch.tensor(v.src.channel_map(), dtype=torch.int32, device=dev)
            if slot is None or slot['w'].numel() != m_pad * taps * cin_k or slot['w'].dtype != torch.int8:
                slot = dict(w=torch.empty(m_pad * taps * cin_k, device=dev, dtype=torch.int8),
                            b=torch.zeros(m_pad, device=dev, dtype=torch.float32), cin_k=cin_k, m_pad=m_pad)
            rc = self.lib.yh_qconv_pack_weights(P(qw), v.s_w, P(cmap), v.C, conv.in_channels, v.k, v.k, cin_k, m_pad, P(slot['w']),
                                                hiplib.stream_ptr())
            hiplib.check(rc, 'yh_qconv_pack_weights')
            slot['b'].zero_()
            slot['b'][:v.C].copy_(qb)
            slot['cmap'] = cmap
        slot['keep'] = [qw, qb]
        self._packed[v.block] = slot
        return slot

    def _pack_dw(self, v):
        conv, bn = v.conv, v.bn
        dev = conv.weight.device
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        w, cb = f32(conv.weight), f32(conv.bias)
        g, be, mu, var = (f32(bn.weight), f32(bn.bias), f32(bn.running_mean), f32(bn.running_var)) if bn is not None \
            else (None, None, None, None)
        eps = float(bn.eps) if bn is not None else 0.0
        keep = [w, cb, g, be, mu, var]
        cmap = None
        if not v.src.is_dense():
            cmap = torch.tensor(v.src.channel_map(), dtype=torch.int32, device=dev)
            keep.append(cmap)
        P = hiplib.ptr
        slot = self._packed.get(v.block)
        taps = v.k * v.k
        if slot is None or slot['w'].numel() != taps * v.c_phys or slot['w'].dtype != self.dtype:
            slot = dict(w=torch.empty(taps * v.c_phys, device=dev, dtype=self.dtype),
                        b=torch.empty(v.c_phys, device=dev, dtype=torch.float32))
        rc = self.lib.yh_dw_pack_weights(self.code, P(w), P(cb), P(g), P(be), P(mu), P(var), eps, P(cmap), v.C, v.k, v.c_phys,
                                         P(slot['w']), P(slot['b']), hiplib.stream_ptr())
        hiplib.check(rc, 'yh_dw_pack_weights')
        slot['keep'] = keep
        self._packed[v.block] = slot
        return slot

    def _pack_se(self, v, N):
        dev = v.fc1.weight.device
        slot = self._packed.get(v.block)
        w1 = v.fc1.weight.detach().float().contiguous()
        w2 = v.fc2.weight.detach().float().contiguous()
        if slot is None or slot['w1'].shape != w1.shape:
            slot = dict(w1=torch.empty_like(w1), w2=torch.empty_like(w2), cmap=None)
            if not v.src.is_dense():
                slot['cmap'] = torch.tensor(v.src.channel_map(), dtype=torch.int32, device=dev)
        slot['w1'].copy_(w1)
        slot['w2'].copy_(w2)
        self._packed[v.block] = slot
        return slot

    # ------------------------------------------------------------------------------------- plan
    def _alloc(self, N, H, W, C, fp32=False):
        return torch.empty((N, H, W, C), device=self.device, dtype=torch.float32 if fp32 else self.dtype)

    def _build_plan(self, N, Cin, H, W):
        values, heads, outs = self._build_values(N, Cin, H, W)
        self._place(values)
        lib = self.lib
        handle = lib.yh_plan_create()
        if not handle:
            raise MemoryError('yh_plan_create failed')
        plan = dict(handle=handle, values=values, heads=heads, outs=outs, storages=[], N=N, ops=[])
        P = hiplib.ptr

        def add(desc, what):
            idx = lib.yh_plan_add(handle, hiplib.OP_KIND[type(desc)], C.byref(desc), C.sizeof(desc))
            if idx < 0:
                hiplib.check(idx, 'yh_plan_add(%s)' % what)
            plan['ops'].append((what, desc))
            return idx

        def fixup(op, desc_type, field, slot, byte_off=0):
            hiplib.check(lib.yh_plan_add_fixup(handle, op, getattr(desc_type, field).offset, slot, byte_off), 'fixup')

        def materialize(v):
            """Give ``v`` an address: its own buffer, or a slice of its parent concat buffer."""
            if v.storage is not None:
                return
            if v.parent is not None:
                materialize(v.parent)
                v.storage, v.c_off, v.ld = v.parent.storage, v.parent.c_off + v.parent_off, v.parent.ld
            else:
                v.storage = self._alloc(N, v.H, v.W, v.c_phys, v.fp32)
                v.c_off, v.ld = 0, v.c_phys
                plan['storages'].append(v.storage)

        for v in values:
            if v.kind == 'input':
                continue
            if v.kind == 'slice':
                v.storage, v.c_off, v.ld = v.src.storage, v.src.c_off + v.first, v.src.ld
                continue
            materialize(v)
            y = P(v.storage, v.c_off)
            if v.kind == 'conv':
                pk = self._packed.get(v.block) or self._pack_conv(v)
                if v.src.kind == 'input':
                    d = StemDesc(x=None, w=P(pk['w']), bias=P(pk['b']), y=y, n=N, cin=v.src.C, h=v.src.H, w_in=v.src.W,
                                 ho=v.Ho, wo=v.Wo, cout=v.c_phys, cout_pad=pk['cout_pad'], kh=v.k, kw=v.k,
                                 stride=v.stride, pad=v.pad, ldy=v.ld, act=v.act, slope=v.slope, dtype=self.code,
                                 out_scale=v.scale if self.q else 0.0)
                    if v.res is not None or v.ups != 1 or v.fp32:
                        raise NotImplementedError('HIP engine: fused epilogue on the first conv')
                    if v.c_phys > pk['cout_pad']:
                        raise NotImplementedError('HIP engine: stem channel padding')
                    op = add(d, 'stem%d' % v.block)
                    fixup(op, StemDesc, 'x', SLOT_INPUT)
                else:
                    s = v.src
                    if s.fp32 and self.code == hiplib.YH_F16:
                        raise NotImplementedError('HIP engine: block %d consumes a yolo-head tensor' % v.block)
                    if self.q and s.scale is None:
                        raise NotImplementedError('HIP int8 engine: block %d reads a tensor that is not on an int8 grid (%s output)'
                                                  % (v.block, s.kind))
                    tile = self.force_tile
                    if 10 <= tile < 20 and pk['cin_k'] % (2 * self.kstep):
                        tile -= 10  # the 8-unit K step needs cin_k to be a multiple of it
                    if tile >= 40 and not (v.k == 3 and v.stride == 1 and v.pad == 1 and s.W <= 160):
                        tile = 0    # halo kernels are 3x3 / stride 1 only
                    d = ConvDesc(x=P(s.storage, s.c_off), w=P(pk['w']), bias=P(pk['b']),
                                 res=None if v.res is None else P(v.res.storage, v.res.c_off), y=y,
                                 n=N, h=s.H, w_in=s.W, cin=s.c_phys, ho=v.Ho, wo=v.Wo, cout=v.c_phys,
                                 kh=v.k, kw=v.k, stride=v.stride, pad=v.pad, ldx=s.ld,
                                 ldr=0 if v.res is None else v.res.ld, ldy=v.ld, cin_k=pk['cin_k'], m_pad=pk['m_pad'],
                                 act=v.act, slope=v.slope, ups=v.ups, out_f32=1 if v.fp32 else 0, dtype=self.code, tile=tile,
                                 acc_scale=(v.s_w * s.scale) if self.q else 0.0, out_scale=v.scale if self.q else 0.0)
                    if self.q and v.res is not None:
                        sx, sa, ssum = v.qadd
                        d.out_scale = v.act_scale
                        d.q_rx, d.q_ra, d.q_scale_x, d.q_scale_a, d.q_inv_scale_sum = v.act_scale / sx, v.res.scale / sa, sx, sa, 1.0 / ssum
                    add(d, 'conv%d' % v.block)
            elif v.kind == 'dw':
                pk = self._packed.get(v.block) or self._pack_dw(v)
                s = v.src
                add(DwDesc(x=P(s.storage, s.c_off), w=P(pk['w']), bias=P(pk['b']), y=y, n=N, h=s.H, w_in=s.W, c=s.c_phys,
                           ho=v.H, wo=v.W, k=v.k, stride=v.stride, pad=v.pad, ldx=s.ld, ldy=v.ld, act=v.act, slope=v.slope,
                           dtype=self.code), 'dw%d' % v.block)
            elif v.kind == 'se':
                pk = self._packed.get(v.block) or self._pack_se(v, N)
                s = v.src
                pooled = torch.empty((N, v.c_phys), device=self.device, dtype=torch.float32)
                gate = torch.empty((N, v.c_phys), device=self.device, dtype=torch.float32)
                plan['storages'].extend((pooled, gate))
                add(SeDesc(x=P(s.storage, s.c_off), y=y, w1=P(pk['w1']), w2=P(pk['w2']), pooled=P(pooled), gate=P(gate),
                           ch_map=P(pk['cmap']), n=N, h=s.H, w_in=s.W, c=v.C, c_phys=v.c_phys, cr=pk['w1'].shape[0],
                           ldx=s.ld, ldy=v.ld, dtype=self.code), 'se%d' % v.block)
            elif v.kind == 'pool':
                s = v.src
                cls = QPoolDesc if self.q else PoolDesc
                add(cls(x=P(s.storage, s.c_off), y=y, n=N, h=s.H, w_in=s.W, c=s.c_phys, ho=v.H, wo=v.W, k=v.k,
                        stride=v.stride, pad_lo=v.pad_lo, edge_zero=v.edge_zero, ldx=s.ld, ldy=v.ld,
                        dtype=self.code), 'pool%d' % v.block)
            elif v.kind == 'copy' and self.q:
                s = v.src
                add(QCopyDesc(x=P(s.storage, s.c_off), y=y, n=N, h=s.H, w_in=s.W, c=s.c_phys, ups=v.ups, ldx=s.ld, ldy=v.ld,
                              ratio=1.0), 'ups%d' % v.block)
            elif v.kind == 'qadd':
                cls = QAddClampedDesc if v.clamp_ops else QAddDesc     # operands clamped after re-quantisation: yh_qadd_clamped
                add(cls(x=P(v.a.storage, v.a.c_off), a=P(v.b.storage, v.b.c_off), y=y, pixels=N * v.H * v.W, c=v.c_phys,
                        ldx=v.a.ld, lda=v.b.ld, ldy=v.ld, rx=v.a.scale / v.scale_x, ra=v.b.scale / v.scale_a,
                        scale_x=v.scale_x, scale_a=v.scale_a, inv_scale_sum=1.0 / v.scale), 'qadd%d' % v.block)
            elif v.kind == 'copy':
                s = v.src
                add(CopyDesc(x=P(s.storage, s.c_off), y=y, n=N, h=s.H, w_in=s.W, c=s.c_phys, ups=v.ups, ldx=s.ld,
                             ldy=v.ld, dtype=self.code), 'ups%d' % v.block)
            elif v.kind == 'add':
                maps = [None, None]
                if getattr(v, 'amap', None) is not None:
                    maps = [torch.tensor(m, dtype=torch.int32).to(self.device) for m in (v.amap, v.bmap)]
                    plan['storages'].extend(maps)
                add(AddDesc(a=P(v.a.storage, v.a.c_off), b=P(v.b.storage, v.b.c_off), y=y, pixels=N * v.H * v.W,
                            c=v.c_phys, lda=v.a.ld, ldb=v.b.ld, ldy=v.ld, dtype=self.code,
                            amap=P(maps[0]) if maps[0] is not None else None,
                            bmap=P(maps[1]) if maps[1] is not None else None), 'add%d' % v.block)
            elif v.kind == 'concat':
                for s, off, inplace in v.parts:
                    if inplace:
                        continue  # its producer writes (or already wrote) the slice
                    if s.fp32:
                        raise NotImplementedError('HIP engine: route over a yolo-head tensor')
                    if self.q:
                        add(QCopyDesc(x=P(s.storage, s.c_off), y=P(v.storage, v.c_off + off), n=N, h=s.H, w_in=s.W, c=s.c_phys,
                                      ups=1, ldx=s.ld, ldy=v.ld, ratio=s.scale / v.scale), 'cat%d' % v.block)
                        continue
                    add(CopyDesc(x=P(s.storage, s.c_off), y=P(v.storage, v.c_off + off), n=N, h=s.H, w_in=s.W,
                                 c=s.c_phys, ups=1, ldx=s.ld, ldy=v.ld, dtype=self.code), 'cat%d' % v.block)

        rows = sum(h.na * h.src.H * h.src.W for h in heads)
        no = heads[0].no
        off = 0
        plan['raw_shapes'] = []
        plan['decode_descs'] = []                       # the heads as yh_yolo_decode_candidates takes them (detect())
        plan['first_decode_op'] = len(plan['ops'])      # the decode ops are the last ops of the plan
        for k, h in enumerate(heads):
            if h.no != no:
                raise ValueError('yolo heads disagree on the class count')
            s = h.src
            d = DecodeDesc(p=P(s.storage, s.c_off), io=None, raw=None, n=N, ny=s.H, nx=s.W, na=h.na, no=h.no, ldp=s.ld,
                           rows_total=rows, row_off=off, stride=h.stride)
            for a in range(h.na):
                d.anchor_w[a] = float(h.anchor_vec[a, 0])
                d.anchor_h[a] = float(h.anchor_vec[a, 1])
            if h.scale_x_y != 1.0:      # a scaled head is YH_OP_DECODE_SXY; an unscaled one keeps the op and the entry it always had
                d = hiplib.DecodeSxyDesc(d=d, scale_x_y=h.scale_x_y)
            op = add(d, 'yolo%d' % h.block)
            fixup(op, DecodeDesc, 'io', SLOT_IO)              # yh_decode_desc sits at offset 0 of yh_decode_sxy_desc
            fixup(op, DecodeDesc, 'raw', SLOT_RAW0 + k)      # bound to NULL per call when the caller does not want the copies
            plan['raw_shapes'].append((N, h.na, s.H, s.W, h.no))
            plan['decode_descs'].append(type(d).from_buffer_copy(d))
            off += h.na * s.H * s.W
        plan['rows'], plan['no'] = rows, no
        return plan

    # ---------------------------------------------------------------------------------- execute
    def refresh_weights(self):
        """Re-pack every conv from the live parameters (buffers are reused; plans stay valid)."""
        for plan in self._plans.values():
            for v in plan['values']:
                if v.kind == 'conv':
                    self._pack_conv(v)
                elif v.kind == 'dw':
                    self._pack_dw(v)
                elif v.kind == 'se':
                    self._pack_se(v, plan['N'])
            break
        self._signature = self._current_signature()

    def __call__(self, x):
        x, plan = self._plan_for(x)
        N = x.shape[0]
        lib, handle = self.lib, plan['handle']
        if 0 < N <= self.graph_max_batch and x.is_cuda and hasattr(lib, 'yh_plan_graph_launch'):
            io, raws = self._run_graph(plan, x)
        else:
            io = torch.empty((N, plan['rows'], plan['no']), device=x.device, dtype=torch.float32)
            raws = [torch.empty(shape, device=x.device, dtype=torch.float32) for shape in plan['raw_shapes']] \
                if self.want_raw else []
            lib.yh_plan_bind_slot(handle, SLOT_INPUT, x.data_ptr())
            lib.yh_plan_bind_slot(handle, SLOT_IO, io.data_ptr())
            for k in range(len(plan['raw_shapes'])):
                lib.yh_plan_bind_slot(handle, SLOT_RAW0 + k, raws[k].data_ptr() if raws else hiplib.SLOT_NULL)
            hiplib.check(lib.yh_plan_run(handle, hiplib.stream_ptr()), 'yh_plan_run')
        if self.return_features == 'attention':
            feats = self._attention(plan)
        else:
            feats = self._features(plan) if self.return_features else []
        return io, tuple(raws), feats

    def detect(self, x, conf_thres=0.3, iou_thres=0.6, multi_label=False, classes=None, agnostic=False, augment=False):
        """``non_max_suppression(model(x)[0], ...)`` (reference detect.py:104-109) without the decoded (N, rows, 5 + nc) tensor: the plan
        runs up to the head convolutions, ``yh_yolo_decode_candidates`` decodes only the rows whose objectness passes ``conf_thres``
        straight into the NMS candidate records, the remaining NMS steps are ``engine/nms.py``'s.  Same list of (n_i, 6) tensors,
        bit for bit (tests/test_gpu_nms.py).  Small batches keep the hipGraph replay of ``__call__`` (launch-bound there).

        ``augment``: ``non_max_suppression(model(x, augment=True)[0], ...)`` - test-time augmentation - the same way
        (``_detect_augmented``)."""
        from . import nms as hnms
        if augment:
            return self._detect_augmented(x, conf_thres, iou_thres, multi_label, classes, agnostic)
        x, plan = self._plan_for(x)
        N = x.shape[0]
        lib, handle = self.lib, plan['handle']
        if (0 < N <= self.graph_max_batch and x.is_cuda and hasattr(lib, 'yh_plan_graph_launch')) or self.return_features \
                or os.environ.get('YOLO_HIP_FUSED_DETECT', '1') == '0' or self._scaled_two_pass(plan):
            keep = self.want_raw
            self.want_raw = False
            try:
                io = self(x)[0]
            finally:
                self.want_raw = keep
            return hnms.non_max_suppression(io, conf_thres, iou_thres, multi_label, classes, agnostic)
        lib.yh_plan_bind_slot(handle, SLOT_INPUT, x.data_ptr())
        hiplib.check(lib.yh_plan_run_range(handle, 0, plan['first_decode_op'], hiplib.stream_ptr()), 'yh_plan_run_range')
        return hnms.non_max_suppression_heads(plan['decode_descs'], N, plan['rows'], plan['no'] - 5, x.device, conf_thres, iou_thres,
                                              multi_label, classes, agnostic)

    def _scaled_two_pass(self, plan):
        """``YOLO_HIP_SCALE_XY=0`` (A/B runs): a model with a scale_x_y head decodes (YH_OP_DECODE_SXY) and then filters, instead of the
        fused candidate pass."""
        if os.environ.get('YOLO_HIP_SCALE_XY', '1') != '0':
            return False
        if plan is not None:
            return any(isinstance(d, hiplib.DecodeSxyDesc) for d in plan['decode_descs'])
        return any(getattr(m, 'scale_x_y', 1.0) != 1.0 for m in self.model.module_list if m.__class__.__name__ == 'YOLOLayer')

    # ------------------------------------------------------------------------ test-time augmentation
    def _tta_inputs(self, x):
        """The augmented views of ``x`` as network inputs: ``(x, views, [(members, xg), ...])`` with one ``(g * N, C, H', W')`` batch
        ``xg`` per group of views that share a padded shape (``yh_tta_view`` writes view ``members[j]`` at image offset ``j * N``).
        The frame itself is passed through when it is alone in its group."""
        if x.dim() != 4:
            raise ValueError('expected an (N, C, H, W) batch')
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        N, Cin, H, W = x.shape
        views = tta_views(H, W)
        if min(min(v[2:4]) for v in views) < 1 or N < 1:
            raise ValueError('augmented inference: a %d x %d frame has an empty 0.67x view' % (H, W))
        out = []
        with hiplib.on_device(x):
            for members in tta_groups(views):
                if members == [0]:
                    out.append((members, x))
                    continue
                oh, ow = views[members[0]][4:6]
                xg = torch.empty((len(members) * N, Cin, oh, ow), dtype=torch.float32, device=x.device)
                for j, k in enumerate(members):
                    _, flip, rh, rw = views[k][:4]
                    d = TtaViewDesc(src=hiplib.ptr(x), dst=hiplib.ptr(xg, j * N * Cin * oh * ow), n=N, c=Cin, ih=H, iw=W, oh=oh, ow=ow,
                                    rh=rh, rw=rw, flip=flip, scale_h=float(np.float32(H) / np.float32(rh)),
                                    scale_w=float(np.float32(W) / np.float32(rw)), pad_value=TTA_PAD)
                    hiplib.check(self.lib.yh_tta_view(C.byref(d), hiplib.stream_ptr()), 'yh_tta_view')
                out.append((members, xg))
        return x, views, out

    @staticmethod
    def _tta_transform(view, W):
        """(scale, flip_w) of a view as the de-augmentation entries take them: the ratio in fp32, the ORIGINAL width or -1."""
        return float(np.float32(view[0])), float(W) if view[1] else -1.0

    def forward_augmented(self, x):
        """``model(x, augment=True)[0]`` (reference models.py:477-506) as a tensor: one forward per group of views, the scaled views'
        rows mapped back in place by ``yh_tta_deaugment`` (IEEE division, like the fused path and the reference's CPU arithmetic),
        concatenated in view order.  The two-pass form of ``detect(..., augment=True)``."""
        x, views, inputs = self._tta_inputs(x)
        N, W = x.shape[0], x.shape[3]
        keep = self.want_raw
        self.want_raw = False
        parts = [None] * len(views)
        try:
            for members, xg in inputs:
                io = self(xg)[0]
                rows, no = io.shape[1], io.shape[2]
                for j, k in enumerate(members):
                    if k:
                        scale, flip_w = self._tta_transform(views[k], W)
                        hiplib.check(self.lib.yh_tta_deaugment(hiplib.ptr(io, j * N * rows * no), N, rows, no, 0, rows, scale, flip_w,
                                                               hiplib.stream_ptr()), 'yh_tta_deaugment')
                    parts[k] = io[j * N:(j + 1) * N]
        finally:
            self.want_raw = keep
        return torch.cat(parts, 1)

    def _detect_augmented(self, x, conf_thres, iou_thres, multi_label, classes, agnostic):
        """``detect`` over the three views: every group's plan runs up to its head convolutions, and ONE candidate pass per (view, head)
        decodes, maps back and filters (``yh_yolo_decode_candidates_tta``) with keys that index the reference's ``torch.cat(y, 1)`` -
        neither the three decoded tensors nor their concatenation are written.  The groups' plans are distinct and stay resident
        until the NMS returns: its retry and count-first passes read the heads again."""
        from . import nms as hnms
        if x.dim() != 4:
            raise ValueError('expected an (N, C, H, W) batch')
        groups = tta_groups(tta_views(x.shape[2], x.shape[3]))
        N = x.shape[0]
        graph = x.is_cuda and hasattr(self.lib, 'yh_plan_graph_launch') and any(0 < len(m) * N <= self.graph_max_batch for m in groups)
        if graph or self.return_features or os.environ.get('YOLO_HIP_FUSED_DETECT', '1') == '0' or len(groups) > self.max_plans \
                or self._scaled_two_pass(None):
            return hnms.non_max_suppression(self.forward_augmented(x), conf_thres, iou_thres, multi_label, classes, agnostic)
        x, views, inputs = self._tta_inputs(x)
        W = x.shape[3]
        ran = []
        for members, xg in inputs:
            xg, plan = self._plan_for(xg)
            self.lib.yh_plan_bind_slot(plan['handle'], SLOT_INPUT, xg.data_ptr())
            hiplib.check(self.lib.yh_plan_run_range(plan['handle'], 0, plan['first_decode_op'], hiplib.stream_ptr()), 'yh_plan_run_range')
            ran.append((members, xg, plan))
        rows_of = {k: plan['rows'] for members, _, plan in ran for k in members}
        total = sum(rows_of.values())
        no = ran[0][2]['no']
        if total * (no - 5) > 0x7fffffff:
            raise ValueError('augmented inference: %d rows x %d classes do not fit the 32-bit candidate key' % (total, no - 5))
        entries = [None] * len(views)
        for members, _, plan in ran:
            if plan['no'] != no:
                raise ValueError('the view plans disagree on the class count')
            for j, k in enumerate(members):
                off = sum(rows_of[i] for i in range(k))
                scale, flip_w = self._tta_transform(views[k], W)
                heads = []
                for desc in plan['decode_descs']:
                    copy = type(desc).from_buffer_copy(desc)         # a scaled head stays a yh_decode_sxy_desc
                    d, e = hiplib.decode_base(desc), hiplib.decode_base(copy)
                    e.p = d.p + j * N * d.ny * d.nx * d.ldp * 4      # this view's images inside the stacked batch
                    e.n, e.rows_total, e.row_off = N, total, off + d.row_off
                    heads.append((copy, scale, flip_w))
                entries[k] = heads
        return hnms.non_max_suppression_heads([h for heads in entries for h in heads], N, total, no - 5, x.device, conf_thres, iou_thres,
                                              multi_label, classes, agnostic)

    def _plan_for(self, x):
        """The checks of a call and the plan of this input shape (built on first use)."""
        if x.dim() != 4:
            raise ValueError('expected an (N, C, H, W) batch')
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        if self.device is None:
            self.device = x.device
        elif self.device != x.device:
            raise RuntimeError('engine was built on %s, input is on %s' % (self.device, x.device))
        first = self.model.module_list[0]
        w0 = first[0].weight if isinstance(first, nn.Sequential) and len(first) else None
        if w0 is None or w0.device != x.device:
            raise RuntimeError('model parameters must live on the input device %s' % x.device)

        sig = self._current_signature()
        if self._signature is None:
            self._signature = sig
        elif sig != self._signature:
            old_shapes = [s[2] for s in self._signature]
            # graph widths changed (pruning): start over.  So does a QAT int8 engine: its plans carry the scales as launch constants
            # (acc_scale, out_scale, the re-quantisation ratios), and a re-calibration moves them
            if old_shapes != [s[2] for s in sig] or self.qat:
                self._drop_plans()
                self._packed = {}
                self._signature = sig
            else:
                self._signature = sig
                if self._plans:
                    self.refresh_weights()
        elif self._plans and os.environ.get('YOLO_HIP_SAFE', '0') == '1':
            # edits through `param.data` views (`p.data.mul_(...)`) do not bump `param._version`: with YOLO_HIP_SAFE=1 every
            # eval call re-packs from the live tensors (one pack launch per conv) instead of trusting the signature
            self.refresh_weights()

        N, Cin, H, W = x.shape
        if bool(self.return_features) != self._plans_with_features:   # feature_out plans are built without epilogue fusion
            self._drop_plans()
            self._plans_with_features = bool(self.return_features)
        key = (N, Cin, H, W)
        plan = self._plans.get(key)
        if plan is None:
            # every plan owns the activation buffers of its input shape; rectangular evaluation (test.py rect=True) walks
            # through dozens of shapes, so only the most recently used few are kept
            while len(self._plans) >= self.max_plans:
                old = self._plans.pop(next(iter(self._plans)))
                self.lib.yh_plan_destroy(old['handle'])
            plan = self._plans[key] = self._build_plan(N, Cin, H, W)
        else:
            self._plans[key] = self._plans.pop(key)   # most recently used last
        return x, plan

    def _run_graph(self, plan, x):
        """Small-batch path: static I/O buffers + one hipGraph launch; results are copied out (fresh tensors).

        Stream capture is not allowed on the legacy default stream, so the graph lives on an engine-owned
        side stream that is ordered against the caller's current stream on both sides."""
        lib, handle = self.lib, plan['handle']
        cur = torch.cuda.current_stream()
        gs = self.__dict__.get('_graph_stream')
        if gs is None:
            gs = self._graph_stream = torch.cuda.Stream(device=x.device)
        gs.wait_stream(cur)
        with torch.cuda.stream(gs):
            sp = C.c_void_p(gs.cuda_stream)
            g = plan.get('graph')
            if g is None or g['want_raw'] != self.want_raw:
                dev = x.device
                g = dict(x=torch.empty_like(x),
                         io=torch.empty((x.shape[0], plan['rows'], plan['no']), device=dev, dtype=torch.float32),
                         raws=[torch.empty(sh, device=dev, dtype=torch.float32) for sh in plan['raw_shapes']]
                         if self.want_raw else [], want_raw=self.want_raw)
                lib.yh_plan_bind_slot(handle, SLOT_INPUT, g['x'].data_ptr())
                lib.yh_plan_bind_slot(handle, SLOT_IO, g['io'].data_ptr())
                for k in range(len(plan['raw_shapes'])):
                    lib.yh_plan_bind_slot(handle, SLOT_RAW0 + k, g['raws'][k].data_ptr() if g['raws'] else hiplib.SLOT_NULL)
                g['x'].copy_(x)
                hiplib.check(lib.yh_plan_run(handle, sp), 'yh_plan_run')   # warm (lazy code loads) before capturing
                hiplib.check(lib.yh_plan_graph_capture(handle, sp), 'yh_plan_graph_capture')
                plan['graph'] = g
            g['x'].copy_(x)
            hiplib.check(lib.yh_plan_graph_launch(handle, sp), 'yh_plan_graph_launch')
            io = g['io'].clone()
            raws = [r.clone() for r in g['raws']]
        cur.wait_stream(gs)
        for t in [io] + raws:
            t.record_stream(cur)
        return io, raws

    def _features(self, plan):
        """NCHW fp32 copies of the conv-block outputs the reference appends to ``feature_out``."""
        feats = []
        mods = self.model.module_list
        for i, m in enumerate(mods):
            if m.__class__.__name__ == 'Sequential' and i + 1 < len(mods) and \
                    mods[i + 1].__class__.__name__ != 'YOLOLayer':
                feats.append(self.block_output(plan, i))
        return feats

    def _attention(self, plan):
        """``return_features == 'attention'``: sum_c |y| of the same blocks as an ``AttentionMaps`` (engine/kd.py) - (N, H, W) fp32
        views of one fresh flat buffer, written by ONE launch straight from the plan's NHWC activations.  No NCHW copy is made.
        Pad lanes of a padded tensor hold zeros (zero weight rows, zero bias, every activation maps 0 to 0) and add nothing."""
        from . import kd
        if self.q:
            raise NotImplementedError('attention maps are taken from a float graph (fp16 / fp32 activations)')
        table = plan.get('kd_table')
        if table is None:
            mods, feats = self.model.module_list, []
            for i, m in enumerate(mods):
                if m.__class__.__name__ == 'Sequential' and i + 1 < len(mods) and mods[i + 1].__class__.__name__ != 'YOLOLayer':
                    v = plan['outs'][i]
                    if v is None or v.kind == 'input' or v.storage is None or v.fp32:
                        raise NotImplementedError('HIP engine: block %d has no activation buffer to take an attention map from' % i)
                    feats.append(dict(y=v.storage.data_ptr(), dy=None, dtype=self.code, n=plan['N'], h=v.H, w=v.W, c=v.c_phys, ld=v.ld,
                                      c_off=v.c_off))
            raw, plan['kd_rows'], plan['kd_chunks'], plan['kd_shapes'] = kd.feature_rows(feats)
            table = plan['kd_table'] = kd.to_device(raw, self.device)
        flat = torch.empty(sum(n * h * w for n, h, w in plan['kd_shapes']), device=self.device, dtype=torch.float32)
        kd.run_attention(table, plan['kd_rows'], plan['kd_chunks'], flat, self.lib)
        return kd.AttentionMaps(flat, plan['kd_shapes'])

    def block_output(self, plan, i):
        """Output of cfg block ``i`` as an NCHW fp32 tensor (debug / feature_out); None if fused away."""
        v = plan['outs'][i]
        if v is None or v.kind == 'input' or v.storage is None:
            return None
        t = v.storage[..., v.c_off:v.c_off + v.c_phys]
        idx = torch.tensor(v.channel_map(), device=t.device)
        return t.index_select(3, idx).permute(0, 3, 1, 2).float().contiguous()

    def _drop_plans(self):
        for plan in self._plans.values():
            self.lib.yh_plan_destroy(plan['handle'])
        self._plans = {}

    def __del__(self):
        try:
            self._drop_plans()
        except Exception:
            pass
