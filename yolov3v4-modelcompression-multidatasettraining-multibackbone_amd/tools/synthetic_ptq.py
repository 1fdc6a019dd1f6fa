"""A COS-PTQ graph with a SYNTHETIC calibrated state, for timing and large-graph parity of the int8 eval path.

Real calibration of YOLOv3-608 / YOLOv4-640 needs images (and the reference cannot calibrate cfgs with max-pools at all,
SURVEY 8c), but the EVAL arithmetic (reference quantized_ptq_cos.py:288-296, 543-567, 717: grid conv + grid bias ->
activation -> round/clamp onto the activation grid; shortcut / concat re-scaling) runs with any scale buffers.  This fills
them deterministically: weight / bias grids from the BN-folded float weights with power-of-two max-abs scales, every
activation, shortcut and concat scale a fixed power of two.  Works on this package's modules and, attribute for attribute,
on the reference's (tests/golden/make_golden_ptq.py uses it to produce reference-side eval goldens).
"""
import math

import torch


def _fold(w, b, g, beta, mean, var, eps):
    """BN folded into the conv, in float64: the grid decisions below (floor(|w| / s + 0.5)) then do not depend on the last fp32
    bit of the fold, which differs between hosts (measured: the fp32 fold gave different grid weights on an EPYC 9575F and on the
    build container - same float state, same scales - and the goldens stopped being reproducible on the GPU box)."""
    w, g, beta, mean, var = (t.detach().double() for t in (w, g, beta, mean, var))
    s = g / torch.sqrt(var + eps)
    shift = beta - mean * s
    return w * s.view(-1, 1, 1, 1), (shift if b is None else shift + b.detach().double() * s)


def _to_grid(t, scale):
    """Round-half-away onto the int8 grid of ``scale`` (reference quantized_ptq_cos.py:14-20), computed in float64, stored as fp32
    (grid values k * 2^e with |k| <= 128 are exact in fp32)."""
    t = t.detach().double()
    return ((torch.sign(t) * torch.floor(t.abs() / scale + 0.5)).clamp(-128, 127) * scale).float()


def pow2_scale(t, levels=127.0):
    """Smallest power of two s with max|t| / s <= levels."""
    return 2.0 ** math.ceil(math.log2(max(float(t), 1e-12) / levels))


def measure_ranges(float_model, x):
    """max|output| of every block of ``float_model`` (eval, float) on the batch ``x``: the data a one-batch max-abs calibration
    would see.  Forward hooks only, so it works on any Darknet implementation with a ``module_list``."""
    peaks = [0.0] * len(float_model.module_list)
    hooks = []
    for i, m in enumerate(float_model.module_list):
        def hook(mod, inp, out, i=i):
            t = out[0] if isinstance(out, (tuple, list)) else out
            if torch.is_tensor(t):
                peaks[i] = float(t.detach().abs().max())
        hooks.append(m.register_forward_hook(hook))
    was_training = float_model.training
    try:
        with torch.no_grad():
            float_model.eval()(x)
    finally:
        for h in hooks:
            h.remove()
        float_model.train(was_training)
    return peaks


def fill_synthetic_state(float_model, q_model, act_scale=2.0 ** -4, sum_scale=2.0 ** -3, ranges=None):
    """Copy ``float_model``'s (seeded) weights onto ``q_model``'s grids; both are Darknet graphs of the same cfg, ``q_model`` built
    with ``quantized=3``.  ``ranges`` (from ``measure_ranges``) puts every activation / shortcut / concat on the power-of-two
    grid that just covers its float range (a live int8 detector); without it every scale is the fixed ``act_scale`` (timing
    only: deep random-weight nets then clamp or die).  Returns ``q_model`` in eval mode."""
    defs = [d for d in getattr(float_model, 'module_defs', []) if d.get('type') != 'net']
    grid = (lambda i: pow2_scale(ranges[i], 127.0)) if ranges is not None else (lambda i: act_scale)
    with torch.no_grad():
        for i, (f, q) in enumerate(zip(float_model.module_list, q_model.module_list)):
            name = q.__class__.__name__
            if isinstance(f, torch.nn.Sequential) and len(f) and isinstance(f[0], torch.nn.Conv2d):
                conv = f[0]
                bn = f[1] if len(f) > 1 and isinstance(f[1], torch.nn.modules.batchnorm.BatchNorm2d) else None
                w, b = (conv.weight.detach().double(), conv.bias.detach().double()) if bn is None else _fold(conv.weight, conv.bias, bn.weight, bn.bias,
                                                                         bn.running_mean, bn.running_var, bn.eps)
                qc = q[0]
                sw, sb = pow2_scale(w.abs().max()), pow2_scale(b.abs().max())
                qc.weight_quantizer.scale.fill_(sw)
                qc.bias_quantizer.scale.fill_(sb)
                qc.activation_quantizer.scale.fill_(grid(i))
                qc.q_weight.copy_(_to_grid(w, sw))
                qc.q_bias.copy_(_to_grid(b, sb))
                qc.quantized = True      # BN already folded, grids in place: eval uses q_weight / q_bias as they are
            elif name.startswith('COSPTQuantizedShortcut'):
                if ranges is None:
                    sx = sa = act_scale
                    ss = sum_scale
                else:   # both operands on the finer of their two grids (what the _min search settles on), the sum on its own
                    frm = [int(k) for k in (defs[i]['from'] if isinstance(defs[i]['from'], (list, tuple)) else [defs[i]['from']])]
                    src = frm[0] if frm[0] >= 0 else i + frm[0]
                    sx = sa = min(grid(i - 1), grid(src))
                    ss = grid(i)
                q.scale_x.fill_(sx)
                q.scale_a.fill_(sa)
                q.scale_sum.fill_(ss)
            elif name == 'COSPTQuantizedFeatureConcat':
                q.scale.fill_(grid(i))
    return q_model.eval()


# ----------------------------------------------------------------------------------------------- QAT (quantized == 1)
QAT_RUNNING_VAR = 0.9999899864196777      # fp32(1 - 1e-5): running_var + eps (1e-5) rounds to exactly 1.0f


def seed_qat_batchnorm_(float_model, x=None, seed=1, peak=8.0):
    """Give every BatchNorm of ``float_model`` the statistics of the synthetic QAT state: ``running_var = fp32(1 - 1e-5)``, so that
    ``running_var + eps == 1.0f`` exactly and the BatchNorm fold is ``W * gamma`` and ``beta - mean * gamma`` - one fp32 product (and
    one difference) per value, with no square root or division that could round differently on another host or device (``_fold``'s
    docstring records that this has happened).  ``gamma`` in [2.2, 2.7]: with the default conv initialisation (weight variance
    1 / (3 fan_in)) and a leaky or Mish activation that keeps a layer's output near its input's magnitude, so activations stay in
    a live range; ``beta`` and ``running_mean`` are small seeded normals.  Residual sums still double the magnitude 23 times in
    YOLOv3, so with a batch ``x`` one forward then settles the depth: every BatchNorm block whose output peak on ``x`` is off
    ``peak`` gets ``gamma`` and ``beta`` scaled by the power of two that brings it nearest (the pre-activation scales with them)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for block in float_model.module_list:
            for bn in (block.children() if isinstance(block, torch.nn.Sequential) else ()):
                if isinstance(bn, torch.nn.modules.batchnorm.BatchNorm2d):
                    assert abs(bn.eps - 1e-5) < 1e-12
                    n = bn.weight.numel()
                    bn.weight.copy_(2.2 + 0.5 * torch.rand(n, generator=g))
                    bn.bias.copy_(0.1 * torch.randn(n, generator=g))
                    bn.running_mean.copy_(0.1 * torch.randn(n, generator=g))
                    bn.running_var.fill_(QAT_RUNNING_VAR)
                    assert bool((bn.running_var + bn.eps == 1.0).all())
    if x is None:
        return float_model

    def settle(block, inp, out):
        bn = next(m for m in block.children() if isinstance(m, torch.nn.modules.batchnorm.BatchNorm2d))
        k = 2.0 ** round(math.log2(peak / max(float(out.detach().abs().max()), 1e-12)))
        if k == 1.0:
            return None
        with torch.no_grad():
            bn.weight.mul_(k)
            bn.bias.mul_(k)
        return block.forward(inp[0])

    hooks = [b.register_forward_hook(settle) for b in float_model.module_list if isinstance(b, torch.nn.Sequential)
             and any(isinstance(m, torch.nn.modules.batchnorm.BatchNorm2d) for m in b.children())]
    was_training = float_model.training
    try:
        with torch.no_grad():
            float_model.eval()(x)
    finally:
        for h in hooks:
            h.remove()
        float_model.train(was_training)
    return float_model


def fill_synthetic_qat_state(float_model, q_model, ranges):
    """The ``quantized == 1`` sibling of ``fill_synthetic_state``: copy ``float_model``'s weights and BatchNorm tensors (see
    ``seed_qat_batchnorm_``) into ``q_model`` - the same cfg built with ``quantized=1`` - and derive every scale the way training
    does, through the modules' own range trackers and ``update_params``: the weight and bias quantisers from the folded tensors,
    the activation quantisers, shortcuts and concats from ``ranges`` (``measure_ranges(float_model, x)``).  Scales are the power
    of two NEAREST to range / 128 (quantized_google.py ``_nearest_pow2``), so some tensors clamp, as in a trained model.
    Returns ``q_model`` in eval mode."""
    from utils.quantized.quantized_google import _nearest_pow2, _symmetric_scale
    defs = [d for d in float_model.module_defs if d.get('type') != 'net']
    span = lambda r: torch.tensor([-float(r), float(r)])

    def track(tracker, r):
        tracker(span(max(float(r), 1e-6)))
        return tracker

    with torch.no_grad():
        for i, (f, q) in enumerate(zip(float_model.module_list, q_model.module_list)):
            name = q.__class__.__name__
            if isinstance(f, torch.nn.Sequential) and len(f) and isinstance(f[0], torch.nn.Conv2d):
                conv, qc = f[0], q[0]
                bn = f[1] if len(f) > 1 and isinstance(f[1], torch.nn.modules.batchnorm.BatchNorm2d) else None
                qc.weight.copy_(conv.weight)
                if conv.bias is not None:
                    qc.bias.copy_(conv.bias)
                if bn is not None:
                    qc.gamma.copy_(bn.weight)
                    qc.beta.copy_(bn.bias)
                    qc.running_mean.copy_(bn.running_mean)
                    qc.running_var.copy_(bn.running_var)
                w, b = qc.BN_fuse()
                for quantizer, t in ((qc.weight_quantizer, w), (qc.bias_quantizer, b)):
                    quantizer.range_tracker(t)
                    quantizer.update_params()
                track(qc.activation_quantizer.range_tracker, ranges[i])
                qc.activation_quantizer.update_params()
            elif name in ('QuantizedShortcut_min', 'QuantizedShortcut_max'):
                frm = defs[i]['from'] if isinstance(defs[i]['from'], (list, tuple)) else [defs[i]['from']]
                src = int(frm[0]) if int(frm[0]) >= 0 else i + int(frm[0])
                tx, ta, ts = track(q.range_tracker_x, ranges[i - 1]), track(q.range_tracker_a, ranges[src]), \
                    track(q.range_tracker_sum, ranges[i])
                if name == 'QuantizedShortcut_min':      # the two scale rules of the modules' training branches (_merge)
                    q.input_scale = _symmetric_scale(max(tx.min_val, ta.min_val), min(tx.max_val, ta.max_val), q.bits)
                    q.scale = _symmetric_scale(ts.min_val, ts.max_val, q.bits)
                else:
                    q.scale = _symmetric_scale(min(ts.min_val, tx.min_val, ta.min_val), max(ts.max_val, tx.max_val, ta.max_val), q.bits)
            elif name == 'QuantizedFeatureConcat' and q.multiple:
                for j, l in enumerate(q.layers):
                    q.float_max_list[j] = max(float(ranges[i + l if l < 0 else l]), 1e-6)
                q.scale = _nearest_pow2(max(q.float_max_list).unsqueeze(0)) / float(1 << (q.bits - 1))
    return q_model.eval()
