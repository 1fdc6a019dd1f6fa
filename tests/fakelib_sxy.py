"""Host emulation of the ``scale_x_y`` entries - ``yh_yolo_decode_sxy``, ``yh_yolo_decode_candidates_sxy``, ``yh_yolo_loss_head_fwd`` /
``_bwd`` and the plan op ``YH_OP_DECODE_SXY`` - on top of ``fakelib_box.FakeLibBox`` and ``fakelib_tta.FakeLibTta`` — TEST
INFRASTRUCTURE ONLY.

With ``s = scale_x_y`` and ``c = 0.5 * (s - 1)`` formed in fp32 from the fp32 ``s``, as the library forms it:

    decode   xy = ((sigmoid(t) * s - c) + cell) * stride         product, difference and sum rounded separately
    loss     pxy = sigmoid(t) * s - c,   d pxy / dt = s * sig * (1 - sig)

``s == 1`` hands the call to the entry it extends (the library runs that entry's kernels), a value that is not finite or outside
[1, 2] is refused with YH_EINVAL before anything is read.  ``box_term`` is ``fakelib_box.box_term`` with the scaled centre as the seed
of the forward-mode chain: value AND derivatives in closed form, in the dtype of its inputs, so the tests can check the hand-written
factor ``s * sig * (1 - sig)`` against autograd in fp64.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import fakelib
import fakelib_box
import fakelib_tta
from engine import hiplib
from engine.hiplib import DecodeDesc, DecodeSxyDesc
from fakelib import flat, pitched
from fakelib_box import (YH_BOX_CIOU, YH_BOX_DIOU, YH_BOX_GIOU, KINDS, _Dual, _clamp0, _datan, _dmax, _dmin, check_box)
from fakelib_focal import check_loss

YH_EINVAL = -1
f32 = np.float32


def scale_ok(s):
    return math.isfinite(s) and 1.0 <= s <= 2.0


def offset_of(s):
    """``c`` as the library forms it: 0.5f * (s - 1.f) on the fp32 ``s``."""
    return float(f32(0.5) * (f32(s) - f32(1.0)))


def box_term(kind, logits4, anchor, tbox, s=1.0):
    """``fakelib_box.box_term`` with the centre ``sigmoid * s - c`` and the seed derivative ``s * sig * (1 - sig)``
    (``box_measure_of<BOX, true>`` of csrc/loss.hip); in fp64 ``c`` is the exact 0.5 * (s - 1)."""
    kind = KINDS.get(kind, kind)
    x = logits4.detach()
    anchor, tb = anchor.to(x.dtype), tbox.to(x.dtype)
    c = lambda v: torch.full_like(x[:, 0], v)
    zero = torch.zeros_like(x[:, 0])
    off = offset_of(s) if x.dtype == torch.float32 else 0.5 * (s - 1)
    sx, sy = torch.sigmoid(x[:, 0]), torch.sigmoid(x[:, 1])
    px = _Dual(sx * s - off, [s * (sx * (1 - sx)), zero, zero, zero])
    py = _Dual(sy * s - off, [zero, s * (sy * (1 - sy)), zero, zero])
    ew, eh = torch.exp(x[:, 2]), torch.exp(x[:, 3])
    wv, hv = ew.clamp(max=1e3) * anchor[:, 0], eh.clamp(max=1e3) * anchor[:, 1]
    pw = _Dual(wv, [zero, zero, torch.where(ew < 1e3, wv, zero), zero])
    ph = _Dual(hv, [zero, zero, zero, torch.where(eh < 1e3, hv, zero)])
    half = _Dual(c(0.5))
    ax1, ax2, ay1, ay2 = px - pw * half, px + pw * half, py - ph * half, py + ph * half
    bx1, bx2 = _Dual(tb[:, 0] - tb[:, 2] / 2), _Dual(tb[:, 0] + tb[:, 2] / 2)
    by1, by2 = _Dual(tb[:, 1] - tb[:, 3] / 2), _Dual(tb[:, 1] + tb[:, 3] / 2)
    inter = _clamp0(_dmin(ax2, bx2) - _dmax(ax1, bx1)) * _clamp0(_dmin(ay2, by2) - _dmax(ay1, by1))
    w1, h1, w2, h2 = ax2 - ax1, ay2 - ay1, bx2 - bx1, by2 - by1
    uni = (w1 * h1 + _Dual(c(1e-16))) + w2 * h2 - inter
    iou = inter / uni
    cw, ch = _dmax(ax2, bx2) - _dmin(ax1, bx1), _dmax(ay2, by2) - _dmin(ay1, by1)
    if kind == YH_BOX_GIOU:
        hull = cw * ch + _Dual(c(1e-16))
        out = iou - (hull - uni) / hull
    else:
        c2 = (cw * cw + ch * ch) + _Dual(c(1e-16))
        dx, dy = (bx1 + bx2) - (ax1 + ax2), (by1 + by2) - (ay1 + ay2)
        rho2 = (dx * dx) * _Dual(c(0.25)) + (dy * dy) * _Dual(c(0.25))
        if kind == YH_BOX_DIOU:
            out = iou - rho2 / c2
        else:
            da = _Dual(torch.atan(w2.v / h2.v)) - _datan(w1 / h1)
            v = _Dual(c(4 / math.pi ** 2)) * (da * da)
            den = (1 - iou.v) + v.v
            dead = den <= 0
            alpha = torch.where(dead, zero, v.v / torch.where(dead, torch.ones_like(den), den))
            out = iou - (rho2 / c2 + v * _Dual(alpha))
    return out.v, torch.stack(out.d, 1)


class _BoxTerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, logits4, anchor, tbox, s):
        v, dv = box_term(kind, logits4, anchor, tbox, s)
        ctx.save_for_backward(dv)
        return v

    @staticmethod
    def backward(ctx, g):
        return None, g[:, None] * ctx.saved_tensors[0], None, None, None


def decode_rows(d, s):
    """(io (n, na, ny, nx, no), raw) of a head descriptor with the scaled centre, torch fp32 in the statement's operation order."""
    c = d.na * d.no
    p = torch.from_numpy(pitched(d.p, d.n * d.ny * d.nx, c, d.ldp, f32).copy())
    raw = p.view(d.n, d.ny, d.nx, d.na, d.no).permute(0, 3, 1, 2, 4).contiguous()
    io = raw.clone()
    gx = torch.arange(d.nx, dtype=torch.float32).view(1, 1, 1, d.nx)
    gy = torch.arange(d.ny, dtype=torch.float32).view(1, 1, d.ny, 1)
    aw = torch.tensor(list(d.anchor_w)[:d.na]).view(1, d.na, 1, 1)
    ah = torch.tensor(list(d.anchor_h)[:d.na]).view(1, d.na, 1, 1)
    off = offset_of(s)
    io[..., 0] = ((torch.sigmoid(raw[..., 0]) * s - off) + gx) * d.stride
    io[..., 1] = ((torch.sigmoid(raw[..., 1]) * s - off) + gy) * d.stride
    io[..., 2] = torch.exp(raw[..., 2]) * aw * d.stride
    io[..., 3] = torch.exp(raw[..., 3]) * ah * d.stride
    io[..., 4:] = torch.sigmoid(raw[..., 4:])
    return io, raw


class FakeLibSxy(fakelib_box.FakeLibBox, fakelib_tta.FakeLibTta):
    def __init__(self):
        super().__init__()
        self.sxy_calls = dict(decode=0, candidates=0, fwd=0, bwd=0)      # calls that ran the scaled form (s != 1)
        self.sxy_args = []                                                # (entry, scale_x_y) of each of them
        self.plan_kinds = []                                              # op kinds as yh_plan_add received them
        self._sxy = 1.0                                                   # the scale of the loss entry that is running

    @staticmethod
    def _obj(dref):
        if dref is None:
            return None
        return dref._obj if hasattr(dref, '_obj') else dref

    # ---- decode
    def yh_yolo_decode(self, dref, stream):
        d = self._obj(dref)
        if isinstance(d, DecodeSxyDesc):        # a replayed YH_OP_DECODE_SXY (yh_plan_add below)
            return self.yh_yolo_decode_sxy(d, stream)
        return super().yh_yolo_decode(d, stream)

    def yh_yolo_decode_sxy(self, dref, stream):
        w = self._obj(dref)
        if w is None or not isinstance(w, DecodeSxyDesc) or not scale_ok(w.scale_x_y):
            return YH_EINVAL
        d, s = w.d, float(w.scale_x_y)
        if s == 1.0:
            return super().yh_yolo_decode(d, stream)
        self.sxy_calls['decode'] += 1
        self.sxy_args.append(('decode', s))
        io, raw = decode_rows(d, s)
        rows = d.na * d.ny * d.nx
        out = flat(d.io, d.n * d.rows_total * d.no, f32).reshape(d.n, d.rows_total, d.no)
        out[:, d.row_off:d.row_off + rows] = io.reshape(d.n, rows, d.no).numpy()
        if fakelib._addr(d.raw):
            flat(d.raw, raw.numel(), f32)[:] = raw.reshape(-1).numpy()
        return 0

    def yh_yolo_decode_candidates_sxy(self, dref, scale, flip_w, conf, ml, class_mask, cand, count, cap, stream):
        w = self._obj(dref)
        if w is None or not isinstance(w, DecodeSxyDesc) or not scale_ok(w.scale_x_y) or not scale > 0 or flip_w != flip_w:
            return YH_EINVAL
        d, s = w.d, float(w.scale_x_y)
        plain = scale == 1.0 and flip_w < 0
        if s == 1.0:
            if plain:
                return self.yh_yolo_decode_candidates(d, conf, ml, class_mask, cand, count, cap, stream)
            return self.yh_yolo_decode_candidates_tta(d, scale, flip_w, conf, ml, class_mask, cand, count, cap, stream)
        self.sxy_calls['candidates'] += 1
        self.sxy_args.append(('candidates', s))
        rows, nc = d.na * d.ny * d.nx, d.no - 5
        io = decode_rows(d, s)[0].reshape(d.n, rows, d.no).numpy()
        if not plain:
            fakelib_tta.deaugment_rows(io, scale, flip_w)      # on the already scaled centre, in models.py's order
        mask = flat(class_mask, nc, np.uint8) if fakelib._addr(class_mask) else None
        for i in range(d.n):
            self._emit(cand, count, cap, i, self._rows_to_records(io[i], d.row_off, nc, conf, ml, mask))
        self.calls.append('decode_candidates_sxy')
        return 0

    # ---- plans: the base emulation keeps its op table private, so a YH_OP_DECODE_SXY op is stored under YH_OP_DECODE with its own
    # descriptor type and yh_yolo_decode above tells the two apart
    def yh_plan_add(self, h, kind, dref, nbytes):
        self.plan_kinds.append(kind)
        if kind != hiplib.OP_DECODE_SXY:
            return super().yh_plan_add(h, kind, dref, nbytes)
        d = self._obj(dref)
        import ctypes as C
        assert nbytes == C.sizeof(DecodeSxyDesc) and isinstance(d, DecodeSxyDesc)
        ops = self.plans[fakelib._addr(h)]['ops']
        ops.append((hiplib.OP_DECODE, DecodeSxyDesc.from_buffer_copy(bytes(d)), []))
        return len(ops) - 1

    # ---- loss
    def _loss_terms(self, d, p):
        if self._sxy == 1.0:
            return super()._loss_terms(d, p)
        tobj = torch.zeros(d.bs, d.na, d.ny, d.nx)
        lbox = p.sum() * 0
        lcls = p.sum() * 0
        idx, tbox, tcls, anc, mask = self._loss_assign(d)
        nb = idx.shape[0]
        if nb:
            b, a, gj, gi = idx.t()
            ps = p[b, a, gj, gi]
            measure = _BoxTerm.apply(self._box, ps[:, :4], anc, tbox, self._sxy)
            lbox = (1.0 - measure).sum()
            tobj[b, a, gj, gi] = (1.0 - d.gr) + d.gr * measure.detach().clamp(0)
            if d.nc > 1:
                t = torch.full_like(ps[:, 5:], d.cn)
                t[range(nb), tcls] = d.cp
                lcls = F.binary_cross_entropy_with_logits(ps[:, 5:], t, pos_weight=torch.tensor([d.cls_pw]), reduction='sum')
        lobj = F.binary_cross_entropy_with_logits(p[..., 4], tobj, pos_weight=torch.tensor([d.obj_pw]), reduction='sum')
        return lbox, lobj, lcls, tobj, nb, mask

    def _head_entry(self, dref, bwd, box, gamma, alpha, s, stream):
        d = self._desc(dref)
        rc = check_loss(d, bwd) or check_box(box, gamma, alpha) or (0 if scale_ok(s) else YH_EINVAL)
        if rc:
            return rc
        if s == 1.0:
            return self._box_entry(dref, bwd, box, gamma, alpha, stream)
        self.sxy_calls['bwd' if bwd else 'fwd'] += 1
        self.sxy_args.append(('bwd' if bwd else 'fwd', s))
        self._box, self._sxy = box, float(f32(s))
        try:
            if gamma > 0:
                return self._focal_bwd(d, gamma, alpha) if bwd else self._focal_fwd(d, gamma, alpha)
            return (self.yh_yolo_loss_bwd if bwd else self.yh_yolo_loss_fwd)(dref, stream)
        finally:
            self._box, self._sxy = YH_BOX_GIOU, 1.0

    def yh_yolo_loss_head_fwd(self, dref, box, gamma, alpha, scale_x_y, stream):
        return self._head_entry(dref, False, box, gamma, alpha, scale_x_y, stream)

    def yh_yolo_loss_head_bwd(self, dref, box, gamma, alpha, scale_x_y, stream):
        return self._head_entry(dref, True, box, gamma, alpha, scale_x_y, stream)
