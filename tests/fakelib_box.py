"""Host emulation of ``yh_yolo_loss_box_fwd`` / ``_bwd`` (csrc/loss.hip) on top of ``fakelib_focal.FakeLibFocal`` — TEST
INFRASTRUCTURE ONLY.

The entries read the descriptor like the existing ones and replace the GIoU of the box term and of the objectness target by the
measure include/yolo_hip.h documents for ``YH_BOX_DIOU`` / ``YH_BOX_CIOU``; with gamma > 0 the two BCE sums take the focal element of
``fakelib_focal``, so focal x box composes as in the kernels.  ``box_term`` evaluates the measure in closed form - value AND the four
derivatives with respect to the raw box logits, forward-mode like the kernel's ``Dual4`` chain, no autograd - in the dtype of its
inputs, so the tests can run it in fp64 against ``utils.bbox_iou`` under autograd and in fp32 on an exact match, where the ``alpha``
rule applies:

    where 1 - iou + v <= 0 (the prediction equals its label: iou == 1 and v == 0), alpha = 0, the limit of v * alpha
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import fakelib_focal
from fakelib import flat
from fakelib_focal import check_focal, check_loss

YH_EINVAL = -1
YH_BOX_GIOU, YH_BOX_DIOU, YH_BOX_CIOU = 0, 1, 2
KINDS = {'giou': YH_BOX_GIOU, 'diou': YH_BOX_DIOU, 'ciou': YH_BOX_CIOU}


class _Dual:
    """Value and the partial derivatives with respect to the four raw box logits, elementwise over the candidates (``Dual4``)."""

    def __init__(self, v, d=None):
        self.v = v
        self.d = d if d is not None else [torch.zeros_like(v) for _ in range(4)]

    def __add__(self, o):
        return _Dual(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])

    def __sub__(self, o):
        return _Dual(self.v - o.v, [a - b for a, b in zip(self.d, o.d)])

    def __mul__(self, o):
        return _Dual(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])

    def __truediv__(self, o):
        inv = 1 / o.v
        v = self.v * inv
        return _Dual(v, [(a - v * b) * inv for a, b in zip(self.d, o.d)])


def _pick(cond, a, b):
    return _Dual(torch.where(cond, a.v, b.v), [torch.where(cond, x, y) for x, y in zip(a.d, b.d)])


def _dmin(a, b):
    return _pick(a.v <= b.v, a, b)


def _dmax(a, b):
    return _pick(a.v >= b.v, a, b)


def _clamp0(a):
    return _pick(a.v > 0, a, _Dual(torch.zeros_like(a.v)))


def _datan(a):
    inv = 1 / (1 + a.v * a.v)
    return _Dual(torch.atan(a.v), [x * inv for x in a.d])


def box_term(kind, logits4, anchor, tbox):
    """(measure (n,), its derivatives (n, 4) with respect to ``logits4``) of candidates ``logits4`` (n, 4) with anchors (n, 2) against
    labels ``tbox`` (n, 4, xywh): ``box_measure_of<BOX>`` of csrc/loss.hip, operation for operation, in ``logits4``'s dtype."""
    kind = KINDS.get(kind, kind)
    x = logits4.detach()
    anchor, tb = anchor.to(x.dtype), tbox.to(x.dtype)
    c = lambda v: torch.full_like(x[:, 0], v)
    zero = torch.zeros_like(x[:, 0])
    sx, sy = torch.sigmoid(x[:, 0]), torch.sigmoid(x[:, 1])
    px = _Dual(sx, [sx * (1 - sx), zero, zero, zero])
    py = _Dual(sy, [zero, sy * (1 - sy), zero, zero])
    ew, eh = torch.exp(x[:, 2]), torch.exp(x[:, 3])
    wv, hv = ew.clamp(max=1e3) * anchor[:, 0], eh.clamp(max=1e3) * anchor[:, 1]
    pw = _Dual(wv, [zero, zero, torch.where(ew < 1e3, wv, zero), zero])          # clamp(max=1e3) cuts the gradient
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
            dead = den <= 0                                                   # a NaN fails the test and propagates
            alpha = torch.where(dead, zero, v.v / torch.where(dead, torch.ones_like(den), den))
            out = iou - (rho2 / c2 + v * _Dual(alpha))                        # alpha: a constant for the derivative
    return out.v, torch.stack(out.d, 1)


class _BoxTerm(torch.autograd.Function):
    """``box_term`` as a node: the closed-form derivatives are what flows back, not autograd's."""

    @staticmethod
    def forward(ctx, kind, logits4, anchor, tbox):
        v, dv = box_term(kind, logits4, anchor, tbox)
        ctx.save_for_backward(dv)
        return v

    @staticmethod
    def backward(ctx, g):
        return None, g[:, None] * ctx.saved_tensors[0], None, None


def check_box(box, gamma, alpha):
    if box not in (YH_BOX_GIOU, YH_BOX_DIOU, YH_BOX_CIOU) or not math.isfinite(gamma) or gamma < 0:
        return YH_EINVAL
    return check_focal(gamma, alpha) if gamma > 0 else 0


class FakeLibBox(fakelib_focal.FakeLibFocal):
    def __init__(self):
        super().__init__()
        self.box_calls = dict(fwd=0, bwd=0)
        self.box_args = []        # (box, gamma, alpha) of every call that would launch
        self._box = YH_BOX_GIOU   # the kind of the entry that is running

    def _loss_terms(self, d, p):
        """``FakeLib._loss_terms`` with the box measure of the running entry (GIoU: the parent's own code)."""
        if self._box == YH_BOX_GIOU:
            return super()._loss_terms(d, p)
        tobj = torch.zeros(d.bs, d.na, d.ny, d.nx)
        lbox = p.sum() * 0
        lcls = p.sum() * 0
        idx, tbox, tcls, anc, mask = self._loss_assign(d)
        nb = idx.shape[0]
        if nb:
            b, a, gj, gi = idx.t()
            ps = p[b, a, gj, gi]
            measure = _BoxTerm.apply(self._box, ps[:, :4], anc, tbox)
            lbox = (1.0 - measure).sum()
            tobj[b, a, gj, gi] = (1.0 - d.gr) + d.gr * measure.detach().clamp(0)
            if d.nc > 1:
                t = torch.full_like(ps[:, 5:], d.cn)
                t[range(nb), tcls] = d.cp
                lcls = F.binary_cross_entropy_with_logits(ps[:, 5:], t, pos_weight=torch.tensor([d.cls_pw]), reduction='sum')
        lobj = F.binary_cross_entropy_with_logits(p[..., 4], tobj, pos_weight=torch.tensor([d.obj_pw]), reduction='sum')
        return lbox, lobj, lcls, tobj, nb, mask

    def _box_entry(self, dref, bwd, box, gamma, alpha, stream):
        d = self._desc(dref)
        rc = check_loss(d, bwd) or check_box(box, gamma, alpha)
        if rc:
            return rc
        self.box_calls['bwd' if bwd else 'fwd'] += 1
        self.box_args.append((box, gamma, alpha))
        self._box = box
        try:
            if gamma > 0:
                return self._focal_bwd(d, gamma, alpha) if bwd else self._focal_fwd(d, gamma, alpha)
            return (self.yh_yolo_loss_bwd if bwd else self.yh_yolo_loss_fwd)(dref, stream)
        finally:
            self._box = YH_BOX_GIOU

    def yh_yolo_loss_box_fwd(self, dref, box, gamma, alpha, stream):
        return self._box_entry(dref, False, box, gamma, alpha, stream)

    def yh_yolo_loss_box_bwd(self, dref, box, gamma, alpha, stream):
        return self._box_entry(dref, True, box, gamma, alpha, stream)

    # the bodies of FakeLibFocal's entries behind their checks and counters (``_focal_parts`` takes the box kind from ``_loss_terms``)
    def _focal_fwd(self, d, gamma, alpha):
        lbox, _, obj, cls, _, tobj, nb, mask = self._focal_parts(d, gamma, alpha)
        flat(d.tobj, tobj.numel(), np.float32)[:] = tobj.reshape(-1).numpy()
        sums = flat(d.sums, 3, np.float32)
        sums[0] += lbox
        sums[1] += float(obj[0].sum())
        sums[2] += float(cls[0].sum()) if cls is not None else 0.0
        count = flat(d.count, 2, np.int32)
        count[0] += nb
        count[1] |= mask
        return 0

    def _focal_bwd(self, d, gamma, alpha):
        scale = float(flat(d.scale, 1, np.float32)[0])
        nb = max(int(flat(d.count, 2, np.int32)[0]), 1)
        _, gbox, obj, cls, idx, _, _, _ = self._focal_parts(d, gamma, alpha)
        g = gbox * (scale * d.g_box / nb)
        g[..., 4] += obj[1] * (scale * d.g_obj / (d.bs * d.na * d.ny * d.nx))
        if cls is not None:
            rows = torch.zeros(idx.shape[0], d.no)
            rows[:, 5:] = cls[1] * (scale * d.g_cls / (nb * d.nc))
            b, a, gj, gi = idx.t()
            g.index_put_((b, a, gj, gi), rows, accumulate=True)
        self._loss_view(d.grad, d, d.gb, d.ga, d.gy, d.gx)[:] = g.numpy()
        return 0
