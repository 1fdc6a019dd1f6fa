"""Host emulation of ``yh_yolo_loss_focal_fwd`` / ``_bwd`` (csrc/loss.hip) on top of ``fakelib.FakeLib`` — TEST INFRASTRUCTURE ONLY.

The entries read the descriptor exactly like ``FakeLib.yh_yolo_loss_fwd`` / ``_bwd`` (same strided views, same target assignment, same
box term, tobj, sums and counts) and replace the two BCE sums by the focal element documented in include/yolo_hip.h:

    s = sigmoid(x)          B = bce(x, t, pos_weight)
    q = t + s * (1 - 2 t)   a = t * alpha + (1 - t) * (1 - alpha)      M = q ^ gamma
    L = B * a * M
    dL/dx = a * (dB/dx * M + B * gamma * q^(gamma - 1) * (1 - 2 t) * s * (1 - s))

with L = dL/dx = 0 where q <= 0 (the limit: B vanishes like q).  ``focal_elem`` evaluates that closed form - value AND derivative, no
autograd - in the dtype of its inputs, so the tests can run it in fp64 against ``utils.utils.FocalLoss`` under autograd and in fp32 on
saturated elements; the backward entry writes the closed-form derivative, not an autograd result.
"""
import math

import numpy as np
import torch

import fakelib
from fakelib import flat

YH_EINVAL = -1


def focal_elem(x, t, pw, gamma, alpha):
    """(L, dL/dx) of the focal element, elementwise, in ``x``'s dtype; ``t`` broadcasts against ``x``."""
    x = x.detach()
    t = torch.as_tensor(t, dtype=x.dtype).expand_as(x)
    s = torch.sigmoid(x)
    sp = (-x).clamp(min=0) + torch.log1p(torch.exp(-x.abs()))          # softplus(-x) = -log sigmoid(x)
    B = (1 - t) * x + (1 + (pw - 1) * t) * sp
    dB = s * (1 - t + pw * t) - pw * t
    u = 1 - 2 * t
    q = t + s * u
    a = t * alpha + (1 - t) * (1 - alpha)
    live = ~(q <= 0)                                                   # a NaN logit stays NaN, as in the BCE
    qs = torch.where(live, q, torch.ones_like(q))
    M = qs ** gamma
    L = B * a * M
    dL = a * (dB * M + (B / qs) * M * gamma * u * s * (1 - s))
    zero = torch.zeros_like(x)
    return torch.where(live, L, zero), torch.where(live, dL, zero)


def check_focal(gamma, alpha):
    ok = math.isfinite(gamma) and gamma > 0 and math.isfinite(alpha) and 0 <= alpha <= 1
    return 0 if ok else YH_EINVAL


def check_loss(d, bwd):
    """check_loss of csrc/loss.hip."""
    if d is None or not d.p or not d.tobj or d.bs <= 0 or d.na <= 0 or d.ny <= 0 or d.nx <= 0 or d.no < 5 or d.nc != d.no - 5:
        return YH_EINVAL
    if d.nt < 0 or not d.count or (d.nt > 0 and (not d.targets or not d.anchors or (not bwd and not d.winner))):
        return YH_EINVAL
    if (not d.grad or not d.scale) if bwd else not d.sums:
        return YH_EINVAL
    return 0


class FakeLibFocal(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.focal_calls = dict(fwd=0, bwd=0)
        self.focal_args = []      # (gamma, alpha) of every call that would launch

    @staticmethod
    def _desc(dref):
        if dref is None:
            return None
        return dref._obj if hasattr(dref, '_obj') else dref

    def _focal_parts(self, d, gamma, alpha):
        """Per-element focal values and derivatives of one head: objectness over every cell, classes over the matched rows
        (None for nc == 1), the box sum / tobj / nb / mask of ``FakeLib._loss_terms`` and the matched index."""
        p = torch.from_numpy(self._loss_view(d.p, d, d.sb, d.sa, d.sy, d.sx).copy())
        with torch.enable_grad():
            pv = p.clone().requires_grad_()
            lbox, _, _, tobj, nb, mask = self._loss_terms(d, pv)
            gbox = torch.autograd.grad(lbox, pv)[0] if nb else torch.zeros_like(p)
        obj = focal_elem(p[..., 4], tobj, d.obj_pw, gamma, alpha)
        idx, cls = None, None
        if nb and d.nc > 1:
            idx, _, tcls, _, _ = self._loss_assign(d)
            b, a, gj, gi = idx.t()
            t = torch.full((nb, d.nc), d.cn)
            t[range(nb), tcls] = d.cp
            cls = focal_elem(p[b, a, gj, gi][:, 5:], t, d.cls_pw, gamma, alpha)
        return float(lbox), gbox, obj, cls, idx, tobj, nb, mask

    def yh_yolo_loss_focal_fwd(self, dref, gamma, alpha, stream):
        d = self._desc(dref)
        rc = check_loss(d, False) or check_focal(gamma, alpha)
        if rc:
            return rc
        self.focal_calls['fwd'] += 1
        self.focal_args.append((gamma, alpha))
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

    def yh_yolo_loss_focal_bwd(self, dref, gamma, alpha, stream):
        d = self._desc(dref)
        rc = check_loss(d, True) or check_focal(gamma, alpha)
        if rc:
            return rc
        self.focal_calls['bwd'] += 1
        self.focal_args.append((gamma, alpha))
        scale = float(flat(d.scale, 1, np.float32)[0])
        nb = max(int(flat(d.count, 2, np.int32)[0]), 1)
        _, gbox, obj, cls, idx, _, _, _ = self._focal_parts(d, gamma, alpha)
        g = gbox * (scale * d.g_box / nb)
        g[..., 4] += obj[1] * (scale * d.g_obj / (d.bs * d.na * d.ny * d.nx))
        if cls is not None:
            rows = torch.zeros(idx.shape[0], d.no)
            rows[:, 5:] = cls[1] * (scale * d.g_cls / (nb * d.nc))
            b, a, gj, gi = idx.t()
            g.index_put_((b, a, gj, gi), rows, accumulate=True)      # several candidates of one cell accumulate, as the kernel's atomics
        self._loss_view(d.grad, d, d.gb, d.ga, d.gy, d.gx)[:] = g.numpy()
        return 0
