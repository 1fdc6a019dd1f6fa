"""Shared pieces of the focal-loss tests (tests/test_focal_loss.py, tests/test_gpu_focal_loss.py) — TEST INFRASTRUCTURE ONLY.

The comparison point of both tiers is the package's torch statement (``utils.utils.compute_loss(..., fused=False)``) evaluated on the
CPU, in fp64 where a test needs an error-free reference.  ``closed_form_focal`` swaps the statement's ``FocalLoss`` for a module with
the same interface whose elements come from ``fakelib_focal.focal_elem`` - the documented closed form with the ``q <= 0`` rule - so the
saturated gamma < 1 cases, where autograd's ``pow`` backward is not finite, have a finite fp64 reference too.
"""
import contextlib

import torch
import torch.nn as nn

import fakelib_focal
from utils import utils as U

HYP = {'giou': 3.54, 'cls': 37.4, 'cls_pw': 1.3, 'obj': 64.3, 'obj_pw': 0.8, 'iou_t': 0.20, 'fl_gamma': 0.0}
GAMMAS = [0.5, 1.0, 1.5, 2.0, 3.0]


class _ClosedElem(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, pw, gamma, alpha):
        L, dL = fakelib_focal.focal_elem(x, t, pw, gamma, alpha)
        ctx.save_for_backward(dL)
        return L

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None, None, None


class ClosedFormFocalLoss(nn.Module):
    """``utils.utils.FocalLoss``'s interface on the closed-form element (value and derivative, no ``pow`` under autograd)."""

    def __init__(self, loss_fcn, gamma=1.5, alpha=0.25):
        super().__init__()
        self.pw, self.gamma, self.alpha, self.reduction = float(loss_fcn.pos_weight), gamma, alpha, loss_fcn.reduction

    def forward(self, pred, true):
        loss = _ClosedElem.apply(pred, true.detach(), self.pw, self.gamma, self.alpha)
        if self.reduction == 'mean':
            return loss.mean()
        return loss.sum() if self.reduction == 'sum' else loss


@contextlib.contextmanager
def closed_form_focal():
    keep, U.FocalLoss = U.FocalLoss, ClosedFormFocalLoss
    try:
        yield
    finally:
        U.FocalLoss = keep


def round_up(n, m):
    return (n + m - 1) // m * m


def nhwc_views(raws, dev, dtype=torch.float32, pad_to=8):
    """The raw heads as the training forward hands them out: ``(bs, na, ny, nx, no)`` views of NHWC bases whose last axis is padded
    (at least one padding channel).  Returns (bases with requires_grad, views)."""
    bases, views = [], []
    for r in raws:
        bs, na, ny, nx, no = r.shape
        base = torch.zeros(bs, ny, nx, round_up(na * no + 1, pad_to), device=dev, dtype=dtype)
        base[..., :na * no] = r.to(device=dev, dtype=dtype).permute(0, 2, 3, 1, 4).reshape(bs, ny, nx, na * no)
        base.requires_grad_()
        bases.append(base)
        views.append(base[..., :na * no].view(bs, ny, nx, na, no).permute(0, 3, 1, 2, 4))
    return bases, views


def torch_statement(raws, targets, model, dtype=torch.float64, closed=False, scale=7.0):
    """(items, [gradient of every NHWC base]) of the package's torch statement on the CPU in ``dtype``, loss scaled before backward."""
    bases, views = nhwc_views(raws, 'cpu', dtype)
    with (closed_form_focal() if closed else contextlib.nullcontext()):
        loss, items = U.compute_loss(views, targets, model, fused=False)
        (loss * scale).backward()
    return items, [b.grad for b in bases]


def saturate(raws, seed, frac=0.02, lo=17.0, hi=60.0):
    """Copies of the raw heads with ``frac`` of the objectness and class logits replaced by values in +-[lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for r in raws:
        r = r.clone()
        part = r[..., 4:]
        hit = torch.rand(part.shape, generator=g) < frac
        mag = torch.rand(part.shape, generator=g) * (hi - lo) + lo
        sign = torch.where(torch.rand(part.shape, generator=g) < 0.5, -1.0, 1.0)
        part[hit] = (mag * sign)[hit]
        out.append(r)
    return out


def assert_close_to(items, grads, ref_items, ref_grads, item_rtol=1e-5, item_atol=1e-6, grad_rel=1e-4, what=''):
    """Loss items ``rtol 1e-5, atol 1e-6``; every head's gradient within ``grad_rel`` of the reference's largest magnitude."""
    items, ref_items = items.detach().double().cpu(), ref_items.detach().double().cpu()
    assert torch.isfinite(items).all(), (what, items)
    assert torch.allclose(items, ref_items, rtol=item_rtol, atol=item_atol), (what, items, ref_items)
    for i, (a, b) in enumerate(zip(grads, ref_grads)):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        assert torch.isfinite(a).all(), (what, i)
        err, top = (a - b).abs().max().item(), b.abs().max().item()
        assert err <= grad_rel * top, (what, i, err, top)
