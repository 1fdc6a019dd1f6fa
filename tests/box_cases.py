"""Shared pieces of the box-loss tests (tests/test_box_loss.py, tests/test_gpu_box_loss.py) — TEST INFRASTRUCTURE ONLY.

There is no reference run of a DIoU / CIoU training loss to record: the reference's ``compute_loss`` hard-codes GIoU and cannot make
one.  What pins these tests is ``utils.bbox_iou``'s golden for all four flags (tests/test_boxutils_golden.py) plus the package's
torch statement around it (``utils.utils.compute_loss(..., fused=False)`` with ``model.box_loss`` set), evaluated on the CPU - in fp64
where a test needs an error-free comparison point.
"""
import math
import os

import torch

import conftest
import focal_cases as fc
import synth
from models import Darknet
from utils import utils as U

KINDS = ('giou', 'diou', 'ciou')
HYP = dict(fc.HYP)
# the two cases of tests/test_gpu_focal_loss.py that reach every branch of the matched kernels: one thread per candidate and no
# class term; the box term in the class-0 thread of 80
CASES = {'hand1': ('yolov3tiny/yolov3-tiny-hand.cfg', 128, 1, 4), 'coco80': ('yolov3/yolov3.cfg', 96, 80, 2)}


def make_case(name):
    """(model, raw heads, labels) of a case: seeded, 12 labels per image so that several targets share a cell."""
    rel, size, nc, batch = CASES[name]
    torch.manual_seed(0)
    model = Darknet(os.path.join(conftest.PKG, 'cfg', rel), (size, size))
    model.nc, model.gr = nc, 0.6
    model.hyp = dict(HYP)
    raws, targets = synth.loss_inputs(model, size, batch=batch, seed=33, labels_per_image=12)
    return model, raws, targets


def configure(model, kind='giou', gamma=0.0, eps=0.0):
    """Set the box kind, gamma and smoothing of a (shared) model: every use sets all three."""
    model.box_loss = kind
    model.hyp = dict(HYP, fl_gamma=gamma, label_smoothing=eps)
    return model


def candidates(n, seed, dtype=torch.float64):
    """Seeded box candidates: logits in [-3, 3], anchors and label sizes in [0.5, 8] grid units, label centres inside the cell;
    followed by three hand-made ones: boxes that do not overlap, a label inside the prediction, and a width logit above ln 1000
    (the clamp cuts its gradient).  Returns (logits (m, 4), anchors (m, 2), labels (m, 4))."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    logits = u(n, 4) * 6 - 3
    anchors = u(n, 2) * 7.5 + 0.5
    tbox = torch.cat((u(n, 2), u(n, 2) * 7.5 + 0.5), 1)
    hand_l = torch.tensor([[3.0, 3.0, -1.0, -1.0],      # centre near (0.95, 0.95), 0.37 x 0.37: clear of the label below
                           [0.2, -0.3, 1.0, 1.2],       # a large prediction around a small label
                           [0.5, 0.1, 7.2, 0.3]], dtype=torch.float64)   # exp(7.2) > 1e3
    hand_a = torch.tensor([[1.0, 1.0], [3.0, 2.0], [0.5, 2.0]], dtype=torch.float64)
    hand_t = torch.tensor([[0.05, 0.05, 0.5, 0.6], [0.5, 0.5, 0.7, 0.5], [0.4, 0.6, 6.0, 2.0]], dtype=torch.float64)
    cat = lambda a, b: torch.cat((a, b)).to(dtype)
    return cat(logits, hand_l), cat(anchors, hand_a), cat(tbox, hand_t)


def decode(logits, anchors):
    """The statement's predicted box (4, n): sigmoid xy, clamped exp wh times the anchor."""
    pxy = torch.sigmoid(logits[:, 0:2])
    pwh = torch.exp(logits[:, 2:4]).clamp(max=1E3) * anchors
    return torch.cat((pxy, pwh), 1).t()


def margins(logits, anchors, tbox):
    """(iou, 1 - iou + v, |atan(w2 / h2) - atan(w1 / h1)|) of every candidate, as ``bbox_iou`` forms them."""
    box = decode(logits, anchors)
    iou = U.bbox_iou(box, tbox, x1y1x2y2=False)
    da = torch.atan(tbox[:, 2] / tbox[:, 3]) - torch.atan(box[2] / box[3])
    v = (4 / math.pi ** 2) * da ** 2
    return iou, 1 - iou + v, da.abs()


def exact_match():
    """A hand-made head with one matched candidate that equals its label exactly: nc 1, one anchor (2, 3), a 4 x 4 grid, the label
    centred in cell (x 1, y 2) with size (2, 3) grid units, zero box logits there (sigmoid 0.5, exp 1) - every number dyadic.
    Returns (raw head (1, 1, 4, 4, 6), anchors (1, 2), labels (1, 6), cell index (b, a, gy, gx))."""
    g = torch.Generator().manual_seed(7)
    raw = torch.randn(1, 1, 4, 4, 6, generator=g) * 0.8
    raw[0, 0, 2, 1, :4] = 0.0
    anchors = torch.tensor([[2.0, 3.0]])
    targets = torch.tensor([[0.0, 0.0, 0.375, 0.625, 0.5, 0.75]])
    return raw, anchors, targets, (0, 0, 2, 1)
