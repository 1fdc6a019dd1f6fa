"""Shared pieces of the scale_x_y tests (tests/test_scale_xy.py, tests/test_gpu_scale_xy.py) — TEST INFRASTRUCTURE ONLY.

The reference ignores ``scale_x_y``, so no recorded run pins these tests.  The pin is the statement itself, written here a second time,
independently of the package's code, in fp64:

    decode   xy = (sigmoid(t) * s - c + cell) * stride,   c = 0.5 * (s - 1)
    loss     pxy = sigmoid(ps[:, 0:2]) * s - c,  then ``utils.bbox_iou`` (pinned by its own golden for all four flags), ``build_targets``,
             the two BCEs and ``FocalLoss`` exactly as ``compute_loss`` uses them

CIoU: the statement's ``alpha = v / (1 - iou + v)`` is 0 / 0 where a prediction equals its label, and the kernels take ``alpha = 0``
there (include/yolo_hip.h).  ``loss_statement`` writes CIoU as ``DIoU - v * alpha`` with that rule, so a case with an exact
match has a finite comparison point.
"""
import ctypes as C
import math
import types

import numpy as np
import torch
import torch.nn as nn

import focal_cases as fc
import models
from engine import hiplib
from engine.hiplib import DecodeDesc, DecodeSxyDesc
from utils import utils as U

SCALES = (1.05, 1.2, 2.0)
STRIDE = 8
ANCHORS_PX = np.array([[8., 12.], [16., 24.], [28., 16.]])      # grid units at stride 8: (1, 1.5), (2, 3), (3.5, 2) - dyadic
NC, NA, NY, NX, BS = 3, 3, 4, 5, 2
EXACT = (0, 1, 1, 2)      # (image, anchor, gy, gx) of the candidate that equals its label
# image, class, x, y, w, h (normalised).  0: equals the zero-logit prediction of anchor 1 in cell (x 2, y 1) exactly; 1: centred on
# a cell border in x and y (x * nx = 2 and y * ny = 2 in fp32 and fp64); 2: offset 0.999 inside cell (x 3, y 2); 3 and 4 share
# cell (0, 0) of image 1; 5: a small box in a corner cell
LABELS = torch.tensor([[0, 1, 0.5, 0.375, 0.4, 0.75],
                       [1, 0, 0.4, 0.5, 0.3, 0.3],
                       [0, 2, 3.999 / 5, 2.999 / 4, 0.5, 0.6],
                       [1, 1, 0.13, 0.13, 0.35, 0.5],
                       [1, 2, 0.15, 0.17, 0.4, 0.45],
                       [0, 0, 0.9, 0.1, 0.2, 0.25]])


def head_model(s, kind='giou', gamma=0.0):
    """A one-head stand-in for a Darknet as ``compute_loss`` reads it: the real ``YOLOLayer`` with ``scale_x_y = s``, hyp, nc, gr."""
    layer = models.YOLOLayer(anchors=ANCHORS_PX, nc=NC, img_size=(NX * STRIDE, NY * STRIDE), yolo_index=0, layers=[], stride=STRIDE,
                             scale_x_y=s)
    return types.SimpleNamespace(module_list=[layer], yolo_layers=[0], hyp=dict(fc.HYP, fl_gamma=gamma), nc=NC, gr=0.6, box_loss=kind)


def raw_head(exact=True, seed=21):
    """The raw head (bs, na, ny, nx, no), seeded; ``exact``: zero box logits where label 0 sits, so that prediction equals its label."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(BS, NA, NY, NX, NC + 5, generator=g) * 0.8
    if exact:
        b, a, gy, gx = EXACT
        raw[b, a, gy, gx, :4] = 0.0
    return raw


def decode_statement(p, anchor_vec, stride, s):
    """fp64 numpy: p (N, na, ny, nx, no) raw -> (N, na * ny * nx, no) decoded, the statement with ``c = 0.5 * (s - 1)``."""
    p = np.asarray(p, np.float64)
    N, na, ny, nx, no = p.shape
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    out = np.empty_like(p)
    c = 0.5 * (s - 1)
    out[..., 0] = (sig(p[..., 0]) * s - c + np.arange(nx).reshape(1, 1, 1, nx)) * stride
    out[..., 1] = (sig(p[..., 1]) * s - c + np.arange(ny).reshape(1, 1, ny, 1)) * stride
    av = np.asarray(anchor_vec, np.float64)
    out[..., 2] = np.exp(p[..., 2]) * av[:, 0].reshape(1, na, 1, 1) * stride
    out[..., 3] = np.exp(p[..., 3]) * av[:, 1].reshape(1, na, 1, 1) * stride
    out[..., 4:] = sig(p[..., 4:])
    return out.reshape(N, -1, no)


def box_measure(pbox, tbox, kind):
    """GIoU / DIoU through ``bbox_iou``; CIoU as DIoU - v * alpha with alpha = 0 where 1 - iou + v <= 0 (see the module docstring)."""
    if kind == 'giou':
        return U.bbox_iou(pbox, tbox, x1y1x2y2=False, GIoU=True)
    diou = U.bbox_iou(pbox, tbox, x1y1x2y2=False, DIoU=True)
    if kind == 'diou':
        return diou
    iou = U.bbox_iou(pbox, tbox, x1y1x2y2=False)
    v = (4 / math.pi ** 2) * (torch.atan(tbox[:, 2] / tbox[:, 3]) - torch.atan(pbox[2] / pbox[3])) ** 2
    with torch.no_grad():
        den = 1 - iou + v
        alpha = torch.where(den <= 0, torch.zeros_like(den), v / torch.where(den <= 0, torch.ones_like(den), den))
    return diou - v * alpha


def loss_statement(raws, targets, model, scales, dtype=torch.float64, scale=7.0):
    """(items [lbox, lobj, lcls, loss], gradient of every raw head) of the loss statement with ``pxy = sigmoid * s - c`` per head, on the
    CPU in ``dtype``, loss scaled by ``scale`` before backward.  Cells matched by several labels take the last label's objectness."""
    ps = [r.detach().cpu().to(dtype).clone().requires_grad_() for r in raws]
    targets = targets.detach().cpu().to(dtype)
    h = model.hyp
    kind = getattr(model, 'box_loss', 'giou')
    tcls, tbox, indices, anchor_vec = U.build_targets(ps, targets, model)
    bce_cls = nn.BCEWithLogitsLoss(pos_weight=torch.tensor([h['cls_pw']], dtype=dtype), reduction='mean')
    bce_obj = nn.BCEWithLogitsLoss(pos_weight=torch.tensor([h['obj_pw']], dtype=dtype), reduction='mean')
    if h['fl_gamma'] > 0:
        bce_cls, bce_obj = U.FocalLoss(bce_cls, h['fl_gamma']), U.FocalLoss(bce_obj, h['fl_gamma'])
    lbox = lobj = lcls = torch.zeros((), dtype=dtype)
    for i, pi in enumerate(ps):
        b, a, gj, gi = indices[i]
        tobj = torch.zeros_like(pi[..., 0])
        if len(b):
            sel = pi[b, a, gj, gi]
            s = scales[i]
            pxy = torch.sigmoid(sel[:, 0:2]) * s - 0.5 * (s - 1)
            pwh = torch.exp(sel[:, 2:4]).clamp(max=1e3) * anchor_vec[i].to(dtype)
            m = box_measure(torch.cat((pxy, pwh), 1).t(), tbox[i].to(dtype), kind)
            lbox = lbox + (1.0 - m).mean()
            tobj[b, a, gj, gi] = (1.0 - model.gr) + model.gr * m.detach().clamp(0)
            if model.nc > 1:
                t = torch.zeros_like(sel[:, 5:])
                t[range(len(b)), tcls[i]] = 1.0
                lcls = lcls + bce_cls(sel[:, 5:], t)
        lobj = lobj + bce_obj(pi[..., 4], tobj)
    lbox, lobj, lcls = lbox * h['giou'], lobj * h['obj'], lcls * h['cls']
    loss = lbox + lobj + lcls
    (loss * scale).backward()
    return torch.stack((lbox, lobj, lcls, loss)).detach(), [p.grad for p in ps]


def head_map(N, ny, nx, na, nc, pitch, seed=14, scale=1.0):
    """A head convolution's output (N, ny, nx, pitch) fp32 with seeded values in its first na * (5 + nc) channels."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(N, ny, nx, pitch)
    p[..., :na * (nc + 5)] = torch.randn(N, ny, nx, na * (nc + 5), generator=g) * scale
    return p


def decode_desc(p, io, raw, na, no, stride, anchor_vec, rows_total, row_off, s=None):
    """yh_decode_desc of a head map ``p`` (N, ny, nx, ldp), or yh_decode_sxy_desc around it when ``s`` is given."""
    N, ny, nx, ldp = p.shape
    d = DecodeDesc(p=hiplib.ptr(p), io=hiplib.ptr(io), raw=hiplib.ptr(raw), n=N, ny=ny, nx=nx, na=na, no=no, ldp=ldp,
                   rows_total=rows_total, row_off=row_off, stride=float(stride))
    for a in range(na):
        d.anchor_w[a] = float(anchor_vec[a][0])
        d.anchor_h[a] = float(anchor_vec[a][1])
    return d if s is None else DecodeSxyDesc(d=d, scale_x_y=s)


def raw_view(p, na, no):
    """(N, na, ny, nx, no) view order of a head map, as YOLOLayer and the decode kernels' ``raw`` output have it."""
    N, ny, nx, _ = p.shape
    return p[..., :na * no].reshape(N, ny, nx, na, no).permute(0, 3, 1, 2, 4).contiguous()


def host_decode(raw, anchors_px, stride, s, nc):
    """The fp32 host statement: the package's ``YOLOLayer`` (eval, CPU) on a raw head in its (N, na, ny, nx, no) order."""
    N, na, ny, nx, no = raw.shape
    layer = models.YOLOLayer(anchors=np.asarray(anchors_px, np.float64), nc=nc, img_size=(nx * stride, ny * stride), yolo_index=0,
                             layers=[], stride=stride, scale_x_y=s).eval()
    p = raw.cpu().permute(0, 1, 4, 2, 3).reshape(N, na * no, ny, nx)
    with torch.no_grad():
        return layer(p, None)[0]


def sorted_records(cand, count, img):
    """The records of one image ordered by key (the slot order depends on the atomics), as int32 bit patterns."""
    k = int(count[img])
    rec = cand[img, :k].cpu().contiguous().view(torch.int32)
    return rec[torch.argsort(rec[:, 6])]


def byref(d):
    return C.byref(d)
