"""compute_loss on the HIP kernels (csrc/loss.hip): the autograd node behind ``utils.utils.compute_loss`` for CUDA tensors.

The reference evaluates the loss with ~200 small torch kernels per step, autograd then builds several full-size
zero-filled temporaries per head (index_put / select backward), and ``build_targets`` reads data-dependent sizes back to
the host three times per head.  Here the forward is three launches per head (target assignment, matched candidates,
objectness over every cell) and the backward two more that write the complete gradient of each raw head tensor, scaled
by autograd's incoming scalar on the device.  Nothing in the step waits for the GPU, so the host keeps enqueuing the
backward while the forward still runs.

The reference's label check (``build_targets`` asserts every class < nc, utils.py:757-760) needs the labels on the host;
here the kernels record a label error mask on the device, the mask is copied to pinned host memory asynchronously and the
same AssertionError is raised by the NEXT ``compute_loss`` call (or ``flush_label_check()``), after the copy has landed.

``hyp['fl_gamma'] > 0`` (the reference wraps both BCEs in ``FocalLoss(gamma, alpha=0.25)``) takes the same node through the focal
entries ``yh_yolo_loss_focal_fwd`` / ``_bwd``: the same launches with the focal element in the objectness and class terms, the same
sums, counts, normalisation and label check.  ``YOLO_HIP_FOCAL_LOSS=0`` keeps the torch statement for focal loss (A/B runs);
``stats()`` counts the focal calls.  Where a logit is saturated on the side of its 0 / 1 target the kernels return the limit 0 and
stay finite; fp32 torch returns inf / nan there for gamma < 1 (include/yolo_hip.h).

``model.box_loss`` in ``('diou', 'ciou')`` (darknet's ``iou_loss``, ``train.py --box-loss``) takes the node through
``yh_yolo_loss_box_fwd`` / ``_bwd``: the matched kernels with that box measure in ``lbox`` and in the objectness target, with or
without the focal element.  GIoU keeps the entries above.  ``YOLO_HIP_BOX_LOSS=0`` keeps the torch statement for DIoU / CIoU (A/B
runs); ``box_stats()`` counts the calls.  Where a prediction equals its label exactly the CIoU kernels take ``alpha = 0`` and stay
finite; the torch statement returns nan there (include/yolo_hip.h).  ``hyp['label_smoothing']`` only changes the two
class targets ``cp`` / ``cn`` of the descriptor, so it never leaves the fused path.

A head whose yolo module has ``scale_x_y != 1`` (darknet's grid sensitivity, ``Darknet(scale_x_y=True)``, ``--scale-x-y``) goes
through ``yh_yolo_loss_head_fwd`` / ``_bwd``: the matched kernels with ``pxy = sigmoid * s - 0.5 (s - 1)`` and its derivative, any box
kind, with or without the focal element; the other heads of the model keep the entries above.  ``YOLO_HIP_SCALE_XY=0`` keeps the
torch statement for a model with such a head (A/B runs); ``scale_stats()`` counts the calls.
"""
import ctypes as C
import os

import torch

from . import hiplib
from .hiplib import LossDesc

_LIB_OVERRIDE = None   # tests inject the host emulation here
FOCAL_ALPHA = 0.25     # utils.utils.compute_loss builds FocalLoss(bce, fl_gamma) with the class's default alpha
_STATS = dict(focal_fwd=0, focal_bwd=0)
BOX_KINDS = {'giou': 0, 'diou': 1, 'ciou': 2}      # YH_BOX_* of include/yolo_hip.h
_BOX_STATS = dict(box_fwd=0, box_bwd=0)
_SCALE_STATS = dict(scale_fwd=0, scale_bwd=0)


def _lib():
    return _LIB_OVERRIDE if _LIB_OVERRIDE is not None else hiplib.load()


def stats():
    """Counters since ``reset_stats``: calls of the focal forward and backward entries (one per head and pass)."""
    return dict(_STATS)


def reset_stats():
    for k in _STATS:
        _STATS[k] = 0


def box_stats():
    """Counters since ``reset_box_stats``: calls of ``yh_yolo_loss_box_fwd`` / ``_bwd`` (one per head and pass, DIoU / CIoU only)."""
    return dict(_BOX_STATS)


def reset_box_stats():
    for k in _BOX_STATS:
        _BOX_STATS[k] = 0


def scale_stats():
    """Counters since ``reset_scale_stats``: calls of ``yh_yolo_loss_head_fwd`` / ``_bwd`` (one per scaled head and pass)."""
    return dict(_SCALE_STATS)


def reset_scale_stats():
    for k in _SCALE_STATS:
        _SCALE_STATS[k] = 0


def head_scales(model, yolo_modules):
    """``scale_x_y`` of the model's yolo modules in head order (1.0 for a module without the attribute)."""
    return [float(getattr(layer, 'scale_x_y', 1.0)) for layer in yolo_modules(model)]


def box_kind(model):
    """``model.box_loss`` ('giou' when the model has none) as YH_BOX_*; an unknown kind raises ValueError naming it."""
    kind = getattr(model, 'box_loss', 'giou')
    if kind not in BOX_KINDS:
        raise ValueError('unknown box loss %r: expected one of %s' % (kind, ', '.join(BOX_KINDS)))
    return BOX_KINDS[kind]


def usable(p, model, scaled=False):
    """Fused path: CUDA (or an injected emulator), fp32 raw heads with unit stride on the last axis; focal loss too unless
    ``YOLO_HIP_FOCAL_LOSS=0`` keeps the torch statement for it, DIoU / CIoU too unless ``YOLO_HIP_BOX_LOSS=0`` does, a head with
    ``scale_x_y != 1`` (``scaled``) too unless ``YOLO_HIP_SCALE_XY=0`` does."""
    if _LIB_OVERRIDE is None and not p[0].is_cuda:
        return False
    if model.hyp.get('fl_gamma', 0.0) > 0 and os.environ.get('YOLO_HIP_FOCAL_LOSS', '1') == '0':
        return False
    if box_kind(model) != BOX_KINDS['giou'] and os.environ.get('YOLO_HIP_BOX_LOSS', '1') == '0':
        return False
    if scaled and os.environ.get('YOLO_HIP_SCALE_XY', '1') == '0':
        return False
    return all(t.dtype == torch.float32 and t.dim() == 5 and t.stride(4) == 1 for t in p)


_pending = []   # (event or None, host int32 tensor (heads, 2), nc) of launched forwards whose label mask is unread


def flush_label_check():
    """Raise for label errors recorded by earlier compute_loss launches (waits for their kernels)."""
    while _pending:
        event, host, nc = _pending.pop(0)
        if event is not None:
            event.synchronize()
        mask = int(host[:, 1].max()) if host.numel() else 0
        if mask & 1:
            raise AssertionError('Model accepts %g classes labeled from 0-%g, however you labelled a class outside that '
                                 'range. See https://docs.ultralytics.com/yolov5/tutorials/train_custom_data' % (nc, nc - 1))
        if mask & 2:
            raise IndexError('a label refers to an image index outside the batch or a box centre outside [0, 1)')


def _head_bases(p):
    """The NHWC head tensors ``(bs, ny, nx, ld)`` the raw heads are views of, when every ``p[i]`` is exactly the view
    ``base[..., :na * no].view(bs, ny, nx, na, no).permute(0, 3, 1, 2, 4)`` the training forward hands out (models.py
    ``_forward_hip_train``); None otherwise.  With the bases as the autograd inputs the loss backward writes the gradient of the
    head tensor itself - autograd's slice / view backward (a zero fill plus a strided copy of every head, ~0.3 ms per step at
    YOLOv3-608 batch 64) disappears."""
    out = []
    for t in p:
        b = t._base
        if b is None or b.dim() != 4 or b.dtype != torch.float32 or not b.is_contiguous() or not b.requires_grad:
            return None
        bs, na, ny, nx, no = t.shape
        ld = b.shape[3]
        if tuple(b.shape[:3]) != (bs, ny, nx) or na * no > ld or t.data_ptr() != b.data_ptr():
            return None
        if tuple(t.stride()) != (ny * nx * ld, no, nx * ld, ld, 1):
            return None
        out.append((b, na, no))
    return out


class _YoloLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *ps):
        lib = _lib()
        dev = ps[0].device
        nh = len(ps)
        ctx.on_bases = meta.get('geom') is not None
        if ctx.on_bases:     # inputs are the NHWC head tensors: rebuild the (bs, na, ny, nx, no) views the kernels address
            ps = tuple(b[..., :na * no].view(b.shape[0], b.shape[1], b.shape[2], na, no).permute(0, 3, 1, 2, 4)
                       for b, (na, no) in zip(ps, meta['geom']))
        targets = meta['targets']
        nt = int(targets.shape[0])
        sums = torch.zeros((nh, 3), device=dev, dtype=torch.float32)
        counts = torch.zeros((nh, 2), device=dev, dtype=torch.int32)
        heads, cells = [], []
        for i, p in enumerate(ps):
            bs, na, ny, nx, no = p.shape
            tobj = torch.zeros((bs, na, ny, nx), device=dev, dtype=torch.float32)
            winner = torch.full((bs, na, ny, nx), -1, device=dev, dtype=torch.int32) if nt else None
            anchors = meta['anchors'][i]
            d = LossDesc(p=hiplib.ptr(p), grad=None, tobj=hiplib.ptr(tobj), winner=hiplib.ptr(winner),
                         targets=hiplib.ptr(targets) if nt else None, anchors=hiplib.ptr(anchors), sums=hiplib.ptr(sums, 3 * i),
                         count=hiplib.ptr(counts, 2 * i), scale=None,
                         sb=p.stride(0), sa=p.stride(1), sy=p.stride(2), sx=p.stride(3), gb=0, ga=0, gy=0, gx=0,
                         bs=bs, na=na, ny=ny, nx=nx, no=no, nc=no - 5, nt=nt, iou_t=meta['iou_t'], gr=meta['gr'],
                         cp=meta['cp'], cn=meta['cn'], cls_pw=meta['cls_pw'], obj_pw=meta['obj_pw'],
                         g_box=meta['giou'], g_obj=meta['obj'], g_cls=meta['cls'])
            if meta['sxy'][i] != 1.0:
                hiplib.check(lib.yh_yolo_loss_head_fwd(C.byref(d), meta['box'], meta['gamma'], meta['alpha'], meta['sxy'][i],
                                                       hiplib.stream_ptr()), 'yh_yolo_loss_head_fwd')
                _SCALE_STATS['scale_fwd'] += 1
                _BOX_STATS['box_fwd'] += meta['box'] > 0
                _STATS['focal_fwd'] += meta['gamma'] > 0
            elif meta['box']:
                hiplib.check(lib.yh_yolo_loss_box_fwd(C.byref(d), meta['box'], meta['gamma'], meta['alpha'], hiplib.stream_ptr()), 'yh_yolo_loss_box_fwd')
                _BOX_STATS['box_fwd'] += 1
                _STATS['focal_fwd'] += meta['gamma'] > 0
            elif meta['gamma'] > 0:
                hiplib.check(lib.yh_yolo_loss_focal_fwd(C.byref(d), meta['gamma'], meta['alpha'], hiplib.stream_ptr()), 'yh_yolo_loss_focal_fwd')
                _STATS['focal_fwd'] += 1
            else:
                hiplib.check(lib.yh_yolo_loss_fwd(C.byref(d), hiplib.stream_ptr()), 'yh_yolo_loss_fwd')
            heads.append((d, tobj, p, meta['sxy'][i]))
            cells.append(float(bs * na * ny * nx))
            del winner   # only the forward needs it (stream-ordered free)
        nc = ps[0].shape[4] - 5
        nb = counts[:, 0].clamp(min=1).to(torch.float32)
        lbox = (sums[:, 0] / nb).sum() * meta['giou']
        lobj = sum(sums[i, 1] / cells[i] for i in range(nh)) * meta['obj']
        lcls = (sums[:, 2] / (nb * nc)).sum() * meta['cls'] if nc > 1 else torch.zeros((), device=dev)
        if dev.type == 'cuda':
            host = torch.empty((nh, 2), dtype=torch.int32, pin_memory=True)
            host.copy_(counts, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            _pending.append((event, host, nc))
        else:
            _pending.append((None, counts, nc))
            flush_label_check()
        ctx.heads, ctx.keep_fwd = heads, (targets, counts, meta['anchors'])
        ctx.focal = (meta['gamma'], meta['alpha'])
        ctx.box = meta['box']
        loss = lbox + lobj + lcls
        ctx.mark_non_differentiable(lbox, lobj, lcls)
        return loss, lbox, lobj, lcls

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_lbox, g_lobj, g_lcls):
        lib = _lib()
        scale = g_loss.detach().float().contiguous().reshape(1)
        gamma, alpha = ctx.focal
        grads = []
        for d, tobj, p, sxy in ctx.heads:
            if ctx.on_bases:
                bs, na, ny, nx, no = p.shape
                ld = p.stride(3)
                full = torch.empty((bs, ny, nx, ld), device=p.device, dtype=torch.float32)      # gradient of the head tensor itself
                if ld > na * no:
                    full[..., na * no:].zero_()                                                  # channel padding of the head conv
                g = full[..., :na * no].view(bs, ny, nx, na, no).permute(0, 3, 1, 2, 4)
            else:
                g = full = torch.empty_strided(p.shape, p.stride(), device=p.device, dtype=torch.float32)
            d.grad, d.scale = hiplib.ptr(g), hiplib.ptr(scale)
            d.gb, d.ga, d.gy, d.gx = g.stride(0), g.stride(1), g.stride(2), g.stride(3)
            with hiplib.on_device(p):
                if sxy != 1.0:
                    hiplib.check(lib.yh_yolo_loss_head_bwd(C.byref(d), ctx.box, gamma, alpha, sxy, hiplib.stream_ptr()), 'yh_yolo_loss_head_bwd')
                    _SCALE_STATS['scale_bwd'] += 1
                    _BOX_STATS['box_bwd'] += ctx.box > 0
                    _STATS['focal_bwd'] += gamma > 0
                elif ctx.box:
                    hiplib.check(lib.yh_yolo_loss_box_bwd(C.byref(d), ctx.box, gamma, alpha, hiplib.stream_ptr()), 'yh_yolo_loss_box_bwd')
                    _BOX_STATS['box_bwd'] += 1
                    _STATS['focal_bwd'] += gamma > 0
                elif gamma > 0:
                    hiplib.check(lib.yh_yolo_loss_focal_bwd(C.byref(d), gamma, alpha, hiplib.stream_ptr()), 'yh_yolo_loss_focal_bwd')
                    _STATS['focal_bwd'] += 1
                else:
                    hiplib.check(lib.yh_yolo_loss_bwd(C.byref(d), hiplib.stream_ptr()), 'yh_yolo_loss_bwd')
            grads.append(full)
        ctx.keep = scale
        return (None,) + tuple(grads)


def compute_loss(p, targets, model, yolo_modules, smooth_bce):
    """Same contract as utils.utils.compute_loss: ``(loss[1], detached [lbox, lobj, lcls, loss])``."""
    flush_label_check()
    h = model.hyp
    cp, cn = smooth_bce(eps=float(h.get('label_smoothing', 0.0)))
    dev = p[0].device
    anchors = [layer.anchor_vec.to(device=dev, dtype=torch.float32).contiguous() for layer in yolo_modules(model)]
    meta = dict(targets=targets.to(device=dev, dtype=torch.float32).contiguous(), anchors=anchors, iou_t=float(h['iou_t']),
                gr=float(model.gr), cp=float(cp), cn=float(cn), cls_pw=float(h['cls_pw']),
                obj_pw=float(h['obj_pw']), giou=float(h['giou']), obj=float(h['obj']), cls=float(h['cls']),
                gamma=float(h.get('fl_gamma', 0.0)), alpha=FOCAL_ALPHA, box=box_kind(model),
                sxy=head_scales(model, yolo_modules))
    bases = _head_bases(p)
    with hiplib.on_device(p[0]):
        if bases is not None:
            meta['geom'] = [(na, no) for _, na, no in bases]
            loss, lbox, lobj, lcls = _YoloLoss.apply(meta, *[b for b, _, _ in bases])
        else:
            loss, lbox, lobj, lcls = _YoloLoss.apply(meta, *p)
    return loss.reshape(1), torch.stack((lbox, lobj, lcls, loss.detach())).detach()
