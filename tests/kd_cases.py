"""Shared cases of the distillation tests (tests/test_kd_losses.py, tests/test_gpu_kd.py) — TEST INFRASTRUCTURE ONLY.

A step is (student, teacher, batch, labels, mode).  ``mode``:
    'plain'    compute_loss alone                                     - the yardstick of every gradient comparison
    'feature'  the attention-transfer term alone (head gradients zero) - exercises nothing but the injection path
    'kd4'      compute_loss + compute_lost_KD4, as train.py --KDstr 4 adds them
``reference_step`` is fp64 autograd of the torch statements on the eager modules (CPU); ``engine_step`` runs the HIP training path
(``lib``: the host emulation on the CPU, None: the real library on a GPU) with the teacher's maps as ``AttentionMaps``.
"""
import copy
import os

import torch

import conftest
import synth
import train_harness as th
from engine import kd
from models import Darknet
from utils import utils as U

HYP = {'giou': 3.54, 'cls': 37.4, 'cls_pw': 1.0, 'obj': 64.3, 'obj_pw': 1.0, 'iou_t': 0.20, 'fl_gamma': 0.0}
TINY_HAND = os.path.join(conftest.PKG, 'cfg', 'yolov3tiny', 'yolov3-tiny-hand.cfg')
PRUNED_MINI = os.path.join(conftest.REPO, 'tests', 'golden', 'slim_prune_mini.cfg')
FEATURE_SCALE = 1.0      # the 'feature' step takes the un-weighted term (Lambda_feature = 0.001 stays in compute_lost_KD4)


def make_model(cfg, size, nc, seed):
    m = th.build(cfg, size, seed=seed)
    m.nc, m.gr, m.hyp = nc, 1.0, dict(HYP)
    return m


def labels(nc, batch=2):
    """A few labels, two of them in image 0, one class per image at least."""
    rows = [[0, 0, 0.30, 0.50, 0.25, 0.30], [0, nc - 1, 0.70, 0.30, 0.40, 0.20], [1, 0, 0.45, 0.55, 0.50, 0.60]]
    return torch.tensor([r for r in rows if r[0] < batch])


def eager_maps(model, x, dtype=torch.float32):
    """abs().sum(1) of the eager feature_out of ``model`` in train mode (no state is changed: a deep copy runs)."""
    m = copy.deepcopy(model).to(dtype).train()
    with torch.no_grad():
        feats = m._forward_eager(x.to(dtype))[1]
    return [f.abs().sum(1) for f in feats]


def as_attention_maps(maps, device):
    flat = torch.cat([a.float().reshape(-1) for a in maps]).to(device)
    return kd.AttentionMaps(flat, [tuple(a.shape) for a in maps])


def feature_statement(maps_s, maps_t, batch, T=3.0):
    """The feature term of compute_lost_KD4 on channel-summed maps, un-weighted."""
    crit = torch.nn.KLDivLoss(reduction='sum')
    total = 0
    for s, t in zip(maps_s, maps_t):
        s, t = s.reshape(s.size(0), -1), t.reshape(t.size(0), -1)
        total = total + crit(torch.log_softmax(s / T, 1), torch.softmax(t / T, 1)) * (T * T) / batch
    return total


def _loss(mode, model, targets, pred, feats_s, out_t, feats_t, batch):
    if mode == 'plain':
        return U.compute_loss(pred, targets, model, fused=False)[0].sum()
    if mode == 'feature':
        if kd.fusable(feats_s, feats_t):
            return kd.attention_kl(feats_s, feats_t, batch).sum() * FEATURE_SCALE
        return feature_statement([f if f.dim() == 3 else f.abs().sum(1) for f in feats_s], list(feats_t), batch) * FEATURE_SCALE
    if mode == 'kd4':
        return (U.compute_loss(pred, targets, model, fused=False)[0] + U.compute_lost_KD4(model, targets, pred, out_t, feats_s, feats_t, batch)).sum()
    raise ValueError(mode)


def teacher_outputs(teacher, x, dtype=torch.float32):
    """(raw heads, maps) of the teacher's eager modules in train mode (batch statistics), detached."""
    t = copy.deepcopy(teacher).to(dtype).train()
    with torch.no_grad():
        out_t, feats = t._forward_eager(x.to(dtype))
    return [o.detach() for o in out_t], [f.abs().sum(1) for f in feats]


def reference_step(student, teacher, x, targets, mode, dtype=torch.float64):
    """fp64 autograd of the torch statements on the eager modules.  Returns {parameter name: gradient (fp32)}."""
    m = copy.deepcopy(student).to(dtype).train()
    for p in m.parameters():
        p.grad = None
    pred, feats_s = m._forward_eager(x.to(dtype))
    out_t, maps_t = teacher_outputs(teacher, x, dtype)
    _loss(mode, m, targets, pred, feats_s, out_t, maps_t, x.shape[0]).backward()
    return {k: (p.grad.float() if p.grad is not None else torch.zeros_like(p).float()) for k, p in m.named_parameters()}


def engine_step(student, teacher, x, targets, mode, precision='fp32', lib=None, device='cpu', model=None, scale=1.0):
    """One step of the HIP training path.  ``model``: run on this (device) model instead of a fresh copy of ``student``.
    Returns (gradients by name (fp32, CPU), the model, the AttentionMaps or [])."""
    from engine.padded import make_train_engine
    m = model if model is not None else copy.deepcopy(student).to(device).train()
    for p in m.parameters():
        p.grad = None
    m.hip_return_features = False if mode == 'plain' else 'attention'
    out_t, maps_t = teacher_outputs(teacher, x)
    os.environ['YOLO_HIP_TRAIN_PRECISION'] = precision
    try:
        if lib is not None and m.__dict__.get('_hip_train_engine') is None:
            m.__dict__['_hip_train_engine'] = make_train_engine(m, precision, x.to(device), lib=lib)
        pred, feats_s = m._forward_hip_train(x.to(device))
        feats_t = as_attention_maps(maps_t, device) if mode != 'plain' else []
        loss = _loss(mode, m, targets.to(device), [p.float() for p in pred], feats_s, [o.to(device) for o in out_t], feats_t, x.shape[0])
        (loss * scale).backward()
    finally:
        del os.environ['YOLO_HIP_TRAIN_PRECISION']
    grads = {k: (p.grad.float().cpu() if p.grad is not None else torch.zeros_like(p).float().cpu()) for k, p in m.named_parameters()}
    return grads, m, feats_s


def distance(a, b):
    """Relative l2 distance of two gradient dicts over all parameters."""
    num = sum((a[k].double() - b[k].double()).pow(2).sum().item() for k in b)
    den = sum(b[k].double().pow(2).sum().item() for k in b)
    return (num / (den + 1e-300)) ** 0.5


def cosine(a, b):
    dot = sum((a[k].double() * b[k].double()).sum().item() for k in b)
    na = sum(a[k].double().pow(2).sum().item() for k in b) ** 0.5
    nb = sum(b[k].double().pow(2).sum().item() for k in b) ** 0.5
    return dot / (na * nb + 1e-300)


def pad_lanes(padded_engine, v):
    """Physical channels of twin value ``v`` that carry no channel of the live model (engine/padded.py layouts)."""
    lay = padded_engine.pad.layouts[v.block]
    assert lay.phys == v.c_phys
    real = set(lay.pos.tolist())
    return [c for c in range(lay.phys) if c not in real]
