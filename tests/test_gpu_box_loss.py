"""GPU tier of the DIoU / CIoU box loss and label smoothing on the fused loss kernels (csrc/loss.hip ``yh_yolo_loss_box_fwd`` / ``_bwd``
behind engine/loss.py, ``model.box_loss``, ``hyp['label_smoothing']``).

The comparison point is the package's torch statement (``utils.utils.compute_loss(..., fused=False)`` with the model's kind set) on the
CPU in fp64, as in tests/test_gpu_focal_loss.py: cells matched by several targets take the LAST target's objectness there, which
the kernels reproduce.  There is no reference run of a CIoU training loss to compare with - the reference's ``compute_loss``
hard-codes GIoU; the pin is ``bbox_iou``'s golden for all four flags (tests/test_boxutils_golden.py) plus the statement around it.
Bounds are ``focal_cases.assert_close_to``'s: loss items ``rtol 1e-5, atol 1e-6``, every head's gradient within 1e-4 of its largest
magnitude; the fp32 statement itself is within 2e-7 / 2.2e-7 of fp64 on these cases, so the bounds leave two orders of magnitude
for ``atanf`` and the reordered sums.  Every test prints its figures before it asserts."""
import copy
import ctypes as C
import functools
import os

import pytest
import torch

import box_cases as bc
import conftest
import fakelib_box
import focal_cases as fc
import synth
from engine import hiplib
from engine import loss as hip_loss
from engine.hiplib import LossDesc
from models import Darknet
from utils import utils as U

pytestmark = pytest.mark.gpu

GPU = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    hiplib.load()


_case = functools.lru_cache(maxsize=None)(bc.make_case)


@functools.lru_cache(maxsize=None)
def _reference(name, kind, gamma, eps=0.0, empty=False):
    """The fp64 torch statement on the CPU, computed once per setting and shared."""
    model, raws, targets = _case(name)
    return fc.torch_statement(raws, targets[:0] if empty else targets, bc.configure(model, kind, gamma, eps))


def _fused(name, kind, gamma, eps=0.0, empty=False):
    model, raws, targets = _case(name)
    bases, views = fc.nhwc_views(raws, GPU)
    hip_loss.flush_label_check()
    hip_loss.reset_stats()
    hip_loss.reset_box_stats()
    loss, items = U.compute_loss(views, (targets[:0] if empty else targets).to(GPU), bc.configure(model, kind, gamma, eps))
    (loss * 7.0).backward()
    torch.cuda.synchronize()
    hip_loss.flush_label_check()
    heads = len(raws)
    assert hip_loss.box_stats() == (dict(box_fwd=heads, box_bwd=heads) if kind != 'giou' else dict(box_fwd=0, box_bwd=0))
    assert hip_loss.stats() == (dict(focal_fwd=heads, focal_bwd=heads) if gamma > 0 else dict(focal_fwd=0, focal_bwd=0))
    for b, r in zip(bases, raws):
        assert b.grad[..., r.shape[1] * r.shape[4]:].abs().max().item() == 0, 'the channel padding of the head got a gradient'
    return items.cpu(), [b.grad.cpu() for b in bases]


def _report(what, items, grads, ref_items, ref_grads):
    rel = [((a.double() - b).abs().max() / b.abs().max()).item() for a, b in zip(grads, ref_grads)]
    irel = ((items.double() - ref_items.double()).abs() / ref_items.double().abs().clamp(min=1e-30)).max().item()
    print('%s: items %s (reference %s, largest relative distance %.2e), gradient distance / largest magnitude per head %s'
          % (what, [float(v) for v in items], [float(v) for v in ref_items], irel, ['%.2e' % v for v in rel]))


def test_cases_have_several_targets_in_one_cell():
    for name in bc.CASES:
        model, raws, targets = _case(name)
        _, _, indices, _ = U.build_targets(raws, targets, model)
        assert any(len(torch.unique(torch.stack(idx, 1), dim=0)) < len(idx[0]) for idx in indices), name


@pytest.mark.parametrize('gamma', [0.0, 1.5])
@pytest.mark.parametrize('kind', bc.KINDS)
@pytest.mark.parametrize('name', list(bc.CASES))
def test_box_kernels_match_the_fp64_torch_statement(name, kind, gamma):
    """Loss items and the gradient of every NHWC head tensor (strided views, padded last axis, loss scaled by 7) against fp64.
    Measured distances (items relative / gradient relative to the head's largest magnitude) are recorded in DESIGN.md 7j."""
    items, grads = _fused(name, kind, gamma)
    ref_items, ref_grads = _reference(name, kind, gamma)
    _report('%s %s gamma %g' % (name, kind, gamma), items, grads, ref_items, ref_grads)
    fc.assert_close_to(items, grads, ref_items, ref_grads, what=(name, kind, gamma))


@pytest.mark.parametrize('kind', bc.KINDS)
def test_label_smoothing_on_the_fused_path(kind):
    """eps 0.1 on ``coco80``: same comparison; the class term moves by more than 1 % against eps 0, the other two items do not move."""
    items, grads = _fused('coco80', kind, 0.0, eps=0.1)
    ref_items, ref_grads = _reference('coco80', kind, 0.0, eps=0.1)
    plain, _ = _reference('coco80', kind, 0.0)
    _report('coco80 %s eps 0.1' % kind, items, grads, ref_items, ref_grads)
    fc.assert_close_to(items, grads, ref_items, ref_grads, what=(kind, 'eps 0.1'))
    assert abs(items[2].item() - plain[2].item()) > 0.01 * plain[2].item(), (items, plain)
    assert torch.allclose(items[:2].double(), plain[:2].double(), rtol=1e-5, atol=1e-6)


def test_the_kind_reaches_the_kernel():
    """``lbox`` of the three kinds on ``coco80`` differs pairwise by more than 1 % (9.59 / 8.81 / 9.04 on the CPU statement)."""
    lbox = {kind: _fused('coco80', kind, 0.0)[0][0].item() for kind in bc.KINDS}
    print('coco80 lbox per kind: %s' % lbox)
    for a, b in (('giou', 'diou'), ('giou', 'ciou'), ('diou', 'ciou')):
        assert abs(lbox[a] - lbox[b]) > 0.01 * max(lbox[a], lbox[b]), lbox


class _GiouThroughTheBoxEntries:
    """The library with its default entries served by ``yh_yolo_loss_box_*`` at ``YH_BOX_GIOU`` (the glue itself never does that)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def yh_yolo_loss_fwd(self, d, stream):
        self.calls += 1
        return self._lib.yh_yolo_loss_box_fwd(d, 0, 0.0, 0.0, stream)

    def yh_yolo_loss_bwd(self, d, stream):
        self.calls += 1
        return self._lib.yh_yolo_loss_box_bwd(d, 0, 0.0, 0.0, stream)

    def yh_yolo_loss_focal_fwd(self, d, gamma, alpha, stream):
        self.calls += 1
        return self._lib.yh_yolo_loss_box_fwd(d, 0, gamma, alpha, stream)

    def yh_yolo_loss_focal_bwd(self, d, gamma, alpha, stream):
        self.calls += 1
        return self._lib.yh_yolo_loss_box_bwd(d, 0, gamma, alpha, stream)


@pytest.mark.parametrize('gamma', [0.0, 1.5])
def test_giou_through_the_new_entries_is_the_existing_loss(gamma):
    """``box == YH_BOX_GIOU`` through ``yh_yolo_loss_box_*`` against the existing entries, within run-to-run bounds (the sums use float
    atomics: no bit equality), and against the fp64 statement."""
    old = _fused('coco80', 'giou', gamma)
    proxy = _GiouThroughTheBoxEntries(hiplib.load())
    hip_loss._LIB_OVERRIDE = proxy
    try:
        new = _fused('coco80', 'giou', gamma)
    finally:
        hip_loss._LIB_OVERRIDE = None
    assert proxy.calls == 6
    _report('coco80 giou gamma %g, box entries against the existing ones' % gamma, new[0], new[1], old[0], [g.double() for g in old[1]])
    fc.assert_close_to(new[0], new[1], old[0], old[1], what='giou, new entry against old')
    ref_items, ref_grads = _reference('coco80', 'giou', gamma)
    fc.assert_close_to(new[0], new[1], ref_items, ref_grads, what='giou through the box entries')


@pytest.mark.parametrize('kind', bc.KINDS)
def test_exact_match_is_finite_and_follows_the_closed_form(kind):
    """The hand-made head of tests/box_cases.py ``exact_match`` - one matched candidate equal to its label - through the ABI directly:
    value and gradient are finite and equal the fp32 closed form (tests/fakelib_box.py ``box_term``: CIoU takes ``alpha = 0`` there,
    where the torch statement is nan) to ``rtol 1e-5``."""
    lib = hiplib.load()
    raw, anchors, targets, (b, a, gy, gx) = bc.exact_match()
    box = fakelib_box.KINDS[kind]
    gr, g_box, scale_v = 0.75, 3.54, 7.0
    p = raw.to(GPU).contiguous()
    dev = lambda t: t.to(GPU).contiguous()
    anc, tg = dev(anchors), dev(targets)
    tobj = torch.zeros(1, 1, 4, 4, device=GPU)
    winner = torch.full((1, 1, 4, 4), -1, device=GPU, dtype=torch.int32)
    sums = torch.zeros(3, device=GPU)
    count = torch.zeros(2, device=GPU, dtype=torch.int32)
    grad = torch.full_like(p, float('nan'))
    scale = torch.tensor([scale_v], device=GPU)
    d = LossDesc(p=hiplib.ptr(p), grad=hiplib.ptr(grad), tobj=hiplib.ptr(tobj), winner=hiplib.ptr(winner), targets=hiplib.ptr(tg),
                 anchors=hiplib.ptr(anc), sums=hiplib.ptr(sums), count=hiplib.ptr(count), scale=hiplib.ptr(scale),
                 sb=p.stride(0), sa=p.stride(1), sy=p.stride(2), sx=p.stride(3), gb=grad.stride(0), ga=grad.stride(1), gy=grad.stride(2),
                 gx=grad.stride(3), bs=1, na=1, ny=4, nx=4, no=6, nc=1, nt=1, iou_t=0.2, gr=gr, cp=1.0, cn=0.0, cls_pw=1.0, obj_pw=1.0,
                 g_box=g_box, g_obj=64.3, g_cls=37.4)
    with hiplib.on_device(p):
        assert lib.yh_yolo_loss_box_fwd(C.byref(d), box, 0.0, 0.0, hiplib.stream_ptr()) == 0
        assert lib.yh_yolo_loss_box_bwd(C.byref(d), box, 0.0, 0.0, hiplib.stream_ptr()) == 0
    torch.cuda.synchronize()
    val, dval = fakelib_box.box_term(kind, raw[b, a, gy, gx, :4][None], anchors, torch.tensor([[0.5, 0.5, 2.0, 3.0]]))
    assert val.dtype == torch.float32 and val.item() == 1.0 and torch.isfinite(dval).all()
    got = grad[b, a, gy, gx, :4].cpu()
    want = -(torch.tensor(scale_v) * g_box / 1.0) * dval[0]
    print('exact match %s: lbox sum %r, tobj %r, box gradient %s, closed form %s'
          % (kind, sums[0].item(), tobj[b, a, gy, gx].item(), got.tolist(), want.tolist()))
    assert count.tolist() == [1, 0]
    assert torch.isfinite(sums).all() and torch.isfinite(grad).all() and torch.isfinite(tobj).all()
    torch.testing.assert_close(1.0 - sums[0].cpu(), val[0], rtol=1e-5, atol=0)          # the measure: lbox sums 1 - measure
    torch.testing.assert_close(tobj[b, a, gy, gx].cpu(), (1.0 - gr) + gr * val[0].clamp(min=0), rtol=1e-5, atol=0)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=0)
    # GIoU's hull term cancels iou's derivative at an exact match (every min / max picks the prediction); DIoU and CIoU keep it
    assert kind == 'giou' or want.abs().max() > 0


@pytest.mark.parametrize('kind', ['diou', 'ciou'])
def test_box_kernels_without_labels(kind):
    items, grads = _fused('coco80', kind, 0.0, empty=True)
    ref_items, ref_grads = _reference('coco80', kind, 0.0, empty=True)
    _report('coco80 %s no labels' % kind, items, grads, ref_items, ref_grads)
    assert items[0] == 0 and items[2] == 0 and items[1] > 0
    fc.assert_close_to(items, grads, ref_items, ref_grads, what=('empty', kind))


def _step_gradient(model, x, targets, kind, fused=None):
    """Parameter gradients of one training step on the HIP step (fp32) with ``compute_loss`` at box kind ``kind``."""
    dev = copy.deepcopy(model).to(GPU)
    dev.hyp, dev.box_loss = dict(model.hyp), kind
    pred, _ = dev(x.to(GPU))
    loss, _ = U.compute_loss(pred, targets.to(GPU), dev, fused=fused)
    loss.backward()
    torch.cuda.synchronize()
    hip_loss.flush_label_check()
    assert dev.__dict__.get('_hip_train_engine') is not None, 'the HIP training path did not engage'
    return [p.grad.double().cpu() for p in dev.parameters()]


def _rel_l2(a, b):
    num = sum(float((u - v).pow(2).sum()) for u, v in zip(a, b))
    den = sum(float(v.pow(2).sum()) for v in b)
    return (num / den) ** 0.5


def test_training_step_with_ciou(monkeypatch):
    """yolov3-tiny-hand, 64 px, batch 2, ``model.train()`` on the HIP step (the setup of test_training_step_with_focal_loss): the
    parameter gradients with the fused CIoU loss against those with the torch statement (``YOLO_HIP_BOX_LOSS=0``) on the same
    device.  Yardstick: the same distance at GIoU between the existing fused kernels and ``compute_loss(..., fused=False)`` - the
    parent commit's code on both sides; the CIoU distance may be three times that.  No two labels share a cell, so torch's
    ``index_put`` on the GPU has no choice to make."""
    monkeypatch.setenv('YOLO_HIP_TRAIN_PRECISION', 'fp32')
    torch.manual_seed(0)
    model = Darknet(os.path.join(conftest.PKG, 'cfg', 'yolov3tiny', 'yolov3-tiny-hand.cfg'), (64, 64)).train()
    model.nc, model.gr, model.hyp = 1, 1.0, dict(fc.HYP, cls_pw=1.0, obj_pw=1.0)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 64, 64, generator=g)
    targets = torch.tensor([[0, 0, 0.2, 0.2, 0.3, 0.35], [0, 0, 0.7, 0.7, 0.4, 0.3], [1, 0, 0.3, 0.7, 0.25, 0.3], [1, 0, 0.8, 0.2, 0.3, 0.5]])
    shapes = [torch.zeros(2, 3, 64 // s, 64 // s, 6) for s in (32, 16)]
    _, _, indices, _ = U.build_targets(shapes, targets, model)
    for idx in indices:
        cells = torch.stack(idx, 1)
        assert len(cells) and len(torch.unique(cells, dim=0)) == len(cells)
    hip_loss.reset_stats()
    hip_loss.reset_box_stats()
    giou_fused = _step_gradient(model, x, targets, 'giou')
    giou_torch = _step_gradient(model, x, targets, 'giou', fused=False)
    assert hip_loss.box_stats() == dict(box_fwd=0, box_bwd=0)
    ciou_fused = _step_gradient(model, x, targets, 'ciou')
    assert hip_loss.box_stats() == dict(box_fwd=2, box_bwd=2)
    monkeypatch.setenv('YOLO_HIP_BOX_LOSS', '0')
    ciou_torch = _step_gradient(model, x, targets, 'ciou')
    assert hip_loss.box_stats() == dict(box_fwd=2, box_bwd=2) and hip_loss.stats() == dict(focal_fwd=0, focal_bwd=0)
    yard, dist = _rel_l2(giou_fused, giou_torch), _rel_l2(ciou_fused, ciou_torch)
    moved = _rel_l2(ciou_fused, giou_fused)
    print('training step, relative l2 distance of the whole gradient: fused CIoU against the torch statement %.3e; '
          'yardstick (GIoU, fused against torch) %.3e; CIoU against GIoU %.3e' % (dist, yard, moved))
    assert all(torch.isfinite(v).all() for v in ciou_fused)
    assert moved > 0.05, 'the box kind did not reach the loss'
    assert dist <= 3 * yard, (dist, yard)


def test_ciou_defers_the_label_check_without_a_host_sync():
    """A class >= nc with ``box_loss='ciou'``: the launch does not raise, the next call raises the reference's AssertionError, a clean
    batch afterwards is unaffected (mirrors test_focal_loss_defers_the_label_check_without_a_host_sync)."""
    torch.manual_seed(0)
    model = Darknet(os.path.join(conftest.PKG, 'cfg', 'yolov3tiny/yolov3-tiny-hand.cfg'), (128, 128))
    model.nc, model.gr, model.hyp, model.box_loss = 1, 1.0, dict(fc.HYP), 'ciou'
    raws, targets = synth.loss_inputs(model, 128, batch=2, seed=3)
    dev_raws = [r.to(GPU) for r in raws]
    bad = targets.clone()
    bad[:, 1] = 1.0
    hip_loss.flush_label_check()
    hip_loss.reset_box_stats()
    U.compute_loss(dev_raws, bad.to(GPU), model)                      # launches, does not raise
    with pytest.raises(AssertionError):
        U.compute_loss(dev_raws, targets.to(GPU), model)              # the next call reports it
    loss, items = U.compute_loss(dev_raws, targets.to(GPU), model)    # a clean batch afterwards is unaffected
    hip_loss.flush_label_check()
    assert hip_loss.box_stats()['box_fwd'] == 4
    _, ref_items = U.compute_loss([r.double() for r in raws], targets, model, fused=False)
    assert torch.allclose(items.cpu().double(), ref_items.double(), rtol=1e-5, atol=1e-6), (items, ref_items)
