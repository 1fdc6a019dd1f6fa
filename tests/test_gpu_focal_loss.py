"""GPU tier of focal loss on the fused loss kernels (csrc/loss.hip ``yh_yolo_loss_focal_fwd`` / ``_bwd`` behind engine/loss.py).

The comparison point is the package's torch statement (``utils.utils.compute_loss(..., fused=False)``) on the CPU, as in
``test_fused_loss_kernels_match_torch_loss``: cells matched by several targets take the LAST target's objectness there, which the
kernels reproduce and torch's ``index_put`` on a GPU does not.  Here the statement runs in fp64 (the raw heads and everything derived
from them; the labels and the target assignment stay fp32, and ``compute_loss`` adds the three heads' means into an fp32 scalar), so
the distance measured is the kernels' own error.  Bounds are that test's: loss items ``rtol 1e-5, atol 1e-6``, every head's gradient
within 1e-4 of its largest magnitude.  Every test prints its figures before it asserts."""
import copy
import functools
import os

import pytest
import torch

import conftest
import focal_cases as fc
import synth
from engine import hiplib
from engine import loss as hip_loss
from models import Darknet
from utils import utils as U

pytestmark = pytest.mark.gpu

GPU = 'cuda'
# the smallest shapes that reach every branch: no class term and several workgroups on the objectness pass (960 cells); three heads
# with the class term; a gradient row wider than one workgroup pass (3 * 96 = 288 > 256); and a head of more grid positions than the
# dense backward has workgroups (12 * 38 * 38 = 17 328 > 16 384), where a workgroup stages the focal derivative of several positions
CASES = {'hand1': ('yolov3tiny/yolov3-tiny-hand.cfg', 128, 1, 4), 'coco80': ('yolov3/yolov3.cfg', 96, 80, 2),
         'wide91': ('yolov3tiny/yolov3-tiny-hand.cfg', 128, 91, 2), 'hand1_17k': ('yolov3tiny/yolov3-tiny-hand.cfg', 608, 1, 12)}


@pytest.fixture(scope='module', autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    hiplib.load()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, raw heads, labels) of a case: seeded, 12 labels per image so that several targets share a cell."""
    rel, size, nc, batch = CASES[name]
    torch.manual_seed(0)
    path = os.path.join(conftest.PKG, 'cfg', rel)
    if nc == 91:
        import tempfile
        text = open(path).read().replace('classes=1', 'classes=91').replace('filters=18', 'filters=288')
        with tempfile.NamedTemporaryFile('w', suffix='.cfg', delete=False) as f:
            f.write(text)
        try:
            model = Darknet(f.name, (size, size))
        finally:
            os.unlink(f.name)
    else:
        model = Darknet(path, (size, size))
    model.nc, model.gr = nc, 0.6
    model.hyp = dict(fc.HYP)
    raws, targets = synth.loss_inputs(model, size, batch=batch, seed=33, labels_per_image=12)
    return model, raws, targets


def _with_gamma(model, gamma):
    model.hyp = dict(model.hyp, fl_gamma=gamma)      # the cached model: every use sets its gamma
    return model


@functools.lru_cache(maxsize=None)
def _reference(name, gamma, saturated=False, closed=False, empty=False):
    """The fp64 torch statement on the CPU, computed once per (case, gamma) and shared."""
    model, raws, targets = _case(name)
    if saturated:
        raws = fc.saturate(raws, seed=5)
    return fc.torch_statement(raws, targets[:0] if empty else targets, _with_gamma(model, gamma), closed=closed)


def _fused(name, gamma, saturated=False, empty=False):
    model, raws, targets = _case(name)
    if saturated:
        raws = fc.saturate(raws, seed=5)
    bases, views = fc.nhwc_views(raws, GPU)
    hip_loss.flush_label_check()
    hip_loss.reset_stats()
    loss, items = U.compute_loss(views, (targets[:0] if empty else targets).to(GPU), _with_gamma(model, gamma))
    (loss * 7.0).backward()
    torch.cuda.synchronize()
    hip_loss.flush_label_check()
    heads = len(raws)
    want = dict(focal_fwd=heads, focal_bwd=heads) if gamma > 0 else dict(focal_fwd=0, focal_bwd=0)
    assert hip_loss.stats() == want
    for b, r in zip(bases, raws):
        assert b.grad[..., r.shape[1] * r.shape[4]:].abs().max().item() == 0, 'the channel padding of the head got a gradient'
    return items.cpu(), [b.grad.cpu() for b in bases]


def _report(what, items, grads, ref_items, ref_grads):
    rel = [((a.double() - b).abs().max() / b.abs().max()).item() for a, b in zip(grads, ref_grads)]
    print('%s: items %s (reference %s), gradient distance / largest magnitude per head %s'
          % (what, [float(v) for v in items], [float(v) for v in ref_items], ['%.2e' % v for v in rel]))


def test_cases_have_several_targets_in_one_cell():
    for name in CASES:
        model, raws, targets = _case(name)
        _, _, indices, _ = U.build_targets(raws, targets, model)
        assert any(len(torch.unique(torch.stack(idx, 1), dim=0)) < len(idx[0]) for idx in indices), name


@pytest.mark.parametrize('gamma', fc.GAMMAS)
@pytest.mark.parametrize('name', list(CASES))
def test_focal_kernels_match_the_fp64_torch_statement(name, gamma):
    """Loss items and the gradient of every NHWC head tensor (strided views, padded last axis, loss scaled by 7) against fp64."""
    items, grads = _fused(name, gamma)
    ref_items, ref_grads = _reference(name, gamma)
    _report('%s gamma %g' % (name, gamma), items, grads, ref_items, ref_grads)
    fc.assert_close_to(items, grads, ref_items, ref_grads, what=(name, gamma))


@pytest.mark.parametrize('gamma', [0.5, 1.5])
def test_focal_kernels_without_labels(gamma):
    items, grads = _fused('coco80', gamma, empty=True)
    ref_items, ref_grads = _reference('coco80', gamma, empty=True)
    _report('coco80 no labels gamma %g' % gamma, items, grads, ref_items, ref_grads)
    assert items[0] == 0 and items[2] == 0 and items[1] > 0
    fc.assert_close_to(items, grads, ref_items, ref_grads, what=('empty', gamma))


@pytest.mark.parametrize('gamma', fc.GAMMAS)
@pytest.mark.parametrize('name', list(CASES))
def test_saturated_logits_stay_finite_and_follow_the_formula(name, gamma):
    """2 % of the objectness and class logits replaced by values in +-[17, 60]: fp32 rounds ``1 - p_t`` of such an element to 0 or
    loses most of its bits.  gamma >= 1: same bounds against the fp64 statement.  gamma = 0.5: autograd's ``pow`` backward is not
    finite where fp64 rounds ``1 - p_t`` to 0 (|x| > 36.7), so the reference is the closed form with the ``q <= 0`` rule in fp64
    (fakelib_focal.focal_elem, checked against autograd on the CPU tier); every output of the kernels must be finite."""
    items, grads = _fused(name, gamma, saturated=True)
    ref_items, ref_grads = _reference(name, gamma, saturated=True, closed=gamma < 1)
    assert torch.isfinite(ref_items).all() and all(torch.isfinite(g).all() for g in ref_grads)
    _report('%s saturated gamma %g' % (name, gamma), items, grads, ref_items, ref_grads)
    fc.assert_close_to(items, grads, ref_items, ref_grads, what=(name, gamma, 'saturated'))


def _step_gradient(model, x, targets, gamma, fused=None):
    """Parameter gradients of one training step on the HIP step (fp32) with ``compute_loss`` at ``gamma``."""
    dev = copy.deepcopy(model).to(GPU)
    dev.hyp = dict(model.hyp, fl_gamma=gamma)
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


def test_training_step_with_focal_loss(monkeypatch):
    """yolov3-tiny-hand, 64 px, batch 2, ``model.train()`` on the HIP step: the parameter gradients with the fused focal loss against
    those with the torch statement (``YOLO_HIP_FOCAL_LOSS=0``) on the same device.  Yardstick: the same distance between the existing
    fused kernels and ``compute_loss(..., fused=False)`` at gamma 0 on the same inputs - the parent commit's code on both sides; the
    focal distance may be three times that.  No two labels share a cell, so torch's ``index_put`` on the GPU has no choice to make."""
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
    plain_fused = _step_gradient(model, x, targets, 0.0)
    plain_torch = _step_gradient(model, x, targets, 0.0, fused=False)
    assert hip_loss.stats() == dict(focal_fwd=0, focal_bwd=0)
    focal_fused = _step_gradient(model, x, targets, 1.5)
    assert hip_loss.stats() == dict(focal_fwd=2, focal_bwd=2)
    monkeypatch.setenv('YOLO_HIP_FOCAL_LOSS', '0')
    focal_torch = _step_gradient(model, x, targets, 1.5)
    assert hip_loss.stats() == dict(focal_fwd=2, focal_bwd=2)
    yard, dist = _rel_l2(plain_fused, plain_torch), _rel_l2(focal_fused, focal_torch)
    print('training step, relative l2 distance of the whole gradient: fused focal against the torch statement %.3e; '
          'yardstick (gamma 0, fused against torch) %.3e' % (dist, yard))
    assert all(torch.isfinite(v).all() for v in focal_fused)
    assert _rel_l2(focal_fused, plain_fused) > 0.05, 'gamma did not reach the loss'
    assert dist <= 3 * yard, (dist, yard)


def test_focal_loss_defers_the_label_check_without_a_host_sync():
    """A class >= nc with gamma 1.5: the launch does not raise, the next call raises the reference's AssertionError, a clean batch
    afterwards is unaffected (mirrors test_fused_loss_defers_the_label_check_without_a_host_sync)."""
    torch.manual_seed(0)
    model = Darknet(os.path.join(conftest.PKG, 'cfg', 'yolov3tiny/yolov3-tiny-hand.cfg'), (128, 128))
    model.nc, model.gr, model.hyp = 1, 1.0, dict(fc.HYP, fl_gamma=1.5)
    raws, targets = synth.loss_inputs(model, 128, batch=2, seed=3)
    dev_raws = [r.to(GPU) for r in raws]
    bad = targets.clone()
    bad[:, 1] = 1.0
    hip_loss.flush_label_check()
    hip_loss.reset_stats()
    U.compute_loss(dev_raws, bad.to(GPU), model)                      # launches, does not raise
    with pytest.raises(AssertionError):
        U.compute_loss(dev_raws, targets.to(GPU), model)              # the next call reports it
    loss, items = U.compute_loss(dev_raws, targets.to(GPU), model)    # a clean batch afterwards is unaffected
    hip_loss.flush_label_check()
    assert hip_loss.stats()['focal_fwd'] == 4
    _, ref_items = U.compute_loss([r.double() for r in raws], targets, model, fused=False)
    assert torch.allclose(items.cpu().double(), ref_items.double(), rtol=1e-5, atol=1e-6), (items, ref_items)


def test_gamma_zero_is_the_existing_path():
    """gamma 0: the focal entries are not called, and items and gradients equal a second run of the same call within the existing
    test's bounds (the sums use float atomics: no bit equality)."""
    first = _fused('coco80', 0.0)
    second = _fused('coco80', 0.0)
    fc.assert_close_to(first[0], first[1], second[0], second[1], what='gamma 0, run to run')
    ref_items, ref_grads = _reference('coco80', 0.0)
    fc.assert_close_to(first[0], first[1], ref_items, ref_grads, what='gamma 0')
