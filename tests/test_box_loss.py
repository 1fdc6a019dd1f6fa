"""CPU tier of the DIoU / CIoU box loss and label smoothing on the fused loss kernels (``model.box_loss``, ``hyp['label_smoothing']``:
csrc/loss.hip ``yh_yolo_loss_box_fwd`` / ``_bwd`` behind engine/loss.py): the emulation's closed form against ``utils.bbox_iou`` under
autograd in fp64, the ``alpha`` rule, the autograd node on the host emulation (tests/fakelib_box.py) against the torch statement,
the C ABI and its argument checks on the real library, and ``train.py --box-loss / --label-smoothing``.  The kernels themselves are
checked on the GPU tier (tests/test_gpu_box_loss.py).

There is no reference run of a CIoU training loss to compare with - the reference's ``compute_loss`` hard-codes GIoU.  The pin is
``bbox_iou``'s golden for all four flags (tests/test_boxutils_golden.py) plus the package's torch statement around it."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import box_cases as bc
import conftest
import fakelib_box
import focal_cases as fc
from engine import hiplib
from engine import loss as hip_loss
from engine.hiplib import LossDesc
from utils import utils as U
from utils.parse_config import parse_model_cfg

HEADER = os.path.join(conftest.REPO, 'include', 'yolo_hip.h')


@pytest.fixture
def fake():
    lib = fakelib_box.FakeLibBox()
    hip_loss._LIB_OVERRIDE = lib
    hip_loss.reset_stats()
    hip_loss.reset_box_stats()
    try:
        yield lib
    finally:
        hip_loss._LIB_OVERRIDE = None


@pytest.mark.parametrize('kind', bc.KINDS)
def test_closed_form_equals_bbox_iou_autograd_in_fp64(kind):
    """``fakelib_box.box_term`` - the kernel's forward-mode chain, value and four derivatives - against ``utils.bbox_iou`` under autograd,
    candidate for candidate in fp64; bounds of the focal closed-form test.  Every candidate keeps ``1 - iou + v`` and
    ``|atan(w2 / h2) - atan(w1 / h1)|`` above 1e-3 (asserted: the seed was picked so that none has to be left out), so no
    cancellation in ``alpha`` or ``v`` costs more than ten of fp64's 53 bits.  The hand-made candidates at the end: boxes that do
    not overlap, a label inside the prediction, a width logit above ln 1000."""
    logits, anchors, tbox = bc.candidates(512, seed=11)
    iou, den, da = bc.margins(logits, anchors, tbox)
    assert den.min() >= 1e-3 and da.min() >= 1e-3, (den.min(), da.min())
    assert iou[-3] == 0 and logits[-1, 2] > math.log(1e3)
    box = bc.decode(logits[-2:-1], anchors[-2:-1])[:, 0]
    t = tbox[-2]
    assert box[0] - box[2] / 2 < t[0] - t[2] / 2 and box[0] + box[2] / 2 > t[0] + t[2] / 2
    assert box[1] - box[3] / 2 < t[1] - t[3] / 2 and box[1] + box[3] / 2 > t[1] + t[3] / 2
    xr = logits.clone().requires_grad_()
    want = U.bbox_iou(bc.decode(xr, anchors), tbox, x1y1x2y2=False, **{U.BOX_LOSSES[kind]: True})
    want.sum().backward()
    got, dgot = fakelib_box.box_term(kind, logits, anchors, tbox)
    assert got.dtype == torch.float64 and torch.isfinite(want).all() and torch.isfinite(xr.grad).all()
    np.testing.assert_allclose(got.numpy(), want.detach().numpy(), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(dgot.numpy(), xr.grad.numpy(), rtol=1e-9, atol=1e-13)
    assert dgot[-1, 2] == 0 and xr.grad[-1, 2] == 0, 'clamp(max=1e3) cuts the width gradient'
    assert dgot.abs().max() > 0.01


def test_the_three_kinds_are_three_measures():
    logits, anchors, tbox = bc.candidates(64, seed=11)
    vals = [fakelib_box.box_term(k, logits, anchors, tbox)[0] for k in bc.KINDS]
    assert (vals[0] - vals[1]).abs().max() > 0.01 and (vals[1] - vals[2]).abs().max() > 0.01
    assert (vals[2] <= vals[1]).all()            # CIoU = DIoU - v * alpha


def test_exact_match_takes_alpha_zero_where_the_statement_is_nan():
    """The ``alpha`` rule on a hand-made exact match (tests/box_cases.py ``exact_match``: dyadic anchor and label, zero logits).  fp32:
    ``iou == 1`` and ``v == 0``, so the statement's ``alpha = v / (1 - iou + v)`` is 0 / 0 and ``bbox_iou`` returns nan; the closed form
    takes ``alpha = 0``, the limit of ``v * alpha``: value 1, derivative finite.  This is the documented, deliberate difference
    between the kernels and the torch statement."""
    raw, anchors, targets, (b, a, gy, gx) = bc.exact_match()
    logits = raw[b, a, gy, gx, :4][None]
    tbox = torch.tensor([[0.5, 0.5, 2.0, 3.0]])
    val, dval = fakelib_box.box_term('ciou', logits, anchors, tbox)
    assert val.dtype == torch.float32 and val.item() == 1.0
    assert torch.isfinite(dval).all()
    stmt = U.bbox_iou(bc.decode(logits, anchors), tbox, x1y1x2y2=False, CIoU=True)
    assert torch.isnan(stmt).all()
    assert torch.isnan(U.bbox_iou(torch.tensor([0.5, 0.5, 2.0, 3.0]), torch.tensor([[0.5, 0.5, 2.0, 3.0]]), x1y1x2y2=False, CIoU=True)).all()
    for kind in ('giou', 'diou'):
        assert fakelib_box.box_term(kind, logits, anchors, tbox)[0].item() == 1.0
    # a NaN logit is not hidden by the rule
    bad = logits.clone()
    bad[0, 2] = float('nan')
    assert torch.isnan(fakelib_box.box_term('ciou', bad, anchors, tbox)[0]).all()


def _checks(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), t.abs().max().item()])


@functools.lru_cache(maxsize=None)
def _case():
    return bc.make_case('coco80')


def _glue(model, raws, targets, scale=3.0):
    bases, views = fc.nhwc_views(raws, 'cpu')
    loss, items = U.compute_loss(views, targets, model)
    (loss * scale).backward()
    return items, bases


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('gamma', [0.0, 1.5])
@pytest.mark.parametrize('kind', ['diou', 'ciou'])
def test_fused_box_glue_matches_the_torch_statement(fake, kind, gamma, eps):
    """engine/loss.py on the emulated box entries, through padded NHWC bases, against the fp32 torch statement on the CPU
    (tolerances of test_fused_focal_glue_matches_reference_goldens); the counters show that the box entries ran - once per head and
    pass - with the kind, gamma and FocalLoss's alpha, and ``stats()`` keeps its two keys and keeps counting focal calls."""
    model, raws, targets = _case()
    bc.configure(model, kind, gamma, eps)
    items, bases = _glue(model, raws, targets)
    nh = len(raws)
    assert hip_loss.box_stats() == dict(box_fwd=nh, box_bwd=nh) and fake.box_calls == dict(fwd=nh, bwd=nh)
    assert hip_loss.stats() == (dict(focal_fwd=nh, focal_bwd=nh) if gamma > 0 else dict(focal_fwd=0, focal_bwd=0))
    assert fake.focal_calls == dict(fwd=0, bwd=0)
    assert fake.box_args == [(fakelib_box.KINDS[kind], gamma, 0.25)] * (2 * nh)
    ref_items, ref_grads = fc.torch_statement(raws, targets, model, dtype=torch.float32, scale=3.0)
    assert hip_loss.box_stats() == dict(box_fwd=nh, box_bwd=nh), 'fused=False went to the entries'
    np.testing.assert_allclose(items.numpy(), ref_items.numpy(), rtol=3e-6)
    for base, ref, r in zip(bases, ref_grads, raws):
        assert base.grad[..., r.shape[1] * r.shape[4]:].abs().max() == 0
        np.testing.assert_allclose(base.grad.reshape(-1)[::97].numpy(), ref.reshape(-1)[::97].numpy(), rtol=2e-5, atol=1e-9)
        np.testing.assert_allclose(_checks(base.grad), _checks(ref), rtol=2e-5)


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('gamma', [0.0, 1.5])
def test_giou_keeps_the_existing_entries(fake, gamma, eps, monkeypatch):
    """GIoU, with or without smoothing: ``yh_yolo_loss_fwd`` / ``_bwd`` at gamma 0 and the focal entries at gamma > 0, as before; smoothing
    only changes ``cp`` / ``cn`` of the descriptor."""
    model, raws, targets = _case()
    bc.configure(model, 'giou', gamma, eps)
    seen = []
    monkeypatch.setattr(fake, 'yh_yolo_loss_fwd', lambda d, s, f=fake.yh_yolo_loss_fwd: (seen.append((d._obj.cp, d._obj.cn)), f(d, s))[1])
    items, bases = _glue(model, raws, targets)
    nh = len(raws)
    assert hip_loss.box_stats() == dict(box_fwd=0, box_bwd=0) and fake.box_calls == dict(fwd=0, bwd=0)
    assert set(hip_loss.stats()) == {'focal_fwd', 'focal_bwd'}
    if gamma > 0:
        assert hip_loss.stats() == dict(focal_fwd=nh, focal_bwd=nh) and fake.focal_calls == dict(fwd=nh, bwd=nh) and not seen
    else:
        assert hip_loss.stats() == dict(focal_fwd=0, focal_bwd=0) and fake.focal_calls == dict(fwd=0, bwd=0)
        assert len(seen) == nh and all(abs(cp - (1 - eps / 2)) < 1e-7 and abs(cn - eps / 2) < 1e-7 for cp, cn in seen)
    ref_items, _ = fc.torch_statement(raws, targets, model, dtype=torch.float32, scale=3.0)
    np.testing.assert_allclose(items.numpy(), ref_items.numpy(), rtol=3e-6)


def test_a_model_without_the_attribute_and_a_hyp_without_the_key_behave_as_before(fake):
    model, raws, targets = _case()
    bc.configure(model, 'giou')
    want, _ = _glue(model, raws, targets)
    del model.box_loss
    model.hyp = {k: v for k, v in model.hyp.items() if k != 'label_smoothing'}
    got, _ = _glue(model, raws, targets)
    stmt, _ = fc.torch_statement(raws, targets, model, dtype=torch.float32)
    assert torch.equal(got, want) and hip_loss.box_stats() == dict(box_fwd=0, box_bwd=0)
    np.testing.assert_allclose(got.numpy(), stmt.numpy(), rtol=3e-6)


def test_label_smoothing_moves_the_class_term_only(fake):
    model, raws, targets = _case()
    plain, _ = _glue(bc.configure(model, 'ciou', 0.0, 0.0), raws, targets)
    smooth, _ = _glue(bc.configure(model, 'ciou', 0.0, 0.1), raws, targets)
    assert plain[0] == smooth[0] and plain[1] == smooth[1]
    assert abs(smooth[2] - plain[2]) > 0.01 * plain[2]


def test_env_switch_keeps_the_torch_statement(fake, monkeypatch):
    monkeypatch.setenv('YOLO_HIP_BOX_LOSS', '0')
    model, raws, targets = _case()
    items, _ = _glue(bc.configure(model, 'ciou', 0.0, 0.1), raws, targets)
    assert hip_loss.box_stats() == dict(box_fwd=0, box_bwd=0) and fake.box_calls == dict(fwd=0, bwd=0)
    ref_items, _ = fc.torch_statement(raws, targets, model, dtype=torch.float32)
    assert torch.equal(items, ref_items)
    # the switch is about DIoU / CIoU only: the default loss stays on the fused entries
    seen = []
    monkeypatch.setattr(fake, 'yh_yolo_loss_fwd', lambda d, s, f=fake.yh_yolo_loss_fwd: (seen.append(1), f(d, s))[1])
    _glue(bc.configure(model, 'giou', 0.0, 0.1), raws, targets)
    assert len(seen) == len(raws)


@pytest.mark.parametrize('fused', [None, False])
def test_an_unknown_kind_raises_a_value_error_that_names_it(fake, fused):
    model, raws, targets = _case()
    bc.configure(model, 'mse')
    try:
        with pytest.raises(ValueError, match='mse'):
            U.compute_loss(raws, targets, model, fused=fused)
    finally:
        bc.configure(model)


def _desc(keep):
    """A descriptor that passes check_loss for both passes (host memory: the entries must return before any launch)."""
    buf = lambda n, dt=np.float32: keep.append(np.zeros(n, dt)) or keep[-1].ctypes.data
    return LossDesc(p=buf(2 * 3 * 4 * 4 * 6), grad=buf(2 * 3 * 4 * 4 * 6), tobj=buf(96), winner=buf(96, np.int32), targets=buf(6),
                    anchors=buf(6), sums=buf(3), count=buf(2, np.int32), scale=buf(1), sb=288, sa=96, sy=24, sx=6, gb=288, ga=96,
                    gy=24, gx=6, bs=2, na=3, ny=4, nx=4, no=6, nc=1, nt=1, iou_t=0.2, gr=1.0, cp=1.0, cn=0.0, cls_pw=1.0,
                    obj_pw=1.0, g_box=1.0, g_obj=1.0, g_cls=1.0)


@pytest.mark.parametrize('which', ['real', 'emulation'])
def test_abi_entries_and_argument_checks(which):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in ('yh_yolo_loss_box_fwd', 'yh_yolo_loss_box_bwd'):
        assert re.search(r'\bint\s+%s\s*\(\s*const\s+yh_loss_desc\s*\*\s*d\s*,\s*int\s+box\s*,\s*float\s+gamma\s*,\s*float\s+alpha\s*,'
                         r'\s*void\s*\*\s*stream\s*\)' % name, text)
        assert name in hiplib.EXPORTS
    assert re.search(r'enum\s*\{\s*YH_BOX_GIOU\s*=\s*0\s*,\s*YH_BOX_DIOU\s*=\s*1\s*,\s*YH_BOX_CIOU\s*=\s*2\s*\}', text)
    assert hip_loss.BOX_KINDS == dict(giou=0, diou=1, ciou=2) == fakelib_box.KINDS
    assert re.search(r'#define\s+YH_ABI_VERSION\s+2\b', text) and hiplib.ABI_VERSION == 2
    lib = hiplib.load() if which == 'real' else fakelib_box.FakeLibBox()
    if which == 'real':
        assert lib.yh_abi_version() == 2 and hasattr(lib, 'yh_yolo_loss_box_fwd') and hasattr(lib, 'yh_yolo_loss_box_bwd')
    keep = []
    d = _desc(keep)
    ref = C.byref(d)
    nan, inf = float('nan'), float('inf')
    # the validation is host code and returns before any launch: every call below is refused, so no GPU is needed
    for fn in (lib.yh_yolo_loss_box_fwd, lib.yh_yolo_loss_box_bwd):
        for box in (-1, 3):
            assert fn(ref, box, 0.0, 0.25, None) == -1 and fn(ref, box, 1.5, 0.25, None) == -1, box
        for gamma in (-1.0, nan, inf):
            for box in (0, 1, 2):
                assert fn(ref, box, gamma, 0.25, None) == -1, (box, gamma)
        for alpha in (1.5, -0.1, nan):                       # check_focal's rules once gamma > 0
            assert fn(ref, 2, 1.5, alpha, None) == -1, alpha
        assert fn(None, 2, 0.0, 0.25, None) == -1
    bad = _desc(keep)
    bad.nc = 2                                   # check_loss applies as for the existing entries
    assert lib.yh_yolo_loss_box_fwd(C.byref(bad), 2, 0.0, 0.25, None) == -1
    bad = _desc(keep)
    bad.scale = None
    assert lib.yh_yolo_loss_box_bwd(C.byref(bad), 2, 0.0, 0.25, None) == -1
    assert all(not a.any() for a in keep), 'a refused call wrote to its buffers'


def test_box_loss_and_label_smoothing_flags_are_validated_by_the_parser(tmp_path, capsys):
    import train as train_mod
    parser = train_mod.make_parser()
    opt = parser.parse_args([])
    assert opt.box_loss == 'giou' and opt.label_smoothing is None
    for kind in ('giou', 'diou', 'ciou', 'cfg'):
        assert parser.parse_args(['--box-loss', kind]).box_loss == kind
    for bad in ('mse', 'iou', 'CIoU', ''):
        with pytest.raises(SystemExit):
            parser.parse_args(['--box-loss', bad])
    assert '--box-loss' in capsys.readouterr().err
    assert parser.parse_args(['--label-smoothing', '0']).label_smoothing == 0.0
    assert parser.parse_args(['--label-smoothing', '0.1']).label_smoothing == 0.1
    for bad in ('-0.1', '1', '1.5', 'nan', 'inf', 'x'):
        with pytest.raises(SystemExit):
            parser.parse_args(['--label-smoothing', bad])
    assert '--label-smoothing' in capsys.readouterr().err
    cfg = lambda rel: parse_model_cfg(os.path.join(conftest.PKG, 'cfg', rel))
    assert train_mod.box_loss_of_cfg(cfg('yolov4/yolov4.cfg')) == 'ciou'
    assert train_mod.box_loss_of_cfg(cfg('yolov4tiny/yolov4-tiny.cfg')) == 'ciou'
    assert train_mod.box_loss_of_cfg(cfg('yolov3/yolov3.cfg')) == 'giou'
    text = open(os.path.join(conftest.PKG, 'cfg', 'yolov4tiny', 'yolov4-tiny.cfg')).read()
    assert text.count('iou_loss=ciou') >= 2
    mse = tmp_path / 'mse.cfg'
    mse.write_text(text.replace('iou_loss=ciou', 'iou_loss=mse'))
    with pytest.raises(ValueError, match='mse'):
        train_mod.box_loss_of_cfg(parse_model_cfg(str(mse)))
    mixed = tmp_path / 'mixed.cfg'
    mixed.write_text(text.replace('iou_loss=ciou', 'iou_loss=diou', 1))
    with pytest.raises(ValueError, match='diou'):
        train_mod.box_loss_of_cfg(parse_model_cfg(str(mixed)))


def test_train_with_ciou_and_label_smoothing_end_to_end(dataset_dir, tiny_cfg, tmp_path, monkeypatch, capsys):
    """``train()`` of the tiny cfg on the synthetic set with ``--box-loss ciou --label-smoothing 0.1`` on the CPU: the kind reaches
    ``bbox_iou`` through the model, the smoothing reaches ``smooth_BCE`` through the hyp copy of the run (not the module's dict), and
    the run ends with a finite loss."""
    monkeypatch.chdir(tmp_path)
    import train as train_mod
    flags, eps = [], []
    real_iou, real_smooth = U.bbox_iou, U.smooth_BCE

    def spy_iou(box1, box2, x1y1x2y2=True, GIoU=False, DIoU=False, CIoU=False):
        if not x1y1x2y2:
            flags.append((GIoU, DIoU, CIoU))
        return real_iou(box1, box2, x1y1x2y2, GIoU, DIoU, CIoU)

    def spy_smooth(eps_=0.1, **kw):
        eps.append(float(kw.get('eps', eps_)))
        return real_smooth(eps=eps[-1])
    monkeypatch.setattr(U, 'bbox_iou', spy_iou)
    monkeypatch.setattr(U, 'smooth_BCE', spy_smooth)
    before = dict(train_mod.hyp)
    opt = train_mod.make_parser().parse_args(['--epochs', '1', '--batch-size', '4', '--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'),
                                              '--img-size', '64', '64', '64', '--device', 'cpu', '--nosave', '--notest',
                                              '--box-loss', 'ciou', '--label-smoothing', '0.1'])
    opt.local_rank = -1
    results = train_mod.train(opt, train_mod.hyp)
    assert len(results) == 7 and all(np.isfinite(results))
    assert flags and set(flags) == {(False, False, True)}
    assert eps and set(eps) == {0.1}
    assert train_mod.hyp == before and 'label_smoothing' not in train_mod.hyp
    assert 'Using box loss ciou, label smoothing 0.1' in capsys.readouterr().out
