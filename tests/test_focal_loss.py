"""CPU tier of focal loss on the fused loss kernels (``hyp['fl_gamma'] > 0``: csrc/loss.hip ``yh_yolo_loss_focal_fwd`` / ``_bwd`` behind
engine/loss.py): the autograd node on the host emulation (tests/fakelib_focal.py) against the reference's own numbers, the emulation's
closed form against ``utils.utils.FocalLoss`` under autograd in fp64, the C ABI and its argument checks on the real library, and
``train.py --fl-gamma``.  The kernels themselves are checked on the GPU tier (tests/test_gpu_focal_loss.py)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import conftest
import fakelib_focal
import focal_cases as fc
import synth
from engine import hiplib
from engine import loss as hip_loss
from engine.hiplib import LossDesc
from models import Darknet
from utils import utils as U

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(conftest.REPO, 'include', 'yolo_hip.h')
GOLD_HYP = {'giou': 3.54, 'cls': 37.4, 'cls_pw': 1.0, 'obj': 64.3, 'obj_pw': 1.0, 'iou_t': 0.20, 'fl_gamma': 0.0}


@pytest.fixture
def fake():
    lib = fakelib_focal.FakeLibFocal()
    hip_loss._LIB_OVERRIDE = lib
    hip_loss.reset_stats()
    try:
        yield lib
    finally:
        hip_loss._LIB_OVERRIDE = None


def _checks(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), t.abs().max().item()])


def _golden_case():
    """The ``focal`` case of tests/golden/loss.npz: yolov3, 320 px, nc 80, batch 3, gamma 1.5."""
    torch.manual_seed(0)
    model = Darknet(os.path.join(conftest.PKG, 'cfg', 'yolov3/yolov3.cfg'), (320, 320))
    model.nc, model.hyp, model.gr = 80, dict(GOLD_HYP, fl_gamma=np.float64(1.5)), 0.7      # a numpy scalar, as a hyp file gives it
    raws, targets = synth.loss_inputs(model, 320, batch=3, seed=21)
    return model, raws, targets


def test_fused_focal_glue_matches_reference_goldens(fake):
    """engine/loss.py on the emulated focal entries, through padded NHWC bases, against the reference's own loss values and gradients
    (tolerances of test_fused_loss_glue_matches_reference_goldens); the counters show that the focal entries ran - once per head and
    pass - and not the torch statement, which produces the same numbers."""
    gold = np.load(os.path.join(HERE, 'golden', 'loss.npz'))
    model, raws, targets = _golden_case()
    bases, views = fc.nhwc_views(raws, 'cpu')
    loss, items = U.compute_loss(views, targets, model)
    (loss * 3.0).backward()
    assert hip_loss.stats() == dict(focal_fwd=3, focal_bwd=3)
    assert fake.focal_calls == dict(fwd=3, bwd=3)
    assert fake.focal_args == [(1.5, 0.25)] * 6
    np.testing.assert_allclose(items.numpy(), gold['focal_items'], rtol=3e-6)
    for i, (r, base) in enumerate(zip(raws, bases)):
        bs, na, ny, nx, no = r.shape
        g = base.grad[..., :na * no].view(bs, ny, nx, na, no).permute(0, 3, 1, 2, 4) / 3.0
        assert base.grad[..., na * no:].abs().max() == 0
        np.testing.assert_allclose(g.reshape(-1)[::97].numpy(), gold['focal_grad%d_rows' % i], rtol=2e-5, atol=1e-9)
        np.testing.assert_allclose(_checks(g), gold['focal_grad%d_checks' % i], rtol=2e-5)


def test_gamma_zero_keeps_the_existing_entries(fake):
    model, raws, targets = _golden_case()
    model.hyp['fl_gamma'] = 0.0
    bases, views = fc.nhwc_views(raws, 'cpu')
    loss, _ = U.compute_loss(views, targets, model)
    loss.backward()
    assert hip_loss.stats() == dict(focal_fwd=0, focal_bwd=0) and fake.focal_calls == dict(fwd=0, bwd=0)
    assert all(b.grad is not None for b in bases)


def test_env_switch_keeps_the_torch_statement(fake, monkeypatch):
    monkeypatch.setenv('YOLO_HIP_FOCAL_LOSS', '0')
    gold = np.load(os.path.join(HERE, 'golden', 'loss.npz'))
    model, raws, targets = _golden_case()
    bases, views = fc.nhwc_views(raws, 'cpu')
    loss, items = U.compute_loss(views, targets, model)
    loss.backward()
    assert hip_loss.stats() == dict(focal_fwd=0, focal_bwd=0) and fake.focal_calls == dict(fwd=0, bwd=0)
    np.testing.assert_allclose(items.numpy(), gold['focal_items'], rtol=3e-6)
    # the switch is about focal loss only: the default loss stays on the fused entries
    model.hyp['fl_gamma'] = 0.0
    seen = []
    monkeypatch.setattr(fake, 'yh_yolo_loss_fwd', lambda d, s, f=fake.yh_yolo_loss_fwd: (seen.append(1), f(d, s))[1])
    U.compute_loss(views, targets, model)
    assert len(seen) == 3


def _elements(n, seed):
    """Logits in [-12, 12] with soft targets in (0, 1) and with 0 / 1 targets, fp64."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(2 * n, generator=g, dtype=torch.float64) * 24 - 12)
    x[:4] = torch.tensor([-12.0, 12.0, 0.0, -0.0], dtype=torch.float64)
    soft = torch.rand(n, generator=g, dtype=torch.float64)
    hard = (torch.rand(n, generator=g) < 0.5).double()
    return x, torch.cat((soft, hard))


@pytest.mark.parametrize('pw', [1.0, 1.3])
@pytest.mark.parametrize('gamma', fc.GAMMAS)
def test_closed_form_equals_focal_loss_autograd_in_fp64(gamma, pw):
    """``fakelib_focal.focal_elem`` - the formula of include/yolo_hip.h, value and derivative - against ``utils.utils.FocalLoss`` around
    ``BCEWithLogitsLoss(pos_weight)`` under autograd, element for element in fp64.  Bound: at |x| <= 12 the statement's ``1 - p_t``
    cancels at most log2(e^12) = 17.3 of fp64's 53 bits, which ``** gamma`` (gamma <= 3) and its derivative amplify by at most
    gamma: 3 * 2^-35.7 = 5.4e-11 relative; 1e-9 leaves room for the remaining roundings.  ``atol`` covers derivatives near their zero
    crossing (soft targets), against values of order 1."""
    x, t = _elements(4096, seed=int(gamma * 10 + pw * 100))
    xr = x.clone().requires_grad_()
    stmt = U.FocalLoss(nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw], dtype=torch.float64), reduction='none'), gamma)
    want = stmt(xr, t)
    want.sum().backward()
    L, dL = fakelib_focal.focal_elem(x, t, pw, gamma, 0.25)
    assert L.dtype == torch.float64 and torch.isfinite(want).all() and torch.isfinite(xr.grad).all()
    np.testing.assert_allclose(L.numpy(), want.detach().numpy(), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(dL.numpy(), xr.grad.numpy(), rtol=1e-9, atol=1e-13)
    assert (L > 0).all() and dL.abs().max() > 0.01


def test_saturated_elements_take_the_limit_where_fp32_torch_is_not_finite():
    """The ``q <= 0`` rule on hand-made elements.  fp32 rounds sigmoid(40) to 1 and sigmoid(-120) to 0, so ``1 - p_t`` is exactly 0
    there: the closed form returns the limit, 0 and 0; the torch statement's autograd multiplies a zero loss by the infinite
    derivative of ``0 ** 0.5``.  This is the documented, deliberate difference between the kernels and fp32 torch."""
    x = torch.tensor([40.0, -120.0])
    t = torch.tensor([1.0, 0.0])
    for gamma in fc.GAMMAS:
        L, dL = fakelib_focal.focal_elem(x, t, 1.0, gamma, 0.25)
        assert L.dtype == torch.float32
        assert torch.equal(L, torch.zeros(2)) and torch.equal(dL, torch.zeros(2)), gamma
    xr = x.clone().requires_grad_()
    stmt = U.FocalLoss(nn.BCEWithLogitsLoss(pos_weight=torch.tensor([1.0]), reduction='none'), 0.5)
    out = stmt(xr, t)
    out.sum().backward()
    assert torch.equal(out.detach(), torch.zeros(2))
    assert not torch.isfinite(xr.grad).any()
    # a NaN logit is not hidden by the rule
    L, dL = fakelib_focal.focal_elem(torch.tensor([float('nan')]), torch.tensor([0.0]), 1.0, 1.5, 0.25)
    assert torch.isnan(L).all() and torch.isnan(dL).all()


def _desc(keep):
    """A descriptor that passes check_loss for both passes (host memory: the entries must return before any launch)."""
    buf = lambda n, dt=np.float32: keep.append(np.zeros(n, dt)) or keep[-1].ctypes.data
    return LossDesc(p=buf(2 * 3 * 4 * 4 * 6), grad=buf(2 * 3 * 4 * 4 * 6), tobj=buf(96), winner=buf(96, np.int32), targets=buf(6),
                    anchors=buf(6), sums=buf(3), count=buf(2, np.int32), scale=buf(1), sb=288, sa=96, sy=24, sx=6, gb=288, ga=96,
                    gy=24, gx=6, bs=2, na=3, ny=4, nx=4, no=6, nc=1, nt=1, iou_t=0.2, gr=1.0, cp=1.0, cn=0.0, cls_pw=1.0,
                    obj_pw=1.0, g_box=1.0, g_obj=1.0, g_cls=1.0)


@pytest.mark.parametrize('which', ['real', 'emulation'])
def test_abi_entries_and_argument_checks(which):
    import ctypes as C
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in ('yh_yolo_loss_focal_fwd', 'yh_yolo_loss_focal_bwd'):
        assert re.search(r'\bint\s+%s\s*\(\s*const\s+yh_loss_desc\s*\*\s*d\s*,\s*float\s+gamma\s*,\s*float\s+alpha\s*,\s*void\s*\*\s*stream\s*\)' % name, text)
        assert name in hiplib.EXPORTS
    assert re.search(r'#define\s+YH_ABI_VERSION\s+2\b', text) and hiplib.ABI_VERSION == 2
    lib = hiplib.load() if which == 'real' else fakelib_focal.FakeLibFocal()
    if which == 'real':
        assert lib.yh_abi_version() == 2 and hasattr(lib, 'yh_yolo_loss_focal_fwd') and hasattr(lib, 'yh_yolo_loss_focal_bwd')
    keep = []
    d = _desc(keep)
    ref = C.byref(d)
    nan, inf = float('nan'), float('inf')
    # the validation is host code and returns before any launch: every call below is refused, so no GPU is needed
    for fn in (lib.yh_yolo_loss_focal_fwd, lib.yh_yolo_loss_focal_bwd):
        for gamma, alpha in ((0.0, 0.25), (-1.0, 0.25), (nan, 0.25), (inf, 0.25), (1.5, 1.5), (1.5, -0.1), (1.5, nan)):
            assert fn(ref, gamma, alpha, None) == -1, (gamma, alpha)
        assert fn(None, 1.5, 0.25, None) == -1
    bad = _desc(keep)
    bad.nc = 2                                   # check_loss applies as for the existing entries
    assert lib.yh_yolo_loss_focal_fwd(C.byref(bad), 1.5, 0.25, None) == -1
    bad = _desc(keep)
    bad.scale = None
    assert lib.yh_yolo_loss_focal_bwd(C.byref(bad), 1.5, 0.25, None) == -1
    assert all(not a.any() for a in keep), 'a refused call wrote to its buffers'


def test_fl_gamma_flag_is_validated_by_the_parser(capsys):
    import train as train_mod
    parser = train_mod.make_parser()
    assert parser.parse_args([]).fl_gamma is None
    assert parser.parse_args(['--fl-gamma', '1.5']).fl_gamma == 1.5
    assert parser.parse_args(['--fl-gamma', '0']).fl_gamma == 0.0
    for bad in ('-1', 'nan', 'inf', 'x'):
        with pytest.raises(SystemExit):
            parser.parse_args(['--fl-gamma', bad])
    assert '--fl-gamma' in capsys.readouterr().err


def test_train_with_fl_gamma_end_to_end(dataset_dir, tiny_cfg, tmp_path, monkeypatch, capsys):
    """``train()`` of the tiny cfg on the synthetic set with ``--fl-gamma 1.5`` on the CPU: the flag reaches the hyp copy of the run
    (not the module's dict), the torch statement builds ``FocalLoss`` with it, and the run ends with a finite loss."""
    monkeypatch.chdir(tmp_path)
    import train as train_mod
    seen = []
    real = U.FocalLoss

    class Spy(real):
        def __init__(self, loss_fcn, gamma=1.5, alpha=0.25):
            seen.append((float(gamma), alpha))
            super().__init__(loss_fcn, gamma, alpha)
    monkeypatch.setattr(U, 'FocalLoss', Spy)
    opt = train_mod.make_parser().parse_args(['--epochs', '1', '--batch-size', '4', '--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'),
                                              '--img-size', '64', '64', '64', '--device', 'cpu', '--nosave', '--notest', '--fl-gamma', '1.5'])
    opt.local_rank = -1
    results = train_mod.train(opt, train_mod.hyp)
    assert len(results) == 7 and all(np.isfinite(results))
    assert seen and set(seen) == {(1.5, 0.25)}
    assert train_mod.hyp['fl_gamma'] == 0.0
    assert 'Using FocalLoss(gamma=1.5)' in capsys.readouterr().out
