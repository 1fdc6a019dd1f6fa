"""CPU tier of darknet's ``scale_x_y`` (``Darknet(scale_x_y=True)``, ``--scale-x-y``): the eager statements of decode and loss against
an independent fp64 formula (tests/sxy_cases.py), the hand-written derivative against autograd, the engine's lowering, decode, fused
candidate filter and fused-loss node on the host emulation of the new entries (tests/fakelib_sxy.py), their identity at
``scale_x_y = 1``, the argument checks of the real library and the emulation, and the flag on the three scripts.  The kernels
themselves are checked on the GPU tier (tests/test_gpu_scale_xy.py).

The reference ignores the key, so there is no recorded run to compare with; with the flag off everything must be what it was, bit
for bit, and that is the first test."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import conftest
import fakelib_sxy
import focal_cases as fc
import sxy_cases as sc
import synth
from engine import hiplib
from engine import loss as hip_loss
from engine import nms as hnms
from engine.hiplib import DecodeSxyDesc, LossDesc
from engine.plan import DarknetEngine
from models import Darknet, YOLOLayer
from utils import torch_utils
from utils import utils as U

HEADER = os.path.join(conftest.REPO, 'include', 'yolo_hip.h')
V4TINY = os.path.join(conftest.PKG, 'cfg', 'yolov4tiny', 'yolov4-tiny.cfg')
V4 = os.path.join(conftest.PKG, 'cfg', 'yolov4', 'yolov4.cfg')
V3TINY = os.path.join(conftest.PKG, 'cfg', 'yolov3tiny', 'yolov3-tiny.cfg')
EPS = 2.0 ** -24      # half an ulp of 1 in fp32: the relative error of one correctly rounded operation


@pytest.fixture
def fake(monkeypatch):
    lib = fakelib_sxy.FakeLibSxy()
    monkeypatch.setattr(hiplib, 'load', lambda: lib)
    monkeypatch.setattr(hnms, '_density', {})
    hip_loss._LIB_OVERRIDE = lib
    hip_loss.reset_stats()
    hip_loss.reset_box_stats()
    hip_loss.reset_scale_stats()
    try:
        yield lib
    finally:
        hip_loss._LIB_OVERRIDE = None


def _seeded(cfg, size, **kw):
    torch.manual_seed(0)
    m = Darknet(cfg, (size, size), **kw)
    m.load_state_dict(synth.randomize_bn_(m.state_dict(), seed=1))
    return m


def _scales(model):
    return [model.module_list[i].scale_x_y for i in model.yolo_layers]


def _loss_and_grads(model, x, targets):
    model = copy.deepcopy(model).train()
    model.nc, model.gr, model.hyp = 80, 1.0, dict(fc.HYP)
    pred, _ = model(x)
    loss, items = U.compute_loss(pred, targets, model)
    loss.backward()
    return items, [p.grad for p in model.parameters()]


# ------------------------------------------------------------------------------------------------ the flag
def test_without_the_flag_nothing_changes_and_with_it_the_layers_take_the_cfg_values():
    plain = _seeded(V4TINY, 64).eval()
    off = _seeded(V4TINY, 64, scale_x_y=False).eval()
    on = _seeded(V4TINY, 64, scale_x_y=True).eval()
    assert plain.scale_x_y is False and off.scale_x_y is False and on.scale_x_y is True
    assert _scales(plain) == [1.0, 1.0] and _scales(off) == [1.0, 1.0] and _scales(on) == [1.05, 1.05]
    x = synth.image_batch(2, 64, seed=3)
    targets = torch.tensor([[0, 3, 0.3, 0.4, 0.3, 0.4], [1, 7, 0.7, 0.6, 0.5, 0.3], [1, 0, 0.5, 0.5, 0.2, 0.6]])
    with torch.no_grad():
        a, b, c = plain(x)[0], off(x)[0], on(x)[0]
    assert torch.equal(a, b)
    assert not torch.equal(a[..., :2], c[..., :2]) and torch.equal(a[..., 2:], c[..., 2:])
    ia, ga = _loss_and_grads(plain, x, targets)
    ib, gb = _loss_and_grads(off, x, targets)
    ic, _ = _loss_and_grads(on, x, targets)
    assert torch.equal(ia, ib) and all(torch.equal(u, v) for u, v in zip(ga, gb))
    assert ic[0] != ia[0], 'the scale did not reach the loss'
    torch.manual_seed(0)
    assert _scales(Darknet(V4, (64, 64), scale_x_y=True)) == [1.2, 1.1, 1.05]


def test_a_cfg_without_the_key_takes_the_flag_as_a_no_op():
    off, on = _seeded(V3TINY, 64).eval(), _seeded(V3TINY, 64, scale_x_y=True).eval()
    assert _scales(on) == [1.0, 1.0] and on.scale_x_y is True
    x = synth.image_batch(1, 64, seed=3)
    with torch.no_grad():
        assert torch.equal(off(x)[0], on(x)[0])


# ------------------------------------------------------------------------------------------------ decode statement
@pytest.mark.parametrize('s', sc.SCALES)
def test_decode_statement_against_fp64(s):
    """``YOLOLayer`` against the fp64 formula on N=2, ny=3, nx=5, na=3, nc=2.  Bound of the centre: the value is built by four fp32
    operations (product, difference, sum, stride) whose results are at most nx * stride in size, each within half an ulp, plus the
    sigmoid (within 2 ulp of a value <= 1, multiplied by s <= 2 and the stride): 8 half-ulps of nx * stride cover it.  Logits +-20
    (sigmoid 1 - 2e-9 and 2e-9) put the centre outside [cell, cell + 1] by c on either side, to the same bound."""
    N, ny, nx, na, nc, stride = 2, 3, 5, 3, 2, 16
    no = nc + 5
    g = torch.Generator().manual_seed(5)
    p = torch.randn(N, na * no, ny, nx, generator=g)
    pv = p.view(N, na, no, ny, nx)
    pv[0, 0, 0, 1, 2], pv[0, 0, 1, 1, 2] = 20.0, -20.0
    layer = YOLOLayer(anchors=np.array([[10., 13.], [16., 30.], [33., 23.]]), nc=nc, img_size=(nx * stride, ny * stride), yolo_index=0,
                      layers=[], stride=stride, scale_x_y=s).eval()
    plain = YOLOLayer(anchors=np.array([[10., 13.], [16., 30.], [33., 23.]]), nc=nc, img_size=(nx * stride, ny * stride), yolo_index=0,
                      layers=[], stride=stride).eval()
    io, raw = layer(p.clone(), None)
    io0, _ = plain(p.clone(), None)
    want = sc.decode_statement(raw.numpy(), layer.anchor_vec.numpy(), stride, s)
    bound = 8 * EPS * nx * stride
    err = np.abs(io.numpy()[..., :2].astype(np.float64) - want[..., :2]).max()
    assert err <= bound, (err, bound)
    assert torch.equal(io[..., 2:], io0[..., 2:]), 'width, height, objectness and classes do not depend on the scale'
    c = 0.5 * (s - 1)
    row = (0 * ny + 1) * nx + 2                                  # anchor 0, y 1, x 2
    assert abs(io[0, row, 0].item() - (2 + 1 + c) * stride) <= bound and io[0, row, 0].item() > 3 * stride
    assert abs(io[0, row, 1].item() - (1 - c) * stride) <= bound and io[0, row, 1].item() < 1 * stride


# ------------------------------------------------------------------------------------------------ loss statement
@pytest.mark.parametrize('gamma', [0.0, 1.5])
@pytest.mark.parametrize('s', [1.2, 2.0])
@pytest.mark.parametrize('kind', ['giou', 'diou', 'ciou'])
def test_loss_statement_against_fp64_autograd(kind, s, gamma):
    """``compute_loss`` (fp32 torch statement) against tests/sxy_cases.py ``loss_statement`` in fp64; labels on a cell border, at offset
    0.999 and two in one cell.  Bounds of tests/focal_cases.py ``assert_close_to``.  No exact match here: the torch statement's CIoU
    is nan there (the fused path's rule is checked below and on the GPU tier)."""
    model = sc.head_model(s, kind, gamma)
    raw = sc.raw_head(exact=False)
    _, tbox, indices, _ = U.build_targets([raw], sc.LABELS, model)
    cells = torch.stack(indices[0], 1)
    assert len(torch.unique(cells, dim=0)) < len(cells), 'two labels share a cell'
    assert (tbox[0][:, :2] == 0).all(1).any(), 'a label centred on a cell border'
    assert ((tbox[0][:, :2] - 0.999).abs() < 1e-4).all(1).any(), 'a label at offset 0.999'
    p = raw.clone().requires_grad_()
    loss, items = U.compute_loss([p], sc.LABELS, model, fused=False)
    (loss * 7.0).backward()
    ref_items, ref_grads = sc.loss_statement([raw], sc.LABELS, model, [s])
    fc.assert_close_to(items, [p.grad], ref_items, ref_grads, what=(kind, s, gamma))
    unscaled, _ = sc.loss_statement([raw], sc.LABELS, model, [1.0])
    assert abs(unscaled[0] - ref_items[0]) > 1e-3 * ref_items[0], 'the scale moves the box term'


@pytest.mark.parametrize('s', [1.2, 2.0])
@pytest.mark.parametrize('kind', ['giou', 'diou', 'ciou'])
def test_closed_form_factor_equals_autograd_in_fp64(kind, s):
    """``fakelib_sxy.box_term`` - the kernel's chain seeded with ``s * sig * (1 - sig)`` - against autograd through the fp64 statement,
    candidate for candidate (bounds of the box-loss closed-form test)."""
    import box_cases as bc
    logits, anchors, tbox = bc.candidates(256, seed=11)
    x = logits.clone().requires_grad_()
    pxy = torch.sigmoid(x[:, 0:2]) * s - 0.5 * (s - 1)
    pwh = torch.exp(x[:, 2:4]).clamp(max=1e3) * anchors
    want = sc.box_measure(torch.cat((pxy, pwh), 1).t(), tbox, kind)
    want.sum().backward()
    got, dgot = fakelib_sxy.box_term(kind, logits, anchors, tbox, s)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), want.detach().numpy(), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(dgot.numpy(), x.grad.numpy(), rtol=1e-9, atol=1e-13)
    sig = torch.sigmoid(logits[:, 0])
    base, dbase = fakelib_sxy.box_term(kind, logits, anchors, tbox, 1.0)
    import fakelib_box
    ref, dref = fakelib_box.box_term(kind, logits, anchors, tbox)
    assert torch.equal(base, ref) and torch.equal(dbase, dref), 's = 1 is the unscaled chain'
    assert (dgot[:, 0].abs() > 0).any() and (sig > 0).all()


# ------------------------------------------------------------------------------------------------ emulated engine
def _kinds(plan):
    return [hiplib.OP_KIND[type(d)] for _, d in plan['ops']]


def test_lowering_uses_the_new_op_for_scaled_heads_only(fake):
    x = synth.image_batch(2, 64, seed=33)
    plain = DarknetEngine(_seeded(V4TINY, 64).eval(), precision='fp32', lib=fake)._plan_for(x)[1]
    scaled = DarknetEngine(_seeded(V4TINY, 64, scale_x_y=True).eval(), precision='fp32', lib=fake)._plan_for(x)[1]
    nokey = DarknetEngine(_seeded(V3TINY, 64, scale_x_y=True).eval(), precision='fp32', lib=fake)._plan_for(x)[1]
    nokey0 = DarknetEngine(_seeded(V3TINY, 64).eval(), precision='fp32', lib=fake)._plan_for(x)[1]
    assert hiplib.OP_DECODE_SXY == 30
    assert _kinds(plain).count(hiplib.OP_DECODE) == 2 and hiplib.OP_DECODE_SXY not in _kinds(plain)
    assert _kinds(scaled).count(hiplib.OP_DECODE_SXY) == 2 and hiplib.OP_DECODE not in _kinds(scaled)
    assert [k if k != hiplib.OP_DECODE_SXY else hiplib.OP_DECODE for k in _kinds(scaled)] == _kinds(plain)
    assert _kinds(nokey) == _kinds(nokey0) and hiplib.OP_DECODE_SXY not in _kinds(nokey)
    assert all(isinstance(d, DecodeSxyDesc) and abs(d.scale_x_y - 1.05) < 1e-7 for d in scaled['decode_descs'])
    assert not any(isinstance(d, DecodeSxyDesc) for d in plain['decode_descs'] + nokey['decode_descs'])
    assert fake.plan_kinds.count(30) == 2


def _same(a, b, tag):      # tests/test_nms_host.py
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), '%s img %d' % (tag, i)
        if x is not None:
            assert x.shape == y.shape and torch.allclose(x, y, rtol=0, atol=2e-3), '%s img %d' % (tag, i)


@pytest.mark.parametrize('ml', [False, True], ids=['best-class', 'multi-label'])
def test_engine_decode_and_detect_equal_the_host_statements(fake, ml, monkeypatch):
    """The emulated engine of yolov4-tiny with the flag at 64 px: the decoded output is the host statement (``YOLOLayer``) on the engine's
    own raw heads, to the decode bound; ``detect`` takes the new candidate entry and equals NMS of that output; so does the TTA
    form; ``YOLO_HIP_SCALE_XY=0`` decodes and then filters."""
    model = _seeded(V4TINY, 64, scale_x_y=True).eval()
    x = synth.image_batch(2, 64, seed=33)
    eng = DarknetEngine(model, precision='fp32', lib=fake)
    io, raws, _ = eng(x)
    assert fake.sxy_calls['decode'] == 2
    off = 0
    for raw, idx in zip(raws, model.yolo_layers):
        m = model.module_list[idx]
        N, na, ny, nx, no = raw.shape
        with torch.no_grad():
            want = m(raw.permute(0, 1, 4, 2, 3).reshape(N, na * no, ny, nx), None)[0]
        rows = na * ny * nx
        got = io[:, off:off + rows]
        assert (got[..., :2] - want[..., :2]).abs().max().item() <= 8 * EPS * nx * m.stride
        assert torch.allclose(got[..., 2:], want[..., 2:], rtol=2e-6, atol=0)
        off += rows
    conf = float((io[..., 5:] * io[..., 4:5]).flatten().topk(60).values[-1]) if ml else float(io[..., 4].flatten().quantile(0.9))
    two = hnms.non_max_suppression(io, conf, 0.6, multi_label=ml)
    assert sum(0 if d is None else d.shape[0] for d in two) >= 4
    del fake.calls[:]
    one = eng.detect(x, conf, 0.6, multi_label=ml)
    assert 'decode_candidates_sxy' in fake.calls and 'decode_candidates' not in fake.calls and 'nms_candidates' not in fake.calls
    _same(one, two, 'heads vs decoded tensor')
    aug = hnms.non_max_suppression(eng.forward_augmented(x), conf, 0.6, multi_label=ml)
    del fake.calls[:]
    _same(eng.detect(x, conf, 0.6, multi_label=ml, augment=True), aug, 'augmented')
    assert fake.calls.count('decode_candidates_sxy') == 6 and 'decode_candidates_tta' not in fake.calls
    monkeypatch.setenv('YOLO_HIP_SCALE_XY', '0')
    del fake.calls[:]
    _same(eng.detect(x, conf, 0.6, multi_label=ml), two, 'switched off')
    _same(eng.detect(x, conf, 0.6, multi_label=ml, augment=True), aug, 'switched off, augmented')
    assert 'decode_candidates_sxy' not in fake.calls and 'nms_candidates' in fake.calls


def _checks(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), t.abs().max().item()])


@pytest.mark.parametrize('gamma', [0.0, 1.5])
@pytest.mark.parametrize('s', [1.2, 2.0])
@pytest.mark.parametrize('kind', ['giou', 'diou', 'ciou'])
def test_fused_loss_node_matches_the_torch_statement(fake, kind, s, gamma):
    """engine/loss.py on the emulated ``yh_yolo_loss_head_*`` entries, through a padded NHWC base, against the fp32 torch statement
    (bounds of tests/test_box_loss.py's glue test); the counters show one scaled call per head and pass with the head's scale."""
    model = sc.head_model(s, kind, gamma)
    raw = sc.raw_head(exact=False)
    bases, views = fc.nhwc_views([raw], 'cpu')
    loss, items = U.compute_loss(views, sc.LABELS, model)
    (loss * 3.0).backward()
    assert hip_loss.scale_stats() == dict(scale_fwd=1, scale_bwd=1) and fake.sxy_calls['fwd'] == 1 and fake.sxy_calls['bwd'] == 1
    assert [round(v, 6) for _, v in fake.sxy_args] == [s, s]
    assert fake.box_calls == dict(fwd=0, bwd=0) and fake.focal_calls == dict(fwd=0, bwd=0)
    ref_items, ref_grads = fc.torch_statement([raw], sc.LABELS, model, dtype=torch.float32, scale=3.0)
    assert hip_loss.scale_stats() == dict(scale_fwd=1, scale_bwd=1), 'fused=False went to the entries'
    np.testing.assert_allclose(items.numpy(), ref_items.numpy(), rtol=3e-6)
    na, no = raw.shape[1], raw.shape[4]
    assert bases[0].grad[..., na * no:].abs().max() == 0
    np.testing.assert_allclose(bases[0].grad.numpy(), ref_grads[0].numpy(), rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(_checks(bases[0].grad), _checks(ref_grads[0]), rtol=2e-5)
    ref64, _ = sc.loss_statement([raw], sc.LABELS, model, [s])
    np.testing.assert_allclose(items.numpy(), ref64.numpy(), rtol=1e-5, atol=1e-6)


def test_exact_match_stays_finite_on_the_fused_node(fake):
    """One prediction equals its label (tests/sxy_cases.py ``EXACT``; with zero logits the centre is 0.5 for every s).  The loss items
    equal the fp64 statement; so does the gradient everywhere but at that candidate's four box logits, where every min / max of the
    measure is a tie and the derivative is a choice (autograd splits a tie, the chain takes the prediction's side): there the node
    gives the closed form of tests/fakelib_sxy.py, finite."""
    s, kind = 2.0, 'ciou'
    model = sc.head_model(s, kind, 0.0)
    raw = sc.raw_head(exact=True)
    p = raw.clone().requires_grad_()
    loss, items = U.compute_loss([p], sc.LABELS, model)
    loss.backward()
    assert torch.isfinite(items).all() and torch.isfinite(p.grad).all()
    ref_items, ref_grads = sc.loss_statement([raw], sc.LABELS, model, [s], scale=1.0)
    b, a, gy, gx = sc.EXACT
    got, want = p.grad.clone(), ref_grads[0].clone()
    at_match = got[b, a, gy, gx, :4].clone()
    got[b, a, gy, gx, :4] = want[b, a, gy, gx, :4] = 0
    fc.assert_close_to(items, [got], ref_items, [want], what='exact match')
    _, _, indices, _ = U.build_targets([raw], sc.LABELS, model)
    nb = len(indices[0][0])
    val, dval = fakelib_sxy.box_term(kind, raw[b, a, gy, gx, :4][None], torch.tensor([[2.0, 3.0]]), torch.tensor([[0.5, 0.5, 2.0, 3.0]]), s)
    assert val.item() == 1.0
    torch.testing.assert_close(at_match, -(model.hyp['giou'] / nb) * dval[0], rtol=1e-5, atol=1e-9)
    _, stmt = U.compute_loss([raw], sc.LABELS, model, fused=False)
    assert torch.isnan(stmt[0]), 'the torch statement divides 0 by 0 there'


def test_env_switch_keeps_the_torch_statement(fake, monkeypatch):
    monkeypatch.setenv('YOLO_HIP_SCALE_XY', '0')
    model = sc.head_model(1.2)
    raw = sc.raw_head(exact=False)
    _, items = U.compute_loss([raw], sc.LABELS, model)
    assert hip_loss.scale_stats() == dict(scale_fwd=0, scale_bwd=0) and fake.sxy_calls['fwd'] == 0
    _, ref = U.compute_loss([raw], sc.LABELS, model, fused=False)
    assert torch.equal(items, ref)
    seen = []      # the switch is about scaled heads only: an unscaled model stays on the fused entries
    monkeypatch.setattr(fake, 'yh_yolo_loss_fwd', lambda d, st, f=fake.yh_yolo_loss_fwd: (seen.append(1), f(d, st))[1])
    U.compute_loss([raw], sc.LABELS, sc.head_model(1.0))
    assert seen == [1]


# ------------------------------------------------------------------------------------------------ identity at 1
def _decode_pair(lib, s, raw_out):
    N, ny, nx, na, nc = 2, 7, 5, 3, 4
    no = nc + 5
    p = sc.head_map(N, ny, nx, na, nc, 32)
    avec = sc.ANCHORS_PX / 16.0
    rows_total = na * ny * nx + 10
    out = []
    for scaled in (False, True):
        io = torch.full((N, rows_total, no), -1.0)
        raw = torch.full((N, na, ny, nx, no), -1.0) if raw_out else None
        d = sc.decode_desc(p, io, raw, na, no, 16.0, avec, rows_total, 6, s if scaled else None)
        rc = (lib.yh_yolo_decode_sxy if scaled else lib.yh_yolo_decode)(C.byref(d), None)
        assert rc == 0
        out.append((io, raw))
    return out


def test_emulated_entries_at_scale_one_are_the_entries_they_extend():
    lib = fakelib_sxy.FakeLibSxy()
    (io0, raw0), (io1, raw1) = _decode_pair(lib, 1.0, True)
    assert torch.equal(io0, io1) and torch.equal(raw0, raw1) and lib.sxy_calls['decode'] == 0
    (io0, _), (io2, _) = _decode_pair(lib, 1.2, False)
    assert not torch.equal(io0, io2) and lib.sxy_calls['decode'] == 1
    # fused candidate filter, plain and TTA form
    N, ny, nx, na, nc = 2, 7, 5, 3, 4
    p = sc.head_map(N, ny, nx, na, nc, 32)
    rows = na * ny * nx
    for ml in (0, 1):
        for scale, flip_w in ((1.0, -1.0), (0.83, 80.0)):
            got = []
            for scaled in (False, True):
                cand = torch.zeros(N, 512, 8)
                count = torch.zeros(N, dtype=torch.int32)
                d = sc.decode_desc(p, None, None, na, nc + 5, 16.0, sc.ANCHORS_PX / 16.0, rows + 10, 6, 1.0 if scaled else None)
                if scaled:
                    rc = lib.yh_yolo_decode_candidates_sxy(C.byref(d), scale, flip_w, 0.3, ml, None, hiplib.ptr(cand), hiplib.ptr(count), 512, None)
                elif flip_w < 0:
                    rc = lib.yh_yolo_decode_candidates(C.byref(d), 0.3, ml, None, hiplib.ptr(cand), hiplib.ptr(count), 512, None)
                else:
                    rc = lib.yh_yolo_decode_candidates_tta(C.byref(d), scale, flip_w, 0.3, ml, None, hiplib.ptr(cand), hiplib.ptr(count), 512, None)
                assert rc == 0 and int(count.min()) > 10
                got.append((cand, count))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert lib.sxy_calls['candidates'] == 0
    # loss
    for kind, gamma in ((0, 0.0), (2, 1.5)):
        res = []
        for head in (False, True):
            raw = sc.raw_head(exact=False)
            keep = dict(tobj=torch.zeros(sc.BS, sc.NA, sc.NY, sc.NX), winner=torch.full((sc.BS, sc.NA, sc.NY, sc.NX), -1, dtype=torch.int32),
                        sums=torch.zeros(3), count=torch.zeros(2, dtype=torch.int32), grad=torch.zeros_like(raw), scale=torch.ones(1),
                        anchors=torch.tensor(sc.ANCHORS_PX / sc.STRIDE, dtype=torch.float32), targets=sc.LABELS.clone())
            d = _loss_desc(raw, keep)
            if head:
                assert lib.yh_yolo_loss_head_fwd(C.byref(d), kind, gamma, 0.25, 1.0, None) == 0
                assert lib.yh_yolo_loss_head_bwd(C.byref(d), kind, gamma, 0.25, 1.0, None) == 0
            else:
                assert lib.yh_yolo_loss_box_fwd(C.byref(d), kind, gamma, 0.25, None) == 0
                assert lib.yh_yolo_loss_box_bwd(C.byref(d), kind, gamma, 0.25, None) == 0
            res.append(keep)
        for k in ('tobj', 'sums', 'count', 'grad'):
            assert torch.equal(res[0][k], res[1][k]), k
        assert res[0]['grad'].abs().max() > 0
    assert lib.sxy_calls['fwd'] == 0 and lib.box_calls == dict(fwd=4, bwd=4)


def _loss_desc(raw, k):
    P = hiplib.ptr
    g = k['grad']
    return LossDesc(p=P(raw), grad=P(g), tobj=P(k['tobj']), winner=P(k['winner']), targets=P(k['targets']), anchors=P(k['anchors']),
                    sums=P(k['sums']), count=P(k['count']), scale=P(k['scale']), sb=raw.stride(0), sa=raw.stride(1), sy=raw.stride(2),
                    sx=raw.stride(3), gb=g.stride(0), ga=g.stride(1), gy=g.stride(2), gx=g.stride(3), bs=sc.BS, na=sc.NA, ny=sc.NY,
                    nx=sc.NX, no=sc.NC + 5, nc=sc.NC, nt=k['targets'].shape[0], iou_t=0.2, gr=0.6, cp=1.0, cn=0.0, cls_pw=1.3,
                    obj_pw=0.8, g_box=3.54, g_obj=64.3, g_cls=37.4)


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize('bad', ['0.9', '2.5', 'nan'])
def test_a_scale_outside_the_range_raises_a_value_error_that_names_the_block(bad, tmp_path):
    text = open(V4TINY).read()
    assert text.count('scale_x_y') == 2
    cfg = tmp_path / 'bad.cfg'
    cfg.write_text(re.sub(r'scale_x_y\s*=\s*[0-9.]+', 'scale_x_y=' + bad, text, count=1))
    blocks = [ln.strip() for ln in text.split('\n') if ln.strip().startswith('[')]
    first_yolo = blocks.index('[yolo]')
    with pytest.raises(ValueError, match=r'block %d \[yolo\].*scale_x_y' % first_yolo):
        Darknet(str(cfg), (64, 64), scale_x_y=True)
    torch.manual_seed(0)
    assert _scales(Darknet(str(cfg), (64, 64))) == [1.0, 1.0], 'without the flag the key stays ignored'


@pytest.mark.parametrize('which', ['real', 'emulation'])
def test_abi_entries_and_argument_checks(which):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'typedef\s+struct\s+yh_decode_sxy_desc\s*\{\s*yh_decode_desc\s+d\s*;\s*float\s+scale_x_y\s*;\s*\}\s*yh_decode_sxy_desc\s*;', text)
    assert re.search(r'\bint\s+yh_yolo_decode_sxy\s*\(\s*const\s+yh_decode_sxy_desc\s*\*\s*d\s*,\s*void\s*\*\s*stream\s*\)', text)
    assert re.search(r'\bint\s+yh_yolo_decode_candidates_sxy\s*\(\s*const\s+yh_decode_sxy_desc\s*\*\s*d\s*,\s*float\s+scale\s*,\s*float\s+flip_w\s*,', text)
    for name in ('yh_yolo_loss_head_fwd', 'yh_yolo_loss_head_bwd'):
        assert re.search(r'\bint\s+%s\s*\(\s*const\s+yh_loss_desc\s*\*\s*d\s*,\s*int\s+box\s*,\s*float\s+gamma\s*,\s*float\s+alpha\s*,'
                         r'\s*float\s+scale_x_y\s*,\s*void\s*\*\s*stream\s*\)' % name, text)
    assert re.search(r'YH_OP_DECODE_SXY\s*=\s*30\b', text) and hiplib.OP_DECODE_SXY == 30
    assert re.search(r'#define\s+YH_ABI_VERSION\s+2\b', text) and hiplib.ABI_VERSION == 2
    names = ('yh_yolo_decode_sxy', 'yh_yolo_decode_candidates_sxy', 'yh_yolo_loss_head_fwd', 'yh_yolo_loss_head_bwd')
    assert all(n in hiplib.EXPORTS for n in names)
    assert C.sizeof(DecodeSxyDesc) == C.sizeof(hiplib.DecodeDesc) + 8 and DecodeSxyDesc.d.offset == 0      # 8-byte aligned struct
    lib = hiplib.load() if which == 'real' else fakelib_sxy.FakeLibSxy()
    if which == 'real':
        assert lib.yh_abi_version() == 2 and all(hasattr(lib, n) for n in names)
    nan, inf = float('nan'), float('inf')
    keep = []
    buf = lambda n, dt=np.float32: keep.append(np.zeros(n, dt)) or keep[-1].ctypes.data
    # the validation is host code and returns before any launch: every call below is refused, so no GPU is needed
    for s in (0.9, 0.999, 2.5, 2.001, -1.2, nan, inf):
        d = hiplib.DecodeDesc(p=buf(2 * 4 * 4 * 32), io=buf(2 * 48 * 9), raw=None, n=2, ny=4, nx=4, na=3, no=9, ldp=32, rows_total=48,
                              row_off=0, stride=8.0)
        w = DecodeSxyDesc(d=d, scale_x_y=s)
        assert lib.yh_yolo_decode_sxy(C.byref(w), None) == -1, s
        assert lib.yh_yolo_decode_candidates_sxy(C.byref(w), 1.0, -1.0, 0.3, 0, None, buf(2 * 64 * 8), buf(2, np.int32), 64, None) == -1, s
        raw = torch.zeros(sc.BS, sc.NA, sc.NY, sc.NX, sc.NC + 5)
        k = dict(tobj=torch.zeros(sc.BS, sc.NA, sc.NY, sc.NX), winner=torch.full((sc.BS, sc.NA, sc.NY, sc.NX), -1, dtype=torch.int32),
                 sums=torch.zeros(3), count=torch.zeros(2, dtype=torch.int32), grad=torch.zeros_like(raw), scale=torch.ones(1),
                 anchors=torch.ones(3, 2), targets=sc.LABELS.clone())
        ld = _loss_desc(raw, k)
        for box in (0, 1, 2):
            assert lib.yh_yolo_loss_head_fwd(C.byref(ld), box, 0.0, 0.25, s, None) == -1, s
            assert lib.yh_yolo_loss_head_bwd(C.byref(ld), box, 1.5, 0.25, s, None) == -1, s
        assert not k['sums'].any() and not k['grad'].any() and not k['count'].any()
    w = DecodeSxyDesc(d=d, scale_x_y=1.2)
    for scale, flip_w in ((0.0, -1.0), (-1.0, 5.0), (nan, -1.0), (1.0, nan)):
        assert lib.yh_yolo_decode_candidates_sxy(C.byref(w), scale, flip_w, 0.3, 0, None, buf(2 * 64 * 8), buf(2, np.int32), 64, None) == -1
    assert lib.yh_yolo_decode_sxy(None, None) == -1
    assert lib.yh_yolo_loss_head_fwd(C.byref(ld), 3, 0.0, 0.25, 1.2, None) == -1      # the rules of yh_yolo_loss_box_* still apply
    assert lib.yh_yolo_loss_head_fwd(C.byref(ld), 2, -1.0, 0.25, 1.2, None) == -1
    assert lib.yh_yolo_loss_head_bwd(C.byref(ld), 2, 1.5, 1.5, 1.2, None) == -1
    assert all(not a.any() for a in keep), 'a refused call wrote to its buffers'


# ------------------------------------------------------------------------------------------------ CLI and copies
def test_the_flag_parses_on_the_three_scripts_and_survives_copies(capsys):
    import detect as detect_mod
    import test as test_mod
    import train as train_mod
    for mod in (train_mod, test_mod, detect_mod):
        parser = mod.make_parser()
        assert parser.parse_args([]).scale_x_y is False and parser.parse_args(['--scale-x-y']).scale_x_y is True
        text = ' '.join(parser.format_help().split())
        assert '--scale-x-y' in text and 'reference ignores' in text and 'grid sensitivity' in text
    torch.manual_seed(0)
    model = Darknet(V4, (64, 64), scale_x_y=True)
    dup = copy.deepcopy(model)
    assert dup.scale_x_y is True and _scales(dup) == [1.2, 1.1, 1.05]
    ema = torch_utils.ModelEMA(model)
    assert ema.ema.scale_x_y is True and _scales(ema.ema) == [1.2, 1.1, 1.05]
    ema.update(model)
    ema.update_attr(model)
    assert ema.ema.scale_x_y is True and _scales(ema.ema) == [1.2, 1.1, 1.05]
