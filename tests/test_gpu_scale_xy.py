"""GPU tier of darknet's ``scale_x_y``: the decode kernels' SXY form (csrc/elementwise.hip, cell and general kernel), the fused decode +
candidate filter (csrc/nms.hip, plain and TTA form), the matched loss kernels (csrc/loss.hip ``box_measure_of<BOX, true>``), the
identity of every new entry at ``scale_x_y = 1``, and yolov4-tiny with the flag end to end: fp32 / fp16 engine, ``hip_detect``, hipGraph
replay, one HIP training step with and without ``YOLO_HIP_SCALE_XY=0``, and the int8 engine.

The comparison points are the host statements (``YOLOLayer`` on the CPU in fp32 for decode, tests/sxy_cases.py ``loss_statement`` in fp64
for the loss); the reference ignores the key, so no recorded run exists.  Every test prints its figures before it asserts."""
import copy
import ctypes as C
import functools
import os

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
from engine.hiplib import DecodeSxyDesc, LossDesc
from models import Darknet
from utils import utils as U

pytestmark = pytest.mark.gpu

GPU = 'cuda'
V4TINY = os.path.join(conftest.PKG, 'cfg', 'yolov4tiny', 'yolov4-tiny.cfg')
ANCHORS16 = np.array([[10., 13.], [16., 30.], [33., 23.]])
P = hiplib.ptr


@pytest.fixture(scope='module', autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    hiplib.load()


def _stream():
    return hiplib.stream_ptr()


# ------------------------------------------------------------------------------------------------ decode
def _head(nc):
    """The head of test_decode_matches_emulation_and_oracle (N=2, ny=7, nx=5, na=3, pitch 32 at nc=4: the cell kernel); nc=81 makes
    na * no = 258 > 256: the general kernel."""
    N, ny, nx, na = 2, 7, 5, 3
    no = nc + 5
    pitch = 32 if na * no <= 32 else (na * no + 7) // 8 * 8
    return sc.head_map(N, ny, nx, na, nc, pitch), na, no, na * ny * nx


def _decode(lib, p, na, no, s, want_raw, rows_total, row_off):
    N, ny, nx, _ = p.shape
    io = torch.full((N, rows_total, no), -1.0, device=GPU)
    raw = torch.full((N, na, ny, nx, no), -1.0, device=GPU) if want_raw else None
    d = sc.decode_desc(p, io, raw, na, no, 16.0, ANCHORS16 / 16.0, rows_total, row_off, s)
    with hiplib.on_device(p):
        rc = (lib.yh_yolo_decode if s is None else lib.yh_yolo_decode_sxy)(C.byref(d), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return io, raw


@pytest.mark.parametrize('want_raw', [False, True], ids=['io', 'io+raw'])
@pytest.mark.parametrize('s', sc.SCALES)
@pytest.mark.parametrize('nc', [4, 81], ids=['cell-kernel', 'general-kernel'])
def test_decode_kernels_match_the_host_statement(nc, s, want_raw):
    """``rtol 2e-6, atol 2e-5 * s``: the bound of test_decode_matches_emulation_and_oracle with the absolute term scaled, because the
    sigmoid's error is multiplied by s."""
    lib = hiplib.load()
    p, na, no, rows = _head(nc)
    io, raw = _decode(lib, p.to(GPU), na, no, s, want_raw, rows + 10, 6)
    want = sc.host_decode(sc.raw_view(p, na, no), ANCHORS16, 16, s, nc)
    got = io[:, 6:6 + rows].cpu()
    err = (got - want).abs()
    print('decode nc %d s %g raw %s: largest distance %.3e (centres %.3e), largest value %.1f'
          % (nc, s, want_raw, err.max().item(), err[..., :2].max().item(), want.abs().max().item()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-6, atol=2e-5 * s)
    assert torch.equal(io[:, :6].cpu(), torch.full((2, 6, no), -1.0)) and torch.equal(io[:, 6 + rows:].cpu(), torch.full((2, 4, no), -1.0))
    if want_raw:
        assert torch.equal(raw.cpu(), sc.raw_view(p, na, no))
    plain = sc.host_decode(sc.raw_view(p, na, no), ANCHORS16, 16, 1.0, nc)
    assert (want[..., :2] - plain[..., :2]).abs().max() > 0.2 * (s - 1) * 16, 'the scale moves the centres'


# ------------------------------------------------------------------------------------------------ identity at 1
@pytest.mark.parametrize('nc', [4, 81], ids=['cell-kernel', 'general-kernel'])
def test_decode_at_scale_one_is_yh_yolo_decode(nc):
    lib = hiplib.load()
    p, na, no, rows = _head(nc)
    io0, raw0 = _decode(lib, p.to(GPU), na, no, None, True, rows + 10, 6)
    io1, raw1 = _decode(lib, p.to(GPU), na, no, 1.0, True, rows + 10, 6)
    assert torch.equal(io0, io1) and torch.equal(raw0, raw1)


def _candidates(lib, p, na, no, s, scale, flip_w, ml, conf, entry):
    """Records of one head through ``entry`` in ('plain', 'tta', 'sxy'), as (cand, count)."""
    N, ny, nx, _ = p.shape
    rows = na * ny * nx
    cap = rows * (no - 5)
    cand = torch.zeros(N, cap, 8, device=GPU)
    count = torch.zeros(N, dtype=torch.int32, device=GPU)
    d = sc.decode_desc(p, None, None, na, no, 16.0, ANCHORS16 / 16.0, rows + 10, 6, s if entry == 'sxy' else None)
    with hiplib.on_device(p):
        if entry == 'sxy':
            rc = lib.yh_yolo_decode_candidates_sxy(C.byref(d), scale, flip_w, conf, ml, None, P(cand), P(count), cap, _stream())
        elif entry == 'tta':
            rc = lib.yh_yolo_decode_candidates_tta(C.byref(d), scale, flip_w, conf, ml, None, P(cand), P(count), cap, _stream())
        else:
            rc = lib.yh_yolo_decode_candidates(C.byref(d), conf, ml, None, P(cand), P(count), cap, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return cand, count.cpu()


def _two_pass(lib, p, na, no, s, scale, flip_w, ml, conf):
    """yh_yolo_decode_sxy, yh_tta_deaugment for a view, then yh_nms_candidates on the decoded tensor."""
    N, ny, nx, _ = p.shape
    rows = na * ny * nx
    io, _ = _decode(lib, p, na, no, s, False, rows + 10, 6)
    cap = rows * (no - 5)
    cand = torch.zeros(N, cap, 8, device=GPU)
    count = torch.zeros(N, dtype=torch.int32, device=GPU)
    with hiplib.on_device(p):
        if not (scale == 1.0 and flip_w < 0):
            assert lib.yh_tta_deaugment(P(io), N, rows + 10, no, 6, rows, scale, flip_w, _stream()) == 0
        assert lib.yh_nms_candidates(P(io), N, rows + 10, no - 5, conf, ml, None, P(cand), P(count), cap, _stream()) == 0
    torch.cuda.synchronize()
    return cand, count.cpu()


def _assert_same_records(a, b, what):
    (ca, na_), (cb, nb_) = a, b
    assert torch.equal(na_, nb_), (what, na_, nb_)
    for img in range(len(na_)):
        assert torch.equal(sc.sorted_records(ca, na_, img), sc.sorted_records(cb, nb_, img)), (what, img)


@pytest.mark.parametrize('ml', [0, 1], ids=['best-class', 'multi-label'])
@pytest.mark.parametrize('nc', [4, 81])
def test_candidates_at_scale_one_are_the_entries_they_extend(nc, ml):
    lib = hiplib.load()
    p, na, no, rows = _head(nc)
    p = p.to(GPU)
    conf = 0.5 if not ml else 0.25
    plain = _candidates(lib, p, na, no, None, 1.0, -1.0, ml, conf, 'plain')
    assert int(plain[1].min()) > 10
    _assert_same_records(_candidates(lib, p, na, no, 1.0, 1.0, -1.0, ml, conf, 'sxy'), plain, 'plain form')
    tta = _candidates(lib, p, na, no, None, 0.83, 80.0, ml, conf, 'tta')
    _assert_same_records(_candidates(lib, p, na, no, 1.0, 0.83, 80.0, ml, conf, 'sxy'), tta, 'tta form')


@pytest.mark.parametrize('form', ['plain', 'tta'])
@pytest.mark.parametrize('ml', [0, 1], ids=['best-class', 'multi-label'])
@pytest.mark.parametrize('s', sc.SCALES)
@pytest.mark.parametrize('nc', [4, 81])
def test_fused_filter_gives_the_records_of_decode_then_filter(nc, s, ml, form):
    """Bit for bit, after sorting by key: the fused pass against yh_yolo_decode_sxy (+ yh_tta_deaugment at scale 0.83, flip_w = W) +
    yh_nms_candidates.  The objectness threshold 0.5 keeps about half the rows (the logits are standard normal)."""
    lib = hiplib.load()
    p, na, no, rows = _head(nc)
    p = p.to(GPU)
    scale, flip_w = (1.0, -1.0) if form == 'plain' else (0.83, 80.0)       # W = nx * stride
    conf = 0.5 if not ml else 0.25
    fused = _candidates(lib, p, na, no, s, scale, flip_w, ml, conf, 'sxy')
    two = _two_pass(lib, p, na, no, s, scale, flip_w, ml, conf)
    print('fused filter nc %d s %g ml %d %s: %s records of %d rows' % (nc, s, ml, form, fused[1].tolist(), rows))
    assert rows // 4 < int(fused[1].min()) if not ml else int(fused[1].min()) > 10
    _assert_same_records(fused, two, (nc, s, ml, form))
    unscaled = _candidates(lib, p, na, no, 1.0, scale, flip_w, ml, conf, 'sxy')
    assert not torch.equal(sc.sorted_records(*fused, 0)[:, :4], sc.sorted_records(*unscaled, 0)[:, :4]) or \
        not torch.equal(fused[1], unscaled[1]), 'the scale moves the boxes'


# ------------------------------------------------------------------------------------------------ loss
def _loss_buffers(raw):
    shape = raw.shape[:4]
    return dict(tobj=torch.zeros(shape, device=GPU), winner=torch.full(shape, -1, dtype=torch.int32, device=GPU),
                sums=torch.zeros(3, device=GPU), count=torch.zeros(2, dtype=torch.int32, device=GPU),
                grad=torch.full_like(raw, float('nan')), scale=torch.tensor([7.0], device=GPU),
                anchors=torch.tensor(sc.ANCHORS_PX / sc.STRIDE, dtype=torch.float32, device=GPU), targets=sc.LABELS.to(GPU).contiguous())


def _loss_desc(raw, k):
    g = k['grad']
    return LossDesc(p=P(raw), grad=P(g), tobj=P(k['tobj']), winner=P(k['winner']), targets=P(k['targets']), anchors=P(k['anchors']),
                    sums=P(k['sums']), count=P(k['count']), scale=P(k['scale']), sb=raw.stride(0), sa=raw.stride(1), sy=raw.stride(2),
                    sx=raw.stride(3), gb=g.stride(0), ga=g.stride(1), gy=g.stride(2), gx=g.stride(3), bs=sc.BS, na=sc.NA, ny=sc.NY,
                    nx=sc.NX, no=sc.NC + 5, nc=sc.NC, nt=k['targets'].shape[0], iou_t=0.2, gr=0.6, cp=1.0, cn=0.0, cls_pw=1.3,
                    obj_pw=0.8, g_box=3.54, g_obj=64.3, g_cls=37.4)


@pytest.mark.parametrize('gamma', [0.0, 1.5])
@pytest.mark.parametrize('box', [0, 1, 2], ids=['giou', 'diou', 'ciou'])
def test_loss_at_scale_one_is_the_box_entries(box, gamma):
    """``yh_yolo_loss_head_*`` at 1.0 against ``yh_yolo_loss_box_*`` through the ABI, ``torch.equal``: both launch the same kernels, one
    workgroup each at this size, and no address receives more than two atomic adds on top of a zero."""
    lib = hiplib.load()
    raw = sc.raw_head(exact=True).to(GPU).contiguous()
    res = []
    for head in (False, True):
        k = _loss_buffers(raw)
        d = _loss_desc(raw, k)
        with hiplib.on_device(raw):
            if head:
                assert lib.yh_yolo_loss_head_fwd(C.byref(d), box, gamma, 0.25, 1.0, _stream()) == 0
                assert lib.yh_yolo_loss_head_bwd(C.byref(d), box, gamma, 0.25, 1.0, _stream()) == 0
            else:
                assert lib.yh_yolo_loss_box_fwd(C.byref(d), box, gamma, 0.25, _stream()) == 0
                assert lib.yh_yolo_loss_box_bwd(C.byref(d), box, gamma, 0.25, _stream()) == 0
        torch.cuda.synchronize()
        res.append(k)
    for name in ('tobj', 'sums', 'count', 'grad'):
        assert torch.equal(res[0][name], res[1][name]), name
    assert torch.isfinite(res[1]['grad']).all() and res[1]['grad'].abs().max() > 0 and res[1]['count'].tolist()[1] == 0


@functools.lru_cache(maxsize=None)
def _loss_reference(kind, s, gamma):
    return sc.loss_statement([sc.raw_head(exact=True)], sc.LABELS, sc.head_model(s, kind, gamma), [s])


@pytest.mark.parametrize('gamma', [0.0, 1.5])
@pytest.mark.parametrize('s', [1.2, 2.0])
@pytest.mark.parametrize('kind', ['giou', 'diou', 'ciou'])
def test_loss_kernels_match_the_fp64_statement(kind, s, gamma):
    """bs 2, na 3, a 4 x 5 grid, nc 3, 6 labels (tests/sxy_cases.py: one on a cell border, one at offset 0.999, two in one cell, one
    equal to its prediction).  Bounds of tests/test_gpu_box_loss.py: items ``rtol 1e-5, atol 1e-6``, gradient within 1e-4 of the largest
    magnitude.  At the four box logits of the exact match every min / max of the measure is a tie and its derivative a choice
    (autograd splits a tie, the kernel's chain takes the prediction's side): there the gradient is compared with the fp32 closed form
    of tests/fakelib_sxy.py to ``rtol 1e-5``, as test_exact_match_is_finite_and_follows_the_closed_form does."""
    model = sc.head_model(s, kind, gamma)
    raw = sc.raw_head(exact=True)
    bases, views = fc.nhwc_views([raw], GPU)
    hip_loss.flush_label_check()
    hip_loss.reset_scale_stats()
    loss, items = U.compute_loss(views, sc.LABELS.to(GPU), model)
    (loss * 7.0).backward()
    torch.cuda.synchronize()
    hip_loss.flush_label_check()
    assert hip_loss.scale_stats() == dict(scale_fwd=1, scale_bwd=1)
    na, no = raw.shape[1], raw.shape[4]
    full = bases[0].grad.cpu()
    assert full[..., na * no:].abs().max().item() == 0
    got = full[..., :na * no].view(sc.BS, sc.NY, sc.NX, na, no).permute(0, 3, 1, 2, 4).clone()
    ref_items, ref_grads = _loss_reference(kind, s, gamma)
    want = ref_grads[0].clone()
    b, a, gy, gx = sc.EXACT
    at_match = got[b, a, gy, gx, :4].clone()
    got[b, a, gy, gx, :4] = want[b, a, gy, gx, :4] = 0
    items = items.cpu()
    rel = ((got.double() - want).abs().max() / want.abs().max()).item()
    irel = ((items.double() - ref_items).abs() / ref_items.abs().clamp(min=1e-30)).max().item()
    print('loss %s s %g gamma %g: items %s (fp64 %s, relative %.2e), gradient distance / largest magnitude %.2e, at the exact match %s'
          % (kind, s, gamma, items.tolist(), ref_items.tolist(), irel, rel, at_match.tolist()))
    assert torch.isfinite(full).all() and torch.isfinite(items).all()
    fc.assert_close_to(items, [got], ref_items, [want], what=(kind, s, gamma))
    _, _, indices, _ = U.build_targets([raw], sc.LABELS, model)
    val, dval = fakelib_sxy.box_term(kind, raw[b, a, gy, gx, :4][None], torch.tensor([[2.0, 3.0]]), torch.tensor([[0.5, 0.5, 2.0, 3.0]]), s)
    assert val.item() == 1.0
    torch.testing.assert_close(at_match, -(7.0 * model.hyp['giou'] / len(indices[0][0])) * dval[0], rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------ end to end
def _v4tiny(**kw):
    torch.manual_seed(0)
    m = Darknet(V4TINY, (64, 64), **kw)
    m.load_state_dict(synth.trained_like_heads_(synth.randomize_bn_(m.state_dict(), seed=1), m.module_defs))
    return m.eval()


def test_engines_match_the_eager_modules_and_detect_is_nms_of_the_output():
    """yolov4-tiny with the flag, 64 px, batch 2.  fp32 engine: boxes within 1e-3 px and confidences within 1e-5 of the eager CPU
    modules; fp16: 0.5 px + 0.4 % of the box size, 5e-3 (the bounds of tests/test_gpu_network.py for this cfg).  ``hip_detect`` - the
    fused candidate pass on scaled heads - is NMS of ``model(x)[0]`` bit for bit, with ``YOLO_HIP_SCALE_XY=0`` (decode, then filter)
    too, and so is the augmented form against ``forward_augmented``; a hipGraph replay gives the bits of the plain replay."""
    model = _v4tiny(scale_x_y=True)
    plain = _v4tiny()
    x = synth.image_batch(2, 64, seed=33)
    with torch.no_grad():
        want, unscaled = model(x)[0], plain(x)[0]
    assert (want[..., :2] - unscaled[..., :2]).abs().max() > 1e-2, 'the scale moves the centres'
    model.cuda()
    xg = x.cuda()
    for precision in ('fp32', 'fp16'):
        model.hip_precision = precision
        with torch.no_grad():
            inf = model(xg)[0]
        torch.cuda.synchronize()
        eng = model.__dict__['_hip_engine']
        assert eng is not None and eng.precision == precision
        plan = eng._plan_for(xg)[1]
        assert sum(isinstance(d, DecodeSxyDesc) for d in plan['decode_descs']) == 2
        d = (inf.cpu() - want).abs()
        print('%s engine against the eager modules: boxes %.3e px, confidences %.3e' % (precision, d[..., :4].max().item(), d[..., 4:].max().item()))
        if precision == 'fp32':
            assert d[..., :4].max().item() <= 1e-3 and d[..., 4:].max().item() <= 1e-5
        else:
            bound = 0.5 + 0.004 * want[..., 2:4].abs().max(-1, keepdim=True)[0]
            assert (d[..., :4] <= bound).all() and d[..., 4:].max().item() <= 5e-3
    model.hip_precision = 'fp32'
    with torch.no_grad():
        inf = model(xg)[0].clone()
        conf = float(inf[..., 4].flatten().quantile(0.9))
        conf_ml = float((inf[..., 5:] * inf[..., 4:5]).flatten().topk(40).values[-1])
        for ml in (False, True):
            two = U.non_max_suppression(inf, conf_ml if ml else conf, 0.6, multi_label=ml)
            one = model.hip_detect(xg, conf_ml if ml else conf, 0.6, multi_label=ml)
            assert sum(0 if t is None else len(t) for t in two) >= 4
            for a, b in zip(one, two):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        eng = model.__dict__['_hip_engine']
        aug = U.non_max_suppression(eng.forward_augmented(xg), conf, 0.6, multi_label=False)
        for a, b in zip(model.hip_detect(xg, conf, 0.6, augment=True), aug):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        os.environ['YOLO_HIP_SCALE_XY'] = '0'
        try:
            for a, b in zip(model.hip_detect(xg, conf, 0.6), U.non_max_suppression(inf, conf, 0.6, multi_label=False)):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        finally:
            del os.environ['YOLO_HIP_SCALE_XY']
        eng.graph_max_batch = 2
        replay = model(xg)[0]
        torch.cuda.synchronize()
        assert torch.equal(replay, inf), 'hipGraph replay of a plan with YH_OP_DECODE_SXY'


def _step(model, x, targets, scales):
    """One HIP training step (fp32): (items, head gradients as (bs, na, ny, nx, no)), and the statement on the step's own raw heads."""
    dev = copy.deepcopy(model).to(GPU).train()
    dev.nc, dev.gr, dev.hyp = model.nc, model.gr, dict(model.hyp)
    pred, _ = dev(x.to(GPU))
    assert dev.__dict__.get('_hip_train_engine') is not None, 'the HIP training path did not engage'
    bases = [p._base for p in pred]
    for b in bases:
        b.retain_grad()
    loss, items = U.compute_loss(pred, targets.to(GPU), dev)
    (loss * 7.0).backward()
    torch.cuda.synchronize()
    hip_loss.flush_label_check()
    grads = []
    for p, b in zip(pred, bases):
        bs, na, ny, nx, no = p.shape
        grads.append(b.grad[..., :na * no].view(bs, ny, nx, na, no).permute(0, 3, 1, 2, 4).cpu())
    ref_items, ref_grads = sc.loss_statement([p.detach() for p in pred], targets, dev, scales)
    return items.cpu(), grads, ref_items, ref_grads


def test_training_step_with_the_flag(monkeypatch):
    """yolov4-tiny with the flag, 64 px, batch 2, one HIP training step (fp32): loss items and head gradients against the statement
    evaluated in fp64 on the step's own raw heads (bounds of the loss test); the scaled counter of engine.loss advances by one per
    head and pass.  With ``YOLO_HIP_SCALE_XY=0`` the same step takes the torch statement: same bounds, the counter does not move.
    No two labels share a cell, so torch's ``index_put`` on the GPU has no choice to make."""
    monkeypatch.setenv('YOLO_HIP_TRAIN_PRECISION', 'fp32')
    torch.manual_seed(0)
    model = Darknet(V4TINY, (64, 64), scale_x_y=True).train()
    model.nc, model.gr, model.hyp = 80, 1.0, dict(fc.HYP)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 64, 64, generator=g)
    targets = torch.tensor([[0, 3, 0.2, 0.2, 0.3, 0.35], [0, 11, 0.7, 0.7, 0.4, 0.3], [1, 0, 0.3, 0.7, 0.25, 0.3], [1, 79, 0.8, 0.2, 0.3, 0.5],
                            [1, 5, 0.5, 0.5, 0.9, 0.9]])      # the last one is large enough for the anchors of the stride-32 head
    scales = [model.module_list[i].scale_x_y for i in model.yolo_layers]
    assert scales == [1.05, 1.05]
    shapes = [torch.zeros(2, 3, 64 // st, 64 // st, 85) for st in (32, 16)]
    _, _, indices, _ = U.build_targets(shapes, targets, model)
    for idx in indices:
        cells = torch.stack(idx, 1)
        assert len(cells) and len(torch.unique(cells, dim=0)) == len(cells)
    hip_loss.reset_scale_stats()
    items, grads, ref_items, ref_grads = _step(model, x, targets, scales)
    assert hip_loss.scale_stats() == dict(scale_fwd=2, scale_bwd=2)
    rel = [((a.double() - b).abs().max() / b.abs().max()).item() for a, b in zip(grads, ref_grads)]
    print('training step: items %s (statement %s), head gradient distance / largest magnitude %s' % (items.tolist(), ref_items.tolist(), rel))
    fc.assert_close_to(items, grads, ref_items, ref_grads, what='fused')
    monkeypatch.setenv('YOLO_HIP_SCALE_XY', '0')
    items0, grads0, ref_items0, ref_grads0 = _step(model, x, targets, scales)
    assert hip_loss.scale_stats() == dict(scale_fwd=2, scale_bwd=2), 'the switch keeps the torch statement'
    fc.assert_close_to(items0, grads0, ref_items0, ref_grads0, what='torch statement')


def test_int8_engine_decodes_its_raw_heads_with_the_scale():
    """The repo's one calibrated COS-PTQ fixture is the mini detector of tests/ptq_minicfg.py (the reference cannot calibrate
    yolov4-tiny: max-pool and grouped routes), so the int8 check runs on that cfg with ``scale_x_y`` 1.05 / 1.2 written into its two
    ``[yolo]`` blocks: the int8 engine's decoded output is the host decode statement on the engine's own raw heads, within the
    decode bound ``rtol 2e-6, atol 2e-5 * s``."""
    import models
    import ptq_standin
    from ptq_minicfg import SIZE, mini_cfg
    ptq_standin.install()
    cfg = mini_cfg()
    want_s = [1.05, 1.2]
    for blk, s in zip([b for b in cfg if b['type'] == 'yolo'], want_s):
        blk['scale_x_y'] = str(s)
    torch.manual_seed(0)
    m = models.Darknet(cfg, (SIZE, SIZE), quantized=3, a_bit=8, w_bit=8, shortcut_way=1, scale_x_y=True)
    m = ptq_standin.load_fixture(m, np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ptq_mini.npz'))).eval()
    layers = [m.module_list[i] for i in m.yolo_layers]
    assert [l.scale_x_y for l in layers] == want_s
    m.cuda()
    x = synth.image_batch(2, SIZE, seed=7)
    with torch.no_grad():
        io, raws, _ = m(x.cuda())
    torch.cuda.synchronize()
    eng = m.__dict__['_hip_engine']
    assert eng is not None and eng.precision == 'int8'
    off = 0
    for raw, layer in zip(raws, layers):
        N, na, ny, nx, no = raw.shape
        rows = na * ny * nx
        want = sc.host_decode(raw.cpu(), (layer.anchor_vec.cpu() * layer.stride).numpy(), layer.stride, layer.scale_x_y, no - 5)
        got = io[:, off:off + rows].cpu()
        print('int8 head at stride %d, s %g: largest distance %.3e' % (layer.stride, layer.scale_x_y, (got - want).abs().max().item()))
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-6, atol=2e-5 * layer.scale_x_y)
        plain = sc.host_decode(raw.cpu(), (layer.anchor_vec.cpu() * layer.stride).numpy(), layer.stride, 1.0, no - 5)
        assert (want[..., :2] - plain[..., :2]).abs().max() > 1e-2, 'the scale moves the centres'
        off += rows
