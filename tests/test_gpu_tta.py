"""GPU tier of augmented inference (``--augment``): the view kernel against the resize kernel and the host emulation, the fused call
against the NMS of a composed tensor whose de-augmentation was done on the HOST (IEEE fp32 division - the device kernels are pinned
to correctly rounded division through it), the two-pass form, the int8 engine and the plan-count fall-back."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fakelib_tta
import synth
from test_oracle_golden import build_mirror
from test_tta import CFGS, _assert_every_view_contributes, _kept, _thresholds, frames, view_rows

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (160, 160), (256, 256), (160, 256)]
CASES = [(c, hw, p) for c in CFGS for hw in SIZES for p in ('fp16', 'fp32')]
IDS = ['%s-%dx%d-%s' % (c, hw[0], hw[1], p) for c, hw, p in CASES]
BATCH = 5
_cache = {}


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _same_bits(a, b, tag):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), '%s img %d' % (tag, i)
        if p is not None:
            assert p.shape == q.shape and torch.equal(p.view(torch.int32), q.view(torch.int32)), '%s img %d' % (tag, i)


def composed_on_host(eng, x):
    """``model(x, augment=True)[0]`` from the engine's per-group forwards with the de-augmentation in numpy fp32 on the host."""
    x, views, inputs = eng._tta_inputs(x)
    n, w = x.shape[0], x.shape[3]
    parts = [None] * len(views)
    for members, xg in inputs:
        io = eng(xg)[0].cpu().numpy()
        for j, k in enumerate(members):
            part = io[j * n:(j + 1) * n].copy()
            if k:
                fakelib_tta.deaugment_rows(part, np.float32(views[k][0]), float(w) if views[k][1] else -1.0)
            parts[k] = part
    return torch.from_numpy(np.concatenate(parts, 1)).to(x.device)


def _case(cfg_dir, which, hw, precision):
    """Model on the GPU with its engine, frames and the host-composed tensor of one case (computed once, shared, never modified)."""
    key = (which, hw, precision)
    if key not in _cache:
        from engine.plan import DarknetEngine
        if which not in _cache:
            _cache[which] = build_mirror(cfg_dir, CFGS[which], 256).cuda()
        model = _cache[which]
        model.hip_precision = precision
        eng = model.__dict__['_hip_engine'] = DarknetEngine(model, precision=precision)
        x = frames(BATCH, hw, seed=41 + hw[0] + hw[1]).cuda()
        with torch.no_grad():
            composed = composed_on_host(eng, x)
        _cache[key] = (model, x, eng, composed, view_rows(composed.shape[1], model, hw))
    model, x, eng, composed, ranges = _cache[key]
    model.hip_precision = precision
    model.__dict__['_hip_engine'] = eng
    return _cache[key]


# ------------------------------------------------------------------------------------------------ (a) the view kernel
@pytest.mark.parametrize('hw', SIZES + [(96, 96), (224, 224)], ids=lambda hw: '%dx%d' % hw)
def test_view_kernel_equals_resize_of_the_flipped_frame_plus_pad_and_the_emulation(hw):
    from engine import hiplib
    from engine.plan import DarknetEngine, tta_views
    from engine.preprocess import resize_bilinear
    x = frames(BATCH, hw, seed=3)
    views = tta_views(*hw)
    dev, host = DarknetEngine.__new__(DarknetEngine), DarknetEngine.__new__(DarknetEngine)
    dev.lib, host.lib = hiplib.load(), fakelib_tta.FakeLibTta()
    _, _, on_dev = dev._tta_inputs(x.cuda())
    _, _, on_host = host._tta_inputs(x)
    torch.cuda.synchronize()
    for (members, xg), (_, xh) in zip(on_dev, on_host):
        assert torch.equal(xg.cpu().view(torch.int32), xh.view(torch.int32)), 'device view vs host emulation, views %s' % members
        for j, k in enumerate(members):
            s, flip, rh, rw, oh, ow = views[k]
            got = xg[BATCH * j:BATCH * (j + 1)]
            src = x.cuda().flip(3).contiguous() if flip else x.cuda()
            want = F.pad(resize_bilinear(src, (rh, rw)), [0, ow - rw, 0, oh - rh], value=0.447)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), 'view %d' % k


def test_identity_view_returns_the_input_bits_on_the_device():
    from engine import hiplib
    x = (torch.randn(2, 3, 33, 131) * 100).cuda()
    out = torch.full((2, 3, 64, 192), 7.0).cuda()
    d = hiplib.TtaViewDesc(src=hiplib.ptr(x), dst=hiplib.ptr(out), n=2, c=3, ih=33, iw=131, oh=64, ow=192, rh=33, rw=131, flip=0,
                           scale_h=1.0, scale_w=1.0, pad_value=0.447)
    hiplib.check(hiplib.load().yh_tta_view(C.byref(d), hiplib.stream_ptr()), 'yh_tta_view')
    torch.cuda.synchronize()
    assert torch.equal(out[:, :, :33, :131].contiguous().view(torch.int32), x.view(torch.int32))
    pad = torch.tensor(0.447, dtype=torch.float32).item()
    assert bool((out[:, :, 33:] == pad).all()) and bool((out[:, :, :, 131:] == pad).all())


# ------------------------------------------------------------------------------------------------ (b) fused against composed
@pytest.mark.parametrize('which,hw,precision', CASES, ids=IDS)
def test_fused_call_equals_nms_of_the_host_composed_tensor(which, hw, precision, cfg_dir, monkeypatch):
    from engine import nms as hnms
    model, x, eng, composed, ranges = _case(cfg_dir, which, hw, precision)
    nc = composed.shape[2] - 5
    with torch.no_grad():
        # the two-pass form's device de-augmentation against the host's division, bit for bit
        assert torch.equal(eng.forward_augmented(x).view(torch.int32), composed.view(torch.int32)), 'yh_tta_deaugment vs IEEE division'
        for ml in (False, True):
            conf = _thresholds(composed.cpu(), ml, 1000 if ml and nc > 1 else 500)
            _assert_every_view_contributes(composed.cpu(), conf, ranges, ml)
            monkeypatch.setattr(hnms, '_density', {})
            two = hnms.non_max_suppression(composed, conf, 0.6, multi_label=ml)
            assert _kept(two) >= 20
            one = model.hip_detect(x, conf, 0.6, multi_label=ml, augment=True)
            _same_bits(one, two, 'fused vs composed, ml %s' % ml)
            if nc > 1:
                pick = [0, nc - 1, 17]
                _same_bits(model.hip_detect(x, conf, 0.6, multi_label=ml, classes=pick, augment=True),
                           hnms.non_max_suppression(composed, conf, 0.6, multi_label=ml, classes=pick), 'class filter, ml %s' % ml)
            # image chunks: two images per pass (tests/test_gpu_nms.py:244)
            mmax = int(max(max(v) for v in hnms._density.values()) * composed.shape[1]) + 1
            cap = hnms._pow2_at_least(mmax)
            monkeypatch.setattr(hnms, '_density', {})
            monkeypatch.setattr(hnms, '_WORK_BUDGET', 2 * (cap * ((cap + 63) // 64) * 8 + cap * 23 * 4 + 14 * cap) + 4096)
            _same_bits(model.hip_detect(x, conf, 0.6, multi_label=ml, augment=True), two, 'image chunks, ml %s' % ml)
            monkeypatch.undo()
        # no density history and more than 256 candidates in an image: the first bound overflows, the candidate pass repeats
        conf = _thresholds(composed.cpu(), True, 2500 if nc > 1 else 10 ** 9)
        monkeypatch.setattr(hnms, '_density', {})
        two = hnms.non_max_suppression(composed, conf, 0.6, multi_label=True)
        if max(hnms._density[1 if nc > 1 else 0]) * composed.shape[1] > 256:      # one class at 64 x 64 has 180 rows per image
            monkeypatch.setattr(hnms, '_density', {})
            _same_bits(model.hip_detect(x, conf, 0.6, multi_label=True, augment=True), two, 'after the retry')
        else:
            assert nc == 1 and hw == (64, 64)


@pytest.mark.parametrize('ml', [0, 1])
def test_neutral_transform_gives_the_plain_entry_s_records_on_the_device(ml, cfg_dir):
    from engine import hiplib
    from engine.plan import SLOT_INPUT
    model, x, eng, composed, _ = _case(cfg_dir, 'tiny', (160, 160), 'fp16')
    lib = hiplib.load()
    x, plan = eng._plan_for(x)
    lib.yh_plan_bind_slot(plan['handle'], SLOT_INPUT, x.data_ptr())
    hiplib.check(lib.yh_plan_run_range(plan['handle'], 0, plan['first_decode_op'], hiplib.stream_ptr()), 'run')
    conf = _thresholds(composed.cpu(), bool(ml), 1000)
    cap = 8192
    out = []
    for tta in (False, True):
        cand = torch.zeros(BATCH, cap, 8, device='cuda')
        count = torch.zeros(BATCH, dtype=torch.int32, device='cuda')
        for d in plan['decode_descs']:
            if tta:
                rc = lib.yh_yolo_decode_candidates_tta(C.byref(d), 1.0, -1.0, conf, ml, None, hiplib.ptr(cand), hiplib.ptr(count), cap,
                                                       hiplib.stream_ptr())
            else:
                rc = lib.yh_yolo_decode_candidates(C.byref(d), conf, ml, None, hiplib.ptr(cand), hiplib.ptr(count), cap, hiplib.stream_ptr())
            hiplib.check(rc, 'candidates')
        torch.cuda.synchronize()
        out.append((cand.cpu(), count.cpu()))
    assert int(out[0][1].sum()) >= 20 and int(out[0][1].max()) <= cap and torch.equal(out[0][1], out[1][1])
    for i in range(BATCH):      # slots are handed out by an atomic cursor: compare the records as sets, ordered by their unique keys
        m = int(out[0][1][i])
        a, b = (o[0][i, :m].view(torch.int32) for o in out)
        assert torch.equal(a[a[:, 6].argsort()], b[b[:, 6].argsort()]), 'img %d' % i


# ------------------------------------------------------------------------------------------------ (c) against the eager modules
@pytest.mark.parametrize('which,hw', [(c, hw) for c in CFGS for hw in SIZES], ids=['%s-%dx%d' % (c, hw[0], hw[1]) for c in CFGS for hw in SIZES])
def test_forward_augmented_against_the_eager_cpu_modules(which, hw, cfg_dir):
    model, x, eng, composed, _ = _case(cfg_dir, which, hw, 'fp32')
    cpu = build_mirror(cfg_dir, CFGS[which], 256)
    with torch.no_grad():
        want = cpu(x.cpu(), augment=True)[0]
        got = eng.forward_augmented(x).cpu()
    assert got.shape == want.shape
    d = (got - want).abs()
    print('%s %s: box drift %.3g px, conf drift %.3g' % (which, hw, d[..., :4].max().item(), d[..., 4:].max().item()))
    assert d[..., :4].max().item() <= 2e-3, 'TTA box drift %g px' % d[..., :4].max().item()
    assert d[..., 4:].max().item() <= 2e-5, 'TTA conf drift %g' % d[..., 4:].max().item()


# ------------------------------------------------------------------------------------------------ (d) the int8 engine
def test_augmented_detection_on_the_int8_engine(monkeypatch):
    from engine import nms as hnms
    from test_ptq import build_qmodel
    from ptq_minicfg import SIZE
    m, _ = build_qmodel()
    x = synth.image_batch(BATCH, SIZE, seed=7).cuda()
    m.cuda()
    with torch.no_grad():
        m(x)
        eng = m.__dict__['_hip_engine']
        assert eng.precision == 'int8'
        composed = composed_on_host(eng, x)
        conf = float(composed[..., 4].flatten().quantile(0.9)) * 0.999
        monkeypatch.setattr(hnms, '_density', {})
        two = hnms.non_max_suppression(composed, conf, 0.6, multi_label=False)
        assert _kept(two) >= 5
        _same_bits(m.hip_detect(x, conf, 0.6, augment=True), two, 'int8 fused vs composed')
        assert m.__dict__['_hip_engine'] is eng


# ------------------------------------------------------------------------------------------------ (e) fewer plans than groups
def test_one_resident_plan_takes_the_two_pass_form(cfg_dir, monkeypatch):
    from engine import nms as hnms
    from engine.plan import DarknetEngine
    model, x, eng, composed, _ = _case(cfg_dir, 'tiny', (160, 256), 'fp16')
    conf = _thresholds(composed.cpu(), False, 500)
    monkeypatch.setattr(hnms, '_density', {})
    two = hnms.non_max_suppression(composed, conf, 0.6, multi_label=False)
    monkeypatch.setenv('YOLO_HIP_MAX_PLANS', '1')
    small = DarknetEngine(model, precision='fp16')
    calls = []
    lib = small.lib
    monkeypatch.setattr(small, 'forward_augmented', lambda t: (calls.append(1), DarknetEngine.forward_augmented(small, t))[1])
    with torch.no_grad():
        got = small.detect(x, conf, 0.6, augment=True)
    assert calls == [1] and len(small._plans) == 1 and lib is eng.lib
    _same_bits(got, two, 'one plan')
    assert _kept(got) >= 20
