"""CPU tier of augmented inference (``--augment``: the frame, a flipped 0.83x view and a 0.67x view; reference models.py:477-506):
the views, their grouping into shared forwards, the de-augmentation inside the candidate pass and the two-pass form, replayed through
the host emulation of the C ABI (tests/fakelib_tta.py) against the eager modules; the header / binding of the three entries against
the compiler; the wiring of test.py and detect.py.  The kernels themselves are checked on the GPU tier (tests/test_gpu_tta.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fakelib_multiscale
import fakelib_tta
from engine import hiplib
from test_abi import HEADER, REPO, _declared
from test_oracle_golden import build_mirror

CFGS = {'tiny': 'yolov3tiny/yolov3-tiny.cfg', 'tiny-hand': 'yolov3tiny/yolov3-tiny-hand.cfg'}
# (h, w) -> indices of the views that share a forward
SIZES = {(64, 64): [[0, 1, 2]], (96, 96): [[0], [1, 2]], (160, 160): [[0], [1], [2]], (224, 224): [[0], [1, 2]], (256, 256): [[0, 1], [2]],
         (160, 256): [[0], [1], [2]]}
CASES = [(c, hw) for c in CFGS for hw in SIZES]
IDS = ['%s-%dx%d' % (c, hw[0], hw[1]) for c, hw in CASES]
BATCH = 3
_cache = {}
LIB = fakelib_tta.FakeLibTta()      # one emulated library: the engines of the cases and engine/nms.py record their calls on it


def frames(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, hw[0], hw[1], generator=g)


def _model(cfg_dir, which):
    if which not in _cache:
        _cache[which] = build_mirror(cfg_dir, CFGS[which], 256)
    return _cache[which]


def view_rows(io_rows, model, hw):
    """Row ranges of the three views inside the concatenated tensor: [(first, last), ...]."""
    from engine.plan import tta_views
    strides = [int(model.module_list[i].stride) for i in model.yolo_layers]
    na = [int(model.module_list[i].na) for i in model.yolo_layers]
    edges = [0]
    for v in tta_views(*hw):
        edges.append(edges[-1] + sum(a * (v[4] // s) * (v[5] // s) for a, s in zip(na, strides)))
    assert edges[-1] == io_rows
    return list(zip(edges[:-1], edges[1:]))


def _case(cfg_dir, which, hw):
    """Model, frames, the engine on the emulated ABI and the composed tensor of one case (computed once, shared, never modified)."""
    key = (which, hw)
    if key not in _cache:
        from engine.plan import DarknetEngine
        model = _model(cfg_dir, which)
        x = frames(BATCH, hw, seed=41 + hw[0] + hw[1])
        eng = DarknetEngine(model, precision='fp32', lib=LIB)
        composed = eng.forward_augmented(x)
        _cache[key] = (model, x, LIB, eng, composed, view_rows(composed.shape[1], model, hw))
    return _cache[key]


@pytest.fixture()
def fake(monkeypatch):
    from engine import nms as hnms
    monkeypatch.setattr(hiplib, 'load', lambda: LIB)
    monkeypatch.setattr(hnms, '_density', {})
    del LIB.calls[:]
    return LIB


def _same_bits(a, b, tag):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), '%s img %d' % (tag, i)
        if p is not None:
            assert p.shape == q.shape and p.numpy().tobytes() == q.numpy().tobytes(), '%s img %d' % (tag, i)


def _kept(dets):
    return sum(0 if d is None else d.shape[0] for d in dets)


def _thresholds(composed, ml, rows_wanted):
    """conf by a quantile of the scores, as tests/test_nms_host.py picks it: about ``rows_wanted`` candidates over the batch."""
    nc = composed.shape[2] - 5
    if ml and nc > 1:
        return float((composed[..., 5:] * composed[..., 4:5]).flatten().topk(rows_wanted).values[-1])
    flat = composed[..., 4].flatten()
    return float(flat.topk(min(rows_wanted, flat.numel() // 2)).values[-1]) * 0.9999


def _assert_every_view_contributes(composed, conf, ranges, ml):
    """At least one row of every view passes the candidate filter (csrc/nms.hip: best class tests the objectness alone)."""
    for k, (a, b) in enumerate(ranges):
        part = composed[:, a:b]
        score = (part[..., 5:] * part[..., 4:5]).max(-1).values if ml and composed.shape[2] > 6 else part[..., 4]
        live = (part[..., 4] > conf) & (score > conf) & (part[..., 2] > 2) & (part[..., 3] > 2)
        assert int(live.sum()) >= 1, 'no candidate row inside view %d: the case is vacuous' % k


# ------------------------------------------------------------------------------------------------ (a), (b) the views
def _views_of(x):
    """[(view index, (ratio, flip, rh, rw, oh, ow), the emulated view)] of a batch, and the grouping the engine chose."""
    from engine.plan import DarknetEngine, tta_views
    views = tta_views(*x.shape[2:])
    eng = DarknetEngine.__new__(DarknetEngine)      # _tta_inputs reads the library handle only
    eng.lib = fakelib_tta.FakeLibTta()
    _, _, inputs = eng._tta_inputs(x)
    n = x.shape[0]
    out = []
    for members, xg in inputs:
        assert xg.shape[0] == len(members) * n
        out += [(k, views[k], xg[n * j:n * (j + 1)]) for j, k in enumerate(members)]
    return out, [m for m, _ in inputs]


@pytest.mark.parametrize('hw', list(SIZES), ids=['%dx%d' % hw for hw in SIZES])
def test_view_emulation_is_the_resize_of_the_flipped_frame_plus_the_pad(hw):
    from engine.plan import tta_groups, tta_views
    from engine.preprocess import resize_bilinear
    x = frames(2, hw, seed=3)
    assert tta_groups(tta_views(*hw)) == SIZES[hw]
    got_views, groups = _views_of(x)
    assert groups == SIZES[hw]
    for k, (s, flip, rh, rw, oh, ow), got in got_views:
        if k == 0:
            assert got.numpy().tobytes() == x.numpy().tobytes(), 'the frame itself must keep its bits'
            continue
        src = x.flip(3).contiguous() if flip else x
        want = F.pad(resize_bilinear(src, (rh, rw), lib=fakelib_multiscale.FakeLibMultiscale()), [0, ow - rw, 0, oh - rh], value=0.447)
        assert got.shape == want.shape and got.numpy().tobytes() == want.numpy().tobytes(), 'view %d' % k


@pytest.mark.parametrize('hw', list(SIZES), ids=['%dx%d' % hw for hw in SIZES])
def test_view_emulation_is_as_close_to_scale_img_as_torch_fp32_is_to_float64(hw):
    """Distance of the view's fp32 arithmetic to ``torch_utils.scale_img`` in fp32 <= distance of that fp32 result to ``scale_img`` in
    float64 (the criterion of tests/test_multiscale.py:113), on frames of the kind the views are built from: detect.py and test.py
    feed ``uint8 / 256`` (detect.py:64, test.py:134), i.e. values on the k / 256 grid (``synth.dyadic_frames``).

    Why the grid matters: the 0.67x view of a 96 px frame has a 64 px content, the scale is exactly 1.5 and every tap weight is 0.25
    or 0.75.  On grid frames every product and sum of that view is then exact in fp32 - ours, torch's and the float64 evaluation
    agree in every bit of the content (distance 0; torch's 3.1e-09 is the border value 0.447 in float against double) - and the
    other views keep inexact weights, so the comparison stays a comparison of roundings there.  With full-mantissa ``torch.rand``
    frames the criterion cannot hold for that one view whatever unfused arithmetic is used: torch's only error is then the rounding
    of its contracted sums (|torch fp32 - float64| 9.7e-08 ... 1.12e-07 over seeds 0-5), and two fp32 results within an ulp of the
    true value can be two ulps apart (|ours - torch fp32| 1.19e-07 every time; |ours - float64| 1.12e-07 ... 1.19e-07)."""
    import synth
    from utils import torch_utils
    x = synth.dyadic_frames(frames(2, hw, seed=3))
    for k, (s, flip, rh, rw, oh, ow), got in _views_of(x)[0][1:]:
        src = x.flip(3) if flip else x
        t32 = torch_utils.scale_img(src, s, same_shape=False)
        t64 = torch_utils.scale_img(src.double(), s, same_shape=False)
        assert t32.shape == got.shape
        ours = (got.double() - t32.double()).abs().max().item()
        torchs = (t32.double() - t64).abs().max().item()
        print('view %d of %s: |ours - torch fp32| %.3g, |torch fp32 - float64| %.3g' % (k, hw, ours, torchs))
        assert ours <= torchs, 'view %d of %s: |ours - torch fp32| %.3g > |torch fp32 - float64| %.3g' % (k, hw, ours, torchs)


def test_identity_view_returns_the_input_bits():
    x = torch.randn(2, 3, 33, 47) * 100
    out = torch.full((2, 3, 64, 64), 7.0)
    d = hiplib.TtaViewDesc(src=hiplib.ptr(x), dst=hiplib.ptr(out), n=2, c=3, ih=33, iw=47, oh=64, ow=64, rh=33, rw=47, flip=0, scale_h=1.0,
                           scale_w=1.0, pad_value=0.447)
    assert fakelib_tta.FakeLibTta().yh_tta_view(C.byref(d), None) == 0
    assert out[:, :, :33, :47].contiguous().numpy().tobytes() == x.numpy().tobytes()
    assert bool((out[:, :, 33:] == np.float32(0.447)).all()) and bool((out[:, :, :, 47:] == np.float32(0.447)).all())


# ------------------------------------------------------------------------------------------------ (c) the composed tensor
@pytest.mark.parametrize('which,hw', CASES, ids=IDS)
def test_forward_augmented_against_the_eager_modules(which, hw, cfg_dir):
    model, x, lib, eng, composed, ranges = _case(cfg_dir, which, hw)
    with torch.no_grad():
        want, none_ = model(x, augment=True)
    assert none_ is None and composed.shape == want.shape
    assert len(eng._plans) == len(SIZES[hw]), 'views of equal padded shape share one plan'
    d = (composed - want).abs()
    print('%s %s: box drift %.3g px, conf drift %.3g' % (which, hw, d[..., :4].max().item(), d[..., 4:].max().item()))
    assert d[..., :4].max().item() <= 2e-3, 'TTA box drift %g px' % d[..., :4].max().item()
    assert d[..., 4:].max().item() <= 2e-5, 'TTA conf drift %g' % d[..., 4:].max().item()


# ------------------------------------------------------------------------------------------------ (d) fused against composed
@pytest.mark.parametrize('ml', [False, True], ids=['best-class', 'multi-label'])
@pytest.mark.parametrize('which,hw', CASES, ids=IDS)
def test_fused_detect_equals_nms_of_the_composed_tensor(which, hw, ml, cfg_dir, fake, monkeypatch):
    from engine import nms as hnms
    model, x, lib, eng, composed, ranges = _case(cfg_dir, which, hw)
    nc = composed.shape[2] - 5
    conf = _thresholds(composed, ml, 600 if ml and nc > 1 else 300)
    _assert_every_view_contributes(composed, conf, ranges, ml)
    two = hnms.non_max_suppression(composed.clone(), conf, 0.6, multi_label=ml)
    assert _kept(two) >= 20
    del lib.calls[:]
    one = eng.detect(x, conf, 0.6, multi_label=ml, augment=True)
    heads = 3 * len(model.yolo_layers)
    assert lib.calls.count('decode_candidates_tta') == heads and 'tta_deaugment' not in lib.calls and 'decode_candidates' not in lib.calls
    assert len(eng._plans) == len(SIZES[hw])
    _same_bits(one, two, 'fused vs composed')
    if nc > 1:
        pick = [0, nc - 1, 17]
        _same_bits(eng.detect(x, conf, 0.6, multi_label=ml, classes=pick, augment=True),
                   hnms.non_max_suppression(composed.clone(), conf, 0.6, multi_label=ml, classes=pick), 'class filter')
    # image chunks: a budget of two images per pass (tests/test_gpu_nms.py:244); the transforms must travel with the narrowed heads
    mmax = int(max(max(v) for v in hnms._density.values()) * composed.shape[1]) + 1
    cap = hnms._pow2_at_least(mmax)
    monkeypatch.setattr(hnms, '_density', {})
    monkeypatch.setattr(hnms, '_WORK_BUDGET', 2 * (cap * ((cap + 63) // 64) * 8 + cap * 23 * 4 + 14 * cap) + 64)
    del lib.calls[:]
    _same_bits(eng.detect(x, conf, 0.6, multi_label=ml, augment=True), two, 'image chunks')
    assert lib.calls.count('decode_candidates_tta') >= heads * 3, 'a count pass and at least two chunks'
    monkeypatch.undo()
    # the two-pass form behind the same call: switched off, and with fewer plans than groups
    monkeypatch.setattr(hiplib, 'load', lambda: lib)
    monkeypatch.setenv('YOLO_HIP_FUSED_DETECT', '0')
    del lib.calls[:]
    _same_bits(eng.detect(x, conf, 0.6, multi_label=ml, augment=True), two, 'switched off')
    assert 'decode_candidates_tta' not in lib.calls and lib.calls.count('tta_deaugment') == 2


OVERFLOW = [(c, hw) for c, hw in CASES if c == 'tiny' or hw[0] >= 160]


@pytest.mark.parametrize('which,hw', OVERFLOW, ids=['%s-%dx%d' % (c, hw[0], hw[1]) for c, hw in OVERFLOW])
def test_an_overflowing_first_bound_repeats_the_candidate_pass_on_intact_heads(which, hw, cfg_dir, fake, monkeypatch):
    """More than 256 candidates in an image and no density history: the first bound overflows and the candidate pass runs again -
    on head buffers that a second run of a shared plan would have overwritten."""
    from engine import nms as hnms
    model, x, lib, eng, composed, ranges = _case(cfg_dir, which, hw)
    nc = composed.shape[2] - 5
    conf = _thresholds(composed, True, 1500 if nc > 1 else 10 ** 9)
    two = hnms.non_max_suppression(composed.clone(), conf, 0.6, multi_label=True)
    most = max(hnms._density[1 if nc > 1 else 0]) * composed.shape[1]
    assert most > 256 and _kept(two) >= 20
    _assert_every_view_contributes(composed, conf, ranges, True)
    monkeypatch.setattr(hnms, '_density', {})
    del lib.calls[:]
    one = eng.detect(x, conf, 0.6, multi_label=True, augment=True)
    assert lib.calls.count('decode_candidates_tta') == 2 * 3 * len(model.yolo_layers), 'the pass was expected to repeat once'
    _same_bits(one, two, 'after the retry')


def test_fewer_plans_than_groups_takes_the_two_pass_form(cfg_dir, fake, monkeypatch):
    from engine import nms as hnms
    from engine.plan import DarknetEngine
    model, x, _, _, composed, _ = _case(cfg_dir, 'tiny-hand', (160, 256))
    monkeypatch.setenv('YOLO_HIP_MAX_PLANS', '1')
    eng = DarknetEngine(model, precision='fp32', lib=fake)
    conf = _thresholds(composed, False, 300)
    got = eng.detect(x, conf, 0.6, augment=True)
    assert 'decode_candidates_tta' not in fake.calls and fake.calls.count('tta_deaugment') == 2 and len(eng._plans) == 1
    _same_bits(got, hnms.non_max_suppression(composed.clone(), conf, 0.6, multi_label=False), 'one plan')


def test_keys_beyond_int32_are_refused(cfg_dir, fake, monkeypatch):
    from engine.plan import DarknetEngine
    model, x, _, _, _, _ = _case(cfg_dir, 'tiny', (64, 64))
    eng = DarknetEngine(model, precision='fp32', lib=fake)
    build = eng._build_plan

    def huge(*a):
        plan = build(*a)
        plan['rows'] = 1 << 26
        return plan
    monkeypatch.setattr(eng, '_build_plan', huge)
    with pytest.raises(ValueError, match='32-bit'):
        eng.detect(x, 0.5, 0.6, augment=True)


# ------------------------------------------------------------------------------------------------ (e) the neutral transform
@pytest.mark.parametrize('ml', [0, 1])
def test_neutral_transform_gives_the_plain_entry_s_records(ml, cfg_dir):
    from engine.plan import SLOT_INPUT
    model, x, lib, eng, composed, _ = _case(cfg_dir, 'tiny', (160, 160))
    x, plan = eng._plan_for(x)
    lib.yh_plan_bind_slot(plan['handle'], SLOT_INPUT, x.data_ptr())
    assert lib.yh_plan_run_range(plan['handle'], 0, plan['first_decode_op'], None) == 0
    conf = _thresholds(composed, bool(ml), 600)
    cap = 4096
    out = []
    for tta in (False, True):
        cand = torch.zeros(BATCH, cap, 8)
        count = torch.zeros(BATCH, dtype=torch.int32)
        for d in plan['decode_descs']:
            if tta:
                rc = lib.yh_yolo_decode_candidates_tta(C.byref(d), 1.0, -1.0, conf, ml, None, hiplib.ptr(cand), hiplib.ptr(count), cap, None)
            else:
                rc = lib.yh_yolo_decode_candidates(C.byref(d), conf, ml, None, hiplib.ptr(cand), hiplib.ptr(count), cap, None)
            assert rc == 0
        out.append((cand, count))
    assert int(out[0][1].sum()) >= 20 and int(out[0][1].max()) <= cap
    assert torch.equal(out[0][1], out[1][1]) and out[0][0].numpy().tobytes() == out[1][0].numpy().tobytes()


# ------------------------------------------------------------------------------------------------ (f) header and binding
def test_header_binding_and_library_agree_on_the_new_entries(tmp_path):
    names = ('yh_tta_view', 'yh_yolo_decode_candidates_tta', 'yh_tta_deaugment')
    declared = _declared()
    lib = hiplib.load()
    for n in names:
        assert n in declared and n in hiplib.EXPORTS and hasattr(lib, n), n
    assert sorted(hiplib.EXPORTS) == declared
    assert lib.yh_abi_version() == 2 == hiplib.ABI_VERSION
    text = open(HEADER).read()
    assert 'yh_decode_desc* d, float scale, float flip_w, float conf_thres, int multi_label' in ' '.join(text.split())
    cls, cname = hiplib.TtaViewDesc, 'yh_tta_view_desc'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolo_hip.h"', 'int main(void){', 'printf("size %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(REPO, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['size']) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname
    # the entries check their arguments on the host: nothing is launched for a bad descriptor
    bad = hiplib.TtaViewDesc(n=1, c=1, ih=4, iw=4, oh=4, ow=4, rh=5, rw=4, flip=0, scale_h=1.0, scale_w=1.0, pad_value=0.0)
    bad.src = bad.dst = 4096
    assert lib.yh_tta_view(C.byref(bad), None) != 0
    assert lib.yh_tta_deaugment(4096, 1, 10, 6, 8, 4, 0.83, -1.0, None) != 0


# ------------------------------------------------------------------------------------------------ (g) the scripts
def _detections(dets):
    return [None if d is None else d.detach().cpu().numpy().copy() for d in dets]


def test_scripts_route_augment_through_hip_detect(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    """test.py --augment and detect.py --augment call hip_detect(augment=True) - one call per batch; YOLO_HIP_TTA=0 keeps the two
    calls, with the same detections.  On the CPU hip_detect(augment=True) is those two eager calls."""
    import models
    import detect as detect_mod
    import test as test_mod
    from utils import utils as uu
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    m = models.Darknet(tiny_cfg, (64, 64))
    torch.save({'model': m.state_dict()}, 'w.pt')
    x = frames(2, (64, 64), seed=9)
    m.eval()
    with torch.no_grad():
        inf = m(x, augment=True)[0]
        conf = float(inf[..., 4].flatten().quantile(0.5))
        _same_bits(m.hip_detect(x, conf, 0.6, multi_label=True, augment=True), uu.non_max_suppression(inf, conf, 0.6, multi_label=True),
                   'eager hip_detect')
    src = tmp_path / 'four'
    src.mkdir()
    for line in open(dataset_dir / 'valid.txt').read().split():
        shutil.copy(line, src)
    assert len(os.listdir(src)) == 4

    fused, seen = [], {}
    orig = models.Darknet.hip_detect

    def counted(self, *a, **k):
        out = orig(self, *a, **k)
        fused.append(bool(k.get('augment')))
        seen.setdefault('dets', []).extend(_detections(out))
        return out
    monkeypatch.setattr(models.Darknet, 'hip_detect', counted)
    for mod in (test_mod, detect_mod):
        nms = mod.non_max_suppression

        def recorded(*a, _nms=nms, **k):
            out = _nms(*a, **k)
            seen.setdefault('dets', []).extend(_detections(out))
            return out
        monkeypatch.setattr(mod, 'non_max_suppression', recorded)

    def run_test():
        test_mod.opt = None
        seen.clear()
        del fused[:]
        res = test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), 'w.pt', batch_size=2, imgsz=64, plot=False, augment=True)
        return res, list(fused), seen.pop('dets')

    def run_detect():
        seen.clear()
        del fused[:]
        dopt = detect_mod.make_parser().parse_args(['--cfg', tiny_cfg, '--weights', 'w.pt', '--source', str(src), '--output', 'out',
                                                    '--img-size', '64', '--conf-thres', '0.001', '--device', 'cpu', '--augment',
                                                    '--names', str(dataset_dir / 'synth.names')])
        res = detect_mod.detect(dopt, save_img=False)
        return res, list(fused), seen.pop('dets')

    for run, calls in ((run_test, 2), (run_detect, 4)):
        monkeypatch.delenv('YOLO_HIP_TTA', raising=False)
        res_on, fused_on, dets_on = run()
        assert fused_on == [True] * calls, 'one hip_detect(augment=True) per batch'
        monkeypatch.setenv('YOLO_HIP_TTA', '0')
        res_off, fused_off, dets_off = run()
        assert fused_off == [] and len(dets_off) == len(dets_on) == 4
        assert sum(0 if d is None else len(d) for d in dets_on) >= 4
        for a, b in zip(dets_on, dets_off):
            assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())
        assert str(res_on) == str(res_off)
