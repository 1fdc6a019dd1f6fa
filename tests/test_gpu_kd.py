"""GPU tier of feature distillation (csrc/kd.hip behind engine/kd.py, engine/train.py, engine/plan.py).

Kernels against fp64 torch statements with bounds derived from the arithmetic (fp32 summation: ``C * 2^-24 * A`` per map element;
the KL entry as tests/test_gpu_focal_loss.py bounds its kernels: loss ``rtol 1e-5, atol 1e-6``, G within 1e-4 of its largest
magnitude; the injection bit for bit).  Whole steps against CPU fp64 autograd of the torch statement on the eager modules, with the
plain step through the same comparison as the yardstick (a KD step may be three times as far).  Every test prints its figures before
it asserts."""
import copy
import ctypes as C
import os
import types

import pytest
import torch

import conftest
import kd_cases as kc
import synth
import train_harness as th
from engine import hiplib, kd
from engine.hiplib import KD_KL_THREADS

pytestmark = pytest.mark.gpu
GPU = 'cuda'
T = 3.0


@pytest.fixture(scope='module', autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    hiplib.load()
    yield
    # keep nothing of this module alive on the device: later modules assert on torch.cuda.memory_reserved()
    import gc
    kd._KL_TABLES.clear()
    gc.collect()
    torch.cuda.synchronize()


def _code(dtype):
    return hiplib.YH_F16 if dtype == torch.float16 else hiplib.YH_F32


def _features(dtype, seed=0, with_grad=False):
    """Feature buffers (N * HW, ld) on the GPU: channel counts 8, 24, 1024, HW 4 and 4096, and one pitched slice (ld > C, c_off > 0);
    zeros planted in every buffer.  Returns (feature dicts for kd.feature_rows, the tensors)."""
    g = torch.Generator().manual_seed(seed)
    geo = [(2, 2, 2, 8, 8, 0), (2, 64, 64, 8, 8, 0), (2, 2, 2, 24, 24, 0), (2, 64, 64, 24, 24, 0), (2, 2, 2, 1024, 1024, 0),
           (2, 64, 64, 1024, 1024, 0), (3, 5, 7, 72, 96, 16)]
    feats, held = [], []
    for n, h, w, c, ld, c_off in geo:
        y = torch.randn(n * h * w, ld, generator=g)
        y[torch.rand(y.shape, generator=g) < 0.05] = 0.0
        y = y.to(GPU, dtype)
        dy = torch.randn(n * h * w, ld, generator=g).to(GPU, dtype) if with_grad else None
        held.append((y, dy))
        feats.append(dict(y=y.data_ptr(), dy=None if dy is None else dy.data_ptr(), dtype=_code(dtype), n=n, h=h, w=w, c=c, ld=ld, c_off=c_off))
    return feats, held


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_attention_kernel(dtype):
    feats, held = _features(dtype)
    raw, n_rows, n_chunks, shapes = kd.feature_rows(feats)
    table = kd.to_device(raw, GPU)
    total = sum(n * h * w for n, h, w in shapes)
    out = torch.full((total + 8,), -7.0, device=GPU)
    kd.run_attention(table, n_rows, n_chunks, out[:total])
    torch.cuda.synchronize()
    assert (out[total:] == -7.0).all()
    maps = kd.AttentionMaps(out[:total], shapes)
    for f, (y, _), a in zip(feats, held, maps):
        want = y[:, f['c_off']:f['c_off'] + f['c']].double().abs().sum(1)
        err = (a.reshape(-1).double() - want).abs()
        bound = f['c'] * 2.0 ** -24 * want
        print('%s C=%d HW=%d ld=%d: largest error %.3g, bound there %.3g' % (dtype, f['c'], f['h'] * f['w'], f['ld'], err.max().item(),
                                                                             bound[err.argmax()].item()))
        assert (err <= bound).all()


# rows of 4 and 4096 elements, and the smallest row that needs a second workgroup pass: YH_KD_KL_THREADS + 1 = 1025 = 25 x 41
KL_SHAPES = [(2, 2, 2), (2, 64, 64), (2, 25, 41)]
assert KD_KL_THREADS + 1 == 25 * 41


def _kl_reference(a_s, a_t, shapes, batch):
    s = kd.AttentionMaps(a_s.double().cpu().requires_grad_(True), shapes)
    t = kd.AttentionMaps(a_t.double().cpu(), shapes)
    loss = kc.feature_statement(list(s), list(t), batch, T)
    loss.backward()
    return loss.detach(), s.flat.grad * batch / T           # d loss / d a_s = (T / batch) * G


def _run_kl(a_s, a_t, shapes, batch):
    raw, n_rows = kd.kl_rows(shapes)
    table = kd.to_device(raw, GPU)
    G, partials, loss = torch.empty_like(a_s), torch.empty(n_rows, device=GPU), torch.empty(1, device=GPU)
    rc = hiplib.load().yh_kd_attention_kl(a_s.data_ptr(), a_t.data_ptr(), G.data_ptr(), table.data_ptr(), n_rows, partials.data_ptr(),
                                          loss.data_ptr(), T, batch, hiplib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return loss, G


@pytest.mark.parametrize('scale', [1.0, 400.0])
def test_attention_kl_kernel(scale):
    """scale 400: maps up to ~1600, exp(A / T) overflows fp32 (exp(89)) without the max subtraction."""
    g = torch.Generator().manual_seed(5)
    total = sum(n * h * w for n, h, w in KL_SHAPES)
    a_s = (torch.rand(total, generator=g) * 4 * scale).to(GPU)
    a_t = (torch.rand(total, generator=g) * 4 * scale).to(GPU)
    assert scale == 1.0 or not torch.isfinite(torch.exp(a_s / T)).all()
    want_loss, want_G = _kl_reference(a_s, a_t, KL_SHAPES, 2)
    loss, G = _run_kl(a_s, a_t, KL_SHAPES, 2)
    loss2, G2 = _run_kl(a_s, a_t, KL_SHAPES, 2)
    err = (G.double().cpu() - want_G).abs().max().item() / want_G.abs().max().item()
    print('scale %g: loss %.9g, fp64 %.9g; G error %.3g of its largest magnitude' % (scale, loss.item(), want_loss.item(), err))
    assert torch.isfinite(loss).all() and torch.isfinite(G).all()
    assert torch.allclose(loss.double().cpu(), want_loss.reshape(1), rtol=1e-5, atol=1e-6)
    assert err <= 1e-4
    assert torch.equal(loss, loss2) and torch.equal(G, G2)
    # the autograd node: gradient of the loss with respect to the student's maps, upstream gradient from device memory
    s = kd.AttentionMaps(a_s.clone().requires_grad_(True), KL_SHAPES)
    out = kd.attention_kl(s, kd.AttentionMaps(a_t, KL_SHAPES), 2, T)
    (out * torch.full((1,), 7.0, device=GPU)).sum().backward()
    gerr = (s.flat.grad.double().cpu() - 7.0 * (T / 2) * want_G).abs().max().item() / (7.0 * (T / 2) * want_G.abs().max().item())
    print('autograd: gradient error %.3g of its largest magnitude' % gerr)
    assert torch.equal(out.detach(), loss) and gerr <= 1e-4


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_inject_kernel(dtype):
    feats, held = _features(dtype, seed=3, with_grad=True)
    raw, n_rows, n_chunks, shapes = kd.feature_rows(feats)
    table = kd.to_device(raw, GPU)
    total = sum(n * h * w for n, h, w in shapes)
    g = torch.Generator().manual_seed(9)
    G = (torch.rand(total, generator=g) - 0.5).to(GPU)
    gs = torch.tensor([1024.0 * 0.25], device=GPU)              # a GradScaler scale times batch / 64
    batch = 2
    before = [dy.clone() for _, dy in held]
    kd.run_inject(table, n_rows, n_chunks, G, gs, T / batch)
    torch.cuda.synchronize()
    off = 0
    for f, (y, dy), dy0 in zip(feats, held, before):
        pix, lo, hi = y.shape[0], f['c_off'], f['c_off'] + f['c']
        t = (gs * (T / batch) * G[off:off + pix]).float()
        want = (dy0[:, lo:hi].float() + t[..., None] * y[:, lo:hi].sign().float()).to(dtype)
        same = torch.equal(dy[:, lo:hi], want)
        print('%s C=%d pixels=%d: equal %s, zeros in y %d' % (dtype, f['c'], pix, same, int((y[:, lo:hi] == 0).sum())))
        assert (y[:, lo:hi] == 0).any() and same
        assert torch.equal(dy[:, :lo], dy0[:, :lo]) and torch.equal(dy[:, hi:], dy0[:, hi:])
        off += pix


# ------------------------------------------------------------------------------------------------ whole steps
@pytest.fixture(scope='module')
def tiny():
    """yolov3-tiny-hand at 64 px, batch 2: feature rows of 4096 down to 4 elements, the stride-1 max-pool among them.  Student,
    two teachers (other seeds), and the fp64 references, computed once."""
    student, teacher, other = (kc.make_model(kc.TINY_HAND, 64, 1, seed) for seed in (0, 3, 4))
    x = synth.image_batch(2, 64, seed=4)
    targets = kc.labels(1)
    ref = {mode: kc.reference_step(student, teacher, x, targets, mode) for mode in ('plain', 'feature', 'kd4')}
    return types.SimpleNamespace(student=student, teacher=teacher, other=other, x=x, targets=targets, ref=ref)


def _map_check(name, maps, model, x, train):
    m = copy.deepcopy(model).double().train(train)
    with torch.no_grad():
        feats = m._forward_eager(x.double())[-1]
    assert len(maps) == len(feats) == 12
    for j, (a, f) in enumerate(zip(maps, feats)):
        want = f.abs().sum(1)
        err = (a.detach().double().cpu() - want).abs()
        bound = f.shape[1] * 2.0 ** -24 * want
        k = (err - bound).argmax()
        print('%s map %d %s (C=%d): largest error %.3g, worst element error %.3g against bound %.3g'
              % (name, j, tuple(a.shape), f.shape[1], err.max().item(), err.flatten()[k].item(), bound.flatten()[k].item()))
        assert tuple(a.shape) == tuple(want.shape)
        assert (err <= bound).all(), (name, j)


def test_maps_of_both_engines(tiny):
    os.environ['YOLO_HIP_TRAIN_PRECISION'] = 'fp32'
    try:
        s = copy.deepcopy(tiny.student).to(GPU).train()
        s.hip_return_features = 'attention'
        _, maps_s = s(tiny.x.to(GPU))
    finally:
        del os.environ['YOLO_HIP_TRAIN_PRECISION']
    assert isinstance(maps_s, kd.AttentionMaps) and maps_s.flat.requires_grad
    assert sorted(a.shape[1] * a.shape[2] for a in maps_s)[0] == 4 and max(a.shape[1] * a.shape[2] for a in maps_s) == 4096
    _map_check('student (train)', maps_s, tiny.student, tiny.x, True)
    t = copy.deepcopy(tiny.teacher).to(GPU).eval()
    t.hip_precision, t.hip_return_features = 'fp32', 'attention'
    with torch.no_grad():
        _, _, maps_t = t(tiny.x.to(GPU))
    assert isinstance(maps_t, kd.AttentionMaps) and not maps_t.flat.requires_grad
    _map_check('teacher (eval)', maps_t, tiny.teacher, tiny.x, False)
    assert maps_s.shapes == maps_t.shapes and kd.fusable(maps_s, maps_t)


def test_kd_step_matches_cpu_fp64_autograd(tiny):
    dist = {}
    for mode in ('plain', 'feature', 'kd4'):
        got, _, _ = kc.engine_step(tiny.student, tiny.teacher, tiny.x, tiny.targets, mode, device=GPU)
        dist[mode] = kc.distance(got, tiny.ref[mode])
        print('%s: relative l2 distance to CPU fp64 autograd %.3g' % (mode, dist[mode]))
        if mode == 'kd4':
            kd4 = got
    yard = dist['plain']
    # the gradient depends on the teacher: another teacher, another gradient
    got_b, _, _ = kc.engine_step(tiny.student, tiny.other, tiny.x, tiny.targets, 'kd4', device=GPU)
    apart = kc.distance(got_b, kd4)
    print('two teachers: KD4 gradients %.3g apart (yardstick %.3g)' % (apart, yard))
    assert dist['feature'] <= 3 * yard and dist['kd4'] <= 3 * yard, dist
    assert apart > 10 * yard


def test_fp16_step_keeps_the_direction(tiny):
    cos = {}
    for mode in ('plain', 'kd4', 'feature'):
        g32, _, _ = kc.engine_step(tiny.student, tiny.teacher, tiny.x, tiny.targets, mode, precision='fp32', device=GPU)
        g16, _, _ = kc.engine_step(tiny.student, tiny.teacher, tiny.x, tiny.targets, mode, precision='fp16', device=GPU, scale=128.0)
        g16 = {k: v / 128.0 for k, v in g16.items()}
        cos[mode] = kc.cosine(g16, g32)
        print('%s: cosine of the fp16 step against the fp32 step %.6f' % (mode, cos[mode]))
    for mode in ('kd4', 'feature'):
        assert 1 - cos[mode] <= 4 * (1 - cos['plain']) + 0.01, cos


def test_padded_twin_student():
    cfg = th.write_cfg(th.mini_cfg_text())
    teacher = kc.make_model(cfg, 64, 2, 3)
    os.unlink(cfg)
    student = kc.make_model(kc.PRUNED_MINI, 64, 2, 0)
    x, targets = synth.image_batch(2, 64, seed=4), kc.labels(2)
    dist = {}
    for mode in ('plain', 'kd4', 'feature'):
        got, m, _ = kc.engine_step(student, teacher, x, targets, mode, device=GPU)
        dist[mode] = kc.distance(got, kc.reference_step(student, teacher, x, targets, mode))
        print('padded twin, %s: relative l2 distance to CPU fp64 autograd %.3g' % (mode, dist[mode]))
    from engine.padded import PaddedTrainEngine
    eng = m.__dict__['_hip_train_engine']
    assert isinstance(eng, PaddedTrainEngine)
    torch.cuda.synchronize()
    plan, padded = eng.inner._current, 0
    for v in plan['kd_values']:
        g = eng.inner._arena.view(v.gstorage.off, v.gstorage.n, v.gstorage.dtype).view(-1, v.ld)[:, v.c_off:v.c_off + v.c_phys]
        pad = kc.pad_lanes(eng, v)
        padded += len(pad)
        assert pad == [] or (g[:, pad] == 0).all(), v.block
        if getattr(v, 'bn', None) is not None and pad:
            for off in (v.g_gamma, v.g_beta):
                assert (plan['grads'].view(off, v.C)[pad] == 0).all(), v.block
    print('pad lanes checked:', padded)
    assert padded > 0
    assert dist['kd4'] <= 3 * dist['plain'] and dist['feature'] <= 3 * dist['plain'], dist


def test_launch_counts(tiny):
    """One attention launch per model and step, one KL launch, one inject launch - through both real engines, as train.py runs them."""
    from utils import utils as U
    os.environ['YOLO_HIP_TRAIN_PRECISION'] = 'fp32'
    try:
        s = copy.deepcopy(tiny.student).to(GPU).train()
        t = copy.deepcopy(tiny.teacher).to(GPU).eval()
        s.hip_return_features = t.hip_return_features = 'attention'
        x, targets = tiny.x.to(GPU), tiny.targets.to(GPU)
        for step in range(2):
            kd.reset_stats()
            pred, fs = s(x)
            with torch.no_grad():
                _, out_t, ft = t(x)
            loss = U.compute_loss(pred, targets, s)[0] + U.compute_lost_KD4(s, targets, pred, out_t, fs, ft, x.shape[0])
            (loss * 0.5).sum().backward()
            torch.cuda.synchronize()
            print('step %d: %s' % (step, kd.stats()))
            assert kd.stats() == dict(attention=2, kl=1, inject=1)
            assert all(torch.isfinite(p.grad).all() for p in s.parameters())
    finally:
        del os.environ['YOLO_HIP_TRAIN_PRECISION']
