"""CPU tier of distillation strategies 2 - 4 (utils/utils.py ``compute_lost_KD2/3/4``, engine/kd.py, train.py).

* The three host statements against recorded runs of the reference (tests/golden/kd_losses.npz, make_golden_kd.py): the same torch
  operations in the same order on the same torch build, so loss, ``reg_ratio`` and every gradient are expected to be EQUAL.
* The engine glue of an attention step on the host emulation (tests/fakelib_kd.py) against fp64 autograd of the torch statement on
  the eager modules.  Yardstick: the plain step through the same comparison; a KD step may be three times as far (the project's
  standing margin, tests/test_gpu_focal_loss.py).
* Plan isolation, the step arena under KD4, and the script's checks.
"""
import copy
import io
import os
import types

import numpy as np
import pytest
import torch

import conftest
import fakelib_kd
import kd_cases as kc
import synth
import train_harness as th
from engine import kd
from models import Darknet
from utils import utils as U

GOLDEN = os.path.join(conftest.REPO, 'tests', 'golden', 'kd_losses.npz')


# ------------------------------------------------------------------------------------------------ golden
@pytest.fixture(scope='module')
def golden():
    rec = dict(np.load(GOLDEN))
    path = th.write_cfg(str(rec['cfg_s']))
    try:
        model = Darknet(path, (64, 64))
    finally:
        os.unlink(path)
    model.nc, model.hyp = 1, {'iou_t': float(rec['iou_t'])}
    n_out = sum(1 for k in rec if k.startswith('out_s'))
    n_f = sum(1 for k in rec if k.startswith('fs'))
    T = lambda k: torch.from_numpy(rec[k])
    return types.SimpleNamespace(rec=rec, model=model, targets=T('targets'), out_s=[T('out_s%d' % i) for i in range(n_out)],
                                 out_t=[T('out_t%d' % i) for i in range(n_out)], fs=[T('fs%d' % j) for j in range(n_f)],
                                 ft=[T('ft%d' % j) for j in range(n_f)], T=T)


def _leaves(ts):
    return [t.clone().requires_grad_(True) for t in ts]


def _check(name, got, want):
    got, want = got.detach(), want
    print('%s: largest difference %.3g (largest magnitude %.3g)' % (name, (got - want).abs().max().item(), want.abs().max().item()))
    assert torch.equal(got, want), name


def test_golden_case_is_the_one_the_issue_asks_for(golden):
    assert len(golden.fs) == 12 and golden.fs[0].shape == (2, 2, 64, 64) and golden.fs[-1].shape[2:] == (4, 4)
    assert min(f.shape[2] * f.shape[3] for f in golden.fs) == 4
    assert any(a.shape[1] != b.shape[1] for a, b in zip(golden.fs, golden.ft))           # the pruned-student case
    t = golden.targets
    assert len(t) >= 3 and (t[:, 0] == 0).sum() >= 2
    assert os.path.getsize(GOLDEN) < (1 << 20)


@pytest.mark.parametrize('k', [2, 3, 4])
def test_host_statements_equal_the_reference(golden, k):
    po, pf = _leaves(golden.out_s), _leaves(golden.fs)
    if k == 2:
        loss, ratio = U.compute_lost_KD2(golden.model, golden.targets, po, golden.out_t)
        print('reg_ratio', ratio, float(golden.rec['kd2_reg_ratio']))
        assert ratio == float(golden.rec['kd2_reg_ratio'])
    elif k == 3:
        loss = U.compute_lost_KD3(golden.model, golden.targets, po, golden.out_t)
    else:
        loss = U.compute_lost_KD4(golden.model, golden.targets, po, golden.out_t, pf, golden.ft, 2)
    loss.sum().backward()
    _check('kd%d loss' % k, loss, golden.T('kd%d_loss' % k))
    for i, p in enumerate(po):
        _check('kd%d d out_s[%d]' % (k, i), p.grad, golden.T('kd%d_dout%d' % (k, i)))
    if k == 4:
        for j, p in enumerate(pf):
            _check('kd4 d fs[%d]' % j, p.grad, golden.T('kd4_dfs%d' % j))


def test_channel_summed_maps_equal_4d_features_bit_for_bit(golden):
    po = _leaves(golden.out_s)
    maps_s = [f.abs().sum(1).requires_grad_(True) for f in golden.fs]
    maps_t = [f.abs().sum(1) for f in golden.ft]
    loss = U.compute_lost_KD4(golden.model, golden.targets, po, golden.out_t, maps_s, maps_t, 2)
    loss.sum().backward()
    assert torch.equal(loss.detach(), golden.T('kd4_loss'))
    # mixed forms too: a 3-D student map against the teacher's 4-D feature
    loss2 = U.compute_lost_KD4(golden.model, golden.targets, _leaves(golden.out_s), golden.out_t, [m.detach() for m in maps_s], golden.ft, 2)
    assert torch.equal(loss2.detach(), golden.T('kd4_loss'))
    for j, (m, f) in enumerate(zip(maps_s, golden.fs)):      # d loss / d fs = d loss / d map * sign(fs)
        assert torch.equal(m.grad[:, None] * f.sign(), golden.T('kd4_dfs%d' % j)), j


def test_feature_mismatch_raises(golden):
    args = (golden.model, golden.targets, golden.out_s, golden.out_t)
    with pytest.raises(ValueError, match='feature mismatch'):
        U.compute_lost_KD4(*args, golden.fs[:-1], golden.ft, 2)
    bad = list(golden.ft)
    bad[3] = bad[3][:, :, :-1]
    with pytest.raises(ValueError, match='feature mismatch'):
        U.compute_lost_KD4(*args, golden.fs, bad, 2)


# ------------------------------------------------------------------------------------------------ engine glue on the emulation
@pytest.fixture(scope='module')
def mini():
    cfg = th.write_cfg(th.mini_cfg_text())
    student, teacher = kc.make_model(cfg, 64, 2, 0), kc.make_model(cfg, 64, 2, 3)
    os.unlink(cfg)
    x = synth.image_batch(2, 64, seed=4)
    targets = kc.labels(2)
    ref = {mode: kc.reference_step(student, teacher, x, targets, mode) for mode in ('plain', 'feature', 'kd4')}
    return types.SimpleNamespace(student=student, teacher=teacher, x=x, targets=targets, ref=ref)


def test_kd_step_on_the_emulation_matches_fp64_autograd(mini):
    lib = fakelib_kd.FakeLibKd()
    dist = {}
    for mode in ('plain', 'feature', 'kd4'):
        kd.reset_stats()
        got, m, feats = kc.engine_step(mini.student, mini.teacher, mini.x, mini.targets, mode, lib=lib)
        dist[mode] = kc.distance(got, mini.ref[mode])
        print('%s: relative l2 distance to fp64 autograd %.3g, launches %s' % (mode, dist[mode], kd.stats()))
        if mode == 'plain':
            assert feats == [] and kd.stats() == dict(attention=0, kl=0, inject=0)
        else:
            assert isinstance(feats, kd.AttentionMaps) and len(feats) == len(kc.eager_maps(mini.student, mini.x))
            assert kd.stats() == dict(attention=1, kl=1, inject=1)
    assert kc.distance(mini.ref['feature'], mini.ref['plain']) > 0.5          # the feature step is another gradient altogether
    assert dist['feature'] <= 3 * dist['plain'], dist
    assert dist['kd4'] <= 3 * dist['plain'], dist


def test_attention_maps_behave_like_the_reference_list(mini):
    lib = fakelib_kd.FakeLibKd()
    _, m, feats = kc.engine_step(mini.student, mini.teacher, mini.x, mini.targets, 'feature', lib=lib)
    want = kc.eager_maps(mini.student, mini.x)
    assert len(feats) == len(want) and [tuple(f.shape) for f in feats] == [tuple(w.shape) for w in want]
    assert feats.flat.dtype == torch.float32 and feats.flat.numel() == sum(w.numel() for w in want)
    for f, w, off in zip(feats, want, feats.offsets):
        assert f.data_ptr() == feats.flat.data_ptr() + 4 * off               # views of the one flat buffer, no copies
        bound = 4 * w.abs().max().item() * 2 ** -20
        assert (f.detach() - w).abs().max().item() <= bound
    assert [f for f in feats][0] is feats[0]


def test_torch_statement_on_the_maps_takes_the_same_injection(mini, monkeypatch):
    """YOLO_HIP_KD=0: autograd hands the engine an ordinary gradient of the flat buffer; one inject launch with g = 1."""
    monkeypatch.setenv('YOLO_HIP_KD', '0')
    lib = fakelib_kd.FakeLibKd()
    kd.reset_stats()
    got, _, _ = kc.engine_step(mini.student, mini.teacher, mini.x, mini.targets, 'feature', lib=lib)
    dist = kc.distance(got, mini.ref['feature'])
    print('torch statement on the maps: distance %.3g, launches %s' % (dist, kd.stats()))
    assert kd.stats() == dict(attention=1, kl=0, inject=1)
    plain, _, _ = kc.engine_step(mini.student, mini.teacher, mini.x, mini.targets, 'plain', lib=lib)
    assert dist <= 3 * kc.distance(plain, mini.ref['plain'])


def test_padded_twin_keeps_pad_lanes_zero(mini):
    lib = fakelib_kd.FakeLibKd()
    student = kc.make_model(kc.PRUNED_MINI, 64, 2, 0)
    ref = {mode: kc.reference_step(student, mini.teacher, mini.x, mini.targets, mode) for mode in ('plain', 'kd4', 'feature')}
    dist = {}
    for mode in ('plain', 'kd4', 'feature'):
        got, m, _ = kc.engine_step(student, mini.teacher, mini.x, mini.targets, mode, lib=lib)
        dist[mode] = kc.distance(got, ref[mode])
    print('padded twin:', dist)
    from engine.padded import PaddedTrainEngine
    eng = m.__dict__['_hip_train_engine']
    assert isinstance(eng, PaddedTrainEngine)
    assert dist['kd4'] <= 3 * dist['plain'] and dist['feature'] <= 3 * dist['plain'], dist
    plan, padded = eng.inner._current, 0
    for v in plan['kd_values']:                 # the gradient buffers after the feature step: pad lanes are exact zeros
        g = eng.inner._arena.view(v.gstorage.off, v.gstorage.n, v.gstorage.dtype).view(-1, v.ld)[:, v.c_off:v.c_off + v.c_phys]
        pad = kc.pad_lanes(eng, v)
        padded += len(pad)
        assert pad == [] or (g[:, pad] == 0).all(), v.block
        assert g.abs().sum() > 0
        if getattr(v, 'bn', None) is not None and pad:
            for off in (v.g_gamma, v.g_beta):
                assert (plan['grads'].view(off, v.C)[pad] == 0).all(), v.block
    assert padded > 0


def test_plan_isolation_plain_step_keeps_its_bits(mini):
    lib = fakelib_kd.FakeLibKd()
    fresh, _, _ = kc.engine_step(mini.student, mini.teacher, mini.x, mini.targets, 'plain', lib=lib)
    m = None
    for mode in ('kd4', 'plain', 'feature', 'plain'):
        got, m, _ = kc.engine_step(mini.student, mini.teacher, mini.x, mini.targets, mode, lib=lib, model=m)
        if mode == 'plain':
            for k in fresh:
                assert torch.equal(got[k], fresh[k]), k
    eng = m.__dict__['_hip_train_engine']
    plain, attn = eng._tplans[tuple(mini.x.shape)], eng._tplans[tuple(mini.x.shape) + (True,)]
    assert 'kd_values' not in plain and len(plain['fwd_ops']) <= len(attn['fwd_ops'])
    assert m.hip_train_stats()['plan_builds'] == 2


def test_arena_under_kd4_allocates_nothing_after_the_reservation(mini):
    from engine.padded import make_train_engine
    lib = fakelib_kd.FakeLibKd()
    m = copy.deepcopy(mini.student).train()
    m.hip_return_features = 'attention'
    shapes = [(2, 3, 64, 64), (2, 3, 32, 32)]
    m.__dict__['_hip_train_engine'] = make_train_engine(m, 'fp32', shapes[1], lib=lib)
    before = m.hip_train_stats()
    m.hip_reserve_train(shapes, 'fp32')
    st = m.hip_train_stats()
    assert st['arena_bytes'] > before['arena_bytes'] and st['plan_bytes'] > before['plan_bytes']
    plan = m.__dict__['_hip_train_engine']._tplans[shapes[0] + (True,)]
    assert plan['arena_need'] >= 8 * plan['kd_maps'].n      # maps and G are pieces of the arena
    allocs = st['arena_allocs']
    for size in (32, 64, 32):
        x = synth.image_batch(2, size, seed=size)
        kc.engine_step(mini.student, mini.teacher, x, mini.targets, 'kd4', lib=lib, model=m)
    assert m.hip_train_stats()['arena_allocs'] == allocs
    assert m.hip_train_stats()['plan_builds'] == st['plan_builds']


def test_true_still_raises_on_the_training_step(mini):
    m = copy.deepcopy(mini.student).train()
    m.hip_return_features = True
    x = types.SimpleNamespace(is_cuda=True)
    with pytest.raises(NotImplementedError, match='attention'):
        m._use_hip_train(x)
    m.hip_return_features = 'attention'
    assert m._use_hip_train(x)


# ------------------------------------------------------------------------------------------------ script
def test_script_wiring(mini, capsys):
    import train as train_mod
    base = ['--cfg', 'a.cfg', '--data', 'a.data']
    for k in (2, 3, 4):
        with pytest.raises(SystemExit):
            train_mod.parse_args(base + ['--KDstr', str(k)])
        assert train_mod.parse_args(base + ['--KDstr', str(k), '--t_cfg', 't.cfg']).KDstr == k
    capsys.readouterr()
    student, teacher = copy.deepcopy(mini.student), copy.deepcopy(mini.teacher).eval()
    with pytest.raises(NotImplementedError, match=r'\.cuda\(\)'):
        train_mod.configure_distillation(student, teacher, 5, 'cpu')
    with pytest.raises(NotImplementedError):
        train_mod.configure_distillation(student, teacher, 7, 'cpu')
    with pytest.raises(NotImplementedError, match=r'\.cuda\(\)'):
        train_mod.distillation_loss(5, student, None, None, None, None, None, 2, 2)
    quantised = types.SimpleNamespace(quantized=1)
    with pytest.raises(ValueError, match='float graph'):
        train_mod.configure_distillation(student, quantised, 4, 'cpu')
    train_mod.configure_distillation(student, teacher, 4, 'cpu')          # CPU: the eager lists
    assert student.hip_return_features is False and teacher.hip_return_features is False
    train_mod.configure_distillation(student, teacher, 4, 'cuda:0')
    assert student.hip_return_features == 'attention' and teacher.hip_return_features == 'attention'
    # strategies 2 - 4 run on the CPU's eager lists
    x, targets = mini.x, mini.targets
    pred, fs = mini.student._forward_eager(x)
    with torch.no_grad():
        out_t, ft = copy.deepcopy(mini.teacher).train()._forward_eager(x)
    for k in (2, 3, 4):
        loss = train_mod.distillation_loss(k, mini.student, targets, pred, out_t, fs, ft, 2, 2)
        assert loss.shape == (1,) and torch.isfinite(loss).all() and loss.requires_grad
