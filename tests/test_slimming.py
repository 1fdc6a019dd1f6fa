"""CPU tier of network slimming without the reference: the layer sets (engine/slimming.py), the channel-prune tool
(tools/slim_prune.py), the sparsity term of the HIP training step on the host emulation of the C ABI (engine/train.py
``set_bn_sparsity``, ``yh_bn_l1_subgrad`` emulated in tests/fakelib_sparsity.py) and ``train.py --prune`` on CPU tensors.

Everything here runs with no reference checkout on the import path: the fixture below takes the reference's ``utils`` directory off
``utils.__path__`` and forgets an already imported ``utils.prune_utils`` for the duration of each test, and each test ends with the
assertion that the module was not imported.  Expected values are recorded results of the reference
(tests/golden/make_golden_slimming.py, tests/golden/slim_prune_0.5_yolov3-mobilenet-coco.cfg).
"""
import copy
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

import conftest
import fakelib_sparsity
import synth
import train_harness as th

GOLDEN = os.path.join(conftest.REPO, 'tests', 'golden')
sys.path.insert(0, os.path.join(conftest.PKG, 'tools'))


@pytest.fixture(autouse=True)
def no_reference(monkeypatch):
    import utils
    monkeypatch.setattr(utils, '__path__', [p for p in utils.__path__ if os.path.isfile(os.path.join(p, 'parse_config.py'))
                                            and not os.path.isfile(os.path.join(p, 'prune_utils.py'))])
    monkeypatch.delitem(sys.modules, 'utils.prune_utils', raising=False)
    monkeypatch.setenv('YOLO_REFERENCE_ROOT', '/nonexistent')
    yield
    assert 'utils.prune_utils' not in sys.modules, 'the reference module was imported'
    with pytest.raises(ImportError):
        import utils.prune_utils  # noqa: F401


# ----------------------------------------------------------------------------------------------- layer sets
SETS = json.load(open(os.path.join(GOLDEN, 'prune_sets.json')))


@pytest.mark.parametrize('rel', sorted(SETS))
def test_layer_sets_equal_the_reference_parsers(rel):
    import models
    from engine import slimming
    if rel == 'mini':
        path = th.write_cfg(th.mini_cfg_text())
    else:
        path = os.path.join(conftest.PKG, 'cfg', rel)
    try:
        defs = models.Darknet(path).module_defs
    finally:
        if rel == 'mini':
            os.unlink(path)
    for mode in (0, 1, 2):
        want = SETS[rel][str(mode)]
        if 'raises' in want:
            with pytest.raises(Exception) as e:
                slimming.layer_sets(defs, mode)
            assert type(e.value).__name__ == want['raises'], (rel, mode)
            continue
        got = slimming.layer_sets(defs, mode)
        ret = want['returns']
        assert got.bn_convs == ret[0] and got.other == ret[1] and list(got.prune) == ret[2], (rel, mode)
        assert slimming.sparsity_blocks(defs, mode) == ret[2]
        if mode == 1:
            assert sorted([k, v] for k, v in got.shortcut_source.items()) == ret[3] and sorted(got.shortcut_members) == ret[4], rel
    with pytest.raises(ValueError):
        slimming.layer_sets(defs, 3)


def test_train_py_picks_its_layers_natively():
    import models
    import train as train_module
    defs = models.Darknet(os.path.join(conftest.PKG, 'cfg', 'yolov3', 'yolov3.cfg')).module_defs
    for mode in (0, 1, 2):
        assert train_module.sparsity_layers(mode, defs) == SETS['yolov3/yolov3.cfg'][str(mode)]['returns'][2]
    assert not hasattr(train_module, 'BNOptimizer')


def test_gather_bn_weights_and_the_torch_form_of_the_term():
    """``gather_bn_weights`` concatenates |gamma| in block order; ``apply_bn_l1_`` is bit-equal to the recorded ``updateBN`` results."""
    from engine import slimming
    z = np.load(os.path.join(GOLDEN, 'bn_l1.npz'))
    rows = [k for k in range(7)]
    blocks = []
    for k in rows:
        bn = torch.nn.BatchNorm2d(len(z['gamma_%d' % k]))
        bn.weight.data = torch.from_numpy(z['gamma_%d' % k].copy())
        blocks.append(torch.nn.Sequential(torch.nn.Identity(), bn))
    got = slimming.gather_bn_weights(blocks, [2, 0, 5])
    want = np.abs(np.concatenate([z['gamma_2'], z['gamma_0'], z['gamma_5']]))
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    for j, s in enumerate(z['s']):
        for k in rows:
            blocks[k][1].weight.grad = torch.from_numpy(z['grad_%d' % k].copy())
        slimming.apply_bn_l1_(blocks, rows, float(s))
        for k in rows:
            assert np.array_equal(blocks[k][1].weight.grad.numpy().view(np.int32), z['out%d_%d' % (j, k)].view(np.int32)), (j, k)


# ----------------------------------------------------------------------------------------------- prune tool
def test_slim_prune_tool_reproduces_the_reference_on_the_mini_cfg(tmp_path, tiny_cfg, monkeypatch):
    """tools/slim_prune.py --no-eval on the spread-gamma mini model of tests/test_reference_scripts.py: compact cfg byte for byte,
    gathered tensors exactly, compensated running_mean / bias within 4 x the recorded fp32-vs-fp64 difference of the reference's own
    result (only the summation order of the fold can differ)."""
    import models
    import slim_prune
    from test_reference_scripts import _prepare
    model, cfg, wfile = _prepare(tmp_path, tiny_cfg, seed=0)
    monkeypatch.chdir(tmp_path)
    cfg_out, w_out = slim_prune.main(['--cfg', cfg, '--data', 'unused.data', '--weights', wfile, '--percent', '0.5', '--img-size', '64',
                                      '--batch-size', '4', '--no-eval'])
    assert cfg_out == os.path.join('cfg', 'slim_prune_0.5mini', 'slim_prune_0.5mini.cfg')
    assert w_out == os.path.join('weights', 'slim_prune_0.5mini', 'slim_prune_0.5_percent.weights')
    assert open(cfg_out, 'rb').read() == open(os.path.join(GOLDEN, 'slim_prune_mini.cfg'), 'rb').read()
    z = np.load(os.path.join(GOLDEN, 'slim_prune_mini.npz'))
    loaded = models.Darknet(cfg, (64, 64))
    models.load_darknet_weights(loaded, wfile)
    res = slim_prune.slim_prune(loaded, 0.5, 0.01, 64)
    assert float(res['threshold']) == float(z['threshold'])
    compact = models.Darknet(cfg_out, (64, 64))
    models.load_darknet_weights(compact, w_out)
    bound = 4 * float(z['bias_comp_bound'])
    assert 0 < bound < 1e-5
    state = compact.state_dict()
    keys = [k[len('state/'):] for k in z.files if k.startswith('state/')]
    assert sorted(keys) == sorted(k for k in state if 'num_batches_tracked' not in k)
    n_comp = 0
    for k in keys:
        want = torch.from_numpy(z['state/' + k])
        assert state[k].shape == want.shape, k
        if k.endswith('running_mean') or k.endswith('Conv2d.bias'):
            n_comp += 1
            d = (state[k] - want).abs().max().item()
            print('%s: |native - reference| = %.3e (bound %.3e)' % (k, d, bound))
            assert d <= bound, (k, d, bound)
        else:
            assert torch.equal(state[k], want), k
    assert n_comp == 14


def _mobilenet_seeded():
    """The seeded YOLOv3-Mobilenetv3 state of tools/make_pruned.py: BatchNorm gammas spread out so the global threshold cuts every layer
    differently."""
    import models
    torch.manual_seed(0)
    model = models.Darknet(os.path.join(conftest.PKG, 'cfg', 'yolov3-mobilenet', 'yolov3-mobilenet-coco.cfg'), (416, 416))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith('BatchNorm2d.weight'):
                v.copy_(torch.rand(v.shape, generator=g) * 1.5 + 0.01)
            elif k.endswith('running_var'):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith('BatchNorm2d.bias') or k.endswith('running_mean'):
                v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    return model


def test_slim_prune_tool_reproduces_the_reference_on_mobilenetv3(tmp_path):
    """Depthwise, squeeze-excite, 37 odd widths: the native tool's compact cfg equals the committed output of the reference's
    slim_prune.py --percent 0.5 byte for byte; the compact model loads its .weights and runs one eval forward."""
    import models
    import slim_prune
    model = _mobilenet_seeded()
    src = os.path.join(conftest.PKG, 'cfg', 'yolov3-mobilenet', 'yolov3-mobilenet-coco.cfg')
    res = slim_prune.slim_prune(model, 0.5, 0.01, 416)
    text = slim_prune.cfg_text(model.hyperparams, res['defs'], slim_prune._anchors_text(src))
    want = open(os.path.join(GOLDEN, 'slim_prune_0.5_yolov3-mobilenet-coco.cfg'), 'rb').read()
    assert text.encode() == want
    widths = [int(d['filters']) for d in res['defs'] if d['type'] == 'convolutional']
    assert sum(1 for w in widths if w % 8) == 37
    cfg_out, w_out = tmp_path / 'compact.cfg', tmp_path / 'compact.weights'
    cfg_out.write_text(text)
    models.save_weights(res['model'], path=str(w_out))
    compact = models.Darknet(str(cfg_out), (96, 96))
    before = [p.clone() for p in compact.parameters()]
    models.load_darknet_weights(compact, str(w_out))
    assert any(not torch.equal(a, b) for a, b in zip(before, compact.parameters()))
    for (k, a), (_, b) in zip(compact.state_dict().items(), res['model'].state_dict().items()):
        if 'num_batches_tracked' not in k:
            assert torch.equal(a, b), k
    with torch.no_grad():
        inf = compact.eval()(torch.rand(1, 3, 96, 96, generator=torch.Generator().manual_seed(2)))[0]
    assert torch.isfinite(inf).all()


# ----------------------------------------------------------------------------------------------- engine plumbing
class _Stepper:
    """One model on the HIP training path over the emulated ABI; ``step()`` = forward + toy loss + backward (no zero_grad)."""

    def __init__(self, model, x, lib):
        from engine.padded import make_train_engine
        self.m = copy.deepcopy(model).train()
        for p in self.m.parameters():
            p.grad = None
        self.x, self.lib = x, lib
        self.m.__dict__['_hip_train_engine'] = make_train_engine(self.m, 'fp32', x, lib=lib)
        self.ws = None

    def step(self):
        raws, _ = self.m._forward_hip_train(self.x)
        self.ws = self.ws or th.loss_weights(raws)
        th.toy_loss(raws, self.ws).backward()
        return self.grads()

    def grads(self):
        return {k: p.grad.clone() for k, p in self.m.named_parameters()}

    def zero(self):
        for p in self.m.parameters():
            p.grad = None

    def gamma_names(self, blocks):
        return {'module_list.%d.BatchNorm2d.weight' % i for i in blocks}

    def term(self, name, s):
        return s * torch.sign(dict(self.m.named_parameters())[name].detach())


@pytest.fixture
def fp32_step(monkeypatch):
    monkeypatch.setenv('YOLO_HIP_TRAIN_PRECISION', 'fp32')


def _check_step(st, plain, blocks, s, times=1):
    got = st.grads()
    listed = st.gamma_names(blocks)
    assert listed <= set(got)
    for k, g in plain.items():
        want = g
        if k in listed:
            want = g + st.term(k, s)
        if times == 2:
            want = want + want
        assert torch.equal(got[k], want), k


def test_engine_adds_the_sparsity_term_inside_the_backward(fp32_step):
    """21-block mini cfg through the emulated ABI: every parameter gets the gradient of the plain step, the listed gammas additionally
    s * sign(gamma) - bit-equal to the torch formula; two micro-steps accumulate two terms; a changed s is honoured; switching the
    term off restores the plain step; a rebound gamma (``param.data = ...``) rewrites the table."""
    from engine import slimming
    path = th.write_cfg(th.mini_cfg_text())
    try:
        model = th.build(path, 64)
    finally:
        os.unlink(path)
    x = synth.image_batch(2, 64, seed=0)
    blocks = slimming.sparsity_blocks(model.module_defs, 1)
    assert len(blocks) == 11
    with torch.no_grad():       # exact zeros and a negative zero among the gammas: sign gives 0 there
        w = model.module_list[blocks[0]][1].weight
        w[0], w[1], w[2] = 0.0, -0.0, -abs(float(w[2])) - 0.1
    plain_st = _Stepper(model, x, fakelib_sparsity.FakeLibSparsity())
    plain = plain_st.step()
    assert plain_st.lib.l1_calls == []                     # off: no launch
    st = _Stepper(model, x, fakelib_sparsity.FakeLibSparsity())
    st.m.hip_set_bn_sparsity(blocks, 1e-3)
    st.step()
    eng = st.m.__dict__['_hip_train_engine']
    nseg = len(eng._current['segments'])
    assert 1 <= len(st.lib.l1_calls) <= nseg               # at most one launch per backward range
    assert sum(b - a for a, b, _ in st.lib.l1_calls) == len(blocks)
    _check_step(st, plain, blocks, 1e-3)
    # second micro-step without zero_grad: autograd accumulates two gradients, each with its term
    st.step()
    _check_step(st, plain, blocks, 1e-3, times=2)
    # s changes between steps: a launch argument, the table stays
    key = eng._current['l1_key']
    st.zero()
    st.m.hip_set_bn_sparsity(blocks, 0.37)
    st.step()
    assert eng._current['l1_key'] == key
    _check_step(st, plain, blocks, 0.37)
    # a rebound gamma: the row must follow the new tensor (the condition of the pack-table refresh: a parameter moved)
    import ctypes as C
    from engine.hiplib import BnL1Row
    bn = st.m.module_list[blocks[3]][1]
    old = bn.weight.data
    row = BnL1Row.from_address(eng._current['l1_table'].data_ptr() + 3 * C.sizeof(BnL1Row))
    assert row.gamma == old.data_ptr() and row.n == old.numel()
    bn.weight.data = old.clone()
    assert bn.weight.data_ptr() != old.data_ptr()
    st.zero()
    st.step()
    assert eng._current['l1_key'] != key
    row = BnL1Row.from_address(eng._current['l1_table'].data_ptr() + 3 * C.sizeof(BnL1Row))
    assert row.gamma == bn.weight.data_ptr()
    _check_step(st, plain, blocks, 0.37)
    # a subset, then off
    st.zero()
    st.m.hip_set_bn_sparsity(blocks[2:5], 0.5)
    st.step()
    _check_step(st, plain, blocks[2:5], 0.5)
    n_calls = len(st.lib.l1_calls)
    st.zero()
    st.m.hip_set_bn_sparsity(None, 0.5)
    st.step()
    assert len(st.lib.l1_calls) == n_calls
    _check_step(st, plain, [], 0.0)
    st.zero()
    st.m.hip_set_bn_sparsity([], 0.5)
    st.step()
    _check_step(st, plain, [], 0.0)
    with pytest.raises(ValueError):
        st.m.hip_set_bn_sparsity([4], 0.1)                 # a shortcut is not a conv + BatchNorm block


def test_setting_survives_an_engine_rebuild(fp32_step):
    from engine import slimming
    from engine.padded import make_train_engine
    path = th.write_cfg(th.mini_cfg_text())
    try:
        model = th.build(path, 64)
    finally:
        os.unlink(path)
    x = synth.image_batch(2, 64, seed=0)
    blocks = slimming.sparsity_blocks(model.module_defs, 0)
    plain = _Stepper(model, x, fakelib_sparsity.FakeLibSparsity()).step()
    st = _Stepper(model, x, fakelib_sparsity.FakeLibSparsity())
    st.m.hip_set_bn_sparsity(blocks, 0.01)
    st.m.hip_refresh()                                      # drops the engine
    assert st.m.__dict__['_hip_train_engine'] is None
    st.m.__dict__['_hip_train_engine'] = make_train_engine(st.m, 'fp32', x, lib=st.lib)
    st.step()
    _check_step(st, plain, blocks, 0.01)


def test_odd_width_graph_carries_the_term_on_its_real_lanes_only(fp32_step):
    """The slim-pruned mini cfg (widths 4, 13, 5 ...) trains through the channel-padded twin: the term is added in the twin's arena, the
    gradients gathered back carry it on every real lane, and the pad lanes of the twin (gamma = 0) received exactly 0."""
    import models
    from engine import slimming
    from engine.padded import PaddedTrainEngine
    torch.manual_seed(0)
    model = models.Darknet(os.path.join(GOLDEN, 'slim_prune_mini.cfg'), (64, 64))
    state = model.state_dict()
    synth.randomize_bn_(state, seed=1)
    model.load_state_dict(state)
    model.train()
    x = synth.image_batch(2, 64, seed=0)
    blocks = slimming.sparsity_blocks(model.module_defs, 1)
    plain_st = _Stepper(model, x, fakelib_sparsity.FakeLibSparsity())
    plain = plain_st.step()
    st = _Stepper(model, x, fakelib_sparsity.FakeLibSparsity())
    st.m.hip_set_bn_sparsity(blocks, 0.25)
    st.step()
    eng = st.m.__dict__['_hip_train_engine']
    assert isinstance(eng, PaddedTrainEngine) and st.lib.l1_calls
    _check_step(st, plain, blocks, 0.25)
    padded = 0
    for e_a, e_b in ((eng, plain_st.m.__dict__['_hip_train_engine']),):
        plan_a, plan_b = e_a.inner._current, e_b.inner._current
        for va, vb in zip(plan_a['values'], plan_b['values']):
            if va.kind == 'conv' and va.bn is not None and va.block in blocks:
                real = st.m.module_list[va.block][0].out_channels
                ga, gb = plan_a['grads'].view(va.g_gamma, va.C), plan_b['grads'].view(vb.g_gamma, vb.C)
                lay = e_a.pad.layouts[va.block]
                pad_lanes = sorted(set(range(va.C)) - set(lay.pos.tolist()))
                assert len(pad_lanes) == va.C - real
                padded += len(pad_lanes)
                assert torch.equal(va.bn.weight.detach()[pad_lanes], torch.zeros(len(pad_lanes)))
                assert torch.equal(ga[pad_lanes], gb[pad_lanes])
    assert padded > 0


# ----------------------------------------------------------------------------------------------- train.py
def test_train_py_sparse_training_runs_without_the_reference(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    """train.py --prune 0 on four synthetic images, CPU tensors: one epoch of two batches runs to completion with no reference
    checkout importable (on the parent commit the flag ends in an ImportError)."""
    monkeypatch.chdir(tmp_path)
    import train as train_mod
    files = (dataset_dir / 'train.txt').read_text().split('\n')[:4]
    (tmp_path / 'four.txt').write_text('\n'.join(files) + '\n')
    (tmp_path / 'four.data').write_text('classes=2\ntrain=%s\nvalid=%s\nnames=%s\n' % (tmp_path / 'four.txt', tmp_path / 'four.txt',
                                                                                 dataset_dir / 'synth.names'))
    opt = train_mod.make_parser().parse_args(['--epochs', '1', '--batch-size', '2', '--cfg', tiny_cfg, '--data', str(tmp_path / 'four.data'),
                                              '--img-size', '64', '64', '64', '--device', 'cpu', '--nosave', '--prune', '0', '--s', '0.01'])
    opt.local_rank = -1
    results = train_mod.train(opt, train_mod.hyp)
    assert len(results) == 7 and all(np.isfinite(results))
    assert os.path.isfile('weights/last.pt')
