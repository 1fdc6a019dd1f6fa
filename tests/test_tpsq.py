"""TPSQ (``--quantized 2``) on this package's own ``utils/quantized/quantized_TPSQ.py``: CPU tier.

Fixtures come from the reference's module family (tests/golden/make_golden_tpsq.py, call sequences in tests/tpsq_cases.py).  The
quantisers one by one are compared exactly, decisions included; the conv module and the micro net within the bounds tests/test_qat.py
uses for the same comparisons in mode 1 (``GRAD_BOUND``, ``FLIP_SHARE``, 1e-4 for the net's iteration-0 gradients), with every
decision value exact.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import qat_cases as qc
import tpsq_cases as tc
from qat_minicfg import PARAMETERS, SIZE, STEPS, micro_cfg
from test_qat import FLIP_SHARE, GRAD_BOUND

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
PKG = os.path.join(os.path.dirname(HERE), 'yolov3v4-modelcompression-multidatasettraining-multibackbone_amd')


def _Q():
    return tc.native_module()


@pytest.fixture(scope='module')
def elementwise_golden():
    return np.load(os.path.join(GOLDEN, 'tpsq_elementwise.npz'))


def same(a, b):
    """Equal, NaNs in the same places."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ------------------------------------------------------------------------------------------------ 1. no reference needed
_STANDALONE = r'''
import os, sys, torch
sys.path[:0] = [%(pkg)r, %(tests)r]
import models
import utils.quantized.quantized_TPSQ as Q
import utils.quantized.quantized_google as G
assert os.path.abspath(Q.__file__).startswith(%(pkg)r + os.sep), Q.__file__
from qat_minicfg import micro_cfg, SIZE, STEPS
torch.manual_seed(0)
m = models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=2, a_bit=8, w_bit=8, steps=STEPS)
assert type(m.module_list[0][0]) is Q.TPSQ_BNFold_QuantizedConv2d_For_FPGA
kinds = {type(b) for b in m.module_list}
assert G.QuantizedFeatureConcat in kinds and models.Shortcut in kinds, kinds
x = torch.rand(2, 3, SIZE, SIZE)
m.train()
heads = m(x)[0]
sum(p.pow(2).mean() for p in heads).backward()
assert all(torch.isfinite(p).all() for p in heads)
grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
assert all(torch.isfinite(g).all() for g in grads.values())
assert sum(k.endswith('quantizer.scale') for k in grads) == 36
m.eval()
with torch.no_grad():
    inf = m(x)[0]
assert torch.isfinite(inf).all()
print('standalone ok')
'''


def test_quantized_2_builds_and_runs_without_a_reference_checkout(tmp_path):
    empty = tmp_path / 'no_reference'
    empty.mkdir()
    env = dict(os.environ, YOLO_REFERENCE_ROOT=str(empty), PYTHONDONTWRITEBYTECODE='1')
    res = subprocess.run([sys.executable, '-c', _STANDALONE % dict(pkg=PKG, tests=HERE)], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0 and 'standalone ok' in res.stdout, res.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ 2. contract
def test_state_dict_contract():
    import models
    _Q()
    z = np.load(os.path.join(GOLDEN, 'tpsq_net.npz'))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init.')}
    assert len(init) == tc.NET_STATE_KEYS
    torch.manual_seed(1)
    m = models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=2, a_bit=8, w_bit=8, steps=STEPS)
    assert sum(p.numel() for p in m.parameters()) == PARAMETERS + tc.NET_SCALES
    own = m.state_dict()
    assert set(own) == set(init)
    for k, v in own.items():
        assert tuple(v.shape) == tuple(init[k].shape) and v.dtype == init[k].dtype, k
    m.load_state_dict(init, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, init[k]), k


def test_constructor_quirks():
    Q = _Q()
    conv = Q.TPSQ_BNFold_QuantizedConv2d_For_FPGA(3, 4, 1, steps=50)
    assert conv.freeze_step == 45 and conv.momentum == 0.01
    assert conv.activation_quantizer.warmup.item() == 1 and conv.weight_quantizer.warmup.item() == 0
    assert isinstance(conv.activation_quantizer.scale, torch.nn.Parameter) and not isinstance(conv.bias_quantizer.scale, torch.nn.Parameter)
    assert tuple(Q.Weight_Quantizer(8, 5, True).scale.shape) == (5, 1, 1, 1) and tuple(Q.Activattion_Quantizer(8, 5, True).scale.shape) == (1, 5, 1, 1)
    with pytest.raises(NotImplementedError):
        Q.TPSQ_BNFold_QuantizedConv2d_For_FPGA(3, 4, 1, quantizer_output=True)(torch.zeros(1, 3, 2, 2))


def test_train_py_groups_the_scales():
    """train.py puts parameters whose name contains 'scale' into their own group: both learnable scales of every block land there."""
    Q = _Q()
    names = [k for k, _ in Q.TPSQ_BNFold_QuantizedConv2d_For_FPGA(3, 4, 1, bn=1).named_parameters()]
    assert [k for k in names if 'scale' in k] == ['activation_quantizer.scale', 'weight_quantizer.scale']


# ------------------------------------------------------------------------------------------------ 3. the quantisers, one by one
def _assert_exact(got, want, what, skip=()):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) | set(skip) == set(w) | set(skip), (what, k, sorted(set(g) ^ set(w)))
        for f in w:
            if f not in skip:
                assert same(g[f], w[f]), '%s call %d %s: got %s want %s' % (what, k, f, g[f].flatten()[:6], w[f].flatten()[:6])


@pytest.mark.parametrize('name', tc.ELEMENTWISE)
def test_quantisers_match_the_reference_exactly(name, elementwise_golden):
    """Outputs, input and scale gradients, the values Search_Pow2 saw (the 99 candidates and the chosen ``step * max_step`` of a
    warm-up call among them) and every buffer and parameter after each call."""
    calls = qc.recorded_calls(elementwise_golden, name)
    want = qc.unflatten(elementwise_golden, name)
    assert len(calls) == len(want) >= 2
    _assert_exact(tc.elementwise_records(_Q(), name, calls), want, name)


def test_fixture_covers_what_it_claims(elementwise_golden):
    z = elementwise_golden
    sp = z['act-leaky-8.0.sp']
    assert sp.size == 4 * 100 and z['act-leaky-8.0.sd.warmup'] == 0 and z['wgt-8.0.sp'].size == 4
    step = sp[0]
    chosen = sp[-4] / step
    assert abs(chosen - round(chosen)) < 1e-3 and 1 <= round(chosen) <= 99                 # step * max_step
    for name in ('act-leaky-8', 'act-leaky-4', 'wgt-8'):
        for k, mult in ((2, 1.3), (3, 0.7)):                                                   # the p / s0 factor is exercised
            s0, p = z['%s.%d.sp' % (name, k)][:2]
            before = z['%s.%d.sd.scale' % (name, k - 1)][0]
            assert s0 == np.float32(before * np.float32(mult)) and s0 != p and p == tc.nearest_pow2(float(s0))
    assert z['act-dead-8.0.sp'][-4] == 0 and np.signbit(z['act-dead-8.0.sp'][-4])             # step 0 * max_step -5
    assert np.isnan(z['act-dead-8.0.out']).all()
    assert z['act-evalwarm-8.0.sp'].size == 400 and z['act-evalwarm-8.0.sd.warmup'] == 0


def test_search_pow2_ties_and_bad_scales():
    Q = _Q()
    for s0, want in ((1.5, 1.0), (float(np.nextafter(np.float32(1.5), np.float32(2))), 2.0), (3.0, 2.0), (0.7, 0.5), (5.2, 4.0), (0.25, 0.25)):
        p = torch.nn.Parameter(torch.tensor([s0]))
        out = Q.Search_Pow2.apply(p)
        assert p.item() == want and out.item() == want
        out.backward(torch.ones(1))
        assert p.grad.item() == np.float32(want) / np.float32(s0)
    for s0 in (0.0, -1.0, float('nan')):
        q = Q.Weight_Quantizer(8, -1, True)
        with torch.no_grad():
            q.scale.fill_(s0)
        assert torch.isnan(q(torch.randn(9))).all()


# ------------------------------------------------------------------------------------------------ 4. the conv module
def check_conv_records(got, want, name):
    """Records with ``bound.<quantiser>.scale`` entries (the fused branch) have their scale gradients held to those."""
    assert len(got) == len(want) == 11
    for k, (g, w) in enumerate(zip(got, want)):
        assert {f for f in g if not f.startswith('bound.')} == set(w)
        for f in w:
            tag = '%s call %d %s' % (name, k, f)
            if 'bound.' + f[3:] in g:
                assert abs(float(g[f]) - float(w[f])) <= float(g['bound.' + f[3:]]), (tag, g[f], w[f], g['bound.' + f[3:]])
            elif f.startswith('sd.') and tc.is_decision(f):
                assert torch.equal(g[f], w[f]), (tag, g[f], w[f])
            elif f == 'out':
                step = float(g['sd.activation_quantizer.scale']) / 128
                d = (g[f] - w[f]).abs()
                moved = d != 0
                assert moved.float().mean().item() <= FLIP_SHARE, tag
                assert bool(((d[moved] - step).abs() <= 1e-6 * step).all()), tag
            else:
                assert qc.rel_l2(g[f], w[f]) <= GRAD_BOUND, (tag, qc.rel_l2(g[f], w[f]))


def _conv_fixture(name):
    z = np.load(os.path.join(GOLDEN, 'tpsq_conv_%s.npz' % name))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init.')}
    calls = [[torch.from_numpy(z['in.%d.0' % k])] for k in range(11)]
    return init, calls, qc.unflatten(z, 'call')


@pytest.mark.parametrize('name', [c[0] for c in tc.CONV_CASES])
def test_bnfold_conv_matches_the_reference(name):
    """Ten training calls (the warm-up, both scales moved off their powers twice, the BN freeze) and one eval call."""
    Q = _Q()
    kwargs = {c[0]: c[1] for c in tc.CONV_CASES}[name]
    init, calls, want = _conv_fixture(name)
    mod = tc.make_conv(Q, kwargs, seed=123)
    mod.load_state_dict(init, strict=True)
    check_conv_records(tc.run_conv(mod, calls), want, name)


# ------------------------------------------------------------------------------------------------ 5. the micro net
def test_micro_net_decisions_and_first_gradients():
    """20 training iterations without weight updates: every decision buffer exactly; iteration-0 gradients within 1e-4 rel-l2."""
    import models
    _Q()
    z = np.load(os.path.join(GOLDEN, 'tpsq_net.npz'))
    m = models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=2, a_bit=8, w_bit=8, steps=STEPS)
    m.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init.')}, strict=True)
    grads, state = qc.run_net(m, z['frames'])
    final = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('final.')}
    assert len(final) > 100 and set(final) == {k for k in state if tc.is_decision(k)}
    for k, v in final.items():
        assert torch.equal(state[k], v), (k, state[k], v)
    want = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('grad0.')}
    assert set(want) == set(grads) and sum(k.endswith('quantizer.scale') for k in want) == tc.NET_SCALES
    for k, v in want.items():
        assert qc.rel_l2(grads[k], v) <= 1e-4, (k, qc.rel_l2(grads[k], v))


# ------------------------------------------------------------------------------------------------ 6. the device branch, emulated
@pytest.fixture
def emulated(monkeypatch):
    import fakelib_tpsq
    from engine import qat, tpsq
    lib = fakelib_tpsq.FakeLibTpsq()
    for mod in (qat, tpsq):
        monkeypatch.setattr(mod, '_lib_override', lib)
        monkeypatch.setattr(mod, '_force_device', True)
    monkeypatch.delenv('YOLO_TPSQ_TORCH', raising=False)
    return lib


def scale_grad_bound(x, p, bits, dy):
    """2^-19 of the absolute sum of each of the four per-element term sets, added up (p / s0 <= 1.5 on the first)."""
    terms = tc.torch_fake_quant(x.reshape(-1), torch.tensor([p]), bits, dy.reshape(-1))[2]
    return 2.0 ** -19 * sum((1.5 if k == 0 else 1.0) * t.double().abs().sum().item() for k, t in enumerate(terms))


@pytest.mark.parametrize('name', tc.ELEMENTWISE)
def test_device_branch_equals_torch_branch_on_the_host_emulation(name, elementwise_golden, emulated):
    """y and dx bit for bit, every decision (snapped scales, the warm-up's choice, the flag, tracker and bias buffers) equal, the scale
    gradient within 2^-19 of its terms' absolute sums."""
    calls = qc.recorded_calls(elementwise_golden, name)
    want = qc.unflatten(elementwise_golden, name)
    got = tc.elementwise_records(_Q(), name, calls, record_sp=False)
    _assert_exact(got, want, name + ' (emulated device branch)', skip=('sp', 'gp.scale'))
    if name.startswith('bias-'):
        assert 'observe' in emulated.qat_calls and 'update' in emulated.qat_calls and 'fwd' in emulated.qat_calls
        return
    bits = {c[0]: c[2] for c in tc.QUANT_CASES}[name]
    for k, (g, w) in enumerate(zip(got, want)):
        p = float(w['sd.scale'])
        if np.isfinite(p) and p > 0:
            bound = scale_grad_bound(calls[k][0], p, bits, qc.upstream(w['out']))
            assert abs(float(g['gp.scale']) - float(w['gp.scale'])) <= bound, (name, k, g['gp.scale'], w['gp.scale'], bound)
        else:
            assert torch.isnan(g['gp.scale']).all() and torch.isnan(w['gp.scale']).all()
    warm = {c[0]: c[3] for c in tc.QUANT_CASES}[name]
    assert emulated.qat_calls.count('tpsq_warmup') == (1 if warm else 0) and emulated.qat_calls.count('tpsq_fwd') == len(calls)


def test_warmup_entry_point_chooses_the_recorded_candidate(elementwise_golden, emulated):
    from engine import tpsq
    for name, bits in (('act-leaky-8', 8), ('act-leaky-4', 4), ('act-relu6-8', 8), ('wgt-warm-8', 8), ('act-dead-8', 8)):
        x = torch.from_numpy(elementwise_golden[name + '.in.0.0'])
        scale, warmup = torch.ones(1), torch.ones(1)
        tpsq.warmup_search(x, scale, warmup, bits)
        want = elementwise_golden[name + '.0.sp'][-4]
        assert scale.item() == want and np.signbit(scale.numpy()[0]) == np.signbit(want) and warmup.item() == 0, (name, scale, want)


@pytest.mark.parametrize('name', [c[0] for c in tc.CONV_CASES])
def test_conv_device_branch_on_the_host_emulation(name, emulated):
    """The conv module's fused branch (host mirrors of step / first_bn / warmup) against the fixture; it reads its buffers once."""
    Q = _Q()
    kwargs = {c[0]: c[1] for c in tc.CONV_CASES}[name]
    init, calls, want = _conv_fixture(name)
    mod = tc.make_conv(Q, kwargs, seed=123)
    mod.load_state_dict(init, strict=True)
    check_conv_records(tc.run_conv(mod, calls, bounds=True), want, name + ' (emulated device branch)')
    assert emulated.qat_calls.count('tpsq_warmup') == 1 and emulated.qat_calls.count('tpsq_fwd') == 22
    assert mod._mirror is not None and mod._mirror[0] == 10 and mod.activation_quantizer._mirror == 0


def test_entry_points_check_their_arguments(emulated):
    x, y, s, snap, g = torch.randn(40), torch.empty(40), torch.ones(1), torch.empty(2), torch.empty(1)
    ws = torch.empty(64, dtype=torch.float64)
    P = lambda t: t.data_ptr()
    lib = emulated
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 40, P(s), 8, P(snap), None) == 0
    assert lib.yh_tpsq_fake_quant_fwd(None, P(y), 40, P(s), 8, P(snap), None) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 40, None, 8, P(snap), None) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 40, P(s), 8, None, None) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 0, P(s), 8, P(snap), None) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 40, P(s), 1, P(snap), None) != 0
    need = lib.yh_tpsq_grad_workspace(40)
    assert need == 16 and lib.yh_tpsq_grad_workspace(0) == 0 and lib.yh_tpsq_grad_workspace(4097) == 32
    assert lib.yh_tpsq_fake_quant_bwd(P(x), P(x), P(y), 40, P(snap), 8, P(ws), need, P(g), None) == 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), P(x), P(y), 40, P(snap), 8, P(ws), need - 4, P(g), None) != 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), None, P(y), 40, P(snap), 8, P(ws), need, P(g), None) != 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), P(x), P(y), 40, P(snap), 8, None, need, P(g), None) != 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), P(x), P(y), 0, P(snap), 8, P(ws), need, P(g), None) != 0
    need = lib.yh_tpsq_warmup_workspace(40)
    step, w = torch.tensor([0.01]), torch.ones(1)
    assert need == 8 * 19 and lib.yh_tpsq_warmup_workspace(0) == 0
    assert lib.yh_tpsq_warmup_search(P(x), 40, P(step), 8, P(ws), need, P(s), P(w), None) == 0 and w.item() == 0
    assert lib.yh_tpsq_warmup_search(P(x), 40, P(step), 8, P(ws), need - 8, P(s), P(w), None) != 0
    assert lib.yh_tpsq_warmup_search(P(x), 40, None, 8, P(ws), need, P(s), P(w), None) != 0
    assert lib.yh_tpsq_warmup_search(P(x), 0, P(step), 8, P(ws), need, P(s), P(w), None) != 0
    assert w.item() == 0


def test_the_emulation_snaps_like_the_reference():
    import fakelib_tpsq
    x = qc.sweep_values()
    got = np.array([fakelib_tpsq.pow2(v) for v in x], dtype=np.float32)
    assert np.array_equal(got, qc.reference_pow2(x))
    z = fakelib_tpsq.pow2(np.float32(-0.0))
    assert z == 0 and not np.signbit(z) and np.isnan(fakelib_tpsq.pow2(-1.0)) and np.isnan(fakelib_tpsq.pow2(np.nan))
