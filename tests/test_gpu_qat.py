"""GPU tier of the QAT kernels (csrc/qat.hip) and of the modules' fused path (utils/quantized/quantized_google.py -> engine/qat.py).

The kernels are called through the C ABI on buffers of this test's own (alignment, guard floats) and compared with the torch
formulas evaluated on the CPU; the modules run their fused path against ``YOLO_QAT_TORCH=1`` in the same process.  Every replaced
operation is one IEEE fp32 operation in a fixed order (or an exact min / max), so there is no tolerance to choose: where the torch
path reproduces itself bit for bit, the fused path must equal it.

Backward reference: autograd through the torch formulas, i.e. ``((dy * s) * mask) / s`` - which is ``dy * mask`` for power-of-two
scales.  Without a clamp the contract is the identity with no launch (include/yolo_hip.h), which is what autograd gives for the
power-of-two scales the clamp-free call sites (``QuantizedShortcut_min``'s inputs) have; there the test expects ``dy`` itself.
"""
import os
import sys

import numpy as np
import pytest
import torch

import conftest

sys.path.insert(0, os.path.join(conftest.REPO, 'tests'))
import qat_cases as qc  # noqa: E402
from qat_minicfg import SIZE, STEPS, micro_cfg  # noqa: E402
from engine import hiplib, qat  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 12345.0
WRAP = 1024 * 256 * 16 + 4096 + 3      # past the block cap of the launch: every thread of the largest grid loops again
COUNTS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4097, WRAP]
SCALES = {'pow2': (2.0 ** -4, 0.0), 'odd': (float(np.float32(3.7) / np.float32(255)), 37.0)}


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load()


@pytest.fixture(scope='module', autouse=True)
def release_cached_blocks():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def Q():
    return qc.native_module()


@pytest.fixture(scope='module')
def elementwise_golden():
    return np.load(os.path.join(conftest.REPO, 'tests', 'golden', 'qat_elementwise.npz'))


@pytest.fixture
def torch_path(monkeypatch):
    def set_(on):
        if on:
            monkeypatch.setenv('YOLO_QAT_TORCH', '1')
        else:
            monkeypatch.delenv('YOLO_QAT_TORCH', raising=False)
    set_(False)
    return set_


def placed(host, offset):
    """``host`` copied into a device buffer ``offset`` floats past a 256-byte-aligned base, one guard float behind it."""
    n = host.numel()
    buf = torch.full((n + offset + 1,), GUARD, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n]
    view.copy_(host)
    return buf, view


def same_values(got, want):
    """Equal as values: NaNs in the same places, the sign of a zero free."""
    got, want = got.cpu(), want.cpu()
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


def special_inputs(n, scale, zp, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    span = (hi - lo) * scale
    x = (torch.rand(n, generator=g) - 0.5) * (1.5 * span) + ((lo + hi) / 2 - zp) * scale      # a quarter of them beyond the clamp ends
    s = np.float32(scale)
    special = [float('nan'), float('inf'), float('-inf'), 0.0, -0.0, 1e-41, float(np.float32(0.49999997) * s)]
    special += [float(np.float32(k + 0.5) * s) for k in (0, 1, 2, 7, -1, -2, -8)]
    special += [float(np.float32(k + 0.5 - zp) * s) for k in (lo, hi, hi - 1, lo - 1, hi + 3)]
    special += [float(np.float32(lo - zp - 40) * s), float(np.float32(hi - zp + 40) * s)]
    special = torch.tensor(special, dtype=torch.float32)
    k = min(n, len(special))
    pick = torch.arange(k) if n >= len(special) else (torch.arange(k) * 5 + seed) % len(special)
    x[:k] = special[pick]
    return x


def torch_fake_quant(Q, x, scale, zp, lo, hi, clamp, dy):
    """The modules' torch formulas (reference quantized_google.py:114-136) on the CPU, and their autograd gradient."""
    x = x.clone().requires_grad_(True)
    s, z = torch.tensor([scale], dtype=torch.float32), torch.tensor([zp], dtype=torch.float32)
    r = Q.Round.apply(x / s + z)
    if clamp:
        r = torch.clamp(r, torch.tensor(lo), torch.tensor(hi))
    y = (r - z) * s
    y.backward(dy)
    return y.detach(), x.grad


# ------------------------------------------------------------------------------------------------ 8. fake-quant forward / backward
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned16', 'offset1'])
@pytest.mark.parametrize('scale_name', ['pow2', 'odd'])
def test_fake_quant_kernels_against_the_torch_formula(lib, Q, scale_name, offset):
    scale, zp = SCALES[scale_name]
    stream = hiplib.stream_ptr()
    sc = torch.tensor([scale], dtype=torch.float32, device='cuda')
    zpt = torch.tensor([zp], dtype=torch.float32, device='cuda')
    for n in COUNTS:
        for sign, bits, clamp in [(s, b, c) for s in (True, False) for b in (8, 4) for c in (True, False)]:
            if n == WRAP and (bits, clamp) != (8, True):
                continue          # the 16 MB case once per sign, alignment and scale
            lo, hi = qat.limits(bits, sign)
            x = special_inputs(n, scale, zp, lo, hi, seed=n % 97 + bits)
            dy = qc.upstream(x)
            want_y, want_dx = torch_fake_quant(Q, x, scale, zp, lo, hi, clamp, dy)
            xb, xv = placed(x, offset)
            yb, yv = placed(torch.zeros(n), offset)
            snap = torch.full((3,), GUARD, device='cuda')
            step = torch.tensor([4.0, GUARD], device='cuda')
            hiplib.check(lib.yh_qat_fake_quant_fwd(hiplib.ptr(xv), hiplib.ptr(yv), n, hiplib.ptr(sc), hiplib.ptr(zpt), float(lo), float(hi),
                                                   1 if clamp else 0, hiplib.ptr(snap), hiplib.ptr(step), stream), 'fwd')
            tag = (scale_name, offset, n, sign, bits, clamp)
            assert same_values(yv, want_y), tag
            assert yb[-1].item() == GUARD and (offset == 0 or yb[0].item() == GUARD), tag
            assert snap.tolist() == [np.float32(scale), zp, GUARD] and step.tolist() == [5.0, GUARD], tag
            assert torch.equal(xb.cpu()[offset:offset + n].isnan(), x.isnan()) and xb[-1].item() == GUARD, tag
            if not clamp:
                continue          # no backward launch without a clamp: the identity (engine/qat.py)
            gb, gv = placed(dy, offset)
            db, dv = placed(torch.zeros(n), offset)
            hiplib.check(lib.yh_qat_fake_quant_bwd(hiplib.ptr(xv), hiplib.ptr(gv), hiplib.ptr(dv), n, hiplib.ptr(snap), float(lo), float(hi),
                                                   stream), 'bwd')
            assert same_values(dv, want_dx), tag
            assert db[-1].item() == GUARD and (offset == 0 or db[0].item() == GUARD), tag
            assert not torch.isnan(dv).any(), tag          # a NaN input is outside the mask: 0


def test_fake_quant_function_without_clamp_is_the_identity_backward(lib, Q, torch_path):
    x = special_inputs(257, 2.0 ** -4, 0.0, -128, 127, seed=3)[3:]          # no NaN / inf: the torch gradient is dy there too
    sc = torch.tensor([2.0 ** -4], device='cuda')
    xd = x.cuda().requires_grad_(True)
    y = qat.fake_quant(xd, sc, None, 8, True, clamp=False)
    dy = qc.upstream(y)
    y.backward(dy)
    want_y, want_dx = torch_fake_quant(Q, x, 2.0 ** -4, 0.0, -128, 127, False, dy.cpu())
    assert same_values(y.detach(), want_y) and torch.equal(xd.grad.cpu(), dy.cpu()) and torch.equal(want_dx, dy.cpu())


# ------------------------------------------------------------------------------------------------ 9. observe
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned16', 'offset1'])
def test_observe_is_exact(lib, offset):
    stream = hiplib.stream_ptr()
    for n in COUNTS:
        g = torch.Generator().manual_seed(n % 89)
        x = torch.randn(n, generator=g) * 3 + 0.5
        xb, xv = placed(x, offset)
        ws = torch.empty(max(int(lib.yh_qat_observe_workspace(n)), 4) // 4 + 1, device='cuda').fill_(GUARD)
        out = torch.full((3,), GUARD, device='cuda')
        hiplib.check(lib.yh_qat_observe(hiplib.ptr(xv), n, hiplib.ptr(ws), (ws.numel() - 1) * 4, hiplib.ptr(out), stream), 'observe')
        assert out.tolist() == [x.min().item(), x.max().item(), GUARD], (n, offset)
        assert ws[-1].item() == GUARD and xb[-1].item() == GUARD
    for n, at in ((1, 0), (257, 256), (4097, 1234), (WRAP, WRAP - 2)):
        x = torch.randn(n)
        x[at] = float('nan')
        _, xv = placed(x, offset)
        assert torch.isnan(qat.observe(xv)).all(), (n, at)
    all_negative = -torch.rand(300) - 1          # the identity of max must not leak into the result
    assert qat.observe(placed(all_negative, offset)[1]).tolist() == [all_negative.min().item(), all_negative.max().item()]


def test_observe_takes_a_permuted_view_without_a_copy(lib):
    t = torch.randn(2, 5, 7, 3, device='cuda')
    view = t.permute(0, 3, 1, 2)
    assert not view.is_contiguous() and qat._dense(view).data_ptr() == t.data_ptr()
    assert qat.observe(view).tolist() == [t.min().item(), t.max().item()]
    strided = t[:, ::2]                           # not dense: copied, same answer
    assert qat.observe(strided).tolist() == [strided.min().item(), strided.max().item()]


# ------------------------------------------------------------------------------------------------ 10. range / scale update
@pytest.mark.parametrize('case', qc.QUANT_CASES, ids=[c[0] for c in qc.QUANT_CASES])
def test_range_update_follows_the_reference_sequence(lib, Q, elementwise_golden, case):
    """observe + range_update on the recorded inputs of the calibrating calls: tracker, flag, scale and zero point after each call
    are the reference's, exactly."""
    name, cls, tracker, sign, bits = case
    want = qc.unflatten(elementwise_golden, 'q.' + name)
    calls = qc.recorded_calls(elementwise_golden, 'q.' + name)
    q = qc.make_quantizer(Q, cls, tracker, sign, bits).cuda()
    first = 'first_a' if tracker.startswith('Averaged') else 'first_w'
    for k in range(qc.QUANT_FREEZE):
        qat.observe_update(calls[k][0].cuda(), q.range_tracker, q)
        got = {'scale': q.scale, 'zero_point': q.zero_point, 'range_tracker.min_val': q.range_tracker.min_val,
               'range_tracker.max_val': q.range_tracker.max_val, 'range_tracker.' + first: getattr(q.range_tracker, first)}
        for key, v in got.items():
            assert torch.equal(v.cpu(), want[k]['sd.' + key]), (name, k, key, v.cpu(), want[k]['sd.' + key])


def test_power_of_two_selection_on_the_device(lib, Q):
    x = qc.sweep_values()
    want = qc.reference_pow2(x)
    q = qc.make_quantizer(Q, 'SymmetricQuantizer', 'AveragedRangeTracker', True, 8).cuda()
    mm = torch.stack([torch.from_numpy(-x / 2), torch.from_numpy(x)], 1).cuda()
    got = []
    for k in range(len(x)):
        q.range_tracker.first_a.zero_(); q.range_tracker.min_val.zero_(); q.range_tracker.max_val.zero_()
        qat.range_update(mm[k], q.range_tracker, q)
        got.append(q.scale.clone())
    assert np.array_equal(torch.cat(got).cpu().numpy() * np.float32(128), want)
    q.range_tracker.first_a.zero_(); q.range_tracker.min_val.zero_(); q.range_tracker.max_val.zero_()
    qat.range_update(torch.zeros(2, device='cuda'), q.range_tracker, q)
    assert q.scale.item() == 0.0 and q.range_tracker.first_a.item() == 1.0          # x == 0 gives scale 0, as in the reference


# ------------------------------------------------------------------------------------------------ 11. modules: fused against torch
def _records_equal(a, b, what):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert set(ra) == set(rb)
        for f in ra:
            assert torch.equal(ra[f], rb[f]), '%s call %d %s: %d of %d differ' % (what, k, f, int((ra[f] != rb[f]).sum()), ra[f].numel())


@pytest.mark.parametrize('name', qc.ELEMENTWISE)
def test_elementwise_modules_fused_equals_torch_on_the_device(lib, Q, elementwise_golden, torch_path, name):
    _, make, _, n_train, fwd = {c[0]: c for c in qc.elementwise_cases(Q)}[name]
    calls = qc.recorded_calls(elementwise_golden, name)
    torch_path(True)
    want = qc.run_sequence(make(), calls, n_train, fwd, device='cuda')
    torch_path(False)
    got = qc.run_sequence(make(), calls, n_train, fwd, device='cuda')
    _records_equal(got, want, name)


def _compare_runs(run, torch_path, what):
    """``run()`` -> {name: host tensor}.  Torch path twice, then the fused path: equal where the torch path reproduces itself,
    otherwise within 4 x its own run-to-run rel-l2; decision buffers always exactly."""
    torch_path(True)
    a, b = run(), run()
    torch_path(False)
    got = run()
    assert set(got) == set(a)
    noise = max(qc.rel_l2(a[k], b[k]) for k in a)
    reproducible = all(torch.equal(a[k], b[k]) for k in a)
    worst = max(qc.rel_l2(got[k], a[k]) for k in a)
    print('%s: torch path run-to-run rel-l2 %.3g (%s), fused against torch %.3g' % (what, noise, 'bit-reproducible' if reproducible else 'not reproducible', worst))
    for k in a:
        if qc.is_decision(k):
            assert torch.equal(got[k], a[k]), (what, k, got[k], a[k])
        elif reproducible:
            assert torch.equal(got[k], a[k]), (what, k, qc.rel_l2(got[k], a[k]))
        else:
            assert qc.rel_l2(got[k], a[k]) <= 4 * noise, (what, k, qc.rel_l2(got[k], a[k]), noise)


@pytest.fixture
def deterministic_convs():
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize('case', qc.CONV_CASES, ids=[c[0] for c in qc.CONV_CASES])
def test_conv_module_fused_equals_torch_on_the_device(lib, Q, torch_path, deterministic_convs, case):
    name, kwargs, _ = case
    z = np.load(os.path.join(conftest.REPO, 'tests', 'golden', 'qat_conv_%s.npz' % name))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init.')}
    calls = [[torch.from_numpy(z['in.%d.0' % k])] for k in range(11)]

    def run():
        mod = qc.make_conv(Q, kwargs, seed=7)
        mod.load_state_dict(init, strict=True)
        rec = qc.run_sequence(mod, calls, 10, qc.fwd_single, device='cuda')
        return {'%d.%s' % (k, f): v for k, r in enumerate(rec) for f, v in r.items()}
    _compare_runs(run, torch_path, name)


@pytest.mark.parametrize('way', [1, 2])
def test_micro_net_fused_equals_torch_on_the_device(lib, Q, torch_path, deterministic_convs, way):
    import models
    z = np.load(os.path.join(conftest.REPO, 'tests', 'golden', 'qat_net_way%d.npz' % way))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init.')}
    frames = torch.from_numpy(z['frames']).float().div(256)

    def run():
        m = models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=1, a_bit=8, w_bit=8, steps=STEPS, shortcut_way=way)
        m.load_state_dict(init, strict=True)
        m.cuda().train()
        out = {}
        for it in range(3):
            m.zero_grad()
            heads = m(frames[it].cuda())[0]
            sum(p.pow(2).mean() for p in heads).backward()
            out.update({'it%d.head%d' % (it, j): p.detach().cpu() for j, p in enumerate(heads)})
            out.update({'it%d.grad.%s' % (it, k): p.grad.cpu().clone() for k, p in m.named_parameters() if p.grad is not None})
        m.eval()
        with torch.no_grad():
            out['eval.inf'] = m(frames[3].cuda())[0].cpu()
        out.update({'sd.' + k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        return out
    _compare_runs(run, torch_path, 'micro net way %d' % way)


# ------------------------------------------------------------------------------------------------ 12. no per-step host reads
def test_training_step_of_a_conv_module_reads_nothing_back(lib, Q, torch_path):
    torch.manual_seed(0)
    mod = Q.BNFold_QuantizedConv2d_For_FPGA(8, 16, 3, padding=1, bn=1, activate='leaky', steps=100).cuda().train()
    x = torch.randn(2, 8, 16, 16, device='cuda', requires_grad=True)
    g = torch.randn(2, 16, 16, 16, device='cuda')
    probe = torch.ones(1, device='cuda')
    (mod(x) * g).sum().backward()          # warm-up: the mirrors' one read per module, kernel loading
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            raised = False
        except RuntimeError:
            raised = True
        if raised:
            mod.zero_grad()
            (mod(x) * g).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not raised:
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag .item() on this build')
    torch.cuda.synchronize()
    assert mod.step.item() == 2 and mod.activation_quantizer.step.item() == 2 and mod.weight_quantizer.range_tracker.first_w.item() == 1
    assert mod.activation_quantizer.scale.item() > 0 and torch.isfinite(mod.weight.grad).all()
