"""GPU tier of the TPSQ kernels (csrc/tpsq.hip) and of the modules' fused path (utils/quantized/quantized_TPSQ.py -> engine/tpsq.py).

The kernels are called through the C ABI on buffers of this test's own (alignment, guard floats) and compared with the modules' torch
formulas (``YOLO_TPSQ_TORCH=1``) evaluated on the same device.  Every operation behind ``y`` and ``dx`` is one IEEE fp32 operation in
torch's order, so those are compared bit for bit (NaNs in the same places).  The scale gradient is a sum, taken in another order than
torch's: it is held to ``2^-19 * sum |t_i|`` per sum of per-element terms - a two-stage tree over at most 2^20 elements has at most 32
roundings of 2^-24 each on any path from a term to the result - against the float64 sum of the same fp32 terms, and torch's own fp32
result is held to the same bound.
"""
import os
import sys

import numpy as np
import pytest
import torch

import conftest

sys.path.insert(0, os.path.join(conftest.REPO, 'tests'))
import qat_cases as qc  # noqa: E402
import tpsq_cases as tc  # noqa: E402
from qat_minicfg import SIZE, STEPS, micro_cfg  # noqa: E402
from engine import hiplib, tpsq  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 12345.0
# The launch has min(1024, ceil(count / 4096)) workgroups of 256 threads; with 16-byte loads one sweep of the largest grid covers
# 1024 * 256 * 4 elements.  1024 * 256 * 16 elements are four full sweeps of it; 4096 + 3 more start a fifth and leave a scalar tail.
WRAP = 1024 * 256 * 16 + 4096 + 3
COUNTS = [1, 255, 1027, 2 * 16 * 52 * 52, WRAP]
ONE_AND_A_HALF_UP = float(np.nextafter(np.float32(1.5 * 2.0 ** -3), np.float32(1)))
SCALES = {'pow2': 2.0 ** -2, 'tie': 1.5 * 2.0 ** -3, 'above-tie': ONE_AND_A_HALF_UP, '0.7': 0.7, '5.2': 5.2}
SNAPPED = {'pow2': 2.0 ** -2, 'tie': 2.0 ** -3, 'above-tie': 2.0 ** -2, '0.7': 0.5, '5.2': 4.0}


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
    return tc.native_module()


@pytest.fixture
def torch_path(monkeypatch):
    def set_(on):
        if on:
            monkeypatch.setenv('YOLO_TPSQ_TORCH', '1')
        else:
            monkeypatch.delenv('YOLO_TPSQ_TORCH', raising=False)
    set_(False)
    return set_


def placed(values, offset):
    """``values`` copied into a device buffer ``offset`` floats past a 16-byte-aligned base, one guard float behind it."""
    n = values.numel()
    buf = torch.full((n + offset + 1,), GUARD, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n]
    view.copy_(values)
    return buf, view


def same_bits(got, want):
    """Bit for bit, NaNs in the same places (their payloads free)."""
    got, want = got.reshape(-1), want.reshape(-1)
    return bool(((got.view(torch.int32) == want.view(torch.int32)) | (got.isnan() & want.isnan())).all())


def special_inputs(n, p, bits, seed):
    """Random values over [-2p, 2p] with, in front, the clamp ends and their float neighbours, rounding ties of the grid, zeros,
    subnormals, infinities and a NaN."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) - 0.5) * (4 * p)
    f, qmul = np.float32, (1 << (bits - 1)) - 1
    special = [p, -p, float(np.nextafter(f(p), f(0))), float(np.nextafter(f(p), f(2 * p))), float(np.nextafter(f(-p), f(0))),
               float(np.nextafter(f(-p), f(-2 * p))), 0.0, -0.0, 1e-41, -1e-41, float('inf'), float('-inf'), float('nan')]
    special += [float(f(p) * f(k + 0.5) / f(qmul)) for k in (0, 1, 2, qmul - 1, -1, -2, -qmul)]
    special = torch.tensor(special, dtype=torch.float32)
    k = min(n, len(special))
    pick = torch.arange(k) if n >= len(special) else (torch.arange(k) * 5 + seed) % len(special)
    x[:k] = special[pick]
    return x


def torch_call(Q, x, s0, bits, dy):
    """One call of a quantiser on the torch formulas, on the device: (y, dx, scale.grad, scale afterwards)."""
    q = Q.Weight_Quantizer(bits, -1, True).cuda()
    with torch.no_grad():
        q.scale.fill_(s0)
    xg = x.clone().requires_grad_(True)
    y = q(xg)
    y.backward(dy)
    return y.detach(), xg.grad, q.scale.grad.clone(), q.scale.detach().clone()


def kernel_call(lib, x, s0, bits, dy, offset):
    """The same call through the C ABI on guarded buffers: (y, dx, scale gradient, scale afterwards, snapshot, workspace)."""
    n, stream = x.numel(), hiplib.stream_ptr()
    xb, xv = placed(x, offset)
    yb, yv = placed(torch.zeros(n), offset)
    scale = torch.tensor([s0, GUARD], dtype=torch.float32, device='cuda')
    snap = torch.full((3,), GUARD, device='cuda')
    hiplib.check(lib.yh_tpsq_fake_quant_fwd(hiplib.ptr(xv), hiplib.ptr(yv), n, hiplib.ptr(scale), bits, hiplib.ptr(snap), stream), 'fwd')
    gb, gv = placed(dy, offset)
    db, dv = placed(torch.zeros(n), offset)
    need = int(lib.yh_tpsq_grad_workspace(n))
    assert need == 16 * max(1, min(1024, -(-n // 4096)))
    ws = torch.full((need // 4 + 1,), GUARD, device='cuda')
    grad = torch.full((2,), GUARD, device='cuda')
    hiplib.check(lib.yh_tpsq_fake_quant_bwd(hiplib.ptr(xv), hiplib.ptr(gv), hiplib.ptr(dv), n, hiplib.ptr(snap), bits, hiplib.ptr(ws), need,
                                            hiplib.ptr(grad), stream), 'bwd')
    for b in (yb, db, xb, gb):
        assert b[-1].item() == GUARD and (offset == 0 or b[0].item() == GUARD)
    assert scale[1].item() == GUARD and snap[2].item() == GUARD and ws[-1].item() == GUARD and grad[1].item() == GUARD
    return yv, dv, grad[:1], scale[:1], snap[:2], ws[:-1]


# ------------------------------------------------------------------------------------------------ 1. forward / backward kernels
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned16', 'offset1'])
@pytest.mark.parametrize('scale_name', list(SCALES))
def test_fake_quant_kernels_against_the_torch_formulas(lib, Q, torch_path, scale_name, offset):
    s0, p = SCALES[scale_name], SNAPPED[scale_name]
    assert tc.nearest_pow2(s0) == p
    torch_path(True)
    for n in COUNTS:
        for bits in (8, 4):
            x = special_inputs(n, p, bits, seed=n % 97 + bits).cuda()
            dy = qc.upstream(x)
            want_y, want_dx, _, want_scale = torch_call(Q, x, s0, bits, dy)
            y, dx, _, scale, snap, _ = kernel_call(lib, x, s0, bits, dy, offset)
            tag = (scale_name, offset, n, bits)
            assert same_bits(y, want_y), tag
            assert same_bits(dx, want_dx), tag
            assert scale.item() == p == want_scale.item() and snap.tolist() == [np.float32(s0), p], tag


@pytest.mark.parametrize('s0', [0.0, -0.25], ids=['zero', 'negative'])
def test_bad_scales_give_torchs_nans(lib, Q, torch_path, s0):
    torch_path(True)
    for n, bits in ((1027, 8), (255, 4)):
        x = special_inputs(n, 0.25, bits, seed=5).cuda()
        dy = qc.upstream(x)
        want_y, want_dx, want_grad, want_scale = torch_call(Q, x, s0, bits, dy)
        y, dx, grad, scale, _, _ = kernel_call(lib, x, s0, bits, dy, 0)
        assert want_y.isnan().all() and torch.equal(y.isnan(), want_y.isnan())
        assert torch.equal(dx.isnan(), want_dx.isnan()) and same_bits(dx, want_dx)
        assert torch.equal(grad.isnan(), want_grad.isnan()) and same_bits(scale, want_scale)


def test_permuted_dense_view_is_not_copied(lib, Q, torch_path):
    t = torch.randn(2, 5, 7, 3, device='cuda')
    view = t.permute(0, 3, 1, 2)
    assert not view.is_contiguous() and tpsq._dense(view).data_ptr() == t.data_ptr()
    scale = torch.nn.Parameter(torch.tensor([0.7], device='cuda'))
    xg = view.clone(memory_format=torch.preserve_format).requires_grad_(True)
    assert xg.stride() == view.stride()
    y = tpsq.fake_quant(xg, scale, 8)
    assert y.stride() == view.stride() and scale.item() == 0.5
    dy = qc.upstream(y)
    y.backward(dy)
    torch_path(True)
    want_y, want_dx, want_grad, _ = torch_call(Q, view.contiguous(), 0.7, 8, dy.contiguous())
    assert torch.equal(y.detach().contiguous(), want_y) and torch.equal(xg.grad.contiguous(), want_dx)
    terms = tc.torch_fake_quant(view.contiguous(), torch.tensor([0.5], device='cuda'), 8, dy.contiguous())[2]
    assert abs(scale.grad.item() - want_grad.item()) <= 2 * 2.0 ** -19 * sum(t.double().abs().sum().item() for t in terms)


def test_entry_points_refuse_bad_arguments(lib):
    """Null pointers, count 0, bits out of range and an undersized workspace return an error code before anything is launched."""
    x, y = torch.zeros(40, device='cuda'), torch.zeros(40, device='cuda')
    s, snap, g, w = torch.ones(1, device='cuda'), torch.zeros(2, device='cuda'), torch.zeros(1, device='cuda'), torch.ones(1, device='cuda')
    ws = torch.zeros(64, dtype=torch.float64, device='cuda')
    P, stream = hiplib.ptr, hiplib.stream_ptr()
    assert lib.yh_tpsq_fake_quant_fwd(None, P(y), 40, P(s), 8, P(snap), stream) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 40, None, 8, P(snap), stream) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 40, P(s), 8, None, stream) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 0, P(s), 8, P(snap), stream) != 0
    assert lib.yh_tpsq_fake_quant_fwd(P(x), P(y), 40, P(s), 1, P(snap), stream) != 0
    need = int(lib.yh_tpsq_grad_workspace(40))
    assert need == 16 and lib.yh_tpsq_grad_workspace(0) == 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), P(x), P(y), 40, P(snap), 8, P(ws), need - 4, P(g), stream) != 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), None, P(y), 40, P(snap), 8, P(ws), need, P(g), stream) != 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), P(x), P(y), 40, P(snap), 8, None, need, P(g), stream) != 0
    assert lib.yh_tpsq_fake_quant_bwd(P(x), P(x), P(y), 0, P(snap), 8, P(ws), need, P(g), stream) != 0
    need = int(lib.yh_tpsq_warmup_workspace(40))
    assert need == 8 * 19 and lib.yh_tpsq_warmup_workspace(0) == 0
    assert lib.yh_tpsq_warmup_search(P(x), 40, P(g), 8, P(ws), need - 8, P(s), P(w), stream) != 0
    assert lib.yh_tpsq_warmup_search(P(x), 40, None, 8, P(ws), need, P(s), P(w), stream) != 0
    assert lib.yh_tpsq_warmup_search(P(x), 0, P(g), 8, P(ws), need, P(s), P(w), stream) != 0
    torch.cuda.synchronize()
    assert s.item() == 1 and w.item() == 1 and not y.any()


# ------------------------------------------------------------------------------------------------ 2. the scale gradient
def grad_case(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    p = 0.5
    if kind == 'one-sided':      # 0 < x < p and dy > 0: the terms of each of the four sums share a sign, nothing can hide in cancellation
        x = (0.05 + 0.9 * torch.rand(n, generator=g)) * p
        dy = 0.25 + torch.rand(n, generator=g)
    else:
        x = torch.randn(n, generator=g) * p
        dy = torch.randn(n, generator=g)
    return x.cuda(), dy.cuda()


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned16', 'offset1'])
@pytest.mark.parametrize('kind', ['mixed', 'one-sided'])
@pytest.mark.parametrize('n', [1027, 2 * 16 * 52 * 52, 1 << 20])
def test_scale_gradient_against_the_float64_sum(lib, Q, torch_path, n, kind, offset):
    s0, p, bits = 0.7, 0.5, 8
    x, dy = grad_case(kind, n, seed=n % 1000 + offset)
    torch_path(True)
    _, _, torch_grad, _ = torch_call(Q, x, s0, bits, dy)
    _, _, grad, _, _, ws = kernel_call(lib, x, s0, bits, dy, offset)
    terms = tc.torch_fake_quant(x, torch.tensor([p], device='cuda'), bits, dy)[2]
    if kind == 'one-sided':
        for t in terms:
            assert bool((t >= 0).all()) or bool((t <= 0).all())
    exact = [t.double().sum().item() for t in terms]
    room = [2.0 ** -19 * t.double().abs().sum().item() for t in terms]
    partial = ws.view(-1, 4).double().sum(0).tolist()      # the per-workgroup partials of each sum, as the finishing wave reads them
    for k in range(4):
        print('sum %d: kernel partials %.9g float64 %.9g bound %.3g' % (k + 1, partial[k], exact[k], room[k]))
        assert abs(partial[k] - exact[k]) <= room[k], (n, kind, offset, k)
    first = float(np.float32(p) / np.float32(s0))
    want = first * exact[0] + exact[1] + exact[2] + exact[3]
    bound = first * room[0] + room[1] + room[2] + room[3]
    print('scale gradient: kernel %.9g torch fp32 %.9g float64 %.9g bound %.3g' % (grad.item(), torch_grad.item(), want, bound))
    assert abs(torch_grad.item() - want) <= bound, 'the bound does not hold for torch itself: re-derive it'
    assert abs(grad.item() - want) <= bound
    _, _, again, _, _, ws2 = kernel_call(lib, x, s0, bits, dy, offset)
    assert same_bits(again, grad) and same_bits(ws2, ws)


# ------------------------------------------------------------------------------------------------ 3. the warm-up search
def warm_input(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    return torch.nn.functional.leaky_relu(x, 0.1) if kind == 'leaky' else torch.nn.functional.relu6(x + 0.5)


def cosine_gap(x, bits):
    """Best minus runner-up cosine over the distinct powers of the 99 candidates, float64 sums of fp32 elements, on the host."""
    step = x.max() / 100
    powers = sorted({tc.nearest_pow2(float(step * i)) for i in range(1, 100)})
    x64, cs = x.double(), []
    for p in powers:
        y = tc.torch_fake_quant(x, torch.tensor([p]), bits).double()
        cs.append(float((x64 * y).sum() / (x64.norm() * y.norm())))
    cs.sort(reverse=True)
    return cs[0] - cs[1]


@pytest.mark.parametrize('bits', [8, 4])
@pytest.mark.parametrize('kind', ['leaky', 'relu6'])
@pytest.mark.parametrize('n', [1027, 2 * 16 * 52 * 52])
def test_warmup_search_equals_the_torch_loop(lib, Q, torch_path, n, kind, bits):
    x = warm_input(kind, n, seed=n % 1000 + bits)
    assert cosine_gap(x, bits) > 1e-4
    xd = x.cuda()
    torch_path(True)
    ref = Q.Activattion_Quantizer(bits, -1, True).cuda()
    ref._search(xd)
    fused = Q.Activattion_Quantizer(bits, -1, True).cuda()
    tpsq.warmup_search(xd, fused.scale, fused.warmup, bits)
    print('warm-up %s n=%d bits=%d: torch %.9g fused %.9g' % (kind, n, bits, ref.scale.item(), fused.scale.item()))
    assert same_bits(fused.scale.detach(), ref.scale.detach()) and fused.warmup.item() == ref.warmup.item() == 0
    assert ref.scale.item() > 0


def test_warmup_search_without_a_winner(lib, Q, torch_path):
    """max(x) == 0: every cosine is NaN, max_step stays -5 and the scale becomes 0 * -5."""
    x = -torch.rand(1027).cuda()
    x[::3] = 0.0
    torch_path(True)
    ref = Q.Activattion_Quantizer(8, -1, True).cuda()
    ref._search(x)
    fused = Q.Activattion_Quantizer(8, -1, True).cuda()
    tpsq.warmup_search(x, fused.scale, fused.warmup, 8)
    assert ref.scale.item() == 0 and same_bits(fused.scale.detach(), ref.scale.detach()) and fused.warmup.item() == ref.warmup.item() == 0


# ------------------------------------------------------------------------------------------------ 4. modules: fused against torch
@pytest.fixture
def deterministic_convs():
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def _compare_runs(run, torch_path, what):
    """``run()`` -> {name: host tensor}; a scale gradient ``..gp.<q>.scale`` has its bound next to it as ``..bound.<q>.scale``.  Torch
    path twice, then the fused path.  Scale gradients: both paths sum the same fp32 terms and each lies within the bound of the exact
    sum (test_scale_gradient_against_the_float64_sum holds both to it), so they are within twice the bound of each other.  Decisions
    exactly.  Everything else bit-equal where the torch path reproduces itself, otherwise within 4 x its own run-to-run rel-l2."""
    torch_path(True)
    a, b = run(), run()
    torch_path(False)
    got = run()
    assert set(got) == set(a)
    bounded = [k for k in a if 'gp.' in k and k.replace('gp.', 'bound.', 1) in a]
    plain = [k for k in a if 'bound.' not in k and k not in bounded]
    reproducible = all(tc_same(a[k], b[k]) for k in plain)
    noise = max(qc.rel_l2(a[k], b[k]) for k in plain)
    worst = max(qc.rel_l2(got[k], a[k]) for k in plain)
    print('%s: torch path run-to-run rel-l2 %.3g (%s), fused against torch %.3g, %d scale gradients held to their bounds'
          % (what, noise, 'bit-reproducible' if reproducible else 'not reproducible', worst, len(bounded)))
    assert bounded
    for k in bounded:
        room = float(a[k.replace('gp.', 'bound.', 1)])
        assert abs(float(got[k]) - float(a[k])) <= 2 * room, (what, k, got[k], a[k], room)
    for k in plain:
        if tc.is_decision(k):
            assert tc_same(got[k], a[k]), (what, k, got[k], a[k])
        elif reproducible:
            assert tc_same(got[k], a[k]), (what, k, qc.rel_l2(got[k], a[k]))
        else:
            assert qc.rel_l2(got[k], a[k]) <= 4 * noise, (what, k, qc.rel_l2(got[k], a[k]), noise)


def tc_same(a, b):
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize('case', tc.CONV_CASES, ids=[c[0] for c in tc.CONV_CASES])
def test_conv_module_fused_equals_torch_on_the_device(lib, Q, torch_path, deterministic_convs, case):
    name, kwargs, _ = case
    z = np.load(os.path.join(conftest.REPO, 'tests', 'golden', 'tpsq_conv_%s.npz' % name))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init.')}
    calls = [[torch.from_numpy(z['in.%d.0' % k])] for k in range(11)]

    def run():
        mod = tc.make_conv(Q, kwargs, seed=7)
        mod.load_state_dict(init, strict=True)
        rec = tc.run_conv(mod, calls, device='cuda', bounds=True)
        return {'%d.%s' % (k, f): v.cpu() for k, r in enumerate(rec) for f, v in r.items()}
    _compare_runs(run, torch_path, name)


def test_micro_net_fused_equals_torch_on_the_device(lib, Q, torch_path, deterministic_convs):
    import models
    z = np.load(os.path.join(conftest.REPO, 'tests', 'golden', 'tpsq_net.npz'))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init.')}
    frames = torch.from_numpy(z['frames']).float().div(256)

    def run():
        m = models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=2, a_bit=8, w_bit=8, steps=STEPS)
        m.load_state_dict(init, strict=True)
        m.cuda().train()
        blocks = {'module_list.%d.%s' % (k, next(iter(b._modules))): b[0] for k, b in enumerate(m.module_list)
                  if isinstance(b, torch.nn.Sequential) and len(b) and hasattr(b[0], 'weight_quantizer')}
        probes = {name: tc.ScaleGradBounds(conv) for name, conv in blocks.items()}
        assert len(probes) == 18
        out = {}
        for it in range(3):
            m.zero_grad()
            heads = m(frames[it].cuda())[0]
            sum(p.pow(2).mean() for p in heads).backward()
            out.update({'it%d.head%d' % (it, j): p.detach().cpu() for j, p in enumerate(heads)})
            out.update({'gp.it%d.%s' % (it, k): p.grad.cpu().clone() for k, p in m.named_parameters() if p.grad is not None})
            for name, probe in probes.items():
                out.update({'bound.it%d.%s.%s' % (it, name, f[len('bound.'):]): v.cpu() for f, v in probe.bounds().items()})
        m.eval()
        with torch.no_grad():
            out['eval.inf'] = m(frames[3].cuda())[0].cpu()
        out.update({'sd.' + k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        return out
    _compare_runs(run, torch_path, 'micro net')


# ------------------------------------------------------------------------------------------------ 5. no per-step host reads
def test_training_step_of_a_conv_module_reads_nothing_back(lib, Q, torch_path):
    torch.manual_seed(0)
    mod = Q.TPSQ_BNFold_QuantizedConv2d_For_FPGA(8, 16, 3, padding=1, bn=1, activate='leaky', steps=100).cuda().train()
    x = torch.randn(2, 8, 16, 16, device='cuda', requires_grad=True)
    g = torch.randn(2, 16, 16, 16, device='cuda')
    probe = torch.ones(1, device='cuda')
    (mod(x) * g).sum().backward()          # the warm-up call: the mirrors' one read per module, kernel loading
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
    assert mod.step.item() == 2 and mod.activation_quantizer.warmup.item() == 0 and mod.bias_quantizer.range_tracker.first_w.item() == 1
    a, w = mod.activation_quantizer.scale, mod.weight_quantizer.scale
    assert a.item() > 0 and tc.nearest_pow2(a.item()) == a.item() and torch.isfinite(a.grad).all() and torch.isfinite(w.grad).all()
    assert torch.isfinite(mod.weight.grad).all()
