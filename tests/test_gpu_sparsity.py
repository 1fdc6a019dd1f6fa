"""GPU tier of the network-slimming sparsity term: ``yh_bn_l1_subgrad`` (csrc/sparsity.hip) against the recorded ``updateBN`` results
and against torch on the device, bit for bit; then whole training steps with ``Darknet.hip_set_bn_sparsity`` against the same
engine's plain step plus the torch formula.  The step is bit-reproducible run to run, so the comparisons are
``torch.equal``."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import conftest
import synth
import train_harness as th
from engine import hiplib, slimming
from engine.hiplib import BnL1Row

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(conftest.REPO, 'tests', 'golden')
ROWS = (1, 3, 13, 64, 65, 255, 1024)
GUARD = 12345.0


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load()


def _layout(lengths):
    """Rows in one flat buffer: every start 16-byte aligned, one guard float right after each row's last element."""
    offs, off = [], 0
    for n in lengths:
        offs.append(off)
        off += (n + 1 + 3) // 4 * 4
    return offs, off


def _table(gamma, grad, offs, lengths):
    items = [BnL1Row(gamma=gamma.data_ptr() + 4 * o, grad=grad.data_ptr() + 4 * o, n=n) for o, n in zip(offs, lengths)]
    raw = bytes((BnL1Row * len(items))(*items))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _run(lib, table, first, last, s):
    hiplib.check(lib.yh_bn_l1_subgrad(table.data_ptr(), first, last, s, hiplib.stream_ptr()), 'yh_bn_l1_subgrad')
    torch.cuda.synchronize()


def test_kernel_is_bit_equal_to_updatebn_and_to_torch(lib):
    z = np.load(os.path.join(GOLDEN, 'bn_l1.npz'))
    offs, total = _layout(ROWS)
    gamma_h, grad_h = torch.full((total,), GUARD), torch.full((total,), GUARD)
    for k, (o, n) in enumerate(zip(offs, ROWS)):
        assert len(z['gamma_%d' % k]) == n
        gamma_h[o:o + n] = torch.from_numpy(z['gamma_%d' % k])
        grad_h[o:o + n] = torch.from_numpy(z['grad_%d' % k])
    gamma = gamma_h.cuda()
    for j, s in enumerate(z['s']):
        s = float(s)
        grad = grad_h.cuda()
        table = _table(gamma, grad, offs, ROWS)
        # an empty range: no launch, nothing changes
        _run(lib, table, 0, 0, s)
        _run(lib, table, 3, 3, s)
        assert np.array_equal(_bits(grad), _bits(grad_h))
        # rows [2, 5) only
        _run(lib, table, 2, 5, s)
        for k, (o, n) in enumerate(zip(offs, ROWS)):
            want = z['out%d_%d' % (j, k)] if 2 <= k < 5 else z['grad_%d' % k]
            assert np.array_equal(_bits(grad[o:o + n]), want.view(np.int32)), (j, k)
        # the whole table on a fresh gradient
        grad = grad_h.cuda()
        table = _table(gamma, grad, offs, ROWS)
        _run(lib, table, 0, len(ROWS), s)
        for k, (o, n) in enumerate(zip(offs, ROWS)):
            got = grad[o:o + n]
            assert np.array_equal(_bits(got), z['out%d_%d' % (j, k)].view(np.int32)), (j, k)
            dev = grad_h[o:o + n].cuda()
            dev.add_(s * torch.sign(gamma[o:o + n]))
            assert np.array_equal(_bits(got), _bits(dev)), (j, k)
            assert float(grad[o + n]) == GUARD and float(gamma[o + n]) == GUARD, (j, k)
        keep = torch.ones(total, dtype=torch.bool)
        for o, n in zip(offs, ROWS):
            keep[o:o + n] = False
        assert bool((grad.cpu()[keep] == GUARD).all())
    assert lib.yh_bn_l1_subgrad(table.data_ptr(), 2, 1, 0.1, hiplib.stream_ptr()) == -1
    assert lib.yh_bn_l1_subgrad(table.data_ptr(), -1, 1, 0.1, hiplib.stream_ptr()) == -1


def test_kernel_on_many_short_rows(lib):
    """130 rows of 7 floats (more rows than a small grid, no row reaches a float4 boundary cleanly)."""
    lengths = (7,) * 130
    offs, total = _layout(lengths)
    g = torch.Generator().manual_seed(3)
    gamma_h, grad_h = torch.randn(total, generator=g), torch.randn(total, generator=g)
    gamma_h[::11] = 0.0
    gamma_h[5::13] = -0.0
    gamma_h[3::17] = float('nan')
    for o, n in zip(offs, lengths):
        gamma_h[o + n], grad_h[o + n] = GUARD, GUARD
    gamma, grad = gamma_h.cuda(), grad_h.cuda()
    table = _table(gamma, grad, offs, lengths)
    _run(lib, table, 0, 130, 0.37)
    want = grad_h.cuda()
    for o, n in zip(offs, lengths):
        want[o:o + n].add_(0.37 * torch.sign(gamma[o:o + n]))
    assert np.array_equal(_bits(grad), _bits(want))
    for o, n in zip(offs, lengths):
        assert float(grad[o + n]) == GUARD


# ------------------------------------------------------------------------------------------ whole steps
def _step(model, x, ws, precision, blocks=None, s=0.0):
    m = copy.deepcopy(model)
    m.hip_set_bn_sparsity(blocks, s)
    _, grads, m = th.engine_step(m, x, ws, precision, device='cuda')
    return grads, m


def _assert_plain_plus_term(model, x, ws, precision, blocks, s):
    plain, _ = _step(model, x, ws, precision)
    again, _ = _step(model, x, ws, precision)
    for k in plain:                                   # the premise of the bit comparison: the plain step repeats itself
        assert torch.equal(plain[k], again[k]), k
    got, m = _step(model, x, ws, precision, blocks, s)
    listed = {'module_list.%d.%s' % (i, n) for i in blocks for n in ('BatchNorm2d.weight',)}
    params = dict(model.named_parameters())
    assert listed <= set(params)
    for k in plain:
        want = plain[k].cuda()
        if k in listed:
            want.add_(s * torch.sign(params[k].detach().cuda()))
        assert torch.equal(got[k], want.cpu()), k
    return m


@pytest.fixture(scope='module')
def mini_case():
    path = th.write_cfg(th.mini_cfg_text())
    try:
        model = th.build(path, 64)
    finally:
        os.unlink(path)
    with torch.no_grad():
        w = model.module_list[1][1].weight
        w[0], w[1], w[2] = 0.0, -0.0, -abs(float(w[2])) - 0.1
    x = synth.image_batch(2, 64, seed=0)
    _, _, _, ws = th.eager_step(model, x)
    return model, x, ws


@pytest.mark.parametrize('segments', ['1', '8'])
@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_mini_step_equals_plain_step_plus_torch_formula(lib, mini_case, monkeypatch, precision, segments):
    monkeypatch.setenv('YOLO_HIP_TRAIN_SEGMENTS', segments)
    model, x, ws = mini_case
    blocks = slimming.sparsity_blocks(model.module_defs, 1)
    m = _assert_plain_plus_term(model, x, ws, precision, blocks, 1e-2)
    plan = m.__dict__['_hip_train_engine']._current
    ranges = plan['l1_ranges']
    assert len(ranges) == len(plan['segments']) and ranges[-1][1] == len(blocks)
    if segments == '1':
        assert ranges == [(0, len(blocks))]
    else:
        assert len(ranges) > 1 and sum(1 for a, b in ranges if b > a) > 1      # sub-range launches


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_pruned_mobilenet_step_equals_plain_step_plus_torch_formula(lib, precision):
    """The reference's slim-pruned YOLOv3-Mobilenetv3 (37 odd widths): padded twin, depthwise blocks with BatchNorm among the rows."""
    import models
    from engine.padded import PaddedTrainEngine
    torch.manual_seed(0)
    model = models.Darknet(os.path.join(GOLDEN, 'slim_prune_0.5_yolov3-mobilenet-coco.cfg'), (96, 96))
    state = model.state_dict()
    synth.randomize_bn_(state, seed=1)
    model.load_state_dict(state)
    model.train()
    x = synth.image_batch(2, 96, seed=0)
    _, _, _, ws = th.eager_step(model, x)
    depthwise = [i for i, d in enumerate(model.module_defs) if d['type'] == 'depthwise' and int(d['batch_normalize'])]
    blocks = sorted(set(slimming.sparsity_blocks(model.module_defs, 1)) | set(depthwise[:6]))
    assert depthwise and len(blocks) > 35
    listed = dict(model.named_parameters())
    names = []
    for i in blocks:
        hit = [k for k in listed if k.startswith('module_list.%d.' % i) and k.endswith('BatchNorm2d.weight')]
        assert len(hit) == 1
        names.append(hit[0])
    plain, _ = _step(model, x, ws, precision)
    got, m = _step(model, x, ws, precision, blocks, 1e-2)
    assert isinstance(m.__dict__['_hip_train_engine'], PaddedTrainEngine)
    for k in plain:
        want = plain[k].cuda()
        if k in names:
            want.add_(1e-2 * torch.sign(listed[k].detach().cuda()))
        assert torch.equal(got[k], want.cpu()), k


def test_three_sgd_steps_shrink_the_penalised_gammas(lib, mini_case):
    """Three SGD steps (the optimizer of test_gpu_train.py::test_mini_sgd_steps_track_eager) with s = 1e-2 against the same run with
    s = 0: the sum of |gamma| over the prunable set ends lower; parameters outside the set stay within that test's tolerance
    (3e-4 relative to the tensor's largest magnitude: one leaky-ReLU kink flipping on a last-bit difference)."""
    model, _, _ = mini_case
    blocks = slimming.sparsity_blocks(model.module_defs, 1)
    listed = {'module_list.%d.BatchNorm2d.weight' % i for i in blocks}
    ends = []
    for s in (0.0, 1e-2):
        m = copy.deepcopy(model).to('cuda').train()
        m.hip_set_bn_sparsity(blocks, s)
        opt = torch.optim.SGD(m.parameters(), lr=2e-6, momentum=0.9)
        ws = None
        for step in range(3):
            x = synth.image_batch(4, 64, seed=step)
            raws = m(x.to('cuda'))[0]
            ws = ws or th.loss_weights(raws)
            opt.zero_grad()
            th.toy_loss(raws, ws).backward()
            opt.step()
        ends.append({k: v.detach().cpu() for k, v in m.state_dict().items() if v.dtype.is_floating_point})
    l1 = [sum(float(e[k].double().abs().sum()) for k in listed) for e in ends]
    print('sum |gamma| over the prunable set: s = 0: %.9f, s = 1e-2: %.9f' % tuple(l1))
    assert l1[1] < l1[0]
    for k, a in ends[0].items():
        if k not in listed:
            d = (a - ends[1][k]).abs().max().item()
            assert d <= 3e-4 * (a.abs().max().item() + 1e-3), (k, d)
