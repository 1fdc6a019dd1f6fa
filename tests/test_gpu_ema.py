"""GPU tier of the device model EMA: ``yh_ema_update`` (csrc/ema.hip) through the C ABI against ``v.mul_(d).add_(src, alpha=1 - d)``
evaluated by torch on the same device, bit for bit - the test that decides which arithmetic the kernel documents (the fused form:
``fma(one_minus_d, src, fl32(ema * d))``) - then ``ModelEMA`` on micro models against its own torch loop, the version counters that
keep the inference engine's packed weights fresh, and ``train.train --ema``."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fakelib_ema
import synth
import train_harness as th
from engine import ema as hip_ema
from engine import hiplib
from engine.hiplib import EMA_CHUNK, EmaRow
from utils.torch_utils import ModelEMA

pytestmark = pytest.mark.gpu

GUARD = 12345.0
LENGTHS = (1, 3, 4, 5, 255, 256, 257, EMA_CHUNK - 1, EMA_CHUNK, EMA_CHUNK + 1, 2 * EMA_CHUNK + 3)
GRID_CAP = 2048
DECAY = lambda n: 0.9999 * (1 - np.exp(-n / 2000))
SPECIALS = [float('nan'), float('inf'), float('-inf'), 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1.1754942e-38, 3.0e38, -3.0e38, 1.0]


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load()


def _layout(lengths, offsets):
    """Element offsets of rows in one flat buffer: every slot starts 16-byte aligned with four guard floats, the row follows
    ``offsets[i]`` bytes (0, 4, 8 or 12) after them, and at least one guard float follows the row."""
    starts, off = [], 0
    for n, b in zip(lengths, offsets):
        assert b in (0, 4, 8, 12)
        starts.append(off + 4 + b // 4)
        off += (4 + b // 4 + n + 1 + 3) // 4 * 4
    return starts, off


def _fill(total, starts, lengths, seed, specials):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((total,), GUARD)
    for o, n in zip(starts, lengths):
        buf[o:o + n] = torch.randn(n, generator=g)
        if specials and n >= 255:
            k = len(SPECIALS)
            # every special value of this side against every special value of the other side (ema: the slow index, src: the fast one)
            idx = torch.arange(k * k)
            vals = torch.tensor(SPECIALS)
            buf[o:o + k * k] = vals[idx // k] if specials == 'ema' else vals[idx % k]
    return buf


def _table(ema, src, e_starts, s_starts, lengths):
    rows, chunk0 = [], 0
    for eo, so, n in zip(e_starts, s_starts, lengths):
        rows.append(EmaRow(ema=ema.data_ptr() + 4 * eo, src=src.data_ptr() + 4 * so, n=n, chunk0=chunk0))
        chunk0 += -(-n // EMA_CHUNK)
    raw = bytes((EmaRow * len(rows))(*rows))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda(), chunk0


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _case(lib, lengths, e_off, s_off, d, seed=0, specials=False, need_differing=False):
    """One table, one launch; the result against torch's statement on the device, the guards, and the source untouched."""
    e_starts, e_total = _layout(lengths, e_off)
    s_starts, s_total = _layout(lengths, s_off)
    ema_h = _fill(e_total, e_starts, lengths, seed, 'ema' if specials else None)
    src_h = _fill(s_total, s_starts, lengths, seed + 1000, 'src' if specials else None)
    ema, src = ema_h.cuda(), src_h.cuda()
    table, n_chunks = _table(ema, src, e_starts, s_starts, lengths)
    hiplib.check(lib.yh_ema_update(table.data_ptr(), len(lengths), n_chunks, d, 1. - d, hiplib.stream_ptr()), 'yh_ema_update')
    torch.cuda.synchronize()
    d32, a32 = np.float32(d), np.float32(1. - d)
    inside = torch.zeros(e_total, dtype=torch.bool)
    differing = 0
    for eo, so, n in zip(e_starts, s_starts, lengths):
        want = ema_h[eo:eo + n].cuda()
        want.mul_(d).add_(src[so:so + n], alpha=1. - d)                    # the statement of ModelEMA.update, on the device
        got = ema[eo:eo + n]
        bad = np.nonzero(_bits(got) != _bits(want))[0]
        assert bad.size == 0, (n, eo, so, d, bad[:8], got.cpu()[bad[:8]], want.cpu()[bad[:8]], ema_h[eo:eo + n][bad[:8]], src_h[so:so + n][bad[:8]])
        inside[eo:eo + n] = True
        e_np, s_np = ema_h[eo:eo + min(n, 1 << 16)].numpy(), src_h[so:so + min(n, 1 << 16)].numpy()      # a sample of a long row
        fused, _ = fakelib_ema.fused(e_np, s_np, d32, a32)
        other = fakelib_ema.two_roundings(e_np, s_np, d32, a32)
        differing += int(((fused.view(np.int32) != other.view(np.int32)) & np.isfinite(fused) & np.isfinite(other)).sum())
    if need_differing:
        assert differing > 0, 'no element of the draw tells the fused form from the two-rounding form'
    assert bool((ema.cpu()[~inside] == GUARD).all()), 'a guard float of the ema side was written'
    assert np.array_equal(_bits(src), _bits(src_h)), 'the source side was written'
    return differing


@pytest.mark.parametrize('updates', [1, 100000])
def test_kernel_is_bit_equal_to_the_torch_statement_on_the_device(lib, updates):
    """Row lengths around the float4 group, the workgroup and the chunk; NaN, infinities, signed zeros and denormals on both sides
    (all pairs); and elements on which the fused and the two-rounding forms give different bits, so passing decides the form."""
    d = float(DECAY(updates))
    zeros = (0,) * len(LENGTHS)
    differing = _case(lib, LENGTHS, zeros, zeros, d, seed=1, need_differing=True)
    print('d = %.9g: %d of %d elements tell the two forms apart' % (d, differing, sum(LENGTHS)))
    _case(lib, LENGTHS, zeros, zeros, d, seed=2, specials=True)


def test_kernel_on_300_one_element_rows(lib):
    """The row search: 300 rows, 300 chunks, the binary search at every depth."""
    lengths = (1,) * 300
    zeros = (0,) * 300
    _case(lib, lengths, zeros, zeros, float(DECAY(50)), seed=3)
    mixed = tuple((0, 4, 8, 12)[i % 4] for i in range(300))
    _case(lib, lengths, mixed, mixed[::-1], float(DECAY(50)), seed=4)


def test_kernel_strides_over_the_chunks_of_a_long_row(lib):
    """One row of more than 2 * 2048 chunks behind and in front of short ones: every workgroup serves at least two chunks."""
    lengths = (5, 2 * GRID_CAP * EMA_CHUNK + 5, 257)
    assert sum(-(-n // EMA_CHUNK) for n in lengths) > 2 * GRID_CAP
    _case(lib, lengths, (0, 0, 0), (0, 0, 0), float(DECAY(2000)), seed=5, need_differing=True)


def test_kernel_on_rows_that_are_not_16_byte_aligned(lib):
    """ema and src each 0, 4, 8 and 12 bytes off a 16-byte boundary, independently: the element loop, nothing outside the row."""
    per = (5, 257, EMA_CHUNK + 1)
    lengths, e_off, s_off = [], [], []
    for eb in (0, 4, 8, 12):
        for sb in (0, 4, 8, 12):
            lengths += per
            e_off += [eb] * len(per)
            s_off += [sb] * len(per)
    _case(lib, tuple(lengths), tuple(e_off), tuple(s_off), float(DECAY(1)), seed=6, need_differing=True)


def test_empty_table_and_bad_arguments(lib):
    ema = torch.full((16,), GUARD).cuda()
    src = torch.ones(16).cuda()
    table, n_chunks = _table(ema, src, (4,), (4,), (3,))
    s = hiplib.stream_ptr()
    assert lib.yh_ema_update(table.data_ptr(), 0, 0, 0.5, 0.5, s) == 0
    assert lib.yh_ema_update(None, 0, 0, 0.5, 0.5, s) == 0
    assert lib.yh_ema_update(None, 1, 1, 0.5, 0.5, s) == -1
    assert lib.yh_ema_update(table.data_ptr(), -1, 1, 0.5, 0.5, s) == -1
    assert lib.yh_ema_update(table.data_ptr(), 1, -1, 0.5, 0.5, s) == -1
    assert lib.yh_ema_update(table.data_ptr(), 1, 0, 0.5, 0.5, s) == -1
    assert lib.yh_ema_update(table.data_ptr() + 4, 1, 1, 0.5, 0.5, s) == -2
    torch.cuda.synchronize()
    assert bool((ema.cpu() == GUARD).all())


# ------------------------------------------------------------------------------------------ ModelEMA
def _perturb(model, step):
    """A deterministic 'optimizer step' on a device model: the same host draw for every run, moved to the device."""
    g = torch.Generator().manual_seed(100 + step)
    with torch.no_grad():
        for v in model.state_dict().values():
            if v.dtype.is_floating_point:
                noise = torch.randn(v.shape, generator=g).to(v.device)
                v.add_((noise * 0.01 * (v.float().abs() + 0.1)).to(v.dtype).view(v.shape))
            else:
                v.add_(1)


def _float_model():
    path = th.write_cfg(th.mini_cfg_text())
    try:
        return th.build(path, 64)
    finally:
        os.unlink(path)


def _qat_model():
    import models
    from qat_minicfg import SIZE, STEPS, micro_cfg
    torch.manual_seed(0)
    return models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=1, a_bit=8, w_bit=8, steps=STEPS, shortcut_way=1)


@pytest.mark.parametrize('kind', ['float', 'quantized'])
def test_model_ema_equals_its_torch_loop_bit_for_bit(lib, monkeypatch, kind):
    """Five updates of the device path and of ``YOLO_HIP_EMA=0`` from equal copies: equal state dicts, one launch an update, one table."""
    live = (_float_model() if kind == 'float' else _qat_model()).to('cuda')
    ends = {}
    for env in ('1', '0'):
        monkeypatch.setenv('YOLO_HIP_EMA', env)
        model = copy.deepcopy(live)
        ema = ModelEMA(model)
        hip_ema.reset_stats()
        for step in range(5):
            _perturb(model, step)
            ema.update(model)
        torch.cuda.synchronize()
        st = hip_ema.stats()
        if env == '1':
            n_float = sum(1 for v in model.state_dict().values() if v.dtype.is_floating_point)
            assert st['launches'] == 5 and st['table_builds'] == 1, st
            assert st['torch_tensors'] == 0, st
            assert ema._hip._n_rows == n_float
            if kind == 'quantized':
                assert sum(1 for v in model.state_dict().values() if v.dtype.is_floating_point and v.numel() == 1) > 10
        else:
            assert st == dict(launches=0, table_builds=0, torch_tensors=0) and ema._hip is None
        ends[env] = {k: v.detach().cpu() for k, v in ema.ema.state_dict().items()}
    start = live.state_dict()
    assert list(ends['1']) == list(ends['0'])
    moved = 0
    for k, a in ends['1'].items():
        b = ends['0'][k]
        assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), k
        moved += int(a.dtype.is_floating_point and not torch.equal(a, start[k].cpu()))
    assert moved > len(ends['1']) // 2


def test_engine_repacks_the_ema_weights_after_an_update(lib):
    """The kernel writes through raw pointers and the inference engine keys its packed weights on ``(data_ptr, _version, shape)``:
    without the version bump after the launch the second evaluation would run on the first one's packed weights."""
    model = _float_model().to('cuda')
    ema = ModelEMA(model)
    x = synth.image_batch(2, 64, seed=0).to('cuda')
    with torch.no_grad():
        first = ema.ema(x)[0].clone()
    assert ema.ema.__dict__.get('_hip_engine') is not None, 'the evaluation did not run on the inference engine'
    _perturb(model, 0)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.5)
    hip_ema.reset_stats()
    ema.update(model)                     # update 1: d = 5e-4, the EMA all but becomes the live model
    assert hip_ema.stats()['launches'] == 1
    with torch.no_grad():
        second = ema.ema(x)[0].clone()
    fresh = _float_model()
    fresh.load_state_dict({k: v.cpu() for k, v in ema.ema.state_dict().items()})
    fresh = fresh.to('cuda').eval()
    with torch.no_grad():
        want = fresh(x)[0]
    torch.cuda.synchronize()
    assert not torch.equal(first, second)
    assert np.array_equal(_bits(second), _bits(want))


def test_train_with_ema_takes_the_device_path(lib, dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    """``train.train --ema`` for one epoch on the synthetic set at 64 px: finishes, updated the EMA on the device, and checkpoints
    finite EMA weights that are not the initial ones."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('YOLO_HIP_EMA', raising=False)
    import models
    import train as train_mod
    from utils import torch_utils
    torch_utils.init_seeds()
    initial = models.Darknet(tiny_cfg).state_dict()
    opt = train_mod.make_parser().parse_args(['--epochs', '1', '--batch-size', '4', '--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'),
                                              '--img-size', '64', '64', '64', '-mpt', '--nosave', '--ema'])
    opt.local_rank = -1
    hip_ema.reset_stats()
    results = train_mod.train(opt, train_mod.hyp)
    st = hip_ema.stats()
    assert len(results) == 7 and all(np.isfinite(results))
    assert st['launches'] >= 1 and st['table_builds'] >= 1 and st['torch_tensors'] == 0, st
    ckpt = torch.load('weights/last.pt', map_location='cpu', weights_only=False)
    state = ckpt['model']
    assert set(state) == set(initial)
    floats = [k for k, v in state.items() if v.dtype.is_floating_point]
    assert all(bool(torch.isfinite(state[k]).all()) for k in floats)
    assert sum(1 for k in floats if not torch.equal(state[k].float(), initial[k].float())) > len(floats) // 2
