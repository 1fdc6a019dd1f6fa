"""CPU tier of the device model EMA (engine/ema.py behind ``ModelEMA.update``): the host emulation of ``yh_ema_update``
(tests/fakelib_ema.py) injected through ``engine.ema._LIB_OVERRIDE`` drives the same table building, launch and version-counter code
on host tensors that the GPU runs on device tensors.

Which arithmetic: the fused form, ``ema = fma(one_minus_d, src, fl32(ema * d))``.  That is what torch's CPU kernels compute for
``v.mul_(d).add_(src, alpha=1 - d)`` (one fused multiply-add with ``alpha`` in fp32) and what tests/test_gpu_ema.py finds on the
device, so the results here are compared BIT FOR BIT against ``ModelEMA``'s torch statement on copies of the same tensors.  The
emulation evaluates the fma through fp64 and counts the inputs on which that is not exact (fakelib_ema: fp32 midpoints); with the
fixed seeds used here that count is 0, which the tests assert."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import conftest
import fakelib_ema
import train_harness as th
from engine import ema as hip_ema
from engine import hiplib
from engine.hiplib import EMA_CHUNK, EmaRow
from utils.torch_utils import ModelEMA

HEADER = os.path.join(conftest.REPO, 'include', 'yolo_hip.h')


@pytest.fixture
def fake():
    lib = fakelib_ema.FakeLibEma()
    hip_ema._LIB_OVERRIDE = lib
    hip_ema.reset_stats()
    try:
        yield lib
    finally:
        hip_ema._LIB_OVERRIDE = None


@pytest.fixture(scope='module')
def mini():
    path = th.write_cfg(th.mini_cfg_text())
    try:
        return th.build(path, 64)
    finally:
        os.unlink(path)


def _floats(model):
    return {k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point}


def _perturb(model, step):
    """A deterministic 'optimizer step': every floating-point state tensor moves by about a percent, every integer one counts up."""
    g = torch.Generator().manual_seed(100 + step)
    with torch.no_grad():
        for v in model.state_dict().values():
            if v.dtype.is_floating_point:
                v.add_((torch.randn(v.shape, generator=g) * 0.01 * (v.float().abs() + 0.1)).to(v.dtype).view(v.shape))
            else:
                v.add_(1)


def _reference_update(ref, model):
    """``ModelEMA.update`` in its torch form: no emulation installed, host tensors."""
    keep, hip_ema._LIB_OVERRIDE = hip_ema._LIB_OVERRIDE, None
    try:
        ref.update(model)
    finally:
        hip_ema._LIB_OVERRIDE = keep


def _assert_same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].contiguous().numpy().tobytes() == b[k].contiguous().numpy().tobytes(), k


def _check_prefix(call):
    chunk0 = 0
    for _, _, n, c0 in call['rows']:
        assert n >= 1 and c0 == chunk0
        chunk0 += -(-n // EMA_CHUNK)
    assert call['n_chunks'] == chunk0


def test_formula_of_the_emulation_is_the_torch_statement():
    """The documented fused form against ``v.mul_(d).add_(src, alpha=1 - d)`` on 2^20 random elements at four decays, bit for bit; the
    two-rounding form differs on some of them at every decay (fewer as 1 - d shrinks), so the comparison does tell the forms apart."""
    g = torch.Generator().manual_seed(7)
    e = torch.randn(1 << 20, generator=g)
    s = torch.randn(1 << 20, generator=g)
    decay = lambda n: 0.9999 * (1 - np.exp(-n / 2000))
    for d in (decay(1), decay(50), decay(2000), 0.9999):
        d = float(d)
        want = e.clone().mul_(d).add_(s, alpha=1. - d).numpy()
        d32, a32 = np.float32(d), np.float32(1. - d)
        got, mid = fakelib_ema.fused(e.numpy(), s.numpy(), d32, a32)
        assert int(mid.sum()) == 0
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), d
        other = fakelib_ema.two_roundings(e.numpy(), s.numpy(), d32, a32)
        assert (other.view(np.int32) != want.view(np.int32)).any(), d


def test_one_call_per_update_on_yolov3(fake, cfg_dir):
    import models
    torch.manual_seed(0)
    model = models.Darknet(os.path.join(cfg_dir, 'yolov3', 'yolov3.cfg'), (64, 64))
    ema = ModelEMA(model)
    ref = copy.deepcopy(ema)
    _perturb(model, 0)
    ema.update(model)
    n_float = len(_floats(model))
    assert n_float == 366 and len(model.state_dict()) > n_float      # the count of the issue's table; integer buffers exist too
    assert len(fake.ema_calls) == 1
    call = fake.ema_calls[0]
    assert call['n_rows'] == n_float == len(call['rows'])
    _check_prefix(call)
    assert call['n_chunks'] == sum(-(-v.numel() // EMA_CHUNK) for v in _floats(model).values())
    for (k, v), (k2, s), (p_ema, p_src, n, _) in zip(_floats(ema.ema).items(), _floats(model).items(), call['rows']):
        assert k == k2 and (p_ema, p_src, n) == (v.data_ptr(), s.data_ptr(), v.numel()), k
    assert hip_ema.stats() == dict(launches=1, table_builds=1, torch_tensors=0)
    _reference_update(ref, model)
    assert fake.midpoints == 0
    _assert_same_bits(ema.ema.state_dict(), ref.ema.state_dict())


@pytest.mark.parametrize('n', [1, 50, 2000])
def test_decay_scalars_are_the_ramp_rounded_once(fake, mini, n):
    model = copy.deepcopy(mini)
    ema = ModelEMA(model)
    ema.updates = n - 1
    ema.update(model)
    assert ema.updates == n
    d = 0.9999 * (1 - np.exp(-n / 2000))
    assert d == ema.decay(n)
    call = fake.ema_calls[0]
    assert isinstance(call['d'], float) and isinstance(call['a'], float)
    assert call['d'] == float(np.float32(d)) and call['a'] == float(np.float32(1. - d))


def test_table_is_uploaded_once_and_rebuilt_when_a_tensor_moves(fake, mini):
    model = copy.deepcopy(mini)
    ema = ModelEMA(model)
    for step in range(5):
        _perturb(model, step)
        ema.update(model)
    assert hip_ema.stats() == dict(launches=5, table_builds=1, torch_tensors=0)
    assert len({c['table'] for c in fake.ema_calls}) == 1
    state = model.state_dict()
    model.load_state_dict({k: v.clone() for k, v in state.items()})      # copies in place: nothing moves
    ema.update(model)
    assert hip_ema.stats()['table_builds'] == 1
    # a parameter of the live model is rebound (the prune scripts' `param.data = ...`)
    w = model.module_list[0][0].weight
    w.data = w.data.clone()
    ema.update(model)
    assert hip_ema.stats()['table_builds'] == 2
    assert fake.ema_calls[-1]['rows'][0][1] == w.data_ptr() != fake.ema_calls[-2]['rows'][0][1]
    # a destination moves
    v = ema.ema.module_list[0][0].weight
    v.data = v.data.clone()
    ema.update(model)
    assert hip_ema.stats()['table_builds'] == 3 and hip_ema.stats()['launches'] == 8
    assert fake.ema_calls[-1]['rows'][0][0] == v.data_ptr() != fake.ema_calls[-2]['rows'][0][0]
    for call in fake.ema_calls:
        _check_prefix(call)


def test_results_equal_the_torch_statement_bit_for_bit(fake, mini):
    model = copy.deepcopy(mini)
    ema = ModelEMA(model)
    ref = copy.deepcopy(ema)
    for step in range(5):
        _perturb(model, step)
        ema.update(model)
        _reference_update(ref, model)
    assert len(fake.ema_calls) == 5 and fake.midpoints == 0
    assert ema.updates == ref.updates == 5
    _assert_same_bits(ema.ema.state_dict(), ref.ema.state_dict())
    start = mini.state_dict()
    assert any(not torch.equal(v, start[k]) for k, v in _floats(ema.ema).items())


def test_half_and_non_contiguous_tensors_keep_the_torch_form(fake, mini):
    model = copy.deepcopy(mini)
    bn = model.module_list[1][1]
    bn.running_mean = bn.running_mean.half()
    ema = ModelEMA(model)
    assert ema.ema.module_list[1][1].running_mean.dtype == torch.float16
    w = model.module_list[3][0].weight
    w.data = w.data.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    assert not w.is_contiguous()
    ref = copy.deepcopy(ema)
    n_float = len(_floats(model))
    for step in range(2):
        _perturb(model, step)
        ema.update(model)
        _reference_update(ref, model)
    assert [c['n_rows'] for c in fake.ema_calls] == [n_float - 2] * 2
    assert hip_ema.stats() == dict(launches=2, table_builds=1, torch_tensors=4)
    assert fake.midpoints == 0
    _assert_same_bits(ema.ema.state_dict(), ref.ema.state_dict())


def test_ema_on_the_host_of_a_device_model_takes_the_torch_form(fake, mini, monkeypatch):
    """``ModelEMA(model, device='cpu')``: under the emulation every host tensor counts as device memory, so the test says which
    tensors are 'on the device' - the live model's, not the EMA's."""
    model = copy.deepcopy(mini)
    ema = ModelEMA(model, device='cpu')
    ref = copy.deepcopy(ema)
    live = {v.data_ptr() for v in model.state_dict().values()}
    monkeypatch.setattr(hip_ema, '_on_device', lambda t: t.data_ptr() in live)
    _perturb(model, 0)
    ema.update(model)
    assert fake.ema_calls == [] and hip_ema.stats()['launches'] == 0
    monkeypatch.undo()
    _reference_update(ref, model)
    _assert_same_bits(ema.ema.state_dict(), ref.ema.state_dict())


def test_integer_buffers_are_untouched(fake, mini):
    model = copy.deepcopy(mini)
    ema = ModelEMA(model)
    ints = [k for k, v in model.state_dict().items() if not v.dtype.is_floating_point]
    assert ints
    before = {k: ema.ema.state_dict()[k].clone() for k in ints}
    _perturb(model, 0)
    ema.update(model)
    for k in ints:
        assert torch.equal(ema.ema.state_dict()[k], before[k]) and not torch.equal(model.state_dict()[k], before[k]), k
    assert all(n for _, _, n, _ in fake.ema_calls[0]['rows']) and fake.ema_calls[0]['n_rows'] == len(_floats(model))


def test_env_switch_keeps_the_torch_loop(fake, mini, monkeypatch):
    monkeypatch.setenv('YOLO_HIP_EMA', '0')
    model = copy.deepcopy(mini)
    ema = ModelEMA(model)
    start = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    _perturb(model, 0)
    ema.update(model)
    assert fake.ema_calls == [] and hip_ema.stats() == dict(launches=0, table_builds=0, torch_tensors=0)
    assert ema.updates == 1 and any(not torch.equal(v, start[k]) for k, v in _floats(ema.ema).items())


def test_every_destination_version_counter_moves_with_each_update(fake, mini):
    """The kernel writes through raw pointers; the inference engine keys its packed weights on ``_version`` (engine/plan.py)."""
    model = copy.deepcopy(mini)
    ema = ModelEMA(model)
    tensors = dict(ema.ema.named_parameters())
    tensors.update({k: b for k, b in ema.ema.named_buffers() if b.dtype.is_floating_point})
    assert set(tensors) == set(_floats(ema.ema))
    last = {k: t._version for k, t in tensors.items()}
    for step in range(3):
        _perturb(model, step)
        ema.update(model)
        for k, t in tensors.items():
            assert t._version > last[k], (k, step)
            last[k] = t._version


def test_cpu_models_never_reach_the_library(mini):
    """No emulation, host tensors: the torch loop, and the module's library is not asked for."""
    hip_ema.reset_stats()
    model = copy.deepcopy(mini)
    ema = ModelEMA(model)
    _perturb(model, 0)
    ema.update(model)
    assert ema._hip is None and hip_ema.stats() == dict(launches=0, table_builds=0, torch_tensors=0)


def test_abi_entry_and_argument_checks(tmp_path):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'\bint\s+yh_ema_update\s*\(\s*const\s+yh_ema_row\s*\*', text)
    assert re.search(r'#define\s+YH_ABI_VERSION\s+2\b', text)
    assert int(re.search(r'#define\s+YH_EMA_CHUNK\s+(\d+)', text).group(1)) == EMA_CHUNK
    assert 'yh_ema_update' in hiplib.EXPORTS and hiplib.ABI_VERSION == 2
    lib = hiplib.load()
    assert hasattr(lib, 'yh_ema_update') and lib.yh_abi_version() == 2
    # the argument checks are host code and return before any launch
    rows = (EmaRow * 3)()
    addr = C.addressof(rows)
    assert addr % 8 == 0
    assert lib.yh_ema_update(None, 0, 0, 0.5, 0.5, None) == 0
    assert lib.yh_ema_update(addr, 0, 0, 0.5, 0.5, None) == 0
    assert lib.yh_ema_update(None, 2, 2, 0.5, 0.5, None) == -1
    assert lib.yh_ema_update(addr, -1, 2, 0.5, 0.5, None) == -1
    assert lib.yh_ema_update(addr, 2, -1, 0.5, 0.5, None) == -1
    assert lib.yh_ema_update(addr, 2, 1, 0.5, 0.5, None) == -1
    assert lib.yh_ema_update(addr + 4, 2, 2, 0.5, 0.5, None) == -2
    # the ctypes mirror has the C compiler's layout
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yolo_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(yh_ema_row), offsetof(yh_ema_row, ema), offsetof(yh_ema_row, src), offsetof(yh_ema_row, n), '
                   'offsetof(yh_ema_row, chunk0));return 0;}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(conftest.REPO, 'include'), str(src), '-o', str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(EmaRow), EmaRow.ema.offset, EmaRow.src.offset, EmaRow.n.offset, EmaRow.chunk0.offset]
