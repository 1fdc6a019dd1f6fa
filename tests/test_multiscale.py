"""Multi-scale training on the emulated ABI: all input shapes of a training engine share one step arena, so a plan may not rely on
what its own build or previous step left in a buffer; the plan cache, the reservation, the stale-backward guard across shapes,
the arithmetic of the device resize and the wiring of ``train.py --multi-scale``."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import conftest
import fakelib_multiscale
import multiscale_harness as mh
from engine import hiplib

FakeLib = fakelib_multiscale.FakeLibMultiscale
_cache = {}


def _model(which):
    if which not in _cache:
        _cache[which] = mh.build_model(which)
    return _cache[which]


def _fresh(which, precision, seq):
    """Engine B over ``seq``: every step on freshly built plans in a fresh arena.  Computed once per case and shared."""
    key = (which, precision, tuple(seq))
    if key not in _cache:
        steps, bn, _ = mh.run(_model(which), precision, seq, lib=FakeLib(), drop=True)
        _cache[key] = (steps, bn)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. interleaved shapes
@pytest.mark.parametrize('nan_fill', [False, True], ids=['arena_as_left', 'arena_nan_filled'])
@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_interleaved_shapes_equal_fresh_engines(precision, nan_fill):
    steps, bn, st = mh.run(_model('mini'), precision, mh.SEQUENCE, lib=FakeLib(), nan_fill=nan_fill)
    mh.assert_same((steps, bn), _fresh('mini', precision, mh.SEQUENCE))
    assert st.m.hip_train_stats()['plans_resident'] == len(set(mh.SEQUENCE))


@pytest.mark.parametrize('which', ['tiny', 'slim'])
def test_interleaved_shapes_on_the_zero_edged_pool_and_the_padded_twin(which):
    """yolov3-tiny has the k = 2 / s = 1 max-pool with the zero edge; slim_prune_mini trains through the channel-padded twin, whose
    pad lanes must come out zero from the kernels, not from what a buffer held before.  The arena is NaN between the steps."""
    from engine.padded import PaddedTrainEngine
    steps, bn, st = mh.run(_model(which), 'fp16', mh.SHORT, lib=FakeLib(), nan_fill=True)
    assert isinstance(st.engine, PaddedTrainEngine) == (which == 'slim')
    mh.assert_same((steps, bn), _fresh(which, 'fp16', mh.SHORT))


# ------------------------------------------------------------------------------------------------ 2. counters
def test_reservation_makes_the_arena_once_and_every_shape_builds_once():
    distinct = len(set(mh.SEQUENCE))
    steps, bn, st = mh.run(_model('mini'), 'fp32', mh.SEQUENCE, lib=FakeLib(), reserve=[mh.largest(mh.SEQUENCE)])
    mh.assert_same((steps, bn), _fresh('mini', 'fp32', mh.SEQUENCE))
    stats = st.m.hip_train_stats()
    assert stats['arena_allocs'] == 1 and stats['plan_builds'] == distinct and stats['plans_resident'] == distinct
    assert stats['arena_bytes'] > 0 and stats['plan_bytes'] > 0
    again, _, _ = mh.run(None, 'fp32', mh.SEQUENCE, stepper=st)          # second pass: nothing is built, nothing allocated
    after = st.m.hip_train_stats()
    assert after['arena_allocs'] == 1 and after['plan_builds'] == distinct and after['arena_bytes'] == stats['arena_bytes']
    for (ha, ga), (hb, gb) in zip(again, steps):                            # heads and gradients do not depend on the running statistics
        assert all(torch.equal(a, b) for a, b in zip(ha, hb)) and all(torch.equal(ga[k], gb[k]) for k in gb)


def test_without_a_reservation_the_arena_grows_only_at_a_new_maximum():
    seq = [(2, 64, 64), (2, 64, 96), (2, 96, 96), (2, 128, 128), (2, 64, 64), (1, 96, 96)]
    steps, bn, st = mh.run(_model('mini'), 'fp32', seq, lib=FakeLib(), nan_fill=True)
    mh.assert_same((steps, bn), _fresh('mini', 'fp32', seq))
    stats = st.m.hip_train_stats()
    assert 1 <= stats['arena_allocs'] <= 4 and stats['plan_builds'] == len(set(seq))


def test_reserving_a_larger_arena_invalidates_a_forward_in_flight():
    st = mh.Stepper(_model('mini'), 'fp32', FakeLib())
    raws = st.forward(mh.batch(0, (2, 64, 64)))
    st.reserve([(2, 3, 128, 128)])                                          # the activations went with the old arena
    with pytest.raises(RuntimeError, match='overwritten by a later'):
        sum(r.sum() for r in raws).backward()


# ------------------------------------------------------------------------------------------------ 3. eviction
def test_eviction_by_count_keeps_the_arena(monkeypatch):
    monkeypatch.setenv('YOLO_HIP_MAX_TRAIN_PLANS', '2')
    lib = FakeLib()
    steps, bn, st = mh.run(_model('mini'), 'fp32', mh.SEQUENCE, lib=lib, reserve=[mh.largest(mh.SEQUENCE)])
    mh.assert_same((steps, bn), _fresh('mini', 'fp32', mh.SEQUENCE))
    stats = st.m.hip_train_stats()
    assert stats['arena_allocs'] == 1 and stats['plans_resident'] == 2 and stats['plan_builds'] > len(set(mh.SEQUENCE))
    assert len(lib.plans) == 4                                              # the evicted plans' native handles are gone
    st.engine._drop_plans()
    assert len(lib.plans) == 0 and st.m.hip_train_stats()['arena_bytes'] == 0


# ------------------------------------------------------------------------------------------------ 4. stale backward
def test_backward_of_another_shape_s_forward_raises():
    st = mh.Stepper(_model('mini'), 'fp32', FakeLib())
    raws_a = st.forward(mh.batch(0, (2, 64, 64)))
    st.forward(mh.batch(1, (2, 96, 96)))
    with pytest.raises(RuntimeError, match='overwritten by a later'):
        sum(r.sum() for r in raws_a).backward()


# ------------------------------------------------------------------------------------------------ 5. resize arithmetic
RESIZE_CASES = [(608, 608, 416, 416), (608, 608, 896, 896), (416, 416, 640, 640), (64, 64, 96, 96), (96, 128, 64, 96), (128, 96, 160, 128)]


@pytest.mark.parametrize('ih,iw,oh,ow', RESIZE_CASES)
def test_resize_emulation_equals_the_restated_formula_and_is_as_close_to_torch_as_torch_is_to_float64(ih, iw, oh, ow):
    """Distance of our fp32 arithmetic to F.interpolate in fp32 <= distance of that fp32 result to F.interpolate in float64."""
    from engine.preprocess import resize_bilinear
    torch.manual_seed(0)
    x = torch.rand(2, 3, ih, iw)
    got = resize_bilinear(x, (oh, ow), lib=FakeLib())
    want = mh.restate_resize(x.numpy(), (oh, ow))
    assert got.shape == (2, 3, oh, ow) and got.numpy().tobytes() == want.tobytes()
    t32 = torch.nn.functional.interpolate(x, size=(oh, ow), mode='bilinear', align_corners=False)
    t64 = torch.nn.functional.interpolate(x.double(), size=(oh, ow), mode='bilinear', align_corners=False)
    ours = (got.double() - t32.double()).abs().max().item()
    torchs = (t32.double() - t64).abs().max().item()
    print('resize %s: |ours - torch fp32| %.3g, |torch fp32 - float64| %.3g' % ((ih, iw, oh, ow), ours, torchs))
    assert ours <= torchs


@pytest.mark.parametrize('shape', [(3, 3, 64, 64), (1, 1, 33, 47)])
def test_resize_to_the_same_size_returns_the_input_bits(shape):
    from engine.preprocess import resize_bilinear
    torch.manual_seed(0)
    x = torch.randn(shape) * 100
    got = resize_bilinear(x, shape[2:], lib=FakeLib())
    assert got.numpy().tobytes() == x.numpy().tobytes()
    assert mh.restate_resize(x.numpy(), shape[2:]).tobytes() == x.numpy().tobytes()


def test_resize_rejects_what_it_does_not_do():
    from engine.preprocess import resize_bilinear
    with pytest.raises(ValueError):
        resize_bilinear(torch.rand(2, 3, 8, 8).half(), (4, 4), lib=FakeLib())
    with pytest.raises(ValueError):
        resize_bilinear(torch.rand(2, 3, 8, 8), (0, 4), lib=FakeLib())


# ------------------------------------------------------------------------------------------------ 6. train.py wiring
def _two_image_run(dataset_dir, tiny_cfg, tmp_path, monkeypatch, hip):
    """train.py --multi-scale on two synthetic images, CPU tensors, one step per epoch; every draw picks the smallest size, so each
    step rescales.  -> (reservations [(model, shapes, precision)], sizes F.interpolate was asked for)."""
    monkeypatch.chdir(tmp_path)
    import models
    import train as train_mod
    files = (dataset_dir / 'train.txt').read_text().split('\n')[:2]
    (tmp_path / 'two.txt').write_text('\n'.join(files) + '\n')
    (tmp_path / 'two.data').write_text('classes=2\ntrain=%s\nvalid=%s\nnames=%s\n' % (tmp_path / 'two.txt', tmp_path / 'two.txt',
                                                                                 dataset_dir / 'synth.names'))
    reservations, resized = [], []
    real_reserve = models.Darknet.hip_reserve_train
    real_interpolate = torch.nn.functional.interpolate

    def reserve(self, shapes, precision=None):
        reservations.append((self, [tuple(s) for s in shapes], precision))
        return real_reserve(self, shapes, precision=precision)

    def interpolate(x, *args, **kw):
        if kw.get('mode') == 'bilinear' and kw.get('align_corners') is False:
            resized.append(tuple(kw['size']))
        return real_interpolate(x, *args, **kw)

    monkeypatch.setattr(models.Darknet, 'hip_reserve_train', reserve)
    monkeypatch.setattr(torch.nn.functional, 'interpolate', interpolate)
    monkeypatch.setattr(train_mod.random, 'randrange', lambda lo, hi: lo)
    if hip:
        # what a GPU run has: the step goes through the HIP engine, here over the emulated ABI (the tensors stay on the CPU)
        lib = FakeLib()
        monkeypatch.setattr(hiplib, 'load', lambda: lib)
        monkeypatch.setattr(train_mod, 'hip_train_path', lambda device, opt: True)
    opt = train_mod.make_parser().parse_args(['--epochs', '2', '--batch-size', '2', '--cfg', tiny_cfg, '--data', str(tmp_path / 'two.data'),
                                              '--img-size', '64', '64', '64', '--device', 'cpu', '--nosave', '--notest', '--multi-scale'])
    opt.local_rank = -1
    results = train_mod.train(opt, train_mod.hyp)
    assert len(results) == 7
    return reservations, resized


def test_train_py_multi_scale_on_the_cpu_reserves_nothing_and_keeps_interpolate(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    reservations, resized = _two_image_run(dataset_dir, tiny_cfg, tmp_path, monkeypatch, hip=False)
    assert reservations == []
    assert resized and set(resized) == {(32, 32)}


def test_train_py_multi_scale_reserves_once_for_the_rounded_largest_size(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    """--img-size 64 with --multi-scale spans int(64 / 0.667) = 95 -> 64 after the grid rounding: that is what is reserved."""
    reservations, resized = _two_image_run(dataset_dir, tiny_cfg, tmp_path, monkeypatch, hip=True)
    assert len(reservations) == 1
    model, shapes, precision = reservations[0]
    assert shapes == [(2, 3, 64, 64)] and precision == 'fp32'
    stats = model.hip_train_stats()
    assert stats['arena_allocs'] == 1 and stats['arena_bytes'] > 0 and stats['plan_builds'] == 1
    assert resized and set(resized) == {(32, 32)}      # CPU tensors: the F.interpolate branch, also when the HIP path is on


# ------------------------------------------------------------------------------------------------ 7. ABI
def test_resize_entry_point_is_exported_and_its_descriptor_matches_the_c_compiler(tmp_path):
    lib = hiplib.load()
    assert hasattr(lib, 'yh_resize_bilinear') and 'yh_resize_bilinear' in hiplib.EXPORTS
    assert lib.yh_abi_version() == hiplib.ABI_VERSION == 2
    cls, cname = hiplib.ResizeDesc, 'yh_resize_desc'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolo_hip.h"', 'int main(void){',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(conftest.REPO, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, fname
    # host-side argument checks run without a GPU: nothing is launched for a descriptor that is refused
    d = hiplib.ResizeDesc(src=4096, dst=8192, n=1, c=1, ih=4, iw=4, oh=0, ow=4, scale_h=1.0, scale_w=1.0)
    assert lib.yh_resize_bilinear(C.byref(d), None) == -1
    d = hiplib.ResizeDesc(src=None, dst=8192, n=1, c=1, ih=4, iw=4, oh=4, ow=4, scale_h=1.0, scale_w=1.0)
    assert lib.yh_resize_bilinear(C.byref(d), None) == -1
    d = hiplib.ResizeDesc(src=4096, dst=8192, n=1, c=1, ih=4, iw=4, oh=4, ow=4, scale_h=float('nan'), scale_w=1.0)
    assert lib.yh_resize_bilinear(C.byref(d), None) == -1
