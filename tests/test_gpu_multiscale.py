"""GPU tier of multi-scale training: ``yh_resize_bilinear`` (csrc/resize.hip) against the numpy restatement of its formula, bit for
bit; whole training steps over interleaved input shapes on one engine (plans aliasing in the step arena, the arena filled with NaN
between steps) against an engine that rebuilds its plan for every step; the counters after a reservation.  The step is
bit-reproducible run to run (tests/test_gpu_train.py), so the comparisons are ``torch.equal``."""
import pytest
import torch

import multiscale_harness as mh
from engine import hiplib

pytestmark = pytest.mark.gpu

GUARD = 12345.0
_cache = {}


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load()


# (n, c, ih, iw) -> (oh, ow): up, down on a rectangle, one channel with odd sizes and row tails, identity
RESIZE_CASES = [((2, 3, 64, 64), (96, 96)), ((2, 3, 96, 128), (64, 96)), ((1, 1, 33, 47), (50, 31)), ((3, 3, 64, 64), (64, 64))]


@pytest.mark.parametrize('inputs', ['rand', 'randn_x100'])
@pytest.mark.parametrize('shape,size', RESIZE_CASES)
def test_resize_kernel_is_bit_equal_to_the_restated_formula(lib, shape, size, inputs):
    """randn * 100 would expose a half-precision intermediate; the guard floats past the output, a store outside it."""
    from engine.preprocess import resize_bilinear
    torch.manual_seed(0)
    x = torch.rand(shape) if inputs == 'rand' else torch.randn(shape) * 100
    n, c = shape[:2]
    numel = n * c * size[0] * size[1]
    flat = torch.full((numel + 64,), GUARD, device='cuda')
    got = resize_bilinear(x.cuda(), size, out=flat[:numel].view(n, c, *size))
    torch.cuda.synchronize()
    want = mh.restate_resize(x.numpy(), size)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(flat[numel:].cpu(), torch.full((64,), GUARD))
    if tuple(shape[2:]) == tuple(size):
        assert got.cpu().numpy().tobytes() == x.numpy().tobytes()


def _fresh(which, precision, seq):
    key = (which, precision, tuple(seq))
    if key not in _cache:
        steps, bn, _ = mh.run(mh.build_model(which), precision, seq, device='cuda', drop=True)
        _cache[key] = (steps, bn)
    return _cache[key]


@pytest.mark.parametrize('which,precision,seq', [('mini', 'fp32', mh.SEQUENCE), ('mini', 'fp16', mh.SEQUENCE), ('tiny', 'fp16', mh.SHORT),
                                                 ('slim', 'fp16', mh.SHORT)], ids=['mini-fp32', 'mini-fp16', 'tiny-fp16', 'slim-fp16'])
def test_interleaved_shapes_equal_fresh_engines(lib, which, precision, seq):
    """Engine A keeps its plans and has its arena filled with NaN before every step; engine B drops its plans (and its arena)
    before every step.  Heads and gradients of every step and the BatchNorm statistics after the sequence are the same bits."""
    steps, bn, st = mh.run(mh.build_model(which), precision, seq, device='cuda', nan_fill=True)
    torch.cuda.synchronize()
    mh.assert_same((steps, bn), _fresh(which, precision, seq))
    for heads, grads in steps:
        assert all(torch.isfinite(h).all() for h in heads) and all(torch.isfinite(g).all() for g in grads.values())


def test_after_a_reservation_a_second_pass_builds_and_allocates_nothing(lib):
    model = mh.build_model('mini')
    steps, bn, st = mh.run(model, 'fp16', mh.SEQUENCE, device='cuda', reserve=[mh.largest(mh.SEQUENCE)])
    torch.cuda.synchronize()
    mh.assert_same((steps, bn), _fresh('mini', 'fp16', mh.SEQUENCE))
    stats = st.m.hip_train_stats()
    reserved = torch.cuda.memory_reserved()
    assert stats['arena_allocs'] == 1 and stats['plan_builds'] == len(set(mh.SEQUENCE))
    mh.run(None, 'fp16', mh.SEQUENCE, stepper=st)
    torch.cuda.synchronize()
    after = st.m.hip_train_stats()
    assert (after['arena_allocs'], after['plan_builds'], after['arena_bytes']) == (1, stats['plan_builds'], stats['arena_bytes'])
    assert torch.cuda.memory_reserved() == reserved
