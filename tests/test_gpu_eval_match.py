"""GPU tier of the device evaluation matcher: the ``yh_eval_match`` kernel (csrc/evalmatch.hip) through ``engine.evalmatch.match_batch``
against the host loop of ``test.py`` (``clip_coords`` + ``_match``) on CPU copies - flags, written-back boxes and the packed conf / cls
bit for bit: every operation is one IEEE fp32 operation in a fixed order, there is no tolerance to choose.  The batch is the mixed one
of tests/evalmatch_cases.py (None images, no labels, no detections, 1 x 1, a 300-row walk, one label past the LDS staging, tied labels,
tied claimants, wrong class, absent class, boxes outside the image, the exact-0.5 pair), its detections are views into two buffers.
Then ``test.test`` on the GPU with the device matcher and with ``YOLO_HIP_EVAL_MATCH=0``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import conftest

sys.path.insert(0, os.path.join(conftest.REPO, 'tests'))
import evalmatch_cases as cases  # noqa: E402
from engine import evalmatch, hiplib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load()


@pytest.fixture(scope='module', autouse=True)
def release_cached_blocks():
    """Later modules assert on torch.cuda.memory_reserved(): hand the small blocks these tests cached back to the driver"""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def batch():
    return cases.build()


@pytest.mark.parametrize('niou', [1, 10])
def test_kernel_is_the_host_loop_bit_for_bit(lib, batch, niou):
    dets, targets = batch
    iouv = cases.IOUV[niou]
    t_host = torch.from_numpy(targets)
    t_dev = t_host.cuda()
    out, bufs = cases.output_views(dets, 'cuda')
    assert out[4].data_ptr() != out[5].data_ptr() and len({b.data_ptr() for b in bufs}) == 2
    stats = evalmatch.match_batch(out, t_host, t_dev, cases.H, cases.W, iouv.cuda())
    cases.check_against_host_loop(stats, out, bufs, dets, targets, iouv)
    assert torch.equal(t_dev.cpu(), t_host)                    # the targets are read only
    # a second call on the same inputs: the same bits (the only atomic is an integer minimum)
    out2, bufs2 = cases.output_views(dets, 'cuda')
    stats2 = evalmatch.match_batch(out2, t_host, t_dev, cases.H, cases.W, iouv.cuda())
    assert len(stats) == len(stats2)
    for a, b in zip(stats, stats2):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
    for a, b in zip(bufs, bufs2):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    # clipping what is already clipped changes nothing, and the flags stay
    stats3 = evalmatch.match_batch(out, t_host, t_dev, cases.H, cases.W, iouv.cuda())
    for a, b in zip(stats, stats3):
        assert torch.equal(a[0], b[0])
    for a, b in zip(bufs, bufs2):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))


def test_detections_the_kernel_cannot_address_are_staged(lib, batch):
    """fp16 or strided detections go through a dense fp32 stand-in and are clipped all the same"""
    dets, targets = batch
    t_host = torch.from_numpy(targets)
    out, _ = cases.output_views(dets, 'cuda')
    wide = torch.zeros(len(dets[4]), 8, device='cuda')
    wide[:, :6] = out[4]
    out[4] = wide[:, :6]                                       # row pitch 8: not dense
    stats = evalmatch.match_batch(out, t_host, t_host.cuda(), cases.H, cases.W, cases.IOUV[10].cuda())
    want = cases.expected(dets, targets, cases.IOUV[10])
    assert torch.equal(stats[3][0], want[4][1])                # stats: images 1, 2 (the empty entry), 3, 4, ...
    assert np.array_equal(out[4].cpu().contiguous().numpy().view(np.int32), want[4][0].numpy().view(np.int32))


def test_argument_validation_launches_nothing(lib):
    assert lib.yh_eval_match(None, None) == -1
    for kw, rc in cases.REFUSED:
        assert lib.yh_eval_match(C.byref(cases.valid_desc(**kw)), hiplib.stream_ptr()) == rc, kw
    assert lib.yh_eval_match(C.byref(cases.valid_desc(images=0)), hiplib.stream_ptr()) == 0
    assert lib.yh_eval_match(C.byref(cases.valid_desc(total=0)), hiplib.stream_ptr()) == 0
    torch.cuda.synchronize()                                   # the fake addresses were never touched


@pytest.mark.parametrize('branch', ['hip_detect', 'two_pass'])
def test_test_py_same_results_with_the_device_matcher_and_the_host_loop(lib, dataset_dir, tiny_cfg, tmp_path, monkeypatch, branch):
    """Both branches of test(): forward + NMS as one engine call, and (a model that carries `hyp`, as under train.py) forward, loss, NMS"""
    monkeypatch.chdir(tmp_path)
    import models
    import test as test_mod
    torch.manual_seed(3)
    model = models.Darknet(tiny_cfg, (64, 64)).cuda()
    if branch == 'two_pass':
        import train as train_mod
        model.nc, model.hyp, model.gr = 2, dict(train_mod.hyp), 1.0
    test_mod.opt = None
    calls = []
    real = evalmatch.match_batch
    monkeypatch.setattr(evalmatch, 'match_batch', lambda *a: calls.append(1) or real(*a))
    run = lambda: test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), batch_size=2, imgsz=64, model=model, plot=False, save_json=True)
    monkeypatch.delenv('YOLO_HIP_EVAL_MATCH', raising=False)
    res_dev, maps_dev = run()
    json_dev = open('results.json').read()
    assert len(calls) == 2                                     # one call per batch
    monkeypatch.setenv('YOLO_HIP_EVAL_MATCH', '0')
    res_host, maps_host = run()
    assert len(calls) == 2
    assert res_dev[:4] == res_host[:4] and np.array_equal(maps_dev, maps_host)
    assert json_dev == open('results.json').read()
