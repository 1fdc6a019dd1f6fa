"""GPU tier of COCO scoring: the ``yh_coco_match`` / ``yh_coco_accumulate`` kernels (csrc/cocoeval.hip) through
``engine.cocoeval.evaluate_device`` against the host statement utils/cocoeval.py - ``precision``, ``recall`` and ``stats`` bit for bit:
every value is one IEEE fp64 operation in a fixed order and the counts are integers, there is no tolerance to choose.  Every pair of
every set is evaluated on both sides and every entry of the arrays is compared.  The sets are those of tests/coco_cases.py: the mixed
generated one, and the directed shapes (0 / 1 / 100 / 101 / 300 detections and 0 / 1 / 63 / 64 / 65 / 130 ground truths in a pair, category
lists of 1 / 255 / 256 / 257 / 700 / 5000 around the 256-element scan chunk, a category ignored in one area range only, K = 1 and 80).
Then ``test.test(..., coco_metrics=True)`` on the GPU against the same call with ``YOLO_HIP_COCO_EVAL=0``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import conftest

sys.path.insert(0, os.path.join(conftest.REPO, 'tests'))
import coco_cases as cases  # noqa: E402
from engine import cocoeval as engine, hiplib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load()


@pytest.fixture(scope='module', autouse=True)
def private_memory_pool():
    """A later module (tests/test_gpu_multiscale.py) asserts that torch.cuda.memory_reserved() does not move, which depends on the
    blocks every earlier module left in the caching allocator - cached or handed back.  These tests allocate from a pool of their
    own and return it whole, so the default pool is as they found it."""
    if not torch.cuda.is_available():
        yield
        return
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
    torch.cuda.synchronize()
    del pool


@pytest.mark.parametrize('name', ['generated', 'directed1', 'directed80'])
def test_kernels_are_the_host_statement_bit_for_bit(lib, name):
    dets, gts, n, K, want = cases.reference(name)
    got = engine.evaluate_device(dets, gts, n, K, 'cuda:0')
    cases.same_bits(got, want)
    assert engine.LAST['hip_launches'] == 2
    # a second run: the same bytes (no atomics anywhere)
    again = engine.evaluate_device(dets, gts, n, K, 'cuda:0')
    for key in ('precision', 'recall', 'stats'):
        assert got[key].tobytes() == again[key].tobytes(), key


def test_empty_sides(lib):
    box = (10., 10., 50., 40.)
    from utils import cocoeval as host
    for d, g in (([], []), ([(0, 0, *box, 0.9)], []), ([], [(1, 1, *box, 2000., 0)])):
        d, g = np.asarray(d, np.float64).reshape(-1, 7), np.asarray(g, np.float64).reshape(-1, 8)
        cases.same_bits(engine.evaluate_device(d, g, 2, 2, 'cuda:0'), host.evaluate(d, g, 2, 2))


def test_argument_validation_launches_nothing(lib):
    assert lib.yh_coco_match(None, None) == -1 and lib.yh_coco_accumulate(None, None) == -1
    for kw, rc in cases.MATCH_REFUSED:
        assert lib.yh_coco_match(C.byref(cases.valid_match_desc(**kw)), hiplib.stream_ptr()) == rc, kw
    for kw, rc in cases.ACCUM_REFUSED:
        assert lib.yh_coco_accumulate(C.byref(cases.valid_accum_desc(**kw)), hiplib.stream_ptr()) == rc, kw
    assert lib.yh_coco_match(C.byref(cases.valid_match_desc(n_pairs=0)), hiplib.stream_ptr()) == 0
    torch.cuda.synchronize()                                   # the fake addresses were never touched


def test_test_py_same_coco_result_on_the_device_and_with_the_host_statement(lib, dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    import models
    import test as test_mod
    torch.manual_seed(3)
    model = models.Darknet(tiny_cfg, (64, 64)).cuda()
    test_mod.opt = None
    calls = []
    real = engine.evaluate_device
    monkeypatch.setattr(engine, 'evaluate_device', lambda *a: calls.append(1) or real(*a))
    run = lambda: test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), batch_size=2, imgsz=64, model=model, plot=False, coco_metrics=True)
    monkeypatch.delenv('YOLO_HIP_COCO_EVAL', raising=False)
    res_dev = run()
    coco_dev = test_mod.coco_result
    assert len(calls) == 1 and (coco_dev['recall'][:, :, 0, 2] > -1).all()
    monkeypatch.setenv('YOLO_HIP_COCO_EVAL', '0')
    res_host = run()
    assert len(calls) == 1 and test_mod.coco_result is not coco_dev
    cases.same_bits(coco_dev, test_mod.coco_result)
    assert res_dev[0][:4] == res_host[0][:4] and np.array_equal(res_dev[1], res_host[1])
