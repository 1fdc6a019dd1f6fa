"""CPU tier of the device evaluation matcher (``yh_eval_match``, engine/evalmatch.py): the C ABI, the binding driven through a host
emulation of the kernel (tests/fakelib_evalmatch.py, written from the documented steps), bit-equal to the host loop of ``test.py``
(``clip_coords`` + ``_match``), to the statistics the reference's ``test()`` records (tests/golden/eval_match.npz), and ``test.test``
end to end with the emulated matcher against the host loop.  The kernel itself: tests/test_gpu_eval_match.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest

sys.path.insert(0, os.path.join(conftest.REPO, 'tests'))
import evalmatch_cases as cases  # noqa: E402
import fakelib_evalmatch  # noqa: E402
from engine import evalmatch, hiplib  # noqa: E402

GOLDEN = os.path.join(conftest.REPO, 'tests', 'golden', 'eval_match.npz')
IOUV = cases.IOUV


@pytest.fixture
def fake():
    lib = fakelib_evalmatch.FakeLibEvalMatch()
    evalmatch._LIB_OVERRIDE = lib
    yield lib
    evalmatch._LIB_OVERRIDE = None


@pytest.mark.parametrize('niou', [1, 10])
def test_emulated_matcher_is_the_host_loop_bit_for_bit(fake, niou):
    dets, targets = cases.build()
    out, bufs = cases.output_views(dets, 'cpu')
    t = torch.from_numpy(targets)
    stats = evalmatch.match_batch(out, t, t.clone(), cases.H, cases.W, IOUV[niou])
    assert fake.match_calls == [(cases.NB, sum(len(d) for d in dets if d is not None), niou)]      # one launch for the batch
    want = cases.check_against_host_loop(stats, out, bufs, dets, targets, IOUV[niou])
    # the batch is not trivially all-false: claims happen, ties are decided, the exact-0.5 pair does not claim
    flags4 = want[4][1][:, 0]
    assert flags4.sum() >= 5 and flags4[1] and not flags4[[40, 41, 299]].any()      # copies of one box: the first claimant only
    assert flags4[0] and not flags4[260] and not flags4[19] and not flags4[20:27].any()
    # the chunked images: winners live in every chunk, and the flags are NOT those of a matcher that stops at the staging capacity,
    # or after two chunks
    cap = hiplib.EVAL_MATCH_LDS_LABELS
    assert want[5][1][:3, 0].all() and want[5][1][1].all() and want[8][1][[0, 1, 2, 3, 5], 0].all() and not want[8][1][4].any()
    one, two = cases.expected(dets, targets, IOUV[niou], keep_labels=cap), cases.expected(dets, targets, IOUV[niou], keep_labels=2 * cap)
    assert not torch.equal(one[5][1], want[5][1]) and not torch.equal(one[8][1], want[8][1]) and not torch.equal(two[8][1], want[8][1])
    assert torch.equal(one[4][1], want[4][1]) and torch.equal(two[5][1], want[5][1])
    assert want[3][1].all() == (niou == 1) and want[3][1][0, 0] and not want[6][1].any() and not want[1][1].any()


def test_empty_batches_launch_nothing(fake):
    t = torch.zeros(0, 6)
    assert evalmatch.match_batch([None, None], t, t, 48, 64, IOUV[1]) == []
    lab = torch.tensor([[1, 0, 0.5, 0.5, 0.2, 0.2]])
    stats = evalmatch.match_batch([None, None, torch.zeros(0, 6)], lab, lab, 48, 64, IOUV[10])
    assert fake.match_calls == [] and len(stats) == 2
    assert tuple(stats[0][0].shape) == (0, 10) and stats[0][3] == [0.0] and stats[1][3] == []


def test_switch_and_cpu_tensors_keep_the_host_loop(monkeypatch):
    monkeypatch.delenv('YOLO_HIP_EVAL_MATCH', raising=False)
    assert not evalmatch.enabled(torch.device('cpu')) and evalmatch.enabled(torch.device('cuda', 0)) and not evalmatch.enabled('cpu')
    monkeypatch.setenv('YOLO_HIP_EVAL_MATCH', '0')
    assert not evalmatch.enabled(torch.device('cuda', 0))


def test_test_py_returns_identical_values_with_the_emulated_matcher(fake, dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    import models
    import test as test_mod
    torch.manual_seed(3)
    model = models.Darknet(tiny_cfg, (64, 64))
    test_mod.opt = None
    # the CPU tier has no CUDA tensors: route test() to match_batch (on the emulated kernel) the way enabled() does on a GPU
    monkeypatch.setattr(evalmatch, 'enabled', lambda device: os.environ.get('YOLO_HIP_EVAL_MATCH', '1') != '0')
    run = lambda: test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), batch_size=2, imgsz=64, model=model, plot=False, save_json=True)
    res_dev, maps_dev = run()
    json_dev = open('results.json').read()
    assert len(fake.match_calls) == 2 and all(c[1] > 0 for c in fake.match_calls)      # one launch per batch, with detections
    monkeypatch.setenv('YOLO_HIP_EVAL_MATCH', '0')
    res_host, maps_host = run()
    assert len(fake.match_calls) == 2
    assert res_dev == res_host and np.array_equal(maps_dev, maps_host)
    assert json_dev == open('results.json').read()       # --save-json saw the same (clipped) boxes


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_and_header_declares_the_matcher(tmp_path):
    lib = hiplib.load()
    assert hasattr(lib, 'yh_eval_match') and 'yh_eval_match' in hiplib.EXPORTS
    header = open(os.path.join(conftest.REPO, 'include', 'yolo_hip.h')).read()
    assert re.search(r'\bint\s+yh_eval_match\s*\(\s*const\s+yh_eval_match_desc\s*\*', header)
    assert int(re.search(r'#define\s+YH_EVAL_MATCH_LDS_LABELS\s+(\d+)', header).group(1)) == hiplib.EVAL_MATCH_LDS_LABELS
    assert int(re.search(r'#define\s+YH_ABI_VERSION\s+(\d+)', header).group(1)) == 2 == lib.yh_abi_version()
    structs = {'yh_eval_match_desc': hiplib.EvalMatchDesc, 'yh_eval_match_row': hiplib.EvalMatchRow}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolo_hip.h"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(conftest.REPO, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, '%s.%s' % (cname, fname)


def test_argument_validation_returns_before_any_launch():
    """Host code: runs without a GPU.  Bad arguments are refused, empty work is YH_OK - neither reaches a launch."""
    lib = hiplib.load()
    assert lib.yh_eval_match(None, None) == -1
    for kw, rc in cases.REFUSED:
        assert lib.yh_eval_match(C.byref(cases.valid_desc(**kw)), None) == rc, kw
    assert lib.yh_eval_match(C.byref(cases.valid_desc(images=0)), None) == 0
    assert lib.yh_eval_match(C.byref(cases.valid_desc(total=0, rows=None, ws=None)), None) == 0
    fake_lib = fakelib_evalmatch.FakeLibEvalMatch()       # the emulation refuses the same things
    for kw, rc in cases.REFUSED:
        assert fake_lib.yh_eval_match(C.byref(cases.valid_desc(**kw)), None) == rc, kw
    assert fake_lib.match_calls == []


# ------------------------------------------------------------------------------------------------ the reference's statistics
def _golden_batches():
    z = np.load(GOLDEN)
    for b in range(int(z['batches'])):
        nb = int(z['b%d_images' % b])
        yield z, b, [z['b%d_out%d' % (b, i)] if 'b%d_out%d' % (b, i) in z.files else None for i in range(nb)]


@pytest.mark.parametrize('matcher', ['emulation', 'host_loop'])
def test_reference_statistics_are_reproduced(fake, matcher):
    """tests/golden/eval_match.npz: the NMS outputs the reference's test() matched and the (tp, conf, pcls, tcls) it handed to
    ap_per_class (tests/golden/make_golden_eval_match.py).  Both the emulated matcher and test._match give those flags exactly."""
    import test as test_mod
    from utils.utils import clip_coords
    tp, conf, pcls, tcls = [], [], [], []
    for z, b, dets in _golden_batches():
        h, w = (int(v) for v in z['b%d_hw' % b])
        targets = torch.from_numpy(z['b%d_targets' % b])
        out = [None if d is None else torch.from_numpy(d.copy()) for d in dets]
        if matcher == 'emulation':
            stats = evalmatch.match_batch(out, targets, targets.clone(), h, w, IOUV[1])
        else:
            stats = []
            whwh = torch.tensor([w, h, w, h], dtype=torch.float32)
            for si, pred in enumerate(out):
                labels = targets[targets[:, 0] == si, 1:]
                if pred is None:
                    if len(labels):
                        stats.append((torch.zeros(0, 1, dtype=torch.bool), torch.Tensor(), torch.Tensor(), labels[:, 0].tolist()))
                    continue
                clip_coords(pred, (h, w))
                stats.append((test_mod._match(pred, labels, whwh, IOUV[1]), pred[:, 4], pred[:, 5], labels[:, 0].tolist()))
        for c, s, k, t in stats:
            tp.append(c.numpy()), conf.append(s.numpy()), pcls.append(k.numpy()), tcls.append(np.asarray(t, np.float64))
    z = np.load(GOLDEN)
    got_tp = np.concatenate(tp, 0)
    assert got_tp.shape == z['tp'].shape and got_tp.shape[0] > 200 and 10 < z['tp'].sum() < got_tp.shape[0]
    assert np.array_equal(got_tp, z['tp'])
    assert np.array_equal(np.concatenate(conf).view(np.int32), z['conf'].view(np.int32))
    assert np.array_equal(np.concatenate(pcls), z['pcls']) and np.array_equal(np.concatenate(tcls), z['tcls'])
