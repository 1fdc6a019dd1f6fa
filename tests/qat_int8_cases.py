"""The graphs of the QAT-on-int8 tests (tests/test_qat_int8.py, tests/test_gpu_qat_int8.py): a ``quantized=1`` model of each cfg in the
synthetic calibrated state of ``tools/synthetic_ptq.py`` (``fill_synthetic_qat_state``), at 64 x 64, batch 2, on dyadic frames - the
stem convolution is then exact in any summation order, and the BatchNorm fold of that state is one fp32 product per value, so the
eager modules on a CPU are the reference for the host emulation AND for the device, bit for bit."""
import copy
import os

import torch

import conftest
import qat_minicfg
import synth

SIZE, BATCH = 64, 2
CFGS = {'micro_min': (None, 1), 'micro_max': (None, 2),
        'yolov3-tiny': ('yolov3tiny/yolov3-tiny.cfg', 1), 'yolov4-tiny': ('yolov4tiny/yolov4-tiny.cfg', 1),
        'yolov3': ('yolov3/yolov3.cfg', 1), 'yolov4': ('yolov4/yolov4.cfg', 1)}
CASES = list(CFGS)


def frames():
    return synth.dyadic_frames(synth.image_batch(BATCH, SIZE, seed=0))


def build(cfg, way, **kw):
    """(float model, quantized=1 model in the synthetic state, frames) of ``cfg``: a path below cfg/, a block list, or None for the
    micro detector of qat_minicfg."""
    import models
    from tools.synthetic_ptq import fill_synthetic_qat_state, measure_ranges, seed_qat_batchnorm_

    def source():
        if cfg is None:
            return qat_minicfg.micro_cfg()
        return copy.deepcopy(cfg) if isinstance(cfg, list) else os.path.join(conftest.PKG, 'cfg', cfg)
    x = frames()
    torch.manual_seed(0)
    fm = models.Darknet(source(), (SIZE, SIZE))
    seed_qat_batchnorm_(fm, x)
    torch.manual_seed(0)
    args = dict(quantized=1, a_bit=8, w_bit=8, shortcut_way=way, steps=qat_minicfg.STEPS)
    args.update(kw)
    qm = models.Darknet(source(), (SIZE, SIZE), **args)
    fill_synthetic_qat_state(fm, qm, measure_ranges(fm, x))
    return fm, qm, x


_CACHE = {}


def case(name):
    """(quantised model, frames, eager CPU outputs ``(inf, raws)``) of a named case.  Built and evaluated once per session; callers
    deep-copy the model before they move or change it, and leave the reference tensors alone."""
    if name not in _CACHE:
        cfg, way = CFGS[name]
        _, qm, x = build(cfg, way)
        ref = copy.deepcopy(qm)
        torch.set_num_threads(min(8, os.cpu_count() or 1))
        with torch.no_grad():
            inf, raws, _ = ref(x)
        _CACHE[name] = (qm, x, (inf, raws))
    qm, x, ref = _CACHE[name]
    return copy.deepcopy(qm), x, ref
