#!/usr/bin/env python3
"""Recorded runs of the reference's distillation losses ``compute_lost_KD2`` / ``KD3`` / ``KD4`` (utils/utils.py:446-564), for tests
that must run without a reference checkout.

    YOLO_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_kd.py

Writes ``tests/golden/kd_losses.npz``.  The case: the yolov3-tiny graph of the package's ``yolov3-tiny-hand.cfg`` (one class, 12
``feature_out`` tensors, one of them the stride-1 max-pool) at 64 px, batch 2, with every conv width divided by 8 for the student and by
4 for the teacher - the pruned-student case: channel counts differ, the file stays small - built and run by the REFERENCE's ``Darknet``
in training mode.  Three labels, two of them in image 0.  Stored:

* ``cfg_s``                      the student's cfg text (the tests build the package's Darknet on it for anchors and strides)
* ``targets``, ``iou_t``         labels and the one hyper-parameter ``build_targets`` reads
* ``out_s<i>``, ``out_t<i>``     raw heads of student and teacher; ``fs<j>``, ``ft<j>`` their feature_out tensors (4-D)
* ``kd2_loss``, ``kd2_reg_ratio``, ``kd3_loss``, ``kd4_loss``
* ``kd<k>_dout<i>``              autograd gradient of the loss with respect to ``out_s<i>``;  ``kd4_dfs<j>`` with respect to ``fs<j>``
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: F401,E402
import refharness  # noqa: E402
import train_harness as th  # noqa: E402

SIZE, BATCH, NC = 64, 2, 1
TARGETS = [[0, 0, 0.30, 0.50, 0.25, 0.30], [0, 0, 0.70, 0.30, 0.40, 0.20], [1, 0, 0.45, 0.55, 0.50, 0.60]]
IOU_T = 0.20


def thin_cfg(div):
    text = open(os.path.join(conftest.PKG, 'cfg', 'yolov3tiny', 'yolov3-tiny-hand.cfg')).read()
    head = 3 * (NC + 5)
    return re.sub(r'filters=(\d+)', lambda m: m.group(0) if int(m.group(1)) == head else 'filters=%d' % (int(m.group(1)) // div), text)


def run_model(ref, text, seed, x):
    path = th.write_cfg(text)
    try:
        torch.manual_seed(seed)
        model = ref.models.Darknet(path, (SIZE, SIZE)).train()
    finally:
        os.unlink(path)
    model.nc, model.hyp = NC, {'iou_t': IOU_T}
    with torch.no_grad():
        out, feats = model(x)
    return model, [o.detach().clone() for o in out], [f.detach().clone() for f in feats]


def main():
    ref = refharness.load()
    g = torch.Generator().manual_seed(11)
    x = torch.rand(BATCH, 3, SIZE, SIZE, generator=g)
    cfg_s = thin_cfg(8)
    student, out_s, fs = run_model(ref, cfg_s, 0, x)
    _, out_t, ft = run_model(ref, thin_cfg(4), 3, x)
    assert len(fs) == len(ft) == 12 and any(a.shape[1] != b.shape[1] for a, b in zip(fs, ft))
    targets = torch.tensor(TARGETS)
    rec = dict(cfg_s=np.array(cfg_s), targets=targets.numpy(), iou_t=np.float32(IOU_T))
    for i, (a, b) in enumerate(zip(out_s, out_t)):
        rec['out_s%d' % i], rec['out_t%d' % i] = a.numpy(), b.numpy()
    for j, (a, b) in enumerate(zip(fs, ft)):
        rec['fs%d' % j], rec['ft%d' % j] = a.numpy(), b.numpy()

    def leaves(ts):
        return [t.clone().requires_grad_(True) for t in ts]

    for k in (2, 3, 4):
        po, pf = leaves(out_s), leaves(fs)
        if k == 2:
            loss, ratio = ref.utils.compute_lost_KD2(student, targets, po, [t.clone() for t in out_t])
            rec['kd2_reg_ratio'] = np.float64(ratio)
        elif k == 3:
            loss = ref.utils.compute_lost_KD3(student, targets, po, [t.clone() for t in out_t])
        else:
            # the reference overwrites the entries of both feature lists: hand it copies of the lists
            loss = ref.utils.compute_lost_KD4(student, targets, po, [t.clone() for t in out_t], list(pf), [t.clone() for t in ft], BATCH)
        loss.sum().backward()
        rec['kd%d_loss' % k] = loss.detach().numpy()
        for i, p in enumerate(po):
            rec['kd%d_dout%d' % (k, i)] = p.grad.numpy()
        if k == 4:
            for j, p in enumerate(pf):
                rec['kd4_dfs%d' % j] = p.grad.numpy()
    path = os.path.join(HERE, 'kd_losses.npz')
    np.savez_compressed(path, **rec)
    print('wrote', path, os.path.getsize(path), 'bytes; losses', [float(rec['kd%d_loss' % k][0]) for k in (2, 3, 4)], 'reg_ratio', rec['kd2_reg_ratio'])


if __name__ == '__main__':
    main()
