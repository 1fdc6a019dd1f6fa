"""``train.py --quantized 1``, then ``test.py`` and ``detect.py`` on the checkpoint, with no checkout of the reference in reach: the
entry points pass ``quantized`` through to ``Darknet`` and the graph is built from this package's own QAT modules."""
import os

import numpy as np
import torch

import qat_cases as qc


def test_train_test_detect_with_quantized_1(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    empty = tmp_path / 'no_reference'
    empty.mkdir()
    monkeypatch.setenv('YOLO_REFERENCE_ROOT', str(empty))
    monkeypatch.chdir(tmp_path)
    Q = qc.native_module()
    import train as train_mod
    import test as test_mod
    import detect as detect_mod
    opt = train_mod.make_parser().parse_args(['--epochs', '5', '--batch-size', '4', '--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'),
                                              '--img-size', '64', '64', '64', '--device', 'cpu', '--nosave', '--notest', '--quantized', '1'])
    opt.local_rank = -1      # 10 steps in all: Scale_freeze_step = 1 (with fewer than 10 it is 0 and the scales never leave 0, as in the reference)
    results = train_mod.train(opt, train_mod.hyp)
    assert len(results) == 7 and all(np.isfinite(results))
    ckpt = torch.load('weights/last.pt', map_location='cpu', weights_only=False)
    scales = [v for k, v in ckpt['model'].items() if k.endswith('activation_quantizer.scale')]
    steps = [v for k, v in ckpt['model'].items() if k.endswith('Conv2d.step')]
    assert scales and all(float(s) > 0 for s in scales) and steps and all(float(s) == 10 for s in steps)      # 5 epochs x 2 batches
    test_mod.opt = None
    (mp, mr, m_ap, mf1, *losses), maps = test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), 'weights/last.pt', batch_size=2, imgsz=64,
                                                       plot=False, quantized=1, shortcut_way=1)
    assert 0.0 <= m_ap <= 1.0 and all(np.isfinite(losses))
    dopt = detect_mod.make_parser().parse_args(['--cfg', tiny_cfg, '--weights', 'weights/last.pt', '--source', str(dataset_dir / 'images'),
                                               '--output', 'out', '--img-size', '64', '--conf-thres', '0.001', '--device', 'cpu',
                                               '--names', str(dataset_dir / 'synth.names'), '--quantized', '1'])
    assert len(detect_mod.detect(dopt)) == 12
    assert os.path.abspath(Q.__file__).startswith(os.path.dirname(os.path.abspath(train_mod.__file__)))
