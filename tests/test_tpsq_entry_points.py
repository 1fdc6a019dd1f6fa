"""``train.py --quantized 2``, then ``test.py`` and ``detect.py`` on the checkpoint, with no checkout of the reference in reach: the
entry points pass ``quantized`` through to ``Darknet`` and the graph is built from this package's own TPSQ modules, whose learnable
scales train in their own Adam parameter group."""
import os

import numpy as np
import torch

import tpsq_cases as tc


def test_train_test_detect_with_quantized_2(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    empty = tmp_path / 'no_reference'
    empty.mkdir()
    monkeypatch.setenv('YOLO_REFERENCE_ROOT', str(empty))
    monkeypatch.chdir(tmp_path)
    Q = tc.native_module()
    import train as train_mod
    import test as test_mod
    import detect as detect_mod
    opt = train_mod.make_parser().parse_args(['--epochs', '1', '--batch-size', '4', '--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'),
                                              '--img-size', '64', '64', '64', '--device', 'cpu', '--nosave', '--notest', '--quantized', '2'])
    opt.local_rank = -1
    results = train_mod.train(opt, train_mod.hyp)
    assert len(results) == 7 and all(np.isfinite(results))
    ckpt = torch.load('weights/last.pt', map_location='cpu', weights_only=False)
    sd = ckpt['model']
    scales = [v for k, v in sd.items() if k.endswith('activation_quantizer.scale') or k.endswith('weight_quantizer.scale')]
    warm = [v for k, v in sd.items() if k.endswith('activation_quantizer.warmup')]
    steps = [v for k, v in sd.items() if k.endswith('Conv2d.step')]
    assert scales and all(float(s) > 0 and np.isfinite(float(s)) for s in scales)
    assert warm and all(float(w) == 0 for w in warm) and steps and all(float(s) == 2 for s in steps)      # 1 epoch x 2 batches
    test_mod.opt = None
    (mp, mr, m_ap, mf1, *losses), maps = test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), 'weights/last.pt', batch_size=2, imgsz=64,
                                                       plot=False, quantized=2)
    assert 0.0 <= m_ap <= 1.0 and all(np.isfinite(losses))
    dopt = detect_mod.make_parser().parse_args(['--cfg', tiny_cfg, '--weights', 'weights/last.pt', '--source', str(dataset_dir / 'images'),
                                               '--output', 'out', '--img-size', '64', '--conf-thres', '0.001', '--device', 'cpu',
                                               '--names', str(dataset_dir / 'synth.names'), '--quantized', '2'])
    assert len(detect_mod.detect(dopt)) == 12
    assert os.path.abspath(Q.__file__).startswith(os.path.dirname(os.path.abspath(train_mod.__file__)))
