#!/usr/bin/env python3
"""Recorded results of the reference's network-slimming code, for tests that must run without a reference checkout.

    YOLO_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_slimming.py

Writes, under tests/golden/:
* ``prune_sets.json``  - ``parse_module_defs`` / ``parse_module_defs2`` / ``parse_module_defs4`` (utils/prune_utils.py) on every cfg of the
  package's cfg/ tree and on the 21-block mini cfg: ``{cfg: {mode: {"returns": [...]} | {"raises": "<exception class>"}}}``; sets are
  stored sorted, the shortcut map as [[key, value], ...].
* ``bn_l1.npz``        - ``BNOptimizer.updateBN`` on gamma vectors with 0, -0, negatives, NaN and denormals: ``gamma_k``, ``grad_k`` and the
  updated gradients ``out<j>_k`` for the two penalties ``s`` (rows of 1, 3, 13, 64, 65, 255, 1024 elements).
* ``slim_prune_mini.npz`` + ``slim_prune_mini.cfg`` - the reference's unmodified ``slim_prune.py --percent 0.5`` on the mini cfg with the
  spread-gamma seeding of tests/test_reference_scripts.py: the compact cfg text, every tensor of the compact state, the global
  threshold, and ``bias_comp_bound``: the largest difference between the reference's fp32 compensated tensors (running_mean of conv +
  BN blocks, bias of convs without BN) and an fp64 evaluation of the same fold on the same operands (tools/slim_prune.py on the
  model cast to float64).
"""
import glob
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: F401,E402
import train_harness as th  # noqa: E402

ROW_LENGTHS = (1, 3, 13, 64, 65, 255, 1024)
PENALTIES = (1e-3, 0.37)


def prune_sets():
    import models
    import utils.prune_utils as pu
    cfgs = {os.path.relpath(p, os.path.join(conftest.PKG, 'cfg')): p
            for p in sorted(glob.glob(os.path.join(conftest.PKG, 'cfg', '**', '*.cfg'), recursive=True))}
    mini = th.write_cfg(th.mini_cfg_text())
    cfgs['mini'] = mini
    plain = lambda v: sorted(v) if isinstance(v, set) else sorted([k, w] for k, w in v.items()) if isinstance(v, dict) else list(v)
    out = {}
    for rel, path in cfgs.items():
        defs = models.Darknet(path).module_defs
        out[rel] = {}
        for mode, fn in ((0, pu.parse_module_defs), (1, pu.parse_module_defs2), (2, pu.parse_module_defs4)):
            try:
                out[rel][str(mode)] = {'returns': [plain(v) for v in fn(defs)]}
            except Exception as e:
                out[rel][str(mode)] = {'raises': type(e).__name__}
    os.unlink(mini)
    path = os.path.join(HERE, 'prune_sets.json')
    json.dump(out, open(path, 'w'), indent=0, sort_keys=True)
    print('wrote', path, os.path.getsize(path), 'bytes')


def bn_l1():
    import utils.prune_utils as pu
    g = torch.Generator().manual_seed(7)
    special = torch.tensor([0.0, -0.0, -1.5, float('nan'), 1e-40, -1e-40, 2.0, -3e-3])
    out = {'s': np.array(PENALTIES, dtype=np.float64)}
    for k, n in enumerate(ROW_LENGTHS):
        gamma = torch.randn(n, generator=g)
        gamma[torch.arange(n) % 5 == 1] *= -1
        m = min(n, special.numel())
        gamma[:m] = special[(torch.arange(m) + k) % special.numel()]
        grad = torch.randn(n, generator=g) * 0.01
        grad[torch.arange(n) % 7 == 3] = 0.0
        out['gamma_%d' % k], out['grad_%d' % k] = gamma.numpy().copy(), grad.numpy().copy()
        for j, s in enumerate(PENALTIES):
            w = torch.nn.Parameter(gamma.clone())
            w.grad = grad.clone()
            pu.BNOptimizer.updateBN(True, [[None, types.SimpleNamespace(weight=w)]], s, [0])
            out['out%d_%d' % (j, k)] = w.grad.numpy().copy()
    path = os.path.join(HERE, 'bn_l1.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


def _dataset(root):
    """Four small images with one box each: slim_prune.py evaluates the model before and after."""
    from PIL import Image
    rng = np.random.RandomState(0)
    os.makedirs(os.path.join(root, 'images'))
    os.makedirs(os.path.join(root, 'labels'))
    files = []
    for i in range(4):
        p = os.path.join(root, 'images', 'im_%d.png' % i)
        Image.fromarray((rng.rand(80, 96, 3) * 255).astype(np.uint8)).save(p)
        open(os.path.join(root, 'labels', 'im_%d.txt' % i), 'w').write('%d 0.5 0.5 0.3 0.4\n' % (i % 2))
        files.append(p)
    open(os.path.join(root, 'valid.txt'), 'w').write('\n'.join(files) + '\n')
    open(os.path.join(root, 'synth.names'), 'w').write('wide\ntall\n')
    data = os.path.join(root, 'synth.data')
    open(data, 'w').write('classes=2\ntrain=%s\nvalid=%s\nnames=%s\n' % (os.path.join(root, 'valid.txt'), os.path.join(root, 'valid.txt'),
                                                                      os.path.join(root, 'synth.names')))
    return data


def slim_prune_mini():
    import pathlib
    import models
    import test_reference_scripts as trs
    import utils.prune_utils as pu
    sys.path.insert(0, os.path.join(conftest.PKG, 'tools'))
    import slim_prune as native
    work = pathlib.Path(tempfile.mkdtemp())
    mini = th.write_cfg(th.mini_cfg_text())
    model, cfg, wfile = trs._prepare(work, mini, seed=0)
    os.unlink(mini)
    data = _dataset(str(work / 'data'))
    out = trs._run('slim_prune.py', ['--cfg', cfg, '--data', data, '--weights', wfile, '--percent', '0.5', '--img-size', '64',
                                     '--batch-size', '4'], work)
    assert 'Compact model has been saved' in out
    cfg_out, = glob.glob(str(work / 'cfg' / '**' / '*slim_prune_0.5*.cfg'), recursive=True)
    w_out, = glob.glob(str(work / 'weights' / '**' / '*slim_prune_0.5*.weights'), recursive=True)
    text = open(cfg_out).read()
    open(os.path.join(HERE, 'slim_prune_mini.cfg'), 'w').write(text)
    compact = models.Darknet(cfg_out, (64, 64))
    models.load_darknet_weights(compact, w_out)
    state = {k: v.numpy().copy() for k, v in compact.state_dict().items() if 'num_batches_tracked' not in k}
    # the threshold the reference used (slim_prune.py:106-113)
    loaded = models.Darknet(str(work / cfg), (64, 64))
    models.load_darknet_weights(loaded, str(work / wfile))
    prune_idx = pu.parse_module_defs2(loaded.module_defs)[2]
    ranked = torch.sort(pu.gather_bn_weights(loaded.module_list, prune_idx))[0]
    thresh = float(ranked[int(len(ranked) * 0.5)])
    # fp64 evaluation of the fold on the same operands
    exact = native.slim_prune(loaded.double(), 0.5, 0.01, 64)['model'].state_dict()
    bound = 0.0
    for k, v in state.items():
        assert tuple(exact[k].shape) == v.shape, k
        comp = k.endswith('running_mean') or k.endswith('Conv2d.bias')
        d = float((exact[k] - torch.from_numpy(v).double()).abs().max())
        if comp:
            bound = max(bound, d)
        else:
            assert d == 0.0, (k, d)
    path = os.path.join(HERE, 'slim_prune_mini.npz')
    np.savez_compressed(path, threshold=np.float64(thresh), bias_comp_bound=np.float64(bound),
                        **{'state/' + k: v for k, v in state.items()})
    print('wrote', path, os.path.getsize(path), 'bytes; threshold %.6f, bias_comp_bound %.3e' % (thresh, bound))


if __name__ == '__main__':
    which = sys.argv[1:] or ['sets', 'l1', 'mini']
    if 'sets' in which:
        prune_sets()
    if 'l1' in which:
        bn_l1()
    if 'mini' in which:
        slim_prune_mini()
