"""Device-resident frame cache, GPU tier: ``yh_mosaic_affine_hsv_batch`` reading a ``DeviceFrameCache`` against the host loader's
items (uint8, / 256 float) and against the per-item launches of the matching recipes (fp16); reuse of the pinned descriptor buffer;
``train.py --device-cache`` end to end."""
import random

import numpy as np
import pytest
import torch

import conftest  # noqa: F401
from engine import framecache
from engine import preprocess as pp
from test_augment import HYPS
from utils import datasets

TRAIN_HYP = HYPS[1]


def _trio(dataset_dir, size, hyp, gray=False):
    kw = dict(img_size=size, batch_size=4, augment=True, hyp=hyp, rect=False, is_gray_scale=gray)
    path = str(dataset_dir / 'train.txt')
    return (datasets.LoadImagesAndLabels(path, **kw), datasets.LoadImagesAndLabels(path, device_augment=True, **kw),
            datasets.LoadImagesAndLabels(path, device_augment=True, device_cache=True, **kw))


def _item(ds, index, seed):
    random.seed(seed)
    np.random.seed(seed)
    return ds[index]


def _case(trio, seeds):
    """(host items stacked, recipes, cached batch) of the seeds, index = seed % 8 as in the CPU tier."""
    host, dev, cached = trio
    want = torch.stack([_item(host, s % len(host), s)[0] for s in seeds])
    recipes = [_item(dev, s % len(dev), s) for s in seeds]
    items = [_item(cached, s % len(cached), s) for s in seeds]
    for a, b in zip(items, recipes):
        assert torch.equal(a.labels, b.labels) and a.flip == b.flip
    return want, recipes, datasets.LoadImagesAndLabels.collate_fn(items)[0]


def _check(want, recipes, batch, cache, maxabs=False):
    u8 = pp.render_cached_mosaic_batch(batch, cache, dtype=torch.uint8)
    f32 = pp.render_cached_mosaic_batch(batch, cache, dtype=torch.float32)
    f16 = pp.render_cached_mosaic_batch(batch, cache, dtype=torch.float16)
    ref16 = pp.render_mosaic_items(recipes, 'cuda', dtype=torch.float16)
    torch.cuda.synchronize()
    diff = (u8.cpu().int() - want.int()).abs()
    assert diff.max().item() == 0, 'uint8 items differ: %d pixels, worst %d' % ((diff > 0).sum().item(), diff.max().item())
    assert torch.equal(f32.cpu(), want.float() / 256.0)            # train.py: imgs.float() / 256.0 of the host items
    assert torch.equal(f16, ref16)
    if maxabs:                                                     # --maxabsscaler: applied after the render on both paths
        ref32 = pp.render_mosaic_items(recipes, 'cuda', dtype=torch.float32)
        assert torch.equal(f32 * 2 - 1, ref32 * 2 - 1) and torch.equal((f32 * 2 - 1).cpu(), (want.float() / 256.0) * 2 - 1)


@pytest.mark.gpu
@pytest.mark.parametrize('hyp', HYPS, ids=['crop', 'train_hyp', 'wild'])
@pytest.mark.parametrize('size,gray', [(96, False), (128, True)])
def test_batch_kernel_equals_the_host_loader(dataset_dir, hyp, size, gray):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    trio = _trio(dataset_dir, size, hyp, gray)
    cache = framecache.DeviceFrameCache.build(trio[2], 'cuda')
    assert cache.arena.is_cuda and cache.nbytes == framecache.plan_arena(trio[2].frame_hw, 1 if gray else 3)[1]
    for i in range(len(cache)):                                    # the staged fill put every frame where the tables say
        assert np.array_equal(cache.frame(i).cpu().numpy(), datasets.load_image(trio[2], i, gray)[0])
    for seeds in (range(8), range(3, 8), [2]):                     # batches of 8, 5 and 1; seeds 2 and 7: empty parts, 2, 6, 7: flipped
        want, recipes, batch = _case(trio, list(seeds))
        if hyp is HYPS[2] and len(batch) > 1:
            assert (batch.index < 0).any() and batch.flip.any() and not batch.flip.all()
        _check(want, recipes, batch, cache, maxabs=hyp is HYPS[2])


@pytest.mark.gpu
def test_batch_kernel_at_608(dataset_dir):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    trio = _trio(dataset_dir, 608, TRAIN_HYP)
    cache = framecache.DeviceFrameCache.build(trio[2], 'cuda')
    _check(*_case(trio, [0, 1, 2, 3]), cache)


@pytest.mark.gpu
def test_descriptor_buffer_reuse_without_synchronising(dataset_dir):
    """More batches in a row than the cache has pinned descriptor slots, no synchronise in between: a slot is rewritten on the host
    while the earlier uploads may still be queued, which the slot's event has to hold back."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    trio = _trio(dataset_dir, 96, TRAIN_HYP)
    cache = framecache.DeviceFrameCache.build(trio[2], 'cuda')
    cases = [_case(trio, seeds) for seeds in ([0, 1, 2, 3], [4, 5, 6, 7], [7, 2, 5, 0], [6, 1])]
    assert len(cases) > framecache.DESC_SLOTS
    torch.cuda.synchronize()
    outs = [pp.render_cached_mosaic_batch(batch, cache, dtype=torch.uint8) for _, _, batch in cases]
    torch.cuda.synchronize()
    for (want, _, _), got in zip(cases, outs):
        assert torch.equal(got.cpu(), want)


@pytest.mark.gpu
def test_train_with_the_device_cache(dataset_dir, tiny_cfg, tmp_path, monkeypatch, capsys):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    monkeypatch.chdir(tmp_path)
    import train as train_mod
    import test as test_mod
    opt = train_mod.parse_args(['--epochs', '2', '--batch-size', '4', '--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'),
                                '--img-size', '64', '64', '64', '-mpt', '--nosave', '--device-cache'])
    opt.local_rank = -1
    results = train_mod.train(opt, train_mod.hyp)
    assert 'Device frame cache: 8 frames' in capsys.readouterr().out
    assert len(results) == 7 and all(np.isfinite(results))
    ckpt = torch.load('weights/last.pt', map_location='cpu', weights_only=False)
    assert ckpt['epoch'] == 1
    test_mod.opt = None
    (mp, mr, m_ap, mf1, *losses), maps = test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), 'weights/last.pt', batch_size=2, imgsz=64, plot=False)
    assert 0.0 <= m_ap <= 1.0 and all(np.isfinite(losses))
