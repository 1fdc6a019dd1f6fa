"""Device-resident frame cache, CPU tier: ``LoadImagesAndLabels(device_cache=True)`` items are geometry alone, consume the random
streams exactly like ``mosaic_item`` and, rendered from a host arena through the emulated ``yh_mosaic_affine_hsv_batch``, equal the
host loader's items bit for bit; the cache holds exactly ``load_image``'s frames; the refusals; the entry point's host validation."""
import ctypes as C
import os
import pickle
import random
import re

import numpy as np
import pytest
import torch

import conftest  # noqa: F401
from engine import framecache, hiplib
from engine import preprocess as pp
from fakelib_framecache import FakeLibFrameCache
from test_augment import HYPS
from utils import datasets

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(96, False), (64, False), (128, True)]


def _trio(dataset_dir, size, hyp, gray=False):
    kw = dict(img_size=size, batch_size=4, augment=True, hyp=hyp, rect=False, is_gray_scale=gray)
    path = str(dataset_dir / 'train.txt')
    host = datasets.LoadImagesAndLabels(path, **kw)
    dev = datasets.LoadImagesAndLabels(path, device_augment=True, **kw)
    cached = datasets.LoadImagesAndLabels(path, device_augment=True, device_cache=True, **kw)
    assert cached.device_cache and cached.device_augment and cached.mosaic
    return host, dev, cached


def _item(ds, index, seed):
    random.seed(seed)
    np.random.seed(seed)
    item = ds[index]
    return item, (random.random(), np.random.rand())


def _render(items, cache, dtype=torch.uint8):
    batch = datasets.LoadImagesAndLabels.collate_fn(items)[0]
    assert isinstance(batch, datasets.CachedMosaicBatch)
    return pp.render_cached_mosaic_batch(batch, cache, dtype=dtype, lib=FakeLibFrameCache())


@pytest.mark.parametrize('hyp', HYPS, ids=['crop', 'train_hyp', 'wild'])
@pytest.mark.parametrize('size,gray', SIZES)
def test_cached_recipe_equals_the_recipe_and_the_host_loader(dataset_dir, hyp, size, gray, monkeypatch):
    host, dev, cached = _trio(dataset_dir, size, hyp, gray)
    cache = framecache.DeviceFrameCache.build(cached, 'cpu')
    # from here on the cached path may not open an image: the items come from the size tables alone
    opened = []
    real_open = datasets.Image.open
    monkeypatch.setattr(datasets.Image, 'open', lambda *a, **k: (opened.append(a), real_open(*a, **k))[1])
    want, items, empties, flips = [], [], [], []
    for seed in range(8):
        index = seed % len(host)
        before = len(opened)
        item, tail_c = _item(cached, index, seed)
        assert len(opened) == before, 'the cached item opened an image'
        (img, labels, path, _), tail_h = _item(host, index, seed)
        recipe, tail_d = _item(dev, index, seed)
        assert isinstance(item, datasets.CachedMosaicItem)
        assert tail_c == tail_h == tail_d, 'the cached path consumed the random streams differently'
        assert item.path == path == recipe.path and torch.equal(item.labels, labels) and torch.equal(item.labels, recipe.labels)
        assert item.flip == recipe.flip and np.array_equal(item.inv, recipe.inv)
        assert [p[0] < 0 for p in item.parts] == [p[0] is None for p in recipe.parts]
        empties.append(sum(p[0] < 0 for p in item.parts))
        flips.append(bool(item.flip))
        want.append(img)
        items.append(item)
    if hyp is HYPS[2]:      # the seed set covers a part the warp cannot touch and the flip
        assert empties[2] == empties[7] == 2 and [s for s in range(8) if flips[s]] == [2, 6, 7], (empties, flips)
    got = _render(items, cache)
    assert torch.equal(got, torch.stack(want))


def test_cache_layout_and_the_memory_check(dataset_dir, monkeypatch):
    for size, gray in ((96, False), (200, False), (128, True)):       # 200: every frame is enlarged
        ds = datasets.LoadImagesAndLabels(str(dataset_dir / 'train.txt'), img_size=size, batch_size=4, augment=True, hyp=HYPS[1],
                                          device_augment=True, device_cache=True, is_gray_scale=gray)
        c = 1 if gray else 3
        predicted = framecache.plan_arena(ds.frame_hw, c)[1]
        cache = framecache.DeviceFrameCache.build(ds, 'cpu')
        assert len(cache) == len(ds) == 8 and cache.nbytes == predicted and cache.arena.numel() == predicted
        assert cache.offsets.dtype == np.int64 and (cache.offsets % 16 == 0).all() and (np.diff(cache.offsets) > 0).all()
        for i in range(len(ds)):
            img, hw0, hw = datasets.load_image(ds, i, gray)
            assert tuple(cache.hw[i]) == tuple(hw) and tuple(cache.hw0[i]) == tuple(hw0)
            assert np.array_equal(cache.frame(i).numpy(), img)
    # a device with too little free memory: refused with both numbers, before anything is allocated
    monkeypatch.setattr(framecache, 'free_memory', lambda device: predicted - 1)
    monkeypatch.setattr(framecache, 'allocate_arena', lambda *a: pytest.fail('allocated before the check'))
    with pytest.raises(RuntimeError) as e:
        framecache.DeviceFrameCache.build(ds, 'cpu')
    assert str(predicted) in str(e.value) and str(predicted - 1) in str(e.value)


def test_collate_of_cached_items(dataset_dir):
    host, dev, cached = _trio(dataset_dir, 64, HYPS[1])
    random.seed(3)
    np.random.seed(3)
    raw = [cached[i] for i in range(3)]
    batch, labels, paths, shapes = datasets.LoadImagesAndLabels.collate_fn(raw)
    random.seed(3)
    np.random.seed(3)
    imgs_h, labels_h, paths_h, _ = datasets.LoadImagesAndLabels.collate_fn([host[i] for i in range(3)])
    assert torch.equal(labels, labels_h) and paths == paths_h and len(batch) == 3 and shapes == (None,) * 3
    blob = pickle.dumps(batch)
    assert len(blob) < 3 * 4096, len(blob)
    clone = pickle.loads(blob)
    assert clone.pin_memory() is clone
    cache = framecache.DeviceFrameCache.build(cached, 'cpu')
    got = pp.render_cached_mosaic_batch(clone, cache, dtype=torch.uint8, lib=FakeLibFrameCache())
    assert torch.equal(got, imgs_h)
    # nothing large hangs on the dataset that the loader workers pickle
    assert len(pickle.dumps(cached)) < len(pickle.dumps(dev)) + 4096


def test_refusals(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    path = str(dataset_dir / 'train.txt')
    kw = dict(img_size=64, batch_size=4, augment=True, hyp=HYPS[1])
    for bad in (dict(device_augment=False), dict(device_augment=True, rect=True), dict(device_augment=True, arith='cv2'),
                dict(device_augment=True, cache_images=True), dict(device_augment=True, augment=False),
                dict(device_augment=True, augment=False, rect=True, device_letterbox=True)):
        with pytest.raises(NotImplementedError):
            datasets.LoadImagesAndLabels(path, device_cache=True, **{**kw, **bad})
    # the refusal that was there before stays as it was
    with pytest.raises(NotImplementedError):
        datasets.LoadImagesAndLabels(path, device_augment=True, arith='cv2', cache_images=True, **kw)
    import train as train_mod
    base = ['--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'), '--device-cache']
    assert train_mod.parse_args(base).device_cache and not train_mod.parse_args(base[:-1]).device_cache
    for extra in (['--cache-images'], ['--host-augment'], ['--rect'], ['--image-arith', 'cv2']):
        with pytest.raises(SystemExit):
            train_mod.parse_args(base + extra)
    assert train_mod.parse_args(base + ['--image-arith', 'pillow']).image_arith == 'pillow'
    monkeypatch.chdir(tmp_path)
    opt = train_mod.parse_args(base + ['--epochs', '1', '--batch-size', '4', '--img-size', '64', '64', '64', '--device', 'cpu', '--nosave'])
    opt.local_rank = -1
    with pytest.raises(NotImplementedError):
        train_mod.train(opt, train_mod.hyp)


def _desc(dst, **kw):
    d = hiplib.MosaicDesc(dst=dst, canvas_h=64, canvas_w=64, out_h=32, out_w=32, c=3, pad_value=114, out_dtype=0, divisor=256.0, arith=0)
    d.inv[0] = d.inv[4] = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_point_and_its_host_validation():
    header = open(os.path.join(REPO, 'include', 'yolo_hip.h')).read()
    assert re.search(r'#define\s+YH_ABI_VERSION\s+2\b', header) and hiplib.ABI_VERSION == 2
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'int\s+yh_mosaic_affine_hsv_batch\s*\(\s*const\s+yh_mosaic_desc\s*\*\s*host_descs\s*,\s*const\s+yh_mosaic_desc\s*\*'
                     r'\s*dev_descs\s*,\s*int\s+n\s*,\s*void\s*\*\s*stream\s*\)\s*;', code)
    assert hiplib._SIGNATURES['yh_mosaic_affine_hsv_batch'] == (C.c_int, [C.POINTER(hiplib.MosaicDesc), C.c_void_p, C.c_int, C.c_void_p])
    assert 'yh_mosaic_affine_hsv_batch' in hiplib.EXPORTS
    lib = hiplib.load()
    assert hasattr(lib, 'yh_mosaic_affine_hsv_batch') and lib.yh_abi_version() == 2
    # every refusal below is decided by host code before anything is launched: it runs without a GPU.  4096: an aligned non-null
    # address nothing reads
    for fake in (lib, FakeLibFrameCache()):
        call = fake.yh_mosaic_affine_hsv_batch
        good = (hiplib.MosaicDesc * 2)(_desc(4096), _desc(8192))
        assert call(good, 4096, 0, None) != 0                      # n = 0
        assert call(good, 4096, -1, None) != 0
        assert call(None, 4096, 2, None) != 0                      # a null table, host or device
        assert call(good, None, 2, None) != 0
        for field, value in (('out_w', 31), ('out_h', 31), ('c', 1), ('out_dtype', 1), ('divisor', 255.0)):
            assert call((hiplib.MosaicDesc * 2)(_desc(4096), _desc(8192, **{field: value})), 4096, 2, None) != 0, field
        assert call((hiplib.MosaicDesc * 2)(_desc(4096), _desc(8192, arith=1)), 4096, 2, None) != 0     # cv2 arithmetic
        assert call((hiplib.MosaicDesc * 2)(_desc(4096, arith=1), _desc(8192, arith=1)), 4096, 2, None) != 0
        assert call((hiplib.MosaicDesc * 2)(_desc(4096), _desc(None)), 4096, 2, None) != 0              # the single entry's rules
        assert call((hiplib.MosaicDesc * 2)(_desc(4096), _desc(8192, x2a=(C.c_int32 * 4)(8, 0, 0, 0), y2a=(C.c_int32 * 4)(8, 0, 0, 0))),
                    4096, 2, None) != 0                            # a non-empty part without a frame


def test_loader_with_the_cache_equals_the_recipe_loader(dataset_dir):
    from torch.utils.data import DataLoader
    host, dev, cached = _trio(dataset_dir, 64, HYPS[1])
    cache = framecache.DeviceFrameCache.build(cached, 'cpu')
    lib = FakeLibFrameCache()
    out = []
    for ds in (dev, cached):
        random.seed(11)
        np.random.seed(11)
        torch.manual_seed(11)
        batches = []
        for imgs, labels, paths, _ in DataLoader(ds, batch_size=4, num_workers=0, shuffle=True, collate_fn=ds.collate_fn):
            if isinstance(imgs, datasets.CachedMosaicBatch):
                u8 = pp.render_cached_mosaic_batch(imgs, cache, dtype=torch.uint8, lib=lib)
            else:
                u8 = torch.from_numpy(np.stack([pp.mosaic_reference(_with_crops(it, imgs)) for it in imgs.items]))
            batches.append((u8, labels, paths))
        out.append(batches)
    assert len(out[0]) == len(out[1]) == 2
    for (a, la, pa), (b, lb, pb) in zip(*out):
        assert pa == pb and torch.equal(la, lb) and a.dtype == b.dtype == torch.uint8 and torch.equal(a, b)
    assert [c for c in lib.calls if c[0] == 'yh_mosaic_affine_hsv_batch'] == [('yh_mosaic_affine_hsv_batch', 4)] * 2


def _with_crops(item, batch):
    """An item of a collated ``MosaicBatch`` with its crops put back (views of the blob), as ``mosaic_reference`` reads it."""
    k0 = sum(len(it.parts) for it in batch.items[:batch.items.index(item)])
    clone = datasets.MosaicItem()
    for name in ('canvas', 'out_hw', 'inv', 'hsv_gains', 'flip', 'channels'):
        setattr(clone, name, getattr(item, name))
    clone.parts = []
    for j, (shape, rect, corner) in enumerate(item.parts):
        crop = None
        if shape is not None:
            o = int(batch.offsets[k0 + j])
            crop = batch.blob.numpy()[o:o + shape[0] * shape[1] * item.channels].reshape(shape[0], shape[1], item.channels)
        clone.parts.append((crop, rect, corner))
    return clone
