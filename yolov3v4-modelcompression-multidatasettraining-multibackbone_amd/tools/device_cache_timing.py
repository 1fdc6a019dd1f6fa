"""What `train.py --device-cache` changes in the input pipeline, measured on one GPU.

    python tools/device_cache_timing.py [--out profiles/device_cache_timing.txt] [--repeats 15]

Inputs: a seeded synthetic set of --images 512 JPEGs of 640 x 480 with one label row each (written to a temporary directory),
--size 608, --batch 64, train.py's hyp.  Three legs, every one with a warm-up first and its forms alternated inside this call:
  (a) render   the same seeded batches as recipes (MosaicBatch: pinned blob of crops -> render_mosaic_items = one upload + one launch
               per item) and as geometry (CachedMosaicBatch -> render_cached_mosaic_batch = descriptor upload + one launch): device
               time between two events on the stream and host time of the call (it returns before the kernels finish), launches
               and uploaded bytes per batch; the two outputs are compared bit for bit
  (b) loader   items/s of a DataLoader with --workers 8 feeding a loop that only renders, for the default recipes (decode + resize
               per item), --cache-images (resized frames in host memory) and --device-cache, per pass of --pass-batches batches:
               from the first batch to the last (an upper bound: what the workers prefetched before the first arrival counts) and
               from before the workers start to the last batch (a lower bound: their start-up counts); the join of the workers
               after the last batch is reported apart
  (c) cache    build time and arena bytes of the device cache, resident set size of this process after each mode's dataset was built
Medians with min - max.  Times are from this run on this machine; nothing here is a share of peak.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP = 3


def make_set(root, n, seed=0):
    from PIL import Image
    os.makedirs(os.path.join(root, 'images'))
    os.makedirs(os.path.join(root, 'labels'))
    rng = np.random.RandomState(seed)
    files = []
    for i in range(n):
        # smooth random colour fields (JPEG-friendly), one bright box: the pixel values do not matter to the timing, the sizes do
        small = rng.randint(0, 255, (15, 20, 3)).astype(np.uint8)
        img = np.asarray(Image.fromarray(small).resize((640, 480), Image.BILINEAR)).copy()
        img[180:300, 240:400] = rng.randint(150, 255, 3)
        p = os.path.join(root, 'images', 'im_%04d.jpg' % i)
        Image.fromarray(img).save(p, quality=90)
        with open(os.path.join(root, 'labels', 'im_%04d.txt' % i), 'w') as f:
            f.write('0 0.5 0.5 0.25 0.25\n')
        files.append(p)
    with open(os.path.join(root, 'train.txt'), 'w') as f:
        f.write('\n'.join(files) + '\n')
    return os.path.join(root, 'train.txt')


def rss_mb():
    with open('/proc/self/status') as f:
        for line in f:
            if line.startswith('VmRSS:'):
                return int(line.split()[1]) / 1024.0
    return float('nan')


def empty_pinned_cache():
    """Give torch's cached pinned-host blocks back.  ``torch._C._host_emptyCache`` is a private hook of the torch this tool was
    written against (2.10); where a torch lacks it nothing is emptied and the output says so."""
    hook = getattr(torch._C, '_host_emptyCache', None)
    if hook is None:
        return False
    hook()
    return True


def pinned_mb():
    """Pinned host bytes torch holds, in MB (``torch.cuda.memory.host_memory_stats``, torch 2.10; nan where it is missing)."""
    try:
        return torch.cuda.memory.host_memory_stats()['allocated_bytes.current'] / 2.0 ** 20
    except Exception:
        return float('nan')


def stats(v, unit):
    return '%9.3f %s   (min %.3f, max %.3f, %d samples)' % (statistics.median(v), unit, min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=512)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--passes', type=int, default=3, help='timed passes per loader mode (after one warm-up pass)')
    ap.add_argument('--pass-batches', type=int, default=40, help='batches of one pass')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'device_cache_timing.txt'))
    args = ap.parse_args()
    assert args.repeats >= 15 and args.passes * args.pass_batches >= 15
    import random
    import train as train_mod
    from engine import preprocess as pp
    from engine.framecache import DeviceFrameCache
    from torch.utils.data import DataLoader
    from utils.datasets import LoadImagesAndLabels
    assert torch.cuda.is_available(), 'the measurement needs a GPU'
    dev = torch.device('cuda', 0)
    hyp = dict(train_mod.hyp)
    tmp = tempfile.TemporaryDirectory()
    train_txt = make_set(tmp.name, args.images)
    kw = dict(img_size=args.size, batch_size=args.batch, augment=True, hyp=hyp, rect=False, rank=1, device_augment=True)

    # ---- (c) datasets, cache, resident set
    rss = [('before any dataset', rss_mb())]
    ds_default = LoadImagesAndLabels(train_txt, **kw)
    rss.append(('default recipes: dataset built', rss_mb()))
    ds_cached = LoadImagesAndLabels(train_txt, device_cache=True, **kw)
    cache = DeviceFrameCache.build(ds_cached, dev)
    rss.append(('--device-cache: dataset + cache built', rss_mb()))
    t0 = time.perf_counter()
    ds_host = LoadImagesAndLabels(train_txt, cache_images=True, **kw)
    host_cache_s = time.perf_counter() - t0
    rss.append(('--cache-images: dataset built', rss_mb()))
    host_cache_bytes = sum(im.nbytes for im in ds_host.imgs)

    # ---- (a) render: the same seeded batches in both forms
    def batches(ds, count=4):
        out = []
        for b in range(count):
            random.seed(100 + b)
            np.random.seed(100 + b)
            out.append(ds.collate_fn([ds[(b * args.batch + i) % len(ds)] for i in range(args.batch)])[0])
        return out
    recipes = [b.pin_memory() for b in batches(ds_host)]       # crops cut from the host cache: the --cache-images form of the recipes
    cached = batches(ds_cached)
    out = torch.empty((args.batch, 3, args.size, args.size), dtype=torch.float32, device=dev)
    forms = {'A': lambda k: pp.render_mosaic_items(recipes[k], dev, out=out), 'B': lambda k: pp.render_cached_mosaic_batch(cached[k], cache, out=out)}
    for k in range(len(cached)):                               # same values, bit for bit, at the size that is timed
        a = forms['A'](k).clone()
        assert torch.equal(a, forms['B'](k))
    dev_ms, host_ms = {'A': [], 'B': []}, {'A': [], 'B': []}
    for r in range(WARMUP + args.repeats):
        for form in ('A', 'B'):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            forms[form](r % len(cached))
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if r >= WARMUP:
                dev_ms[form].append(e0.elapsed_time(e1))
                host_ms[form].append((t1 - t0) * 1e3)
    up_a = statistics.mean(b.blob.numel() for b in recipes)
    up_b = args.batch * pp._MOSAIC_DTYPE.itemsize

    # ---- (b) loader feeding a render-only loop
    def render(imgs):
        if torch.is_tensor(imgs):
            return imgs.to(dev).float() / 256.0
        if hasattr(imgs, 'blob'):
            return pp.render_mosaic_items(imgs, dev, out=out)
        return pp.render_cached_mosaic_batch(imgs, cache, out=out)
    modes = [('default (decode + resize per item)', ds_default), ('--cache-images', ds_host), ('--device-cache', ds_cached)]
    # items drawn with replacement, so that a pass is --pass-batches long whatever the size of the set; the workers of a loader live
    # for one pass only (at most --workers processes next to this one at any time), their start-up is inside the timed pass
    loaders = [DataLoader(ds, batch_size=args.batch, num_workers=args.workers, pin_memory=True, collate_fn=ds.collate_fn,
                          sampler=torch.utils.data.RandomSampler(ds, replacement=True, num_samples=args.batch * args.pass_batches))
               for _, ds in modes]
    # a pass is clocked at three points: t0 before the workers start, the arrival (rendered and synchronised) of its first and of its
    # last batch.  What comes after the last batch - the iterator joining its workers - belongs to no rate and is reported on its own
    # The recipe modes pin a blob of crops per batch, and torch keeps freed pinned blocks; the workers of the next pass are forked
    # from a process that holds them.  That cache is emptied before every pass, so that no pass inherits what another mode pinned;
    # the pinned bytes this process still holds when the workers start are reported per mode.
    rate, steady, startup, teardown, pinned = ([[] for _ in modes] for _ in range(5))
    for p in range(1 + args.passes):
        for m, loader in enumerate(loaders):
            torch.cuda.synchronize()
            emptied = empty_pinned_cache()
            pinned[m].append(pinned_mb())
            t0 = time.perf_counter()
            n, t_first, t_last = 0, None, None
            for imgs, targets, paths, _ in loader:
                render(imgs)
                n += len(paths)
                if t_first is None or n == args.batch * args.pass_batches:
                    torch.cuda.synchronize()
                    t_last = time.perf_counter()
                    t_first = t_first or t_last
            t_end = time.perf_counter()
            assert n == args.batch * args.pass_batches
            if p >= 1:
                rate[m].append(n / (t_last - t0))
                steady[m].append((n - args.batch) / (t_last - t_first))
                startup[m].append(t_first - t0)
                teardown[m].append(t_end - t_last)
    rss.append(('after the loader passes (this process, without its workers)', rss_mb()))
    per_pass = args.pass_batches

    lines = ['Device-resident frame cache (train.py --device-cache): render, loader and cache figures',
             'tools/device_cache_timing.py on %s (%s); torch %s; %d CPUs usable' %
             (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.__version__,
              len(os.sched_getaffinity(0))),
             'inputs: %d synthetic JPEGs of 640 x 480 (seeded), img_size %d, batch %d, train.py hyp, fp32 / 256 output' %
             (args.images, args.size, args.batch), '',
             '(a) render of one batch, %d warm-up rounds, %d alternating repeats over %d seeded batches; outputs bit-identical' %
             (WARMUP, args.repeats, len(cached)),
             '  A  render_mosaic_items        (blob upload + %d launches)   device %s' % (args.batch, stats(dev_ms['A'], 'ms')),
             '                                                               host   %s' % stats(host_ms['A'], 'ms'),
             '  B  render_cached_mosaic_batch (descriptor upload + 1 launch) device %s' % stats(dev_ms['B'], 'ms'),
             '                                                               host   %s' % stats(host_ms['B'], 'ms'),
             '  per batch: A %d kernel launches, %.0f bytes uploaded (mean);  B 1 kernel launch, %d bytes uploaded' % (args.batch, up_a, up_b),
             '  device: median A - median B = %.3f ms; combined spread (max - min of A plus max - min of B) = %.3f ms' %
             (statistics.median(dev_ms['A']) - statistics.median(dev_ms['B']),
              max(dev_ms['A']) - min(dev_ms['A']) + max(dev_ms['B']) - min(dev_ms['B'])), '',
             '(b) DataLoader with %d workers (forked per pass, as train.py forks them per epoch) feeding a render-only loop; %d batches a '
             'pass, 1 warm-up pass, %d timed passes, modes alternated; one sample per pass; torch\'s cache of pinned host blocks %s '
             'before every pass' % (args.workers, per_pass, args.passes, 'emptied' if emptied else 'NOT emptied (no hook in this torch)')]
    for m, (name, _) in enumerate(modes):
        lines += ['  %s' % name,
                  '    items/s from the first batch to the last                  %s' % stats(steady[m], 'items/s'),
                  '    items/s from before the workers start to the last batch   %s' % stats(rate[m], 'items/s'),
                  '    start of the workers to the first batch                   %s' % stats(startup[m], 's'),
                  '    last batch to the end of the pass (workers joined)        %s' % stats(teardown[m], 's'),
                  '    pinned host memory held when the workers start            %s' % stats(pinned[m][1:], 'MB')]
    lines += ['', '(c) cache',
              '  device cache: %d frames, %d bytes in one arena, built in %.2f s (decode + resize on at most 16 threads, staged uploads)' %
              (len(cache), cache.nbytes, cache.build_seconds),
              '  --cache-images: %d bytes of frames in host memory of this process (and of every DDP rank), built in %.2f s on one thread' %
              (host_cache_bytes, host_cache_s),
              '  resident set of this process, in the order the modes were built (each line includes what the earlier ones left):']
    lines += ['    %-62s %9.1f MB' % row for row in rss]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    tmp.cleanup()


if __name__ == '__main__':
    main()
