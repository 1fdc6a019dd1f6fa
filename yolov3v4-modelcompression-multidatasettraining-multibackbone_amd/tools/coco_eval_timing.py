"""Time of COCO scoring (test.py --coco-metrics, after the detections exist): the host statement against the device path.

    python tools/coco_eval_timing.py [--out profiles/coco_eval_timing.txt] [--repeats 3]

Inputs (synthetic, fixed seed, the same arrays for both forms), sized like COCO val2017: IMAGES = 5000 images, NC = 80 categories, a
Poisson(GTS = 7) number of ground truths per image in 1-4 of the categories (5 % crowd, boxes of every size class), DETS = 100
detections per image: COPY_SHARE = 40 % of them ground-truth boxes with a jitter of up to +-JITTER = 6 pixels and the ground truth's
category, the rest random boxes in the image's categories or (one in five) any category; scores rounded to 5 decimals like results.json.
  host statement   utils/cocoeval.py evaluate: numpy, the loops of the protocol (what a CPU run and YOLO_HIP_COCO_EVAL=0 take)
  device path      engine/cocoeval.py evaluate_device: one upload, torch.sort ordering, yh_coco_match, yh_coco_accumulate, one read
Synchronised wall clock around each form; one untimed device round (library load, allocator), then --repeats rounds that alternate
the two; medians with the spread, and that both forms gave the same bits.  The baseline is the host statement of this same commit:
pycocotools is not available to this project, so there is no pycocotools number.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

IMAGES, NC, GTS, DETS, COPY_SHARE, JITTER, W, H = 5000, 80, 7, 100, 0.4, 6.0, 640.0, 480.0


def make_set():
    rng = np.random.RandomState(0)
    dets, gts = [], []
    for i in range(IMAGES):
        cats = rng.choice(NC, rng.randint(1, 5), replace=False)
        n = rng.poisson(GTS)
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (n, 2)))
        wh[:, 1] = np.minimum(wh[:, 1], H)
        xy = rng.uniform(0, 1, (n, 2)) * (np.array([W, H]) - wh)
        gcat = rng.choice(cats, n)
        gts.append(np.concatenate([np.full((n, 1), i), gcat[:, None], xy, wh, (wh[:, 0] * wh[:, 1])[:, None], (rng.rand(n) < 0.05)[:, None]], 1))
        dwh = np.exp(rng.uniform(np.log(8), np.log(300), (DETS, 2)))
        dxy = rng.uniform(-0.02, 1, (DETS, 2)) * np.array([W, H])
        dcat = np.where(rng.rand(DETS) < 0.2, rng.randint(0, NC, DETS), rng.choice(cats, DETS))
        for p in (np.nonzero(rng.rand(DETS) < COPY_SHARE)[0] if n else ()):
            t = rng.randint(n)
            dxy[p], dwh[p], dcat[p] = xy[t] + rng.uniform(-JITTER, JITTER, 2), np.maximum(wh[t] + rng.uniform(-JITTER, JITTER, 2), 1), gcat[t]
        score = np.round(rng.uniform(0.001, 1, DETS) ** 2, 5)
        dets.append(np.concatenate([np.full((DETS, 1), i), dcat[:, None], np.round(dxy, 3), np.round(dwh, 3), score[:, None]], 1))
    return np.concatenate(dets).astype(np.float64), np.concatenate(gts).astype(np.float64)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'coco_eval_timing.txt'))
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    from engine import cocoeval as engine
    from utils import cocoeval as host
    dets, gts = make_set()
    dev = torch.device('cuda', 0)
    forms = {'host': lambda: host.evaluate(dets, gts, IMAGES, NC), 'device': lambda: engine.evaluate_device(dets, gts, IMAGES, NC, dev)}
    timed(forms['device'])
    sec = {'host': [], 'device': []}
    res = {}
    for r in range(args.repeats):
        for name in ('host', 'device'):
            t, res[name] = timed(forms[name])
            sec[name].append(t)
            print('round %d %-6s %.3f s' % (r, name, t), flush=True)
    same = all(res['host'][k].tobytes() == res['device'][k].tobytes() for k in ('precision', 'recall', 'stats'))
    mh, md = statistics.median(sec['host']), statistics.median(sec['device'])
    last = engine.LAST
    lines = [
        'COCO scoring (test.py --coco-metrics): host statement (utils/cocoeval.py) against the device path (engine/cocoeval.py, csrc/cocoeval.hip)',
        'tools/coco_eval_timing.py on %s (%s); torch %s' % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.__version__),
        'inputs: %d images, %d categories, %d ground truths (Poisson %d per image, 5 %% crowd), %d detections (%d per image, %.0f %% of them '
        'ground-truth boxes with +-%.0f px jitter); %d (image, category) pairs, %d detections within the first 100 of their pair'
        % (IMAGES, NC, len(gts), GTS, len(dets), DETS, 100 * COPY_SHARE, JITTER, last['pairs'], last['slots']),
        'synchronised wall clock, one untimed device round, median of %d alternating repeats' % args.repeats,
        'baseline: the host statement of this same commit (numpy, loops in the shape of the protocol); no pycocotools number exists here',
        '',
        'host statement (YOLO_HIP_COCO_EVAL=0)      %10.3f s    (min %.3f, max %.3f)' % (mh, min(sec['host']), max(sec['host'])),
        'device path (yh_coco_match + _accumulate)  %10.3f s    (min %.3f, max %.3f)' % (md, min(sec['device']), max(sec['device'])),
        'host statement / device path               %10.1f x;   precision, recall and stats of the two forms %s' % (mh / md, 'IDENTICAL (bit for bit)' if same else 'DIFFER'),
        '',
        'device path per call: %d HIP launches (matcher: one workgroup per pair; accumulation: one per category x 4 ranges x 3 maxDets x 10 '
        'thresholds) plus the torch ordering (6 stable sorts, unique, searchsorted, gathers)' % last['hip_launches'],
        'host to device  %10d bytes in one copy (detections, ground truth, iouThrs, recThrs, area ranges)' % last['bytes_to_device'],
        'device to host  %10d bytes in one copy (precision 10 x 101 x %d x 4 x 3 and recall 10 x %d x 4 x 3, fp64)' % (last['bytes_to_host'], NC, NC),
        'workspace       %10d bytes (8 per ground truth: the matched bits); pr is never stored' % last['workspace_bytes'],
        '',
        'AP@[.5:.95] %.4f  AP50 %.4f  AP75 %.4f  AR@100 %.4f (synthetic boxes: the numbers only show that the set is not degenerate)'
        % (res['device']['stats'][0], res['device']['stats'][1], res['device']['stats'][2], res['device']['stats'][8]),
    ]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
