"""Detection / ground-truth sets shared by tests/test_coco_eval.py (host statement, emulated ABI) and tests/test_gpu_coco_eval.py (the
kernels).  Arrays in the layout of utils/cocoeval.py: dets (N, 7) image, category, x, y, w, h, score; gts (G, 8) image, category,
x, y, w, h, area, iscrowd.  The host statement's result of a set is computed once per process (``reference``) and shared.
"""
import functools

import numpy as np

from utils import cocoeval as host

W, H = 640.0, 480.0


def _boxes(rng, n, side=None):
    """n boxes x, y, w, h on a 0.5 grid inside the image.  ``side``: a size class per box - 0 small, 1 medium, 2 large, 3 / 4 the
    borders 32 x 32 and 96 x 96 (areas 1024 and 9216 exactly)."""
    side = rng.randint(0, 5, n) if side is None else np.asarray(side)
    lo = np.array([4, 34, 100, 32, 96])[side]
    hi = np.array([30, 90, 200, 32, 96])[side]
    w = np.round(rng.uniform(lo, hi) * 2) / 2
    h = np.where(side >= 3, w, np.clip(np.round(w * rng.uniform(0.6, 1.4, n) * 2) / 2, lo, hi))
    x = np.round(rng.uniform(0, W - w) * 2) / 2
    y = np.round(rng.uniform(0, H - h) * 2) / 2
    return np.stack([x, y, w, h], 1)


def make_pair(rng, image, cat, D, G, crowd_frac=0.1, side=None):
    """One (image, category) pair: G ground truths, D detections - jittered copies of the ground truths (so that IoUs around every
    threshold, exact duplicates and IoU ties occur) filled up with random boxes; scores on a 0.01 grid."""
    g = _boxes(rng, G, side)
    crowd = (rng.rand(G) < crowd_frac).astype(np.float64)
    # an annotation's area is not its box area: three in ten differ, still inside or on the border of some class
    area = g[:, 2] * g[:, 3] * np.where(rng.rand(G) < 0.3, rng.choice([0.5, 0.75, 1.0], G), 1.0)
    gts = np.concatenate([np.full((G, 1), float(image)), np.full((G, 1), float(cat)), g, area[:, None], crowd[:, None]], 1)
    n_copy = min(D, int(round(G * 1.5))) if G else 0
    src = g[rng.randint(0, G, n_copy)] if n_copy else np.zeros((0, 4))
    jit = np.round(rng.normal(0, 1, (n_copy, 4)) * rng.choice([0, 1, 4], (n_copy, 1)) * 2) / 2
    copies = src + jit
    copies[:, 2:] = np.maximum(copies[:, 2:], 0.5)
    d = np.concatenate([copies, _boxes(rng, D - n_copy)], 0)[rng.permutation(D)] if D else np.zeros((0, 4))
    score = np.round(rng.uniform(0.01, 1.0, D), 2)
    dets = np.concatenate([np.full((D, 1), float(image)), np.full((D, 1), float(cat)), d, score[:, None]], 1)
    return dets, gts


def _join(parts):
    dets = np.concatenate([p[0] for p in parts], 0) if parts else np.zeros((0, 7))
    gts = np.concatenate([p[1] for p in parts], 0) if parts else np.zeros((0, 8))
    return dets, gts


def generated(seed=0, images=40, K=5):
    """The mixed set: ``images`` x ``K`` pairs, 0-130 ground truths per pair (mostly few; 63 / 64 / 65 / 130 occur), 10 % crowd, every
    size class and both borders, some pairs with more than 100 detections, some pairs absent.  The rows are shuffled: the input order
    is not the evaluation order."""
    rng = np.random.RandomState(seed)
    big = {3: (120, 63), 7: (100, 64), 11: (101, 65), 19: (160, 130), 23: (300, 9), 29: (40, 100)}
    parts = []
    for n in range(images * K):
        image, cat = divmod(n, K)
        if n in big:
            D, G = big[n]
        else:
            G = int(rng.choice([0, 0, 1, 1, 2, 3, 5, 8, 13]))
            D = int(rng.choice([0, 1, 2, 4, 8, 12, 20, 30]))
        if D or G:
            parts.append(make_pair(rng, image, cat, D, G))
    dets, gts = _join(parts)
    return dets[rng.permutation(len(dets))], gts[rng.permutation(len(gts))], images, K


def directed(K):
    """The shapes at which the kernels take another path.  Pairs with D = 0, 1, 100, 101, 300 detections and G = 0, 1, 63, 64, 65, 130
    ground truths (the passes of 64 lanes); with K = 80 also category lists of 1, 255, 256, 257, 700 and 5000 detections (the
    accumulation scans chunks of 256) and a category whose ground truths are ignored in ONE area range only (area 1024: small and
    medium, so 'large' alone has none).  K = 1: everything of category 0 in one list."""
    rng = np.random.RandomState(100 + K)
    images = 50
    spec = [(0, 0, 0, 1), (1, 0, 1, 0), (2, 0, 100, 63), (3, 0, 101, 64), (4, 0, 300, 65), (5, 0, 1, 130), (6, 0, 100, 1), (7, 0, 0, 130)]
    parts = [make_pair(rng, i, c, D, G) for i, c, D, G in spec]
    if K > 1:
        assert K >= 80
        parts.append(make_pair(rng, 9, 11, 1, 1))                                         # a list of 1
        for cat, last in ((22, 55), (33, 56), (44, 57)):                                  # 255, 256, 257
            parts += [make_pair(rng, i, cat, D, 2) for i, D in ((10, 100), (20, 100), (30, last))]
        parts += [make_pair(rng, i, 55, 100, 2) for i in range(7)]                        # 700
        parts += [make_pair(rng, i, 79, 100, 3) for i in range(50)]                       # 5000
        parts += [make_pair(rng, i, 66, 6, 4, crowd_frac=0.0, side=[3] * 4) for i in (12, 13)]
        for p in parts[-2:]:
            p[1][:, 6] = 1024.0                                                           # the border: small and medium, not large
        parts.append(make_pair(rng, 14, 70, 5, 0))                                        # detections only: the category stays -1
        parts.append(make_pair(rng, 15, 71, 3, 2, crowd_frac=1.0))                        # crowd only: -1 as well
    dets, gts = _join(parts)
    return dets[rng.permutation(len(dets))], gts[rng.permutation(len(gts))], images, K


@functools.lru_cache(maxsize=None)
def reference(name):
    """(dets, gts, num_images, K, host statement's result) of a named set; computed once."""
    dets, gts, n, K = {'generated': generated, 'directed1': lambda: directed(1), 'directed80': lambda: directed(80)}[name]()
    return dets, gts, n, K, host.evaluate(dets, gts, n, K)


def same_bits(got, want):
    """precision, recall and stats equal bit for bit (every entry; -1 included)."""
    for key, shape in (('precision', want['precision'].shape), ('recall', want['recall'].shape), ('stats', (12,))):
        a, b = np.ascontiguousarray(got[key], np.float64), np.ascontiguousarray(want[key], np.float64)
        assert a.shape == b.shape == shape, key
        diff = np.flatnonzero(a.view(np.int64).ravel() != b.view(np.int64).ravel())
        assert diff.size == 0, '%s: %d of %d entries differ, first at %s: %r != %r' % (
            key, diff.size, a.size, np.unravel_index(diff[0], a.shape), a.ravel()[diff[0]], b.ravel()[diff[0]])


# ---- argument checks of yh_coco_match / yh_coco_accumulate (host code)
def valid_match_desc(**kw):
    from engine import hiplib
    base = dict(dets=4096, gts=4096, pairs=4096, iou_thrs=4096, area_rng=4096, dt_matched=4096, dt_ignore=4096, gt_ignore=4096, ws=4096,
                ws_bytes=8 * 3, n_pairs=2, n_dets=10, n_gts=3)       # any aligned non-null address: a refused call reads no memory
    base.update(kw)
    return hiplib.CocoMatchDesc(**base)


def valid_accum_desc(**kw):
    from engine import hiplib
    base = dict(cat_dets=4096, cat_first=4096, det_rank=4096, cat_gts=4096, gt_first=4096, dt_matched=4096, dt_ignore=4096, gt_ignore=4096,
                rec_thrs=4096, precision=4096, recall=4096, n_dets=10, n_gts=3, K=3)
    base.update(kw)
    return hiplib.CocoAccumDesc(**base)


MATCH_REFUSED = [({'n_pairs': -1}, -1), ({'n_dets': -1}, -1), ({'n_gts': -1}, -1), ({'pairs': None}, -1), ({'iou_thrs': None}, -1),
                 ({'area_rng': None}, -1), ({'dets': None}, -1), ({'dt_ignore': None}, -1), ({'gts': None}, -1), ({'gt_ignore': None}, -1),
                 ({'ws': None}, -1), ({'ws_bytes': 23}, -1), ({'dets': 4100}, -2), ({'gts': 4100}, -2), ({'area_rng': 4100}, -2),
                 ({'pairs': 4098}, -2), ({'dt_matched': 4097}, -2), ({'ws': 4097}, -2)]
ACCUM_REFUSED = [({'n_dets': -1}, -1), ({'n_gts': -1}, -1), ({'K': 0}, -1), ({'K': 65536}, -1), ({'cat_first': None}, -1),
                 ({'gt_first': None}, -1), ({'rec_thrs': None}, -1), ({'precision': None}, -1), ({'recall': None}, -1),
                 ({'cat_dets': None}, -1), ({'det_rank': None}, -1), ({'cat_gts': None}, -1), ({'gt_ignore': None}, -1),
                 ({'rec_thrs': 4100}, -2), ({'recall': 4100}, -2), ({'cat_dets': 4098}, -2), ({'gt_first': 4098}, -2), ({'dt_ignore': 4097}, -2)]
