"""COCO bbox scoring (the twelve numbers of ``COCOeval.summarize``) stated in plain numpy: the host path of ``test.py --coco-metrics``,
the oracle of the device path (engine/cocoeval.py, csrc/cocoeval.hip) and the slow leg of tools/coco_eval_timing.py.

This is a RESTATEMENT of the protocol (bbox, ``useCats = 1``, default parameters), written from its description; pycocotools is
not available to this project and nothing here was pinned against a run of it (the same standing as oracle/cv2_restated.py).

All arithmetic is IEEE float64, one operation at a time.  Boxes are ``x, y, w, h`` with the top-left corner in original-image pixels
and ``w, h >= 0``.

    dets  (N, 7) float64   image index, category index, x, y, w, h, score
    gts   (G, 8) float64   image index, category index, x, y, w, h, area, iscrowd

Image indices are ``0..num_images-1`` in ascending image-id order, category indices ``0..K-1`` in ascending category-id order
(``load_coco_json`` / ``dets_from_jdict`` map ids to indices).
"""
import json
import os

import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))     # all, small, medium, large
EPS = float(np.spacing(1))      # 2^-52
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)


def box_iou(d, g, crowd):
    """IoU of every detection row of ``d`` (D, 4) with every ground-truth row of ``g`` (G, 4): (D, G).  A crowd ground truth divides
    by the detection's own area."""
    dx, dy, dw, dh = (d[:, i:i + 1] for i in range(4))
    gx, gy, gw, gh = (g[None, :, i] for i in range(4))
    w = np.minimum(dx + dw, gx + gw) - np.maximum(dx, gx)
    h = np.minimum(dy + dh, gy + gh) - np.maximum(dy, gy)
    i = w * h
    da = dw * dh
    u = np.where(crowd[None, :], np.broadcast_to(da, i.shape), (da + gw * gh) - i)
    with np.errstate(invalid='ignore', divide='ignore'):
        iou = i / u
    return np.where((w <= 0) | (h <= 0), 0.0, iou)


def match_pair(d, g, lo, hi):
    """One (image, category) pair in one area range.  ``d`` (D, 5): x, y, w, h, score in descending score order, at most 100 rows;
    ``g`` (G, 6): x, y, w, h, area, iscrowd.  Returns ``dtm`` (T, D) bool, ``dtig`` (T, D) bool and ``gig`` (G,) bool in the order of g."""
    D, G = len(d), len(g)
    crowd_in = g[:, 5] != 0
    gig_in = crowd_in | (g[:, 4] < lo) | (g[:, 4] > hi)
    order = np.argsort(gig_in, kind='mergesort')          # non-ignored first, stable
    g, gig, crowd = g[order], gig_in[order], crowd_in[order]
    dtm = np.zeros((T, D), bool)
    dtig = np.zeros((T, D), bool)
    if D and G:
        ious = box_iou(d[:, :4], g[:, :4], crowd).tolist()
        gig_l, crowd_l = gig.tolist(), crowd.tolist()
        for ti, t in enumerate(IOU_THRS.tolist()):
            matched = [False] * G
            for di in range(D):
                best = min(t, 1 - 1e-10)
                m = -1
                row = ious[di]
                for gj in range(G):
                    if matched[gj] and not crowd_l[gj]:
                        continue
                    if m > -1 and not gig_l[m] and gig_l[gj]:
                        break
                    if row[gj] < best:
                        continue
                    best = row[gj]
                    m = gj
                if m == -1:
                    continue
                dtm[ti, di] = True
                dtig[ti, di] = gig_l[m]
                matched[m] = True
    area = d[:, 2] * d[:, 3]
    outside = (area < lo) | (area > hi)
    dtig |= ~dtm & outside[None, :]
    return dtm, dtig, gig_in


def _group(keys):
    """Rows grouped by key, stable: ``{key: row indices in input order}``."""
    order = np.argsort(keys, kind='mergesort')
    cuts = np.flatnonzero(np.diff(keys[order])) + 1
    return {int(keys[seg[0]]): seg for seg in np.split(order, cuts) if len(seg)}


def evaluate(dets, gts, num_images, K):
    """``dict(precision (T, R, K, A, M), recall (T, K, A, M), stats (12,))``; entries nothing was evaluated for are -1."""
    dets = np.asarray(dets, np.float64).reshape(-1, 7)
    gts = np.asarray(gts, np.float64).reshape(-1, 8)
    check_indices(dets, gts, num_images, K)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    dgrp = _group(dets[:, 0].astype(np.int64) * K + dets[:, 1].astype(np.int64))
    ggrp = _group(gts[:, 0].astype(np.int64) * K + gts[:, 1].astype(np.int64))
    empty = np.zeros(0, np.int64)
    # evaluate every existing pair, in (image, category) order
    per_cat = [[] for _ in range(K)]          # category -> [(scores, [(dtm, dtig, gig) per area])] in image order
    for key in sorted(set(dgrp) | set(ggrp)):
        rows = dgrp.get(key, empty)
        d = dets[rows]
        d = d[np.argsort(-d[:, 6], kind='mergesort')][:MAX_DETS[-1], 2:7]
        g = gts[ggrp.get(key, empty)][:, 2:8]
        per_cat[key % K].append((d[:, 4], [match_pair(d, g, lo, hi) for lo, hi in AREA_RNG]))
    for k in range(K):
        pairs = per_cat[k]
        if not pairs:
            continue
        for a in range(A):
            gig = np.concatenate([p[1][a][2] for p in pairs])
            npig = int(np.count_nonzero(~gig))
            if npig == 0:
                continue
            for mi, md in enumerate(MAX_DETS):
                scores = np.concatenate([p[0][:md] for p in pairs])
                inds = np.argsort(-scores, kind='mergesort')
                dtm = np.concatenate([p[1][a][0][:, :md] for p in pairs], axis=1)[:, inds]
                dtig = np.concatenate([p[1][a][1][:, :md] for p in pairs], axis=1)[:, inds]
                tp_sum = np.cumsum(dtm & ~dtig, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~dtm & ~dtig, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + EPS)
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    # pr[i-1] = max(pr[i-1], pr[i]) running from the end: the reverse running maximum (exact, max rounds nothing)
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    q = np.zeros(R)
                    pi = np.searchsorted(rc, REC_THRS, side='left')
                    ok = pi < nd
                    q[ok] = pr[pi[ok]]
                    precision[t, :, k, a, mi] = q
    return dict(precision=precision, recall=recall, stats=summarize(precision, recall))


def check_indices(dets, gts, num_images, K):
    for name, rows in (('detection', dets), ('ground-truth', gts)):
        if len(rows) and not (np.all(rows[:, 0] == np.floor(rows[:, 0])) and rows[:, 0].min() >= 0 and rows[:, 0].max() < num_images
                              and np.all(rows[:, 1] == np.floor(rows[:, 1])) and rows[:, 1].min() >= 0 and rows[:, 1].max() < K):
            raise ValueError('%s rows carry an image index outside [0, %d) or a category index outside [0, %d)' % (name, num_images, K))


def summarize(precision, recall):
    """The twelve numbers: the mean over the entries > -1 of each slice, -1 for a slice without any."""
    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    ap = lambda t, a, m: mean(precision[:, :, :, a, m] if t is None else precision[t, :, :, a, m])
    ar = lambda a, m: mean(recall[:, :, a, m])
    return np.array([ap(None, 0, 2), ap(0, 0, 2), ap(5, 0, 2), ap(None, 1, 2), ap(None, 2, 2), ap(None, 3, 2),
                     ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)])


def format_stats(stats):
    """The twelve lines in the layout of ``COCOeval.summarize``."""
    line = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
    rows = [('Average Precision', '(AP)', '0.50:0.95', 'all', 100), ('Average Precision', '(AP)', '0.50', 'all', 100),
            ('Average Precision', '(AP)', '0.75', 'all', 100), ('Average Precision', '(AP)', '0.50:0.95', 'small', 100),
            ('Average Precision', '(AP)', '0.50:0.95', 'medium', 100), ('Average Precision', '(AP)', '0.50:0.95', 'large', 100),
            ('Average Recall', '(AR)', '0.50:0.95', 'all', 1), ('Average Recall', '(AR)', '0.50:0.95', 'all', 10),
            ('Average Recall', '(AR)', '0.50:0.95', 'all', 100), ('Average Recall', '(AR)', '0.50:0.95', 'small', 100),
            ('Average Recall', '(AR)', '0.50:0.95', 'medium', 100), ('Average Recall', '(AR)', '0.50:0.95', 'large', 100)]
    return [line.format(*row, float(v)) for row, v in zip(rows, stats)]


# ------------------------------------------------------------------------------------------------ ground truth and detections
def image_id_of(path):
    """The image id ``test.py`` writes into ``results.json``: the digits after the last underscore of the file stem, else the stem."""
    stem = os.path.splitext(os.path.basename(str(path)))[0]
    tail = stem.split('_')[-1]
    return int(tail) if tail.isdigit() else stem


def load_coco_json(path, image_ids):
    """Mode (a): ground truth from a COCO annotation file, restricted to ``image_ids`` (the evaluated images, ids as ``image_id_of``
    derives them).  Returns ``(gts (G, 8) with image / category INDICES, image id list, category id list)``, both lists ascending."""
    with open(path) as f:
        js = json.load(f)
    known = {im['id'] for im in js.get('images', [])}
    wanted = sorted(set(image_ids), key=lambda v: (isinstance(v, str), v))
    missing = [i for i in wanted if i not in known]
    if missing:
        raise ValueError('%s lists no image %r (%d evaluated images are not in it)' % (path, missing[0], len(missing)))
    cat_ids = sorted(c['id'] for c in js['categories'])
    img_index = {v: i for i, v in enumerate(wanted)}
    cat_index = {v: i for i, v in enumerate(cat_ids)}
    rows = []
    for an in js.get('annotations', []):
        if an['image_id'] in img_index and an['category_id'] in cat_index:
            x, y, w, h = (float(v) for v in an['bbox'])
            rows.append((img_index[an['image_id']], cat_index[an['category_id']], x, y, w, h, float(an['area']), float(bool(an.get('iscrowd', 0)))))
    return np.asarray(rows, np.float64).reshape(-1, 8), wanted, cat_ids


def gts_from_labels(labels, shapes):
    """Mode (b): ground truth from a data set's own label files.  ``labels[i]`` is image i's (n, 5) float32 ``cls, x, y, w, h`` with
    the box normalised (centre form), ``shapes[i]`` its original ``(h0, w0)``.  Image index = data set index, category index = class,
    ``area = w * h``, nothing is a crowd."""
    rows = []
    for i, (lab, hw) in enumerate(zip(labels, shapes)):
        lab = np.asarray(lab, np.float32).reshape(-1, 5).astype(np.float64)
        h0, w0 = float(hw[0]), float(hw[1])
        w, h = lab[:, 3] * w0, lab[:, 4] * h0
        x, y = lab[:, 1] * w0 - w / 2, lab[:, 2] * h0 - h / 2
        rows.append(np.stack([np.full(len(lab), float(i)), lab[:, 0], x, y, w, h, w * h, np.zeros(len(lab))], 1))
    return np.concatenate(rows, 0) if rows else np.zeros((0, 8))


def dets_from_jdict(jdict, image_ids, cat_ids):
    """``results.json`` rows as the (N, 7) detection array: ids to indices by the two ascending lists.  A row of an image that was not
    evaluated is an error; a row of a category the ground truth does not list is left out, like a category filter would."""
    img_index = {v: i for i, v in enumerate(image_ids)}
    cat_index = {v: i for i, v in enumerate(cat_ids)}
    rows = []
    for r in jdict:
        if r['image_id'] not in img_index:
            raise ValueError('detection of image %r, which is not among the evaluated images' % (r['image_id'],))
        if r['category_id'] in cat_index:
            rows.append((img_index[r['image_id']], cat_index[r['category_id']], *r['bbox'], r['score']))
    return np.asarray(rows, np.float64).reshape(-1, 7)
