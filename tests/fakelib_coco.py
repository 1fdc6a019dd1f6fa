"""Host emulation of ``yh_coco_workspace`` / ``yh_coco_match`` / ``yh_coco_accumulate`` (csrc/cocoeval.hip) on top of ``fakelib.FakeLib``
— TEST INFRASTRUCTURE ONLY.

Reads the descriptors and every table at their raw host addresses, like the kernels do on the device, and evaluates the steps the
header documents (include/yolo_hip.h) in the kernels' own formulation: per detection and threshold ONE winner by the order (not ignored,
IoU, latest index) instead of the serial walk, and the accumulation from integer counts with the lower bounds taken per element.  All
arithmetic is numpy float64, one rounding per operation.  It does not call utils/cocoeval.py: the tests compare the two.
"""
import ctypes as C

import numpy as np

import fakelib
from engine.hiplib import CocoAccumDesc, CocoMatchDesc

F = np.float64
T, R, A = 10, 101, 4
MAX_DETS = (1, 10, 100)


def _desc(dref, cls):
    d = dref._obj if hasattr(dref, '_obj') else dref
    assert isinstance(d, cls)
    return d


class FakeLibCoco(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.coco_calls = []      # ('match', pairs, dets, gts) / ('accumulate', K, dets, gts) of every call that would launch

    def yh_coco_workspace(self, n_dets, n_gts):
        return -1 if n_dets < 0 or n_gts < 0 else 8 * n_gts

    def yh_coco_match(self, dref, stream):
        if dref is None:
            return -1
        d = _desc(dref, CocoMatchDesc)
        if d.n_pairs < 0 or d.n_dets < 0 or d.n_gts < 0:
            return -1
        if d.n_pairs == 0:
            return 0
        if not (d.pairs and d.iou_thrs and d.area_rng) or (d.n_dets > 0 and not (d.dets and d.dt_matched and d.dt_ignore)):
            return -1
        if (d.n_gts > 0 and not (d.gts and d.gt_ignore and d.ws)) or d.ws_bytes < 8 * d.n_gts:
            return -1
        if any((p or 0) & 7 for p in (d.dets, d.gts, d.iou_thrs, d.area_rng)) or d.pairs & 3:
            return -2
        if any((p or 0) & 1 for p in (d.dt_matched, d.dt_ignore, d.ws)):
            return -2
        self.coco_calls.append(('match', int(d.n_pairs), int(d.n_dets), int(d.n_gts)))
        nd, ng = d.n_dets, d.n_gts
        dets = fakelib.flat(d.dets, nd * 4, F).reshape(nd, 4) if nd else np.zeros((0, 4), F)
        gts = fakelib.flat(d.gts, ng * 6, F).reshape(ng, 6) if ng else np.zeros((0, 6), F)
        pairs = fakelib.flat(d.pairs, d.n_pairs * 4, np.int32).reshape(d.n_pairs, 4)
        thr = np.minimum(fakelib.flat(d.iou_thrs, T, F), F(1) - F(1e-10))
        rng = fakelib.flat(d.area_rng, 2 * A, F).reshape(A, 2)
        dtm = fakelib.flat(d.dt_matched, A * nd, np.uint16).reshape(A, nd) if nd else np.zeros((A, 0), np.uint16)
        dti = fakelib.flat(d.dt_ignore, A * nd, np.uint16).reshape(A, nd) if nd else np.zeros((A, 0), np.uint16)
        gig = fakelib.flat(d.gt_ignore, A * ng, np.uint8).reshape(A, ng) if ng else np.zeros((A, 0), np.uint8)
        for d0, D, g0, G in pairs.tolist():
            if d0 < 0 or D < 0 or g0 < 0 or G < 0 or d0 + D > nd or g0 + G > ng:
                continue
            g = gts[g0:g0 + G]
            crowd = g[:, 5] != 0
            for a in range(A):
                lo, hi = rng[a]
                ig = crowd | (g[:, 4] < lo) | (g[:, 4] > hi)
                gig[a, g0:g0 + G] = ig
                matched = np.zeros((T, G), bool)
                for di in range(D):
                    dx, dy, dw, dh = dets[d0 + di]
                    da = dw * dh
                    w = np.minimum(dx + dw, g[:, 0] + g[:, 2]) - np.maximum(dx, g[:, 0])
                    h = np.minimum(dy + dh, g[:, 1] + g[:, 3]) - np.maximum(dy, g[:, 1])
                    i = w * h
                    with np.errstate(invalid='ignore', divide='ignore'):
                        iou = np.where((w > 0) & (h > 0), i / np.where(crowd, da, (da + g[:, 2] * g[:, 3]) - i), F(0))
                    dm = dg = 0
                    for t in range(T if (iou >= thr[0]).any() else 0):
                        cand = np.flatnonzero((crowd | ~matched[t]) & (iou >= thr[t]))
                        if not len(cand):
                            continue
                        # not ignored first, then the largest IoU, then the latest index
                        win = max(cand.tolist(), key=lambda j: (not ig[j], iou[j], j))
                        dm |= 1 << t
                        dg |= int(ig[win]) << t
                        matched[t, win] = True
                    if da < lo or da > hi:
                        dg |= ~dm & 0x3ff
                    dtm[a, d0 + di], dti[a, d0 + di] = dm, dg
        return 0

    def yh_coco_accumulate(self, dref, stream):
        if dref is None:
            return -1
        d = _desc(dref, CocoAccumDesc)
        if d.n_dets < 0 or d.n_gts < 0 or not 1 <= d.K <= 65535:
            return -1
        if not (d.cat_first and d.gt_first and d.rec_thrs and d.precision and d.recall):
            return -1
        if (d.n_dets > 0 and not (d.cat_dets and d.det_rank and d.dt_matched and d.dt_ignore)) or (d.n_gts > 0 and not (d.cat_gts and d.gt_ignore)):
            return -1
        if any((p or 0) & 7 for p in (d.rec_thrs, d.precision, d.recall)) or any((p or 0) & 3 for p in (d.cat_dets, d.cat_first, d.cat_gts, d.gt_first)):
            return -2
        if any((p or 0) & 1 for p in (d.dt_matched, d.dt_ignore)):
            return -2
        self.coco_calls.append(('accumulate', int(d.K), int(d.n_dets), int(d.n_gts)))
        nd, ng, K = d.n_dets, d.n_gts, d.K
        cat_dets = fakelib.flat(d.cat_dets, nd, np.int32) if nd else np.zeros(0, np.int32)
        cat_gts = fakelib.flat(d.cat_gts, ng, np.int32) if ng else np.zeros(0, np.int32)
        cat_first = fakelib.flat(d.cat_first, K + 1, np.int32)
        gt_first = fakelib.flat(d.gt_first, K + 1, np.int32)
        rank = fakelib.flat(d.det_rank, nd, np.uint8) if nd else np.zeros(0, np.uint8)
        dtm = fakelib.flat(d.dt_matched, A * nd, np.uint16).reshape(A, nd) if nd else np.zeros((A, 0), np.uint16)
        dti = fakelib.flat(d.dt_ignore, A * nd, np.uint16).reshape(A, nd) if nd else np.zeros((A, 0), np.uint16)
        gig = fakelib.flat(d.gt_ignore, A * ng, np.uint8).reshape(A, ng) if ng else np.zeros((A, 0), np.uint8)
        rec = fakelib.flat(d.rec_thrs, R, F)
        precision = fakelib.flat(d.precision, T * R * K * A * 3, F).reshape(T, R, K, A, 3)
        recall = fakelib.flat(d.recall, T * K * A * 3, F).reshape(T, K, A, 3)
        eps = F(2.0) ** -52
        for k in range(K):
            slots = cat_dets[cat_first[k]:cat_first[k + 1]]
            grows = cat_gts[gt_first[k]:gt_first[k + 1]]
            for a in range(A):
                npig = int(np.count_nonzero(gig[a, grows] == 0))
                if npig == 0:
                    precision[:, :, k, a, :] = -1
                    recall[:, k, a, :] = -1
                    continue
                for mi, md in enumerate(MAX_DETS):
                    live = rank[slots] < md
                    for t in range(T):
                        m = ((dtm[a, slots] >> t) & 1).astype(bool)
                        ig = ((dti[a, slots] >> t) & 1).astype(bool)
                        tp = np.cumsum(live & m & ~ig)
                        fp = np.cumsum(live & ~m & ~ig)
                        n = len(slots)
                        tpf, fpf = tp.astype(F), fp.astype(F)
                        pr = tpf / ((fpf + tpf) + eps)
                        sm = np.maximum.accumulate(pr[::-1])[::-1]
                        q = np.zeros(R)
                        # element i is the first to reach the thresholds in (rc of i - 1, rc of i]: element 0 and every true positive
                        first = np.flatnonzero(np.diff(tp, prepend=-1) != 0) if n else np.zeros(0, np.int64)
                        jlo = np.searchsorted(rec, (tpf[first] - F(1)) / F(npig), side='right')
                        jhi = np.searchsorted(rec, tpf[first] / F(npig), side='right')
                        for i, lo_j, hi_j in zip(first.tolist(), jlo.tolist(), jhi.tolist()):
                            q[(0 if i == 0 else lo_j):hi_j] = sm[i]
                        precision[t, :, k, a, mi] = q
                        recall[t, k, a, mi] = (tpf[-1] if n else F(0)) / F(npig)
        return 0
