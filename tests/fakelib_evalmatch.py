"""Host emulation of ``yh_eval_match`` (csrc/evalmatch.hip) on top of ``fakelib.FakeLib`` — TEST INFRASTRUCTURE ONLY.

Reads the descriptor, the per-image table, the detections, the targets and the label order at their raw host addresses, like the
kernel does on the device, and evaluates the four documented steps (include/yolo_hip.h) with numpy in fp32, one rounding per
operation: clip in place, label boxes, best same-class label per detection (first maximum), lowest-index claimant per label.
It does not call ``test._match``: the tests compare the two.
"""
import ctypes as C

import numpy as np

import fakelib
from engine.hiplib import EvalMatchDesc, EvalMatchRow

F = np.float32
FREE = 0x7fffffff


def _clamp_keep_nan(v, lo, hi):
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v).astype(F)


class FakeLibEvalMatch(fakelib.FakeLib):
    def __init__(self):
        super().__init__()
        self.match_calls = []      # (images, total, niou) of every call that would launch

    def yh_eval_match(self, dref, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        assert isinstance(d, EvalMatchDesc)
        if d.images < 0 or d.nt < 0 or d.total < 0 or not 1 <= d.niou <= 10:
            return -1
        if d.images == 0 or d.total == 0:
            return 0
        if not (d.rows and d.iouv and d.correct and d.conf_cls and d.ws) or (d.nt > 0 and not (d.targets and d.label_index)):
            return -1
        if not (d.width > 0 and d.height > 0) or d.ws_bytes < 8 * d.total + 4 * d.nt:
            return -1
        if d.rows & 7:
            return -2
        if any((p or 0) & 3 for p in (d.targets, d.label_index, d.iouv, d.conf_cls, d.ws)):
            return -2
        self.match_calls.append((int(d.images), int(d.total), int(d.niou)))
        W, H = F(d.width), F(d.height)
        iouv = fakelib.flat(d.iouv, d.niou, F)
        correct = fakelib.flat(d.correct, d.total * d.niou, np.uint8).reshape(d.total, d.niou)
        conf_cls = fakelib.flat(d.conf_cls, d.total * 2, F).reshape(d.total, 2)
        targets = fakelib.flat(d.targets, d.nt * 6, F).reshape(d.nt, 6) if d.nt else np.zeros((0, 6), F)
        index = fakelib.flat(d.label_index, d.nt, np.int32) if d.nt else np.zeros(0, np.int32)
        for b in range(d.images):
            row = EvalMatchRow.from_address(d.rows + b * C.sizeof(EvalMatchRow))
            n, nl = row.n, row.nl
            if not row.pred or n <= 0:
                continue
            pred = fakelib.flat(row.pred, n * 6, F).reshape(n, 6)
            # 1. clip, in place
            pred[:, 0] = _clamp_keep_nan(pred[:, 0], F(0), W)
            pred[:, 1] = _clamp_keep_nan(pred[:, 1], F(0), H)
            pred[:, 2] = _clamp_keep_nan(pred[:, 2], F(0), W)
            pred[:, 3] = _clamp_keep_nan(pred[:, 3], F(0), H)
            out = slice(row.out_off, row.out_off + n)
            conf_cls[out] = pred[:, 4:6]
            correct[out] = 0
            if nl == 0:
                continue
            # 2. label boxes in pixels
            lab = targets[index[row.lab_first:row.lab_first + nl]]
            hw, hh = lab[:, 4] / F(2), lab[:, 5] / F(2)
            lx1, ly1 = (lab[:, 2] - hw) * W, (lab[:, 3] - hh) * H
            lx2, ly2 = (lab[:, 2] + hw) * W, (lab[:, 3] + hh) * H
            a2 = (lx2 - lx1) * (ly2 - ly1)
            # 3. per detection the same-class label of the largest IoU, the first one on a tie
            best_t = np.full(n, -1, np.int64)
            best_iou = np.zeros(n, F)
            with np.errstate(invalid='ignore', divide='ignore'):
                for p in range(n):
                    x1, y1, x2, y2 = pred[p, :4]
                    a1 = (x2 - x1) * (y2 - y1)
                    same = np.nonzero(lab[:, 1] == pred[p, 5])[0]
                    if not len(same):
                        continue
                    iw = np.minimum(x2, lx2[same]) - np.maximum(x1, lx1[same])
                    ih = np.minimum(y2, ly2[same]) - np.maximum(y1, ly1[same])
                    iw = np.where(iw < 0, F(0), iw)
                    ih = np.where(ih < 0, F(0), ih)
                    inter = (iw * ih).astype(F)
                    iou = (inter / ((a1 + a2[same]) - inter)).astype(F)
                    if np.isnan(iou).any():
                        best_t[p], best_iou[p] = same[0], F('nan')
                        continue
                    k = int(np.argmax(iou))          # numpy's argmax: the first maximum
                    best_t[p], best_iou[p] = same[k], iou[k]
            # 4. every label goes to its lowest-index claimant
            claim = np.full(nl, FREE, np.int64)
            for p in range(n):
                if best_t[p] >= 0 and best_iou[p] > iouv[0]:
                    claim[best_t[p]] = min(claim[best_t[p]], p)
            for p in range(n):
                if best_t[p] >= 0 and best_iou[p] > iouv[0] and claim[best_t[p]] == p:
                    correct[row.out_off + p] = best_iou[p] > iouv
        return 0
