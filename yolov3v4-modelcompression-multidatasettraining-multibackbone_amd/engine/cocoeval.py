"""COCO bbox scoring on the device: ``yh_coco_match`` / ``yh_coco_accumulate`` (csrc/cocoeval.hip) behind ``test.py --coco-metrics``.

The protocol and the host path are utils/cocoeval.py; its per-image, per-category, per-area-range loops are what this module moves to
the GPU.  ``evaluate`` packs detections, ground truth and the parameter tables into ONE host-to-device copy, orders them with
``torch.sort(stable=True)`` (by pair then descending score; by category then descending score with the image order as the tie-break),
launches the matcher and the accumulation, and reads ``precision`` / ``recall`` back in ONE copy (0.98 M doubles, 7.8 MB, at 80 categories).  The
twelve numbers are the host module's own ``summarize`` of those arrays, so both paths give the same bits.

There is no fallback: on a CUDA device a missing library or entry point raises (engine/hiplib.py).
"""
import ctypes as C
import os

import numpy as np
import torch

from utils import cocoeval as host

from . import hiplib
from .hiplib import CocoAccumDesc, CocoMatchDesc

_LIB_OVERRIDE = None   # tests inject the host emulation here
LAST = {}              # launches and bytes moved by the last evaluate_device call (tools/coco_eval_timing.py)


def _lib():
    return _LIB_OVERRIDE if _LIB_OVERRIDE is not None else hiplib.load()


def enabled(device):
    """The device path serves CUDA devices; ``YOLO_HIP_COCO_EVAL=0`` keeps the host statement there too, for A/B runs."""
    return device is not None and torch.device(device).type == 'cuda' and os.environ.get('YOLO_HIP_COCO_EVAL', '1') != '0'


def evaluate(dets, gts, num_images, K, device=None):
    """``dict(precision, recall, stats)`` of utils.cocoeval.evaluate: on the device when ``device`` is a GPU, by the host statement
    otherwise."""
    if enabled(device):
        return evaluate_device(dets, gts, num_images, K, device)
    return host.evaluate(dets, gts, num_images, K)


def _offsets(sorted_keys, n):
    """(n + 1,) int32 offsets of the runs of keys 0..n-1 in an ascending key list."""
    edges = torch.arange(n + 1, dtype=sorted_keys.dtype, device=sorted_keys.device)
    return torch.searchsorted(sorted_keys, edges).to(torch.int32)


def evaluate_device(dets, gts, num_images, K, device):
    dets = np.ascontiguousarray(np.asarray(dets, np.float64).reshape(-1, 7))
    gts = np.ascontiguousarray(np.asarray(gts, np.float64).reshape(-1, 8))
    host.check_indices(dets, gts, num_images, K)
    lib = _lib()
    dev = torch.device(device)
    pin = dev.type == 'cuda'
    N, G = len(dets), len(gts)
    T, R, A, M = host.T, host.R, host.A, host.M

    # one host-to-device copy: detections, ground truth, iouThrs, recThrs, area ranges
    parts = [dets.ravel(), gts.ravel(), host.IOU_THRS, host.REC_THRS, np.asarray(host.AREA_RNG, np.float64).ravel()]
    host_in = torch.from_numpy(np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]))
    if pin:
        host_in = host_in.pin_memory()
    dev_in = host_in.to(dev, non_blocking=True)
    cuts = np.cumsum([0] + [p.size for p in parts])
    d, g, thr, rec, rng = (dev_in[cuts[i]:cuts[i + 1]] for i in range(5))
    d, g = d.view(N, 7), g.view(G, 8)

    # ordering (torch plumbing): pair = image * K + category
    by_score = torch.sort(d[:, 6], descending=True, stable=True).indices
    dkey = (d[:, 0].long() * K + d[:, 1].long())[by_score]
    dkey, o = torch.sort(dkey, stable=True)
    dperm = by_score[o]                                        # detections by pair, then descending score (stable)
    gkey, gperm = torch.sort(g[:, 0].long() * K + g[:, 1].long(), stable=True)      # ground truth by pair, input order inside
    pairs = torch.unique(torch.cat([dkey, gkey]))              # ascending: every pair with a detection or a ground truth
    P = int(pairs.numel())
    d_first = torch.searchsorted(dkey, pairs)
    d_count = torch.searchsorted(dkey, pairs, right=True) - d_first
    g_first = torch.searchsorted(gkey, pairs)
    g_count = torch.searchsorted(gkey, pairs, right=True) - g_first
    # only the first 100 detections of a pair count: they get the slots
    rank = torch.arange(N, device=dev) - d_first[torch.searchsorted(pairs, dkey)]
    keep = rank < host.MAX_DETS[-1]
    slot_src, slot_key, slot_rank = dperm[keep], dkey[keep], rank[keep].to(torch.uint8)
    Nk = int(slot_src.numel())
    k_count = d_count.clamp(max=host.MAX_DETS[-1])
    k_first = torch.cumsum(k_count, 0) - k_count
    det_box = d[slot_src][:, 2:6].contiguous()
    gt_box = g[gperm][:, 2:8].contiguous()
    pair_tab = torch.stack([k_first, k_count, g_first, g_count], 1).to(torch.int32).contiguous()
    # the category lists: by category, then descending score, then slot order (= image order)
    c_score = torch.sort(d[slot_src][:, 6], descending=True, stable=True).indices
    c_key, o = torch.sort((slot_key % K)[c_score], stable=True)
    cat_dets = c_score[o].to(torch.int32)
    cat_first = _offsets(c_key, K)
    gc_key, cat_gts = torch.sort(gkey % K, stable=True)
    cat_gts = cat_gts.to(torch.int32)
    gt_first = _offsets(gc_key, K)

    dt_flags = torch.empty(2 * A * max(Nk, 1), dtype=torch.int16, device=dev)       # dt_matched, then dt_ignore
    gt_ignore = torch.empty(A * max(G, 1), dtype=torch.uint8, device=dev)
    ws_bytes = int(lib.yh_coco_workspace(Nk, G))
    if ws_bytes < 0:
        raise RuntimeError('libyolo_hip yh_coco_workspace failed (code %d)' % ws_bytes)
    ws = torch.empty(max(ws_bytes, 8) // 2, dtype=torch.int16, device=dev)
    out = torch.empty(T * R * K * A * M + T * K * A * M, dtype=torch.float64, device=dev)
    ptr = lambda t, n=1: t.data_ptr() if n else None
    md = CocoMatchDesc(dets=ptr(det_box, Nk), gts=ptr(gt_box, G), pairs=ptr(pair_tab, P), iou_thrs=thr.data_ptr(), area_rng=rng.data_ptr(),
                       dt_matched=ptr(dt_flags, Nk), dt_ignore=dt_flags.data_ptr() + 2 * A * Nk if Nk else None, gt_ignore=ptr(gt_ignore, G),
                       ws=ptr(ws, G), ws_bytes=ws_bytes, n_pairs=P, n_dets=Nk, n_gts=G)
    ad = CocoAccumDesc(cat_dets=ptr(cat_dets, Nk), cat_first=cat_first.data_ptr(), det_rank=ptr(slot_rank, Nk), cat_gts=ptr(cat_gts, G),
                       gt_first=gt_first.data_ptr(), dt_matched=md.dt_matched, dt_ignore=md.dt_ignore, gt_ignore=md.gt_ignore,
                       rec_thrs=rec.data_ptr(), precision=out.data_ptr(), recall=out.data_ptr() + 8 * T * R * K * A * M,
                       n_dets=Nk, n_gts=G, K=K)
    with hiplib.on_device(dev_in):
        stream = hiplib.stream_ptr() if pin else None
        rc = lib.yh_coco_match(C.byref(md), stream)
        if rc != 0:
            raise RuntimeError('libyolo_hip yh_coco_match failed (code %d)' % rc)
        rc = lib.yh_coco_accumulate(C.byref(ad), stream)
        if rc != 0:
            raise RuntimeError('libyolo_hip yh_coco_accumulate failed (code %d)' % rc)
    host_out = torch.empty(out.numel(), dtype=torch.float64, pin_memory=pin)
    host_out.copy_(out, non_blocking=True)          # the one device-to-host read
    if pin:
        torch.cuda.current_stream(dev).synchronize()
    res = host_out.numpy()
    precision = res[:T * R * K * A * M].reshape(T, R, K, A, M).copy()
    recall = res[T * R * K * A * M:].reshape(T, K, A, M).copy()
    LAST.update(pairs=P, dets=N, slots=Nk, gts=G, hip_launches=(1 if P else 0) + 1, bytes_to_device=8 * host_in.numel(),
                bytes_to_host=8 * host_out.numel(), workspace_bytes=ws_bytes)
    return dict(precision=precision, recall=recall, stats=host.summarize(precision, recall))
