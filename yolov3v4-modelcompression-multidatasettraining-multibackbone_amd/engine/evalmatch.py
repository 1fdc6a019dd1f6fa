"""Per-batch evaluation statistics on the device: ``yh_eval_match`` (csrc/evalmatch.hip) behind ``test.py``.

The mAP protocol's per-image loop (reference test.py:123-185; ``test._match`` here) costs hundreds of host/device round trips per
image on device tensors: a ``tolist`` per image, two ``nonzero`` per label class, one ``int()`` per over-threshold detection, three
``.cpu()`` reads.  ``match_batch`` does the same work for the whole batch with one small host-to-device copy (the per-image pointer
table and the label order), ONE launch and ONE device-to-host read into pinned memory - flags, confidences and classes of every
detection of the batch together.  The detections are clipped in place on the way, like ``clip_coords`` did, so whatever reads
``output`` afterwards (``--save-json``, the plots) sees the clipped boxes.

There is no fallback: on a CUDA tensor a missing library or entry point raises (engine/hiplib.py).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import hiplib
from .hiplib import EvalMatchDesc, EvalMatchRow

_LIB_OVERRIDE = None   # tests inject the host emulation here


def _lib():
    return _LIB_OVERRIDE if _LIB_OVERRIDE is not None else hiplib.load()


def enabled(device):
    """The device matcher serves CUDA tensors; ``YOLO_HIP_EVAL_MATCH=0`` keeps the host loop there too, for A/B runs."""
    return torch.device(device).type == 'cuda' and os.environ.get('YOLO_HIP_EVAL_MATCH', '1') != '0'


def label_order(targets_host, nb):
    """``targets`` rows grouped by image, stable within an image: (order int32 (nt,), first (nb,), count (nb,)).  Image ``si``'s labels
    are ``targets[order[first[si]:first[si] + count[si]]]`` - the rows, in the order, of ``targets[targets[:, 0] == si]``."""
    img = targets_host[:, 0].numpy() if len(targets_host) else np.zeros(0, np.float32)
    order = np.argsort(img, kind='stable').astype(np.int32)
    srt = img[order]
    ids = np.arange(nb, dtype=np.float32)
    first = np.searchsorted(srt, ids, side='left')
    count = np.searchsorted(srt, ids, side='right') - first
    return order, first, count


def match_batch(output, targets_host, targets_dev, height, width, iouv):
    """The ``stats`` entries of one evaluation batch, in image order: ``(correct bool (n, niou), conf (n,), cls (n,), tcls list)`` as host
    tensors for every image with detections, the empty entry for an image with labels and no detections, nothing for an image with
    neither (reference test.py:130-133, 185).  ``output`` is the NMS result (a list of ``(n, 6)`` tensors or None); its boxes are
    clipped to the image in place.  ``targets_host`` is the loader's host copy of ``targets_dev``: label counts and ``tcls`` come
    from it, never from a device read."""
    lib = _lib()
    nb = len(output)
    niou = int(iouv.numel())
    targets_host = targets_host.detach().to('cpu', torch.float32).contiguous()
    nt = int(targets_host.shape[0])
    order, first, count = label_order(targets_host, nb)
    tcls_all = targets_host[:, 1].numpy()[order] if nt else np.zeros(0, np.float32)

    rows = (EvalMatchRow * max(nb, 1))()
    staged = []      # (pred, dense fp32 stand-in) of detections the kernel cannot address directly
    total = 0
    for si, pred in enumerate(output):
        r = rows[si]
        r.lab_first, r.nl, r.out_off = int(first[si]), int(count[si]), total
        if pred is None or pred.shape[0] == 0:
            continue
        box = pred
        if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.data_ptr() % 4:
            box = pred.detach().float().contiguous()
            staged.append((pred, box))
        r.pred, r.n = box.data_ptr(), int(pred.shape[0])
        total += r.n

    conf = cls = correct = None
    if total:
        dev = targets_dev.device
        pin = dev.type == 'cuda'
        tdev = targets_dev if targets_dev.dtype == torch.float32 and targets_dev.is_contiguous() else targets_dev.float().contiguous()
        idev = iouv if iouv.dtype == torch.float32 and iouv.is_contiguous() else iouv.float().contiguous()
        # one host-to-device copy: the pointer table, then the label order
        table_bytes = C.sizeof(EvalMatchRow) * nb
        host_in = torch.empty(table_bytes + 4 * nt, dtype=torch.uint8, pin_memory=pin)
        host_in[:table_bytes] = torch.frombuffer(bytearray(bytes(rows)[:table_bytes]), dtype=torch.uint8)
        if nt:
            host_in[table_bytes:] = torch.from_numpy(order.view(np.uint8))
        dev_in = host_in.to(dev, non_blocking=True)
        # one buffer for everything the host reads back: conf / cls of every detection, then the flags
        out = torch.empty(8 * total + niou * total, dtype=torch.uint8, device=dev)
        ws = torch.empty(2 * total + nt, dtype=torch.int32, device=dev)
        d = EvalMatchDesc(rows=dev_in.data_ptr(), targets=tdev.data_ptr() if nt else None,
                          label_index=dev_in.data_ptr() + table_bytes if nt else None, iouv=idev.data_ptr(),
                          correct=out.data_ptr() + 8 * total, conf_cls=out.data_ptr(), ws=ws.data_ptr(), ws_bytes=4 * ws.numel(),
                          images=nb, nt=nt, total=total, niou=niou, width=float(width), height=float(height))
        with hiplib.on_device(targets_dev):
            rc = lib.yh_eval_match(C.byref(d), hiplib.stream_ptr() if pin else None)
        if rc != 0:
            raise RuntimeError('libyolo_hip yh_eval_match failed (code %d)' % rc)
        for pred, box in staged:
            pred.copy_(box)
        host_out = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=pin)
        host_out.copy_(out, non_blocking=True)       # the batch's one device-to-host read
        if pin:
            torch.cuda.current_stream(dev).synchronize()
        conf_cls = host_out[:8 * total].view(torch.float32).view(total, 2)
        conf, cls = conf_cls[:, 0].contiguous(), conf_cls[:, 1].contiguous()
        correct = host_out[8 * total:].view(total, niou) != 0

    stats = []
    for si, pred in enumerate(output):
        tcls = tcls_all[first[si]:first[si] + count[si]].tolist()
        if pred is None:
            if tcls:
                stats.append((torch.zeros(0, niou, dtype=torch.bool), torch.Tensor(), torch.Tensor(), tcls))
            continue
        n, o = int(pred.shape[0]), rows[si].out_off
        if n == 0:
            stats.append((torch.zeros(0, niou, dtype=torch.bool), torch.zeros(0), torch.zeros(0), tcls))
        else:
            stats.append((correct[o:o + n], conf[o:o + n], cls[o:o + n], tcls))
    return stats
