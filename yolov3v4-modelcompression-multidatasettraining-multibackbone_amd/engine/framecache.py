"""Device-resident frame cache (``train.py --device-cache``): every training frame, decoded and resized once exactly as
``utils.datasets.load_image`` does it, in ONE uint8 arena in device memory.  A training item is then geometry alone
(``utils.datasets.CachedMosaicItem``) and a batch is rendered by one ``yh_mosaic_affine_hsv_batch`` launch that reads the arena
(``engine.preprocess.render_cached_mosaic_batch``): after the build no pixel crosses the host.

The cache lives outside the dataset, so nothing large is pickled to the loader workers; the dataset keeps only the ``(h, w)`` table
it builds the items from (``utils.datasets.frame_size_tables``: image headers, no decode).  With ``device='cpu'`` the arena is a
host tensor - what the CPU test tier renders from through the emulated library.
"""
import ctypes as C
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .hiplib import MosaicDesc

ALIGN = 16                   # frame offsets in the arena
MAX_THREADS = 16             # decode + resize pool of the fill
STAGING_BYTES = 64 << 20     # one pinned staging chunk (two are in flight); a larger frame gets a chunk of its own size
DESC_SLOTS = 2               # pinned descriptor tables in rotation (render_cached_mosaic_batch)


def free_memory(device):
    """Bytes the arena may take on ``device`` right now."""
    device = torch.device(device)
    if device.type == 'cuda':
        return int(torch.cuda.mem_get_info(device)[0])
    return int(os.sysconf('SC_AVPHYS_PAGES')) * int(os.sysconf('SC_PAGE_SIZE'))


def allocate_arena(nbytes, device):
    return torch.empty(max(nbytes, ALIGN), dtype=torch.uint8, device=device)


def plan_arena(hw, channels):
    """``(offsets int64 [n + 1], total bytes)`` of frames of ``hw[i]`` = (h, w) with ``channels`` interleaved bytes per pixel, every
    offset rounded up to ``ALIGN``; ``offsets[n]`` is the total."""
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1].astype(np.int64) * channels
    padded = (sizes + ALIGN - 1) // ALIGN * ALIGN
    offsets = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    return offsets, int(offsets[-1])


class _DescSlot:
    __slots__ = ('buf', 'event', 'busy')


class DeviceFrameCache:
    """``arena`` (uint8, on ``device``), ``offsets`` (int64, n + 1), ``hw`` / ``hw0`` (int32 (n, 2): resized / decoded size)."""

    def __init__(self, arena, offsets, hw, hw0, channels, build_seconds=0.0):
        self.arena, self.offsets, self.hw, self.hw0, self.channels = arena, offsets, hw, hw0, channels
        self.device, self.nbytes, self.build_seconds = arena.device, int(offsets[-1]), build_seconds
        self._slots, self._next = [], 0

    def __len__(self):
        return len(self.hw)

    def frame(self, i):
        """Frame ``i`` as an ``(h, w, c)`` view of the arena."""
        h, w = int(self.hw[i][0]), int(self.hw[i][1])
        return self.arena[int(self.offsets[i]):int(self.offsets[i]) + h * w * self.channels].view(h, w, self.channels)

    @classmethod
    def build(cls, dataset, device):
        """Size the arena from the image headers, refuse before allocating when it does not fit, then fill it with exactly the
        frames ``utils.datasets.load_image(dataset, i)`` returns."""
        from utils import datasets
        t0 = time.time()
        device = torch.device(device)
        if getattr(dataset, 'frame_hw', None) is not None:
            hw0, hw = dataset.frame_hw0, dataset.frame_hw
        else:
            hw0, hw = datasets.frame_size_tables(dataset)
        gray = bool(dataset.is_gray_scale)
        c = 1 if gray else 3
        offsets, total = plan_arena(hw, c)
        free = free_memory(device)
        if total > free:
            raise RuntimeError('the frame cache needs %d bytes for %d frames at img_size %d but %s has %d bytes free'
                               % (total, len(hw), dataset.img_size, device, free))
        arena = allocate_arena(total, device)
        n = len(hw)

        def load(i, dst, base):
            img = datasets.load_image(dataset, i, gray)[0]
            if tuple(img.shape) != (int(hw[i][0]), int(hw[i][1]), c):
                raise RuntimeError('%s decodes to %s, its header promised %s' % (dataset.img_files[i], img.shape, tuple(hw[i]) + (c,)))
            o = int(offsets[i]) - base
            dst[o:o + img.size] = img.reshape(-1)

        with ThreadPoolExecutor(max_workers=max(1, min(MAX_THREADS, n))) as pool:
            if device.type != 'cuda':
                flat = arena.numpy()
                list(pool.map(lambda i: load(i, flat, 0), range(n)))
            else:
                chunk = max(STAGING_BYTES, int(np.diff(offsets).max()))
                staging = [torch.zeros(chunk, dtype=torch.uint8).pin_memory() for _ in range(2)]
                events = [None, None]
                first, k = 0, 0
                with torch.cuda.device(device):
                    while first < n:
                        last = first + 1          # frames [first, last) fill one staging chunk
                        while last < n and int(offsets[last + 1] - offsets[first]) <= chunk:
                            last += 1
                        if events[k] is not None:
                            events[k].synchronize()     # the copy that last read this staging buffer has finished
                        base, flat = int(offsets[first]), staging[k].numpy()
                        list(pool.map(lambda i: load(i, flat, base), range(first, last)))
                        nbytes = int(offsets[last]) - base
                        arena[base:base + nbytes].copy_(staging[k][:nbytes], non_blocking=True)
                        events[k] = torch.cuda.Event()
                        events[k].record()
                        first, k = last, k ^ 1
                    torch.cuda.synchronize(device)
        return cls(arena, offsets, hw, hw0, c, time.time() - t0)

    # ------------------------------------------------------------------ descriptor tables of render_cached_mosaic_batch
    def desc_slot(self, n):
        """A host buffer for ``n`` descriptors that nothing in flight still reads: pinned on a GPU cache, where the slot's event (set
        by ``release_slot`` after the upload was queued) is waited for before the buffer is handed out again."""
        need = n * C.sizeof(MosaicDesc)
        if not self._slots:
            for _ in range(DESC_SLOTS):
                s = _DescSlot()
                s.buf, s.event, s.busy = None, None, False
                self._slots.append(s)
        s = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        if s.busy:
            s.event.synchronize()
            s.busy = False
        if s.buf is None or s.buf.numel() < need:
            s.buf = torch.empty(max(need, 64 * C.sizeof(MosaicDesc)), dtype=torch.uint8)
            if self.device.type == 'cuda':
                s.buf = s.buf.pin_memory()
                s.event = torch.cuda.Event()
        return s

    def release_slot(self, s):
        """Call after the non-blocking upload of the slot was queued on the current stream."""
        if self.device.type == 'cuda':
            s.event.record()
            s.busy = True
