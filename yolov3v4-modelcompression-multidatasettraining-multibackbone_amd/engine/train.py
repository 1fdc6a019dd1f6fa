"""Training step of the cfg graph on the HIP kernels.

Replaces, for CUDA tensors in ``model.train()`` mode, what the reference gets from eager PyTorch + autograd:
``Darknet.forward`` in training mode (models.py:414-492: conv -> train-mode BatchNorm -> activation per block, shortcut
adds, route concats, upsample, raw ``p`` per yolo head, models.py:336-340) and the backward of all of it.  The loss
(``compute_loss``, utils.py:368) stays a torch function on the three raw head tensors; its gradient enters here as
fp32 head gradients and leaves as fp32 parameter gradients (fp16 compute with fp32 master weights and gradients, the
``-mpt`` mixed-precision recipe of train.py; or fp32 throughout).

Lowering is shared with the inference engine (``DarknetEngine._build_values`` / ``_place``): the same values, the same
zero-copy concat placement, the same fused residual / 2x-upsample stores.  Per conv block the forward plan runs

    conv (linear, MFMA implicit GEMM) -> z      yh_conv2d_fwd / yh_conv2d_stem_fwd
    batch statistics of z                      yh_bn_stats, yh_bn_finalize (also the running-stat update)
    y = act(bn(z)) [+ residual] [2x store]     yh_bn_act_fwd

and the backward plan, walking the values in reverse,

    dy of a fused upsample                     yh_upsample2_bwd
    residual: grad(res) += dy                  yh_add_channels / yh_copy_channels
    dgamma, dbeta (or conv-bias grad)          yh_bn_act_bwd_reduce   (written straight into the gradient arena)
    dz                                         yh_bn_act_bwd_apply
    dW                                         yh_conv2d_wgrad (first layer: through an 8-channel NHWC copy of the image)
    grad(input) (+)= conv(dz, W^T flipped)     yh_conv2d_fwd on the dgrad weight image (stride 2: four parity phases)

Every activation, z and gradient buffer is kept for the whole step (288 GB of HBM: YOLOv3-608 batch 64 needs ~40 GB).
They are pieces of ONE byte arena per engine that the plans of all input shapes share (``_StepArena``; multi-scale training draws
a new shape every step): a plan records offsets and binds the arena through a plan slot, so it may not assume that a buffer still
holds what its build or its previous step left there.  ``reserve`` sizes the arena ahead of the first step.
Depthwise blocks, squeeze-excite, max-pools (incl. SPP) and CSP group-split routes are lowered too (csrc/depthwise.hip,
csrc/train.hip).  Graphs whose widths are not multiples of 8 (slim-pruned nets, GhostNet) train through the channel-padded twin
of ``engine/padded.py``; what neither form covers (weighted shortcuts, grouped convs other than depthwise) raises
NotImplementedError at plan build - ``models.Darknet`` has no eager fallback for training.

The plans are built by ``_TrainPlanBuilder`` (``engine/train_plan.py``: one emitter per block kind and pass); this module keeps the
engine, the arenas and the run path.
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import hiplib
from .hiplib import PackItem, BnL1Row
from .plan import DarknetEngine, ALIGN_C, _round_up

# stride-2 data gradients with at most this many input channels run as ONE four-phase pass (ups = 4: 16 tap-GEMMs instead of 9, dz read
# once); above it the four parity-phase launches.  Measured (profiles/r05_fused_dgrad_ab.txt): 64 input channels (152^2, 128 -> 64) 0.642 ms
# fused against 0.704 in four launches; 128 channels (76^2) 0.480 against 0.441 - the 78 % of extra tap work outweighs the dz re-reads from
# there on.  A/B knob: YOLO_HIP_FUSED_DGRAD_MAX
_FUSED_DGRAD_MAX_CIN = int(os.environ.get('YOLO_HIP_FUSED_DGRAD_MAX', '64'))

SLOT_INPUT = 0
SLOT_WS = 1          # shared fp32 workspace of the two-stage reductions
SLOT_HEAD0 = 2       # forward: head output tensors; backward: head gradient tensors (fp32 NHWC)
LINEAR = hiplib.ACT_CODES['linear']


class ChannelAlignmentError(NotImplementedError):
    """The aligned lowering wants every tensor width to be a multiple of 8: ``engine/padded.py`` trains such graphs through a
    channel-padded twin."""


class _Arena:
    """One flat fp32 tensor handed out in 16-byte aligned pieces (per-channel statistics, parameter gradients)."""

    def __init__(self):
        self.size = 0
        self.items = []

    def reserve(self, n):
        off = self.size
        self.size += _round_up(n, 4)
        return off

    def allocate(self, state):
        self.buf = state.tensor(max(self.size, 4), torch.float32, zero=True)
        return self.buf

    def ptr(self, off):
        return self.buf.data_ptr() + 4 * off

    def view(self, off, n):
        return self.buf[off:off + n]


SLOT_ARENA = 62      # base of the engine's step arena: every activation / gradient / scratch pointer of a plan is a fixup on it
ARENA_ALIGN = 512    # what torch's allocator gave these buffers when each was a tensor of its own
# While a plan is being built its step buffers have no address yet: a pointer into piece k reads TAG | k << 40 | byte offset.  Bit 62
# makes it a non-canonical address no allocator returns, so a descriptor field holding one is recognised by value; equal buffers
# still compare equal and keep their alignment, which is all the library's geometry queries look at.
_PIECE_TAG, _PIECE_SHIFT = 1 << 62, 40


class _Piece:
    """A step buffer of one plan: a byte range of the engine's step arena, placed when the plan is complete."""
    __slots__ = ('arena', 'index', 'n', 'dtype', 'off')

    def __init__(self, arena, index, n, dtype):
        self.arena, self.index, self.n, self.dtype, self.off = arena, index, int(n), dtype, None

    def numel(self):
        return self.n

    def element_size(self):
        return torch.empty(0, dtype=self.dtype).element_size()

    def nbytes(self):
        return self.n * self.element_size()

    def data_ptr(self):
        return _PIECE_TAG | (self.index << _PIECE_SHIFT)

    def zero_(self):
        self.arena.view(self.off, self.n, self.dtype).zero_()


class _StepArena:
    """The byte arena all plans of a training engine carve their step buffers from.  Only one plan's step is alive at a time, so
    plans alias each other; it only grows, to the largest requirement met (or reserved) so far."""

    def __init__(self):
        self.buf, self.base, self.capacity, self.allocs = None, 0, 0, 0

    def ensure(self, nbytes, device):
        """True when a new arena had to be allocated (every plan must then re-bind, and a step in flight is lost)."""
        if nbytes <= self.capacity and self.buf is not None:
            return False
        self.buf = None                       # release first: the old and the new arena never coexist
        self.buf = torch.empty(nbytes + ARENA_ALIGN, device=device, dtype=torch.uint8)
        self.base = _round_up(self.buf.data_ptr(), ARENA_ALIGN)
        self.capacity = nbytes
        self.allocs += 1
        return True

    def release(self):
        self.buf, self.base, self.capacity = None, 0, 0

    def view(self, off, n, dtype):
        first = self.base - self.buf.data_ptr() + off
        return self.buf[first:first + n * torch.empty(0, dtype=dtype).element_size()].view(dtype)


class _PlanState:
    """The state a plan keeps outside the arena (weight images, statistics / gradient arenas, tables), carved at 512-byte alignment
    from a few chunks of at least 4 MiB instead of one device allocation per tensor: a plan build then leaves a handful of large
    blocks in torch's allocator, not some hundred small ones scattered among the step's transient tensors, where they would pin
    fragments that later steps can no longer reuse."""
    CHUNK = 4 << 20

    def __init__(self, device):
        self.device, self.chunks, self.left, self.used = device, [], 0, 0

    def tensor(self, n, dtype, zero=False):
        nbytes = max(int(n), 1) * torch.empty(0, dtype=dtype).element_size()
        room = _round_up(nbytes, ARENA_ALIGN)
        if room > self.left:
            size = max(room, min(self.CHUNK << len(self.chunks), 64 << 20))
            chunk = torch.empty(size + ARENA_ALIGN, device=self.device, dtype=torch.uint8)
            self.chunks.append(chunk)
            self.pos = _round_up(chunk.data_ptr(), ARENA_ALIGN) - chunk.data_ptr()
            self.left = size
        t = self.chunks[-1][self.pos:self.pos + nbytes].view(dtype)[:int(n)]
        self.pos += room
        self.left -= room
        self.used += room
        return t.zero_() if zero else t


class TrainEngine(DarknetEngine):
    def __init__(self, model, precision='fp16', lib=None):
        if precision not in ('fp16', 'fp32'):
            raise ValueError("training precision must be 'fp16' or 'fp32'")
        super().__init__(model, precision, lib)
        self._tplans = {}
        # plans own descriptors and small per-shape state only (the step buffers live in the arena), so many stay resident:
        # 17 multi-scale sizes plus the shorter last batch of an epoch at each
        self.max_train_plans = max(1, int(os.environ.get('YOLO_HIP_MAX_TRAIN_PLANS', '40')))
        self._arena = _StepArena()
        self.plan_builds = 0
        self._current = None
        self.steps = 0   # forward count; the autograd node checks it so a stale backward fails loudly
        self._l1_blocks = ()   # network-slimming sparsity: blocks whose BatchNorm gamma carries the L1 penalty (set_bn_sparsity)
        self._l1_s = 0.0
        # feature distillation (engine/kd.py): steps whose plans also write the attention maps sum_c |y| of every conv block the
        # reference lists in feature_out, and take the gradient of a loss on them (models.Darknet.hip_return_features = 'attention')
        self.attention = False
        self.step_maps = None
        self._building_attention = False

    # --------------------------------------------------------------------------------- parameters
    def parameters(self):
        """Trainable tensors in the order the autograd function receives them (and returns gradients for)."""
        out = []
        for block in self.model.module_list:
            if isinstance(block, nn.Sequential) and len(block) and isinstance(block[0], nn.Conv2d):
                conv, bn = block[0], None
                for k in list(block.children())[1:]:
                    if isinstance(k, nn.modules.batchnorm.BatchNorm2d):
                        bn = k
                out.append(conv.weight)
                if conv.bias is not None:
                    out.append(conv.bias)
                if bn is not None:
                    out.extend((bn.weight, bn.bias))
            elif isinstance(block, nn.Sequential) and len(block) and block[0].__class__.__name__ == 'SE':
                out.extend((block[0].fc[0].weight, block[0].fc[2].weight))
        return out

    # --------------------------------------------------------------------------------- weights
    def _pack_items(self, plan):
        """Host image of the yh_pack_item table: every weight image of the step (forward, data gradient or its four
        stride-2 phases, first layer) straight from the live fp32 parameters."""
        items = []
        P = hiplib.ptr
        for v in plan['values']:
            if v.kind == 'dw':
                conv = v.conv
                for t in (conv.weight, conv.bias):
                    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                        raise NotImplementedError('HIP training path: parameters must be contiguous fp32 (master weights)')
                items.append(PackItem(w=P(conv.weight), bias=P(conv.bias), packed=P(v.tpack['w']), bias_out=P(v.tpack['b']), mode=4,
                                      dtype=self.code, cout=v.C, cin=1, kh=v.k, kw=v.k, k_pad=v.c_phys, pad=v.pad))
                continue
            if v.kind != 'conv':
                continue
            conv, pk = v.conv, v.tpack
            for t in (conv.weight, conv.bias):
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                    raise NotImplementedError('HIP training path: parameters must be contiguous fp32 (master weights)')
            w, cb = P(conv.weight), P(conv.bias)
            geo = dict(dtype=self.code, cout=v.C, cin=conv.in_channels, kh=v.k, kw=v.k, pad=v.pad)
            if v.src.kind == 'input':
                items.append(PackItem(w=w, bias=cb, packed=P(pk['w']), bias_out=P(pk['b']), mode=3, cout_pad=pk['cout_pad'], **geo))
                continue
            items.append(PackItem(w=w, bias=cb, packed=P(pk['w']), bias_out=P(pk['b']), mode=0, k_pad=pk['cin_k'], m_pad=pk['m_pad'],
                                  **geo))
            if v.stride == 2 and pk.get('stem_fused'):
                # its data gradient runs inside the first block's backward pass (csrc/stem_bwd.hip): the plain flipped-tap image
                items.append(PackItem(w=w, packed=P(pk['wt']), mode=1, k_pad=pk['cout_k'], m_pad=pk['dm_pad'], **geo))
            elif v.stride == 2 and 'wt_fused' in pk:
                items.append(PackItem(w=w, packed=P(pk['wt_fused']), mode=5, k_pad=pk['cout_k'], m_pad=pk['fused_m_pad'],
                                      cout_pad=v.src.c_phys, **geo))
            elif v.stride == 2:
                for (a, b), img in zip(((0, 0), (0, 1), (1, 0), (1, 1)), pk['wt_phase']):
                    items.append(PackItem(w=w, packed=P(img), mode=2, k_pad=pk['cout_k'], m_pad=pk['dm_pad'], pa=a, pb=b, **geo))
            else:
                items.append(PackItem(w=w, packed=P(pk['wt']), mode=1, k_pad=pk['cout_k'], m_pad=pk['dm_pad'], **geo))
        arr = (PackItem * len(items))(*items)
        return bytes(arr), len(items)

    def _refresh_pack_table(self, plan):
        """(Re)write the device table when a parameter moved (plan build, ``param.data = ...``)."""
        ptrs = tuple(t.data_ptr() for t in self.parameters())
        if plan.get('pack_ptrs') == ptrs:
            return
        raw, n = self._pack_items(plan)
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        if plan.get('pack_table') is None or plan['pack_table'].numel() != host.numel():
            raise RuntimeError('pack table size changed: rebuild the plan')
        plan['pack_table'].copy_(host)
        plan['pack_ptrs'] = ptrs

    # --------------------------------------------------------------------------------- sparsity (network slimming)
    def set_bn_sparsity(self, block_indices, s):
        """L1 penalty s * sum |gamma| on the BatchNorm gammas of the cfg blocks ``block_indices`` (reference train.py:443-448 calls
        ``BNOptimizer.updateBN`` after every backward, utils/prune_utils.py:130-138): every backward range adds s * sign(gamma) to the
        gradients of its rows with one ``yh_bn_l1_subgrad`` launch, before the gradients are handed to autograd.  ``s`` may change
        from step to step (it is a launch argument, not part of the table); ``None`` / an empty list switches the term off."""
        blocks = tuple(sorted({int(b) for b in block_indices})) if block_indices is not None else ()
        if blocks:
            have = {}
            for i, block in enumerate(self.model.module_list):
                if isinstance(block, nn.Sequential) and len(block) and isinstance(block[0], nn.Conv2d):
                    have[i] = any(isinstance(k, nn.modules.batchnorm.BatchNorm2d) for k in list(block.children())[1:])
            bad = [b for b in blocks if not have.get(b, False)]
            if bad:
                raise ValueError('set_bn_sparsity: blocks %s are not conv blocks with BatchNorm' % bad)
        if blocks != self._l1_blocks:
            self._l1_blocks = blocks
            for plan in self._tplans.values():
                plan['l1_key'] = None         # rewritten before the next forward
        self._l1_s = float(s) if blocks else 0.0

    def _l1_values(self, plan):
        """The values whose gamma is a row, in ``parameters()`` order (= value order), with the backward range each belongs to."""
        want = set(self._l1_blocks)
        out = []
        for k, seg in enumerate(plan['segments']):
            lo, hi = seg['values']
            for v in plan['values'][lo:hi]:
                if v.kind in ('conv', 'dw') and v.bn is not None and v.block in want:
                    out.append((k, v))
        return out

    def _refresh_l1_table(self, plan):
        """(Re)write the device table of yh_bn_l1_row when the set changed or a gamma moved (plan build, ``param.data = ...``): the
        condition of ``_refresh_pack_table``.  Row r: the live gamma, its slice of the plan's gradient arena, its width."""
        if not self._l1_blocks:
            plan['l1_key'], plan['l1_ranges'] = None, None
            return
        rows = self._l1_values(plan)
        key = (self._l1_blocks, tuple(v.bn.weight.data_ptr() for _, v in rows))
        if plan.get('l1_key') == key:
            return
        missing = set(self._l1_blocks) - {v.block for _, v in rows}
        if missing:
            raise RuntimeError('set_bn_sparsity: blocks %s have no BatchNorm gradient in the training plan' % sorted(missing))
        grads = plan['grads']
        items = []
        for _, v in rows:
            g = v.bn.weight
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise NotImplementedError('HIP training path: BatchNorm tensors must be contiguous fp32')
            items.append(BnL1Row(gamma=g.data_ptr(), grad=grads.ptr(v.g_gamma), n=v.C))
        raw = bytes((BnL1Row * len(items))(*items))
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        table = plan.get('l1_table')
        if table is None or table.numel() < host.numel():
            # sized for every BatchNorm of the graph, so a later change of the set rewrites it in place
            cap = sum(1 for v in plan['values'] if v.kind in ('conv', 'dw') and getattr(v, 'bn', None) is not None)
            table = plan['l1_table'] = plan['state'].tensor(max(cap, len(items)) * C.sizeof(BnL1Row), torch.uint8, zero=True)
        table[:host.numel()].copy_(host)
        ranges, r = [], 0
        for k in range(len(plan['segments'])):
            n = sum(1 for kk, _ in rows if kk == k)
            ranges.append((r, r + n))
            r += n
        plan['l1_ranges'], plan['l1_key'] = ranges, key

    # --------------------------------------------------------------------------------- plans
    def _check_supported(self, values):
        for v in values:
            if v.kind in ('dw', 'se') and v.c_phys != v.C:
                raise ChannelAlignmentError('HIP training path: depthwise / SE blocks need channel counts that are multiples of %d' % ALIGN_C)
            if v.kind in ('qadd',):
                raise NotImplementedError('HIP training path: %s blocks are not lowered yet (block %s)' % (v.kind, v.block))
            if v.kind == 'conv':
                if v.src.kind != 'input' and (v.src.C % ALIGN_C or v.src.c_phys != v.src.C):
                    raise ChannelAlignmentError('HIP training path: channel counts must be multiples of %d' % ALIGN_C)
                if not v.fp32 and v.C % ALIGN_C:
                    raise ChannelAlignmentError('HIP training path: channel counts must be multiples of %d' % ALIGN_C)
                if v.src.kind == 'input' and (v.src.C > 4 or v.src.C > ALIGN_C):
                    raise NotImplementedError('HIP training path: the first conv reads at most 4 image channels')
                if v.stride == 2 and not (v.k == 3 and v.pad == 1):
                    raise NotImplementedError('HIP training path: stride-2 convs must be 3x3 pad 1')
                if v.stride not in (1, 2):
                    raise NotImplementedError('HIP training path: conv stride %d' % v.stride)
                if v.bn is not None and v.fp32:
                    raise NotImplementedError('HIP training path: BatchNorm on a yolo-head conv')

    def _build_train_plan(self, N, Cin, H, W, attention=False):
        # attention plans are built like the evaluation engine's feature_out plans: every conv block keeps its own output (no
        # shortcut / upsample fused into its store), and the next block's data gradient is never folded into the first block's
        # one-pass backward (that form does not materialise the gradient the injection lands in)
        from .train_plan import _TrainPlanBuilder     # imports this module
        self.return_features = self._building_attention = bool(attention)
        try:
            return _TrainPlanBuilder(self, N, Cin, H, W, bool(attention)).build()
        finally:
            self.return_features = self._building_attention = False

    def _attention_values(self, outs):
        """The values whose maps are taken: the blocks ``DarknetEngine._features`` selects (a Sequential not followed by a yolo layer)."""
        mods, feats = self.model.module_list, []
        for i, m in enumerate(mods):
            if m.__class__.__name__ == 'Sequential' and i + 1 < len(mods) and mods[i + 1].__class__.__name__ != 'YOLOLayer':
                v = outs[i]
                if v is None or v.kind == 'input' or v.fp32:
                    raise NotImplementedError('HIP training path: block %d has no activation buffer to take an attention map from' % i)
                feats.append(v)
        if not feats:
            raise NotImplementedError('HIP training path: the graph has no feature_out block')
        return feats

    def _bind(self, plan):
        """Give the plan the arena's current address (after its build, and again after the arena grew)."""
        base = self._arena.base
        if plan['bound'] == base:
            return
        lib = self.lib
        for handle in (plan['fwd'], plan['bwd']):
            lib.yh_plan_bind_slot(handle, SLOT_ARENA, base)
            lib.yh_plan_bind_slot(handle, SLOT_WS, base + plan['ws'].off)
        plan['bound'] = base
        if plan.get('kd_values'):
            # the row table of the attention / inject launches holds addresses: rewritten whenever the arena moved
            from . import kd
            esz = plan['kd_values'][0].storage.element_size()
            raw, plan['kd_rows'], plan['kd_chunks'], plan['kd_shapes'] = kd.feature_rows(
                [dict(y=base + u.storage.off, dy=base + u.gstorage.off, dtype=self.code, n=plan['N'], h=u.H, w=u.W, c=u.c_phys, ld=u.ld,
                      c_off=u.c_off) for u in plan['kd_values']])
            assert all((base + u.storage.off) % 16 == 0 and (u.c_off * esz) % 16 == 0 for u in plan['kd_values'])
            plan['kd_table'].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))

    # --------------------------------------------------------------------------------- execute
    def _get_plan(self, x):
        if x.dim() != 4:
            raise ValueError('expected an (N, C, H, W) batch')
        if self.device is None:
            self.device = x.device
        elif self.device != x.device:
            raise RuntimeError('engine was built on %s, input is on %s' % (self.device, x.device))
        return self._plan_for(self._plan_key(x.shape))

    def _plan_key(self, shape):
        """Plans are keyed by the input shape; the plans of attention steps (other ops, other buffers) carry the flag on top, so
        the plain plan of a shape is the same object, with the same ops, whether or not attention steps run in between."""
        key = tuple(int(k) for k in shape)
        return key + (True,) if self.attention else key

    def _cached_plan(self, key):
        """The plan of input shape ``key``, built on first use.  Plans hold descriptors and small per-shape state; the step buffers
        of all of them alias in the engine's arena, so the least recently used ones are evicted by count only (their native handles
        go, the arena is not touched)."""
        plan = self._tplans.get(key)
        if plan is None:
            while len(self._tplans) >= self.max_train_plans:
                old = self._tplans.pop(next(iter(self._tplans)))
                for h in ('fwd', 'bwd'):
                    self.lib.yh_plan_destroy(old[h])
                if self._current is old:
                    self._current = None
            plan = self._build_train_plan(*key)
            self.plan_builds += 1
            self._tplans[key] = plan
        else:
            self._tplans[key] = self._tplans.pop(key)   # most recently used last
        return plan

    def _ensure_arena(self, nbytes):
        if self._arena.ensure(nbytes, self.device):
            # a new arena: the activations of a forward still waiting for its backward went with the old one
            self._current = None
            self.steps += 1

    def _plan_for(self, key):
        plan = self._cached_plan(key)
        self._ensure_arena(plan['arena_need'])
        return plan

    def reserve(self, shapes):
        """Size the arena for the input shapes ``shapes`` [(N, C, H, W)] without running a step: their plans are built (and stay
        in the cache), the arena is allocated once for the largest.  Fails here, not at the first step of that shape, when the
        device cannot hold it."""
        shapes = [tuple(int(k) for k in shape) for shape in shapes]
        if any(len(shape) != 4 for shape in shapes):
            raise ValueError('reserve() takes (N, C, H, W) shapes')
        if self.device is None:
            self.device = next(self.model.parameters()).device
        self._ensure_arena(max([self._cached_plan(self._plan_key(key))['arena_need'] for key in shapes] + [self._arena.capacity]))

    def train_stats(self):
        plans = list(self._tplans.values())
        return dict(plan_builds=self.plan_builds, arena_allocs=self._arena.allocs, arena_bytes=self._arena.capacity,
                    plans_resident=len(plans),
                    plan_bytes=sum(p['state'].used for p in plans))

    def forward(self, x):
        """Run the training forward; returns the fp32 NHWC head tensors [(N, ny, nx, c_phys)] (fresh tensors)."""
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        plan = self._get_plan(x)
        self._bind(plan)
        self._refresh_pack_table(plan)   # the packing itself is op 0 of the forward plan (one launch)
        self._refresh_l1_table(plan)
        lib = self.lib
        plan['stats'].buf.zero_()
        heads = [torch.empty(shape, device=x.device, dtype=torch.float32) for shape in plan['head_shapes']]
        lib.yh_plan_bind_slot(plan['fwd'], SLOT_INPUT, x.data_ptr())
        for k, h in enumerate(heads):
            lib.yh_plan_bind_slot(plan['fwd'], SLOT_HEAD0 + k, h.data_ptr())
        hiplib.check(lib.yh_plan_run(plan['fwd'], hiplib.stream_ptr()), 'yh_plan_run(train forward)')
        self.step_maps = None
        if plan.get('kd_values'):
            # one launch after the forward plan: the maps of every feature, out of the activations where they lie
            from . import kd
            sink = plan['kd_sink']
            self.step_maps = self._arena.view(plan['kd_maps'].off, plan['kd_maps'].n, torch.float32)
            sink.G = self._arena.view(plan['kd_G'].off, plan['kd_G'].n, torch.float32)
            sink.partials = self._arena.view(plan['kd_partials'].off, plan['kd_partials'].n, torch.float32)
            sink.pending = None
            kd.run_attention(plan['kd_table'], plan['kd_rows'], plan['kd_chunks'], self.step_maps, self.lib)
        counters = [v.bn.num_batches_tracked for v in plan['values']
                    if v.kind == 'conv' and v.bn is not None and v.bn.num_batches_tracked is not None]
        if counters:
            torch._foreach_add_(counters, 1)
        if self._current is not None:      # many plans stay resident: only the plan of the step in flight keeps its input and head gradients
            self._current['x'], self._current['bwd_keep'] = None, []
        plan['x'] = x
        self._current = plan
        self.steps += 1
        return heads

    def _make_segments(self, plan, values, heads, bwd_pos):
        """Cut the backward plan into ranges of about equal parameter size (forward order of the conv blocks).

        Each range is one autograd node in ``models.Darknet``: its parameter gradients are handed to autograd (and to
        DistributedDataParallel's bucket hooks) as soon as the range has run, so the RCCL all-reduce of a bucket overlaps
        with the backward kernels of the earlier layers instead of starting after the whole backward plan."""
        want = max(1, int(os.environ.get('YOLO_HIP_TRAIN_SEGMENTS', '8')))
        convs = [i for i, v in enumerate(values) if v.kind == 'conv']
        total = sum(values[i].conv.weight.numel() for i in convs)
        cuts, acc, target = [1], 0, total / want           # value index where each segment starts (value 0 is the input)
        for i in convs:
            if acc >= target * len(cuts) and i > cuts[-1]:
                cuts.append(i)
            acc += values[i].conv.weight.numel()
        cuts.append(len(values))
        nparams = len(plan['param_slices'])
        segs = []
        for k in range(len(cuts) - 1):
            lo, hi = cuts[k], cuts[k + 1]
            cv = [values[i] for i in range(lo, hi) if hasattr(values[i], 'p_first')]
            p_lo = cv[0].p_first if cv else nparams
            nxt = [values[i] for i in range(hi, len(values)) if hasattr(values[i], 'p_first')]
            p_hi = nxt[0].p_first if nxt else nparams
            segs.append(dict(values=(lo, hi), ops=(bwd_pos[id(values[hi - 1])], bwd_pos[id(values[lo - 1])]), params=(p_lo, p_hi),
                             heads=[j for j, h in enumerate(heads) if any(h.src is values[i] for i in range(lo, hi))]))
        assert segs[0]['ops'][1] == len(plan['bwd_ops']) and segs[-1]['ops'][0] == 0
        return segs

    def attention_maps(self, flat):
        """The step's ``AttentionMaps`` over ``flat`` - the autograd output that aliases ``step_maps``."""
        from . import kd
        plan = self._current
        return kd.AttentionMaps(flat, plan['kd_shapes'], sink=plan['kd_sink'])

    def _inject_feature_grads(self, plan, maps_grad):
        """The ONE place where the gradient of a loss on the attention maps enters: after the gradient buffers were zeroed, before
        the first backward op.  The fused KL node left (g, coef, G) in the plan's sink; a torch statement on the maps arrives as an
        ordinary gradient of the flat buffer and takes the same launch with g = 1."""
        from . import kd
        sink = plan['kd_sink']
        pending, sink.pending = sink.pending, None
        if pending is not None:
            g, coef, G = pending
            plan['bwd_keep'] += [g, G]
            kd.run_inject(plan['kd_table'], plan['kd_rows'], plan['kd_chunks'], G, g, coef, self.lib)
        if maps_grad is not None:
            G = maps_grad.contiguous().float()
            if G.numel() != plan['kd_maps'].n:
                raise ValueError('gradient of the attention maps has %d elements, expected %d' % (G.numel(), plan['kd_maps'].n))
            plan['bwd_keep'].append(G)
            kd.run_inject(plan['kd_table'], plan['kd_rows'], plan['kd_chunks'], G, plan['kd_one'], 1.0, self.lib)

    def backward_segment(self, k, head_grads, maps_grad=None):
        """Run backward range ``k`` (the last range first).  ``head_grads``: fp32 gradients of this range's heads, in the
        order of ``plan['segments'][k]['heads']``; ``maps_grad`` (last range of an attention step only): the gradient of the flat
        attention-map buffer, if autograd produced one.  Returns the fp32 gradients of the range's parameters."""
        plan = self._current
        if plan is None:
            raise RuntimeError('backward() without a preceding forward()')
        lib, x = self.lib, plan['x']
        seg, nseg = plan['segments'][k], len(plan['segments'])
        if k == nseg - 1:
            plan['grads'].buf.zero_()
            for t in plan['zero_list']:
                t.zero_()
            lib.yh_plan_bind_slot(plan['bwd'], SLOT_INPUT, x.data_ptr())
            plan['bwd_next'] = nseg - 1
            plan['bwd_keep'] = []
            if plan.get('kd_values'):
                self._inject_feature_grads(plan, maps_grad)
        if plan.get('bwd_next') != k:
            raise RuntimeError('backward ranges must run last to first (expected %s, got %d)' % (plan.get('bwd_next'), k))
        for j, g in zip(seg['heads'], head_grads):
            shape = plan['head_shapes'][j]
            if g is None:
                g = torch.zeros(shape, device=x.device, dtype=torch.float32)
            g = g.contiguous().float()
            if tuple(g.shape) != tuple(shape):
                raise ValueError('head gradient %d has shape %s, expected %s' % (j, tuple(g.shape), shape))
            plan['bwd_keep'].append(g)
            lib.yh_plan_bind_slot(plan['bwd'], SLOT_HEAD0 + j, g.data_ptr())
        first, last = seg['ops']
        if last > first:
            hiplib.check(lib.yh_plan_run_range(plan['bwd'], first, last, hiplib.stream_ptr()), 'yh_plan_run_range(train backward)')
        plan['bwd_next'] = k - 1
        if plan.get('l1_ranges') is not None:
            # the sparsity term of this range's gammas: after the ops that wrote their gradients, before the clone below leaves the arena
            r_lo, r_hi = plan['l1_ranges'][k]
            if r_hi > r_lo:
                hiplib.check(lib.yh_bn_l1_subgrad(plan['l1_table'].data_ptr(), r_lo, r_hi, self._l1_s, hiplib.stream_ptr()),
                             'yh_bn_l1_subgrad')
        p_lo, p_hi = seg['params']
        if p_hi == p_lo:
            return []
        off_lo = plan['param_slices'][p_lo][0]
        off_hi = plan['param_slices'][p_hi - 1][0] + _round_up(plan['param_slices'][p_hi - 1][1], 4)
        flat = plan['grads'].buf[off_lo:off_hi].clone()   # autograd may keep (and later accumulate into) what we return
        return [flat[off - off_lo:off - off_lo + n].view(shape) for off, n, shape in plan['param_slices'][p_lo:p_hi]]

    def backward(self, head_grads):
        """All ranges at once: fp32 head gradients (``forward``'s order) -> list of fp32 parameter gradients."""
        plan = self._current
        if plan is None:
            raise RuntimeError('backward() without a preceding forward()')
        out = [None] * len(plan['segments'])
        for k in reversed(range(len(plan['segments']))):
            out[k] = self.backward_segment(k, [head_grads[j] for j in plan['segments'][k]['heads']])
        return [g for seg in out for g in seg]

    def segment_parameters(self, plan):
        """The parameter list split per backward range (same order as ``parameters()``)."""
        params = self.parameters()
        return [params[seg['params'][0]:seg['params'][1]] for seg in plan['segments']]

    def _drop_plans(self):
        super()._drop_plans()
        for plan in getattr(self, '_tplans', {}).values():
            for key in ('fwd', 'bwd'):
                try:
                    self.lib.yh_plan_destroy(plan[key])
                except Exception:
                    pass
        self._tplans = {}
        self._current = None
        if getattr(self, '_arena', None) is not None:
            self._arena.release()
