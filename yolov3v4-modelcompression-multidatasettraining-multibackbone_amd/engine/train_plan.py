"""Builder of the training plans of ``engine/train.py``: lowers the placed values of one input shape to the forward and the backward
op list of the plan API and lays the step buffers out in the engine's arena.  The per-block op tables are in the module docstring
of ``engine/train.py``; ``TrainEngine._build_train_plan`` is the entry."""
import ctypes as C
import os

import torch

from . import hiplib
from . import train as _train          # _FUSED_DGRAD_MAX_CIN is looked up at build time (an A/B knob tests patch)
from .hiplib import (ConvDesc, StemDesc, CopyDesc, AddDesc, BnStatsDesc, BnFinalizeDesc, BnActFwdDesc, BnBwdReduceDesc,
                     BnBwdApplyDesc, WgradDesc, StemWgradDesc, StemBwdDesc, UpsampleBwdDesc, CastDesc, LayoutDesc, PoolDesc, PoolBwdDesc,
                     PackBatchDesc, DwDesc, SeDesc, DwWgradDesc, DwDgradDesc, SeBwdDesc)
from .plan import ALIGN_C, _round_up
from .train import (_Arena, _Piece, _PlanState, _PIECE_TAG, _PIECE_SHIFT, ARENA_ALIGN, SLOT_INPUT, SLOT_WS, SLOT_HEAD0, SLOT_ARENA,
                    LINEAR)

P = hiplib.ptr
_PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))


class _TrainPlanBuilder:
    """One training plan of ``engine`` for an (N, Cin, H, W) input: ``build()`` returns the plan dict the run path reads
    (``fwd`` / ``bwd`` handles, ``fwd_ops``, ``bwd_ops``, ``zero_list``, ``segments``, ``grads``, ``param_slices``, ``arena_need``, ...).

    Three passes over the values: ``reserve`` (step buffers, parameter slots, weight images), ``emit_forward`` and
    ``emit_backward`` (values in reverse), each dispatching on ``v.kind`` to one emitter per block kind.

    A gradient buffer's first writer must cover it entirely; otherwise the buffer is zeroed before the backward plan runs and every
    contribution accumulates.  ``contribution_mode`` is the one function every writer of a gradient buffer asks; it also holds the
    seal: once a data gradient has taken the BatchNorm backward sums of block ``s`` (``sealed``), no op may write grad(s) until s's
    own backward has consumed it.

    Attributes kept on the ``Value`` objects, beyond what ``_build_values`` / ``_place`` left there:

    =====================  ==========================================  =====================================================
    attribute              set by                                      read by
    =====================  ==========================================  =====================================================
    storage, gstorage,     _materialize, reserve (slices);             every emitter; TrainEngine._bind (kd rows);
    c_off, ld              gstorage re-pointed by _bwd_conv_dy         engine/kd.py
    galias                 _bwd_conv_dy (buffer shared with a          _bwd_conv_dy
                           residual source)
    p_first                _reserve_params, _reserve_se                TrainEngine._make_segments
    g_w, g_b, g_gamma,     _reserve_params                             backward emitters; TrainEngine._refresh_l1_table
    g_beta                                                             (g_gamma); tests
    g_w1, g_w2, pooled,    _reserve_se                                 _fwd_se, _bwd_se
    gate, scratch(2)
    s_sum, s_sumsq,        _reserve_params                             _bn_args
    s_mean, s_invstd
    tpack                  _reserve_conv, _reserve_dw                  emitters; TrainEngine._pack_items
    plain, z               _reserve_conv, _reserve_dw                  forward / backward emitters; _completes_bn_block
    res, ups, Ho, Wo,      _reserve_dw (a dw block then reads like     _fwd_bn_act, _bwd_dw
    fp32 (dw only)         a conv block without fusions)
    bn_args                _fwd_bn_act                                 _bwd_conv_bn_act, _bwd_dw, _dgrad_plain (of v.src)
    fused_dgrad            _dgrad_in_first_block (on v.src)            _bwd_first_block
    dbn_done               _dgrad_plain (on v.src)                     _bwd_conv_bn_act
    =====================  ==========================================  =====================================================
    """

    def __init__(self, engine, N, Cin, H, W, attention):
        self.eng, self.N, self.attention = engine, N, attention
        self.lib, self.code, self.dtype = engine.lib, engine.code, engine.dtype
        self.values, self.heads, self.outs = engine._build_values(N, Cin, H, W)
        engine._check_supported(self.values)
        engine._place(self.values)
        self.plan = plan = dict(values=self.values, heads=self.heads, N=N, storages=[], fwd_ops=[], bwd_ops=[], zero_list=[], ws_floats=0,
                                arena=engine._arena, arena_refs=[], state=_PlanState(engine.device), bound=None, param_slices=[])
        plan['fwd'] = self.lib.yh_plan_create()
        plan['bwd'] = self.lib.yh_plan_create()
        if not plan['fwd'] or not plan['bwd']:
            raise MemoryError('yh_plan_create failed')
        self.stats = plan['stats'] = _Arena()      # zeroed before every forward: BN sums
        self.saved = plan['saved'] = _Arena()      # mean / invstd per BN (kept from forward to backward)
        self.grads = plan['grads'] = _Arena()      # parameter gradients (zeroed before every backward)
        self.pieces = []
        self.head_index = {id(h.src): k for k, h in enumerate(self.heads)}
        # Who reads each value (by identity), in forward order: the backward runs over `values` in reverse, so the LAST contribution to
        # a value's gradient comes from its consumer with the smallest index.
        self.index = {id(u): i for i, u in enumerate(self.values)}
        self.consumers = {}
        for u in self.values:
            for t in self._inputs_of(u):
                if id(t) in self.index:
                    self.consumers.setdefault(id(t), []).append(u)
        self.fuse_dbn = os.environ.get('YOLO_HIP_FUSE_DBN', '1') != '0'
        self.initialised = set()    # ids of the gradient buffers that hold a contribution (or zeros) at this point of the backward
        self.holders = {}           # id of a gradient buffer -> how many values address it
        self.sealed = {}            # id of a gradient buffer -> the block whose BatchNorm backward sums were taken from it
        self.bwd_pos = {}           # value -> index of its first backward op (ops of value i span [pos[i], pos[i-1]) in emission order)

    def build(self):
        self.reserve()
        self._reserve_shared()
        self.emit_forward()
        self.emit_backward()
        return self._finish()

    @staticmethod
    def _inputs_of(u):
        """The values `u` reads."""
        ins = [getattr(u, 'src', None), getattr(u, 'res', None), getattr(u, 'a', None), getattr(u, 'b', None)]
        ins += [part[0] for part in getattr(u, 'parts', None) or []]
        return [t for t in ins if t is not None]

    # --------------------------------------------------------------------------------- plan API
    def _add(self, side, desc, what):
        plan = self.plan
        handle = plan[side]
        idx = self.lib.yh_plan_add(handle, hiplib.OP_KIND[type(desc)], C.byref(desc), C.sizeof(desc))
        if idx < 0:
            hiplib.check(idx, 'yh_plan_add(%s)' % what)
        plan[side + '_ops'].append((what, desc))
        for name, ctype in desc._fields_:
            val = getattr(desc, name) if ctype is C.c_void_p else None
            if val and val >> 62 == 1:          # a step buffer: becomes a fixup on the arena slot once the pieces are placed
                plan['arena_refs'].append((handle, idx, getattr(type(desc), name).offset, (val ^ _PIECE_TAG) >> _PIECE_SHIFT,
                                           val & ((1 << _PIECE_SHIFT) - 1), what))
        return idx

    def _fixup(self, side, op, desc_type, field, slot):
        hiplib.check(self.lib.yh_plan_add_fixup(self.plan[side], op, getattr(desc_type, field).offset, slot, 0), 'fixup')

    def _needs_ws(self, floats):
        self.plan['ws_floats'] = max(self.plan['ws_floats'], floats)

    def _add_reduction(self, side, desc, what):
        """Reductions get the shared workspace (bound to SLOT_WS at run time) sized by the library's own query."""
        lib = self.lib
        query = lib.yh_conv2d_wgrad_workspace if isinstance(desc, WgradDesc) and not isinstance(desc, StemWgradDesc) \
            else lib.yh_dw_wgrad_workspace if isinstance(desc, DwWgradDesc) else lib.yh_bn_reduce_workspace
        need = int(query(C.byref(desc)))
        desc.ws_floats = need
        self._needs_ws(need)
        op = self._add(side, desc, what)
        if need:
            self._fixup(side, op, type(desc), 'ws', SLOT_WS)
        return op

    # --------------------------------------------------------------------------------- buffers
    def _alloc(self, shape, fp32=False):
        """A step buffer: a piece of the engine's arena, which other plans overwrite between two steps of this one - nothing
        may rely on what an earlier step (or the build) left in it."""
        n = 1
        for k in shape:
            n *= int(k)
        t = _Piece(self.eng._arena, len(self.pieces), n, torch.float32 if fp32 else self.dtype)
        self.pieces.append(t)
        self.plan['storages'].append(t)
        return t

    def _keep(self, n, dtype, zero=False):
        """State the plan keeps for itself, outside the arena (counted in plan_bytes)."""
        return self.plan['state'].tensor(n, dtype, zero)

    def _materialize(self, v):
        if v.storage is not None:
            return
        if v.parent is not None:
            self._materialize(v.parent)
            v.storage, v.c_off, v.ld = v.parent.storage, v.parent.c_off + v.parent_off, v.parent.ld
            v.gstorage = v.parent.gstorage
        else:
            shape = (self.N, v.H, v.W, v.c_phys)
            v.storage = None if v.fp32 else self._alloc(shape)
            v.gstorage = None if v.fp32 else self._alloc(shape)
            v.c_off, v.ld = 0, v.c_phys

    def _junk(self, n):
        """Scratch accumulator for a reduction output nobody reads (lives past the parameter slices)."""
        junk = self.plan.get('junk')
        if junk is None or self.plan['junk_n'] < n:
            raise RuntimeError('junk accumulator was not reserved')
        return junk

    # --------------------------------------------------------------------------------- pass 1: buffers, parameter slots
    def reserve(self):
        reserve = {'conv': self._reserve_conv, 'dw': self._reserve_dw, 'se': self._reserve_se}
        for v in self.values:
            if v.kind == 'input':
                continue
            if v.kind == 'slice':   # a channel range of its source: same buffers, forward and gradient
                self._materialize(v.src)
                v.storage, v.gstorage, v.c_off, v.ld = v.src.storage, v.src.gstorage, v.src.c_off + v.first, v.src.ld
                continue
            self._materialize(v)
            if v.kind in reserve:
                reserve[v.kind](v)

    def _reserve_params(self, v, conv, bn):
        """Gradient slots in parameters() order (weight, bias, gamma, beta), batch sums and saved mean / invstd of a conv or dw block."""
        slices, grads = self.plan['param_slices'], self.grads      # (arena offset, numel, shape) in parameters() order
        v.p_first = len(slices)
        v.g_w = grads.reserve(conv.weight.numel())
        slices.append((v.g_w, conv.weight.numel(), tuple(conv.weight.shape)))
        v.g_b = None
        if conv.bias is not None:
            v.g_b = grads.reserve(v.c_phys)
            slices.append((v.g_b, v.C, (v.C,)))
        if bn is not None:
            v.g_gamma, v.g_beta = grads.reserve(v.C), grads.reserve(v.C)
            slices.append((v.g_gamma, v.C, (v.C,)))
            slices.append((v.g_beta, v.C, (v.C,)))
            v.s_sum, v.s_sumsq = self.stats.reserve(v.C), self.stats.reserve(v.C)
            v.s_mean, v.s_invstd = self.saved.reserve(v.C), self.saved.reserve(v.C)

    def _reserve_dw(self, v):
        self._reserve_params(v, v.conv, v.bn)
        v.tpack = dict(w=self._keep(v.k * v.k * v.c_phys, self.dtype), b=self._keep(v.c_phys, torch.float32))
        v.plain = v.bn is None and v.act == LINEAR
        v.z = None if v.plain else self._alloc((self.N, v.H, v.W, v.c_phys))
        v.res, v.ups, v.Ho, v.Wo, v.fp32 = None, 1, v.H, v.W, False

    def _reserve_se(self, v):
        slices = self.plan['param_slices']
        v.p_first = len(slices)
        v.g_w1 = self.grads.reserve(v.fc1.weight.numel())
        slices.append((v.g_w1, v.fc1.weight.numel(), tuple(v.fc1.weight.shape)))
        v.g_w2 = self.grads.reserve(v.fc2.weight.numel())
        slices.append((v.g_w2, v.fc2.weight.numel(), tuple(v.fc2.weight.shape)))
        for t in (v.fc1.weight, v.fc2.weight):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise NotImplementedError('HIP training path: parameters must be contiguous fp32 (master weights)')
        rows = (self.N, v.c_phys)
        v.pooled, v.gate, v.scratch = self._alloc(rows, fp32=True), self._alloc(rows, fp32=True), self._alloc(rows, fp32=True)
        v.scratch2 = self._alloc((self.N, v.c_phys + 2 * v.fc1.weight.shape[0]), fp32=True)      # factors of the two weight gradients per image

    def _reserve_conv(self, v):
        self._reserve_params(v, v.conv, v.bn)
        keep, taps = self._keep, v.k * v.k
        if v.src.kind == 'input':
            cout_pad = _round_up(v.C, 32) if v.C % 32 == 0 else _round_up(v.C, 16)
            v.tpack = dict(w=keep(taps * v.src.C * cout_pad, torch.float32), b=keep(cout_pad, torch.float32), cout_pad=cout_pad)
        else:
            kstep = self.eng.kstep
            cin_k = _round_up(v.src.c_phys, kstep)
            m_pad = _round_up(v.c_phys, 128)
            cout_k = _round_up(v.c_phys, kstep)          # dgrad: K runs over the output channels
            dm_pad = _round_up(v.src.c_phys, 128)
            v.tpack = dict(w=keep(m_pad * taps * cin_k, self.dtype),
                           b=keep(m_pad, torch.float32), cin_k=cin_k, m_pad=m_pad,
                           wt=None if v.stride == 2 else keep(dm_pad * taps * cout_k, self.dtype),
                           cout_k=cout_k, dm_pad=dm_pad)
            if self._dgrad_fused_into_stem(v):
                v.tpack['stem_fused'] = True
                v.tpack['wt'] = keep(dm_pad * taps * cout_k, self.dtype)
            elif v.stride == 2 and 16 <= v.src.c_phys <= _train._FUSED_DGRAD_MAX_CIN and v.src.c_phys % 4 == 0:
                # few input channels: the data gradient is bound by reading dz and writing dx, so all four parity phases
                # run as ONE 2x2-tap GEMM with 4 * cin rows (16 tap-GEMMs instead of 9, but dz is read once, not four
                # times, and each workgroup writes whole rows of dx): yh_conv2d_fwd ups = 4
                v.tpack['fused_m_pad'] = _round_up(4 * v.src.c_phys, 128)
                v.tpack['wt_fused'] = keep(v.tpack['fused_m_pad'] * 4 * cout_k, self.dtype)
            elif v.stride == 2:
                # parity (a, b) sees ((a + pad) // 2 + 1) x ((b + pad) // 2 + 1) taps
                v.tpack['phase_taps'] = [((a + v.pad) // 2 + 1, (b + v.pad) // 2 + 1) for a, b in _PHASES]
                v.tpack['wt_phase'] = [keep(dm_pad * th * tw * cout_k, self.dtype) for th, tw in v.tpack['phase_taps']]
        # z: the conv output before BN / activation.  Blocks with neither BN nor activation store straight to y.
        v.plain = v.bn is None and v.act == LINEAR and v.res is None and v.ups == 1
        if v.fp32 and not v.plain:
            raise NotImplementedError('HIP training path: yolo-head conv with BN / activation / residual')
        v.z = None if v.plain else self._alloc((self.N, v.Ho, v.Wo, v.c_phys))

    def _reserve_shared(self):
        """What the plan has once: the junk accumulator, the three small arenas, the zero bias row, the dz scratch, the pack table
        (and with it op 0 of the forward plan)."""
        plan, values, keep = self.plan, self.values, self._keep
        plan['junk_n'] = max(v.c_phys for v in values if v.kind in ('conv', 'dw'))
        plan['junk'] = self.grads.reserve(plan['junk_n'])
        for arena in (self.stats, self.saved, self.grads):
            arena.allocate(plan['state'])
        # one zero row serves every data gradient as its bias: as long as the longest m_pad among them, incl. the one-pass stride-2 form's
        # 4 * cin rows (a narrow / pruned net whose widest conv input is <= 128 but that has a stride-2 conv with 33 .. 64
        # inputs needs 256 there and failed at plan build)
        # (it is read-only and its length does not depend on the input shape: the plan's own, outside the arena, so no step has to
        # zero it again after another plan used the arena)
        self.zero_bias = keep(max([max(_round_up(v.src.c_phys, 128), v.tpack.get('fused_m_pad', 0))
                                   for v in values if v.kind == 'conv' and v.src.kind != 'input'] + [128]), torch.float32, zero=True)
        dz_elems = max(self.N * v.Ho * v.Wo * v.c_phys for v in values if v.kind in ('conv', 'dw'))
        # one dz scratch, one stream: a side lane for the weight gradients and a reduce stream were measured and removed
        self.dz_buf = self._alloc((dz_elems,))
        raw, n_items = self.eng._pack_items(plan)
        plan['pack_table'] = keep(len(raw), torch.uint8, zero=True)
        self._add('fwd', PackBatchDesc(items=plan['pack_table'].data_ptr(), n_items=n_items), 'pack')

    # --------------------------------------------------------------------------------- first-block forms
    def _stem_bwd_fused(self, v, s):
        """The one-pass backward of the first block applies: fp16 step, 3x3 / stride 1 / pad 1 on a 1- or 3-channel image, 16 or
        32 output channels, BatchNorm + activation, nothing fused into its store (YOLO_HIP_STEM_BWD=0: the four-launch form)."""
        if os.environ.get('YOLO_HIP_STEM_BWD', '1') == '0':
            return False
        return (self.code == hiplib.YH_F16 and v.bn is not None and v.k == 3 and v.stride == 1 and v.pad == 1 and s.C in (1, 3)
                and v.c_phys in (16, 32) and v.C == v.c_phys and v.ups == 1 and v.res is None and v.conv.bias is None)

    def _dgrad_fused_into_stem(self, v):
        """conv `v` is the ONLY consumer of the first block, a 3x3 / stride 2 / pad 1 conv with 64 output channels on its 32
        channels, and the first block takes the one-pass backward: then v's data gradient is computed inside that pass
        (YOLO_HIP_STEM_DGRAD=0 keeps it a launch of its own)."""
        s = v.src
        if os.environ.get('YOLO_HIP_STEM_DGRAD', '1') == '0':
            return False
        if self.attention:      # the first block's dy takes an injection: it has to exist as a buffer
            return False
        if v.kind != 'conv' or s.kind != 'conv' or s.src.kind != 'input' or not self._stem_bwd_fused(s, s.src):
            return False
        if not (v.k == 3 and v.stride == 2 and v.pad == 1 and v.C == 64 and v.c_phys == 64 and s.c_phys == 32 and not v.fp32):
            return False
        if s.parent is not None or s.c_off != 0 or s.ld != s.c_phys:
            return False
        return all(u is v for u in self.consumers.get(id(s), []))

    # --------------------------------------------------------------------------------- pass 2: forward ops
    def emit_forward(self):
        emit = {'conv': self._fwd_conv, 'dw': self._fwd_dw, 'se': self._fwd_se, 'pool': self._fwd_pool, 'copy': self._fwd_copy,
                'add': self._fwd_add, 'concat': self._fwd_concat}
        for v in self.values:
            if v.kind in emit:
                emit[v.kind](v)

    @staticmethod
    def _y(v):
        return None if v.storage is None else P(v.storage, v.c_off)

    def _fwd_conv(self, v):
        # blocks with neither BN nor activation: the conv epilogue writes the block output itself
        fused_stats = self._fwd_stem_conv(v) if v.src.kind == 'input' else self._fwd_gemm_conv(v)
        if not v.plain:
            self._fwd_bn_act(v, fused_stats)

    def _fused_stats(self, v, d, rows_query):
        """BatchNorm statistics ride in the conv epilogue: per-tile partial sums into the shared workspace.  Returns the number of
        partial rows conv `d` of block `v` will leave there (0: a yh_bn_stats pass takes them)."""
        rows = int(rows_query(C.byref(d))) if v.bn is not None and not v.plain else 0
        if rows:
            d.stats_ws_floats = rows * 2 * v.c_phys
            self._needs_ws(d.stats_ws_floats)
        return rows

    def _fwd_stem_conv(self, v):
        pk, s, direct, lib = v.tpack, v.src, v.plain, self.lib
        d = StemDesc(x=None, w=P(pk['w']), bias=P(pk['b']), y=self._y(v) if direct else P(v.z), n=self.N, cin=s.C, h=s.H,
                     w_in=s.W, ho=v.Ho, wo=v.Wo, cout=v.c_phys, cout_pad=pk['cout_pad'], kh=v.k, kw=v.k,
                     stride=v.stride, pad=v.pad, ldy=v.ld if direct else v.c_phys, act=LINEAR, slope=0.0,
                     dtype=self.code, out_scale=0.0)
        if v.c_phys > pk['cout_pad'] or v.fp32:
            raise NotImplementedError('HIP training path: stem geometry')
        # the MFMA first-layer kernel also emits the BatchNorm partial sums of what it stores (no yh_bn_stats pass)
        fused_stats = self._fused_stats(v, d, lib.yh_conv2d_stem_stats_rows) if os.environ.get('YOLO_HIP_STEM_STATS', '1') != '0' else 0
        op = self._add('fwd', d, 'stem%d' % v.block)
        self._fixup('fwd', op, StemDesc, 'x', SLOT_INPUT)
        if fused_stats:
            self._fixup('fwd', op, StemDesc, 'stats_ws', SLOT_WS)
        return fused_stats

    def _fwd_gemm_conv(self, v):
        pk, s, direct, lib = v.tpack, v.src, v.plain, self.lib
        d = ConvDesc(x=P(s.storage, s.c_off), w=P(pk['w']), bias=P(pk['b']), res=None,
                     y=None if v.fp32 else (self._y(v) if direct else P(v.z)), n=self.N, h=s.H, w_in=s.W, cin=s.c_phys,
                     ho=v.Ho, wo=v.Wo, cout=v.c_phys, kh=v.k, kw=v.k, stride=v.stride, pad=v.pad, ldx=s.ld,
                     ldr=0, ldy=v.c_phys if (v.fp32 or not direct) else v.ld, cin_k=pk['cin_k'],
                     m_pad=pk['m_pad'], act=LINEAR, slope=0.0, ups=1, out_f32=1 if v.fp32 else 0,
                     dtype=self.code, tile=self.eng.force_tile, acc_scale=0.0, out_scale=0.0)
        fused_stats = self._fused_stats(v, d, lib.yh_conv2d_stats_rows)
        op = self._add('fwd', d, 'conv%d' % v.block)
        if fused_stats:
            self._fixup('fwd', op, ConvDesc, 'stats_ws', SLOT_WS)
        if v.fp32:
            self._fixup('fwd', op, ConvDesc, 'y', SLOT_HEAD0 + self.head_index[id(v)])
        return fused_stats

    def _bn_args(self, v, bn):
        """The BatchNorm fields the statistics, finalize, activation and backward descriptors share, after validating the module."""
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError('HIP training path: BatchNorm without momentum / running stats / affine')
        for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise NotImplementedError('HIP training path: BatchNorm tensors must be contiguous fp32')
        saved, stats = self.saved, self.stats
        return dict(gamma=P(bn.weight), beta=P(bn.bias), mean=saved.ptr(v.s_mean), invstd=saved.ptr(v.s_invstd),
                    sum=stats.ptr(v.s_sum), sumsq=stats.ptr(v.s_sumsq), eps=float(bn.eps), momentum=float(bn.momentum))

    def _fwd_bn_act(self, v, fused_stats):
        """z -> y of a conv or dw block: batch statistics (unless the conv left them as ``fused_stats`` partial rows), finalize,
        y = act(bn(z)) [+ residual] [2x store]."""
        bn, what = v.bn, v.block
        base = dict(z=P(v.z), pixels=self.N * v.Ho * v.Wo, n=self.N, h=v.Ho, w_in=v.Wo, c=v.c_phys, ldz=v.c_phys, act=v.act,
                    slope=v.slope, dtype=self.code, ups=v.ups)
        bnp = dict()
        if bn is not None:
            bnp = self._bn_args(v, bn)
            if not fused_stats:
                self._add_reduction('fwd', BnStatsDesc(**base, **bnp), 'bnstat%d' % what)
            fin = BnFinalizeDesc(**base, **bnp, running_mean=P(bn.running_mean), running_var=P(bn.running_var),
                                 nparts=fused_stats, ws_floats=fused_stats * 2 * v.c_phys)
            op = self._add('fwd', fin, 'bnfin%d' % what)
            if fused_stats:
                self._fixup('fwd', op, BnFinalizeDesc, 'ws', SLOT_WS)
        v.bn_args = (base, bnp)
        self._add('fwd', BnActFwdDesc(**base, **bnp, out=self._y(v), ldo=v.ld, res=None if v.res is None else P(v.res.storage, v.res.c_off),
                                      ldr=0 if v.res is None else v.res.ld), 'bnact%d' % what)

    def _fwd_dw(self, v):
        s, pk = v.src, v.tpack
        self._add('fwd', DwDesc(x=P(s.storage, s.c_off), w=P(pk['w']), bias=P(pk['b']), y=self._y(v) if v.plain else P(v.z), n=self.N,
                                h=s.H, w_in=s.W, c=s.c_phys, ho=v.H, wo=v.W, k=v.k, stride=v.stride, pad=v.pad, ldx=s.ld,
                                ldy=v.ld if v.plain else v.c_phys, act=LINEAR, slope=0.0, dtype=self.code), 'dw%d' % v.block)
        if not v.plain:
            self._fwd_bn_act(v, 0)

    def _fwd_se(self, v):
        s = v.src
        self._add('fwd', SeDesc(x=P(s.storage, s.c_off), y=self._y(v), w1=P(v.fc1.weight), w2=P(v.fc2.weight), pooled=P(v.pooled),
                                gate=P(v.gate), ch_map=None, n=self.N, h=s.H, w_in=s.W, c=v.C, c_phys=v.c_phys, cr=v.fc1.weight.shape[0],
                                ldx=s.ld, ldy=v.ld, dtype=self.code), 'se%d' % v.block)

    def _fwd_pool(self, v):
        s = v.src
        self._add('fwd', PoolDesc(x=P(s.storage, s.c_off), y=self._y(v), n=self.N, h=s.H, w_in=s.W, c=s.c_phys, ho=v.H, wo=v.W,
                                  k=v.k, stride=v.stride, pad_lo=v.pad_lo, edge_zero=v.edge_zero, ldx=s.ld,
                                  ldy=v.ld, dtype=self.code), 'pool%d' % v.block)

    def _fwd_copy(self, v):
        s = v.src
        self._add('fwd', CopyDesc(x=P(s.storage, s.c_off), y=self._y(v), n=self.N, h=s.H, w_in=s.W, c=s.c_phys, ups=v.ups,
                                  ldx=s.ld, ldy=v.ld, dtype=self.code), 'ups%d' % v.block)

    def _fwd_add(self, v):
        self._add('fwd', AddDesc(a=P(v.a.storage, v.a.c_off), b=P(v.b.storage, v.b.c_off), y=self._y(v),
                                 pixels=self.N * v.H * v.W, c=v.c_phys, lda=v.a.ld, ldb=v.b.ld, ldy=v.ld,
                                 dtype=self.code), 'add%d' % v.block)

    def _fwd_concat(self, v):
        for s, off, inplace in v.parts:
            if not inplace:
                self._add('fwd', CopyDesc(x=P(s.storage, s.c_off), y=P(v.storage, v.c_off + off), n=self.N, h=s.H,
                                          w_in=s.W, c=s.c_phys, ups=1, ldx=s.ld, ldy=v.ld, dtype=self.code), 'cat%d' % v.block)

    # --------------------------------------------------------------------------------- pass 3: backward ops
    def emit_backward(self):
        plan, values = self.plan, self.values
        if self.attention:
            # Feature distillation injects into the gradient of every feature value BEFORE the first backward op runs (one place:
            # backward_segment of the last range).  So these buffers start as zeros and every contribution accumulates - also the
            # ones that would otherwise have been the first, full-width write; a concat buffer one of them is produced into is zeroed
            # as a whole, and the injection touches that value's lanes only.  The fusions that take a block's BatchNorm backward sums
            # while completing its dy (_completes_bn_block) stay on: they reduce the values they STORE, residual accumulate
            # included, and the injection is already part of what they accumulate onto.
            plan['kd_values'] = self.eng._attention_values(self.outs)
            for u in plan['kd_values']:
                if id(u.gstorage) not in self.initialised:
                    self.initialised.add(id(u.gstorage))
                    plan['zero_list'].append(u.gstorage)
        # gradient buffers addressed by more than one value (a concat and the parts produced into it, a tensor and its channel
        # slices): the residual-gradient aliasing in _bwd_conv_dy re-points ONE value's buffer and must leave these alone
        for u in values:
            if getattr(u, 'gstorage', None) is not None:
                self.holders[id(u.gstorage)] = self.holders.get(id(u.gstorage), 0) + 1
        emit = {'conv': self._bwd_conv, 'dw': self._bwd_dw, 'se': self._bwd_se, 'pool': self._bwd_pool, 'copy': self._bwd_copy,
                'add': self._bwd_add, 'concat': self._bwd_concat}
        for v in reversed(values):
            self.bwd_pos[id(v)] = len(plan['bwd_ops'])
            if v.kind in ('input', 'slice'):
                continue   # contributions to a slice were written straight into the source's gradient buffer
            if v.kind not in emit:
                raise NotImplementedError('HIP training path: backward of %s' % v.kind)
            if self._has_grad(v):      # else a dead branch: its parameters get zero gradients
                emit[v.kind](v)

    def _completes_bn_block(self, v, s):
        """conv `v` (1x1 / stride 1) writes the last contribution to grad(s), s a conv with BatchNorm whose gradient buffer is its own.
        When the library can run v's data gradient on its persistent kernel, the backward sums of s (sum g, sum g xhat) can then be
        taken by that very launch - it has the finished dy rows in registers and reads z on top - instead of by a reduction pass
        over dy and z (yh_conv_desc.bwd_z, round 6; YOLO_HIP_FUSE_DBN=0 switches it off)."""
        if not self.fuse_dbn or v.k != 1 or v.stride != 1 or v.pad != 0 or s.kind != 'conv' or s.bn is None or s.plain or s.fp32 or s.ups != 1:
            return False
        if s.src.kind == 'input' or getattr(s, 'parent', None) is not None or s.c_off != 0 or s.ld != s.c_phys:
            return False
        if getattr(s, 'z', None) is None or not hasattr(s, 'bn_args'):
            return False
        return min(self.index[id(u)] for u in self.consumers.get(id(s), [v])) == self.index[id(v)]

    def contribution_mode(self, t, full_width, what):
        """How op `what` enters grad(t): 'write' (the first writer, covering the buffer) or 'acc'.  Every writer of a gradient buffer
        asks here, so this is where a write into a sealed buffer is caught."""
        key = id(t.gstorage)
        if key in self.sealed:
            raise RuntimeError('%s writes the gradient buffer of block %d after a data gradient took its BatchNorm backward sums'
                               % (what, self.sealed[key].block))
        if key in self.initialised:
            return 'acc'
        self.initialised.add(key)
        if full_width and t.c_off == 0 and t.ld == t.c_phys:
            return 'write'
        self.plan['zero_list'].append(t.gstorage)
        return 'acc'

    @staticmethod
    def _gptr(t):
        return P(t.gstorage, t.c_off)

    def _has_grad(self, t):
        return t.fp32 or id(t.gstorage) in self.initialised

    def _contribute(self, t, src_ptr, src_ld, what):
        """grad(t) (+)= rows at src_ptr (same spatial size and channel count as t)."""
        g = self._gptr(t)
        if self.contribution_mode(t, True, what) == 'write':
            self._add('bwd', CopyDesc(x=src_ptr, y=g, n=self.N, h=t.H, w_in=t.W, c=t.c_phys, ups=1, ldx=src_ld,
                                      ldy=t.ld, dtype=self.code), what)
        else:
            self._add('bwd', AddDesc(a=g, b=src_ptr, y=g, pixels=self.N * t.H * t.W, c=t.c_phys, lda=t.ld,
                                     ldb=src_ld, ldy=t.ld, dtype=self.code), what)

    def _bwd_concat(self, v):
        for s, off, inplace in v.parts:
            if not inplace:
                self._contribute(s, P(v.gstorage, v.c_off + off), v.ld, 'dcat%d' % v.block)

    def _bwd_add(self, v):
        self._contribute(v.a, self._gptr(v), v.ld, 'dadd%d' % v.block)
        self._contribute(v.b, self._gptr(v), v.ld, 'dadd%d' % v.block)

    def _bwd_se(self, v):
        s, grads, what = v.src, self.grads, 'dse%d' % v.block
        mode = self.contribution_mode(s, True, what)
        self._add('bwd', SeBwdDesc(x=P(s.storage, s.c_off), dy=self._gptr(v), dx=self._gptr(s), w1=P(v.fc1.weight), w2=P(v.fc2.weight),
                                   pooled=P(v.pooled), gate=P(v.gate), dw1=grads.ptr(v.g_w1), dw2=grads.ptr(v.g_w2), scratch=P(v.scratch),
                                   scratch2=P(v.scratch2), scratch2_floats=v.scratch2.numel(),
                                   n=self.N, h=s.H, w_in=s.W, c=v.c_phys, cr=v.fc1.weight.shape[0], ldx=s.ld, lddy=v.ld, lddx=s.ld,
                                   accumulate=1 if mode == 'acc' else 0, dtype=self.code), what)

    def _bias_or_junk_sums(self, v):
        """Where the two backward sums of a block without BatchNorm go: sum dz is the conv-bias gradient (z already holds the bias)."""
        junk = self._junk(v.c_phys)
        return dict(sum=self.grads.ptr(v.g_b if v.g_b is not None else junk), sumsq=self.grads.ptr(junk))

    def _bwd_dw(self, v):
        s, pk, grads, N = v.src, v.tpack, self.grads, self.N
        dyp, lddy = self._gptr(v), v.ld
        if v.plain:
            dzp, lddz = dyp, lddy
        else:
            dzp, lddz = P(self.dz_buf), v.c_phys
            base, bnp = v.bn_args
            acc = dict(bnp, sum=grads.ptr(v.g_beta), sumsq=grads.ptr(v.g_gamma)) if v.bn is not None else self._bias_or_junk_sums(v)
            self._add_reduction('bwd', BnBwdReduceDesc(**base, **acc, dy=dyp, lddy=lddy), 'dbn%d' % v.block)
            self._add('bwd', BnBwdApplyDesc(**base, **acc, dy=dyp, lddy=lddy, out=dzp, ldo=v.c_phys), 'dbnx%d' % v.block)
        geo = dict(n=N, h=s.H, w_in=s.W, c=v.c_phys, ho=v.H, wo=v.W, k=v.k, stride=v.stride, pad=v.pad, ldx=s.ld, lddz=lddz,
                   dtype=self.code)
        self._add_reduction('bwd', DwWgradDesc(x=P(s.storage, s.c_off), dz=dzp, dw=grads.ptr(v.g_w), lddx=0, accumulate=0, **geo),
                            'dwwgrad%d' % v.block)
        if s.kind != 'input':
            mode = self.contribution_mode(s, True, 'dwdgrad%d' % v.block)
            self._add('bwd', DwDgradDesc(dz=dzp, w=P(pk['w']), dx=self._gptr(s), lddx=s.ld,
                                         accumulate=1 if mode == 'acc' else 0, **geo), 'dwdgrad%d' % v.block)

    def _bwd_pool(self, v):
        s = v.src
        self.contribution_mode(s, False, 'dpool%d' % v.block)   # scatter-add: the target must hold zeros or an earlier contribution
        self._add('bwd', PoolBwdDesc(x=P(s.storage, s.c_off), dy=self._gptr(v), dx=self._gptr(s), n=self.N, h=s.H, w_in=s.W, c=s.c_phys,
                                     ho=v.H, wo=v.W, k=v.k, stride=v.stride, pad_lo=v.pad_lo, edge_zero=v.edge_zero, ldx=s.ld, lddy=v.ld,
                                     lddx=s.ld, dtype=self.code), 'dpool%d' % v.block)

    def _bwd_copy(self, v):
        s, what = v.src, 'dups%d' % v.block
        geo = dict(n=self.N, h=s.H, w_in=s.W, c=s.c_phys, big_h=2 * s.H, big_w=2 * s.W, ldx=v.ld, dtype=self.code)
        if self.contribution_mode(s, True, what) == 'write':
            self._add('bwd', UpsampleBwdDesc(x=self._gptr(v), y=self._gptr(s), ldy=s.ld, **geo), what)
        else:
            tmp = self._alloc((self.N, s.H, s.W, s.c_phys))
            self._add('bwd', UpsampleBwdDesc(x=self._gptr(v), y=P(tmp), ldy=s.c_phys, **geo), what)
            self._add('bwd', AddDesc(a=self._gptr(s), b=P(tmp), y=self._gptr(s), pixels=self.N * s.H * s.W, c=s.c_phys,
                                     lda=s.ld, ldb=s.c_phys, ldy=s.ld, dtype=self.code), what)

    # ---- backward of a conv block: head cast and bias | upsample and residual | BatchNorm / activation | weight gradient | data gradient
    def _bwd_conv(self, v):
        if v.fp32:
            dz = self._bwd_conv_head(v)
        else:
            dyp, lddy = self._bwd_conv_dy(v)
            dz = self._bwd_conv_bn_act(v, dyp, lddy)
        if dz is None:
            return      # the one-pass first block: its weight gradient is taken, it has no data gradient
        dzp, lddz = dz
        if v.src.kind == 'input':
            self._wgrad_image(v, dzp, lddz)
        else:
            self._wgrad(v, dzp, lddz)
            self._dgrad(v, dzp, lddz)

    def _bias_grad(self, v, dzp, lddz):
        """Conv-bias gradient of a block without BatchNorm and activation = sum over pixels of dz."""
        self._add_reduction('bwd', BnBwdReduceDesc(z=dzp, dy=dzp, pixels=self.N * v.Ho * v.Wo, n=self.N, h=v.Ho, w_in=v.Wo, c=v.c_phys,
                                                   ldz=lddz, lddy=lddz, act=LINEAR, slope=0.0, dtype=self.code, ups=1,
                                                   sum=self.grads.ptr(v.g_b), sumsq=self.grads.ptr(self._junk(v.c_phys))),
                            'dbias%d' % v.block)

    def _bwd_conv_head(self, v):
        """Head: fp32 gradient from autograd -> dtype, and the bias gradient."""
        dzp = P(self.dz_buf)
        op = self._add('bwd', CastDesc(x=None, y=dzp, pixels=self.N * v.Ho * v.Wo, c=v.c_phys, ldx=v.c_phys, ldy=v.c_phys,
                                       dtype=self.code), 'dhead%d' % v.block)
        self._fixup('bwd', op, CastDesc, 'x', SLOT_HEAD0 + self.head_index[id(v)])
        if v.g_b is not None:
            self._bias_grad(v, dzp, v.c_phys)
        return dzp, v.c_phys

    def _owns_gstorage(self, u):
        return u.parent is None and u.c_off == 0 and u.ld == u.c_phys and self.holders.get(id(u.gstorage), 0) == 1

    def _bwd_conv_dy(self, v):
        """dy of the block's own output: through a fused 2x upsample, and on to the source of a fused residual.  Returns (dy, lddy)."""
        dyp, lddy = self._gptr(v), v.ld
        if v.ups == 2:
            small = self._alloc((self.N, v.Ho, v.Wo, v.c_phys))
            self._add('bwd', UpsampleBwdDesc(x=dyp, y=P(small), n=self.N, h=v.Ho, w_in=v.Wo, c=v.c_phys, big_h=2 * v.Ho, big_w=2 * v.Wo,
                                             ldx=lddy, ldy=v.c_phys, dtype=self.code), 'dups%d' % v.block)
            dyp, lddy = P(small), v.c_phys
        t = v.res
        if t is not None:
            if (id(t.gstorage) not in self.initialised and v.ups == 1 and self._owns_gstorage(t) and self._owns_gstorage(v) and not t.fp32
                    and (t.H, t.W, t.c_phys) == (v.H, v.W, v.c_phys) and not getattr(t, 'galias', False)):
                # first contribution to the residual source is dy itself: share the buffer instead of copying it.
                # Later contributions (the data gradient of the source's other consumer) accumulate in place, after
                # this block's backward has consumed dy.
                plan = self.plan
                plan['storages'] = [u for u in plan['storages'] if u is not t.gstorage]   # free the unused buffer
                t.gstorage, t.galias = v.gstorage, True
            else:
                self._contribute(t, dyp, lddy, 'dres%d' % v.block)
        return dyp, lddy

    def _bwd_conv_bn_act(self, v, dyp, lddy):
        """dy -> dz and the gradients of gamma / beta (or of the conv bias).  Returns (dz, lddz), or None when the one-pass first
        block took the weight gradient along."""
        if v.plain:                   # no BN, linear: dz is dy itself
            if v.g_b is not None:
                self._bias_grad(v, dyp, lddy)
            return dyp, lddy
        base, bnp = v.bn_args
        base = dict(base, ups=1)
        if v.src.kind == 'input' and self._stem_bwd_fused(v, v.src):
            self._bwd_first_block(v, base, bnp, dyp, lddy)
            return None
        acc = dict(bnp, sum=self.grads.ptr(v.g_beta), sumsq=self.grads.ptr(v.g_gamma)) if v.bn is not None else self._bias_or_junk_sums(v)
        dzp = P(self.dz_buf)
        if getattr(v, 'dbn_done', False):
            # the launch that completed dy took the sums (_dgrad_plain); dy is consumed below, so its buffer may be written again
            del self.sealed[id(v.gstorage)]
        else:
            self._add_reduction('bwd', BnBwdReduceDesc(**base, **acc, dy=dyp, lddy=lddy), 'dbn%d' % v.block)
        self._add('bwd', BnBwdApplyDesc(**base, **acc, dy=dyp, lddy=lddy, out=dzp, ldo=v.c_phys), 'dbnx%d' % v.block)
        return dzp, v.c_phys

    def _bwd_first_block(self, v, base, bnp, dyp, lddy):
        """First block: BatchNorm backward + weight gradient as ONE pass over dy and z (csrc/stem_bwd.hip) - its dz has no other
        reader (no data gradient into the image), so it is never written."""
        s, grads = v.src, self.grads
        sd = StemBwdDesc(x=None, dy=dyp, z=base['z'], gamma=bnp['gamma'], beta=bnp['beta'], mean=bnp['mean'],
                         invstd=bnp['invstd'], dgamma=grads.ptr(v.g_gamma), dbeta=grads.ptr(v.g_beta),
                         dw=grads.ptr(v.g_w), n=self.N, cin=s.C, h=s.H, w_in=s.W, cout=v.c_phys, lddy=lddy,
                         ldz=v.c_phys, act=v.act, slope=v.slope)
        fused_dgrad = getattr(v, 'fused_dgrad', None)
        for key, val in (fused_dgrad or {}).items():
            setattr(sd, key, val)
        need = int(self.lib.yh_stem_bwd_workspace(C.byref(sd)))
        if need <= 0:
            raise RuntimeError('yh_stem_bwd_workspace rejected a geometry _stem_bwd_fused accepted')
        sd.ws_floats = need
        self._needs_ws(need)
        op = self._add('bwd', sd, ('stembwd_dgrad%d' if fused_dgrad else 'stembwd%d') % v.block)
        self._fixup('bwd', op, StemBwdDesc, 'ws', SLOT_WS)
        self._fixup('bwd', op, StemBwdDesc, 'x', SLOT_INPUT)

    def _wgrad_image(self, v, dzp, lddz):
        """First layer: the image as NHWC dtype with 8 channels (3..7 zero), so that it uses the MFMA wgrad kernel."""
        s, N = v.src, self.N
        img = self._alloc((N, s.H, s.W, ALIGN_C))
        op = self._add('bwd', LayoutDesc(x=None, y=P(img), n=N, c=s.C, h=s.H, w_in=s.W, c_pad=ALIGN_C, ldy=ALIGN_C,
                                         dtype=self.code), 'image%d' % v.block)
        self._fixup('bwd', op, LayoutDesc, 'x', SLOT_INPUT)
        self._add_reduction('bwd', WgradDesc(x=P(img), dz=dzp, dw=self.grads.ptr(v.g_w), n=N, h=s.H, w_in=s.W, cin=ALIGN_C, ho=v.Ho,
                                             wo=v.Wo, cout=v.C, kh=v.k, kw=v.k, stride=v.stride, pad=v.pad, ldx=ALIGN_C, lddz=lddz,
                                             dtype=self.code, splits=0, cin_w=s.C), 'wgrad%d' % v.block)

    def _wgrad(self, v, dzp, lddz):
        s = v.src
        self._add_reduction('bwd', WgradDesc(x=P(s.storage, s.c_off), dz=dzp, dw=self.grads.ptr(v.g_w), n=self.N, h=s.H, w_in=s.W,
                                             cin=s.C, ho=v.Ho, wo=v.Wo, cout=v.C, kh=v.k, kw=v.k, stride=v.stride, pad=v.pad, ldx=s.ld,
                                             lddz=lddz, dtype=self.code, splits=0), 'wgrad%d' % v.block)

    def _dgrad(self, v, dzp, lddz):
        """grad(src) (+)= conv(dz, W^T flipped), as yh_conv2d_fwd on the data-gradient weight image, in one of four forms."""
        s, pk, force_tile = v.src, v.tpack, self.eng.force_tile
        mode = self.contribution_mode(s, True, 'dgrad%d' % v.block)
        g = self._gptr(s)
        common = dict(x=dzp, res=g if mode == 'acc' else None, y=g, h=v.Ho, w_in=v.Wo,
                      bias=P(self.zero_bias), n=self.N, cin=v.c_phys, cout=s.c_phys, stride=1, ldx=lddz, ldr=s.ld if mode == 'acc' else 0,
                      ldy=s.ld, cin_k=pk['cout_k'], m_pad=pk['dm_pad'], act=LINEAR, slope=0.0, out_f32=0, dtype=self.code,
                      tile=force_tile if force_tile < 40 else 0, acc_scale=0.0, out_scale=0.0)
        if pk.get('stem_fused'):
            self._dgrad_in_first_block(v, mode, dzp, lddz)
        elif v.stride == 2 and 'wt_fused' in pk:
            self._dgrad_four_phase(v, common)
        elif v.stride == 2:
            self._dgrad_parity(v, common)
        else:
            self._dgrad_plain(v, common)

    def _dgrad_in_first_block(self, v, mode, dzp, lddz):
        """No launch: the first block's backward computes this data gradient from dz on the fly (yh_stem_bwd dz1 / w1) and
        never materialises it.  dz stays valid until then: the first block writes no dz of its own."""
        if mode != 'write':
            raise RuntimeError('fused first-block data gradient must be the only contribution to its gradient')
        pk = v.tpack
        v.src.fused_dgrad = dict(dz1=dzp, lddz1=lddz, w1=P(pk['wt']), h1=v.Ho, w1_in=v.Wo, k1=v.c_phys, k1_pad=pk['cout_k'])

    def _dgrad_four_phase(self, v, common):
        """Stride 2, few input channels: all four parity phases as one 2x2-tap pass (ups = 4, see _reserve_conv)."""
        s, pk = v.src, v.tpack
        if self.zero_bias.numel() < pk['fused_m_pad']:
            raise RuntimeError('zero bias row is shorter than the fused data-gradient image')
        fused = dict(common, cout=4 * s.c_phys, m_pad=pk['fused_m_pad'])
        self._add('bwd', ConvDesc(w=P(pk['wt_fused']), ho=(s.H + 1) // 2, wo=(s.W + 1) // 2, kh=2, kw=2, pad=0, ups=4, y_h=s.H, y_w=s.W, **fused),
                  'dgrad%d' % v.block)

    def _dgrad_parity(self, v, common):
        """Stride 2: input pixels of parity (a, b) only see the taps r = a + pad - 2t, s = b + pad - 2u: four small correlations
        of dz scattered onto every other pixel, 9 tap-GEMMs in total (a dilated pass runs 36)."""
        s, pk = v.src, v.tpack
        for (a, b), (th, tw), img in zip(_PHASES, pk['phase_taps'], pk['wt_phase']):
            hp, wp = (s.H - a + 1) // 2, (s.W - b + 1) // 2
            if hp > 0 and wp > 0:
                self._add('bwd', ConvDesc(w=P(img), ho=hp, wo=wp, kh=th, kw=tw, pad=0, ups=3, y_h=s.H, y_w=s.W, y_off_h=a, y_off_w=b,
                                          **common), 'dgrad%d' % v.block)

    def _dgrad_plain(self, v, common):
        """Stride 1.  When it completes the dy of BatchNorm block `s` (_completes_bn_block), the launch also leaves the rows of s's
        backward sums in the shared workspace; they are added into dbeta / dgamma of `s` right away (the workspace is free game
        for the next op), s's own backward then starts at its apply pass, and grad(s) is sealed until it has."""
        s, pk = v.src, v.tpack
        dg = ConvDesc(w=P(pk['wt']), ho=s.H, wo=s.W, kh=v.k, kw=v.k, pad=v.k - 1 - v.pad, ups=1, **common)
        rows = 0
        if self._completes_bn_block(v, s):
            sbase, sbnp = s.bn_args
            for key, val in dict(bwd_z=sbase['z'], bwd_ldz=s.c_phys, bwd_act=s.act, bwd_slope=s.slope, bwd_gamma=sbnp['gamma'],
                                 bwd_beta=sbnp['beta'], bwd_mean=sbnp['mean'], bwd_invstd=sbnp['invstd']).items():
                setattr(dg, key, val)
            rows = int(self.lib.yh_conv2d_bwd_stats_rows(C.byref(dg)))
            if rows <= 0:
                for key in ('bwd_z', 'bwd_gamma', 'bwd_beta', 'bwd_mean', 'bwd_invstd'):
                    setattr(dg, key, None)
        if rows > 0:
            dg.stats_ws_floats = rows * 2 * s.c_phys
            self._needs_ws(dg.stats_ws_floats)
        op = self._add('bwd', dg, 'dgrad%d' % v.block)
        if rows > 0:
            self._fixup('bwd', op, ConvDesc, 'stats_ws', SLOT_WS)
            sacc = dict(sbnp, sum=self.grads.ptr(s.g_beta), sumsq=self.grads.ptr(s.g_gamma))
            self._add_reduction('bwd', BnBwdReduceDesc(**dict(sbase, ups=1), **sacc, dy=self._gptr(s), lddy=s.ld, nparts=rows),
                                'dbn%d' % s.block)
            s.dbn_done = True
            self.sealed[id(s.gstorage)] = s

    # --------------------------------------------------------------------------------- layout
    def _finish(self):
        plan, N = self.plan, self.N
        plan['head_shapes'] = [(N, h.src.H, h.src.W, h.src.c_phys) for h in self.heads]
        plan['segments'] = self.eng._make_segments(plan, self.values, self.heads, self.bwd_pos)
        if self.attention:
            self._reserve_attention(plan['kd_values'])
        plan['ws'] = self._alloc((max(plan['ws_floats'], 4),), fp32=True)
        # place the pieces that are still in use (the residual-gradient aliasing dropped some) and turn every pointer into
        # them into a fixup on the arena slot: the plan holds offsets, `_bind` gives it the arena's address
        need = 0
        for t in plan['storages']:
            t.off = need
            need += _round_up(t.nbytes(), ARENA_ALIGN)
        plan['arena_need'] = need
        for handle, op, field, index, inner, what in plan['arena_refs']:
            t = self.pieces[index]
            if t.off is None or inner >= max(t.nbytes(), 1):
                raise RuntimeError('%s points into a step buffer the plan does not keep' % what)
            hiplib.check(self.lib.yh_plan_add_fixup(handle, op, field, SLOT_ARENA, t.off + inner), 'fixup')
        del plan['arena_refs']
        # what stays per plan: statistics, saved, gradient arenas, pack table, zero bias row and the weight images
        return plan

    def _reserve_attention(self, feats):
        """Maps, G = p_s - p_t and the KL row partials are pieces of the step arena like every other step buffer: a reservation
        over all shapes covers them (train_stats' arena_bytes), the two tables are the plan's own (plan_bytes)."""
        from . import kd
        plan, N, keep = self.plan, self.N, self._keep
        total = sum(N * u.H * u.W for u in feats)
        sink = plan['kd_sink'] = kd.KdSink()
        sink.lib = self.lib
        raw, sink.n_kl_rows = kd.kl_rows([(N, u.H, u.W) for u in feats])
        plan['kd_maps'], plan['kd_G'] = self._alloc((total,), fp32=True), self._alloc((total,), fp32=True)
        plan['kd_partials'] = self._alloc((max(sink.n_kl_rows, 4),), fp32=True)
        sink.kl_table = keep(len(raw), torch.uint8)
        sink.kl_table.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        plan['kd_table'] = keep(len(feats) * C.sizeof(hiplib.KdRow), torch.uint8, zero=True)
        plan['kd_one'] = keep(1, torch.float32, zero=True).fill_(1.0)
