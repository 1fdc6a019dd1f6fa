"""The shared library must load without a GPU and export exactly the C ABI that include/yolo_hip.h declares."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from engine import hiplib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, 'include', 'yolo_hip.h')


def _declared():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(yh_[a-z0-9_]+)\s*\(', text)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = hiplib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), 'libyolo_hip.so does not export ' + n
    assert sorted(hiplib.EXPORTS) == names, 'ctypes binding and header disagree'
    assert lib.yh_abi_version() == hiplib.ABI_VERSION
    assert b'misaligned' in lib.yh_error_string(-2)


def test_struct_layout_matches_c_compiler(tmp_path):
    """ctypes mirrors must have the C compiler's sizeof/offsetof (gcc, no GPU needed)."""
    structs = {'yh_conv_desc': hiplib.ConvDesc, 'yh_stem_desc': hiplib.StemDesc, 'yh_pool_desc': hiplib.PoolDesc,
               'yh_copy_desc': hiplib.CopyDesc, 'yh_add_desc': hiplib.AddDesc, 'yh_decode_desc': hiplib.DecodeDesc,
               'yh_dw_desc': hiplib.DwDesc, 'yh_se_desc': hiplib.SeDesc, 'yh_qcopy_desc': hiplib.QCopyDesc,
               'yh_qadd_desc': hiplib.QAddDesc, 'yh_letterbox_desc': hiplib.LetterboxDesc, 'yh_mosaic_desc': hiplib.MosaicDesc,
               'yh_stem_bwd_desc': hiplib.StemBwdDesc, 'yh_wgrad_desc': hiplib.WgradDesc, 'yh_bn_desc': hiplib.BnDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolo_hip.h"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(REPO, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, '%s.%s' % (cname, fname)


def test_plan_api_runs_without_gpu():
    """Plan bookkeeping is host code: create/add/fixup/destroy work on a machine without a GPU."""
    lib = hiplib.load()
    h = lib.yh_plan_create()
    assert h
    d = hiplib.CopyDesc(n=1, h=2, w_in=2, c=8, ups=1, ldx=8, ldy=8, dtype=0)
    idx = lib.yh_plan_add(h, hiplib.OP_COPY, C.byref(d), C.sizeof(d))
    assert idx == 0 and lib.yh_plan_num_ops(h) == 1
    assert lib.yh_plan_add(h, hiplib.OP_COPY, C.byref(d), 4) == -1  # wrong size is rejected
    assert lib.yh_plan_add_fixup(h, 0, hiplib.CopyDesc.x.offset, 0, 0) == 0
    assert lib.yh_plan_add_fixup(h, 5, 0, 0, 0) == -5  # YH_ERANGE
    assert lib.yh_plan_run(h, None) == -1  # unbound slot -> YH_EINVAL, nothing launched
    # the scheduling hints of ABI 2 (accepted and ignored): on a two-op plan they still answer what they always answered
    assert lib.yh_plan_add(h, hiplib.OP_COPY, C.byref(d), C.sizeof(d)) == 1 and lib.yh_plan_num_ops(h) == 2
    EINVAL, ERANGE = -1, -5
    assert [lib.yh_plan_set_lane(h, op, lane) for op in (0, 1) for lane in (0, 1)] == [0] * 4
    assert lib.yh_plan_add_dep(h, 1, 0) == 0 and lib.yh_plan_set_async_reduce(h, 1) == 0 and lib.yh_plan_set_async_reduce(h, 0) == 0
    assert lib.yh_plan_set_lane(h, 2, 1) == ERANGE and lib.yh_plan_set_lane(h, -1, 0) == ERANGE     # op index past the end
    assert lib.yh_plan_set_lane(h, 0, 2) == ERANGE and lib.yh_plan_set_lane(h, 0, -1) == ERANGE     # no such lane
    assert lib.yh_plan_add_dep(h, 2, 0) == ERANGE                                                   # op index past the end
    assert lib.yh_plan_add_dep(h, 1, 1) == ERANGE and lib.yh_plan_add_dep(h, 0, 0) == ERANGE        # dep == op
    assert lib.yh_plan_add_dep(h, 1, 2) == ERANGE and lib.yh_plan_add_dep(h, 1, -1) == ERANGE       # dep past the end
    assert lib.yh_plan_set_lane(None, 0, 1) == EINVAL and lib.yh_plan_add_dep(None, 1, 0) == EINVAL
    assert lib.yh_plan_set_async_reduce(None, 1) == EINVAL
    assert lib.yh_plan_num_ops(h) == 2 and lib.yh_plan_run(h, None) == -1                           # and they changed nothing
    lib.yh_plan_destroy(h)


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(hiplib, '_lib', None)
    monkeypatch.setattr(hiplib, 'LIB_PATH', '/nonexistent/libyolo_hip.so')
    with pytest.raises(hiplib.HipLibraryError):
        hiplib.load()


def _conv(dtype, n, hw, cin, cout, k, s, res=False, stats=False, act=1):
    esz = 1 if dtype == hiplib.YH_I8 else 2
    step = 64 if dtype == hiplib.YH_I8 else 32
    ho = (hw + 2 * (k // 2) - k) // s + 1
    d = hiplib.ConvDesc(n=n, h=hw, w_in=hw, cin=cin, ho=ho, wo=ho, cout=cout, kh=k, kw=k, stride=s, pad=k // 2, ldx=cin, ldr=cout if res else 0,
                        ldy=cout, cin_k=-(-cin // step) * step, m_pad=-(-cout // 128) * 128, act=act, slope=0.1, ups=1, dtype=dtype,
                        acc_scale=1.0, out_scale=1.0)
    d.x = d.w = d.bias = d.y = 4096          # any aligned non-null address: the picker reads alignment only
    if res:
        d.res = 4096
        d.q_rx = d.q_ra = d.q_scale_x = d.q_scale_a = d.q_inv_scale_sum = 1.0
    if stats:
        d.stats_ws, d.stats_ws_floats = 4096, 1 << 40
    return d


def test_kernel_selection_on_the_headline_network():
    """Which kernel family a layer of YOLOv3-608 at batch 64 runs on (yh_conv2d_tile is host code): the few-channel layers of the
    608 / 304 stages on the streaming kernels, the 3x3 layers from 128 channels on the halo ping-pong kernel, 1x1 layers on the ring."""
    lib = hiplib.load()
    F16, I8 = hiplib.YH_F16, hiplib.YH_I8
    tile = lambda d: lib.yh_conv2d_tile(C.byref(d))
    # (dtype, hw, cin, cout, k, s, residual) -> tile code; inference forms
    expect = [((F16, 608, 32, 64, 3, 2, False), 72), ((F16, 304, 32, 64, 3, 1, True), 72), ((I8, 608, 32, 64, 3, 2, False), 72),
              ((I8, 304, 32, 64, 3, 1, True), 72), ((I8, 304, 64, 128, 3, 2, False), 72), ((I8, 152, 64, 128, 3, 1, True), 72),
              ((F16, 304, 64, 32, 1, 1, False), 71), ((I8, 152, 128, 64, 1, 1, False), 71),
              ((F16, 76, 128, 256, 3, 1, True), 43), ((F16, 38, 256, 512, 3, 1, True), 43), ((F16, 19, 512, 1024, 3, 1, True), 43),
              ((I8, 76, 128, 256, 3, 1, False), 43), ((I8, 38, 256, 512, 3, 1, True), 43), ((F16, 152, 64, 128, 3, 1, True), 43),
              # round 6 (profiles/r06_ring_tile_sweep.txt): int8 with two channel chunks AND the fused quantised shortcut is ahead on the ring
              ((I8, 76, 128, 256, 3, 1, True), 26)]
    for (dt, hw, cin, cout, k, s, res), want in expect:
        assert tile(_conv(dt, 64, hw, cin, cout, k, s, res)) == want, (dt, hw, cin, cout, k, s, res)
    # 1x1 layers of the deeper stages and the fp16 64 -> 128 stride-2 layer stay on the LDS-DMA ring / ping-pong kernels
    for d in (_conv(F16, 64, 76, 256, 128, 1, 1), _conv(F16, 64, 38, 512, 256, 1, 1), _conv(F16, 64, 304, 64, 128, 3, 2)):
        assert tile(d) not in (43, 71, 72)
    # the training forward (statistics epilogue): the streaming 3x3 kernel carries them in fp16, one partial row per wave of its launch
    d = _conv(F16, 64, 304, 32, 64, 3, 1, stats=True, act=0)
    assert tile(d) == 72 and lib.yh_conv2d_stats_rows(C.byref(d)) == 512 * 4
    d = _conv(F16, 2, 40, 32, 64, 3, 1, stats=True, act=0)        # a small grid keeps the ring kernel: rows per (128-pixel tile, wave column)
    assert tile(d) not in (72,) and lib.yh_conv2d_stats_rows(C.byref(d)) == -(-2 * 40 * 40 // 128) * 2
    # what the streaming kernels do not do is refused when asked for explicitly, not approximated
    bad = _conv(F16, 64, 304, 32, 48, 3, 1)
    bad.tile = 72
    assert lib.yh_conv2d_fwd(C.byref(bad), None) != 0


def _dgrad_descs(n, h, w, cin, cout, k, stride, pad, dtype, acc, pitch):
    """The yh_conv2d_fwd descriptor(s) engine/train_plan.py TrainPlanBuilder._dgrad emits for the data gradient of a conv layer
    (h, w, cin: its input; the gradient buffer has `pitch` x its channels when it is a slice of a concat parent) -> (form, desc)."""
    from engine import train as _train
    round_up = lambda a, b: -(-a // b) * b
    kstep = 32 if dtype == hiplib.YH_F16 else 16
    c_phys, s_phys = round_up(cout, 8), round_up(cin, 8)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    ld = pitch * s_phys
    common = dict(h=ho, w_in=wo, n=n, cin=c_phys, cout=s_phys, stride=1, ldx=c_phys, ldr=ld if acc else 0, ldy=ld,
                  cin_k=round_up(c_phys, kstep), m_pad=round_up(s_phys, 128), act=0, slope=0.0, out_f32=0, dtype=dtype, tile=0)
    if stride == 2 and 16 <= s_phys <= _train._FUSED_DGRAD_MAX_CIN and s_phys % 4 == 0:
        descs = [('fused', hiplib.ConvDesc(ho=(h + 1) // 2, wo=(w + 1) // 2, kh=2, kw=2, pad=0, ups=4, y_h=h, y_w=w,
                                           **dict(common, cout=4 * s_phys, m_pad=round_up(4 * s_phys, 128))))]
    elif stride == 2:
        descs = [('phase', hiplib.ConvDesc(ho=(h - a + 1) // 2, wo=(w - b + 1) // 2, kh=(a + pad) // 2 + 1, kw=(b + pad) // 2 + 1, pad=0, ups=3,
                                           y_h=h, y_w=w, y_off_h=a, y_off_w=b, **common))
                 for a in (0, 1) for b in (0, 1) if (h - a + 1) // 2 > 0 and (w - b + 1) // 2 > 0]
    else:
        descs = [('plain3' if k == 3 else 'plain1' if k == 1 else 'plain%d' % k,
                  hiplib.ConvDesc(ho=h, wo=w, kh=k, kw=k, pad=k - 1 - pad, ups=1, **common))]
    for _, d in descs:
        d.x = d.w = d.bias = 4096          # any aligned non-null address: the picker reads alignment only
        d.y = 4096 + (2 if dtype == hiplib.YH_F16 else 4) * (ld - s_phys)      # the last slice of the parent
        d.res = d.y if acc else None       # accumulate: the planner passes the gradient itself as the residual
    return descs


def test_data_gradient_kernels_are_the_tested_ones():
    """Every data gradient of every shipped cfg (bench batch, the cfg's own size; YOLOv3 also at 608 / batch 64), in write and in
    accumulate mode, fp16 and fp32, contiguous and as a slice of a wider gradient buffer: the kernel yh_conv2d_tile chooses for it must
    be one tests/test_gpu_dgrad_forms.py exercises IN DATA-GRADIENT FORM (its ACCEPTED table).  No tile number is pinned - the picker
    may be retuned - but a data gradient must not land on a kernel that conformance file does not run (host code: no GPU needed)."""
    import glob
    sys.path.insert(0, os.path.join(REPO, 'tests', 'golden'))
    try:
        from make_golden_wgrad_selection import conv_layers
    finally:
        sys.path.pop(0)
    import conftest
    import test_gpu_dgrad_forms as forms
    lib = hiplib.load()
    cfgs = [(p, None, 32 if 'yolov4' in os.path.basename(p) else 64) for p in sorted(glob.glob(os.path.join(conftest.PKG, 'cfg', '**', '*.cfg'), recursive=True))]
    cfgs.append((os.path.join(conftest.PKG, 'cfg', 'yolov3', 'yolov3.cfg'), 608, 64))
    assert len(cfgs) > 5
    seen, chosen = set(), {}
    for path, size, batch in cfgs:
        for (h, w, cin, cout, k, stride, pad) in conv_layers(path, size):
            if cin == 3 or (h, w, cin, cout, k, stride, pad, batch) in seen:      # no data gradient into the image
                continue
            seen.add((h, w, cin, cout, k, stride, pad, batch))
            assert stride in (1, 2), (path, stride)
            for dtype in (hiplib.YH_F16, hiplib.YH_F32):
                for acc in (False, True):
                    for pitch in (1, 2):
                        for form, d in _dgrad_descs(batch, h, w, cin, cout, k, stride, pad, dtype, acc, pitch):
                            tile = int(lib.yh_conv2d_tile(C.byref(d)))
                            what = (os.path.basename(path), h, w, cin, cout, k, stride, dtype, acc, pitch, form, tile)
                            assert form in forms.ACCEPTED, what
                            if form == 'fused' and not 21 <= tile <= 35:
                                tile = 24      # yh_conv2d_fwd: only the LDS-DMA ring kernels carry the four-phase scatter
                            assert tile in forms.ACCEPTED[form] and tile != 0, what
                            assert dtype == hiplib.YH_F16 or tile in forms.F32_TILES, what
                            assert not (tile == 71 and acc), what
                            chosen.setdefault(form, set()).add(tile)
    assert len(seen) > 100 and set(chosen) == set(forms.FORMS), (len(seen), sorted(chosen))


def _roll_workspace(r):
    """Floats of partial tiles conv_wgrad_roll_kernel writes for a 3x3 / s1 row (csrc/conv_wgrad_roll.hip, wgrad_roll_geometry): one
    128 x [9 x 64] tile per (split, tile); 256 / tiles splits of the 32-position steps of the padded pixel space, at least 8 steps each."""
    tiles = (r['cout'] // 128) * (r['cin'] // 64)
    steps = -(-r['n'] * (r['h'] + 1) * (r['w'] + 1) // 32)
    splits = max(1, min(256 // tiles, steps // 8))
    per_split = -(-steps // splits)
    return -(-steps // per_split) * tiles * 128 * 576


def test_wgrad_kernel_selection_is_pinned():
    """Which weight-gradient kernel every conv layer of every shipped cfg runs on, and the workspace it asks for, against the table
    recorded before the superseded forms (round-3 halo kernel, 128 x 256 / 256 x 256 im2col tiles) were deleted
    (tests/golden/make_golden_wgrad_selection.py; yh_conv2d_wgrad_kernel / _workspace are host code).  Rows whose `halo` flag is set
    had their workspace sized by the deleted kernel's geometry where that was the larger: they run on the rolling form (91), and
    the workspace must cover what that form writes."""
    lib = hiplib.load()
    rows = json.load(open(os.path.join(REPO, 'tests', 'golden', 'wgrad_selection.json')))
    assert len(rows) > 300 and {r['kernel'] for r in rows} == {1, 22, 42, 82, 91}
    for r in rows:
        pad, k, s = r['pad'], r['k'], r['stride']
        d = hiplib.WgradDesc(n=r['n'], h=r['h'], w_in=r['w'], cin=r['cin'], ho=(r['h'] + 2 * pad - k) // s + 1, wo=(r['w'] + 2 * pad - k) // s + 1,
                             cout=r['cout'], kh=k, kw=k, stride=s, pad=pad, ldx=r['cin'], lddz=-(-r['cout'] // 8) * 8, dtype=r['dtype'], splits=0,
                             cin_w=r['cin_w'])
        d.x = d.dz = d.dw = 4096          # any aligned non-null address: the pickers read no memory
        assert lib.yh_conv2d_wgrad_kernel(C.byref(d)) == r['kernel'], r
        ws = lib.yh_conv2d_wgrad_workspace(C.byref(d))
        if r['halo']:
            assert r['kernel'] == 91 and _roll_workspace(r) <= ws <= r['workspace'], (r, ws)
        else:
            assert ws == r['workspace'], (r, ws)
