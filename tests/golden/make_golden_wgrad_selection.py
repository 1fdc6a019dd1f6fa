#!/usr/bin/env python3
"""Which weight-gradient kernel every conv layer of every shipped cfg runs on, as recorded results (host code: no GPU needed).

    [YOLO_HIP_LIB=path/to/libyolo_hip.so] python tests/golden/make_golden_wgrad_selection.py

Writes tests/golden/wgrad_selection.json: one row per distinct descriptor over every [convolutional] block of every cfg/**/*.cfg at
the cfg's own [net] size and the benchmark's batch (64; 32 for the YOLOv4 cfgs), plus the pruned fixture
slim_prune_0.5_yolov3-mobilenet-coco.cfg at 416, batch 64, and the headline workload (yolov3.cfg at 608, batch 64), in fp16 and fp32.  A row holds the descriptor, `yh_conv2d_wgrad_kernel`
and `yh_conv2d_wgrad_workspace` under the default environment, and `halo`: whether the library answered 90 under YH_WGRAD_HALO=1.

The committed file was recorded with the library of the commit BEFORE conv_wgrad_halo_kernel and the unreachable forms were deleted
(tests/test_abi.py::test_wgrad_kernel_selection_is_pinned holds the library to it); the `halo` column marks the rows whose workspace
that library sized by the deleted kernel's geometry and cannot be regenerated with a later library, which no longer answers 90.
"""
import ctypes as C
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402
from engine import hiplib  # noqa: E402
from utils.parse_config import parse_model_cfg  # noqa: E402

FIELDS = ('n', 'h', 'w', 'cin', 'cin_w', 'cout', 'k', 'stride', 'dtype')


def conv_layers(cfg_path, size=None):
    """(h, w, cin, cout, k, stride, pad) of every [convolutional] block: the channel / stride walk of models.create_modules."""
    blocks = parse_model_cfg(cfg_path)
    net, blocks = blocks[0], blocks[1:]
    height, width = (size, size) if size else (int(net['height']), int(net['width']))
    chans, scales, out = [3], [1.0], []
    for b in blocks:
        kind, c, s = b['type'], chans[-1], scales[-1]
        if kind in ('convolutional', 'depthwise'):
            k, st = int(b['size']), int(b['stride'])
            if kind == 'convolutional':
                out.append((int(height / s), int(width / s), c, int(b['filters']), k, st, (k - 1) // 2 if int(b['pad']) else 0))
            c, s = int(b['filters']), s * st
        elif kind == 'maxpool':
            s = s * int(b['stride'])
        elif kind == 'upsample':
            s = s / int(b['stride'])
        elif kind == 'se':
            c = int(b['filters']) if 'filters' in b else c
        elif kind == 'route':
            layers = b['layers']
            c = sum(chans[l + 1 if l > 0 else l] for l in layers) // (2 if 'groups' in b else 1)
            s = scales[layers[0] + 1 if layers[0] > 0 else layers[0]]
        chans.append(c)
        scales.append(s)
    return out


def descriptor(row):
    """The yh_wgrad_desc of a row, as engine/train.py builds it (the 3-channel image is stored with 8 channels, cin_w = 3)."""
    n, h, w, cin, cin_w, cout, k, stride, dtype = (row[f] for f in FIELDS)
    pad = row['pad']
    d = hiplib.WgradDesc(n=n, h=h, w_in=w, cin=cin, ho=(h + 2 * pad - k) // stride + 1, wo=(w + 2 * pad - k) // stride + 1, cout=cout,
                         kh=k, kw=k, stride=stride, pad=pad, ldx=cin, lddz=-(-cout // 8) * 8, dtype=dtype, splits=0, cin_w=cin_w)
    d.x = d.dz = d.dw = 4096      # any aligned non-null address: the pickers read no memory
    return d


def main():
    lib = hiplib.load()
    cfgs = [(p, None, 32 if 'yolov4' in os.path.basename(p) else 64) for p in sorted(glob.glob(os.path.join(conftest.PKG, 'cfg', '**', '*.cfg'), recursive=True))]
    cfgs.append((os.path.join(HERE, 'slim_prune_0.5_yolov3-mobilenet-coco.cfg'), 416, 64))
    cfgs.append((os.path.join(conftest.PKG, 'cfg', 'yolov3', 'yolov3.cfg'), 608, 64))
    rows = {}
    for path, size, batch in cfgs:
        for (h, w, cin, cout, k, stride, pad) in conv_layers(path, size):
            for dtype in (hiplib.YH_F16, hiplib.YH_F32):
                row = dict(n=batch, h=h, w=w, cin=8 if cin == 3 else cin, cin_w=3 if cin == 3 else 0, cout=cout, k=k, stride=stride, dtype=dtype, pad=pad)
                rows.setdefault(tuple(row[f] for f in FIELDS), row)
    for env, keys in (({}, ('kernel', 'workspace')), ({'YH_WGRAD_HALO': '1'}, ('halo',))):
        os.environ.update(env)
        for row in rows.values():
            d = descriptor(row)
            code = int(lib.yh_conv2d_wgrad_kernel(C.byref(d)))
            if 'halo' in keys:
                row['halo'] = code == 90
            else:
                row['kernel'], row['workspace'] = code, int(lib.yh_conv2d_wgrad_workspace(C.byref(d)))
        for k in env:
            del os.environ[k]
    out = os.path.join(HERE, 'wgrad_selection.json')
    with open(out, 'w') as fh:
        fh.write('[\n' + ',\n'.join(json.dumps(rows[key]) for key in sorted(rows)) + '\n]\n')
    print('%d rows -> %s; kernels %s; halo rows %d' % (len(rows), out, sorted({r['kernel'] for r in rows.values()}), sum(r['halo'] for r in rows.values())))


if __name__ == '__main__':
    main()
