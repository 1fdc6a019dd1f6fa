"""What darknet's scale_x_y costs: decode, compute_loss + backward and hip_detect with and without it, and the default path against a parent.

    python tools/scale_xy_timing.py [--iters 20] [--warmup 5] [--rounds 3] [--parent CHECKOUT] [--pairs 3] [--out profiles/scale_xy_timing.txt]

One device, the head shapes of YOLOv4-608 (76 / 38 / 19 cells at strides 8 / 16 / 32, 3 anchors, nc 80, NHWC head tensors of 256
channels), the scales of cfg/yolov4/yolov4.cfg (1.2 / 1.1 / 1.05).  Legs, alternated in one call after warm-up:
  (a) decode, unscaled     yh_yolo_decode on the three heads, batch 16 (io and raw written)
  (b) decode, scaled       yh_yolo_decode_sxy on the same buffers
  (c) loss, unscaled       compute_loss + backward, batch 64, 640 labels: the default loss (GIoU, gamma 0) on yh_yolo_loss_fwd / _bwd
  (d) loss, scaled         the same through yh_yolo_loss_head_fwd / _bwd
  (e) hip_detect, plain    Darknet(yolov4.cfg) at 608, batch 16, fp16 engine, conf 0.3: forward + fused decode / candidate filter + NMS
  (f) hip_detect, flag     the same model built with scale_x_y=True
Every iteration records the device ms between two events on the stream and the host ms until the call returns.  Reported: median and
min .. max over all timed iterations of a leg.

--parent CHECKOUT: the unscaled default legs (a) and (c) - entries the parent has too - in fresh processes, alternately from a checkout
of the parent commit (its own libyolo_hip.so, built beforehand) and from this tree, `--pairs` times; the rule of DESIGN.md 7j decides:
the default path is not behind when the difference of the medians of the process medians lies inside the combined spread (max - min
of each set, added).

These are the head operations alone on seeded random values.  Step time is NOT measured here.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
HYP = {'giou': 3.54, 'cls': 37.4, 'cls_pw': 1.0, 'obj': 64.3, 'obj_pw': 1.0, 'iou_t': 0.20, 'fl_gamma': 0.0}
CFG = os.path.join('cfg', 'yolov4', 'yolov4.cfg')


def events(fn, n, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        host = (time.perf_counter() - t0) * 1e3
        b.record()
        torch.cuda.synchronize()
        out.append((a.elapsed_time(b), host))
    return out


def decode_leg(model, size, batch, dev, scaled):
    """A closure that decodes the three heads of `model` through the ABI (scaled: yh_yolo_decode_sxy with the modules' scales)."""
    import torch
    from engine import hiplib
    lib = hiplib.load()
    g = torch.Generator().manual_seed(21)
    layers = [model.module_list[j] for j in model.yolo_layers]
    rows = sum(m.na * (size // int(m.stride)) ** 2 for m in layers)
    no = layers[0].no
    io = torch.empty(batch, rows, no, device=dev)
    keep, calls, off = [io], [], 0
    for m in layers:
        n = size // int(m.stride)
        ld = (m.na * m.no + 7) // 8 * 8
        p = (torch.randn(batch, n, n, ld, generator=g) * 0.8).to(dev)
        raw = torch.empty(batch, m.na, n, n, m.no, device=dev)
        d = hiplib.DecodeDesc(p=hiplib.ptr(p), io=hiplib.ptr(io), raw=hiplib.ptr(raw), n=batch, ny=n, nx=n, na=m.na, no=m.no, ldp=ld,
                              rows_total=rows, row_off=off, stride=float(m.stride))
        av = m.anchor_vec.cpu()
        for a in range(m.na):
            d.anchor_w[a], d.anchor_h[a] = float(av[a, 0]), float(av[a, 1])
        if scaled:
            d = hiplib.DecodeSxyDesc(d=d, scale_x_y=float(m.scale_x_y))
            calls.append((lib.yh_yolo_decode_sxy, d))
        else:
            calls.append((lib.yh_yolo_decode, d))
        keep += [p, raw]
        off += m.na * n * n

    def run():
        s = hiplib.stream_ptr()
        for fn, d in calls:
            hiplib.check(fn(C.byref(d), s), 'decode')
    run.keep = keep
    return run


def loss_leg(model, size, batch, labels, dev):
    sys.path.insert(0, HERE)
    import focal_loss_timing as flt
    bases, targets = flt.make_inputs(model, size, batch, labels, dev)
    return lambda: flt.one(bases, targets, model)


def detect_leg(model, size, batch, dev):
    import torch
    g = torch.Generator().manual_seed(5)
    x = torch.rand(batch, 3, size, size, generator=g).to(dev)
    model.to(dev).eval()
    model.hip_precision = 'fp16'

    def run():
        with torch.no_grad():
            model.hip_detect(x, 0.3, 0.6)
    return run


def build(pkg, size, flag):
    import torch
    from models import Darknet
    torch.manual_seed(0)
    model = Darknet(os.path.join(pkg, CFG), (size, size), **({'scale_x_y': True} if flag else {}))
    model.nc, model.gr, model.hyp = 80, 1.0, dict(HYP)
    return model


def stat(times):
    dv, hs = [t[0] for t in times], [t[1] for t in times]
    return (statistics.median(dv), min(dv), max(dv), statistics.median(hs), min(hs), max(hs))


def default_legs(args):
    """The child of --parent: legs (a) and (c) from the tree `--pkg`, one JSON line."""
    sys.path.insert(0, args.pkg)
    import torch
    dev = torch.device('cuda', 0)
    model = build(args.pkg, args.size, False)
    legs = {'a': decode_leg(model, args.size, args.decode_batch, dev, False), 'c': loss_leg(model, args.size, args.batch, args.labels, dev)}
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].extend(events(fn, args.iters, args.warmup))
    from engine import loss as hip_loss
    hip_loss.flush_label_check()
    print(json.dumps({k: stat(v) for k, v in times.items()}))


def parent_comparison(args, lines):
    own = os.path.abspath(PKG)
    parent = os.path.abspath(args.parent)
    if not os.path.isfile(os.path.join(parent, 'models.py')):      # a checkout of the repository: the package is one level down
        parent = os.path.join(parent, os.path.basename(own))
    rows = []
    for pair in range(args.pairs):
        order = (('parent', parent), ('new', own)) if pair % 2 == 0 else (('new', own), ('parent', parent))
        for tag, pkg in order:
            cmd = [sys.executable, os.path.abspath(__file__), '--default-legs', '--pkg', pkg, '--iters', str(args.iters), '--warmup',
                   str(args.warmup), '--rounds', str(args.rounds), '--size', str(args.size), '--batch', str(args.batch), '--decode-batch',
                   str(args.decode_batch), '--labels', str(args.labels)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300, cwd=pkg).stdout
            rows.append((pair + 1, tag, json.loads(out.strip().splitlines()[-1])))
    lines += ['', 'the unscaled default legs of this tree against the parent commit (%s): one process each, interleaved on the same device'
              % args.parent, 'per process the median and min .. max of %d iterations (%d alternating runs of %d), device ms between stream events'
              % (args.rounds * args.iters, args.rounds, args.iters), '']
    for key, label in (('a', 'yh_yolo_decode, YOLOv4-%d heads, batch %d' % (args.size, args.decode_batch)),
                       ('c', 'compute_loss + backward, GIoU gamma 0, batch %d' % args.batch)):
        lines.append('(%s) %s' % (key, label))
        lines.append('pair tree     device ms           min .. max   host ms           min .. max')
        for pair, tag, res in rows:
            lines.append('%-4d %-8s %9.3f %9.3f ..%8.3f %9.3f %9.3f ..%8.3f' % (pair, tag, *res[key]))
        med = {t: [res[key][0] for _, tag, res in rows if tag == t] for t in ('parent', 'new')}
        mp, mn = statistics.median(med['parent']), statistics.median(med['new'])
        spread = (max(med['parent']) - min(med['parent'])) + (max(med['new']) - min(med['new']))
        verdict = 'the default path is not behind the parent by more than the spread' if mn - mp <= spread else \
            'the default path IS behind the parent by more than the spread'
        lines.append('median of the %d process medians: parent %.4f ms (%.4f .. %.4f), this tree %.4f ms (%.4f .. %.4f)'
                     % (len(med['new']), mp, min(med['parent']), max(med['parent']), mn, min(med['new']), max(med['new'])))
        lines.append('difference %+.4f ms; combined spread of the two sets of process medians %.4f ms -> %s' % (mn - mp, spread, verdict))
        lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20, help='timed iterations per run')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='alternating runs per leg')
    ap.add_argument('--batch', type=int, default=64, help='batch of the loss legs')
    ap.add_argument('--decode-batch', type=int, default=16, help='batch of the decode and hip_detect legs')
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--labels', type=int, default=10, help='labels per image')
    ap.add_argument('--no-detect', action='store_true', help='skip the hip_detect legs')
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built: compare the default legs')
    ap.add_argument('--pairs', type=int, default=3, help='process pairs of the parent comparison')
    ap.add_argument('--default-legs', action='store_true', help='(internal) run legs (a) and (c) from --pkg and print one JSON line')
    ap.add_argument('--pkg', default=PKG, help='(internal) the package tree to import')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'scale_xy_timing.txt'))
    args = ap.parse_args()
    if args.default_legs:
        return default_legs(args)
    sys.path.insert(0, PKG)
    import torch
    from engine import loss as hip_loss
    dev = torch.device('cuda', 0)
    plain, flag = build(PKG, args.size, False), build(PKG, args.size, True)
    scales = [flag.module_list[j].scale_x_y for j in flag.yolo_layers]
    legs = [('a', 'decode, unscaled', decode_leg(plain, args.size, args.decode_batch, dev, False), 1),
            ('b', 'decode, scaled', decode_leg(flag, args.size, args.decode_batch, dev, True), 1),
            ('c', 'loss, unscaled', loss_leg(plain, args.size, args.batch, args.labels, dev), 1),
            ('d', 'loss, scaled', loss_leg(flag, args.size, args.batch, args.labels, dev), 1)]
    if not args.no_detect:
        legs += [('e', 'hip_detect, plain', detect_leg(plain, args.size, args.decode_batch, dev), 2),
                 ('f', 'hip_detect, flag', detect_leg(flag, args.size, args.decode_batch, dev), 2)]
    times = {k: [] for k, _, _, _ in legs}
    for _ in range(args.rounds):
        for k, _, fn, div in legs:
            times[k].extend(events(fn, max(args.iters // div, 1), max(args.warmup // div, 1)))
    hip_loss.reset_scale_stats()
    legs[2][2]()
    unscaled_calls = hip_loss.scale_stats()
    legs[3][2]()
    torch.cuda.synchronize()
    hip_loss.flush_label_check()
    assert unscaled_calls == dict(scale_fwd=0, scale_bwd=0) and hip_loss.scale_stats() == dict(scale_fwd=3, scale_bwd=3), hip_loss.scale_stats()
    lines = ['scale_x_y (%s on the three heads) against the unscaled heads, %s' % (' / '.join('%g' % s for s in scales), torch.cuda.get_device_name(0)),
             'head shapes of YOLOv4-%d, nc 80, NHWC head tensors of 256 channels; decode and hip_detect at batch %d, compute_loss + backward '
             'at batch %d with %d labels' % (args.size, args.decode_batch, args.batch, args.batch * args.labels),
             'median and min .. max per leg (%d alternating runs of %d iterations, hip_detect half as many); device ms between stream '
             'events, host ms until the call returns' % (args.rounds, args.iters), '',
             '%-22s %9s %20s %9s %20s' % ('leg', 'device ms', 'min .. max', 'host ms', 'min .. max')]
    st = {}
    for k, label, _, _ in legs:
        st[k] = stat(times[k])
        lines.append('%-22s %9.4f %9.4f ..%8.4f %9.4f %9.4f ..%8.4f' % (('(%s) ' % k) + label, *st[k]))
    lines.append('')
    for x, y, what in (('b', 'a', 'decode'), ('d', 'c', 'compute_loss + backward'), ('f', 'e', 'hip_detect')):
        if x in st:
            spread = (st[x][2] - st[x][1]) + (st[y][2] - st[y][1])
            lines.append('(%s) - (%s): device time %+.4f ms, host time %+.4f ms; combined spread of the two legs (device time) %.4f ms: what '
                         'the scale costs %s' % (x, y, st[x][0] - st[y][0], st[x][3] - st[y][3], spread, what))
    if args.parent:
        parent_comparison(args, lines)
    lines.append('the head operations alone on seeded random values; step time is not measured by this tool')
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
