"""Times of `compute_loss` + backward with focal loss: the torch statement against the fused focal kernels, and the fused default loss.

    python tools/focal_loss_timing.py [--iters 20] [--warmup 5] [--rounds 3] [--batch 64] [--out profiles/focal_loss_timing.txt]

One device, the raw heads of YOLOv3-608 (NHWC head tensors of 256 channels, the views the training forward hands out), nc 80, about
10 labels per image, `train.py`'s gains.  Three legs, alternated in one call after warm-up:
  (a) torch, gamma 1.5     YOLO_HIP_FOCAL_LOSS=0: `utils.utils.compute_loss`'s torch statement with FocalLoss, autograd backward
  (b) fused, gamma 1.5     csrc/loss.hip through yh_yolo_loss_focal_fwd / _bwd
  (c) fused, gamma 0       the default loss on yh_yolo_loss_fwd / _bwd, for scale
Every iteration records
  device ms   between two events on the stream, around compute_loss + backward
  host ms     the time until backward returns (no synchronisation by this tool; the torch statement synchronises on its own)
Reported: median and min .. max over all timed iterations of a leg and - where torch's profiler gives them - the kernel launches of
one iteration and the ms the device was busy in them, and for the fused legs the same per kernel of csrc/loss.hip.  The last lines apply the rule that decides the default: the fused focal path
stays on unless its device time is above leg (a)'s by more than the two legs' combined spread (max - min of each, added).

This is the loss alone on seeded random heads.  Step time with focal loss is NOT measured here.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
HYP = {'giou': 3.54, 'cls': 37.4, 'cls_pw': 1.0, 'obj': 64.3, 'obj_pw': 1.0, 'iou_t': 0.20, 'fl_gamma': 0.0}
LEGS = (('a', 'torch, gamma 1.5', 1.5, '0'), ('b', 'fused, gamma 1.5', 1.5, '1'), ('c', 'fused, gamma 0', 0.0, '1'))


def make_inputs(model, size, batch, labels_per_image, dev):
    """Seeded NHWC head tensors (channel axis padded to a multiple of 8), their raw-head views, and the labels."""
    import torch
    g = torch.Generator().manual_seed(21)
    bases = []
    for j in model.yolo_layers:
        m = model.module_list[j]
        n = size // int(m.stride)
        ld = (m.na * m.no + 7) // 8 * 8
        base = torch.zeros(batch, n, n, ld)
        base[..., :m.na * m.no] = torch.randn(batch, n, n, m.na * m.no, generator=g) * 0.8
        bases.append((base.to(dev).requires_grad_(), m.na, m.no))
    rows = []
    for b in range(batch):
        for _ in range(labels_per_image):
            cls = int(torch.randint(0, model.nc, (1,), generator=g))
            wh = torch.rand(2, generator=g) * 0.5 + 0.03
            xy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
            rows.append([b, cls, xy[0].item(), xy[1].item(), wh[0].item(), wh[1].item()])
    return bases, torch.tensor(rows, dtype=torch.float32).to(dev)


def one(bases, targets, model):
    from utils.utils import compute_loss
    views = []
    for base, na, no in bases:
        base.grad = None
        bs, ny, nx, _ = base.shape
        views.append(base[..., :na * no].view(bs, ny, nx, na, no).permute(0, 3, 1, 2, 4))
    loss, items = compute_loss(views, targets, model)
    loss.backward()
    return items


def timed(bases, targets, model, n, warmup):
    import torch
    for _ in range(warmup):
        one(bases, targets, model)
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        one(bases, targets, model)
        host = (time.perf_counter() - t0) * 1e3
        b.record()
        torch.cuda.synchronize()
        out.append((a.elapsed_time(b), host))
    return out


def launches(bases, targets, model):
    """(kernel launches, ms the device was busy in them, [(kernel name, launches, ms)] of csrc/loss.hip's kernels) of one iteration
    under torch's profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile as prof
    torch.cuda.synchronize()
    with prof(activities=[ProfilerActivity.CUDA]) as p:
        one(bases, targets, model)
        torch.cuda.synchronize()
    kernels = [e for e in p.key_averages() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower()]
    dev_us = lambda e: getattr(e, 'self_device_time_total', getattr(e, 'self_cuda_time_total', 0))
    own = sorted(((e.key.split('(')[0].split('::')[-1], e.count, dev_us(e) / 1e3) for e in kernels if 'loss_' in e.key), key=lambda r: -r[2])
    return sum(e.count for e in kernels), sum(dev_us(e) for e in kernels) / 1e3, own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20, help='timed iterations per run')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='alternating runs per leg')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--labels', type=int, default=10, help='labels per image')
    ap.add_argument('--no-launches', action='store_true', help='skip the profiled iteration')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'focal_loss_timing.txt'))
    args = ap.parse_args()
    sys.path.insert(0, PKG)
    import torch
    from engine import loss as hip_loss
    from models import Darknet
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = Darknet(os.path.join(PKG, 'cfg', 'yolov3', 'yolov3.cfg'), (args.size, args.size))
    model.nc, model.gr = 80, 1.0
    bases, targets = make_inputs(model, args.size, args.batch, args.labels, dev)
    res = {key: dict(times=[], launches=None, busy=None, items=None, own=[]) for key, _, _, _ in LEGS}
    before = os.environ.get('YOLO_HIP_FOCAL_LOSS')

    def setup(gamma, env):
        model.hyp = dict(HYP, fl_gamma=gamma)
        os.environ['YOLO_HIP_FOCAL_LOSS'] = env
    try:
        for _ in range(args.rounds):
            for key, _, gamma, env in LEGS:
                setup(gamma, env)
                res[key]['times'].extend(timed(bases, targets, model, args.iters, args.warmup))
        for key, _, gamma, env in LEGS:
            setup(gamma, env)
            hip_loss.reset_stats()
            res[key]['items'] = [float(v) for v in one(bases, targets, model).cpu()]
            res[key]['focal_calls'] = hip_loss.stats()
            if not args.no_launches:
                try:
                    res[key]['launches'], res[key]['busy'], res[key]['own'] = launches(bases, targets, model)
                except Exception:      # the profiler is optional equipment
                    pass
        hip_loss.flush_label_check()
    finally:
        if before is None:
            os.environ.pop('YOLO_HIP_FOCAL_LOSS', None)
        else:
            os.environ['YOLO_HIP_FOCAL_LOSS'] = before
    assert res['a']['focal_calls'] == dict(focal_fwd=0, focal_bwd=0) and res['b']['focal_calls'] == dict(focal_fwd=3, focal_bwd=3)
    n = args.rounds * args.iters
    cells = sum(b.shape[0] * b.shape[1] * b.shape[2] * na for b, na, _ in bases)
    lines = ['compute_loss + backward with focal loss: torch statement (YOLO_HIP_FOCAL_LOSS=0) against the fused focal kernels, %s'
             % torch.cuda.get_device_name(0),
             'raw heads of YOLOv3-%d, batch %d, nc 80, %d labels (%d per image), %d cells; NHWC head tensors of %d channels'
             % (args.size, args.batch, targets.shape[0], args.labels, cells, bases[0][0].shape[3]),
             'median and min .. max of %d iterations per leg (%d alternating runs of %d, %d warm-up iterations each); device ms between '
             'stream events, host ms until backward returns' % (n, args.rounds, args.iters, args.warmup), '',
             '%-22s %9s %20s %9s %20s %9s %10s' % ('leg', 'device ms', 'min .. max', 'host ms', 'min .. max', 'launches', 'kernel ms')]
    stat = {}
    for key, label, _, _ in LEGS:
        r = res[key]
        dv, hs = [t[0] for t in r['times']], [t[1] for t in r['times']]
        stat[key] = (statistics.median(dv), min(dv), max(dv), statistics.median(hs), min(hs), max(hs))
        lines.append('%-22s %9.3f %9.3f ..%8.3f %9.3f %9.3f ..%8.3f %9s %10s'
                     % (('(%s) ' % key) + label, *stat[key], '-' if r['launches'] is None else r['launches'],
                        '-' if r['busy'] is None else '%.3f' % r['busy']))
    lines.append('')
    for key, label, _, _ in LEGS:
        lines.append('(%s) lbox, lobj, lcls, loss: %s' % (key, ', '.join('%.6f' % v for v in res[key]['items'])))
    for key in ('b', 'c'):
        for name, count, ms in res[key]['own']:
            lines.append('(%s) %-48s %2d launches %8.3f ms' % (key, name[:48], count, ms))
    a, b = stat['a'], stat['b']
    spread = (a[2] - a[1]) + (b[2] - b[1])
    lines.append('')
    lines.append('(b) - (a): device time %+.3f ms, host time %+.3f ms; combined spread of the two legs (device time) %.3f ms'
                 % (b[0] - a[0], b[3] - a[3], spread))
    lines.append('rule: the fused focal path is the default unless it is slower than (a) by more than the combined spread -> %s'
                 % ('default ON' if b[0] - a[0] <= spread else 'default OFF (YOLO_HIP_FOCAL_LOSS would have to default to 0)'))
    lines.append('(b) - (c): device time %+.3f ms: what the focal element costs on top of the default fused loss' % (b[0] - stat['c'][0]))
    lines.append('the loss alone on seeded random heads; step time with focal loss is not measured by this tool')
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
