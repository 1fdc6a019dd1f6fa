"""Times of `compute_loss` + backward per box measure: the fused kernels at GIoU / DIoU / CIoU against the torch statement.

    python tools/box_loss_timing.py [--iters 20] [--warmup 5] [--rounds 3] [--batch 64] [--out profiles/box_loss_timing.txt]

One device, the raw heads of YOLOv3-608 (NHWC head tensors of 256 channels, the views the training forward hands out), nc 80, about
10 labels per image, `train.py`'s gains, gamma 0.  Five legs, alternated in one call after warm-up:
  (a) fused, giou      the default loss on yh_yolo_loss_fwd / _bwd
  (b) fused, diou      csrc/loss.hip through yh_yolo_loss_box_fwd / _bwd
  (c) fused, ciou      the same entries
  (d) torch, ciou      YOLO_HIP_BOX_LOSS=0: `utils.utils.compute_loss`'s torch statement, autograd backward
  (e) torch, giou      the torch statement of the default loss (`fused=False`), for scale
Every iteration records
  device ms   between two events on the stream, around compute_loss + backward
  host ms     the time until backward returns (no synchronisation by this tool; the torch statement synchronises on its own)
Reported: median and min .. max over all timed iterations of a leg and - where torch's profiler gives them - the kernel launches of
one iteration and the ms the device was busy in them, and for the fused legs the same per kernel of csrc/loss.hip.  The last lines
apply the rule that decides the default: the fused path stays the default for DIoU / CIoU only if its device time is below leg (d)'s by
more than the two legs' combined spread (max - min of each, added).

This is the loss alone on seeded random heads.  Step time is NOT measured here.
"""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from focal_loss_timing import HYP, launches, make_inputs, timed  # noqa: E402  (the same inputs and clocks as the focal tool)

# key, label, model.box_loss, YOLO_HIP_BOX_LOSS, compute_loss's fused argument
LEGS = (('a', 'fused, giou', 'giou', '1', None), ('b', 'fused, diou', 'diou', '1', None), ('c', 'fused, ciou', 'ciou', '1', None),
        ('d', 'torch, ciou', 'ciou', '0', None), ('e', 'torch, giou', 'giou', '1', False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20, help='timed iterations per run')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='alternating runs per leg')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--labels', type=int, default=10, help='labels per image')
    ap.add_argument('--no-launches', action='store_true', help='skip the profiled iteration')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'box_loss_timing.txt'))
    args = ap.parse_args()
    sys.path.insert(0, PKG)
    import torch
    import focal_loss_timing as flt
    from engine import loss as hip_loss
    from models import Darknet
    from utils import utils as U
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = Darknet(os.path.join(PKG, 'cfg', 'yolov3', 'yolov3.cfg'), (args.size, args.size))
    model.nc, model.gr, model.hyp = 80, 1.0, dict(HYP)
    bases, targets = make_inputs(model, args.size, args.batch, args.labels, dev)
    res = {leg[0]: dict(times=[], launches=None, busy=None, items=None, own=[]) for leg in LEGS}
    before = os.environ.get('YOLO_HIP_BOX_LOSS')
    real = U.compute_loss

    def setup(kind, env, fused):
        model.box_loss = kind
        os.environ['YOLO_HIP_BOX_LOSS'] = env
        U.compute_loss = real if fused is None else (lambda p, t, m: real(p, t, m, fused=fused))      # `one` calls it by name
    try:
        for _ in range(args.rounds):
            for key, _, kind, env, fused in LEGS:
                setup(kind, env, fused)
                res[key]['times'].extend(timed(bases, targets, model, args.iters, args.warmup))
        for key, _, kind, env, fused in LEGS:
            setup(kind, env, fused)
            hip_loss.reset_box_stats()
            res[key]['items'] = [float(v) for v in flt.one(bases, targets, model).cpu()]
            res[key]['box_calls'] = hip_loss.box_stats()
            if not args.no_launches:
                try:
                    res[key]['launches'], res[key]['busy'], res[key]['own'] = launches(bases, targets, model)
                except Exception:      # the profiler is optional equipment
                    pass
        hip_loss.flush_label_check()
    finally:
        U.compute_loss = real
        if before is None:
            os.environ.pop('YOLO_HIP_BOX_LOSS', None)
        else:
            os.environ['YOLO_HIP_BOX_LOSS'] = before
    none, three = dict(box_fwd=0, box_bwd=0), dict(box_fwd=3, box_bwd=3)
    assert [res[k]['box_calls'] for k in 'abcde'] == [none, three, three, none, none], [res[k]['box_calls'] for k in 'abcde']
    n = args.rounds * args.iters
    cells = sum(b.shape[0] * b.shape[1] * b.shape[2] * na for b, na, _ in bases)
    lines = ['compute_loss + backward per box measure: the fused kernels against the torch statement (YOLO_HIP_BOX_LOSS=0), %s'
             % torch.cuda.get_device_name(0),
             'raw heads of YOLOv3-%d, batch %d, nc 80, %d labels (%d per image), %d cells; NHWC head tensors of %d channels; gamma 0'
             % (args.size, args.batch, targets.shape[0], args.labels, cells, bases[0][0].shape[3]),
             'median and min .. max of %d iterations per leg (%d alternating runs of %d, %d warm-up iterations each); device ms between '
             'stream events, host ms until backward returns' % (n, args.rounds, args.iters, args.warmup), '',
             '%-22s %9s %20s %9s %20s %9s %10s' % ('leg', 'device ms', 'min .. max', 'host ms', 'min .. max', 'launches', 'kernel ms')]
    stat = {}
    for key, label, _, _, _ in LEGS:
        r = res[key]
        dv, hs = [t[0] for t in r['times']], [t[1] for t in r['times']]
        stat[key] = (statistics.median(dv), min(dv), max(dv), statistics.median(hs), min(hs), max(hs))
        lines.append('%-22s %9.3f %9.3f ..%8.3f %9.3f %9.3f ..%8.3f %9s %10s'
                     % (('(%s) ' % key) + label, *stat[key], '-' if r['launches'] is None else r['launches'],
                        '-' if r['busy'] is None else '%.3f' % r['busy']))
    lines.append('')
    for key, label, _, _, _ in LEGS:
        lines.append('(%s) lbox, lobj, lcls, loss: %s' % (key, ', '.join('%.6f' % v for v in res[key]['items'])))
    for key in ('a', 'b', 'c'):
        for name, count, ms in res[key]['own']:
            lines.append('(%s) %-48s %2d launches %8.3f ms' % (key, name[:48], count, ms))
    spread = lambda x, y: (stat[x][2] - stat[x][1]) + (stat[y][2] - stat[y][1])
    lines.append('')
    lines.append('(c) - (a): device time %+.3f ms, host time %+.3f ms; combined spread of the two legs (device time) %.3f ms: what CIoU '
                 'costs on top of the default fused loss' % (stat['c'][0] - stat['a'][0], stat['c'][3] - stat['a'][3], spread('c', 'a')))
    lines.append('(b) - (a): device time %+.3f ms, host time %+.3f ms; combined spread %.3f ms'
                 % (stat['b'][0] - stat['a'][0], stat['b'][3] - stat['a'][3], spread('b', 'a')))
    lines.append('(c) - (d): device time %+.3f ms, host time %+.3f ms; combined spread %.3f ms'
                 % (stat['c'][0] - stat['d'][0], stat['c'][3] - stat['d'][3], spread('c', 'd')))
    lines.append('rule: the fused path is the default for DIoU / CIoU only if it is ahead of (d) by more than the combined spread -> %s'
                 % ('default ON' if stat['d'][0] - stat['c'][0] > spread('c', 'd') else 'default OFF (YOLO_HIP_BOX_LOSS would have to default to 0)'))
    lines.append('(d) - (e): device time %+.3f ms: what CIoU costs the torch statement' % (stat['d'][0] - stat['e'][0]))
    lines.append('the loss alone on seeded random heads; step time is not measured by this tool')
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
