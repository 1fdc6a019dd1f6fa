"""Step times of TPSQ training (`train.py --quantized 2`) with the fused quantiser kernels and with the torch formulas.

    python tools/tpsq_timing.py [--batch 16] [--size 416] [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/tpsq_timing.txt]

Trains cfg/yolov3tiny/yolov3-tiny.cfg with ``quantized=2`` on synthetic images and labels on one device: forward, compute_loss,
backward, Adam step (train.py's optimiser for quantised graphs, so the learnable scales leave their powers of two every step).  Runs
of the fused path (csrc/tpsq.hip through engine/tpsq.py) and of ``YOLO_TPSQ_TORCH=1`` (the reference's eager arithmetic with its host
reads) alternate, each on a fresh model from the same seed, after one discarded run that loads kernels and lets the convolution
library choose its algorithms.  Timed per run:
  first step    every activation quantiser runs its 99-candidate warm-up search
  steady        the steps after ``--warmup`` more untimed ones
Reported: the median over the runs' first steps, the median over all timed steady steps of a path, and the kernel launches of one
steady step where torch's profiler gives them.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

HYP = {'giou': 3.54, 'cls': 37.4, 'cls_pw': 1.0, 'obj': 64.3, 'obj_pw': 1.0, 'iou_t': 0.20, 'fl_gamma': 0.0}


def make_model(cfg, size, dev, total_steps):
    from models import Darknet
    torch.manual_seed(0)
    model = Darknet(cfg, (size, size), quantized=2, a_bit=8, w_bit=8, steps=total_steps).to(dev).train()
    model.nc, model.gr, model.hyp = 80, 1.0, HYP
    return model


def synthetic(batch, size, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(batch, 3, size, size, generator=g)
    rows = [[b, (3 * b + k) % 80, 0.2 + 0.6 * torch.rand(1, generator=g).item(), 0.2 + 0.6 * torch.rand(1, generator=g).item(),
             0.1 + 0.3 * torch.rand(1, generator=g).item(), 0.1 + 0.3 * torch.rand(1, generator=g).item()] for b in range(batch) for k in range(3)]
    return x.to(dev), torch.tensor(rows).to(dev)


def step(model, opt, x, targets):
    from utils.utils import compute_loss
    pred, _ = model(x)
    loss, _ = compute_loss(pred, targets, model)
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)


def run(path, args, dev, x, targets, profile=False):
    """(first step ms, [steady step ms]) of one fresh model, or the launch count of one steady step."""
    os.environ['YOLO_TPSQ_TORCH'] = '1' if path == 'torch' else '0'
    model = make_model(args.cfg, args.size, dev, 1000000)
    opt = torch.optim.Adam(model.parameters(), lr=1e-5, fused=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step(model, opt, x, targets)
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    for _ in range(args.warmup):
        step(model, opt, x, targets)
    torch.cuda.synchronize()
    if profile:
        from torch.profiler import ProfilerActivity, profile as prof
        with prof(activities=[ProfilerActivity.CUDA]) as p:
            step(model, opt, x, targets)
            torch.cuda.synchronize()
        return sum(e.count for e in p.key_averages() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower())
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        step(model, opt, x, targets)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return first, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=os.path.join(os.path.dirname(HERE), 'cfg', 'yolov3tiny', 'yolov3-tiny.cfg'))
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--steps', type=int, default=20, help='timed steady steps per run')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='alternating runs per path')
    ap.add_argument('--no-launches', action='store_true', help='skip the profiled step')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(HERE), 'profiles', 'tpsq_timing.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    x, targets = synthetic(args.batch, args.size, dev)
    before = os.environ.get('YOLO_TPSQ_TORCH')
    for path in ('fused', 'torch'):      # discarded: kernel loading, the convolution library's algorithm choice
        run(path, argparse.Namespace(**dict(vars(args), steps=1, warmup=1)), dev, x, targets)
    first, steady = {'fused': [], 'torch': []}, {'fused': [], 'torch': []}
    for _ in range(args.rounds):
        for path in ('fused', 'torch'):
            f, t = run(path, args, dev, x, targets)
            first[path].append(f)
            steady[path].extend(t)
    lines = ['TPSQ step times: %s, quantized=2, fp32, batch %d, %d x %d, Adam, %s' % (os.path.basename(args.cfg), args.batch, args.size, args.size,
                                                                                    torch.cuda.get_device_name(0)),
             'medians over %d alternating runs per path, fresh model each: the first step (warm-up search), %d steady steps per run after %d untimed'
             % (args.rounds, args.steps, args.warmup),
             '%-12s %12s %12s %8s' % ('phase', 'fused ms', 'torch ms', 'ratio')]
    for phase, d in (('first step', first), ('steady', steady)):
        f, t = statistics.median(d['fused']), statistics.median(d['torch'])
        lines.append('%-12s %12.2f %12.2f %8.2f' % (phase, f, t, t / f))

    def write():
        text = '\n'.join(lines) + '\n'
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(text)
        return text
    write()
    if not args.no_launches:
        try:
            n = {path: run(path, args, dev, x, targets, profile=True) for path in ('fused', 'torch')}
            lines.append('kernel launches per steady step: fused %d, torch %d' % (n['fused'], n['torch']))
        except Exception as e:      # the profiler is optional equipment
            lines.append('kernel launches per steady step: not available (%s)' % type(e).__name__)
    print(write(), end='')
    if before is None:
        os.environ.pop('YOLO_TPSQ_TORCH', None)
    else:
        os.environ['YOLO_TPSQ_TORCH'] = before


if __name__ == '__main__':
    main()
