"""Step times of multi-scale training (`train.py --multi-scale`, reference train.py:72-79, 368-374) on the HIP engine.

    python tools/multiscale_timing.py [--batch 64] [--size 608] [--visits 3] [--out profiles/multiscale_timing.txt]

For every image size of the multi-scale range of --size (608: the 17 sizes 384 .. 896) it reports
  fixed      ms of a training step at that size alone: one engine, that size only, warm
  first      ms of the first step at that size inside the multi-scale run (plan build included)
  steady     ms of a step at that size inside a random multi-scale sequence after every size was visited once (median of --visits)
and the memory the run holds: arena_bytes and plan_bytes of Darknet.hip_train_stats().

The script uses model(imgs), backward() and - behind hasattr - hip_reserve_train / hip_train_stats only, so the same file runs on a
commit without the step arena and gives that commit's cost per step in the same sequence (its rebuilds included).
"""
import argparse
import gc
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402


def sizes_of(base, gs=32):
    lo, hi = int(base // 1.5) // gs, int(base // 0.667) // gs        # train.py: the grid rounding of the multi-scale range
    return [g * gs for g in range(lo, hi + 1)]


def make_model(cfg, size, dev):
    from models import Darknet
    torch.manual_seed(0)
    return Darknet(cfg, (size, size)).to(dev).train()


def step(model, x):
    with torch.autocast('cuda', dtype=torch.float16):
        pred, _ = model(x)
    loss = sum(p.float().pow(2).mean() for p in pred)
    loss.backward()
    for p in model.parameters():
        p.grad = None


def timed(model, x):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step(model, x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=os.path.join(os.path.dirname(HERE), 'cfg', 'yolov3', 'yolov3.cfg'))
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--visits', type=int, default=3, help='steady-state visits of every size')
    ap.add_argument('--skip-fixed', action='store_true', help='only the multi-scale sequence')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(HERE), 'profiles', 'multiscale_timing.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    sizes = sizes_of(args.size)
    images = {s: torch.rand(args.batch, 3, s, s, device=dev) for s in sizes}
    lines = ['multi-scale step times: %s, fp16, batch %d, sizes %d .. %d (%d)' % (os.path.basename(args.cfg), args.batch, sizes[0], sizes[-1],
                                                                                 len(sizes))]

    # ---- the multi-scale run: first visits, then a random sequence
    model = make_model(args.cfg, sizes[-1], dev)
    has_arena = hasattr(model, 'hip_reserve_train')
    t_reserve = None
    if has_arena:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.hip_reserve_train([(args.batch, 3, sizes[-1], sizes[-1])], precision='fp16')
        torch.cuda.synchronize()
        t_reserve = (time.perf_counter() - t0) * 1e3
    rng = random.Random(0)
    order = list(sizes)
    rng.shuffle(order)
    first = {s: timed(model, images[s]) for s in order}
    seq = [s for _ in range(args.visits) for s in sizes]
    rng.shuffle(seq)
    steady = {s: [] for s in sizes}
    t_seq0 = time.perf_counter()
    for s in seq:
        steady[s].append(timed(model, images[s]))
    seq_ms = (time.perf_counter() - t_seq0) * 1e3 / len(seq)
    stats = model.hip_train_stats() if hasattr(model, 'hip_train_stats') else None
    peak = torch.cuda.max_memory_allocated()
    del model
    gc.collect()
    torch.cuda.empty_cache()

    # ---- every size alone
    fixed = {}
    if not args.skip_fixed:
        for s in sizes:
            model = make_model(args.cfg, s, dev)
            for _ in range(2):
                step(model, images[s])
            fixed[s] = statistics.median(timed(model, images[s]) for _ in range(3))
            del model
            gc.collect()
            torch.cuda.empty_cache()

    lines.append('step arena: %s' % ('yes' if has_arena else 'no (plans own their buffers; two shapes resident)'))
    if t_reserve is not None:
        lines.append('hip_reserve_train(largest): %.0f ms' % t_reserve)
    lines.append('%6s %10s %10s %10s %8s' % ('size', 'fixed ms', 'first ms', 'steady ms', 'ratio'))
    for s in sizes:
        med = statistics.median(steady[s])
        lines.append('%6d %10s %10.1f %10.1f %8s' % (s, '%.1f' % fixed[s] if s in fixed else '-', first[s], med,
                                                      '%.3f' % (med / fixed[s]) if s in fixed else '-'))
    lines.append('mean step of the random sequence (%d steps): %.1f ms' % (len(seq), seq_ms))
    if fixed:
        lines.append('mean fixed-shape step over the same sizes: %.1f ms' % (sum(fixed[s] for s in seq) / len(seq)))
    if stats is not None:
        lines.append('arena_bytes %d  plan_bytes %d  plans_resident %d  plan_builds %d  arena_allocs %d'
                     % (stats['arena_bytes'], stats['plan_bytes'], stats['plans_resident'], stats['plan_builds'], stats['arena_allocs']))
    lines.append('torch.cuda.max_memory_allocated of the multi-scale run: %d' % peak)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
