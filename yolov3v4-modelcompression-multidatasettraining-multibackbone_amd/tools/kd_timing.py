"""Times of one training step with feature distillation (`train.py --KDstr 4`) on one gfx950 device.

    python tools/kd_timing.py [--cfg cfg/yolov3/yolov3.cfg] [--img 416] [--batch 16] [--steps 8] [--warmup 3] [--rounds 3]
                              [--out profiles/kd_timing.txt]

Three legs, alternating per round, fp16 compute under autocast (the -mpt recipe), student and teacher of the same cfg:
  (a) plain    the HIP training step: forward, compute_loss, backward
  (b) KD4      the same with the teacher's forward on the evaluation engine, both models handing out attention maps
               (hip_return_features = 'attention'), compute_lost_KD4 on them: the unfused plan, the teacher, and the three launches
               (yh_kd_attention per model, yh_kd_attention_kl, yh_kd_inject; counted by engine.kd.stats())
  (c) eager    the reference's way: the eager modules (_forward_eager) of student and teacher with their full feature_out lists
               and the torch statement.  The baseline: without the attention maps KD4 cannot run on the HIP step at all.
Every step records the device ms between two stream events around it and the host ms until the calls return.  Reported: median and
min .. max over all timed steps of a leg.  (b) - (a) is what distillation costs on the HIP step.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, PKG)

HYP = {'giou': 3.54, 'cls': 37.4, 'cls_pw': 1.0, 'obj': 64.3, 'obj_pw': 1.0, 'iou_t': 0.20, 'fl_gamma': 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=os.path.join('cfg', 'yolov3', 'yolov3.cfg'))
    ap.add_argument('--img', type=int, default=416)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=8, help='timed steps per run')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3, help='alternating runs per leg')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'kd_timing.txt'))
    args = ap.parse_args()
    import torch
    from engine import kd
    from models import Darknet
    from utils.utils import compute_loss, compute_lost_KD4
    dev = torch.device('cuda', 0)
    cfg = args.cfg if os.path.isfile(args.cfg) else os.path.join(PKG, args.cfg)

    def build(seed):
        torch.manual_seed(seed)
        m = Darknet(cfg, (args.img, args.img)).to(dev)
        m.nc, m.gr, m.hyp = int(m.module_defs[-1]['classes']), 1.0, dict(HYP)
        return m
    student, teacher = build(0).train(), build(1).eval()
    g = torch.Generator().manual_seed(2)
    x = torch.rand(args.batch, 3, args.img, args.img, generator=g).to(dev)
    rows = [[b, int(torch.randint(0, student.nc, (1,), generator=g)), *(0.2 + 0.6 * torch.rand(2, generator=g)).tolist(),
             *(0.05 + 0.3 * torch.rand(2, generator=g)).tolist()] for b in range(args.batch) for _ in range(8)]
    targets = torch.tensor(rows, device=dev)

    def step(leg):
        for p in student.parameters():
            p.grad = None
        attention = leg == 'kd4'
        student.hip_return_features = teacher.hip_return_features = 'attention' if attention else False
        with torch.autocast('cuda', dtype=torch.float16):
            pred, fs = student._forward_eager(x) if leg == 'eager' else student(x)
        pred = [p.float() for p in pred]
        loss = compute_loss(pred, targets, student)[0]
        if leg != 'plain':
            with torch.no_grad():
                if leg == 'eager':
                    with torch.autocast('cuda', dtype=torch.float16):
                        _, out_t, ft = teacher._forward_eager(x)
                else:
                    _, out_t, ft = teacher(x)
            loss = loss + compute_lost_KD4(student, targets, pred, [o.float() for o in out_t], fs, ft, args.batch)
        (loss * (128.0 * args.batch / 64)).sum().backward()

    def run(leg):
        for _ in range(args.warmup):
            step(leg)
        torch.cuda.synchronize()
        out = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            step(leg)
            host = (time.perf_counter() - t0) * 1e3
            b.record()
            torch.cuda.synchronize()
            out.append((a.elapsed_time(b), host))
        return out

    legs = ('plain', 'kd4', 'eager')
    times = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            times[leg].extend(run(leg))
    kd.reset_stats()
    step('kd4')
    torch.cuda.synchronize()
    launches = kd.stats()
    student.hip_return_features = 'attention'
    _, maps = student(x)
    label = {'plain': '(a) plain HIP step', 'kd4': '(b) KD4 HIP step', 'eager': '(c) KD4 eager + lists'}
    n = args.rounds * args.steps
    lines = ['Training step with feature distillation (--KDstr 4): %s, %d px, batch %d, fp16 under autocast, %s'
             % (os.path.basename(cfg), args.img, args.batch, torch.cuda.get_device_name(0)),
             'median and min .. max of %d steps per leg (%d alternating runs of %d steps, %d warm-up steps each); device ms between stream '
             'events around the step, host ms until its calls return' % (n, args.rounds, args.steps, args.warmup),
             '%d attention maps per model, %d floats per model and step' % (len(maps), maps.flat.numel()), '',
             '%-24s %9s %20s %9s %20s' % ('leg', 'device ms', 'min .. max', 'host ms', 'min .. max')]
    med = {}
    for leg in legs:
        dv, hs = [t[0] for t in times[leg]], [t[1] for t in times[leg]]
        med[leg] = statistics.median(dv)
        lines.append('%-24s %9.3f %9.3f ..%8.3f %9.3f %9.3f ..%8.3f' % (label[leg], med[leg], min(dv), max(dv), statistics.median(hs), min(hs), max(hs)))
    lines += ['', '(b) - (a): %.3f ms for the unfused plan, the teacher forward and the distillation launches' % (med['kd4'] - med['plain']),
              '(c) / (b): %.2f' % (med['eager'] / med['kd4']),
              'distillation launches of one (b) step (engine.kd.stats()): %s' % launches]
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
