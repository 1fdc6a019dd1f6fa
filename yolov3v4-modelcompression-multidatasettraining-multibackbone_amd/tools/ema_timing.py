"""Times of one `ModelEMA.update` (`train.py --ema`) as one `yh_ema_update` launch and as the per-tensor torch loop.

    python tools/ema_timing.py [--updates 30] [--warmup 5] [--rounds 3] [--parent DIR] [--out profiles/ema_timing.txt]

Builds the YOLOv3 and YOLOv4 graphs on one device (state dicts only: no forward pass), and for each graph alternates runs of the
device path (csrc/ema.hip through engine/ema.py) and of ``YOLO_HIP_EMA=0`` (the torch statement per tensor).  Every update records
  device ms   between two events on the stream, around the update
  host ms     the time the call takes to return (no synchronisation inside), i.e. what the training loop's thread pays
Both legs are bound by the host on these graphs, so the device ms is the span of the update on the stream, not the time the device
is busy.  Reported: median and min .. max over all timed updates of a leg, and - where torch's profiler gives them - the kernel
launches of one update and the ms the device was busy in them (kernel ms).  ``--parent DIR`` names the package directory of a
checkout of the parent commit: its ``ModelEMA`` (the torch loop, nothing else exists there) is timed the same way in a child
process of its own, as the check that the torch baseline of this file is the parent's.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
GRAPHS = (('YOLOv3', os.path.join('cfg', 'yolov3', 'yolov3.cfg')), ('YOLOv4', os.path.join('cfg', 'yolov4', 'yolov4.cfg')))


def timed_updates(ema, model, n, warmup):
    """[(device ms, host ms)] of n updates after ``warmup`` untimed ones."""
    import torch
    for _ in range(warmup):
        ema.update(model)
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        ema.update(model)
        host = (time.perf_counter() - t0) * 1e3
        b.record()
        torch.cuda.synchronize()
        out.append((a.elapsed_time(b), host))
    return out


def launches(ema, model):
    """(kernel launches, ms the device was busy in them) of one update under torch's profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile as prof
    torch.cuda.synchronize()
    with prof(activities=[ProfilerActivity.CUDA]) as p:
        ema.update(model)
        torch.cuda.synchronize()
    kernels = [e for e in p.key_averages() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower()]
    busy = sum(getattr(e, 'self_device_time_total', getattr(e, 'self_cuda_time_total', 0)) for e in kernels)
    return sum(e.count for e in kernels), busy / 1e3


def measure(pkg, legs, args):
    """{graph: {leg: dict(times=[(device, host)], launches=int or None)}} with the package at ``pkg``; the legs alternate per round."""
    sys.path.insert(0, pkg)
    import torch
    from models import Darknet
    from utils.torch_utils import ModelEMA
    dev = torch.device('cuda', 0)
    before = os.environ.get('YOLO_HIP_EMA')
    res = {}
    try:
        for name, cfg in GRAPHS:
            torch.manual_seed(0)
            model = Darknet(os.path.join(pkg, cfg), (608, 608)).to(dev)
            emas = {leg: ModelEMA(model) for leg in legs}
            res[name] = {leg: dict(times=[], launches=None, busy=None) for leg in legs}
            tensors = [v for v in model.state_dict().values() if v.dtype.is_floating_point]
            res[name]['_shape'] = (len(tensors), sum(v.numel() for v in tensors))
            for _ in range(args.rounds):
                for leg in legs:
                    os.environ['YOLO_HIP_EMA'] = '0' if leg == 'torch' else '1'
                    res[name][leg]['times'].extend(timed_updates(emas[leg], model, args.updates, args.warmup))
            if not args.no_launches:
                for leg in legs:
                    os.environ['YOLO_HIP_EMA'] = '0' if leg == 'torch' else '1'
                    try:
                        res[name][leg]['launches'], res[name][leg]['busy'] = launches(emas[leg], model)
                    except Exception:      # the profiler is optional equipment
                        pass
            del model, emas
            torch.cuda.empty_cache()
    finally:
        if before is None:
            os.environ.pop('YOLO_HIP_EMA', None)
        else:
            os.environ['YOLO_HIP_EMA'] = before
    return res


def row(label, r):
    dv, hs = [t[0] for t in r['times']], [t[1] for t in r['times']]
    return '%-22s %9.3f %9.3f ..%8.3f %9.3f %9.3f ..%8.3f %9s %10s' % (label, statistics.median(dv), min(dv), max(dv), statistics.median(hs), min(hs),
                                                                      max(hs), '-' if r['launches'] is None else r['launches'],
                                                                      '-' if r['busy'] is None else '%.3f' % r['busy'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--updates', type=int, default=30, help='timed updates per run')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='alternating runs per leg')
    ap.add_argument('--parent', default='', help='package directory of a checkout of the parent commit')
    ap.add_argument('--no-launches', action='store_true', help='skip the profiled update')
    ap.add_argument('--child', default='', help=argparse.SUPPRESS)      # internal: measure the torch leg of the package at this path
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'ema_timing.txt'))
    args = ap.parse_args()
    if args.child:
        res = measure(os.path.abspath(args.child), ('torch',), args)
        print('EMA_TIMING_CHILD ' + json.dumps(res))
        return
    import torch
    res = measure(PKG, ('device', 'torch'), args)
    parent = None
    if args.parent:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', args.parent, '--updates', str(args.updates), '--warmup', str(args.warmup),
               '--rounds', str(args.rounds)] + (['--no-launches'] if args.no_launches else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        hit = [l for l in out.stdout.splitlines() if l.startswith('EMA_TIMING_CHILD ')]
        if out.returncode != 0 or not hit:
            raise RuntimeError('the parent-commit run failed:\n' + out.stdout[-2000:] + out.stderr[-2000:])
        parent = json.loads(hit[-1][len('EMA_TIMING_CHILD '):])
    n = args.rounds * args.updates
    lines = ['ModelEMA.update: one yh_ema_update launch (device) against the per-tensor torch loop (YOLO_HIP_EMA=0), fp32 state dicts, %s'
             % torch.cuda.get_device_name(0),
             'median and min .. max of %d updates per leg (%d alternating runs of %d updates, %d warm-up updates each); device ms between '
             'stream events, host ms until the call returns' % (n, args.rounds, args.updates, args.warmup)]
    for name, _ in GRAPHS:
        tensors, elements = res[name]['_shape']
        lines.append('')
        lines.append('%s: %d floating-point tensors, %d elements' % (name, tensors, elements))
        lines.append('%-22s %9s %20s %9s %20s %9s %10s' % ('leg', 'device ms', 'min .. max', 'host ms', 'min .. max', 'launches', 'kernel ms'))
        lines.append(row('device (one launch)', res[name]['device']))
        lines.append(row('torch loop', res[name]['torch']))
        if parent is not None:
            lines.append(row('torch loop, parent', parent[name]['torch']))
        med = lambda leg, i: statistics.median(t[i] for t in res[name][leg]['times'])
        lines.append('torch / device: device time %.2f, host time %.2f' % (med('torch', 0) / med('device', 0), med('torch', 1) / med('device', 1)))
        busy = res[name]['device']['busy']
        lines.append('bytes one pass moves (read ema, read src, write ema): %.0f MB%s'
                     % (12 * elements / 1e6, '' if not busy else '; over the kernel ms of the one launch: %.0f GB/s' % (12 * elements / 1e9 / (busy / 1e3))))
    text = '\n'.join(lines) + '\n'
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)
    print(text, end='')


if __name__ == '__main__':
    main()
