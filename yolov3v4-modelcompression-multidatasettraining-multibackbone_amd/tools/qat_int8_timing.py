"""Time of one evaluation batch of a QAT (``--quantized 1``) model: the eager modules against the int8 engine.

    python tools/qat_int8_timing.py [--out profiles/qat_int8_timing.txt] [--repeats 15]
    python tools/qat_int8_timing.py --eager-only --pkg <package dir of another checkout>      # the baseline figure

Workload: YOLOv3 (80 classes), --batch 16 frames of --size 608 x 608, ``quantized=1`` in the synthetic calibrated state of
``tools/synthetic_ptq.py`` (``fill_synthetic_qat_state``; ranges measured on two frames), eval mode, on the GPU.
  E  YOLO_HIP_QAT_INT8=0: the eager modules - ATen fp32 convolutions around the fused fake-quant passes of engine/qat.py
  I  the int8 engine: the lowered plan on the MFMA-i8 kernels (engine/plan.py), the step counters advanced by one multi-tensor add
each in detect.py's form (``model.hip_detect(x, conf, iou)``, best class) and in test.py's form (``model(x)`` + multi-label
``non_max_suppression``).  Random heads score every row near the same value, so each form's confidence threshold is placed by a
quantile of the engine's scores: OBJ_SHARE of the rows above the objectness threshold for detect.py's form, the ML_PER_IMAGE best
(row, class) scores per image for test.py's.  Synchronised wall clock around each call, WARMUP untimed rounds, then --repeats rounds
that alternate the legs; median and spread (max - min) per leg, kernel launches of one call from torch's profiler where available.

``--eager-only`` times leg E alone and, with the switch at 0, calls nothing but ``models.Darknet``: with ``--pkg`` pointing at a
checkout that has no QAT lowering (the parent commit) it gives the baseline the eager leg of this commit must agree with.  The
synthetic state always comes from THIS file's directory."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))

import torch  # noqa: E402

WARMUP, OBJ_SHARE, ML_PER_IMAGE = 3, 0.004, 2000


def make_model(cfg, size, dev):
    import models
    spec = importlib.util.spec_from_file_location('qat_int8_timing_synthetic', os.path.join(HERE, 'synthetic_ptq.py'))
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    frames = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(3))
    torch.manual_seed(0)
    fm = models.Darknet(cfg, (size, size))
    synth.seed_qat_batchnorm_(fm, frames)
    torch.manual_seed(0)
    qm = models.Darknet(cfg, (size, size), quantized=1, a_bit=8, w_bit=8, shortcut_way=1, steps=0)
    synth.fill_synthetic_qat_state(fm, qm, synth.measure_ranges(fm, frames))
    return qm.to(dev).eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def launches(fn):
    from torch.profiler import ProfilerActivity, profile as prof
    with prof(activities=[ProfilerActivity.CUDA]) as p:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in p.key_averages() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower())


def count(dets):
    return sum(0 if d is None else len(d) for d in dets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pkg', default=os.path.dirname(HERE), help='package directory to import models / engine from')
    ap.add_argument('--cfg', default=None)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--eager-only', action='store_true', help='leg E alone (the baseline run on another checkout)')
    ap.add_argument('--conf', type=float, nargs=2, default=None, help="the two thresholds (an --eager-only run takes the full run's)")
    ap.add_argument('--no-launches', action='store_true', help='skip the profiled calls')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.repeats >= 10
    pkg = os.path.abspath(args.pkg)
    sys.path.insert(0, pkg)
    cfg = args.cfg or os.path.join(pkg, 'cfg', 'yolov3', 'yolov3.cfg')
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(HERE)), 'profiles',
                                   'qat_int8_timing_eager_only.txt' if args.eager_only else 'qat_int8_timing.txt')
    from utils.utils import non_max_suppression
    dev = torch.device('cuda', 0)
    model = make_model(cfg, args.size, dev)
    x = torch.rand(args.batch, 3, args.size, args.size, generator=torch.Generator().manual_seed(2)).to(dev)

    def leg(switch, fn):
        def run():
            os.environ['YOLO_HIP_QAT_INT8'] = switch
            return fn()
        return run
    with torch.no_grad():
        os.environ['YOLO_HIP_QAT_INT8'] = '0' if args.eager_only else '1'
        inf = model(x)[0]
        rows = inf.shape[1]
        if args.conf:
            conf_detect, conf_test = args.conf
        else:
            obj = inf[..., 4].flatten()
            conf_detect = float(obj.float().kthvalue(max(1, int(obj.numel() * (1 - OBJ_SHARE)))).values)
            conf_test = float((inf[..., 5:] * inf[..., 4:5]).flatten().topk(ML_PER_IMAGE * args.batch).values[-1])
            del obj
        del inf
        on_engine = getattr(model.__dict__.get('_hip_engine'), 'precision', None)
        forms = [("detect.py's form: hip_detect, best class", conf_detect, lambda: model.hip_detect(x, conf_detect, 0.6, multi_label=False)),
                 ("test.py's form: model(x) + multi-label NMS", conf_test,
                  lambda: non_max_suppression(model(x)[0], conf_test, 0.6, multi_label=True))]
        lines = ['Evaluation batch of a QAT (--quantized 1) model: eager modules (E, YOLO_HIP_QAT_INT8=0) against the int8 engine (I)',
                 'tools/qat_int8_timing.py on %s (%s); torch %s; package %s' % (
                     torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.__version__,
                     'of this checkout' if pkg == os.path.dirname(HERE) else 'of another checkout (--pkg)'),
                 'inputs: %s, batch %d, %d x %d, %d rows per image; synthetic QAT state, seeded weights' %
                 (os.path.basename(cfg), args.batch, args.size, args.size, rows),
                 'synchronised wall clock, %d warm-up rounds, median and spread (max - min) of %d alternating repeats' % (WARMUP, args.repeats),
                 'first call ran on: %s' % ('the eager modules' if on_engine is None else 'the %s engine' % on_engine), '']
        for name, conf, fn in forms:
            legs = {'E': leg('0', fn)} if args.eager_only else {'E': leg('0', fn), 'I': leg('1', fn)}
            ms, res = {k: [] for k in legs}, {}
            for r in range(WARMUP + args.repeats):
                for k in legs:
                    t, res[k] = timed(legs[k])
                    if r >= WARMUP:
                        ms[k].append(t)
            lines.append('%s; conf %.6g, iou 0.6' % (name, conf))
            label = {'E': 'E  eager modules', 'I': 'I  int8 engine  '}
            for k in legs:
                med = statistics.median(ms[k])
                lines.append('  %s  %9.3f ms   (min %.3f, max %.3f, spread %.3f)   %8.1f images/s   %d detections' %
                             (label[k], med, min(ms[k]), max(ms[k]), max(ms[k]) - min(ms[k]), args.batch / med * 1e3, count(res[k])))
            if 'I' in legs:
                me, mi = statistics.median(ms['E']), statistics.median(ms['I'])
                spread = max(max(ms['E']) - min(ms['E']), max(ms['I']) - min(ms['I']))
                lines.append('  E / I %.2f x;  E - I = %.3f ms against the larger spread %.3f ms: %s' %
                             (me / mi, me - mi, spread, 'the engine is ahead by more than both spreads' if me - mi > spread else
                              'NOT ahead by more than both spreads'))
            if not args.no_launches:
                try:
                    lines.append('  kernel launches per call: ' + ', '.join('%s %d' % (k, launches(legs[k])) for k in legs))
                except Exception as e:      # the profiler is optional equipment
                    lines.append('  kernel launches per call: not available (%s)' % type(e).__name__)
            lines.append('')
    os.environ.pop('YOLO_HIP_QAT_INT8', None)
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, 'w').write(text)


if __name__ == '__main__':
    main()
