"""Time of one augmented-inference batch (`--augment`): the three forwards + torch glue + row-tensor NMS against the one engine call.

    python tools/tta_timing.py [--out profiles/tta_timing.txt] [--repeats 15]

Inputs (synthetic, fixed seed, the same frames for both forms): --batch 16 frames of --size 608 x 608, YOLOv3 (80 classes) with
seeded random weights and BatchNorm statistics, --precision fp16.  Random heads score every row near the same value, so each
setting's confidence threshold is placed by a quantile of the scores of the composed tensor: OBJ_SHARE = 0.4 % of the rows above the
objectness threshold at detect.py's setting (best class - its conf 0.3 keeps that share of a trained model's rows), and the
ML_PER_IMAGE = 20 000 best (row, class) scores per image at test.py's (multi-label - what its conf 0.001 leaves of a trained model).
  A  non_max_suppression(model(x, augment=True)[0], ...): what the scripts ran before hip_detect took `augment` (YOLO_HIP_TTA=0) -
     flip / F.interpolate / F.pad per view, three engine forwards with their decoded tensors, torch's de-augmentation, torch.cat, the
     row-tensor NMS
  B  model.hip_detect(x, ..., augment=True): yh_tta_view per scaled view, the plans up to their head convolutions, one decode +
     de-augment + filter pass per (view, head), the NMS steps
Synchronised wall clock around each form, WARMUP = 3 untimed rounds, then --repeats rounds that alternate the two; medians.  The
detection lists of the two forms are compared by twins (same class, IoU >= TWIN_IOU = 0.98): they are close, not identical - A resizes
its views with ATen's bilinear kernel and divides by multiplying with a reciprocal, B with yh_tta_view and IEEE division, and an
fp16 network sits behind the views.  The kernel launches of one call are counted with torch's profiler where it is available.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, PKG)

import torch  # noqa: E402

WARMUP, OBJ_SHARE, ML_PER_IMAGE, TWIN_IOU = 3, 0.004, 20000, 0.98


def make_model(cfg, size, precision, dev):
    import models
    torch.manual_seed(0)
    m = models.Darknet(cfg, (size, size))
    g = torch.Generator().manual_seed(1)
    state = m.state_dict()
    for k, v in state.items():
        if k.endswith('running_var') or k.endswith('BatchNorm2d.weight'):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith('running_mean') or k.endswith('BatchNorm2d.bias'):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    m.load_state_dict(state)
    m.to(dev).eval()
    m.hip_precision = precision
    m.hip_return_raw = False
    return m


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


def compare(a, b):
    """How close two detection lists are: (detections of a, of b, detections of a with a twin in b, of b with a twin in a).  A twin has
    the same class and IoU >= TWIN_IOU.  The two forms resize their views with different kernels (ATen's bilinear against
    yh_tta_view: same formula, other rounding) in front of an fp16 network, so rows next to the threshold come and go and the lists
    are not expected to be identical; what each form computes is pinned by tests/test_gpu_tta.py and tests/test_gpu_network.py."""
    from utils.utils import box_iou
    na = nb = ta = tb = 0
    for p, q in zip(a, b):
        na += 0 if p is None else len(p)
        nb += 0 if q is None else len(q)
        if p is None or q is None:
            continue
        for lo in range(0, len(p), 2048):
            part = p[lo:lo + 2048]
            twin = (box_iou(part[:, :4], q[:, :4]) >= TWIN_IOU) & (part[:, 5:6] == q[:, 5][None])
            ta += int(twin.any(1).sum())
        for lo in range(0, len(q), 2048):
            part = q[lo:lo + 2048]
            twin = (box_iou(part[:, :4], p[:, :4]) >= TWIN_IOU) & (part[:, 5:6] == p[:, 5][None])
            tb += int(twin.any(1).sum())
    return na, nb, ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=os.path.join(PKG, 'cfg', 'yolov3', 'yolov3.cfg'))
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=608)
    ap.add_argument('--precision', default='fp16')
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--no-launches', action='store_true', help='skip the profiled calls')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'tta_timing.txt'))
    args = ap.parse_args()
    assert args.repeats >= 10
    from utils.utils import non_max_suppression
    dev = torch.device('cuda', 0)
    model = make_model(args.cfg, args.size, args.precision, dev)
    x = torch.rand(args.batch, 3, args.size, args.size, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        inf = model(x, augment=True)[0]
        rows = inf.shape[1]
        obj = inf[..., 4].flatten()
        conf_detect = float(obj.float().kthvalue(max(1, int(obj.numel() * (1 - OBJ_SHARE)))).values)
        conf_test = float((inf[..., 5:] * inf[..., 4:5]).flatten().topk(ML_PER_IMAGE * args.batch).values[-1])
        del inf, obj
        settings = [("detect.py's (best class)", conf_detect, False), ("test.py's (multi-label)", conf_test, True)]
        lines = ['Augmented inference (--augment) per batch: three forwards + torch glue + row-tensor NMS (A) against one engine call (B)',
                 'tools/tta_timing.py on %s (%s); torch %s' % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                                               torch.__version__),
                 'inputs: %s, batch %d, %d x %d, %s, %d rows per image over the three views; seeded random weights' %
                 (os.path.basename(args.cfg), args.batch, args.size, args.size, args.precision, rows),
                 'synchronised wall clock, %d warm-up rounds, median of %d alternating repeats' % (WARMUP, args.repeats), '']
        for name, conf, ml in settings:
            forms = {'A': lambda: non_max_suppression(model(x, augment=True)[0], conf, 0.6, multi_label=ml),
                     'B': lambda: model.hip_detect(x, conf, 0.6, multi_label=ml, augment=True)}
            ms, res = {'A': [], 'B': []}, {}
            for r in range(WARMUP + args.repeats):
                for form in ('A', 'B'):
                    t, res[form] = timed(forms[form])
                    if r >= WARMUP:
                        ms[form].append(t)
            ma, mb = statistics.median(ms['A']), statistics.median(ms['B'])
            na, nb, ta, tb = compare(res['A'], res['B'])
            lines += ['%s setting: conf %.6g, iou 0.6' % (name, conf),
                      '  A  model(x, augment=True) + non_max_suppression  %9.3f ms   (min %.3f, max %.3f)' % (ma, min(ms['A']), max(ms['A'])),
                      '  B  hip_detect(x, ..., augment=True)              %9.3f ms   (min %.3f, max %.3f)' % (mb, min(ms['B']), max(ms['B'])),
                      '  A / B %.3f x;  detections in the batch: A %d, B %d; with a twin in the other list (same class, IoU >= %.2f): '
                      '%d of A (%.2f %%), %d of B (%.2f %%)' % (ma / mb, na, nb, TWIN_IOU, ta, 100.0 * ta / max(na, 1), tb, 100.0 * tb / max(nb, 1))]
            if not args.no_launches:
                try:
                    lines.append('  kernel launches per call: A %d, B %d' % (launches(forms['A']), launches(forms['B'])))
                except Exception as e:      # the profiler is optional equipment
                    lines.append('  kernel launches per call: not available (%s)' % type(e).__name__)
            lines.append('')
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
