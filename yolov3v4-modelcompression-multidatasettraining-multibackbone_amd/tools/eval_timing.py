"""Time of the statistics stage of an evaluation batch (test.py, after forward + NMS): the per-image host loop against the device matcher.

    python tools/eval_timing.py [--out profiles/eval_match_timing.txt] [--repeats 15]

Inputs (synthetic, fixed seed, the same tensors for both forms): a batch of BATCH = 16 images of SIZE = 512 x 512, ROWS = 1000 NMS
survivors and LABELS = 20 labels of NC = 80 classes per image; COPY_SHARE = 30 % of the rows are label boxes with a jitter of up to
+-JITTER = 4 pixels per corner and the label's class (so that claims actually happen), the rest random boxes of random class, some
of them over the image border.  iouv is test.py's (one threshold, 0.5).
  host loop      test.host_stats, the loop test.py runs with YOLO_HIP_EVAL_MATCH=0 (and ran before the device matcher existed): per
                 image a mask over the targets, tolist, clip_coords, test._match, three .cpu() reads
  match_batch    engine/evalmatch.py: one table copy, one launch of yh_eval_match, one read
Synchronised wall clock around each form, WARMUP = 3 untimed rounds, then --repeats rounds that alternate the two; the medians are
reported, and that both forms gave the same statistics.  Then test.test end to end on the synthetic image set of tests/conftest.py
(12 PNG images, 4 of them in the validation split; the 21-block cfg of tests/train_harness.py, random weights, 64 x 64) both ways,
alternating, median seconds.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402
import torch  # noqa: E402

BATCH, SIZE, ROWS, LABELS, NC, COPY_SHARE, JITTER, WARMUP = 16, 512, 1000, 20, 80, 0.3, 4.0, 3


def make_batch(dev):
    rng = np.random.RandomState(0)
    out, targets = [], []
    for i in range(BATCH):
        wh = rng.uniform(0.05, 0.5, (LABELS, 2))
        xy = rng.uniform(0, 1, (LABELS, 2)) * (1 - wh) + wh / 2
        cls = rng.randint(0, NC, LABELS)
        targets.append(np.concatenate([np.full((LABELS, 1), i), cls[:, None], xy, wh], 1))
        x1, y1 = rng.uniform(-20, SIZE, ROWS), rng.uniform(-20, SIZE, ROWS)
        box = np.stack([x1, y1, x1 + rng.uniform(4, 200, ROWS), y1 + rng.uniform(4, 200, ROWS)], 1)
        pcls = rng.randint(0, NC, ROWS).astype(np.float64)
        for p in np.nonzero(rng.uniform(size=ROWS) < COPY_SHARE)[0]:
            t = rng.randint(LABELS)
            box[p] = np.concatenate([xy[t] - wh[t] / 2, xy[t] + wh[t] / 2]) * SIZE + rng.uniform(-JITTER, JITTER, 4)
            pcls[p] = cls[t]
        conf = np.sort(rng.uniform(0.001, 1, ROWS))[::-1]
        out.append(np.concatenate([box, conf[:, None], pcls[:, None]], 1).astype(np.float32))
    buf = torch.from_numpy(np.stack(out)).to(dev)                 # (BATCH, ROWS, 6): NMS hands out views into one buffer
    return [buf[i] for i in range(BATCH)], torch.from_numpy(np.concatenate(targets).astype(np.float32))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def synthetic_dataset(root):
    """the image set of tests/conftest.py (dataset_dir): same recipe and seed"""
    from PIL import Image
    os.makedirs(os.path.join(root, 'images'))
    os.makedirs(os.path.join(root, 'labels'))
    rng = np.random.RandomState(0)
    files = []
    for i in range(12):
        w, h = int(rng.randint(90, 160)), int(rng.randint(70, 140))
        img = (rng.rand(h, w, 3) * 40).astype(np.uint8)
        rows = []
        for _ in range(rng.randint(1, 4)):
            bw, bh = rng.uniform(0.2, 0.5), rng.uniform(0.2, 0.5)
            cx, cy = rng.uniform(bw / 2, 1 - bw / 2), rng.uniform(bh / 2, 1 - bh / 2)
            x1, x2, y1, y2 = int((cx - bw / 2) * w), int((cx + bw / 2) * w), int((cy - bh / 2) * h), int((cy + bh / 2) * h)
            img[y1:y2, x1:x2] = rng.randint(150, 255, 3)
            rows.append('%d %.6f %.6f %.6f %.6f' % (0 if bw * w > bh * h else 1, cx, cy, bw, bh))
        p = os.path.join(root, 'images', 'im_%02d.png' % i)
        Image.fromarray(img).save(p)
        open(os.path.join(root, 'labels', 'im_%02d.txt' % i), 'w').write('\n'.join(rows) + '\n')
        files.append(p)
    for name, part in (('train', files[:8]), ('valid', files[8:])):
        open(os.path.join(root, name + '.txt'), 'w').write('\n'.join(part) + '\n')
    open(os.path.join(root, 'synth.names'), 'w').write('wide\ntall\n')
    data = os.path.join(root, 'synth.data')
    open(data, 'w').write('classes=2\ntrain=%s\nvalid=%s\nnames=%s\n' % (os.path.join(root, 'train.txt'), os.path.join(root, 'valid.txt'),
                                                                      os.path.join(root, 'synth.names')))
    return data


def end_to_end(test_mod, repeats):
    sys.path.insert(0, os.path.join(os.path.dirname(PKG), 'tests'))
    import train_harness as th
    from models import Darknet
    times = {'0': [], '1': []}
    with tempfile.TemporaryDirectory() as tmp:
        data = synthetic_dataset(tmp)
        cfg = os.path.join(tmp, 'mini2.cfg')
        open(cfg, 'w').write(th.mini_cfg_text())
        torch.manual_seed(3)
        model = Darknet(cfg, (64, 64)).cuda()
        test_mod.opt = None
        results = {}
        for r in range(WARMUP + repeats):
            for flag in ('0', '1'):
                os.environ['YOLO_HIP_EVAL_MATCH'] = flag
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results[flag] = test_mod.test(cfg, data, batch_size=2, imgsz=64, model=model, plot=False)
                torch.cuda.synchronize()
                if r >= WARMUP:
                    times[flag].append(time.perf_counter() - t0)
        os.environ.pop('YOLO_HIP_EVAL_MATCH', None)
    same = results['0'][0][:4] == results['1'][0][:4] and np.array_equal(results['0'][1], results['1'][1])
    return statistics.median(times['0']), statistics.median(times['1']), same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(PKG), 'profiles', 'eval_match_timing.txt'))
    ap.add_argument('--repeats', type=int, default=15)
    args = ap.parse_args()
    assert args.repeats >= 10
    import test as test_mod
    from engine import evalmatch
    dev = torch.device('cuda', 0)
    output, t_host = make_batch(dev)
    t_dev = t_host.to(dev)
    iouv = torch.linspace(0.5, 0.95, 10).to(dev)[0].view(1)
    forms = {'host': lambda: test_mod.host_stats(output, t_dev, SIZE, SIZE, iouv),
             'device': lambda: evalmatch.match_batch(output, t_host, t_dev, SIZE, SIZE, iouv)}
    ms = {'host': [], 'device': []}
    res = {}
    for r in range(WARMUP + args.repeats):
        for name in ('host', 'device'):
            t, res[name] = timed(forms[name])
            if r >= WARMUP:
                ms[name].append(t)
    same = len(res['host']) == len(res['device']) and all(
        torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] for a, b in zip(res['host'], res['device']))
    tp = int(sum(int(s[0].sum()) for s in res['device']))
    mh, md = statistics.median(ms['host']), statistics.median(ms['device'])
    e0, e1, esame = end_to_end(test_mod, 5)
    lines = [
        'Statistics stage of an evaluation batch (test.py after forward + NMS): per-image host loop against the device matcher',
        'tools/eval_timing.py on %s (%s); torch %s' % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, torch.__version__),
        'inputs: batch %d, %d x %d, %d NMS rows and %d labels of %d classes per image, %.0f %% of the rows label boxes with +-%.0f px jitter; '
        'niou 1; %d true positives in the batch' % (BATCH, SIZE, SIZE, ROWS, LABELS, NC, 100 * COPY_SHARE, JITTER, tp),
        'synchronised wall clock, %d warm-up rounds, median of %d alternating repeats' % (WARMUP, args.repeats),
        '',
        'per batch   host loop (YOLO_HIP_EVAL_MATCH=0)  %9.3f ms   (min %.3f, max %.3f)' % (mh, min(ms['host']), max(ms['host'])),
        'per batch   match_batch (yh_eval_match)       %9.3f ms   (min %.3f, max %.3f)' % (md, min(ms['device']), max(ms['device'])),
        'per batch   host loop / match_batch            %9.1f x;  statistics of the two forms %s' % (mh / md, 'IDENTICAL' if same else 'DIFFER'),
        '',
        'test.test end to end, synthetic image set of tests/conftest.py (4 validation images, 2 batches, 64 x 64, random weights), median of 5:',
        'end to end  host loop (YOLO_HIP_EVAL_MATCH=0)  %9.4f s' % e0,
        'end to end  match_batch                        %9.4f s' % e1,
        'end to end  host loop / match_batch            %9.2f x;  (mp, mr, map50, mf1) and maps %s' % (e0 / e1, 'IDENTICAL' if esame else 'DIFFER'),
    ]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write(text)


if __name__ == '__main__':
    main()
