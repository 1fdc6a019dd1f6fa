"""The mixed evaluation batch shared by tests/test_eval_match.py (host emulation) and tests/test_gpu_eval_match.py (the kernel), and
its expected results from the host loop of ``test.py``: ``clip_coords`` plus ``test._match`` per image on CPU copies.

One batch on a 64 x 48 image holds every case of the matcher's contract:
  image 0  no detections (None), no labels            image 1  detections, no labels
  image 2  labels, no detections (None)               image 3  1 detection, 1 label
  image 4  300 detections (a 256-thread group walks them in two trips, the last wave straddles the end), 12 labels: two duplicated
           labels (tie on the label index), four exact copies of one label box (tie on the claimant), a wrong-class copy, detections
           of a class no label has, a label class no detection has, boxes partly and wholly outside the image, NaN / inf corners
  image 5  40 detections, one label more than the kernel stages in LDS (its chunked form): a detection whose best label of the first
           chunk is beaten by the one label of the second
  image 8  30 detections, two chunks and three labels: winners in every chunk, a label duplicated across chunks (tie to the earlier)
  image 6  the exact-0.5 pair: detection (0, 0, 32, 16) against label xywh (8, 8, 16, 16) / (64, 48) - IoU 256 / 512, no claim
  image 7  an empty (0, 6) detection tensor with labels
The targets of the images are interleaved at random, so the rows of one image are neither adjacent nor first; the detections are views into TWO buffers.
"""
import numpy as np
import torch

from engine import hiplib
from engine.hiplib import EVAL_MATCH_LDS_LABELS

W, H = 64, 48
NB = 9
IOUV = {1: torch.tensor([0.5]), 10: torch.linspace(0.5, 0.95, 10)}


def _labels(rng, n, classes):
    wh = rng.uniform(0.1, 0.5, (n, 2))
    xy = rng.uniform(0, 1, (n, 2)) * (1 - wh) + wh / 2
    return np.concatenate([rng.choice(classes, (n, 1)).astype(np.float64), xy, wh], 1).astype(np.float32)


def _pixels(lab):
    """float32 xyxy of label rows (cls, x, y, w, h), with the operation order of xywh2xyxy(...) * whwh"""
    x, y, w, h = (lab[:, i].astype(np.float32) for i in (1, 2, 3, 4))
    two = np.float32(2)
    return np.stack([(x - w / two) * np.float32(W), (y - h / two) * np.float32(H), (x + w / two) * np.float32(W),
                     (y + h / two) * np.float32(H)], 1).astype(np.float32)


def _dets(rng, n, lab, classes, copy_share=0.3):
    """n detections: a share copied from the labels with jitter (so that claims happen), the rest random boxes that may leave the image"""
    x1 = rng.uniform(-12, W, n)
    y1 = rng.uniform(-12, H, n)
    box = np.stack([x1, y1, x1 + rng.uniform(1, 30, n), y1 + rng.uniform(1, 30, n)], 1)
    cls = rng.choice(classes, n).astype(np.float64)
    if len(lab):
        px = _pixels(lab)
        for p in np.nonzero(rng.uniform(size=n) < copy_share)[0]:
            t = rng.randint(len(lab))
            box[p] = px[t] + rng.uniform(-2.5, 2.5, 4)
            cls[p] = lab[t, 0]
    conf = rng.uniform(0.001, 1, n)
    return np.concatenate([box, conf[:, None], cls[:, None]], 1).astype(np.float32)


def build():
    """(dets: list of (n, 6) float32 arrays or None per image, targets (nt, 6) float32 array, shuffled)"""
    rng = np.random.RandomState(7)
    dets, labs = [None] * NB, [np.zeros((0, 5), np.float32)] * NB
    dets[1] = _dets(rng, 9, labs[1], [0, 1])
    labs[2] = _labels(rng, 3, [0, 1])
    labs[3] = np.array([[1, 0.5, 0.5, 0.4, 0.5]], np.float32)
    dets[3] = np.array([[20, 13, 44, 35, 0.9, 1]], np.float32)

    lab4 = _labels(rng, 12, [0, 1, 2])
    lab4[5] = lab4[1]                    # duplicated labels: the lower index wins the tie
    lab4[9] = lab4[1]
    lab4[7] = lab4[2]
    lab4[11, 0] = 5                      # a label class no detection has
    d4 = _dets(rng, 300, lab4[:11], [0, 1, 2, 3])      # class 3: no label has it
    px = _pixels(lab4)
    for p in (1, 40, 41, 299):          # exact copies of one label box: the lowest detection index wins it
        d4[p, :4], d4[p, 5] = px[3], lab4[3, 0]
    d4[0, :4], d4[0, 5] = px[1], lab4[1, 0]            # exact copies of the duplicated label
    d4[260, :4], d4[260, 5] = px[1], lab4[1, 0]
    d4[19, :4], d4[19, 5] = px[4], (lab4[4, 0] + 1) % 3      # wrong-class copy
    d4[20, :4] = (-30, -20, -5, -2)      # wholly outside: zero area after the clip
    d4[21, :4] = (70, 10, 90, 30)
    d4[22, :4] = (-10, -10, 80, 60)      # covers the image
    d4[23, :4] = (10, 50, 30, 70)
    d4[24, 0] = np.nan                   # non-finite corners: all-false rows, the NaN is kept by the clip
    d4[25, 3] = np.nan
    d4[26, :4] = (-np.inf, 5, np.inf, 30)
    dets[4], labs[4] = d4, lab4

    # one label more than the staging holds: two chunks, the second of one label.  Classes 7 / 8 belong to the placed labels alone, and
    # the placed detections come first, so what they win is known: the label of the second chunk (in-image index CAP) is a shifted copy
    # (IoU 0.78) of label 5, and detection 1 sits exactly on it - its running best of the first chunk (label 5, 0.78) is beaten in the
    # second.  Detection 0 sits on label 0 and wins it, so a kernel that drops the chunk offset sends detection 1 to a taken slot.
    CAP = EVAL_MATCH_LDS_LABELS
    B0, B1, C2 = (7, 0.5, 0.5, 0.5, 0.5), (7, 0.5625, 0.5, 0.5, 0.5), (8, 0.3, 0.3, 0.2, 0.25)
    copy_of = lambda lab, t: np.concatenate([_pixels(lab[t:t + 1])[0], [0.5, lab[t, 0]]]).astype(np.float32)
    lab5 = _labels(rng, CAP + 1, [0, 1, 2])
    lab5[5], lab5[CAP] = B0, B1
    d5 = _dets(rng, 40, lab5, [0, 1, 2], copy_share=0.6)
    d5[0], d5[1], d5[2] = copy_of(lab5, 0), copy_of(lab5, CAP), copy_of(lab5, 5)
    dets[5], labs[5] = d5, lab5

    labs[6] = np.array([[2, 8 / 64, 8 / 48, 16 / 64, 16 / 48]], np.float32)
    dets[6] = np.array([[0, 0, 32, 16, 0.7, 2]], np.float32)
    labs[7] = _labels(rng, 2, [0, 1])
    dets[7] = np.zeros((0, 6), np.float32)

    # three chunks, the last of three labels: label CAP + 9 improves on label 5 for detection 2; label 2 CAP + 1 duplicates label 5 (the
    # tie goes to the earlier chunk: detections 3 and 4 both sit on it, 3 wins label 5, 4 wins nothing); label 2 CAP + 2 is alone in
    # its class, detection 5 sits on it.  Detections 0 and 1 win labels 9 and 2, the slots a dropped chunk offset would hit.
    lab8 = _labels(rng, 2 * CAP + 3, [0, 1, 2])
    lab8[5], lab8[CAP + 9], lab8[2 * CAP + 1], lab8[2 * CAP + 2] = B0, B1, B0, C2
    d8 = _dets(rng, 30, lab8, [0, 1, 2], copy_share=0.6)
    for p, t in enumerate((9, 2, CAP + 9, 5, 2 * CAP + 1, 2 * CAP + 2)):
        d8[p] = copy_of(lab8, t)
    dets[8], labs[8] = d8, lab8

    # shuffled over the batch, the order inside an image kept: the rows of one image are neither adjacent nor first, and the in-image
    # label index - the order of appearance, which is what targets[targets[:, 0] == si] and the kernel's label_index see - is labs[si]'s
    ids = rng.permutation(np.concatenate([np.full(len(l), i) for i, l in enumerate(labs)]))
    rows = np.zeros((len(ids), 6), np.float32)
    for i, l in enumerate(labs):
        rows[ids == i, 0], rows[ids == i, 1:] = i, l
    assert len(np.unique(np.diff(np.nonzero(ids == 5)[0]))) > 1
    return dets, rows


def output_views(dets, device):
    """The detections as views into two device buffers, like a chunked NMS call returns them"""
    groups = [[i for i, d in enumerate(dets) if d is not None and i <= 4], [i for i, d in enumerate(dets) if d is not None and i > 4]]
    out, bufs = [None] * len(dets), []
    for g in groups:
        cap = max(len(dets[i]) for i in g) + 3
        buf = torch.full((len(g), cap, 6), 777.0, device=device)       # rows past n keep the fill: nothing is written beyond n
        for k, i in enumerate(g):
            buf[k, :len(dets[i])] = torch.from_numpy(dets[i]).to(device)
            out[i] = buf[k, :len(dets[i])]
        bufs.append(buf)
    return out, bufs


def expected(dets, targets, iouv, keep_labels=None):
    """Per image: (clipped detections, correct) from clip_coords + test._match on CPU tensors; None where there are no detections.
    keep_labels: only the first so many labels of every image (what a matcher that stops after so many labels would see)"""
    import test as test_module
    from utils.utils import clip_coords
    t = torch.from_numpy(targets)
    whwh = torch.tensor([W, H, W, H], dtype=torch.float32)
    res = []
    for si, d in enumerate(dets):
        if d is None:
            res.append(None)
            continue
        pred = torch.from_numpy(d.copy())
        clip_coords(pred, (H, W))
        res.append((pred, test_module._match(pred, t[t[:, 0] == si, 1:][:keep_labels], whwh, iouv)))
    return res


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def check_against_host_loop(stats, out, bufs, dets, targets, iouv):
    """What both tiers assert: the stats entries, the written-back boxes and everything past them, bit for bit"""
    want = expected(dets, targets, iouv)
    t = torch.from_numpy(targets)
    k = 0
    for si, d in enumerate(dets):
        tcls = t[t[:, 0] == si, 1].tolist()
        if d is None:
            if tcls:
                correct, conf, cls, got_tcls = stats[k]
                k += 1
                assert tuple(correct.shape) == (0, iouv.numel()) and correct.dtype == torch.bool and got_tcls == tcls
                assert conf.numel() == 0 and cls.numel() == 0
            continue
        correct, conf, cls, got_tcls = stats[k]
        k += 1
        pred, flags = want[si]
        assert correct.dtype == torch.bool and not correct.is_cuda and tuple(correct.shape) == (len(d), iouv.numel())
        assert torch.equal(correct, flags), 'image %d: %s' % (si, (correct != flags).nonzero().tolist()[:8])
        assert np.array_equal(_bits(out[si]), _bits(pred)), 'image %d: clipped boxes' % si
        assert np.array_equal(_bits(conf), _bits(pred[:, 4])) and np.array_equal(_bits(cls), _bits(pred[:, 5]))
        assert got_tcls == tcls
    assert k == len(stats)
    for buf in bufs:       # nothing is written past an image's n rows
        used = {o.data_ptr(): len(o) for o in out if o is not None}
        for i in range(buf.shape[0]):
            n = used.get(buf[i].data_ptr(), 0)
            assert (buf[i, n:] == 777.0).all()
    return want


# ---- yh_eval_match argument checks (host code)
def valid_desc(**kw):
    """A descriptor that passes every check (fake aligned addresses: the checks read no memory), then the overrides"""
    d = hiplib.EvalMatchDesc(rows=4096, targets=4096, label_index=4096, iouv=4096, correct=4096, conf_cls=4096, ws=4096, ws_bytes=8 * 10 + 4 * 3,
                             images=2, nt=3, total=10, niou=10, width=64.0, height=48.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REFUSED = [(dict(niou=0), -1), (dict(niou=11), -1), (dict(images=-1), -1), (dict(nt=-1), -1), (dict(total=-1), -1),
           (dict(rows=None), -1), (dict(targets=None), -1), (dict(label_index=None), -1), (dict(iouv=None), -1), (dict(correct=None), -1),
           (dict(conf_cls=None), -1), (dict(ws=None), -1), (dict(ws_bytes=8 * 10 + 4 * 3 - 1), -1), (dict(width=0.0), -1),
           (dict(height=float('nan')), -1), (dict(rows=4100), -2), (dict(targets=4098), -2), (dict(label_index=4097), -2),
           (dict(iouv=4098), -2), (dict(conf_cls=4098), -2), (dict(ws=4099), -2)]
