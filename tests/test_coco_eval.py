"""CPU tier of COCO scoring without pycocotools (``test.py --coco-metrics``): the host statement utils/cocoeval.py against values derived
by hand, then ``engine.cocoeval`` driven through a host emulation of the three entry points (tests/fakelib_coco.py, written in the
kernels' formulation) against the host statement bit for bit, the C ABI, and ``test.test(..., coco_metrics=...)`` end to end.  The
kernels themselves: tests/test_gpu_coco_eval.py.

The protocol is a restatement (README): the expected values below follow from the issue's text, none was recorded from pycocotools.

One constant appears in every derivation: pr = tp / (fp + tp + 2^-52).  With tp = 1, fp = 0 that is P1 = 1 / (1 + 2^-52), the double
just below 1 (1 + 2^-52 is representable), not 1.0; with fp + tp = 2 or 3 the sum rounds back to 2 or 3 (2^-52 is half an ulp there,
ties go to the even mantissa), so 1/2 and 2/3 come out as the plain quotients.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest

sys.path.insert(0, os.path.join(conftest.REPO, 'tests'))
import coco_cases as cases  # noqa: E402
import fakelib_coco  # noqa: E402
from engine import cocoeval as engine, hiplib  # noqa: E402
from utils import cocoeval as host  # noqa: E402

P1 = 1.0 / (1.0 + 2.0 ** -52)
ALL, SMALL, MEDIUM, LARGE = range(4)
M1, M10, M100 = range(3)


def det(image, cat, box, score):
    return (image, cat, *box, score)


def gt(image, cat, box, area=None, crowd=0):
    return (image, cat, *box, box[2] * box[3] if area is None else area, crowd)


def ev(dets, gts, images=1, K=1):
    return host.evaluate(np.asarray(dets, np.float64).reshape(-1, 7), np.asarray(gts, np.float64).reshape(-1, 8), images, K)


def pair(dets, gts, rng):
    """match_pair on rows of det() / gt(): detections in the given (score) order"""
    d = np.asarray(dets, np.float64).reshape(-1, 7)[:, 2:7]
    g = np.asarray(gts, np.float64).reshape(-1, 8)[:, 2:8]
    return host.match_pair(d, g, *host.AREA_RNG[rng])


@pytest.fixture
def fake():
    lib = fakelib_coco.FakeLibCoco()
    engine._LIB_OVERRIDE = lib
    yield lib
    engine._LIB_OVERRIDE = None


# ------------------------------------------------------------------------------------------------ the host statement, by hand
def test_parameters():
    assert host.IOU_THRS[0] == 0.5 and host.IOU_THRS[5] == 0.75 and len(host.IOU_THRS) == 10 and abs(host.IOU_THRS[9] - 0.95) < 1e-15
    assert host.REC_THRS[0] == 0 and host.REC_THRS[50] == 0.5 and host.REC_THRS[100] == 1 and len(host.REC_THRS) == 101
    assert host.MAX_DETS == (1, 10, 100) and host.EPS == 2.0 ** -52
    assert host.AREA_RNG == ((0, 1e10), (0, 1024), (1024, 9216), (9216, 1e10))
    assert 2.0 + host.EPS == 2.0 and 3.0 + host.EPS == 3.0 and 1.0 + host.EPS > 1.0 and P1 < 1.0


def test_one_identical_detection_scores_one():
    """IoU 1 passes every threshold: tp = [1], fp = [0], rc = [1], pr = [P1], so all 101 recall points read P1 and every AR is 1.  The box
    is 50 x 40 = 2000: medium.  In small and large its ground truth is ignored, npig = 0, the entries stay -1."""
    box = (10, 10, 50, 40)
    r = ev([det(0, 0, box, 0.9)], [gt(0, 0, box)])
    assert r['precision'].shape == (10, 101, 1, 4, 3) and r['recall'].shape == (10, 1, 4, 3)
    for a in (ALL, MEDIUM):
        assert np.all(r['precision'][:, :, 0, a, :] == P1) and np.all(r['recall'][:, 0, a, :] == 1.0)
    for a in (SMALL, LARGE):
        assert np.all(r['precision'][:, :, 0, a, :] == -1) and np.all(r['recall'][:, 0, a, :] == -1)
    want = [P1, P1, P1, -1, P1, -1, 1, 1, 1, -1, 1, -1]
    assert np.allclose(r['stats'], want, rtol=0, atol=1e-13)
    assert r['stats'][6] == r['stats'][7] == r['stats'][8] == r['stats'][10] == 1.0 and r['stats'][3] == -1.0
    lines = host.format_stats(r['stats'])
    assert len(lines) == 12
    assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000'
    assert lines[1] == ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 1.000'
    assert lines[3] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000'
    assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000'
    assert lines[11] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 1.000'.replace('1.000', '-1.000')


def test_false_positive_above_the_true_positive_halves_precision():
    """Score order FP, TP: tp = [0, 1], fp = [1, 1], pr = [0, 1/2], envelope [1/2, 1/2]; rc = [0, 1]: r = 0 reads index 0, every other
    r index 1 - 1/2 at all 101 points, at every threshold (the TP's IoU is 1)."""
    box = (0, 0, 20, 20)
    r = ev([det(0, 0, (100, 100, 20, 20), 0.9), det(0, 0, box, 0.8)], [gt(0, 0, box)])
    assert np.all(r['precision'][:, :, 0, ALL, M100] == 0.5)
    assert r['stats'][1] == 0.5 and r['stats'][0] == 0.5 and r['stats'][8] == 1.0
    assert np.all(r['precision'][:, :, 0, ALL, M1] == 0.0) and np.all(r['recall'][:, 0, ALL, M1] == 0.0)     # maxDets 1 keeps the FP only


def test_tp_fp_tp_gives_the_envelope_one_two_thirds_two_thirds():
    """tp = [1, 1, 2], fp = [0, 1, 1]: pr = [P1, 1/2, 2/3], envelope [P1, 2/3, 2/3]; rc = [1/2, 1/2, 1].  r <= 1/2 (the 51 points 0 ..
    0.5) read index 0, the other 50 read index 2: AP50 = (51 P1 + 50 (2/3)) / 101."""
    g1, g2 = (0, 0, 20, 20), (100, 0, 20, 20)
    r = ev([det(0, 0, g1, 0.9), det(0, 0, (300, 300, 20, 20), 0.8), det(0, 0, g2, 0.7)], [gt(0, 0, g1), gt(0, 0, g2)])
    p = r['precision'][0, :, 0, ALL, M100]
    assert np.all(p[:51] == P1) and np.all(p[51:] == 2.0 / 3.0)
    assert abs(r['stats'][1] - (51 * P1 + 50 * (2.0 / 3.0)) / 101) < 1e-13 and r['stats'][8] == 1.0


def test_iou_exactly_at_a_threshold_matches_there_and_not_above():
    """[0, 0, 10, 10] in [0, 0, 10, 20]: i = 100, u = 100 + 200 - 100 = 200, IoU = 0.5 exactly; 0.5 >= min(0.5, 1 - 1e-10) matches,
    0.5 < 0.55 does not."""
    r = ev([det(0, 0, (0, 0, 10, 10), 0.9)], [gt(0, 0, (0, 0, 10, 20))])
    assert r['recall'][0, 0, ALL, M100] == 1.0 and np.all(r['recall'][1:, 0, ALL, M100] == 0.0)
    assert np.all(r['precision'][0, :, 0, ALL, M100] == P1) and np.all(r['precision'][1:, :, 0, ALL, M100] == 0.0)
    assert float(host.box_iou(np.array([[0., 0, 10, 10]]), np.array([[0., 0, 10, 20]]), np.array([False]))[0, 0]) == 0.5
    # against a crowd the union is the detection's own area: IoU 1
    assert float(host.box_iou(np.array([[0., 0, 10, 10]]), np.array([[0., 0, 10, 20]]), np.array([True]))[0, 0]) == 1.0


def test_detections_on_a_crowd_are_ignored_and_a_crowd_only_category_stays_empty():
    """Two detections inside one crowd box: IoU = i / own area = 1 for both, both match it (a crowd can be matched again) and both are
    ignored - neither tp nor fp.  The third detection is the TP of the one plain ground truth: tp = [1], pr = P1 everywhere; had the
    two counted as FPs it would be 1/3.  Category 1 has a crowd ground truth only: npig = 0, -1."""
    crowd, plain = (0, 0, 100, 100), (200, 200, 20, 20)
    d = [det(0, 0, (10, 10, 20, 20), 0.95), det(0, 0, (40, 40, 20, 20), 0.9), det(0, 0, plain, 0.5), det(0, 1, (10, 10, 20, 20), 0.9)]
    g = [gt(0, 0, crowd, crowd=1), gt(0, 0, plain), gt(0, 1, crowd, crowd=1)]
    dtm, dtig, gig = pair(d[:3], g[:2], ALL)
    assert dtm.all() and dtig[:, :2].all() and not dtig[:, 2].any() and gig.tolist() == [True, False]
    r = ev(d, g, K=2)
    assert np.all(r['precision'][:, :, 0, ALL, M100] == P1) and np.all(r['recall'][:, 0, ALL, M100] == 1.0)
    assert np.all(r['precision'][:, :, 1] == -1) and np.all(r['recall'][:, 1] == -1)
    assert abs(r['stats'][0] - P1) < 1e-13              # the mean runs over category 0 alone


def test_a_ground_truth_that_counts_wins_over_an_ignored_one_with_the_larger_iou():
    """Range small.  A = 30 x 28 (area 840, counts), B = the detection's own box annotated with area 20000 (ignored in small).  IoU with A
    is 840 / 900 = 0.933, with B 1.  Up to t = 0.9 the detection takes A although B overlaps more: not ignored.  At t = 0.95 A is out
    of reach, only then B is taken: matched and ignored."""
    d = [det(0, 0, (0, 0, 30, 30), 0.9)]
    g = [gt(0, 0, (0, 0, 30, 28)), gt(0, 0, (0, 0, 30, 30), area=20000)]
    for order in (g, g[::-1]):
        dtm, dtig, gig = pair(d, order, SMALL)
        assert dtm[:, 0].all() and dtig[:, 0].tolist() == [False] * 9 + [True]


def test_equal_ious_take_the_later_ground_truth():
    """d1 = [2, 0, 20, 20] overlaps g0 = [0, ...] and g1 = [4, ...] by 18 x 20 each: IoU 360 / 440 = 0.818 with both, the later (g1) is
    taken.  d2 is g0's own box: at t = 0.7 .. 0.8 it finds g0 free (IoU 1).  Had d1 taken g0, d2 would be left with g1 at IoU
    320 / 480 = 0.667 < 0.7 and stay unmatched there."""
    d = [det(0, 0, (2, 0, 20, 20), 0.9), det(0, 0, (0, 0, 20, 20), 0.8)]
    g = [gt(0, 0, (0, 0, 20, 20)), gt(0, 0, (4, 0, 20, 20))]
    iou = host.box_iou(np.array([[2., 0, 20, 20]]), np.array([[0., 0, 20, 20], [4., 0, 20, 20]]), np.array([False, False]))
    assert iou[0, 0] == iou[0, 1] == 360.0 / 440.0
    dtm, dtig, _ = pair(d, g, ALL)
    assert dtm[:, 0].tolist() == [True] * 7 + [False] * 3          # 0.818 reaches 0.5 .. 0.8
    assert dtm[:, 1].all() and not dtig.any()                      # d2 matched at EVERY threshold


def test_area_borders_belong_to_both_ranges():
    """32 x 32 = 1024 is small and medium, 96 x 96 = 9216 medium and large (both bounds belong to a range)."""
    a, b = (0, 0, 32, 32), (200, 200, 96, 96)
    g = [gt(0, 0, a), gt(0, 0, b)]
    d = [det(0, 0, a, 0.9), det(0, 0, b, 0.8)]
    assert [pair(d, g, rng)[2].tolist() for rng in (ALL, SMALL, MEDIUM, LARGE)] == [[False, False], [False, True], [False, False], [True, False]]
    r = ev(d, g)
    assert np.all(r['recall'][:, 0, :, M100] == 1.0)                                   # every range has ground truth, all of it found
    # medium counts both: tp = [1, 2], pr = [P1, 2 / (2 + 2^-52) = 1.0], and the envelope carries the 1.0 to the front
    assert np.all(r['precision'][:, :, 0, MEDIUM, M100] == 1.0)
    # the detections sit on the borders too: neither is an unmatched-outside case anywhere, the other range's box is matched-and-ignored
    assert np.all(r['precision'][:, :, 0, SMALL, M100] == P1) and np.all(r['precision'][:, :, 0, LARGE, M100] == P1)


def test_unmatched_outside_the_range_is_ignored_and_a_matched_one_inherits_its_ground_truth():
    """A 200 x 200 false positive above the TP of a 20 x 20 ground truth: in 'all' it is a FP (tp = [0, 1], fp = [1, 1]: 1/2
    everywhere); in small its own area lies outside and it is ignored: P1.  In large the ground truth is ignored: -1.  A matched
    detection takes its ground truth's flag whatever its own area: a 40 x 40 detection (1600, medium) on a ground truth annotated
    with area 900 counts in small."""
    box = (0, 0, 20, 20)
    r = ev([det(0, 0, (100, 100, 200, 200), 0.9), det(0, 0, box, 0.8)], [gt(0, 0, box)])
    assert np.all(r['precision'][:, :, 0, ALL, M100] == 0.5) and np.all(r['precision'][:, :, 0, SMALL, M100] == P1)
    assert np.all(r['precision'][:, :, 0, LARGE] == -1) and np.all(r['precision'][:, :, 0, MEDIUM] == -1)
    dtm, dtig, gig = pair([det(0, 0, (0, 0, 40, 40), 0.9)], [gt(0, 0, (0, 0, 40, 40), area=900)], SMALL)
    assert dtm.all() and not dtig.any() and not gig.any()
    dtm, dtig, gig = pair([det(0, 0, (0, 0, 40, 40), 0.9)], [gt(0, 0, (0, 0, 40, 40), area=900)], MEDIUM)
    assert dtm.all() and dtig.all() and gig.all()                                       # matched to an ignored ground truth: ignored


def test_the_101st_detection_of_a_pair_never_counts():
    """100 false positives scored above the one true positive: it is the 101st and is dropped, recall 0, precision 0.  With 99 above it is
    the 100th: recall 1, pr = 1 / 100 at the end, the envelope carries 0.01 to every recall point."""
    box = (0, 0, 20, 20)
    fps = [det(0, 0, (100 + i, 100, 20, 20), 0.99 - 0.001 * i) for i in range(100)]
    r = ev(fps + [det(0, 0, box, 0.1)], [gt(0, 0, box)])
    assert np.all(r['recall'][:, 0, ALL, :] == 0.0) and np.all(r['precision'][:, :, 0, ALL, :] == 0.0)
    r = ev(fps[:99] + [det(0, 0, box, 0.1)], [gt(0, 0, box)])
    assert np.all(r['recall'][:, 0, ALL, M100] == 1.0) and np.all(r['precision'][:, :, 0, ALL, M100] == 1.0 / (100.0 + host.EPS))
    assert 100.0 + host.EPS == 100.0


def test_ar1_against_ar10_with_two_ground_truths():
    """Two ground truths, both found: maxDets 1 keeps one detection, recall 1/2; maxDets 10 keeps both, recall 1."""
    g1, g2 = (0, 0, 20, 20), (100, 0, 20, 20)
    r = ev([det(0, 0, g1, 0.9), det(0, 0, g2, 0.8)], [gt(0, 0, g1), gt(0, 0, g2)])
    assert r['stats'][6] == 0.5 and r['stats'][7] == 1.0 and r['stats'][8] == 1.0
    p = r['precision'][0, :, 0, ALL, M1]
    assert np.all(p[:51] == P1) and np.all(p[51:] == 0.0)


def test_equal_scores_across_images_keep_the_image_order():
    """One FP and one TP with the same score in two images.  The category's list is ordered by score, stable over the image order - not
    over the input order: FP in image 0 first gives tp = [0, 1], fp = [1, 1]: 1/2; TP in image 0 first gives P1 at every point."""
    box = (0, 0, 20, 20)
    tp_fp = lambda tp_img: [det(1 - tp_img, 0, (100, 100, 20, 20), 0.5), det(tp_img, 0, box, 0.5)]
    for rows in (tp_fp(1), tp_fp(1)[::-1]):
        r = ev(rows, [gt(1, 0, box)], images=2)
        assert np.all(r['precision'][:, :, 0, ALL, M100] == 0.5)
    for rows in (tp_fp(0), tp_fp(0)[::-1]):
        r = ev(rows, [gt(0, 0, box)], images=2)
        assert np.all(r['precision'][:, :, 0, ALL, M100] == P1)


def test_a_category_without_ground_truth_stays_out_of_the_means():
    box = (10, 10, 50, 40)
    r = ev([det(0, 0, box, 0.9), det(0, 1, box, 0.9), det(0, 1, (0, 0, 5, 5), 0.8)], [gt(0, 0, box)], K=3)
    assert np.all(r['precision'][:, :, 1:] == -1) and np.all(r['recall'][:, 1:] == -1)
    assert abs(r['stats'][0] - P1) < 1e-13 and r['stats'][8] == 1.0
    empty = ev([], [], images=3, K=2)
    assert np.all(empty['precision'] == -1) and np.all(empty['stats'] == -1)
    with pytest.raises(ValueError):
        ev([det(0, 3, box, 0.9)], [], K=3)


# ------------------------------------------------------------------------------------------------ the emulated ABI
@pytest.mark.parametrize('name', ['generated', 'directed1', 'directed80'])
def test_driver_on_the_emulated_kernels_is_the_host_statement_bit_for_bit(fake, name):
    dets, gts, n, K, want = cases.reference(name)
    got = engine.evaluate_device(dets, gts, n, K, 'cpu')
    cases.same_bits(got, want)
    assert [c[0] for c in fake.coco_calls] == ['match', 'accumulate']                  # two launches, whatever the size
    assert engine.LAST['hip_launches'] == 2 and engine.LAST['bytes_to_host'] == 8 * (10 * 101 * K * 12 + 10 * K * 12)
    assert engine.LAST['bytes_to_device'] == 8 * (dets.size + gts.size + 10 + 101 + 8)
    if name == 'generated':
        # the set is what the issue asks for: ties, crowds, borders, > 100 detections, > 64 ground truths, and a result that is not trivial
        assert n == 40 and K == 5 and len(np.unique(dets[:, 6])) <= 100 and np.all(dets[:, 2:6] * 2 == np.round(dets[:, 2:6] * 2))
        assert 0.05 < gts[:, 7].mean() < 0.15 and {1024.0, 9216.0} <= set(gts[:, 6].tolist())
        key = lambda rows: np.unique(rows[:, 0] * K + rows[:, 1], return_counts=True)[1]
        assert key(dets).max() > 100 and set(key(gts).tolist()) >= {63, 64, 65, 130}
        assert np.all(want['stats'] > 0.02) and np.all(want['stats'] < 0.9) and (want['precision'] > -1).all()
        assert engine.LAST['slots'] < len(dets)                                        # detections past the 100th got no slot
    if name == 'directed80':
        lens = np.bincount(dets[:, 1].astype(int), minlength=80)
        assert {1, 255, 256, 257, 700, 5000} <= set(lens.tolist())
        p = want['precision']
        assert np.all(p[:, :, 66, LARGE] == -1) and np.all(p[:, :, 66, [ALL, SMALL, MEDIUM]] > -1)   # ignored in ONE range only
        assert np.all(p[:, :, 70] == -1) and np.all(p[:, :, 71] == -1) and np.all(p[:, :, 1] == -1)


def test_driver_handles_empty_sides(fake):
    box = (10, 10, 50, 40)
    for d, g in (([], []), ([det(0, 0, box, 0.9)], []), ([], [gt(1, 1, box)])):
        d, g = np.asarray(d, np.float64).reshape(-1, 7), np.asarray(g, np.float64).reshape(-1, 8)
        cases.same_bits(engine.evaluate_device(d, g, 2, 2, 'cpu'), host.evaluate(d, g, 2, 2))


def test_switch_and_cpu_keep_the_host_statement(monkeypatch):
    monkeypatch.delenv('YOLO_HIP_COCO_EVAL', raising=False)
    assert not engine.enabled('cpu') and not engine.enabled(None) and engine.enabled(torch.device('cuda', 0))
    monkeypatch.setenv('YOLO_HIP_COCO_EVAL', '0')
    assert not engine.enabled(torch.device('cuda', 0))
    dets, gts, n, K, want = cases.reference('directed1')
    monkeypatch.setattr(engine, 'evaluate_device', lambda *a: pytest.fail('the device path ran'))
    cases.same_bits(engine.evaluate(dets, gts, n, K, device='cpu'), want)
    cases.same_bits(engine.evaluate(dets, gts, n, K, device='cuda:0'), want)           # switched off: no GPU is touched


def test_ground_truth_from_a_coco_json(fake, tmp_path):
    """The generated set written as an annotation file and a results list, with ids that are not indices (images 1000 + 7 i, categories
    1, 3, 5, 8, 13), images nobody evaluated and a category nobody lists: loaded back it is the same set."""
    dets, gts, n, K, want = cases.reference('generated')
    img_id = lambda i: 1000 + 7 * int(i)
    cat_ids = [1, 3, 5, 8, 13]
    files = ['/data/val/COCO_val2014_%012d.jpg' % img_id(i) for i in range(n)]
    assert [host.image_id_of(f) for f in files] == [img_id(i) for i in range(n)] and host.image_id_of('a/b/street.png') == 'street'
    anns = [dict(id=j, image_id=img_id(r[0]), category_id=cat_ids[int(r[1])], bbox=r[2:6].tolist(), area=float(r[6]), iscrowd=int(r[7]))
            for j, r in enumerate(gts)]
    anns += [dict(id=10 ** 6, image_id=5, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)]       # an image not evaluated
    js = dict(images=[dict(id=img_id(i)) for i in range(n)][::-1] + [dict(id=5)], annotations=anns, categories=[dict(id=c) for c in cat_ids[::-1]])
    path = tmp_path / 'instances.json'
    path.write_text(json.dumps(js))
    jdict = [dict(image_id=img_id(r[0]), category_id=cat_ids[int(r[1])], bbox=r[2:6].tolist(), score=float(r[6])) for r in dets]
    jdict.append(dict(image_id=img_id(0), category_id=99, bbox=[0, 0, 5, 5], score=0.5))                     # a category without ground truth
    g2, image_ids, cats = host.load_coco_json(str(path), [host.image_id_of(f) for f in files])
    d2 = host.dets_from_jdict(jdict, image_ids, cats)
    assert image_ids == [img_id(i) for i in range(n)] and cats == cat_ids and len(g2) == len(gts) and len(d2) == len(dets)
    cases.same_bits(host.evaluate(d2, g2, len(image_ids), len(cats)), want)
    cases.same_bits(engine.evaluate_device(d2, g2, len(image_ids), len(cats), 'cpu'), want)
    with pytest.raises(ValueError):
        host.load_coco_json(str(path), [1000, 4])
    with pytest.raises(ValueError):
        host.dets_from_jdict([dict(image_id=4, category_id=1, bbox=[0, 0, 1, 1], score=1.0)], image_ids, cats)


def test_ground_truth_from_label_files(fake):
    """Normalised centre boxes (float32, cast to float64) times the original size: x = cx w0 - w / 2, area = w h, no crowd."""
    lab = [np.array([[1, 0.5, 0.25, 0.25, 0.5]], np.float32), np.zeros((0, 5), np.float32), np.array([[0, 0.3, 0.3, 0.1, 0.2], [2, 0.5, 0.5, 1, 1]], np.float32)]
    shapes = [(100, 200), (50, 60), (480, 640)]
    g = host.gts_from_labels(lab, shapes)
    assert g.shape == (3, 8) and g[0].tolist() == [0, 1, 75.0, 0.0, 50.0, 50.0, 2500.0, 0]
    f = lambda v: float(np.float32(v))
    assert g[1].tolist() == [2, 0, f(0.3) * 640 - f(0.1) * 640 / 2, f(0.3) * 480 - f(0.2) * 480 / 2, f(0.1) * 640, f(0.2) * 480,
                             (f(0.1) * 640) * (f(0.2) * 480), 0]
    assert g[2].tolist() == [2, 2, 0.0, 0.0, 640.0, 480.0, 640.0 * 480.0, 0]
    d = np.array([det(0, 1, (75, 0, 50, 50), 0.9), det(2, 2, (0, 0, 640, 470), 0.8), det(2, 0, (0, 0, 5, 5), 0.7)], np.float64)
    cases.same_bits(engine.evaluate_device(d, g, 3, 3, 'cpu'), host.evaluate(d, g, 3, 3))
    assert host.evaluate(d, g, 3, 3)['stats'][1] > 0.6


# ------------------------------------------------------------------------------------------------ the C ABI
NAMES = ('yh_coco_workspace', 'yh_coco_match', 'yh_coco_accumulate')


def test_library_exports_and_header_declares_the_entries(tmp_path):
    lib = hiplib.load()
    header = open(os.path.join(conftest.REPO, 'include', 'yolo_hip.h')).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in hiplib.EXPORTS and re.search(r'\b%s\s*\(' % n, header), n
    assert int(re.search(r'#define\s+YH_ABI_VERSION\s+(\d+)', header).group(1)) == 2 == lib.yh_abi_version() == hiplib.ABI_VERSION
    structs = {'yh_coco_match_desc': hiplib.CocoMatchDesc, 'yh_coco_accum_desc': hiplib.CocoAccumDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolo_hip.h"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(conftest.REPO, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, '%s.%s' % (cname, fname)


def test_argument_validation_returns_before_any_launch():
    """Host code: runs without a GPU.  Bad arguments are refused, empty work is YH_OK - neither reaches a launch."""
    real, emu = hiplib.load(), fakelib_coco.FakeLibCoco()
    for lib in (real, emu):
        assert lib.yh_coco_workspace(1000, 50) == 400 and lib.yh_coco_workspace(0, 0) == 0 and lib.yh_coco_workspace(-1, 0) < 0
        assert lib.yh_coco_match(None, None) == -1 and lib.yh_coco_accumulate(None, None) == -1
        for kw, rc in cases.MATCH_REFUSED:
            assert lib.yh_coco_match(C.byref(cases.valid_match_desc(**kw)), None) == rc, kw
        for kw, rc in cases.ACCUM_REFUSED:
            assert lib.yh_coco_accumulate(C.byref(cases.valid_accum_desc(**kw)), None) == rc, kw
        assert lib.yh_coco_match(C.byref(cases.valid_match_desc(n_pairs=0)), None) == 0
    assert emu.coco_calls == []


# ------------------------------------------------------------------------------------------------ test.py
def _run_test_py(dataset_dir, tiny_cfg, model, **kw):
    import test as test_mod
    test_mod.opt = None
    return test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), batch_size=2, imgsz=64, model=model, plot=False, **kw)


def test_test_py_coco_metrics(fake, dataset_dir, tiny_cfg, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    import models
    import test as test_mod
    torch.manual_seed(3)
    model = models.Darknet(tiny_cfg, (64, 64))
    plain = _run_test_py(dataset_dir, tiny_cfg, model, save_json=True)
    json_plain = open('results.json').read()
    os.remove('results.json')
    capsys.readouterr()
    test_mod.coco_result = None
    with_flag = _run_test_py(dataset_dir, tiny_cfg, model, coco_metrics=True)
    out = capsys.readouterr().out
    assert not os.path.exists('results.json')                                           # the flag alone writes no file
    assert with_flag[0] == plain[0] and np.array_equal(with_flag[1], plain[1])          # the return value does not change
    res = test_mod.coco_result
    assert res is test_mod.test.coco_result and set(res) == {'precision', 'recall', 'stats'}
    assert res['precision'].shape == (10, 101, 2, 4, 3) and res['recall'].shape == (10, 2, 4, 3) and res['stats'].shape == (12,)
    assert out.count('Average Precision  (AP) @[') == 6 and out.count('Average Recall     (AR) @[') == 6
    assert fake.coco_calls == []                                                        # a CPU model: the host statement
    # label-file ground truth, recomputed here from the results file and the label files
    both = _run_test_py(dataset_dir, tiny_cfg, model, save_json=True, coco_metrics=True)
    assert both[0] == plain[0] and json_plain == open('results.json').read()            # the same results.json as --save-json alone
    cases.same_bits(test_mod.coco_result, res)
    jdict = json.loads(json_plain)
    assert len(jdict) > 20
    from utils.datasets import LoadImagesAndLabels
    ds = LoadImagesAndLabels(str(dataset_dir / 'valid.txt'), 64, 2, rect=True)
    from PIL import Image
    shapes = [Image.open(f).size[::-1] for f in ds.img_files]
    gts = host.gts_from_labels(ds.labels, shapes)
    index = {host.image_id_of(f): i for i, f in enumerate(ds.img_files)}
    dets = np.array([(index[r['image_id']], r['category_id'] - 1, *r['bbox'], r['score']) for r in jdict], np.float64)   # coco91: 0 -> 1, 1 -> 2
    cases.same_bits(host.evaluate(dets, gts, len(ds.img_files), 2), res)
    assert (res['recall'][:, :, 0, 2] > -1).all()                                       # both classes have ground truth
    # the driver on the emulated kernels, routed the way enabled() routes on a GPU
    monkeypatch.setattr(engine, 'enabled', lambda device: True)
    monkeypatch.setattr(engine, 'evaluate_device', lambda d, g, n, k, device, real=engine.evaluate_device: real(d, g, n, k, 'cpu'))
    _run_test_py(dataset_dir, tiny_cfg, model, coco_metrics=True)
    assert [c[0] for c in fake.coco_calls] == ['match', 'accumulate']
    cases.same_bits(test_mod.coco_result, res)


def test_test_py_coco_metrics_with_an_annotation_file(dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    """Mode (a): image ids from the file stems (im_08 -> 8), category ids as results.json carries them (coco91: 1, 2)."""
    monkeypatch.chdir(tmp_path)
    import models
    import test as test_mod
    from PIL import Image
    torch.manual_seed(3)
    model = models.Darknet(tiny_cfg, (64, 64))
    files = open(dataset_dir / 'valid.txt').read().split()
    anns, images = [], []
    for f in files + [open(dataset_dir / 'train.txt').read().split()[0]]:               # one image more than is evaluated
        w0, h0 = Image.open(f).size
        iid = host.image_id_of(f)
        images.append(dict(id=iid, width=w0, height=h0))
        for c, cx, cy, bw, bh in np.loadtxt(f.replace('images', 'labels').replace('.png', '.txt'), ndmin=2):
            anns.append(dict(id=len(anns), image_id=iid, category_id=int(c) + 1, iscrowd=0, area=bw * w0 * bh * h0,
                             bbox=[(cx - bw / 2) * w0, (cy - bh / 2) * h0, bw * w0, bh * h0]))
    path = tmp_path / 'ann.json'
    path.write_text(json.dumps(dict(images=images, annotations=anns, categories=[dict(id=1, name='wide'), dict(id=2, name='tall')])))
    _run_test_py(dataset_dir, tiny_cfg, model, save_json=True, coco_metrics=str(path))
    res = test_mod.coco_result
    ids = sorted(host.image_id_of(f) for f in files)
    assert ids == [8, 9, 10, 11]
    gts, image_ids, cats = host.load_coco_json(str(path), ids)
    assert image_ids == ids and cats == [1, 2] and len(gts) == sum(a['image_id'] in ids for a in anns) < len(anns)
    cases.same_bits(host.evaluate(host.dets_from_jdict(json.load(open('results.json')), image_ids, cats), gts, 4, 2), res)
    assert res['stats'][8] >= 0
