#!/usr/bin/env python3
"""What the training-plan builder hands the plan API, and what it leaves in the plan dict, as recorded digests (host emulation: no
GPU, no library).

    python tests/golden/make_golden_train_plan.py

Writes tests/golden/train_plan_ops.json: per case of train_harness.PLAN_CASES the number of forward and backward ops,
train_harness.plan_fingerprint's ``sha256`` over the op sequence and its ``layout_sha256`` over the host-side plan contents the run
path reads (arena size, workspace, parameter slices, zero list, piece offsets, backward ranges, attention buffers).  The cases:
yolov3, yolov4 and yolov3-mobilenet at 64 x 64, batch 2, fp16 and fp32, the tiny cfgs, a slim-pruned cfg that trains through the
channel-padded twin, the test harness's mini cfg, three attention plans, another shape, and yolov3 fp16 under each builder knob.
tests/test_train_emulated.py::test_train_plan_ops_are_pinned holds the builder to it.

The committed file was recorded with engine/train.py of commit 47582ea ("Training backward on one stream: drop side lane and async
reduce"), the last one whose builder was the single method TrainEngine._build_train_plan_: it pins that engine/train_plan.py emits the
same ops, descriptors, fixups, arena offsets and plan contents.  With that commit's engine/train.py in place of today's, this script
rewrites the file byte for byte.  (The ``sha256`` of the first seven rows goes back further: to the last builder that still had the
side lane and the second workspace.)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import train_harness as th  # noqa: E402


def main():
    rows = []
    for case in th.PLAN_CASES:
        row = th.plan_case_fingerprint(case)
        print(row)
        del row['arena_need']       # reported; pinned through layout_sha256
        rows.append(row)
    out = os.path.join(HERE, 'train_plan_ops.json')
    with open(out, 'w') as fh:
        fh.write('[\n' + ',\n'.join(json.dumps(r) for r in rows) + '\n]\n')
    print('%d cases -> %s' % (len(rows), out))


if __name__ == '__main__':
    main()
