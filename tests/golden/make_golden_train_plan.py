#!/usr/bin/env python3
"""What the training-plan builder (engine/train.py) hands the plan API, as recorded digests (host emulation: no GPU, no library).

    python tests/golden/make_golden_train_plan.py

Writes tests/golden/train_plan_ops.json: per case of train_harness.PLAN_CASES (yolov3, yolov4 and yolov3-mobilenet at 64 x 64,
batch 2, fp16 and fp32, plus one attention plan) the number of forward and backward ops and train_harness.plan_fingerprint's sha256
over the op sequence.  tests/test_train_emulated.py::test_train_plan_ops_are_pinned holds the builder to it.

The committed file was recorded at the last commit whose builder still had the side lane and the second workspace (both off by
default), so it pins that the builder without them emits the same ops, descriptors, fixups and arena offsets.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import train_harness as th  # noqa: E402


def main():
    rows = []
    for cfg, precision, attention in th.PLAN_CASES:
        row = th.plan_fingerprint(cfg, precision, attention)
        print(row)
        del row['arena_need']       # reported, not pinned
        rows.append(row)
    out = os.path.join(HERE, 'train_plan_ops.json')
    with open(out, 'w') as fh:
        fh.write('[\n' + ',\n'.join(json.dumps(r) for r in rows) + '\n]\n')
    print('%d cases -> %s' % (len(rows), out))


if __name__ == '__main__':
    main()
