#!/usr/bin/env python3
"""Recorded results of the reference's cfg parser, for tests that must run without a reference checkout.

    YOLO_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_refparse.py

Writes tests/golden/ref_parse.json:
* ``cfg_blocks[rel]``: the reference's ``utils.parse_config.parse_model_cfg`` of its own cfg/<rel> for every cfg this package
  generates (tests/test_cfggen.py); numpy arrays are stored as {"ndarray": nested list}.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: F401,E402
import refharness  # noqa: E402
from test_cfggen import PAIRS  # noqa: E402


def plain(v):
    if isinstance(v, np.ndarray):
        return {'ndarray': v.tolist()}
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    return v


def main():
    ref = refharness.load()
    blocks = {rel: [{k: plain(v) for k, v in b.items()} for b in ref.parse_config.parse_model_cfg(os.path.join(refharness.REF, 'cfg', rel))]
              for rel in PAIRS}
    path = os.path.join(HERE, 'ref_parse.json')
    json.dump({'cfg_blocks': blocks}, open(path, 'w'), indent=0, sort_keys=True)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
