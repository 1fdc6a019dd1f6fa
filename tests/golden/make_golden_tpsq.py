#!/usr/bin/env python3
"""Golden fixtures of the TPSQ module family (``quantized == 2``), produced by the REFERENCE's own
``utils/quantized/quantized_TPSQ.py``.  Runs in the build container only.

    python tests/golden/make_golden_tpsq.py

* ``tpsq_elementwise.npz``   the activation and weight quantisers (8 / 4 bits; a warm-up call, calls right after the scale was moved off
                             its power by x 1.3 and x 0.7, an eval call, a first call in eval, an input whose maximum is 0) and the
                             bias quantiser over the call sequences of tests/tpsq_cases.py: inputs, outputs, input and scale gradients,
                             the values ``Search_Pow2`` saw and every buffer and parameter after each call.
* ``tpsq_conv_<case>.npz``   ``TPSQ_BNFold_QuantizedConv2d_For_FPGA`` in three shapes: initial state, the inputs of ten training calls
                             and one eval call, outputs, gradients and the state after each call.
* ``tpsq_net.npz``           the micro net of tests/qat_minicfg.py: initial state, four uint8 frame batches, the parameter gradients of
                             iteration 0 and the decision buffers after 20 training iterations without weight updates.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: F401
import refharness
import qat_cases as qc
import tpsq_cases as tc
from qat_minicfg import PARAMETERS, SIZE, STEPS, micro_cfg


def save(name, out):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    print('%-24s %4d arrays %7.1f KB' % (name, len(out), size / 1024))


def elementwise(Q):
    out = {}
    for name in tc.ELEMENTWISE:
        calls = tc.elementwise_inputs(name)
        for k, ins in enumerate(calls):
            out['%s.in.%d.0' % (name, k)] = ins[0].numpy()
        out.update(qc.flatten(name, tc.elementwise_records(Q, name, calls)))
    save('tpsq_elementwise.npz', out)


def convs(Q):
    for n, (name, kwargs, shape) in enumerate(tc.CONV_CASES):
        mod = tc.make_conv(Q, kwargs)
        out = {'init.' + k: v.detach().clone().numpy() for k, v in mod.state_dict().items()}
        calls = qc.conv_inputs(500 + n, shape)
        for k, ins in enumerate(calls):
            out['in.%d.0' % k] = ins[0].numpy()
        out.update(qc.flatten('call', tc.run_conv(mod, calls)))
        save('tpsq_conv_%s.npz' % name, out)


def net(ref):
    torch.manual_seed(0)
    model = ref.models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=2, a_bit=8, w_bit=8, steps=STEPS)
    assert sum(p.numel() for p in model.parameters()) == PARAMETERS + tc.NET_SCALES
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert len(init) == tc.NET_STATE_KEYS, len(init)
    frames = qc.net_frames()
    grads, state = qc.run_net(model, frames)
    out = {'frames': frames}
    out.update({'init.' + k: v.numpy() for k, v in init.items()})
    out.update({'grad0.' + k: v.numpy() for k, v in grads.items()})
    out.update({'final.' + k: v.numpy() for k, v in state.items() if tc.is_decision(k)})
    save('tpsq_net.npz', out)


def main():
    ref = refharness.load()
    import importlib
    Q = ref._modules.get('utils.quantized.quantized_TPSQ') or importlib.import_module('utils.quantized.quantized_TPSQ')
    assert os.path.abspath(Q.__file__).startswith(os.path.abspath(ref.root)), Q.__file__
    only = sys.argv[1:]
    if not only or 'elementwise' in only:
        elementwise(Q)
    if not only or 'conv' in only:
        convs(Q)
    if not only or 'net' in only:
        net(ref)


if __name__ == '__main__':
    main()
