#!/usr/bin/env python3
"""Golden fixtures of the QAT module family (``quantized == 1``), produced by the REFERENCE's own
``utils/quantized/quantized_google.py``.  Runs in the build container only.

    python tests/golden/make_golden_qat.py

* ``qat_elementwise.npz``   the quantisers (symmetric / asymmetric x both trackers x signed / unsigned x 8 / 4 bits), the two
                            shortcuts and the concat over the call sequences of tests/qat_cases.py: inputs, outputs, input
                            gradients and every buffer after each call.
* ``qat_conv_<case>.npz``   ``BNFold_QuantizedConv2d_For_FPGA`` in three shapes: initial state, the inputs of ten training calls and
                            one eval call, outputs, gradients and the state after each call.
* ``qat_net_way<k>.npz``    the micro net of tests/qat_minicfg.py: initial state, four uint8 frames batches, the parameter gradients
                            of iteration 0 and the decision buffers after 20 training iterations without weight updates.
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
from qat_minicfg import PARAMETERS, SIZE, STATE_KEYS, STEPS, micro_cfg


def save(name, out):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    print('%-24s %4d arrays %7.1f KB' % (name, len(out), size / 1024))


def elementwise(Q):
    out = {}
    for name, make, make_calls, n_train, fwd in qc.elementwise_cases(Q):
        calls = make_calls()
        for k, ins in enumerate(calls):
            for j, t in enumerate(ins):
                out['%s.in.%d.%d' % (name, k, j)] = t.numpy()
        out.update(qc.flatten(name, qc.run_sequence(make(), calls, n_train, fwd)))
    save('qat_elementwise.npz', out)


def convs(Q):
    for n, (name, kwargs, shape) in enumerate(qc.CONV_CASES):
        mod = qc.make_conv(Q, kwargs)
        out = {'init.' + k: v.detach().clone().numpy() for k, v in mod.state_dict().items()}
        calls = qc.conv_inputs(400 + n, shape)
        for k, ins in enumerate(calls):
            out['in.%d.0' % k] = ins[0].numpy()
        out.update(qc.flatten('call', qc.run_sequence(mod, calls, 10, qc.fwd_single)))
        save('qat_conv_%s.npz' % name, out)


def net(ref, way):
    torch.manual_seed(0)
    model = ref.models.Darknet(micro_cfg(), (SIZE, SIZE), quantized=1, a_bit=8, w_bit=8, steps=STEPS, shortcut_way=way)
    assert sum(p.numel() for p in model.parameters()) == PARAMETERS
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert len(init) == STATE_KEYS[way], len(init)
    frames = qc.net_frames()
    grads, state = qc.run_net(model, frames)
    out = {'frames': frames}
    out.update({'init.' + k: v.numpy() for k, v in init.items()})
    out.update({'grad0.' + k: v.numpy() for k, v in grads.items()})
    out.update({'final.' + k: v.numpy() for k, v in state.items() if qc.is_decision(k)})
    save('qat_net_way%d.npz' % way, out)


def main():
    ref = refharness.load()
    Q = ref._modules['utils.quantized.quantized_google']
    only = sys.argv[1:]
    if not only or 'elementwise' in only:
        elementwise(Q)
    if not only or 'conv' in only:
        convs(Q)
    for way in (1, 2):
        if not only or 'net' in only:
            net(ref, way)


if __name__ == '__main__':
    main()
