"""The micro detector of the QAT (``quantized == 1``) fixtures and GPU tests: the topology of ``ptq_minicfg.mini_cfg`` with every
width divided by 4 (the 24-channel head convs stay), 64 x 64 input, batch 2, ``steps=20`` - so the quantiser scales freeze at step 2
and the BatchNorm fold switches to running statistics at step 18.  37,228 parameters."""
import copy

from ptq_minicfg import mini_cfg

SIZE = 64
BATCH = 2
STEPS = 20
PARAMETERS = 37228
STATE_KEYS = {1: 525, 2: 522}      # reference state_dict sizes by shortcut_way (1: QuantizedShortcut_min, 2: _max)


def micro_cfg():
    blocks = copy.deepcopy(mini_cfg())
    blocks[0].update(width=SIZE, height=SIZE)
    for b in blocks[1:]:
        if b['type'] == 'convolutional' and b['filters'] != 24:
            b['filters'] //= 4
    return blocks
