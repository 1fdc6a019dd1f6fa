"""Call sequences of the QAT (``quantized == 1``) module tests, shared by the fixture generator (which drives the REFERENCE's
classes, tests/golden/make_golden_qat.py) and the tests (which drive this package's).  Every function takes the namespace ``Q`` that
holds the classes; inputs are created here once, stored in the fixture, and replayed from it."""
import itertools

import numpy as np
import torch

DECISION_SUFFIXES = ('scale', 'zero_point', 'input_scale', 'step', 'first_bn', 'first_a', 'first_w')


def native_module():
    """This package's own ``utils.quantized.quantized_google``.  tests/test_ptq.py installs an eval-only stand-in package under
    ``utils.quantized`` when it runs first (it has no search path): drop it, like tests/test_ptq_calibration.py does."""
    import sys
    import conftest
    foreign = lambda mod: not (getattr(mod, '__file__', None) or '').startswith(conftest.PKG)
    for name in ('utils.quantized.quantized_ptq_cos', 'utils.quantized'):
        if name in sys.modules and foreign(sys.modules[name]):
            del sys.modules[name]
    import utils
    if hasattr(utils, 'quantized') and foreign(utils.quantized):
        del utils.quantized
    import utils.quantized.quantized_google as Q
    assert not foreign(Q), Q.__file__
    return Q


def upstream(out):
    """The gradient fed into a module's output: small dyadic values, a function of the shape alone."""
    return ((torch.arange(out.numel(), dtype=torch.float32) % 7) - 3).mul(0.25).reshape(out.shape).to(out.device)


def is_decision(key):
    return key.split('.')[-1] in DECISION_SUFFIXES


# ------------------------------------------------------------------------------------------------ elementwise / tracker modules
QUANT_FREEZE = 3
QUANT_GAINS = (1.0, 2.5, 0.6, 4.0, 1.0, 3.0)        # five training calls (three before the scale freeze), then one eval call
QUANT_CASES = [('%s-%s-%s-%d' % (c[:4], t[:4], 's' if s else 'u', b), c, t, s, b)
               for c, t, s, b in itertools.product(('SymmetricQuantizer', 'AsymmetricQuantizer'),
                                                   ('GlobalRangeTracker', 'AveragedRangeTracker'), (True, False), (8, 4))]
SHORTCUT_CASES = [('min-same', 'QuantizedShortcut_min', 6, 6), ('min-wide', 'QuantizedShortcut_min', 6, 4),
                  ('max-same', 'QuantizedShortcut_max', 6, 6), ('max-narrow', 'QuantizedShortcut_max', 4, 6)]
PAIR_GAINS = (1.0, 3.0, 0.5, 2.0, 6.0)              # four training calls, then one eval call (beyond the tracked range)


def make_quantizer(Q, cls, tracker, sign, bits):
    rt = getattr(Q, tracker)(q_level='L', out_channels=-1)
    return getattr(Q, cls)(bits=bits, range_tracker=rt, out_channels=-1, Scale_freeze_step=QUANT_FREEZE, sign=sign)


def quantizer_inputs(seed, sign):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(2, 3, 5, 7, generator=g) * gain + (0.0 if sign else 0.75 * gain) for gain in QUANT_GAINS]
    xs[1].view(-1)[:4] = torch.tensor([0.5, -0.5, 1.5, -2.5]) * 2.0 ** -5      # rounding ties of a power-of-two scale
    return [[x] for x in xs]


def pair_inputs(seed, cx, ca, zero_first=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, gain in enumerate(PAIR_GAINS):
        x = torch.randn(2, cx, 4, 5, generator=g) * gain
        a = torch.randn(2, ca, 4, 5, generator=g) * (gain * 0.5 + 0.25)
        if zero_first and k == 0:
            a.zero_()              # its float_max_list entry stays 0: the concat's first-call rule fires for it one call later
        out.append([x, a])
    return out


def run_sequence(mod, calls, n_train, fwd, device='cpu'):
    """Replay ``calls`` (a list of input lists): the first ``n_train`` in train mode, the rest in eval.  Per call: output, input
    gradients, parameter gradients and the whole state afterwards (as host tensors)."""
    rec = []
    mod.to(device)
    for k, ins in enumerate(calls):
        mod.train(k < n_train)
        mod.zero_grad()
        ins = [t.clone().to(device).requires_grad_(True) for t in ins]
        out = fwd(mod, ins)
        (out * upstream(out)).sum().backward()
        r = {'out': out.detach().cpu().clone()}
        for j, t in enumerate(ins):
            r['gin%d' % j] = t.grad.cpu().clone()
        for name, p in mod.named_parameters():
            if p.grad is not None:
                r['gp.' + name] = p.grad.cpu().clone()
        for key, v in mod.state_dict().items():
            r['sd.' + key] = v.detach().cpu().clone()
        rec.append(r)
    return rec


def fwd_single(mod, ins):
    return mod(ins[0])


def fwd_shortcut(mod, ins):
    return mod(ins[0], [ins[1]])


def fwd_concat(mod, ins):
    return mod(None, list(ins))


def elementwise_cases(Q):
    """(name, module factory, calls factory, number of training calls, forward) of every elementwise / tracker case."""
    cases = []
    for n, (name, cls, tracker, sign, bits) in enumerate(QUANT_CASES):
        cases.append(('q.' + name, lambda cls=cls, tracker=tracker, sign=sign, bits=bits: make_quantizer(Q, cls, tracker, sign, bits),
                      lambda n=n, sign=sign: quantizer_inputs(100 + n, sign), 5, fwd_single))
    for n, (name, cls, cx, ca) in enumerate(SHORTCUT_CASES):
        cases.append(('s.' + name, lambda cls=cls: getattr(Q, cls)(layers=[0], bits=8),
                      lambda n=n, cx=cx, ca=ca: pair_inputs(200 + n, cx, ca), 4, fwd_shortcut))
    cases.append(('c.concat', lambda: Q.QuantizedFeatureConcat(layers=[0, 1], groups=False, bits=8),
                  lambda: pair_inputs(300, 6, 4, zero_first=True), 4, fwd_concat))
    return cases


ELEMENTWISE = [c[0] for c in elementwise_cases(None)]


# ------------------------------------------------------------------------------------------------ the conv module
CONV_STEPS = 10       # Scale_freeze_step 1, BN_freeze_step 9: ten training calls cross both, then one eval call
CONV_CASES = [
    ('c3x3', dict(in_channels=8, out_channels=16, kernel_size=3, stride=1, padding=1, bias=False, bn=1, activate='leaky'), (2, 8, 16, 16)),
    ('c1x1', dict(in_channels=16, out_channels=24, kernel_size=1, stride=1, padding=0, bias=True, bn=0, activate='linear'), (2, 16, 16, 16)),
    ('dw3x3', dict(in_channels=16, out_channels=16, kernel_size=3, stride=2, padding=1, groups=16, bias=False, bn=1, activate='h_swish'),
     (2, 16, 16, 16)),
]


def make_conv(Q, kwargs, seed=0):
    torch.manual_seed(seed)
    return Q.BNFold_QuantizedConv2d_For_FPGA(a_bits=8, w_bits=8, steps=CONV_STEPS, **kwargs)


def conv_inputs(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(shape, generator=g) * (1.0 + 0.5 * (k % 3))] for k in range(11)]


# ------------------------------------------------------------------------------------------------ the micro net
NET_ITERS = 20


def net_frames(seed=5):
    """Four uint8 batches; iteration ``it`` sees batch ``it % 4`` as k / 256."""
    from qat_minicfg import BATCH, SIZE
    return np.random.RandomState(seed).randint(0, 256, (4, BATCH, 3, SIZE, SIZE)).astype(np.uint8)


def run_net(model, frames, iters=NET_ITERS, device='cpu'):
    """``iters`` training forwards without weight updates; returns (iteration-0 parameter gradients, state after the last)."""
    model.train()
    grads = {}
    for it in range(iters):
        x = (torch.from_numpy(frames[it % len(frames)]).float() / 256).to(device)
        res = model(x)
        heads = res[0] if isinstance(res, tuple) else res
        if it == 0:
            model.zero_grad()
            sum(p.float().pow(2).mean() for p in heads).backward()
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return grads, {k: v.detach().clone() for k, v in model.state_dict().items()}


# ------------------------------------------------------------------------------------------------ fixture layout
def flatten(prefix, rec):
    """{'<prefix>.<call>.<field>': ndarray} of a run_sequence record."""
    return {'%s.%d.%s' % (prefix, k, f): v.numpy() for k, r in enumerate(rec) for f, v in r.items()}


def unflatten(npz, prefix):
    rec = {}
    for key in npz.files:
        if key.startswith(prefix + '.'):
            k, f = key[len(prefix) + 1:].split('.', 1)
            if k.isdigit():
                rec.setdefault(int(k), {})[f] = torch.from_numpy(npz[key])
    return [rec[k] for k in sorted(rec)]


def recorded_calls(z, prefix):
    """The input lists of a case's calls, as recorded in the fixture."""
    calls, k = [], 0
    while '%s.in.%d.0' % (prefix, k) in z.files:
        j, ins = 0, []
        while '%s.in.%d.%d' % (prefix, k, j) in z.files:
            ins.append(torch.from_numpy(z['%s.in.%d.%d' % (prefix, k, j)]))
            j += 1
        calls.append(ins)
        k += 1
    return calls


def rel_l2(a, b):
    a, b = a.double(), b.double()
    den = b.norm().item()
    return (a - b).norm().item() / den if den else (a - b).norm().item()


# ------------------------------------------------------------------------------------------------ power-of-two selection
def sweep_values():
    """x = m 2^k, k = -10 .. 10, m around the 0.75 decision point and at both ends of [0.5, 1)."""
    one = np.float32(1)
    ms = [np.float32(0.5), np.nextafter(np.float32(0.75), np.float32(0)), np.float32(0.75), np.nextafter(np.float32(0.75), one),
          np.nextafter(one, np.float32(0))]
    return np.array([np.ldexp(m, k) for k in range(-10, 11) for m in ms], dtype=np.float32)


def reference_pow2(x):
    """The reference's expression (quantized_google.py:189-194) in torch, element by element."""
    out = []
    for v in torch.from_numpy(x):
        v = v.reshape(1)
        lo, hi = 2 ** v.log2().floor(), 2 ** v.log2().ceil()
        out.append(float(hi if abs(hi - v) < abs(lo - v) else lo))
    return np.array(out, dtype=np.float32)
