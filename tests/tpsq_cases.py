"""Call sequences of the TPSQ (``quantized == 2``) module tests, shared by the fixture generator (which drives the REFERENCE's classes,
tests/golden/make_golden_tpsq.py) and the tests (which drive this package's).  Every function takes the namespace ``Q`` that holds the
classes; inputs are created here once, stored in the fixture, and replayed from it."""
import contextlib

import torch

import qat_cases as qc

DECISION_SUFFIXES = ('scale', 'warmup', 'step', 'first_bn', 'first_w')


def native_module():
    """This package's own ``utils.quantized.quantized_TPSQ`` (see ``qat_cases.native_module``)."""
    import conftest
    qc.native_module()
    import utils.quantized.quantized_TPSQ as Q
    assert (Q.__file__ or '').startswith(conftest.PKG), Q.__file__
    return Q


def is_decision(key):
    return key.split('.')[-1] in DECISION_SUFFIXES


@contextlib.contextmanager
def spy(Q):
    """Every raw value ``Search_Pow2`` is applied to while the context is open: per quantiser call [s0, p, p, p], and for a warm-up
    call the 99 candidates' [step * i, p_i, p_i, p_i] before them - the chosen ``step * max_step`` is the fourth from the end."""
    real = Q.Search_Pow2
    seen = []

    class Spy(real):
        @staticmethod
        def forward(ctx, input):
            seen.append(input.data.clone().reshape(-1))
            return real.forward(ctx, input)

    Q.Search_Pow2 = Spy
    try:
        yield seen
    finally:
        Q.Search_Pow2 = real


# ------------------------------------------------------------------------------------------------ the quantisers, one by one
# (name, class, bits, warmup flag set, input kind, number of training calls, scale factor applied before each call)
#   six calls: [warm-up +] train, train, scale x 1.3 then train, scale x 0.7 then train, train, eval
MOVES = (1.0, 1.0, 1.3, 0.7, 1.0, 1.0)
GAINS = (1.0, 2.5, 0.6, 4.0, 1.0, 3.0)
QUANT_CASES = [
    ('act-leaky-8', 'Activattion_Quantizer', 8, True, 'leaky', 5, MOVES),
    ('act-leaky-4', 'Activattion_Quantizer', 4, True, 'leaky', 5, MOVES),
    ('act-relu6-8', 'Activattion_Quantizer', 8, True, 'relu6', 5, MOVES),
    ('act-evalwarm-8', 'Activattion_Quantizer', 8, True, 'leaky', 0, (1.0, 1.3)),      # the first call in eval warms up too
    ('wgt-8', 'Weight_Quantizer', 8, False, 'weight', 5, MOVES),
    ('wgt-4', 'Weight_Quantizer', 4, False, 'weight', 5, MOVES),
    ('wgt-warm-8', 'Weight_Quantizer', 8, True, 'weight', 5, MOVES),                    # the flag set by hand, as a checkpoint could
    ('act-dead-8', 'Activattion_Quantizer', 8, True, 'dead', 2, (1.0, 1.0)),            # max(x) == 0: max_step stays -5, NaN output
]
ELEMENTWISE = [c[0] for c in QUANT_CASES] + ['bias-8', 'bias-4']


def make_quantizer(Q, cls, bits, warm):
    q = getattr(Q, cls)(bits=bits, out_channels=-1, warmup=True)
    with torch.no_grad():
        q.warmup.fill_(1.0 if warm else 0.0)
    return q


def quantizer_inputs(seed, kind, n):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        x = torch.randn(2, 3, 5, 7, generator=g) * GAINS[k % len(GAINS)]
        if kind == 'leaky':
            x = torch.nn.functional.leaky_relu(x, 0.1)
        elif kind == 'relu6':
            x = torch.nn.functional.relu6(x)
        elif kind == 'weight':
            x = x * 0.25
        elif kind == 'dead':
            x = -x.abs()
            x.view(-1)[::3] = 0.0
        if k == 1:
            x.view(-1)[:4] = torch.tensor([0.5, -0.5, 1.5, -2.5]) / 127      # rounding ties when the scale snaps to 1
        out.append([x])
    return out


def run_quantizer(Q, mod, calls, n_train, moves, device='cpu', record_sp=True):
    """Replay ``calls``: the first ``n_train`` in train mode, the rest in eval; before call k the scale parameter is multiplied by
    ``moves[k]`` (what an optimiser step does to it).  Per call: output, input gradient, scale gradient, every buffer and parameter
    afterwards, and (``record_sp``) the values Search_Pow2 saw."""
    rec = []
    mod.to(device)
    for k, ins in enumerate(calls):
        mod.train(k < n_train)
        mod.zero_grad()
        if moves[k] != 1.0:
            with torch.no_grad():
                mod.scale.mul_(moves[k])
        x = ins[0].clone().to(device).requires_grad_(True)
        with spy(Q) as seen:
            out = mod(x)
        (out * qc.upstream(out)).sum().backward()
        r = {'out': out.detach().cpu().clone(), 'gin0': x.grad.cpu().clone(), 'gp.scale': mod.scale.grad.cpu().clone()}
        if record_sp:
            r['sp'] = torch.cat(seen).cpu()
        for key, v in mod.state_dict().items():
            r['sd.' + key] = v.detach().cpu().clone()
        rec.append(r)
    return rec


def make_bias_quantizer(Q, bits):
    return Q.Bias_Quantizer(bits=bits, range_tracker=Q.GlobalRangeTracker())


def bias_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(24, generator=g) * gain + off] for gain, off in ((1.0, 0.0), (2.5, 0.5), (0.6, 1.0), (0.3, -1.0), (4.0, 0.0))]


def elementwise_records(Q, name, calls, device='cpu', record_sp=True):
    """The record of case ``name`` over ``calls`` (its recorded inputs)."""
    if name.startswith('bias-'):
        return qc.run_sequence(make_bias_quantizer(Q, int(name[5:])), calls, 4, qc.fwd_single, device=device)
    _, cls, bits, warm, _, n_train, moves = {c[0]: c for c in QUANT_CASES}[name]
    return run_quantizer(Q, make_quantizer(Q, cls, bits, warm), calls, n_train, moves, device=device, record_sp=record_sp)


def elementwise_inputs(name):
    if name.startswith('bias-'):
        return bias_inputs(700 + int(name[5:]))
    n, case = [(n, c) for n, c in enumerate(QUANT_CASES) if c[0] == name][0]
    return quantizer_inputs(600 + n, case[4], len(case[6]))


# ------------------------------------------------------------------------------------------------ the conv module
CONV_STEPS = qc.CONV_STEPS      # freeze_step 9: ten training calls cross it, then one eval call
CONV_CASES = qc.CONV_CASES


def make_conv(Q, kwargs, seed=0):
    torch.manual_seed(seed)
    return Q.TPSQ_BNFold_QuantizedConv2d_For_FPGA(a_bits=8, w_bits=8, steps=CONV_STEPS, **kwargs)


class ScaleGradBounds:
    """Hooks on the two learnable-scale quantisers of a conv module: after a backward, ``bounds()`` gives per scale gradient
    2^-19 of the absolute sums of its four per-element term sets (the first weighted 1.5 >= p / s0), from the quantiser's input, its
    snapped scale and the gradient that reached its output."""

    def __init__(self, mod):
        self.seen = {}
        for name in ('activation_quantizer', 'weight_quantizer'):
            getattr(mod, name).register_forward_hook(lambda m, ins, out, name=name: self._take(name, m, ins[0], out))

    def _take(self, name, m, x, out):
        entry = self.seen[name] = {'x': x.detach(), 'p': m.scale.detach().clone(), 'bits': m.bits}
        if out.requires_grad:
            out.register_hook(lambda g: entry.__setitem__('dy', g.detach()))

    def bounds(self):
        out = {}
        for name, e in self.seen.items():
            terms = torch_fake_quant(e['x'].reshape(-1), e['p'], e['bits'], e['dy'].reshape(-1))[2]
            out['bound.%s.scale' % name] = torch.tensor(2.0 ** -19 * sum((1.5 if k == 0 else 1.0) * t.double().abs().sum().item()
                                                                         for k, t in enumerate(terms)))
        return out


def run_conv(mod, calls, device='cpu', bounds=False):
    """Ten training calls and one eval call; before calls 4 and 7 both learnable scales move off their powers (x 1.3, x 0.7).
    ``bounds``: add the ``ScaleGradBounds`` of every call to its record."""
    rec = []
    mod.to(device)
    probe = ScaleGradBounds(mod) if bounds else None
    for k, ins in enumerate(calls):
        mod.train(k < 10)
        mod.zero_grad()
        if k in (4, 7):
            with torch.no_grad():
                mod.activation_quantizer.scale.mul_(1.3 if k == 4 else 0.7)
                mod.weight_quantizer.scale.mul_(0.7 if k == 4 else 1.3)
        rec.extend(_one_call(mod, ins, device))
        if probe is not None:
            rec[-1].update(probe.bounds())
    return rec


def _one_call(mod, ins, device):
    ins = [t.clone().to(device).requires_grad_(True) for t in ins]
    out = mod(ins[0])
    (out * qc.upstream(out)).sum().backward()
    r = {'out': out.detach().cpu().clone(), 'gin0': ins[0].grad.cpu().clone()}
    for name, p in mod.named_parameters():
        if p.grad is not None:
            r['gp.' + name] = p.grad.cpu().clone()
    for key, v in mod.state_dict().items():
        r['sd.' + key] = v.detach().cpu().clone()
    return [r]


# ------------------------------------------------------------------------------------------------ the kernels' element arithmetic
def torch_fake_quant(x, scale, bits, dy=None):
    """The torch formulas of one quantiser call (reference quantized_TPSQ.py:84-116) with the snapped scale ``p`` given as a
    one-element tensor on ``x``'s device: (y, dx, [t1, t2, t3, t4]) - the per-element terms of the four scale-gradient sums as
    autograd forms them."""
    qmul, qdiv = float((1 << (bits - 1)) - 1), float(1 << (bits - 1))
    p = scale
    a, b = x + p, x - p
    m = (0.5 * (a.abs() - b.abs())) * qmul
    q = m / p
    r = torch.sign(q) * torch.floor(q.abs() + 0.5)
    y = (r * p) / qdiv
    if dy is None:
        return y
    g_n = dy / qdiv
    g_q = g_n * p
    g_d = ((g_q / p) * qmul) * 0.5
    g_a, g_b = g_d * torch.sign(a), (-g_d) * torch.sign(b)
    return y, g_a + g_b, [g_a, -g_b, (-g_q) * ((m / p) / p), g_n * r]


def nearest_pow2(v):
    """Reference :37-42 on one float."""
    t = torch.tensor([v], dtype=torch.float32)
    hi, lo = 2 ** t.log2().ceil(), 2 ** t.log2().floor()
    return float(hi if abs(hi - t) < abs(lo - t) else lo)


# ------------------------------------------------------------------------------------------------ the micro net (tests/qat_minicfg.py)
NET_SCALES = 36             # a learnable activation and weight scale per conv block, on top of qat_minicfg.PARAMETERS
NET_STATE_KEYS = 312        # reference state_dict size (plain Shortcut: shortcut_way does not matter)
