"""GPU tier: the data gradient in the descriptor form of engine/train_plan.py ``_dgrad``, on every kernel that accepts it.

The planner runs every data gradient as ``yh_conv2d_fwd`` on the transposed weight image: x = dz read at pitch lddz (wider than
its channel count inside a concat parent), y = a channel slice of a wider gradient buffer, and in accumulate mode res is the SAME
pointer as y (ldr = ldy): the kernel reads its residual from the rows it is about to overwrite.  Here that form is built for one
kernel at a time (``tile``), at sizes of a few thousand pixels, and compared with float64 ``torch.nn.grad.conv2d_input`` on the
same stored operands plus the prior buffer content, computed on the CPU:

  (a) integer operands: every product and partial sum is exact in fp32 in any order and the result is an integer of magnitude
      <= 2048, exact in fp16 - the kernel must give the reference bit for bit;
  (b) quarter / eighth operands in accumulate mode: still exact in fp32, but the true sum needs ONE fp16 rounding - a kernel that
      rounds the convolution before it adds the residual differs in a few per cent of the outputs;
  (c) random operands within the bound tests/test_gpu_train.py::test_dgrad_matches_autograd uses.

Everything outside the slice must keep its sentinel, a written slice must hold none, dz must be unchanged.  ACCEPTED / REFUSED below
are the tile codes csrc/conv_igemm.hip yh_conv2d_fwd takes or refuses for each form (read off the dispatcher and the pick_* /
*_supported functions); tests/test_abi.py::test_data_gradient_kernels_are_the_tested_ones holds the automatic choice of every
shipped network to ACCEPTED.  Runs on the host emulation under YOLO_TEST_DRY_GPU=1 (which vets this file, not the kernels).
"""
import collections
import functools
import os

import pytest
import torch

import conftest  # noqa: F401
import fakelib
import ops_harness as oh
from engine import hiplib

pytestmark = pytest.mark.gpu

F16, F32, I8 = hiplib.YH_F16, hiplib.YH_F32, hiplib.YH_I8
DRY = bool(os.environ.get('YOLO_TEST_DRY_GPU'))
GPU = 'cpu' if DRY else 'cuda'
EINVAL, EUNSUPPORTED = -1, -3      # include/yolo_hip.h
SENT = -1234.5                     # exact in fp16; no result of (a) (integers) or (c) (|values| << 1000) equals it


@pytest.fixture(scope='module')
def libs():
    if DRY:
        return fakelib.FakeLib(), fakelib.FakeLib()
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load(), fakelib.FakeLib()


# ------------------------------------------------------------------------------------------------------------------- tables
FORMS = ('plain3', 'plain1', 'phase', 'fused')     # 3x3 / s1; 1x1; stride 2 as four ups = 3 launches; stride 2 as one ups = 4 launch
GEOMETRY = {'plain3': (3, 1, 1), 'plain1': (1, 1, 0), 'phase': (3, 2, 1), 'fused': (3, 2, 1)}       # k, stride, pad of the layer

RING_REG = (1, 2, 3, 4, 5, 6)                       # register-staged tiles, 4-unit K step
RING_K8 = (11, 12, 14, 15, 16)                      # the same with an 8-unit K step (K a multiple of 64 fp16 / 32 fp32 channels)
RING_LDS = (21, 22, 24, 25, 26, 27, 31, 32, 34, 35)   # LDS-DMA ring, 3 / 4 stages
HALO = (41, 42)                                     # 3x3 / s1 / p1 halo kernel, 128 / 256 rows
PP = (61, 62, 63, 64, 65, 66, 67, 68, 69)           # full-line K step and ping-pong kernels: fp16, K == cin_k, a multiple of 64
RING = RING_REG + RING_K8 + RING_LDS

# tile codes yh_conv2d_fwd accepts for the form (0 = the automatic choice); fp32 only has the ring and halo kernels
ACCEPTED = {
    'plain3': (0,) + RING + HALO + (43,) + PP + (72,),      # 72: 32 / 64 rows over one K step, and the two-step 64 -> 32 form
    'plain1': (0,) + RING + PP + (71, 73),                  # 71: write mode only; 73: the instantiated (MT, KS, MS)
    'phase': (0,) + RING + PP,
    'fused': (0,) + RING_LDS,
}
F32_TILES = (0,) + RING + HALO

# (form, tile, dtype or None = both, mode or None = both, why): refused with YH_EINVAL / YH_EUNSUPPORTED, buffer untouched.
# 51 / 52 are the no-load / no-MFMA ablation codes of the profiling runs (garbage by design): neither accepted nor refused here.
NO_SUCH = 'no such tile code'
REFUSED = (
    [('plain3', t, None, None, NO_SUCH) for t in (7, 13, 23, 28, 33, 36, 44, 60, 70, 74)] +
    [('plain3', 71, None, None, 'the streaming 1x1 kernel has no 3x3 window'),
     ('plain3', 73, None, None, 'the LDS-weights kernel is 1x1 only'),
     ('plain3', 43, F32, None, 'halo ping-pong: fp16 / int8 only'),
     ('plain3', 72, F32, None, 'streaming 3x3: fp16 / int8 only')] +
    [('plain3', t, F32, None, 'full-line K step kernels: fp16 / int8 only') for t in PP] +
    [('plain1', t, None, None, NO_SUCH) for t in (13, 23, 33, 44, 70, 74)] +
    [('plain1', t, None, None, 'the halo kernels are 3x3 / s1 / p1 only') for t in HALO + (43,)] +
    [('plain1', 72, None, None, 'the streaming 3x3 kernel has no 1x1 window'),
     ('plain1', 71, F16, 'acc', 'the streaming 1x1 kernel has no residual'),
     ('plain1', 71, F32, None, 'streaming 1x1: fp16 / int8 only'),
     ('plain1', 73, F32, None, 'LDS-weights 1x1: fp16 / int8 only')] +
    [('plain1', t, F32, None, 'full-line K step kernels: fp16 / int8 only') for t in PP] +
    [('phase', t, None, None, NO_SUCH) for t in (13, 23, 33, 70)] +
    [('phase', t, None, None, 'the halo kernels have no phase scatter') for t in HALO + (43,)] +
    [('phase', t, None, None, 'the streaming kernels have no phase scatter') for t in (71, 72, 73)] +
    [('phase', t, F32, None, 'full-line K step kernels: fp16 / int8 only') for t in PP] +
    [('fused', t, None, None, 'the four-phase scatter is in the LDS-DMA ring epilogue only')
     for t in RING_REG + RING_K8 + HALO + (43,) + PP + (71, 72, 73)] +
    [('fused', t, None, None, NO_SUCH) for t in (23, 28, 33, 36)])

Case = collections.namedtuple('Case', 'form N H W K M dz_off lddz g_ld g_off only')


def _case(form, N, H, W, K, M, dz_off=0, lddz=None, g_ld=None, g_off=0, only=None):
    """(N, H, W) of the gradient buffer; K dz channels -> M gradient rows; dz = channels [dz_off, dz_off + K) of lddz, the data
    gradient = channels [g_off, g_off + M) of g_ld; ``only``: the tiles this extra shape is for (None: every accepted tile)."""
    return Case(form, N, H, W, K, M, dz_off, lddz or dz_off + K, g_ld or g_off + M, g_off, only)


def _sliced(c, dz_off=32, g_off=48, tail=16):
    return c._replace(dz_off=dz_off, lddz=dz_off + c.K + 32, g_off=g_off, g_ld=g_off + c.M + tail)


_S2 = [(2, 21, 24, 128, 64), (1, 25, 27, 64, 32), (1, 9, 9, 64, 24)]      # odd sizes: the four phases have different extents
CASES = {
    'plain3': [_case('plain3', 2, 19, 19, 128, 64), _case('plain3', 5, 7, 5, 256, 64),                 # several images per pixel tile
               _case('plain3', 2, 13, 17, 64, 96, dz_off=32, lddz=128, g_ld=160, g_off=48),             # non-square, three slices
               _case('plain3', 2, 20, 20, 128, 24),                                                     # row tail
               _case('plain3', 1, 10, 10, 1024, 512),                                                   # sixteen chunks, K = 9216
               _case('plain3', 1, 24, 152, 128, 64),                                                    # wide rows for the halo kernels
               # the streaming 3x3 kernel: one K step onto 64 / 32 rows, and its two-step 64 -> 32 form
               _case('plain3', 2, 13, 17, 32, 64, dz_off=32, lddz=96, g_ld=160, g_off=48, only=(0, 72)),
               _case('plain3', 1, 9, 11, 32, 32, only=(0, 72)), _case('plain3', 2, 20, 20, 64, 32, g_ld=64, g_off=16, only=(0, 72))],
    'plain1': [_case('plain1', 3, 37, 41, 128, 256), _case('plain1', 1, 3, 5, 128, 64),
               _case('plain1', 2, 29, 30, 64, 32, dz_off=32, lddz=128, g_ld=96, g_off=48)] +
              # the other instantiated (MT, KS, MS) of the LDS-weights kernel and (MT, KS) of the streaming kernel
              [_case('plain1', 1, 9, 11, K, M, only=(0, 71, 73)) for K, M in ((32, 64), (64, 128), (256, 128), (128, 128), (32, 128), (128, 32))] +
              [_sliced(_case('plain1', 1, 9, 11, 64, 64, only=(0, 71, 73)))],
    'phase': [_case('phase', *c) for c in _S2] + [_sliced(_case('phase', *c)) for c in _S2],
    'fused': [_case('fused', *c) for c in _S2] + [_sliced(_case('fused', *c)) for c in _S2],
}


def _round_up(a, b):
    return (a + b - 1) // b * b


def _hpp_geometry_ok(W, cin_k, bk=32):
    """csrc/conv_halo_pp.hip hpp_geometry: the halo image of a 512-position tile must fit the LDS in 5 .. 9 load pieces."""
    rows = _round_up(512 + 2 * (W + 1) + 2, 16)
    pieces, chunks = -(-(rows // 16) // 8), cin_k // bk
    pieces = 9 if pieces == 8 else pieces
    if pieces < 5 or pieces > 9 or (chunks > 1 and pieces > 7):
        return False
    return (4 * 128 * 4 + (2 if chunks > 1 else 1) * rows * 4 + 64) * 16 + rows * 4 <= 160 * 1024


_PWL_F16 = {(2, 2, 1), (4, 1, 1), (4, 4, 1), (8, 2, 1), (8, 8, 1), (8, 4, 2), (8, 4, 1), (4, 2, 1)}      # conv_pw_lds.hip pwl_f16_case
_PW = {(2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (8, 1)}                                                   # conv_pointwise.hip launch_pw


def applicable(c, tile, code, acc):
    """The documented shape conditions of a tile (row count, whole K steps, K == cin_k, 16-byte slices); form, dtype and residual
    are the tables' business."""
    if c.only is not None and tile not in c.only:
        return False
    if code == F32:
        return tile in RING_REG + RING_LDS + HALO + (0,) or (tile in RING_K8 and c.K % 32 == 0)
    cin_k = _round_up(c.K, 32)
    vec_ok = c.g_ld % 8 == 0 and c.g_off % 8 == 0 and c.lddz % 8 == 0 and c.dz_off % 8 == 0 and c.M % 8 == 0
    if tile in RING_K8:
        return cin_k % 64 == 0
    if tile in PP:
        return c.K == cin_k and cin_k % 64 == 0
    if tile == 43:
        return vec_ok and _hpp_geometry_ok(c.W, cin_k)
    if tile == 72:
        return vec_ok and ((cin_k == 32 and c.M in (32, 64)) or (cin_k == 64 and c.M == 32))
    if tile == 71:
        mt = 2 if c.M <= 32 else (4 if c.M <= 64 else 8)
        return vec_ok and not acc and c.K == cin_k and c.M <= 128 and (mt, cin_k // 32) in _PW
    if tile == 73:
        if not vec_ok or c.K != cin_k or c.M % 16 or not 32 <= c.M <= 256 or cin_k > 256 or c.M * cin_k * 2 > 64 * 1024:
            return False
        ms = 2 if c.M > 128 else 1
        return (c.M // (16 * ms), cin_k // 32, ms) in _PWL_F16
    return True


def _id(c, tile, code, mode):
    return '%s-t%d-n%d_%dx%d_c%d-%d%s-%s-%s' % (c.form, tile, c.N, c.H, c.W, c.K, c.M, '_sl' if c.g_off or c.dz_off else '',
                                                 'fp16' if code == F16 else 'fp32', mode)


def _params(codes, modes):
    out = []
    for form in FORMS:
        for c in CASES[form]:
            for code in codes:
                for mode in modes:
                    for tile in ACCEPTED[form]:
                        if (code == F32 and tile not in F32_TILES) or (form == 'plain1' and tile == 71 and mode == 'acc'):
                            continue       # REFUSED rows: dtype / residual
                        if applicable(c, tile, code, mode == 'acc'):
                            out.append(pytest.param(c, tile, code, mode, id=_id(c, tile, code, mode)))
    return out


EXACT = _params((F16, F32), ('write', 'acc'))
ONE_ROUNDING = _params((F16,), ('acc',))


# ---------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=4)
def _operands(c, code, part):
    """CPU operands of a case (shared by all tiles and both modes): w, the wide dz buffer, the prior content of the slice, and
    the float64 data gradient of the stored operands, (N, H, W, M)."""
    k, stride, pad = GEOMETRY[c.form]
    dt = oh.tdtype(code)
    g = torch.Generator().manual_seed(1000 * FORMS.index(c.form) + sum(c[1:10]) + {'a': 0, 'b': 1, 'c': 2}[part])
    Ho, Wo = (c.H + 2 * pad - k) // stride + 1, (c.W + 2 * pad - k) // stride + 1
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    if part == 'a':
        w, dz, prior = ri(-2, 2, (c.K, c.M, k, k)), ri(-3, 3, (c.N, Ho, Wo, c.lddz)), ri(-8, 8, (c.N, c.H, c.W, c.M))
    elif part == 'b':
        top = 64 if k == 1 else 32
        w, dz, prior = ri(-4, 4, (c.K, c.M, k, k)), ri(-top, top, (c.N, Ho, Wo, c.lddz)) / 4, ri(-64, 64, (c.N, c.H, c.W, c.M)) / 8
    else:
        w = (torch.randn(c.K, c.M, k, k, generator=g) * (c.K * k * k) ** -0.5).to(dt).float()
        dz, prior = torch.randn(c.N, Ho, Wo, c.lddz, generator=g).to(dt).float(), torch.randn(c.N, c.H, c.W, c.M, generator=g).to(dt).float()
    def dgrad64(dz):
        dzs = dz[..., c.dz_off:c.dz_off + c.K].double().permute(0, 3, 1, 2)
        return torch.nn.grad.conv2d_input((c.N, c.M, c.H, c.W), w.double(), dzs, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()

    conv = dgrad64(dz)
    while part == 'b' and _share(conv, prior) < 0.01 and k * k * c.K * 4 * (2 * top) * 4 < 2 ** 24 and 2 * conv.abs().max().item() + 8 < 30000:
        # Short sums (few dz channels, or the one to four taps a stride-2 pixel sees) stay below 512, where fp16 still holds every
        # quarter: the convolution then needs no rounding of its own and one rounding cannot be told from two.  The range of k is
        # doubled until 1 % of the REFERENCE's outputs can, while every partial sum stays below 2^24 quarters (exact in fp32) and
        # the result well within fp16's range.
        top *= 2
        dz = ri(-top, top, (c.N, Ho, Wo, c.lddz)) / 4
        conv = dgrad64(dz)
    return dict(w=w, dz=dz.to(dt), prior=prior.to(dt), conv=conv, dev={})


def _share(conv, prior):
    """Share of the outputs at which fp16(conv + prior) differs from fp16(fp16(conv) + prior): both from the float64 reference."""
    once = (conv + prior.double()).to(torch.float16)
    twice = (conv.to(torch.float16).double() + prior.double()).to(torch.float16)
    return (once != twice).float().mean().item()


def _run(lib, c, tile, code, mode, part, rcs=None):
    """One data gradient the way the planner emits it -> (wide buffer after, wide buffer before, operands), all on the CPU."""
    k, stride, pad = GEOMETRY[c.form]
    op = _operands(c, code, part)
    if 'dz' not in op['dev']:
        op['dev'].update(dz=op['dz'].to(GPU), w=op['w'].to(GPU))
    before = torch.full((c.N, c.H, c.W, c.g_ld), SENT, dtype=oh.tdtype(code))
    if mode == 'acc':
        before[..., c.g_off:c.g_off + c.M] = op['prior']
    buf = before.to(GPU).clone()
    kw = dict(acc=buf) if mode == 'acc' else dict(out=buf)
    got = oh.dgrad(lib, code, op['dev']['dz'], op['dev']['w'], (c.H, c.W), stride, pad, fused=c.form == 'fused', tile=tile,
                   dz_off=c.dz_off, g_ld=c.g_ld, g_off=c.g_off, rcs=rcs, **kw)
    if GPU == 'cuda':
        torch.cuda.synchronize()
    assert got is buf
    assert torch.equal(op['dev']['dz'].cpu(), op['dz']), 'dz was written'
    return buf.cpu(), before, op


def _check_outside(c, after, before):
    keep = torch.ones(c.g_ld, dtype=torch.bool)
    keep[c.g_off:c.g_off + c.M] = False
    assert torch.equal(after[..., keep], before[..., keep]), 'channels outside the slice were written'


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('c,tile,code,mode', EXACT)
def test_dgrad_is_exact_on_integers(libs, c, tile, code, mode):
    """(a): w in [-2, 2], dz in [-3, 3], prior gradient in [-8, 8], all integers - the float64 reference cast to the storage type,
    bit for bit; sentinels outside the slice kept, none left inside, dz unchanged."""
    lib, _ = libs
    after, before, op = _run(lib, c, tile, code, mode, 'a')
    ref = op['conv'] + (op['prior'].double() if mode == 'acc' else 0)
    assert ref.abs().max().item() <= 2048
    got = after[..., c.g_off:c.g_off + c.M]
    bad = got.double() != ref
    assert torch.equal(got, ref.to(got.dtype)), (int(bad.sum()), bad.nonzero()[:4].tolist(), (got.double() - ref).abs().max().item())
    assert not (got == SENT).any()
    _check_outside(c, after, before)


@pytest.mark.parametrize('c,tile,code,mode', ONE_ROUNDING)
def test_dgrad_accumulate_rounds_once(libs, c, tile, code, mode):
    """(b): w integers in [-4, 4], dz = k / 4 with |k| <= 32 (1x1: 64; the range doubled on short sums, see _operands),
    prior = k / 8: exact in fp32, and the true sum conv + prior needs one fp16 rounding.  At least 1 % of the outputs tell one
    rounding from two (a condition on the operands, asserted on the reference)."""
    lib, _ = libs
    after, before, op = _run(lib, c, tile, code, mode, 'b')
    ref = op['conv'] + op['prior'].double()
    assert ref.abs().max().item() < 30000
    once = ref.to(torch.float16)
    twice = (op['conv'].to(torch.float16).double() + op['prior'].double()).to(torch.float16)
    share = _share(op['conv'], op['prior'])
    assert share >= 0.01, share
    got = after[..., c.g_off:c.g_off + c.M]
    bad = got != once
    assert torch.equal(got, once), (int(bad.sum()), int((bad & (got == twice)).sum()), bad.nonzero()[:4].tolist())
    _check_outside(c, after, before)


RANDOM = [pytest.param(c, tile, code, mode, id=_id(c, tile, code, mode))
          for c in (CASES['plain3'][0], CASES['plain1'][0], CASES['phase'][3], CASES['fused'][3])
          for code in (F16, F32) for mode in ('write', 'acc') for tile in (0, 24, 41, 43, 64, 73)
          if tile in ACCEPTED[c.form] and (code == F16 or tile in F32_TILES) and applicable(c, tile, code, mode == 'acc')]


@pytest.mark.parametrize('c,tile,code,mode', RANDOM)
def test_dgrad_on_random_operands(libs, c, tile, code, mode):
    """(c): the bound of test_gpu_train.py::test_dgrad_matches_autograd, 2.5e-3 (fp16) / 2e-5 (fp32) of max |ref|."""
    lib, _ = libs
    after, before, op = _run(lib, c, tile, code, mode, 'c')
    ref = op['conv'] + (op['prior'].double() if mode == 'acc' else 0)
    got = after[..., c.g_off:c.g_off + c.M]
    tol = 2e-5 if code == F32 else 2.5e-3
    assert (got.double() - ref).abs().max().item() <= tol * ref.abs().max().item()
    assert not (got == SENT).any()
    _check_outside(c, after, before)


def _refusals():
    out = []
    for form, tile, code, mode, why in REFUSED:
        for cd in ((F16, F32) if code is None else (code,)):
            for md in (('write', 'acc') if mode is None else (mode,)):
                # where the tile runs the form in fp16 write mode: a shape it takes there, so that dtype / residual is the one reason
                fit = [c for c in CASES[form] if tile in ACCEPTED[form] and applicable(c._replace(only=None), tile, F16, False)]
                c = (fit or CASES[form])[0]
                out.append(pytest.param(c, tile, cd, md, id=_id(c, tile, cd, md)))
    return out


@pytest.mark.parametrize('c,tile,code,mode', _refusals())
def test_refused_tiles_leave_the_buffer_alone(libs, c, tile, code, mode):
    """Every (form, tile) of REFUSED on real, correctly sized tensors: YH_EINVAL / YH_EUNSUPPORTED from every launch of the form,
    and not a byte of the gradient buffer changed ("refused, not approximated")."""
    lib, _ = libs
    rcs = []
    after, before, _ = _run(lib, c, tile, code, mode, 'a', rcs=rcs)
    assert len(rcs) == (4 if c.form == 'phase' else 1) and all(rc in (EINVAL, EUNSUPPORTED) for rc in rcs), rcs
    assert torch.equal(after, before)


def test_tables_are_disjoint_and_every_accepted_tile_has_three_cases():
    """Each tile of ACCEPTED ran at least three cases of (a) + (b) in its form (the parametrisation holds no skips, so what was
    generated is what ran); no (form, tile) is both accepted and refused without a dtype / mode condition."""
    ran = collections.Counter((p.values[0].form, p.values[1]) for p in EXACT + ONE_ROUNDING)
    for form in FORMS:
        for tile in ACCEPTED[form]:
            assert ran[(form, tile)] >= 3, (form, tile, ran[(form, tile)])
            modes = {p.values[3] for p in EXACT if p.values[0].form == form and p.values[1] == tile}
            assert modes == ({'write'} if (form, tile) == ('plain1', 71) else {'write', 'acc'}), (form, tile, modes)
    for form, tile, code, mode, _ in REFUSED:
        assert tile not in ACCEPTED[form] or code is not None or mode is not None, (form, tile)
        assert tile not in (0, 51, 52)


def cases_per_tile():
    """{(form, tile): cases of (a) + (b)} - for the record in the pull request."""
    return collections.Counter((p.values[0].form, p.values[1]) for p in EXACT + ONE_ROUNDING)


# ------------------------------------------------------------------------------------------ forward counterpart
FWD_F16 = [(24, 2, 13, 17, 64, 96, 3, 1), (26, 5, 7, 5, 256, 64, 3, 0), (43, 2, 19, 19, 128, 64, 3, 1), (64, 1, 10, 10, 1024, 512, 3, 0),
           (72, 1, 25, 27, 64, 32, 3, 1), (73, 3, 37, 41, 128, 256, 1, 1)]
FWD_I8 = [(24, 2, 13, 17, 64, 96, 3, 1), (43, 2, 19, 19, 128, 64, 3, 0), (72, 1, 25, 27, 64, 32, 3, 1)]


def _leaky8(t, act):
    return torch.where(t > 0, t, t * 0.125) if act == 1 else t


@pytest.mark.parametrize('case', [('f16',) + c for c in FWD_F16] + [('i8',) + c for c in FWD_I8],
                         ids=lambda c: '%s_t%d_n%d_%dx%d_c%d-%d_k%d_a%d' % c)
def test_conv_residual_from_a_channel_slice(libs, case):
    """The forward form nothing else builds: the residual is a channel slice of a wider buffer (res_off > 0, ldr != cout) and y is a
    slice of a buffer of ANOTHER pitch.  Integer operands, linear or leaky with slope 1/8: the float64 reference (int8: the eval
    arithmetic as test_int8_conv_matches_torch_directly restates it, then the quantised shortcut with power-of-two ratios) is
    matched exactly, and both wide buffers keep what lies outside the slices."""
    lib, _ = libs
    kind, tile, N, H, W, cin, cout, k, act = case
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(sum(case[1:]))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    pad = (k - 1) // 2
    x_off, ldx, res_off, ldr, y_off, ldy = 32, cin + 64, 16, cout + 48, 32, cout + 80
    if kind == 'f16':
        w, cb = ri(-2, 2, (cout, cin, k, k)).float(), ri(-4, 4, (cout,)).float()
        x, res = ri(-3, 3, (N, H, W, ldx)).half(), ri(-8, 8, (N, H, W, ldr)).half()
        y = torch.full((N, H, W, ldy), SENT, dtype=torch.float16)
        packed, bias, cin_k, m_pad = oh.pack_conv(lib, F16, w.to(GPU), cb=cb.to(GPU))
        yd, rd, xd = y.to(GPU), res.to(GPU), x.to(GPU)
        oh.conv(lib, F16, xd, packed, bias, cin_k, m_pad, cout, k, 1, pad, act=act, slope=0.125, res=rd, tile=tile, cin=cin,
                x_off=x_off, y=yd, y_off=y_off, res_off=res_off)
        conv = F.conv2d(x[..., x_off:x_off + cin].double().permute(0, 3, 1, 2), w.double(), cb.double(), 1, pad)
        want = _leaky8(conv, act).permute(0, 2, 3, 1) + res[..., res_off:res_off + cout].double()
        assert torch.equal(want.half().double(), want) and want.abs().max().item() <= 2048      # representable: a condition on the operands
        want = want.half()
    else:
        acc_scale, out_scale, qadd = 2.0 ** -6, 1.0, (4.0, 1.0, 2.0 ** -6, 2.0 ** -6, 2.0 ** 5)
        w, qb = ri(-8, 8, (cout, cin, k, k)).float(), ri(-64, 64, (cout,)).float() / 4
        x, res = ri(-16, 16, (N, H, W, ldx)).to(torch.int8), ri(-128, 127, (N, H, W, ldr)).to(torch.int8)
        y = torch.full((N, H, W, ldy), 99, dtype=torch.int8)
        yd, rd, xd = y.to(GPU), res.to(GPU), x.to(GPU)
        oh.qconv(lib, xd, w.to(GPU), 1.0, qb.to(GPU), acc_scale, out_scale, k, 1, pad, act=act, slope=0.125, tile=tile, cin=cin,
                 x_off=x_off, y=yd, y_off=y_off, res=rd, res_off=res_off, qadd=qadd)
        rnd = lambda t: torch.sign(t) * torch.floor(t.abs() + 0.5)
        acc = F.conv2d(x[..., x_off:x_off + cin].double().permute(0, 3, 1, 2), w.double(), None, 1, pad)      # exact integers
        assert acc.abs().max().item() < 2 ** 24
        q = torch.clamp(rnd(_leaky8(acc * acc_scale + qb.double().view(1, -1, 1, 1), act) / out_scale), -128, 127).permute(0, 2, 3, 1)
        r = res[..., res_off:res_off + cout].double()
        want = torch.clamp(rnd((rnd(q * qadd[0]) * qadd[2] + rnd(r * qadd[1]) * qadd[3]) * qadd[4]), -128, 127).to(torch.int8)
        assert want.abs().max().item() > 20 and (want.abs() >= 127).float().mean().item() < 0.5      # a meaningful range, not saturated
    if GPU == 'cuda':
        torch.cuda.synchronize()
    got = yd.cpu()
    bad = got[..., y_off:y_off + cout] != want
    assert torch.equal(got[..., y_off:y_off + cout], want), (int(bad.sum()), bad.nonzero()[:4].tolist())
    keep = torch.ones(ldy, dtype=torch.bool)
    keep[y_off:y_off + cout] = False
    assert torch.equal(got[..., keep], y[..., keep]), 'y outside its slice was written'
    assert torch.equal(rd.cpu(), res) and torch.equal(xd.cpu(), x), 'an input was written'
