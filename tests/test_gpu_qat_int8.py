"""QAT deployment on the MI355X: a ``quantized=1`` model in eval mode runs on the MFMA-i8 engine.

Reference of the network tests: the eager quantized=1 modules on the CPU with the same ``state_dict`` (tests/qat_int8_cases.py: the
fold of the synthetic state is one fp32 product per value and the frames are dyadic, so nothing depends on the host or on a
summation order) - the raw heads must be equal, whole tensors.  The decoded rows then differ only by the fp32 exp / sigmoid of the
decode kernel: the bound tests/test_ptq_large.py holds the int8 engine to on bit-exact heads (1e-5 relative, 1e-6 absolute).
``yh_qadd_clamped`` is called through the C ABI on buffers of this test's own against the header's formula in torch on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import conftest
import qat_int8_cases as cases
import synth
from engine import hiplib
from fakelib_qat_int8 import qadd_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return hiplib.load()


@pytest.fixture(scope='module', autouse=True)
def release_cached_blocks():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def engine_on(monkeypatch):
    monkeypatch.delenv('YOLO_HIP_QAT_INT8', raising=False)


# ------------------------------------------------------------------------------------------------------ 1. the networks
@pytest.mark.parametrize('name', cases.CASES)
def test_qat_model_runs_on_the_int8_engine_bit_exactly(lib, name):
    qm, x, (inf, ref_raws) = cases.case(name)
    qm.cuda()
    with torch.no_grad():
        io, raws, _ = qm(x.cuda())
    torch.cuda.synchronize()
    eng = qm.__dict__['_hip_engine']
    assert eng is not None and eng.precision == 'int8'
    for k, (a, b) in enumerate(zip(raws, ref_raws)):
        a = a.cpu()
        assert a.shape == b.shape and torch.equal(a, b), 'head %d: %d of %d values differ' % (k, (a != b).sum().item(), b.numel())
    d = (io.cpu() - inf).abs()
    print('decoded rows %s: max abs difference %.3g' % (name, d.max().item()))
    assert torch.allclose(io.cpu(), inf, rtol=1e-5, atol=1e-6), d.max().item()


# ------------------------------------------------------------------------------------------------------ 2. yh_qadd_clamped
GUARD = 3
# (rx, ra, scale_x, scale_a, scale_sum): ratios on both sides of 1; with a ratio of 2 or 4 every |operand| > 63 (> 31) clamps
RATIOS = [(2.0, 1.0, 2.0 ** -5, 2.0 ** -5, 2.0 ** -5), (0.5, 4.0, 2.0 ** -4, 2.0 ** -6, 2.0 ** -5), (1.0, 1.0, 2.0 ** -4, 2.0 ** -4, 2.0 ** -3),
          (0.25, 0.5, 2.0 ** -3, 2.0 ** -4, 2.0 ** -5), (2.0, 2.0, 2.0 ** -6, 2.0 ** -6, 2.0 ** -7)]
# sha256 of the plain yh_qadd formula (no operand clamp) evaluated with torch on a CPU for the inputs of _qadd_inputs, per (c, pixels)
# and ratio set: recorded when yh_qadd_clamped was added, so that yh_qadd itself is pinned to what it computed before
QADD_RECORDED = {
    (16, 1): 'e2ecaaaf8cf4add2e85cb9d2f689c1b7e34fe6e1515b38f6576e415fe6af87da', (16, 255): '34f35335e99a66fd716b12cf3c96395379e5eccfbea9e1fb9d09b04ed26a4b93', (16, 257): '1139facfff46daf885ef45fc2b165c5157ff7ddee4e51c2d4597c69a5ae73ca4', (48, 1): '0558bbaf27a65ddb6fc9e72a91236f87ad67b9d203cd6abbb1e1807d4fe93222', (48, 255): '3b6c06d1dd1b774df2a141d93a89a16bde0b75b9292dff840a0e21146ba6f37d', (48, 257): '05c12a187e2190f78dea5244220e5490fedcd4fbb2b7681558f2bd19acad1f44'}


def _qadd_inputs(c, pixels):
    g = torch.Generator().manual_seed(1000 * c + pixels)
    x = torch.randint(-128, 128, (pixels, c), generator=g, dtype=torch.int32)
    a = torch.randint(-128, 128, (pixels, c), generator=g, dtype=torch.int32)
    x.view(-1)[:4] = torch.tensor([127, -128, 64, -64], dtype=torch.int32)       # the ends of the range and the first value a ratio of 2 clamps
    a.view(-1)[:4] = torch.tensor([127, -128, -128, 127], dtype=torch.int32)
    return x.to(torch.int8), a.to(torch.int8)


def _run_qadd(lib, entry, x, a, ratios):
    """The entry on pitched device buffers (pitches larger than c, a different one per tensor) with a guard row behind the output."""
    pixels, c = x.shape
    ldx, lda, ldy = c + 16, c + 32, c + 48
    dx = torch.full((pixels, ldx), GUARD, dtype=torch.int8, device='cuda')
    da = torch.full((pixels, lda), GUARD, dtype=torch.int8, device='cuda')
    dy = torch.full((pixels + 1, ldy), GUARD, dtype=torch.int8, device='cuda')
    dx[:, :c] = x.cuda()
    da[:, :c] = a.cuda()
    rx, ra, sx, sa, ssum = ratios
    d = hiplib.QAddDesc(x=dx.data_ptr(), a=da.data_ptr(), y=dy.data_ptr(), pixels=pixels, c=c, ldx=ldx, lda=lda, ldy=ldy, rx=rx, ra=ra,
                        scale_x=sx, scale_a=sa, inv_scale_sum=1.0 / ssum)
    rc = getattr(lib, entry)(C.byref(d), hiplib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = dy.cpu()
    assert (out[pixels] == GUARD).all() and (out[:pixels, c:] == GUARD).all(), 'wrote outside its rows'
    return out[:pixels, :c]


@pytest.mark.parametrize('pixels', [1, 255, 257])
@pytest.mark.parametrize('c', [16, 48])
def test_qadd_clamped_against_the_torch_formula(lib, c, pixels):
    x, a = _qadd_inputs(c, pixels)
    plain = []
    acted = 0
    for ratios in RATIOS:
        rx, ra, sx, sa, ssum = ratios
        want = qadd_reference(x.float(), a.float(), rx, ra, sx, sa, 1.0 / ssum, True).to(torch.int8)
        unclamped = qadd_reference(x.float(), a.float(), rx, ra, sx, sa, 1.0 / ssum, False).to(torch.int8)
        got = _run_qadd(lib, 'yh_qadd_clamped', x, a, ratios)
        assert torch.equal(got, want), (ratios, (got != want).sum().item())
        got_plain = _run_qadd(lib, 'yh_qadd', x, a, ratios)
        assert torch.equal(got_plain, unclamped), (ratios, (got_plain != unclamped).sum().item())
        if max(rx, ra) <= 1:
            assert torch.equal(want, unclamped)          # the clamp cannot act on an int8 operand
        else:
            acted += int((want != unclamped).sum())
        assert int(want.min()) == -128 and int(want.max()) == 127      # the output clamp acts at both ends
        plain.append(got_plain)
    assert acted > 0, 'no input exercised the operand clamp'
    assert synth.tensor_digest(torch.stack(plain)) == QADD_RECORDED[(c, pixels)], 'yh_qadd changed'


# -------------------------------------------------------------------------------------------------------- 3. hip_detect
def _same_detections(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.shape == w.shape and torch.equal(g, w)


@pytest.mark.parametrize('multi_label', [False, True], ids=['best_class', 'multi_label'])
@pytest.mark.parametrize('name', ['yolov3-tiny', 'yolov3'])
def test_hip_detect_equals_nms_of_the_engines_own_rows(lib, name, multi_label):
    from utils.utils import non_max_suppression
    qm, x, (inf, _) = cases.case(name)
    qm.cuda()
    score = inf[..., 4] * inf[..., 5:].max(-1)[0] if multi_label else inf[..., 4]
    conf = float(torch.quantile(score.flatten(), 0.6)) * 0.999
    with torch.no_grad():
        rows = qm(x.cuda())[0]
        want = non_max_suppression(rows, conf, 0.6, multi_label=multi_label)
        got = qm.hip_detect(x.cuda(), conf, 0.6, multi_label=multi_label)
    torch.cuda.synchronize()
    assert qm.__dict__['_hip_engine'].precision == 'int8'
    assert sum(0 if w is None else len(w) for w in want) >= 4
    _same_detections(got, want)
    steps = {float(v) for k, v in qm.state_dict().items() if k.endswith('_quantizer.step')}
    assert steps == {2.0}                                  # two calls, two eager forwards' worth of step counters


# ------------------------------------------------------------------------------------- 4. train.py, test.py, detect.py
def _train_test_detect(dataset_dir, tiny_cfg, workdir, monkeypatch, engine):
    import models
    import train as train_mod
    import test as test_mod
    import detect as detect_mod
    workdir.mkdir()
    monkeypatch.chdir(workdir)
    if engine:
        monkeypatch.delenv('YOLO_HIP_QAT_INT8', raising=False)
    else:
        monkeypatch.setenv('YOLO_HIP_QAT_INT8', '0')
    seen = []
    forward_hip, hip_detect = models.Darknet._forward_hip, models.Darknet.hip_detect

    def spy_forward(self, x):
        out = forward_hip(self, x)
        seen.append(self.__dict__['_hip_engine'].precision)
        return out

    def spy_detect(self, x, *args, **kw):
        out = hip_detect(self, x, *args, **kw)
        eng = self.__dict__.get('_hip_engine')
        seen.append(eng.precision if eng is not None and self._use_hip(x) else 'eager')
        return out
    monkeypatch.setattr(models.Darknet, '_forward_hip', spy_forward)
    monkeypatch.setattr(models.Darknet, 'hip_detect', spy_detect)
    torch.manual_seed(0)
    np.random.seed(0)
    opt = train_mod.make_parser().parse_args(['--epochs', '3', '--batch-size', '2', '--cfg', tiny_cfg, '--data', str(dataset_dir / 'synth.data'),
                                              '--img-size', '64', '64', '64', '--device', '0', '--nosave', '--quantized', '1'])
    opt.local_rank = -1
    results = train_mod.train(opt, train_mod.hyp)
    assert len(results) == 7 and all(np.isfinite(results))
    during_training = list(seen)
    ckpt = torch.load('weights/last.pt', map_location='cpu', weights_only=False)['model']
    test_mod.opt = None
    (mp, mr, m_ap, mf1, *losses), maps = test_mod.test(tiny_cfg, str(dataset_dir / 'synth.data'), 'weights/last.pt', batch_size=2, imgsz=64,
                                                       plot=False, quantized=1, shortcut_way=1)
    assert 0.0 <= m_ap <= 1.0 and all(np.isfinite(losses))
    dopt = detect_mod.make_parser().parse_args(['--cfg', tiny_cfg, '--weights', 'weights/last.pt', '--source', str(dataset_dir / 'images'),
                                               '--output', 'out', '--img-size', '64', '--conf-thres', '0.001', '--device', '0',
                                               '--names', str(dataset_dir / 'synth.names'), '--quantized', '1'])
    assert len(detect_mod.detect(dopt)) == 12
    return ckpt, during_training, seen[len(during_training):]


def test_train_test_detect_evaluate_on_the_int8_engine(lib, dataset_dir, tiny_cfg, tmp_path, monkeypatch):
    ckpt, in_training, after = _train_test_detect(dataset_dir, tiny_cfg, tmp_path / 'engine', monkeypatch, True)
    assert in_training and set(in_training) == {'int8'}, in_training      # the per-epoch evaluation of train.py
    assert after and set(after) == {'int8'}, after                        # test.py and detect.py on the checkpoint
    eager, in_training0, after0 = _train_test_detect(dataset_dir, tiny_cfg, tmp_path / 'eager', monkeypatch, False)
    assert not in_training0 and set(after0) <= {'eager'}
    steps = [k for k in ckpt if k.endswith('.step')]
    assert len(steps) >= 4 * 11 and list(ckpt) == list(eager)
    for k in steps:
        assert torch.equal(ckpt[k], eager[k]), k
    assert max(float(ckpt[k]) for k in steps if k.endswith('_quantizer.step')) > 12      # the evaluations advanced them past the 12 training steps
