"""QAT deployment (``--quantized 1`` checkpoints on the int8 engine), CPU tier: the lowering of the QAT eval graph replayed through the
host emulation of the C ABI against the eager ``quantized=1`` modules, the operand clamp of ``QuantizedShortcut_max``, eligibility
and fallback, the step counters, re-packing, and the ABI of the new entry."""
import copy
import os
import re
import types

import pytest
import torch

import conftest
import fakelib
import qat_int8_cases as cases
import qat_minicfg
from fakelib_qat_int8 import FakeLibQatInt8


def _engine(qm, lib=None):
    from engine.plan import DarknetEngine
    return DarknetEngine(qm, precision='int8', lib=lib or FakeLibQatInt8())


def _ops(eng):
    plan = next(iter(eng._plans.values()))
    kinds = [''.join(c for c in w if not c.isdigit()) for w, _ in plan['ops']]
    fused = [int(w[4:]) + 1 for w, d in plan['ops'] if w.startswith('conv') and d.res]      # the shortcut blocks inside conv epilogues
    return plan, kinds, fused


def _assert_heads_equal(raws, ref_raws):
    assert len(raws) == len(ref_raws)
    for k, (a, b) in enumerate(zip(raws, ref_raws)):
        assert a.shape == b.shape and torch.equal(a, b), 'head %d: %d of %d values differ' % (k, (a != b).sum().item(), b.numel())


# ------------------------------------------------------------------------------------------------------ 1. the lowering
@pytest.mark.parametrize('name', cases.CASES)
def test_qat_int8_lowering_is_bit_exact(name):
    """The raw heads of the int8 plan of a QAT graph equal the eager quantized=1 modules on the CPU, whole tensors (the comparison
    test_cfg_int8_lowering_is_bit_exact makes for the COS-PTQ graphs).  The micro detector's widths are no multiples of 16."""
    qm, x, (inf, ref_raws) = cases.case(name)
    eng = _engine(qm)
    io, raws, _ = eng(x)
    _assert_heads_equal(raws, ref_raws)
    assert torch.isfinite(inf).all() and max(r.unique().numel() for r in ref_raws) > 32      # a live detector, not a dead grid
    assert torch.allclose(io, inf, rtol=1e-5, atol=1e-6)
    _, kinds, fused = _ops(eng)
    assert 'stem' in kinds and 'yolo' in kinds
    if name in ('yolov3', 'yolov4'):
        assert len(fused) == 23 and kinds.count('qadd') == 0      # every residual of the backbone rides in a conv epilogue


def test_synthetic_qat_state_folds_without_rounding():
    """running_var + eps is exactly 1.0f: the fold is W * gamma and beta - mean * gamma, nothing a host could round differently."""
    qm, _, _ = cases.case('micro_min')
    n = 0
    for m in qm.modules():
        if m.__class__.__name__ == 'BNFold_QuantizedConv2d_For_FPGA' and m.bn:
            w, b = m.BN_fuse()
            assert bool((m.running_var + m.eps == 1.0).all())
            assert torch.equal(w, m.weight * m.gamma.reshape(-1, 1, 1, 1)) and torch.equal(b, m.beta - m.running_mean * m.gamma)
            n += 1
    assert n >= 10


# ------------------------------------------------------------------------------------------- 2. QuantizedShortcut_max's clamp
class _NoOperandClamp(FakeLibQatInt8):
    """yh_qadd's arithmetic where the plan asks for yh_qadd_clamped: what the engine would compute without the new kernel."""

    def yh_qadd_clamped(self, dref, stream):
        return fakelib.FakeLib.yh_qadd(self, dref, stream)


def _coarse_operand_state():
    """micro_max with one shortcut put on HALF its x operand's grid step: rx = 2, and that operand's clamped peaks (|q| up to 127)
    re-quantise to 254 - the clamp of QuantizedShortcut_max acts."""
    qm, x, _ = cases.case('micro_max')
    _, _, fused = _ops_of_fresh(qm, x)
    j = fused[0]                                            # a shortcut that rides in its conv's epilogue in the default state
    sc = qm.module_list[j]
    assert sc.__class__.__name__ == 'QuantizedShortcut_max'
    sc.scale = qm.module_list[j - 1][0].activation_quantizer.scale.clone() / 2
    return qm, x, j


def _ops_of_fresh(qm, x):
    eng = _engine(copy.deepcopy(qm))
    eng(x)
    return _ops(eng)


def test_shortcut_max_operand_clamp_equals_eager_and_needs_the_clamp():
    qm, x, j = _coarse_operand_state()
    with torch.no_grad():
        _, ref_raws, _ = copy.deepcopy(qm)(x)
    eng = _engine(qm)
    _, raws, _ = eng(x)
    plan, kinds, fused = _ops(eng)
    assert j not in fused and 'qadd%d' % j in [w for w, _ in plan['ops']]      # rx > 1: the separate op, not the epilogue
    d = next(d for w, d in plan['ops'] if w == 'qadd%d' % j)
    assert d.rx == 2.0 and type(d).__name__ == 'QAddClampedDesc' and 'qadd_clamped' in eng.lib.calls
    # the operand really reaches values the clamp changes
    a = eng.block_output(plan, j - 1)
    assert (a.abs() / float(qm.module_list[j - 1][0].activation_quantizer.scale)).max().item() * d.rx > 127
    _assert_heads_equal(raws, ref_raws)
    _, plain, _ = _engine(copy.deepcopy(qm), lib=_NoOperandClamp())(x)
    assert any(not torch.equal(a, b) for a, b in zip(plain, ref_raws)), 'the state does not exercise the operand clamp'


def test_shortcut_max_with_fine_operands_takes_the_fused_epilogue():
    """rx <= 1 and ra <= 1: the clamp cannot act on an int8 operand, the shortcut rides in the conv epilogue and equals eager."""
    qm, x, (_, ref_raws) = cases.case('micro_max')
    eng = _engine(qm)
    _, raws, _ = eng(x)
    plan, kinds, fused = _ops(eng)
    assert len(fused) == 2
    for j in fused:
        sc, d = qm.module_list[j], next(d for w, d in plan['ops'] if w == 'conv%d' % (j - 1))
        assert sc.__class__.__name__ == 'QuantizedShortcut_max' and 0 < d.q_rx <= 1 and 0 < d.q_ra <= 1
    _assert_heads_equal(raws, ref_raws)


# ---------------------------------------------------------------------------------------------- 3. eligibility and fallback
def _fresh():
    import models
    torch.manual_seed(0)
    return models.Darknet(qat_minicfg.micro_cfg(), (cases.SIZE, cases.SIZE), quantized=1, a_bit=8, w_bit=8, shortcut_way=1,
                          steps=qat_minicfg.STEPS).eval()


def _four_bit():
    return cases.build(None, 1, a_bit=4)[1]


def _mobilenet():
    return cases.build('yolov3-mobilenet/yolov3-mobilenet-coco.cfg', 1)[1]


def _edited_shortcut(edit):
    blocks = qat_minicfg.micro_cfg()
    j = next(i for i, b in enumerate(blocks) if b['type'] == 'shortcut')
    edit(blocks, j)
    return cases.build(blocks, 1)[1]


def _weighted():
    return _edited_shortcut(lambda blocks, j: blocks[j].update(weights_type='sigmoid'))


def _width_mismatch():
    return _edited_shortcut(lambda blocks, j: blocks[j - 1].update(filters=blocks[j - 1]['filters'] + 8))


@pytest.mark.parametrize('make, word', [(_fresh, 'power of two'), (_four_bit, 'bits'), (_mobilenet, 'depthwise'), (_weighted, 'weighted'),
                                        (_width_mismatch, 'widths')])
def test_graphs_that_do_not_qualify_fall_back_and_the_engine_refuses(make, word, monkeypatch):
    from engine.plan import qat_int8_reason
    monkeypatch.delenv('YOLO_HIP_QAT_INT8', raising=False)
    qm = make()
    block, text = qat_int8_reason(qm)
    assert word in text
    on_gpu = types.SimpleNamespace(is_cuda=True)          # _use_hip reads the flag alone
    assert qm._use_hip(on_gpu) is False and qm.__dict__['_qat_int8'] is False      # decided once, cached
    x = cases.frames()
    with torch.no_grad():
        inf = qm(x)[0]                                     # the eager modules run it, no exception
    assert inf.shape[0] == cases.BATCH
    with pytest.raises(NotImplementedError, match='block %d' % block):
        _engine(qm)(x)


def test_qualifying_graph_is_selected_and_the_switch_keeps_eager(monkeypatch):
    monkeypatch.delenv('YOLO_HIP_QAT_INT8', raising=False)
    qm, _, _ = cases.case('micro_min')
    on_gpu = types.SimpleNamespace(is_cuda=True)
    assert qm._use_hip(on_gpu) is True and qm._hip_eval_precision() == 'int8'
    assert qm._use_hip(types.SimpleNamespace(is_cuda=False)) is False
    monkeypatch.setenv('YOLO_HIP_QAT_INT8', '0')
    assert qm._use_hip(on_gpu) is False
    monkeypatch.delenv('YOLO_HIP_QAT_INT8')
    monkeypatch.setenv('YOLO_QAT_TORCH', '1')              # the quantiser passes of the eager modules: does not select the engine
    assert qm._use_hip(on_gpu) is True
    qm.train()
    assert qm.__dict__['_qat_int8'] is None and qm._use_hip(on_gpu) is False
    qm.eval()
    assert qm._use_hip(on_gpu) is True
    for drop in (lambda: qm.load_state_dict(qm.state_dict()), lambda: qm.float(), qm.hip_refresh):
        drop()
        assert qm.__dict__['_qat_int8'] is None
        assert qm._use_hip(on_gpu) is True


def test_cos_ptq_and_float_refusals_are_unchanged():
    """A float conv in an int8 plan still raises; a TPSQ graph (quantized == 2) is never routed to the engine."""
    import models
    fm = models.Darknet(qat_minicfg.micro_cfg(), (cases.SIZE, cases.SIZE)).eval()
    with pytest.raises(NotImplementedError):
        _engine(fm)(cases.frames())
    tm = models.Darknet(qat_minicfg.micro_cfg(), (cases.SIZE, cases.SIZE), quantized=2, a_bit=8, w_bit=8, steps=qat_minicfg.STEPS).eval()
    assert tm._use_hip(types.SimpleNamespace(is_cuda=True)) is False


# ------------------------------------------------------------------------------------------------------ 4. state fidelity
def _quantizers(qm):
    return [q for m in qm.modules() if m.__class__.__name__ == 'BNFold_QuantizedConv2d_For_FPGA'
            for q in (m.weight_quantizer, m.bias_quantizer, m.activation_quantizer)]


def test_engine_path_leaves_the_state_dict_of_the_eager_path():
    qa, x, (_, ref_raws) = cases.case('micro_min')
    qb = copy.deepcopy(qa)
    qa.__dict__['_hip_engine'] = _engine(qa)
    for q in _quantizers(qa)[::2]:
        q._mirror = float(q.step)                          # host mirrors from earlier fused calls (the others have none)
    with torch.no_grad():
        for _ in range(3):
            out_a = qa._forward_hip(x)                     # what forward_once calls for a GPU batch
            out_b = qb(x)
    _assert_heads_equal(out_a[1], ref_raws)
    sa, sb = qa.state_dict(), qb.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    steps = [float(q.step) for q in _quantizers(qa)]
    assert steps and set(steps) == {3.0}
    assert all(q._mirror is None or q._mirror == float(q.step) for q in _quantizers(qa))      # none is stale
    assert sum(q._mirror is not None for q in _quantizers(qa)) == len(_quantizers(qa)[::2])
    # one training forward from there: the freeze schedule (Scale_freeze_step = 2, the counters are at 3) behaves the same
    qa.train()
    qb.train()
    assert qa.__dict__['_hip_engine'] is None
    ya, yb = qa(x)[0], qb(x)[0]
    for a, b in zip(ya, yb):
        assert torch.equal(a, b)
    sa, sb = qa.state_dict(), qb.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_augmented_detect_counts_three_forwards():
    qm, x, _ = cases.case('micro_min')
    qm._qat_advance_steps(3)
    assert set(float(q.step) for q in _quantizers(qm)) == {3.0}


# ------------------------------------------------------------------------------------------------------------ 5. re-pack
def test_weight_update_and_recalibration_repack():
    qm, x, _ = cases.case('micro_min')
    eng = _engine(qm)
    eng(x)
    sig = eng._current_signature()
    conv = qm.module_list[2][0]
    with torch.no_grad():
        conv.weight.mul_(-0.5)                             # an optimizer step: in place
    assert eng._current_signature() != sig
    with torch.no_grad():
        _, ref_raws, _ = copy.deepcopy(qm)(x)
    _assert_heads_equal(eng(x)[1], ref_raws)
    sig = eng._current_signature()
    q = conv.activation_quantizer
    q.scale = q.scale * 2                                  # update_params rebinds the buffer
    assert eng._current_signature() != sig
    with torch.no_grad():
        _, ref2, _ = copy.deepcopy(qm)(x)
    assert any(not torch.equal(a, b) for a, b in zip(ref2, ref_raws))
    _assert_heads_equal(eng(x)[1], ref2)


# ---------------------------------------------------------------------------------------------------------------- 6. ABI
def test_qadd_clamped_is_exported_and_the_abi_version_stays():
    from engine import hiplib
    lib = hiplib.load()
    assert lib.yh_abi_version() == 2 == hiplib.ABI_VERSION
    assert 'yh_qadd_clamped' in hiplib.EXPORTS and hasattr(lib, 'yh_qadd_clamped')
    header = open(os.path.join(conftest.REPO, 'include', 'yolo_hip.h')).read()
    assert int(re.search(r'YH_OP_QADD_CLAMPED = (\d+)', header).group(1)) == hiplib.OP_QADD_CLAMPED
    assert hiplib.OP_KIND[hiplib.QAddClampedDesc] == hiplib.OP_QADD_CLAMPED
    # host-side argument checks (no launch): misaligned channel count, null pointers
    d = hiplib.QAddDesc(pixels=4, c=24, ldx=32, lda=32, ldy=32, rx=1.0, ra=1.0, scale_x=1.0, scale_a=1.0, inv_scale_sum=1.0)
    assert lib.yh_qadd_clamped(d, None) == -1
    d.x = d.a = d.y = 4096
    assert lib.yh_qadd_clamped(d, None) == -2
