"""Shared drivers for the training-path tests — TEST INFRASTRUCTURE ONLY.

``MINI_CFG`` is a 21-block cfg with every structure YOLOv3 trains through (3x3 / 1x1 / stride-2 convs with train-mode
BatchNorm + leaky, residual shortcuts, a multi-consumer tensor, route + 2x upsample + concat, two yolo heads) that is
shallow enough for fp32 gradients to be well conditioned: the eager fp32 autograd result and the HIP path must then
agree to round-off.  (Through the full 75-conv YOLOv3 with random weights the leaky-ReLU kinks make eager fp32 itself
differ from an fp64 run by ~1e-2 relative, so deep-net checks compare error against that eager-vs-fp64 error instead.)
"""
import copy
import os
import tempfile

import torch

import conftest  # noqa: F401
import synth
from models import Darknet

_CONV = '[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n'
_HEAD = '[convolutional]\nsize=1\nstride=1\npad=1\nfilters=21\nactivation=linear\n\n'
_YOLO = ('[yolo]\nmask = %s\nanchors = 4,5, 8,10, 13,16, 30,33, 42,40, 50,55\nclasses=2\nnum=6\njitter=.3\n'
         'ignore_thresh = .7\ntruth_thresh = 1\nrandom=1\n\n')


def mini_cfg_text(act='leaky'):
    c = lambda f, k, s: _CONV % (f, k, s, act)
    sc = '[shortcut]\nfrom=-3\nactivation=linear\n\n'
    return ('[net]\nbatch=1\nwidth=64\nheight=64\nchannels=3\n\n'
            + c(8, 3, 1) + c(16, 3, 2) + c(8, 1, 1) + c(16, 3, 1) + sc            # 0-4
            + c(32, 3, 2) + c(16, 1, 1) + c(32, 3, 1) + sc                        # 5-8
            + c(16, 1, 1) + c(32, 3, 1) + _HEAD + _YOLO % '3,4,5'                 # 9-12
            + '[route]\nlayers = -4\n\n' + c(8, 1, 1) + '[upsample]\nstride=2\n\n'  # 13-15
            + '[route]\nlayers = -1, 4\n\n' + c(16, 1, 1) + c(32, 3, 1) + _HEAD + _YOLO % '0,1,2')


def write_cfg(text):
    f = tempfile.NamedTemporaryFile('w', suffix='.cfg', delete=False)
    f.write(text)
    f.close()
    return f.name


def build(cfg_path, size, seed=0):
    torch.manual_seed(seed)
    model = Darknet(cfg_path, (size, size))
    state = model.state_dict()
    synth.randomize_bn_(state, seed=1)
    model.load_state_dict(state)
    return model.train()


def loss_weights(raws, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(tuple(p.shape), generator=g) for p in raws]


def toy_loss(raws, ws):
    """Smooth, dense function of every raw head element (linear + small quadratic term)."""
    return sum((p * w.to(p.device, p.dtype)).sum() + 0.005 * (p * p).sum() for p, w in zip(raws, ws))


def eager_step(model, x, ws=None, dtype=torch.float32):
    """Reference: the eager modules + autograd on ``model``'s device (CPU).  Returns raws, grads (by parameter name)."""
    m = copy.deepcopy(model).to(dtype).train()
    for p in m.parameters():
        p.grad = None
    raws = m._forward_eager(x.to(dtype))[0]
    ws = ws or loss_weights(raws)
    toy_loss(raws, ws).backward()
    grads = {k: (p.grad.float() if p.grad is not None else torch.zeros_like(p).float()) for k, p in m.named_parameters()}
    return [r.detach().float() for r in raws], grads, m, ws


def engine_step(model, x, ws, precision, lib=None, device='cpu'):
    """The HIP training path through ``Darknet._forward_hip_train`` (``lib`` = FakeLib on CPU, None = the real library)."""
    from engine.padded import make_train_engine
    m = copy.deepcopy(model).to(device).train()
    for p in m.parameters():
        p.grad = None
    os.environ['YOLO_HIP_TRAIN_PRECISION'] = precision
    try:
        if lib is not None:
            m.__dict__['_hip_train_engine'] = make_train_engine(m, precision, x.to(device), lib=lib)
        raws, feats = m._forward_hip_train(x.to(device))
        toy_loss(raws, ws).backward()
    finally:
        del os.environ['YOLO_HIP_TRAIN_PRECISION']
    grads = {k: (p.grad.float().cpu() if p.grad is not None else torch.zeros_like(p).float().cpu())
             for k, p in m.named_parameters()}
    return [r.detach().float().cpu() for r in raws], grads, m


PLAN_CASES = [(cfg, precision, False) for cfg in ('yolov3/yolov3.cfg', 'yolov4/yolov4.cfg', 'yolov3-mobilenet/yolov3-mobilenet-coco.cfg')
              for precision in ('fp16', 'fp32')] + [('yolov3/yolov3.cfg', 'fp16', True)]
# Further cases carry options after the three fields: size / batch, env (builder knobs, set around the build) and patch (attributes of
# engine.train set around the build: _FUSED_DGRAD_MAX_CIN is read at import).  ``cfg`` is a path below cfg/, a path below the
# repository (tests/golden/...) or one of the MINI_CFGS names.
MINI_CFGS = {"mini_cfg_text()": 'leaky', "mini_cfg_text('mish')": 'mish'}
_V3 = 'yolov3/yolov3.cfg'
PLAN_CASES += [
    ('yolov3tiny/yolov3-tiny.cfg', 'fp16', False),
    ('yolov3tiny/yolov3-tiny-hand.cfg', 'fp16', False),
    ('yolov4tiny/yolov4-tiny.cfg', 'fp16', False),
    ('yolov4tiny/yolov4-tiny.cfg', 'fp32', False),
    ('tests/golden/slim_prune_0.5_yolov3-mobilenet-coco.cfg', 'fp16', False),     # through the channel-padded twin
    ("mini_cfg_text()", 'fp16', False),
    ("mini_cfg_text('mish')", 'fp32', False),
    ('yolov4/yolov4.cfg', 'fp16', True),
    ('yolov3-mobilenet/yolov3-mobilenet-coco.cfg', 'fp16', True),
    (_V3, 'fp16', False, dict(size=96, batch=1)),
    (_V3, 'fp16', False, dict(env={'YOLO_HIP_FUSE_DBN': '0'})),
    (_V3, 'fp16', False, dict(env={'YOLO_HIP_STEM_STATS': '0'})),
    (_V3, 'fp16', False, dict(env={'YOLO_HIP_STEM_BWD': '0'})),
    (_V3, 'fp16', False, dict(env={'YOLO_HIP_STEM_DGRAD': '0'})),
    (_V3, 'fp16', False, dict(env={'YOLO_HIP_TILE': '24'})),
    (_V3, 'fp16', False, dict(env={'YOLO_HIP_TRAIN_SEGMENTS': '3'})),
    # every stride-2 data gradient in four parity phases
    (_V3, 'fp16', False, dict(env={'YOLO_HIP_STEM_DGRAD': '0'}, patch={'_FUSED_DGRAD_MAX_CIN': 0})),
]


def plan_case_options(case):
    return dict(case[3]) if len(case) > 3 else {}


def plan_case_id(case):
    opts = plan_case_options(case)
    words = [os.path.basename(case[0]), case[1]] + ['attention'] * bool(case[2])
    words += ['%s%s' % (k, opts[k]) for k in ('size', 'batch') if k in opts]
    words += ['%s=%s' % kv for k in ('env', 'patch') for kv in sorted(opts.get(k, {}).items())]
    return '-'.join(words)


def plan_case_fingerprint(case):
    """``plan_fingerprint`` of one PLAN_CASES entry: resolves its cfg, applies its options, and reports the cfg under the
    name the case gives it (the recorded rows hold no absolute path)."""
    import engine.train
    cfg, precision, attention = case[:3]
    opts = plan_case_options(case)
    patch = opts.pop('patch', {})
    path, temp = cfg, None
    if cfg in MINI_CFGS:
        path = temp = write_cfg(mini_cfg_text(MINI_CFGS[cfg]))
    elif cfg.startswith('tests/'):
        path = os.path.join(conftest.REPO, cfg)
    before = {k: getattr(engine.train, k) for k in patch}
    try:
        for k, val in patch.items():
            setattr(engine.train, k, val)
        row = plan_fingerprint(path, precision, attention, **opts)
    finally:
        for k, val in before.items():
            setattr(engine.train, k, val)
        if temp:
            os.unlink(temp)
    row['cfg'] = cfg
    if len(case) > 3:
        row['options'] = case[3]
    return row


def _plan_layout(plan):
    """The host-side plan contents the run path reads, as plain numbers (pieces by index and arena offset)."""
    out = dict(arena_need=plan['arena_need'], ws_floats=plan['ws_floats'], junk_n=plan['junk_n'], junk=plan['junk'],
               head_shapes=[list(s) for s in plan['head_shapes']],
               param_slices=[[off, n, list(shape)] for off, n, shape in plan['param_slices']],
               zero_list=[[t.index, t.off] for t in plan['zero_list']],
               storages=[len(plan['storages'])] + [t.off for t in plan['storages']],
               segments=[[list(seg['values']), list(seg['ops']), list(seg['params']), list(seg['heads'])] for seg in plan['segments']])
    if plan.get('kd_values'):
        out['kd'] = [[plan[k].n, plan[k].off] for k in ('kd_maps', 'kd_G', 'kd_partials')] + [len(plan['kd_values'])]
    return out


def plan_fingerprint(cfg, precision, attention=False, size=64, batch=2, env=None):
    """Build (never run) the training plan of ``cfg`` (a path below cfg/, or an absolute path) on the host emulation, with the
    environment variables ``env`` set around the build, and digest what the builder handed the plan API.  ``sha256``, per op: log
    name, kind, every non-pointer field (arrays as bytes), per pointer field null / fixup / other, and
    the sorted fixups (field offset, slot, byte offset) - the byte offsets pin the arena layout of every piece.  The emulation's
    weight-gradient workspace queries answer a non-zero constant, so the weight gradients' workspace fixups are in the digest.
    ``layout_sha256``: what the plan dict itself tells the run path (``_plan_layout``)."""
    import ctypes as C
    import hashlib
    import json
    import fakelib
    from engine.padded import make_train_engine

    class Lib(fakelib.FakeLib):
        def yh_conv2d_wgrad_workspace(self, dref):
            return 4096

        def yh_dw_wgrad_workspace(self, dref):
            return 4096

    lib = Lib()
    torch.manual_seed(0)
    model = Darknet(os.path.join(conftest.PKG, 'cfg', cfg), (size, size)).train()
    shape = (batch, 3, size, size)
    before = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        eng = make_train_engine(model, precision, shape, lib=lib)
        eng = getattr(eng, 'inner', eng)
        eng.attention = attention
        plan = eng._cached_plan(eng._plan_key(shape))
    finally:
        for k, val in before.items():
            if val is None:
                del os.environ[k]
            else:
                os.environ[k] = val
    out = dict(cfg=cfg, precision=precision, attention=attention, arena_need=plan['arena_need'])
    h = hashlib.sha256()
    for side in ('fwd', 'bwd'):
        ops, log = lib.plans[fakelib._addr(plan[side])]['ops'], plan[side + '_ops']
        assert len(ops) == len(log)
        out['n_' + side] = len(ops)
        for (kind, desc, fixups), (what, _) in zip(ops, log):
            fixed = {off for off, _, _ in fixups}
            h.update(('%s|%d|' % (what, kind)).encode())
            for name, ctype in desc._fields_:
                field = getattr(type(desc), name)
                raw = bytes(desc)[field.offset:field.offset + field.size]
                pointer = ctype is C.c_void_p or getattr(ctype, '_type_', None) is C.c_void_p
                h.update(('%s=' % name).encode())
                h.update((b'fixup' if field.offset in fixed else b'other' if any(raw) else b'null') if pointer else raw)
                h.update(b';')
            h.update(repr(sorted(fixups)).encode())
            h.update(b'\n')
    out['sha256'] = h.hexdigest()
    out['layout_sha256'] = hashlib.sha256(json.dumps(_plan_layout(plan), sort_keys=True).encode()).hexdigest()
    return out


def rel_l2(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-20)


def cosine(a, b):
    return (a.flatten() @ b.flatten()).item() / (a.norm().item() * b.norm().item() + 1e-20)
