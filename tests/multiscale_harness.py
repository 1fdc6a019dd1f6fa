"""Shared drivers of the multi-scale tests (tests/test_multiscale.py, tests/test_gpu_multiscale.py) — TEST INFRASTRUCTURE ONLY.

``run`` steps ONE model through a sequence of input shapes on the HIP training path (emulated ABI on the CPU, the real library on
a GPU): forward, toy loss, backward, a different input every step.  Engine "A" keeps its plans, which alias each other in the
engine's step arena; engine "B" has ``_drop_plans()`` called before every step, so each of its steps runs on a freshly built plan in
a fresh arena - what the parent commit did for every third shape.  The two must agree bit for bit.
"""
import copy
import os

import numpy as np
import torch

import conftest  # noqa: F401
import train_harness as th

# (N, H, W): 64^2, 96^2, 128^2, 64^2 again, a rectangle, 128^2 again, then the shorter last batch of an epoch
SEQUENCE = [(2, 64, 64), (2, 96, 96), (2, 128, 128), (2, 64, 64), (2, 64, 96), (2, 128, 128), (1, 96, 96)]
SHORT = [(2, 64, 64), (2, 96, 96), (2, 64, 64), (1, 96, 96)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def build_model(which):
    import models
    import synth
    if which == 'mini':
        path = th.write_cfg(th.mini_cfg_text())
        try:
            return th.build(path, 64)
        finally:
            os.unlink(path)
    cfg = {'tiny': os.path.join(conftest.PKG, 'cfg', 'yolov3tiny', 'yolov3-tiny.cfg'), 'slim': os.path.join(GOLDEN, 'slim_prune_mini.cfg')}[which]
    torch.manual_seed(0)
    model = models.Darknet(cfg, (64, 64))
    state = model.state_dict()
    synth.randomize_bn_(state, seed=1)
    model.load_state_dict(state)
    return model.train()


def batch(step, shape, device='cpu'):
    n, h, w = shape
    g = torch.Generator().manual_seed(100 + step)
    return torch.rand(n, 3, h, w, generator=g).to(device)


def largest(seq):
    n, h, w = max(seq, key=lambda s: s[0] * s[1] * s[2])
    return (n, 3, h, w)


class Stepper:
    def __init__(self, model, precision, lib=None, device='cpu'):
        self.m = copy.deepcopy(model).to(device).train()
        self.precision, self.lib, self.device = precision, lib, device

    @property
    def engine(self):
        return self.m.__dict__.get('_hip_train_engine')

    def make_engine(self, first):
        """``first``: a batch or an (N, C, H, W) shape."""
        from engine.padded import make_train_engine
        self.m.__dict__['_hip_train_engine'] = make_train_engine(self.m, self.precision, first, lib=self.lib)

    def reserve(self, shapes):
        if self.engine is None and self.lib is not None:
            self.make_engine(max(shapes, key=lambda s: s[0] * s[2] * s[3]))
        self.m.hip_reserve_train(shapes, precision=self.precision)

    def forward(self, x):
        os.environ['YOLO_HIP_TRAIN_PRECISION'] = self.precision
        try:
            if self.engine is None and self.lib is not None:
                self.make_engine(x)
            return self.m._forward_hip_train(x)[0]
        finally:
            del os.environ['YOLO_HIP_TRAIN_PRECISION']

    def step(self, x):
        for p in self.m.parameters():
            p.grad = None
        raws = self.forward(x)
        th.toy_loss(raws, th.loss_weights(raws, seed=5)).backward()
        heads = [r.detach().float().cpu().clone() for r in raws]
        grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad).float().cpu().clone() for k, p in self.m.named_parameters()}
        return heads, grads

    def bn_state(self):
        return {k: v.detach().cpu().clone() for k, v in self.m.state_dict().items()
                if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}

    def fill_arena_with_nan(self):
        arena = self.engine._arena
        if arena.buf is not None:
            arena.buf.fill_(255)         # 0xFFFF / 0xFFFFFFFF: a NaN in fp16 and in fp32


def run(model, precision, seq, lib=None, device='cpu', drop=False, nan_fill=False, reserve=None, stepper=None):
    """-> (per-step (heads, grads), BatchNorm state after the sequence, the stepper)."""
    st = stepper or Stepper(model, precision, lib, device)
    device = st.device
    if reserve:
        st.reserve(reserve)
    out = []
    for k, shape in enumerate(seq):
        if drop and st.engine is not None:
            st.engine._drop_plans()
        if nan_fill and st.engine is not None:
            st.fill_arena_with_nan()
        out.append(st.step(batch(k, shape, device)))
    return out, st.bn_state(), st


def assert_same(got, want):
    steps_a, bn_a = got
    steps_b, bn_b = want
    assert len(steps_a) == len(steps_b)
    for k, ((ha, ga), (hb, gb)) in enumerate(zip(steps_a, steps_b)):
        for a, b in zip(ha, hb):
            assert torch.equal(a, b), 'heads of step %d' % k
        assert set(ga) == set(gb)
        for name in gb:
            assert torch.equal(ga[name], gb[name]), 'gradient of %s in step %d' % (name, k)
    assert set(bn_a) == set(bn_b)
    for name in bn_b:
        assert torch.equal(bn_a[name], bn_b[name]), name


def restate_resize(x, size):
    """The formula of ``yh_resize_bilinear`` (include/yolo_hip.h) in numpy float32, every operation rounded once.
    ``x``: float32 array (N, C, H, W) -> (N, C, oh, ow)."""
    f32 = np.float32
    x = np.ascontiguousarray(x, dtype=f32)
    ih, iw = x.shape[2:]
    oh, ow = int(size[0]), int(size[1])

    def taps(in_size, out_size):
        scale = f32(in_size) / f32(out_size)
        s = scale * (np.arange(out_size, dtype=f32) + f32(0.5)) - f32(0.5)
        s = np.maximum(s, f32(0))
        i0 = np.minimum(s.astype(np.int32), in_size - 1)
        i1 = np.minimum(i0 + 1, in_size - 1)
        l1 = s - i0.astype(f32)
        return i0, i1, f32(1) - l1, l1

    y0, y1, hy0, hy1 = taps(ih, oh)
    x0, x1, wx0, wx1 = taps(iw, ow)
    r0, r1 = x[:, :, y0, :], x[:, :, y1, :]
    top = wx0 * r0[..., x0] + wx1 * r0[..., x1]
    bot = wx0 * r1[..., x0] + wx1 * r1[..., x1]
    out = hy0[:, None] * top + hy1[:, None] * bot
    assert out.dtype == f32
    return out
