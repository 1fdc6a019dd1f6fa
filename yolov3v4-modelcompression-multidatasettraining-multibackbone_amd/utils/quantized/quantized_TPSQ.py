"""Quantization-aware training with BatchNorm folding and learnable power-of-two scales, TPSQ (``--quantized 2``).

Fresh, condensed implementation of the module family the reference keeps in ``utils/quantized/quantized_TPSQ.py`` (same class names,
constructor signatures, parameters, buffers and ``state_dict`` keys, so checkpoints move in both directions with ``strict=True``).
The graph takes its concat from ``quantized_google.QuantizedFeatureConcat`` and keeps the plain ``Shortcut``, as the reference's
``models.py`` does (:253-267, :273).  What the reference does and a reader might take for a slip is kept:

* ``Search_Pow2`` (reference :29-63) snaps the scale PARAMETER itself, in place, to the power of two nearest in absolute distance (the tie
  ``1.5 * 2^e`` goes down, :39-42) and returns it.  A quantiser call applies it four times (:85, :91, :102): the first application sees
  the raw value ``s0`` and backpropagates with the factor ``p / s0`` (:50-51), the other three see ``p`` and have the factor 1.  Its two
  range clamps (:35-36) write into copies and do nothing, so they are not here; a scale of 0, a negative scale and a NaN scale give
  NaN outputs, as torch computes them.
* ``Quantizer`` (:66-130): ``clamp`` is ``0.5 * (|x + p| - |x - p|)`` (:84-85); ``quantize`` multiplies by ``2^(bits-1) - 1`` (127, :90-91)
  and ``dequantize`` divides by ``2^(bits-1)`` (128, :101-102).
* ``Weight_Quantizer.__init__`` passes ``warmup`` in ``out_channels``' place (:247), so its ``warmup`` buffer is 0 at construction and only
  the activation quantiser warms up.  The warm-up (:262-282, :307-328) runs whenever the buffer is non-zero, in eval too:
  ``step = max(x) / 100``, candidates ``step * i`` for ``i = 1 .. 99``, cosine similarity of the fake-quantised tensor, a strict ``>`` from
  ``max_metrics = -1, max_step = -5`` (the first maximum; all-NaN cosines leave ``-5``), ``scale = step * max_step`` not snapped - the
  forward that follows snaps it.
* ``GlobalRangeTracker`` (:147-163) reads its own buffers through aliases like the Google one: after the first call it tracks
  ``min(0, current min)`` / ``max(0, current max)``.  ``Bias_Quantizer.scale`` (:171, :186) is a buffer that ``update_params`` rebinds.
* ``TPSQ_BNFold_QuantizedConv2d_For_FPGA`` (:349-589): BN momentum 0.01, ``torch.var`` unbiased (also for ``running_var``),
  ``freeze_step = int(0.9 * steps)``, ``step`` advances in training only, the ``first_bn`` rule (:424-428).

Host tensors run the reference's arithmetic operation for operation.  Dense fp32 GPU tensors with a one-element scale run the same
arithmetic as fused HIP passes (``engine/tpsq.py`` -> ``csrc/tpsq.hip``): one forward kernel per quantiser call (which snaps the
parameter), one backward kernel plus a finishing wave for ``dx`` and the scale's gradient, one search pass for the warm-up; the bias
quantiser runs on mode 1's kernels.  The Python-side decisions (``warmup``, ``step < freeze_step``, the ``first_bn`` rule) use host
mirrors, initialised by one read per module after construction or ``load_state_dict``; a training step after warm-up reads nothing
back.  ``YOLO_TPSQ_TORCH=1`` forces the torch formulas on GPU tensors too (the reference's eager arithmetic with its host reads).  fp16
tensors (autocast) and per-channel scales always take the torch formulas.

The reference's text dumps for its FPGA flow (``quantizer_output=True``) are not part of this package.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.nn import init
from torch.nn.parameter import Parameter

from .quantized_google import _Mirrored, _no_fpga_dump, reshape_to_activation, reshape_to_bias, reshape_to_weight  # noqa: F401


def _tpsq():
    from engine import tpsq
    return tpsq


def _torch_forced():
    return os.environ.get('YOLO_TPSQ_TORCH', '0') == '1'


# ---------------------------------------------------------------------------------------------- quantisers
class Round(Function):
    """Round half away from zero, straight-through gradient (:15-26)."""

    @staticmethod
    def forward(self, input):
        sign = torch.sign(input)
        return sign * torch.floor(torch.abs(input) + 0.5)

    @staticmethod
    def backward(self, grad_output):
        return grad_output.clone()


class Search_Pow2(Function):
    """(:29-63) ``input`` is the scale parameter: its value is replaced by the nearest power of two and the parameter is returned."""

    @staticmethod
    def forward(self, input):
        input_data = input.data.clone()
        output = input
        ceil_float_range = 2 ** output.log2().ceil()
        floor_float_range = 2 ** output.log2().floor()
        if abs(ceil_float_range - output) < abs(floor_float_range - output):
            output.data.copy_(ceil_float_range.data)      # in place (the reference rebinds .data): the same value at a stable address
        else:
            output.data.copy_(floor_float_range.data)
        output_data = output.data.clone()
        self.save_for_backward(input_data, output_data)
        return output

    @staticmethod
    def backward(self, grad_output):
        input, output = self.saved_tensors
        scale = output / input
        return scale * grad_output.clone()


class Quantizer(_Mirrored, nn.Module):
    def __init__(self, bits, out_channels, warmup=False):
        super().__init__()
        self.first = True
        self.momentum = 0.1
        self.bits = bits
        self.register_buffer('warmup', torch.ones(1) if warmup else torch.zeros(1))

    def clamp(self, input):
        return 0.5 * (torch.abs(input + Search_Pow2.apply(self.scale)) - torch.abs(input - Search_Pow2.apply(self.scale)))

    def quantize(self, input):
        quantized_range = torch.tensor((1 << (self.bits - 1)) - 1)
        return (input * quantized_range) / Search_Pow2.apply(self.scale)

    def round(self, input):
        return Round.apply(input)

    def dequantize(self, input):
        quantized_range = torch.tensor((1 << (self.bits - 1)))
        return (input * Search_Pow2.apply(self.scale)) / quantized_range

    def _chain(self, input):
        return self.dequantize(self.round(self.quantize(self.clamp(input))))

    def _search(self, input):
        """The warm-up of the first call (:262-282, :307-328)."""
        with torch.no_grad():
            max_metrics = -1
            max_step = -5
            step = (torch.max(input)) / 100
            for i in range(1, 100):
                self.scale.data.copy_(torch.Tensor([step * i]))
                output = self._chain(input)
                cosine_similarity = torch.cosine_similarity(input.reshape(-1), output.reshape(-1), dim=0)
                if cosine_similarity > max_metrics:
                    max_metrics = cosine_similarity
                    max_step = i
                del output
            self.scale.data.copy_(torch.Tensor([step * max_step]))
            self.warmup.add_(-1)

    def forward(self, input):
        if self.bits == 32:
            return input
        assert self.bits != 1, 'binary quantisation is not supported'
        if not _torch_forced() and _tpsq().eligible(input, self.scale):
            if self._mirror is None:
                self._mirror = float(self.warmup)      # the one host read of this module
            if self._mirror:
                _tpsq().warmup_search(input, self.scale, self.warmup, self.bits)
                self._mirror += -1
            return _tpsq().fake_quant(input, self.scale, self.bits)
        self._mirror = None
        if self.warmup:
            self._search(input)
        return self._chain(input)

    def get_quantize_value(self, input):
        if self.bits == 32:
            return input
        assert self.bits != 1, 'binary quantisation is not supported'
        return self.clamp(self.round(self.quantize(input)))


class RangeTracker(nn.Module):
    def __init__(self):
        super().__init__()

    def update_range(self, min_val, max_val):
        raise NotImplementedError

    @torch.no_grad()
    def forward(self, input):
        min_val = torch.min(input)
        max_val = torch.max(input)
        self.update_range(min_val, max_val)


class GlobalRangeTracker(RangeTracker):
    def __init__(self):
        super().__init__()
        self.register_buffer('min_val', torch.zeros(1))
        self.register_buffer('max_val', torch.zeros(1))
        self.register_buffer('first_w', torch.zeros(1))

    def update_range(self, min_val, max_val):
        temp_minval = self.min_val      # aliases, not copies (:155-156): the add_(-temp) below zeroes them too
        temp_maxval = self.max_val
        if self.first_w == 0:
            self.first_w.add_(1)
            self.min_val.add_(min_val)
            self.max_val.add_(max_val)
        else:
            self.min_val.add_(-temp_minval).add_(torch.min(temp_minval, min_val))
            self.max_val.add_(-temp_maxval).add_(torch.max(temp_maxval, max_val))


class Bias_Quantizer(nn.Module):
    def __init__(self, bits, range_tracker):
        super().__init__()
        self.bits = bits
        self.range_tracker = range_tracker
        self.register_buffer('scale', torch.zeros(1))

    def update_params(self):
        min_val = torch.tensor(-(1 << (self.bits - 1)))
        max_val = torch.tensor((1 << (self.bits - 1)) - 1)
        quantized_range = torch.max(torch.abs(min_val), torch.abs(max_val))
        float_max = torch.max(torch.abs(self.range_tracker.min_val), torch.abs(self.range_tracker.max_val))
        floor_float_range = 2 ** float_max.log2().floor()
        ceil_float_range = 2 ** float_max.log2().ceil()
        if abs(ceil_float_range - float_max) < abs(floor_float_range - float_max):
            float_range = ceil_float_range
        else:
            float_range = floor_float_range
        self.scale = float_range / quantized_range

    def quantize(self, input):
        return input / self.scale

    def round(self, input):
        return Round.apply(input)

    def clamp(self, input):
        # (:198-202) with the bounds as numbers: torch.clamp refuses the reference's 0-d host tensors next to a GPU tensor
        return torch.clamp(input, -(1 << (self.bits - 1)), (1 << (self.bits - 1)) - 1)

    def dequantize(self, input):
        return (input) * self.scale

    def forward(self, input):
        if self.bits == 32:
            return input
        assert self.bits != 1, 'binary quantisation is not supported'
        from engine import qat
        if not _torch_forced() and qat.eligible(input) and self.scale.numel() == 1:
            if self.training == True:
                _tpsq().bias_observe_update(input, self)
            return _tpsq().bias_fake_quant(input, self)
        if self.training == True:
            self.range_tracker(input)
            self.update_params()
        return self.dequantize(self.clamp(self.round(self.quantize(input))))

    def get_quantize_value(self, input):
        if self.bits == 32:
            return input
        assert self.bits != 1, 'binary quantisation is not supported'
        return self.clamp(self.round(self.quantize(input)))

    def get_scale(self):
        return np.array(math.log2(self.scale)).reshape(1, -1)


class Weight_Quantizer(Quantizer):
    def __init__(self, bits, out_channels, warmup):
        super().__init__(bits, warmup)      # (:247) `warmup` lands in `out_channels`: the buffer starts at 0
        self.out_channels = out_channels
        if self.out_channels == -1:
            self.scale = Parameter(torch.Tensor(1))
        else:
            self.scale = Parameter(torch.Tensor(self.out_channels, 1, 1, 1))
        init.ones_(self.scale)


class Activattion_Quantizer(Quantizer):
    def __init__(self, bits, out_channels, warmup):
        super().__init__(bits, out_channels, warmup)
        self.out_channels = out_channels
        if self.out_channels == -1:
            self.scale = Parameter(torch.Tensor(1))
        else:
            self.scale = Parameter(torch.Tensor(1, self.out_channels, 1, 1))
        init.ones_(self.scale)


# ---------------------------------------------------------------------------------------------- BN-folding quantised conv
class TPSQ_BNFold_QuantizedConv2d_For_FPGA(_Mirrored, nn.Conv2d):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False, eps=1e-5,
                 momentum=0.01, a_bits=8, w_bits=8, bn=0, activate='leaky', steps=0, quantizer_output=False, maxabsscaler=False,
                 warmup=True):
        super().__init__(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                         padding=padding, dilation=dilation, groups=groups, bias=bias)
        self.bn = bn
        self.activate = activate
        self.eps = eps
        self.momentum = momentum
        self.freeze_step = int(steps * 0.9)
        self.gamma = Parameter(torch.Tensor(out_channels))
        self.beta = Parameter(torch.Tensor(out_channels))
        for name_ in ('running_mean', 'running_var', 'batch_mean', 'batch_var'):
            self.register_buffer(name_, torch.zeros(out_channels))
        self.register_buffer('first_bn', torch.zeros(1))
        self.register_buffer('step', torch.zeros(1))
        self.quantizer_output = quantizer_output
        self.maxabsscaler = maxabsscaler
        init.normal_(self.gamma, 1, 0.5)
        init.zeros_(self.beta)

        self.activation_quantizer = Activattion_Quantizer(bits=a_bits, out_channels=-1, warmup=warmup)
        self.weight_quantizer = Weight_Quantizer(bits=w_bits, out_channels=-1, warmup=warmup)
        self.bias_quantizer = Bias_Quantizer(bits=w_bits, range_tracker=GlobalRangeTracker())

    def _decisions(self, input):
        """(fold with batch statistics?, first BatchNorm update?) of this training call, and the step counter's advance.

        Host tensors: the reference's tensor comparisons (:424-425, :433).  The fused path: host mirrors, read once."""
        if not _torch_forced() and _tpsq().eligible(input, self.step):
            if self._mirror is None:
                flags = torch.cat([self.step.reshape(1), self.first_bn.reshape(1), (self.running_mean == 0).all().reshape(1).float(),
                                   (self.running_var == 0).all().reshape(1).float()]).tolist()      # the one host read of this module
                self._mirror = [flags[0], flags[1] == 0 and flags[2] != 0 and flags[3] != 0]
            self.step += 1
            self._mirror[0] += 1
            first = self._mirror[1]
            # once the running statistics hold a batch's they are never all zero again (and first_bn is 1 after the first rule)
            self._mirror[1] = False
            return self._mirror[0] < self.freeze_step, first
        self._mirror = None
        self.step += 1
        if not self.bn:
            return None, None
        first = bool(self.first_bn == 0 and torch.equal(self.running_mean, torch.zeros_like(self.running_mean))
                     and torch.equal(self.running_var, torch.zeros_like(self.running_var)))
        return bool(self.step < self.freeze_step), first

    def _fold(self, mean, var):
        """BatchNorm folded into weight and bias with the given statistics (:433-454)."""
        if self.bias is not None:
            bias = reshape_to_bias(self.beta + (self.bias - mean) * (self.gamma / torch.sqrt(var + self.eps)))
        else:
            bias = reshape_to_bias(self.beta - mean * (self.gamma / torch.sqrt(var + self.eps)))
        weight = self.weight * reshape_to_weight(self.gamma / torch.sqrt(var + self.eps))
        return weight, bias

    def forward(self, input):
        _no_fpga_dump(self.quantizer_output)
        if self.training:
            batch_fold, first = self._decisions(input)
            if self.bn:
                output = F.conv2d(input=input, weight=self.weight, bias=self.bias, stride=self.stride, padding=self.padding,
                                  dilation=self.dilation, groups=self.groups)
                dims = [dim for dim in range(4) if dim != 1]
                self.batch_mean = torch.mean(output, dim=dims)
                self.batch_var = torch.var(output, dim=dims)
                with torch.no_grad():
                    if first:
                        self.first_bn.add_(1)
                        self.running_mean.add_(self.batch_mean)
                        self.running_var.add_(self.batch_var)
                    else:
                        self.running_mean.mul_(1 - self.momentum).add_(self.batch_mean * self.momentum)
                        self.running_var.mul_(1 - self.momentum).add_(self.batch_var * self.momentum)
                if batch_fold:
                    weight, bias = self._fold(self.batch_mean, self.batch_var)
                else:
                    weight, bias = self._fold(self.running_mean, self.running_var)
            else:
                bias = self.bias
                weight = self.weight
        else:
            weight, bias = self.BN_fuse()
        q_weight = self.weight_quantizer(weight)
        q_bias = self.bias_quantizer(bias)
        output = F.conv2d(input=input, weight=q_weight, bias=q_bias, stride=self.stride, padding=self.padding,
                          dilation=self.dilation, groups=self.groups)
        if self.activate == 'leaky':
            output = F.leaky_relu(output, 0.1 if not self.maxabsscaler else 0.25, inplace=True)
        elif self.activate == 'relu6':
            output = F.relu6(output, inplace=True)
        elif self.activate == 'h_swish':
            output = output * (F.relu6(output + 3.0, inplace=True) / 6.0)
        elif self.activate == 'relu':
            output = F.relu(output, inplace=True)
        elif self.activate == 'mish':
            output = output * F.softplus(output).tanh()
        elif self.activate == 'linear':
            pass
        else:
            print(self.activate + "%s is not supported !")
        return self.activation_quantizer(output)

    def BN_fuse(self):
        if self.bn:
            if self.bias is not None:
                bias = reshape_to_bias(self.beta + (self.bias - self.running_mean) * (
                    self.gamma / torch.sqrt(self.running_var + self.eps)))
            else:      # (:467-469, :581-583: multiplies before it divides, unlike the training branch)
                bias = reshape_to_bias(self.beta - self.running_mean * self.gamma / torch.sqrt(self.running_var + self.eps))
            weight = self.weight * reshape_to_weight(self.gamma / torch.sqrt(self.running_var + self.eps))
        else:
            bias = self.bias
            weight = self.weight
        return weight, bias
