"""Quantization-aware training with BatchNorm folding and power-of-two scales (``--quantized 1``).

Fresh, condensed implementation of the module family the reference keeps in ``utils/quantized/quantized_google.py`` (same class
names, constructor signatures, buffers and ``state_dict`` keys, so checkpoints move in both directions with ``strict=True``):

* ``GlobalRangeTracker`` / ``AveragedRangeTracker`` (reference :35-77) - the float range a quantiser sees.  The global tracker's
  ``update_range`` reads its own buffer through an alias (:47-55), so after the first call it tracks ``min(0, current min)`` and
  ``max(0, current max)``, not a running extreme; kept.
* ``SymmetricQuantizer`` / ``AsymmetricQuantizer`` (:95-219) - ``scale`` is the power of two nearest to the tracked range (absolute
  distance, ties to the lower one) over the integer range (128 for signed symmetric, not 127); ranges move only while the
  quantiser's own ``step < Scale_freeze_step``; ``step`` advances on every call, in eval too; ``steps == 0`` never calibrates.
* ``BNFold_QuantizedConv2d_For_FPGA`` (:235-836) - conv, batch statistics (``torch.var``, unbiased, also for ``running_var``;
  momentum 0.01), fold with batch statistics while ``step < BN_freeze_step`` and running statistics after, fake-quantised weight,
  bias and output.
* ``QuantizedShortcut_max`` / ``_min`` (:839-1302) and ``QuantizedFeatureConcat`` (:1305-1479) - the re-scaling data movement.

Host tensors run the reference's arithmetic operation for operation.  Dense fp32 GPU tensors run the same arithmetic as fused HIP
passes (``engine/qat.py`` -> ``csrc/qat.hip``): one min/max pass, one one-wave range / scale update, one fake-quant forward and one
backward kernel per quantiser call, with ``scale``, ``zero_point``, ``first_a`` / ``first_w`` and ``step`` read and written on the
device.  The Python-side decisions (``step < freeze``, the ``first_bn`` rule) use host mirrors, initialised by one read per module
after construction or ``load_state_dict``; a training step reads nothing back.  ``YOLO_QAT_TORCH=1`` forces the torch formulas on
GPU tensors too (the reference's eager arithmetic with its host reads).  fp16 tensors (autocast) and per-channel quantisers always
take the torch formulas.  The scale choice of the shortcut and concat modules combines several trackers with Python ``max`` /
``min`` and stays as tiny torch ops with their host reads; their min/max passes and fake-quant chains use the kernels.

The reference's text / binary dumps for its FPGA flow (``quantizer_output=True``) are not part of this package.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.nn import init
from torch.nn.parameter import Parameter


def _qat():
    from engine import qat
    return qat


def _fused(*tensors):
    """True when every tensor takes the HIP passes: dense-able fp32 on a GPU, and the torch formulas are not forced."""
    if os.environ.get('YOLO_QAT_TORCH', '0') == '1':
        return False
    qat = _qat()
    return all(qat.eligible(t) for t in tensors)


def _no_fpga_dump(flag):
    if flag:
        raise NotImplementedError('quantizer_output: the FPGA text / binary dumps are not part of this package')


def _int_limits(bits, sign=True):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)


def _limits(bits, sign=True):
    """Integer range as the 0-d tensors the reference builds (:124-129, :180-184)."""
    lo, hi = _int_limits(bits, sign)
    return torch.tensor(lo), torch.tensor(hi)


def _clamp(input, bits, sign=True):
    """(:123-131) with the bounds as numbers: the reference's 0-d host tensors give the same values and the same gradient mask, but
    ``torch.clamp`` refuses them next to a GPU tensor."""
    lo, hi = _int_limits(bits, sign)
    return torch.clamp(input, lo, hi)


def _nearest_pow2(float_range):
    """The power of two nearest to ``float_range`` in absolute distance, the lower one on a tie (:189-194, :212-217)."""
    floor_float_range = 2 ** float_range.log2().floor()
    ceil_float_range = 2 ** float_range.log2().ceil()
    if abs(ceil_float_range - float_range) < abs(floor_float_range - float_range):
        return ceil_float_range
    return floor_float_range


def _symmetric_scale(float_min_val, float_max_val, bits):
    """Scale of the shortcut / concat modules from one range (:908-919)."""
    lo, hi = _limits(bits)
    quantized_range = torch.max(torch.abs(lo), torch.abs(hi))
    float_max = torch.max(torch.abs(float_min_val), torch.abs(float_max_val))
    return _nearest_pow2(float_max) / quantized_range


class _Mirrored:
    """Host mirrors of device-resident decision buffers: dropped whenever the buffers may have changed behind them."""
    _mirror = None

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._mirror = None


# ---------------------------------------------------------------------------------------------- range trackers
class RangeTracker(nn.Module):
    def __init__(self, q_level):
        super().__init__()
        self.q_level = q_level

    def update_range(self, min_val, max_val):
        raise NotImplementedError

    @torch.no_grad()
    def forward(self, input):
        if self.q_level == 'L' and _fused(input):
            _qat().observe_update(input, self)
            return
        if self.q_level == 'L':
            min_val = torch.min(input)
            max_val = torch.max(input)
        elif self.q_level == 'C':
            min_val = torch.min(torch.min(torch.min(input, 3, keepdim=True)[0], 2, keepdim=True)[0], 1, keepdim=True)[0]
            max_val = torch.max(torch.max(torch.max(input, 3, keepdim=True)[0], 2, keepdim=True)[0], 1, keepdim=True)[0]
        self.update_range(min_val, max_val)


def _range_buffers(module, out_channels):
    shape = (1,) if module.q_level == 'L' else (out_channels, 1, 1, 1)
    module.register_buffer('min_val', torch.zeros(shape))
    module.register_buffer('max_val', torch.zeros(shape))


class GlobalRangeTracker(RangeTracker):
    def __init__(self, q_level, out_channels):
        super().__init__(q_level)
        _range_buffers(self, out_channels)
        self.register_buffer('first_w', torch.zeros(1))

    def update_range(self, min_val, max_val):
        temp_minval = self.min_val      # aliases, not copies (:47-48): the add_(-temp) below zeroes them too
        temp_maxval = self.max_val
        if self.first_w == 0:
            self.first_w.add_(1)
            self.min_val.add_(min_val)
            self.max_val.add_(max_val)
        else:
            self.min_val.add_(-temp_minval).add_(torch.min(temp_minval, min_val))
            self.max_val.add_(-temp_maxval).add_(torch.max(temp_maxval, max_val))


class AveragedRangeTracker(RangeTracker):
    def __init__(self, q_level, out_channels, momentum=0.1):
        super().__init__(q_level)
        self.momentum = momentum
        _range_buffers(self, out_channels)
        self.register_buffer('first_a', torch.zeros(1))

    def update_range(self, min_val, max_val):
        if self.first_a == 0:
            self.first_a.add_(1)
            self.min_val.add_(min_val)
            self.max_val.add_(max_val)
        else:
            self.min_val.mul_(1 - self.momentum).add_(min_val * self.momentum)
            self.max_val.mul_(1 - self.momentum).add_(max_val * self.momentum)


# ---------------------------------------------------------------------------------------------- quantisers
class Round(Function):
    """Round half away from zero, straight-through gradient (:81-92)."""

    @staticmethod
    def forward(self, input):
        return torch.sign(input) * torch.floor(torch.abs(input) + 0.5)

    @staticmethod
    def backward(self, grad_output):
        return grad_output.clone()


class Quantizer(_Mirrored, nn.Module):
    asymmetric = False

    def __init__(self, bits, range_tracker, out_channels, Scale_freeze_step, sign=True):
        super().__init__()
        self.bits = bits
        self.range_tracker = range_tracker
        self.register_buffer('step', torch.zeros(1))
        self.Scale_freeze_step = Scale_freeze_step
        self.sign = sign
        shape = (1,) if out_channels == -1 else (out_channels, 1, 1, 1)
        self.register_buffer('scale', torch.zeros(shape))
        self.register_buffer('zero_point', torch.zeros(shape))

    def update_params(self):
        raise NotImplementedError

    def quantize(self, input):
        return input / self.scale + self.zero_point

    def round(self, input):
        return Round.apply(input)

    def clamp(self, input):
        return _clamp(input, self.bits, self.sign)

    def dequantize(self, input):
        return (input - self.zero_point) * self.scale

    def _per_tensor(self):
        return self.scale.numel() == 1 and self.range_tracker.q_level == 'L'

    def forward(self, input):
        if self.bits == 32:
            return input
        assert self.bits != 1, 'binary quantisation is not supported'
        if self._per_tensor() and _fused(input):
            if self._mirror is None:
                self._mirror = float(self.step)      # the one host read of this module
            if self.training and self._mirror < self.Scale_freeze_step:
                _qat().observe_update(input, self.range_tracker, self)
            self._mirror += 1
            return _qat().fake_quant(input, self.scale, self.zero_point, self.bits, self.sign, True, step=self.step)
        self._mirror = None
        if self.training == True and self.step < self.Scale_freeze_step:
            self.range_tracker(input)
            self.update_params()
        output = self.quantize(input)
        output = self.round(output)
        output = self.clamp(output)
        output = self.dequantize(output)
        self.step += 1
        return output

    def get_quantize_value(self, input):
        if self.bits == 32:
            return input
        assert self.bits != 1, 'binary quantisation is not supported'
        return self.clamp(self.round(self.quantize(input)))

    def get_scale(self):
        import math
        import numpy as np
        return np.array(math.log2(self.scale)).reshape(1, -1)


class SymmetricQuantizer(Quantizer):
    def update_params(self):
        min_val, max_val = _limits(self.bits, self.sign)
        quantized_range = torch.max(torch.abs(min_val), torch.abs(max_val))
        float_max = torch.max(torch.abs(self.range_tracker.min_val), torch.abs(self.range_tracker.max_val))
        self.scale = _nearest_pow2(float_max) / quantized_range
        self.zero_point = torch.zeros_like(self.scale)


class AsymmetricQuantizer(Quantizer):
    asymmetric = True

    def update_params(self):
        min_val, max_val = _limits(self.bits, self.sign)
        quantized_range = max_val - min_val
        float_range = self.range_tracker.max_val - self.range_tracker.min_val
        self.scale = _nearest_pow2(float_range) / quantized_range
        self.zero_point = torch.round(max_val - self.range_tracker.max_val / self.scale)


def reshape_to_activation(input):
    return input.reshape(1, -1, 1, 1)


def reshape_to_weight(input):
    return input.reshape(-1, 1, 1, 1)


def reshape_to_bias(input):
    return input.reshape(-1)


# ---------------------------------------------------------------------------------------------- BN-folding quantised conv
class BNFold_QuantizedConv2d_For_FPGA(_Mirrored, nn.Conv2d):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False, eps=1e-5,
                 momentum=0.01, a_bits=8, w_bits=8, q_type=0, bn=0, activate='leaky', steps=0, quantizer_output=False,
                 reorder=False, TM=32, TN=32, name='', layer_idx=-1, maxabsscaler=False):
        super().__init__(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                         padding=padding, dilation=dilation, groups=groups, bias=bias)
        self.bn = bn
        self.activate = activate
        self.eps = eps
        self.momentum = momentum
        self.BN_freeze_step = int(steps * 0.9)
        self.Scale_freeze_step = int(steps * 0.1)
        self.gamma = Parameter(torch.Tensor(out_channels))
        self.beta = Parameter(torch.Tensor(out_channels))
        for name_ in ('running_mean', 'running_var', 'batch_mean', 'batch_var'):
            self.register_buffer(name_, torch.zeros(out_channels))
        self.register_buffer('first_bn', torch.zeros(1))
        self.register_buffer('step', torch.zeros(1))
        self.quantizer_output = quantizer_output
        self.reorder, self.TM, self.TN = reorder, TM, TN
        self.name, self.layer_idx = name, layer_idx
        self.w_bits, self.a_bits = w_bits, a_bits
        self.maxabsscaler = maxabsscaler
        init.normal_(self.gamma, 1, 0.5)
        init.zeros_(self.beta)

        cls, sign = (SymmetricQuantizer, True) if q_type == 0 else (AsymmetricQuantizer, False)
        make = lambda bits, tracker: cls(bits=bits, range_tracker=tracker(q_level='L', out_channels=-1), out_channels=-1,
                                         Scale_freeze_step=self.Scale_freeze_step, sign=sign)
        self.activation_quantizer = make(a_bits, AveragedRangeTracker)
        self.weight_quantizer = make(w_bits, GlobalRangeTracker)
        self.bias_quantizer = make(w_bits, GlobalRangeTracker)

    def _decisions(self, input):
        """(fold with batch statistics?, first BatchNorm update?) of this training call, and the step counter's advance.

        Host tensors: the reference's tensor comparisons (:340-341, :349).  The fused path: host mirrors, read once."""
        if _fused(input):
            if self._mirror is None:
                flags = torch.cat([self.step.reshape(1), self.first_bn.reshape(1), (self.running_mean == 0).all().reshape(1).float(),
                                   (self.running_var == 0).all().reshape(1).float()]).tolist()      # the one host read of this module
                self._mirror = [flags[0], flags[1] == 0 and flags[2] != 0 and flags[3] != 0]
            self.step += 1
            self._mirror[0] += 1
            first = self._mirror[1]
            # once the running statistics hold a batch's they are never all zero again (and first_bn is 1 after the first rule)
            self._mirror[1] = False
            return self._mirror[0] < self.BN_freeze_step, first
        self._mirror = None
        self.step += 1
        if not self.bn:
            return None, None
        first = bool(self.first_bn == 0 and torch.equal(self.running_mean, torch.zeros_like(self.running_mean))
                     and torch.equal(self.running_var, torch.zeros_like(self.running_var)))
        return bool(self.step < self.BN_freeze_step), first

    def _fold(self, mean, var):
        """BatchNorm folded into weight and bias with the given statistics (:349-370)."""
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
            else:      # (:383-385: multiplies before it divides, unlike the training branch)
                bias = reshape_to_bias(self.beta - self.running_mean * self.gamma / torch.sqrt(self.running_var + self.eps))
            weight = self.weight * reshape_to_weight(self.gamma / torch.sqrt(self.running_var + self.eps))
        else:
            bias = self.bias
            weight = self.weight
        return weight, bias


# ---------------------------------------------------------------------------------------------- shortcuts and concat
class _QuantizedShortcut(nn.Module):
    def __init__(self, layers, weight=False, bits=8, quantizer_output=False, reorder=False, TM=32, TN=32, name='', layer_idx=-1):
        super().__init__()
        self.layers = layers
        self.weight = weight
        self.n = len(layers) + 1
        self.bits = bits
        self.range_tracker_x = AveragedRangeTracker(q_level='L', out_channels=-1)
        self.range_tracker_a = AveragedRangeTracker(q_level='L', out_channels=-1)
        self.range_tracker_sum = AveragedRangeTracker(q_level='L', out_channels=-1)
        self._scale_buffers()
        self.quantizer_output = quantizer_output
        self.reorder, self.TM, self.TN, self.name, self.layer_idx = reorder, TM, TN, name, layer_idx
        if weight:
            self.w = nn.Parameter(torch.zeros(self.n), requires_grad=True)

    def round(self, input):
        return Round.apply(input)

    def clamp(self, input):
        return _clamp(input, self.bits)

    def _fake_quant(self, t, scale, clamp, fused):
        """quantize, round, (clamp,) dequantize with ``scale`` - one HIP pass on the fused path."""
        if fused:
            return _qat().fake_quant(t, scale, None, self.bits, True, clamp)
        t = self.round(t / scale)
        if clamp:
            t = self.clamp(t)
        return t * scale

    @staticmethod
    def _add(x, a):
        nx, na = x.shape[1], a.shape[1]
        if nx == na:
            x = x + a
        elif nx > na:
            x[:, :na] = x[:, :na] + a
        else:
            x = x + a[:, :nx]
        return x

    def forward(self, x, outputs):
        _no_fpga_dump(self.quantizer_output)
        if self.weight:
            w = torch.sigmoid(self.w) * (2 / self.n)
            x = x * w[0]
        for i in range(self.n - 1):
            a = outputs[self.layers[i]] * w[i + 1] if self.weight else outputs[self.layers[i]]
            x = self._merge(x, a, _fused(x, a))
        return x


class QuantizedShortcut_max(_QuantizedShortcut):
    def _scale_buffers(self):
        self.register_buffer('scale', torch.zeros(1))

    def quantize(self, input):
        return input / self.scale

    def dequantize(self, input):
        return input * self.scale

    def _merge(self, x, a, fused):
        nx, na = x.shape[1], a.shape[1]
        if self.training == True:
            self.range_tracker_a(x)      # (:896-897: x feeds tracker a, a feeds tracker x)
            self.range_tracker_x(a)
            if nx == na:
                self.range_tracker_sum(x + a)
            elif nx > na:
                self.range_tracker_sum(x[:, :na] + a)
            else:
                self.range_tracker_sum(x + a[:, :nx])
            float_max_val = max(self.range_tracker_sum.max_val, self.range_tracker_x.max_val, self.range_tracker_a.max_val)
            float_min_val = min(self.range_tracker_sum.min_val, self.range_tracker_x.min_val, self.range_tracker_a.min_val)
            self.scale = _symmetric_scale(float_min_val, float_max_val, self.bits)
        x = self._fake_quant(x, self.scale, True, fused)
        a = self._fake_quant(a, self.scale, True, fused)
        return self._fake_quant(self._add(x, a), self.scale, True, fused)


class QuantizedShortcut_min(_QuantizedShortcut):
    def _scale_buffers(self):
        self.register_buffer('input_scale', torch.zeros(1))
        self.register_buffer('scale', torch.zeros(1))

    def quantize(self, input, featrure_in=False):
        return input / (self.input_scale if featrure_in else self.scale)

    def dequantize(self, input, featrure_in=False):
        return input * (self.input_scale if featrure_in else self.scale)

    def _merge(self, x, a, fused):
        if self.training == True:
            self.range_tracker_a(a)
            self.range_tracker_x(x)
            float_max_val = min(self.range_tracker_x.max_val, self.range_tracker_a.max_val)
            float_min_val = max(self.range_tracker_x.min_val, self.range_tracker_a.min_val)
            self.input_scale = _symmetric_scale(float_min_val, float_max_val, self.bits)
        x = self._fake_quant(x, self.input_scale, False, fused)      # (:1148-1155: no clamp on the inputs)
        a = self._fake_quant(a, self.input_scale, False, fused)
        x = self._add(x, a)
        if self.training == True:
            self.range_tracker_sum(x)
            self.scale = _symmetric_scale(self.range_tracker_sum.min_val, self.range_tracker_sum.max_val, self.bits)
        return self._fake_quant(x, self.scale, True, fused)


class QuantizedFeatureConcat(nn.Module):
    def __init__(self, layers, groups, bits=8, quantizer_output=False, reorder=False, TM=32, TN=32, name='', layer_idx=-1):
        super().__init__()
        self.layers = layers
        self.groups = groups
        self.multiple = len(layers) > 1
        self.register_buffer('scale', torch.zeros(1))
        self.register_buffer('float_max_list', torch.zeros(len(layers)))
        self.bits = bits
        self.momentum = 0.1
        self.quantizer_output = quantizer_output
        self.reorder, self.TM, self.TN, self.name, self.layer_idx = reorder, TM, TN, name, layer_idx

    def quantize(self, input):
        return input / self.scale

    def round(self, input):
        return Round.apply(input)

    def clamp(self, input):
        return _clamp(input, self.bits)

    def dequantize(self, input):
        return input * self.scale

    def forward(self, x, outputs):
        if not self.multiple:
            if self.groups:
                return x[:, (x.shape[1] // 2):]
            return outputs[self.layers[0]]
        _no_fpga_dump(self.quantizer_output)
        fused = _fused(*[outputs[i] for i in self.layers])
        if self.training == True:
            lo, hi = _limits(self.bits)
            quantized_range = torch.max(torch.abs(lo), torch.abs(hi))
            for j, i in enumerate(self.layers):
                temp = outputs[i].detach()
                if fused:
                    mm = _qat().observe(temp)
                    float_max = torch.max(mm[1], torch.abs(mm[0]))
                else:
                    float_max = torch.max(torch.max(temp), torch.abs(torch.min(temp)))
                if self.float_max_list[j] == 0:      # per entry (:1353-1358)
                    self.float_max_list[j].add_(float_max)
                else:
                    self.float_max_list[j].mul_(1 - self.momentum).add_(float_max * self.momentum)
            float_max = max(self.float_max_list).unsqueeze(0)
            self.scale = _nearest_pow2(float_max) / quantized_range
        for i in self.layers:      # the fake-quantised tensors replace the routed ones (:1469-1474)
            if fused:
                outputs[i] = _qat().fake_quant(outputs[i], self.scale, None, self.bits, True, True)
            else:
                outputs[i] = self.dequantize(self.clamp(self.round(self.quantize(outputs[i]))))
        return torch.cat([outputs[i] for i in self.layers], 1)
