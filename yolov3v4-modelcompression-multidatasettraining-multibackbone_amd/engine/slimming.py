"""Network slimming (Liu et al., "Learning Efficient Convolutional Networks through Network Slimming", ICCV 2017) on darknet cfg graphs: which BatchNorm layers take part.

Sparse training puts an L1 penalty on BatchNorm gammas, the prune step cuts the channels whose |gamma| falls under a global
threshold.  Which layers may be touched depends on how their output is consumed - a channel can only disappear where every
consumer can drop the matching input.  The three policies of ``train.py --prune 0 / 1 / 2`` (reference train.py:237-262 picks them
from ``utils/prune_utils.py``; this module states them natively, so neither sparse training nor ``tools/slim_prune.py`` needs a
checkout of the reference):

    0  regular        conv + BN blocks whose output feeds nothing but the next layer: layers joined by a shortcut keep their width
    1  shortcut-aware the same, but shortcut operands take part (the prune step later merges their masks per shortcut chain)
    2  layer prune    only the conv in front of each shortcut: its gammas rank whole residual blocks

Never pruned in modes 0 and 1: the conv in front of an SPP block (max-pool followed by a route), in front of a group-split route, in
front of a depthwise conv (the depthwise filter count is tied to it), and in front of an upsample.

All functions take ``Darknet.module_defs`` (the blocks after ``[net]``) and return cfg block indices.
"""
import collections

import torch

LayerSets = collections.namedtuple('LayerSets', 'bn_convs other prune shortcut_source shortcut_members')
LayerSets.__doc__ = """bn_convs: conv blocks with BatchNorm; other: the blocks with weights that are copied, never pruned (convs
without BatchNorm; modes 0 / 1 also depthwise and squeeze-excite blocks); prune: the blocks under the penalty / the threshold;
shortcut_source (mode 1): {block in front of a shortcut: the block that produced the shortcut's other operand}; shortcut_members
(mode 1): every block on either side of some shortcut."""


def _kind(defs, i):
    return defs[i]['type']


def _shortcut_source(defs, i):
    """The block whose BatchNorm output is the `from` operand of shortcut ``i``: the conv itself, or - when the operand is another
    shortcut's sum - the conv in front of that shortcut.  None for any other producer."""
    src = i + int(defs[i]['from'][0])
    if _kind(defs, src) == 'convolutional':
        return src
    if _kind(defs, src) == 'shortcut':
        return src - 1
    return None


def layer_sets(module_defs, mode):
    """The layer sets of prune mode 0, 1 or 2 as a ``LayerSets``."""
    defs = module_defs
    if mode not in (0, 1, 2):
        raise ValueError('--prune must be 0, 1 or 2')
    bn_convs, other, keep = [], [], set()
    source, members, before_shortcut = {}, set(), []
    for i, d in enumerate(defs):
        kind = d['type']
        if kind == 'convolutional':
            (bn_convs if d['batch_normalize'] else other).append(i)
            if mode == 2:
                continue
            follower = _kind(defs, i + 1)
            if follower == 'maxpool' and _kind(defs, i + 2) == 'route':      # entry of an SPP block (a tiny net's pool is not followed by a route)
                keep.add(i)
            if follower == 'route' and 'groups' in defs[i + 1]:              # CSP group split
                keep.add(i)
        elif mode == 2:
            if kind == 'shortcut':
                before_shortcut.append(i - 1)
        elif kind == 'depthwise':
            other.append(i)
            keep.add(i - 1)
        elif kind == 'se':
            other.append(i)
        elif kind == 'upsample':
            keep.add(i - 1)
        elif kind == 'shortcut':
            src = _shortcut_source(defs, i)
            if mode == 0:
                keep.add(i - 1)
                if src is not None:
                    keep.add(src)
            else:
                if src is not None:
                    source[i - 1] = src
                    members.add(src)
                members.add(i - 1)
    if mode == 2:
        return LayerSets(bn_convs, other, before_shortcut, {}, set())
    prune = [i for i in bn_convs if i not in keep]
    return LayerSets(bn_convs, other, prune, source, members)


def sparsity_blocks(module_defs, mode):
    """The blocks whose BatchNorm gamma carries the L1 penalty during ``train.py --prune mode``."""
    return layer_sets(module_defs, mode).prune


def bn_of(block):
    """The BatchNorm2d of a conv / depthwise block (``nn.Sequential(conv, bn, activation)``)."""
    for child in list(block.children())[1:]:
        if isinstance(child, torch.nn.modules.batchnorm.BatchNorm2d):
            return child
    raise ValueError('block has no BatchNorm2d')


def gather_bn_weights(module_list, blocks):
    """|gamma| of the listed blocks as one 1-D tensor (block order), on the parameters' device."""
    parts = [bn_of(module_list[i]).weight.detach().abs().reshape(-1) for i in blocks]
    return torch.cat(parts) if parts else torch.zeros(0)


def apply_bn_l1_(module_list, blocks, s):
    """``grad += s * sign(gamma)`` on the listed blocks in torch - the CPU form of the term the HIP step adds inside its backward
    (csrc/sparsity.hip); same formula, same bits."""
    for i in blocks:
        bn = bn_of(module_list[i])
        if bn.weight.grad is not None:
            bn.weight.grad.add_(s * torch.sign(bn.weight.detach()))
