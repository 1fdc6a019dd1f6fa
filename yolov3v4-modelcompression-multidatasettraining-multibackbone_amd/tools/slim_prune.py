"""Network slimming, stage two: cut the channels of a sparsity-trained model whose BatchNorm |gamma| falls under a global
threshold and write the compact cfg + darknet weights (the reference's ``slim_prune.py``; same options, same output names, same
compact model).  Runs on this package alone - no checkout of the reference is needed.

    python tools/slim_prune.py --cfg cfg/yolov3/yolov3.cfg --data data/coco.data --weights weights/last.pt --percent 0.8

Steps (``slim_prune`` below): the shortcut-aware layer set (engine/slimming.py mode 1) -> sorted |gamma| of the set -> threshold at
``percent`` -> per-layer masks with a floor of ``layer_keep`` of the channels -> masks merged over every shortcut chain (tensors that
are added keep ONE channel set: the union) -> the pruned channels' constant output act(beta) is folded into whatever consumes it
(next BatchNorm's running_mean, or the bias of a conv without BatchNorm) -> compact cfg -> weights gathered into the compact
``Darknet`` -> ``.weights``.  All tensor work stays on the model's device in torch (it runs once: no kernel to write); the
before / after evaluations (``test.test``; skipped by ``--no-eval``) run on the HIP engine when the device is a GPU.

Outputs for ``cfg/<family>/<net>.cfg`` at percent P (the reference's names, ``tools/pruned_finetune.py`` reads them):
``cfg/slim_prune_P<family>/slim_prune_P<net>.cfg`` and ``weights/slim_prune_P<family>/slim_prune_P_percent.weights``.

One deliberate difference from the reference: a pruned leaky-ReLU channel's constant is leaky(beta) with the layer's own slope (the
reference hard-codes 0.1, which is wrong for ``--maxabsscaler`` graphs; equal everywhere else).
"""
import argparse
import copy
import os
import sys

import torch
import torch.nn.functional as F

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from engine.slimming import bn_of, gather_bn_weights, layer_sets  # noqa: E402


# ----------------------------------------------------------------------------------------------- masks
def global_threshold(model, prune, percent):
    ranked = torch.sort(gather_bn_weights(model.module_list, prune))[0]
    return ranked[int(len(ranked) * percent)]


def channel_masks(model, sets, thresh, layer_keep):
    """{conv+BN block: 0/1 float mask of the channels that stay}: |gamma| > thresh on the prunable blocks, but never fewer than
    ``layer_keep`` of a layer's channels (at least one) - the largest gammas fill up; all ones elsewhere."""
    prunable = set(sets.prune)
    masks = {}
    for i in sets.bn_convs:
        mag = bn_of(model.module_list[i]).weight.detach().abs()
        if i not in prunable:
            masks[i] = torch.ones_like(mag)
            continue
        floor = max(int(mag.numel() * layer_keep), 1)
        mask = (mag > thresh).to(mag.dtype)
        if int(mask.sum()) < floor:
            mask[torch.sort(mag, descending=True)[1][:floor]] = 1.0
        masks[i] = mask
    return masks


def merge_shortcut_masks(defs, masks):
    """Tensors joined by a shortcut must keep the same channels.  A chain is a shortcut, the conv in front of it, and whatever its
    `from` points at - a conv, or another shortcut whose chain continues.  Every conv + BN on a chain gets the union of their masks."""
    is_bn_conv = lambda j: defs[j]['type'] == 'convolutional' and int(defs[j]['batch_normalize'])
    seen = set()
    for i in range(len(defs) - 1, -1, -1):
        if defs[i]['type'] != 'shortcut' or i in seen:
            continue
        chain, j = [], i
        while defs[j]['type'] == 'shortcut':
            seen.add(j)
            if is_bn_conv(j - 1):
                chain.append(j - 1)
            j += int(defs[j]['from'][0])
        if is_bn_conv(j):
            chain.append(j)
        if not chain:
            raise NotImplementedError('shortcut %d joins no conv + BatchNorm block' % i)
        union = (torch.stack([masks[k] for k in chain]).sum(0) > 0).to(masks[chain[0]].dtype)
        for k in chain:
            masks[k] = union
    return masks


# ----------------------------------------------------------------------------------------------- pruned channels' constants
def _act_of(block):
    act = getattr(block, 'activation', None)
    name = act.__class__.__name__ if act is not None else ''
    if name == 'LeakyReLU':
        return lambda x: F.leaky_relu(x, act.negative_slope)
    if name == 'ReLU6':
        return F.relu6
    if name == 'HardSwish':
        return lambda x: x * (F.relu6(x + 3.0) / 6.0)
    if name == 'ReLU':
        return F.relu
    if name == 'Mish':
        return lambda x: x * F.softplus(x).tanh()
    return lambda x: x


def fold_pruned_constants(model, sets, masks):
    """A pruned channel (gamma := 0) still outputs the constant act(beta).  Return a copy of ``model`` in which that constant has moved
    into the consumers: for a conv reading the tensor, W summed over its taps times the constant vector is subtracted from its
    BatchNorm's running_mean (or added to its bias when it has no BatchNorm), and gamma / beta of the pruned channels are zero.  The
    constant travels with the tensor through shortcuts (sum), routes (concat / second half of a group split), upsample and max-pool;
    depthwise and squeeze-excite blocks only ever read unpruned tensors (the conv in front of a depthwise block is never prunable)
    and emit no constant."""
    loose = copy.deepcopy(model)
    defs, prunable, with_bn = model.module_defs, set(sets.prune), set(sets.bn_convs)
    const = []          # per block: the constant per output channel (zeros where nothing was pruned), None for yolo

    def consume(j, c):
        """Block j reads a tensor carrying constant c."""
        if j >= len(defs) or defs[j]['type'] != 'convolutional' or c is None:
            return
        conv = loose.module_list[j][0]
        shift = conv.weight.detach().sum(dim=(2, 3)).matmul(c.reshape(-1, 1)).reshape(-1)
        if j in with_bn:
            bn_of(loose.module_list[j]).running_mean.sub_(shift)
        else:
            conv.bias.data.add_(shift)

    with torch.no_grad():
        for i, d in enumerate(defs):
            kind = d['type']
            if kind in ('convolutional', 'depthwise', 'se'):
                if kind == 'convolutional':
                    width = loose.module_list[i][0].out_channels
                else:
                    width = const[i - 1].numel()
                ref = next(loose.parameters())
                c = torch.zeros(width, dtype=ref.dtype, device=ref.device)
                if i in prunable:
                    bn = bn_of(loose.module_list[i])
                    mask = masks[i].to(bn.weight.dtype)
                    bn.weight.mul_(mask)
                    c = _act_of(loose.module_list[i])((1 - mask) * bn.bias.detach())
                    bn.bias.mul_(mask)
            elif kind == 'shortcut':
                c = const[i - 1] + const[i + int(d['from'][0])]
            elif kind == 'route':
                parts = [const[i + l if l < 0 else l] for l in d['layers']]
                if any(p is None for p in parts):
                    c = None
                elif 'groups' in d:
                    c = parts[0][parts[0].numel() // 2:]
                else:
                    c = torch.cat(parts)
            elif kind in ('upsample', 'maxpool'):      # max(x + c) = max(x) + c per channel
                c = const[i - 1]
            elif kind == 'yolo':
                c = None
            else:
                raise NotImplementedError('slim_prune: block type %r' % kind)
            const.append(c)
            if kind != 'yolo':
                consume(i + 1, c)
    return loose


# ----------------------------------------------------------------------------------------------- compact model
def tensor_mask(defs, masks, i, in_channels):
    """0/1 mask over the channels of block i's output (block -1: the image)."""
    if i < 0:
        return torch.ones(in_channels)
    d = defs[i]
    kind = d['type']
    if kind == 'convolutional':
        return masks[i].cpu() if i in masks else torch.ones(int(d['filters']))
    if kind == 'route':
        parts = [tensor_mask(defs, masks, i + l if l < 0 else l, in_channels) for l in d['layers']]
        if 'groups' in d:
            return parts[0][parts[0].numel() // 2:]
        return torch.cat(parts)
    # depthwise, se, shortcut (its operands share one merged mask), upsample, maxpool: the channels of what they read
    return tensor_mask(defs, masks, i - 1, in_channels)


def compact_defs(defs, masks):
    out = copy.deepcopy(defs)
    for i, mask in masks.items():
        out[i]['filters'] = str(int(mask.sum()))
    return out


def gather_weights(compact, loose, sets, masks):
    """Copy the surviving channels of ``loose`` into ``compact``: conv + BN blocks by (output mask, mask of the tensor they read), the
    rest whole except for the input channels of convs without BatchNorm."""
    defs = loose.module_defs
    in_ch = loose.module_list[0][0].in_channels
    nz = lambda m, dev: torch.nonzero(m, as_tuple=False)[:, 0].to(dev)
    with torch.no_grad():
        for i in sets.bn_convs:
            cb, lb = compact.module_list[i], loose.module_list[i]
            dev = lb[0].weight.device
            keep_out, keep_in = nz(masks[i], dev), nz(tensor_mask(defs, masks, i - 1, in_ch), dev)
            cbn, lbn = bn_of(cb), bn_of(lb)
            for name in ('weight', 'bias', 'running_mean', 'running_var'):
                getattr(cbn, name).data = getattr(lbn, name).data[keep_out].clone()
            cb[0].weight.data = lb[0].weight.data[:, keep_in][keep_out].clone()
        for i in sets.other:
            cb, lb = compact.module_list[i], loose.module_list[i]
            kind = defs[i]['type']
            if kind == 'convolutional':
                keep_in = nz(tensor_mask(defs, masks, i - 1, in_ch), lb[0].weight.device)
                cb[0].weight.data = lb[0].weight.data[:, keep_in].clone()
                cb[0].bias.data = lb[0].bias.data.clone()
            elif kind == 'se':
                for k in (0, 2):
                    cb[0].fc[k].weight.data = lb[0].fc[k].weight.data.clone()
            else:       # depthwise: never cut
                cb[0].weight.data = lb[0].weight.data.clone()
                cbn, lbn = bn_of(cb), bn_of(lb)
                for name in ('weight', 'bias', 'running_mean', 'running_var'):
                    getattr(cbn, name).data = getattr(lbn, name).data.clone()


def slim_prune(model, percent, layer_keep=0.01, img_size=416, verbose=False):
    """``model`` (a ``Darknet`` with sparsity-trained weights, any device / float dtype) -> dict(threshold, masks, defs = compact
    block dicts, model = compact ``Darknet`` with the gathered weights on the same device and dtype, loose = the keep-size model)."""
    import models
    defs = model.module_defs
    sets = layer_sets(defs, 1)
    thresh = global_threshold(model, sets.prune, percent)
    masks = channel_masks(model, sets, thresh, layer_keep)
    if verbose:
        cut = sum(int(m.numel() - m.sum()) for m in masks.values())
        print('Global threshold %.4f: %d of %d channels under it' % (float(thresh), cut, sum(m.numel() for m in masks.values())))
    masks = merge_shortcut_masks(defs, masks)
    loose = fold_pruned_constants(model, sets, masks)
    cdefs = compact_defs(defs, masks)
    ref = next(model.parameters())
    with torch.random.fork_rng(devices=[]):
        compact = models.Darknet([copy.deepcopy(model.hyperparams)] + copy.deepcopy(cdefs), (img_size, img_size),
                                 is_gray_scale=bool(getattr(model, 'is_gray_scale', False))).to(device=ref.device, dtype=ref.dtype)
    gather_weights(compact, loose, sets, masks)
    if verbose:
        for i in sets.bn_convs:
            print('layer index: %3d \t total channel: %4d \t remaining channel: %4d' % (i, masks[i].numel(), int(masks[i].sum())))
    return dict(threshold=thresh, masks=masks, defs=cdefs, model=compact, loose=loose, sets=sets)


# ----------------------------------------------------------------------------------------------- files
def _anchors_text(cfg_path):
    """The anchors line of the source cfg as written (the parsed block holds an array)."""
    for line in open(cfg_path).read().split('\n'):
        for sep in (' = ', '='):
            if line.split(sep)[0] == 'anchors':
                return line.split(sep)[1]
    return None


def cfg_text(hyperparams, defs, anchors):
    """Darknet cfg text of ``[net]`` + blocks: one ``key=value`` line per entry in the parsed order; list-valued entries (shortcut
    from, route layers, yolo mask) comma-joined, anchors as in the source file."""
    lines = []
    for block in [dict(hyperparams)] + [dict(d) for d in defs]:
        kind = block['type']
        if kind == 'shortcut':
            block['from'] = str(block['from'][0])
        elif kind == 'route':
            block['layers'] = ','.join('%s' % v for v in block['layers'])
        elif kind == 'yolo':
            block['mask'] = ','.join('%s' % v for v in block['mask'])
            block['anchors'] = anchors
        lines.append('[%s]\n' % kind)
        lines.extend('%s=%s\n' % (k, v) for k, v in block.items() if k != 'type')
        lines.append('\n')
    return ''.join(lines)


def output_paths(cfg_path, percent):
    """cfg/<family>/<net>.cfg -> (cfg/slim_prune_P<family>/slim_prune_P<net>.cfg, weights/slim_prune_P<family>/slim_prune_P_percent.weights)"""
    tag = 'slim_prune_%s' % percent
    family_dir, net = os.path.split(cfg_path)
    root, family = os.path.split(family_dir)
    cfg_dir = os.path.join(root, tag + family)
    head, tail = os.path.split(root)
    weights_root = os.path.join(head, 'weights') if tail == 'cfg' else os.path.join(root, 'weights')
    return os.path.join(cfg_dir, tag + net), os.path.join(weights_root, tag + family, tag + '_percent.weights')


def make_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--cfg', type=str, default='cfg/yolov3.cfg', help='cfg file path')
    parser.add_argument('--data', type=str, default='data/coco.data', help='*.data file path')
    parser.add_argument('--weights', type=str, default='weights/last.pt', help='sparse model weights')
    parser.add_argument('--percent', type=float, default=0.8, help='global channel prune percent')
    parser.add_argument('--layer_keep', type=float, default=0.01, help='channel keep percent per layer')
    parser.add_argument('--img-size', type=int, default=416, help='inference size (pixels)')
    parser.add_argument('--batch-size', type=int, default=16, help='batch-size')
    parser.add_argument('--no-eval', action='store_true', help='skip the test.test runs before and after')
    return parser


def main(argv=None):
    import models
    opt = make_parser().parse_args(argv)
    print(opt)
    device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    model = models.Darknet(opt.cfg, (opt.img_size, opt.img_size)).to(device)
    if opt.weights.endswith('.pt'):
        model.load_state_dict(torch.load(opt.weights, map_location=device, weights_only=False)['model'])
    else:
        models.load_darknet_weights(model, opt.weights)
    print('\nloaded weights from ', opt.weights)

    def evaluate(m):
        from test import test
        with torch.no_grad():
            return test(model=m, cfg=opt.cfg, data=opt.data, batch_size=opt.batch_size, imgsz=opt.img_size, rank=-1)

    count = lambda m: sum(p.nelement() for p in m.parameters())
    before = None if opt.no_eval else evaluate(model)
    res = slim_prune(model, opt.percent, opt.layer_keep, opt.img_size, verbose=True)
    compact = res['model']
    after = None if opt.no_eval else evaluate(compact)
    from terminaltables import AsciiTable
    table = [['Metric', 'Before', 'After'], ['Parameters', '%d' % count(model), '%d' % count(compact)]]
    if not opt.no_eval:
        table.insert(1, ['mAP', '%.6f' % before[0][2], '%.6f' % after[0][2]])
    print(AsciiTable(table).table)

    cfg_out, weights_out = output_paths(opt.cfg, opt.percent)
    for path in (cfg_out, weights_out):
        os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(cfg_out, 'w') as f:
        f.write(cfg_text(model.hyperparams, res['defs'], _anchors_text(opt.cfg)))
    print('Config file has been saved: %s' % cfg_out)
    models.save_weights(compact, path=weights_out)
    print('Compact model has been saved: %s' % weights_out)
    return cfg_out, weights_out


if __name__ == '__main__':
    main()
