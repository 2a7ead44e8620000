"""The UNet trunk's topology, read once from the parameter names and shapes (no GPU, no values).

Both UNets of the reference (CFG = classifier_free_guidance.py:302-466, DDP = denoising_diffusion_pytorch.py:315-447)
share one trunk after ``init_conv`` (CFG:432-466 / DDP:413-447):

  downs.i  = ResnetBlock, ResnetBlock, Residual(PreNorm(LinearAttention)), Downsample     (i < ns)
  mid      = ResnetBlock, Residual(PreNorm(Attention)), ResnetBlock
  ups.i    = ResnetBlock(cat skip), ResnetBlock(cat skip), Residual(PreNorm(LinearAttention)), Upsample
  final_res_block(cat init_conv output)

``unet_layout`` turns that into the ordered list of ``Node``s that the sampling engine (engine.py) and the training tape
(train.py) walk.  The skip stack: the init_conv output is pushed first, then every node with ``push``; every node with
``c1 > 0`` pops the top of the stack as the second half of its input, so final_res_block pops the init_conv output last.
"""
import math
from dataclasses import dataclass

import torch

HEADS, DIM_HEAD = 4, 32     # CFG:246,275
HIDDEN = HEADS * DIM_HEAD
ATTN_SCALE = DIM_HEAD ** -0.5


def sinusoidal_freq(dim, device):
    """N7 frequency table of SinusoidalPosEmb, computed as the reference does it on the host (CFG:167-169)"""
    half = dim // 2
    f = math.log(10000) / (half - 1)
    return torch.exp(torch.arange(half) * -f).to(device)


@dataclass(frozen=True)
class Node:
    """one trunk module.  kind: 'res' (ResnetBlock), 'linattn' / 'attn' (Residual(PreNorm(LinearAttention / Attention))),
    'down4' (4x4 / stride 2 conv, CFG:110-111), 'unshuffle' (pixel-unshuffle + 1x1, DDP:110-113), 'same3' (the last
    stage's 3x3 conv, CFG:378,394), 'up3' (nearest x2 + 3x3, CFG:106-107).  The input is c0 channels, cat with c1 popped
    skip channels; keys maps the kind's roles to state-dict keys."""
    name: str
    kind: str
    c0: int
    c1: int
    cout: int
    push: bool
    keys: dict
    ss_off: int = None          # 'res': first column of its (scale, shift) in the concatenated mlp.1 output


@dataclass(frozen=True)
class Layout:
    dim: int                    # width of the time embedding fed to time_mlp.1
    has_classes: bool           # CFG Unet (class embedding) vs DDP Unet (time only)
    fourier: bool               # RandomOrLearnedSinusoidalPosEmb (time_mlp.0.weights, CFG:175-190) instead of SinusoidalPosEmb
    cin: int
    cin_pad: int                # init_conv input channels padded to a multiple of 4 (zero weights)
    init_dim: int
    out_dim: int
    ss_total: int
    nodes: tuple


def _res_keys(p, shapes):
    keys = dict(w1=p + '.block1.proj.weight', b1=p + '.block1.proj.bias', g1=p + '.block1.norm.weight',
                be1=p + '.block1.norm.bias', w2=p + '.block2.proj.weight', b2=p + '.block2.proj.bias',
                g2=p + '.block2.norm.weight', be2=p + '.block2.norm.bias', mlp_w=p + '.mlp.1.weight', mlp_b=p + '.mlp.1.bias')
    if p + '.res_conv.weight' in shapes:
        keys.update(rw=p + '.res_conv.weight', rb=p + '.res_conv.bias')
    return keys


def _attn_keys(p, linear):
    keys = dict(g=p + '.fn.norm.g', qkv=p + '.fn.fn.to_qkv.weight')
    if linear:
        keys.update(ow=p + '.fn.fn.to_out.0.weight', ob=p + '.fn.fn.to_out.0.bias', og=p + '.fn.fn.to_out.1.g')
    else:
        keys.update(ow=p + '.fn.fn.to_out.weight', ob=p + '.fn.fn.to_out.bias')
    return keys


def unet_layout(named_params):
    """``named_params``: (name, tensor) pairs or a {name: tensor} dict of a cfg.Unet / ddpm.Unet -> Layout"""
    shapes = {k: tuple(v.shape) for k, v in dict(named_params).items()}
    init_dim, cin = shapes['init_conv.weight'][:2]
    nodes, skip, ss = [], [init_dim], 0

    def add(name, kind, c0, cout, keys, push=False, c1=0, ss_off=None):
        nodes.append(Node(name, kind, c0, c1, cout, push, keys, ss_off))
        if push:
            skip.append(cout)
        return cout

    def res(name, c, push=False, pop=False):
        nonlocal ss
        keys = _res_keys(name, shapes)
        cout = shapes[keys['w1']][0]
        off, ss = ss, ss + 2 * cout
        return add(name, 'res', c, cout, keys, push, skip.pop() if pop else 0, off)

    def conv(name, c, kind, w):
        return add(name, kind, c, shapes[w][0], dict(w=w, b=w[:-len('weight')] + 'bias'))

    ns = 1 + max(int(k.split('.')[1]) for k in shapes if k.startswith('downs.'))
    c = init_dim
    for i in range(ns):
        p = f'downs.{i}'
        res(p + '.0', c, push=True)
        res(p + '.1', c)
        add(p + '.2', 'linattn', c, c, _attn_keys(p + '.2', True), push=True)
        if p + '.3.1.weight' in shapes:
            c = conv(p + '.3', c, 'unshuffle', p + '.3.1.weight')
        else:
            c = conv(p + '.3', c, 'down4' if shapes[p + '.3.weight'][-1] == 4 else 'same3', p + '.3.weight')
    c = res('mid_block1', c)
    add('mid_attn', 'attn', c, c, _attn_keys('mid_attn', False))
    c = res('mid_block2', c)
    for i in range(ns):
        p = f'ups.{i}'
        c = res(p + '.0', c, pop=True)
        c = res(p + '.1', c, pop=True)
        add(p + '.2', 'linattn', c, c, _attn_keys(p + '.2', True))
        if p + '.3.1.weight' in shapes:
            c = conv(p + '.3', c, 'up3', p + '.3.1.weight')
        else:
            c = conv(p + '.3', c, 'same3', p + '.3.weight')
    res('final_res_block', c, pop=True)
    assert not skip
    return Layout(dim=shapes['time_mlp.1.weight'][1], has_classes='classes_emb.weight' in shapes,
                  fourier='time_mlp.0.weights' in shapes, cin=cin, cin_pad=(cin + 3) // 4 * 4, init_dim=init_dim,
                  out_dim=shapes['final_conv.weight'][0], ss_total=ss, nodes=tuple(nodes))
