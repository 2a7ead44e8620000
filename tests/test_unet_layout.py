"""CPU: layout.unet_layout, the one reading of the UNet trunk that the sampling engine and the training tape walk, checked
against the parameters it claims and against the oracle's independent walk (its tap order)."""
from collections import Counter

import pytest
import torch
from torch import nn

CASES = [
    ('cfg', dict(dim=8, dim_mults=(1, 2), channels=6, num_classes=1)),
    ('ddpm', dict(dim=8, dim_mults=(1, 2), channels=3)),
    ('cfg', dict(dim=64, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)),
    ('ddpm', dict(dim=64, dim_mults=(1, 2, 4, 8), channels=3)),
    ('cfg', dict(dim=16, dim_mults=(1,), channels=3, num_classes=2)),
    ('ddpm', dict(dim=16, dim_mults=(1,), channels=6)),
    ('cfg', dict(dim=16, dim_mults=(1, 2, 4), channels=3, num_classes=1)),
    ('ddpm', dict(dim=16, dim_mults=(1, 2, 4), channels=6)),
    ('cfg', dict(dim=16, dim_mults=(1, 2), channels=6, num_classes=1, init_dim=24)),
    ('ddpm', dict(dim=16, dim_mults=(1, 2), channels=3, init_dim=24)),
    ('ddpm', dict(dim=8, dim_mults=(1, 2), channels=3, self_condition=True)),
    ('cfg', dict(dim=8, dim_mults=(1, 2), channels=6, num_classes=1, learned_variance=True)),
    ('ddpm', dict(dim=8, dim_mults=(1, 2), channels=6, learned_variance=True)),
]
EMBEDDING = ('time_mlp.', 'classes_mlp.', 'classes_emb.', 'null_classes_emb')
# role -> (holder module type, parameter name): catches a role bound to the wrong kind of parameter
ROLE_PARAM = dict(w1=(nn.Conv2d, 'weight'), w2=(nn.Conv2d, 'weight'), rw=(nn.Conv2d, 'weight'), qkv=(nn.Conv2d, 'weight'),
                  ow=(nn.Conv2d, 'weight'), w=(nn.Conv2d, 'weight'), b1=(nn.Conv2d, 'bias'), b2=(nn.Conv2d, 'bias'),
                  rb=(nn.Conv2d, 'bias'), ob=(nn.Conv2d, 'bias'), b=(nn.Conv2d, 'bias'), g1=(nn.GroupNorm, 'weight'),
                  g2=(nn.GroupNorm, 'weight'), be1=(nn.GroupNorm, 'bias'), be2=(nn.GroupNorm, 'bias'), g=(nn.Module, 'g'),
                  og=(nn.Module, 'g'), mlp_w=(nn.Linear, 'weight'), mlp_b=(nn.Linear, 'bias'))


def _build(which, kw):
    from dmhomo_amd import cfg, ddpm
    torch.manual_seed(0)
    return (cfg if which == 'cfg' else ddpm).Unet(**kw)


def _oracle_taps(which, m, kw):
    """the oracle's walk at 8x8 on the CPU -> (tap names in order, exception or None)"""
    from oracle import unet as OU
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    B, S, ch = 2, 8, kw['channels']
    x = torch.randn(B, ch, S, S, generator=g)
    t = torch.tensor([3, 700])
    taps, err = {}, None
    try:
        with torch.no_grad():
            if which == 'cfg':
                OU.cfg_unet_forward(sd, x, t, torch.zeros(B, dtype=torch.long), torch.rand(B, 3, S, S, generator=g),
                                    torch.ones(B, 1, S, S), torch.tensor([True, False]), taps=taps)
            else:
                sc = kw.get('self_condition', False)
                OU.ddp_unet_forward(sd, x, t, torch.randn(B, ch, S, S, generator=g) if sc else None, sc, taps=taps)
    except RuntimeError as e:
        err = e
    return list(taps), err


def _in_out(n, shapes):
    """(input channels, output channels) of node n as its weights state them"""
    k = n.keys
    if n.kind == 'res':
        assert shapes[k['w2']][:2] == (n.cout, n.cout)
        if 'rw' in k:
            assert shapes[k['rw']][:2] == shapes[k['w1']][:2]
        return shapes[k['w1']][1], shapes[k['w1']][0]
    if n.kind in ('linattn', 'attn'):
        return shapes[k['qkv']][1], shapes[k['ow']][0]
    return shapes[k['w']][1] // (4 if n.kind == 'unshuffle' else 1), shapes[k['w']][0]


@pytest.mark.parametrize('which,kw', CASES, ids=[f'{w}-{i}' for i, (w, _) in enumerate(CASES)])
def test_unet_layout(which, kw):
    from dmhomo_amd.layout import HIDDEN, unet_layout
    m = _build(which, kw)
    params = dict(m.named_parameters())
    shapes = {k: tuple(v.shape) for k, v in params.items()}
    L = unet_layout(m.named_parameters())
    nodes = L.nodes
    init_dim = kw.get('init_dim', kw['dim'])

    # the embedding facts
    assert (L.dim, L.has_classes, L.fourier) == (kw['dim'], which == 'cfg', False)
    assert (L.init_dim, L.out_dim, L.cin) == (init_dim, m.out_dim, shapes['init_conv.weight'][1])
    assert L.cin_pad % 4 == 0 and L.cin <= L.cin_pad < L.cin + 4

    # every trunk parameter is claimed exactly once, by a parameter of the role's kind and shape, under its node's name
    claimed = Counter(['init_conv.weight', 'init_conv.bias', 'final_conv.weight', 'final_conv.bias'])
    for n in nodes:
        for role, key in n.keys.items():
            claimed[key] += 1
            assert key.startswith(n.name + '.'), (n.name, role, key)
            typ, pname = ROLE_PARAM[role]
            mod, _, leaf = key.rpartition('.')
            assert leaf == pname and isinstance(m.get_submodule(mod), typ), (n.name, role, key)
            assert shapes[key][0] == {'qkv': 3 * HIDDEN, 'g': 1, 'og': 1, 'mlp_w': 2 * n.cout,
                                      'mlp_b': 2 * n.cout}.get(role, n.cout), (n.name, role, key)
    trunk = [k for k in params if not k.startswith(EMBEDDING)]
    assert sorted(claimed) == sorted(trunk)
    assert all(c == 1 for c in claimed.values()), [k for k, c in claimed.items() if c != 1]

    # (scale, shift) columns: one 2 * cout slice per ResnetBlock, in node order, filling the mlp.1 rows
    off = 0
    for n in nodes:
        assert (n.ss_off is not None) == (n.kind == 'res'), n.name
        if n.kind == 'res':
            assert n.ss_off == off, n.name
            off += 2 * n.cout
    assert L.ss_total == off == sum(v[0] for k, v in shapes.items() if k.endswith('.mlp.1.weight'))

    # the skip stack balances: the init_conv output first, every pop takes the channels of the matching push
    stack, c, mismatched = [('init_conv', init_dim)], init_dim, []
    for n in nodes:
        assert n.c0 == c, (n.name, n.c0, c)
        if n.c1:
            _, c1 = stack.pop()
            assert n.c1 == c1, n.name
        if n.push:
            stack.append((n.name, n.cout))
        cin, cout = _in_out(n, shapes)
        assert cout == n.cout, n.name
        if cin != n.c0 + n.c1:
            mismatched.append(n.name)
        c = n.cout
    assert stack == []
    assert c == shapes['final_conv.weight'][1]
    assert [n.name for n in nodes if n.kind == 'res' and n.c1] == \
        [f'ups.{i}.{j}' for i in range(len(kw['dim_mults'])) for j in (0, 1)] + ['final_res_block']

    # the oracle's walk taps init_conv, then every trunk module in the order it runs them
    taps, err = _oracle_taps(which, m, kw)
    assert taps[0] == 'init_conv'
    if init_dim == kw['dim']:
        assert err is None and mismatched == []
        assert taps[1:] == [n.name for n in nodes]
    else:
        # the reference's final_res_block is built for dim * 2 input channels but receives 2 * init_dim (CFG:400, 464):
        # the layout reports what the walk feeds it, and the oracle fails at that same block
        assert mismatched == ['final_res_block'] and err is not None
        assert taps[1:] == [n.name for n in nodes][:-1]


def test_unet_layout_flags_learned_sinusoidal_embedding():
    from dmhomo_amd.layout import unet_layout
    for which, kw in (('cfg', dict(num_classes=1)), ('ddpm', {})):
        for flag in ('learned_sinusoidal_cond', 'random_fourier_features'):
            m = _build(which, dict(dim=8, dim_mults=(1, 2), channels=3, **kw, **{flag: True}))
            L = unet_layout(m.named_parameters())
            assert L.fourier and L.dim == 17          # time_mlp.1 takes learned_sinusoidal_dim + 1 inputs
