"""CPU half of tests/test_gpu_grad_conv.py: the case table, references and yardsticks of tests/grad_conv_cases.py hold on
their own.

1. the restated dispatch and split plan against dmh_conv_wgrad_workspace_floats / dmh_conv_unshuffle_wgrad_workspace_floats;
2. every unit of every case (rows and columns of the exact-fp32 instances, (64-o tile, 32-c block, tap) of the fp16-piece
   instances, db per channel, and dx / dw / db of the composites) has e32 < CAP: a condition on the inputs, decided by the
   references alone;
3. the written-out formula is float64 autograd of F.conv2d, for every mode; the one-hot expectations are the formula's;
4. the table really holds the edges the GPU file claims to reach;
5. wrong kernels, built by mutating the reference, miss their gate — the factor is printed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grad_conv_cases as gc
from dmhomo_amd import _lib


def _find(inst, **kw):
    names = ('inst', 'mode', 'B', 'H', 'W', 'C0', 'C1', 'Cout', 'kind', 'db', 'seed')
    hit = [c for c in gc.CASES if c[0] == inst and all(c[names.index(k)] == v for k, v in kw.items())]
    assert hit, (inst, kw)
    return hit[0]


def _base(inst, kind='unit'):
    c0, co = gc.base_channels(inst)
    return _find(inst, mode='plain', B=gc.CH_B, H=gc.CH_HW[0], W=gc.CH_HW[1], C0=c0, Cout=co, kind=kind, db=True)


# ------------------------------------------------------------------ 1. dispatch and plan
def test_plan_matches_the_workspace_size_functions():
    h = _lib.lib()
    for case in gc.CASES:
        inst, _, B, H, W, C0, C1, Cout = case[:8]
        p = gc.plan(case)
        if inst == 'wu':
            got = h.dmh_conv_unshuffle_wgrad_workspace_floats(B, 2 * H, 2 * W, C0, Cout)
            assert gc.instance_of('dmh_conv_unshuffle_wgrad', 1) == inst
        else:
            got = h.dmh_conv_wgrad_workspace_floats(B, H, W, C0, C1, Cout, gc.INSTANCES[inst]['k'])
            assert gc.instance_of('dmh_conv_wgrad', gc.INSTANCES[inst]['k']) == inst
        assert got == p['workspace'], (gc.case_id(case), got, p)
        assert p['part_w'] + p['part_b'] <= p['workspace'] and p['per'] * p['nsplit'] >= p['nitems']
        assert p['family'] == ('f16' if inst in gc.F16 else 'fp32')
    assert h.dmh_conv_wgrad_workspace_floats(1, 4, 4, 4, 0, 4, 0) == -1
    assert h.dmh_conv_unshuffle_wgrad_workspace_floats(1, 3, 4, 4, 4) == -1       # odd H


# ------------------------------------------------------------------ 2. e32 < CAP for every unit
@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_yardsticks(inst):
    mine = [c for c in gc.CASES if c[0] == inst]
    top = {}
    for case in mine:
        r = gc.wgrad_reference(case)
        assert bool(torch.isfinite(r['dw64']).all()) and bool(torch.isfinite(r['dw32']).all())
        assert set(r['e32']) == ({'rows', 'cols', 'db'} if inst in gc.FP32 else {'blocks', 'db'})
        for u, e in gc.worst_e32(r).items():
            assert e < gc.CAP, f'{gc.case_id(case)}: e32 of {u} = {e:.3e} is over the cap {gc.CAP:.0e}: give the case another seed'
            if e > top.get(u, (0.0, ''))[0]:
                top[u] = (e, gc.case_id(case))
        if inst in gc.F16:                   # the yardstick itself has exact zeros where the reference block is zero
            zero = gc.block_amax(r['dw64']) == 0
            assert bool((gc.block_amax(r['dw32'].double())[zero] == 0).all())
    print(f'[yardstick] grad_conv {inst}: {len(mine)} cases; worst e32 ' +
          ', '.join(f'{u} {e:.3e} ({cid})' for u, (e, cid) in top.items()))


def test_composite_yardsticks():
    top = {}
    for c in gc.COMPOSITES:
        r = gc.composite_reference(c)
        for u, e in r['e32'].items():
            assert e.max().item() < gc.CAP, (gc.composite_id(c), u, e.max().item())
            if e.max().item() > top.get((c[0], u), (0.0, ''))[0]:
                top[(c[0], u)] = (e.max().item(), gc.composite_id(c))
    for (name, u), (e, cid) in top.items():
        print(f'[yardstick] grad_conv composite {name} {u}: worst e32 {e:.3e} ({cid})')


# ------------------------------------------------------------------ 3. the formula is float64 autograd of F.conv2d
def _autograd_wgrad(case, inp):
    """dW, db by autograd of F.conv2d over the input built with torch's own upsample / unshuffle / SiLU, NCHW float64"""
    inst, mode = case[:2]
    d = gc.INSTANCES[inst]
    x = inp['x0'].double().permute(0, 3, 1, 2)
    if inp['in_coef'] is not None:
        c = inp['in_coef'].double()
        x = F.silu(c[:, 0, :, None, None] * x + c[:, 1, :, None, None])
    if inp['x1'] is not None:
        x = torch.cat([x, inp['x1'].double().permute(0, 3, 1, 2)], 1)
    if mode == 'ups':
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    if inst == 'wu':
        x = F.pixel_unshuffle(x, 2)
    dy = inp['dy'].double().permute(0, 3, 1, 2)
    w = torch.zeros((dy.shape[1], x.shape[1], d['k'], d['k']), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((dy.shape[1],), dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.conv2d(x, w, b, 1, d['pad']), (w, b), dy)


def test_formula_is_conv2d_autograd():
    picks = [_find('w3', mode='plain', B=3, H=5, W=17, C0=36, Cout=68, kind='unit', db=True),
             _find('w3', mode='concat', C0=36, C1=20, kind='unit'), _find('w3', mode='coef', C0=36),
             _find('w3', mode='ups', B=3, H=6, W=18, C0=36), _find('w2', B=3, H=5, W=17, C0=36, Cout=68, kind='unit', db=True),
             _find('w1', mode='concat', C0=60, C1=8), _find('w1', mode='coef', C0=36), _find('w7', mode='concat'),
             _find('w7', mode='coef', C0=36), _find('w7', mode='plain', B=3, H=3, W=7), _find('wu', B=3, H=5, W=17, C0=20, Cout=68, kind='unit', db=True),
             _find('w3', B=1, H=1, W=1), _find('w2', B=1, H=1, W=1), _find('wu', B=1, H=1, W=1)]
    for case in picks:
        r = gc.wgrad_reference(case)
        aw, ab = _autograd_wgrad(case, r['inp'])
        ew = ((aw - r['dw64']).abs().max() / r['dw64'].abs().max()).item()
        eb = ((ab - r['db64']).abs().max() / r['dysum'].max()).item()
        print(f'[yardstick] grad_conv {gc.case_id(case)}: formula vs F.conv2d autograd, float64: dW {ew:.2e} db {eb:.2e}')
        assert ew <= 1e-13 and eb <= 1e-13, gc.case_id(case)


@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_onehot_expectation_is_the_formula(inst):
    """the index-written window of `onehot_expected` against the formula (every product exact, every other term zero)"""
    mode = 'ups' if inst == 'w3' else 'plain'
    for m in dict.fromkeys(('plain', mode)):
        hw = (6, 18) if m == 'ups' else (5, 17)
        c0, co = gc.base_channels(inst)
        case = (inst, m, 2, hw[0], hw[1], c0, 0, co, 'unit', True, 0)
        hin, win = gc.stored_hw(case)
        x = gc.eighths((2, hin, win, c0), 5100)
        for (y0, x0) in [(0, 0), (hw[0] - 1, hw[1] - 1), (3, 15), (4, 16)]:
            dy = torch.zeros((2, hw[0], hw[1], co))
            dy[1, y0, x0, 5] = 1.0
            dw, db = gc.wgrad_formula(dict(dy=dy, x0=x, x1=None, in_coef=None), case, torch.float32)
            assert torch.equal(dw, gc.onehot_expected(case, x, 1, y0, x0, 5)), (inst, m, y0, x0)
            assert torch.equal(db, dy[1, y0, x0])


# ------------------------------------------------------------------ 4. the table holds the edges
def test_case_table_reaches_the_edges():
    ids = [gc.case_id(c) for c in gc.CASES]
    assert len(set(ids)) == len(ids)
    for inst, d in gc.INSTANCES.items():
        mine = [c for c in gc.CASES if c[0] == inst]
        assert {c[1] for c in mine} == set(d['modes']), inst
        assert any((c[3], c[4], c[2]) == (1, 1, 1) for c in mine), inst                  # one pixel, one sample
        assert {(c[3], c[4]) for c in mine if c[1] == 'plain'} >= set(gc.GEOMETRIES), inst
        assert {c[2] for c in mine} == {1, 3}
        assert sum(1 for c in mine if not c[9]) == 1, inst                               # db = NULL once
        assert all(gc.plan(c)['per'] == 1 for c in mine), inst     # (several items per workgroup: tests/test_gpu_wgrad_splits.py)
        assert any(c[7] == 4 for c in mine) and any(c[7] > 128 for c in mine), inst
        assert inst in ('w7', 'wu') or any(c[7] == 64 for c in mine), inst
        assert all(c[2] <= 3 and c[3] <= 9 and c[4] <= 33 for c in mine)
    for inst in gc.F16:
        mine = [c for c in gc.CASES if c[0] == inst]
        cins = {gc.cin_of(c) for c in mine}
        assert any(c <= 32 for c in cins) and 4 in cins, inst                            # the second workgroup of a pair returns
        assert any(gc.plan(c)['idle'] > 0 for c in mine)
        assert any(c % 32 for c in cins), inst                                           # a ragged 32-block
        assert any(c > 64 and c % 64 for c in cins), inst                                # a second, ragged c tile
        assert any(c[7] == 4 for c in mine), inst
        assert {c[8] for c in mine} >= {'unit', 'otile', 'cblock'}
    w3 = [c for c in gc.CASES if c[0] == 'w3']
    assert {(c[5], c[6]) for c in w3 if c[1] == 'concat'} >= set(gc.CONCATS)
    assert {(c[5], c[6]) for c in w3 if c[8] == 'jump'} == {(32, 64), (36, 20)}          # boundary on / inside a 32-block
    assert {(c[3], c[4]) for c in w3 if c[1] == 'ups'} >= set(gc.UPS_GEOMETRIES)
    w7 = [c for c in gc.CASES if c[0] == 'w7']
    assert any(gc.cin_of(c) % 16 and gc.cin_of(c) > 16 for c in w7) and any(gc.cin_of(c) < 16 for c in w7)   # ragged 16-blocks
    assert {gc.cin_of(c) for c in w7} >= {4, 12, 16, 20, 36}
    wu = [c for c in gc.CASES if c[0] == 'wu']
    assert {(c[5], c[7]) for c in wu} >= {(a, b) for a in (4, 8, 16, 20, 36) for b in (4, 68, 132)}
    for inst in gc.FP32:
        assert {c[8] for c in gc.CASES if c[0] == inst} == {'unit', 'ochan', 'cchan'}
    print('[yardstick] grad_conv cases per instance: ' +
          ', '.join(f'{i} {sum(1 for c in gc.CASES if c[0] == i)}' for i in gc.INSTANCES) + f'; composites {len(gc.COMPOSITES)}')


# ------------------------------------------------------------------ 5. wrong kernels miss their gate
def _factor(name, case, r, dw, db):
    f, where = gc.worst(case, r, dw, db)
    print(f'[mutation] grad_conv {gc.case_id(case)}: {name}: worst err / gate = {f:.3g} at {where}')
    return f


def test_right_answer_passes_every_gate():
    """the fp32 yardstick passes (10 x its own error), so the gates below are not failed by everything"""
    for inst in gc.INSTANCES:
        case = _base(inst)
        r = gc.wgrad_reference(case)
        assert _factor('fp32 yardstick', case, r, r['dw32'], r['db32']) <= 0.1 + 1e-12


@pytest.mark.parametrize('inst', ['w3', 'w2', 'w7'])
def test_mutation_two_taps_exchanged(inst):
    case = _base(inst)
    r = gc.wgrad_reference(case)
    dw = r['dw32'].clone()
    dw[:, :, 0, 0], dw[:, :, 0, 1] = r['dw32'][:, :, 0, 1], r['dw32'][:, :, 0, 0]
    assert _factor('taps (0,0) and (0,1) exchanged', case, r, dw, r['db32']) > 100


@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_mutation_last_pixel_of_an_item_dropped(inst):
    case = _base(inst)
    r = gc.wgrad_reference(case)
    dy = r['inp']['dy'].clone()
    dy[:, gc.TH - 1::gc.TH, gc.TW - 1::gc.TW] = 0
    assert bool((dy != r['inp']['dy']).any())
    dw, db = gc.wgrad_formula(r['inp'], case, torch.float32, dy=dy)
    assert _factor('pixel (3, 15) of every item dropped', case, r, dw, db) > 100
    assert _factor('... from db only', case, r, r['dw32'], db) > 100


def test_mutation_unshuffle_order():
    for case in (_base('wu'), _find('wu', C0=4, Cout=4)):
        r = gc.wgrad_reference(case)
        dw, db = gc.wgrad_formula(r['inp'], case, torch.float32, order='px*2+py')
        assert _factor('channel order c*4 + px*2 + py', case, r, dw, db) > 100


@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_mutation_db_from_the_wrong_tile(inst):
    case = _find(inst, mode='plain', B=3, H=5, W=17, Cout=132, kind='unit')
    r = gc.wgrad_reference(case)
    db = r['db32'].clone()
    db[:64], db[64:128] = r['db32'][64:128], r['db32'][:64]
    assert _factor('db of tile 1 in tile 0 and back', case, r, r['dw32'], db) > 100


@pytest.mark.parametrize('inst', gc.F16)
def test_mutation_one_scale_for_all_input_channels(inst):
    """the `cblock` cases through the two-piece fp16 split emulated in numpy (IEEE fp16 with gradual underflow), once with one
    scale per 32-channel block, as the kernel has it, once with one scale for all 68 channels.
    cblock (blocks at 1e3, 1, 1e-3): the 1e-3 block sits 2^20 below the maximum, only its SECOND piece is an fp16 subnormal
    and it keeps about 20 bits: > 10x the error of the per-block split, but still inside the gate (0.75 of it for the 3x3) —
    this kind alone would not notice such a kernel, and the figure is printed, not hidden.
    cblockw (1e4, 1, 1e-4): the 1e-4 block's FIRST piece is subnormal, about 10 bits are left, and the gate is missed."""
    f = {kind: _one_scale_factors(inst, kind) for kind in ('cblock', 'cblockw')}
    for kind in f:
        assert f[kind]['one scale per 32-channel block'] < 0.1, f
    assert f['cblock']['one scale for all input channels'] > 10 * f['cblock']['one scale per 32-channel block'], f
    assert f['cblockw']['one scale for all input channels'] > 10, f


def _one_scale_factors(inst, kind):
    case = _find(inst, kind=kind)
    r = gc.wgrad_reference(case)
    d = gc.INSTANCES[inst]
    k, pad = d['k'], d['pad']
    X = gc.conv_input(r['inp'], case, torch.float64)
    Xp = F.pad(X, (0, 0, pad, pad, pad, pad)).numpy()
    dy = r['inp']['dy'].double().numpy()
    B, H, W, Cout = dy.shape
    cin = X.shape[3]
    dyf = dy.reshape(-1, Cout)
    sd = np.array([gc.max_exponent(dyf[:, o // gc.OT * gc.OT:(o // gc.OT + 1) * gc.OT]) for o in range(Cout)])
    Xn = X.numpy()
    per_block = np.array([gc.max_exponent(Xn[..., c // gc.CB * gc.CB:(c // gc.CB + 1) * gc.CB]) for c in range(cin)])
    one = np.full((cin,), gc.max_exponent(Xn))
    f = {}
    for name, sx in (('one scale per 32-channel block', per_block), ('one scale for all input channels', one)):
        dw = np.zeros((Cout, cin, k, k))
        for ky in range(k):
            for kx in range(k):
                dw[:, :, ky, kx] = gc.split2_product(dyf, Xp[:, ky:ky + H, kx:kx + W].reshape(-1, cin), sd, sx)
        f[name] = _factor(name, case, r, torch.from_numpy(dw), r['db32'])
    return f
