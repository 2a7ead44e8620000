"""CPU half of tests/test_gpu_linattn_fused.py: every case of tests/linattn_fused_cases.py reaches the branch of
csrc/linattn_fused.hip its table row names, its fp32 yardstick stays under the cap, and the stress kinds really put their
inputs where they claim to.

The launch plan of the fused passes has one export, dmh_linattn_fused_splits (a pure host function); the sub-tile count per
workgroup (`fused_tiles`) and the two sub-tile loops have none and are restated in linattn_fused_cases.plan — the kernel
file points back at this test from all three places."""
import math

import pytest
import torch

import linattn_fused_cases as lc


@pytest.fixture(scope='module')
def splits():
    from dmhomo_amd import _lib
    return _lib.lib().dmh_linattn_fused_splits


def test_plan_matches_the_library(splits):
    """the restated plan gives the library's split count for every n of the table and around every tile threshold"""
    ns = sorted({c.n for c in lc.CASES} | {t * 32 * 64 + d for t in range(1, 10) for d in (-1, 0, 1)} | {2240, 1 << 20})
    for n in ns:
        p = lc.plan(n)
        assert p['tiles'] == min(max(lc.cdiv(n, 64) // 32, 1), 8)
        for B in (1, 2, 50):            # the plan is a function of n only
            assert splits(B, n) == p['ns'], (B, n)
        assert (p['ns'] - 1) * p['tiles'] + p['last_tiles'] == p['nt'] and 1 <= p['last_tiles'] <= p['tiles']


def test_case_table_reaches_the_branches_it_names(splits):
    """tiles, split count, a short last split and a ragged last sub-tile of every pixel count of the table, from the library's
    split count and the restated tiles = clamp(cdiv(n, 64) // 32, 1, 8)"""
    def row(n):
        tiles = min(max(lc.cdiv(n, 64) // 32, 1), 8)
        ns = splits(2, n)
        nt = lc.cdiv(n, 64)
        assert ns == lc.cdiv(nt, tiles)
        return tiles, ns, nt - (ns - 1) * tiles < tiles, n % 64 != 0       # tiles, splits, short last split, ragged
    want = {1: (1, 1, False, True), 4: (1, 1, False, True), 63: (1, 1, False, True), 64: (1, 1, False, False),
            65: (1, 2, False, True),                 # the second split: one sub-tile with one pixel
            4095: (2, 32, False, True),              # a ragged last sub-tile inside a full split
            4096: (2, 32, False, False),
            4097: (2, 33, True, True),               # a 33rd split of one sub-tile with one pixel: the `break`, the prefetch guard
            4160: (2, 33, True, False),              # 65 sub-tiles: the 33rd split holds one full sub-tile
            6150: (3, 33, True, True),               # 97 sub-tiles: an odd number of staged chunks per workgroup for every C
            16384: (8, 32, False, False),
            16512: (8, 33, True, False)}             # the last split holds 2 of 8 sub-tiles
    assert {c.n for c in lc.CASES} == set(want)
    for n, w in want.items():
        assert row(n) == w, (n, row(n), w)
    p = lc.plan(16512)
    assert p['last_tiles'] == 2 and lc.plan(4097)['last_pixels'] == 1 and lc.plan(65)['last_pixels'] == 1
    # chunks staged by a full workgroup of n = 6150: tiles * (C / 32), odd only where C / 32 is; at C = 96 the two-buffer
    # alternation therefore changes parity from one sub-tile to the next at every n
    assert lc.plan(6150)['tiles'] % 2 == 1
    # every width at every pixel count, the odd widths and every kind where the table says, B = 1 and B = 3 at n = 4097
    have = set(lc.CASES)
    assert len(have) == len(lc.CASES)
    for n in lc.SMALL_N + lc.MID_N + lc.BIG_N + (4160,):
        for C in lc.WIDTHS:
            assert any(c.n == n and c.C == C and c.kind == 'plain' for c in have), (n, C)
    for n in lc.KIND_N:
        assert all(lc.Case(n, C, 2, 'plain') in have for C in lc.ODD_WIDTHS)
        assert all(lc.Case(n, C, 2, k) in have for C in lc.WIDTHS for k in lc.KINDS)
    assert {c.B for c in have if c.n == 4097} == {1, 2, 3}
    assert all(c.B == 1 and c.kind in ('plain', 'rising') for c in have if c.n in lc.BIG_N)
    assert lc.plan(4160)['tiles'] == 2 and 4160 % 64 == 0 and lc.plan(4160)['last_tiles'] == 1


@pytest.mark.parametrize('case', lc.CASES, ids=lc.case_id)
def test_yardstick_and_input_conditions(case):
    r = lc.case_reference(case)
    p, st = r['plan'], r['stats']
    for name, e in r['e32'].items():
        worst = float(e.max())
        print(f'[yardstick] {lc.case_id(case)} {name}: e32={worst:.3e}')
        assert math.isfinite(worst) and worst <= lc.CAP, f'{name}: e32 = {worst:.3e} is over the cap {lc.CAP:.0e}: soften the kind'
    for key in ('ctx', 'out', 'lse', 'wm') + (('y', 'r') if 'y' in r else ()):
        assert bool(torch.isfinite(r[key]).all()), key
    if r['zero']:
        assert not r['ctx'].any() and not r['out'].any()
        if 'y' in r and case.kind == 'constant_image':      # (zero_v: y = x + LN(b) * g_out, the bias is not constant there)
            assert torch.equal(r['y'], r['inp']['x'].double())
    else:
        assert float(r['ctx'].abs().amax((2, 3)).min()) > 0 and float(r['out'].abs().max()) > 0
        if 'y' in r:      # the block's result depends on the attention: to_out's result is not buried under the bias (0.1)
            assert r['t_rms'] >= 0.09, r['t_rms']
    if case.kind in ('rising', 'falling') and p['tiles'] >= 2:
        # at least half of the (row, head, d) columns meet, inside some workgroup, a running maximum that leaves the first
        # sub-tile's exponentials below 1e-3 of their first value: a missing rescale of s or ctx cannot hide
        frac = float((st['k']['first'] < 1e-3).double().mean())
        print(f'[yardstick] {lc.case_id(case)}: {frac:.2f} of the columns rescale by < 1e-3 inside a workgroup')
        assert frac >= 0.5, frac
    if case.kind == 'sharp_k':
        print(f'[yardstick] {lc.case_id(case)}: {st["k"]["under"]:.3f} of the pixels underflow exp2 in some column')
        assert st['k']['under'] > 0.9
    if case.kind == 'tiny_head':
        ratio = float(st['ctxmax'][3] / st['ctxmax'].max())
        assert ratio < 2.0 ** -10, ratio
    if case.kind == 'v_outlier' and case.n > lc.V_OUTLIER_AT:
        vp = st['v_pix']                                         # (B, n): max |v| of a pixel over heads and e
        big = vp[:, lc.V_OUTLIER_AT::lc.TP]
        mask = torch.ones(case.n, dtype=torch.bool)
        mask[lc.V_OUTLIER_AT::lc.TP] = False
        assert float(big.min() / vp[:, mask].max()) >= 2.0 ** 12
    if case.kind == 'gain_outlier':
        g = r['inp']['g'].abs()
        assert float(g.max() / g.sort().values[-2]) > 256
    if case.kind == 'one_hot_pixel':
        inp = r['inp']
        j = int(inp['g'].abs().argmax())
        for pix in lc.hot_pixels(case.n):
            ln = lc.layernorm(inp['x'][:, pix].double(), torch.ones(case.C, dtype=torch.float64))
            assert float((ln[:, j] - math.sqrt(case.C - 1)).abs().max()) < 1e-6      # the bound the static scale rests on
    if case.kind == 'constant_image':
        x = r['inp']['x']
        assert bool((x == x[..., :1]).all()) and (case.C != 64 or float(r['inp']['bo'].std()) == 0.0)
    if case.kind == 'zero_v':
        assert not r['inp']['w'][256:].any()


def test_gates_accept_fp32_and_reject_a_missing_rescale():
    """the pass-1 units of a tiles = 2 case: plain fp32 on the CPU passes the gates by construction (e32 <= 10 e32); a
    context whose running sum is not rescaled when the maximum rises (the mutation the GPU test must catch) does not"""
    case = lc.Case(4097, 64, 2, 'plain')
    inp = lc.inputs(case)
    r = lc._run(inp, torch.float64)
    lse, wm = lc.split_units(r['k'], r['v'], case.n)
    p = lc.plan(case.n)
    k, v = r['k'][..., :2 * lc.TP], r['v'][..., :2 * lc.TP]          # split 0 = two sub-tiles
    m0, m1 = k[..., :lc.TP].amax(3), k.amax(3)
    s_bad = (k[..., :lc.TP] - m0[..., None]).exp().sum(3) + (k[..., lc.TP:] - m1[..., None]).exp().sum(3)   # no rescale
    lse_bad = m1 + s_bad.log()
    err = (lse_bad - lse[:, 0]).abs().amax(2)
    assert p['tiles'] == 2 and float(err.min()) > 100 * lc.FLOOR * max(1.0, float(r['k'].abs().max()))
    assert bool((lc.unit_err(wm.float(), wm) <= lc.FLOOR).all())
