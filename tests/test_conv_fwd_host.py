"""CPU half of tests/test_gpu_conv_fwd.py: the references, yardsticks and case tables of tests/conv_fwd_cases.py hold on
their own.

Every case's per-channel fp32 yardstick e32_c is computed here and held under CAP = 2e-5, so that no GPU gate exceeds 2e-4,
and every channel's sum of |terms| over its largest |output| under gate / (8 u) (`host_condition`); the float64 reference
of every case is finite and its non-zero outputs are fp32-normal; the formula agrees with a restatement that uses none of torch's convolution, interpolation or activation functions; the stat-tile bound accepts the fp32 yardstick;
the tap-probe expectations are F.conv2d's; and the case table reaches every instance with every geometry, option and kind
it names."""
import pytest
import torch
import torch.nn.functional as F

import conv_fwd_cases as cf

FP32_TINY = torch.finfo(torch.float32).tiny


def _hold(case, r):
    ref64, e32 = r['ref64'], r['e32']
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(r['ref32']).all()), 'not finite'
    nz = ref64[ref64 != 0].abs()
    assert nz.numel() > 0 and nz.min().item() >= FP32_TINY and nz.max().item() < 3e38, (nz.min().item(), nz.max().item())
    worst = e32.max().item()
    print(f'[yardstick] {cf.case_id(case)}: worst e32_c={worst:.3e} (channel {int(e32.argmax())}) worst kappa_c='
          f'{r["kappa"].max().item():.1f}; {int((r["draw"] > 0).sum())} of {e32.numel()} channels redrawn (at most {int(r["draw"].max())} '
          f'times) ref_absmax={ref64.abs().max().item():.3e}')
    assert worst < cf.CAP, f'e32 = {worst:.3e} of channel {int(e32.argmax())} is over the cap {cf.CAP:.0e}: make the input milder'
    assert bool(cf.host_condition(r).all()), f'channel {int((~cf.host_condition(r)).nonzero()[0])} found no well-conditioned draw'
    return worst


@pytest.mark.parametrize('inst', list(cf.INSTANCES))
def test_yardsticks_and_references(inst):
    """every case of the instance: finite, fp32-normal, e32_c < CAP; stat tiles of the fp32 yardstick within their bound"""
    mine = [c for c in cf.CASES if c[0] == inst]
    assert mine
    worst = 0.0
    for case in mine:
        r = cf.conv_reference(case)
        worst = max(worst, _hold(case, r))
        B, Cout = case[1], case[6]
        assert r['ref64'].shape == (B, Cout) + cf.out_hw(inst, case[2], case[3])
        if 'stats' in cf.opt_set(case):
            ref, bound = cf.stat_reference(r['ref64'], r['gate'])
            got, _ = cf.stat_reference(r['ref32'].double(), r['gate'])      # exact sums of the fp32 outputs
            assert bool(((got - ref).abs() <= bound).all()), cf.case_id(case)
    print(f'[yardstick] {inst}: {len(mine)} cases, worst e32_c={worst:.3e}')


def test_packpw_case_yardstick():
    r = cf.packpw_reference()
    _hold(cf.PACKPW_CASE, r)
    inst, B, H, W = cf.PACKPW_CASE[:4]
    assert W == 3853 and 17 * W + 17 == 65518 and H > 2 * cf.INSTANCES[inst]['tile'][0]     # (16 bits hold 65535)
    assert bool((r['inp']['x0'] != 0).all())


@pytest.mark.parametrize('inst', list(cf.INSTANCES))
def test_formula_is_the_plain_restatement(inst):
    """two cases per instance — the fullest option set the instance takes and a data kind — in float64 and in fp32"""
    mine = [c for c in cf.CASES if c[0] == inst]
    full = max(mine, key=lambda c: len(cf.opt_set(c)))
    kind = next(c for c in mine if c[8] != 'unit')
    assert full != kind
    for case in (full, kind):
        inp = cf.conv_reference(case)['inp']
        a, b = cf.conv_formula(inp, inst, torch.float64), cf.conv_plain(inp, inst, torch.float64)
        e64 = cf.chan_rel(b, a).max().item()
        e32 = cf.chan_rel(cf.conv_plain(inp, inst, torch.float32), a).max().item()
        print(f'[yardstick] {cf.case_id(case)}: plain restatement vs formula float64 {e64:.3e}, fp32 restatement {e32:.3e}')
        assert e64 <= 1e-13 and e32 < cf.CAP


def test_case_table_is_complete():
    ids = [cf.case_id(c) for c in cf.CASES + [cf.PACKPW_CASE]]
    assert len(set(ids)) == len(ids)
    assert len(cf.INSTANCES) == 13 and len(cf.F16) == 11
    for case in cf.CASES + [cf.PACKPW_CASE]:
        inst, B, H, W, C0, C1, Cout, opt, kind = case
        d = cf.INSTANCES[inst]
        assert cf.instance_of(d['k'], d['s'], d['ups'], d['sub'], C0, C1, Cout) == inst, cf.case_id(case)
        assert cf.opt_set(case) <= set(cf.OPTION_WORDS) and kind in cf.KINDS and B in (1, 3)
        assert C0 % 4 == 0 and C1 % 4 == 0 and Cout % 4 == 0
        assert inst != '2x2i' or (H % 2 == 0 and W % 2 == 0)
        assert 'incoef' not in cf.opt_set(case) or (C1 == 0 and C0 % cf.PRO_GROUPS == 0 and inst not in cf.NO_PROLOGUE)
    for inst in cf.INSTANCES:
        mine = [c for c in cf.CASES if c[0] == inst]
        TH, TW = cf.INSTANCES[inst]['tile']
        for name, (H, W) in cf.geometries(inst).items():
            for B in ((1,) if name == 'deal' else (1, 3)):
                assert any(c[1:4] == (B, H, W) for c in mine), (inst, name, B)
        ho, wo = cf.out_hw(inst, *cf.geometries(inst)['px'])
        assert (ho, wo) == ((2, 2) if cf.INSTANCES[inst]['ups'] else (1, 1))
        gh, gw = cf.geometries(inst)['tile']
        assert (gh, gw) == (TH, TW) if inst == 'up2' else cf.out_hw(inst, gh, gw) == (TH, TW)
        for o in cf.options(inst):
            assert any(c[7] == o and c[1] == 3 for c in mine), (inst, o)
        assert ('stats' in cf.options(inst)) == (inst not in cf.NO_STATS)
        assert any({'incoef', 'inbound', 'rescoef'} <= cf.opt_set(c) for c in mine) == (inst not in cf.NO_PROLOGUE)
        for k, *_ in cf.kinds(inst):
            assert any(c[8] == k for c in mine), (inst, k)
        assert {c[8] for c in mine} >= {'perchan', 'zero-sample', 'outlier', 'tiny', 'huge'}
        if inst != '7x7p':
            assert {c[8] for c in mine} >= {'grow', 'shrink', 'zero-chunk'}
        if inst in cf.F16:
            wg = [cf.workgroups(c) for c in mine]
            assert any(n >= 8 and n % 8 and ct >= 2 for n, ct in wg), inst           # a re-deal with a ragged last round
            assert any(ct >= 2 and cf.out_hw(inst, c[2], c[3])[0] <= 32 for c, (n, ct) in zip(mine, wg))      # xcd == 2
            assert any(ct >= 2 and cf.out_hw(inst, c[2], c[3])[0] in (33, 34) for c, (n, ct) in zip(mine, wg))   # xcd == 1
    print(f'[yardstick] {len(cf.CASES)} cases: ' + ', '.join(f'{i} {sum(c[0] == i for c in cf.CASES)}' for i in cf.INSTANCES))


def test_chunk_scales():
    assert cf.chunk_scales('grow', 3, 0)[0] == pytest.approx([1e-4, 10 ** -0.5, 1e3])
    assert cf.chunk_scales('shrink', 2, 1) == ([pytest.approx(1e3), pytest.approx(10 ** -0.5)], [pytest.approx(1e-4)])
    assert cf.chunk_scales('jump01', 2, 1) == ([1e-3, 1e-3], [1e3])
    assert cf.chunk_scales('jump10', 2, 1) == ([1e3, 1e3], [1e-3])
    assert cf.chunk_scales('zero-chunk', 3, 0)[0] == [1.0, 0.0, 1.0]
    # s2d: the scale follows (pixel parity of the shifted view, 32 channels)
    x = cf._scaled(torch.ones((1, 64, 4, 6)), list(range(1, 9)), 's2dn')
    assert x[0, 0, 1, 1].item() == 1 and x[0, 40, 1, 1].item() == 2 and x[0, 0, 1, 0].item() == 3
    assert x[0, 0, 0, 1].item() == 5 and x[0, 63, 0, 0].item() == 8 and torch.equal(x[..., 2:, 2:4], x[..., :2, :2])


def test_stat_reference_tiles():
    """tile (srow, tx) = srow * tilesX + tx holds the sums of its own valid pixels; the bound is that of the docstring"""
    ref64 = torch.arange(2 * 4 * 9 * 17, dtype=torch.float64).reshape(2, 4, 9, 17) - 300
    g = torch.full((4,), 1e-5, dtype=torch.float64)
    ref, bound = cf.stat_reference(ref64, g)
    assert ref.shape == (2, 4, 4, 2)
    assert ref[1, 1, 2, 0].item() == ref64[1, 2, :8, 16:].sum().item()        # srow 0, tx 1: 8 x 1 pixels
    assert ref[0, 2, 3, 1].item() == (ref64[0, 3, 8:, :16] ** 2).sum().item()  # srow 1, tx 0: 1 x 16 pixels
    assert ref[..., 0].sum(1).eq(ref64.sum((2, 3))).all()
    S, n, m = ref64[:, 3].abs().max().item(), 16, 24
    gm = m * cf.U / (1 - m * cf.U)
    assert bound[0, 2, 3, 0].item() == pytest.approx(n * 1e-5 * S + gm * ref64[0, 3, 8:, :16].abs().sum().item(), rel=1e-12)
    assert bound[0, 2, 3, 1].item() == pytest.approx(2 * n * 1e-5 * S * S * (1 + 1e-5) + gm * ref[0, 2, 3, 1].item(), rel=1e-12)
    # a partial one slot off is outside the bound
    assert not bool(((ref.roll(1, 1) - ref).abs() <= bound).all())


@pytest.mark.parametrize('inst', cf.PROBE_INSTANCES)
def test_tap_probe_expectations_are_conv2d(inst):
    d = cf.INSTANCES[inst]
    k, s = d['k'], d['s']
    x = cf.probe_input(inst)
    assert bool((x != 0).all()) and torch.equal(x.half().float(), x)          # fp16-representable
    X = F.interpolate(x.double(), scale_factor=2, mode='nearest') if d['ups'] else x.double()
    pad = k // 2 if s == 1 else 1
    seen = set()
    for ky in range(k):
        for kx in range(k):
            want = F.conv2d(X, cf.probe_weight(inst, ky, kx).double(), None, s, pad)
            exp = cf.probe_expected(inst, x, ky, kx)
            assert exp.dtype == torch.float32 and torch.equal(exp.double(), want), (inst, ky, kx)
            seen.add(exp.numpy().tobytes())
    assert len(seen) == k * k                                                  # no two taps give the same picture


def test_mutations_miss_the_gates():
    """what a per-channel gate sees and a per-tensor rtol 1e-4 / atol 2e-5 (test_conv2d) does not: a dropped h2*g1 term (the
    second fp16 piece of the activations, 2^-11 of an operand) restated on the CPU on a `perchan` case — in the output
    channels whose weights are scaled by 1e-4 .. 1e-2 the whole error is below atol, and every one of them misses its gate"""
    case = next(c for c in cf.CASES if c[0] == '3x3n' and c[8] == 'perchan')
    r = cf.conv_reference(case)
    inp = dict(r['inp'])
    x = inp['x0']
    s = 2.0 ** (14 - torch.floor(torch.log2(x.abs().max())))                  # block maximum in [2^14, 2^15)
    inp['x0'] = (x * s).half().float() / s                                   # h1 alone
    bad = cf.conv_formula(inp, case[0], torch.float32)
    ratio = cf.chan_rel(bad, r['ref64']) / r['gate']
    small = torch.arange(case[6]) % 9 <= 2
    old_ok = ((bad - r['ref32']).abs() <= 2e-5 + 1e-4 * r['ref32'].abs()).all(0).all(-1).all(-1)     # per channel
    print(f'[mutation] {cf.case_id(case)}: activations cut to their first fp16 piece: err_c / gate_c = {ratio.min().item():.1f} .. '
          f'{ratio.max().item():.1f}; rtol 1e-4 / atol 2e-5 accepts {int(old_ok.sum())} of {old_ok.numel()} channels '
          f'({int(old_ok[small].sum())} of the {int(small.sum())} small-scale ones)')
    assert bool((ratio > 5).all()) and bool(old_ok[small].all())
