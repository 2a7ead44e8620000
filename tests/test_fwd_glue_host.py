"""CPU half of tests/test_gpu_fwd_glue.py: the references, yardsticks and bounds of tests/fwd_glue_cases.py hold on their own.

Every float64-gated case has its fp32 yardstick e32 computed here and held under CAP = 2e-5, so that no GPU gate exceeds
2e-4; the per-element bounds of dmh_final_conv_nchw, dmh_diff_mean and dmh_loss_combine accept the fp32 torch statement of
every case; the case tables reach the template arms they name; and wrong kernels restated on the CPU miss the gates, each by
the factor its [mutation] line prints."""
import numpy as np
import pytest
import torch

import fwd_glue_cases as fg


def _yardstick(name, ref64, ref32, may_be_zero=()):
    worst = 0.0
    for k, r64 in ref64.items():
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(ref32[k]).all()), f'{name} {k}: not finite'
        if k not in may_be_zero:
            assert r64.abs().max().item() > 0.0, f'{name} {k}: the reference is identically zero'
        e32 = fg.rel(ref32[k], r64)
        print(f'[yardstick] {name} {k}: e32={e32:.3e} gate={fg.gate(e32):.3e} ref_absmax={r64.abs().max().item():.3e}')
        assert e32 <= fg.CAP, f'{name} {k}: e32 = {e32:.3e} is over the cap {fg.CAP:.0e}: make the input milder'
        worst = max(worst, e32)
    return worst


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize('case', fg.LN_CASES, ids=fg.ln_id)
def test_layernorm_yardstick(case):
    C, bhw, kind = case
    r = fg.ln_reference(case)
    _yardstick('layernorm ' + fg.ln_id(case), r['ref64'], r['ref32'], may_be_zero=('out',) if kind == 'const' else ())
    x = r['inp']['x']
    if kind == 'const':        # every sum is exact: the float64 and the fp32 formula agree to the bit
        assert not r['ref64']['out'].any() and not r['ref32']['out'].any()
        assert torch.equal(r['ref32']['out_res'], r['inp']['res'])
        assert bool((r['ref32']['mean'] == 2.5).all()) and bool((r['ref64']['mean'] == 2.5).all())
        assert abs(r['ref64']['rstd'].max().item() - fg.EPS ** -0.5) < 1e-9
    if kind == 'offset30':
        ratio = (x.double().mean(-1).abs() / x.double().std(-1).clamp_min(1e-30)).median().item()
        assert 25.0 < ratio < 40.0 or C < 32, ratio
    if kind == 'scale1e-4':
        assert x.double().var(-1, unbiased=False).max().item() < fg.EPS


def test_layernorm_reference_is_the_oracle():
    """the float64 formula of fwd_glue_cases agrees with oracle.unet.chan_layernorm in float64 (which sets eps = 1e-3 there)"""
    from oracle import unet as OU
    for case in [(12, (3, 7, 9), 'unit'), (132, (3, 7, 9), 'offset30'), (516, (1, 5, 7), 'unit')]:
        inp = fg.ln_inputs(case)
        x, g = inp['x'].double(), inp['g'].double()
        mine = fg.ln_formula(x, g, eps=1e-3)[0]
        theirs = OU.chan_layernorm(x.permute(0, 3, 1, 2), g.reshape(1, -1, 1, 1)).permute(0, 2, 3, 1)
        e = fg.rel(mine, theirs)
        print(f'[yardstick] layernorm formula vs oracle.unet.chan_layernorm, float64, {fg.ln_id(case)}: {e:.3e}')
        assert e <= 1e-14
        assert fg.rel(fg.ln_formula(x, g)[0], theirs) > 1e-6     # (eps matters: the two calls above are not vacuous)


def test_layernorm_loop_case_yardstick():
    r = fg.ln_loop_reference()
    _yardstick('layernorm ' + fg.ln_id(fg.LN_LOOP_CASE), r['ref64'], r['ref32'])


# ------------------------------------------------------------------ GroupNorm + SiLU + residual
@pytest.mark.parametrize('case', fg.GS_CASES, ids=fg.gs_id)
def test_gn_silu_residual_yardstick(case):
    C, bhw, kind, with_res = case
    r = fg.gs_reference(case)
    _yardstick('gn_silu_residual ' + fg.gs_id(case), r['ref64'], r['ref32'])
    assert (r['inp']['res'] is not None) == with_res
    if kind == 'saturated':       # exp(-z) overflows fp32 above 88.73 on the negative side; sigmoid is 1 on the other
        zmin, zmax = r['z'].min().item(), r['z'].max().item()
        print(f'[yardstick] saturated z in [{zmin:.1f}, {zmax:.1f}]')
        assert zmin < -90.0 and zmax > 90.0


def test_gn_silu_residual_loop_case_yardstick():
    r = fg.gs_loop_reference()
    _yardstick('gn_silu_residual ' + fg.gs_id(fg.GS_LOOP_CASE), r['ref64'], r['ref32'])


# ------------------------------------------------------------------ the tables reach what they name
def test_case_tables_reach_every_arm():
    """nine <LPP, NV> arms of dmh_chan_layernorm and seven of dmh_pixel_stats, each full and ragged where it can be; the
    32-lane arm at an odd pixel count; both loops past their block caps; the four gn_silu_residual arms; eight Cout on both
    final-conv paths; four assemble templates and the generic kernel"""
    full = {arm[:2] for C in fg.LN_WIDTHS for arm in [fg.arm(C)] if not arm[2]}
    ragged = {arm[:2] for C in fg.LN_WIDTHS for arm in [fg.arm(C)] if arm[2]}
    assert full == set(fg.LN_LADDER), full
    assert ragged == set(fg.LN_LADDER), ragged
    assert fg.arm(4) == (2, 1, True) and fg.arm(8) == (2, 1, False)    # (C = 4: one idle lane per pixel of the 2-lane arm)
    ps_full = {a[:2] for C in fg.LN_WIDTHS for a in [fg.arm(C, fg.PS_LADDER)] if not a[2]}
    ps_ragged = {a[:2] for C in fg.LN_WIDTHS for a in [fg.arm(C, fg.PS_LADDER)] if a[2]}
    assert ps_full == set(fg.PS_LADDER) and ps_ragged == set(fg.PS_LADDER)
    assert sorted(C // 4 for C in fg.LN_WIDTHS if C // 4 % 2) == [1, 3, 5, 9, 17, 33, 65, 129, 257]
    assert {fg.arm(C)[:2] for C in fg.LN_KIND_WIDTHS} == {(4, 1), (16, 1), (64, 1), (64, 4)}
    npix = [B * H * W for B, H, W in fg.LN_PIX]
    assert npix == [1, 35, 189] and npix[2] % 2 == 1                  # 32 lanes per pixel: two pixels per wave, the last wave half used
    C, (B, H, W), _ = fg.LN_LOOP_CASE
    lpp = fg.arm(C)[0]
    assert B * H * W == fg.LN_BLOCK_CAP * (256 // lpp) + 3 and fg.arm(C, fg.PS_LADDER)[0] == lpp
    assert {C for C, *_ in fg.GS_CASES if C in fg.GS_STATS_ARM} == {64, 128, 256}
    C, (B, H, W), _, _ = fg.GS_LOOP_CASE
    blocks = -(-(B * H * W * C // 4) // 256)
    assert blocks == fg.GS_BLOCK_CAP + 1 and (B * H * W * C // 4) % 64 != 0    # one more round, ending inside a wave
    for path in (lambda C: C <= 64, lambda C: C > 64):
        assert {co for C, co in fg.FC_PAIRS if path(C)} == set(fg.FC_COUTS)
    assert {C for C, co in fg.FC_PAIRS if co == 6} == set(fg.FC_WIDTHS) == {C for C, co in fg.FC_PAIRS if co == 16}
    assert 68 // 4 == 17                                              # lane 0 walks two quads
    assert [R * H * W for R, H, W in fg.FC_PIX] == [1, 105, 378] and 35 % 16 and 189 % 16
    assert [c // 4 for c in fg.AS_CPADS] == [1, 2, 3, 4, 5, 6]
    for cpad in fg.AS_CPADS:
        (a0, b0), (a1, b1), (a2, b2) = fg.as_splits(cpad)
        assert a0 + b0 == cpad and a1 + b1 < cpad and b1 > 0 and b2 == 0 and min(a0, a1, a2) > 0
    assert [C * H * W for C, H, W in fg.DM_SHAPES] == [1, 255, 16384, 16385, 6 * 40 * 56]
    assert all(C > 1 for C, H, W in fg.DM_SHAPES[1:]) and max(fg.DM_B) > 64
    assert len(fg.EW_COMBOS) == 8 and fg.EW_PER == [1, 255, 257]


# ------------------------------------------------------------------ per-element bounds accept the fp32 statement
@pytest.mark.parametrize('pair', fg.FC_PAIRS, ids=fg.fc_id)
def test_final_conv_bound_accepts_fp32(pair):
    C, cout = pair
    for bhw in fg.FC_PIX:
        inp = fg.fc_inputs(C, cout, bhw)
        for bias in (inp['bias'], None):
            ref, bound = fg.fc_reference(inp['x'], inp['w'], bias)
            err = (fg.fc_fp32(inp['x'], inp['w'], bias).double() - ref).abs()
            assert bool((err <= bound).all()), (pair, bhw, (err / bound).max().item())
            assert ref.shape == (bhw[0], cout, bhw[1], bhw[2])


@pytest.mark.parametrize('case', fg.DM_CASES, ids=fg.dm_id)
def test_diff_mean_bound_accepts_fp32(case):
    inp = fg.dm_inputs(case)
    for m in (None, inp['m']):
        for squared in (False, True):
            ref, bound = fg.dm_reference(inp['a'], inp['b'], m, squared)
            assert bool((ref >= 0).all()) and ref.max().item() > 0      # (a masked-out single pixel: exactly 0, bound 0)
            err = (fg.dm_fp32(inp['a'], inp['b'], m, squared).double() - ref).abs()
            print(f'[yardstick] diff_mean {fg.dm_id(case)} mask={m is not None} squared={squared}: worst |err| / bound = '
                  f'{(err / bound).max().item():.3e}')
            assert bool((err <= bound).all())


def test_loss_combine_bound_accepts_fp32():
    for B in fg.LC_B:
        l, ph, w = fg.lc_inputs(B)
        ref, bound = fg.lc_reference(l, ph, w)
        assert abs(fg.lc_fp32(l, ph, w).double().item() - ref.item()) <= bound.item()


def test_uint8_table():
    tab = fg.u8_table()
    assert tab.shape == (770,) and np.unique(tab).shape == (770,)
    prod = tab * np.float32(255)
    k = np.arange(256)
    exact = np.nonzero(prod[256:512] == k)[0]                # fl(fl(k / 255) * 255) lands exactly on k ...
    below = np.nonzero(prod[256:512] < k)[0]                 # ... or just under it, where truncation gives k - 1
    print(f'[yardstick] uint8 table: {exact.size} of 256 products fl(fl(k/255) * 255) are exactly k, {below.size} fall below k')
    assert exact.size >= 128 and exact.size + below.size + np.count_nonzero(prod[256:512] > k) == 256
    ref = fg.u8_reference(tab)
    assert np.array_equal(ref[256:512][exact], k[exact].astype(np.uint8))
    assert np.array_equal(ref[:256][exact[exact > 0]], (k[exact[exact > 0]] - 1).astype(np.uint8))   # the lower neighbour truncates to k - 1
    assert ref[768] == 127 and ref[0] == 0 and ref[767] == 255


def test_embedding_references():
    """the float64 references are the sines of the fp32 arguments: fp32 torch evaluates them within the gate, and at
    t = 123456 the argument product formed in float64 instead lies far outside it"""
    for dim in fg.SIN_DIMS:
        t, f = fg.emb_times(37), fg.sin_freq(dim)
        ref = fg.sin_reference(t, f)
        arg = t.float()[:, None] * f[None, :]
        assert (torch.cat([arg.sin(), arg.cos()], 1).double() - ref).abs().max().item() <= fg.EMBED_ATOL
        assert ref.shape == (37, dim) and {0, 1, 999, 123456} <= set(t.tolist())
    wrong = (t.double()[:, None] * f.double()[None, :]).sin()
    assert (wrong - ref[:, :f.shape[0]]).abs().max().item() > 100 * fg.EMBED_ATOL
    for half in fg.FOURIER_HALVES:
        ref = fg.fourier_reference(fg.emb_times(5), fg.rand((half,), 18500 + half))
        assert ref.shape == (5, 2 * half + 1) and ref[:, 0].tolist() == [123456.0, 0.0, 1.0, 999.0, ref[4, 0].item()]


# ------------------------------------------------------------------ wrong kernels miss
def _miss(name, bad, ref64, ref32):
    """-> by how many times its gate the wrong result misses"""
    f = fg.rel(bad, ref64) / fg.gate(fg.rel(ref32, ref64))
    print(f'[mutation] {name}: misses its gate by {f:.3g}x')
    return f


def test_gates_reject_a_layernorm_without_its_last_quad():
    """a LayerNorm whose lanes drop the last channel quad where C/4 is off the arm's lane count: the quad enters neither sum
    and is not written (it keeps the prefilled zero).  Measured: out misses its gate 1.1e5 ... 1.6e5 times, mean 2.8e3 ... 1.2e5
    times, rstd 1.6e3 ... 2.1e5 times (the smallest at C = 1028, where one quad is 1 / 257 of the pixel)"""
    for C in (12, 20, 36, 68, 132, 260, 516, 1028):
        case = (C, fg.LN_PIX[2], 'unit')
        assert fg.arm(C)[2]
        r = fg.ln_reference(case)
        x = r['inp']['x'].clone()
        x[..., C - 4:] = 0.0
        mean = x.sum(-1, keepdim=True) / C
        d = x - mean
        d[..., C - 4:] = 0.0
        rstd = ((d * d).sum(-1, keepdim=True) / C + fg.EPS).rsqrt()
        out = d * rstd * r['inp']['g']
        f = [_miss(f'LayerNorm without its last quad, C = {C}: {k}', v, r['ref64'][k], r['ref32'][k])
             for k, v in (('out', out), ('mean', mean[..., 0]), ('rstd', rstd[..., 0]))]
        assert min(f) >= 100.0, (C, f)


def test_gates_reject_a_one_pass_variance():
    """var = E[x^2] - mean^2 in fp32 at mean = 30 standard deviations: the cancellation costs (mean / std)^2 = 900 roundings.
    Measured: out misses its gate 6.5 ... 12.6 times, rstd 24 ... 60 times (the gate of out is 10 x the two-pass fp32 error at
    this mean, itself 1.9e-6 ... 3.1e-6)"""
    for C in fg.LN_KIND_WIDTHS:
        r = fg.ln_reference((C, fg.LN_PIX[2], 'offset30'))
        x, g = r['inp']['x'], r['inp']['g']
        mean = x.mean(-1, keepdim=True)
        rstd = ((x * x).mean(-1, keepdim=True) - mean * mean + fg.EPS).rsqrt()
        out = (x - mean) * rstd * g
        fo = _miss(f'one-pass variance at mean = 30 std, C = {C}: out', out, r['ref64']['out'], r['ref32']['out'])
        fr = _miss(f'one-pass variance at mean = 30 std, C = {C}: rstd', rstd[..., 0], r['ref64']['rstd'], r['ref32']['rstd'])
        assert fo > 1.0 and fr > 1.0, (C, fo, fr)


def test_bounds_reject_a_final_conv_that_stops_at_16_quads():
    """the C <= 64 path taken at C > 64: channels 64 and up never enter.  Measured: the worst element is 1.2e4 ... 4.2e4 times
    its bound, every element over it"""
    for C in (68, 128, 320):
        inp = fg.fc_inputs(C, 6, fg.FC_PIX[1])
        ref, bound = fg.fc_reference(inp['x'], inp['w'], inp['bias'])
        bad = fg.fc_fp32(inp['x'][..., :64], inp['w'][:, :64], inp['bias'])
        ratio = ((bad.double() - ref).abs() / bound)
        print(f'[mutation] final conv that stops at 16 quads, C = {C}: worst element {ratio.max().item():.3g}x its bound, '
              f'{(ratio > 1).double().mean().item():.1%} of the elements over it')
        assert ratio.max().item() >= 100.0 and (ratio > 1).double().mean().item() > 0.9


def test_bounds_reject_a_diff_mean_mask_indexed_by_element():
    """m[s * HW + i] instead of m[s * HW + i % HW] (restated with the index wrapped at the end of the mask).  Measured: the
    worst sample is 4.3e4 ... 8.5e5 times its bound, every sample over it"""
    for case in fg.DM_CASES:
        (C, H, W), B = case
        inp = fg.dm_inputs(case)
        for squared in (False, True):
            ref, bound = fg.dm_reference(inp['a'], inp['b'], inp['m'], squared)
            bad = fg.dm_fp32(inp['a'], inp['b'], inp['m'], squared, mask_index_wraps=True)
            if C == 1:      # i % HW == i: the wrong index is the right one
                assert bool(((bad.double() - ref).abs() <= bound).all())
                continue
            ratio = (bad.double() - ref).abs() / bound
            print(f'[mutation] diff_mean mask indexed by i, {fg.dm_id(case)} squared={squared}: worst sample '
                  f'{ratio.max().item():.3g}x its bound, {int((ratio > 1).sum())} of {B} samples over it')
            assert ratio.max().item() >= 100.0 and int((ratio > 1).sum()) >= B - 1
    # (sample 0 reads its own mask for the first HW elements only)


def test_table_rejects_a_uint8_export_that_rounds():
    """measured: 257 of the 770 entries differ (the lower neighbour of every k / 255 with k >= 1, 0.5 and 0.999999)"""
    tab = fg.u8_table()
    wrong = int((fg.u8_reference(tab, nearest=True) != fg.u8_reference(tab)).sum())
    print(f'[mutation] uint8 export that rounds to nearest: {wrong} of {tab.size} table entries differ')
    assert wrong >= 256
