"""-m gpu: the forward-path glue kernels between the matrix-core kernels, each ALONE through the C ABI — dmh_chan_layernorm,
dmh_pixel_stats, dmh_gn_silu_residual(_stats) and dmh_gn_finalize(_bound) of csrc/norm.hip; dmh_final_conv_nchw,
dmh_assemble_input, dmh_diff_mean, dmh_loss_combine, the elementwise kernels, dmh_to_uint8 and dmh_sampler_seek of
csrc/sampler.hip; the embeddings and table gathers of csrc/embed.hip — against the plain operation in float64 on the CPU, or
bit for bit against fp32 torch / numpy where the kernel keeps that op order.  Cases, references and gates:
tests/fwd_glue_cases.py (its yardsticks and bounds are held on the CPU by tests/test_fwd_glue_host.py).  The older tests of
tests/test_gpu_kernels.py stay; where one covers a case exactly it is cited.  Every assertion prints a [parity] line."""
import ctypes as C

import numpy as np
import pytest
import torch

import fwd_glue_cases as fg
from gpu_util import dev, rand

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope='module')
def ops():
    from dmhomo_amd import ops as _ops
    _ops.lib()
    return _ops


def _d(t):
    return None if t is None else t.to(dev()).contiguous()


def _within(name, got, ref, bound):
    """elementwise |got - ref| <= bound, printing the worst ratio"""
    got = got.double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f'{name}: not finite'
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    print(f'[parity] {name}: worst |err| / bound = {ratio.max().item():.3e} (max_abs={err.max().item():.3e}, bound there '
          f'{bound.flatten()[ratio.argmax()].item():.3e})')
    bad = (err > bound).nonzero()
    assert bad.shape[0] == 0, f'{name}: {bad.shape[0]} elements over their bound, first at {bad[0].tolist()}: ' \
                             f'err {err[tuple(bad[0])].item():.3e} > {bound[tuple(bad[0])].item():.3e}'


def _bitwise(name, got, want):
    """got == want bit for bit (NaN == NaN: compared as integers), printing the mismatch count"""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    view = {4: torch.int32, 8: torch.int64, 1: torch.uint8}[got.element_size()]
    bad = int((got.view(view) != want.view(view)).sum())
    print(f'[parity] {name}: {bad} of {got.numel()} elements differ bitwise, allowed 0')
    assert bad == 0, name


def _pixel_stats(ops, x, rows=None, out=None):
    B, H, W, Cc = x.shape
    st = torch.full((B, H * W, 2), float('nan'), device=x.device) if out is None else out
    ops.call('dmh_pixel_stats', ops.ptr(x), ops.ptr(st), B * H * W, Cc, fg.EPS, ops.ptr(rows, torch.int32), H * W)
    return st


# ------------------------------------------------------------------ dmh_chan_layernorm / dmh_pixel_stats
def _ln_run(ops, tag, r, kind):
    inp, ref64, ref32 = r['inp'], r['ref64'], r['ref32']
    x, g, res = _d(inp['x']), _d(inp['g']), _d(inp['res'])
    out = ops.chan_layernorm(x, g, eps=fg.EPS)
    out_res = ops.chan_layernorm(x, g, res=res, eps=fg.EPS)
    st = _pixel_stats(ops, x).reshape(*x.shape[:3], 2)
    fg.check(f'chan_layernorm {tag} out', out, ref64['out'], ref32['out'])
    fg.check(f'chan_layernorm {tag} out+res', out_res, ref64['out_res'], ref32['out_res'])
    fg.check(f'pixel_stats {tag} mean', st[..., 0], ref64['mean'], ref32['mean'])
    fg.check(f'pixel_stats {tag} rstd', st[..., 1], ref64['rstd'], ref32['rstd'])
    assert torch.equal(x.cpu(), inp['x']) and torch.equal(res.cpu(), inp['res'])
    return out, out_res, st


@pytest.mark.parametrize('case', fg.LN_CASES, ids=fg.ln_id)
def test_chan_layernorm_and_pixel_stats(ops, case):
    """every <LPP, NV> arm of both ladders, full and with C/4 off the arm's lane count, at 1, 35 and 189 pixels; out, out + res,
    mean and rstd within max(5e-6, 10 * e32) of float64.  The constant kind is a known answer: every sum is exact, so out is
    exactly 0, out + res exactly res and mean exactly 2.5 (rstd within the gate of 1 / sqrt(eps)).
    (test_chan_layernorm of tests/test_gpu_kernels.py keeps C = 8, 64, 128, 512 at 126 pixels against the oracle.)"""
    C_, bhw, kind = case
    out, out_res, st = _ln_run(ops, fg.ln_id(case), fg.ln_reference(case), kind)
    if kind == 'const':
        nz, nr, nm = int(torch.count_nonzero(out)), int((out_res.cpu() != fg.ln_reference(case)['inp']['res']).sum()), \
            int((st[..., 0] != 2.5).sum())
        print(f'[parity] chan_layernorm {fg.ln_id(case)}: {nz} outputs not exactly 0, {nr} not exactly res, {nm} means not '
              f'exactly 2.5; allowed 0')
        assert nz == 0 and nr == 0 and nm == 0


def test_chan_layernorm_and_pixel_stats_grid_stride(ops):
    """C = 132 (4 pixels per block) at 65536 + 3 pixels: the 16384-block cap is reached and block 0 walks a second round.  The
    last three pixels are held to the gate on their own scale, as the first three are"""
    r = fg.ln_loop_reference()
    tag = fg.ln_id(fg.LN_LOOP_CASE)
    out, out_res, st = _ln_run(ops, tag, r, 'unit')
    for name, sl in (('first 3 pixels', slice(0, 3)), ('last 3 pixels', slice(-3, None))):
        for key, got in (('out', out), ('out_res', out_res)):
            fg.check(f'chan_layernorm {tag} {key}, {name}', got[0, sl], r['ref64'][key][0, sl], r['ref32'][key][0, sl])
        for i, key in enumerate(('mean', 'rstd')):
            fg.check(f'pixel_stats {tag} {key}, {name}', st[0, sl, 0, i], r['ref64'][key][0, sl, 0], r['ref32'][key][0, sl, 0])


# ------------------------------------------------------------------ dmh_gn_silu_residual / dmh_gn_silu_residual_stats
def _gs_run(ops, tag, r, C_):
    inp, ref64, ref32 = r['inp'], r['ref64'], r['ref32']
    y, coef, res = _d(inp['y']), _d(inp['coef']), _d(inp['res'])
    out = ops.gn_silu_residual(y, coef, res)
    fg.check(f'gn_silu_residual {tag} out', out, ref64['out'], ref32['out'])
    st = None
    if C_ in fg.GS_STATS_ARM:
        out2, st = ops.gn_silu_residual(y, coef, res, pixel_stats=True, eps=fg.EPS)
        st = st.reshape(*y.shape[:3], 2)
        fg.check(f'gn_silu_residual_stats {tag} out', out2, ref64['out'], ref32['out'])
        fg.check(f'gn_silu_residual_stats {tag} mean', st[..., 0], ref64['mean'], ref32['mean'])
        fg.check(f'gn_silu_residual_stats {tag} rstd', st[..., 1], ref64['rstd'], ref32['rstd'])
        _bitwise(f'gn_silu_residual_stats {tag} out vs the plain launch', out2, out)
    return out, st


@pytest.mark.parametrize('case', fg.GS_CASES, ids=fg.gs_id)
def test_gn_silu_residual(ops, case):
    """SiLU(a * y + b) (+ res) at any C % 4 == 0, and at C = 64 / 128 / 256 the <16 / 32 / 64> statistics arms (out, mean, rstd
    against float64; test_gn_silu_residual_pixel_stats_bitwise of tests/test_gpu_kernels.py keeps the bitwise comparison with
    dmh_pixel_stats).  Saturated: |z| reaches 95 on both sides — the output stays finite (fg.check turns a non-finite output
    into an infinite error), is below 95 exp(-90) < 1e-37 in magnitude where z < -90, and within 3 u of z where z > 90 (the
    rounding of the fma, and the hardware reciprocal's one ulp = 2 u)"""
    C_, bhw, kind, with_res = case
    r = fg.gs_reference(case)
    out, _ = _gs_run(ops, fg.gs_id(case), r, C_)
    if kind == 'saturated':
        z = r['z']
        res = r['inp']['res'].double() if with_res else torch.zeros_like(z)
        act = out.double().cpu() - res           # (with res: out = fl(SiLU + res), one more rounding of |res| + 95)
        lo, hi = z < -90.0, z > 90.0
        slack = fg.U * (res.abs() + fg.GS_SATURATED_AT * 2)
        e_lo = (act[lo].abs() - slack[lo] * with_res).max().item()
        e_hi = ((act[hi] - z[hi]).abs() - slack[hi] * with_res - 3 * fg.U * z[hi].abs()).max().item()
        print(f'[parity] gn_silu_residual {fg.gs_id(case)}: {int(lo.sum())} elements at z < -90, worst |SiLU| over its allowance '
              f'{e_lo:.3e} (allowed 1e-37); {int(hi.sum())} at z > 90, worst |SiLU - z| over 3 u |z| {e_hi:.3e} (allowed 0)')
        assert int(lo.sum()) > 0 and int(hi.sum()) > 0 and e_lo <= 1e-37 and e_hi <= 0.0


def test_gn_silu_residual_past_the_block_cap(ops):
    """C = 64, 131072 + 5 pixels with statistics: 8193 blocks' worth of quads on 8192 blocks — block 0 walks a second round that
    ends inside a wave (clamped index, guarded store).  The last pixel's output and statistics are held to the gate alone"""
    r = fg.gs_loop_reference()
    tag = fg.gs_id(fg.GS_LOOP_CASE)
    out, st = _gs_run(ops, tag, r, 64)
    for name, sl in (('first pixel', slice(0, 1)), ('last pixel', slice(-1, None))):
        fg.check(f'gn_silu_residual_stats {tag} out, {name}', out[0, sl], r['ref64']['out'][0, sl], r['ref32']['out'][0, sl])
        for i, key in enumerate(('mean', 'rstd')):
            fg.check(f'gn_silu_residual_stats {tag} {key}, {name}', st[0, sl, 0, i], r['ref64'][key][0, sl, 0],
                     r['ref32'][key][0, sl, 0])
    _bitwise(f'gn_silu_residual_stats {tag} stats vs dmh_pixel_stats(out)', st.reshape(1, -1, 2), _pixel_stats(ops, out))


# ------------------------------------------------------------------ row subsets, strided ss
def _gn_stats(y, tiles):
    """per-tile (sum, sum of squares) of y (B, HW, C) in fp32, as a producing conv would write them: (B, tiles, C, 2)"""
    parts = torch.tensor_split(y, tiles, dim=1)
    return torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], -1) for p in parts], 1).contiguous()


def _subset(name, got, full, keep):
    for b, k in enumerate(keep):
        if k:
            _bitwise(f'{name}: kept row {b} vs the full launch', got[b], full[b])
        else:
            n = int((got[b] != SENTINEL).sum())
            print(f'[parity] {name}: dropped row {b}: {n} of {got[b].numel()} sentinels overwritten, allowed 0')
            assert n == 0, name


@pytest.mark.parametrize('C_', [12, 64, 132])
def test_row_subset_writes_only_its_rows(ops, C_):
    """B = 3 with rows_from_keep([1, 0, 1]) and sentinel-filled outputs: the kept rows are bitwise the full launch's rows and
    the dropped row keeps its sentinel — dmh_chan_layernorm, dmh_pixel_stats, dmh_gn_silu_residual (at C = 64 also _stats),
    dmh_gn_finalize and dmh_gn_finalize_bound"""
    B, H, W, groups, tiles = 3, 5, 7, 4, 3
    keep = [1, 0, 1]
    rows = ops.rows_from_keep(torch.tensor(keep, dtype=torch.uint8, device=dev()))
    assert rows[:3].tolist() == [2, 0, 2]
    rp = ops.ptr(rows, torch.int32)
    x, res = _d(rand((B, H, W, C_), 19000 + C_)), _d(rand((B, H, W, C_), 19001 + C_))
    g = _d(1 + 0.2 * rand((C_,), 19002))
    coef = _d(torch.stack([1 + 0.2 * rand((B, C_), 19003), 0.3 * rand((B, C_), 19004)], 1))
    fill = lambda *shape: torch.full(shape, SENTINEL, device=dev())
    tag = f'rows C={C_}'

    out = fill(B, H, W, C_)
    ops.call('dmh_chan_layernorm', ops.ptr(x), ops.ptr(g), ops.ptr(res), ops.ptr(out), B * H * W, C_, fg.EPS, rp, H * W)
    _subset(f'{tag} chan_layernorm', out, ops.chan_layernorm(x, g, res=res, eps=fg.EPS), keep)
    _subset(f'{tag} pixel_stats', _pixel_stats(ops, x, rows=rows, out=fill(B, H * W, 2)), _pixel_stats(ops, x), keep)

    out = fill(B, H, W, C_)
    ops.call('dmh_gn_silu_residual', ops.ptr(x), ops.ptr(coef), ops.ptr(res), ops.ptr(out), B, H * W, C_, rp)
    _subset(f'{tag} gn_silu_residual', out, ops.gn_silu_residual(x, coef, res), keep)
    if C_ in fg.GS_STATS_ARM:
        out, st = fill(B, H, W, C_), fill(B, H * W, 2)
        ops.call('dmh_gn_silu_residual_stats', ops.ptr(x), ops.ptr(coef), ops.ptr(res), ops.ptr(out), ops.ptr(st), B, H * W, C_,
                 fg.EPS, rp)
        full = ops.gn_silu_residual(x, coef, res, pixel_stats=True, eps=fg.EPS)
        _subset(f'{tag} gn_silu_residual_stats out', out, full[0], keep)
        _subset(f'{tag} gn_silu_residual_stats stats', st, full[1], keep)

    stats = _d(_gn_stats(x.reshape(B, H * W, C_).cpu(), tiles))
    beta, ss = _d(0.2 * rand((C_,), 19005)), _d(0.3 * rand((B, 2 * C_), 19006))
    full_coef, full_bound = ops.gn_finalize(stats, g, beta, H * W, groups, ss=ss, eps=fg.EPS, want_bound=True)
    _bitwise(f'{tag} gn_finalize vs gn_finalize_bound', ops.gn_finalize(stats, g, beta, H * W, groups, ss=ss, eps=fg.EPS), full_coef)
    co = fill(B, 2, C_)
    ops.call('dmh_gn_finalize', ops.ptr(stats), tiles, ops.ptr(g), ops.ptr(beta), ops.ptr(ss), 2 * C_, ops.ptr(co), B, C_, groups,
             H * W, fg.EPS, rp)
    _subset(f'{tag} gn_finalize', co, full_coef, keep)
    co, bd = fill(B, 2, C_), fill(B, groups)
    ops.call('dmh_gn_finalize_bound', ops.ptr(stats), tiles, ops.ptr(g), ops.ptr(beta), ops.ptr(ss), 2 * C_, ops.ptr(co),
             ops.ptr(bd), B, C_, groups, H * W, fg.EPS, rp)
    _subset(f'{tag} gn_finalize_bound coef', co, full_coef, keep)
    _subset(f'{tag} gn_finalize_bound bound', bd, full_bound, keep)


@pytest.mark.parametrize('C_', [12, 64, 132])
def test_gn_finalize_strided_ss(ops, C_):
    """ss passed as a column view of a wider matrix (row stride 2C + 12, starting 5 floats into a row): bitwise the contiguous
    ss.  (The numerics of the finalize arithmetic: test_gn_finalize_train of tests/test_gpu_norm_backward.py.)"""
    B, HW, groups, tiles = 3, 35, 4, 3
    stats = _d(_gn_stats(rand((B, HW, C_), 19100 + C_), tiles))
    g, beta = _d(1 + 0.2 * rand((C_,), 19101)), _d(0.2 * rand((C_,), 19102))
    ss = _d(0.3 * rand((B, 2 * C_), 19103))
    wide = torch.full((B, 2 * C_ + 12), SENTINEL, device=dev())
    wide[:, 5:5 + 2 * C_] = ss
    view = wide[:, 5:5 + 2 * C_]
    assert view.stride() == (2 * C_ + 12, 1) and not view.is_contiguous()
    want, want_bound = ops.gn_finalize(stats, g, beta, HW, groups, ss=ss, eps=fg.EPS, want_bound=True)
    _bitwise(f'gn_finalize C={C_} strided ss', ops.gn_finalize(stats, g, beta, HW, groups, ss=view, eps=fg.EPS), want)
    got, got_bound = ops.gn_finalize(stats, g, beta, HW, groups, ss=view, eps=fg.EPS, want_bound=True)
    _bitwise(f'gn_finalize_bound C={C_} strided ss coef', got, want)
    _bitwise(f'gn_finalize_bound C={C_} strided ss bound', got_bound, want_bound)
    none = ops.gn_finalize(stats, g, beta, HW, groups, eps=fg.EPS)
    assert not torch.equal(none, want)       # (ss is read at all)


# ------------------------------------------------------------------ dmh_final_conv_nchw
@pytest.mark.parametrize('pair', fg.FC_PAIRS, ids=fg.fc_id)
def test_final_conv_nchw(ops, pair):
    """every Cout instantiation on both paths (C <= 64: a lane owns one quad, lanes past C/4 none; C > 64: the strided quad
    loop), 1 / 105 / 378 pixels, with and without bias: every element within (C + 2) u (sum |x w| + |bias|) of float64; the
    output is prefilled with NaN, so an element the kernel does not write fails too"""
    C_, cout = pair
    for bhw in fg.FC_PIX:
        R, H, W = bhw
        inp = fg.fc_inputs(C_, cout, bhw)
        x, w = _d(inp['x']), _d(inp['w'])
        for bias in (inp['bias'], None):
            ref, bound = fg.fc_reference(inp['x'], inp['w'], bias)
            out, bd = torch.full((R, cout, H, W), float('nan'), device=dev()), _d(bias)
            ops.call('dmh_final_conv_nchw', ops.ptr(x), ops.ptr(w), ops.ptr(bd), ops.ptr(out), R, H * W, C_, cout)
            _within(f'final_conv {fg.fc_id(pair)} {fg.hw_id(bhw)} {"bias" if bias is not None else "nobias"}', out, ref, bound)


def test_final_conv_nchw_refuses_cout_5(ops):
    from dmhomo_amd._lib import DmhError
    x, w = torch.zeros((1, 2, 2, 64), device=dev()), torch.zeros((5, 64), device=dev())
    with pytest.raises(DmhError, match='unsupported Cout=5'):
        ops.final_conv_nchw(x, w, None)


# ------------------------------------------------------------------ dmh_assemble_input
@pytest.mark.parametrize('cpad', fg.AS_CPADS, ids=fg.as_id)
def test_assemble_input(ops, cpad):
    """the four per-pixel templates and the generic kernel: Ca + Cb == Cpad and < Cpad, Cb = 0 with b = None, mask absent and
    present, reps 1 and 3, HW 1 and 99 — bit for bit torch.cat((a, b * m, zeros)) repeated, NHWC, into a NaN-filled output.
    (test_assemble_and_final_conv of tests/test_gpu_kernels.py keeps Cpad = 12, Ca = 6, Cb = 3 with a mask at reps = 2.)"""
    for ca, cb in fg.as_splits(cpad):
        for hw in fg.AS_HW:
            inp = fg.as_inputs(cpad, ca, cb, hw)
            for m in (None, inp['m']):
                for reps in fg.AS_REPS:
                    out = torch.full((reps * fg.AS_B, hw[0], hw[1], cpad), float('nan'), device=dev())
                    ops.assemble_input(_d(inp['a']), _d(inp['b']), _d(m), reps=reps, cpad=cpad, out=out)
                    _bitwise(f'assemble_input {fg.as_id(cpad)} Ca={ca} Cb={cb} HW={hw[0] * hw[1]} mask={m is not None} reps={reps}',
                             out, fg.as_reference(inp['a'], inp['b'], m, reps, cpad))


# ------------------------------------------------------------------ dmh_diff_mean / dmh_loss_combine
@pytest.mark.parametrize('case', fg.DM_CASES, ids=fg.dm_id)
def test_diff_mean(ops, case):
    """per-sample mean of m * |a - b| / m * (a - b)^2 within 6 u of float64, with the f64 workspace prefilled with NaN: a
    partial block that owns no element (C * HW < 16129) must still write its zero.  With C > 1 the mask is read at i % HW"""
    (C_, H, W), B = case
    inp = fg.dm_inputs(case)
    a, b = _d(inp['a']), _d(inp['b'])
    for m in (None, inp['m']):
        md = _d(m)
        for squared in (False, True):
            ws = torch.full((B, 64), float('nan'), device=dev(), dtype=torch.float64)
            out = torch.full((B,), float('nan'), device=dev())
            ops.call('dmh_diff_mean', ops.ptr(a), ops.ptr(b), ops.ptr(md), int(squared), ops.ptr(ws, torch.float64),
                     ops.ptr(out), B, C_, H * W)
            ref, bound = fg.dm_reference(inp['a'], inp['b'], m, squared)
            name = f'diff_mean {fg.dm_id(case)} {"mask" if m is not None else "nomask"} {"L2" if squared else "L1"}'
            _within(name, out, ref, bound)
            empty = int((ws == 0).sum())
            print(f'[parity] {name}: {int(torch.isnan(ws).sum())} workspace slots left NaN, allowed 0 ({empty} hold zero)')
            assert not bool(torch.isnan(ws).any())
            if m is None and C_ * H * W < 63 * 256:
                assert empty >= B * (64 - -(-C_ * H * W // 256))


@pytest.mark.parametrize('B', fg.LC_B)
def test_loss_combine(ops, B):
    l, ph, w = fg.lc_inputs(B)
    out, ld, pd, wd = torch.full((1,), float('nan'), device=dev()), _d(l), _d(ph), _d(w)
    ops.call('dmh_loss_combine', ops.ptr(ld), ops.ptr(pd), ops.ptr(wd), ops.ptr(out), B)
    ref, bound = fg.lc_reference(l, ph, w)
    _within(f'loss_combine B={B}', out, ref.reshape(1), bound.reshape(1))


# ------------------------------------------------------------------ elementwise kernels, bit-exact
@pytest.mark.parametrize('per', fg.EW_PER)
def test_rows_lincomb_q_sample_affine(ops, per):
    """csrc/sampler.hip compiles with contraction off: bit for bit fp32 torch in the same op order.  dmh_rows_lincomb in all
    eight y / div / clamp combinations with values on both sides of +-1, dmh_q_sample and dmh_affine at B = 3 with 1, 255 and
    257 elements per sample, dmh_affine_tail at c0 = 0 and C - 1.  (test_affine_uint8_qsample of tests/test_gpu_kernels.py
    keeps one 2 x 6 x 5 x 5 case of each.)"""
    inp = fg.ew_inputs(per)
    x, y, ca, cb, dv = (inp[k] for k in ('x', 'y', 'ca', 'cb', 'dv'))
    assert per == 1 or (x.abs() > 1).any() and (x.abs() < 1).any()
    for with_y, with_div, clamp in fg.EW_COMBOS:
        got = ops.rows_lincomb(_d(x), _d(ca), y=_d(y) if with_y else None, cb=_d(cb) if with_y else None,
                               div=_d(dv) if with_div else None, clamp=clamp)
        want = fg.lincomb_fp32(x, ca, y if with_y else None, cb, dv if with_div else None, clamp)
        _bitwise(f'rows_lincomb per={per} y={with_y} div={with_div} clamp={clamp}', got, want)
    _bitwise(f'q_sample per={per}', ops.q_sample(_d(x), _d(y), _d(ca), _d(cb)), ca[:, None] * x + cb[:, None] * y)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)      # (the kernels receive their scalars as fp32)
    _bitwise(f'affine per={per}', ops.affine(_d(x), 0.37, -1.3), x * f32(0.37) + f32(-1.3))
    Cc = 3
    t = rand((fg.EW_B, Cc, per, 1), 17500 + per)
    for c0 in (0, Cc - 1):
        want = t.clone()
        want[:, c0:] = want[:, c0:] * f32(1.7) + f32(0.21)
        _bitwise(f'affine_tail per={per} c0={c0}', ops.affine_tail_(_d(t.clone()), c0, 1.7, 0.21), want)


def test_to_uint8_table(ops):
    """every k / 255 in fp32 with its two fp32 neighbours (and 0.5, 0.999999): numpy's fp32 product truncated to uint8"""
    tab = fg.u8_table()
    got = ops.to_uint8(torch.from_numpy(tab).to(dev())).cpu().numpy()
    want = fg.u8_reference(tab)
    bad = int((got != want).sum())
    print(f'[parity] to_uint8: {bad} of {tab.size} table entries differ, allowed 0')
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ dmh_sampler_seek
def test_sampler_seek(ops):
    """k = -1 advances and stays at S - 1, an explicit k jumps; cur is byte for byte table[cursor] and tcond (B = 130: the
    64-lane fill loops) is times[cursor] everywhere"""
    from dmhomo_amd._lib import DmhStep
    S, B = 5, 130
    steps = [DmhStep(objective=i % 3, clip=i % 2, mode=ops.MODE_LAST if i == S - 1 else ops.MODE_DDIM, cond_scale=1.5 + i,
                     sqrt_recip_ac=1.1 + 0.01 * i, sqrt_recipm1_ac=0.4 + 0.03 * i, sqrt_ac=0.9 - 0.02 * i,
                     sqrt_1m_ac=0.3 + 0.05 * i, c0=0.83 + i, c1=0.41 - i, c2=0.37 * (i + 1)) for i in range(S)]
    times = [999, 750, 500, 123456789012, 0]
    table, tt, cursor, cur = ops.step_table(steps, times, dev())
    sz = C.sizeof(DmhStep)
    assert table.shape == (S * sz,) and cur.shape == (sz,)
    tcond = torch.full((B,), -1, dtype=torch.int64, device=dev())
    for k, want in ((0, 0), (-1, 1), (-1, 2), (4, 4), (-1, 4), (-1, 4), (1, 1), (-1, 2), (-1, 3), (3, 3)):
        cur.fill_(255)
        tcond.fill_(-1)
        ops.sampler_seek(cursor, k, table, tt, cur, tcond)
        c = int(cursor.item())
        bad_cur = int((cur != table[want * sz:(want + 1) * sz]).sum())
        bad_t = int((tcond != times[want]).sum())
        print(f'[parity] sampler_seek k={k}: cursor {c} (expected {want}), {bad_cur} of {sz} bytes of cur differ, '
              f'{bad_t} of {B} tcond entries differ; allowed 0')
        assert c == want and bad_cur == 0 and bad_t == 0
    assert torch.equal(table.cpu(), ops.step_table(steps, times, dev())[0].cpu())     # (the table itself is only read)


# ------------------------------------------------------------------ embeddings
@pytest.mark.parametrize('R', fg.EMB_ROWS)
@pytest.mark.parametrize('dim', fg.SIN_DIMS)
def test_sinusoidal_embed(ops, dim, R):
    """(test_embeddings of tests/test_gpu_kernels.py keeps dim = 64 at four rows against the oracle)"""
    t, f = fg.emb_times(R), fg.sin_freq(dim)
    out, td, fd = torch.full((R, dim), float('nan'), device=dev()), _d(t), _d(f)
    ops.call('dmh_sinusoidal_embed', ops.ptr(td, torch.int64), ops.ptr(fd), ops.ptr(out), R, dim)
    err = (out.double().cpu() - fg.sin_reference(t, f)).abs().max().item()
    print(f'[parity] sinusoidal_embed dim={dim} R={R}: max_abs={err:.3e} allowed {fg.EMBED_ATOL:.1e}')
    assert err <= fg.EMBED_ATOL      # (a NaN left in `out` fails the comparison)


@pytest.mark.parametrize('R', fg.EMB_ROWS)
@pytest.mark.parametrize('half', fg.FOURIER_HALVES)
def test_fourier_embed(ops, half, R):
    t, w = fg.emb_times(R), rand((half,), 18500 + half)
    out, td, wd = torch.full((R, 2 * half + 1), float('nan'), device=dev()), _d(t), _d(w)
    ops.call('dmh_fourier_embed', ops.ptr(td, torch.int64), ops.ptr(wd), ops.ptr(out), R, half)
    ref = fg.fourier_reference(t, w)
    err = (out.double().cpu() - ref)[:, 1:].abs().max().item()
    print(f'[parity] fourier_embed half={half} R={R}: max_abs={err:.3e} allowed {fg.EMBED_ATOL:.1e}')
    assert err <= fg.EMBED_ATOL
    _bitwise(f'fourier_embed half={half} R={R} column 0 vs fl(t)', out[:, 0], t.float())


@pytest.mark.parametrize('dim', [1, 64, 130])
def test_class_embed_rows(ops, dim):
    """keep absent: ids -1 and num_classes give a NaN row and only that row, every other row is bitwise the table's; with
    keep, a dropped row is the null row whatever its id is"""
    ncls = 5
    table, null = rand((ncls, dim), 18600 + dim), rand((dim,), 18601 + dim)
    classes = torch.tensor([0, 4, -1, 2, 5, 1, 3, 0, 4], dtype=torch.int64)
    valid = (classes >= 0) & (classes < ncls)
    nan_row = torch.full((dim,), float('nan'))
    for keep in (None, torch.tensor([1, 0, 1, 1, 0, 0, 1, 1, 1], dtype=torch.uint8)):
        got = ops.class_embed(_d(classes), _d(keep), _d(table), _d(null))
        kept = torch.ones_like(valid) if keep is None else keep.bool()
        want = torch.stack([(table[c] if v else nan_row) if k else null for c, v, k in zip(classes.tolist(), valid, kept)])
        bad_rows = torch.isnan(got).any(1).cpu()
        print(f'[parity] class_embed dim={dim} keep={keep is not None}: NaN rows {bad_rows.nonzero().flatten().tolist()}, '
              f'expected {(kept & ~valid).nonzero().flatten().tolist()}')
        assert torch.equal(bad_rows, kept & ~valid) and torch.equal(torch.isnan(got).all(1).cpu(), bad_rows)
        ok = ~bad_rows
        _bitwise(f'class_embed dim={dim} keep={keep is not None}: the other rows', got[ok.to(dev())], want[ok])


@pytest.mark.parametrize('N', fg.SSG_N)
def test_ss_gather_rows(ops, N):
    """out[b] = (T[cursor] + C[row]) + bias bit for bit in fp32; a cursor equal to S and an out-of-table class id of a kept row
    give NaN in exactly those rows"""
    S, ncls, B = 5, 3, 6
    T, Ct, bias = rand((S, N), 18700 + N), rand((ncls + 1, N), 18701 + N), rand((N,), 18702 + N)
    classes = torch.tensor([0, 2, 3, 1, -1, 2], dtype=torch.int64)
    for keep in (None, torch.tensor([1, 1, 1, 0, 0, 1], dtype=torch.uint8), torch.tensor([1, 1, 0, 1, 1, 0], dtype=torch.uint8)):
        kept = torch.ones(B, dtype=torch.bool) if keep is None else keep.bool()
        for step in (0, S - 1, S):
            cursor = torch.tensor([step], dtype=torch.int32, device=dev())
            out = torch.full((B, N), SENTINEL, device=dev())
            ops.ss_gather(_d(T), _d(Ct), _d(bias), cursor, _d(classes), _d(keep), out=out)
            bad = kept & ((classes < 0) | (classes >= ncls)) | (step >= S)
            nan_rows = torch.isnan(out).all(1).cpu()
            name = f'ss_gather N={N} keep={None if keep is None else keep.tolist()} cursor={step}'
            print(f'[parity] {name}: NaN rows {nan_rows.nonzero().flatten().tolist()}, expected {bad.nonzero().flatten().tolist()}')
            assert torch.equal(nan_rows, bad) and torch.equal(torch.isnan(out).any(1).cpu(), bad)
            if step < S:
                row = torch.where(kept, classes.clamp(0, ncls - 1), torch.full_like(classes, ncls))
                want = (T[step][None] + Ct[row]) + bias[None]
                ok = ~bad
                _bitwise(name + ': the other rows', out[ok.to(dev())], want[ok])
