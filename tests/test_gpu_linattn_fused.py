"""-m gpu: the fused LinearAttention passes of csrc/linattn_fused.hip — pass 1 (context partials), the merge of the splits
(dmh_linattn_merge_n of csrc/attention.hip) and pass 2 (q projection, softmax over d, product with the context; at C == 64
also to_out, LayerNorm and the residual) — each ALONE through the C ABI and together through ops.linear_attention_fused,
against the unfused mathematics in float64, at the pixel counts where a workgroup owns 1, 2, 3 and 8 sub-tiles.

Cases, references, error measures and gates: tests/linattn_fused_cases.py (its plan and yardsticks are checked on the CPU by
tests/test_linattn_fused_host.py).  Every comparison is per head (contexts: per head and batch row; pass-1 partials: per
head, row and split); `plain` is held to 2e-5, every other kind to max(2e-5, 10 * e32), e32 being plain fp32 torch on
the CPU measured the same way.  Every assertion prints its measurement as a [parity] line.  The module-scoped case fixture
makes pytest visit the table case by case, so one reference is alive at a time."""
import types

import pytest
import torch

import linattn_fused_cases as lc
from gpu_util import dev, rand

pytestmark = pytest.mark.gpu

SENT = -1.2345678e30      # no kernel output takes this value
GUARD = 4096              # floats on either side of an output buffer


@pytest.fixture(scope='module')
def ops():
    from dmhomo_amd import ops as _ops
    _ops.lib()
    return _ops


def _guarded(shape):
    """-> (whole, view): a sentinel-filled buffer with a guard band in front of and behind the view of `shape`"""
    numel = 1
    for s in shape:
        numel *= s
    whole = torch.full((numel + 2 * GUARD,), SENT, device=dev())
    return whole, whole[GUARD:GUARD + numel].view(shape)


def _guards_intact(name, whole):
    assert bool((whole[:GUARD] == SENT).all()) and bool((whole[-GUARD:] == SENT).all()), f'{name}: guard band written'
    assert not bool((whole[GUARD:-GUARD] == SENT).any()), f'{name}: a sentinel survived inside the output'


def _pixel_stats(ops, x, rows=None, out=None):
    B, _, n, C = x.shape
    st = torch.empty((B, n, 2), device=dev()) if out is None else out
    ops.call('dmh_pixel_stats', ops.ptr(x), ops.ptr(st), B * n, C, lc.EPS, ops._rows(rows), n)
    return st


def _on_device(ops, case):
    """the case on the device: inputs, packed weights, LayerNorm statistics, and the CPU reference record"""
    r = lc.case_reference(case)
    inp = r['inp']
    d = types.SimpleNamespace(case=case, r=r, name=lc.case_id(case), B=case.B, n=case.n, C=case.C, kind=case.kind)
    d.x = inp['x'].reshape(case.B, 1, case.n, case.C).to(dev())
    d.g = inp['g'].to(dev())
    d.pla = ops.PackedLinAttn(inp['w'].reshape(384, case.C, 1, 1).to(dev()))
    d.plo = None
    if 'wo' in inp:
        d.plo = ops.PackedLinAttnOut(inp['wo'].reshape(64, 128, 1, 1).to(dev()), inp['bo'].to(dev()), inp['go'].to(dev()))
    d.stats = _pixel_stats(ops, d.x)
    d.ns = ops.lib().dmh_linattn_fused_splits(case.B, case.n)
    assert d.ns == r['plan']['ns']
    return d


@pytest.fixture(scope='module', params=lc.CASES, ids=lc.case_id)
def dc(request, ops):
    return _on_device(ops, request.param)


@pytest.fixture(scope='module', params=[c for c in lc.CASES if c.C == 64], ids=lc.case_id)
def dc64(request, ops):
    """the cases of the fully fused width, for the block form and for the merge (which does not see C)"""
    return _on_device(ops, request.param)


def _context(ops, d, partial, rows=None):
    ops.call('dmh_linattn_fused_context', ops.ptr(d.x), ops.ptr(d.stats), ops.ptr(d.g), ops.ptr(d.pla.wpack), ops.ptr(partial),
             d.B, d.n, d.C, ops._rows(rows))


def _apply(ops, d, ctx, out):
    ops.call('dmh_linattn_fused_apply', ops.ptr(d.x), ops.ptr(d.stats), ops.ptr(d.g), ops.ptr(d.pla.wpack), ops.ptr(ctx),
             ops.ptr(out), d.B, d.n, d.C, lc.SCALE, None)


def _apply_out(ops, d, ctx, plo, y):
    ops.call('dmh_linattn_fused_apply_out', ops.ptr(d.x), ops.ptr(d.stats), ops.ptr(d.g), ops.ptr(d.pla.wpack), ops.ptr(ctx),
             ops.ptr(plo.wpack), ops.ptr(plo.bias), ops.ptr(plo.ln_g), ops.ptr(y), d.B, d.n, d.C, lc.SCALE, lc.EPS, None)


def _check_out(d, tag, out):
    """core output (B, 1, n, 128) per head"""
    r = d.r
    o = out.reshape(d.B, d.n, 128).cpu()
    assert bool(torch.isfinite(o).all()), f'{d.name} {tag}: not finite'
    if r['zero']:
        assert not bool(o.any()), f'{d.name} {tag}: the output must be exactly zero'
        print(f'[parity] {d.name} {tag} out: exactly zero')
        return
    lc.check(f'{d.name} {tag} out', d.kind, lc.head_err(o, r['out']), r['e32']['out'])


def _check_y(d, tag, y):
    """block output (B, 1, n, 64) per batch row"""
    r = d.r
    yc = y.reshape(d.B, d.n, 64).cpu()
    assert bool(torch.isfinite(yc).all()), f'{d.name} {tag}: not finite'
    if d.kind == 'constant_image':
        assert torch.equal(yc, r['inp']['x']), f'{d.name} {tag}: y must be x bitwise'
        print(f'[parity] {d.name} {tag} y: bitwise x')
        return
    lc.check(f'{d.name} {tag} y', d.kind, lc.y_err(yc, r['y'], r['r']), r['e32']['y'])


# ------------------------------------------------------------------ pass 1 alone
def test_pass1_context_partials(ops, dc):
    """dmh_pixel_stats + dmh_linattn_fused_context into a sentinel-filled partial [B][ns][4][1088].  A split stores its own
    maximum, so the invariant forms are compared, per (row, split, head): m[d] + log s[d] against the float64 logsumexp of
    k[d] over the split's pixels (absolute, in units of max(1, max |k|)), and ctx[d][e] / s[d] against the softmax-weighted
    mean of v[e] over them.  The split's pixel range comes from the restated plan (linattn_fused_cases.plan), not from the
    kernel.  No sentinel survives inside the partial, the guard bands around it stay."""
    d, r = dc, dc.r
    whole, partial = _guarded((d.B, d.ns, 4, lc.LA_PART))
    _context(ops, d, partial)
    _guards_intact(f'{d.name} partial', whole)
    p = partial.cpu().double()
    assert bool(torch.isfinite(p).all()), f'{d.name}: partial not finite'
    m, s, c = p[..., :32], p[..., 32:64], p[..., 64:].reshape(d.B, d.ns, 4, 32, 32)
    assert bool((s > 0).all())
    err_lse = ((m + s.log()) - r['lse']).abs().amax(3) / r['kmax']
    lc.check(f'{d.name} pass1 m + log s (units of max(1, max|k|) = {r["kmax"]:.3g})', d.kind, err_lse, r['e32']['lse_abs'])
    if r['zero']:
        assert not bool(c.any()), f'{d.name}: the context partial must be exactly zero'
        print(f'[parity] {d.name} pass1 ctx: exactly zero')
        return
    lc.check(f'{d.name} pass1 ctx / s', d.kind, lc.unit_err(c / s[..., None], r['wm']), r['e32']['wm'])


# ------------------------------------------------------------------ merge alone
def test_merge_alone(ops, dc64):
    """dmh_linattn_merge_n on partials built on the CPU from the float64 logits and rounded to fp32, every split's stored
    maximum moved off its true one by a different amount (a merge that took the maxima for equal would fail): the context
    per (row, head).  The merge does not see C: run at the C == 64 cases only."""
    d, r = dc64, dc64.r
    whole, ctx = _guarded((d.B, 4, 32, 32))
    part = r['partial'].to(dev())
    ops.call('dmh_linattn_merge_n', ops.ptr(part), ops.ptr(ctx), d.B, d.n, d.ns, None)
    _guards_intact(f'{d.name} merged ctx', whole)
    if r['zero']:
        assert not bool(ctx.any())
        print(f'[parity] {d.name} merge: exactly zero')
        return
    lc.check(f'{d.name} merge ctx', d.kind, lc.ctx_err(ctx, r['merged']), r['e32']['merged'])


# ------------------------------------------------------------------ pass 2 alone
def test_pass2_apply_alone(ops, dc):
    """dmh_linattn_fused_apply on the float64 context rounded to fp32: the core output per head"""
    d, r = dc, dc.r
    ctx = r['ctx'].float().to(dev())
    whole, out = _guarded((d.B, 1, d.n, 128))
    _apply(ops, d, ctx, out)
    _guards_intact(f'{d.name} out', whole)
    _check_out(d, 'pass2', out)


def test_pass2_apply_out_alone(ops, dc64):
    """C == 64: dmh_linattn_fused_apply_out (pass 2 + to_out + bias + LayerNorm + x) on the float64 context rounded to fp32.
    tiny_head: head 3's context is 2^-12 of the block maximum the static output scale is taken from while its to_out columns
    are 2^12 times the others', and its own contribution, y - y(head-3 columns of w_out zeroed), is compared kernel against
    reference — an error confined to that head cannot hide behind the other three."""
    d, r = dc64, dc64.r
    ctx = r['ctx'].float().to(dev())
    whole, y = _guarded((d.B, 1, d.n, 64))
    _apply_out(ops, d, ctx, d.plo, y)
    _guards_intact(f'{d.name} y', whole)
    _check_y(d, 'pass2', y)
    if d.kind == 'tiny_head':
        inp = r['inp']
        plz = ops.PackedLinAttnOut(lc.wo_without_head3(inp['wo']).reshape(64, 128, 1, 1).to(dev()), inp['bo'].to(dev()),
                                   inp['go'].to(dev()))
        yz = torch.empty_like(y)
        _apply_out(ops, d, ctx, plz, yz)
        got = (y.double() - yz.double()).reshape(d.B, d.n, 64).cpu()
        # both y carry the rounding of their final addition: two fp32 ulps of |y| off every element first (lc.y_err)
        e = ((got - r['d3']).abs() - 2.0 ** -22 * r['y'].abs()).clamp_min(0.0)
        err = e.amax((1, 2)) / r['d3'].abs().amax((1, 2))
        lc.check(f'{d.name} pass2 head 3 alone in y', d.kind, err, r['e32']['d3'])


# ------------------------------------------------------------------ composite
def test_composite(ops, dc):
    """ops.linear_attention_fused without and (C == 64) with out=: pixel statistics, pass 1, merge, pass 2"""
    d = dc
    _check_out(d, 'composite', ops.linear_attention_fused(d.x, d.g, d.pla, lc.SCALE))
    if d.plo is not None:
        _check_y(d, 'composite', ops.linear_attention_fused(d.x, d.g, d.pla, lc.SCALE, out=d.plo))


@pytest.mark.parametrize('C', [64, 128, 256])
def test_composite_with_producer_statistics_is_bitwise(ops, C):
    """stats= from ops.gn_silu_residual(pixel_stats=True), the producer in front of every fused LinearAttention of the
    UNet, gives bitwise the result of stats=None (dmh_pixel_stats), at a tiles = 2 pixel count"""
    assert C in ops.PIXEL_STATS_FUSABLE and set(ops.PIXEL_STATS_FUSABLE) == {64, 128, 256}
    B, n = 2, 4097
    yin = (rand((B, 1, n, C), 81) * 1.5).to(dev())
    res = (rand((B, 1, n, C), 82) * 1.7 + 0.3).to(dev())
    coef = torch.stack([1 + 0.2 * rand((B, C), 83), 0.3 * rand((B, C), 84)], 1).contiguous().to(dev())
    x, st = ops.gn_silu_residual(yin, coef, res, pixel_stats=True)
    g = (1 + 0.2 * rand((C,), 85)).to(dev())
    pla = ops.PackedLinAttn(rand((384, C, 1, 1), 86, C ** -0.5).to(dev()))
    assert torch.equal(st, _pixel_stats(ops, x))
    assert torch.equal(ops.linear_attention_fused(x, g, pla, lc.SCALE, stats=st), ops.linear_attention_fused(x, g, pla, lc.SCALE))
    if C == 64:
        plo = ops.PackedLinAttnOut((rand((64, 128, 1, 1), 87, 128 ** -0.5) * 30.0 * n).to(dev()), rand((64,), 88, 0.1).to(dev()),
                                   (1 + 0.2 * rand((64,), 89)).to(dev()))
        assert torch.equal(ops.linear_attention_fused(x, g, pla, lc.SCALE, out=plo, stats=st),
                           ops.linear_attention_fused(x, g, pla, lc.SCALE, out=plo))


# ------------------------------------------------------------------ rows
def _stages(ops, x, g, pla, plo, rows):
    """the four launches of the composite into sentinel-filled buffers -> stats, partial, ctx, out (or y)"""
    B, _, n, C = x.shape
    ns = ops.lib().dmh_linattn_fused_splits(B, n)
    st = torch.full((B, n, 2), SENT, device=dev())
    partial = torch.full((B, ns, 4, lc.LA_PART), SENT, device=dev())
    ctx = torch.full((B, 4, 32, 32), SENT, device=dev())
    out = torch.full((B, 1, n, 128 if plo is None else 64), SENT, device=dev())
    rp = ops._rows(rows)
    ops.call('dmh_pixel_stats', ops.ptr(x), ops.ptr(st), B * n, C, lc.EPS, rp, n)
    ops.call('dmh_linattn_fused_context', ops.ptr(x), ops.ptr(st), ops.ptr(g), ops.ptr(pla.wpack), ops.ptr(partial), B, n, C, rp)
    ops.call('dmh_linattn_merge_n', ops.ptr(partial), ops.ptr(ctx), B, n, ns, rp)
    if plo is None:
        ops.call('dmh_linattn_fused_apply', ops.ptr(x), ops.ptr(st), ops.ptr(g), ops.ptr(pla.wpack), ops.ptr(ctx), ops.ptr(out),
                 B, n, C, lc.SCALE, rp)
    else:
        ops.call('dmh_linattn_fused_apply_out', ops.ptr(x), ops.ptr(st), ops.ptr(g), ops.ptr(pla.wpack), ops.ptr(ctx),
                 ops.ptr(plo.wpack), ops.ptr(plo.bias), ops.ptr(plo.ln_g), ops.ptr(out), B, n, C, lc.SCALE, lc.EPS, rp)
    return dict(stats=st, partial=partial, ctx=ctx, out=out)


@pytest.mark.parametrize('C,with_out', [(64, False), (64, True), (128, False)], ids=['C64', 'C64-out', 'C128'])
def test_rows_subset(ops, C, with_out):
    """the CFG row subset (common.h: rows[0] active rows, rows[1 + j] the physical row of logical row j) handed to all four
    launches, B = 4, rows = [2, 3, 1], n = 4097: statistics, partials, contexts and outputs of physical rows 3 and 1 are
    bitwise what a launch of those two samples alone gives, and physical rows 0 and 2 of every buffer keep their sentinel"""
    B, n = 4, 4097
    x = (rand((B, 1, n, C), 91) * 1.7 + 0.3).to(dev())
    g = (1 + 0.2 * rand((C,), 92)).to(dev())
    pla = ops.PackedLinAttn(rand((384, C, 1, 1), 93, C ** -0.5).to(dev()))
    plo = None
    if with_out:
        plo = ops.PackedLinAttnOut((rand((64, 128, 1, 1), 94, 128 ** -0.5) * 30.0 * n).to(dev()), rand((64,), 95, 0.1).to(dev()),
                                   (1 + 0.2 * rand((64,), 96)).to(dev()))
    rows = torch.tensor([2, 3, 1, 0, 0], dtype=torch.int32, device=dev())
    full = _stages(ops, x, g, pla, plo, rows)
    alone = _stages(ops, x[[3, 1]].contiguous(), g, pla, plo, None)
    for name, t in full.items():
        a = alone[name]
        assert not bool((a == SENT).any()), name
        assert torch.equal(t[3], a[0]) and torch.equal(t[1], a[1]), f'{name}: an active row differs from the launch alone'
        assert bool((t[0] == SENT).all()) and bool((t[2] == SENT).all()), f'{name}: an inactive row was written'


# ------------------------------------------------------------------ widths
@pytest.mark.parametrize('C', [0, 16, 48, 72])
def test_widths_that_are_no_multiple_of_32_are_refused(ops, C):
    """the four entry points take every C % 32 == 0 (32 and 96 run above, in no UNet) and refuse the rest"""
    x = torch.zeros((1, 1, 4, max(C, 4)), device=dev())
    buf = torch.zeros((4096,), device=dev())
    with pytest.raises(ops._lib.DmhError):
        ops.call('dmh_linattn_fused_context', ops.ptr(x), ops.ptr(buf), ops.ptr(buf), ops.ptr(buf), ops.ptr(buf), 1, 4, C, None)
    with pytest.raises(ops._lib.DmhError):
        ops.call('dmh_linattn_fused_apply', ops.ptr(x), ops.ptr(buf), ops.ptr(buf), ops.ptr(buf), ops.ptr(buf), ops.ptr(buf),
                 1, 4, C, lc.SCALE, None)
    with pytest.raises(ops._lib.DmhError):
        ops.call('dmh_linattn_fused_pack', ops.ptr(buf), ops.ptr(buf), C)
