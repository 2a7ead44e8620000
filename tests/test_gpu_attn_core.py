"""-m gpu: the kernels of csrc/attention.hip — linattn_context (pass-1 partials), linattn_merge (with and without the saved
(M, S)), linattn_apply, attention_kernel — and the seven launches behind dmh_linattn_backward (csrc/attention_backward.hip),
each ALONE through the C ABI against float64, at the smallest pixel counts that reach every split, chunk and tile boundary:
a split, chunk or key tile of one pixel, B >= 2 with several splits (forward partials [b][split], backward [split][b]),
k shifted by 90, k maxima that move by e^12 from split to split, a running maximum that rises at every key tile, a
dominating first / last key, sharp q, v outliers.  The backward is fed the float64 ctx and (M, S) rounded to fp32, not the
forward kernels' outputs, so that a forward and a backward error cannot cancel.

Cases, references, error measures and gates: tests/attn_core_cases.py (its plan, yardsticks and gates are checked on the CPU
by tests/test_attn_core_host.py).  Every comparison is per (batch row, head) — pass-1 partials per (row, split, head);
`plain` is held to 1e-5 forward / 2e-5 for gradients, every other kind to max(that, 10 * e32).  Every output buffer is
prefilled with a sentinel and has guard bands on both sides.  Every assertion prints its measurement as a [parity] line."""
import pytest
import torch

import attn_core_cases as ac
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
    band = int((whole[:GUARD] != SENT).sum()) + int((whole[-GUARD:] != SENT).sum())
    left = int((whole[GUARD:-GUARD] == SENT).sum())
    print(f'[parity] {name}: {band} guard floats written, {left} sentinels left among the {whole.numel() - 2 * GUARD} '
          f'output floats')
    assert band == 0, f'{name}: guard band written'
    assert left == 0, f'{name}: a sentinel survived inside the output'


def _bitwise(name, got, want):
    """print the [parity] line of a bitwise comparison and hold it"""
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    diff = int((got != want).sum())
    print(f'[parity] {name}: {diff} of {got.numel()} floats differ (bitwise)')
    assert diff == 0 and torch.equal(got, want), f'{name}: not bitwise equal'


# ------------------------------------------------------------------ the launches, each into guarded buffers
def _context(ops, qkv):
    B, n, _ = qkv.shape
    whole, partial = _guarded((B, ac.splits(n), 4, ac.LA_PART))
    assert partial.numel() == ops.lib().dmh_linattn_partial_floats(B, n)
    ops.call('dmh_linattn_context', ops.ptr(qkv), ops.ptr(partial), B, n, None)
    _guards_intact('partial', whole)
    return partial


def _merge(ops, partial, n):
    B = partial.shape[0]
    whole, ctx = _guarded((B, 4, 32, 32))
    ops.call('dmh_linattn_merge', ops.ptr(partial), ops.ptr(ctx), B, n, None)
    _guards_intact('ctx (merge)', whole)
    return ctx


def _merge_ms(ops, partial, n):
    B = partial.shape[0]
    whole, ctx = _guarded((B, 4, 32, 32))
    whole_ms, ms = _guarded((B, 4, 32, 2))
    ops.call('dmh_linattn_merge_ms', ops.ptr(partial), ops.ptr(ctx), ops.ptr(ms), B, n)
    _guards_intact('ctx (merge_ms)', whole)
    _guards_intact('ms', whole_ms)
    return ctx, ms


def _apply(ops, qkv, ctx):
    B, n, _ = qkv.shape
    whole, out = _guarded((B, n, 128))
    ops.call('dmh_linattn_apply', ops.ptr(qkv), ops.ptr(ctx), ops.ptr(out), B, n, ac.SCALE, None)
    _guards_intact('out (apply)', whole)
    return out


def _attention(ops, qkv):
    B, n, _ = qkv.shape
    whole, out = _guarded((B, n, 128))
    ops.call('dmh_attention', ops.ptr(qkv), ops.ptr(out), B, n, ac.SCALE, None)
    _guards_intact('out (attention)', whole)
    return out


def _backward(ops, qkv, ctx, ms, dout):
    """-> dqkv (B, n, 384) and the workspace (flat), both written in full between intact guard bands"""
    B, n, _ = qkv.shape
    whole, dqkv = _guarded((B, n, 384))
    nwork = ops.lib().dmh_linattn_bwd_workspace_floats(B, n)
    assert nwork == ac.bwd_workspace_floats(B, n)
    whole_w, work = _guarded((nwork,))
    ops.call('dmh_linattn_backward', ops.ptr(qkv), ops.ptr(ctx), ops.ptr(ms), ops.ptr(dout), ops.ptr(dqkv), ops.ptr(work), B, n,
             ac.SCALE)
    _guards_intact('dqkv', whole)
    _guards_intact('backward workspace', whole_w)
    return dqkv, work


def _ms_from(M, S):
    """(B, 4, 32) float64 each -> ms (B, 4, 32, 2) fp32 on the device"""
    return torch.stack([M, S], 3).float().contiguous().to(dev())


# ------------------------------------------------------------------ LinearAttention forward
@pytest.fixture(scope='module', params=ac.LA_CASES, ids=ac.case_id)
def la(request):
    r = ac.la_reference(request.param)
    return dict(r, name=ac.case_id(request.param), qkv=r['inp']['qkv'].to(dev()), dout=r['inp']['dout'].to(dev()))


def test_linattn_context_alone(ops, la):
    """dmh_linattn_context: per (row, split, head) m + log s against the float64 logsumexp of the split (absolute, in units of
    max(1, max |k|)), ctx / s against the softmax-weighted mean of v, and m bitwise the split's fp32 maximum of k"""
    c, name = la['case'], la['name']
    p = _context(ops, la['qkv']).cpu()
    assert bool(torch.isfinite(p).all()), f'{name}: partial not finite'
    m, s, cx = p[..., :32], p[..., 32:64].double(), p[..., 64:].reshape(c.B, -1, 4, 32, 32).double()
    _bitwise(f'{name} context m vs the fp32 maximum of every split', m, la['m32'])
    assert bool((s > 0).all())
    err = ((m.double() + s.log()) - la['lse']).abs().amax(3) / la['kmax']
    ac.check(f'{name} context m + log s (units of max(1, max|k|) = {la["kmax"]:.3g})', c.kind, err, la['e32']['lse_abs'], ac.FWD)
    ac.check(f'{name} context ctx / s', c.kind, ac.unit_err(cx / s[..., None], la['wm']), la['e32']['wm'], ac.FWD)


def test_linattn_merge_alone(ops, la):
    """dmh_linattn_merge and dmh_linattn_merge_ms on the context kernel's own partials: the two contexts bitwise equal, M
    bitwise the fp32 maximum of k over the pixels, S against the float64 sum of exp(k - M), the context against float64"""
    c, name, r64 = la['case'], la['name'], la['r64']
    partial = _context(ops, la['qkv'])
    ctx = _merge(ops, partial, c.n)
    ctx2, ms = _merge_ms(ops, partial, c.n)
    _bitwise(f'{name} merge ctx of dmh_linattn_merge vs dmh_linattn_merge_ms', ctx, ctx2)
    ms = ms.cpu()
    _bitwise(f'{name} merge M vs the fp32 maximum of k', ms[..., 0], la['M32'])
    ac.check(f'{name} merge S', c.kind, ac.vec_err(ms[..., 1], r64['S']), la['e32']['S'], ac.FWD)
    ac.check(f'{name} merge ctx', c.kind, ac.ctx_err(ctx, r64['ctx']), la['e32']['ctx'], ac.FWD)


def test_linattn_apply_alone(ops, la):
    """dmh_linattn_apply on the float64 context rounded to fp32: the output per (row, head)"""
    c, name, r64 = la['case'], la['name'], la['r64']
    out = _apply(ops, la['qkv'], r64['ctx'].float().to(dev())).cpu()
    assert bool(torch.isfinite(out).all()), f'{name}: not finite'
    ac.check(f'{name} apply out', c.kind, ac.bh_err(out, r64['out']), la['e32']['out'], ac.FWD)


# ------------------------------------------------------------------ LinearAttention backward
def _check_grads(la, tag, dqkv):
    c, r64 = la['case'], la['r64']
    g = dqkv.reshape(c.B, c.n, 384).cpu()
    assert bool(torch.isfinite(g).all()), f'{la["name"]} {tag}: not finite'
    for name, e in ac.dqkv_err(g, r64['dqkv'], la['zero_scale']).items():
        ac.check(f'{la["name"]} {tag} {name}', c.kind, e, la['e32'][name], ac.GRAD)


def test_linattn_backward_alone(ops, la):
    """dmh_linattn_backward on the float64 ctx and (M, S) rounded to fp32: dq, dk, dv per (row, head) against float64
    autograd; dctx and t read back from the workspace at the restated offsets; every float of dqkv and of the workspace
    written; dout = 0 gives dqkv exactly zero"""
    c, name, r64 = la['case'], la['name'], la['r64']
    ctx, ms = r64['ctx'].float().to(dev()), _ms_from(r64['M'], r64['S'])
    dqkv, work = _backward(ops, la['qkv'], ctx, ms, la['dout'])
    _check_grads(la, 'backward', dqkv)
    reg = ac.bwd_regions(c.B, c.n)
    (o, size) = reg['dctx']
    ac.check(f'{name} backward dctx (workspace)', c.kind, ac.ctx_err(work[o:o + size].reshape(c.B, 4, 32, 32), r64['dctx']),
             la['e32']['dctx'], ac.GRAD)
    (o, size) = reg['t']
    ac.check(f'{name} backward t (workspace)', c.kind, ac.vec_err(work[o:o + size].reshape(c.B, 4, 32), r64['t']), la['e32']['t'],
             ac.GRAD)
    zero, _ = _backward(ops, la['qkv'], ctx, ms, torch.zeros_like(la['dout']))
    print(f'[parity] {name} backward dout = 0: {int((zero != 0).sum())} of {zero.numel()} floats of dqkv are not zero')
    assert not bool(zero.any()), f'{name}: dout = 0 must give dqkv exactly zero'


def test_linattn_composite(ops, la):
    """ops.linear_attention_core_train and ops.linear_attention_core_backward (the forward kernels' own ctx and (M, S) feed the
    backward), held to the same gates"""
    c, name, r64 = la['case'], la['name'], la['r64']
    out, sv = ops.linear_attention_core_train(la['qkv'].reshape(c.B, 1, c.n, 384), ac.SCALE)
    o = out.reshape(c.B, c.n, 128).cpu()
    assert bool(torch.isfinite(o).all()), f'{name}: not finite'
    ac.check(f'{name} composite out', c.kind, ac.bh_err(o, r64['out']), la['e32']['out'], ac.FWD)
    _check_grads(la, 'composite', ops.linear_attention_core_backward(sv, la['dout'].reshape(c.B, 1, c.n, 128)))


# ------------------------------------------------------------------ attention
@pytest.mark.parametrize('case', ac.ATT_CASES, ids=ac.case_id)
def test_attention_alone(ops, case):
    """dmh_attention per (row, head) against float64"""
    r = ac.att_reference(case)
    out = _attention(ops, r['inp']['qkv'].to(dev())).cpu()
    assert bool(torch.isfinite(out).all()), f'{ac.case_id(case)}: not finite'
    ac.check(f'{ac.case_id(case)} attention out', case.kind, ac.bh_err(out, r['out']), r['e32']['out'], ac.FWD)


@pytest.mark.parametrize('n', ac.ATT_N)
def test_attention_constant_v_gives_v(ops, n):
    """known answer: v the same at every pixel -> out = v at every query — the weights of a row sum to one; a masked key that
    leaks a weight, or a weight lost in a rescale, breaks the row sum.  With equal keys and v on a 2^-8 grid every sum of
    the kernel is exact (ac.att_constant_v): within 4 fp32 ulps.  With plain keys (the running maximum moves, the sums
    round): within ac.constant_v_gate = 10 x plain fp32 torch on the CPU, per element.  Measured on MI355X with plain
    keys: 7 ulps at n = 31, 20 at n = 256, 39 at n = 1025 — plain fp32 torch on the CPU: 5, 16, 20 — so the 4-ulp bound
    belongs to the exact form only."""
    qkv = ac.att_constant_v(n, equal_keys=True)
    out = _attention(ops, qkv.to(dev())).cpu().double()
    v = qkv[:, :1, 256:].double()
    ulps = ((out - v).abs() / ac.ulp32(v)).max().item()
    print(f'[parity] n{n} attention constant v, equal keys: out = v within {ulps:.2f} fp32 ulps (allowed 4)')
    assert ulps <= 4.0, ulps
    qkv = ac.att_constant_v(n, equal_keys=False)
    out = _attention(ops, qkv.to(dev())).cpu().double()
    v = qkv[:, :1, 256:].double()
    rel = ac.constant_v_rel(out, qkv)
    gate, e32 = ac.constant_v_gate(qkv)
    print(f'[parity] n{n} attention constant v, plain keys: err={rel:.3e} of |v| per element '
          f'({((out - v).abs() / ac.ulp32(v)).max().item():.0f} ulps) e32={e32:.3e} gate={gate:.3e} '
          f'(summation bound {ac.constant_v_bound(n):.3e})')
    assert rel <= gate, rel


@pytest.mark.parametrize('n', ac.ATT_N)
def test_attention_equal_keys_give_mean_v(ops, n):
    """known answer: all keys equal -> uniform weights -> out = the mean of v over the pixels at every query"""
    qkv = ac.att_equal_keys(n)
    out = _attention(ops, qkv.to(dev())).cpu()
    ref = qkv[..., 256:].double().mean(1, keepdim=True).expand(-1, n, -1)
    ac.check(f'n{n} attention equal keys: mean of v', 'plain', ac.bh_err(out, ref), torch.zeros(2, 4), ac.FWD)


# ------------------------------------------------------------------ bitwise properties
def _la_forward(ops, qkv):
    B, n, _ = qkv.shape
    partial = _context(ops, qkv)
    ctx, ms = _merge_ms(ops, partial, n)
    return dict(partial=partial, ctx=ctx, ms=ms, out=_apply(ops, qkv, ctx))


def test_rows_of_a_batch_equal_launches_alone(ops):
    """n = 257 (three splits, two chunks), B = 3: every row of dmh_attention, of the three forward launches (partials
    [b][split]) and of dmh_linattn_backward (partials [split][b]) is bitwise what a B = 1 launch of that row returns"""
    n = 257
    qkv = ac.la_inputs(ac.Case(n, 3, 'plain'))
    qkv, dout = qkv['qkv'].to(dev()), qkv['dout'].to(dev())
    att = _attention(ops, qkv)
    fwd = _la_forward(ops, qkv)
    dqkv, _ = _backward(ops, qkv, fwd['ctx'], fwd['ms'], dout)
    for b in range(3):
        q1 = qkv[b:b + 1].contiguous()
        _bitwise(f'dmh_attention row {b} of B = 3 vs alone', att[b], _attention(ops, q1)[0])
        f1 = _la_forward(ops, q1)
        for key, t in fwd.items():
            _bitwise(f'linattn forward {key} row {b} of B = 3 vs alone', t[b], f1[key][0])
        d1, _ = _backward(ops, q1, f1['ctx'], f1['ms'], dout[b:b + 1].contiguous())
        _bitwise(f'dmh_linattn_backward dqkv row {b} of B = 3 vs alone', dqkv[b], d1[0])


def test_repeated_launches_are_identical(ops):
    n = 257
    inp = ac.la_inputs(ac.Case(n, 3, 'plain'))
    qkv, dout = inp['qkv'].to(dev()), inp['dout'].to(dev())
    att = _attention(ops, qkv)
    fwd = _la_forward(ops, qkv)
    dqkv, work = _backward(ops, qkv, fwd['ctx'], fwd['ms'], dout)
    for i in range(3):
        _bitwise(f'dmh_attention repeat {i}', _attention(ops, qkv), att)
        again = _la_forward(ops, qkv)
        for key, t in fwd.items():
            _bitwise(f'linattn forward {key} repeat {i}', again[key], t)
        d2, w2 = _backward(ops, qkv, fwd['ctx'], fwd['ms'], dout)
        _bitwise(f'dmh_linattn_backward dqkv repeat {i}', d2, dqkv)
        _bitwise(f'dmh_linattn_backward workspace repeat {i}', w2, work)


def test_attention_rows_independent_under_load(ops):
    """dmh_attention at B = 50, n = 1024 (1600 workgroups: more than the chip holds at once) returns for rows 0 and 1 bitwise
    what a launch of those two rows alone returns, launch after launch"""
    qkv = (rand((50, 1024, 384), 9701) * 1.5).to(dev())
    alone = _attention(ops, qkv[:2].contiguous())
    for i in range(3):
        _bitwise(f'dmh_attention rows 0, 1 of B = 50, n = 1024 vs a 2-row launch, launch {i}', _attention(ops, qkv)[:2], alone)


def test_linattn_backward_rows_independent_under_load(ops):
    """dmh_linattn_backward at B = 16, n = 4096 returns for rows 0 and 1 bitwise what a 2-row launch returns, launch after
    launch"""
    B, n = 16, 4096
    qkv = (rand((B, n, 384), 9702) * 1.5).to(dev())
    dout = rand((B, n, 128), 9703).to(dev())
    fwd = _la_forward(ops, qkv)
    two = [t[:2].contiguous() for t in (qkv, fwd['ctx'], fwd['ms'], dout)]
    alone, _ = _backward(ops, *two)
    for i in range(3):
        dqkv, _ = _backward(ops, qkv, fwd['ctx'], fwd['ms'], dout)
        _bitwise(f'dmh_linattn_backward rows 0, 1 of B = 16, n = 4096 vs a 2-row launch, launch {i}', dqkv[:2], alone)
