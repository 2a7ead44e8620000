"""-m gpu: the normalisation-backward kernels (csrc/norm_backward.hip, dmh_gn_finalize_train of csrc/norm.hip) and the
small-GEMM / row-softmax kernels (csrc/gemm_small.hip), each ALONE through the C ABI against torch autograd of the plain
operation on the CPU in float64.  Cases, references and gates: tests/norm_bwd_cases.py (its yardsticks are capped on the
CPU by tests/test_norm_backward_host.py).  Every assertion prints its measurement as a [parity] line."""
import pytest
import torch

import norm_bwd_cases as nb
from gpu_util import dev, nhwc, nchw, rand

pytestmark = pytest.mark.gpu


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
    assert bool(torch.isfinite(got).all()), f'{name}: not finite'
    err = (got - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f'[parity] {name}: worst |err| / bound = {ratio:.3e} (max_abs={err.max().item():.3e}, bound there '
          f'{bound.flatten()[(err / bound.clamp_min(1e-300)).argmax()].item():.3e})')
    bad = (err > bound).nonzero()
    assert bad.shape[0] == 0, f'{name}: {bad.shape[0]} elements over their bound, first at {bad[0].tolist()}: ' \
                             f'err {err[tuple(bad[0])].item():.3e} > {bound[tuple(bad[0])].item():.3e}'


# ------------------------------------------------------------------ GroupNorm -> (scale + 1, shift) -> SiLU backward
def _gn_backward(ops, r, coef, mr):
    inp = r['inp']
    return ops.gn_silu_backward(nhwc(inp['dout']), nhwc(inp['y']), _d(coef), _d(mr), _d(inp['gamma']), _d(inp['beta']),
                                inp['groups'], ss=_d(inp['ss']))


def _gn_check(tag, r, out):
    dy, dgamma, dbeta, dss = out
    ref64, ref32 = r['ref64'], r['ref32']
    nb.check(tag + ' dy', nchw(dy), ref64['dy'], ref32['dy'])
    nb.check(tag + ' dgamma', dgamma, ref64['dgamma'], ref32['dgamma'])
    nb.check(tag + ' dbeta', dbeta, ref64['dbeta'], ref32['dbeta'])
    if r['inp']['ss'] is None:
        assert dss is None
    else:
        nb.check(tag + ' dss', dss, ref64['dss'], ref32['dss'])


@pytest.mark.parametrize('case', nb.GN_CASES, ids=nb.gn_id)
def test_gn_silu_backward(ops, case):
    """dmh_gn_silu_backward (reduce, finalize, apply) + the batch sum of its parameter parts, given coef / mr by the float64
    formula: dy, dgamma, dbeta, dss within max(5e-6, 10 * e32) of float64 autograd.  The saturated kind (|z| past 88.7 on
    both sides, where exp(-z) overflows fp32) must also stay finite: nb.check turns a non-finite output into an error."""
    r = nb.gn_reference(case)
    _gn_check('gn_silu_bwd ' + nb.gn_id(case), r, _gn_backward(ops, r, r['coef'], r['mr']))


@pytest.mark.parametrize('fcase', nb.GN_FINALIZE_CASES, ids=lambda c: f'{nb.gn_id((c[0], "unit", c[2]))}-tiles{c[1]}')
def test_gn_finalize_train(ops, fcase):
    """dmh_gn_finalize_train on per-tile (sum, sum of squares) partials: coef and (mean, rstd) against the float64 formula
    (yardstick: the formula in fp32), then those outputs through dmh_gn_silu_backward within its own gate"""
    f = nb.gn_finalize_reference(fcase)
    r = f['back']
    inp = r['inp']
    coef, mr = ops.gn_finalize_train(_d(f['stats']), _d(inp['gamma']), _d(inp['beta']), f['hw'], inp['groups'],
                                     ss=_d(inp['ss']), eps=nb.EPS)
    tag = f'gn_finalize_train {nb.gn_id((fcase[0], "unit", fcase[2]))} tiles={fcase[1]}'
    for name, got in (('a', coef[:, 0]), ('c', coef[:, 1]), ('mean', mr[..., 0]), ('rstd', mr[..., 1])):
        nb.check(f'{tag} {name}', got, f['ref64'][name], f['ref32'][name])
    _gn_check(tag + ' -> gn_silu_bwd', r, _gn_backward(ops, r, coef, mr))


# ------------------------------------------------------------------ weight standardisation backward
@pytest.mark.parametrize('case', nb.WS_CASES, ids=nb.ws_id)
def test_ws_backward(ops, case):
    r = nb.ws_reference(case)
    dw = ops.ws_backward(_d(r['inp']['w']), _d(r['inp']['dwh']), eps=nb.EPS)
    assert dw.shape == r['inp']['w'].shape
    nb.check('ws_bwd ' + nb.ws_id(case) + ' dw', dw, r['ref64']['dw'], r['ref32']['dw'])


# ------------------------------------------------------------------ channel LayerNorm backward
@pytest.mark.parametrize('case', nb.LN_CASES, ids=nb.ln_id)
def test_chan_layernorm_backward_arms(ops, case):
    """the dispatch arms, ragged channel quads and the grid-stride loop that test_chan_layernorm_backward leaves out"""
    r = nb.ln_reference(case)
    inp = r['inp']
    dx, dg = ops.chan_layernorm_backward(nhwc(inp['x']), _d(inp['g']), nhwc(inp['dout']), eps=nb.EPS)
    nb.check('ln_bwd ' + nb.ln_id(case) + ' dx', nchw(dx), r['ref64']['dx'], r['ref32']['dx'])
    nb.check('ln_bwd ' + nb.ln_id(case) + ' dg', dg, r['ref64']['dg'], r['ref32']['dg'])


# ------------------------------------------------------------------ dmh_sum_over_batch
@pytest.mark.parametrize('per', nb.SOB_PER)
@pytest.mark.parametrize('B', nb.SOB_B)
def test_sum_over_batch(ops, B, per):
    """out[i] = sum_b in[b][i] within B u sum_b |in[b][i]| per element, nothing written past `per`, and a second launch
    bitwise the first"""
    guard = -12345.5
    x = rand((B, per), 7000 + 31 * B + per)
    xg = _d(x)
    outs = []
    for _ in range(2):
        out = torch.full((per + 32,), guard, device=dev())
        ops.call('dmh_sum_over_batch', ops.ptr(xg), ops.ptr(out), B, per)
        outs.append(out.cpu())
    ref, bound = nb.sum_over_batch_bound(x)
    _within(f'sum_over_batch B={B} per={per}', outs[0][:per], ref, bound)
    assert bool((outs[0][per:] == guard).all()), f'B={B} per={per}: wrote past the end'
    assert torch.equal(outs[0], outs[1]), f'B={B} per={per}: two launches differ'


# ------------------------------------------------------------------ dmh_bgemm
def _operand(t, transposed):
    """t (nbo, nbi, R, Cc) logical -> (device buffer, strides (outer, inner, row, column)); transposed: stored (.., Cc, R)"""
    nbo, nbi, R, Cc = t.shape
    if transposed:
        return _d(t.transpose(2, 3)), (nbi * R * Cc, R * Cc, 1, R)
    return _d(t), (nbi * R * Cc, R * Cc, Cc, 1)


@pytest.mark.parametrize('shape', nb.BGEMM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bgemm_elementwise(ops, shape):
    """every element of C = alpha * A @ B within the dot-product bound, for A and B row-major and transposed through their
    strides; C is prefilled with NaN, so an element the kernel does not write fails too"""
    M, N, K, nbo, nbi = shape
    a, b = nb.bgemm_inputs(shape)
    for alpha in nb.BGEMM_ALPHAS:
        ref, bound = nb.bgemm_reference(a, b, alpha)
        for ta in (False, True):
            for tb in (False, True):
                ab, sa = _operand(a, ta)
                bb, sb = _operand(b, tb)
                c = torch.full((nbo, nbi, M, N), float('nan'), device=dev())
                ops.bgemm(ab, sa, bb, sb, c, (nbi * M * N, M * N, N, 1), M, N, K, nbo, nbi, alpha)
                _within(f'bgemm {shape} alpha={alpha} A{"^T" if ta else ""} B{"^T" if tb else ""}', c, ref, bound)


def test_bgemm_strided_output(ops):
    """C written with column stride 2 at a float offset inside a larger buffer: the addressed floats within the bound, every
    other float still the sentinel"""
    shape = M, N, K, nbo, nbi = (33, 31, 7, 2, 3)
    a, b = nb.bgemm_inputs(shape)
    alpha, off, sentinel = -0.37, 5, -777.25
    ref, bound = nb.bgemm_reference(a, b, alpha)
    sc = (nbi * M * 2 * N, M * 2 * N, 2 * N, 2)
    size = off + nbo * sc[0] + 7
    idx = (off + torch.arange(nbo)[:, None, None, None] * sc[0] + torch.arange(nbi)[None, :, None, None] * sc[1] +
           torch.arange(M)[None, None, :, None] * sc[2] + torch.arange(N)[None, None, None, :] * sc[3])
    assert int(idx.max()) < size and idx.unique().numel() == idx.numel()
    buf = torch.full((size,), sentinel, device=dev())
    ab, sa = _operand(a, False)
    bb, sb = _operand(b, True)
    ops.bgemm(ab, sa, bb, sb, (buf, off), sc, M, N, K, nbo, nbi, alpha)
    out = buf.cpu()
    _within('bgemm strided C', out[idx], ref, bound)
    rest = torch.ones(size, dtype=torch.bool)
    rest[idx.flatten()] = False
    touched = int((out[rest] != sentinel).sum())
    print(f'[parity] bgemm strided C: {touched} of {int(rest.sum())} floats outside the addressed set changed')
    assert touched == 0


# ------------------------------------------------------------------ dmh_softmax_rows / dmh_softmax_rows_backward
@pytest.mark.parametrize('case', nb.SM_CASES, ids=nb.sm_id)
def test_softmax_rows_forward(ops, case):
    (rows, n), kind = case
    r = nb.sm_reference(case)
    s = _d(r['inp']['s'])
    p = torch.full_like(s, float('nan'))
    ops.call('dmh_softmax_rows', ops.ptr(s), ops.ptr(p), rows, n)
    nb.check('softmax fwd ' + nb.sm_id(case), p, r['ref64']['p'], r['ref32']['p'])
    dev1 = (p.double().cpu().sum(1) - 1).abs().max().item()
    print(f'[parity] softmax fwd {nb.sm_id(case)}: max |row sum - 1| = {dev1:.3e}, allowed {n * nb.U:.3e}')
    assert dev1 <= n * nb.U
    assert torch.equal(s.cpu(), r['inp']['s'])


@pytest.mark.parametrize('case', nb.SM_CASES, ids=nb.sm_id)
def test_softmax_rows_backward(ops, case):
    """dS = P * (dP - sum_j dP P) in place on dP, P (the float64 softmax rounded to fp32) untouched.  Where the gradient is
    exactly zero in fp32 (nb.sm_grad_is_zero) the reference has no scale to be relative to: the kernel must return zeros."""
    (rows, n), kind = case
    r = nb.sm_reference(case)
    p, d = _d(r['p32']), _d(r['inp']['dp'])
    ops.call('dmh_softmax_rows_backward', ops.ptr(p), ops.ptr(d), rows, n)
    nb.check('softmax bwd ' + nb.sm_id(case), d, r['ref64']['ds'], r['ref32']['ds'])
    if nb.sm_grad_is_zero(case):
        nonzero = int(torch.count_nonzero(d))
        print(f'[parity] softmax bwd {nb.sm_id(case)}: {nonzero} of {d.numel()} elements are not exactly zero, allowed 0')
        assert nonzero == 0
    assert torch.equal(p.cpu(), r['p32'])
