"""CPU half of tests/test_gpu_norm_backward.py: the yardstick of every case of tests/norm_bwd_cases.py stays under its cap.

The GPU tests hold a kernel to max(5e-6, 10 * e32), e32 being the error of torch's own fp32 autograd on the CPU against
the float64 reference.  Here every e32 is computed and must be <= CAP = 2e-5, so that no gate exceeds 2e-4, and every
reference gradient must be finite and non-zero.  A case that breaks the cap gets a milder input; the cap does not move."""
import pytest
import torch

import norm_bwd_cases as nb


def _yardstick(name, ref64, ref32):
    worst = 0.0
    for k, r64 in ref64.items():
        if r64 is None:
            assert ref32[k] is None
            continue
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(ref32[k]).all()), f'{name} {k}: not finite'
        assert r64.abs().max().item() > 0.0, f'{name} {k}: the reference is identically zero'
        e32 = nb.rel(ref32[k], r64)
        print(f'[yardstick] {name} {k}: e32={e32:.3e} gate={nb.gate(e32):.3e} ref_absmax={r64.abs().max().item():.3e}')
        assert e32 <= nb.CAP, f'{name} {k}: e32 = {e32:.3e} is over the cap {nb.CAP:.0e}: make the input milder'
        worst = max(worst, e32)
    return worst


@pytest.mark.parametrize('case', nb.GN_CASES, ids=nb.gn_id)
def test_gn_silu_backward_yardstick(case):
    r = nb.gn_reference(case)
    _yardstick('gn_silu_bwd ' + nb.gn_id(case), r['ref64'], r['ref32'])
    assert (r['ref64']['dss'] is None) == (r['inp']['ss'] is None)
    if case[1] == 'saturated':       # exp(-z) overflows fp32 above 88.73 on the negative side; sigmoid is 1 on the other
        print(f'[yardstick] saturated z in [{r["zmin"]:.1f}, {r["zmax"]:.1f}]')
        assert r['zmin'] < -90.0 and r['zmax'] > 90.0
    if case[1] == 'scale1e-4':
        y = r['inp']['y']
        assert y.reshape(y.shape[0], r['inp']['groups'], -1).var(2).max().item() < nb.EPS


@pytest.mark.parametrize('fcase', nb.GN_FINALIZE_CASES, ids=lambda c: f'{nb.gn_id((c[0], "unit", c[2]))}-tiles{c[1]}')
def test_gn_finalize_train_yardstick(fcase):
    r = nb.gn_finalize_reference(fcase)
    _yardstick(f'gn_finalize_train tiles={fcase[1]}', r['ref64'], r['ref32'])
    B, tiles, C, two = r['stats'].shape
    assert (tiles, two) == (fcase[1], 2) and r['hw'] == fcase[0][3] * fcase[0][4]
    # the tiles partition the pixels: their sums add up to the whole
    y = r['back']['inp']['y'].double().reshape(B, C, -1)
    assert nb.rel(r['stats'].double().sum(1)[..., 0], y.sum(2)) < 1e-6
    assert nb.rel(r['stats'].double().sum(1)[..., 1], (y * y).sum(2)) < 1e-6


@pytest.mark.parametrize('case', nb.WS_CASES, ids=nb.ws_id)
def test_ws_backward_yardstick(case):
    r = nb.ws_reference(case)
    _yardstick('ws_bwd ' + nb.ws_id(case), r['ref64'], r['ref32'])
    if case[1] == 'const_row':
        row = r['inp']['w'][case[0][0] // 2]
        assert bool((row == row.flatten()[0]).all())


@pytest.mark.parametrize('case', nb.LN_CASES, ids=nb.ln_id)
def test_chan_layernorm_backward_yardstick(case):
    r = nb.ln_reference(case)
    _yardstick('ln_bwd ' + nb.ln_id(case), r['ref64'], r['ref32'])


@pytest.mark.parametrize('case', nb.SM_CASES, ids=nb.sm_id)
def test_softmax_rows_yardstick(case):
    """(n = 1: softmax is the constant 1 and its gradient identically zero — the one reference that may be zero.  In the
    one_hot200 kind the float64 gradient is of the order exp(-200): non-zero, and nothing against the floor of `rel`.  For
    both the fp32 gradient is exactly zero, and the GPU test asks for exact zeros on top of its gate: nb.sm_grad_is_zero.)"""
    (rows, n), kind = case
    r = nb.sm_reference(case)
    keys = ('p',) if n == 1 else ('p', 'ds')
    _yardstick('softmax ' + nb.sm_id(case), {k: r['ref64'][k] for k in keys}, {k: r['ref32'][k] for k in keys})
    if n == 1:
        assert not r['ref64']['ds'].any() and not r['ref32']['ds'].any()
    zero = not r['ref32']['ds'].any() and r['ref64']['ds'].abs().max().item() < nb.SCALE_FLOOR
    assert zero == nb.sm_grad_is_zero(case)
    if kind == 'one_hot200' and n > 1:
        assert int((r['p32'] == 0).sum()) == rows * (n - 1) and int((r['p32'] == 1).sum()) == rows


def test_case_tables_reach_the_branches_they_name():
    """each table row reaches the branch its comment names.  Chunk and partial-row counts come from the library; the
    256-thread plans of gn_silu_bwd_reduce_kernel and the <LPP, NV> ladder of dmh_chan_layernorm_backward have no export
    and are restated here (csrc/norm_backward.hip points back at this test from both places)."""
    from dmhomo_amd import _lib
    lib = _lib.lib()
    plans = {}
    for (B, C, G, H, W) in nb.GN_SHAPES:
        c4 = C // 4
        qpt = min(c4, 256)
        plans[(C, H * W)] = dict(chunks=lib.dmh_gn_bwd_chunks(H * W), qb_rounds=-(-c4 // qpt), lanes=256 // qpt,
                                 idle=256 - (256 // qpt) * qpt, cg=C // G)
    assert plans[(64, 256)]['chunks'] == 1 and plans[(64, 437)]['chunks'] == 2
    assert plans[(24, 9)]['idle'] == 4 and plans[(24, 9)]['lanes'] > 9
    assert plans[(48, 272)]['idle'] == 4 and plans[(512, 16)]['lanes'] == 2
    assert plans[(1024, 9)]['cg'] == 128 and plans[(1024, 9)]['lanes'] == 1
    assert plans[(2048, 6)]['qb_rounds'] == 2 and plans[(8, 35)]['cg'] == 1

    def arm(C):
        c4 = C // 4
        for lpp, nv, top in ((8, 1, 8), (16, 1, 16), (32, 1, 32), (64, 1, 64), (64, 2, 128), (64, 4, 256)):
            if c4 <= top:
                return lpp, nv, c4 < lpp * nv
    arms = {(C, B * H * W): arm(C) for C, (B, H, W), _ in nb.LN_CASES}
    assert arms[(256, 70)] == (64, 1, False) and arms[(1024, 9)] == (64, 4, False)
    assert arms[(40, 70)] == (16, 1, True) and arms[(260, 20)] == (64, 2, True) and arms[(516, 9)] == (64, 4, True)
    blocks = lib.dmh_lnb_blocks()
    assert arms[(64, 4608)][0] == 16 and 4608 > blocks * (256 // 16)
    assert arms[(8, 10368)][0] == 8 and 10368 > blocks * (256 // 8)
    # sum_over_batch: rows g, g + 16, ...; the unrolled loop needs b + 48 < B; both loops and their edges are in the table
    assert {1, 16, 17, 48, 49, 64, 65} <= set(nb.SOB_B) and {1, 15, 16, 17} <= set(nb.SOB_PER)
    # bgemm: an odd K (the half-filled last instruction), ragged M and N tiles, more than one tile each way
    assert any(K % 2 for _, _, K, _, _ in nb.BGEMM_SHAPES) and any(M > 32 and M % 32 for M, *_ in nb.BGEMM_SHAPES)
    assert any(N > 64 and N % 32 for _, N, *_ in nb.BGEMM_SHAPES)


def test_derived_bounds_accept_fp32_and_reject_a_dropped_term():
    """the elementwise bounds of dmh_sum_over_batch and dmh_bgemm pass a plain fp32 evaluation on the CPU and fail one that
    leaves out a single row / a single k"""
    for B in (2, 17, 113, 1024):
        x = nb.rand((B, 256), 6000 + B)
        ref, bound = nb.sum_over_batch_bound(x)
        seq = torch.zeros(256)
        for b in range(B):
            seq = seq + x[b]
        assert bool(((seq.double() - ref).abs() <= bound).all())
        assert bool(((x.sum(0).double() - ref).abs() <= bound).all())
        assert not bool(((x[:-1].sum(0).double() - ref).abs() <= bound).all())
    for shape in nb.BGEMM_SHAPES:
        a, b = nb.bgemm_inputs(shape)
        for alpha in nb.BGEMM_ALPHAS:
            ref, bound = nb.bgemm_reference(a, b, alpha)
            got = (a @ b) * torch.tensor(alpha, dtype=torch.float32)
            assert bool(((got.double() - ref).abs() <= bound).all()), (shape, alpha)
            short = (a[..., :-1] @ b[..., :-1, :]) * torch.tensor(alpha, dtype=torch.float32)
            assert not bool(((short.double() - ref).abs() <= bound).all()), (shape, alpha)
    x = torch.tensor([0.0, 1.0, 1.5, -3.0], dtype=torch.float64)
    assert nb.ulp32(x).tolist() == [0.0, 2.0 ** -23, 2.0 ** -23, 2.0 ** -22]
