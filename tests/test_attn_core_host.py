"""CPU half of tests/test_gpu_attn_core.py: the launch plan tests/attn_core_cases.py restates from csrc/attention.hip and
csrc/attention_backward.hip is the library's, every pixel count of the tables reaches the split, chunk and tile boundary its
row names, every case has a finite fp32 yardstick under the cap and inputs that do what their kind claims, the float64
references agree with an independent statement, and the gates reject four wrong kernels while accepting plain fp32.

The split count, the partial size and the workspace size have exports (pure host functions), and they pin LA_NS, LA_PART,
LAB_NS, the colsum128 chunk and the sizes of the five workspace regions; the kernel files point back at this test from
those.  The ORDER of the regions has no export: the GPU test reads dctx and t back at the restated offsets.  Nothing on the
CPU depends on the 32-pixel tiles and the 4-tile blocks (LA_TILES, LAB_TILES, the attention tiles): they only choose the
pixel counts of the tables, and the sentinel and parity runs of tests/test_gpu_attn_core.py around them are their test."""
import math

import pytest
import torch

import attn_core_cases as ac


@pytest.fixture(scope='module')
def lib():
    from dmhomo_amd import _lib
    return _lib.lib()


def _plan_ns():
    around = {k * step + d for k in range(1, 10) for step in (128, 256) for d in (-1, 0, 1)}
    return sorted(set(ac.LA_N) | set(ac.ATT_N) | around)


def test_plan_matches_the_library(lib):
    """dmh_linattn_splits, dmh_linattn_partial_floats and dmh_linattn_bwd_workspace_floats against the restatement, at
    every n of the tables and around every multiple of the split and of the chunk; the workspace total is the sum of the
    five restated regions, which lie back to back in the restated order"""
    for n in _plan_ns():
        assert lib.dmh_linattn_splits(n) == ac.splits(n) == ac.cdiv(n, ac.LA_NS), n
        for B in (1, 2, 16):
            assert lib.dmh_linattn_partial_floats(B, n) == ac.partial_floats(B, n), (B, n)
            reg = ac.bwd_regions(B, n)
            assert list(reg) == ['qs', 'dctx_part', 'dctx', 't_part', 't']
            off = 0
            for o, size in reg.values():
                assert o == off and size > 0
                off += size
            assert lib.dmh_linattn_bwd_workspace_floats(B, n) == off == ac.bwd_workspace_floats(B, n), (B, n)
            assert reg['qs'][1] == B * n * 128 and reg['dctx'][1] == B * 4096 and reg['t'][1] == B * 128
            assert reg['dctx_part'][1] == ac.cdiv(n, ac.LAB_NS) * reg['dctx'][1]
            assert reg['t_part'][1] == ac.cdiv(n, ac.COLSUM_CHUNK) * reg['t'][1]


def test_case_tables_reach_the_branches_they_name(lib):
    """n -> (splits, pixels in the last split, colsum128 chunks, pixels in the last chunk, key tiles, keys in the last tile)"""
    want = {1: (1, 1, 1, 1, 1, 1),
            31: (1, 31, 1, 31, 1, 31),
            32: (1, 32, 1, 32, 1, 32),                # exactly one apply / backward tile, one key tile
            33: (1, 33, 1, 33, 2, 1),                 # a second 32-pixel tile / key tile of one
            63: (1, 63, 1, 63, 2, 31),
            64: (1, 64, 1, 64, 2, 32),
            65: (1, 65, 1, 65, 3, 1),
            127: (1, 127, 1, 127, 4, 31),
            128: (1, 128, 1, 128, 4, 32),             # exactly one split and one 4-tile block
            129: (2, 1, 1, 129, 5, 1),                # a second split of one pixel (upper lane half all masked), a second block
            255: (2, 127, 1, 255, 8, 31),
            256: (2, 128, 1, 256, 8, 32),             # exactly one colsum128 chunk
            257: (3, 1, 2, 1, 9, 1),                  # a third split and a second chunk of one pixel
            1000: (8, 104, 4, 232, 32, 8),
            1025: (9, 1, 5, 1, 33, 1)}
    assert set(want) == set(ac.LA_N) | set(ac.ATT_N)
    for n, w in want.items():
        assert ac.row(n) == w, (n, ac.row(n), w)
        assert lib.dmh_linattn_splits(n) == w[0]
    for cases, ns, kind_n, kinds in ((ac.LA_CASES, ac.LA_N, ac.LA_KIND_N, ac.LA_KINDS),
                                     (ac.ATT_CASES, ac.ATT_N, ac.ATT_KIND_N, ac.ATT_KINDS)):
        have = set(cases)
        assert len(have) == len(cases)
        assert all(ac.Case(n, 2, 'plain') in have for n in ns)
        assert all(ac.Case(n, 2, k) in have for n in kind_n for k in kinds)
        assert {c.B for c in have if c.n == 257} == {1, 2, 3} and {c.B for c in have if c.n != 257} == {2}
    assert set(ac.LA_KINDS) == {'plain', 'sharp_k', 'sharp_q', 'rising', 'falling', 'offset90', 'v_outlier'}
    assert set(ac.ATT_KINDS) == {'plain', 'big_logits', 'rising', 'falling', 'last_key', 'first_key', 'v_outlier'}


def _yardsticks(cid, e32):
    for name, e in e32.items():
        w = float(e.max())
        print(f'[yardstick] {cid} {name}: e32={w:.3e}')
        assert math.isfinite(w) and w <= ac.CAP, f'{name}: e32 = {w:.3e} is over the cap {ac.CAP:.0e}: soften the kind'


@pytest.mark.parametrize('case', ac.LA_CASES, ids=ac.case_id)
def test_linattn_yardstick_and_input_conditions(case):
    r = ac.la_reference(case)
    cid = ac.case_id(case)
    _yardsticks(cid, r['e32'])
    for dt in ('r64', 'r32'):
        for key, t in r[dt].items():
            assert bool(torch.isfinite(t).all()), (dt, key)
    assert bool(torch.isfinite(r['lse']).all()) and bool(torch.isfinite(r['wm']).all())
    assert float(r['r64']['out'].abs().max()) > 0 and float(r['r64']['dqkv'].abs().max()) > 0
    k = r['r64']['k']
    if case.kind in ('rising', 'falling') and ac.splits(case.n) >= 2:
        frac = float((ac.neighbour_weight(k) < 1e-3).double().mean())
        print(f'[yardstick] {cid}: {frac:.2f} of the columns have a neighbouring-split weight below 1e-3')
        assert frac >= 0.5, frac
    if case.kind == 'sharp_k':
        under = ac.underflow_fraction(k)
        print(f'[yardstick] {cid}: {under:.3f} of the pixels underflow in some column')
        assert under > 0.9
    if case.kind == 'offset90':      # exp of the raw logits overflows fp32 (88.7) / underflows to zero without the max
        q = ac.heads(r['inp']['qkv'])[0]
        assert float(k.min()) > 80 and float(q.max()) < -80
    if case.kind == 'v_outlier' and case.n > ac.V_OUTLIER_AT:
        vp = r['r64']['v'].abs().amax((1, 2))                                # (B, n)
        mask = torch.ones(case.n, dtype=torch.bool)
        mask[ac.V_OUTLIER_AT::128] = False
        assert float(vp[:, ac.V_OUTLIER_AT::128].min() / vp[:, mask].max()) >= 2.0 ** 8


@pytest.mark.parametrize('case', ac.ATT_CASES, ids=ac.case_id)
def test_attention_yardstick_and_input_conditions(case):
    r = ac.att_reference(case)
    cid = ac.case_id(case)
    _yardsticks(cid, r['e32'])
    assert bool(torch.isfinite(r['out']).all()) and float(r['out'].abs().max()) > 0
    if case.kind in ac.DOMINANT:
        # the softmax weight of the dominant key is 1.0 in fp32 for every query: out is that key's v, the yardstick exact
        assert r['dominant_weight'] == 1.0, r['dominant_weight']
        assert float(r['e32']['out'].max()) == 0.0
        j = ac.dominant_key(case)
        v = r['inp']['qkv'][:, j, 256:].double()
        assert float((r['out'] - v[:, None, :]).abs().max()) < 1e-30
    if case.kind == 'rising' and case.n >= 2 * ac.ATT_TILE:
        # the ramp moves a logit by 3 * scale * sum_d q[d] per key tile, about 4.5 z for a standard normal z, against tile
        # maxima that scatter by about 1: a query with z above ~ 0.5 (a third of them) meets a larger maximum at EVERY full
        # key tile, so alpha < 1 each time; asked for: a tenth of the queries (the gate is per (row, head), over its queries)
        q, k, _ = ac.heads(r['inp']['qkv'].double())
        sim = torch.einsum('bhdi,bhdj->bhij', q * ac.SCALE, k)
        full = case.n // ac.ATT_TILE
        tmax = sim[..., :full * ac.ATT_TILE].reshape(sim.shape[:3] + (full, ac.ATT_TILE)).amax(4)
        every = (tmax[..., 1:] > tmax.cummax(3).values[..., :-1]).all(3).double().mean().item()
        print(f'[yardstick] {cid}: {every:.2f} of the queries raise the running maximum at every full key tile')
        assert every >= 0.1, every


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize('case', [ac.Case(257, 2, 'plain'), ac.Case(1000, 2, 'rising'), ac.Case(33, 2, 'offset90')],
                         ids=ac.case_id)
def test_references_agree_with_the_kernel_header_formulas(case):
    """the backward as the header of csrc/attention_backward.hip writes it, in float64 from the float64 ctx and (M, S),
    against float64 autograd: dq, dk, dv, dctx and t to 1e-12 of each tensor's maximum; and the merge of the float64
    per-split statistics against the direct context"""
    r = ac.la_reference(case)
    r64, inp = r['r64'], r['inp']
    f = ac.la_formulas(inp['qkv'].double(), r64['ctx'], r64['M'], r64['S'], inp['dout'].double())
    for key in ('dqkv', 'dctx', 't'):
        e = _rel(f[key], r64[key])
        print(f'[yardstick] {ac.case_id(case)} formulas vs autograd {key}: {e:.3e}')
        assert e <= 1e-12, (key, e)
    kp, vp = ac.split_pad(r64['k'], r64['v'])
    m = kp.amax(4)
    w = (kp - m[..., None]).exp()
    ctx, M, S = ac.merge_splits(m.permute(0, 3, 1, 2), w.sum(4).permute(0, 3, 1, 2),
                                torch.einsum('bhdsl,bhesl->bshde', w, vp), case.n)
    assert _rel(ctx, r64['ctx']) <= 1e-12 and torch.equal(M, r64['M']) and _rel(S, r64['S']) <= 1e-12


MUTATION_CASE = ac.Case(257, 2, 'plain')      # three context splits and two colsum128 chunks, the last of each one pixel


def _ratio(kind, err, e32, floor):
    """-> (the worst unit's err / gate, the best unit's)"""
    g = ac.gate(kind, e32, floor)
    return float((err / g).max()), float((err / g).min())


def test_gates_accept_fp32_and_reject_a_merge_without_weights():
    case = MUTATION_CASE
    r = ac.la_reference(case)
    kp, vp = ac.split_pad(r['r32']['k'], r['r32']['v'])
    m = kp.amax(4)
    w = (kp - m[..., None]).exp()
    parts = (m.permute(0, 3, 1, 2), w.sum(4).permute(0, 3, 1, 2), torch.einsum('bhdsl,bhesl->bshde', w, vp))
    good, M, S = ac.merge_splits(*parts, case.n)
    bad, _, Sbad = ac.merge_splits(*parts, case.n, weights=False)
    assert torch.equal(M, r['M32'])
    hi, _ = _ratio(case.kind, ac.ctx_err(good, r['r64']['ctx']), r['e32']['ctx'], ac.FWD)
    assert hi <= 1.0, hi
    assert _ratio(case.kind, ac.vec_err(S, r['r64']['S']), r['e32']['S'], ac.FWD)[0] <= 1.0
    hi, lo = _ratio(case.kind, ac.ctx_err(bad, r['r64']['ctx']), r['e32']['ctx'], ac.FWD)
    print(f'[mutation] merge without exp(m - M): ctx misses its gate by {lo:.3g}x ... {hi:.3g}x')
    assert lo >= 100.0, lo
    hi, lo = _ratio(case.kind, ac.vec_err(Sbad, r['r64']['S']), r['e32']['S'], ac.FWD)
    print(f'[mutation] merge without exp(m - M): S misses its gate by {lo:.3g}x ... {hi:.3g}x')
    assert lo >= 100.0, lo


def test_gates_accept_fp32_and_reject_an_online_softmax_without_alpha():
    case = MUTATION_CASE
    r = ac.att_reference(case)
    qkv = r['inp']['qkv']
    good = ac.att_online(qkv, torch.float32)
    bad = ac.att_online(qkv, torch.float32, rescale=False)
    hi, _ = _ratio(case.kind, ac.bh_err(good, r['out']), r['e32']['out'], ac.FWD)
    assert hi <= 1.0, hi
    hi, lo = _ratio(case.kind, ac.bh_err(bad, r['out']), r['e32']['out'], ac.FWD)
    print(f'[mutation] online softmax without the alpha rescale: out misses its gate by {lo:.3g}x ... {hi:.3g}x')
    assert lo >= 100.0, lo


def test_gates_accept_fp32_and_reject_a_dropped_last_chunk_or_split():
    case = MUTATION_CASE
    r = ac.la_reference(case)
    inp, r64, e32 = r['inp'], r['r64'], r['e32']
    args = (inp['qkv'], r64['ctx'].float(), r64['M'].float(), r64['S'].float(), inp['dout'])

    def ratios(f):
        out = dict(dctx=_ratio(case.kind, ac.ctx_err(f['dctx'], r64['dctx']), e32['dctx'], ac.GRAD),
                   t=_ratio(case.kind, ac.vec_err(f['t'], r64['t']), e32['t'], ac.GRAD))
        for name, e in ac.dqkv_err(f['dqkv'], r64['dqkv']).items():
            out[name] = _ratio(case.kind, e, e32[name], ac.GRAD)
        return out

    good = ratios(ac.la_formulas(*args))
    assert all(hi <= 1.0 for hi, _ in good.values()), good
    no_chunk = ratios(ac.la_formulas(*args, drop_last_chunk=True))
    print(f'[mutation] t without the last 256-pixel chunk (one pixel): t misses its gate by {no_chunk["t"][1]:.3g}x ... '
          f'{no_chunk["t"][0]:.3g}x, dk by {no_chunk["dk"][1]:.3g}x ... {no_chunk["dk"][0]:.3g}x')
    assert no_chunk['t'][1] >= 100.0 and no_chunk['dk'][1] >= 100.0, no_chunk
    assert no_chunk['dctx'][0] <= 1.0 and no_chunk['dq'][0] <= 1.0 and no_chunk['dv'][0] <= 1.0
    no_split = ratios(ac.la_formulas(*args, drop_last_split=True))
    print(f'[mutation] dctx without the last 128-pixel split (one pixel): dctx misses its gate by {no_split["dctx"][1]:.3g}x '
          f'... {no_split["dctx"][0]:.3g}x, dk by {no_split["dk"][1]:.3g}x ..., dv by {no_split["dv"][1]:.3g}x ...')
    assert no_split['dctx'][1] >= 100.0 and no_split['dk'][1] >= 100.0 and no_split['dv'][1] >= 100.0, no_split
    assert no_split['dq'][0] <= 1.0


@pytest.mark.parametrize('n', ac.ATT_N)
def test_constant_v_gate_accepts_an_fp32_online_softmax(n):
    """the plain-key form of the constant-v known answer: its gate (10 x plain fp32 torch, between 4 ulps and the summation
    bound) accepts the key-tile loop in fp32 on the CPU and rejects the loop without the alpha rescale by 100 x wherever
    there is more than one key tile; the equal-key form is exact in that loop"""
    qkv = ac.att_constant_v(n, equal_keys=False)
    gate, e32 = ac.constant_v_gate(qkv)
    good = ac.constant_v_rel(ac.att_online(qkv, torch.float32), qkv)
    print(f'[yardstick] n{n} constant v, plain keys: fp32 online softmax {good:.3e}, e32={e32:.3e}, gate={gate:.3e}')
    assert 2.0 ** -22 <= gate <= ac.constant_v_bound(n) and good <= gate
    if n > ac.ATT_TILE:
        bad = ac.constant_v_rel(ac.att_online(qkv, torch.float32, rescale=False), qkv)
        assert bad >= 100 * gate, (bad, gate)
    eq = ac.att_constant_v(n, equal_keys=True)
    assert ac.constant_v_rel(ac.att_online(eq, torch.float32), eq) <= 2.0 ** -23
