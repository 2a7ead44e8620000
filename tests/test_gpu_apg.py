"""-m gpu: adaptive projected guidance of the conditional sampler (``apg_eta``, ``apg_norm_threshold``, ``apg_momentum``): the
kernels (dmh_apg_coef[_dev], dmh_apg_apply) and cfg.GaussianDiffusion with the switch on, eager and captured.

1. the kernels alone against the float64 statement of tests/apg_cases.py, over its sizes, batches, kinds and pointer phases;
2. the eager loops against a float64 loop fed the same network outputs: per-step coefficients, x_start and image;
3. captured == eager, dedup on == off, 'batched' == 'streams', the capture cache, cond_scale 1, row independence."""
import math

import pytest
import torch

import apg_cases as AC
import guidance_cases as GC
import threshold_cases as TC
from gpu_util import dev
from test_gpu_guidance import _guarded, _recording, _step, g, same
from test_gpu_solver import _cfg_diffusion, _cfg_model, _cond_inputs

pytestmark = pytest.mark.gpu

GUARD = float('nan')                                         # the words around every output: they must stay NaN


# --------------------------------------------------------------------------------------------- 1. the kernels alone
@pytest.fixture(scope='module')
def table():
    """the case table with its float64 references, computed once"""
    from dmhomo_amd import ops
    ragged = tuple(AC.ragged_size(ops.apg_splits, B)[0] for B in AC.BATCHES)
    out = []
    for name, case in AC.cases(ragged):
        case['ref'] = AC.reference(case)
        out.append((name, case))
    return out, ragged


def _untouched(buf, lo, hi):
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all())


def _launch(case, phase, which='calls', dev_struct=False):
    """the case's calls on one running average, every buffer ``phase`` floats off a 16-byte boundary inside guard words -> per
    call (coef (B, 2), run or None, guided), on the CPU"""
    from dmhomo_amd import ops
    off_c, off_n, off_r = phase
    B, n = case[which][0][1].shape
    need = 3 * B * ops.apg_splits(B, n)
    step = _step(cs=case['cs'])
    if dev_struct:
        table_, tt, cursor, cur = ops.step_table([step], [0], dev())
        ops.sampler_seek(cursor, 0, table_, tt, cur, torch.zeros((B,), dtype=torch.int64, device=dev()))
    run = rbuf = None
    if case['beta'] != 0.:
        run, rbuf = _guarded(torch.zeros((B, n)), off_r, GUARD)
    out = []
    for cond, null in case[which]:
        cond, _ = _guarded(cond, off_c)
        null, _ = _guarded(null, off_n)
        wbuf = torch.full((need + 8,), GUARD, device=dev(), dtype=torch.float64)
        cbuf = torch.full((2 * B + 16,), GUARD, device=dev())
        coef = cbuf[8:8 + 2 * B].view(B, 2)
        guided, gbuf = _guarded(torch.full((B, n), 777.), off_c, GUARD)
        args = (cond, null, case['eta'], case['rho'], case['beta'])
        kw = dict(keep=g(case['keep']), run=run, ws=wbuf[4:4 + need], coef=coef)
        got = ops.apg_coef_dev(cur, *args, **kw) if dev_struct else ops.apg_coef(step, *args, **kw)
        assert got is coef
        assert ops.apg_apply(cond, null, coef, keep=g(case['keep']), run=run, out=guided) is guided
        assert _untouched(cbuf, 8, 8 + 2 * B) and _untouched(wbuf, 4, 4 + need) and _untouched(gbuf, 4 + off_c, 4 + off_c + B * n)
        assert rbuf is None or _untouched(rbuf, 4 + off_r, 4 + off_r + B * n)
        out.append((coef.cpu(), None if run is None else run.cpu().clone(), guided.cpu()))
    return out


def _check_case(name, case):
    """-> the worst deviation of a coefficient from the float64 statement, in fp32 ulps of its value"""
    B, n = case['calls'][0][1].shape
    worst = 0.
    w1 = float(case['cs']) - 1.
    for phase in AC.PHASES:
        if phase[2] != phase[1] and case['beta'] == 0.:       # (run alone out of phase: cases with a running average only)
            continue
        what = (name, phase)
        first = _launch(case, phase)
        if phase == AC.PHASES[0]:
            for other in (_launch(case, phase), _launch(case, phase, dev_struct=True)):      # repeatable; the _dev twin
                for a, b in zip(first, other):
                    assert same(a[0], b[0]) and same(a[2], b[2]) and (a[1] is None or same(a[1], b[1])), what
        clean = _launch(case, phase, 'clean') if case['kind'] == 'nan' else None
        run_prev = torch.zeros((B, n))
        for k, ((coef, run, guided), ref) in enumerate(zip(first, case['ref'])):
            cond, null = case['calls'][k]
            c, d = AC.update32(cond, null, case['keep'], case['beta'], run_prev)
            if run is not None:
                assert same(run, d), (what, k, 'run')         # bitwise d + beta * run_prev, torch fp32 on the CPU
                run_prev = run
            if case['kind'] == 'nan':
                row = case['nan_row']
                for b in range(B):
                    if b == row:
                        assert bool(torch.isnan(coef[b]).all()), (what, coef)
                    else:
                        assert same(coef[b], clean[k][0][b]) and bool(torch.isfinite(coef[b]).all()), (what, b, coef)
                        assert same(guided[b], clean[k][2][b]), (what, b)
            else:
                u = AC.ulps(coef, ref['coef'])
                assert bool((u <= AC.ULPS).all()), (what, k, u, coef, ref['coef'])
                worst = max(worst, float(u.max()))
            if case['kind'] == 'equal':
                assert coef.tolist() == [[1., w1]] * B and same(guided, c), what
            if case['kind'] == 'czero':
                assert coef[:, 0].tolist() == [1.] * B, (what, coef)
            if case['kind'] == 'keep':
                dropped = case['keep'] == 0
                assert coef[dropped].tolist() == [[1., w1]] * int(dropped.sum()) and same(guided[dropped], null[dropped]), what
            want = AC.guided32(c, d, coef)                    # bitwise (A * c) + (Cc * d), fp32 ops on the CPU
            if case['kind'] == 'nan':                         # (which NaN a NaN product is differs from machine to machine)
                ok = torch.arange(B) != case['nan_row']
                assert bool(torch.isnan(guided[~ok]).all()) and same(guided[ok], want[ok]), (what, k, 'guided')
            else:
                assert same(guided, want), (what, k, 'guided')
    return worst


@pytest.mark.parametrize('kind', AC.KINDS)
def test_kernels_small_sizes(table, kind):
    cases, ragged = table
    mine = [(name, c) for name, c in cases if c['kind'] == kind and c['calls'][0][1].shape[1] != AC.BIG[0]]
    assert len(mine) == len(AC.SIZES) * len(AC.BATCHES) + len(ragged)
    worst = max(_check_case(name, c) for name, c in mine)
    print(f'[parity] apg {kind}, {len(mine)} cases (n = 1 .. {max(ragged)}): worst |coef - float64| = {worst:.3f} fp32 ulp '
          f'(gate {AC.ULPS:.0f}); run and guided bitwise')


def test_ragged_sizes_are_split(table):
    from dmhomo_amd import ops
    _, ragged = table
    for B, n in zip(AC.BATCHES, ragged):
        s = ops.apg_splits(B, n)
        assert s >= 2 and n % (4 * s) != 0, (B, n, s)


def test_kernels_workload_row(table):
    from dmhomo_amd import ops
    cases, _ = table
    mine = [(name, c) for name, c in cases if c['calls'][0][1].shape[1] == AC.BIG[0]]
    assert len(mine) == 1 and ops.apg_splits(AC.BIG[1], AC.BIG[0]) == 24
    worst = _check_case(*mine[0])
    print(f'[parity] apg {mine[0][0]}: worst |coef - float64| = {worst:.3f} fp32 ulp (gate {AC.ULPS:.0f}); run and guided bitwise')


def test_every_einval_and_every_wrapper_error():
    from dmhomo_amd import _lib, ops
    assert AC.check_einval(_lib, ops) > 60
    x = torch.zeros((2, 3, 4, 4), device=dev())
    step, coef = _step(), torch.ones((2, 2), device=dev())
    cur = torch.zeros((44,), dtype=torch.uint8, device=dev())
    for fn, s in ((ops.apg_coef, step), (ops.apg_coef_dev, cur)):
        for args, kw in (((x, None, 0.), {}),                                          # no null pass
                         ((x, x[:1].clone(), 0.), {}),                                 # null of another shape
                         ((x, x, 0., 0., -0.5), {}),                                   # momentum without a running average
                         ((x, x, 0., 0., 0.), {'run': x.clone()}),                     # a running average without momentum
                         ((x, x, 0., 0., -0.5), {'run': x[:1].clone()}),               # ... of another shape
                         ((x, x, 0.), {'coef': torch.ones((2,), device=dev())}),
                         ((x, x, 0.), {'coef': torch.ones((3, 2), device=dev())}),
                         ((x, x, 0.), {'ws': torch.zeros((5,), device=dev(), dtype=torch.float64)})):
            with pytest.raises(ValueError):
                fn(s, *args, **kw)
        for args, word in (((x, x, 1.5), 'eta'), ((x, x, 0., -1.), 'rho'), ((x, x, 0., float('inf')), 'rho')):
            with pytest.raises(_lib.DmhError, match=word):
                fn(s, *args)
        with pytest.raises(_lib.DmhError, match='beta'):
            fn(s, x, x, 0., 0., 1., run=x.clone())
    for args, kw in (((x, None, coef), {}), ((x, x[:1].clone(), coef), {}), ((x, x, coef[:1]), {}),
                     ((x, x, coef), {'run': x[:1].clone()}), ((x, x, coef), {'out': x[:1].clone()})):
        with pytest.raises(ValueError):
            ops.apg_apply(*args, **kw)
    y, z = x.clone(), x.clone()
    for kw in ({'out': x}, {'out': y}, {'run': z, 'out': z}):
        with pytest.raises(_lib.DmhError, match='overlaps'):
            ops.apg_apply(x, y, coef, **kw)
    with pytest.raises(ValueError):
        ops.apg_splits(0, 4)


# --------------------------------------------------------------------------------------------- 2. the loops, restated
T_, S_, B_, P_ = 100, 5, 3, 0.995
# gates of the loop parity: 10x the worst error measured on MI355X against the float64 loop; the measurements are in
# the docstring of test_loops_vs_float64_loop
GATE_X0, GATE_IMG = 4.4e-6, 4.2e-6
SETTINGS = {'eta0': (0., None, 0.), 'eta.5-rho-momentum': (0.5, 0.5, -0.5)}    # (eta, rho as a part of the first |d|, beta)


def _set(d, eta, rho=0., beta=0.):
    d.apg_eta, d.apg_norm_threshold, d.apg_momentum = eta, rho, beta


def _reference_loop(d, nets, draws, apg, dynamic, cs):
    """the loop in float64 on the recorded network outputs and noise: the update in fp32 (the running average too), sums and
    coefficients in float64, the guided logits, threshold and step in float64 -> per step (coef, x_start, img, s)"""
    eta, rho, beta = apg
    cpu = lambda t: None if t is None else t.cpu()
    img, hist, ni, run, out = draws[0].cpu().double(), None, 1, None, []
    ones = torch.ones(img.shape[0])
    for (time, step, _), (cond, null, keep) in zip(d._sampler_steps(True, cs), nets):
        cond, null, keep = cpu(cond), cpu(null), cpu(keep)
        if beta != 0. and run is None:
            run = torch.zeros_like(null)
        c, dd = AC.update32(cond, null, keep, beta, run)
        if beta != 0.:
            run = dd
        B = c.shape[0]
        coef, s, _ = AC.coef_ref(c.reshape(B, -1), dd.reshape(B, -1), cs, eta, rho)
        guided = AC.guided_ref(c, dd, coef)
        noise = None
        if step.mode == 0:
            noise, ni = draws[ni].cpu(), ni + 1
        thr = None
        if dynamic:
            raw = GC.statement(step, guided, None, None, img, noise, hist, None, ones)[2]
            thr = TC.threshold_ref(raw, P_)[1]
        img, x0, _ = GC.statement(step, guided, None, None, img, noise, hist, thr, ones)
        hist = x0
        out.append((coef, x0, img, s))
    assert ni == len(draws)
    return out


def _loop_setup(sampler, clip_mode, monkeypatch, drop=0.5):
    m, _ = _cfg_model(drop)
    d = _cfg_diffusion(m, size=16, T=T_, S=S_, objective='pred_x0' if sampler == 'ddim' else 'pred_v')
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile = sampler, clip_mode, P_
    nets, draws = _recording(d, monkeypatch)
    ins = tuple(g(t) for t in _cond_inputs(B_, 16))
    return d, nets, draws, ins


def _eager(d, ins, sampler, seed=11):
    from dmhomo_amd import ops
    c, rf01, fl, mk = ins
    torch.manual_seed(seed)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, (B_, 6, 16, 16), GC.CS, trace=trace)
    return got, trace


@pytest.mark.parametrize('setting', list(SETTINGS))
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_vs_float64_loop(sampler, clip_mode, setting, monkeypatch):
    """measured on MI355X over the eight runs: coefficients <= 0.497 fp32 ulp of their value (gate apg_cases.ULPS = 2), per-step
    x_start <= 4.40e-7, image <= 4.18e-7 (gates 10x that: GATE_X0 / GATE_IMG)"""
    from dmhomo_amd import ops
    d, nets, draws, ins = _loop_setup(sampler, clip_mode, monkeypatch)
    eta, rho_part, beta = SETTINGS[setting]
    c, rf01, fl, mk = ins
    torch.manual_seed(11)
    before = d.sample(c, rf01, fl, mk, cond_scale=GC.CS)[0]   # the switch has never been on
    nets.clear(), draws.clear()
    rho = 0.
    if rho_part is not None:
        # the first network call does not depend on the setting: its recorded |d| per row chooses a cap that binds in the
        # widest row (a dropped row has d == 0 and the cap never binds there)
        _set(d, eta, 0., beta)
        _eager(d, ins, sampler)
        cond, null, keep = (None if t is None else t.cpu() for t in nets[0])
        norms = AC.sums(*AC.update32(cond, null, keep))[0].sqrt()
        rho = rho_part * float(norms.max())
        assert rho > 0.
        nets.clear(), draws.clear()
    _set(d, eta, rho, beta)
    got, trace = _eager(d, ins, sampler)
    assert len(trace) == len(nets) == S_ and len(draws) == 1 + (S_ - 1 if sampler == 'ddim' else 0)
    ref = _reference_loop(d, nets, draws, (eta, rho, beta), clip_mode == 'dynamic', GC.CS)
    ec = max(float(AC.ulps(e['apg'].cpu(), r[0]).max()) for e, r in zip(trace, ref))
    ex = max(float((e['x_start'].cpu().double() - r[1]).abs().max()) for e, r in zip(trace, ref))
    ei = max(float((e['img'].cpu().double() - r[2]).abs().max()) for e, r in zip(trace, ref))
    coefs = torch.stack([e['apg'] for e in trace])
    print(f'[parity] apg {setting} (rho {rho:.3f}) {sampler} {clip_mode}: A in {float(coefs[..., 0].min()):.3f} .. '
          f'{float(coefs[..., 0].max()):.3f}, Cc in {float(coefs[..., 1].min()):.3f} .. {float(coefs[..., 1].max()):.3f}; '
          f'max|coef - float64| = {ec:.3f} ulp, max|x_start - float64| = {ex:.2e}, max|img - float64| = {ei:.2e}')
    assert all(e['apg'].shape == (B_, 2) for e in trace) and ('thr' in trace[0]) == (clip_mode == 'dynamic')
    if rho_part is not None:
        assert bool((ref[0][3] < 1.).any()) and float(coefs[0, :, 1].min()) < GC.CS - 1.       # the cap binds at the first step
    else:
        assert bool((coefs[..., 1] == GC.CS - 1.).all())
    assert ec <= AC.ULPS and ex <= GATE_X0 and ei <= GATE_IMG, (ec, ex, ei)
    assert torch.equal(got, ops.affine(trace[-1]['img'], 0.5, 0.5))
    # sample() is the same call; off is another sample, and exactly the one it was before the switch was ever on
    torch.manual_seed(11)
    assert torch.equal(d.sample(c, rf01, fl, mk, cond_scale=GC.CS)[0], got)
    _set(d, None, rho, beta)
    torch.manual_seed(11)
    off = d.sample(c, rf01, fl, mk, cond_scale=GC.CS)[0]
    assert not torch.equal(off, got) and torch.equal(off, before)


# --------------------------------------------------------------------------------------------- 3. captured, dedup, streams
def _keyed_runner(d, ins, seed=5, first_id=40):
    c, rf01, fl, mk = ins

    def run(lo=0, hi=None, **kw):
        hi = c.shape[0] if hi is None else hi
        d.rng.key_by_sample(seed, range(first_id + lo, first_id + hi), dev())
        return d.sample(c[lo:hi].contiguous(), rf01[lo:hi].contiguous(), fl[lo:hi].contiguous(), mk[lo:hi].contiguous(),
                        **kw)[0].clone()
    return run


@pytest.mark.parametrize('beta', [0., -0.5], ids=['no-momentum', 'momentum'])
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_captured_equals_eager_in_every_mode(sampler, clip_mode, beta):
    """bitwise: hip_graph against the eager loop under 'batched' and 'streams', dedup_dropped_rows on and off (the eager loop
    itself gives one tensor in all four modes: rows are independent and a dropped row's update is exactly 0)"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.sampler, d.clip_mode = sampler, clip_mode
    _set(d, 0.25, 20., beta)
    d.rng = cfg.DeviceRng()
    run = _keyed_runner(d, tuple(g(t) for t in _cond_inputs(B_, 16)))
    want = run()
    for mode in ('batched', 'streams'):
        for dedup in (False, True):
            m.cfg_mode, m.dedup_dropped_rows = mode, dedup
            d.hip_graph = False
            assert torch.equal(run(), want), (mode, dedup, 'eager')
            d.hip_graph = True
            assert torch.equal(run(), want), (mode, dedup, 'captured')
            assert torch.equal(run(), want), (mode, dedup, 'replayed: fill zeroes the running average')
    assert d.graph_captures == 4
    d.hip_graph, m.dedup_dropped_rows, m.cfg_mode = False, False, 'batched'
    _set(d, None)
    assert not torch.equal(run(), want)


def test_capture_cache_counts():
    """a second call with the same settings captures nothing, a changed apg_eta exactly once, None is the default's entry"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.rng = cfg.DeviceRng()
    d.hip_graph = True
    run = _keyed_runner(d, tuple(g(t) for t in _cond_inputs(B_, 16)))
    default = run()
    assert d.graph_captures == 1
    _set(d, 0., 20., -0.5)
    a = run()
    assert d.graph_captures == 2 and not torch.equal(a, default)
    assert torch.equal(run(), a) and d.graph_captures == 2
    _set(d, 0.5, 20., -0.5)
    b = run()
    assert d.graph_captures == 3 and not torch.equal(b, a)
    _set(d, None, 20., -0.5)                                  # off: the other two values are not in the key
    assert torch.equal(run(), default) and d.graph_captures == 3
    _set(d, 0., 20., -0.5)
    assert torch.equal(run(), a) and d.graph_captures == 3
    d.hip_graph = False
    assert torch.equal(run(), a)
    _set(d, None)
    assert torch.equal(run(), default)


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_cond_scale_1_ignores_the_settings(sampler):
    """no null pass, nothing to project: bit for bit the default, eager and captured"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.sampler = sampler
    d.rng = cfg.DeviceRng()
    run = _keyed_runner(d, tuple(g(t) for t in _cond_inputs(2, 16)))
    for clip_mode in ('static', 'dynamic'):
        d.clip_mode, d.hip_graph = clip_mode, False
        _set(d, None)
        want = run(cond_scale=1.)
        _set(d, 0., 2., -0.5)
        assert torch.equal(run(cond_scale=1.), want)
        d.hip_graph = True
        assert torch.equal(run(cond_scale=1.), want)
        assert not torch.equal(run(cond_scale=3.), want)
    d.hip_graph = False


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_row_independence(sampler):
    """a B = 3 call == the three B = 1 calls with the same global sample ids, bitwise: a row's coefficients, its cap and its
    running average come from that row alone"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.sampler, d.clip_mode = sampler, 'dynamic'
    _set(d, 0., 20., -0.5)
    d.rng = cfg.DeviceRng()
    run = _keyed_runner(d, tuple(g(t) for t in _cond_inputs(B_, 16)))
    whole = run()
    assert not torch.equal(whole[0], whole[1]) and math.isfinite(float(whole.sum()))
    for b in range(B_):
        assert torch.equal(run(b, b + 1)[0], whole[b]), b
    d.hip_graph = True
    assert torch.equal(run(0, 1)[0], whole[0])
    d.hip_graph = False
