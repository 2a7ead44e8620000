"""-m gpu: dynamic thresholding of the guided sampler (``clip_mode = 'dynamic'``): the row-quantile selector
(dmh_row_quantile_abs), the threshold and step kernels (dmh_sampler_threshold[_dev], dmh_sampler_step_thr[_dev]) and
cfg.GaussianDiffusion with the switch on, eager and captured.

1. the selector alone against a float64 sort, over the sizes, percentiles and kinds of tests/threshold_cases.py;
2. argument validation of the new entry points;
3. the step kernels alone: against a float64 statement, against each other, and against the existing step kernels where the
   threshold is 1;
4. the sampler against a restatement written here (the oracle's network and raw predictions per step; threshold and update in
   float64), DDIM at eta 0 and the multistep solver, on weights that saturate and on weights that straddle the threshold;
5. dynamic == static where no quantile exceeds 1;
6. the captured loop equals the eager loop, bitwise, output and generator;
7. dedup_dropped_rows and the keyed generator's row independence."""
import ctypes
import math

import pytest
import torch

import threshold_cases as TC
from gpu_util import ReplayDeviceRng, dev, report
from oracle import diffusion as OD
from oracle import unet as OU
from test_gpu_solver import _cfg_diffusion, _cfg_model, _coefficients, _cond_inputs

pytestmark = pytest.mark.gpu


def g(x):
    return x.to(dev())


def bits(x):
    return x.contiguous().view(torch.int32)


def same(a, b):
    """bitwise, NaN included"""
    return torch.equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------- 1. the selector alone
@pytest.fixture(scope='module')
def selector_cases():
    return TC.selector_cases()


def _check_selector(name, x, p, kinds):
    """one case: rows at a 16-byte boundary and one float past it, inside NaN guards (a read past the rows would answer NaN);
    the result between guard floats; two calls; the floor; every row against the float64 sort -> the worst interpolation error
    as a fraction of its bound"""
    from dmhomo_amd import ops
    B, n = x.shape
    k, frac = TC.rank_of(p, n)
    worst, first = 0., None
    for off in (0, 1):
        buf = torch.full((B * n + 8,), float('nan'), device=dev())
        xd = buf[off:off + B * n].view(B, n)
        xd.copy_(x)
        obuf = torch.full((B + 16,), 777., device=dev())
        out = obuf[8:8 + B]
        assert ops.row_quantile_abs(xd, k, frac, 0., out=out) is out
        assert bool((obuf[:8] == 777.).all()) and bool((obuf[8 + B:] == 777.).all()), name
        assert same(ops.row_quantile_abs(xd, k, frac), out), name           # bitwise repeatable
        first = out.clone() if first is None else first
        assert same(out, first), (name, 'alignment')
        floored = ops.row_quantile_abs(xd, k, frac, 1.).cpu()
        got = out.cpu()
        want_floored = torch.where(got < 1., torch.ones_like(got), got)     # (NaN stays)
        assert same(floored, want_floored), (name, 'floor')
        for b, kind in enumerate(kinds):
            if kind == 'nan':
                assert math.isnan(float(got[b])), (name, b)
                continue
            _, _, a, bb, q = TC.quantile_ref(x[b], p)
            o = float(got[b])
            if frac == 0. or a == bb:
                assert same(got[b:b + 1], torch.tensor([a], dtype=torch.float32)), (name, b, o, a)
            elif math.isinf(bb):
                assert o == bb, (name, b, o)
            else:
                bound = 4. * 2. ** -24 * bb + 2. ** -148
                assert a <= o <= bb and abs(o - q) <= bound, (name, b, o, a, bb, q)
                worst = max(worst, abs(o - q) / bound)
    return worst


def test_selector_small_sizes(selector_cases):
    small = [c for c in selector_cases if c[1].shape[1] in TC.SIZES]
    assert len(small) == len(TC.SIZES) * 6 * 2
    worst = max(_check_selector(*c) for c in small)
    print(f'[parity] row_quantile_abs, {len(small)} cases: worst interpolation error = {worst:.3f} of its bound '
          f'(4 * 2^-24 * v[k+1] + 2^-148)')


@pytest.mark.parametrize('shape', [(25, 98304), (2, 393216)], ids=['workload-row', '256x256-row'])
def test_selector_large_rows(selector_cases, shape):
    case, = [c for c in selector_cases if tuple(c[1].shape) == shape]
    worst = _check_selector(*case)
    print(f'[parity] row_quantile_abs {shape}: worst interpolation error = {worst:.3f} of its bound')


# --------------------------------------------------------------------------------------------- 2. argument validation
RC, RM1, SA, S1M, C0, C1, C2, CS = 1.3, 0.8, 0.7, 0.6, 0.9, 0.3, -0.4, 3.


def _step(objective, clip, mode, c2):
    from dmhomo_amd import _lib
    return _lib.DmhStep(objective=objective, clip=clip, mode=mode, cond_scale=CS, sqrt_recip_ac=RC, sqrt_recipm1_ac=RM1,
                        sqrt_ac=SA, sqrt_1m_ac=S1M, c0=C0, c1=C1, c2=c2)


def test_arguments_are_validated():
    from dmhomo_amd import _lib, ops
    x = torch.zeros((2, 3, 4, 4), device=dev())
    n = 48
    keep = torch.ones((2,), dtype=torch.uint8, device=dev())
    thr = torch.ones((2,), device=dev())
    flat = x.view(2, n)
    for k, frac in ((-1, 0.), (n, 0.), (0, 1.), (0, -0.25), (0, float('nan')), (n - 1, 0.5)):
        with pytest.raises(_lib.DmhError, match='rank'):
            ops.row_quantile_abs(flat, k, frac)
        for fn, s in ((ops.sampler_threshold, _step(1, 1, ops.MODE_LAST, 0.)),
                      (ops.sampler_threshold_dev, torch.zeros((44,), dtype=torch.uint8, device=dev()))):
            with pytest.raises(_lib.DmhError, match='rank'):
                fn(s, x, None, x, k, frac)
    with pytest.raises(_lib.DmhError, match='floor'):
        ops.row_quantile_abs(flat, 0, 0., floor=float('nan'))
    with pytest.raises(ValueError):
        ops.row_quantile_abs(flat, 0, 0., out=torch.zeros((3,), device=dev()))
    cur = torch.zeros((44,), dtype=torch.uint8, device=dev())
    last, ddim, ms = _step(1, 1, ops.MODE_LAST, 0.), _step(1, 1, ops.MODE_DDIM, 0.), _step(1, 1, ops.MODE_MULTISTEP, 0.)
    with pytest.raises(_lib.DmhError, match='keep'):
        ops.sampler_threshold(last, x, None, x, 0, 0., keep=keep)
    with pytest.raises(_lib.DmhError, match='keep'):
        ops.sampler_threshold_dev(cur, x, None, x, 0, 0., keep=keep)
    with pytest.raises(_lib.DmhError, match='enum'):
        ops.sampler_threshold(_step(3, 1, ops.MODE_LAST, 0.), x, None, x, 0, 0.)
    with pytest.raises(ValueError):
        ops.sampler_threshold(last, x, None, x, 0, 0., thr=torch.zeros((3,), device=dev()))
    with pytest.raises(ValueError):
        ops.sampler_threshold(last, x, None, x, 0, 0., x0_raw=x[:1].clone())
    with pytest.raises(_lib.DmhError, match='noise'):        # a DDIM entry without noise
        ops.sampler_step_thr(ddim, x, None, x, None, None, thr)
    with pytest.raises(_lib.DmhError, match='hist'):         # a multistep entry without history
        ops.sampler_step_thr(ms, x, None, x, None, None, thr)
    with pytest.raises(_lib.DmhError, match='enum'):         # the DDPM posterior step has no thresholded form
        ops.sampler_step_thr(_step(1, 1, ops.MODE_DDPM, 0.), x, None, x, x.clone(), None, thr)
    with pytest.raises(_lib.DmhError, match='enum'):
        ops.sampler_step_thr(_step(-1, 1, ops.MODE_LAST, 0.), x, None, x, None, None, thr)
    for fn, s in ((ops.sampler_step_thr, last), (ops.sampler_step_thr_dev, cur)):
        with pytest.raises(_lib.DmhError, match='exclude'):
            fn(s, x, None, x, x.clone(), x.clone(), thr)
        with pytest.raises(_lib.DmhError, match='keep'):
            fn(s, x, None, x, None, None, thr, keep=keep)
        with pytest.raises(ValueError):
            fn(s, x, None, x, None, None, thr[:1])
        with pytest.raises(ValueError):
            fn(s, x, None, x, None, x[:1].clone(), thr)
    p = lambda t: _lib.ptr(t)
    for name, s in (('dmh_sampler_step_thr', ctypes.byref(last)), ('dmh_sampler_step_thr_dev', _lib.ptr(cur, torch.uint8))):
        for total, per_row in ((96, 0), (96, 36), (0, 48)):  # thr holds one value per row of per_row elements
            with pytest.raises(_lib.DmhError, match='per_row'):
                _lib.call(name, s, p(x), None, p(x), None, None, p(thr), p(x), None, total, None, per_row)
        with pytest.raises(_lib.DmhError, match='null'):
            _lib.call(name, s, p(x), None, p(x), None, None, None, p(x), None, 96, None, 48)


# --------------------------------------------------------------------------------------------- 3. the step kernels alone
@pytest.mark.parametrize('shape', [(2, 3, 3, 5), (2, 3, 4, 5)], ids=['1-pixel', '4-pixel'])
def test_step_kernels_alone(shape):
    from dmhomo_amd import ops
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(3)
    mc0 = g(torch.randn(shape, generator=gen) * 1.5)
    mn = g(torch.randn(shape, generator=gen) * 1.5)
    x = g(torch.randn(shape, generator=gen))
    hist_rand = g(torch.randn(shape, generator=gen))
    noise_rand = g(torch.randn(shape, generator=gen))
    keep = g(torch.tensor([1, 0], dtype=torch.uint8))        # row 1 dropped: its conditional logits are never read
    tcond = torch.zeros((B,), dtype=torch.int64, device=dev())
    thr = g(torch.tensor([1., 2.5]))
    ones = torch.ones_like(thr)
    thr_nan = g(torch.tensor([1., float('nan')]))
    mc = mc0.clone()
    mc[0, 1, 2, 3] = float('nan')                            # (a kept row)
    nan_at = torch.zeros(shape, dtype=torch.bool, device=dev())
    nan_at[0, 1, 2, 3] = True
    row1 = torch.zeros(shape, dtype=torch.bool, device=dev())
    row1[1] = True
    worst, checked, above = 0., 0, 0
    for objective in (0, 1, 2):
        for clip in (0, 1):
            for guided in (True, False):
                for kind in ('ddim', 'last', 'first', 'second'):
                    mode = {'ddim': ops.MODE_DDIM, 'last': ops.MODE_LAST}.get(kind, ops.MODE_MULTISTEP)
                    step = _step(objective, clip, mode, C2 if kind in ('ddim', 'second') else 0.)
                    multistep = kind in ('first', 'second')
                    noise = noise_rand if kind == 'ddim' else None
                    hist0 = (hist_rand if kind == 'second' else torch.full_like(x, float('nan'))) if multistep else None
                    clone = lambda t: None if t is None else t.clone()
                    nl, kp = (mn, keep) if guided else (None, None)
                    what = (shape, objective, clip, guided, kind)
                    # the host-struct entry point, out of place
                    h_a = clone(hist0)
                    img_a, xs_a = ops.sampler_step_thr(step, mc, nl, x, noise, h_a, thr, want_x_start=True, keep=kp)
                    assert h_a is None or same(h_a, xs_a), what
                    # ... in place
                    h_b, img_b = clone(hist0), x.clone()
                    ops.sampler_step_thr(step, mc, nl, img_b, noise, h_b, thr, out=img_b, keep=kp)
                    assert same(img_b, img_a) and (h_b is None or same(h_b, xs_a)), what
                    # the device-struct entry point (MODE_LAST belongs to the last entry of a table)
                    if kind == 'last':
                        steps, k = [_step(objective, clip, ops.MODE_MULTISTEP, 0.), step], 1
                    else:
                        steps, k = [step, _step(objective, clip, ops.MODE_LAST, 0.)], 0
                    table, tt, cursor, cur = ops.step_table(steps, [5, 0], dev())
                    ops.sampler_seek(cursor, k, table, tt, cur, tcond)
                    h_c, xs_c = clone(hist0), torch.empty_like(x)
                    img_c = ops.sampler_step_thr_dev(cur, mc, nl, x, noise, h_c, thr, x_start=xs_c, keep=kp)
                    assert same(img_c, img_a) and same(xs_c, xs_a) and (h_c is None or same(h_c, xs_a)), what
                    h_d, img_d = clone(hist0), x.clone()
                    ops.sampler_step_thr_dev(cur, mc, nl, img_d, noise, h_d, thr, out=img_d, keep=kp)
                    assert same(img_d, img_a) and (h_d is None or same(h_d, xs_a)), what
                    # NaN: the one in model_cond stays where it is, the history's does not leak where c2 == 0
                    assert torch.equal(torch.isnan(img_a), nan_at) and torch.equal(torch.isnan(xs_a), nan_at), what
                    want_img, want_xs = TC.statement(step, mc, nl, kp, x, noise, hist0, thr)
                    for name, got, want in (('img', img_a, want_img), ('x_start', xs_a, want_xs)):
                        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=2e-5, equal_nan=True,
                                                   msg=lambda m: f'{what} {name}: {m}')
                        worst = max(worst, float((got.double() - want)[~nan_at].abs().max()))
                    # the raw x_start of dmh_sampler_threshold[_dev]: what the existing step returns without a clamp
                    raw_step = _step(objective, 0, ops.MODE_LAST, 0.)
                    _, raw_want, _ = ops.sampler_step(raw_step, mc, nl, x, None, want_x_start=True, keep=kp)
                    n = C * H * W
                    kq, fq = TC.rank_of(0.9, n)
                    gbuf = torch.full((B * n + 16,), 777., device=dev())
                    scratch = gbuf[8:8 + B * n].view(shape)
                    t_a, raw_a = ops.sampler_threshold(step, mc, nl, x, kq, fq, keep=kp, x0_raw=scratch)
                    assert raw_a is scratch and same(raw_a, raw_want), what
                    assert bool((gbuf[:8] == 777.).all()) and bool((gbuf[8 + B * n:] == 777.).all()), what
                    t_b, raw_b = ops.sampler_threshold_dev(cur, mc, nl, x, kq, fq, keep=kp)
                    assert same(raw_b, raw_want) and same(t_b, t_a), what
                    assert same(t_a, ops.row_quantile_abs(raw_want, kq, fq, 1.)), what
                    assert math.isnan(float(t_a[0])) and float(t_a[1]) >= 1., what     # (row 0 holds the NaN)
                    above += int(float(t_a[1]) > 1.)
                    # thr == 1: the existing kernels with the static clamp; clip == 0: thr is not read
                    if multistep:
                        h_e = clone(hist0)
                        img_e, xs_e = ops.sampler_step_ms(step, mc, nl, x, h_e, want_x_start=True, keep=kp)
                    else:
                        img_e, xs_e, _ = ops.sampler_step(step, mc, nl, x, noise, want_x_start=True, keep=kp)
                    for t in ((ones,) if clip else (ones, thr, thr_nan)):
                        h_f = clone(hist0)
                        img_f, xs_f = ops.sampler_step_thr(step, mc, nl, x, noise, h_f, t, want_x_start=True, keep=kp)
                        assert same(img_f, img_e) and same(xs_f, xs_e) and (h_f is None or same(h_f, xs_e)), (what, t)
                    # a NaN threshold poisons exactly its row
                    if clip:
                        h_g = clone(hist0)
                        img_g, xs_g = ops.sampler_step_thr(step, mc, nl, x, noise, h_g, thr_nan, want_x_start=True, keep=kp)
                        assert torch.equal(torch.isnan(xs_g), nan_at | row1) and torch.equal(torch.isnan(img_g), nan_at | row1), what
                        assert same(xs_g[0], xs_e[0]) and same(img_g[0], img_e[0]), what      # (row 0 at thr 1: the static clamp)
                    checked += 1
    assert checked == 3 * 2 * 2 * 4 and above > 0
    print(f'[parity] thresholded step kernels {shape}: max|hip - float64| = {worst:.3e} (gate rtol 1e-4 / atol 2e-5)')


# --------------------------------------------------------------------------------------------- 4. the sampler, restated
T_, S_, B_, CS_, P_ = 100, 8, 2, 3., 0.995


def _scaled(sd, scale):
    return {k: v * scale if k.startswith('final_conv') else v for k, v in sd.items()}


def _restate(sd, objective, drop, sampler, noise, uniforms, conds):
    """the sampling loop in the oracle's terms: its network and raw x_start per step (fp32, CPU); the row quantile, the
    threshold and the update in float64 here -> (image in [0, 1], per-step x_start, per-step raw quantiles (B,))"""
    c, rf01, fl, mk = conds
    buf = OD.schedule_buffers(T_, 'cosine')
    abar = buf['alphas_cumprod'].double()
    if sampler == 'dpmpp_2m':
        entries = _coefficients(buf, T_, S_)
    else:                                                    # DDIM at eta = 0 (CFG:697-707): c0 = sqrt(abar'), c1 = sqrt(1 - abar')
        entries = [(t, math.sqrt(float(abar[tn])), math.sqrt(1. - float(abar[tn])), 0.) if tn >= 0 else (t, None)
                   for t, tn in OD.ddim_time_pairs(T_, S_)]
    rgbn = rf01 * 2 - 1
    img, prev, xs, qs = noise, None, [], []
    with torch.no_grad():
        for k, entry in enumerate(entries):
            t = torch.full((B_,), entry[0], dtype=torch.long)
            keep = (uniforms[k] < 1 - drop) if uniforms else torch.zeros(B_, dtype=torch.bool)
            out = OU.cfg_unet_forward_with_cond_scale(sd, img, t, c, rgbn, mk, keep, CS_)
            _, raw = OD._predictions(buf, objective, out, img, t, False)
            q, thr = TC.threshold_ref(raw, P_)
            x0 = TC.apply_threshold(raw, thr)
            qs.append(q)
            xs.append(x0)
            if entry[1] is None:
                img = x0.float()
            elif sampler == 'dpmpp_2m':
                _, c0, c1, c2 = entry
                o = c1 * img.double() + c0 * x0
                img = (o + c2 * prev if c2 != 0. else o).float()
            else:
                _, c0, c1, _ = entry
                rc = float(buf['sqrt_recip_alphas_cumprod'][entry[0]])
                rm1 = float(buf['sqrt_recipm1_alphas_cumprod'][entry[0]])
                pn = (rc * img.double() - x0) / rm1          # CFG:590-594, from the thresholded x_start
                img = (c0 * x0 + c1 * pn).float()
            prev = x0
    return (img + 1) * 0.5, xs, qs


@pytest.mark.parametrize('weights', ['plain', 'x0.15'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
@pytest.mark.parametrize('objective,drop', [('pred_x0', 0.5), ('pred_v', 1.0)])
def test_sampler_vs_restatement(objective, drop, sampler, weights):
    """the sampler gate of DESIGN 4 is 4e-4; measured on MI355X over the eight runs: per-step x_start <= 5.5e-6, thr <= 1.6e-6
    of its value, image <= 2.7e-6 — more than 10x inside, so the gates here are 10x the measured figures (6e-5, 2e-5, 3e-5)"""
    from dmhomo_amd import ops
    m, sd = _cfg_model(drop)
    if weights != 'plain':
        sd = _scaled(sd, 0.15)
        m.load_state_dict(sd)
    d = _cfg_diffusion(m, T=T_, S=S_, objective=objective)
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile, d.ddim_sampling_eta = sampler, 'dynamic', P_, 0.
    conds = _cond_inputs(B_, 16)
    c, rf01, fl, mk = conds
    gen = torch.Generator().manual_seed(21)
    shape = (B_, 6, 16, 16)
    noise = torch.randn(shape, generator=gen)
    uniforms = [torch.rand(B_, generator=gen) for _ in range(S_)] if 0 < drop < 1 else []
    step_noise = [torch.randn(shape, generator=gen) for _ in range(S_ - 1)] if sampler == 'ddim' else []
    ref, ref_xs, ref_q = _restate(sd, objective, drop, sampler, noise, uniforms, conds)
    q = torch.stack(ref_q)
    print(f'[parity] dynamic {sampler} {objective} {weights}: the restatement\'s raw quantiles range '
          f'{float(q.min()):.3f} .. {float(q.max()):.3f}')
    if weights == 'plain':                                   # every (step, row) thresholds
        assert float(q.min()) > 1., q
    else:                                                    # both branches of max(1, q) in one run
        assert float(q.max()) > 1.05 and float(q.min()) < 0.95, q
    draws = [noise]
    for k in range(S_):                                      # the loop's call order: class dropout in the network, then noise
        draws += ([uniforms[k]] if uniforms else []) + ([step_noise[k]] if k < len(step_noise) else [])
    d.rng = ReplayDeviceRng(draws)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(g(c), ops.affine(g(rf01), 2., -1.), g(fl), g(mk), shape, CS_, trace=trace)
    assert d.rng.i == len(draws) and len(trace) == S_
    drift = [float((a['x_start'].cpu().double() - b).abs().max()) for a, b in zip(trace, ref_xs)]
    tdrift = [float(((a['thr'].cpu().double() - b.clamp(min=1.)).abs() / b.clamp(min=1.)).max()) for a, b in zip(trace, ref_q)]
    print(f'[parity] dynamic {sampler} {objective} {weights}: per-step max|x_start - restatement| = '
          + ' '.join(f'{e:.1e}' for e in drift))
    print(f'[parity] dynamic {sampler} {objective} {weights}: per-step max|thr - restatement| / thr = '
          + ' '.join(f'{e:.1e}' for e in tdrift))
    err, _ = report(f'dynamic {sampler} {objective} {weights} img', got.cpu(), ref)
    assert max(drift) <= 6e-5 and max(tdrift) <= 2e-5 and err <= 3e-5, (max(drift), max(tdrift), err)
    # sample() is the same call
    d.rng = ReplayDeviceRng(draws)
    assert torch.equal(d.sample(g(c), g(rf01), g(fl), g(mk), cond_scale=CS_)[0], got)


# --------------------------------------------------------------------------------------------- 5. dynamic == static below 1
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_dynamic_equals_static_where_nothing_exceeds_one(sampler):
    """final_conv x 0.15, pred_x0, the 0.9 quantile: every threshold is 1 (asserted on the trace), so the sample is the
    static clamp's bit for bit, eager and captured"""
    from dmhomo_amd import cfg, ops
    S, B = 6, 2
    m, sd = _cfg_model()
    m.load_state_dict(_scaled(sd, 0.15))
    d = _cfg_diffusion(m, size=16, T=100, S=S)
    d.sampler, d.dynamic_threshold_percentile = sampler, 0.9
    ins = [g(t) for t in _cond_inputs(B, 16)]
    d.rng = cfg.DeviceRng()

    def run(mode, graph):
        d.clip_mode, d.hip_graph = mode, graph
        torch.manual_seed(3)
        return d.sample(*ins)[0].clone()
    static = run('static', False)
    assert torch.equal(run('dynamic', False), static)
    assert torch.equal(run('dynamic', True), static)
    assert torch.equal(run('static', True), static)
    d.clip_mode, d.hip_graph = 'dynamic', False
    torch.manual_seed(3)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    c, rf01, fl, mk = ins
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, tuple(static.shape), 3., trace=trace)
    assert torch.equal(got, static) and len(trace) == S
    assert all(bool((e['thr'] == 1.).all()) for e in trace), [e['thr'].tolist() for e in trace]


# --------------------------------------------------------------------------------------------- 6. captured == eager
@pytest.mark.parametrize('S,size', [(6, 32), (1, 16)])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
@pytest.mark.parametrize('mode', ['batched', 'streams'])
def test_captured_equals_eager(mode, sampler, S, size):
    """bitwise, output and generator (left where the eager loop leaves it): the capturing call, new inputs on the same graph,
    clip_mode switched to 'static' and back (one capture each)"""
    from dmhomo_amd import cfg
    B = 2
    m, sd = _cfg_model()
    m.cfg_mode = mode
    d = _cfg_diffusion(m, size=size, T=100, S=S)
    d.sampler = sampler
    ins = {3: [g(t) for t in _cond_inputs(B, size, 9)], 4: [g(t) for t in _cond_inputs(B, size, 10)]}
    d.rng = cfg.DeviceRng()

    def run(graph, seed):
        d.hip_graph = graph
        torch.manual_seed(seed)
        out = d.sample(*ins[seed])[0].clone()
        return out, torch.rand(4, device=dev())

    def check(got, want, what):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (mode, sampler, S, what)
    d.clip_mode = 'dynamic'
    e3, e4 = run(False, 3), run(False, 4)
    assert not torch.equal(e3[0], e4[0])
    check(run(True, 3), e3, 'the capturing call')
    check(run(True, 4), e4, 'new inputs on the same graph')
    assert d.graph_captures == 1
    d.clip_mode = 'static'
    es = run(False, 3)
    assert not torch.equal(es[0], e3[0])                     # (the plain test weights saturate: thresholds above 1)
    check(run(True, 3), es, 'static, capturing')
    assert d.graph_captures == 2
    d.clip_mode = 'dynamic'
    check(run(True, 3), e3, 'back on dynamic')
    d.clip_mode = 'static'
    check(run(True, 4), run(False, 4), 'back on static')
    assert d.graph_captures == 2                             # each mode captured once
    d.clip_mode, d.dynamic_threshold_percentile = 'dynamic', 0.9
    e3p = run(False, 3)
    assert not torch.equal(e3p[0], e3[0])
    check(run(True, 3), e3p, 'another percentile')
    assert d.graph_captures == 3                             # (the rank is baked into the captured launches)
    d.hip_graph, m.cfg_mode = False, 'batched'


# --------------------------------------------------------------------------------------------- 7. row handling
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_dedup_and_row_independence_with_the_keyed_generator(sampler):
    """dedup_dropped_rows on == off, and a B = 3 call == the three B = 1 calls with the same global sample ids (bitwise): a
    row's threshold comes from that row alone; the draw counts are the static clamp's"""
    from dmhomo_amd import cfg
    S, B = 6, 3
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=100, S=S)
    d.sampler, d.clip_mode = sampler, 'dynamic'
    c, rf01, fl, mk = (g(t) for t in _cond_inputs(B, 16))
    d.rng = cfg.DeviceRng()
    draws = 1 + S + (S - 1 if sampler == 'ddim' else 0)      # the initial noise, S class-dropout draws, DDIM's step noise

    def run(lo, hi):
        d.rng.key_by_sample(5, range(40 + lo, 40 + hi), dev())
        out = d.sample(c[lo:hi].contiguous(), rf01[lo:hi].contiguous(), fl[lo:hi].contiguous(), mk[lo:hi].contiguous())[0]
        assert d.rng.state.tolist()[1] == draws
        return out.clone()
    whole = run(0, B)
    assert not torch.equal(whole[0], whole[1])
    for b in range(B):
        assert torch.equal(run(b, b + 1)[0], whole[b]), b
    m.dedup_dropped_rows = True
    assert torch.equal(run(0, B), whole)
    d.hip_graph = True
    assert torch.equal(run(0, B), whole)                      # ... and captured, with the dropped rows skipped
    m.cfg_mode = 'streams'
    assert torch.equal(run(0, B), whole)
    m.stream_splits = 2
    assert torch.equal(run(0, B), whole)
    d.hip_graph, m.dedup_dropped_rows, m.cfg_mode, m.stream_splits = False, False, 'batched', 1
