"""-m gpu: guidance rescale of the conditional sampler (``guidance_rescale``): the factor kernels (dmh_guidance_factor[_dev]),
the step and threshold kernels on the rescaled blend (dmh_sampler_step_gr[_dev], dmh_sampler_threshold_gr[_dev]) and
cfg.GaussianDiffusion with the switch on, eager and captured.

1. the factor alone against the float64 reference of tests/guidance_cases.py, over its sizes, batches and kinds;
2. the step and threshold kernels alone: against a float64 statement, against the existing kernels where every factor is 1;
3. the eager loops against a float64 loop fed the same network outputs: per-step factor, x_start and image;
4. captured == eager, dedup on == off, 'batched' == 'streams', cond_scale 1, the capture cache."""
import math

import pytest
import torch

import guidance_cases as GC
import threshold_cases as TC
from gpu_util import dev
from test_gpu_solver import _cfg_diffusion, _cfg_model, _cond_inputs

pytestmark = pytest.mark.gpu


def g(x):
    return None if x is None else x.to(dev())


def bits(x):
    return x.contiguous().view(torch.int32)


def same(a, b):
    """bitwise, NaN included"""
    return torch.equal(bits(a), bits(b))


def _step(objective=1, clip=1, mode=1, c2=0., cs=GC.CS):
    from dmhomo_amd import _lib
    return _lib.DmhStep(objective=objective, clip=clip, mode=mode, cond_scale=cs, sqrt_recip_ac=1.3, sqrt_recipm1_ac=0.8,
                        sqrt_ac=0.7, sqrt_1m_ac=0.6, c0=0.9, c1=0.3, c2=c2)


# --------------------------------------------------------------------------------------------- 1. the factor alone
@pytest.fixture(scope='module')
def factor_cases():
    from dmhomo_amd import ops
    ragged = tuple(GC.ragged_size(ops.guidance_splits, B)[0] for B in GC.BATCHES)
    return GC.factor_cases(ragged), ragged


def _guarded(x, off, fill=float('nan')):
    """x (B, n) inside a buffer of ``fill``, ``off`` floats past a 16-byte boundary -> (the view, the buffer)"""
    B, n = x.shape
    buf = torch.full((B * n + 16,), fill, device=dev(), dtype=x.dtype)
    view = buf[4 + off:4 + off + B * n].view(B, n)
    view.copy_(x)
    return view, buf


def _factor(case, off_c=0, off_n=0, dev_struct=False):
    """one guarded launch pair -> g (B,) on the CPU; the floats around gfac and around the workspace stay untouched"""
    from dmhomo_amd import ops
    B, n = case['cond'].shape
    cond, _ = _guarded(case['cond'], off_c)
    null, _ = _guarded(case['null'], off_n)
    need = 4 * B * ops.guidance_splits(B, n)
    wbuf = torch.full((need + 8,), 777., device=dev(), dtype=torch.float64)
    obuf = torch.full((B + 16,), 777., device=dev())
    out, step = obuf[8:8 + B], _step(cs=case['cs'])
    if dev_struct:
        table, tt, cursor, cur = ops.step_table([step], [0], dev())
        ops.sampler_seek(cursor, 0, table, tt, cur, torch.zeros((B,), dtype=torch.int64, device=dev()))
        got = ops.guidance_factor_dev(cur, cond, null, case['phi'], keep=g(case['keep']), ws=wbuf[4:4 + need], gfac=out)
    else:
        got = ops.guidance_factor(step, cond, null, case['phi'], keep=g(case['keep']), ws=wbuf[4:4 + need], gfac=out)
    assert got is out
    assert bool((obuf[:8] == 777.).all()) and bool((obuf[8 + B:] == 777.).all())
    assert bool((wbuf[:4] == 777.).all()) and bool((wbuf[4 + need:] == 777.).all())
    return out.cpu()


def _check_factor(name, case):
    """-> the worst |g - reference| / |reference| of a case gated against the reference (0 for the exact kinds)"""
    B, n = case['cond'].shape
    first = _factor(case)
    assert same(_factor(case), first), (name, 'two launches')                        # (i)
    assert same(_factor(case, dev_struct=True), first), (name, 'device struct')
    worst = 0.
    for off_c, off_n in ((0, 0), (1, 1), (3, 2)):           # rows on and off 16 B, cond and null in and out of phase
        got = first if (off_c, off_n) == (0, 0) else _factor(case, off_c, off_n)
        expect = case['expect']
        if isinstance(expect, float):                        # (b), (c), (d): that value, exactly
            assert got.tolist() == [expect] * B, (name, off_c, off_n, got)
        elif isinstance(expect, tuple):                      # (g): the broken row NaN, the others as without it
            clean = _factor(case['clean'], off_c, off_n)
            for b in range(B):
                if b == expect[1]:
                    assert math.isnan(float(got[b])), (name, b, got)
                else:
                    assert same(got[b:b + 1], clean[b:b + 1]) and math.isfinite(float(got[b])), (name, b, got, clean)
        else:
            ref = GC.factor_ref(case['cond'], case['null'], case['keep'], case['cs'], case['phi'])
            err = ((got.double() - ref).abs() / ref.abs()).max().item()
            assert err <= GC.GATE, (name, off_c, off_n, err, got, ref)
            worst = max(worst, err)
            if case['phi'] == 1.:                            # (h): cfg * g has the population std of cond
                mo, cfg = GC.blend32(case['cond'], case['null'], case['keep'], case['cs'])
                sc = mo.double().std(dim=1, unbiased=False)
                sg = (cfg.double() * got.double().reshape(B, 1)).std(dim=1, unbiased=False)
                ok = (sg - sc).abs() <= GC.GATE * sc
                assert bool((ok | (cfg.double().std(dim=1, unbiased=False) == 0.)).all()), (name, sg, sc)
    return worst


@pytest.mark.parametrize('kind', GC.KINDS)
def test_factor_small_sizes(factor_cases, kind):
    cases, ragged = factor_cases
    mine = [(name, c) for name, c in cases if c['kind'] == kind and c['cond'].shape[1] != GC.BIG[0]]
    assert len(mine) == (len(GC.SIZES) + len(ragged)) * len(GC.BATCHES)
    worst = max(_check_factor(name, c) for name, c in mine)
    print(f'[parity] guidance_factor {kind}, {len(mine)} cases (n = 1 .. {max(ragged)}): worst |g - float64| / g = {worst:.3e} '
          f'(gate {GC.GATE:.3e})')


def test_factor_ragged_sizes_are_split(factor_cases):
    from dmhomo_amd import ops
    _, ragged = factor_cases
    for B, n in zip(GC.BATCHES, ragged):
        s = ops.guidance_splits(B, n)
        assert s >= 2 and n % (4 * s) != 0, (B, n, s)


@pytest.mark.parametrize('which', ['normal+keep', 'offset'])
def test_factor_workload_row(factor_cases, which):
    cases, _ = factor_cases
    mine = [(name, c) for name, c in cases if c['cond'].shape[1] == GC.BIG[0] and name.startswith(which)]
    assert len(mine) == (1 if which == 'normal+keep' else len(GC.BATCHES))
    worst = max(_check_factor(name, c) for name, c in mine)
    print(f'[parity] guidance_factor {which} at n = {GC.BIG[0]}: worst |g - float64| / g = {worst:.3e} (gate {GC.GATE:.3e})')


def test_ops_refuse_wrong_shapes():
    from dmhomo_amd import _lib, ops
    x = torch.zeros((2, 3, 4, 4), device=dev())
    step, gf = _step(), torch.ones((2,), device=dev())
    with pytest.raises(ValueError):
        ops.guidance_factor(step, x, None, 0.7)
    with pytest.raises(ValueError):
        ops.guidance_factor(step, x, x[:1].clone(), 0.7)
    with pytest.raises(ValueError):
        ops.guidance_factor(step, x, x, 0.7, gfac=torch.ones((3,), device=dev()))
    with pytest.raises(ValueError):
        ops.guidance_factor(step, x, x, 0.7, ws=torch.zeros((7,), device=dev(), dtype=torch.float64))
    with pytest.raises(_lib.DmhError, match='phi'):
        ops.guidance_factor(step, x, x, 1.5)
    cur = torch.zeros((44,), dtype=torch.uint8, device=dev())
    for fn, s in ((ops.sampler_step_gr, step), (ops.sampler_step_gr_dev, cur)):
        with pytest.raises(ValueError):
            fn(s, x, x, x, None, None, None, gf[:1])
        with pytest.raises(ValueError):
            fn(s, x, x, x, None, None, torch.ones((3,), device=dev()), gf)
        with pytest.raises(ValueError):
            fn(s, x, x, x, None, x[:1].clone(), None, gf)
        with pytest.raises(_lib.DmhError, match='exclude'):
            fn(s, x, x, x, x.clone(), x.clone(), None, gf)
    with pytest.raises(ValueError):
        ops.sampler_threshold_gr(step, x, x, x, gf[:1], 0, 0.)
    with pytest.raises(_lib.DmhError, match='rank'):
        ops.sampler_threshold_gr(step, x, x, x, gf, 48, 0.)


# --------------------------------------------------------------------------------------------- 2. the step kernels alone
@pytest.mark.parametrize('shape', [(3, 3, 3, 5), (3, 3, 4, 5)], ids=['1-pixel', '4-pixel'])
def test_step_kernels_alone(shape):
    """against the float64 statement (measured on MI355X: 8.7e-7 / 8.8e-7 on values up to 20; gate rtol 1e-5 / atol 5e-6); the
    host-struct, device-struct and in-place forms bitwise; a factor of 1 bitwise the existing kernels"""
    from dmhomo_amd import ops
    B = shape[0]
    n = shape[1] * shape[2] * shape[3]
    gen = torch.Generator().manual_seed(4)
    mc, mn, x, hist_rand, noise_rand = (g(torch.randn(shape, generator=gen) * s) for s in (1.5, 1.5, 1., 1., 1.))
    keep = g(torch.tensor([1, 0, 1], dtype=torch.uint8))
    thr = g(torch.tensor([1., 2.5, 1.25]))
    gf = g(torch.tensor([0.625, 1., 0.8125]))
    ones = torch.ones_like(gf)
    tcond = torch.zeros((B,), dtype=torch.int64, device=dev())
    kq, fq = TC.rank_of(0.9, n)
    clone = lambda t: None if t is None else t.clone()
    worst, checked = 0., 0
    for objective in (0, 1, 2):
        for clip in (0, 1):
            for kind in ('ddim', 'last', 'first', 'second'):
                for dynamic in (False, True):
                    mode = {'ddim': ops.MODE_DDIM, 'last': ops.MODE_LAST}.get(kind, ops.MODE_MULTISTEP)
                    step = _step(objective, clip, mode, -0.4 if kind in ('ddim', 'second') else 0.)
                    multistep = kind in ('first', 'second')
                    noise = noise_rand if kind == 'ddim' else None
                    hist0 = (hist_rand if kind == 'second' else torch.full_like(x, float('nan'))) if multistep else None
                    t = thr if dynamic else None
                    what = (shape, objective, clip, kind, dynamic)
                    h_a = clone(hist0)
                    img_a, xs_a = ops.sampler_step_gr(step, mc, mn, x, noise, h_a, t, gf, want_x_start=True, keep=keep)
                    assert h_a is None or same(h_a, xs_a), what
                    h_b, img_b = clone(hist0), x.clone()     # in place
                    ops.sampler_step_gr(step, mc, mn, img_b, noise, h_b, t, gf, out=img_b, keep=keep)
                    assert same(img_b, img_a) and (h_b is None or same(h_b, xs_a)), what
                    if kind == 'last':                       # the device struct (MODE_LAST belongs to a table's last entry)
                        steps, k = [_step(objective, clip, ops.MODE_MULTISTEP, 0.), step], 1
                    else:
                        steps, k = [step, _step(objective, clip, ops.MODE_LAST, 0.)], 0
                    table, tt, cursor, cur = ops.step_table(steps, [5, 0], dev())
                    ops.sampler_seek(cursor, k, table, tt, cur, tcond)
                    h_c, xs_c = clone(hist0), torch.empty_like(x)
                    img_c = ops.sampler_step_gr_dev(cur, mc, mn, x, noise, h_c, t, gf, x_start=xs_c, keep=keep)
                    assert same(img_c, img_a) and same(xs_c, xs_a) and (h_c is None or same(h_c, xs_a)), what
                    assert bool(torch.isfinite(img_a).all()), what          # (the NaN history is not read where c2 == 0)
                    cpu = lambda v: None if v is None else v.cpu()
                    want_img, want_xs, want_raw = GC.statement(step, mc.cpu(), mn.cpu(), keep.cpu(), x.cpu(), cpu(noise), cpu(hist0),
                                                               None if t is None else t.cpu().double(), gf.cpu())
                    for name, got, want in (('img', img_a, want_img), ('x_start', xs_a, want_xs)):
                        torch.testing.assert_close(got.cpu().double(), want.cpu(), rtol=1e-5, atol=5e-6,
                                                   msg=lambda m: f'{what} {name}: {m}')
                        worst = max(worst, float((got.cpu().double() - want.cpu()).abs().max()))
                    # the threshold entry: its scratch is the step's x_start without a clamp; its threshold the selector's
                    raw_step = _step(objective, 0, ops.MODE_LAST, 0.)
                    _, raw_want = ops.sampler_step_gr(raw_step, mc, mn, x, None, None, None, gf, want_x_start=True, keep=keep)
                    torch.testing.assert_close(raw_want.cpu().double(), want_raw.cpu(), rtol=1e-5, atol=5e-6)
                    t_a, raw_a = ops.sampler_threshold_gr(step, mc, mn, x, gf, kq, fq, keep=keep)
                    t_b, raw_b = ops.sampler_threshold_gr_dev(cur, mc, mn, x, gf, kq, fq, keep=keep)
                    assert same(raw_a, raw_want) and same(raw_b, raw_want) and same(t_a, t_b), what
                    assert same(t_a, ops.row_quantile_abs(raw_want, kq, fq, 1.)), what
                    # a factor of 1: the existing kernels, bit for bit
                    h_e, h_f = clone(hist0), clone(hist0)
                    img_f, xs_f = ops.sampler_step_gr(step, mc, mn, x, noise, h_f, t, ones, want_x_start=True, keep=keep)
                    if dynamic:
                        img_e, xs_e = ops.sampler_step_thr(step, mc, mn, x, noise, h_e, thr, want_x_start=True, keep=keep)
                    elif multistep:
                        img_e, xs_e = ops.sampler_step_ms(step, mc, mn, x, h_e, want_x_start=True, keep=keep)
                    else:
                        img_e, xs_e, _ = ops.sampler_step(step, mc, mn, x, noise, want_x_start=True, keep=keep)
                    assert same(img_f, img_e) and same(xs_f, xs_e) and (h_f is None or same(h_f, h_e)), what
                    t_e, raw_e = ops.sampler_threshold(step, mc, mn, x, kq, fq, keep=keep)
                    t_f, raw_f = ops.sampler_threshold_gr(step, mc, mn, x, ones, kq, fq, keep=keep)
                    assert same(t_f, t_e) and same(raw_f, raw_e), what
                    checked += 1
    assert checked == 3 * 2 * 4 * 2
    print(f'[parity] rescaled step kernels {shape}: max|hip - float64| = {worst:.3e} (gate rtol 1e-5 / atol 5e-6)')


@pytest.mark.parametrize('how', ['cond-equals-null', 'keep-all-zero'])
def test_factor_one_rows_take_the_existing_steps_bits(how):
    """(b): the factor kernel itself answers exactly 1.0 for rows whose conditional logits are their null logits, and the
    step on it is dmh_sampler_step's, dmh_sampler_step_ms's and dmh_sampler_step_thr's, torch.equal"""
    from dmhomo_amd import ops
    shape = (3, 6, 5, 7)
    gen = torch.Generator().manual_seed(6)
    mn, x, noise, hist0 = (g(torch.randn(shape, generator=gen) * 1.5) for _ in range(4))
    if how == 'cond-equals-null':
        mc, keep = mn.clone(), None
    else:
        mc, keep = torch.full_like(mn, float('nan')), torch.zeros((3,), dtype=torch.uint8, device=dev())
    thr = g(torch.tensor([1., 2.5, 1.25]))
    for objective in (0, 1, 2):
        ddim, ms = _step(objective, 1, 0, -0.4), _step(objective, 1, 3, -0.4)
        gf = ops.guidance_factor(ddim, mc, mn, 0.7, keep=keep)
        assert gf.tolist() == [1., 1., 1.]
        img_a, xs_a = ops.sampler_step_gr(ddim, mc, mn, x, noise, None, None, gf, want_x_start=True, keep=keep)
        img_b, xs_b, _ = ops.sampler_step(ddim, mc, mn, x, noise, want_x_start=True, keep=keep)
        assert torch.equal(img_a, img_b) and torch.equal(xs_a, xs_b)
        h_a, h_b = hist0.clone(), hist0.clone()
        img_a, xs_a = ops.sampler_step_gr(ms, mc, mn, x, None, h_a, None, gf, want_x_start=True, keep=keep)
        img_b, xs_b = ops.sampler_step_ms(ms, mc, mn, x, h_b, want_x_start=True, keep=keep)
        assert torch.equal(img_a, img_b) and torch.equal(xs_a, xs_b) and torch.equal(h_a, h_b)
        for step, nz, h in ((ddim, noise, None), (ms, None, hist0)):
            h_a, h_b = (None, None) if h is None else (h.clone(), h.clone())
            img_a, xs_a = ops.sampler_step_gr(step, mc, mn, x, nz, h_a, thr, gf, want_x_start=True, keep=keep)
            img_b, xs_b = ops.sampler_step_thr(step, mc, mn, x, nz, h_b, thr, want_x_start=True, keep=keep)
            assert torch.equal(img_a, img_b) and torch.equal(xs_a, xs_b)


# --------------------------------------------------------------------------------------------- 3. the loops, restated
T_, S_, B_, P_ = 100, 4, 3, 0.995
# gates of the loop parity: <= 10x the error measured on MI355X against the float64 loop
GATE_X0, GATE_IMG = 3e-6, 3.9e-6


def _recording(d, monkeypatch):
    """d with its network calls and noise draws recorded -> (network outputs per step, draws of randn)"""
    from dmhomo_amd import cfg
    nets = []

    class Rng(cfg.DeviceRng):
        def __init__(self):
            super().__init__()
            self.rec = []

        def randn(self, shape, device):
            out = super().randn(shape, device)
            self.rec.append(out.clone())
            return out
    network = d._network

    def recorded(*a):
        out = network(*a)
        nets.append(tuple(None if t is None else t.clone() for t in out))
        return out
    monkeypatch.setattr(d, '_network', recorded)
    d.rng = Rng()
    return nets, d.rng.rec


def _reference_loop(d, nets, draws, phi, dynamic, cs):
    """the loop in float64 on the recorded network outputs and noise: factor (the blend in fp32, moments in float64),
    threshold, step -> per step (g, x_start, img)"""
    cpu = lambda t: None if t is None else t.cpu()
    img, hist, ni, out = draws[0].cpu().double(), None, 1, []
    for (time, step, _), (cond, null, keep) in zip(d._sampler_steps(True, cs), nets):
        cond, null, keep = cpu(cond), cpu(null), cpu(keep)
        gf = GC.factor_ref(cond, null, keep, cs, phi)
        noise = None
        if step.mode == 0:
            noise, ni = draws[ni].cpu(), ni + 1
        thr = None
        if dynamic:
            raw = GC.statement(step, cond, null, keep, img, noise, hist, None, gf)[2]
            thr = TC.threshold_ref(raw, P_)[1]
        img, x0, _ = GC.statement(step, cond, null, keep, img, noise, hist, thr, gf)
        hist = x0
        out.append((gf, x0, img))
    assert ni == len(draws)
    return out


@pytest.mark.parametrize('phi', [0.7, 1.0])
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_vs_float64_loop(sampler, clip_mode, phi, monkeypatch):
    """measured on MI355X over the eight runs and the 40 x 40 one: factor <= 3.7e-8 of its value (gate: one fp32 ulp,
    guidance_cases.GATE), per-step x_start <= 3.0e-7, image <= 3.9e-7 (gates 10x that: GATE_X0 / GATE_IMG)"""
    from dmhomo_amd import ops
    m, _ = _cfg_model(0.5)
    d = _cfg_diffusion(m, size=16, T=T_, S=S_, objective='pred_x0' if sampler == 'ddim' else 'pred_v')
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile, d.guidance_rescale = sampler, clip_mode, P_, phi
    nets, draws = _recording(d, monkeypatch)
    c, rf01, fl, mk = (g(t) for t in _cond_inputs(B_, 16))
    torch.manual_seed(11)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, (B_, 6, 16, 16), GC.CS, trace=trace)
    assert len(trace) == len(nets) == S_ and len(draws) == 1 + (S_ - 1 if sampler == 'ddim' else 0)
    ref = _reference_loop(d, nets, draws, phi, clip_mode == 'dynamic', GC.CS)
    eg = max(float(((e['gfac'].cpu().double() - r[0]).abs() / r[0]).max()) for e, r in zip(trace, ref))
    ex = max(float((e['x_start'].cpu().double() - r[1]).abs().max()) for e, r in zip(trace, ref))
    ei = max(float((e['img'].cpu().double() - r[2]).abs().max()) for e, r in zip(trace, ref))
    gs = torch.stack([e['gfac'] for e in trace])
    print(f'[parity] guidance_rescale {phi} {sampler} {clip_mode}: g in {float(gs.min()):.3f} .. {float(gs.max()):.3f}; '
          f'max|g - float64| / g = {eg:.2e}, max|x_start - float64| = {ex:.2e}, max|img - float64| = {ei:.2e}')
    assert float(gs.min()) < 0.95 and float(gs.max()) <= 1.  # (cond_scale 3: kept rows are scaled down; dropped rows: exactly 1)
    assert ('thr' in trace[0]) == (clip_mode == 'dynamic')
    assert eg <= GC.GATE and ex <= GATE_X0 and ei <= GATE_IMG, (eg, ex, ei)
    assert torch.equal(got, ops.affine(trace[-1]['img'], 0.5, 0.5))
    # sample() is the same call, and phi = 0 another sample
    torch.manual_seed(11)
    assert torch.equal(d.sample(c, rf01, fl, mk, cond_scale=GC.CS)[0], got)
    d.guidance_rescale = 0.
    torch.manual_seed(11)
    assert not torch.equal(d.sample(c, rf01, fl, mk, cond_scale=GC.CS)[0], got)


def test_loop_vs_float64_loop_at_40(monkeypatch):
    """one 40 x 40 run (rows of 9600 values: three splits per row), dynamic clipping, the multistep solver"""
    from dmhomo_amd import ops
    m, _ = _cfg_model(0.5)
    d = _cfg_diffusion(m, size=40, T=T_, S=S_, objective='pred_x0')
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile, d.guidance_rescale = 'dpmpp_2m', 'dynamic', P_, 0.7
    nets, draws = _recording(d, monkeypatch)
    c, rf01, fl, mk = (g(t) for t in _cond_inputs(B_, 40))
    torch.manual_seed(12)
    trace = []
    d._dpmpp_sample(c, ops.affine(rf01, 2., -1.), fl, mk, (B_, 6, 40, 40), GC.CS, trace=trace)
    assert ops.guidance_splits(B_, 9600) == 3
    ref = _reference_loop(d, nets, draws, 0.7, True, GC.CS)
    eg = max(float(((e['gfac'].cpu().double() - r[0]).abs() / r[0]).max()) for e, r in zip(trace, ref))
    ex = max(float((e['x_start'].cpu().double() - r[1]).abs().max()) for e, r in zip(trace, ref))
    ei = max(float((e['img'].cpu().double() - r[2]).abs().max()) for e, r in zip(trace, ref))
    print(f'[parity] guidance_rescale 0.7 dpmpp_2m dynamic 40x40: max|g - float64| / g = {eg:.2e}, max|x_start - float64| = '
          f'{ex:.2e}, max|img - float64| = {ei:.2e}')
    assert eg <= GC.GATE and ex <= GATE_X0 and ei <= GATE_IMG, (eg, ex, ei)


# --------------------------------------------------------------------------------------------- 4. captured, dedup, streams
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_captured_equals_eager_and_the_cache_keeps_one_capture_per_phi(sampler, clip_mode):
    """bitwise, output and generator (left where the eager loop leaves it): the capturing call, new inputs on the same graph,
    phi changed and changed back (one capture per value, then replays from the cache)"""
    from dmhomo_amd import cfg
    B, size = 3, 16
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=size, T=100, S=S_)
    d.sampler, d.clip_mode = sampler, clip_mode
    ins = {3: [g(t) for t in _cond_inputs(B, size, 9)], 4: [g(t) for t in _cond_inputs(B, size, 10)]}
    d.rng = cfg.DeviceRng()

    def run(graph, seed, phi):
        d.hip_graph, d.guidance_rescale = graph, phi
        torch.manual_seed(seed)
        out = d.sample(*ins[seed])[0].clone()
        return out, torch.rand(4, device=dev())

    def check(got, want, what):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (sampler, clip_mode, what)
    e3, e4, e3_1, e3_0 = run(False, 3, 0.7), run(False, 4, 0.7), run(False, 3, 1.), run(False, 3, 0.)
    assert not torch.equal(e3[0], e3_0[0]) and not torch.equal(e3[0], e3_1[0]) and not torch.equal(e3[0], e4[0])
    check(run(True, 3, 0.7), e3, 'the capturing call')
    check(run(True, 4, 0.7), e4, 'new inputs on the same graph')
    assert d.graph_captures == 1
    check(run(True, 3, 1.), e3_1, 'phi = 1, capturing')
    check(run(True, 3, 0.), e3_0, 'phi = 0, capturing')
    assert d.graph_captures == 3
    check(run(True, 3, 0.7), e3, 'back on 0.7')
    check(run(True, 3, 1.), e3_1, 'back on 1')
    check(run(True, 4, 0.), run(False, 4, 0.), 'back on 0')
    assert d.graph_captures == 3                             # one capture per value, replayed from the cache afterwards
    d.hip_graph = False


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_dedup_streams_and_row_independence(sampler):
    """dedup_dropped_rows on == off, 'batched' == 'streams', captured == eager, and a B = 3 call == the three B = 1 calls with
    the same global sample ids, all bitwise: a dropped row's factor is exactly 1 whether its logits were computed or not,
    and a row's factor comes from that row alone"""
    from dmhomo_amd import cfg
    S, B = S_, 3
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=100, S=S)
    d.sampler, d.clip_mode, d.guidance_rescale = sampler, 'dynamic', 0.7
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
    m.cfg_mode = 'streams'
    assert torch.equal(run(0, B), whole)
    m.cfg_mode, m.dedup_dropped_rows = 'batched', True
    assert torch.equal(run(0, B), whole)
    d.hip_graph = True
    assert torch.equal(run(0, B), whole)                      # ... and captured, with the dropped rows skipped
    m.cfg_mode = 'streams'
    assert torch.equal(run(0, B), whole)
    m.dedup_dropped_rows = False
    assert torch.equal(run(0, B), whole)
    d.guidance_rescale = 0.
    assert not torch.equal(run(0, B), whole)
    d.hip_graph, m.dedup_dropped_rows, m.cfg_mode = False, False, 'batched'


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_cond_scale_1_ignores_phi(sampler):
    """no null pass, nothing to rescale: phi = 0.7 is phi = 0 bit for bit, eager and captured"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=100, S=S_)
    d.sampler = sampler
    ins = [g(t) for t in _cond_inputs(2, 16)]
    d.rng = cfg.DeviceRng()

    def run(graph, phi, clip_mode):
        d.hip_graph, d.guidance_rescale, d.clip_mode = graph, phi, clip_mode
        torch.manual_seed(3)
        return d.sample(*ins, cond_scale=1.)[0].clone()
    for clip_mode in ('static', 'dynamic'):
        want = run(False, 0., clip_mode)
        assert torch.equal(run(False, 0.7, clip_mode), want)
        assert torch.equal(run(True, 0.7, clip_mode), want)
    d.hip_graph = False
