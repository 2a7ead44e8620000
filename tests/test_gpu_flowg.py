"""GPU: guidance on the flow condition (``flow_guidance``) and the training switch ``flow_drop_prob``.  1. the two kernels alone,
bitwise against the fp32 statement of tests/flowg_cases.py, inside NaN guards, at every size / batch / pointer phase; 2. the
network method row by row against separate passes; 3. the sampling loops: against a loop composed from existing pieces (bitwise),
against a float64 loop (gated), captured against eager (bitwise), flow_guidance = 1 and a sample without flow information; 4. the
training step with dropped flow conditions against the existing path on an edited batch (bitwise)."""
import pytest
import torch

import flowg_cases as FC
import guidance_cases as GC
import threshold_cases as TC
from detweights import det_state_dict, shapes_of
from gpu_util import dev
from test_gpu_guidance import _recording, g, same
from test_gpu_solver import _cond_inputs

pytestmark = pytest.mark.gpu

NAN = float('nan')


# --------------------------------------------------------------------------------------------- 1. the kernels alone
def _guarded(x, off, fill=NAN):
    """x (B, n) inside a buffer of ``fill``, ``off`` floats past a 16-byte boundary -> (the view, the buffer, a copy of it)"""
    B, n = x.shape
    buf = torch.full((B * n + 16,), fill, device=dev(), dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[4 + off:4 + off + B * n].view(B, n)
    view.copy_(x)
    return view, buf, buf.clone()


def _guards_untouched(buf, before, off, numel):
    lo, hi = 4 + off, 4 + off + numel
    return same(buf[:lo], before[:lo]) and same(buf[hi:], before[hi:])


def _shift(case, phase=(0, 0, 0)):
    """one guarded launch -> (cond', null' or None) on the CPU; guards and uncond untouched"""
    from dmhomo_amd import ops
    numel = case['uncond'].numel()
    cond, cbuf, cwas = _guarded(case['cond'], phase[0])
    uncond, ubuf, uwas = _guarded(case['uncond'], phase[2])
    null = nbuf = nwas = None
    if case['null'] is not None:
        null, nbuf, nwas = _guarded(case['null'], phase[1])
    got = ops.flow_guidance_shift(cond, null, uncond, case['w'], keep=g(case['keep']))
    assert got[0] is cond and got[1] is null
    assert _guards_untouched(cbuf, cwas, phase[0], numel) and same(ubuf, uwas)
    if null is not None:
        assert _guards_untouched(nbuf, nwas, phase[1], numel)
    return cond.cpu(), None if null is None else null.cpu()


@pytest.fixture(scope='module')
def table():
    """the case table with the fp32 statement of every case, computed once"""
    out = {}
    for name, case in FC.cases():
        out[name] = (case, FC.shift32(case['cond'], case['null'], case['uncond'], case['w'], case['keep']))
    return out


@pytest.mark.parametrize('n', FC.SIZES)
def test_shift_is_bitwise_the_fp32_statement(table, n):
    """every batch, pointer phase, case A with keep None / mixed / all zero and case B; the rows of cond with keep == 0 are NaN
    going in: they come back with their bits and leak into nothing"""
    seen = 0
    for name, (case, (want_c, want_n)) in table.items():
        if case['uncond'].shape[1] != n:
            continue
        for phase in FC.PHASES:
            got_c, got_n = _shift(case, phase)
            assert same(got_c, want_c), (name, phase)
            if want_n is not None:
                assert same(got_n, want_n) and bool(torch.isfinite(got_n).all()), (name, phase)
            seen += 1
        if case['keep'] is not None:
            dropped = ~case['keep'].bool()
            assert same(got_c[dropped], case['cond'][dropped]) and bool(torch.isnan(got_c[dropped]).all())
        first = _shift(case)
        again = _shift(case)                                  # two launches on equal inputs: equal bits
        assert same(first[0], again[0]) and (first[1] is None or same(first[1], again[1])), name
    assert seen == len(FC.BATCHES) * 4 * len(FC.PHASES)


def test_shift_with_w_0_leaves_every_value(table):
    for name, (case, _) in table.items():
        if case['keep'] is not None and not bool(case['keep'].all()):
            continue                                          # (NaN rows: covered bitwise above)
        got_c, got_n = _shift(dict(case, w=0.), (1, 1, 1))
        assert torch.equal(got_c, case['cond']), name
        assert got_n is None or torch.equal(got_n, case['null']), name


def test_shift_at_the_workload_size():
    B, n = FC.BIG
    cond, null, uncond = FC.inputs(B, n, 5)
    keep = (torch.arange(B) % 3 != 1).to(torch.uint8)
    cond[~keep.bool()] = NAN
    case = dict(cond=cond, null=null, uncond=uncond, keep=keep, w=1.5)
    got_c, got_n = _shift(case)
    want_c, want_n = FC.shift32(cond, null, uncond, 1.5, keep)
    assert same(got_c, want_c) and same(got_n, want_n) and bool(torch.isfinite(got_n).all())


@pytest.mark.parametrize('n', FC.SIZES)
def test_affine_rows_keep_is_affine_on_kept_rows_and_zero_on_dropped(n):
    from dmhomo_amd import ops
    for B in FC.BATCHES:
        x = FC.inputs(B, n, 40 + B)[0]
        full = ops.affine(g(x), 2., -1.).cpu()                # dmh_affine on the whole tensor
        assert same(full, FC.affine_keep32(x, 2., -1., torch.ones(B, dtype=torch.uint8)))
        for kind, keep in FC.keeps_for(B).items():
            keep = torch.ones(B, dtype=torch.uint8) if keep is None else keep
            xin = x.clone()
            xin[~keep.bool()] = NAN                           # a dropped row's x is not read: nothing of it shows
            for phase in FC.PHASES:
                xs, xbuf, xwas = _guarded(xin, phase[0])
                ys, ybuf, ywas = _guarded(torch.full((B, n), NAN), phase[1])
                got = ops.affine_rows_keep(xs, 2., -1., g(keep), out=ys)
                assert got is ys and same(xbuf, xwas) and _guards_untouched(ybuf, ywas, phase[1], B * n)
                y = ys.cpu()
                kept = keep.bool()
                assert same(y[kept], full[kept]), (B, kind, phase)
                assert bool((y[~kept].view(torch.int32) == 0).all()), (B, kind, phase)       # +0.0: the sign bit clear
        keep = FC.keeps_for(B)['mixed']
        fresh = ops.affine_rows_keep(g(x), 2., -1., g(keep))  # without out=
        assert same(fresh.cpu(), FC.affine_keep32(x, 2., -1., keep))


def test_entries_and_wrappers_refuse_bad_arguments():
    from dmhomo_amd import _lib, ops
    assert FC.check_einval(_lib) == FC.N_EINVAL
    x = torch.zeros((2, 8), device=dev())
    keep = torch.ones(2, dtype=torch.uint8, device=dev())
    for args, kw in (((x, None, x[:1], 1.), {}), ((x, x[:1], x.clone(), 1.), {}), ((x, None, x.clone(), 1.), {'keep': keep}),
                     ((x, x.clone(), x.clone(), 1.), {'keep': keep[:1]}), ((x, x.clone(), x.clone(), 1.), {'keep': keep.bool()}),
                     ((x, None, x.clone(), NAN), {}), ((x, None, x.clone(), float('inf')), {})):
        with pytest.raises(ValueError, match='flow_guidance_shift'):
            ops.flow_guidance_shift(*args, **kw)
    with pytest.raises(_lib.DmhError, match='uncond overlaps'):
        ops.flow_guidance_shift(x, None, x, 1.)
    with pytest.raises(_lib.DmhError, match='model_cond overlaps model_null'):
        ops.flow_guidance_shift(x, x, x.clone(), 1.)
    with pytest.raises(_lib.DmhError):
        ops.flow_guidance_shift(x, None, x.clone().double(), 1.)
    for args, kw in (((x, 2., -1., None), {}), ((x, 2., -1., keep[:1]), {}), ((x, 2., -1., keep.float()), {}),
                     ((x, 2., -1., keep), {'out': x[:1]})):
        with pytest.raises(ValueError, match='affine_rows_keep'):
            ops.affine_rows_keep(*args, **kw)
    buf = torch.zeros(24, device=dev())
    with pytest.raises(_lib.DmhError, match='y overlaps x'):
        ops.affine_rows_keep(buf[:16].view(2, 8), 2., -1., keep, out=buf[4:20].view(2, 8))


# --------------------------------------------------------------------------------------------- the tiny model
T_, S_, B_, SIZE, P_ = 20, 4, 3, 16, 0.995


def _tiny(drop=0.5, seed=0):
    from dmhomo_amd import cfg
    m = cfg.Unet(dim=8, dim_mults=(1, 2), channels=6, num_classes=1, cond_drop_prob=drop)
    m.load_state_dict(det_state_dict(shapes_of(m), seed, 0.2))            # (de-saturated: little of x_start sits on the clamp)
    return m.to(dev())


def _diffusion(m, objective='pred_x0'):
    from dmhomo_amd import cfg
    return cfg.GaussianDiffusion(m, image_size=SIZE, timesteps=T_, sampling_timesteps=S_, objective=objective).to(dev())


def _net_inputs(seed=3):
    from dmhomo_amd import ops
    gen = torch.Generator().manual_seed(seed)
    x = g(torch.randn(B_, 6, SIZE, SIZE, generator=gen))
    t = torch.full((B_,), 7, dtype=torch.long, device=dev())
    c, rf01, _, mk = (g(v) for v in _cond_inputs(B_, SIZE))
    return x, t, c, ops.affine(rf01, 2., -1.), mk


# --------------------------------------------------------------------------------------------- 2. the network
@pytest.mark.parametrize('dedup', [False, True], ids=['all-rows', 'dedup'])
@pytest.mark.parametrize('cond_scale', [3., 1.])
def test_every_row_is_the_row_of_a_separate_pass(cond_scale, dedup, monkeypatch):
    m = _tiny()
    m.dedup_dropped_rows = dedup
    x, t, c, rf, mk = _net_inputs()
    keep = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev())
    monkeypatch.setattr(m, '_keep_mask', lambda batch, p, device: keep)   # the same keep bits in every call below
    cond, null, uncond, computed = m._cond_null_noflow(x, t, c, rf, mk, cond_scale)
    zero = torch.zeros_like(rf)
    if cond_scale == 1:
        assert null is None and computed is None
        assert same(cond, m.forward(x, t, c, rf, mk))
        assert same(uncond, m.forward(x, t, c, zero, mk))     # the same keep bits, on zero flow
        return
    assert (computed is keep) if dedup else (computed is None)
    want_c, want_n, want_computed = m._cond_null(x, t, c, rf, mk)
    rows = keep.bool() if dedup else torch.ones(B_, dtype=torch.bool, device=dev())
    assert same(cond[rows], want_c[rows]) and same(null, want_n)
    assert same(uncond, m._run(x, t, c, zero, mk, [m._null_mask(B_, x.device)]))
    assert not same(uncond, null) and not same(cond[rows], null[rows])


# --------------------------------------------------------------------------------------------- 3. the loops
def _keyed(d, seed=5, first_id=40, rows=B_):
    d.rng.key_by_sample(seed, range(first_id, first_id + rows), dev())


def _sample_inputs():
    return tuple(g(v) for v in _cond_inputs(B_, SIZE))


def _composed_loop(d, ins, cond_scale, w):
    """the loop written from existing pieces: the passes one by one, the fp32 shift with torch on the CPU, the existing step"""
    from dmhomo_amd import ops
    m = d.model
    c, rf01, fl, mk = ins
    rf = ops.affine(rf01, 2., -1.)
    zero = torch.zeros_like(rf)
    shape = (B_, 6, SIZE, SIZE)
    solver = d.sampler == 'dpmpp_2m'
    rank = d._dynamic_rank(shape, True)
    img = d.rng.randn(shape, dev()).contiguous()
    hist = torch.empty_like(img)
    for time, step, draws in d._sampler_steps(True, cond_scale):
        t = torch.full((B_,), time, device=dev(), dtype=torch.long)
        keep = m._keep_mask(B_, m.cond_drop_prob, dev())       # the one draw of the step
        if cond_scale == 1:
            cond, null = m._run(img, t, c, rf, mk, [keep]), None
            uncond = m._run(img, t, c, zero, mk, [keep])
        else:
            cond = m._run(img, t, c, rf, mk, [keep])
            null = m._run(img, t, c, rf, mk, [m._null_mask(B_, dev())])
            uncond = m._run(img, t, c, zero, mk, [m._null_mask(B_, dev())])
        sc, sn = FC.shift32(cond.cpu(), None if null is None else null.cpu(), uncond.cpu(), w)
        cond, null = g(sc), g(sn)
        noise = d.rng.randn(shape, dev()).contiguous() if (draws and not solver) else None
        if rank is not None:
            thr, _ = ops.sampler_threshold(step, cond, null, img, *rank)
            img, _ = ops.sampler_step_thr(step, cond, null, img, noise, hist if solver else None, thr)
        elif solver:
            img, _ = ops.sampler_step_ms(step, cond, null, img, hist)
        else:
            img, _, _ = ops.sampler_step(step, cond, null, img, noise, want_x_start=False)
    return ops.affine(img, 0.5, 0.5)


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('cond_scale', [3., 1.])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_eager_loop_is_the_composition_of_existing_pieces(sampler, cond_scale, clip_mode):
    from dmhomo_amd import cfg
    d = _diffusion(_tiny())
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile = sampler, clip_mode, P_
    d.rng = cfg.DeviceRng()
    ins = _sample_inputs()
    d.flow_guidance = 2.5
    _keyed(d)
    got = d.sample(*ins, cond_scale=cond_scale)[0]
    _keyed(d)
    want = _composed_loop(d, ins, cond_scale, 1.5)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    d.flow_guidance = None
    _keyed(d)
    assert not torch.equal(d.sample(*ins, cond_scale=cond_scale)[0], got)


# gates of the loop parity: 10x the worst relative deviation measured on MI355X against the float64 loop; the
# measurements are in the docstring of test_loops_vs_float64_loop
GATE_X0, GATE_IMG = 2.6e-6, 2.5e-6


def _float64_loop(d, nets, draws, w, dynamic, cs):
    """the loop in float64 on the recorded network outputs and noise: shift, blend, threshold, step -> per step (x_start, img)"""
    cpu = lambda v: None if v is None else v.cpu()
    img, hist, ni, out = draws[0].cpu().double(), None, 1, []
    ones = torch.ones(img.shape[0])
    for (time, step, _), (cond, null, uncond, keep) in zip(d._sampler_steps(True, cs), nets):
        cond, null, _ = FC.shift64(cpu(cond), cpu(null), cpu(uncond), w, cpu(keep))
        noise = None
        if step.mode == 0:
            noise, ni = draws[ni].cpu(), ni + 1
        thr = None
        if dynamic:
            raw = GC.statement(step, cond, null, cpu(keep), img, noise, hist, None, ones)[2]
            thr = TC.threshold_ref(raw, P_)[1]
        img, x0, _ = GC.statement(step, cond, null, cpu(keep), img, noise, hist, thr, ones)
        hist = x0
        out.append((x0, img))
    assert ni == len(draws)
    return out


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('cond_scale', [3., 1.])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_vs_float64_loop(sampler, cond_scale, clip_mode, monkeypatch):
    """measured on MI355X over the eight runs, relative to the largest value of the float64 tensor: per-step x_start <= 2.51e-7,
    image <= 2.47e-7 (gates 10x that: GATE_X0 / GATE_IMG)"""
    from dmhomo_amd import ops
    m = _tiny()
    m.dedup_dropped_rows = True                              # (the dropped rows of cond are then unwritten: keep must reach the shift)
    d = _diffusion(m, 'pred_x0' if sampler == 'ddim' else 'pred_v')
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile = sampler, clip_mode, P_
    _, draws = _recording(d, monkeypatch)
    nets, noflow = [], m._cond_null_noflow

    def recorded(*a):
        out = noflow(*a)
        nets.append(tuple(None if v is None else v.clone() for v in out))
        return out
    monkeypatch.setattr(m, '_cond_null_noflow', recorded)
    c, rf01, fl, mk = _sample_inputs()
    d.flow_guidance = 2.
    torch.manual_seed(11)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, (B_, 6, SIZE, SIZE), cond_scale, trace=trace)
    assert len(trace) == len(nets) == S_ and all(e['flow'] is True for e in trace)
    ref = _float64_loop(d, nets, draws, 1., clip_mode == 'dynamic', cond_scale)
    rel = lambda a, b: float((a.cpu().double() - b).abs().max() / b.abs().max())
    ex = max(rel(e['x_start'], r[0]) for e, r in zip(trace, ref))
    ei = max(rel(e['img'], r[1]) for e, r in zip(trace, ref))
    print(f'[parity] flow_guidance 2 {sampler} cond_scale {cond_scale} {clip_mode}: max rel |x_start - float64| = {ex:.3e}, '
          f'max rel |img - float64| = {ei:.3e}')
    assert ex <= GATE_X0 and ei <= GATE_IMG, (ex, ei)
    assert torch.equal(got, ops.affine(trace[-1]['img'], 0.5, 0.5))


def _runner(d, ins):
    def run(**kw):
        _keyed(d)
        return d.sample(*ins, **kw)[0].clone()
    return run


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_captured_equals_eager(sampler, clip_mode):
    """bitwise, cond_scale 1 and 3, dedup_dropped_rows off and on; a second replay of the same capture gives the same samples"""
    from dmhomo_amd import cfg
    m = _tiny()
    d = _diffusion(m)
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile = sampler, clip_mode, P_
    d.rng = cfg.DeviceRng()
    d.flow_guidance = 2.
    run = _runner(d, _sample_inputs())
    for cond_scale in (3., 1.):
        want = None
        for dedup in (False, True):
            m.dedup_dropped_rows, d.hip_graph = dedup, False
            eager = run(cond_scale=cond_scale)
            want = eager if want is None else want
            assert torch.equal(eager, want), (cond_scale, dedup, 'eager: dedup changes nothing')
            d.hip_graph = True
            assert torch.equal(run(cond_scale=cond_scale), want), (cond_scale, dedup, 'captured')
            assert torch.equal(run(cond_scale=cond_scale), want), (cond_scale, dedup, 'replayed')
    assert d.graph_captures == 4


@pytest.mark.parametrize('setting', ['guidance_rescale', 'apg', 'photo_guidance'])
def test_captured_equals_eager_beside_the_other_switches(setting):
    from dmhomo_amd import cfg
    m = _tiny()
    m.dedup_dropped_rows = True
    d = _diffusion(m)
    d.rng = cfg.DeviceRng()
    if setting == 'guidance_rescale':
        d.guidance_rescale = 0.7
    elif setting == 'apg':
        d.apg_eta, d.apg_momentum = 0., -0.5
    else:
        d.photo_guidance = 0.5
    run = _runner(d, _sample_inputs())
    off = run()
    d.flow_guidance = 2.
    want = run()
    assert not torch.equal(want, off) and bool(torch.isfinite(want).all())
    d.hip_graph = True
    assert torch.equal(run(), want) and torch.equal(run(), want) and d.graph_captures == 1


def test_capture_cache_counts():
    """a second value of flow_guidance captures once more, None is the default's entry"""
    from dmhomo_amd import cfg
    d = _diffusion(_tiny())
    d.rng = cfg.DeviceRng()
    d.hip_graph = True
    run = _runner(d, _sample_inputs())
    default = run()
    assert d.graph_captures == 1
    d.flow_guidance = 2.
    a = run()
    assert d.graph_captures == 2 and not torch.equal(a, default)
    assert torch.equal(run(), a) and d.graph_captures == 2
    d.flow_guidance = 3.
    b = run()
    assert d.graph_captures == 3 and not torch.equal(b, a)
    d.flow_guidance = None
    assert torch.equal(run(), default) and d.graph_captures == 3
    d.flow_guidance = 2.
    assert torch.equal(run(), a) and d.graph_captures == 3
    d.hip_graph = False
    assert torch.equal(run(), a)


@pytest.mark.parametrize('cond_scale', [3., 1.])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_flow_guidance_1_gives_the_samples_of_none(sampler, cond_scale):
    """from the same generator state, with torch's own generator (every draw moves it): no draw was added"""
    d = _diffusion(_tiny())
    d.sampler = sampler
    ins = _sample_inputs()
    torch.manual_seed(21)
    off = d.sample(*ins, cond_scale=cond_scale)[0]
    after_off = torch.cuda.get_rng_state(dev())
    d.flow_guidance = 1.
    torch.manual_seed(21)
    on = d.sample(*ins, cond_scale=cond_scale)[0]
    assert torch.equal(on, off) and torch.equal(torch.cuda.get_rng_state(dev()), after_off)
    d.flow_guidance = 2.
    torch.manual_seed(21)
    assert not torch.equal(d.sample(*ins, cond_scale=cond_scale)[0], off)


@pytest.mark.parametrize('cond_scale', [3., 1.])
def test_a_sample_without_flow_information_is_left_as_it_is(cond_scale):
    """rgb_flow = 0.5 everywhere is +0.0 after 2x - 1: the no-flow pass's own input, n == u (c == u) bitwise, e == 0"""
    from dmhomo_amd import cfg
    d = _diffusion(_tiny())
    d.rng = cfg.DeviceRng()
    c, rf01, fl, mk = _sample_inputs()
    rf01 = rf01.clone()
    rf01[1] = 0.5
    run = _runner(d, (c, rf01, fl, mk))
    off = run(cond_scale=cond_scale)
    d.flow_guidance = 2.
    on = run(cond_scale=cond_scale)
    assert torch.equal(on[1], off[1])
    assert not torch.equal(on[0], off[0]) and not torch.equal(on[2], off[2])


# --------------------------------------------------------------------------------------------- 4. training
@pytest.fixture()
def train_setup():
    """the fixture model of the training tests (test_gpu_backward._train_setup) on a batch of four: (m, d, ts, img, classes,
    draws)"""
    from test_gpu_unet import make_cfg
    from dmhomo_amd import cfg, train
    m, _ = make_cfg(8)
    d = cfg.GaussianDiffusion(m, image_size=16, timesteps=1000, sampling_timesteps=4, objective='pred_x0', loss_type='l1').to(dev())
    ts = train.TrainStep(d, lr=1e-3, betas=(0.9, 0.99))
    gen = torch.Generator().manual_seed(17)
    img = torch.rand(4, 12, 16, 16, generator=gen)
    img[:, 6] = (img[:, 6] > 0.4).float()                     # the mask
    # the flow, in pixels: one whole pixel along one axis per sample.  The backward of flow_warp adds with float atomics
    # (train_misc.hip: the one place where the summation order is not fixed); with these flows a target receives at most two
    # non-zero contributions (two at the clamped border), whose sum does not depend on their order: the existing path is
    # then bitwise repeatable, which a bitwise comparison against it needs (asserted below)
    img[:, -2:] = torch.tensor([[1., 0.], [0., -1.], [-1., 0.], [0., 1.]]).reshape(4, 2, 1, 1).expand(4, 2, 16, 16)
    draws = dict(t=g(torch.tensor([5, 300, 700, 999])), noise=g(torch.randn(4, 6, 16, 16, generator=gen)),
                 keep=g(torch.tensor([1, 1, 0, 1], dtype=torch.uint8)))
    return m, d, ts, g(img), torch.zeros(4, dtype=torch.long, device=dev()), draws


def test_dropped_flow_conditions_are_the_existing_path_on_an_edited_batch(train_setup):
    """loss and every parameter gradient, bitwise: flow_keep = [1, 0, 1, 0] against the batch whose dropped samples carry
    rgb_flow = 0.5 (2 * 0.5 - 1 is +0.0)"""
    m, d, ts, img, classes, draws = train_setup
    flow_keep = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=dev())
    loss, grads = ts.loss_and_grads(img, classes, **draws, flow_keep=flow_keep)
    edited = img.clone()
    edited[1::2, -5:-2] = 0.5
    want_loss, want = ts.loss_and_grads(edited, classes, **draws)
    again_loss, again = ts.loss_and_grads(edited, classes, **draws)
    assert same(again_loss, want_loss) and all(same(again[k], want[k]) for k in want), 'the reference is not repeatable'
    plain_loss, _ = ts.loss_and_grads(img, classes, **draws)
    assert same(loss, want_loss) and not same(loss, plain_loss)
    assert set(grads) == set(want) == {k for k, _ in m.named_parameters()}
    for k in want:
        assert same(grads[k], want[k]), k


def test_the_draw_sits_between_the_noise_and_the_class_dropout(train_setup, monkeypatch):
    from dmhomo_amd import cfg
    m, d, ts, img, classes, _ = train_setup
    B = img.shape[0]
    d.rng = cfg.DeviceRng()
    seen = []
    forward = ts.ut.forward

    def spy(x, t, cls, rgb_flow, mask, keep, *a, **k):
        seen.append((x.clone(), t.clone(), rgb_flow.clone(), keep.clone()))
        return forward(x, t, cls, rgb_flow, mask, keep, *a, **k)
    monkeypatch.setattr(ts.ut, 'forward', spy)

    def run(p):
        d.flow_drop_prob = p
        torch.manual_seed(3)
        d.rng.key_by_sample(9, range(B), dev())
        return ts.loss_and_grads(img, classes)[0]
    loss0, loss5 = run(0.), run(0.5)
    (x0, t0, rf0, keep0), (x5, t5, rf5, keep5) = seen
    assert torch.equal(t0, t5) and same(x0, x5)               # t and the noise (x = q_sample(x_start, t, noise)) as at 0.
    # the reference's order with one more uniform in between
    d.rng.key_by_sample(9, range(B), dev())
    d.rng.randn(x0.shape, dev())
    u = d.rng.uniform(B, dev())
    keep_want = m._keep_mask(B, m.cond_drop_prob, dev())
    flow_keep = u < 0.5
    assert torch.equal(keep5, keep_want) and 0 < int(flow_keep.sum()) < B
    assert bool((rf5[~flow_keep].view(torch.int32) == 0).all()) and same(rf5[flow_keep], rf0[flow_keep])
    assert not same(loss0, loss5)
    # p_losses under no_grad: the same draws, the same loss value (the project's bound between the two forward paths: 2e-5
    # of the loss, test_train_step_gradients_vs_reference)
    torch.manual_seed(3)
    d.rng.key_by_sample(9, range(B), dev())
    with torch.no_grad():
        val = d(img, classes=classes)
    assert abs(float(val) - float(loss5)) <= 2e-5 * abs(float(loss5)), (float(val), float(loss5))
    assert abs(float(val) - float(loss0)) > 2e-5 * abs(float(loss0))
