"""GPU: perturbed-attention guidance (``pag_scale``).  1. the two kernels alone: the identity arm of dmh_attention_pag at the tile
edges of K4 (bitwise v on perturbed rows, bitwise dmh_attention on the others, NaN where no row is listed), dmh_pag_shift bitwise
against the fp32 statement of tests/pag_cases.py inside NaN guards at every size / batch / pointer phase; 2. the network method
row by row against separate passes, and its perturbed rows against the float64 oracle with the identity map; 3. the sampling
loops: against a loop composed from existing pieces (bitwise), against a float64 loop (gated), captured against eager (bitwise),
pag_scale = 0 and None."""
import pytest
import torch
import torch.nn.functional as F

import guidance_cases as GC
import pag_cases as PC
import threshold_cases as TC
from detweights import det_state_dict, shapes_of
from gpu_util import dev
from test_gpu_guidance import _recording, g, same
from test_gpu_solver import _cond_inputs

pytestmark = pytest.mark.gpu

NAN = float('nan')
ATTN_SCALE = 32 ** -0.5


# --------------------------------------------------------------------------------------------- 1. the kernels alone
def _attention_pag(qkv, rows, pert_lo):
    """one launch of dmh_attention_pag into an out tensor full of NaN -> out"""
    from dmhomo_amd import ops
    B, n = qkv.shape[0], qkv.shape[1]
    out = torch.full((B, n, 1, 128), NAN, device=dev(), dtype=torch.float32)
    ops.call('dmh_attention_pag', ops.ptr(qkv), ops.ptr(out), B, n, ATTN_SCALE, ops.ptr(rows, torch.int32), pert_lo)
    return out


@pytest.mark.parametrize('n', PC.ATTN_NS)
def test_attention_identity_arm(n):
    """B = 3, pert_lo = 0 .. 3, every row or a list without physical row 1: perturbed rows are v bitwise, the other listed rows
    bitwise dmh_attention's, unlisted rows keep their NaN; through the wrapper too"""
    from dmhomo_amd import ops
    B = PC.ATTN_B
    gen = torch.Generator().manual_seed(500 + n)
    qkv = g(torch.randn(B, n, 1, 384, generator=gen))
    before = qkv.clone()
    want_v = PC.attention_identity(qkv).contiguous()
    for listed in PC.ATTN_ROWS:
        rows = None
        if listed is not None:
            keep = torch.zeros(B, dtype=torch.uint8)
            keep[list(listed)] = 1
            rows = ops.rows_from_keep(g(keep))
        plain = ops.attention_core(qkv, ATTN_SCALE, rows=rows)
        for pert_lo in range(B + 1):
            out = _attention_pag(qkv, rows, pert_lo)
            for b in range(B):
                if listed is not None and b not in listed:
                    assert bool(torch.isnan(out[b]).all()), (listed, pert_lo, b)
                elif b >= pert_lo:
                    assert same(out[b], want_v[b]), (listed, pert_lo, b)
                else:
                    assert same(out[b], plain[b]) and bool(torch.isfinite(out[b]).all()), (listed, pert_lo, b)
            via = ops.attention_core(qkv, ATTN_SCALE, rows=rows, pert_lo=pert_lo)
            live = list(range(B)) if listed is None else list(listed)
            assert same(via[live], out[live]), (listed, pert_lo)
    assert same(qkv, before)
    assert not same(plain[0], want_v[0]) or n == 1           # (one key: softmax is 1, the map IS the identity up to rounding)


def test_attention_pag_refuses_a_pert_lo_outside_the_batch():
    from dmhomo_amd import _lib, ops
    qkv = torch.zeros((3, 4, 1, 384), device=dev())
    out = torch.zeros((3, 4, 1, 128), device=dev())
    for lo in (-1, 4):
        with pytest.raises(ValueError, match='pert_lo'):
            ops.attention_core(qkv, ATTN_SCALE, pert_lo=lo)
        with pytest.raises(_lib.DmhError, match='pert_lo'):
            ops.call('dmh_attention_pag', ops.ptr(qkv), ops.ptr(out), 3, 4, ATTN_SCALE, None, lo)


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
    """one guarded launch -> (cond', null' or None) on the CPU; guards and pert untouched"""
    from dmhomo_amd import ops
    numel = case['pert'].numel()
    cond, cbuf, cwas = _guarded(case['cond'], phase[0])
    pert, pbuf, pwas = _guarded(case['pert'], phase[2])
    null = nbuf = nwas = None
    if case['null'] is not None:
        null, nbuf, nwas = _guarded(case['null'], phase[1])
    got = ops.pag_shift(cond, null, pert, case['s'], keep=g(case['keep']))
    assert got[0] is cond and got[1] is null
    assert _guards_untouched(cbuf, cwas, phase[0], numel) and same(pbuf, pwas)
    if null is not None:
        assert _guards_untouched(nbuf, nwas, phase[1], numel)
    return cond.cpu(), None if null is None else null.cpu()


@pytest.fixture(scope='module')
def table():
    """the case table, built once"""
    return dict(PC.cases())


@pytest.mark.parametrize('n', PC.SIZES)
def test_shift_is_bitwise_the_fp32_statement(table, n):
    """every batch, pointer phase, case A with keep None / mixed / all zero and case B, s = 0, 0.5 and 3; the rows of cond with
    keep == 0 are NaN going in: they come back with their bits and leak into nothing"""
    seen = 0
    for name, case in table.items():
        if case['pert'].shape[1] != n:
            continue
        for s in PC.SCALES:
            cs = dict(case, s=s)
            want_c, want_n = PC.shift32(case['cond'], case['null'], case['pert'], s, case['keep'])
            for phase in PC.PHASES:
                got_c, got_n = _shift(cs, phase)
                assert same(got_c, want_c), (name, s, phase)
                if want_n is not None:
                    assert same(got_n, want_n) and bool(torch.isfinite(got_n).all()), (name, s, phase)
                seen += 1
            if case['keep'] is not None:
                dropped = ~case['keep'].bool()
                assert same(got_c[dropped], case['cond'][dropped]) and bool(torch.isnan(got_c[dropped]).all())
    assert seen == len(PC.BATCHES) * 4 * len(PC.PHASES) * len(PC.SCALES)


def test_shift_with_s_0_or_equal_passes_leaves_every_value(table):
    for name, case in table.items():
        if case['keep'] is not None and not bool(case['keep'].all()):
            continue                                          # (NaN rows: covered bitwise above)
        got_c, got_n = _shift(dict(case, s=0.), (1, 1, 1))
        assert torch.equal(got_c, case['cond']), name        # (==: e is a zero of either sign)
        assert got_n is None or torch.equal(got_n, case['null']), name
        got_c, got_n = _shift(dict(case, pert=case['cond'].clone(), s=3.), (1, 1, 1))
        assert same(got_c, case['cond']), name               # cond == pert: e is +0.0, every value bitwise
        assert got_n is None or same(got_n, case['null']), name


def test_shift_at_the_workload_size():
    B, n = PC.BIG
    cond, null, pert = PC.FC.inputs(B, n, 5)
    keep = (torch.arange(B) % 3 != 1).to(torch.uint8)
    cond[~keep.bool()] = NAN
    case = dict(cond=cond, null=null, pert=pert, keep=keep, s=3.)
    got_c, got_n = _shift(case)
    want_c, want_n = PC.shift32(cond, null, pert, 3., keep)
    assert same(got_c, want_c) and same(got_n, want_n) and bool(torch.isfinite(got_n).all())


def test_entries_and_wrapper_refuse_bad_arguments():
    from dmhomo_amd import _lib, ops
    assert PC.check_einval(_lib) == PC.N_EINVAL
    x = torch.zeros((2, 8), device=dev())
    keep = torch.ones(2, dtype=torch.uint8, device=dev())
    for args, kw in (((x, None, x[:1], 1.), {}), ((x, x[:1], x.clone(), 1.), {}), ((x, None, x.clone(), 1.), {'keep': keep}),
                     ((x, x.clone(), x.clone(), 1.), {'keep': keep[:1]}), ((x, x.clone(), x.clone(), 1.), {'keep': keep.bool()}),
                     ((x, None, x.clone(), NAN), {}), ((x, None, x.clone(), float('inf')), {}), ((x, None, x.clone(), -0.5), {})):
        with pytest.raises(ValueError, match='pag_shift'):
            ops.pag_shift(*args, **kw)
    with pytest.raises(_lib.DmhError, match='pert overlaps'):
        ops.pag_shift(x, None, x, 1.)
    with pytest.raises(_lib.DmhError, match='model_cond overlaps model_null'):
        ops.pag_shift(x, x, x.clone(), 1.)
    with pytest.raises(_lib.DmhError):
        ops.pag_shift(x, None, x.clone().double(), 1.)
    for bad in (-1., NAN, float('inf')):                      # the entry itself, behind the wrapper's own check
        with pytest.raises(_lib.DmhError, match='finite number >= 0'):
            ops.call('dmh_pag_shift', ops.ptr(x), None, ops.ptr(x.clone()), None, bad, 2, 8)


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
    cond, null, pert, computed = m._cond_null_pag(x, t, c, rf, mk, cond_scale)
    want_p = m._run(x, t, c, rf, mk, [keep], pert_lo=0)      # a separate B-row perturbed pass
    assert same(pert, want_p) and bool(torch.isfinite(pert).all())
    if cond_scale == 1:
        assert null is None and computed is None
        want_c = m.forward(x, t, c, rf, mk)
        assert same(cond, want_c)
    else:
        assert (computed is keep) if dedup else (computed is None)
        want_c, want_n, want_computed = m._cond_null(x, t, c, rf, mk)
        assert (want_computed is keep) if dedup else (want_computed is None)
        rows = keep.bool() if dedup else torch.ones(B_, dtype=torch.bool, device=dev())
        assert same(cond[rows], want_c[rows]) and same(null, want_n)
    for b in range(B_):                                       # the feature is not vacuous: every perturbed row differs
        assert not same(pert[b], want_c[b]), b
    assert m._engine._pert_lo is None                        # cleared behind the pass: the next pass perturbs nothing


# gate of the perturbed rows against the float64 oracle with the identity map: 10x the relative error measured on MI355X
# (DESIGN 4); the measurements are in the docstring of test_perturbed_rows_vs_float64_oracle
GATE_PERT = 4.6e-6


def test_perturbed_rows_vs_float64_oracle(monkeypatch):
    """the oracle's cfg_unet_forward on the CPU in float64, with oracle.unet.attention replaced HERE by the identity map (out = v
    through to_out) for the perturbed rows, and unpatched for the conditional rows.  The oracle picks eps = 1e-3 in its weight
    standardisation and channel LayerNorm for any dtype but fp32 (the reference's rule, CFG:121); the model under test is the fp32
    model, so both are given the fp32 rule's eps = 1e-5 here (ws_fold is the oracle's own function) — otherwise the float64 run
    is a different function and the conditional rows show it.  Measured on MI355X, relative to the largest value of the float64
    output: conditional rows 7.14e-7, perturbed rows 4.68e-7 (gate 10x that: GATE_PERT)."""
    from oracle import unet as OU
    m = _tiny()
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}
    x, t, c, rf, mk = _net_inputs()
    keep = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev())
    monkeypatch.setattr(m, '_keep_mask', lambda batch, p, device: keep)
    cond, null, pert, _ = m._cond_null_pag(x, t, c, rf, mk, 1.)

    def chan_layernorm(xx, gg):
        var = torch.var(xx, dim=1, unbiased=False, keepdim=True)
        return (xx - torch.mean(xx, dim=1, keepdim=True)) * (var + 1e-5).rsqrt() * gg
    monkeypatch.setattr(OU, 'ws_conv3x3', lambda xx, w, b: F.conv2d(xx, OU.ws_fold(w, 1e-5), b, 1, 1))
    monkeypatch.setattr(OU, 'chan_layernorm', chan_layernorm)
    args = (sd, x.cpu().double(), t.cpu(), c.cpu(), rf.cpu().double(), mk.cpu().double(), keep.cpu().bool())

    def identity(p, xx):
        v = F.conv2d(xx, p['to_qkv.weight']).chunk(3, dim=1)[2]
        return F.conv2d(v, p['to_out.weight'], p['to_out.bias'])
    was = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                   # (the oracle's sinusoidal embedding takes the default dtype)
    try:
        with torch.no_grad():
            ref_c = OU.cfg_unet_forward(*args)
            monkeypatch.setattr(OU, 'attention', identity)
            ref_p = OU.cfg_unet_forward(*args)
    finally:
        torch.set_default_dtype(was)
    assert ref_c.dtype == ref_p.dtype == torch.float64
    rel = lambda a, b: float((a.cpu().double() - b).abs().max() / b.abs().max())
    ec, ep = rel(cond, ref_c), rel(pert, ref_p)
    apart = rel(pert, ref_c)
    print(f'[parity] pag network vs float64 oracle: conditional rows {ec:.3e}, perturbed rows (identity map) {ep:.3e}; '
          f'perturbed vs conditional oracle {apart:.3e}')
    assert ep <= GATE_PERT, (ep, ec)
    assert ec <= 2e-5, ec                                     # (the project's gate for the UNet forward)
    assert apart > 100 * GATE_PERT                            # the two references are far enough apart to tell them from each other


# --------------------------------------------------------------------------------------------- 3. the loops
def _keyed(d, seed=5, first_id=40, rows=B_):
    d.rng.key_by_sample(seed, range(first_id, first_id + rows), dev())


def _sample_inputs():
    return tuple(g(v) for v in _cond_inputs(B_, SIZE))


def _composed_loop(d, ins, cond_scale, s):
    """the loop written from existing pieces: the passes one by one, the fp32 shift with torch on the CPU, the existing step"""
    from dmhomo_amd import ops
    m = d.model
    c, rf01, fl, mk = ins
    rf = ops.affine(rf01, 2., -1.)
    shape = (B_, 6, SIZE, SIZE)
    solver = d.sampler == 'dpmpp_2m'
    rank = d._dynamic_rank(shape, True)
    img = d.rng.randn(shape, dev()).contiguous()
    hist = torch.empty_like(img)
    for time, step, draws in d._sampler_steps(True, cond_scale):
        t = torch.full((B_,), time, device=dev(), dtype=torch.long)
        keep = m._keep_mask(B_, m.cond_drop_prob, dev())       # the one draw of the step
        cond = m._run(img, t, c, rf, mk, [keep])
        null = None if cond_scale == 1 else m._run(img, t, c, rf, mk, [m._null_mask(B_, dev())])
        pert = m._run(img, t, c, rf, mk, [keep], pert_lo=0)
        sc, sn = PC.shift32(cond.cpu(), None if null is None else null.cpu(), pert.cpu(), s)
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
    d.pag_scale = 2.5
    _keyed(d)
    got = d.sample(*ins, cond_scale=cond_scale)[0]
    _keyed(d)
    want = _composed_loop(d, ins, cond_scale, 2.5)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    d.pag_scale = None
    _keyed(d)
    assert not torch.equal(d.sample(*ins, cond_scale=cond_scale)[0], got)


# gates of the loop parity: 10x the worst relative deviation measured on MI355X against the float64 loop; the
# measurements are in the docstring of test_loops_vs_float64_loop
GATE_X0, GATE_IMG = 3.1e-6, 2.5e-6


def _float64_loop(d, nets, draws, s, dynamic, cs):
    """the loop in float64 on the recorded network outputs and noise: shift, blend, threshold, step -> per step (x_start, img)"""
    cpu = lambda v: None if v is None else v.cpu()
    img, hist, ni, out = draws[0].cpu().double(), None, 1, []
    ones = torch.ones(img.shape[0])
    for (time, step, _), (cond, null, pert, keep) in zip(d._sampler_steps(True, cs), nets):
        cond, null, _ = PC.shift64(cpu(cond), cpu(null), cpu(pert), s, cpu(keep))
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
    """measured on MI355X over the eight runs, relative to the largest value of the float64 tensor: per-step x_start <=
    3.13e-7, image <= 2.60e-7 (gates 10x that: GATE_X0 / GATE_IMG)"""
    from dmhomo_amd import ops
    m = _tiny()
    m.dedup_dropped_rows = True                              # (the dropped rows of cond are then unwritten: keep must reach the shift)
    d = _diffusion(m, 'pred_x0' if sampler == 'ddim' else 'pred_v')
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile = sampler, clip_mode, P_
    _, draws = _recording(d, monkeypatch)
    nets, pag = [], m._cond_null_pag

    def recorded(*a):
        out = pag(*a)
        nets.append(tuple(None if v is None else v.clone() for v in out))
        return out
    monkeypatch.setattr(m, '_cond_null_pag', recorded)
    c, rf01, fl, mk = _sample_inputs()
    d.pag_scale = 2.5
    torch.manual_seed(11)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, (B_, 6, SIZE, SIZE), cond_scale, trace=trace)
    assert len(trace) == len(nets) == S_ and all(e['pag'] is True for e in trace)
    ref = _float64_loop(d, nets, draws, 2.5, clip_mode == 'dynamic', cond_scale)
    rel = lambda a, b: float((a.cpu().double() - b).abs().max() / b.abs().max())
    ex = max(rel(e['x_start'], r[0]) for e, r in zip(trace, ref))
    ei = max(rel(e['img'], r[1]) for e, r in zip(trace, ref))
    print(f'[parity] pag_scale 2.5 {sampler} cond_scale {cond_scale} {clip_mode}: max rel |x_start - float64| = {ex:.3e}, '
          f'max rel |img - float64| = {ei:.3e}')
    assert ex <= GATE_X0 and ei <= GATE_IMG, (ex, ei)
    assert torch.equal(got, ops.affine(trace[-1]['img'], 0.5, 0.5))


def _runner(d, ins):
    def run(**kw):
        _keyed(d)
        return d.sample(*ins, **kw)[0].clone()
    return run


def test_captured_equals_eager():
    """bitwise, cond_scale 3 and 1, dedup_dropped_rows off and on; a second replay of the same capture gives the same samples"""
    from dmhomo_amd import cfg
    m = _tiny()
    d = _diffusion(m)
    d.rng = cfg.DeviceRng()
    d.pag_scale = 2.5
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
    d.pag_scale = 2.5
    want = run()
    assert not torch.equal(want, off) and bool(torch.isfinite(want).all())
    d.hip_graph = True
    assert torch.equal(run(), want) and torch.equal(run(), want) and d.graph_captures == 1


def test_capture_cache_counts():
    """a second value of pag_scale captures once more, None is the default's entry, going back hits the cache; None after use
    gives the default samples bitwise"""
    from dmhomo_amd import cfg
    d = _diffusion(_tiny())
    d.rng = cfg.DeviceRng()
    d.hip_graph = True
    run = _runner(d, _sample_inputs())
    default = run()
    assert d.graph_captures == 1
    d.pag_scale = 2.5
    a = run()
    assert d.graph_captures == 2 and not torch.equal(a, default)
    assert torch.equal(run(), a) and d.graph_captures == 2
    d.pag_scale = 3.
    b = run()
    assert d.graph_captures == 3 and not torch.equal(b, a)
    d.pag_scale = None
    assert same(run(), default) and d.graph_captures == 3
    d.pag_scale = 2.5
    assert torch.equal(run(), a) and d.graph_captures == 3
    d.hip_graph = False
    assert torch.equal(run(), a)
    d.pag_scale = None
    assert same(run(), default)                               # eager, after use: the default samples bitwise


@pytest.mark.parametrize('cond_scale', [3., 1.])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_pag_scale_0_gives_the_samples_of_none(sampler, cond_scale):
    """from the same generator state, with torch's own generator (every draw moves it): no draw was added"""
    d = _diffusion(_tiny())
    d.sampler = sampler
    ins = _sample_inputs()
    torch.manual_seed(21)
    off = d.sample(*ins, cond_scale=cond_scale)[0]
    after_off = torch.cuda.get_rng_state(dev())
    d.pag_scale = 0.
    torch.manual_seed(21)
    on = d.sample(*ins, cond_scale=cond_scale)[0]
    assert bool((on == off).all()) and torch.equal(torch.cuda.get_rng_state(dev()), after_off)
    d.pag_scale = 2.5
    torch.manual_seed(21)
    assert not torch.equal(d.sample(*ins, cond_scale=cond_scale)[0], off)
    d.pag_scale = None
    torch.manual_seed(21)
    assert same(d.sample(*ins, cond_scale=cond_scale)[0], off)
