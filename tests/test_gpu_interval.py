"""-m gpu: the guidance interval of the conditional sampler (``guidance_interval``): the two kernels that let one captured step
serve guided and unguided entries (dmh_rows_gated, dmh_guidance_gate) and cfg.GaussianDiffusion with the switch on, eager and
captured.

1. the row-list builder alone: every case of tests/interval_cases.py at the first, a middle and the last entry of a table;
2. the gate alone: bitwise copy at an unguided entry, nothing touched at a guided one, guards, pointers on and off 16 bytes;
3. behind the gate the existing factor and step kernels give what their calls without a null pass give;
4. the eager loops against a float64 loop fed the same network outputs, the interval as a per-entry flag;
5. identities ((0, 1) == None, nothing guided == cond_scale 1), captured == eager, the capture cache, dedup, streams, rows."""
import pytest
import torch

import guidance_cases as GC
import interval_cases as IC
import threshold_cases as TC
from gpu_util import dev
from test_gpu_guidance import _guarded, _recording, _step, bits, g, same
from test_gpu_solver import _cfg_diffusion, _cfg_model, _cond_inputs

pytestmark = pytest.mark.gpu


def _tables(S, pos, flag):
    """(cursor at pos, guided [S] whose entry pos holds ``flag`` and every other entry the opposite)"""
    guided = torch.full((S,), 0 if flag else 1, dtype=torch.uint8)
    guided[pos] = 1 if flag else 0
    return torch.tensor([pos], dtype=torch.int32, device=dev()), guided.to(dev())


# --------------------------------------------------------------------------------------------- 1. the row-list builder alone
def test_rows_gated_every_case():
    """rows[0 .. n] exact; the slots behind it and a guard word behind the buffer keep their sentinel"""
    from dmhomo_amd import ops
    checked = 0
    for name, B, keep, extra, null_side in IC.row_cases():
        kd = None if keep is None else torch.tensor(keep, dtype=torch.uint8, device=dev())
        for pos in (0, 2, 3):                                # first, middle and last entry of an S = 4 table
            for flag in (True, False):
                cursor, guided = _tables(4, pos, flag)
                size = 1 + B + extra
                buf = torch.full((size + 2,), IC.SENTINEL, dtype=torch.int32, device=dev())
                got = ops.rows_gated(kd, B, extra, cursor, guided, null_side=null_side, rows=buf[:size])
                assert got.data_ptr() == buf.data_ptr()
                want = IC.rows_ref(keep, B, extra, flag, null_side)
                out = buf.cpu().tolist()
                assert out[:len(want)] == want, (name, pos, flag, out, want)
                assert out[len(want):] == [IC.SENTINEL] * (size + 2 - len(want)), (name, pos, flag, out)
                checked += 1
    assert checked == 44 * 3 * 2


def test_rows_gated_guided_is_rows_from_keep_and_wide_batches():
    """a guided entry of the conditional side is dmh_rows_from_keep's list; more rows than one wave (B = 65, 200)"""
    from dmhomo_amd import ops
    gen = torch.Generator().manual_seed(3)
    for B, extra in ((5, 5), (64, 3), (65, 0), (200, 200)):
        keep = (torch.rand((B,), generator=gen) < 0.5).to(torch.uint8)
        for flag in (True, False):
            cursor, guided = _tables(3, 1, flag)
            rows = ops.rows_gated(keep.to(dev()), B, extra, cursor, guided).cpu().tolist()
            want = IC.rows_ref(keep.tolist(), B, extra, flag, False)
            assert rows[:len(want)] == want, (B, extra, flag)
            if flag:
                old = ops.rows_from_keep(keep.to(dev()), extra=extra).cpu().tolist()
                assert old[:len(want)] == want
    with pytest.raises(ValueError):
        ops.rows_gated(keep.to(dev()), 3, 0, cursor, guided)
    with pytest.raises(ValueError):
        ops.rows_gated(None, 3, 0, cursor[:0], guided)


# --------------------------------------------------------------------------------------------- 2. the gate alone
def _gate_values(B, n, seed):
    gen = torch.Generator().manual_seed(seed)
    cond, null = torch.randn((B, n), generator=gen) * 1.5, torch.randn((B, n), generator=gen) * 1.5
    flat, special = cond.view(-1), (float('nan'), -0.0, float('inf'), float('-inf'))
    m = flat.numel()
    where = (0, m // 3, (2 * m) // 3, m - 1) if m >= 4 else range(m)     # head, body and tail; the first m of them below 4
    for i, v in zip(where, special):
        flat[i] = v
    assert bool(torch.isnan(flat).any()) and (m < 3 or bool(torch.isinf(flat).any()))
    return cond, null


@pytest.mark.parametrize('B', GC.BATCHES)
def test_gate_copies_bitwise_or_touches_nothing(B):
    """sizes of guidance_cases.SIZES; cond and null on 16 bytes, both one float past it (the vector path with a scalar head),
    and out of phase (the word path).  The NaN guards around both tensors stay as they were"""
    from dmhomo_amd import ops
    assert GC.BATCHES == (1, 3)
    for k, n in enumerate(GC.SIZES):
        cond0, null0 = _gate_values(B, n, 50 + k)
        for off_c, off_n in ((0, 0), (1, 1), (3, 3), (3, 2), (0, 1)):
            for flag in (False, True):
                cond, cbuf = _guarded(cond0, off_c)
                null, nbuf = _guarded(null0, off_n)
                cbuf0, nbuf0 = cbuf.clone(), nbuf.clone()
                cursor, guided = _tables(4, 2, flag)
                got = ops.guidance_gate(cursor, guided, cond, null)
                what = (B, n, off_c, off_n, flag)
                assert got.data_ptr() == null.data_ptr()
                assert same(cbuf, cbuf0), what               # cond and its guards: never written
                if flag:
                    assert same(nbuf, nbuf0), what           # guided: null and its guards untouched
                else:
                    assert same(null, cond), what            # unguided: null is cond, bit for bit
                    lo, hi = 4 + off_n, 4 + off_n + B * n
                    assert same(nbuf[:lo], nbuf0[:lo]) and same(nbuf[hi:], nbuf0[hi:]), what


def test_gate_refuses_wrong_shapes_and_overlap():
    from dmhomo_amd import _lib, ops
    cursor, guided = _tables(4, 0, False)
    x = torch.zeros((2, 8), device=dev())
    with pytest.raises(ValueError):
        ops.guidance_gate(cursor, guided, x, x[:1].clone())
    with pytest.raises(ValueError):
        ops.guidance_gate(cursor, guided[:0], x, x.clone())
    with pytest.raises(_lib.DmhError, match='overlap'):
        ops.guidance_gate(cursor, guided, x, x)
    both = torch.zeros((24,), device=dev())
    with pytest.raises(_lib.DmhError, match='overlap'):
        ops.guidance_gate(cursor, guided, both[:16], both[8:])


# --------------------------------------------------------------------------------------------- 3. behind the gate
@pytest.mark.parametrize('keep', [None, [1, 0, 1]], ids=['all-rows', 'keep'])
def test_behind_the_gate_the_existing_kernels_do_the_unguided_step(keep):
    """at an unguided entry null <- cond; then dmh_guidance_factor answers exactly 1 in every row, and dmh_sampler_step / _ms /
    _thr / _gr give, under torch.equal, what their calls without a null pass give — rows with keep == 0 read a null row that
    holds their own conditional logits.  The one difference, pinned here: the blend returns +0.0 for a logit of -0.0."""
    from dmhomo_amd import ops
    shape = (3, 3, 4, 5)
    gen = torch.Generator().manual_seed(4)
    mc, mn, x, hist0, noise = (g(torch.randn(shape, generator=gen) * s) for s in (1.5, 1.5, 1., 1., 1.))
    mc[1, 2, 3, 4] = -0.0
    kd = None if keep is None else g(torch.tensor(keep, dtype=torch.uint8))
    thr = g(torch.tensor([1., 2.5, 1.25]))
    cursor, guided = _tables(4, 1, True)
    before = mn.clone()
    ops.guidance_gate(cursor, guided, mc, mn)
    assert same(mn, before)                                  # a guided entry: the null logits stay
    cursor, guided = _tables(4, 1, False)
    ops.guidance_gate(cursor, guided, mc, mn)
    assert same(mn, mc)
    kq, fq = TC.rank_of(0.9, 3 * 4 * 5)
    checked = 0
    for objective in (0, 1, 2):
        for clip in (0, 1):
            for kind in ('ddim', 'last', 'second'):
                mode = {'ddim': ops.MODE_DDIM, 'last': ops.MODE_LAST}.get(kind, ops.MODE_MULTISTEP)
                step = _step(objective, clip, mode, -0.4 if kind != 'last' else 0.)
                nz = noise if kind == 'ddim' else None
                what = (keep, objective, clip, kind)
                gf = ops.guidance_factor(step, mc, mn, 0.7, keep=kd)
                assert gf.tolist() == [1., 1., 1.], what
                if kind == 'second':
                    h_a, h_b = hist0.clone(), hist0.clone()
                    a = ops.sampler_step_ms(step, mc, mn, x, h_a, want_x_start=True, keep=kd)
                    b = ops.sampler_step_ms(step, mc, None, x, h_b, want_x_start=True)
                    assert torch.equal(h_a, h_b), what
                else:
                    a = ops.sampler_step(step, mc, mn, x, nz, want_x_start=True, keep=kd)[:2]
                    b = ops.sampler_step(step, mc, None, x, nz, want_x_start=True)[:2]
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what
                if (objective, clip, kind) == (1, 0, 'last'):        # img = x_start = the logit itself
                    assert bits(b[0])[1, 2, 3, 4].item() == -2 ** 31 and bits(a[0])[1, 2, 3, 4].item() == 0
                t_a, raw_a = ops.sampler_threshold(step, mc, mn, x, kq, fq, keep=kd)
                t_b, raw_b = ops.sampler_threshold(step, mc, None, x, kq, fq)
                assert torch.equal(t_a, t_b) and torch.equal(raw_a, raw_b), what
                hist = lambda: hist0.clone() if kind == 'second' else None
                a = ops.sampler_step_thr(step, mc, mn, x, nz, hist(), thr, want_x_start=True, keep=kd)
                b = ops.sampler_step_thr(step, mc, None, x, nz, hist(), thr, want_x_start=True)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what
                for t in (None, thr):                        # the rescaled entry on the factor of 1 it is handed
                    a = ops.sampler_step_gr(step, mc, mn, x, nz, hist(), t, gf, want_x_start=True, keep=kd)
                    if t is not None:
                        b = ops.sampler_step_thr(step, mc, None, x, nz, hist(), thr, want_x_start=True)
                    elif kind == 'second':
                        b = ops.sampler_step_ms(step, mc, None, x, hist(), want_x_start=True)
                    else:
                        b = ops.sampler_step(step, mc, None, x, nz, want_x_start=True)[:2]
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (what, t is None)
                t_b, raw_b = ops.sampler_threshold(step, mc, None, x, kq, fq)
                t_a, raw_a = ops.sampler_threshold_gr(step, mc, mn, x, gf, kq, fq, keep=kd)
                assert torch.equal(t_a, t_b) and torch.equal(raw_a, raw_b), what
                checked += 1
    assert checked == 18


# --------------------------------------------------------------------------------------------- 4. the loops, restated
T_, S_, B_, P_ = 100, 6, 3, 0.995
INTERVAL = (0.3, 0.7)
PATTERN = IC.PATTERNS[0][3]
# the project's gates for these loops at this size (tests/test_gpu_guidance.py; DESIGN 4: <= 10x the measured error)
GATE_X0, GATE_IMG = 3e-6, 3.9e-6


def _reference_loop(d, nets, draws, flags, phi, dynamic, cs):
    """the loop in float64 on the recorded network outputs and noise; ``flags[k]``: entry k is guided.  An unguided entry has no
    null pass, no blend and a factor of 1 -> per step (g or None, x_start, img)"""
    cpu = lambda t: None if t is None else t.cpu()
    img, hist, ni, out = draws[0].cpu().double(), None, 1, []
    ones = torch.ones(img.shape[0], dtype=torch.float64)
    for (time, step, _), (cond, null, keep), on in zip(d._sampler_steps(True, cs), nets, flags):
        cond, null, keep = cpu(cond), cpu(null), cpu(keep)
        assert (null is not None) == on
        gf = GC.factor_ref(cond, null, keep, cs, phi) if (on and phi) else ones
        noise = None
        if step.mode == 0:
            noise, ni = draws[ni].cpu(), ni + 1
        thr = None
        if dynamic:
            raw = GC.statement(step, cond, null, keep, img, noise, hist, None, gf)[2]
            thr = TC.threshold_ref(raw, P_)[1]
        img, x0, _ = GC.statement(step, cond, null, keep, img, noise, hist, thr, gf)
        hist = x0
        out.append((gf if (on and phi) else None, x0, img))
    assert ni == len(draws)
    return out


@pytest.mark.parametrize('phi', [0., 0.7])
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_eager_loops_vs_float64_loop(sampler, clip_mode, phi, monkeypatch):
    """interval (0.3, 0.7) over six entries: unguided, unguided, guided x 3, unguided.  Measured on MI355X over the eight runs:
    factor <= 3.2e-8 of its value (gate: one fp32 ulp, guidance_cases.GATE), per-step x_start <= 3.5e-7, image <= 4.3e-7.  Ten
    times that is not below the project's gates for these loops at this size (GATE_X0 / GATE_IMG), so they stand as they are"""
    from dmhomo_amd import ops
    m, _ = _cfg_model(0.5)
    d = _cfg_diffusion(m, size=16, T=T_, S=S_, objective='pred_x0' if sampler == 'ddim' else 'pred_v')
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile, d.guidance_rescale = sampler, clip_mode, P_, phi
    d.guidance_interval = INTERVAL
    nets, draws = _recording(d, monkeypatch)
    c, rf01, fl, mk = (g(t) for t in _cond_inputs(B_, 16))
    torch.manual_seed(11)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, (B_, 6, 16, 16), GC.CS, trace=trace)
    assert len(trace) == len(nets) == S_ and len(draws) == 1 + (S_ - 1 if sampler == 'ddim' else 0)
    assert [e['guided'] for e in trace] == PATTERN == IC.guided_pattern([e['time'] for e in trace], T_, INTERVAL)
    assert [n[1] is not None for n in nets] == PATTERN      # the null pass ran at the guided entries only
    for e in trace:
        if not e['guided']:
            assert 'gfac' not in e or e['gfac'].tolist() == [1.] * B_
        else:
            assert ('gfac' in e) == bool(phi)
    ref = _reference_loop(d, nets, draws, PATTERN, phi, clip_mode == 'dynamic', GC.CS)
    eg = max([float(((e['gfac'].cpu().double() - r[0]).abs() / r[0]).max()) for e, r in zip(trace, ref) if r[0] is not None],
             default=0.)
    ex = max(float((e['x_start'].cpu().double() - r[1]).abs().max()) for e, r in zip(trace, ref))
    ei = max(float((e['img'].cpu().double() - r[2]).abs().max()) for e, r in zip(trace, ref))
    print(f'[parity] guidance_interval {INTERVAL} phi {phi} {sampler} {clip_mode}: max|g - float64| / g = {eg:.2e}, '
          f'max|x_start - float64| = {ex:.2e}, max|img - float64| = {ei:.2e} (gates {GATE_X0:.1e} / {GATE_IMG:.1e})')
    assert ('thr' in trace[0]) == (clip_mode == 'dynamic')
    assert eg <= GC.GATE and ex <= GATE_X0 and ei <= GATE_IMG, (eg, ex, ei)
    assert torch.equal(got, ops.affine(trace[-1]['img'], 0.5, 0.5))
    torch.manual_seed(11)                                    # sample() is the same call
    assert torch.equal(d.sample(c, rf01, fl, mk, cond_scale=GC.CS)[0], got)


# --------------------------------------------------------------------------------------------- 5. identities, captured, rows
def _runner(d, ins):
    def run(graph, seed, interval, cond_scale=GC.CS):
        d.hip_graph, d.guidance_interval = graph, interval
        torch.manual_seed(seed)
        out = d.sample(*ins[seed], cond_scale=cond_scale)[0].clone()
        return out, torch.rand(4, device=dev())
    return run


def _check(got, want, what):
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_identities_eager_and_captured(sampler):
    """(0, 1) is no interval; an interval that holds no sampled time is cond_scale = 1 with the same seed; a proper interval is
    neither — output and generator state, eager and captured"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.sampler, d.guidance_rescale = sampler, 0.7
    ins = {3: [g(t) for t in _cond_inputs(B_, 16, 9)]}
    d.rng = cfg.DeviceRng()
    run = _runner(d, ins)
    for graph in (False, True):
        none, full = run(graph, 3, None), run(graph, 3, (0., 1.))
        _check(full, none, (sampler, graph, '(0, 1)'))
        nothing, one = run(graph, 3, IC.NOTHING), run(graph, 3, None, cond_scale=1.)
        _check(nothing, one, (sampler, graph, 'nothing guided'))
        proper = run(graph, 3, INTERVAL)
        assert not torch.equal(proper[0], none[0]) and not torch.equal(proper[0], one[0])
        assert torch.equal(proper[1], none[1])               # the generator ends where it ends without an interval
    d.hip_graph = False


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_captured_equals_eager_on_one_capture_for_every_interval(sampler, clip_mode):
    """bitwise, output and generator: the capturing call, new inputs on the same graph, two other intervals WITHOUT another
    capture (the flags are a table the call fills, not part of the graph), then None (its own capture) and back"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.sampler, d.clip_mode, d.guidance_rescale = sampler, clip_mode, 0.7
    ins = {3: [g(t) for t in _cond_inputs(B_, 16, 9)], 4: [g(t) for t in _cond_inputs(B_, 16, 10)]}
    d.rng = cfg.DeviceRng()
    run = _runner(d, ins)
    others = ((0.5, 1.), (0., 0.2))
    e3, e4, e_none = run(False, 3, INTERVAL), run(False, 4, INTERVAL), run(False, 3, None)
    e_others = [run(False, 3, gi) for gi in others]
    assert len({tuple(x[0].flatten().tolist()) for x in [e3, e_none] + e_others}) == 4       # four different samples
    what = (sampler, clip_mode)
    _check(run(True, 3, INTERVAL), e3, what + ('the capturing call',))
    _check(run(True, 4, INTERVAL), e4, what + ('new inputs on the same graph',))
    assert d.graph_captures == 1
    for gi, want in zip(others, e_others):
        _check(run(True, 3, gi), want, what + (gi,))
    _check(run(True, 3, IC.NOTHING), run(False, 3, IC.NOTHING), what + ('nothing guided',))
    assert d.graph_captures == 1
    _check(run(True, 3, None), e_none, what + ('None, capturing',))
    assert d.graph_captures == 2
    _check(run(True, 3, INTERVAL), e3, what + ('back',))
    _check(run(True, 4, None), run(False, 4, None), what + ('and back on None',))
    assert d.graph_captures == 2
    d.hip_graph = False


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_dedup_streams_and_row_independence(sampler, monkeypatch):
    """'batched' == 'streams' (also in two sub-batches), dedup_dropped_rows on == off, captured == eager, and a B = 3 call == the
    three B = 1 calls with the same global sample ids, all bitwise, with cond_drop_prob = 0.5: dropped rows occur at unguided
    entries, where they are computed; the keyed generator's draw index ends where it ends without an interval"""
    from dmhomo_amd import cfg
    S, B = S_, 3
    m, _ = _cfg_model(0.5)
    d = _cfg_diffusion(m, size=16, T=T_, S=S)
    d.sampler, d.clip_mode, d.guidance_rescale, d.guidance_interval = sampler, 'dynamic', 0.7, INTERVAL
    c, rf01, fl, mk = (g(t) for t in _cond_inputs(B, 16))
    d.rng = cfg.DeviceRng()
    draws = 1 + S + (S - 1 if sampler == 'ddim' else 0)      # the initial noise, S class-dropout draws, DDIM's step noise

    def run(lo, hi):
        d.rng.key_by_sample(5, range(40 + lo, 40 + hi), dev())
        out = d.sample(c[lo:hi].contiguous(), rf01[lo:hi].contiguous(), fl[lo:hi].contiguous(), mk[lo:hi].contiguous())[0]
        assert d.rng.state.tolist()[1] == draws
        return out.clone()
    masks = []
    with monkeypatch.context() as mp:                        # the class-dropout masks of the eager run, entry by entry
        keep_mask = m._keep_mask
        mp.setattr(m, '_keep_mask', lambda *a: masks.append(keep_mask(*a)) or masks[-1])
        whole = run(0, B)
    assert len(masks) == S
    dropped = [int((k == 0).sum()) for k in masks]
    assert any(n > 0 for n, on in zip(dropped, PATTERN) if not on) and any(n > 0 for n, on in zip(dropped, PATTERN) if on), dropped
    assert not torch.equal(whole[0], whole[1])
    for b in range(B):
        assert torch.equal(run(b, b + 1)[0], whole[b]), b
    m.cfg_mode = 'streams'
    assert torch.equal(run(0, B), whole)
    m.cfg_mode, m.dedup_dropped_rows = 'batched', True
    assert torch.equal(run(0, B), whole)
    d.hip_graph = True
    assert torch.equal(run(0, B), whole)                      # captured, batched, dedup
    m.cfg_mode = 'streams'
    assert torch.equal(run(0, B), whole)                      # captured, streams, dedup
    m.stream_splits = 2
    assert torch.equal(run(0, B), whole)                      # ... in two sub-batches per pass
    m.dedup_dropped_rows = False
    assert torch.equal(run(0, B), whole)
    m.stream_splits = 1
    assert torch.equal(run(0, B), whole)
    m.cfg_mode = 'batched'
    assert torch.equal(run(0, B), whole)                      # captured, batched, every row computed
    for b in range(B):
        assert torch.equal(run(b, b + 1)[0], whole[b]), b     # captured B = 1 calls
    d.guidance_interval = None
    assert not torch.equal(run(0, B), whole)
    d.hip_graph, m.dedup_dropped_rows, m.cfg_mode, m.stream_splits = False, False, 'batched', 1


def test_unconditional_class_refuses_an_interval():
    from test_gpu_solver import _ddp_model
    from dmhomo_amd import ddpm
    m, _ = _ddp_model(False)
    d = ddpm.GaussianDiffusion(m, image_size=16, timesteps=T_, sampling_timesteps=S_).to(dev())
    d.guidance_interval = INTERVAL
    with pytest.raises(ValueError, match='unconditional'):
        d.sample(batch_size=2)


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_cond_scale_1_ignores_the_interval(sampler):
    """no null pass, nothing to leave out: bit for bit the samples without an interval, eager and captured, on today's capture"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.sampler = sampler
    ins = {3: [g(t) for t in _cond_inputs(2, 16)]}
    d.rng = cfg.DeviceRng()
    run = _runner(d, ins)
    want = run(False, 3, None, cond_scale=1.)
    _check(run(False, 3, INTERVAL, cond_scale=1.), want, 'eager')
    _check(run(True, 3, INTERVAL, cond_scale=1.), want, 'captured')
    _check(run(True, 3, None, cond_scale=1.), want, 'captured, no interval')
    assert d.graph_captures == 1
    d.hip_graph = False
