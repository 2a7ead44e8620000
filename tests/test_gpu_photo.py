"""-m gpu: photometric-consistency guidance of the conditional sampler (``photo_guidance``): the kernels (dmh_photo_weights,
dmh_photo_guide[_dev], dmh_photo_energy) and cfg.GaussianDiffusion with the switch on, eager and captured.

1. the kernels alone against the float64 statement of tests/photo_cases.py, over its shapes, batches, flow and mask kinds and
   the three forms of the network output (cond only, cond + null, cond + null + keep with a dropped row);
2. bitwise repeatability where many pixels add into one target, and the accumulator left zero;
3. the eager loops against a float64 loop fed the same network outputs;
4. captured == eager, dedup on == off, 'batched' == 'streams', another flow / mask / weight on a captured step, the refusals."""
import pytest
import torch

import guidance_cases as GC
import photo_cases as PC
import threshold_cases as TC
from gpu_util import dev
from test_gpu_guidance import _recording, g, same
from test_gpu_solver import _cfg_diffusion, _cfg_model, _cond_inputs

pytestmark = pytest.mark.gpu

# Gates of the fp32 outputs: 10x the worst error measured on MI355X against the float64 statement.  Measured over the
# 192 cases x 3 forms of the table: guided logits 6.59e-7 absolute (blended logits up to 13 in magnitude, where an fp32 ulp is
# 9.5e-7); s 9.66e-8 of max(1, s) (s reaches the hundreds where every pixel lands on a corner: an absolute figure would be an ulp
# of that), which is the one rounding of the fixed-point sum to fp32 (2^-24 = 5.96e-8) and that of the products mask * weight.
GATE_Y, GATE_S = 6.6e-6, 9.7e-7
# The energy is float64 throughout (the fp32 taps are the statement's too): kernel and statement differ in summation order only.
# Each of the n = 3 H W terms m * (u - x)^2 carries at most 8 roundings relative to m * (|u| + |x|)^2 (four products and three
# sums in u, the difference, the square, the product with m: the difference can cancel, hence the scale), a sum of n nonnegative
# terms in any order at most n - 1 more: |E - E64| <= (n + 8) * 2^-53 * Escale, Escale = mean m * (|u| + |x|)^2
# (photo_cases.energy_scale); the gate is that bound, in units of 2^-53 * Escale ("ulps of the scale").
energy_gate = lambda H, W: 3. * H * W + 8.


def _pstep(sqrt_ac=0.7, cs=3.):
    from dmhomo_amd import _lib
    return _lib.DmhStep(objective=1, clip=1, mode=1, cond_scale=cs, sqrt_recip_ac=1.3, sqrt_recipm1_ac=0.8, sqrt_ac=sqrt_ac,
                        sqrt_1m_ac=0.6, c0=0.9, c1=0.3, c2=0.)


def _guarded4(x, fill=float('nan')):
    """x inside a buffer of ``fill`` -> (the view, the buffer, the offset): the words around an output must stay what they were"""
    buf = torch.full((x.numel() + 32,), fill, device=dev(), dtype=x.dtype)
    view = buf[16:16 + x.numel()].view(x.shape)
    view.copy_(x)
    return view, buf


def _untouched(buf, n):
    return bool(torch.isnan(buf[:16]).all()) and bool(torch.isnan(buf[16 + n:]).all())


def _guide(case, which, step, w, acc, s, dev_struct=False):
    """one guarded dmh_photo_guide[_dev] -> guided on the CPU"""
    from dmhomo_amd import ops
    cond, null, keep = (g(t) for t in PC.variant(case, which))
    out, obuf = _guarded4(torch.full(case['cond'].shape, 777.))
    if dev_struct:
        table_, tt, cursor, cur = ops.step_table([step], [0], dev())
        ops.sampler_seek(cursor, 0, table_, tt, cur, torch.zeros((case['B'],), dtype=torch.int64, device=dev()))
        got = ops.photo_guide_dev(cur, cond, null, keep, g(case['flow']), g(case['mask']), s, w, acc, out=out)
    else:
        got = ops.photo_guide(step, cond, null, keep, g(case['flow']), g(case['mask']), s, w, acc, out=out)
    assert got is out and _untouched(obuf, out.numel())
    return out.cpu()


# --------------------------------------------------------------------------------------------- 1. the kernels alone
@pytest.mark.parametrize('B', PC.BATCHES)
@pytest.mark.parametrize('shape', PC.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_kernels_against_the_statement(shape, B):
    from dmhomo_amd import ops
    H, W = shape
    table = PC.cases(shapes=(shape,), batches=(B,))
    assert len(table) == len(PC.FLOWS) * len(PC.MASKS)
    acc = ops.photo_acc(B, H, W, dev())
    step, w = _pstep(), 1.
    lam = PC.lam32(w, step.sqrt_ac)
    ey = es = ee = 0.
    for name, c in table:
        mats = PC.matrices(c['flow'])
        flow, mask = g(c['flow']), g(c['mask'])
        sbuf_view, sbuf = _guarded4(torch.full((B, H, W), 777.))
        s = ops.photo_weights(flow, mask, acc, out=sbuf_view)
        assert s is sbuf_view and _untouched(sbuf, s.numel()) and not bool(acc.any()), name
        s_ref = PC.weights_ref(c['flow'], c['mask'], mats)
        es = max(es, float(((s.cpu().double() - s_ref).abs() / s_ref.clamp(min=1.)).max()))
        for which in PC.VARIANTS:
            what = (name, which)
            x = PC.blend32(*PC.variant(c, which), step.cond_scale)
            y = _guide(c, which, step, w, acc, s)
            assert not bool(acc.any()), what                 # the pass that finishes im2 leaves the accumulator zero
            y_ref = PC.guide_ref(x, c['flow'], c['mask'], lam, mats=mats)
            ey = max(ey, float((y.double() - y_ref).abs().max()))
            e = ops.photo_energy(g(x), flow, mask).cpu()
            e_ref = PC.energy_ref(x, c['flow'], c['mask'], mats)
            scale = PC.energy_scale(x, c['flow'], c['mask'], mats)
            if c['mask_kind'] == 'zero':                      # nothing to pull on: the blend bit for bit, and no energy
                assert same(y, x) and e.tolist() == [0.] * B, what
            else:
                live = scale > 0.                             # (a binary draw over the four pixels of 2 x 2 can be all zero)
                assert e[~live].tolist() == [0.] * int((~live).sum()), what
                if bool(live.any()):
                    ee = max(ee, float(((e - e_ref).abs()[live] / (2. ** -53 * scale[live])).max()))
                # the statement descends (tests/test_photo_host.py), and so does what the kernel wrote
                after = PC.energy_ref(y, c['flow'], c['mask'], mats)
                assert bool((after[e_ref > 0.] < e_ref[e_ref > 0.]).all()), (what, after, e_ref)
            if which == 'cond+null+keep':                     # the dropped row's conditional logits are its null logits
                drop = c['B'] // 2
                alone = dict(c, cond=c['null'])
                assert same(y[drop], _guide(alone, 'cond+null', step, w, acc, s)[drop]), what
        if (name, B) == (table[0][0], PC.BATCHES[0]) or c['flow_kind'] == 'fold' and c['mask_kind'] == 'fraction':
            a = _guide(c, 'cond+null+keep', step, w, acc, s)
            assert same(a, _guide(c, 'cond+null+keep', step, w, acc, s, dev_struct=True)), name       # the _dev twin
    print(f'[parity] photo kernels {B} x {H} x {W}, {len(table)} cases x {len(PC.VARIANTS)} forms: max|guided - float64| = {ey:.2e} '
          f'(gate {GATE_Y:.1e}), max|s - float64| / max(1, s) = {es:.2e} (gate {GATE_S:.1e}), max|E - float64| = {ee:.1f} ulps of the scale '
          f'(gate {energy_gate(H, W):.0f})')
    assert ey <= GATE_Y and es <= GATE_S and ee <= energy_gate(H, W), (ey, es, ee)


@pytest.mark.parametrize('shape', PC.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_zero_flow_full_mask_lambda_1_makes_the_two_images_equal(shape):
    """d' = (1 - lambda) d: at lambda = 1 (w = 1 at alpha_bar = 1) both images land on their mean"""
    from dmhomo_amd import ops
    H, W = shape
    (name, c), = PC.cases(shapes=(shape,), batches=(3,), flows=('zero',), masks=('one',))
    acc = ops.photo_acc(3, H, W, dev())
    s = ops.photo_weights(g(c['flow']), g(c['mask']), acc)
    # the fp32 taps of a zero flow miss the pixel by a rounding of the normalised coordinate (not at 2 x 2; 3.8e-6 at 33 x 47):
    # ``miss`` is how far the warp is from the identity, as a bound on |u - im2| / max|im2|; 0 where the taps are exact
    eye = torch.eye(H * W, dtype=torch.float64)
    miss = max(float((M - eye).abs().sum(dim=1).max()) for M in PC.matrices(c['flow']))
    assert miss <= 2. ** -18 and (miss == 0.) == (shape == (2, 2))
    assert float((s.cpu().double() - 1.).abs().max()) <= miss + GATE_S
    for which in PC.VARIANTS:
        y = _guide(c, which, _pstep(sqrt_ac=1.), 1., acc, s)
        x = PC.blend32(*PC.variant(c, which), 3.).double()
        slack = 2. * miss * float(x.abs().max())
        err = float((y[:, :3] - y[:, 3:]).abs().max())
        assert err <= 2. * GATE_Y + slack, (name, which, err)
        assert float((y[:, :3].double() - 0.5 * (x[:, :3] + x[:, 3:])).abs().max()) <= GATE_Y + slack, (name, which)


# --------------------------------------------------------------------------------------------- 2. repeatable, whatever adds first
@pytest.mark.parametrize('flow_kind', ['far', 'fold'])
def test_scatter_is_bitwise_repeatable_and_leaves_the_accumulator_zero(flow_kind):
    """33 x 47: seven workgroups per sample and channel add into the same few targets ('far': every pixel lands on a border)"""
    from dmhomo_amd import ops
    (name, c), = PC.cases(shapes=(PC.SHAPES[-1],), batches=(3,), flows=(flow_kind,), masks=('fraction',))
    acc = ops.photo_acc(3, c['H'], c['W'], dev())
    runs = []
    for _ in range(3):
        s = ops.photo_weights(g(c['flow']), g(c['mask']), acc)
        assert not bool(acc.any())
        y = _guide(c, 'cond+null+keep', _pstep(), 1., acc, s)
        assert not bool(acc.any())
        runs.append((s.cpu(), y))
    assert float(runs[0][0].max()) > 4.                       # targets that many pixels add into (ten folded columns x mask 0.5)
    for s, y in runs[1:]:
        assert same(s, runs[0][0]) and same(y, runs[0][1]), name


def test_wrapper_errors():
    from dmhomo_amd import _lib, ops
    x = torch.zeros((2, 6, 4, 4), device=dev())
    flow, mask = torch.zeros((2, 2, 4, 4), device=dev()), torch.ones((2, 1, 4, 4), device=dev())
    acc = ops.photo_acc(2, 4, 4, dev())
    s = ops.photo_weights(flow, mask, acc)
    for args in ((x[:, :3].contiguous(), None, None, flow, mask, s, 0.5, acc), (x, x[:1].clone(), None, flow, mask, s, 0.5, acc),
                 (x, None, None, flow[:1].clone(), mask, s, 0.5, acc), (x, None, None, flow, mask[:1].clone(), s, 0.5, acc),
                 (x, None, None, flow, mask, s[:1].clone(), 0.5, acc), (x, None, None, flow, mask, s, 0.5, acc[:10])):
        with pytest.raises(ValueError):
            ops.photo_guide(_pstep(), *args)
    with pytest.raises(_lib.DmhError, match='overlaps'):
        ops.photo_guide(_pstep(), x, None, None, flow, mask, s, 0.5, acc, out=x)
    with pytest.raises(_lib.DmhError, match='w='):
        ops.photo_guide(_pstep(), x, None, None, flow, mask, s, 0., acc)
    with pytest.raises(_lib.DmhError, match='keep needs model_null'):
        ops.photo_guide(_pstep(), x, None, torch.ones(2, dtype=torch.uint8, device=dev()), flow, mask, s, 0.5, acc)
    with pytest.raises(ValueError):
        ops.photo_energy(x[:, :5].contiguous(), flow, mask)
    with pytest.raises(ValueError):
        ops.photo_acc(1, 1, 4, dev())
    assert not bool(acc.any())


# --------------------------------------------------------------------------------------------- 3. the loops, restated
T_, S_, B_, P_, W_ = 100, 4, 3, 0.995, 0.5
# gates of the loop parity: 10x the worst error measured on MI355X against the float64 loop; the measurements are in
# the docstring of test_loops_vs_float64_loop
GATE_X0, GATE_IMG = 1.4e-6, 3.3e-6


def _reference_loop(d, nets, draws, ins, w, dynamic, cs):
    """the loop in float64 on the recorded network outputs and noise: the blend in fp32, the correction, the threshold and the
    step in float64 -> per step (E of the blend, x_start, img)"""
    _, _, flow, mask = (t.cpu() for t in ins)
    mats = PC.matrices(flow)
    cpu = lambda t: None if t is None else t.cpu()
    img, hist, ni, out = draws[0].cpu().double(), None, 1, []
    ones = torch.ones(img.shape[0])
    for (time, step, _), (cond, null, keep) in zip(d._sampler_steps(True, cs), nets):
        x = PC.blend32(cpu(cond), cpu(null), cpu(keep), cs)
        y = PC.guide_ref(x, flow, mask, PC.lam32(w, step.sqrt_ac), mats=mats)
        noise = None
        if step.mode == 0:
            noise, ni = draws[ni].cpu(), ni + 1
        thr = None
        if dynamic:
            raw = GC.statement(step, y, None, None, img, noise, hist, None, ones)[2]
            thr = TC.threshold_ref(raw, P_)[1]
        img, x0, _ = GC.statement(step, y, None, None, img, noise, hist, thr, ones)
        hist = x0
        out.append((PC.energy_ref(x, flow, mask, mats), x0, img, PC.energy_scale(x, flow, mask, mats)))
    assert ni == len(draws)
    return out


@pytest.mark.parametrize('cs', [1., 3.])
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_vs_float64_loop(sampler, clip_mode, cs, monkeypatch):
    """measured on MI355X over the eight runs: per-step x_start <= 1.39e-7, image <= 3.25e-7 (gates 10x that: GATE_X0 /
    GATE_IMG); trace['photo'] <= 1.9 ulps of its scale (the energy gate at 16 x 16: 776)"""
    from dmhomo_amd import ddpm, ops
    m, _ = _cfg_model(0.5)
    d = _cfg_diffusion(m, size=16, T=T_, S=S_, objective='pred_x0')
    d.sampler, d.clip_mode, d.dynamic_threshold_percentile = sampler, clip_mode, P_
    nets, draws = _recording(d, monkeypatch)
    ins = tuple(g(t) for t in _cond_inputs(B_, 16))
    c, rf01, fl, mk = ins
    torch.manual_seed(11)
    before = d.sample(c, rf01, fl, mk, cond_scale=cs)[0]      # the switch has never been on
    nets.clear(), draws.clear()
    d.photo_guidance = W_
    torch.manual_seed(11)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, (B_, 6, 16, 16), cs, trace=trace)
    assert len(trace) == len(nets) == S_ and len(draws) == 1 + (S_ - 1 if sampler == 'ddim' else 0)
    assert all((n[1] is None) == (cs == 1.) for n in nets)
    ref = _reference_loop(d, nets, draws, ins, W_, clip_mode == 'dynamic', cs)
    ex = max(float((e['x_start'].cpu().double() - r[1]).abs().max()) for e, r in zip(trace, ref))
    ei = max(float((e['img'].cpu().double() - r[2]).abs().max()) for e, r in zip(trace, ref))
    ee = max(float(((e['photo'].cpu() - r[0]).abs() / (2. ** -53 * r[3])).max()) for e, r in zip(trace, ref))
    print(f'[parity] photo {sampler} {clip_mode} cond_scale {cs}: E of the blend {float(ref[0][0].mean()):.3e} -> '
          f'{float(ref[-1][0].mean()):.3e}; max|x_start - float64| = {ex:.2e}, max|img - float64| = {ei:.2e}, '
          f'max|E - float64| = {ee:.1f} ulps of the scale')
    assert all(e['photo'].shape == (B_,) and e['photo'].dtype == torch.float64 for e in trace)
    assert ex <= GATE_X0 and ei <= GATE_IMG and ee <= energy_gate(16, 16), (ex, ei, ee)
    assert torch.equal(got, ops.affine(trace[-1]['img'], 0.5, 0.5))
    # the public score of the returned sample is the statement's
    score = ddpm.photometric_error(got, fl, mk).cpu()
    want = PC.energy_ref(got.cpu(), fl.cpu(), mk.cpu())
    scale = PC.energy_scale(got.cpu(), fl.cpu(), mk.cpu())
    assert score.dtype == torch.float64 and bool(((score - want).abs() <= energy_gate(16, 16) * 2. ** -53 * scale).all())
    # sample() is the same call; off is another sample, and exactly the one it was before the switch was ever on
    torch.manual_seed(11)
    assert torch.equal(d.sample(c, rf01, fl, mk, cond_scale=cs)[0], got)
    d.photo_guidance = None
    torch.manual_seed(11)
    off = d.sample(c, rf01, fl, mk, cond_scale=cs)[0]
    assert not torch.equal(off, got) and torch.equal(off, before)


# --------------------------------------------------------------------------------------------- 4. captured, dedup, streams
def _keyed_runner(d, seed=5, first_id=40):
    def run(ins, **kw):
        c, rf01, fl, mk = ins
        d.rng.key_by_sample(seed, range(first_id, first_id + c.shape[0]), dev())
        return d.sample(c, rf01, fl, mk, **kw)[0].clone()
    return run


@pytest.mark.parametrize('cs', [1., 3.])
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_captured_equals_eager_in_every_mode(sampler, clip_mode, cs):
    """bitwise: hip_graph against the eager loop under 'batched' and 'streams', dedup_dropped_rows on and off"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.sampler, d.clip_mode = sampler, clip_mode
    d.photo_guidance = W_
    d.rng = cfg.DeviceRng()
    run = _keyed_runner(d)
    ins = tuple(g(t) for t in _cond_inputs(B_, 16))
    want = run(ins, cond_scale=cs)
    for mode in ('batched', 'streams'):
        for dedup in (False, True):
            m.cfg_mode, m.dedup_dropped_rows = mode, dedup
            d.hip_graph = False
            assert torch.equal(run(ins, cond_scale=cs), want), (mode, dedup, 'eager')
            d.hip_graph = True
            assert torch.equal(run(ins, cond_scale=cs), want), (mode, dedup, 'captured')
            assert torch.equal(run(ins, cond_scale=cs), want), (mode, dedup, 'replayed')
    d.hip_graph, m.dedup_dropped_rows, m.cfg_mode = False, False, 'batched'
    d.photo_guidance = None
    assert not torch.equal(run(ins, cond_scale=cs), want)


def test_captured_step_takes_this_calls_flow_mask_and_weight():
    """nothing of flow, mask or s is baked into a capture: a second call with other conditions on the same captured step is the
    eager loop's sample; another weight is right too; None is the default's entry"""
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.rng = cfg.DeviceRng()
    run = _keyed_runner(d)
    ins_a = tuple(g(t) for t in _cond_inputs(B_, 16))
    c, rf01, fl, mk = (g(t) for t in _cond_inputs(B_, 16, seed=23))
    ins_b = (c, rf01, fl * 2., mk)                            # other conditions altogether: another flow, another mask
    default = run(ins_a)
    d.photo_guidance = W_
    eager_a, eager_b = run(ins_a), run(ins_b)
    assert not torch.equal(eager_a, eager_b) and not torch.equal(eager_a, default)
    d.photo_guidance = 0.25
    eager_quarter = run(ins_b)
    assert not torch.equal(eager_quarter, eager_b)
    d.hip_graph = True
    d.photo_guidance = W_
    assert torch.equal(run(ins_a), eager_a) and d.graph_captures == 1
    assert torch.equal(run(ins_b), eager_b) and d.graph_captures == 1
    assert torch.equal(run(ins_a), eager_a) and d.graph_captures == 1
    d.photo_guidance = 0.25
    assert torch.equal(run(ins_b), eager_quarter)
    d.photo_guidance = None
    assert torch.equal(run(ins_a), default)
    d.photo_guidance = W_
    n = d.graph_captures
    assert torch.equal(run(ins_b), eager_b) and d.graph_captures == n
    d.hip_graph = False


@pytest.mark.parametrize('other, value', [('guidance_rescale', 0.7), ('apg_eta', 0.), ('guidance_interval', (0.25, 0.75)),
                                          ('objective', 'pred_v')])
def test_refusals_raise_in_sample(other, value):
    from dmhomo_amd import cfg
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=T_, S=S_)
    d.rng = cfg.DeviceRng()
    ins = tuple(g(t) for t in _cond_inputs(2, 16))
    d.photo_guidance = W_
    setattr(d, other, value)
    for graph in (False, True):
        d.hip_graph = graph
        with pytest.raises(ValueError, match=f'photo_guidance.*{other}'):
            _keyed_runner(d)(ins)
    d.hip_graph = False
