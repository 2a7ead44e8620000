"""-m gpu: sampling around known pixels (cfg.GaussianDiffusion.sample_known): the kernels (dmh_known_blend, dmh_known_error) and
the conditional sampler with kept pixels, eager and captured.

1. dmh_known_blend alone, into NaN-guarded buffers at every 16-byte phase, bitwise against the statement of
   tests/known_cases.py; dmh_known_error against the exact score;
2. the sampler: nothing kept == sample(), kept elements and their bytes exact, the eager loops against a float64 loop fed the
   same network outputs, captured == eager, dedup on == off, 'batched' == 'streams', capture counts, photo guidance, pag_scale
   and flow_guidance on top, the score and the trace, Trainer.keep, the refusals.

The score's bound.  x (the fp32 logits) and K are taken as given; the statement is exact rational arithmetic rounded to float64
once.  The kernel forms d = x - K in float64 (one rounding: the two fp32 values may be far apart in exponent), squares it (the
error of d twice, one more rounding), adds the n kept terms, all >= 0, in some fixed order (n - 1 roundings, each relative to a
partial sum that is at most the total) and divides by the exact count (one more): |E - E_exact| <= (3 + (n - 1) + 1 + 1/2) u E
with u = 2^-53, the last half for the statement's own rounding.  error_gate(n) = n + 4, in units of 2^-53 * E."""
import pytest
import torch

import known_cases as KC
import photo_cases as PC
from gpu_util import dev
from test_gpu_guidance import _recording, g, same
from test_gpu_solver import _cfg_diffusion, _cfg_model, _cond_inputs

pytestmark = pytest.mark.gpu

error_gate = lambda n: n + 4.


# --------------------------------------------------------------------------------------------- 1. the kernels alone
def _place(x, off, fill=float('nan')):
    """x inside a buffer of ``fill``, starting ``off`` elements past a 16-byte boundary -> (the view, the buffer, where it
    starts): the words around an output must stay what they were"""
    x = x.contiguous()
    lo = 16 + off
    buf = torch.full((x.numel() + lo + 20,), fill, device=dev(), dtype=x.dtype)
    assert buf.data_ptr() % 16 == 0
    view = buf[lo:lo + x.numel()].view(x.shape)
    view.copy_(x)
    return view, buf, lo


def _untouched(buf, lo, n):
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())


# where the operands sit relative to the output: all floats in the output's 16-byte phase with the mask bytes of a vector on a
# 4-byte boundary (the vector path, one 32-bit mask load), the mask one byte off (the vector path, byte loads), ``known`` one
# float off (no common phase: the scalar path)
LAYOUTS = ('vector', 'mask-off', 'known-off')


def _blend(c, off, layout, in_place):
    """one guarded dmh_known_blend of case c -> (out on the CPU, guards untouched)"""
    from dmhomo_amd import ops
    cond, cbuf, clo = _place(c['cond'], off)
    null = None if c['null'] is None else _place(c['null'], off)[0]
    keep = None if c['keep'] is None else g(c['keep'])
    known = _place(c['K'], off + (1 if layout == 'known-off' else 0))[0]
    kmask = _place(c['mask'], off + (1 if layout == 'mask-off' else 0), fill=0)[0]
    if in_place:
        got = ops.known_blend(cond, null, keep, KC.CS, known, kmask)
        assert got is cond
        return got.cpu(), _untouched(cbuf, clo, cond.numel())    # (in place the output buffer is cond's: its guards)
    out, obuf, olo = _place(torch.full(c['cond'].shape, 777.), off)
    got = ops.known_blend(cond, null, keep, KC.CS, known, kmask, out=out)
    assert got is out and same(cond.cpu(), c['cond'])         # (the inputs are left as they were)
    return out.cpu(), _untouched(obuf, olo, out.numel())


@pytest.mark.parametrize('B', KC.BATCHES)
@pytest.mark.parametrize('n', KC.PER_ROW)
def test_blend_is_the_statement_bit_for_bit(n, B):
    table = KC.cases(per_row=(n,), batches=(B,))
    assert len(table) == len(KC.FORMS) * len(KC.MASKS)
    launches = nan_kept_free = 0
    for name, c in table:
        x = KC.blend32(c['cond'], c['null'], c['keep'], KC.CS)
        want = KC.select(x, c['K'], c['mask'])
        kept = c['mask'] != 0
        assert not bool(torch.isnan(want[kept]).any())        # a NaN logit under a kept element is gone ...
        assert torch.equal(torch.isnan(want[~kept]), torch.isnan(x[~kept])), name      # ... one elsewhere stays
        nan_kept_free += int(torch.isnan(want[~kept]).any())
        if c['mask_kind'] == 'zero':
            assert same(want, x)
        for off in KC.OFFSETS:
            for layout in LAYOUTS:
                for in_place in (False, True):
                    what = (name, off, layout, in_place)
                    got, guards = _blend(c, off, layout, in_place)
                    launches += 1
                    assert guards, what
                    assert same(got, want), what
                    if c['mask_kind'] == 'zero':
                        assert same(got, x), what            # nothing kept: guided_logit bit for bit
    assert launches == len(table) * len(KC.OFFSETS) * len(LAYOUTS) * 2
    assert nan_kept_free >= (4 if n > 3 else 0)               # (the table does hold NaN logits that must survive)


def test_in_place_leaves_the_words_around_cond():
    """the guard check of the in-place form, on a cond without NaN of its own at its ends"""
    from dmhomo_amd import ops
    for n, B in ((5, 3), (210, 3), (1536, 1)):
        c = KC.make_case(B, n, 'cond+null', 'random', 7, nan_kept=False)
        for off in KC.OFFSETS:
            cond, cbuf, clo = _place(c['cond'], off)
            ops.known_blend(cond, _place(c['null'], off)[0], None, KC.CS, _place(c['K'], off)[0], _place(c['mask'], off, fill=0)[0])
            assert _untouched(cbuf, clo, cond.numel()), (n, B, off)
            assert same(cond.cpu(), KC.blend_ref(c['cond'], c['null'], None, KC.CS, c['K'], c['mask']))


def test_write_back_form_returns_the_callers_values():
    """null = NULL, cond_scale = 1, in place on the unnormalised image with ``known`` itself: every byte value comes back"""
    from dmhomo_amd import ops
    k = KC.all_bytes().repeat(18).reshape(3, 6, 16, 16)
    two, one, half = (torch.tensor(v, dtype=torch.float32) for v in (2., 1., 0.5))
    img = (k * two - one) * half + half
    assert not same(img, k)
    mask = torch.zeros((3, 6 * 256), dtype=torch.uint8)
    mask[:, :3 * 256] = 1
    out = ops.known_blend(g(img), None, None, 1., g(k), g(mask))
    assert same(out.cpu()[:, :3], k[:, :3]) and same(out.cpu()[:, 3:], img[:, 3:])
    assert torch.equal(ops.to_uint8(out).cpu()[:, :3].reshape(3, -1), torch.arange(256, dtype=torch.uint8).repeat(3, 3))


ERR_SIZES = (1, 5, 210, 1536, 9600)                            # 9600 = 6 * 40^2: three workgroups per row at B = 3


@pytest.mark.parametrize('B', KC.BATCHES)
@pytest.mark.parametrize('n', ERR_SIZES)
def test_error_against_the_exact_score(n, B):
    from dmhomo_amd import ops
    assert ops.known_error_splits(B, n) == min((n + 4095) // 4096, max(1024 // B, 1))
    masks = KC.MASKS if n < 9600 else ('all', 'random')
    worst = 0.
    for i, (form, mask_kind) in enumerate((f, mk) for f in KC.FORMS for mk in masks):
        name = f'{form}-{mask_kind}-{B}x{n}'
        c = KC.make_case(B, n, form, mask_kind, 500 + 31 * i + n + B, nan_kept=False)         # NaN under free elements only
        x = KC.blend32(c['cond'], c['null'], c['keep'], KC.CS)
        want, cnt = KC.error_ref(x, c['K'], c['mask'])
        args = (g(c['cond']), None if c['null'] is None else g(c['null']), None if c['keep'] is None else g(c['keep']), KC.CS,
                g(c['K']), g(c['mask']))
        ws = ops.known_error_workspace(args[0])
        assert ws.dtype == torch.float64 and ws.numel() == 2 * B * ops.known_error_splits(B, n)
        got = ops.known_error(*args, ws=ws)
        again = ops.known_error(*args)
        assert got.dtype == torch.float64 and tuple(got.shape) == (B,)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64)), name       # two calls, the same bits
        got = got.cpu()
        for b in range(B):
            if cnt[b] == 0:
                assert float(got[b]) == 0., (name, b)        # nothing kept: exactly 0
            else:
                ulps = abs(float(got[b]) - float(want[b])) / (2. ** -53 * float(want[b]))
                worst = max(worst, ulps / error_gate(cnt[b]))
                assert ulps <= error_gate(cnt[b]), (name, b, float(got[b]), float(want[b]), ulps)
    print(f'[parity] known error {B} x {n}: largest |E - exact| / gate = {worst:.3f}')


def test_wrapper_errors():
    from dmhomo_amd import _lib, ops
    x = torch.zeros((2, 6, 4, 4), device=dev())
    K = torch.zeros_like(x)
    m = torch.zeros((2, 96), device=dev(), dtype=torch.uint8)
    keep = torch.ones(2, dtype=torch.uint8, device=dev())
    for args in ((x, x[:1].clone(), None, 3., K, m), (x, None, None, 1., K[:, :3].contiguous(), m), (x, None, None, 1., K, m[:1].clone()),
                 (x, None, None, 1., K, m.float()), (x, None, keep, 1., K, m), (x, x.clone(), keep[:1], 3., K, m),
                 (x, None, None, float('nan'), K, m)):
        with pytest.raises(ValueError):
            ops.known_blend(*args)
    for out in (K, x[:1].clone()):
        with pytest.raises(ValueError):
            ops.known_blend(x, None, None, 1., K, m, out=out)
    null = x.clone()
    with pytest.raises(ValueError):
        ops.known_blend(x, null, None, 3., K, m, out=null)
    with pytest.raises(_lib.DmhError, match='in part'):
        buf = torch.zeros(2 * 96 + 8, device=dev())
        ops.known_blend(buf[:192].view(2, 96), None, None, 1., K.view(2, 96), m, out=buf[4:196].view(2, 96))
    with pytest.raises(ValueError):
        ops.known_error(x, None, None, 1., K, m, ws=torch.zeros(1, dtype=torch.float64, device=dev()))
    with pytest.raises(ValueError):
        ops.known_error(x, None, None, 1., K, m, out=torch.zeros(3, dtype=torch.float64, device=dev()))
    with pytest.raises(ValueError):
        ops.known_error_splits(0, 5)


# --------------------------------------------------------------------------------------------- 2. the sampler
T_, S_, B_, SIZE = 100, 5, 3, 16
SHAPE = (B_, 6, SIZE, SIZE)
# Gates of the loop parity: 10x the worst error measured on MI355X against the float64 loop.  Measured over ddim at
# known_resample 1 and 3 and dpmpp_2m at 1, cond_scale 3: per-entry x_start 0 — under pred_x0 it is the clamp of the fp32 logits,
# resp. K itself, and the float64 loop takes those fp32 values as given: the gate is equality —, image 3.76e-7 (the numbers per
# run are in the docstring of test_loops_vs_float64_loop); with photo_guidance = 0.5 on top, where the correction is fp32
# arithmetic of its own: x_start 8.98e-8, image 3.76e-7.
GATE_X0, GATE_IMG = 0., 3.8e-6
GATE_PHOTO_X0, GATE_PHOTO_IMG = 9.0e-7, 3.8e-6


def _known_pair(seed=31):
    """a pair in [0, 1] whose source half holds every value n / 255 (three times over per sample)"""
    gen = torch.Generator().manual_seed(seed)
    known = torch.rand(SHAPE, generator=gen)
    known[:, :3] = KC.all_bytes().repeat(3 * B_).reshape(B_, 3, SIZE, SIZE)
    return known


@pytest.fixture(scope='module')
def tiny():
    m, _ = _cfg_model()
    return m


def _diffusion(m, **attrs):
    from dmhomo_amd import cfg
    m.cfg_mode, m.dedup_dropped_rows = 'batched', False
    d = _cfg_diffusion(m, size=SIZE, T=T_, S=S_)
    d.rng = cfg.DeviceRng()
    for k, v in attrs.items():
        setattr(d, k, v)
    return d


def _runner(d, seed=5, first_id=40):
    def run(ins, known=None, kmask=None, **kw):
        c, rf01, fl, mk = ins
        d.rng.key_by_sample(seed, range(first_id, first_id + c.shape[0]), dev())
        if known is None:
            return d.sample(c, rf01, fl, mk, **kw)[0].clone()
        return d.sample_known(known, kmask, c, rf01, fl, mk, **kw)[0].clone()
    return run


def _ins(seed=9):
    return tuple(g(t) for t in _cond_inputs(B_, SIZE, seed=seed))


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_nothing_kept_is_sample_bit_for_bit(tiny, sampler):
    """an all-zero mask: the samples of sample(), eager and captured, and the generator left where sample() leaves it"""
    d = _diffusion(tiny, sampler=sampler)
    run, ins, known = _runner(d), _ins(), g(_known_pair())
    zero = torch.zeros(SHAPE, device=dev())
    want = run(ins)
    state = d.rng.state.clone()
    for graph in (False, True):
        d.hip_graph = graph
        for _ in range(2):                                    # (the capturing call, then a replay)
            assert torch.equal(run(ins, known, zero), want), (graph,)
            assert torch.equal(d.rng.state, state)
        assert torch.equal(run(ins), want)
    d.hip_graph = False
    d.rng.unkey()                                             # torch's generator: the same draws as well
    torch.manual_seed(3)
    a = d.sample(*ins)[0]
    after = torch.cuda.get_rng_state(dev())
    torch.manual_seed(3)
    b = d.sample_known(known, 0, *ins)[0]
    assert torch.equal(a, b) and torch.equal(torch.cuda.get_rng_state(dev()), after)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'captured'])
def test_source_is_kept_bit_for_bit_and_so_are_its_bytes(tiny, graph):
    from dmhomo_amd import ddpm
    d = _diffusion(tiny, hip_graph=graph)
    run, ins = _runner(d), _ins()
    known = g(_known_pair())
    free = run(ins, known, torch.zeros(SHAPE, device=dev()))
    img = run(ins, known, 'source')
    assert same(img[:, :3], known[:, :3])
    record = ddpm.saveTrainPair(img, ins[3], ins[2])['imgs']
    assert record.dtype.name == 'uint8' and record.shape == SHAPE
    want = torch.arange(256, dtype=torch.uint8).repeat(B_, 3).reshape(B_, 3, SIZE, SIZE).numpy()
    assert (record[:, :3] == want).all()                      # every byte value n / 255 comes back as n
    assert not torch.equal(img[:, 3:], free[:, 3:])           # the target is generated around the source
    assert bool(((img >= 0.) & (img <= 1.)).all())
    tgt = run(ins, known, 'target')
    assert same(tgt[:, 3:], known[:, 3:]) and not torch.equal(tgt[:, :3], free[:, :3])
    one = torch.zeros(SHAPE, device=dev())
    one[1, 4, 7, 9] = 1.
    pix = run(ins, known, one)
    assert float(pix[1, 4, 7, 9]) == float(known[1, 4, 7, 9]) and not torch.equal(pix, free)


def _float64_parity(d, ins, known, kmask, sampler, cs, monkeypatch, correct=None):
    """the eager loop with its network outputs and draws recorded, against the float64 loop on the same -> (trace, reference,
    max|x_start - float64|, max|img - float64|, the returned image, K, mask)"""
    from dmhomo_amd import ops
    nets, draws = _recording(d, monkeypatch)
    c, rf01, fl, mk = ins
    kn = d._known_inputs(known, kmask, SHAPE)
    torch.manual_seed(11)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, SHAPE, cs, trace=trace, known=kn)
    steps = d._sampler_steps(True, cs, kn['stays'])
    assert len(trace) == len(nets) == len(steps) == (kn['stays'] + 1) * S_
    assert len(draws) == 1 + sum(dr for _, _, dr in steps)
    K = ops.affine(kn['known'], 2., -1.).cpu()                # (the fp32 values the loop keeps, taken as given)
    mask = kn['mask'].cpu().reshape(SHAPE)
    ref = KC.reference_loop(steps, nets, draws, K, mask, cs, correct)
    ex = max(float((e['x_start'].cpu().double() - r[1]).abs().max()) for e, r in zip(trace, ref))
    ei = max(float((e['img'].cpu().double() - r[2]).abs().max()) for e, r in zip(trace, ref))
    return trace, ref, ex, ei, got, K, mask, kn


@pytest.mark.parametrize('sampler, r', [('ddim', 1), ('ddim', 3), ('dpmpp_2m', 1)])
def test_loops_vs_float64_loop(tiny, sampler, r, monkeypatch):
    """measured on MI355X: max|img - float64| = 3.76e-7 (ddim, r = 1), 3.28e-7 (ddim, r = 3), 3.29e-7 (dpmpp_2m); x_start equal to
    the float64 loop's in all three (gates 10x the largest: GATE_IMG; GATE_X0 is equality)"""
    from dmhomo_amd import ops
    d = _diffusion(tiny, sampler=sampler, known_resample=r)
    known = g(_known_pair())
    trace, ref, ex, ei, got, K, mask, kn = _float64_parity(d, _ins(), known, 'source', sampler, 3., monkeypatch)
    print(f'[parity] known {sampler} r = {r}: max|x_start - float64| = {ex:.2e} (gate {GATE_X0:.1e}), max|img - float64| = {ei:.2e} '
          f'(gate {GATE_IMG:.1e})')
    assert ex <= GATE_X0 and ei <= GATE_IMG, (ex, ei)
    for e in trace:                                           # x_start on a kept element is K itself at every entry
        assert same(e['x_start'].cpu()[:, :3], K[:, :3])
    assert [bool(e.get('stay')) for e in trace] == [k % r != r - 1 for k in range(r * S_)]
    assert sum(bool(e.get('stay')) for e in trace) == (r - 1) * S_
    want = ops.affine(trace[-1]['img'], 0.5, 0.5)
    assert torch.equal(got[:, 3:], want[:, 3:]) and same(got[:, :3], known[:, :3])
    # the score of every entry is the exact score of the logits the float64 loop saw (fp32 values, taken as given)
    for e, rr in zip(trace, ref):
        exact, cnt = KC.error_ref(rr[0], K, mask)
        err = e['known_err'].cpu()
        assert err.dtype == torch.float64 and tuple(err.shape) == (B_,)
        for b in range(B_):
            assert abs(float(err[b]) - float(exact[b])) <= error_gate(cnt[b]) * 2. ** -53 * float(exact[b]), (e['time'], b)


@pytest.mark.parametrize('sampler, r', [('ddim', 1), ('ddim', 3), ('dpmpp_2m', 1)])
def test_captured_equals_eager_in_every_mode(tiny, sampler, r):
    """bitwise: hip_graph against the eager loop under 'batched' and 'streams', dedup_dropped_rows on and off"""
    d = _diffusion(tiny, sampler=sampler, known_resample=r)
    run, ins, known = _runner(d), _ins(), g(_known_pair())
    want = run(ins, known, 'source')
    for mode in ('batched', 'streams'):
        for dedup in (False, True):
            tiny.cfg_mode, tiny.dedup_dropped_rows = mode, dedup
            d.hip_graph = False
            assert torch.equal(run(ins, known, 'source'), want), (mode, dedup, 'eager')
            d.hip_graph = True
            assert torch.equal(run(ins, known, 'source'), want), (mode, dedup, 'captured')
            assert torch.equal(run(ins, known, 'source'), want), (mode, dedup, 'replayed')
    d.hip_graph, tiny.dedup_dropped_rows, tiny.cfg_mode = False, False, 'batched'
    if r > 1:
        d.known_resample = 1
        assert not torch.equal(run(ins, known, 'source'), want)


def test_capture_counts(tiny):
    """the pixels and the mask are no part of a capture: another source and mask replay it; known_resample and score_known are;
    sample() keeps its own"""
    d = _diffusion(tiny)
    run, ins = _runner(d), _ins()
    known_a, known_b = g(_known_pair(31)), g(_known_pair(32))
    pix = torch.zeros((B_, 1, SIZE, SIZE), device=dev())
    pix[:, :, 3:9, 2:] = 1.
    eager = [run(ins, known_a, 'source'), run(ins, known_b, 'target'), run(ins, known_b, pix), run(ins)]
    assert not torch.equal(eager[1], eager[2])
    d.known_resample = 2
    eager_r2 = run(ins, known_a, 'source')
    d.known_resample = 1
    d.hip_graph = True
    assert torch.equal(run(ins), eager[3]) and d.graph_captures == 1
    assert torch.equal(run(ins, known_a, 'source'), eager[0]) and d.graph_captures == 2
    assert torch.equal(run(ins, known_b, 'target'), eager[1]) and d.graph_captures == 2
    assert torch.equal(run(ins, known_b, pix), eager[2]) and d.graph_captures == 2
    assert torch.equal(run(ins, known_a, 'source'), eager[0]) and d.graph_captures == 2
    assert torch.equal(run(ins), eager[3]) and d.graph_captures == 2             # sample() still hits its own capture
    d.known_resample = 2
    assert torch.equal(run(ins, known_a, 'source'), eager_r2) and d.graph_captures == 3
    d.known_resample, d.score_known = 1, True
    assert torch.equal(run(ins, known_a, 'source'), eager[0]) and d.graph_captures == 4
    score = d.last_known_error.clone()
    d.score_known = False
    assert torch.equal(run(ins, known_a, 'source'), eager[0]) and d.graph_captures == 4
    d.hip_graph, d.score_known = False, True
    run(ins, known_a, 'source')
    assert torch.equal(d.last_known_error.view(torch.int64), score.view(torch.int64))       # the captured score is the eager one


PHOTO_W, PHOTO_SEED = 0.5, 9
# (PHOTO_SEED: the seed of the conditions, the default of _cond_inputs.  It was checked on the GPU that at this seed the float64
#  loop ALONE — fed the recorded network outputs of the run with and of the run without photo guidance — shows the photometric
#  energy of every sample's result drop (the figures are in the test's docstring); the assertion on the kernels' own images is
#  made at that seed.)


def test_photo_guidance_on_top(tiny, monkeypatch):
    """correction first, overwrite behind it.  Measured on MI355X: per-entry max|x_start - float64| = 8.98e-8, max|img - float64|
    = 3.76e-7 (gates 10x that: GATE_PHOTO_X0 / GATE_PHOTO_IMG); photometric error of the three results 0.130, 0.150, 0.129 without
    and 0.120, 0.133, 0.115 with photo guidance; on the float64 loops 0.146, 0.145, 0.149 and 0.125, 0.126, 0.129"""
    from dmhomo_amd import ddpm
    ins = _ins(PHOTO_SEED)
    c, rf01, fl, mk = ins
    known = g(_known_pair())
    d = _diffusion(tiny)
    run = _runner(d)
    off = run(ins, known, 'source')
    d.photo_guidance = PHOTO_W
    on = run(ins, known, 'source')
    assert same(on[:, :3], known[:, :3]) and not torch.equal(on, off)
    d.hip_graph = True
    assert torch.equal(run(ins, known, 'source'), on) and torch.equal(run(ins, known, 'source'), on)
    d.hip_graph = False
    e_on, e_off = ddpm.photometric_error(on, fl, mk).cpu(), ddpm.photometric_error(off, fl, mk).cpu()
    print(f'[known] photometric error of the result, photo guidance off -> on: {e_off.tolist()} -> {e_on.tolist()}')
    assert bool((e_on <= e_off).all()), (e_on, e_off)
    # against the float64 loop, and the drop on the float64 loop alone
    mats = PC.matrices(fl.cpu())
    flc, mkc = fl.cpu(), mk.cpu()
    correct = lambda step, x: PC.guide_ref(x, flc, mkc, PC.lam32(PHOTO_W, step.sqrt_ac), mats=mats)
    d2 = _diffusion(tiny, photo_guidance=PHOTO_W)
    trace, ref, ex, ei, got, K, mask, kn = _float64_parity(d2, ins, known, 'source', 'ddim', 3., monkeypatch, correct)
    print(f'[parity] known + photo: max|x_start - float64| = {ex:.2e} (gate {GATE_PHOTO_X0:.1e}), max|img - float64| = {ei:.2e} '
          f'(gate {GATE_PHOTO_IMG:.1e})')
    assert ex <= GATE_PHOTO_X0 and ei <= GATE_PHOTO_IMG, (ex, ei)
    d3 = _diffusion(tiny)
    _, ref_off, _, _, _, _, _, _ = _float64_parity(d3, ins, known, 'source', 'ddim', 3., monkeypatch)
    final = lambda rr: KC.select(rr[-1][2] * 0.5 + 0.5, known.cpu().double(), mask)
    r_on, r_off = (PC.energy_ref(final(rr), flc, mkc, mats) for rr in (ref, ref_off))
    print(f'[known] the same on the float64 loops: {r_off.tolist()} -> {r_on.tolist()}')
    assert bool((r_on < r_off).all()), (r_on, r_off)


@pytest.mark.parametrize('switch, value', [('pag_scale', 2.), ('flow_guidance', 2.)])
def test_extra_pass_guidance_on_top(tiny, switch, value):
    d = _diffusion(tiny)
    run, ins, known = _runner(d), _ins(), g(_known_pair())
    plain = run(ins, known, 'source')
    setattr(d, switch, value)
    on = run(ins, known, 'source')
    assert same(on[:, :3], known[:, :3]) and not torch.equal(on, plain)
    d.hip_graph = True
    assert torch.equal(run(ins, known, 'source'), on) and torch.equal(run(ins, known, 'source'), on)
    d.hip_graph = False


def test_score_is_the_exact_score_of_the_last_logits(tiny, monkeypatch):
    """last_known_error against the exact score of the recorded last entry's logits, within the bound of the header; 0 for a
    sample with nothing kept; without score_known nothing is left"""
    d = _diffusion(tiny, known_resample=2)
    nets, draws = _recording(d, monkeypatch)
    ins, known = _ins(), g(_known_pair())
    kmask = torch.zeros(SHAPE, device=dev())
    kmask[0, :3] = 1.
    kmask[2, :, 5:11] = 1.                                    # (sample 1 keeps nothing)
    torch.manual_seed(4)
    d.sample_known(known, kmask, *ins)
    assert not hasattr(d, 'last_known_error')
    d.score_known = True
    nets.clear()
    torch.manual_seed(4)
    d.sample_known(known, kmask, *ins)
    assert len(nets) == 2 * S_
    cond, null, keep = (None if t is None else t.cpu() for t in nets[-1])
    K = known.cpu() * 2. - 1.
    exact, cnt = KC.error_ref(KC.blend32(cond, null, keep, 3.), K, kmask.cpu())
    got = d.last_known_error.cpu()
    assert got.dtype == torch.float64 and cnt == [3 * 256, 0, 6 * 6 * 16] and float(got[1]) == 0.
    for b in (0, 2):
        assert abs(float(got[b]) - float(exact[b])) <= error_gate(cnt[b]) * 2. ** -53 * float(exact[b]), (b, got, exact)
    assert float(got[0]) > 0.


def test_trainer_keeps_the_source_of_its_batches(tiny):
    from dmhomo_amd import ddpm
    d = _diffusion(tiny)
    data, classes = next(ddpm.SyntheticConditions(SIZE, B_, seed=1000))
    data = data.clone()
    data[:, :6] = g(_known_pair())
    tr = ddpm.Trainer(d, [(data, classes), (data, classes)], train_batch_size=B_)
    tr.keep, tr.score_known = 'source', True
    ret = tr.sample(0, 0)
    want = torch.arange(256, dtype=torch.uint8).repeat(B_, 3).reshape(B_, 3, SIZE, SIZE).numpy()
    assert ret['imgs'].shape == SHAPE and (ret['imgs'][:, :3] == want).all() and ret['homos'].shape == (B_, 3, 3)
    assert tr.last_known_error.shape == (B_,) and tr.last_known_error.dtype == torch.float64
    assert tr.ema.ema_model.score_known is False              # (the sampler's own switch is put back)
    tr.keep = 'both'
    with pytest.raises(ValueError, match='keep'):
        tr.sample(0, 0)


@pytest.mark.parametrize('setting, value', [('objective', 'pred_v'), ('clip_mode', 'dynamic'), ('guidance_rescale', 0.7),
                                            ('known_resample', 0), ('known_resample', 2.)])
def test_refusals_raise_in_sample_known(tiny, setting, value):
    d = _diffusion(tiny)
    setattr(d, setting, value)
    run, ins, known = _runner(d), _ins(), g(_known_pair())
    for graph in (False, True):
        d.hip_graph = graph
        with pytest.raises(ValueError, match=setting):
            run(ins, known, 'source')
    d.hip_graph = False


def test_resampling_with_the_multistep_solver_and_bad_pixels_are_refused(tiny):
    d = _diffusion(tiny, sampler='dpmpp_2m', known_resample=2)
    run, ins, known = _runner(d), _ins(), g(_known_pair())
    with pytest.raises(ValueError, match='dpmpp_2m'):
        run(ins, known, 'source')
    d.known_resample = 1
    bad = known.clone()
    bad[0, 0, 0, 0] = 1.5
    for k in (bad, known[:, :3].contiguous(), known[:2].contiguous()):
        with pytest.raises(ValueError, match='known'):
            run(ins, k, 'source')
    with pytest.raises(ValueError, match='known_mask'):
        run(ins, known, 'left')
