"""-m gpu: starting the sampler from a given pair (cfg.GaussianDiffusion.sample_from): the kernel (dmh_start_mix) and the
conditional sampler started at a later entry of its time list, eager and captured.

1. dmh_start_mix alone, into NaN-guarded buffers at every 16-byte phase of out, init and noise, bitwise against the statement
   of tests/start_cases.py; the keyed arm's draw is dmh_rng_indexed's own and leaves the generator where that launch would;
2. the sampler: the start image is q_sample(affine(init), t*, eps) fed to the loop, the eager loops against a float64 loop fed
   the same network outputs (the gates of tests/test_gpu_known.py: the update kernels are the same ones), captured == eager,
   capture counts, the generator state, kept pixels with ``known``, every guidance switch on top, dedup on == off, 'batched' ==
   'streams', Trainer.strength, the refusals."""
import pytest
import torch

import known_cases as KC
import start_cases as SC
from dmhomo_amd.schedule import ddim_pairs
from gpu_util import dev
from test_gpu_guidance import _recording, g, same
from test_gpu_known import GATE_IMG, GATE_X0, _known_pair, _place, _untouched
from test_gpu_solver import _cfg_diffusion, _cfg_model, _cond_inputs

pytestmark = pytest.mark.gpu

CA, CB = 0.62341517, 0.78189385                               # (any finite pair: the kernel takes them as given)
SEED, DRAW = 0x1234567890, 7


# --------------------------------------------------------------------------------------------- 1. the kernel alone
def _state(draw=DRAW, seed=SEED):
    return torch.tensor([seed, draw, 0, 0], dtype=torch.int64, device=dev())


def _ids(B, first=10):
    return torch.arange(first, first + B, dtype=torch.int64, device=dev())


@pytest.fixture(scope='module')
def kernel_cases():
    """per shape: init, noise, the keyed generator's own draw (ops.rng_indexed from an identically keyed state) and the statement
    for both noise sources, computed once and left unchanged"""
    from dmhomo_amd import ops
    out = {}
    for i, (B, per) in enumerate(SC.SHAPES):
        init, noise = SC.kernel_inputs(B, per, 100 + i)
        eps = ops.rng_indexed((B, per), _ids(B), _state(), 0).cpu()
        out[(B, per)] = {'init': g(init), 'noise': g(noise), 'want_keyed': g(SC.mix32(init, eps, CA, CB)),
                         'want_given': g(SC.mix32(init, noise, CA, CB))}
    return out


@pytest.mark.parametrize('B, per', SC.SHAPES)
def test_keyed_arm_is_the_statement_on_the_generators_own_draw(kernel_cases, B, per):
    from dmhomo_amd import ops
    c = kernel_cases[(B, per)]
    ids = _ids(B)
    assert not same(c['want_keyed'], c['want_given'])
    for off_out in SC.OFFSETS:
        for off_in in SC.OFFSETS:
            what = (B, per, off_out, off_in)
            init, ibuf, ilo = _place(c['init'], off_in)
            out, obuf, olo = _place(torch.full((B, per), 777.), off_out)
            state = _state()
            got = ops.start_mix(init, CA, CB, sample_ids=ids, state=state, out=out)
            assert got is out and same(out, c['want_keyed']), what
            assert _untouched(obuf, olo, out.numel()) and same(init, c['init']), what             # guards and the input stay
            assert state.tolist() == [SEED, DRAW + 1, 0, 0], what
    fresh = ops.start_mix(c['init'], CA, CB, sample_ids=ids, state=_state())                   # out None: a new tensor
    assert same(fresh, c['want_keyed'])


@pytest.mark.parametrize('B, per', SC.SHAPES)
def test_given_noise_arm_is_the_statement(kernel_cases, B, per):
    from dmhomo_amd import ops
    c = kernel_cases[(B, per)]
    launches = 0
    for off_out in SC.OFFSETS:
        for off_in in SC.OFFSETS:
            init, _, _ = _place(c['init'], off_in)
            for off_n in SC.OFFSETS:
                what = (B, per, off_out, off_in, off_n)
                noise, _, _ = _place(c['noise'], off_n)
                out, obuf, olo = _place(torch.full((B, per), 777.), off_out)
                got = ops.start_mix(init, CA, CB, noise=noise, out=out)
                launches += 1
                assert got is out and same(out, c['want_given']), what
                assert _untouched(obuf, olo, out.numel()), what
                assert same(noise, c['noise']) and same(init, c['init']), what
            # in place: out == noise (its guards are the output's)
            noise, nbuf, nlo = _place(c['noise'], off_out)
            got = ops.start_mix(init, CA, CB, noise=noise, out=noise)
            launches += 1
            assert got is noise and same(noise, c['want_given']), (B, per, off_out, off_in, 'in place')
            assert _untouched(nbuf, nlo, noise.numel()) and same(init, c['init'])
    assert launches == 4 * 4 * 5


def test_keyed_arm_advances_the_draw_like_rng_indexed():
    """two launches in a row give the draws d and d + 1; alternating with ops.rng_indexed keeps one stream"""
    from dmhomo_amd import ops
    for B, per in ((3, 210), (3, 1536), (64, 16388)):
        ids = _ids(B)
        init = g(SC.kernel_inputs(B, per, 5)[0])
        ref_state = _state()
        draws = [ops.rng_indexed((B, per), ids, ref_state, 0).cpu() for _ in range(4)]          # draws d .. d + 3
        assert ref_state.tolist() == [SEED, DRAW + 4, 0, 0] and not same(draws[0], draws[1])
        state = _state()
        a = ops.start_mix(init, CA, CB, sample_ids=ids, state=state)
        b = ops.start_mix(init, CA, CB, sample_ids=ids, state=state)
        assert state.tolist() == [SEED, DRAW + 2, 0, 0]
        assert same(a.cpu(), SC.mix32(init.cpu(), draws[0], CA, CB)) and same(b.cpu(), SC.mix32(init.cpu(), draws[1], CA, CB))
        state = _state()
        a = ops.start_mix(init, CA, CB, sample_ids=ids, state=state)
        r1 = ops.rng_indexed((B, per), ids, state, 0)
        c = ops.start_mix(init, CA, CB, sample_ids=ids, state=state)
        r3 = ops.rng_indexed((B, per), ids, state, 0)
        assert state.tolist() == [SEED, DRAW + 4, 0, 0]
        assert same(r1.cpu(), draws[1]) and same(r3.cpu(), draws[3])
        assert same(a.cpu(), SC.mix32(init.cpu(), draws[0], CA, CB)) and same(c.cpu(), SC.mix32(init.cpu(), draws[2], CA, CB))


def test_rows_of_a_shard_are_the_rows_of_the_whole_batch():
    from dmhomo_amd import ops
    for per in (210, 1536):
        init = g(SC.kernel_inputs(4, per, 6)[0])
        whole = ops.start_mix(init, CA, CB, sample_ids=_ids(4, 10), state=_state())
        lo = ops.start_mix(init[:2].contiguous(), CA, CB, sample_ids=_ids(2, 10), state=_state())
        hi = ops.start_mix(init[2:].contiguous(), CA, CB, sample_ids=_ids(2, 12), state=_state())
        assert same(whole[:2], lo) and same(whole[2:], hi) and not same(lo, hi)


def test_wrapper_errors():
    from dmhomo_amd import _lib, ops
    x = torch.rand((2, 96), device=dev())
    ids, state = _ids(2), _state()
    with pytest.raises(_lib.DmhError, match='no noise source'):
        ops.start_mix(x, CA, CB)
    with pytest.raises(_lib.DmhError, match='two noise sources'):
        ops.start_mix(x, CA, CB, noise=torch.zeros_like(x), sample_ids=ids, state=state)
    with pytest.raises(_lib.DmhError, match='finite'):
        ops.start_mix(x, float('nan'), CB, noise=torch.zeros_like(x))
    with pytest.raises(_lib.DmhError, match='out overlaps init01'):
        ops.start_mix(x, CA, CB, noise=torch.zeros_like(x), out=x)
    with pytest.raises(_lib.DmhError, match='in part'):
        buf = torch.zeros(2 * 96 + 8, device=dev())
        ops.start_mix(x, CA, CB, noise=buf[:192].view(2, 96), out=buf[4:196].view(2, 96))
    for bad in (dict(noise=torch.zeros((2, 95), device=dev())), dict(noise=torch.zeros_like(x), out=torch.zeros((1, 96), device=dev())),
                dict(sample_ids=_ids(3), state=state), dict(sample_ids=ids, state=torch.zeros(3, dtype=torch.int64, device=dev()))):
        with pytest.raises(ValueError, match='start_mix'):
            ops.start_mix(x, CA, CB, **bad)
    assert state.tolist() == [SEED, DRAW, 0, 0]               # nothing was launched


# --------------------------------------------------------------------------------------------- 2. the sampler
T_, S_, B_, SIZE = 100, 5, 3, 16
SHAPE = (B_, 6, SIZE, SIZE)
PAIRS = ddim_pairs(T_, S_)
STRENGTHS = ((0.2, 4), (0.6, 2), (1.0, 0))                   # (strength, k0)


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


def _ins(seed=9):
    return tuple(g(t) for t in _cond_inputs(B_, SIZE, seed=seed))


def _init(seed=77):
    return g(torch.rand(SHAPE, generator=torch.Generator().manual_seed(seed)))


def _runner(d, seed=5, first_id=40):
    def run(ins, init=None, strength=None, known=None, kmask=None, **kw):
        c, rf01, fl, mk = ins
        d.rng.key_by_sample(seed, range(first_id, first_id + c.shape[0]), dev())
        if init is None and known is None:
            return d.sample(c, rf01, fl, mk, **kw)[0].clone()
        if init is None:
            return d.sample_known(known, kmask, c, rf01, fl, mk, **kw)[0].clone()
        return d.sample_from(init, strength, c, rf01, fl, mk, known=known, known_mask=kmask, **kw)[0].clone()
    return run


def _first_inputs(d, monkeypatch):
    """the image every network call of d receives, recorded"""
    seen = []
    network = d._network

    def spy(x, *a):
        seen.append(x.clone())
        return network(x, *a)
    monkeypatch.setattr(d, '_network', spy)
    return seen


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
@pytest.mark.parametrize('strength, k0', STRENGTHS)
def test_start_image_is_q_sample_of_the_normalised_pair(tiny, sampler, strength, k0, monkeypatch):
    from dmhomo_amd import ops
    d = _diffusion(tiny, sampler=sampler)
    seen = _first_inputs(d, monkeypatch)
    c, rf01, fl, mk = ins = _ins()
    init = _init()
    t = PAIRS[k0][0]
    tt = torch.full((B_,), t, device=dev(), dtype=torch.long)
    st = d._start_inputs(init, strength, SHAPE)
    assert (st['k0'], st['t']) == (k0, t)
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    # keyed: eps is the draw an identically keyed generator hands out first
    d.rng.key_by_sample(5, range(40, 40 + B_), dev())
    eps = ops.rng_indexed(SHAPE, d.rng.sample_ids, d.rng.state.clone(), 0)
    trace = []
    loop(c, ops.affine(rf01, 2., -1.), fl, mk, SHAPE, 3., trace=trace, start=st)
    want = d.q_sample(ops.affine(init, 2., -1.), tt, eps)
    assert same(seen[0], want) and same(want.cpu(), SC.mix32(init.cpu(), eps.cpu(), st['ca'], st['cb']))
    assert [e['time'] for e in trace] == [tm for tm, _ in PAIRS[k0:]] and len(seen) == S_ - k0
    # the public call: the same image, the same entries, last_start
    seen.clear()
    d.rng.key_by_sample(5, range(40, 40 + B_), dev())
    d.sample_from(init, strength, *ins)
    assert same(seen[0], want) and len(seen) == S_ - k0 and d.last_start == (k0, t)
    # torch's stream generator: eps is the randn sample() would draw first
    d.rng.unkey()
    seen.clear()
    torch.manual_seed(3)
    eps = torch.randn(SHAPE, device=dev())
    torch.manual_seed(3)
    d.sample_from(init, strength, *ins)
    assert same(seen[0], d.q_sample(ops.affine(init, 2., -1.), tt, eps)) and len(seen) == S_ - k0


@pytest.mark.parametrize('eta', [0., 1.])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
@pytest.mark.parametrize('strength, k0', STRENGTHS)
def test_loops_vs_float64_loop(tiny, sampler, strength, k0, eta, monkeypatch):
    """the eager loop with its network outputs and draws recorded, against the float64 loop of tests/known_cases.py (nothing kept)
    on the same, begun at the start image (fp32, taken as given: the test above holds it bit for bit).  The gates are those of
    tests/test_gpu_known.py: x_start equal (under pred_x0 it is the clamp of the fp32 logits), image 3.8e-6.  Measured on MI355X:
    x_start equal in all twelve runs; max|img - float64| = 0 at strength 0.2 (one entry: the image is x_start), 2.40e-7 / 2.02e-7
    (ddim, eta 0 / 1) and 2.38e-7 (dpmpp_2m) at 0.6, 4.39e-7 / 2.54e-7 and 3.60e-7 at 1.0."""
    from dmhomo_amd import ops
    d = _diffusion(tiny, sampler=sampler, ddim_sampling_eta=eta)
    nets, draws = _recording(d, monkeypatch)
    c, rf01, fl, mk = _ins()
    init = _init()
    st = d._start_inputs(init, strength, SHAPE)
    torch.manual_seed(11)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    got, _, _ = loop(c, ops.affine(rf01, 2., -1.), fl, mk, SHAPE, 3., trace=trace, start=st)
    steps = d._sampler_steps(True, 3., 0, k0)
    assert len(trace) == len(nets) == len(steps) == S_ - k0
    assert len(draws) == 1 + sum(dr for _, _, dr in steps)
    x0 = SC.mix32(init.cpu(), draws[0].cpu(), st['ca'], st['cb'])
    zero = torch.zeros(SHAPE)
    ref = KC.reference_loop(steps, nets, [x0] + list(draws[1:]), zero, zero.to(torch.uint8), 3.)
    ex = max(float((e['x_start'].cpu().double() - r[1]).abs().max()) for e, r in zip(trace, ref))
    ei = max(float((e['img'].cpu().double() - r[2]).abs().max()) for e, r in zip(trace, ref))
    print(f'[parity] start {sampler} strength {strength} eta {eta}: max|x_start - float64| = {ex:.2e} (gate {GATE_X0:.1e}), '
          f'max|img - float64| = {ei:.2e} (gate {GATE_IMG:.1e})')
    assert ex <= GATE_X0 and ei <= GATE_IMG, (ex, ei)
    assert torch.equal(got, ops.affine(trace[-1]['img'], 0.5, 0.5))
    if sampler == 'dpmpp_2m' and len(steps) > 1:
        assert steps[0][1].c2 == 0.                           # the first entry that runs is first order


@pytest.mark.parametrize('keyed', [True, False], ids=['keyed', 'stream'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_captured_equals_eager(tiny, sampler, keyed):
    """bit for bit, the capturing call included, with both generators"""
    d = _diffusion(tiny, sampler=sampler)
    ins, init = _ins(), _init()
    if keyed:
        run = _runner(d)
    else:
        def run(ins, init=None, strength=None):
            torch.manual_seed(3)
            return (d.sample(*ins) if init is None else d.sample_from(init, strength, *ins))[0].clone()
    eager = {s: run(ins, init, s) for s, _ in STRENGTHS}
    plain = run(ins)
    assert len({tuple(v.flatten()[:8].tolist()) for v in eager.values()}) == 3 and not torch.equal(eager[1.0], plain)
    d.hip_graph = True
    for s, _ in STRENGTHS:
        assert torch.equal(run(ins, init, s), eager[s]), (s, 'the capturing call')
        assert torch.equal(run(ins, init, s), eager[s]), (s, 'replayed')
    assert torch.equal(run(ins), plain)
    assert torch.equal(run(ins, init, 0.6), eager[0.6])       # back again, behind sample()
    other = _init(78)
    d.hip_graph = False
    want = run(ins, other, 0.6)
    d.hip_graph = True
    assert torch.equal(run(ins, other, 0.6), want) and not torch.equal(want, eager[0.6])


def test_capture_counts(tiny):
    """under 'ddim' sample_from replays sample()'s capture whatever the strength; under 'dpmpp_2m' every distinct k0 > 0 is a
    capture of its own, k0 = 0 is sample()'s"""
    ins, init = _ins(), _init()
    d = _diffusion(tiny, hip_graph=True)
    run = _runner(d)
    run(ins)
    assert d.graph_captures == 1
    for s, _ in STRENGTHS:
        run(ins, init, s)
        run(ins, _init(79), s)
    assert d.graph_captures == 1
    d = _diffusion(tiny, hip_graph=True, sampler='dpmpp_2m')
    run = _runner(d)
    run(ins)
    assert d.graph_captures == 1
    for n, (s, k0) in enumerate(((1.0, 0), (0.6, 2), (0.6, 2), (0.7, 2), (0.2, 4), (0.6, 2))):
        run(ins, init, s)
        assert d.graph_captures == (1, 2, 2, 2, 3, 3)[n], (s, k0)


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_generator_is_left_where_sample_leaves_it_minus_the_skipped_entries(tiny, sampler, monkeypatch):
    d = _diffusion(tiny, sampler=sampler)
    ins, init = _ins(), _init()
    run = _runner(d)
    full = []
    network = d._network

    def spy(*a):
        full.append(int(d.rng.state[1]))                      # the draw index at the head of every entry
        return network(*a)
    with monkeypatch.context() as mp:                         # (the eager sample() only: a capture cannot read the device)
        mp.setattr(d, '_network', spy)
        run(ins)
    end = int(d.rng.state[1])
    assert len(full) == S_ and full[0] == 1                   # one initial draw in front of entry 0
    for strength, k0 in STRENGTHS:
        for graph in (False, True):
            d.hip_graph = graph
            run(ins, init, strength)
            assert d.rng.state.tolist() == [5, end - (full[k0] - full[0]), 0, 0], (strength, graph)
        d.hip_graph = False
    # torch's generator: at k0 = 0 exactly what sample() consumes
    d.rng.unkey()
    torch.manual_seed(3)
    d.sample(*ins)
    after = torch.cuda.get_rng_state(dev())
    torch.manual_seed(3)
    d.sample_from(init, 1., *ins)
    assert torch.equal(torch.cuda.get_rng_state(dev()), after)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'captured'])
def test_kept_pixels_come_back_and_the_rest_starts_from_init(tiny, graph):
    """with known: sample_known's loop (known_resample = 2 under 'ddim') started from the mixed image"""
    from dmhomo_amd import ddpm
    d = _diffusion(tiny, known_resample=2)
    run, ins = _runner(d), _ins()
    known = g(_known_pair())
    eager = run(ins, known, 0.6, known=known, kmask='source')
    from_noise = run(ins, known=known, kmask='source')
    d.hip_graph = graph
    img = run(ins, known, 0.6, known=known, kmask='source')
    assert torch.equal(img, eager)
    assert same(img[:, :3], known[:, :3])
    record = ddpm.saveTrainPair(img, ins[3], ins[2])['imgs']
    want = torch.arange(256, dtype=torch.uint8).repeat(B_, 3).reshape(B_, 3, SIZE, SIZE).numpy()
    assert (record[:, :3] == want).all()                      # every byte value n / 255 comes back as n
    assert not torch.equal(img[:, 3:], from_noise[:, 3:])     # the start did take effect
    assert not torch.equal(img[:, 3:], run(ins, _init(), 0.6, known=known, kmask='source')[:, 3:])      # ... and it is init's
    if graph:                                                 # sample_known's capture, replayed from entry k0 * 2 on
        caps = d.graph_captures
        assert torch.equal(run(ins, known=known, kmask='source'), from_noise) and d.graph_captures == caps
        assert torch.equal(run(ins, known, 0.2, known=known, kmask='source'), _eager(d, run, ins, known, 0.2)) and d.graph_captures == caps
    d.hip_graph = False


def _eager(d, run, ins, known, strength):
    d.hip_graph = False
    try:
        return run(ins, known, strength, known=known, kmask='source')
    finally:
        d.hip_graph = True


GUIDANCE = [dict(photo_guidance=0.5), dict(pag_scale=2.), dict(flow_guidance=2.), dict(apg_eta=0., apg_momentum=-0.5),
            dict(guidance_interval=(0., 0.3)), dict(clip_mode='dynamic'), dict(guidance_rescale=0.7)]


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
@pytest.mark.parametrize('switch', GUIDANCE, ids=lambda s: next(iter(s)))
def test_guidance_on_top(tiny, switch, sampler):
    """every per-step switch acts per entry and knows nothing of where the list starts: captured == eager, and it does act.  (The
    interval guides the last of the three entries that run at strength 0.6, times 59, 39, 19 of 99, and leaves two unguided.)"""
    d = _diffusion(tiny, sampler=sampler)
    run, ins, init = _runner(d), _ins(), _init()
    plain = run(ins, init, 0.6)
    for k, v in switch.items():
        setattr(d, k, v)
    on = run(ins, init, 0.6)
    assert not torch.equal(on, plain)
    d.hip_graph = True
    assert torch.equal(run(ins, init, 0.6), on) and torch.equal(run(ins, init, 0.6), on)
    assert torch.equal(run(ins, init, 0.6), on)
    d.hip_graph = False


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_dedup_and_streams_give_the_same_samples(tiny, sampler):
    d = _diffusion(tiny, sampler=sampler)
    run, ins, init = _runner(d), _ins(), _init()
    want = run(ins, init, 0.6)
    for mode in ('batched', 'streams'):
        for dedup in (False, True):
            tiny.cfg_mode, tiny.dedup_dropped_rows = mode, dedup
            for graph in (False, True):
                d.hip_graph = graph
                assert torch.equal(run(ins, init, 0.6), want), (mode, dedup, graph)
    d.hip_graph, tiny.dedup_dropped_rows, tiny.cfg_mode = False, False, 'batched'


def test_trainer_starts_from_its_batches(tiny):
    from dmhomo_amd import ddpm
    d = _diffusion(tiny)
    data, classes = next(ddpm.SyntheticConditions(SIZE, B_, seed=1000))
    data = data.clone()
    data[:, :6] = g(_known_pair())
    tr = ddpm.Trainer(d, [(data, classes)] * 6, train_batch_size=B_)
    sampler = tr.ema.ema_model
    assert tr.strength is None and sampler.last_start is None
    base = tr.sample(0, 0)
    assert sampler.last_start is None                         # off: sample(), as before
    tr.strength = 0.6
    ret = tr.sample(0, 0)
    assert sampler.last_start == (2, PAIRS[2][0])
    assert ret['imgs'].shape == SHAPE and ret['imgs'].dtype.name == 'uint8' and ret['homos'].shape == (B_, 3, 3)
    assert sorted(ret) == sorted(base)                        # the record format is unchanged
    tr.keep = 'source'
    ret = tr.sample(0, 0)
    want = torch.arange(256, dtype=torch.uint8).repeat(B_, 3).reshape(B_, 3, SIZE, SIZE).numpy()
    assert (ret['imgs'][:, :3] == want).all() and sampler.last_start == (2, PAIRS[2][0])
    tr.strength = 0.1
    with pytest.raises(ValueError, match='smallest strength'):
        tr.sample(0, 0)


def test_refusals_raise_in_sample_from(tiny):
    d = _diffusion(tiny)
    run, ins, init = _runner(d), _ins(), _init()
    for graph in (False, True):
        d.hip_graph = graph
        for bad in (0., 1.5, float('nan'), None):
            with pytest.raises(ValueError, match='strength'):
                run(ins, init, bad)
        with pytest.raises(ValueError, match=r'smallest strength.*1 / 5'):
            run(ins, init, 0.19)
        x = init.clone()
        x[0, 0, 0, 0] = 1.5
        for k in (x, init[:, :3].contiguous(), init[:2].contiguous()):
            with pytest.raises(ValueError, match='init'):
                run(ins, k, 0.6)
        with pytest.raises(ValueError, match='known and known_mask'):
            d.sample_from(init, 0.6, *ins, known=init)
        d.clip_mode = 'dynamic'
        with pytest.raises(ValueError, match='clip_mode'):
            run(ins, init, 0.6, known=init, kmask='source')
        d.clip_mode = 'static'
    d.hip_graph = False
    assert d.graph_captures == 0                              # every refusal came before a capture
