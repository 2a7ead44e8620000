"""CPU: the host side of guidance rescale (``guidance_rescale``): the switch and its check, the unconditional class's refusal,
the loops' dispatch (phi = 0 or cond_scale == 1 makes none of the new calls), the capture key, the case list and float64
reference of tests/guidance_cases.py, and the argument validation of the new entry points."""
import ctypes

import pytest
import torch

import guidance_cases as GC

NEW_OPS = ('guidance_workspace', 'guidance_factor', 'guidance_factor_dev', 'sampler_threshold_gr', 'sampler_threshold_gr_dev',
           'sampler_step_gr', 'sampler_step_gr_dev')
NEW_ENTRY_POINTS = ('dmh_guidance_splits', 'dmh_guidance_factor', 'dmh_guidance_factor_dev', 'dmh_sampler_threshold_gr',
                    'dmh_sampler_threshold_gr_dev', 'dmh_sampler_step_gr', 'dmh_sampler_step_gr_dev')


def _host():
    from dmhomo_amd.sampling import ScheduleHost

    class H(ScheduleHost):
        pass
    return H()


def test_default_is_off_and_the_check_accepts_and_refuses():
    h = _host()
    assert h.guidance_rescale == 0. and h._check_guidance_rescale() == 0.
    for phi in (0, 0., 0.7, 1, 1., 1e-9):
        h.guidance_rescale = phi
        assert h._check_guidance_rescale() == float(phi)
    for phi in (-0.1, 1.0000001, 2, float('nan'), float('inf'), None, '0.7', True, [0.7]):
        h.guidance_rescale = phi
        with pytest.raises(ValueError, match='guidance_rescale'):
            h._check_guidance_rescale()


def test_unconditional_class_refuses_a_non_zero_value():
    from dmhomo_amd import ddpm
    m = ddpm.Unet(dim=8, dim_mults=(1, 2), channels=3)
    d = ddpm.GaussianDiffusion(m, image_size=16, timesteps=10, sampling_timesteps=4)
    d.guidance_rescale = 0.7
    with pytest.raises(ValueError, match='unconditional'):
        d.sample(batch_size=2)
    d.guidance_rescale = 3.
    with pytest.raises(ValueError, match='guidance_rescale'):
        d.sample(batch_size=2)


def _diffusion(S=4):
    from dmhomo_amd import cfg
    m = cfg.Unet(dim=8, dim_mults=(1, 2), channels=6, num_classes=1)
    return cfg.GaussianDiffusion(m, image_size=8, timesteps=20, sampling_timesteps=S, objective='pred_x0')


def _stub_loop(d, monkeypatch):
    """the eager loops with the network, the generator and every step-side ops function replaced by counting stand-ins ->
    the counter {ops name: calls}"""
    from dmhomo_amd import ops
    calls = {}

    def fake(name, result):
        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return result(*a, **k)
        monkeypatch.setattr(ops, name, f)

    def fake_network(x, t, classes, rgb_flow, mask, cs):
        return torch.zeros_like(x), (None if cs == 1 else torch.zeros_like(x)), None

    class Rng:
        def randn(self, shape, device):
            return torch.zeros(tuple(shape))
    x_of = lambda a: a[3]                                    # (step, cond, null, x, ...)
    fake('sampler_step', lambda *a, **k: (x_of(a).clone(), x_of(a).clone(), None))
    fake('sampler_step_ms', lambda *a, **k: (x_of(a).clone(), x_of(a).clone()))
    fake('sampler_threshold', lambda *a, **k: (torch.ones(x_of(a).shape[0]), None))
    fake('sampler_step_thr', lambda *a, **k: (x_of(a).clone(), x_of(a).clone()))
    fake('guidance_workspace', lambda x: torch.zeros(4, dtype=torch.float64))
    fake('guidance_factor', lambda step, cond, null, phi, **k: torch.ones(cond.shape[0]))
    fake('sampler_threshold_gr', lambda *a, **k: (torch.ones(x_of(a).shape[0]), None))
    fake('sampler_step_gr', lambda *a, **k: (x_of(a).clone(), x_of(a).clone()))
    monkeypatch.setattr(ops, 'affine', lambda x, a, b, out=None: x)
    monkeypatch.setattr(d, '_network', fake_network)
    d.rng = Rng()
    return calls


def _run_loop(d, sampler, cond_scale):
    B, S = 2, d.image_size
    shape = (B, d.channels, S, S)
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    trace = []
    loop(torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)), shape,
         cond_scale, trace=trace)
    return trace


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_take_the_new_path_only_with_phi_and_a_null_pass(sampler, clip_mode, monkeypatch):
    S = 4
    d = _diffusion(S)
    d.sampler, d.clip_mode = sampler, clip_mode
    calls = _stub_loop(d, monkeypatch)
    old_step = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler] if clip_mode == 'static' else 'sampler_step_thr'
    for phi, cond_scale in ((0., 3.), (0.7, 1.), (0.7, 1), (0., 1.)):       # today's calls, exactly
        calls.clear()
        d.guidance_rescale = phi
        trace = _run_loop(d, sampler, cond_scale)
        assert not any(name in calls for name in NEW_OPS), (phi, cond_scale, calls)
        assert calls[old_step] == S and all('gfac' not in e for e in trace)
        assert ('sampler_threshold' in calls) == (clip_mode == 'dynamic')
    for phi in (0.7, 1.):                                                    # the rescaled path: factor, threshold, step
        calls.clear()
        d.guidance_rescale = phi
        trace = _run_loop(d, sampler, 3.)
        assert calls == {'guidance_workspace': 1, 'guidance_factor': S, 'sampler_step_gr': S,
                         **({'sampler_threshold_gr': S} if clip_mode == 'dynamic' else {})}, calls
        assert len(trace) == S and all(e['gfac'].shape == (2,) for e in trace)
        assert all(('thr' in e) == (clip_mode == 'dynamic') for e in trace)
    d.guidance_rescale = 1.5
    with pytest.raises(ValueError, match='guidance_rescale'):
        _run_loop(d, sampler, 3.)


def test_capture_key_carries_phi(monkeypatch):
    d = _diffusion()
    keys = []

    def fake_replay(shape, device, key, tables, buffers, fill):
        keys.append(tuple(key))
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    B, S = 2, d.image_size
    args = (torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)),
            (B, d.channels, S, S), 3.)
    for phi in (0., 0.7, 1., 0.7):
        d.guidance_rescale = phi
        d._sample_graphed(*args)
    assert keys[1] == keys[3] and len({keys[0], keys[1], keys[2]}) == 3
    assert keys[0][-1] == 0. and keys[1][-1] == 0.7 and keys[0][:-1] == keys[1][:-1]    # phi is all that differs
    d.guidance_rescale = -1.
    with pytest.raises(ValueError, match='guidance_rescale'):
        d._sample_graphed(*args)


# ------------------------------------------------------------------------------------------ the case list and its reference
def _restated_splits(B, n):
    """dmh_guidance_splits as guidance.hip states it: one workgroup per 4096 elements of a row, at most 1024 in all"""
    return min((n + 4095) // 4096, max(1024 // B, 1))


def test_splits_agree_with_the_restatement_and_cut_the_workload_row():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for B in (1, 3, 25, 300, 5000):
        for n in GC.SIZES + GC.RAGGED_CANDIDATES[:8] + (98304, 393216, 2 ** 31 - 1):
            assert lib.dmh_guidance_splits(B, n) == _restated_splits(B, n) == ops.guidance_splits(B, n), (B, n)
    assert lib.dmh_guidance_splits(25, 98304) == 24          # 600 workgroups on 256 CUs, not 25
    for B, n in ((0, 4), (-1, 4), (1, 0), (1, 2 ** 31)):
        assert lib.dmh_guidance_splits(B, n) == -1 and lib.dmh_last_error(), (B, n)
        with pytest.raises(ValueError):
            ops.guidance_splits(B, n)
    for B in GC.BATCHES:
        n, s = GC.ragged_size(_restated_splits, B)
        assert s >= 2 and n % (4 * s) != 0 and n < GC.BIG[0]


def test_case_list_covers_what_it_claims():
    ragged = tuple(GC.ragged_size(_restated_splits, B)[0] for B in GC.BATCHES)
    cases = GC.factor_cases(ragged)
    seen = {}
    for name, c in cases:
        B, n = c['cond'].shape
        assert c['cond'].dtype == c['null'].dtype == torch.float32 and c['null'].shape == (B, n), name
        assert c['keep'] is None or (c['keep'].dtype == torch.uint8 and c['keep'].shape == (B,)), name
        seen.setdefault((n, B), set()).add(c['kind'])
    for n in GC.SIZES + ragged:
        for B in GC.BATCHES:
            assert seen[(n, B)] == set(GC.KINDS), (n, B)
    assert seen[GC.BIG] == {'normal'} and all('offset' in seen[(GC.BIG[0], B)] for B in GC.BATCHES)
    assert len(cases) == (len(GC.SIZES) + len(ragged)) * len(GC.BATCHES) * len(GC.KINDS) + 1 + len(GC.BATCHES)


def test_reference_on_the_exact_kinds():
    ragged = tuple(GC.ragged_size(_restated_splits, B)[0] for B in GC.BATCHES)
    checked = 0
    for name, c in GC.factor_cases(ragged):
        if c['cond'].shape[1] > 9600:
            continue
        g = GC.factor_ref(c['cond'], c['null'], c['keep'], c['cs'], c['phi'])
        if isinstance(c['expect'], float):                   # 'equal', 'keep0', 'pow2', 'const': exact in the reference too
            assert g.tolist() == [c['expect']] * g.shape[0], (name, g)
            checked += 1
        elif isinstance(c['expect'], tuple):
            row = c['expect'][1]
            clean = GC.factor_ref(c['clean']['cond'], c['clean']['null'], None, c['cs'], c['phi'])
            assert bool(torch.isnan(g[row])) and all(float(g[b]) == float(clean[b]) for b in range(g.shape[0]) if b != row), name
        else:
            assert bool(torch.isfinite(g).all()) and bool((g > 1. - c['phi'] - 1e-12).all()), (name, g)
    assert checked == 4 * (len(GC.SIZES) + len(ragged)) * len(GC.BATCHES)


def test_offset_rows_need_more_than_one_pass_fp32():
    """kind (e): rows with |mean| / std = 1e3 at n = 98304.  E[x^2] - mean^2 summed in fp32 misses the variance ratio by
    percents; the float64 two-pass reference agrees with a float64 one-pass on shifted data to 1e-12"""
    c = GC.make_case('offset', 3, GC.BIG[0], 11)
    mo, cfg = GC.blend32(c['cond'], c['null'], None, c['cs'])
    assert 900. < float((mo.double().mean(dim=1).abs() / mo.double().std(dim=1)).min()) < 1100.
    want = mo.double().var(dim=1, unbiased=False) / cfg.double().var(dim=1, unbiased=False)
    fp32 = GC.one_pass_fp32_variance_ratio(c['cond'], c['null'], None, c['cs']).double()
    off = float(((fp32 - want).abs() / want).max())
    print(f'[parity] one-pass fp32 variance ratio on offset rows: {off:.3f} of the float64 ratio')
    assert not off <= 1e-2                                   # (NaN counts: a negative fp32 variance)
    shifted = []
    for x in (mo.double(), cfg.double()):
        d = x - x[:, :1]
        shifted.append((d * d).mean(dim=1) - d.mean(dim=1) ** 2)
    assert float(((shifted[0] / shifted[1] - want).abs() / want).max()) < 1e-12


def test_statement_reduces_to_the_threshold_statement_at_g_1():
    import threshold_cases as TC
    from dmhomo_amd import _lib, ops
    gen = torch.Generator().manual_seed(5)
    shape = (2, 3, 4, 5)
    mc, mn, x, nz, hist = (torch.randn(shape, generator=gen) for _ in range(5))
    keep = torch.tensor([1, 0], dtype=torch.uint8)
    ones, thr = torch.ones(2), torch.tensor([1., 2.5], dtype=torch.float64)
    for objective in (0, 1, 2):
        for mode, c2 in ((ops.MODE_DDIM, -0.4), (ops.MODE_LAST, 0.), (ops.MODE_MULTISTEP, 0.), (ops.MODE_MULTISTEP, -0.4)):
            step = _lib.DmhStep(objective=objective, clip=1, mode=mode, cond_scale=3., sqrt_recip_ac=1.3, sqrt_recipm1_ac=0.8,
                                sqrt_ac=0.7, sqrt_1m_ac=0.6, c0=0.9, c1=0.3, c2=c2)
            for t in (thr, None):
                got = GC.statement(step, mc, mn, keep, x, nz, hist, t, ones)
                want = TC.statement(step, mc, mn, keep, x, nz, hist, torch.ones(2, dtype=torch.float64) if t is None else t)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            half = GC.statement(step, mc, mn, keep, x, nz, hist, None, torch.tensor([1., 0.5]))
            assert torch.equal(half[2][0], got[2][0]) and not torch.equal(half[2][1], got[2][1])


# ------------------------------------------------------------------------------------------ the binding
def test_binding_has_the_new_entry_points():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in NEW_OPS + ('guidance_splits',):
        assert callable(getattr(ops, name)), name
    assert _lib.ABI_VERSION == 500                           # additions: nothing existing changed


def test_every_new_entry_point_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    buf = ctypes.cast((ctypes.c_char * 256)(), ctypes.c_void_p)
    mk = lambda objective=1, mode=ops.MODE_LAST: ctypes.byref(_lib.DmhStep(objective=objective, clip=1, mode=mode, cond_scale=3.))

    def refused(name, args, word):
        assert getattr(lib, name)(*args, None) == -1, (name, args)
        msg = lib.dmh_last_error().decode()
        assert name + ':' in msg and word in msg, (name, word, msg)
    for name, s in (('dmh_guidance_factor', mk()), ('dmh_guidance_factor_dev', buf)):
        #                 s   cond null keep phi  ws   gfac B  n
        good = [s, buf, buf, None, 0.7, buf, buf, 2, 8]
        for i, word in ((0, 'null'), (1, 'null'), (5, 'null'), (6, 'null'), (2, 'model_null')):
            refused(name, good[:i] + [None] + good[i + 1:], word)
        refused(name, [s, buf, None, buf, 0.7, buf, buf, 2, 8], 'keep needs model_null')
        for B, n, word in ((0, 8, 'B=0'), (-3, 8, 'B=-3'), (2, 0, 'n=0'), (2, 2 ** 31, '2^31')):
            refused(name, good[:7] + [B, n], word)
        for phi in (-0.1, 1.5, float('nan'), float('inf')):
            refused(name, good[:4] + [phi] + good[5:], 'phi')
    for name, s in (('dmh_sampler_threshold_gr', mk()), ('dmh_sampler_threshold_gr_dev', buf)):
        #       s  cond null  x   keep  gfac x0raw thr  B  n  k  frac
        good = [s, buf, buf, buf, None, buf, buf, buf, 2, 8, 3, 0.5]
        for i in (0, 1, 3, 5, 6, 7):
            refused(name, good[:i] + [None] + good[i + 1:], 'null')
        refused(name, [s, buf, None, buf, buf] + good[5:], 'keep needs model_null')
        for B, n, word in ((0, 8, 'B=0'), (2, 0, 'n=0'), (2, 2 ** 31, '2^31')):
            refused(name, good[:8] + [B, n, 0, 0.], word)
        for k, frac in ((-1, 0.), (8, 0.), (0, 1.), (0, -0.5), (7, 0.5), (0, float('nan'))):
            refused(name, good[:10] + [k, frac], 'rank')
    refused('dmh_sampler_threshold_gr', [mk(objective=3), buf, buf, buf, None, buf, buf, buf, 2, 8, 3, 0.5], 'enum')
    for name, s in (('dmh_sampler_step_gr', mk()), ('dmh_sampler_step_gr_dev', buf)):
        #       s  cond null  x  noise hist  thr  gfac out  xs    n  keep per_row
        good = [s, buf, buf, buf, None, None, None, buf, buf, None, 16, None, 8]
        for i in (0, 1, 3, 7, 8):
            refused(name, good[:i] + [None] + good[i + 1:], 'null')
        refused(name, [s, buf, None] + good[3:11] + [buf, 8], 'keep needs model_null')
        refused(name, good[:4] + [buf, buf] + good[6:], 'exclude')
        for total, per_row in ((16, 0), (16, 5), (0, 8), (-16, 8)):
            refused(name, good[:10] + [total, None, per_row], 'per_row')
    for objective, mode, noise, hist, word in ((3, ops.MODE_LAST, None, None, 'enum'), (-1, ops.MODE_LAST, None, None, 'enum'),
                                               (1, ops.MODE_DDPM, buf, None, 'enum'), (1, ops.MODE_DDIM, None, None, 'noise'),
                                               (1, ops.MODE_DDIM, None, buf, 'noise'),
                                               (1, ops.MODE_MULTISTEP, None, None, 'hist'),
                                               (1, ops.MODE_MULTISTEP, buf, None, 'hist')):
        refused('dmh_sampler_step_gr', [mk(objective, mode), buf, buf, buf, noise, hist, None, buf, buf, None, 16, None, 8], word)
