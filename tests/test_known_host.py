"""CPU: the host side of sampling around known pixels (cfg.GaussianDiffusion.sample_known): the stay coefficients of
known_resample against the closed form and the identity behind them, the reason for the write-back (kept bytes do not survive
the sampler's own normalisation), the refusals and the mask forms, the loops' dispatch (off makes none of the new calls), the
capture key, the binding of the new entry points in a table of their own, and their argument validation."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import known_cases as KC
from dmhomo_amd.schedule import ddim_pairs
from test_guidance_host import _run_loop, _stub_loop
from test_solver_host import _abar64, _diffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ('dmh_known_blend', 'dmh_known_error', 'dmh_known_error_splits')
NEW_OPS = ('known_blend', 'known_error', 'known_error_splits', 'known_error_workspace')

# entry -> the test file that launches it ALONE (the rule of tests/test_abi_coverage_host.py, for the table of
# include/dmhomo_hip_known.h); the size query points at this file, which holds it against a restated plan
ALONE = {'dmh_known_blend': ('test_gpu_known.py', 'ops.known_blend'),
         'dmh_known_error': ('test_gpu_known.py', 'ops.known_error'),
         'dmh_known_error_splits': ('test_known_host.py', 'dmh_known_error_splits')}


# ------------------------------------------------------------------------------------------ the stay entries
STAY_CASES = [(sch, T, S, eta) for sch in ('cosine', 'linear') for T in (100, 1000) for S in (1, 5, 32) for eta in (0., 1.)]


@pytest.mark.parametrize('schedule,T,S,eta', STAY_CASES, ids=lambda v: str(v))
def test_stay_coefficients_against_the_closed_form(schedule, T, S, eta):
    d = _diffusion(T, S, schedule, eta=eta)
    abar, host = _abar64(d), d._host()
    pairs = ddim_pairs(T, S)
    plain = d._ddim_steps(True, 3.)
    # r = 1: the list as it is, entry for entry
    again = d._ddim_steps(True, 3., 0)
    assert len(again) == len(plain) == S
    for (t, a, dr), (t2, b, dr2) in zip(plain, again):
        assert (t, dr) == (t2, dr2) and bytes(a) == bytes(b)
    for r in (2, 3):
        steps = d._ddim_steps(True, 3., r - 1)
        assert len(steps) == r * S
        assert [t for t, _, _ in steps] == [t for t, _ in pairs for _ in range(r)]
        assert [dr for _, _, dr in steps] == [1] * (r * S - 1) + [0]
        for k, (t, tn) in enumerate(pairs):
            assert bytes(steps[k * r + r - 1][1]) == bytes(plain[k][1])          # the entry itself is untouched
            want = KC.stay_ref(abar, t, tn, eta)
            got64 = d._stay_coef(host, t, tn)
            a = abar[t]
            # the identity: c1^2 + c2^2 = 1 - abar_t, to float64 rounding: a / a' is rounded at 2^-53 of a number up to 1 before 1 - a / a'
            # is formed, so the figure is absolute — a few roundings of 2^-53 — not one relative to 1 - a
            assert abs(got64[1] ** 2 + got64[2] ** 2 - (1. - a)) <= 8. * 2. ** -53, (t, tn, got64)
            assert abs(want[1] ** 2 + want[2] ** 2 - (1. - a)) <= 8. * 2. ** -53
            for j in range(r - 1):
                st = steps[k * r + j][1]
                assert st.mode == 0 and st.clip == 1 and st.objective == 1 and st.cond_scale == 3.
                assert st.sqrt_ac == plain[k][1].sqrt_ac and st.sqrt_recipm1_ac == plain[k][1].sqrt_recipm1_ac
                for g64, g32, w in zip(got64, (st.c0, st.c1, st.c2), want):
                    # float64 against the closed form written another way.  Compared as squares: each is a short sum of products of
                    # numbers in [0, 1], so a few roundings of 2^-53 ABSOLUTE (c^2 = 1 - a' - sigma^2 cancels: at the first entry of a
                    # cosine schedule it is 1e-9, and a relative figure on c itself would be one of that cancellation); the record
                    # holds the float64 value rounded to fp32 once
                    assert abs(g64 * g64 - w * w) <= 16. * 2. ** -53, (t, tn, g64, w)
                    assert g32 == float(np.float32(g64))
            if tn < 0:
                assert want[1] == 0. and abs(want[2] - math.sqrt(1. - a)) <= 2. ** -52
            elif eta == 0.:                                   # sigma = 0: the stay still draws, c2^2 = 1 - a / a'
                assert abs(want[2] - math.sqrt(1. - a / abar[tn])) <= 2. ** -52


@pytest.mark.parametrize('eta', [0., 0.5, 1.])
def test_entry_then_renoise_is_the_stay_entry(eta):
    """float64, random inputs: the entry t -> s with noise e1, then q(x_t | x_s) with noise e2, equals the stay entry with the
    noise e = (sqrt(a / a') sigma e1 + sqrt(1 - a / a') e2) / c2; the entry that returns x_0 included (a' = 1, sigma = c = 0)"""
    d = _diffusion(100, 5, 'cosine', eta=eta)
    abar = _abar64(d)
    gen = torch.Generator().manual_seed(3)
    worst = 0.
    for t, tn in ddim_pairs(100, 5):
        a = abar[t]
        a1 = 1. if tn < 0 else abar[tn]
        x0 = torch.rand(64, generator=gen, dtype=torch.float64) * 2. - 1.
        xt = torch.randn(64, generator=gen, dtype=torch.float64)
        e1, e2 = (torch.randn(64, generator=gen, dtype=torch.float64) for _ in range(2))
        pn = (xt - math.sqrt(a) * x0) / math.sqrt(1. - a)     # the noise x_t implies relative to x0
        if tn < 0:
            xs, sigma = x0, 0.
        else:
            c0, c, sigma = KC.ddim_ref(abar, t, tn, eta)
            xs = c0 * x0 + c * pn + sigma * e1
        back = math.sqrt(a / a1) * xs + math.sqrt(1. - a / a1) * e2
        s0, s1, s2 = KC.stay_ref(abar, t, tn, eta)
        e = (math.sqrt(a / a1) * sigma * e1 + math.sqrt(1. - a / a1) * e2) / s2
        stay = s0 * x0 + s1 * pn + s2 * e
        worst = max(worst, float((stay - back).abs().max()))
    print(f'[parity] entry + re-noise against the stay entry, eta {eta}: max difference {worst:.2e}')
    assert worst <= 1e-13


# ------------------------------------------------------------------------------------------ why there is a write-back
def test_kept_bytes_need_the_write_back():
    """for all 256 values k = n / 255: the caller's own value truncates to byte n; the value that went through the sampler's
    normalisation, 0.5 * (2 k - 1) + 0.5 in fp32, does not for every n — the reason the kept elements are written back in [0, 1]"""
    k = KC.all_bytes()
    n = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(KC.bytes_of(k), n)
    two, one, half = (torch.tensor(v, dtype=torch.float32) for v in (2., 1., 0.5))
    loop_only = (k * two - one) * half + half
    wrong = KC.bytes_of(loop_only) != n
    print(f'[known] {int((loop_only == k).sum())} of 256 values survive the normalisation; {int(wrong.sum())} bytes come back wrong')
    assert int(wrong.sum()) > 0 and int((loop_only == k).sum()) < 256
    assert torch.equal(KC.bytes_of(loop_only)[wrong].to(torch.int32), n[wrong].to(torch.int32) - 1)
    # the write-back is the select on the unnormalised image with the caller's values
    img = KC.select(loop_only, k, torch.ones(256, dtype=torch.uint8))
    assert torch.equal(KC.bytes_of(img), n)


# ------------------------------------------------------------------------------------------ the switches and the refusals
def _cfg(S=4):
    return _diffusion(20, S)


def test_defaults_are_off():
    from dmhomo_amd import ddpm
    from dmhomo_amd.denoising_diffusion_models import classifier_free_guidance as alias
    d = _cfg()
    assert d.known_resample == 1 and d.score_known is False and d._check_known() == 0
    assert callable(alias.GaussianDiffusion.sample_known)
    assert not hasattr(ddpm.GaussianDiffusion, 'sample_known')
    assert ddpm.Trainer.keep is None and ddpm.Trainer.score_known is False and ddpm.Trainer.last_known_error is None


@pytest.mark.parametrize('bad', [0, -1, 1.0, 2.5, '2', None, True, False, [2]])
def test_known_resample_must_be_an_int_of_at_least_one(bad):
    d = _cfg()
    d.known_resample = bad
    with pytest.raises(ValueError, match='known_resample'):
        d._check_known()


@pytest.mark.parametrize('setting, value, word', [('objective', 'pred_noise', 'pred_x0'), ('objective', 'pred_v', 'pred_x0'),
                                                  ('clip_mode', 'dynamic', 'division'), ('guidance_rescale', 0.7, 'rescale')])
def test_refusals_name_the_setting_and_say_why(setting, value, word):
    d = _cfg()
    setattr(d, setting, value)
    shape = (2, 6, 8, 8)
    with pytest.raises(ValueError, match=f'sample_known.*{setting}.*{word}'):
        d._check_known()
    with pytest.raises(ValueError, match=f'sample_known.*{setting}'):    # in front of the first launch (no GPU here)
        d.sample_known(torch.zeros(shape), 'source', torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, 8, 8),
                       torch.zeros(2, 2, 8, 8), torch.zeros(2, 1, 8, 8))


def test_resampling_is_refused_with_the_multistep_solver():
    d = _cfg()
    d.sampler = 'dpmpp_2m'
    assert d._check_known() == 0                              # r = 1: both samplers
    d.known_resample = 2
    with pytest.raises(ValueError, match='known_resample.*dpmpp_2m.*history'):
        d._check_known()
    with pytest.raises(ValueError, match='dpmpp_2m'):
        d._sampler_steps(True, 3., 1)
    d.sampler = 'ddim'
    assert d._check_known() == 1 and len(d._sampler_steps(True, 3., 1)) == 8


def test_known_is_checked_once_per_call():
    d = _cfg()
    shape = (2, 6, 8, 8)
    ok = torch.rand(shape)
    for bad in (torch.rand(2, 6, 8, 7), torch.rand(2, 3, 8, 8), torch.rand(1, 6, 8, 8), [[0.]]):
        with pytest.raises(ValueError, match='known'):
            d._known_inputs(bad, 'source', shape)
    for v in (-1e-6, 1.0001, float('nan'), float('inf')):
        k = ok.clone()
        k[1, 4, 3, 2] = v
        with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
            d._known_inputs(k, 'source', shape)
    edge = ok.clone()
    edge[0, 0, 0, 0], edge[0, 0, 0, 1] = 0., 1.
    kn = d._known_inputs(edge, 'target', shape)
    assert torch.equal(kn['known'], edge) and kn['stays'] == 0 and kn['score'] is False


def test_mask_forms_broadcast_to_the_pair():
    d = _cfg()
    shape = (2, 6, 8, 8)
    known = torch.rand(shape)
    m = lambda km: d._known_inputs(known, km, shape)['mask']
    src, tgt = m('source').reshape(shape), m('target').reshape(shape)
    assert src.dtype == torch.uint8 and tuple(m('source').shape) == (2, 6 * 64)
    assert bool(src[:, :3].all()) and not bool(src[:, 3:].any()) and bool(tgt[:, 3:].all()) and not bool(tgt[:, :3].any())
    assert int(m(torch.ones(1)).sum()) == 2 * 6 * 64 and int(m(0).sum()) == 0 and int(m(True).sum()) == 2 * 6 * 64
    pix = torch.zeros(2, 1, 8, 8)
    pix[1, 0, 2:4, 5] = -0.5                                  # any nonzero value keeps
    got = m(pix).reshape(shape)
    assert int(got.sum()) == 12 and bool(got[1, :, 2:4, 5].all()) and not bool(got[0].any())
    chan = torch.tensor([1, 0, 0, 0, 0, 2]).reshape(6, 1, 1)
    got = m(chan).reshape(shape)
    assert bool(got[:, 0].all()) and bool(got[:, 5].all()) and not bool(got[:, 1:5].any())
    assert torch.equal(m(src.bool()), m('source'))
    for bad in ('both', 'Source', torch.ones(2, 5, 8, 8), torch.ones(3, 1, 1, 1)):
        with pytest.raises(ValueError, match='known_mask'):
            m(bad)
    d.known_resample, d.score_known = 3, True
    kn = d._known_inputs(known, 'source', shape)
    assert kn['stays'] == 2 and kn['score'] is True


# ------------------------------------------------------------------------------------------ the loops' dispatch
def _stub_known(monkeypatch, calls):
    from dmhomo_amd import ops

    def fake(name, result):
        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return result(*a, **k)
        monkeypatch.setattr(ops, name, f)
    fake('known_error_workspace', lambda x: torch.zeros(2, dtype=torch.float64))
    fake('known_error', lambda cond, *a, **k: torch.zeros(cond.shape[0], dtype=torch.float64))
    fake('known_blend', lambda cond, null, keep, cs, known, kmask, out=None: cond if out is None else out)


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_take_the_new_path_only_with_known(sampler, monkeypatch):
    from dmhomo_amd import ops
    S = 4
    d = _cfg(S)
    d.sampler = sampler
    calls = _stub_loop(d, monkeypatch)
    _stub_known(monkeypatch, calls)
    old_step = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler]
    d.known_resample, d.score_known = (3 if sampler == 'ddim' else 1), True      # the attributes alone change nothing
    for cond_scale in (3., 1.):
        calls.clear()
        trace = _run_loop(d, sampler, cond_scale)
        assert calls == {old_step: S} and all('known_err' not in e and 'stay' not in e for e in trace)
    shape = (2, 6, 8, 8)
    seen = []
    inner = getattr(ops, old_step)

    def spy(step, cond, null, *a, **k):
        seen.append((cond, null, k.get('keep')))
        return inner(step, cond, null, *a, **k)
    monkeypatch.setattr(ops, old_step, spy)
    r = d.known_resample
    args = (torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8), torch.zeros(2, 1, 8, 8))
    for cond_scale in (3., 1.):
        calls.clear(), seen.clear()
        d.sample_known(torch.rand(shape), 'source', *args, cond_scale=cond_scale)
        # r * S updates; the score on the last entry only (two launches inside one call); the blend per entry + the write-back
        assert calls == {old_step: r * S, 'known_blend': r * S + 1, 'known_error': 1, 'known_error_workspace': 1}, calls
        assert all(null is None and keep is None for _, null, keep in seen) and len({id(c) for c, _, _ in seen}) == 1
        assert d.last_known_error.shape == (2,) and d.last_known_error.dtype == torch.float64
    kn = d._known_inputs(torch.rand(shape), 'source', shape)
    trace = []
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    loop(*args, shape, 3., trace=trace, known=kn)
    assert len(trace) == r * S and all(e['known_err'].shape == (2,) for e in trace)
    assert [bool(e.get('stay')) for e in trace] == [k % r != r - 1 for k in range(r * S)]
    assert [e['time'] for e in trace] == [t for t, _ in ddim_pairs(20, S) for _ in range(r)]


def test_capture_key_carries_the_feature_but_not_the_pixels(monkeypatch):
    d = _cfg()
    keys, lens = [], []

    def fake_replay(shape, device, key, tables, buffers, fill):
        keys.append(tuple(key))
        lens.append(len(tables()[0]))
        d.__dict__['_graph_state'] = {'known_err': torch.zeros(shape[0], dtype=torch.float64)}
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    shape = (2, 6, 8, 8)
    args = (torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8), torch.zeros(2, 1, 8, 8), shape, 3.)
    d._sample_graphed(*args)                                  # 0: the default
    d.known_resample, d.score_known = 2, True                 # 1: the attributes alone change nothing
    d._sample_graphed(*args)
    for mask in ('source', 'target'):                         # 2, 3: on; another source and mask, the same key
        d._sample_graphed(*args, known=d._known_inputs(torch.rand(shape), mask, shape))
    d.known_resample = 1                                      # 4
    d._sample_graphed(*args, known=d._known_inputs(torch.rand(shape), 'source', shape))
    d.score_known = False                                     # 5
    d._sample_graphed(*args, known=d._known_inputs(torch.rand(shape), 'source', shape))
    assert keys[0][-1] == 0. and keys[1] == keys[0]           # (the default key still ends with guidance_rescale)
    assert keys[2] == keys[3] == keys[0] + (('known', 2, True),)
    assert keys[4] == keys[0] + (('known', 1, True),) and keys[5] == keys[0] + (('known', 1, False),)
    assert lens == [4, 4, 8, 8, 4, 4]


def test_cli_flags_parse_and_the_docstring_warns_about_synthetic_conditions():
    src = open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    doc = src.split('"""')[1]
    assert '--keep' in doc and '--known_resample' in doc and 'SyntheticConditions' in doc and 'black' in doc
    head = src[:src.index('args = parser.parse_args()')]
    head = head[head.index('parser = argparse.ArgumentParser()'):]
    ns = {}
    exec('import argparse\n' + head, ns)                     # the parser alone (the script's imports need the built package)
    p = ns['parser']
    a = p.parse_args([])
    assert a.keep is None and a.known_resample == 1
    a = p.parse_args(['--keep', 'target', '--known_resample', '3'])
    assert a.keep == 'target' and a.known_resample == 3
    for bad in (['--keep'], ['--keep', 'both'], ['--known_resample', 'x']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert 'trainer.keep, sampler.known_resample = args.keep, args.known_resample' in src and 'last_known_error' in src


# ------------------------------------------------------------------------------------------ the binding
def _known_header_functions():
    src = open(os.path.join(ROOT, 'include', 'dmhomo_hip_known.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(dmh_[a-z0-9_]+)\s*\(', src)))


def test_the_new_entries_have_a_header_and_a_table_of_their_own():
    from dmhomo_amd import _lib, ops
    names = _known_header_functions()
    assert names == sorted(_lib.EXTENSIONS) == sorted(NEW_ENTRY_POINTS)
    assert not set(names) & set(_lib.SIGNATURES)
    main = open(os.path.join(ROOT, 'include', 'dmhomo_hip.h')).read()
    assert 'dmh_known' not in main
    assert _lib.ABI_VERSION == 500
    h = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for name in names:
        assert hasattr(h, name), name
        res, args = _lib.EXTENSIONS[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args), name
    for name in NEW_OPS:
        assert callable(getattr(ops, name)), name


def test_every_new_entry_names_the_test_that_launches_it_alone():
    from dmhomo_amd import _lib
    assert sorted(ALONE) == sorted(_lib.EXTENSIONS)
    tests = os.path.dirname(os.path.abspath(__file__))
    for entry, (file, name) in ALONE.items():
        src = open(os.path.join(tests, file)).read()
        assert re.search(r'\b' + re.escape(name) + r'\s*\(', src) or f"'{entry}'" in src, (entry, file)
    ops_src = open(os.path.join(ROOT, 'dmhomo_amd', 'ops.py')).read()
    for entry in ('dmh_known_blend', 'dmh_known_error'):
        assert f"call('{entry}'" in ops_src                   # (the thin wrapper the row names calls the entry and nothing else)


def test_a_library_without_the_new_symbols_fails_loudly(monkeypatch):
    from dmhomo_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setitem(_lib.EXTENSIONS, 'dmh_known_missing', (C.c_int, []))
    with pytest.raises(AttributeError, match='dmh_known_missing'):
        _lib.lib()


def test_error_splits_plan():
    from dmhomo_amd import _lib
    lib = _lib.lib()
    for B, n in ((1, 1), (3, 1536), (25, 98304), (25, 393216), (1, 2 ** 31 - 1), (65535, 5), (2000, 10 ** 6)):
        assert lib.dmh_known_error_splits(B, n) == min((n + 4095) // 4096, max(1024 // B, 1)), (B, n)
    assert lib.dmh_known_error_splits(3, 1536) == 1 and lib.dmh_known_error_splits(25, 98304) == 24
    for B, n in ((0, 4), (-1, 4), (65536, 4), (1, 0), (1, -5), (1, 2 ** 31), (1, 2 ** 62), (2, 2 ** 63 - 1)):
        assert lib.dmh_known_error_splits(B, n) <= 0, (B, n)
        assert b'dmh_known_error_splits' in lib.dmh_last_error()


def test_every_new_entry_point_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * (16 * 4096))()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda k=0, off=0: C.c_void_p(base + 4096 * k + off)  # disjoint host addresses: only ever compared, never read
    n = 0

    def refused(name, args, word):
        nonlocal n
        assert getattr(lib, name)(*args, None) == -1, (name, word)
        assert name.encode() in lib.dmh_last_error() and word.encode() in lib.dmh_last_error(), (name, lib.dmh_last_error())
        n += 1
    #         cond  null  keep  cs  known kmask out   B  per_row          (2 x 24 floats = 192 bytes per tensor)
    blend = [p(0), p(1), p(2), 3., p(3), p(4), p(5), 2, 24]
    #         cond  null  keep  cs  known kmask ws    out   B  per_row
    error = [p(0), p(1), p(2), 3., p(3), p(4), p(5), p(6), 2, 24]
    for name, good, must in (('dmh_known_blend', blend, (0, 4, 5, 6)), ('dmh_known_error', error, (0, 4, 5, 6, 7))):
        for i in must:
            refused(name, good[:i] + [None] + good[i + 1:], 'null pointer')
        refused(name, good[:1] + [None] + good[2:], 'keep needs model_null')
        for cs in (float('nan'), float('inf'), -float('inf')):
            refused(name, good[:3] + [cs] + good[4:], 'cond_scale')
        for B, per_row in ((0, 24), (-1, 24), (65536, 24), (2, 0), (2, -1), (2, 2 ** 31), (2, 2 ** 62)):
            refused(name, good[:-2] + [B, per_row], 'per_row')
        refused(name, [p(0, 2)] + good[1:], 'aligned')
        refused(name, good[:4] + [p(3, 1)] + good[5:], 'aligned')
    # aliasing of the blend: in place on cond is the one alias allowed, and only whole
    for i, word in ((1, 'model_null or known'), (4, 'model_null or known'), (5, 'kmask')):
        refused('dmh_known_blend', blend[:6] + [blend[i]] + blend[7:], word)
    refused('dmh_known_blend', blend[:6] + [p(1, 188)] + blend[7:], 'model_null or known')    # the last float of null
    refused('dmh_known_blend', blend[:6] + [p(4, 44)] + blend[7:], 'kmask')                   # the last four mask bytes
    refused('dmh_known_blend', blend[:6] + [p(0, 16)] + blend[7:], 'in part')
    refused('dmh_known_blend', blend[:6] + [p(5, 2)] + blend[7:], 'aligned')
    refused('dmh_known_error', error[:6] + [p(5, 4)] + error[7:], '8-byte')
    refused('dmh_known_error', error[:7] + [p(5)] + error[8:], 'ws overlaps out')
    refused('dmh_known_error', error[:7] + [p(5, 24)] + error[8:], 'ws overlaps out')        # inside ws (2 rows x 1 split x 16 bytes)
    assert n == (4 + 1 + 3 + 7 + 2) + (5 + 1 + 3 + 7 + 2) + 7 + 3
