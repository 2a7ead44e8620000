"""CPU: the host side of starting the sampler from a given pair (cfg.GaussianDiffusion.sample_from): the strength -> first entry
map against its restatement, the sliced step lists, the capture keys, the binding of the new entry point in a table of its own,
its argument validation (before any launch: no GPU here), the CLI flag."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import start_cases as SC
from dmhomo_amd.schedule import ddim_pairs
from test_guidance_host import _stub_loop
from test_solver_host import _abar64, _diffusion, _rel, reference_coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry -> the test file that launches it ALONE (the rule of tests/test_abi_coverage_host.py, for the table of
# include/dmhomo_hip_start.h)
ALONE = {'dmh_start_mix': ('test_gpu_start.py', 'ops.start_mix')}


# ------------------------------------------------------------------------------------------ strength -> first entry
SIZES = (1, 5, 10, 32, 250)


def _grid(S):
    """strengths: a uniform grid, every exact multiple k / S and its neighbours in double, the ends"""
    out = [i / 64 for i in range(1, 65)]
    for k in range(1, S + 1):
        v = SC.exact_multiple(k, S)
        out += [v, math.nextafter(v, 0.), math.nextafter(v, 2.)]
    return [v for v in out if 0. < v <= 1.]


@pytest.mark.parametrize('S', SIZES)
def test_start_entry_against_the_restatement(S):
    from dmhomo_amd.schedule import start_entry
    ran = set()
    for s in _grid(S):
        want = SC.first_entry(S, s)
        if want is None:
            with pytest.raises(ValueError, match='smallest strength'):
                start_entry(S, s)
            continue
        got = start_entry(S, s)
        assert got == want and 0 <= got < S, (S, s, got, want)
        ran.add(S - got)
    assert ran == set(range(1, S + 1))                        # every entry count is reached
    assert start_entry(S, 1.) == 0 and start_entry(S, 1) == 0
    assert start_entry(S, SC.exact_multiple(1, S)) == S - 1   # the smallest strength that runs


def test_exact_multiples_run_their_entries():
    """k / S written as a decimal must run k entries although S * (k / S) can land below k in double"""
    from dmhomo_amd.schedule import start_entry
    assert 22 * (15 / 22) < 15. and start_entry(22, 15 / 22) == 7               # (the reason for the 1e-9)
    assert start_entry(5, 0.6) == 2 and start_entry(10, 0.3) == 7 and start_entry(10, 0.7) == 3
    assert start_entry(5, 0.2) == 4 and start_entry(5, 0.4) == 3 and start_entry(5, 0.8) == 1 and start_entry(5, 1.0) == 0
    for S in SIZES:
        for k in range(1, S + 1):
            assert start_entry(S, SC.exact_multiple(k, S)) == S - k, (S, k)


@pytest.mark.parametrize('bad', [0., -0.5, 1.0000001, 2, float('nan'), float('inf'), -float('inf'), None, '0.5', True, False, [0.5]])
def test_start_entry_refuses_what_is_no_strength(bad):
    from dmhomo_amd.schedule import start_entry
    with pytest.raises(ValueError, match='strength'):
        start_entry(5, bad)


def test_a_strength_that_runs_nothing_names_the_smallest_that_does():
    from dmhomo_amd.schedule import start_entry
    with pytest.raises(ValueError, match=r'smallest strength.*1 / 5 = 0\.2'):
        start_entry(5, 0.19)
    with pytest.raises(ValueError, match=r'1 / 250'):
        start_entry(250, 0.003)
    assert start_entry(250, 0.004) == 249


# ------------------------------------------------------------------------------------------ the sliced step lists
CASES = [(sch, T, S, eta) for sch in ('cosine', 'linear') for T, S in ((100, 5), (1000, 32), (20, 4)) for eta in (0., 1.)]


@pytest.mark.parametrize('schedule,T,S,eta', CASES, ids=lambda v: str(v))
def test_ddim_slice_is_the_tail_of_the_full_table(schedule, T, S, eta):
    d = _diffusion(T, S, schedule, eta=eta)
    pairs = ddim_pairs(T, S)
    for stays in (0, 1, 2):
        full = d._ddim_steps(True, 3., stays)
        assert len(full) == S * (stays + 1)
        again = d._ddim_steps(True, 3., stays, 0)
        assert [(t, bytes(st), dr) for t, st, dr in again] == [(t, bytes(st), dr) for t, st, dr in full]
        for k0 in range(S):
            cut = d._ddim_steps(True, 3., stays, first=k0)
            tail = full[k0 * (stays + 1):]
            assert len(cut) == (S - k0) * (stays + 1)
            assert [t for t, _, _ in cut] == [t for t, _ in pairs[k0:] for _ in range(stays + 1)]
            for (t, a, dr), (t2, b, dr2) in zip(cut, tail):
                assert (t, dr) == (t2, dr2)
                for name, _ in a._fields_:                    # field for field
                    assert getattr(a, name) == getattr(b, name), (k0, stays, t, name)
            assert cut[-1][2] == 0 and all(dr == 1 for _, _, dr in cut[:-1])


# (a linear schedule of 20 steps reaches alphas_cumprod == 0 in fp32, where the solver's log-SNR does not exist)
SOLVER_CASES = [c for c in CASES if c[:2] != ('linear', 20)]


@pytest.mark.parametrize('schedule,T,S,eta', SOLVER_CASES, ids=lambda v: str(v))
def test_solver_slice_is_the_solver_of_the_list_that_begins_there(schedule, T, S, eta, monkeypatch):
    from dmhomo_amd import ops, sampling
    d = _diffusion(T, S, schedule, eta=eta)
    abar = _abar64(d)
    pairs = ddim_pairs(T, S)
    full = d._dpmpp_steps(True, 3.)
    assert [(t, bytes(st)) for t, st, _ in d._dpmpp_steps(True, 3., 0)] == [(t, bytes(st)) for t, st, _ in full]
    for k0 in range(S):
        cut = d._dpmpp_steps(True, 3., first=k0)
        assert [t for t, _, _ in cut] == [t for t, _ in pairs[k0:]] and all(dr == 0 for _, _, dr in cut)
        assert cut[-1][1].mode == ops.MODE_LAST
        upd = [st for _, st, _ in cut[:-1]]
        if upd:
            assert upd[0].c2 == 0. and upd[-1].c2 == 0. and all(st.c2 != 0. for st in upd[1:-1])     # first order, lower order final
        # the coefficients from the definitions over pairs[k0:] (the tolerance of tests/test_solver_host.py: float64 rounded to fp32)
        for st, w in zip(upd, reference_coefficients(abar, pairs[k0:])):
            for got, ref in zip((st.c0, st.c1, st.c2), w):
                ref32 = float(torch.tensor(ref, dtype=torch.float32))
                assert _rel(got, ref32) <= 1e-6 if ref32 != 0. else got == 0., (k0, got, ref32)
        # and, record for record, the product's own list over a time list that begins at k0
        with monkeypatch.context() as mp:
            mp.setattr(sampling, 'ddim_pairs', lambda T_, S_: pairs[k0:])
            own = d._dpmpp_steps(True, 3.)
        assert [(t, bytes(st)) for t, st, _ in own] == [(t, bytes(st)) for t, st, _ in cut], k0
        if 0 < k0 < S - 2:                                    # ... which is NOT the tail of the full list: entry k0 there is second order
            assert bytes(cut[0][1]) != bytes(full[k0][1])
    d.sampler = 'dpmpp_2m'                                    # the selected sampler's list passes ``first`` on
    for k0 in range(S):
        assert [bytes(st) for _, st, _ in d._sampler_steps(True, 3., 0, k0)] == [bytes(st) for _, st, _ in d._dpmpp_steps(True, 3., k0)]


# ------------------------------------------------------------------------------------------ the helper, the loops
def _cfg(S=4):
    return _diffusion(20, S)


SHAPE = (2, 6, 8, 8)
ARGS = lambda: (torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8), torch.zeros(2, 1, 8, 8))


def test_defaults_are_off():
    from dmhomo_amd import ddpm
    from dmhomo_amd.denoising_diffusion_models import classifier_free_guidance as alias
    assert callable(alias.GaussianDiffusion.sample_from) and alias.GaussianDiffusion.last_start is None
    assert not hasattr(ddpm.GaussianDiffusion, 'sample_from')
    assert ddpm.Trainer.strength is None


def test_start_inputs_hold_the_buffer_values_of_the_start_time():
    d = _cfg(4)
    host = d._host()
    pairs = ddim_pairs(20, 4)
    init = torch.rand(SHAPE)
    init[0, 0, 0, 0], init[0, 0, 0, 1] = 0., 1.
    for strength, k0 in ((0.25, 3), (0.5, 2), (0.75, 1), (1., 0), (0.3, 3), (0.99, 1)):
        st = d._start_inputs(init, strength, SHAPE)
        t = pairs[k0][0]
        assert st['k0'] == k0 and st['t'] == t and torch.equal(st['init'], init)
        assert st['ca'] == float(host['sqrt_alphas_cumprod'][t]) and st['cb'] == float(host['sqrt_one_minus_alphas_cumprod'][t])
        assert st['ca'] == float(SC.f32(st['ca'])) and st['cb'] == float(SC.f32(st['cb']))       # fp32 values
    assert d._start_inputs(init.double(), 1., SHAPE)['init'].dtype == torch.float32


def test_refusals_come_before_the_first_launch():
    d = _cfg(4)
    ok = torch.rand(SHAPE)
    for bad in (0., 1.5, float('nan'), None, '1', True):
        with pytest.raises(ValueError, match='strength'):
            d.sample_from(ok, bad, *ARGS())
    with pytest.raises(ValueError, match=r'smallest strength.*1 / 4 = 0\.25'):
        d.sample_from(ok, 0.2, *ARGS())
    for bad in (torch.rand(2, 6, 8, 7), torch.rand(2, 3, 8, 8), torch.rand(1, 6, 8, 8), [[0.]]):
        with pytest.raises(ValueError, match='init'):
            d.sample_from(bad, 0.5, *ARGS())
    for v in (-1e-6, 1.0001, float('nan'), float('inf')):
        x = ok.clone()
        x[1, 4, 3, 2] = v
        with pytest.raises(ValueError, match=r'init.*outside \[0, 1\]'):
            d.sample_from(x, 0.5, *ARGS())
    with pytest.raises(ValueError, match='known and known_mask'):
        d.sample_from(ok, 0.5, *ARGS(), known=ok)
    with pytest.raises(ValueError, match='known and known_mask'):
        d.sample_from(ok, 0.5, *ARGS(), known_mask='source')
    d.clip_mode = 'dynamic'                                   # every refusal of _check_known applies with known
    with pytest.raises(ValueError, match='sample_known.*clip_mode'):
        d.sample_from(ok, 0.5, *ARGS(), known=ok, known_mask='source')
    d.clip_mode = 'static'
    full = _diffusion(20, 20)                                 # neither DDIM nor the solver: sample()'s TypeError
    assert not full.is_ddim_sampling
    with pytest.raises(TypeError, match='p_sample_loop'):
        full.sample_from(ok, 0.5, *ARGS())
    with pytest.raises(TypeError, match='p_sample_loop'):
        full.sample(*ARGS())


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_begin_at_the_start_entry(sampler, monkeypatch):
    """through the stubs of tests/test_guidance_host.py: the loop makes one start_mix call in place of its first draw and walks
    pairs[k0:]; without ``start`` it makes none"""
    S = 4
    d = _cfg(S)
    d.sampler = sampler
    calls = _stub_loop(d, monkeypatch)
    mixes = []

    def start_mix(init01, ca, cb, out=None):
        mixes.append((init01, ca, cb))
        return torch.zeros(tuple(init01.shape))
    d.rng.start_mix = start_mix
    draws = []
    randn = d.rng.randn
    d.rng.randn = lambda shape, device: draws.append(1) or randn(shape, device)
    step = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler]
    pairs = ddim_pairs(20, S)
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    trace = []
    loop(*ARGS(), SHAPE, 3., trace=trace)
    assert not mixes and calls == {step: S} and [e['time'] for e in trace] == [t for t, _ in pairs]
    per_entry = 1 if sampler == 'ddim' else 0
    assert len(draws) == 1 + per_entry * (S - 1)
    init = torch.rand(SHAPE)
    for strength, k0 in ((0.25, 3), (0.5, 2), (0.8, 1), (1., 0)):
        calls.clear(), mixes.clear(), draws.clear()
        trace = []
        st = d._start_inputs(init, strength, SHAPE)
        loop(*ARGS(), SHAPE, 3., trace=trace, start=st)
        assert len(mixes) == 1 and mixes[0][0] is st['init'] and mixes[0][1:] == (st['ca'], st['cb'])
        assert calls == {step: S - k0} and [e['time'] for e in trace] == [t for t, _ in pairs[k0:]]
        assert len(draws) == per_entry * (S - k0 - 1)         # the initial draw is the kernel's; the skipped entries draw nothing
        calls.clear()
        d.sample_from(init, strength, *ARGS())
        assert calls == {step: S - k0} and d.last_start == (k0, pairs[k0][0])


# ------------------------------------------------------------------------------------------ the capture keys
def _keys_of(d, monkeypatch):
    keys, lens, firsts = [], [], []

    def fake_replay(shape, device, key, tables, buffers, fill, **kw):
        keys.append(tuple(key))
        lens.append(len(tables()[0]))
        firsts.append(kw)
        d.__dict__['_graph_state'] = {'known_err': torch.zeros(shape[0], dtype=torch.float64)}
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    return keys, lens, firsts


def test_capture_key_under_ddim_knows_nothing_of_the_start(monkeypatch):
    S = 4
    d = _cfg(S)
    keys, lens, firsts = _keys_of(d, monkeypatch)
    args = ARGS() + (SHAPE, 3.)
    start = lambda s: d._start_inputs(torch.rand(SHAPE), s, SHAPE)
    d._sample_graphed(*args)                                  # 0: the default
    for s in (0.25, 0.5, 1.):                                 # 1-3
        d._sample_graphed(*args, start=start(s))
    assert keys[0][-1] == 0.                                  # (the default key still ends with guidance_rescale)
    assert keys[1] == keys[2] == keys[3] == keys[0] and lens == [S] * 4
    assert firsts == [{}, {'first': 3}, {'first': 2}, {}]     # (k0 = 0: the call sample() makes, argument for argument)
    d.known_resample = 2
    kn = lambda: d._known_inputs(torch.rand(SHAPE), 'source', SHAPE)
    d._sample_graphed(*args, known=kn())                      # 4: sample_known's key
    d._sample_graphed(*args, known=kn(), start=start(0.5))    # 5
    assert keys[4] == keys[0] + (('known', 2, False),) and keys[5] == keys[4]
    assert lens[4:] == [2 * S] * 2 and firsts[4:] == [{}, {'first': 4}]      # first = k0 * (stays + 1)


def test_capture_key_under_the_solver_gains_the_first_entry(monkeypatch):
    S = 4
    d = _cfg(S)
    d.sampler = 'dpmpp_2m'
    keys, lens, firsts = _keys_of(d, monkeypatch)
    args = ARGS() + (SHAPE, 3.)
    start = lambda s: d._start_inputs(torch.rand(SHAPE), s, SHAPE)
    d._sample_graphed(*args)
    for s in (1., 0.75, 0.5, 0.25, 0.3):
        d._sample_graphed(*args, start=start(s))
    assert keys[1] == keys[0]                                 # k0 = 0: unchanged
    assert [k[len(keys[0]):] for k in keys[2:]] == [(('first', 1),), (('first', 2),), (('first', 3),), (('first', 3),)]
    assert all(k[:len(keys[0])] == keys[0] for k in keys)
    assert lens == [S, S, S - 1, S - 2, S - 3, S - 3] and firsts == [{}] * 6       # the table begins at k0: the replay at its entry 0
    kn = d._known_inputs(torch.rand(SHAPE), 'target', SHAPE)
    d._sample_graphed(*args, known=kn)
    d._sample_graphed(*args, known=kn, start=start(0.5))
    assert keys[6] == keys[0] + (('known', 1, False),) and keys[7] == keys[6] + (('first', 2),)      # behind the 'known' part


def test_guided_flags_come_from_the_table_the_capture_holds(monkeypatch):
    """under guidance_interval fill writes a flag per entry of the capture's own table: the full one under 'ddim', the one over
    pairs[k0:] under the solver"""
    S = 4
    for sampler in ('ddim', 'dpmpp_2m'):
        d = _cfg(S)
        d.sampler, d.guidance_interval = sampler, (0., 0.5)
        seen = {}

        def fake_replay(shape, device, key, tables, buffers, fill, **kw):
            seen['times'] = tables()[1]
            seen['key'] = key
            return torch.zeros(shape)
        monkeypatch.setattr(d, '_replay_captured', fake_replay)
        d._sample_graphed(*ARGS(), SHAPE, 3., start=d._start_inputs(torch.rand(SHAPE), 0.5, SHAPE))
        pairs = ddim_pairs(20, S)
        want = [t for t, _ in (pairs if sampler == 'ddim' else pairs[2:])]
        assert seen['times'] == want and 'guidance_interval' in seen['key']
        assert d._guided_entries(seen['times'], 3.) == [0. <= t / 19. <= 0.5 for t in want]


# ------------------------------------------------------------------------------------------ the binding
def _header_functions(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(dmh_[a-z0-9_]+)\s*\(', src)))


def test_the_new_entry_has_a_header_and_a_table_of_its_own():
    from dmhomo_amd import _lib, ops
    names = _header_functions('dmhomo_hip_start.h')
    assert names == sorted(_lib.START_EXTENSIONS) == ['dmh_start_mix']
    assert not set(names) & set(_lib.SIGNATURES) and not set(names) & set(_lib.EXTENSIONS)
    for other in ('dmhomo_hip.h', 'dmhomo_hip_known.h'):
        assert 'dmh_start' not in open(os.path.join(ROOT, 'include', other)).read()
    assert _lib.ABI_VERSION == 500
    h = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    for name in names:
        assert hasattr(h, name), name
        res, args = _lib.START_EXTENSIONS[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args), name
    assert callable(ops.start_mix)
    assert "call('dmh_start_mix'" in open(os.path.join(ROOT, 'dmhomo_amd', 'ops.py')).read()


def test_the_new_entry_names_the_test_that_launches_it_alone():
    from dmhomo_amd import _lib
    assert sorted(ALONE) == sorted(_lib.START_EXTENSIONS)
    tests = os.path.dirname(os.path.abspath(__file__))
    for entry, (file, name) in ALONE.items():
        src = open(os.path.join(tests, file)).read()
        assert re.search(r'\b' + re.escape(name) + r'\s*\(', src), (entry, file)


def test_a_library_without_the_new_symbol_fails_loudly(monkeypatch):
    from dmhomo_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setitem(_lib.START_EXTENSIONS, 'dmh_start_missing', (C.c_int, []))
    with pytest.raises(AttributeError, match='dmh_start_missing'):
        _lib.lib()


def test_the_makefile_builds_the_new_source_with_its_header():
    mk = open(os.path.join(ROOT, 'dmhomo_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bstart\.hip\b', mk, flags=re.M)
    rules = [ln for ln in mk.splitlines() if re.match(r'^(asan/)?%\.o: %\.hip', ln)]
    assert len(rules) == 2 and all('include/dmhomo_hip_start.h' in ln for ln in rules)


def test_the_entry_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * (16 * 4096))()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda k=0, off=0: C.c_void_p(base + 4096 * k + off)  # disjoint host addresses: only ever compared, never read
    n = 0

    def refused(args, word):
        nonlocal n
        assert lib.dmh_start_mix(*args, None) == -1, (args, word)
        assert b'dmh_start_mix' in lib.dmh_last_error() and word.encode() in lib.dmh_last_error(), (word, lib.dmh_last_error())
        n += 1
    #        init  noise ids   state ca   cb   out   B  per_sample      (2 x 24 floats = 192 bytes per tensor)
    given = [p(0), p(1), None, None, 0.6, 0.8, p(4), 2, 24]
    keyed = [p(0), None, p(2), p(3), 0.6, 0.8, p(4), 2, 24]
    for good in (given, keyed):
        for i in (0, 6):
            refused(good[:i] + [None] + good[i + 1:], 'null pointer')
        for B, per in ((0, 24), (-1, 24), (65536, 24), (2, 0), (2, -1), (2, 2 ** 31), (2, 2 ** 62)):
            refused(good[:-2] + [B, per], 'per_sample')
        for bad in (float('nan'), float('inf'), -float('inf')):
            refused(good[:4] + [bad] + good[5:], 'finite')
            refused(good[:5] + [bad] + good[6:], 'finite')
        refused([p(0, 2)] + good[1:], '4-byte')
        refused(good[:6] + [p(4, 1)] + good[7:], '4-byte')
        refused(good[:6] + [good[0]] + good[7:], 'out overlaps init01')
        refused(good[:6] + [p(0, 188)] + good[7:], 'out overlaps init01')          # the last float of init
        refused([p(4, 188)] + good[1:], 'out overlaps init01')                      # init begins on the last float of out
    # exactly one noise source
    refused([p(0), None, None, None, 0.6, 0.8, p(4), 2, 24], 'no noise source')
    refused([p(0), None, p(2), None, 0.6, 0.8, p(4), 2, 24], 'no noise source')
    refused([p(0), None, None, p(3), 0.6, 0.8, p(4), 2, 24], 'no noise source')
    refused([p(0), p(1), p(2), p(3), 0.6, 0.8, p(4), 2, 24], 'two noise sources')
    refused([p(0), p(1), p(2), None, 0.6, 0.8, p(4), 2, 24], 'two noise sources')
    refused([p(0), p(1), None, p(3), 0.6, 0.8, p(4), 2, 24], 'two noise sources')
    # the noise: misaligned, overlapped in part (in place means out == noise, which only a launch can answer: the GPU test)
    refused(given[:1] + [p(1, 2)] + given[2:], '4-byte')
    refused(given[:6] + [p(1, 16)] + given[7:], 'in part')
    refused(given[:6] + [p(1, 188)] + given[7:], 'in part')
    refused(given[:1] + [p(4, 4)] + given[2:], 'in part')
    # the keyed arm's words
    refused(keyed[:2] + [p(2, 4)] + keyed[3:], '8-byte')
    refused(keyed[:3] + [p(3, 4)] + keyed[4:], '8-byte')
    refused(keyed[:3] + [p(4, 8)] + keyed[4:], 'sample_ids or state')
    refused(keyed[:2] + [p(4, 184)] + keyed[3:], 'sample_ids or state')
    assert n == 2 * (2 + 7 + 6 + 2 + 3) + 6 + 4 + 4


# ------------------------------------------------------------------------------------------ the CLI
def test_cli_flag_parses_and_the_docstring_warns_about_synthetic_conditions():
    src = open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    doc = src.split('"""')[1]
    assert '[--strength 0.5]' in doc.split('\n\n')[1]         # the usage line
    para = [p for p in doc.split('  * ') if p.startswith('--strength')]
    assert len(para) == 1 and 'SyntheticConditions' in para[0] and 'noised black pair' in para[0] and '--conditions' in para[0]
    head = src[:src.index('args = parser.parse_args()')]
    head = head[head.index('parser = argparse.ArgumentParser()'):]
    ns = {}
    exec('import argparse\n' + head, ns)                     # the parser alone (the script's imports need the built package)
    p = ns['parser']
    assert p.parse_args([]).strength is None                  # off by default
    assert p.parse_args(['--strength', '0.5']).strength == 0.5
    a = p.parse_args(['--strength', '1', '--keep', 'source'])
    assert a.strength == 1. and a.keep == 'source'
    for bad in (['--strength'], ['--strength', 'half']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert 'trainer.keep, sampler.known_resample = args.keep, args.known_resample' in src
    assert 'trainer.strength = args.strength' in src
