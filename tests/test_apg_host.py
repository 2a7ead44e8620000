"""CPU: the host side of adaptive projected guidance (``apg_eta``, ``apg_norm_threshold``, ``apg_momentum``): the switch and its
check, the two refused combinations, the loops' dispatch (None or cond_scale == 1 makes none of the new calls), the capture key,
the CLI flags, the float64 statement of tests/apg_cases.py with its identities and the condition its ulp gate assumes, and the
argument validation of the new entry points."""
import os
import subprocess
import sys

import pytest
import torch

import apg_cases as AC
import guidance_cases as GC
from test_guidance_host import _diffusion, _run_loop, _stub_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ('apg_workspace', 'apg_coef', 'apg_coef_dev', 'apg_apply')
NEW_ENTRY_POINTS = ('dmh_apg_splits', 'dmh_apg_coef', 'dmh_apg_coef_dev', 'dmh_apg_apply')


# ------------------------------------------------------------------------------------------ the switch
def test_default_is_off_and_the_check_accepts_and_refuses():
    d = _diffusion()
    assert d.apg_eta is None and d.apg_norm_threshold == 0. and d.apg_momentum == 0. and d._check_apg() is None
    for eta in (0, 0., 0.5, 1, 1.):
        for rho in (0, 0., 2.5, 1e9):
            for beta in (0, 0., -0.5, 0.999, -0.999):
                d.apg_eta, d.apg_norm_threshold, d.apg_momentum = eta, rho, beta
                assert d._check_apg() == (float(eta), float(rho), float(beta))
                assert d._apg_on(3.) == d._check_apg() and d._apg_on(1.) is None and d._apg_on(1) is None
    for name, good, bad in (('apg_eta', 0.5, (-0.1, 1.0000001, 2, float('nan'), float('inf'), '0.5', True, [0.5])),
                            ('apg_norm_threshold', 0., (-1e-9, -1, float('nan'), float('inf'), None, '1', True)),
                            ('apg_momentum', 0., (-1, 1, 1., -1., 1.5, float('nan'), float('inf'), None, '0', True))):
        d.apg_eta, d.apg_norm_threshold, d.apg_momentum = 0.5, 0., 0.
        for v in bad:
            setattr(d, name, v)
            with pytest.raises(ValueError, match=name):
                d._check_apg()
        setattr(d, name, good)
        assert d._check_apg() is not None
    # the other two are checked while the switch is off too: a typo does not wait for the day it is switched on
    d.apg_eta, d.apg_momentum = None, 2.
    with pytest.raises(ValueError, match='apg_momentum'):
        d._check_apg()


def test_the_unconditional_class_does_not_have_the_switch():
    from dmhomo_amd import ddpm
    assert not hasattr(ddpm.GaussianDiffusion, 'apg_eta') and not hasattr(ddpm.GaussianDiffusion, '_check_apg')


def _loop_args(d, cond_scale=3.):
    B, S = 2, d.image_size
    return (torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)),
            (B, d.channels, S, S), cond_scale)


@pytest.mark.parametrize('other, value', [('guidance_rescale', 0.7), ('guidance_interval', (0.25, 0.75))])
def test_refused_combinations_name_both_settings(other, value):
    """in the check itself and in front of the first launch of every loop (no GPU here: the loops raise before they draw)"""
    d = _diffusion()
    d.apg_eta = 0.
    setattr(d, other, value)
    with pytest.raises(ValueError, match=f'apg_eta.*{other}'):
        d._check_apg()
    for loop in (d._ddim_sample, d._dpmpp_sample, d._sample_graphed):
        with pytest.raises(ValueError, match=f'apg_eta.*{other}'):
            loop(*_loop_args(d))
    d.apg_eta = None                                          # off: the other setting is on its own again
    assert d._check_apg() is None


# ------------------------------------------------------------------------------------------ the loops' dispatch
def _stub_apg(monkeypatch, calls):
    from dmhomo_amd import ops

    def fake(name, result):
        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return result(*a, **k)
        monkeypatch.setattr(ops, name, f)
    fake('apg_workspace', lambda x: torch.zeros(3, dtype=torch.float64))
    fake('apg_coef', lambda step, cond, null, eta, rho, beta, **k: torch.ones((cond.shape[0], 2)))
    fake('apg_apply', lambda cond, null, coef, **k: k['out'])


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_take_the_new_path_only_with_eta_and_a_null_pass(sampler, clip_mode, monkeypatch):
    from dmhomo_amd import ops
    S = 4
    d = _diffusion(S)
    d.sampler, d.clip_mode = sampler, clip_mode
    calls = _stub_loop(d, monkeypatch)
    _stub_apg(monkeypatch, calls)
    old_step = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler] if clip_mode == 'static' else 'sampler_step_thr'
    for eta, cond_scale in ((None, 3.), (0., 1.), (0.5, 1), (None, 1.)):      # today's calls, exactly
        calls.clear()
        d.apg_eta, d.apg_norm_threshold, d.apg_momentum = eta, 2.5, -0.5
        trace = _run_loop(d, sampler, cond_scale)
        assert not any(name in calls for name in NEW_OPS), (eta, cond_scale, calls)
        assert calls[old_step] == S and all('apg' not in e for e in trace)
    # the projected path: coefficients, apply, then the existing update on (guided, no null pass, no keep)
    seen = []
    inner = getattr(ops, old_step)

    def spy(step, cond, null, *a, **k):
        seen.append((cond, null, k.get('keep')))
        return inner(step, cond, null, *a, **k)
    monkeypatch.setattr(ops, old_step, spy)
    for beta in (0., -0.5):
        calls.clear()
        seen.clear()
        d.apg_eta, d.apg_norm_threshold, d.apg_momentum = 0., 2.5, beta
        trace = _run_loop(d, sampler, 3.)
        assert calls == {'apg_workspace': 1, 'apg_coef': S, 'apg_apply': S, old_step: S,
                         **({'sampler_threshold': S} if clip_mode == 'dynamic' else {})}, calls
        assert len(trace) == S and all(e['apg'].shape == (2, 2) for e in trace)
        assert len(seen) == S and all(null is None and keep is None for _, null, keep in seen)
        assert len({id(cond) for cond, _, _ in seen}) == 1          # the one guided buffer of the loop
    d.apg_eta = 1.5
    with pytest.raises(ValueError, match='apg_eta'):
        _run_loop(d, sampler, 3.)


def test_capture_key_carries_the_three_values_only_when_on(monkeypatch):
    d = _diffusion()
    keys = []

    def fake_replay(shape, device, key, tables, buffers, fill):
        keys.append(tuple(key))
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    d._sample_graphed(*_loop_args(d))                         # 0: the default
    d.apg_norm_threshold, d.apg_momentum = 2.5, -0.5          # 1: the switch is off: the other two change nothing
    d._sample_graphed(*_loop_args(d))
    d.apg_eta = 0.                                            # 2, 3: on
    d._sample_graphed(*_loop_args(d))
    d.apg_eta = 0.5
    d._sample_graphed(*_loop_args(d))
    d._sample_graphed(*_loop_args(d, 1.))                     # 4, 5: cond_scale 1: no null pass, nothing to project
    d.apg_eta = None
    d._sample_graphed(*_loop_args(d, 1.))
    assert keys[0] == keys[1] and keys[0][-1] == 0.           # (the default key still ends with guidance_rescale)
    assert keys[2] == keys[0] + (('apg', 0., 2.5, -0.5),) and keys[3] == keys[0] + (('apg', 0.5, 2.5, -0.5),)
    assert keys[4] == keys[5] and 'apg' not in str(keys[4])


def test_cli_flags_parse():
    src = open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    for flag in ('--apg_eta', '--apg_norm_threshold', '--apg_momentum'):
        assert flag in src.split('"""')[1]                    # listed among the additions in the docstring
    head = src[:src.index('args = parser.parse_args()')]
    head = head[head.index('parser = argparse.ArgumentParser()'):]
    ns = {}
    exec('import argparse\n' + head, ns)                     # the parser alone (the script's imports need the built package)
    p = ns['parser']
    a = p.parse_args([])
    assert a.apg_eta is None and a.apg_norm_threshold == 0. and a.apg_momentum == 0.
    a = p.parse_args(['--apg_eta', '0', '--apg_norm_threshold', '15', '--apg_momentum', '-0.5'])
    assert (a.apg_eta, a.apg_norm_threshold, a.apg_momentum) == (0., 15., -0.5) and a.apg_eta is not None
    for bad in (['--apg_eta'], ['--apg_eta', 'x'], ['--apg_momentum', 'a']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert 'sampler.apg_eta, sampler.apg_norm_threshold, sampler.apg_momentum = ' in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'dgm_sample.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--apg_eta' in r.stdout and '--apg_momentum' in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------ the statement and the case table
def _restated_splits(B, n):
    """dmh_apg_splits as apg.hip states it: one workgroup per 4096 elements of a row, at most 1024 in all"""
    return min((n + 4095) // 4096, max(1024 // B, 1))


def _inputs(B=3, n=1536, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((B, n), generator=gen) * 1.5, torch.randn((B, n), generator=gen) * 1.5


def test_statement_is_cfg_at_eta_1():
    cond, null = _inputs()
    c, d = AC.update32(cond, null, None)
    coef, s, p = AC.coef_ref(c, d, 3., 1., 0.)
    assert coef[:, 0].tolist() == [1.] * 3 and coef[:, 1].tolist() == [2.] * 3 and s.tolist() == [1.] * 3
    cfg = null.double() + (cond.double() - null.double()) * 3.
    # (d is formed in fp32: 2^-24 of it per element, times w - 1; the identity itself holds to 1e-12 on float64 d)
    exact = coef[:, :1] * cond.double() + coef[:, 1:] * (cond.double() - null.double())
    assert float((exact - cfg).abs().max()) <= 1e-12
    assert float((AC.guided_ref(c, d, coef) - cfg).abs().max()) <= 2. * 2. ** -24 * float(d.abs().max())


def test_statement_at_eta_0_is_orthogonal_to_c():
    cond, null = _inputs(seed=4)
    for keep in (None, torch.tensor([1, 0, 1], dtype=torch.uint8)):
        c, d = AC.update32(cond, null, keep)
        coef, _, _ = AC.coef_ref(c, d, 3., 0., 0.)
        upd = AC.guided_ref(c, d, coef) - c.double()
        dot = (upd * c.double()).sum(dim=1).abs()
        assert bool((dot <= 1e-9 * c.double().norm(dim=1) * upd.norm(dim=1)).all()), dot
        if keep is not None:
            assert coef[1].tolist() == [1., 2.] and bool((upd[1] == 0.).all())      # the dropped row: d == 0, guided == c


def test_statement_with_a_small_rho_caps_the_update():
    cond, null = _inputs(seed=5)
    c, d = AC.update32(cond, null, None)
    for eta in (1., 0.25):
        rho = 0.125
        coef, s, _ = AC.coef_ref(c, d, 3., eta, rho)
        assert bool((s < 0.01).all())
        upd = AC.guided_ref(c, d, coef) - c.double()
        if eta == 1.:                                         # the whole update survives: its norm is (w - 1) * rho
            assert float((upd.norm(dim=1) - 2. * rho).abs().max()) <= 1e-12
        else:                                                 # a part of it was projected away
            assert bool((upd.norm(dim=1) < 2. * rho).all())
    coef, s, _ = AC.coef_ref(c, d, 3., 1., 1e6)
    assert s.tolist() == [1.] * 3 and coef[:, 1].tolist() == [2.] * 3


def test_statement_momentum_nan_and_zero_rows():
    cond, null = _inputs(seed=6)
    run = torch.zeros_like(null)
    c, r1 = AC.update32(cond, null, None, -0.5, run)
    assert torch.equal(r1, cond - null)                       # the first step: the average starts at zero
    c, r2 = AC.update32(cond, null, None, -0.5, r1)
    assert torch.equal(r2, (cond - null) + torch.tensor(-0.5) * r1)
    dirty = cond.clone()
    dirty[1, 7] = float('nan')
    coef, _, _ = AC.coef_ref(*AC.update32(dirty, null, None), 3., 0.25, 2.)
    clean, _, _ = AC.coef_ref(*AC.update32(cond, null, None), 3., 0.25, 2.)
    assert bool(torch.isnan(coef[1]).all()) and torch.equal(coef[[0, 2]], clean[[0, 2]])
    dirty[1, 7] = float('inf')
    coef, _, _ = AC.coef_ref(*AC.update32(dirty, null, None), 3., 0.25, 2.)
    assert bool(torch.isnan(coef[1]).all()) and torch.equal(coef[[0, 2]], clean[[0, 2]])
    zero = torch.zeros_like(cond)
    coef, _, p = AC.coef_ref(*AC.update32(zero, null, None), 3., 0.25, 0.)
    assert p.tolist() == [0.] * 3 and coef[:, 0].tolist() == [1.] * 3
    u = AC.ulps(torch.tensor([1. + 2. ** -23, 3.]), torch.tensor([1., 3.], dtype=torch.float64))
    assert u.tolist() == [1., 0.]


def test_case_table_covers_what_it_claims_and_its_sums_do_not_cancel():
    """the ulp gate of the coefficients assumes |sum d*c| >= 1e-3 * sum |d*c| in every row whose coefficients are compared with the
    float64 statement: checked here for every such case, at every call"""
    ragged = tuple(AC.ragged_size(_restated_splits, B)[0] for B in AC.BATCHES)
    table = AC.cases(ragged)
    seen, worst = {}, 1.
    for name, case in table:
        cond, null = case['calls'][0]
        B, n = null.shape
        assert cond.dtype == null.dtype == torch.float32 and cond.shape == (B, n), name
        assert case['keep'] is None or (case['keep'].dtype == torch.uint8 and case['keep'].shape == (B,)), name
        assert len(case['calls']) == (3 if case['beta'] != 0. else 1)
        seen.setdefault((n, B), set()).add(case['kind'])
        refs = AC.reference(case, 'clean' if case['kind'] == 'nan' else 'calls')
        for r in refs:
            assert bool(torch.isfinite(r['coef']).all()), name
            if case['kind'] != 'czero':                       # (c == 0: Sdc is an exact 0 and p is 0 by definition)
                assert bool((r['cancel'] >= 1e-3).all()), (name, r['cancel'])
                worst = min(worst, float(r['cancel'].min()))
            if n >= 63 and case['kind'] == 'rho_bind':
                assert bool((r['s'] < 1.).all()), name
            if case['kind'] in ('rho_loose', 'normal', 'keep', 'equal'):
                assert bool((r['s'] == 1.).all()), name
            if case['kind'] == 'equal':
                assert r['coef'].tolist() == [[1., 2.]] * B and torch.equal(AC.guided32(r['c'], r['d'], r['coef']), r['c'])
            if case['kind'] == 'czero':
                assert r['coef'][:, 0].tolist() == [1.] * B and r['p'].tolist() == [0.] * B
        if n >= 63 and case['kind'] == 'momentum':            # the cap binds at some call, the average differs from the update
            assert any(bool((r['s'] < 1.).any()) for r in refs), name
    for n in AC.SIZES:
        for B in AC.BATCHES:
            assert seen[(n, B)] == set(AC.KINDS), (n, B)
    for B, n in zip(AC.BATCHES, ragged):
        s = _restated_splits(B, n)
        assert seen[(n, B)] == set(AC.KINDS) and s >= 2 and n % (4 * s) != 0 and n < AC.BIG[0]
    assert seen[AC.BIG] == {'momentum'}
    assert len(table) == (len(AC.SIZES) * len(AC.BATCHES) + len(ragged)) * len(AC.KINDS) + 1
    print(f'[parity] apg case table: {len(table)} cases, smallest |sum d*c| / sum |d*c| = {worst:.3e} (assumed >= 1e-3)')


# ------------------------------------------------------------------------------------------ the binding
def test_splits_agree_with_the_restatement_and_cut_the_workload_row():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for B in (1, 3, 25, 300, 5000):
        for n in AC.SIZES + GC.RAGGED_CANDIDATES[:8] + (98304, 393216, 2 ** 31 - 1):
            assert lib.dmh_apg_splits(B, n) == _restated_splits(B, n) == ops.apg_splits(B, n), (B, n)
    assert lib.dmh_apg_splits(25, 98304) == 24
    for B, n in ((0, 4), (-1, 4), (1, 0), (1, 2 ** 31)):
        with pytest.raises(ValueError):
            ops.apg_splits(B, n)


def test_binding_has_the_new_entry_points():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in NEW_OPS + ('apg_splits',):
        assert callable(getattr(ops, name)), name
    assert _lib.ABI_VERSION == 500                           # additions: nothing existing changed


def test_every_new_entry_point_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib, ops
    assert AC.check_einval(_lib, ops) == 4 + 2 * (6 + 5 + 4 + 3 + 6 + 2) + 5 + 3 + 3
