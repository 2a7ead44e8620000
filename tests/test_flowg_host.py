"""CPU: the host side of guidance on the flow condition (``flow_guidance``) and of the training switch ``flow_drop_prob``: the
two attributes and their checks, the refused combinations, the fp32 statement of tests/flowg_cases.py against its float64 form,
the loops' dispatch (None makes none of the new calls; on, the shift is the first call behind the network), the capture key,
the CLI flags and the argument validation of the two new entry points."""
import os
import subprocess
import sys

import pytest
import torch

import flowg_cases as FC
from test_apg_host import _stub_apg
from test_guidance_host import _diffusion, _run_loop, _stub_loop
from test_photo_host import _stub_photo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ('flow_guidance_shift', 'affine_rows_keep')
NEW_ENTRY_POINTS = ('dmh_flow_guidance_shift', 'dmh_affine_rows_keep')


# ------------------------------------------------------------------------------------------ the switches
def test_defaults_are_off_and_the_checks_accept_and_refuse():
    from dmhomo_amd import cfg
    d = _diffusion()
    assert cfg.GaussianDiffusion.flow_guidance is None and cfg.GaussianDiffusion.flow_drop_prob == 0.
    assert d._check_flow_guidance() is None and d._check_flow_drop_prob() == 0.
    for s in (0, 0., 0.5, 1, 1., 2, 7.5, 1e9):
        d.flow_guidance = s
        assert d._check_flow_guidance() == float(s) - 1.
    for s in (-1e-9, -1, float('nan'), float('inf'), float('-inf'), '2', True, False, [2.], (1., 2.)):
        d.flow_guidance = s
        with pytest.raises(ValueError, match='flow_guidance'):
            d._check_flow_guidance()
    d.flow_guidance = None
    for p in (0, 0., 0.1, 0.5, 0.999):
        d.flow_drop_prob = p
        assert d._check_flow_drop_prob() == float(p)
    for p in (-1e-9, -1, 1, 1., 1.5, float('nan'), float('inf'), None, '0.1', True, False, [0.1]):
        d.flow_drop_prob = p
        with pytest.raises(ValueError, match='flow_drop_prob'):
            d._check_flow_drop_prob()


def test_the_unconditional_class_does_not_have_the_switches():
    from dmhomo_amd import ddpm
    for name in ('flow_guidance', '_check_flow_guidance', 'flow_drop_prob', '_check_flow_drop_prob'):
        assert not hasattr(ddpm.GaussianDiffusion, name), name


def _loop_args(d, cond_scale=3.):
    B, S = 2, d.image_size
    return (torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)),
            (B, d.channels, S, S), cond_scale)


@pytest.mark.parametrize('cond_scale', [3., 1.])
def test_guidance_interval_is_refused_beside_the_switch(cond_scale):
    """in the check itself and in front of the first launch of every loop (no GPU here: the loops raise before they draw)"""
    d = _diffusion()
    d.flow_guidance, d.guidance_interval = 2., (0.25, 0.75)
    with pytest.raises(ValueError, match='flow_guidance.*guidance_interval'):
        d._check_flow_guidance()
    for loop in (d._ddim_sample, d._dpmpp_sample, d._sample_graphed):
        with pytest.raises(ValueError, match='flow_guidance.*guidance_interval'):
            loop(*_loop_args(d, cond_scale))
    d.flow_guidance = None                                    # off: the interval is on its own again
    assert d._check_flow_guidance() is None


@pytest.mark.parametrize('cond_scale', [3., 1.])
def test_streams_mode_is_refused_beside_the_switch(cond_scale):
    d = _diffusion()
    d.flow_guidance, d.model.cfg_mode = 2., 'streams'
    with pytest.raises(ValueError, match="flow_guidance.*'streams'"):
        d._check_flow_guidance()
    for loop in (d._ddim_sample, d._dpmpp_sample, d._sample_graphed):
        with pytest.raises(ValueError, match="flow_guidance.*'streams'"):
            loop(*_loop_args(d, cond_scale))
    x = torch.zeros((2, 6, 8, 8))
    with pytest.raises(ValueError, match="flow_guidance.*'streams'"):         # the network method itself refuses too
        d.model._cond_null_noflow(x, torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), x[:, :3], x[:, :1],
                                  cond_scale)
    d.flow_guidance = None
    assert d._check_flow_guidance() is None


# ------------------------------------------------------------------------------------------ the statement
def test_fp32_statement_agrees_with_float64_within_one_rounding_per_operation():
    """e = w * (b - u) and x' = x + e.  The fp32 difference is exact to half an ulp of itself, the product adds half an ulp of
    e: |e32 - e64| <= 2^-24 * (|w| * |b - u| + |e|) (the first term: the difference's rounding carried through the product);
    the sum adds half an ulp of the result: |x'32 - x'64| <= |e32 - e64| + 2^-24 * |x'|."""
    h = 2. ** -24
    n_checked = 0
    for name, case in FC.cases():
        cond, null, uncond, keep, w = (case[k] for k in ('cond', 'null', 'uncond', 'keep', 'w'))
        c32, n32 = FC.shift32(cond, null, uncond, w, keep)
        c64, n64, e64 = FC.shift64(cond, null, uncond, w, keep)
        b = cond if null is None else null
        tol_e = h * (abs(w) * (b.double() - uncond.double()).abs() + e64.abs())
        tol_e = tol_e * (1. + 2. * h) + 1e-45                 # (the bound is stated on exact values, checked on rounded ones)
        pairs = [(n32, n64)] if null is not None else []
        rows = torch.ones(cond.shape[0], dtype=torch.bool) if keep is None else keep.bool()
        if bool(rows.any()):
            pairs.append((c32[rows], c64[rows]))
            tol_rows = tol_e[rows]
        for i, (x32, x64) in enumerate(pairs):
            tol = (tol_e if (null is not None and i == 0) else tol_rows) + h * x64.abs() * (1. + 2. * h)
            assert bool(((x32.double() - x64).abs() <= tol).all()), name
            n_checked += x32.numel()
        if keep is not None and not bool(rows.all()):        # the dropped rows: the bits they had
            assert torch.equal(c32[~rows].view(torch.int32), cond[~rows].view(torch.int32)), name
    assert n_checked > 100000


def test_statement_identities():
    cond, null, uncond = FC.inputs(3, 1536, 7)
    # w == 0 (flow_guidance = 1): every value as it was
    c, n = FC.shift32(cond, null, uncond, 0.)
    assert torch.equal(c, cond) and torch.equal(n, null)
    assert torch.equal(FC.shift32(cond, None, uncond, 0.)[0], cond)
    # a sample without flow information: n == u bitwise, e == 0 whatever w is
    c, n = FC.shift32(cond, null, null.clone(), 2.5)
    assert torch.equal(c, cond) and torch.equal(n, null)
    # w == -1 (flow_guidance = 0): the no-flow logits themselves, up to the rounding of (b - u)
    c, _ = FC.shift32(cond, None, uncond, -1.)
    assert float((c - uncond).abs().max()) <= 2. ** -23 * float(cond.abs().max() + uncond.abs().max())
    # the two-scale form in float64: null' + (cond' - null') * s_c == u + s_f * (n - u) + s_c * (c - n)
    c64, n64, _ = FC.shift64(cond, null, uncond, 1.)
    two = uncond.double() + 2. * (null.double() - uncond.double()) + 3. * (cond.double() - null.double())
    assert float((n64 + (c64 - n64) * 3. - two).abs().max()) <= 1e-12
    # affine_keep32: kept rows are the affine, dropped rows +0.0 (sign bit clear)
    keep = torch.tensor([1, 0, 1], dtype=torch.uint8)
    y = FC.affine_keep32(cond, 2., -1., keep)
    assert torch.equal(y[[0, 2]], cond[[0, 2]] * 2. - 1.) and bool((y[1].view(torch.int32) == 0).all())


def test_case_table_covers_what_it_claims():
    table = FC.cases()
    assert len(table) == len(FC.SIZES) * len(FC.BATCHES) * 4
    seen = {}
    for name, case in table:
        B, n = case['uncond'].shape
        kind = 'B' if case['null'] is None else ('none' if case['keep'] is None else ('zero' if not bool(case['keep'].any())
                                                                                       else 'mixed'))
        seen.setdefault((n, B), set()).add(kind)
        assert case['cond'].shape == (B, n) and case['cond'].dtype == torch.float32
        if case['keep'] is not None:
            dropped = ~case['keep'].bool()
            assert bool(torch.isnan(case['cond'][dropped]).all()) and bool(torch.isfinite(case['cond'][~dropped]).all())
    assert all(seen[(n, B)] == {'B', 'none', 'zero', 'mixed'} for n in FC.SIZES for B in FC.BATCHES)
    assert any(n % 4 for n in FC.SIZES) and any(n > 256 * 4 for n in FC.SIZES) and FC.BIG == (25, 6 * 128 * 128)
    assert (0, 0, 0) in FC.PHASES and any(len(set(p)) == 1 and p[0] for p in FC.PHASES) and any(len(set(p)) == 3 for p in FC.PHASES)


# ------------------------------------------------------------------------------------------ the loops' dispatch
def _fake_noflow(calls):
    def fake(x, t, classes, rgb_flow, mask, cs):
        calls['_cond_null_noflow'] = calls.get('_cond_null_noflow', 0) + 1
        return torch.zeros_like(x), (None if cs == 1 else torch.zeros_like(x)), torch.zeros_like(x), None
    return fake


def _ordered(monkeypatch, names, order):
    from dmhomo_amd import ops
    for name in names:
        inner = getattr(ops, name)

        def f(*a, _inner=inner, _name=name, **k):
            order.append(_name)
            return _inner(*a, **k)
        monkeypatch.setattr(ops, name, f)


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_off_is_todays_calls_and_on_puts_the_shift_first(sampler, clip_mode, monkeypatch):
    from dmhomo_amd import ops
    S = 4
    d = _diffusion(S)
    d.sampler, d.clip_mode = sampler, clip_mode
    calls = _stub_loop(d, monkeypatch)                        # (its _network takes today's six positional arguments, no more)
    _stub_apg(monkeypatch, calls)
    _stub_photo(monkeypatch, calls)
    monkeypatch.setattr(d.model, '_cond_null_noflow', _fake_noflow(calls))
    monkeypatch.setattr(ops, 'flow_guidance_shift',
                        lambda cond, null, uncond, w, keep=None: calls.__setitem__('flow_guidance_shift',
                                                                                   calls.get('flow_guidance_shift', 0) + 1))
    six = []
    network = d._network
    monkeypatch.setattr(d, '_network', lambda *a: (six.append(len(a)), network(*a))[1])
    old_step = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler] if clip_mode == 'static' else 'sampler_step_thr'
    for cond_scale in (3., 1.):                               # off: the network through _network, none of the new calls
        calls.clear(), six.clear()
        trace = _run_loop(d, sampler, cond_scale)
        assert six == [6] * S and '_cond_null_noflow' not in calls and 'flow_guidance_shift' not in calls
        assert calls[old_step] == S and all('flow' not in e for e in trace)
    order = []
    _ordered(monkeypatch, ('flow_guidance_shift', 'apg_coef', 'apg_apply', 'photo_guide', 'guidance_factor', 'sampler_threshold',
                           'sampler_threshold_gr', 'sampler_step', 'sampler_step_ms', 'sampler_step_thr', 'sampler_step_gr'), order)
    settings = ({}, {'guidance_rescale': 0.7}, {'apg_eta': 0., 'apg_momentum': -0.5}, {'photo_guidance': 0.5})
    for extra in settings:
        for cond_scale in (3., 1.):
            d.flow_guidance = 2.
            for k, v in extra.items():
                setattr(d, k, v)
            calls.clear(), six.clear(), order.clear()
            trace = _run_loop(d, sampler, cond_scale)
            assert six == [] and calls['_cond_null_noflow'] == S and calls['flow_guidance_shift'] == S, (extra, calls)
            assert len(trace) == S and all(e['flow'] is True for e in trace)
            per_step = len(order) // S
            assert len(order) == per_step * S and per_step >= 2
            for k in range(S):                                # the shift: once per step, in front of everything else
                chunk = order[k * per_step:(k + 1) * per_step]
                assert chunk[0] == 'flow_guidance_shift' and chunk.count('flow_guidance_shift') == 1, (extra, chunk)
            if cond_scale != 1:
                for name in {'guidance_rescale': ('guidance_factor',), 'apg_eta': ('apg_coef', 'apg_apply'),
                             'photo_guidance': ('photo_guide',)}.get(next(iter(extra), None), ()):
                    assert calls[name] == S, (extra, calls)
            for k in extra:
                setattr(d, k, getattr(type(d), k))
    d.flow_guidance = -1.
    with pytest.raises(ValueError, match='flow_guidance'):
        _run_loop(d, sampler, 3.)


def test_the_shift_gets_w_and_the_computed_rows(monkeypatch):
    from dmhomo_amd import ops
    d = _diffusion()
    _stub_loop(d, monkeypatch)
    keep = torch.tensor([1, 0], dtype=torch.uint8)
    outs = []

    def noflow(x, t, classes, rgb_flow, mask, cs):
        outs.append((torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), keep))
        return outs[-1]
    seen = []
    monkeypatch.setattr(d.model, '_cond_null_noflow', noflow)
    monkeypatch.setattr(ops, 'flow_guidance_shift', lambda cond, null, uncond, w, keep=None: seen.append((cond, null, uncond, w, keep)))
    d.flow_guidance = 2.5
    _run_loop(d, 'ddim', 3.)
    assert len(seen) == 4
    for got, out in zip(seen, outs):
        assert got[0] is out[0] and got[1] is out[1] and got[2] is out[2] and got[3] == 1.5 and got[4] is keep


def test_capture_key_carries_w_only_when_on(monkeypatch):
    d = _diffusion()
    keys = []

    def fake_replay(shape, device, key, tables, buffers, fill):
        keys.append(tuple(key))
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    d._sample_graphed(*_loop_args(d))                         # 0: the default
    d.flow_drop_prob = 0.3                                    # 1: the training switch is not the sampler's business
    d._sample_graphed(*_loop_args(d))
    d.flow_guidance = 2.                                      # 2, 3: on
    d._sample_graphed(*_loop_args(d))
    d.flow_guidance = 1
    d._sample_graphed(*_loop_args(d))
    d._sample_graphed(*_loop_args(d, 1.))                     # 4: on at cond_scale 1 (case B)
    d.flow_guidance = None
    d._sample_graphed(*_loop_args(d, 1.))                     # 5: off at cond_scale 1
    d._sample_graphed(*_loop_args(d))                         # 6: off again: the default's key
    assert keys[0] == keys[1] == keys[6] and keys[0][-1] == 0.           # (the default key still ends with guidance_rescale)
    assert keys[2] == keys[0] + (('flow_guidance', 1.),) and keys[3] == keys[0] + (('flow_guidance', 0.),)
    assert keys[4] == keys[5] + (('flow_guidance', 0.),) and 'flow_guidance' not in str(keys[5])


def test_cli_flags_parse():
    for script, flag, default, given in (('dgm_sample.py', '--flow_guidance', None, 2.), ('demo.py', '--flow_drop_prob', 0., 0.1)):
        src = open(os.path.join(ROOT, 'scripts', script)).read()
        assert flag in src.split('"""')[1]                    # listed among the additions in the docstring
        head = src[:src.index('args = parser.parse_args()')]
        head = head[head.index('parser = argparse.ArgumentParser()'):]
        ns = {}
        exec('import argparse\n' + head, ns)                 # the parser alone (the script's imports need the built package)
        p = ns['parser']
        assert getattr(p.parse_args([]), flag[2:]) == default
        assert getattr(p.parse_args([flag, str(given)]), flag[2:]) == given
        for bad in ([flag], [flag, 'x']):
            with pytest.raises(SystemExit):
                p.parse_args(bad)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script), '--help'], capture_output=True, text=True)
        assert r.returncode == 0 and flag in r.stdout, r.stderr[-2000:]
    assert 'sampler.flow_guidance = args.flow_guidance' in open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    assert 'diffusion.flow_drop_prob = args.flow_drop_prob' in open(os.path.join(ROOT, 'scripts', 'demo.py')).read()


# ------------------------------------------------------------------------------------------ the binding
def test_binding_has_the_new_entry_points():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in NEW_OPS:
        assert callable(getattr(ops, name)), name
    assert _lib.ABI_VERSION == 500                           # additions: nothing existing changed


def test_every_new_entry_point_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib
    assert FC.check_einval(_lib) == FC.N_EINVAL


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    from dmhomo_amd import _lib, ops
    x = torch.zeros((2, 8))
    keep = torch.ones(2, dtype=torch.uint8)
    with pytest.raises(_lib.DmhError):                       # there is no CPU path
        ops.flow_guidance_shift(x, None, x.clone(), 1.)
    with pytest.raises(_lib.DmhError):
        ops.affine_rows_keep(x, 2., -1., keep)
    for args, kw in (((x, None, x[:1], 1.), {}), ((x, x[:1], x.clone(), 1.), {}), ((x, None, x.clone(), 1.), {'keep': keep}),
                     ((x, x.clone(), x.clone(), 1.), {'keep': keep[:1]}), ((x, x.clone(), x.clone(), 1.), {'keep': keep.bool()}),
                     ((x, None, x.clone(), float('nan')), {}), ((x, None, x.clone(), float('inf')), {})):
        with pytest.raises(ValueError, match='flow_guidance_shift'):
            ops.flow_guidance_shift(*args, **kw)
    for args, kw in (((x, 2., -1., None), {}), ((x, 2., -1., keep[:1]), {}), ((x, 2., -1., keep.float()), {}),
                     ((x, 2., -1., keep), {'out': x[:1]})):
        with pytest.raises(ValueError, match='affine_rows_keep'):
            ops.affine_rows_keep(*args, **kw)
