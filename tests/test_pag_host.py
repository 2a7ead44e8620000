"""CPU: the host side of perturbed-attention guidance (``pag_scale``): the attribute and its check, the refused combinations,
the fp32 statement of tests/pag_cases.py against its float64 form, the loops' dispatch (None makes none of the new calls; on, the
shift is the first call behind the network, once per step), the capture key, the CLI flag and the argument validation of the two
new entry points."""
import os
import subprocess
import sys

import pytest
import torch

import pag_cases as PC
from test_apg_host import _stub_apg
from test_guidance_host import _diffusion, _run_loop, _stub_loop
from test_photo_host import _stub_photo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ('dmh_attention_pag', 'dmh_pag_shift')


# ------------------------------------------------------------------------------------------ the switch
def test_default_is_off_and_the_check_accepts_and_refuses():
    from dmhomo_amd import cfg, sampling
    d = _diffusion()
    assert cfg.GaussianDiffusion.pag_scale is None and sampling.ScheduleHost.pag_scale is None
    assert d._check_pag() is None
    for s in (0, 0., 0.5, 1, 2.5, 3, 1e9):
        d.pag_scale = s
        got = d._check_pag()
        assert got == float(s) and type(got) is float
    for s in (-1e-9, -1, float('nan'), float('inf'), float('-inf'), '2', True, False, [2.], (1., 2.)):
        d.pag_scale = s
        with pytest.raises(ValueError, match='pag_scale'):
            d._check_pag()
    d.pag_scale = None
    assert d._check_pag() is None


def _loop_args(d, cond_scale=3.):
    B, S = 2, d.image_size
    return (torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)),
            (B, d.channels, S, S), cond_scale)


def _refused_everywhere(d, cond_scale, match):
    """in the check itself and in front of the first launch of every loop (no GPU here: the loops raise before they draw)"""
    with pytest.raises(ValueError, match=match):
        d._check_pag()
    for loop in (d._ddim_sample, d._dpmpp_sample, d._sample_graphed):
        with pytest.raises(ValueError, match=match):
            loop(*_loop_args(d, cond_scale))


@pytest.mark.parametrize('cond_scale', [3., 1.])
def test_flow_guidance_is_refused_beside_the_switch(cond_scale):
    d = _diffusion()
    d.pag_scale, d.flow_guidance = 2., 2.
    _refused_everywhere(d, cond_scale, 'pag_scale.*flow_guidance')
    d.pag_scale = None                                       # off: flow_guidance is on its own again
    assert d._check_pag() is None and d._check_flow_guidance() == 1.


@pytest.mark.parametrize('cond_scale', [3., 1.])
def test_guidance_interval_is_refused_beside_the_switch(cond_scale):
    d = _diffusion()
    d.pag_scale, d.guidance_interval = 2., (0.25, 0.75)
    _refused_everywhere(d, cond_scale, 'pag_scale.*guidance_interval')
    d.pag_scale = None
    assert d._check_pag() is None


@pytest.mark.parametrize('cond_scale', [3., 1.])
def test_streams_mode_is_refused_beside_the_switch(cond_scale):
    d = _diffusion()
    d.pag_scale, d.model.cfg_mode = 2., 'streams'
    _refused_everywhere(d, cond_scale, "pag_scale.*'streams'")
    x = torch.zeros((2, 6, 8, 8))
    with pytest.raises(ValueError, match="pag_scale.*'streams'"):             # the network method itself refuses too
        d.model._cond_null_pag(x, torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), x[:, :3], x[:, :1], cond_scale)
    d.pag_scale = None
    assert d._check_pag() is None


def test_the_unconditional_class_refuses_the_switch():
    from dmhomo_amd import ddpm
    m = ddpm.Unet(dim=8, dim_mults=(1, 2), channels=3)
    d = ddpm.GaussianDiffusion(m, image_size=8, timesteps=20, sampling_timesteps=4)
    assert d.pag_scale is None
    for s in (2., 0.):
        d.pag_scale = s
        with pytest.raises(ValueError, match='pag_scale is not available in the unconditional class'):
            d.sample(batch_size=1)


# ------------------------------------------------------------------------------------------ the statement
def test_fp32_statement_agrees_with_float64_within_one_rounding_per_operation():
    """e = s * (c - p) and x' = x + e.  The fp32 difference is exact to half an ulp of itself, the product adds half an ulp of
    e: |e32 - e64| <= 2^-24 * (s * |c - p| + |e|); the sum adds half an ulp of the result: |x'32 - x'64| <= |e32 - e64| +
    2^-24 * |x'| — a few ulp of the largest value."""
    h = 2. ** -24
    n_checked = 0
    for name, case in PC.cases():
        cond, null, pert, keep, s = (case[k] for k in ('cond', 'null', 'pert', 'keep', 's'))
        c32, n32 = PC.shift32(cond, null, pert, s, keep)
        c64, n64, e64 = PC.shift64(cond, null, pert, s, keep)
        tol_e = h * 2. * e64.abs() * (1. + 2. * h) + 1e-45    # (s * |c - p| == |e| in float64)
        rows = torch.ones(cond.shape[0], dtype=torch.bool) if keep is None else keep.bool()
        pairs = [(n32, n64, tol_e)] if null is not None else []
        if bool(rows.any()):
            pairs.append((c32[rows], c64[rows], tol_e[rows]))
        for x32, x64, te in pairs:
            assert bool(torch.isfinite(x32).all()), name
            assert bool(((x32.double() - x64).abs() <= te + h * x64.abs() * (1. + 2. * h)).all()), name
            n_checked += x32.numel()
        if keep is not None and not bool(rows.all()):        # the dropped rows: the bits they had
            assert torch.equal(c32[~rows].view(torch.int32), cond[~rows].view(torch.int32)), name
    assert n_checked > 100000


def test_statement_identities():
    cond, null, pert = PC.FC.inputs(3, 1536, 7)
    keep = torch.tensor([1, 0, 1], dtype=torch.uint8)
    # s == 0: every value as it was (==: e is a zero of either sign)
    for kp in (None, keep):
        c, n = PC.shift32(cond, null, pert, 0., kp)
        assert bool((c == cond).all()) and bool((n == null).all())
    assert bool((PC.shift32(cond, None, pert, 0.)[0] == cond).all())
    # cond == pert (the perturbation changed nothing): e == +0.0, every value bitwise
    c, n = PC.shift32(cond, null, cond.clone(), 3.)
    assert torch.equal(c.view(torch.int32), cond.view(torch.int32)) and torch.equal(n.view(torch.int32), null.view(torch.int32))
    c, _ = PC.shift32(cond, None, cond.clone(), 3.)
    assert torch.equal(c.view(torch.int32), cond.view(torch.int32))
    # rows with keep == 0: null is the base of e, cond is untouched (NaN: never computed)
    cn = cond.clone()
    cn[1] = float('nan')
    c, n = PC.shift32(cn, null, pert, 3., keep)
    assert torch.equal(c[1].view(torch.int32), cn[1].view(torch.int32))
    assert torch.equal(n[1], null[1] + torch.tensor(3.) * (null[1] - pert[1]))
    assert torch.equal(n[0], null[0] + torch.tensor(3.) * (cond[0] - pert[0]))
    assert torch.equal(c[[0, 2]], cond[[0, 2]] + torch.tensor(3.) * (cond[[0, 2]] - pert[[0, 2]]))
    # the blend in float64: null' + (cond' - null') * s_c == n + s_c * (c - n) + s * (c - p)
    c64, n64, _ = PC.shift64(cond, null, pert, 2.5)
    want = null.double() + 3. * (cond.double() - null.double()) + 2.5 * (cond.double() - pert.double())
    assert float((n64 + (c64 - n64) * 3. - want).abs().max()) <= 1e-12


def test_case_tables_cover_what_they_claim():
    table = PC.cases()
    assert len(table) == len(PC.SIZES) * len(PC.BATCHES) * 4
    seen, scales = {}, {}
    for name, case in table:
        B, n = case['pert'].shape
        kind = 'B' if case['null'] is None else ('none' if case['keep'] is None else ('zero' if not bool(case['keep'].any())
                                                                                       else 'mixed'))
        seen.setdefault((n, B), set()).add(kind)
        scales.setdefault(kind, set()).add(case['s'])
        if case['keep'] is not None:
            dropped = ~case['keep'].bool()
            assert bool(torch.isnan(case['cond'][dropped]).all()) and bool(torch.isfinite(case['cond'][~dropped]).all())
    assert all(seen[(n, B)] == {'B', 'none', 'zero', 'mixed'} for n in PC.SIZES for B in PC.BATCHES)
    assert all(scales[k] == set(PC.SCALES) for k in ('B', 'none', 'zero', 'mixed')) and PC.SCALES == (0., 0.5, 3.)
    assert any(n % 4 for n in PC.SIZES) and any(n < 4 for n in PC.SIZES) and PC.BIG == (25, 6 * 128 * 128)
    assert PC.ATTN_B == 3 and PC.ATTN_NS == (1, 31, 32, 33, 64, 65, 256) and PC.ATTN_ROWS == (None, (0, 2))


# ------------------------------------------------------------------------------------------ the loops' dispatch
def _fake_pag(calls):
    def fake(x, t, classes, rgb_flow, mask, cs):
        calls['_cond_null_pag'] = calls.get('_cond_null_pag', 0) + 1
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
    monkeypatch.setattr(d.model, '_cond_null_pag', _fake_pag(calls))
    monkeypatch.setattr(ops, 'pag_shift',
                        lambda cond, null, pert, s, keep=None: calls.__setitem__('pag_shift', calls.get('pag_shift', 0) + 1))
    six = []
    network = d._network
    monkeypatch.setattr(d, '_network', lambda *a: (six.append(len(a)), network(*a))[1])
    old_step = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler] if clip_mode == 'static' else 'sampler_step_thr'
    for cond_scale in (3., 1.):                               # off: the network through _network, none of the new calls
        calls.clear(), six.clear()
        trace = _run_loop(d, sampler, cond_scale)
        assert six == [6] * S and '_cond_null_pag' not in calls and 'pag_shift' not in calls
        assert calls[old_step] == S and all('pag' not in e for e in trace)
    order = []
    _ordered(monkeypatch, ('pag_shift', 'apg_coef', 'apg_apply', 'photo_guide', 'guidance_factor', 'sampler_threshold',
                           'sampler_threshold_gr', 'sampler_step', 'sampler_step_ms', 'sampler_step_thr', 'sampler_step_gr'), order)
    settings = ({}, {'guidance_rescale': 0.7}, {'apg_eta': 0., 'apg_momentum': -0.5}, {'photo_guidance': 0.5})
    for extra in settings:
        for cond_scale in (3., 1.):
            d.pag_scale = 2.5
            for k, v in extra.items():
                setattr(d, k, v)
            calls.clear(), six.clear(), order.clear()
            trace = _run_loop(d, sampler, cond_scale)
            assert six == [] and calls['_cond_null_pag'] == S and calls['pag_shift'] == S, (extra, calls)
            assert len(trace) == S and all(e['pag'] is True for e in trace)
            per_step = len(order) // S
            assert len(order) == per_step * S and per_step >= 2
            for k in range(S):                                # the shift: once per step, in front of everything else
                chunk = order[k * per_step:(k + 1) * per_step]
                assert chunk[0] == 'pag_shift' and chunk.count('pag_shift') == 1, (extra, chunk)
            if cond_scale != 1:
                for name in {'guidance_rescale': ('guidance_factor',), 'apg_eta': ('apg_coef', 'apg_apply'),
                             'photo_guidance': ('photo_guide',)}.get(next(iter(extra), None), ()):
                    assert calls[name] == S, (extra, calls)
            for k in extra:
                setattr(d, k, getattr(type(d), k))
    d.pag_scale = -1.
    with pytest.raises(ValueError, match='pag_scale'):
        _run_loop(d, sampler, 3.)


def test_the_shift_gets_s_and_the_computed_rows(monkeypatch):
    from dmhomo_amd import ops
    d = _diffusion()
    _stub_loop(d, monkeypatch)
    keep = torch.tensor([1, 0], dtype=torch.uint8)
    outs = []

    def pag(x, t, classes, rgb_flow, mask, cs):
        outs.append((torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), keep))
        return outs[-1]
    seen = []
    monkeypatch.setattr(d.model, '_cond_null_pag', pag)
    monkeypatch.setattr(ops, 'pag_shift', lambda cond, null, pert, s, keep=None: seen.append((cond, null, pert, s, keep)))
    d.pag_scale = 2.5
    _run_loop(d, 'ddim', 3.)
    assert len(seen) == 4
    for got, out in zip(seen, outs):
        assert got[0] is out[0] and got[1] is out[1] and got[2] is out[2] and got[3] == 2.5 and got[4] is keep


def test_the_trunk_hands_pert_lo_to_the_attention_member_only():
    """UnetEngine.trunk carries pert_lo like its row list and clears it behind the pass; _attn gives it to attention_core"""
    import inspect
    from dmhomo_amd import engine, ops
    assert inspect.signature(engine.UnetEngine.trunk).parameters['pert_lo'].default is None
    assert inspect.signature(ops.attention_core).parameters['pert_lo'].default is None
    src = inspect.getsource(engine.UnetEngine._attn)
    assert src.count('pert_lo=') == 1 and 'ops.attention_core(qkv, ATTN_SCALE, rows=rows, pert_lo=self._pert_lo)' in src
    d = _diffusion()
    assert d.model._engine._pert_lo is None


def test_capture_key_carries_s_only_when_on(monkeypatch):
    d = _diffusion()
    keys = []

    def fake_replay(shape, device, key, tables, buffers, fill):
        keys.append(tuple(key))
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    d._sample_graphed(*_loop_args(d))                         # 0: the default
    d.pag_scale = 2.5                                         # 1, 2: on
    d._sample_graphed(*_loop_args(d))
    d.pag_scale = 0
    d._sample_graphed(*_loop_args(d))
    d._sample_graphed(*_loop_args(d, 1.))                     # 3: on at cond_scale 1 (case B)
    d.pag_scale = None
    d._sample_graphed(*_loop_args(d, 1.))                     # 4: off at cond_scale 1
    d._sample_graphed(*_loop_args(d))                         # 5: off again: the default's key
    assert keys[0] == keys[5] and keys[0][-1] == 0.                       # (the default key still ends with guidance_rescale)
    assert keys[1] == keys[0] + (('pag_scale', 2.5),) and keys[2] == keys[0] + (('pag_scale', 0.),)
    assert keys[3] == keys[4] + (('pag_scale', 0.),) and 'pag_scale' not in str(keys[4]) and 'pag_scale' not in str(keys[0])


def test_cli_flag_parses():
    src = open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    flag = '--pag_scale'
    assert flag in src.split('"""')[1]                        # listed among the additions in the docstring
    head = src[:src.index('args = parser.parse_args()')]
    head = head[head.index('parser = argparse.ArgumentParser()'):]
    ns = {}
    exec('import argparse\n' + head, ns)                     # the parser alone (the script's imports need the built package)
    p = ns['parser']
    assert p.parse_args([]).pag_scale is None
    assert p.parse_args([flag, '2.5']).pag_scale == 2.5
    for bad in ([flag], [flag, 'x']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'dgm_sample.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and flag in r.stdout, r.stderr[-2000:]
    assert 'sampler.pag_scale = args.pag_scale' in src


# ------------------------------------------------------------------------------------------ the binding
def test_binding_has_the_new_entry_points():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is _lib.SIGNATURES['dmh_attention'][0]        # a status, like dmh_attention's
    assert callable(ops.pag_shift)
    assert _lib.ABI_VERSION == 500                           # additions: nothing existing changed


def test_every_new_entry_point_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib
    assert PC.check_einval(_lib) == PC.N_EINVAL


def test_wrappers_refuse_cpu_tensors_and_wrong_arguments():
    from dmhomo_amd import _lib, ops
    x = torch.zeros((2, 8))
    keep = torch.ones(2, dtype=torch.uint8)
    with pytest.raises(_lib.DmhError):                       # there is no CPU path
        ops.pag_shift(x, None, x.clone(), 1.)
    for args, kw in (((x, None, x[:1], 1.), {}), ((x, x[:1], x.clone(), 1.), {}), ((x, None, x.clone(), 1.), {'keep': keep}),
                     ((x, x.clone(), x.clone(), 1.), {'keep': keep[:1]}), ((x, x.clone(), x.clone(), 1.), {'keep': keep.bool()}),
                     ((x, None, x.clone(), float('nan')), {}), ((x, None, x.clone(), float('inf')), {}),
                     ((x, None, x.clone(), -0.5), {}), ((x, x.clone(), x.clone(), -1e-9), {})):
        with pytest.raises(ValueError, match='pag_shift'):
            ops.pag_shift(*args, **kw)
    qkv = torch.zeros((3, 2, 2, 384))
    for lo in (-1, 4, 1.5, True, '1'):
        with pytest.raises(ValueError, match='pert_lo'):
            ops.attention_core(qkv, 0.5, pert_lo=lo)
    with pytest.raises(_lib.DmhError):
        ops.attention_core(qkv, 0.5, pert_lo=1)
