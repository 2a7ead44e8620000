"""CPU: the host side of the guidance interval (``guidance_interval``): the switch and its check, which entries it guides,
the step lists it leaves alone, the eager loops' dispatch, the capture key, the unconditional class's refusal, the CLI flag, the
row-list contract of tests/interval_cases.py, and the argument validation of the two new entry points."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import interval_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host():
    from dmhomo_amd.sampling import ScheduleHost

    class H(ScheduleHost):
        pass
    return H()


def _diffusion(T=100, S=6):
    from dmhomo_amd import cfg
    m = cfg.Unet(dim=8, dim_mults=(1, 2), channels=6, num_classes=1)
    return cfg.GaussianDiffusion(m, image_size=8, timesteps=T, sampling_timesteps=S, objective='pred_x0')


def test_default_is_off_and_the_check_accepts_and_refuses():
    h = _host()
    assert h.guidance_interval is None and h._check_guidance_interval() is None
    for gi in ((0, 1), (0.3, 0.3), (0., 1.), [0.25, 0.75], (0, 0), (1, 1)):
        h.guidance_interval = gi
        got = h._check_guidance_interval()
        assert got == (float(gi[0]), float(gi[1])) and all(type(v) is float for v in got)
    for gi in (True, (True, 1.), (0., True), (0.2, 0.5, 0.7), (0.5,), (), (0.7, 0.3), (-0.1, 0.5), (0.5, 1.0000001), 0.5, '01',
               ('0', '1'), (None, 1.), (float('nan'), 1.), (0., float('nan')), (0., float('inf')), {0., 1.}):
        h.guidance_interval = gi
        with pytest.raises(ValueError, match='guidance_interval'):
            h._check_guidance_interval()


@pytest.mark.parametrize('T,S,interval,want', IC.PATTERNS)
def test_guided_pattern(T, S, interval, want):
    d = _diffusion(T, S)
    for sampler in ('ddim', 'dpmpp_2m'):
        d.sampler = sampler
        times = [t for t, _, _ in d._sampler_steps(True, 3.)]
        assert times == IC.sample_times(T, S)
        d.guidance_interval = interval
        got = d._guided_entries(times, 3.)
        assert got == want == IC.guided_pattern(times, T, interval), (T, S, interval, got)
        assert d._guided_entries(times, 1.) is None and d._guided_entries(times, 1) is None     # no null pass to leave out
    d.guidance_interval = None
    assert d._guided_entries(times, 3.) is None


def test_the_first_pattern_has_both_transitions_and_an_unguided_last_entry():
    T, S, interval, want = IC.PATTERNS[0]
    assert (T, S, interval) == (100, 6, (0.3, 0.7))
    pairs = list(zip(want[:-1], want[1:]))
    assert (False, True) in pairs and (True, False) in pairs and want[-1] is False and want[0] is False
    assert not any(IC.guided_pattern(IC.sample_times(100, 6), 100, IC.NOTHING))


@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_step_lists_do_not_depend_on_the_interval(sampler):
    d = _diffusion()
    d.sampler = sampler
    as_tuples = lambda steps: [(t, tuple(getattr(s, n) for n, _ in s._fields_), dr) for t, s, dr in steps]
    want = as_tuples(d._sampler_steps(True, 3.))
    for gi in ((0.3, 0.7), (0., 1.), IC.NOTHING):
        d.guidance_interval = gi
        assert as_tuples(d._sampler_steps(True, 3.)) == want


def test_unconditional_class_refuses_an_interval():
    from dmhomo_amd import ddpm
    m = ddpm.Unet(dim=8, dim_mults=(1, 2), channels=3)
    d = ddpm.GaussianDiffusion(m, image_size=16, timesteps=10, sampling_timesteps=4)
    d.guidance_interval = (0.3, 0.7)
    with pytest.raises(ValueError, match='unconditional'):
        d.sample(batch_size=2)
    d.guidance_interval = (0.7, 0.3)
    with pytest.raises(ValueError, match='guidance_interval'):
        d.sample(batch_size=2)


# ------------------------------------------------------------------------------------------ the eager loops' dispatch
def _stub_loop(d, monkeypatch):
    """the eager loops with the network, the generator and every step-side ops function replaced by counting stand-ins ->
    (the counter {ops name: calls}, the cond_scale of every network call)"""
    from dmhomo_amd import ops
    calls, scales = {}, []

    def fake(name, result):
        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            if name != 'guidance_workspace':
                null = a[2]                                  # (step, cond, null, x, ...)
                calls.setdefault(name + ':null', []).append(null is not None)
            return result(*a, **k)
        monkeypatch.setattr(ops, name, f)

    def fake_network(x, t, classes, rgb_flow, mask, cs):
        scales.append(cs)
        return torch.zeros_like(x), (None if cs == 1 else torch.zeros_like(x)), None

    class Rng:
        def randn(self, shape, device):
            return torch.zeros(tuple(shape))
    x_of = lambda a: a[3]
    fake('sampler_step', lambda *a, **k: (x_of(a).clone(), x_of(a).clone(), None))
    fake('sampler_step_ms', lambda *a, **k: (x_of(a).clone(), x_of(a).clone()))
    fake('sampler_threshold', lambda *a, **k: (torch.ones(x_of(a).shape[0]), None))
    fake('sampler_step_thr', lambda *a, **k: (x_of(a).clone(), x_of(a).clone()))
    fake('guidance_workspace', lambda x: torch.zeros(4, dtype=torch.float64))
    fake('guidance_factor', lambda step, cond, null, phi, **k: torch.ones(cond.shape[0]))
    fake('sampler_threshold_gr', lambda *a, **k: (torch.ones(x_of(a).shape[0]), None))
    fake('sampler_step_gr', lambda *a, **k: (x_of(a).clone(), x_of(a).clone()))
    for name in ('rows_gated', 'guidance_gate'):             # the eager loops never touch the device-side gating
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail('the eager loop called the captured step\'s gating'))
    monkeypatch.setattr(ops, 'affine', lambda x, a, b, out=None: x)
    monkeypatch.setattr(d, '_network', fake_network)
    d.rng = Rng()
    return calls, scales


def _run_loop(d, sampler, cond_scale):
    B, S = 2, d.image_size
    shape = (B, d.channels, S, S)
    loop = d._dpmpp_sample if sampler == 'dpmpp_2m' else d._ddim_sample
    trace = []
    loop(torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)), shape,
         cond_scale, trace=trace)
    return trace


@pytest.mark.parametrize('phi', [0., 0.7])
@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_eager_loops_run_unguided_entries_as_cond_scale_1(sampler, clip_mode, phi, monkeypatch):
    T, S, interval, want = IC.PATTERNS[0]
    d = _diffusion(T, S)
    d.sampler, d.clip_mode, d.guidance_rescale = sampler, clip_mode, phi
    calls, scales = _stub_loop(d, monkeypatch)
    plain = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler] if clip_mode == 'static' else 'sampler_step_thr'
    n_on = sum(want)
    # no interval: every entry guided, the calls of today
    trace = _run_loop(d, sampler, 3.)
    assert scales == [3.] * S and all(e['guided'] is True for e in trace)
    assert calls[('sampler_step_gr' if phi else plain)] == S
    # the interval: unguided entries call the network at cond_scale 1 and take the plain or thresholded call without a null pass
    calls.clear(), scales.clear()
    d.guidance_interval = interval
    trace = _run_loop(d, sampler, 3.)
    assert scales == [3. if on else 1 for on in want]
    assert [e['guided'] for e in trace] == want and [e['time'] for e in trace] == IC.sample_times(T, S)
    if phi:
        assert calls['guidance_factor'] == calls['sampler_step_gr'] == n_on and calls[plain] == S - n_on
        assert calls[plain + ':null'] == [False] * (S - n_on)
        assert [('gfac' in e) for e in trace] == want
        assert calls.get('sampler_threshold_gr', 0) == (n_on if clip_mode == 'dynamic' else 0)
        assert calls.get('sampler_threshold', 0) == (S - n_on if clip_mode == 'dynamic' else 0)
    else:
        assert calls[plain] == S and calls[plain + ':null'] == want and 'guidance_factor' not in calls
        assert calls.get('sampler_threshold', 0) == (S if clip_mode == 'dynamic' else 0)
    assert all(('thr' in e) == (clip_mode == 'dynamic') for e in trace)
    # cond_scale 1: the interval does nothing
    calls.clear(), scales.clear()
    trace = _run_loop(d, sampler, 1.)
    assert scales == [1.] * S and all(e['guided'] is True for e in trace) and calls[plain] == S
    d.guidance_interval = (0.7, 0.3)
    with pytest.raises(ValueError, match='guidance_interval'):
        _run_loop(d, sampler, 3.)


def test_capture_key_carries_that_an_interval_is_set_and_not_its_value(monkeypatch):
    d = _diffusion()
    keys = []

    def fake_replay(shape, device, key, tables, buffers, fill):
        keys.append(tuple(key))
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    B, S = 2, d.image_size
    args = (torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)),
            (B, d.channels, S, S))
    for gi in (None, (0.3, 0.7), (0., 1.), IC.NOTHING, None):
        d.guidance_interval = gi
        d._sample_graphed(*args, 3.)
    assert keys[0] == keys[4] and keys[1] == keys[2] == keys[3] and keys[0] != keys[1]
    assert keys[1][:len(keys[0])] == keys[0] and len(keys[1]) == len(keys[0]) + 1     # None: today's key, to the last element
    d.guidance_interval = (0.3, 0.7)
    d._sample_graphed(*args, 1.)                             # cond_scale 1: no null pass, nothing to gate
    d.guidance_interval = None
    d._sample_graphed(*args, 1.)
    assert keys[5] == keys[6] and len(keys[5]) == len(keys[0])
    d.guidance_interval = (0.7, 0.3)
    with pytest.raises(ValueError, match='guidance_interval'):
        d._sample_graphed(*args, 3.)


def test_cli_flag_parses():
    src = open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    assert '--guidance_interval' in src.split('"""')[1]       # listed among the additions in the docstring
    head = src[:src.index('args = parser.parse_args()')]
    head = head[head.index('parser = argparse.ArgumentParser()'):]
    ns = {}
    exec('import argparse\n' + head, ns)                     # the parser alone (the script's imports need the built package)
    p = ns['parser']
    assert p.parse_args([]).guidance_interval is None
    assert p.parse_args(['--guidance_interval', '0.25', '0.75']).guidance_interval == [0.25, 0.75]
    for bad in (['--guidance_interval', '0.25'], ['--guidance_interval', 'a', 'b']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert 'sampler.guidance_interval = ' in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'dgm_sample.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--guidance_interval LO HI' in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------ the row-list contract
def test_row_list_contract_restated():
    cases = IC.row_cases()
    assert len(cases) == (3 + 4 + 4) * 2 * 2
    for name, B, keep, extra, null_side in cases:
        on, off = IC.rows_ref(keep, B, extra, True, null_side), IC.rows_ref(keep, B, extra, False, null_side)
        assert on[0] == len(on) - 1 and off[0] == len(off) - 1 and on[1:] == sorted(on[1:]), name
        assert max(on[0], off[0]) <= B + extra                # fits the buffer of 1 + B + extra words
        assert on[1 + on[0] - extra:] == list(range(B, B + extra)), name       # a guided entry ends with the extras
        if null_side:
            assert off == [0] and on[1:] == list(range(B + extra)), name
        else:
            assert off == [B] + list(range(B)), name           # every slot, no extras: also the dropped rows
            kept = [b for b in range(B) if keep is None or keep[b]]
            assert on[1:1 + len(kept)] == kept and on[0] == len(kept) + extra, name
    # without a keep mask and guided, the list is every row: what rows=None means
    assert IC.rows_ref(None, 3, 3, True, False) == [6, 0, 1, 2, 3, 4, 5]
    assert IC.rows_ref([1, 0, 1], 3, 3, True, False) == [5, 0, 2, 3, 4, 5]    # dmh_rows_from_keep's list
    assert IC.rows_ref([1, 0, 1], 3, 3, False, False) == [3, 0, 1, 2]


# ------------------------------------------------------------------------------------------ the binding
def test_binding_has_the_new_entry_points():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for name in ('dmh_rows_gated', 'dmh_guidance_gate'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(ops.rows_gated) and callable(ops.guidance_gate)
    assert _lib.ABI_VERSION == 500                           # additions: nothing existing changed


def test_new_entry_points_validate_their_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib
    lib = _lib.lib()
    raw = (ctypes.c_char * 512)()
    base = ctypes.addressof(raw) + (-ctypes.addressof(raw)) % 16
    buf, buf2 = ctypes.c_void_p(base), ctypes.c_void_p(base + 256)

    def refused(name, args, word):
        assert getattr(lib, name)(*args, None) == -1, (name, args)               # DMH_EINVAL
        msg = lib.dmh_last_error().decode()
        assert name + ':' in msg and word in msg, (name, word, msg)
    #       keep  B  extra cursor guided S null_side rows
    good = [buf, 3, 3, buf, buf, 4, 0, buf2]
    for i in (3, 4, 7):
        refused('dmh_rows_gated', good[:i] + [None] + good[i + 1:], 'null pointer')
    for B in (0, -1, -2 ** 31):
        refused('dmh_rows_gated', [buf, B] + good[2:], f'B={B}')
    for extra in (-1, -25):
        refused('dmh_rows_gated', good[:2] + [extra] + good[3:], f'extra={extra}')
    refused('dmh_rows_gated', good[:2] + [2 ** 31 - 2] + good[3:], 'extra=')      # B + extra past int32
    for S in (0, -4):
        refused('dmh_rows_gated', good[:5] + [S] + good[6:], f'S={S}')
    for side in (2, -1):
        refused('dmh_rows_gated', good[:6] + [side] + good[7:], 'null_side')
    #       cursor guided S cond null n
    good = [buf, buf, 4, buf, buf2, 8]
    for i in (0, 1, 3, 4):
        refused('dmh_guidance_gate', good[:i] + [None] + good[i + 1:], 'null pointer')
    for n in (0, -1, -2 ** 40):
        refused('dmh_guidance_gate', good[:5] + [n], f'n={n}')
    for S in (0, -1):
        refused('dmh_guidance_gate', good[:2] + [S] + good[3:], f'S={S}')
    refused('dmh_guidance_gate', good[:3] + [ctypes.c_void_p(base + 2)] + good[4:], 'aligned')
    refused('dmh_guidance_gate', good[:4] + [ctypes.c_void_p(base + 258)] + good[5:], 'aligned')
    for null in (base, base + 4, base + 28):                 # null inside cond's 32 bytes
        refused('dmh_guidance_gate', good[:4] + [ctypes.c_void_p(null), 8], 'overlap')
    refused('dmh_guidance_gate', [buf, buf, 4, buf2, buf, 65], 'overlap')          # cond behind null, null reaching into it
