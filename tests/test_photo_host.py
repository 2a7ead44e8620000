"""CPU: the host side of photometric-consistency guidance (``photo_guidance``): the float64 statement of tests/photo_cases.py and
the descent it promises (the kernel tests lean on it), the switch with its check and its four refusals, lambda per entry, the
loops' dispatch (None makes none of the new calls), the capture key, the CLI flag and the argument validation of the new entry
points."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import photo_cases as PC
from test_guidance_host import _diffusion, _run_loop, _stub_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_OPS = ('photo_acc', 'photo_weights', 'photo_guide', 'photo_guide_dev', 'photo_energy', 'photo_energy_workspace',
           'photo_energy_splits')
NEW_ENTRY_POINTS = ('dmh_photo_acc_words', 'dmh_photo_energy_splits', 'dmh_photo_weights', 'dmh_photo_guide', 'dmh_photo_guide_dev',
                    'dmh_photo_energy')


# ------------------------------------------------------------------------------------------ the statement descends
@pytest.fixture(scope='module')
def table():
    return PC.cases(batches=(1,))


def test_case_table_covers_what_it_claims(table):
    assert len(table) == len(PC.SHAPES) * len(PC.FLOWS) * len(PC.MASKS)
    assert PC.SHAPES[-1][0] * PC.SHAPES[-1][1] > 6 * 256 and (PC.SHAPES[-1][0] * PC.SHAPES[-1][1]) % 256 != 0
    for name, c in table:
        assert c['flow'].dtype == c['mask'].dtype == c['cond'].dtype == torch.float32, name
        s = PC.weights_ref(c['flow'], c['mask'])
        rows = torch.stack([PC.warp_matrix(c['flow'][b]).sum(dim=1) for b in range(c['B'])])
        assert float(rows.max()) <= 1. + 1e-6, name          # the rows of W sum to at most 1: what the descent argument uses
        if c['mask_kind'] == 'one' and c['H'] >= 5:
            if c['flow_kind'] in ('far', 'fold'):             # many pixels sample one target: the division matters here
                assert float(s.max()) > 2., (name, float(s.max()))
            if c['flow_kind'] == 'shift':                     # a part of the shifted grid leaves the image and is clamped
                assert float(s.max()) >= 2. and float(s.min()) == 0., name


@pytest.mark.parametrize('lam', PC.LAMBDAS)
def test_the_statement_lowers_the_energy_in_every_case(table, lam):
    """E(after) < E(before) wherever E(before) > 0, for every flow kind, mask kind and shape: the claim of the header, on the
    float64 statement itself"""
    worst = 0.
    for name, c in table:
        x = PC.blend32(c['cond'], c['null'], None, 3.)
        before = PC.energy_ref(x, c['flow'], c['mask'])
        after = PC.energy_ref(PC.guide_ref(x, c['flow'], c['mask'], lam), c['flow'], c['mask'])
        for b in range(c['B']):
            if float(before[b]) > 0.:
                assert float(after[b]) < float(before[b]), (name, lam, float(after[b]), float(before[b]))
                worst = max(worst, float(after[b] / before[b]))
            else:
                # (an all-zero mask: the kind 'zero', or a binary draw over the four pixels of 2 x 2)
                assert float(c['mask'][b].abs().sum()) == 0. and float(after[b]) == 0., name
    print(f'[parity] photo statement, lambda {lam}: {len(table)} cases, largest E(after) / E(before) = {worst:.4f}')
    assert worst < 1.


def test_zero_flow_scales_the_energy_by_one_minus_lambda_squared(table):
    """zero flow, a binary mask: u = im2, so the residual d becomes (1 - lambda) d where the mask is 1: E' = (1 - lambda)^2 E.  To
    float64 rounding where the fp32 taps of the zero flow land on the pixel exactly; where they miss it by an fp32 rounding
    of the normalised coordinate (the warp is within 2^-18 of the identity at these sizes) to twice that"""
    exact = 0
    for name, c in table:
        if c['flow_kind'] != 'zero' or c['mask_kind'] not in ('one', 'binary'):
            continue
        x = PC.blend32(c['cond'], None, None, 1.)
        before = PC.energy_ref(x, c['flow'], c['mask'])
        ident = PC.is_identity(c['flow'])
        exact += ident
        for lam in PC.LAMBDAS:
            after = PC.energy_ref(PC.guide_ref(x, c['flow'], c['mask'], lam), c['flow'], c['mask'])
            want = (1. - lam) ** 2 * before
            tol = 1e-13 if ident else 2. ** -17
            assert bool(((after - want).abs() <= tol * before).all()), (name, lam, after, want)
            if lam == 1. and ident:
                assert float(after.max()) <= 1e-28, (name, after)
    assert exact >= 2                                         # (2 x 2 under both masks: W - 1 == 1, no rounding anywhere)


def test_without_the_division_the_step_diverges_where_pixels_pile_up():
    c = dict(PC.cases(shapes=((16, 16),), batches=(1,), flows=('far',), masks=('one',)))['far-one-1x16x16']
    x = PC.blend32(c['cond'], None, None, 1.)
    before = PC.energy_ref(x, c['flow'], c['mask'])
    plain = PC.energy_ref(PC.guide_ref(x, c['flow'], c['mask'], 1., precondition=False), c['flow'], c['mask'])
    assert float(plain[0]) > 10. * float(before[0])


# ------------------------------------------------------------------------------------------ the switch
def test_default_is_off_and_the_check_accepts_and_refuses():
    d = _diffusion()
    assert d.photo_guidance is None and d._check_photo_guidance() is None
    for w in (1e-3, 0.25, 0.5, 1, 1.):
        d.photo_guidance = w
        got = d._check_photo_guidance()
        assert got == float(w) and isinstance(got, float)
    for bad in (0, 0., -0.1, 1.0000001, 2, float('nan'), float('inf'), '0.5', True, False, [0.5]):
        d.photo_guidance = bad
        with pytest.raises(ValueError, match='photo_guidance'):
            d._check_photo_guidance()


def test_the_unconditional_class_does_not_have_the_switch():
    from dmhomo_amd import ddpm
    assert not hasattr(ddpm.GaussianDiffusion, 'photo_guidance') and not hasattr(ddpm.GaussianDiffusion, '_check_photo_guidance')
    assert callable(ddpm.photometric_error)


def _loop_args(d, cond_scale=3.):
    B, S = 2, d.image_size
    return (torch.zeros(B, dtype=torch.long), torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)),
            (B, d.channels, S, S), cond_scale)


@pytest.mark.parametrize('other, value, why', [('guidance_rescale', 0.7, 'order'), ('apg_eta', 0., 'order'),
                                               ('guidance_interval', (0.25, 0.75), 'unguided'), ('objective', 'pred_v', 'pred_x0')])
def test_refused_combinations_name_both_settings_and_say_why(other, value, why):
    """in the check itself and in front of the first launch of every loop (no GPU here: the loops raise before they draw)"""
    d = _diffusion()
    d.photo_guidance = 0.5
    setattr(d, other, value)
    with pytest.raises(ValueError, match=f'photo_guidance.*{other}.*{why}'):
        d._check_photo_guidance()
    for cond_scale in (3., 1.):                               # (at cond_scale 1 too: the feature acts there)
        for loop in (d._ddim_sample, d._dpmpp_sample, d._sample_graphed):
            with pytest.raises(ValueError, match=f'photo_guidance.*{other}'):
                loop(*_loop_args(d, cond_scale))
    d.photo_guidance = None                                   # off: the other setting is on its own again
    assert d._check_photo_guidance() is None


def test_lambda_is_the_weight_times_alpha_bar_of_the_entry():
    """what dmh_photo_guide forms from the DmhStep of an entry is w * alphas_cumprod[t], CFG:804's weight, to fp32 rounding"""
    for sampler in ('ddim', 'dpmpp_2m'):
        d = _diffusion(6)
        d.sampler = sampler
        entries = list(d._sampler_steps(True, 3.))
        assert len(entries) == 6
        for w in (0.25, 1.):
            for t, step, _ in entries:
                want = w * float(d.alphas_cumprod[t].double())
                got = PC.lam32(w, step.sqrt_ac)
                # (four fp32 roundings: the square root, its square — twice its error —, and the product with w)
                assert abs(got - want) <= 5. * 2. ** -24 * want and 0. < got <= 1., (sampler, t, got, want)
        lams = [PC.lam32(1., step.sqrt_ac) for _, step, _ in entries]
        assert lams == sorted(lams)                           # the pull grows as the noise goes


# ------------------------------------------------------------------------------------------ the loops' dispatch
def _stub_photo(monkeypatch, calls):
    from dmhomo_amd import ops

    def fake(name, result):
        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return result(*a, **k)
        monkeypatch.setattr(ops, name, f)
    fake('photo_acc', lambda B, H, W, device: torch.zeros(3 * B * H * W, dtype=torch.int64))
    fake('photo_weights', lambda flow, mask, acc=None, out=None: torch.zeros(flow.shape[0], *flow.shape[2:]))
    fake('photo_guide', lambda step, cond, null, keep, flow, mask, s, w, acc, out=None: out)
    fake('photo_energy', lambda x, flow, mask, **k: torch.zeros(x.shape[0], dtype=torch.float64))


@pytest.mark.parametrize('clip_mode', ['static', 'dynamic'])
@pytest.mark.parametrize('sampler', ['ddim', 'dpmpp_2m'])
def test_loops_take_the_new_path_only_with_a_weight(sampler, clip_mode, monkeypatch):
    from dmhomo_amd import ops
    S = 4
    d = _diffusion(S)
    d.sampler, d.clip_mode = sampler, clip_mode
    calls = _stub_loop(d, monkeypatch)
    _stub_photo(monkeypatch, calls)
    old_step = {'ddim': 'sampler_step', 'dpmpp_2m': 'sampler_step_ms'}[sampler] if clip_mode == 'static' else 'sampler_step_thr'
    for cond_scale in (3., 1., 1):                            # off: today's calls, exactly
        calls.clear()
        trace = _run_loop(d, sampler, cond_scale)
        assert not any(name in calls for name in NEW_OPS), (cond_scale, calls)
        assert calls[old_step] == S and all('photo' not in e for e in trace)
    seen = []
    inner = getattr(ops, old_step)

    def spy(step, cond, null, *a, **k):
        seen.append((cond, null, k.get('keep')))
        return inner(step, cond, null, *a, **k)
    monkeypatch.setattr(ops, old_step, spy)
    d.photo_guidance = 0.5
    for cond_scale in (3., 1.):                               # on, with and without a null pass
        calls.clear()
        seen.clear()
        trace = _run_loop(d, sampler, cond_scale)
        want = {'photo_acc': 1, 'photo_weights': 1, 'photo_guide': S, 'photo_energy': S, old_step: S,
                **({'sampler_threshold': S} if clip_mode == 'dynamic' else {})}
        if cond_scale != 1:                                   # (the blend the trace's energy is taken of: a sampler_step call)
            want['sampler_step'] = want.get('sampler_step', 0) + S
        assert calls == want, (cond_scale, calls)
        assert len(trace) == S and all(e['photo'].shape == (2,) and e['photo'].dtype == torch.float64 for e in trace)
        updates = [s for s in seen if s[1] is None]           # the update: (guided, no null pass, no keep)
        assert len(updates) == S and all(keep is None for _, _, keep in updates)
        assert len({id(cond) for cond, _, _ in updates}) == 1          # the one guided buffer of the loop
    d.photo_guidance = 1.5
    with pytest.raises(ValueError, match='photo_guidance'):
        _run_loop(d, sampler, 3.)


def test_capture_key_carries_the_weight_only_when_on(monkeypatch):
    d = _diffusion()
    keys = []

    def fake_replay(shape, device, key, tables, buffers, fill):
        keys.append(tuple(key))
        return torch.zeros(shape)
    monkeypatch.setattr(d, '_replay_captured', fake_replay)
    d._sample_graphed(*_loop_args(d))                         # 0: the default
    d.photo_guidance = 0.5                                    # 1, 2: on
    d._sample_graphed(*_loop_args(d))
    d.photo_guidance = 0.25
    d._sample_graphed(*_loop_args(d))
    d._sample_graphed(*_loop_args(d, 1.))                     # 3: on at cond_scale 1 as well
    d.photo_guidance = None
    d._sample_graphed(*_loop_args(d, 1.))                     # 4, 5: off
    d._sample_graphed(*_loop_args(d))
    assert keys[0][-1] == 0.                                  # (the default key still ends with guidance_rescale)
    assert keys[1] == keys[0] + (('photo', 0.5),) and keys[2] == keys[0] + (('photo', 0.25),)
    assert keys[3] == keys[4] + (('photo', 0.25),) and 'photo' not in str(keys[4])
    assert keys[5] == keys[0]


def test_cli_flag_parses_and_help_lists_it():
    src = open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    assert '--photo_guidance' in src.split('"""')[1]          # listed among the additions in the docstring
    head = src[:src.index('args = parser.parse_args()')]
    head = head[head.index('parser = argparse.ArgumentParser()'):]
    ns = {}
    exec('import argparse\n' + head, ns)                     # the parser alone (the script's imports need the built package)
    p = ns['parser']
    assert p.parse_args([]).photo_guidance is None
    assert p.parse_args(['--photo_guidance', '0.5']).photo_guidance == 0.5
    for bad in (['--photo_guidance'], ['--photo_guidance', 'x']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert 'sampler.photo_guidance = args.photo_guidance' in src and 'last_photometric_error' in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'dgm_sample.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--photo_guidance' in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------ the binding
def test_binding_has_the_new_entry_points():
    from dmhomo_amd import _lib, ops
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in NEW_OPS:
        assert callable(getattr(ops, name)), name
    assert _lib.ABI_VERSION == 500                           # additions: nothing existing changed


def test_pure_size_functions():
    from dmhomo_amd import _lib
    lib = _lib.lib()
    for B, H, W in ((1, 2, 2), (3, 33, 47), (25, 128, 128), (25, 256, 256), (65535, 2, 2), (1, 4096, 4096)):
        assert lib.dmh_photo_acc_words(B, H, W) == 3 * B * H * W
        assert lib.dmh_photo_energy_splits(B, H, W) == min((H * W + 1023) // 1024, max(1024 // B, 1))
    assert lib.dmh_photo_energy_splits(3, 33, 47) == 2 and lib.dmh_photo_energy_splits(25, 128, 128) == 16
    for B, H, W in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 1, 4), (1, 4, 1), (1, 0, 0), (1, 4097, 4096), (1, 2 ** 30, 2 ** 30)):
        assert lib.dmh_photo_acc_words(B, H, W) == -1 and lib.dmh_photo_energy_splits(B, H, W) == -1, (B, H, W)
        assert b'dmh_photo_energy_splits' in lib.dmh_last_error()


def test_every_new_entry_point_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * 65536)()
    p = lambda k=0: C.c_void_p(C.addressof(buf) + 4096 * k)   # disjoint host addresses: only ever compared, never read
    step = _lib.DmhStep(1, 1, 1, 3., 1., 1., 0.7, 0.6, 0., 0., 0.)
    n = 0

    def refused(name, args, word):
        nonlocal n
        assert getattr(lib, name)(*args, None) == -1, (name, word)
        assert name.encode() in lib.dmh_last_error() and word.encode() in lib.dmh_last_error(), (name, lib.dmh_last_error())
        n += 1
    good = [p(0), p(1), p(2), p(3), 2, 4, 4]                  # flow, mask, acc, s, B, H, W
    for i in range(4):
        refused('dmh_photo_weights', good[:i] + [None] + good[i + 1:], 'null pointer')
    good = [p(0), p(1), p(2), p(3), p(4), 2, 4, 4]            # x, flow, mask, ws, E, B, H, W
    for i in range(5):
        refused('dmh_photo_energy', good[:i] + [None] + good[i + 1:], 'null pointer')
    for name, s in (('dmh_photo_guide', C.byref(step)), ('dmh_photo_guide_dev', p(9))):
        #       step cond null  keep  flow  mask  s     w    acc   guided B  H  W
        good = [s, p(0), p(1), p(2), p(3), p(4), p(5), 0.5, p(6), p(7), 2, 4, 4]
        for i in (0, 1, 4, 5, 6, 8, 9):
            refused(name, good[:i] + [None] + good[i + 1:], 'null pointer')
        refused(name, good[:2] + [None] + good[3:], 'keep needs model_null')
        for w in (0., -0.5, 1.5, float('nan'), float('inf')):
            refused(name, good[:7] + [w] + good[8:], 'w=')
        refused(name, good[:9] + [p(0)] + good[10:], 'overlaps')
        refused(name, good[:9] + [p(1)] + good[10:], 'overlaps')
        refused(name, good[:9] + [C.c_void_p(p(1).value + 2 * 6 * 16 * 4 - 4)] + good[10:], 'overlaps')
    for name, head in (('dmh_photo_weights', [p(0), p(1), p(2), p(3)]), ('dmh_photo_energy', [p(0), p(1), p(2), p(3), p(4)]),
                       ('dmh_photo_guide', [C.byref(step), p(0), p(1), p(2), p(3), p(4), p(5), 0.5, p(6), p(7)]),
                       ('dmh_photo_guide_dev', [p(9), p(0), p(1), p(2), p(3), p(4), p(5), 0.5, p(6), p(7)])):
        for B, H, W in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 1, 4), (1, 4, 1), (1, 4097, 4096), (2, 2 ** 30, 2 ** 30)):
            refused(name, head + [B, H, W], 'H >= 2')
    assert n == 4 + 5 + 2 * (7 + 1 + 5 + 3) + 4 * 7
