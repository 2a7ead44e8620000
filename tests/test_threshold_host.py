"""CPU: the host side of dynamic thresholding (``clip_mode = 'dynamic'``): the switch and its checks, the (k, frac) rank helper,
the float64 quantile reference of tests/threshold_cases.py against torch.quantile, the unconditional class's refusal, and the
new entry points in the binding."""
import pytest
import torch

import threshold_cases as TC


def _host():
    from dmhomo_amd.sampling import ScheduleHost

    class H(ScheduleHost):
        pass
    return H()


def test_defaults_leave_the_static_clamp():
    h = _host()
    assert h.clip_mode == 'static' and h.CLIP_MODES == ('static', 'dynamic') and h.dynamic_threshold_percentile == 0.995
    assert h._check_clip_mode() == 'static'


def test_check_clip_mode_accepts_and_refuses():
    h = _host()
    h.clip_mode = 'dynamic'
    for p in (0.995, 1.0, 1, 1e-6, 0.5):
        h.dynamic_threshold_percentile = p
        assert h._check_clip_mode() == 'dynamic'
    for p in (0., -0.1, 1.0000001, 2, float('nan'), float('inf'), None, '0.9'):
        h.dynamic_threshold_percentile = p
        with pytest.raises(ValueError, match='dynamic_threshold_percentile'):
            h._check_clip_mode()
    h.dynamic_threshold_percentile = 0.995
    for mode in ('Dynamic', 'imagen', None, ''):
        h.clip_mode = mode
        with pytest.raises(ValueError, match='clip_mode'):
            h._check_clip_mode()
    h.clip_mode, h.dynamic_threshold_percentile = 'static', 7.       # (checked whatever the mode: a typo shows at once)
    with pytest.raises(ValueError, match='dynamic_threshold_percentile'):
        h._check_clip_mode()


def test_quantile_rank():
    from dmhomo_amd.sampling import ScheduleHost
    rank = ScheduleHost._quantile_rank
    for p in (1e-3, 0.5, 0.995, 1.0):
        assert rank(p, 1) == (0, 0.)                         # one value: it is every quantile
    for n in (2, 3, 1024, 98304):
        assert rank(1.0, n) == (n - 1, 0.)                   # the maximum: no v[k+1] exists
    assert rank(0.5, 3) == (1, 0.) and rank(0.5, 1025) == (512, 0.) and rank(0.25, 65) == (16, 0.)   # integral ranks
    k, frac = rank(0.995, 98304)                             # the workload's row: 0.995 * 98303 = 97811.485
    assert k == 97811 and frac == torch.tensor(0.995 * 98303 - 97811, dtype=torch.float64).float().item()
    assert abs(frac - 0.485) < 1e-6
    k, frac = rank(0.5 / 64, 64)
    assert k == 0 and 0. < frac < 1.
    for n in TC.SIZES + (TC.BIG[0], TC.HUGE[0]):             # the tests' own statement of it agrees, and stays in range
        for p in TC.percentiles(n):
            k, frac = rank(p, n)
            assert (k, frac) == TC.rank_of(p, n) and 0 <= k < n and 0. <= frac < 1. and (frac == 0. or k + 1 < n)
    for p, n in ((0., 4), (1.5, 4), (0.5, 0)):
        with pytest.raises(ValueError):
            rank(p, n)


def test_case_list_covers_what_it_claims():
    cases = TC.selector_cases()
    seen = {}
    for name, x, p, kinds in cases:
        B, n = x.shape
        assert x.dtype == torch.float32 and len(kinds) == B and len(set(kinds)) == min(B, len(TC.KINDS))   # rows of different kinds
        seen.setdefault(n, set()).update(kinds)
    for n in TC.SIZES:
        assert seen[n] == set(TC.KINDS), (n, seen[n])        # every kind at every size
    ranks = [TC.rank_of(p, x.shape[1]) + (x.shape[1],) for _, x, p, _ in cases]
    assert any(f == 0. and 0 < k < n - 1 for k, f, n in ranks)           # an integral rank inside the row
    assert any(k == 0 and f != 0. for k, f, n in ranks) and any(k == n - 1 for k, f, n in ranks)
    assert {tuple(x.shape) for _, x, _, _ in cases} >= {(25, 98304), (2, 393216), (1, 1), (3, 1025)}


def test_reference_agrees_with_torch_quantile():
    """float64 torch.quantile of the same |x| (linear interpolation at rank p * (n - 1)): the only difference is the fp32
    frac, at most 2^-24 of b - a.  Rows with inf or NaN are left out: torch's lerp answers NaN next to an infinity"""
    checked = 0
    for name, x, p, _ in TC.selector_cases():
        for row in x:
            if not bool(torch.isfinite(row).all()):
                continue
            k, frac, a, b, q = TC.quantile_ref(row, p)
            want = float(torch.quantile(row.abs().double(), torch.tensor(p, dtype=torch.float64)))
            assert a <= q <= b and abs(q - want) <= 2. ** -23 * (b - a) + 1e-300, (name, q, want)
            if frac == 0.:
                assert q == a
            checked += 1
    assert checked > 200


def test_apply_threshold_reference():
    x = torch.tensor([[-3., 0.5, 2.], [-3., 0.5, 2.], [1., 2., 3.]])
    got = TC.apply_threshold(x, torch.tensor([1., 2., float('nan')]))
    assert torch.equal(got[0], torch.tensor([-1., 0.5, 1.], dtype=torch.float64))       # thr 1: the static clamp
    assert torch.equal(got[1], torch.tensor([-1., 0.25, 1.], dtype=torch.float64))
    assert bool(torch.isnan(got[2]).all())
    q, thr = TC.threshold_ref(x, 1.0)
    assert q.tolist() == [3., 3., 3.] and thr.tolist() == [3., 3., 3.]
    q, thr = TC.threshold_ref(x * 0.1, 0.5)
    assert thr.tolist() == [1., 1., 1.] and abs(float(q[0]) - 0.2) < 1e-7


def test_unconditional_class_refuses_dynamic_without_a_device():
    from dmhomo_amd import ddpm
    m = ddpm.Unet(dim=8, dim_mults=(1, 2), channels=3)
    d = ddpm.GaussianDiffusion(m, image_size=16, timesteps=10, sampling_timesteps=4)
    d.clip_mode = 'dynamic'
    with pytest.raises(ValueError, match='unconditional'):
        d.sample(batch_size=2)
    d.dynamic_threshold_percentile = 3.
    with pytest.raises(ValueError, match='dynamic_threshold_percentile'):
        d.sample(batch_size=2)


def test_binding_has_the_new_entry_points():
    import ctypes
    from dmhomo_amd import _lib, ops
    names = ('dmh_row_quantile_abs', 'dmh_sampler_threshold', 'dmh_sampler_threshold_dev', 'dmh_sampler_step_thr',
             'dmh_sampler_step_thr_dev')
    lib = _lib.lib()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ('row_quantile_abs', 'sampler_threshold', 'sampler_threshold_dev', 'sampler_step_thr', 'sampler_step_thr_dev'):
        assert callable(getattr(ops, name)), name
    assert _lib.ABI_VERSION == 500                           # an addition: nothing existing changed
    # refused through the error channel before anything is launched (no GPU here)
    buf = ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p)
    for args, word in (((None, buf, 1, 4, 0, 0., 0.), 'null'), ((buf, buf, 0, 4, 0, 0., 0.), 'B=0'),
                       ((buf, buf, 1, 0, 0, 0., 0.), 'n=0'), ((buf, buf, 1, 2 ** 31, 0, 0., 0.), '2^31'),
                       ((buf, buf, 1, 4, 4, 0., 0.), 'rank'), ((buf, buf, 1, 4, -1, 0., 0.), 'rank'),
                       ((buf, buf, 1, 4, 0, 1., 0.), 'rank'), ((buf, buf, 1, 4, 0, -0.5, 0.), 'rank'),
                       ((buf, buf, 1, 4, 3, 0.5, 0.), 'rank'), ((buf, buf, 1, 4, 0, float('nan'), 0.), 'rank'),
                       ((buf, buf, 1, 4, 0, 0., float('nan')), 'floor')):
        assert lib.dmh_row_quantile_abs(*args, None) == -1 and word in lib.dmh_last_error().decode(), (args, lib.dmh_last_error())
