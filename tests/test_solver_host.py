"""CPU: the host side of the second-order multistep sampler (``sampler = 'dpmpp_2m'``, ScheduleHost._dpmpp_steps).

1. the step list against an independent float64 computation written here (coefficients, modes, draws, timesteps);
2. every first-order entry equals the DDIM update at eta = 0, rewritten in (x0, xt) form;
3. on a Gaussian data model, whose denoiser and probability-flow solution are known in closed form, the solver's
   discretisation error is below DDIM's (eta = 0) at the same step count, and at 16 steps below DDIM's at 32.  This is a
   statement about discretisation error on an analytic model, not about sample quality with trained weights;
4. an unknown ``sampler`` is refused at sample(), and the new entry points validate their arguments (no launch here)."""
import math

import numpy as np
import pytest
import torch

from dmhomo_amd import cfg, ddpm, ops
from dmhomo_amd.schedule import ddim_pairs


def _diffusion(T, S, schedule='cosine', objective='pred_x0', eta=1., kind='cfg'):
    if kind == 'cfg':
        m = cfg.Unet(dim=8, dim_mults=(1, 2), channels=6, num_classes=1)
        return cfg.GaussianDiffusion(m, image_size=8, timesteps=T, sampling_timesteps=S, objective=objective,
                                     beta_schedule=schedule, ddim_sampling_eta=eta)
    m = ddpm.Unet(dim=8, dim_mults=(1, 2), channels=3)
    return ddpm.GaussianDiffusion(m, image_size=8, timesteps=T, sampling_timesteps=S, objective=objective,
                                  beta_schedule=schedule, ddim_sampling_eta=eta)


def _abar64(d):
    return d.alphas_cumprod.detach().cpu().numpy().astype(np.float64)     # the fp32 buffer, widened


def reference_coefficients(abar, pairs):
    """[(c0, c1, c2) or None for the entry that returns x0], float64, from the definitions"""
    lam = lambda t: 0.5 * (math.log(abar[t]) - math.log1p(-abar[t]))      # ln(a / s), written another way
    upd = [(t, tn) for t, tn in pairs if tn >= 0]
    out = []
    for k, (t, tn) in enumerate(upd):
        h = lam(tn) - lam(t)
        base = math.sqrt(abar[tn]) * (1. - math.exp(-h))
        c1 = math.sqrt((1. - abar[tn]) / (1. - abar[t]))
        if k == 0 or k == len(upd) - 1:
            out.append((base, c1, 0.))
        else:
            tp = upd[k - 1][0]
            r = (lam(t) - lam(tp)) / h
            out.append((base * (1. + 0.5 / r), c1, -base * 0.5 / r))
    return out + [None] * (len(pairs) - len(upd))


def _rel(got, want):
    return abs(got - want) / max(abs(want), 1e-300)


CASES = [('cosine', 1000, 32), ('cosine', 1000, 4), ('linear', 200, 7), ('cosine', 50, 49), ('cosine', 100, 1)]


@pytest.mark.parametrize('schedule,T,S', CASES, ids=lambda v: str(v))
@pytest.mark.parametrize('kind', ['cfg', 'ddp'])
def test_coefficients_against_float64(schedule, T, S, kind):
    d = _diffusion(T, S, schedule, kind=kind)
    d.ddim_sampling_eta = 0.7                                 # ignored by the solver
    pairs = ddim_pairs(T, S)
    steps = d._dpmpp_steps(True, 3.)
    want = reference_coefficients(_abar64(d), pairs)
    assert [t for t, _, _ in steps] == [t for t, _ in pairs] and len(steps) == S
    assert all(draws == 0 for _, _, draws in steps)
    assert steps[-1][1].mode == ops.MODE_LAST and pairs[-1][1] < 0
    upd = [st for _, st, _ in steps[:-1]]
    assert all(st.mode == ops.MODE_MULTISTEP for st in upd)
    if upd:
        assert upd[0].c2 == 0. and upd[-1].c2 == 0.
    assert all(st.c2 != 0. for st in upd[1:-1])
    worst = 0.
    for st, w in zip(upd, want):
        for got, ref in zip((st.c0, st.c1, st.c2), w):
            ref32 = float(np.float32(ref))
            worst = max(worst, _rel(got, ref32))
            assert _rel(got, ref32) <= 1e-6 if ref32 != 0. else got == 0., (got, ref32)
    print(f'[solver] {schedule} T={T} S={S}: worst relative coefficient difference {worst:.2e}')
    # the other scalars are _step's, as for DDIM
    for (_, a, _), (_, b, _) in zip(steps, d._ddim_steps(True, 3.)):
        for f in ('objective', 'clip', 'cond_scale', 'sqrt_recip_ac', 'sqrt_recipm1_ac', 'sqrt_ac', 'sqrt_1m_ac'):
            assert getattr(a, f) == getattr(b, f)
    # S == T is allowed although is_ddim_sampling is False there
    if (T, S) == (100, 1):
        full = _diffusion(20, 20, kind=kind)
        assert not full.is_ddim_sampling and len(full._dpmpp_steps(True)) == 20


def test_times_that_do_not_decrease_are_refused(monkeypatch):
    d = _diffusion(20, 5)
    from dmhomo_amd import sampling
    monkeypatch.setattr(sampling, 'ddim_pairs', lambda T, S: [(19, 10), (10, 10), (10, 3), (3, -1)])
    with pytest.raises(ValueError):
        d._dpmpp_steps(True)


@pytest.mark.parametrize('schedule,T,S', CASES, ids=lambda v: str(v))
def test_first_order_entries_are_ddim_at_eta_zero(schedule, T, S):
    """DDIM at eta = 0: img' = sqrt(abar') x0 + c (xt - a_k x0) / s_k, so c1 = c / s_k and c0 = sqrt(abar') - c1 a_k"""
    d = _diffusion(T, S, schedule, eta=0.)
    abar, host = _abar64(d), d._host()
    checked = 0
    for (t, tn), (_, st, _) in zip(ddim_pairs(T, S), d._dpmpp_steps(True)):
        if st.mode != ops.MODE_MULTISTEP or st.c2 != 0.:
            continue
        sq_next, c, sigma = d._ddim_coef(host, t, tn)
        assert sigma == 0.
        a_k, s_k = math.sqrt(abar[t]), math.sqrt(1. - abar[t])
        c1 = c / s_k
        c0 = sq_next - c1 * a_k
        assert _rel(st.c1, c1) <= 1e-5 and _rel(st.c0, c0) <= 1e-5, (t, tn, st.c0, c0, st.c1, c1)
        checked += 1
    assert checked == min(2, S - 1)


# ---- the Gaussian model: x0 ~ N(MU, SD^2) per element
MU, SD = 0.3, 0.5


def _denoiser(x, a, sig):
    return MU + a * SD ** 2 / (a ** 2 * SD ** 2 + sig ** 2) * (x - a * MU)


def _run(steps, abar, x):
    """denoise_step's formulas (objective pred_x0, no clamp) in float64 over a step list -> the sampler's output"""
    prev = None
    for t, st, _ in steps:
        a, sig = math.sqrt(abar[t]), math.sqrt(1. - abar[t])
        x0 = _denoiser(x, a, sig)
        pn = (st.sqrt_recip_ac * x - x0) / st.sqrt_recipm1_ac
        if st.mode == ops.MODE_DDIM:
            assert st.c2 == 0.                                # eta = 0: no noise term
            x = x0 * st.c0 + st.c1 * pn
        elif st.mode == ops.MODE_LAST:
            x = x0
        else:
            assert st.mode == ops.MODE_MULTISTEP
            o = st.c0 * x0 + st.c1 * x
            x = o + st.c2 * prev if st.c2 != 0. else o
        prev = x0
    return x


def _errors(S):
    d = _diffusion(1000, S, objective='pred_x0', eta=0.)
    abar = _abar64(d)
    x_T = np.random.default_rng(0).standard_normal(4096)
    t_first, t_last = ddim_pairs(1000, S)[0][0], ddim_pairs(1000, S)[-1][0]
    a_T, s_T = math.sqrt(abar[t_first]), math.sqrt(1. - abar[t_first])
    zeta = (x_T - a_T * MU) / math.sqrt(a_T ** 2 * SD ** 2 + s_T ** 2)     # conserved along the probability flow
    a, sig = math.sqrt(abar[t_last]), math.sqrt(1. - abar[t_last])
    exact = _denoiser(a * MU + math.sqrt(a ** 2 * SD ** 2 + sig ** 2) * zeta, a, sig)
    e_ddim = float(np.abs(_run(d._ddim_steps(False), abar, x_T) - exact).max())
    e_2m = float(np.abs(_run(d._dpmpp_steps(False), abar, x_T) - exact).max())
    return e_ddim, e_2m


def test_convergence_on_the_gaussian_model():
    """measured with exactly these inputs: DDIM 0.199 / 0.138 / 0.0800, 2M 0.119 / 0.0315 / 0.00126 at S = 8 / 16 / 32"""
    err = {S: _errors(S) for S in (8, 16, 32)}
    for S, (e_ddim, e_2m) in err.items():
        print(f'[solver] Gaussian model S={S}: max error DDIM(eta=0) {e_ddim:.4g}, dpmpp_2m {e_2m:.4g}')
    for S in (8, 16, 32):
        assert err[S][1] < err[S][0], (S, err[S])
    assert err[16][1] < err[32][0], (err[16], err[32])
    assert err[32][1] < 0.1 * err[32][0], err[32]


def test_unknown_sampler_is_refused():
    assert cfg.GaussianDiffusion.sampler == 'ddim' and ddpm.GaussianDiffusion.sampler == 'ddim'
    d = _diffusion(20, 5)
    d.sampler = 'euler'
    z = torch.zeros
    with pytest.raises(ValueError, match='euler'):
        d.sample(z(2, dtype=torch.long), z(2, 3, 8, 8), z(2, 2, 8, 8), z(2, 1, 8, 8))
    u = _diffusion(20, 5, kind='ddp')
    u.sampler = 'euler'
    with pytest.raises(ValueError, match='euler'):
        u.sample(batch_size=2)


def test_entry_points_validate_their_arguments():
    import ctypes as C
    from dmhomo_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * 4096)()
    hp = C.cast(buf, C.c_void_p)                              # (host memory: every call below is refused before any launch)

    def step(mode, objective=1):
        return C.byref(_lib.DmhStep(objective, 0, mode, 1., 1., 1., 1., 1., 0., 0., 0.))
    for mode in (0, 2, -1, 4):
        assert lib.dmh_sampler_step_ms(step(mode), hp, None, hp, hp, hp, None, 16, None, 0, None) == -1
        assert b'dmh_sampler_step_ms' in lib.dmh_last_error()
    assert lib.dmh_sampler_step_ms(step(3, objective=3), hp, None, hp, hp, hp, None, 16, None, 0, None) == -1
    assert lib.dmh_sampler_step_ms(step(3), hp, None, hp, None, hp, None, 16, None, 0, None) == -1       # no history
    assert lib.dmh_sampler_step_ms(step(3), hp, None, hp, hp, hp, None, 0, None, 0, None) == -1          # n <= 0
    assert lib.dmh_sampler_step_ms(step(3), hp, None, hp, hp, hp, None, 16, hp, 8, None) == -1           # keep, no model_null
    assert lib.dmh_sampler_step_ms_dev(None, hp, None, hp, hp, hp, None, 16, None, 0, None) == -1
    assert lib.dmh_sampler_step_ms_dev(hp, hp, None, hp, hp, hp, None, 16, hp, 8, None) == -1
    assert lib.dmh_sampler_step_ddp_ms_dev(hp, hp, hp, hp, None, None, None, 2, 3, 16, 4, 0, None) == -1   # no history
    assert lib.dmh_sampler_step_ddp_ms_dev(hp, hp, hp, hp, hp, None, None, 2, 3, 16, 4, 1, None) == -1     # cpad < 2 C
    assert lib.dmh_sampler_step_ddp_ms_dev(hp, hp, hp, hp, hp, None, None, 2, 3, 16, 4, 2, None) == -1     # self_cond
    assert b'dmh_sampler_step_ddp_ms_dev' in lib.dmh_last_error()
    # the existing step kernel keeps refusing the new mode
    assert lib.dmh_sampler_step(step(3), hp, None, hp, hp, hp, None, None, 16, None, 0, None) == -1
    assert b'bad enum' in lib.dmh_last_error()
    with pytest.raises(ValueError):
        ops.step_table([_lib.DmhStep(1, 0, 4, 1., 1., 1., 1., 1., 0., 0., 0.)], [0], 'cpu')
