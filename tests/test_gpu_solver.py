"""-m gpu: the second-order multistep sampler (``sampler = 'dpmpp_2m'``): its step kernels (dmh_sampler_step_ms, _ms_dev,
dmh_sampler_step_ddp_ms_dev) and both diffusion classes, eager and captured.

1. the three kernels against each other (bitwise) and against a float64 statement, at a size that takes the 1-pixel path and
   one that takes the 4-pixel path;
2. where every update is first order (S = 2, 3) the sampler IS DDIM at eta = 0: against the oracle's cfg_sample;
3. second-order entries (S = 8) and the unconditional class (S = 6) against a restatement written here: the oracle's network
   and predictions per step, the update in float64 from coefficients computed here;
4. the captured loop equals the eager loop, bitwise, output and generator;
5. dedup_dropped_rows and the keyed generator's row independence."""
import math

import pytest
import torch

from gpu_util import ReplayDeviceRng, dev, report
from detweights import det_state_dict, shapes_of
from oracle import diffusion as OD
from oracle import unet as OU

pytestmark = pytest.mark.gpu


def g(x):
    return x.to(dev())


def bits(x):
    return x.contiguous().view(torch.int32)


def same(a, b):
    """bitwise, NaN included"""
    return torch.equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------- 1. the kernels alone
RC, RM1, SA, S1M, C0, C1, C2, CS = 1.3, 0.8, 0.7, 0.6, 0.9, 0.3, -0.4, 3.


def _step(objective, clip, mode, c2):
    from dmhomo_amd import _lib
    return _lib.DmhStep(objective=objective, clip=clip, mode=mode, cond_scale=CS, sqrt_recip_ac=RC, sqrt_recipm1_ac=RM1,
                        sqrt_ac=SA, sqrt_1m_ac=S1M, c0=C0, c1=C1, c2=c2)


def _statement(step, mc, mn, keep, x, hist):
    """float64: guided blend (CFG:410, a dropped row's logits are the null logits), objective branch, clamp, update"""
    f = lambda name: float(getattr(step, name))              # (the fp32 values the kernel reads)
    mc, x, hist = mc.double(), x.double(), hist.double()
    if mn is not None:
        nl = mn.double()
        mo = mc if keep is None else torch.where(keep.bool().reshape(-1, 1, 1, 1), mc, nl)
        mo = nl + (mo - nl) * f('cond_scale')
    else:
        mo = mc
    if step.objective == 0:
        x0 = f('sqrt_recip_ac') * x - f('sqrt_recipm1_ac') * mo
    elif step.objective == 1:
        x0 = mo
    else:
        x0 = f('sqrt_ac') * x - f('sqrt_1m_ac') * mo
    if step.clip:
        x0 = x0.clamp(-1., 1.)
    if step.mode == 1:
        return x0, x0
    o = f('c0') * x0 + f('c1') * x
    if step.c2 != 0.:
        o = o + f('c2') * hist
    return o, x0


@pytest.mark.parametrize('shape', [(2, 3, 3, 5), (2, 3, 4, 5)], ids=['1-pixel', '4-pixel'])
def test_kernels_alone(shape):
    from dmhomo_amd import ops
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(3)
    mc0 = g(torch.randn(shape, generator=gen) * 1.5)
    mn = g(torch.randn(shape, generator=gen) * 1.5)
    x = g(torch.randn(shape, generator=gen))
    hist_rand = g(torch.randn(shape, generator=gen))
    keep = g(torch.tensor([1, 0], dtype=torch.uint8))        # row 1 dropped: its conditional logits are never read
    tcond = torch.zeros((B,), dtype=torch.int64, device=dev())
    mc = mc0.clone()
    mc[0, 1, 2, 3] = float('nan')                            # (a kept row)
    nan_at = torch.zeros(shape, dtype=torch.bool, device=dev())
    nan_at[0, 1, 2, 3] = True
    worst, checked = 0., 0
    for objective in (0, 1, 2):
        for clip in (0, 1):
            for guided in (True, False):
                for kind in ('first', 'second', 'last'):
                    mode = ops.MODE_LAST if kind == 'last' else ops.MODE_MULTISTEP
                    step = _step(objective, clip, mode, C2 if kind == 'second' else 0.)
                    hist0 = hist_rand if kind == 'second' else torch.full_like(x, float('nan'))
                    nl, kp = (mn, keep) if guided else (None, None)
                    what = (shape, objective, clip, guided, kind)
                    # the host-struct entry point, out of place
                    h_a = hist0.clone()
                    img_a, xs_a = ops.sampler_step_ms(step, mc, nl, x, h_a, want_x_start=True, keep=kp)
                    assert same(h_a, xs_a), what
                    # ... in place
                    h_b, img_b = hist0.clone(), x.clone()
                    ops.sampler_step_ms(step, mc, nl, img_b, h_b, out=img_b, keep=kp)
                    assert same(img_b, img_a) and same(h_b, xs_a), what
                    # the device-struct entry point (MODE_LAST belongs to the last entry of a table)
                    if kind == 'last':
                        steps, k = [_step(objective, clip, ops.MODE_MULTISTEP, 0.), step], 1
                    else:
                        steps, k = [step, _step(objective, clip, ops.MODE_LAST, 0.)], 0
                    table, tt, cursor, cur = ops.step_table(steps, [5, 0], dev())
                    ops.sampler_seek(cursor, k, table, tt, cur, tcond)
                    h_c, xs_c = hist0.clone(), torch.empty_like(x)
                    img_c = ops.sampler_step_ms_dev(cur, mc, nl, x, h_c, x_start=xs_c, keep=kp)
                    assert same(img_c, img_a) and same(xs_c, xs_a) and same(h_c, xs_a), what
                    h_d, img_d = hist0.clone(), x.clone()
                    ops.sampler_step_ms_dev(cur, mc, nl, img_d, h_d, out=img_d, keep=kp)
                    assert same(img_d, img_a) and same(h_d, xs_a), what
                    # NaN: the one in model_cond stays, the history's does not leak where c2 == 0
                    assert torch.equal(torch.isnan(img_a), nan_at) and torch.equal(torch.isnan(xs_a), nan_at), what
                    want_img, want_xs = _statement(step, mc, nl, kp, x, hist0)
                    for name, got, want in (('img', img_a, want_img), ('x_start', xs_a, want_xs)):
                        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=2e-5, equal_nan=True,
                                                   msg=lambda m: f'{what} {name}: {m}')
                        worst = max(worst, float((got.double() - want)[~nan_at].abs().max()))
                    # the unconditional loop's fused launch (no model_null): the same bits, plus the next network input
                    if not guided:
                        for sc in (False, True):
                            cin = C * (2 if sc else 1)
                            for cpad in ((cin + 3) // 4 * 4, (cin + 3) // 4 * 4 + 4):
                                h_e, img_e = hist0.clone(), x.clone()
                                xs_e = torch.full_like(x, 7.)
                                xin = torch.full((B, H, W, cpad), float('nan'), device=dev())
                                ops.sampler_step_ddp_ms_dev(cur, cursor, mc, img_e, h_e, x_start=xs_e, xin=xin, self_cond=sc)
                                assert same(img_e, img_a) and same(xs_e, xs_a) and same(h_e, xs_a), (what, sc, cpad)
                                want_in = (ops.assemble_input(xs_a, img_a, None, cpad=cpad) if sc
                                           else ops.assemble_input(img_a, None, None, cpad=cpad))
                                assert same(xin, want_in), (what, sc, cpad)   # (padding channels included: no NaN left there)
                        img_f, h_f = x.clone(), hist0.clone()
                        ops.sampler_step_ddp_ms_dev(cur, cursor, mc, img_f, h_f)       # img alone
                        assert same(img_f, img_a) and same(h_f, xs_a), what
                    checked += 1
    assert checked == 3 * 2 * 2 * 3
    print(f'[parity] multistep step kernels {shape}: max|hip - float64| = {worst:.3e} (gate rtol 1e-4 / atol 2e-5)')


def test_kernel_arguments_are_validated():
    from dmhomo_amd import _lib, ops
    x = torch.zeros((2, 3, 4, 4), device=dev())
    keep = torch.ones((2,), dtype=torch.uint8, device=dev())
    with pytest.raises(_lib.DmhError, match='enum'):         # a DDIM entry has no place in the multistep kernel
        ops.sampler_step_ms(_step(1, 0, ops.MODE_DDIM, 0.), x, None, x, x.clone())
    with pytest.raises(_lib.DmhError, match='keep'):
        ops.sampler_step_ms(_step(1, 0, ops.MODE_MULTISTEP, 0.), x, None, x, x.clone(), keep=keep)
    with pytest.raises(_lib.DmhError, match='enum'):         # ... and the existing step kernel keeps refusing mode 3
        ops.sampler_step(_step(1, 0, ops.MODE_MULTISTEP, 0.), x, None, x, x.clone())
    with pytest.raises(ValueError):
        ops.sampler_step_ms(_step(1, 0, ops.MODE_MULTISTEP, 0.), x, None, x, x[:1].clone())


# --------------------------------------------------------------------------------------------- the tiny models
def _cfg_model(drop=0.5, seed=0):
    from dmhomo_amd import cfg
    m = cfg.Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1, cond_drop_prob=drop)
    sd = det_state_dict(shapes_of(m), seed)
    m.load_state_dict(sd)
    return m.to(dev()), sd


def _cfg_diffusion(m, size=16, T=100, S=5, objective='pred_x0', schedule='cosine'):
    from dmhomo_amd import cfg
    return cfg.GaussianDiffusion(m, image_size=size, timesteps=T, sampling_timesteps=S, objective=objective,
                                 beta_schedule=schedule).to(dev())


def _cond_inputs(B, size, seed=9):
    gen = torch.Generator().manual_seed(seed)
    rf01 = torch.rand(B, 3, size, size, generator=gen)
    mk = (torch.rand(B, 1, size, size, generator=gen) > 0.4).float()
    fl = torch.randn(B, 2, size, size, generator=gen)
    return torch.zeros(B, dtype=torch.long), rf01, fl, mk


def _ddp_model(sc, seed=1):
    from dmhomo_amd import ddpm
    m = ddpm.Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=3, self_condition=sc)
    sd = det_state_dict(shapes_of(m), seed)
    m.load_state_dict(sd)
    return m.to(dev()), sd


def _coefficients(buf, T, S):
    """[(time, c0, c1, c2) or (time, None) for the entry that returns x0] in float64 from the fp32 alphas_cumprod"""
    abar = buf['alphas_cumprod'].double().tolist()
    lam = lambda t: 0.5 * (math.log(abar[t]) - math.log1p(-abar[t]))
    pairs = OD.ddim_time_pairs(T, S)
    upd = [(t, tn) for t, tn in pairs if tn >= 0]
    out = []
    for k, (t, tn) in enumerate(upd):
        h = lam(tn) - lam(t)
        base = math.sqrt(abar[tn]) * (1. - math.exp(-h))
        c1 = math.sqrt((1. - abar[tn]) / (1. - abar[t]))
        if k == 0 or k == len(upd) - 1:
            out.append((t, base, c1, 0.))
        else:
            r = (lam(t) - lam(upd[k - 1][0])) / h
            out.append((t, base * (1. + 0.5 / r), c1, -base * 0.5 / r))
    return out + [(pairs[-1][0], None)]


# --------------------------------------------------------------------------------------------- 2. first order == DDIM, eta 0
@pytest.mark.parametrize('S', [2, 3])
def test_first_order_equals_the_oracles_ddim_at_eta_zero(S):
    """at S = 2 and S = 3 no entry is second order (entry 0, and the last entry that updates), so the sampler must reproduce
    the reference's DDIM arithmetic at eta = 0 — and consume the initial noise and the class-dropout draws, nothing else"""
    m, sd = _cfg_model()
    d = _cfg_diffusion(m, S=S)
    c, rf01, fl, mk = _cond_inputs(2, 16)
    torch.manual_seed(4)
    rec = OD.RecordRng()
    with torch.no_grad():
        ref, _, _ = OD.cfg_sample(sd, OD.schedule_buffers(100, 'cosine'), c, rf01, fl, mk, image_size=16, channels=6,
                                  sampling_timesteps=S, objective='pred_x0', cond_scale=3., cond_drop_prob=0.5, eta=0., rng=rec)
    assert len(rec.draws) == 1 + S + (S - 1)
    draws = [x for i, x in enumerate(rec.draws) if i == 0 or x.dim() == 1]      # the per-step noise draws left out
    assert len(draws) == 1 + S
    d.sampler = 'dpmpp_2m'
    assert all(st.c2 == 0. for _, st, _ in d._dpmpp_steps(True, 3.))
    d.rng = ReplayDeviceRng(draws)
    img, _, _ = d.sample(g(c), g(rf01), g(fl), g(mk), cond_scale=3.)
    assert d.rng.i == len(draws)
    err, _ = report(f'dpmpp_2m S={S} (all first order) vs oracle DDIM eta=0', img.cpu(), ref)
    assert err <= 4e-4, err


# --------------------------------------------------------------------------------------------- 3. second order, restated
@pytest.mark.parametrize('objective,drop', [('pred_x0', 0.5), ('pred_v', 1.0)])
def test_second_order_entries_vs_restatement(objective, drop):
    T, S, B, cs = 100, 8, 2, 3.
    m, sd = _cfg_model(drop)
    d = _cfg_diffusion(m, T=T, S=S, objective=objective)
    d.sampler = 'dpmpp_2m'
    c, rf01, fl, mk = _cond_inputs(B, 16)
    gen = torch.Generator().manual_seed(21)
    shape = (B, 6, 16, 16)
    noise = torch.randn(shape, generator=gen)
    uniforms = [torch.rand(B, generator=gen) for _ in range(S)] if 0 < drop < 1 else []
    buf = OD.schedule_buffers(T, 'cosine')
    coef = _coefficients(buf, T, S)
    assert sum(1 for e in coef if e[1] is not None and e[3] != 0.) == S - 3     # the second-order entries
    rgbn = rf01 * 2 - 1
    img, prev, ref_xs = noise, None, []
    with torch.no_grad():
        for k, entry in enumerate(coef):
            t = torch.full((B,), entry[0], dtype=torch.long)
            keep = (uniforms[k] < 1 - drop) if uniforms else torch.zeros(B, dtype=torch.bool)
            out = OU.cfg_unet_forward_with_cond_scale(sd, img, t, c, rgbn, mk, keep, cs)
            _, x0 = OD._predictions(buf, objective, out, img, t, True)
            ref_xs.append(x0)
            if entry[1] is None:
                img = x0
            else:
                _, c0, c1, c2 = entry
                o = c1 * img.double() + c0 * x0.double()
                img = (o + c2 * prev.double() if c2 != 0. else o).float()
            prev = x0
    ref = (img + 1) * 0.5
    from dmhomo_amd import ops
    d.rng = ReplayDeviceRng([noise] + uniforms)
    trace = []
    got, _, _ = d._dpmpp_sample(g(c), ops.affine(g(rf01), 2., -1.), g(fl), g(mk), shape, cs, trace=trace)
    assert d.rng.i == 1 + len(uniforms) and len(trace) == S
    drift = [float((a['x_start'].cpu() - b).abs().max()) for a, b in zip(trace, ref_xs)]
    print(f'[parity] dpmpp_2m S={S} {objective} drop={drop}: per-step max|x_start - restatement| = '
          + ' '.join(f'{e:.1e}' for e in drift))
    err, _ = report(f'dpmpp_2m S={S} {objective} drop={drop} img', got.cpu(), ref)
    assert max(drift) <= 4e-4 and err <= 4e-4, (max(drift), err)
    # sample() is the same call
    d.rng = ReplayDeviceRng([noise] + uniforms)
    assert torch.equal(d.sample(g(c), g(rf01), g(fl), g(mk), cond_scale=cs)[0], got)


@pytest.mark.parametrize('sc', [False, True], ids=['nosc', 'sc'])
def test_unconditional_class_vs_restatement(sc):
    """ddpm.GaussianDiffusion with the solver: ddim_sample's loop and output mapping (the last two channels x 512, DDP:728,
    so their gate is 512 x the image gate)"""
    from dmhomo_amd import ddpm
    T, S, B = 100, 6, 2
    m, sd = _ddp_model(sc)
    d = ddpm.GaussianDiffusion(m, image_size=16, timesteps=T, sampling_timesteps=S, objective='pred_x0').to(dev())
    d.sampler = 'dpmpp_2m'
    shape = (B, 3, 16, 16)
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(31))
    buf = OD.schedule_buffers(T, 'cosine')
    img, prev, x0 = noise, None, None
    with torch.no_grad():
        for entry in _coefficients(buf, T, S):
            t = torch.full((B,), entry[0], dtype=torch.long)
            out = OD._ddp_model(sd, img, t, x0 if sc else None, sc, 8)
            _, x0 = OD._predictions(buf, 'pred_x0', out, img, t, True)
            if entry[1] is None:
                img = x0
            else:
                _, c0, c1, c2 = entry
                o = c1 * img.double() + c0 * x0.double()
                img = (o + c2 * prev.double() if c2 != 0. else o).float()
            prev = x0
    ref = ((img + 1) * 0.5).clone()
    ref[:, -2:] = (ref[:, -2:] * 2 - 1) * 512
    d.rng = ReplayDeviceRng([noise])
    got = d.sample(batch_size=B).cpu()
    assert d.rng.i == 1
    e_img, _ = report(f'dpmpp_2m unconditional S={S} sc={sc} image channels', got[:, :-2], ref[:, :-2])
    e_flow, _ = report(f'dpmpp_2m unconditional S={S} sc={sc} flow channels (x512)', got[:, -2:], ref[:, -2:])
    assert e_img <= 4e-4 and e_flow <= 4e-4 * 512, (e_img, e_flow)


# --------------------------------------------------------------------------------------------- 4. captured == eager
@pytest.mark.parametrize('S,size', [(6, 32), (1, 16)])
@pytest.mark.parametrize('which', ['cfg-batched', 'cfg-streams', 'ddp', 'ddp-sc'])
def test_captured_equals_eager(which, S, size):
    """bitwise, output and generator (left where the eager loop leaves it): the capturing call, new inputs on the same graph,
    the sampler switched to 'ddim' and back (one capture each), a weight update"""
    from dmhomo_amd import cfg, ddpm
    B = 2
    if which.startswith('cfg'):
        m, sd = _cfg_model()
        m.cfg_mode = which.split('-')[1]
        d = _cfg_diffusion(m, size=size, T=100, S=S)
        ins = {3: [g(t) for t in _cond_inputs(B, size, 9)], 4: [g(t) for t in _cond_inputs(B, size, 10)]}
        call = lambda seed: d.sample(*ins[seed])[0]
        head = 'final_conv'
    else:
        m, sd = _ddp_model(which == 'ddp-sc')
        d = ddpm.GaussianDiffusion(m, image_size=size, timesteps=100, sampling_timesteps=S, objective='pred_noise').to(dev())
        call = lambda seed: d.sample(batch_size=B)
        head = 'final_conv'
    d.rng = cfg.DeviceRng()

    def run(graph, seed):
        d.hip_graph = graph
        torch.manual_seed(seed)
        out = call(seed).clone()
        return out, torch.rand(4, device=dev())

    def check(got, want, what):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (which, S, what)
    d.sampler = 'dpmpp_2m'
    e3, e4 = run(False, 3), run(False, 4)
    assert not torch.equal(e3[0], e4[0])
    check(run(True, 3), e3, 'the capturing call')
    check(run(True, 4), e4, 'new inputs on the same graph')
    assert d.graph_captures == 1
    d.sampler = 'ddim'
    ed = run(False, 3)
    assert torch.equal(ed[0], e3[0]) == (S == 1)             # (one step: both return its x_start)
    check(run(True, 3), ed, 'ddim, capturing')
    assert d.graph_captures == 2
    d.sampler = 'dpmpp_2m'
    check(run(True, 3), e3, 'back on the solver')
    d.sampler = 'ddim'
    check(run(True, 4), run(False, 4), 'back on ddim')
    assert d.graph_captures == 2                              # each sampler captured once
    d.sampler = 'dpmpp_2m'
    m.load_state_dict({k: v * 1.01 if k.startswith(head) else v for k, v in sd.items()})
    e3b = run(False, 3)
    assert not torch.equal(e3b[0], e3[0])
    check(run(True, 3), e3b, 'after a weight update')
    assert d.graph_captures == 3
    d.hip_graph = False
    if which.startswith('cfg'):
        m.cfg_mode = 'batched'


# --------------------------------------------------------------------------------------------- 5. switches
def test_dedup_and_row_independence_with_the_keyed_generator():
    """dedup_dropped_rows on == off, and a B = 3 call == the three B = 1 calls with the same global sample ids (bitwise); a
    call consumes the initial noise and one uniform draw per step, nothing else"""
    from dmhomo_amd import cfg
    S, B = 6, 3
    m, _ = _cfg_model()
    d = _cfg_diffusion(m, size=16, T=100, S=S)
    d.sampler = 'dpmpp_2m'
    c, rf01, fl, mk = (g(t) for t in _cond_inputs(B, 16))
    d.rng = cfg.DeviceRng()

    def run(lo, hi):
        d.rng.key_by_sample(5, range(40 + lo, 40 + hi), dev())
        out = d.sample(c[lo:hi].contiguous(), rf01[lo:hi].contiguous(), fl[lo:hi].contiguous(), mk[lo:hi].contiguous())[0]
        assert d.rng.state.tolist()[1] == 1 + S               # draw index: the initial noise + S class-dropout draws
        return out.clone()
    whole = run(0, B)
    assert not torch.equal(whole[0], whole[1])
    for b in range(B):
        assert torch.equal(run(b, b + 1)[0], whole[b]), b
    m.dedup_dropped_rows = True
    assert torch.equal(run(0, B), whole)
    d.hip_graph = True
    assert torch.equal(run(0, B), whole)                      # ... and captured, with the dropped rows skipped
    m.cfg_mode = 'streams'
    assert torch.equal(run(0, B), whole)
    d.hip_graph, m.dedup_dropped_rows, m.cfg_mode = False, False, 'batched'
