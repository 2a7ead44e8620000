"""CPU: the host side of the replayed unconditional sampler (ddpm.GaussianDiffusion.hip_graph).

The step / timestep / draws tables that the captured step reads through its cursor must hold, entry by entry, exactly the
DmhStep, the timestep and the "draws noise" decision that the eager p_sample_loop / ddim_sample pass at the same step.  The
eager loops run here with the network, the step kernel and the generator stubbed out (recording what they are handed), so
no GPU is needed.  The fused step's entry point answers bad arguments through the error channel before any launch."""
import ctypes

import pytest
import torch

from dmhomo_amd import _lib, ddpm, ops

FIELDS = [f for f, _ in _lib.DmhStep._fields_]


def fields(step):
    return tuple(getattr(step, f) for f in FIELDS)


def eager_record(d, kind, monkeypatch):
    """(steps, times, draws) the eager loop passes, recorded from its calls"""
    rec, times = [], []

    def fake_model(x, t, x_self_cond=None):
        times.append(int(t[0]))
        return torch.zeros_like(x)

    def fake_step(step, model_cond, model_null, x, noise, want_x_start=True, want_pred_noise=False, keep=None):
        rec.append((fields(step), int(noise is not None)))
        return x.clone(), x.clone(), None

    class Rng:
        def randn(self, shape, device):
            return torch.zeros(tuple(shape))
    monkeypatch.setattr(d.model, 'forward', fake_model)
    monkeypatch.setattr(ops, 'sampler_step', fake_step)
    monkeypatch.setattr(ops, 'affine', lambda x, a, b, out=None: x)
    monkeypatch.setattr(ops, 'affine_tail_', lambda x, c0, a, b: None)
    d.rng = Rng()
    shape = (2, d.channels, d.image_size, d.image_size)
    d.p_sample_loop(shape) if kind == 'ddpm' else d.ddim_sample(shape)
    return [r[0] for r in rec], times, [r[1] for r in rec]


@pytest.mark.parametrize('objective', ['pred_noise', 'pred_x0', 'pred_v'])
@pytest.mark.parametrize('kind,T,S,eta', [('ddpm', 12, None, 1.), ('ddim', 20, 5, 1.), ('ddim', 20, 4, 0.3), ('ddim', 10, 1, 1.)])
def test_tables_match_the_eager_loop(kind, T, S, eta, objective, monkeypatch):
    m = ddpm.Unet(dim=8, dim_mults=(1, 2), channels=3, self_condition=True)
    d = ddpm.GaussianDiffusion(m, image_size=8, timesteps=T, sampling_timesteps=S, objective=objective,
                               ddim_sampling_eta=eta)
    assert d.is_ddim_sampling == (kind == 'ddim')
    steps, times, draws = d._graph_tables(kind)
    want_steps, want_times, want_draws = eager_record(d, kind, monkeypatch)
    assert len(steps) == len(want_steps) == (T if kind == 'ddpm' else S)
    assert [fields(s) for s in steps] == want_steps           # bitwise: the same floats, entry by entry
    assert times == want_times and draws == want_draws
    if kind == 'ddpm':
        assert times == list(range(T - 1, -1, -1)) and draws == [1] * (T - 1) + [0]
        assert all(s.mode == ops.MODE_DDPM for s in steps)
    else:
        assert draws == [1] * (S - 1) + [0] and steps[-1].mode == ops.MODE_LAST
    assert all(s.objective == ops.OBJECTIVE[objective] and s.clip == 1 for s in steps)


def test_graph_is_off_by_default_and_needs_the_device_generator():
    m = ddpm.Unet(dim=8, dim_mults=(1, 2), channels=3)
    d = ddpm.GaussianDiffusion(m, image_size=8, timesteps=10)
    assert ddpm.GaussianDiffusion.hip_graph is False and not d._graphed()
    d.hip_graph = True
    assert not d._graphed()                                   # CPU buffers: no graph
    assert d.graph_captures == 0 and d.graph_cache_size >= 1
    with pytest.raises(ValueError):
        d._graph_tables('ancestral')


def test_fused_step_rejects_bad_arguments():
    """every refusal happens in host-side validation, before a launch (host pointers: nothing here may pass validation)"""
    lib = _lib.lib()
    fn = lib.dmh_sampler_step_ddp_dev
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(**kw):
        a = dict(cur=p, cursor=p, draws=p, mo=p, img=p, noise=None, ids=p, state=p, xs=None, xin=p, B=2, C=3, HW=64, cpad=4,
                 sc=0)
        a.update(kw)
        rc = fn(a['cur'], a['cursor'], a['draws'], a['mo'], a['img'], a['noise'], a['ids'], a['state'], a['xs'], a['xin'],
                a['B'], a['C'], a['HW'], a['cpad'], a['sc'], None)
        return rc, lib.dmh_last_error().decode()
    for null in ('cur', 'cursor', 'draws', 'mo', 'img'):
        rc, msg = call(**{null: None})
        assert rc != 0 and 'dmh_sampler_step_ddp_dev' in msg, null
    for bad in (dict(B=0), dict(B=-1), dict(C=0), dict(HW=0), dict(HW=-5), dict(sc=2),
                dict(cpad=2), dict(cpad=6), dict(sc=1, cpad=4),                  # cpad < channels / not a multiple of 4
                dict(B=2 ** 30, HW=2 ** 30), dict(B=65535, HW=2 ** 30, C=3),      # B*HW*cpad overflows
                dict(C=2 ** 30, HW=2 ** 30, cpad=2 ** 30),
                dict(noise=p),                                                     # two noise sources
                dict(state=None), dict(ids=None)):                                 # half a keyed generator
        rc, msg = call(**bad)
        assert rc == -1 and 'dmh_sampler_step_ddp_dev' in msg, (bad, rc, msg)
