"""CPU: the host side of the replayed conditional sampler (cfg.GaussianDiffusion.hip_graph).

The step / timestep / draws tables that the captured step reads through its cursor must hold, entry by entry, exactly the
DmhStep, the timestep and the "draws noise" decision that the eager _ddim_sample passes at the same step.  The eager loop
runs here with the network, the step kernel and the generator stubbed out (recording what they are handed), so no GPU is
needed."""
import pytest
import torch

from dmhomo_amd import _lib, cfg, ops

FIELDS = [f for f, _ in _lib.DmhStep._fields_]


def fields(step):
    return tuple(getattr(step, f) for f in FIELDS)


def eager_record(d, cond_scale, monkeypatch):
    """(steps, times, draws) _ddim_sample passes, recorded from its calls"""
    rec, times = [], []

    def fake_network(x, t, classes, rgb_flow, mask, cs):
        assert cs == cond_scale
        times.append(int(t[0]))
        return torch.zeros_like(x), (None if cs == 1 else torch.zeros_like(x)), None

    def fake_step(step, model_cond, model_null, x, noise, want_x_start=True, want_pred_noise=False, keep=None):
        rec.append((fields(step), int(noise is not None)))
        return x.clone(), x.clone(), None

    class Rng:
        def randn(self, shape, device):
            return torch.zeros(tuple(shape))
    monkeypatch.setattr(d, '_network', fake_network)
    monkeypatch.setattr(ops, 'sampler_step', fake_step)
    monkeypatch.setattr(ops, 'affine', lambda x, a, b, out=None: x)
    d.rng = Rng()
    B, S = 2, d.image_size
    shape = (B, d.channels, S, S)
    classes = torch.zeros(B, dtype=torch.long)
    d._ddim_sample(classes, torch.zeros((B, 3, S, S)), torch.zeros((B, 2, S, S)), torch.zeros((B, 1, S, S)), shape,
                   cond_scale)
    return [r[0] for r in rec], times, [r[1] for r in rec]


@pytest.mark.parametrize('objective', ['pred_noise', 'pred_x0', 'pred_v'])
@pytest.mark.parametrize('T,S,eta,cond_scale', [(20, 5, 1., 3.), (20, 4, 0.3, 1.), (10, 1, 1., 3.), (1000, 8, 1., 3.),
                                                (1000, 32, 0., 2.5)])
def test_tables_match_the_eager_loop(T, S, eta, cond_scale, objective, monkeypatch):
    m = cfg.Unet(dim=8, dim_mults=(1, 2), channels=6, num_classes=1)
    d = cfg.GaussianDiffusion(m, image_size=8, timesteps=T, sampling_timesteps=S, objective=objective,
                              ddim_sampling_eta=eta)
    steps, times, draws = d._graph_tables(cond_scale)
    want_steps, want_times, want_draws = eager_record(d, cond_scale, monkeypatch)
    assert len(steps) == len(want_steps) == S
    assert [fields(s) for s in steps] == want_steps           # bitwise: the same floats, entry by entry
    assert times == want_times and draws == want_draws
    assert draws == [1] * (S - 1) + [0] and steps[-1].mode == ops.MODE_LAST
    assert all(s.mode == ops.MODE_DDIM for s in steps[:-1])
    assert all(s.objective == ops.OBJECTIVE[objective] and s.clip == 1 and s.cond_scale == cond_scale for s in steps)


def test_graph_is_off_by_default():
    m = cfg.Unet(dim=8, dim_mults=(1, 2), channels=6, num_classes=1)
    d = cfg.GaussianDiffusion(m, image_size=8, timesteps=10, sampling_timesteps=5)
    assert cfg.GaussianDiffusion.hip_graph is False and d.graph_captures == 0 and d.graph_cache_size >= 1
