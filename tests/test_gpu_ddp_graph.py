"""-m gpu: the replayed unconditional sampler (ddpm.GaussianDiffusion.hip_graph) and its fused step kernel
(dmh_sampler_step_ddp_dev).

1. one fused launch == rng_indexed -> sampler_step_dev -> assemble_input, bitwise (img, x_start, the padded input with its
   zero channels, the generator state), for every objective / mode / clip / self-conditioning / noise source, at odd sizes;
2. the graphed p_sample_loop / ddim_sample == the eager loops, bitwise, output and generator state, keyed and unkeyed;
3. the F6 geometry (p_sample_loop T = 10, ddim_sample S = 4) replayed through the graph against the CPU oracle at F6's
   tolerances.  The stored F6 draws cannot feed the graph: ReplayDeviceRng hands over recorded host tensors one call at a
   time, and a captured step replays one launch sequence whose noise must come from device state.  So the oracle gets the
   keyed generator's own draws (recorded with ops.rng_indexed), and item 2 ties the graph to the eager path F6 pins;
4. the capture cache: replays, re-captures after a weight update (dropping the stale entry), one capture per batch shape;
5. after capture the eager per-step path is never entered."""

import pytest
import torch

from gpu_util import dev
from detweights import det_state_dict, shapes_of
from oracle import diffusion as OD

pytestmark = pytest.mark.gpu


def _lincomb_step(objective, clip, mode):
    from dmhomo_amd import _lib
    return _lib.DmhStep(objective=objective, clip=clip, mode=mode, cond_scale=1., sqrt_recip_ac=1.3, sqrt_recipm1_ac=0.8,
                        sqrt_ac=0.7, sqrt_1m_ac=0.6, c0=0.9, c1=0.3, c2=0.2)


def _three_launches(cur, mo, img0, noise, sc, cpad):
    """the eager sequence the fused kernel replaces: sampler_step_dev (with x_start) then assemble_input"""
    from dmhomo_amd import ops
    img, xs = torch.empty_like(img0), torch.empty_like(img0)
    ops.call('dmh_sampler_step_dev', ops.ptr(cur, torch.uint8), ops.ptr(mo), None, ops.ptr(img0), ops.ptr(noise), ops.ptr(img),
             ops.ptr(xs), None, img0.numel(), None, img0.numel() // img0.shape[0])
    xin = ops.assemble_input(xs, img, None, cpad=cpad) if sc else ops.assemble_input(img, None, None, cpad=cpad)
    return img, xs, xin


@pytest.mark.parametrize('shape', [(3, 3, 40, 24), (2, 6, 16, 16), (2, 3, 5, 7)])
def test_fused_step_equals_three_launches(shape):
    from dmhomo_amd import ops
    torch.manual_seed(0)
    B, C, H, W = shape
    mo = torch.randn(shape, device=dev()) * 1.5
    img0 = torch.randn(shape, device=dev())
    ext_noise = torch.randn(shape, device=dev())
    ids = torch.arange(100, 100 + B, dtype=torch.int64, device=dev())
    state0 = torch.tensor([1234, 7, 0, 0], dtype=torch.int64, device=dev())
    tcond = torch.zeros((B,), dtype=torch.int64, device=dev())
    checked = 0
    for objective in (0, 1, 2):
        for clip in (0, 1):
            for mode in (ops.MODE_DDPM, ops.MODE_DDIM, ops.MODE_LAST):
                step = _lincomb_step(objective, clip, mode)
                if mode == ops.MODE_LAST:
                    steps, k = [_lincomb_step(objective, clip, ops.MODE_DDIM), step], 1
                else:
                    steps, k = [step, _lincomb_step(objective, clip, ops.MODE_LAST)], 0
                table, tt, cursor, cur = ops.step_table(steps, [5, 0], dev())
                ops.sampler_seek(cursor, k, table, tt, cur, tcond)
                # drawing entries (DDPM t > 0, DDIM), and the no-draw entries (DDPM t == 0, LAST)
                for drawn in ((1, 0) if mode == ops.MODE_DDPM else ((1,) if mode == ops.MODE_DDIM else (0,))):
                    flags = [0, 0]
                    flags[k] = drawn
                    draws = torch.tensor(flags, dtype=torch.int32, device=dev())
                    for keyed in (True, False):
                        for sc in (False, True):
                            cpad = (C * (2 if sc else 1) + 3) // 4 * 4
                            st_ref = state0.clone()
                            noise = None
                            if drawn:
                                noise = ops.rng_indexed(shape, ids, st_ref) if keyed else ext_noise
                            img_r, xs_r, xin_r = _three_launches(cur, mo, img0, noise, sc, cpad)
                            st_f = state0.clone()
                            img = img0.clone()
                            xs = torch.full_like(img0, float('nan'))
                            xin = torch.full((B, H, W, cpad), float('nan'), device=dev())
                            ops.sampler_step_ddp_dev(cur, cursor, draws, mo, img, None if keyed else ext_noise,
                                                     ids if keyed else None, st_f if keyed else None, x_start=xs, xin=xin,
                                                     self_cond=sc)
                            what = (shape, objective, clip, mode, drawn, keyed, sc)
                            assert torch.equal(img, img_r), what
                            assert torch.equal(xs, xs_r), what
                            assert torch.equal(xin, xin_r), what          # padding channels included (no NaN left)
                            assert torch.equal(st_f, st_ref), what
                            if not drawn:
                                assert torch.equal(st_f, state0), what    # no draw, no advance
                            checked += 1
    assert checked == 3 * 2 * (2 + 1 + 1) * 2 * 2
    # no x_start / xin requested: img alone, same values
    table, tt, cursor, cur = ops.step_table([_lincomb_step(2, 1, ops.MODE_DDPM)], [3], dev())
    ops.sampler_seek(cursor, 0, table, tt, cur, tcond)
    draws = torch.ones((1,), dtype=torch.int32, device=dev())
    img_r, _, _ = _three_launches(cur, mo, img0, ext_noise, False, (C + 3) // 4 * 4)
    img = img0.clone()
    ops.sampler_step_ddp_dev(cur, cursor, draws, mo, img, ext_noise)
    assert torch.equal(img, img_r)


def test_fused_step_draws_advance_across_launches():
    """two drawing launches = two rng_indexed draws (the draw index advances once per launch, tickets put back)"""
    from dmhomo_amd import ops
    shape = (3, 3, 40, 24)
    mo, img0 = torch.randn(shape, device=dev()), torch.randn(shape, device=dev())
    ids = torch.tensor([5, 9, 2], dtype=torch.int64, device=dev())
    table, tt, cursor, cur = ops.step_table([_lincomb_step(0, 1, ops.MODE_DDPM)], [3], dev())
    ops.sampler_seek(cursor, 0, table, tt, cur, torch.zeros((3,), dtype=torch.int64, device=dev()))
    draws = torch.ones((1,), dtype=torch.int32, device=dev())
    s_ref = torch.tensor([77, 0, 0, 0], dtype=torch.int64, device=dev())
    s_f = s_ref.clone()
    img_r, img = img0.clone(), img0.clone()
    for _ in range(2):
        img_r, _, _ = _three_launches(cur, mo, img_r, ops.rng_indexed(shape, ids, s_ref), False, 4)
        ops.sampler_step_ddp_dev(cur, cursor, draws, mo, img, None, ids, s_f)
    assert torch.equal(img, img_r) and torch.equal(s_f, s_ref) and s_f.tolist() == [77, 2, 0, 0]


def _ddp(dim, sc, seed=1, channels=3):
    from dmhomo_amd import ddpm
    m = ddpm.Unet(dim=dim, dim_mults=(1, 2, 4, 8), channels=channels, self_condition=sc)
    sd = det_state_dict(shapes_of(m), seed)
    m.load_state_dict(sd)
    return m.to(dev()), sd


def _diffusion(m, kind, objective, T=10, S=4, size=16):
    from dmhomo_amd import ddpm
    return ddpm.GaussianDiffusion(m, image_size=size, timesteps=T, sampling_timesteps=S if kind == 'ddim' else None,
                                  objective=objective).to(dev())


@pytest.mark.parametrize('kind', ['ddpm', 'ddim'])
@pytest.mark.parametrize('sc', [False, True])
@pytest.mark.parametrize('objective', ['pred_noise', 'pred_x0', 'pred_v'])
def test_graph_equals_eager(kind, sc, objective):
    from dmhomo_amd import cfg
    m, _ = _ddp(8, sc)
    d = _diffusion(m, kind, objective)
    d.rng = cfg.DeviceRng()

    def keyed(graph, seed):
        d.hip_graph = graph
        d.rng.key_by_sample(seed, range(40, 42), dev())
        out = d.sample(batch_size=2)
        return out, d.rng.state.clone()

    def unkeyed(graph, seed):
        d.hip_graph = graph
        torch.manual_seed(seed)
        out = d.sample(batch_size=2)
        return out, torch.rand(4, device=dev())          # the torch generator is left where the eager loop leaves it
    for run in (keyed, unkeyed):
        d.rng = cfg.DeviceRng()
        e1, e2 = run(False, 3), run(False, 4)
        assert not torch.equal(e1[0], e2[0])
        for got, want in ((run(True, 3), e1), (run(True, 4), e2), (run(True, 3), e1)):   # capturing call, then replays
            assert torch.equal(got[0], want[0]), (run.__name__, kind, sc, objective)
            assert torch.equal(got[1], want[1]), (run.__name__, kind, sc, objective)
        assert d.graph_captures == (1 if run is keyed else 2)
    # a second call from where the first one left the generator also matches
    d.rng = cfg.DeviceRng().key_by_sample(9, range(2), dev())
    d.hip_graph = False
    a1, a2 = d.sample(batch_size=2), d.sample(batch_size=2)
    d.rng.key_by_sample(9, range(2), dev())
    d.hip_graph = True
    assert torch.equal(d.sample(batch_size=2), a1) and torch.equal(d.sample(batch_size=2), a2)
    d.hip_graph = False


@pytest.mark.parametrize('tag', ['nosc', 'sc'])
def test_graph_vs_oracle_at_the_golden_geometry(tag):
    """F6's geometry and tolerances (tests/test_gpu_unet.py::test_ddpm_trace_vs_golden) through the graph, the oracle fed
    the keyed generator's draws"""
    from dmhomo_amd import cfg, ops
    sc = tag == 'sc'
    m, sd = _ddp(8, sc)
    shape, ids = (2, 3, 16, 16), torch.arange(2, dtype=torch.int64, device=dev())

    def draws(seed, n):
        st = torch.tensor([seed, 0, 0, 0], dtype=torch.int64, device=dev())
        return [ops.rng_indexed(shape, ids, st).cpu() for _ in range(n)]
    d = _diffusion(m, 'ddpm', 'pred_noise')
    d.hip_graph, d.rng = True, cfg.DeviceRng().key_by_sample(21, range(2), dev())
    got = d.sample(batch_size=2).cpu()
    assert d.graph_captures == 1
    with torch.no_grad():
        ref = OD.ddp_p_sample_loop(sd, OD.schedule_buffers(10, 'cosine'), shape, self_condition=sc, objective='pred_noise',
                                   rng=OD.ReplayRng(draws(21, 10)))
    torch.testing.assert_close(got, ref, rtol=0, atol=1e-3 if sc else 1e-4)
    d2 = _diffusion(m, 'ddim', 'pred_x0')
    d2.hip_graph, d2.rng = True, cfg.DeviceRng().key_by_sample(22, range(2), dev())
    got = d2.sample(batch_size=2).cpu()
    assert d2.graph_captures == 1
    with torch.no_grad():
        ref = OD.ddp_ddim_sample(sd, OD.schedule_buffers(10, 'cosine'), shape, sampling_timesteps=4, objective='pred_x0',
                                 self_condition=sc, rng=OD.ReplayRng(draws(22, 4)))
    torch.testing.assert_close(got[:, :-2], ref[:, :-2], rtol=0, atol=2e-4)
    torch.testing.assert_close(got[:, -2:], ref[:, -2:], rtol=0, atol=6e-2)


def test_graph_cache():
    from dmhomo_amd import cfg
    m, sd = _ddp(8, True)
    d = _diffusion(m, 'ddim', 'pred_v')
    d.rng = cfg.DeviceRng()

    def run(graph, n, seed=5):
        d.hip_graph = graph
        d.rng.key_by_sample(seed, range(60, 63), dev())
        return d.sample(batch_size=n)
    e3, e2 = run(False, 3), run(False, 2)
    assert torch.equal(run(True, 3), e3) and d.graph_captures == 1
    assert torch.equal(run(True, 3), e3) and d.graph_captures == 1            # same shape: replayed, not captured
    cache = d.__dict__['_graph_states']
    old = list(cache)
    # a weight update: re-capture, the new weights' result, the stale entry gone
    sd2 = {k: v * 1.01 if k.startswith('final_conv') else v for k, v in sd.items()}
    m.load_state_dict(sd2)
    e3b = run(False, 3)
    assert not torch.equal(e3b, e3)
    assert torch.equal(run(True, 3), e3b) and d.graph_captures == 2
    assert len(cache) == 1 and not any(k in cache for k in old)
    # alternating batch shapes: one capture each
    for _ in range(2):
        assert torch.equal(run(True, 2), run(False, 2))
        assert torch.equal(run(True, 3), e3b)
    assert d.graph_captures == 3 and len(cache) == 2
    d.hip_graph = False


@pytest.mark.parametrize('kind', ['ddpm', 'ddim'])
def test_graph_replays_without_the_eager_step(kind, monkeypatch):
    """hip_graph = True: neither the eager step kernel wrapper, p_sample nor Unet.forward run — not while capturing, not on
    replay (the eager loop would call all three every step)"""
    from dmhomo_amd import cfg, ddpm, ops
    m, _ = _ddp(8, True)
    d = _diffusion(m, kind, 'pred_noise')
    d.rng = cfg.DeviceRng().key_by_sample(3, range(2), dev())
    want = d.sample(batch_size=2)
    d.rng.key_by_sample(3, range(2), dev())

    def boom(*a, **k):
        raise AssertionError('the eager per-step path ran')
    monkeypatch.setattr(ops, 'sampler_step', boom)
    monkeypatch.setattr(ddpm.GaussianDiffusion, 'p_sample', boom)
    monkeypatch.setattr(ddpm.Unet, 'forward', boom)
    d.hip_graph = True
    assert torch.equal(d.sample(batch_size=2), want)
    d.rng.key_by_sample(3, range(2), dev())
    assert torch.equal(d.sample(batch_size=2), want)
    assert d.graph_captures == 1
    st = d.__dict__['_graph_state']
    assert st['nsteps'] == (10 if kind == 'ddpm' else 4)
