"""Conditional sampler: the guided blend as it is against adaptive projected guidance (``apg_eta``), in ms per denoise step, and
the three launches of APG (dmh_apg_coef's two, dmh_apg_apply) alone.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, cond_scale 3, cfg_mode 'streams', the captured step, noise
keyed by sample id, random weights, the static clamp — for six settings: {ddim, dpmpp_2m} x {off, eta 0, eta 0 with a norm
threshold and momentum -0.5}.  The six run interleaved in one process (round-robin, --rounds times, after a warm-up call each
that also captures), each call timed with a host clock around work that ends in a device synchronise; the median per setting
is reported with the spread.  Then the launches alone, by HIP events around --reps back-to-back calls after a warm-up, at (25,
98304) and (25, 393216) on N(0, 1.5) logits, without and with the running average.  Writes profiles/apg.json and prints the
same JSON line.  A measurement tool: nothing gates on it, and it says nothing about sample quality.  Not bench.py: that is the
project's yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

RHO, BETA = 100., -0.5
APG = {'off': None, 'eta0': (0., 0., 0.), 'eta0+rho+momentum': (0., RHO, BETA)}
SETTINGS = tuple((name, apg) for name in ('ddim', 'dpmpp_2m') for apg in APG)
SHAPES = ((25, 98304), (25, 393216))


def _timed(fn, reps):
    """us per call: the median of five batches of back-to-back calls between HIP events, after a warm-up"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(per), [round(min(per), 2), round(max(per), 2)]


def launches_alone(dev, reps):
    from dmhomo_amd import _lib, ops
    rows = []
    step = _lib.DmhStep(objective=1, clip=1, mode=ops.MODE_LAST, cond_scale=3., sqrt_recip_ac=1., sqrt_recipm1_ac=1., sqrt_ac=1.,
                        sqrt_1m_ac=1., c0=0., c1=0., c2=0.)
    for B, n in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        cond = torch.randn((B, n), device=dev, generator=gen) * 1.5
        null = torch.randn((B, n), device=dev, generator=gen) * 1.5
        ws, coef, guided = ops.apg_workspace(cond), torch.empty((B, 2), device=dev), torch.empty_like(cond)
        for beta in (0., BETA):
            run = torch.zeros_like(cond) if beta != 0. else None
            rho = 2. * n ** 0.5                                  # (|d| is about 2.1 sqrt(n): the cap binds)
            us_c, mm_c = _timed(lambda: ops.apg_coef(step, cond, null, 0., rho, beta, run=run, ws=ws, coef=coef), reps)
            us_a, mm_a = _timed(lambda: ops.apg_apply(cond, null, coef, run=run, out=guided), reps)
            if run is None:                                  # the orthogonal update: <guided - c, c> == 0
                upd = guided.double() - cond.double()
                dot = (upd * cond.double()).sum(dim=1).abs() / (upd.norm(dim=1) * cond.double().norm(dim=1))
                assert float(dot.max()) <= 1e-6 and bool((upd.norm(dim=1) <= 2. * rho * (1. + 1e-6)).all())
            assert bool(torch.isfinite(guided).all())
            moved_c = (2 + (2 if run is not None else 0)) * B * n * 4        # cond, null (+ run read and written)
            moved_a = (3 + (1 if run is not None else 0)) * B * n * 4        # cond, null (+ run), guided written
            rows.append({'B': B, 'n': n, 'momentum': beta, 'splits': ops.apg_splits(B, n),
                         'coef_us_per_call': round(us_c, 2), 'coef_us_min_max': mm_c, 'coef_launches': 2,
                         'coef_gb_per_s': round(moved_c / us_c * 1e-3, 1),
                         'apply_us_per_call': round(us_a, 2), 'apply_us_min_max': mm_a, 'apply_launches': 1,
                         'apply_gb_per_s': round(moved_a / us_a * 1e-3, 1), 'calls_per_batch': reps})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'apg.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_apg.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    runs = []
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    for name, apg in SETTINGS:                               # (one diffusion object per setting: each keeps its capture)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.hip_graph = name, True
        if APG[apg] is not None:
            d.apg_eta, d.apg_norm_threshold, d.apg_momentum = APG[apg]
        d.rng.key_by_sample(99, range(a.bs), dev)
        runs.append((name, apg, d, []))

    def call(d):
        t0 = time.perf_counter()
        img, _, _ = d.sample(classes, rgb_flow, flow, mask)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(img).all())
        return time.perf_counter() - t0
    for _, _, d, _ in runs:                                  # warm-up: capture + one replayed call
        call(d), call(d)
    for _ in range(a.rounds):
        for _, _, d, times in runs:
            times.append(call(d))
    res = {'tool': 'bench_apg', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True,
           'clip_mode': 'static', 'generator': 'keyed', 'rounds': a.rounds, 'order': 'interleaved round-robin in one process',
           'device': torch.cuda.get_device_name(0), 'settings': []}
    for name, apg, d, times in runs:
        med = statistics.median(times)
        res['settings'].append({'sampler': name, 'apg': apg, 'eta_rho_beta': APG[apg], 'images_per_s': round(a.bs / med, 3),
                                'ms_per_call': round(med * 1e3, 3), 'ms_per_step': round(med * 1e3 / a.s_step, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'graph_captures': d.graph_captures})
    by = {(r['sampler'], r['apg']): r for r in res['settings']}
    for name in ('ddim', 'dpmpp_2m'):
        for apg in ('eta0', 'eta0+rho+momentum'):
            off, on = by[(name, 'off')], by[(name, apg)]
            on['ms_per_step_over_off'] = round(on['ms_per_step'] - off['ms_per_step'], 4)
            on['step_time_over_off'] = round(on['ms_per_step'] / off['ms_per_step'], 4)
    res['launches_alone'] = launches_alone(dev, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
