"""Conditional sampler: the guided blend as it is against rescaled guidance (``guidance_rescale = 0.7``), in ms per denoise
step, and the factor launch pair (dmh_guidance_factor) alone.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, cond_scale 3, cfg_mode 'streams', the captured step, noise
keyed by sample id, random weights, the static clamp — for four settings: {ddim, dpmpp_2m} x {phi = 0, phi = 0.7}.  The four
run interleaved in one process (round-robin, --rounds times, after a warm-up call each that also captures), each call timed
with a host clock around work that ends in a device synchronise; the median per setting is reported with the spread.  Then the
two launches of the factor alone, by HIP events around --reps back-to-back calls after a warm-up, at (25, 98304) and (25,
393216) on N(0, 1.5) logits.  Writes profiles/guidance_rescale.json and prints the same JSON line.  A measurement tool: nothing
gates on it, and it says nothing about sample quality.  Not bench.py: that is the project's yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PHI = 0.7
SETTINGS = (('ddim', 0.), ('ddim', PHI), ('dpmpp_2m', 0.), ('dpmpp_2m', PHI))
FACTOR_SHAPES = ((25, 98304), (25, 393216))


def factor_alone(dev, reps):
    from dmhomo_amd import _lib, ops
    rows = []
    step = _lib.DmhStep(objective=1, clip=1, mode=ops.MODE_LAST, cond_scale=3., sqrt_recip_ac=1., sqrt_recipm1_ac=1., sqrt_ac=1.,
                        sqrt_1m_ac=1., c0=0., c1=0., c2=0.)
    for B, n in FACTOR_SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        cond = torch.randn((B, n), device=dev, generator=gen) * 1.5
        null = torch.randn((B, n), device=dev, generator=gen) * 1.5
        ws, gfac = ops.guidance_workspace(cond), torch.empty((B,), device=dev)
        for _ in range(10):
            ops.guidance_factor(step, cond, null, PHI, ws=ws, gfac=gfac)
        torch.cuda.synchronize()
        per = []
        for _ in range(5):                                   # five batches of back-to-back calls: the median batch
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                ops.guidance_factor(step, cond, null, PHI, ws=ws, gfac=gfac)
            b.record()
            b.synchronize()
            per.append(a.elapsed_time(b) * 1e3 / reps)
        blend = null + (cond - null) * 3.
        want = 1. + PHI * (cond.double().std(dim=1, unbiased=False) / blend.double().std(dim=1, unbiased=False) - 1.)
        assert float((gfac.double() - want).abs().max()) <= 1e-6
        us = statistics.median(per)
        rows.append({'B': B, 'n': n, 'phi': PHI, 'splits': ops.guidance_splits(B, n), 'us_per_call': round(us, 2),
                     'us_per_call_min_max': [round(min(per), 2), round(max(per), 2)], 'calls_per_batch': reps,
                     'launches_per_call': 2, 'bytes_read_per_call': 2 * B * n * 4,
                     'read_gb_per_s': round(2 * B * n * 4 / us * 1e-3, 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guidance_rescale.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_guidance.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    runs = []
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    for name, phi in SETTINGS:                               # (one diffusion object per setting: each keeps its capture)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.guidance_rescale, d.hip_graph = name, phi, True
        d.rng.key_by_sample(99, range(a.bs), dev)
        runs.append((name, phi, d, []))

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
    res = {'tool': 'bench_guidance', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True,
           'clip_mode': 'static', 'generator': 'keyed', 'rounds': a.rounds, 'order': 'interleaved round-robin in one process',
           'device': torch.cuda.get_device_name(0), 'settings': []}
    for name, phi, d, times in runs:
        med = statistics.median(times)
        res['settings'].append({'sampler': name, 'guidance_rescale': phi, 'images_per_s': round(a.bs / med, 3),
                                'ms_per_call': round(med * 1e3, 3), 'ms_per_step': round(med * 1e3 / a.s_step, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'graph_captures': d.graph_captures})
    by = {(r['sampler'], r['guidance_rescale']): r for r in res['settings']}
    for name in ('ddim', 'dpmpp_2m'):
        off, on = by[(name, 0.)], by[(name, PHI)]
        on['ms_per_step_over_phi_0'] = round(on['ms_per_step'] - off['ms_per_step'], 4)
        on['step_time_over_phi_0'] = round(on['ms_per_step'] / off['ms_per_step'], 4)
    res['factor_alone'] = factor_alone(dev, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
