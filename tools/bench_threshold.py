"""Conditional sampler: the static clamp against dynamic thresholding (``clip_mode = 'dynamic'``), in ms per denoise step, and
the row-quantile selector (dmh_row_quantile_abs) alone.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, cond_scale 3, cfg_mode 'streams', the captured step, noise
keyed by sample id, random weights — for four settings: {ddim, dpmpp_2m} x {static, dynamic}.  The four run interleaved in one
process (round-robin, --rounds times, after a warm-up call each that also captures), each call timed with a host clock around
work that ends in a device synchronise; the median per setting is reported with the spread.  Then the selector launch alone,
by HIP events around --reps back-to-back launches after a warm-up, at (25, 98304) and (25, 393216) on N(0, 1.5) rows at the
0.995 quantile.  Writes profiles/dynamic_threshold.json and prints the same JSON line.  A measurement tool: nothing gates on
it, and it says nothing about sample quality.  Not bench.py: that is the project's yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SETTINGS = (('ddim', 'static'), ('ddim', 'dynamic'), ('dpmpp_2m', 'static'), ('dpmpp_2m', 'dynamic'))
SELECTOR_SHAPES = ((25, 98304), (25, 393216))


def selector_alone(dev, p, reps):
    from dmhomo_amd import ops
    from dmhomo_amd.sampling import ScheduleHost
    rows = []
    for B, n in SELECTOR_SHAPES:
        x = torch.randn((B, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 1.5
        k, frac = ScheduleHost._quantile_rank(p, n)
        out = torch.empty((B,), device=dev)
        for _ in range(10):
            ops.row_quantile_abs(x, k, frac, 1., out=out)
        torch.cuda.synchronize()
        per = []
        for _ in range(5):                                   # five batches of back-to-back launches: the median batch
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                ops.row_quantile_abs(x, k, frac, 1., out=out)
            b.record()
            b.synchronize()
            per.append(a.elapsed_time(b) * 1e3 / reps)
        want = torch.quantile(x.abs().double(), torch.tensor(p, dtype=torch.float64, device=dev), dim=1).clamp(min=1.)
        assert float((out.double() - want).abs().max()) <= 1e-6 * float(want.max())
        rows.append({'B': B, 'n': n, 'percentile': p, 'us_per_launch': round(statistics.median(per), 2),
                     'us_per_launch_min_max': [round(min(per), 2), round(max(per), 2)], 'launches_per_batch': reps,
                     'bytes_read_per_launch': 4 * B * n * 4, 'note': 'four passes over the rows, L2-resident after the first'})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--percentile', type=float, default=0.995)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dynamic_threshold.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_threshold.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    runs = []
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    for name, mode in SETTINGS:                              # (one diffusion object per setting: each keeps its capture)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.clip_mode, d.dynamic_threshold_percentile, d.hip_graph = name, mode, a.percentile, True
        d.rng.key_by_sample(99, range(a.bs), dev)
        runs.append((name, mode, d, []))

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
    res = {'tool': 'bench_threshold', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True,
           'generator': 'keyed', 'rounds': a.rounds, 'order': 'interleaved round-robin in one process',
           'device': torch.cuda.get_device_name(0), 'percentile': a.percentile, 'settings': []}
    for name, mode, d, times in runs:
        med = statistics.median(times)
        res['settings'].append({'sampler': name, 'clip_mode': mode, 'images_per_s': round(a.bs / med, 3),
                                'ms_per_call': round(med * 1e3, 3), 'ms_per_step': round(med * 1e3 / a.s_step, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'graph_captures': d.graph_captures})
    by = {(r['sampler'], r['clip_mode']): r for r in res['settings']}
    for name in ('ddim', 'dpmpp_2m'):
        s, dy = by[(name, 'static')], by[(name, 'dynamic')]
        dy['ms_per_step_over_static'] = round(dy['ms_per_step'] - s['ms_per_step'], 4)
        dy['step_time_over_static'] = round(dy['ms_per_step'] / s['ms_per_step'], 4)
    res['selector_alone'] = selector_alone(dev, a.percentile, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
