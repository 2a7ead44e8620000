"""Conditional sampler: DDIM against the second-order multistep solver (``sampler = 'dpmpp_2m'``), in images/s.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, cond_scale 3, cfg_mode 'streams', the captured step, noise keyed
by sample id, random weights — for three settings: ddim at S = 32, dpmpp_2m at S = 32, dpmpp_2m at S = 16.  The three run
interleaved in one process (round-robin, --rounds times, after a warm-up call each that also captures), each call timed with
a host clock around work that ends in a device synchronise; the median per setting is reported with the spread.  Writes
profiles/solver_dpmpp.json and prints the same JSON line.  A measurement tool: nothing gates on it, and it says nothing
about sample quality.  Not bench.py: that is the project's yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SETTINGS = (('ddim', 32), ('dpmpp_2m', 32), ('dpmpp_2m', 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'solver_dpmpp.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_solver.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    runs = []
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    for name, S in SETTINGS:                                 # (one diffusion object per setting: each keeps its capture)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=S, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.hip_graph = name, True
        d.rng.key_by_sample(99, range(a.bs), dev)
        runs.append((name, S, d, []))

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
    res = {'tool': 'bench_solver', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True, 'generator': 'keyed',
           'rounds': a.rounds, 'order': 'interleaved round-robin in one process', 'device': torch.cuda.get_device_name(0),
           'settings': []}
    for name, S, d, times in runs:
        med = statistics.median(times)
        res['settings'].append({'sampler': name, 'sampling_timesteps': S, 'images_per_s': round(a.bs / med, 3),
                                'ms_per_call': round(med * 1e3, 3), 'ms_per_step': round(med * 1e3 / S, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'graph_captures': d.graph_captures})
    base = res['settings'][0]['images_per_s']
    for row in res['settings']:
        row['images_per_s_over_ddim_s32'] = round(row['images_per_s'] / base, 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
