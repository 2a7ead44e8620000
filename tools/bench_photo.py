"""Conditional sampler: the sampler as it is against photometric-consistency guidance (``photo_guidance``), in ms per denoise
step, and the launches of the feature (dmh_photo_guide's two, dmh_photo_weights' two, dmh_photo_energy's two) alone.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, cond_scale 3, cfg_mode 'streams', the captured step, noise
keyed by sample id, random weights, the static clamp — for four settings: {ddim, dpmpp_2m} x {off, w = 0.5}.  The four run
interleaved in one process (round-robin, --rounds times, after a warm-up call each that also captures), each call timed with a
host clock around work that ends in a device synchronise; the median per setting is reported with the spread.  Then the launches
alone, by HIP events around --reps back-to-back calls after a warm-up, at 25 samples of 128^2 and of 256^2 on N(0, 1.5) logits
with the synthetic conditions' flow and mask, and with a flow that clamps every pixel of a sample onto one corner pixel (the
most contended target the 64-bit integer atomics can meet).  Writes profiles/photo_guidance.json and prints the same JSON line.
A measurement tool: nothing gates on it, and it says nothing about sample quality.  Not bench.py: that is the project's
yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

W = 0.5
SETTINGS = tuple((name, w) for name in ('ddim', 'dpmpp_2m') for w in (None, W))
SIZES = (128, 256)


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


def launches_alone(dev, reps, bs):
    from dmhomo_amd import _lib, ddpm, ops
    rows = []
    step = _lib.DmhStep(objective=1, clip=1, mode=ops.MODE_LAST, cond_scale=3., sqrt_recip_ac=1., sqrt_recipm1_ac=1., sqrt_ac=0.8,
                        sqrt_1m_ac=0.6, c0=0., c1=0., c2=0.)
    for size in SIZES:
        gen = torch.Generator(device=dev).manual_seed(1)
        cond = torch.randn((bs, 6, size, size), device=dev, generator=gen) * 1.5
        null = torch.randn((bs, 6, size, size), device=dev, generator=gen) * 1.5
        data, _ = next(ddpm.SyntheticConditions(size, bs, seed=1000, device=dev))
        flows = {'synthetic': data[:, -2:].contiguous().float(), 'far': torch.full((bs, 2, size, size), 1000., device=dev)}
        mask = data[:, -6:-5].contiguous().float()
        acc, guided = ops.photo_acc(bs, size, size, dev), torch.empty_like(cond)
        for kind, flow in flows.items():
            s = ops.photo_weights(flow, mask, acc)
            us_w, mm_w = _timed(lambda: ops.photo_weights(flow, mask, acc, out=s), reps)
            us_g, mm_g = _timed(lambda: ops.photo_guide(step, cond, null, None, flow, mask, s, W, acc, out=guided), reps)
            us_c, mm_c = _timed(lambda: ops.photo_guide(step, cond, None, None, flow, mask, s, W, acc, out=guided), reps)
            ws, E = ops.photo_energy_workspace(cond), torch.empty((bs,), device=dev, dtype=torch.float64)
            us_e, mm_e = _timed(lambda: ops.photo_energy(cond, flow, mask, ws=ws, out=E), reps)
            assert not bool(acc.any()) and bool(torch.isfinite(guided).all())
            before = ops.photo_energy(cond, flow, mask)
            ops.photo_guide(step, cond, None, None, flow, mask, s, W, acc, out=guided)
            after = ops.photo_energy(guided, flow, mask)
            assert bool((after < before).all())              # the step is a descent
            taps = int((mask != 0).sum()) * 3 * 4
            rows.append({'B': bs, 'H': size, 'W': size, 'flow': kind, 'mask_mean': round(float(mask.mean()), 4),
                         's_max': round(float(s.max()), 2), 'atomic_adds_at_most': taps, 'atomic_mbytes_at_most': round(taps * 8e-6, 1),
                         'guide_us_per_call': round(us_g, 2), 'guide_us_min_max': mm_g, 'guide_launches': 2,
                         'guide_cond_only_us_per_call': round(us_c, 2), 'guide_cond_only_us_min_max': mm_c,
                         'weights_us_per_call': round(us_w, 2), 'weights_us_min_max': mm_w, 'weights_launches': 2,
                         'energy_us_per_call': round(us_e, 2), 'energy_us_min_max': mm_e, 'energy_launches': 2,
                         'energy_ratio_after_one_step': round(float((after / before).mean()), 4), 'calls_per_batch': reps})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'photo_guidance.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_photo.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    runs = []
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    for name, w in SETTINGS:                                 # (one diffusion object per setting: each keeps its capture)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.hip_graph, d.photo_guidance = name, True, w
        d.rng.key_by_sample(99, range(a.bs), dev)
        runs.append((name, w, d, [], []))

    def call(d):
        t0 = time.perf_counter()
        img, _, _ = d.sample(classes, rgb_flow, flow, mask)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(img).all())
        return dt, float(ddpm.photometric_error(img, flow, mask).mean())
    for _, _, d, _, _ in runs:                               # warm-up: capture + one replayed call
        call(d), call(d)
    for _ in range(a.rounds):
        for _, _, d, times, errs in runs:
            dt, e = call(d)
            times.append(dt), errs.append(e)
    res = {'tool': 'bench_photo', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True,
           'clip_mode': 'static', 'generator': 'keyed', 'weights': 'random (no checkpoint): the errors say nothing about quality',
           'rounds': a.rounds, 'order': 'interleaved round-robin in one process', 'device': torch.cuda.get_device_name(0),
           'settings': []}
    for name, w, d, times, errs in runs:
        med = statistics.median(times)
        res['settings'].append({'sampler': name, 'photo_guidance': w, 'images_per_s': round(a.bs / med, 3),
                                'ms_per_call': round(med * 1e3, 3), 'ms_per_step': round(med * 1e3 / a.s_step, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'mean_photometric_error': errs[-1], 'graph_captures': d.graph_captures})
    by = {(r['sampler'], r['photo_guidance']): r for r in res['settings']}
    for name in ('ddim', 'dpmpp_2m'):
        off, on = by[(name, None)], by[(name, W)]
        on['ms_per_step_over_off'] = round(on['ms_per_step'] - off['ms_per_step'], 4)
        on['step_time_over_off'] = round(on['ms_per_step'] / off['ms_per_step'], 4)
    res['launches_alone'] = launches_alone(dev, a.reps, a.bs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
