"""Conditional sampler: what a guidance interval (``guidance_interval``) costs and saves per denoise step, and the two launches
it adds to the captured step (dmh_rows_gated, dmh_guidance_gate) alone.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, cond_scale 3, cfg_mode 'streams', the captured step, noise
keyed by sample id, random weights, the static clamp — for {ddim, dpmpp_2m} x dedup_dropped_rows {off, on} x four intervals:
None (today's step), (0, 1) (every entry guided, through the gated step), (0.25, 0.75) and one that guides nothing.  The sixteen
settings run interleaved in one process (round-robin, --rounds times, after two warm-up calls each, the first of which captures),
each call timed with a host clock around work that ends in a device synchronise; the median per setting is reported with the
spread.  The three intervals of a (sampler, dedup) pair replay ONE capture (graph_captures says so).  From the all-guided and
the nothing-guided setting: ms per guided and per unguided entry and their ratio.  Then the two new launches alone, by HIP
events around --reps back-to-back calls after a warm-up (eager launches: what they show is the launch rate unless the kernel is
longer than a launch).  Writes profiles/guidance_interval.json and prints the same JSON line; a 'bench_py_default_path' record
already in that file (bench.py on the parent commit against this tree, written by hand) is carried over.
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

INTERVALS = (('none', None), ('all', (0., 1.)), ('middle', (0.25, 0.75)), ('nothing', (0.99, 0.995)))
GATE_SHAPE = (25, 98304)


def _events(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(5):                                       # five batches of back-to-back calls: the median batch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / reps)
    return {'us_per_call': round(statistics.median(per), 2), 'us_per_call_min_max': [round(min(per), 2), round(max(per), 2)],
            'calls_per_batch': reps}


def launches_alone(dev, reps):
    from dmhomo_amd import ops
    B, n = GATE_SHAPE
    gen = torch.Generator(device=dev).manual_seed(1)
    cond = torch.randn((B, n), device=dev, generator=gen) * 1.5
    null = torch.randn((B, n), device=dev, generator=gen) * 1.5
    keep = (torch.arange(B, device=dev) % 2).to(torch.uint8)
    cursor = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = []
    for name, flag in (('guided', 1), ('unguided', 0)):
        guided = torch.full((32,), flag, dtype=torch.uint8, device=dev)
        rows = torch.empty((1 + 2 * B,), dtype=torch.int32, device=dev)
        r = _events(lambda: ops.rows_gated(keep, B, B, cursor, guided, rows=rows), reps)
        out.append({'launch': 'dmh_rows_gated', 'entry': name, 'B': B, 'extra': B, **r})
        r = _events(lambda: ops.guidance_gate(cursor, guided, cond, null), reps)
        moved = 0 if flag else 2 * B * n * 4
        out.append({'launch': 'dmh_guidance_gate', 'entry': name, 'B': B, 'n': n, 'bytes_moved_per_call': moved,
                    'gb_per_s': round(moved / r['us_per_call'] * 1e-3, 1), **r})
        assert torch.equal(null, cond) == (flag == 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guidance_interval.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_interval.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    runs = []
    for name in ('ddim', 'dpmpp_2m'):                        # (one diffusion object per sampler: it keeps its four captures)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.hip_graph, d.graph_cache_size = name, True, 8
        d.rng.key_by_sample(99, range(a.bs), dev)
        times = [t for t, _, _ in d._sampler_steps(True, 3.)]
        for dedup in (False, True):
            for iname, gi in INTERVALS:
                d.guidance_interval = gi
                flags = d._guided_entries(times, 3.)
                runs.append({'sampler': name, 'dedup': dedup, 'iname': iname, 'interval': gi, 'd': d, 'times': [],
                             'guided': a.s_step if flags is None else sum(flags)})
    by = {(r['sampler'], r['dedup'], r['iname']): r for r in runs}
    assert all(by[(s, dd, 'nothing')]['guided'] == 0 and by[(s, dd, 'all')]['guided'] == a.s_step
               for s in ('ddim', 'dpmpp_2m') for dd in (False, True))

    def call(r):
        d = r['d']
        model.dedup_dropped_rows, d.guidance_interval = r['dedup'], r['interval']
        t0 = time.perf_counter()
        img, _, _ = d.sample(classes, rgb_flow, flow, mask)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(img).all())
        return time.perf_counter() - t0
    for r in runs:                                           # warm-up: capture (where the pair has none yet) + a replayed call
        call(r), call(r)
    for _ in range(a.rounds):
        for r in runs:
            r['times'].append(call(r))
    res = {'tool': 'bench_interval', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True,
           'clip_mode': 'static', 'generator': 'keyed', 'rounds': a.rounds, 'order': 'interleaved round-robin in one process',
           'device': torch.cuda.get_device_name(0), 'settings': [], 'per_entry': []}
    for r in runs:
        med, none_med = statistics.median(r['times']), statistics.median(by[(r['sampler'], r['dedup'], 'none')]['times'])
        r['ms_per_call'] = med * 1e3
        res['settings'].append({'sampler': r['sampler'], 'dedup_dropped_rows': r['dedup'], 'guidance_interval': r['interval'],
                                'guided_entries': r['guided'], 'unguided_entries': a.s_step - r['guided'],
                                'images_per_s': round(a.bs / med, 3), 'ms_per_call': round(med * 1e3, 3),
                                'ms_per_step': round(med * 1e3 / a.s_step, 4),
                                'ms_per_call_min_max': [round(min(r['times']) * 1e3, 3), round(max(r['times']) * 1e3, 3)],
                                'images_per_s_over_none': round(none_med / med, 4)})
    for name in ('ddim', 'dpmpp_2m'):
        d = by[(name, False, 'none')]['d']
        for dedup in (False, True):
            none, full, nothing = (by[(name, dedup, k)]['ms_per_call'] / a.s_step for k in ('none', 'all', 'nothing'))
            res['per_entry'].append({'sampler': name, 'dedup_dropped_rows': dedup, 'ms_per_step_no_interval': round(none, 4),
                                     'ms_per_guided_entry': round(full, 4), 'ms_per_unguided_entry': round(nothing, 4),
                                     'guided_over_unguided': round(full / nothing, 4),
                                     'gated_step_over_todays_step': round(full / none, 4)})
        res.setdefault('graph_captures', {})[name] = d.graph_captures      # 4: {dedup off, on} x {no interval, an interval}
    res['launches_alone'] = launches_alone(dev, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if os.path.exists(a.out):                                # (the bench.py A/B of the default path is recorded by hand: keep it)
        with open(a.out) as f:
            old = json.load(f)
        if 'bench_py_default_path' in old:
            res['bench_py_default_path'] = old['bench_py_default_path']
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
