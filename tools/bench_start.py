"""Conditional sampler: sample() against sample_from() at four strengths, in ms per call and per denoise entry, and the launch of
the feature (dmh_start_mix, keyed arm) alone beside the three launches it stands for (dmh_rng_indexed, dmh_affine,
dmh_q_sample).

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, cond_scale 3, cfg_mode 'streams', the captured step, noise
keyed by sample id, random weights, the static clamp — for {ddim, dpmpp_2m} x {sample(), sample_from at strength 0.25, 0.5, 0.75,
1.0}.  The settings run interleaved in one process (round-robin, --rounds times, after a warm-up call each that also captures),
each call timed with a host clock around work that ends in a device synchronise; the median per setting is reported with the
spread of its calls.  The expectation is n / S of a call with the per-entry time of an ordinary entry; nothing is fixed: what
comes out is recorded.  Then the launches alone, by HIP events around --reps back-to-back calls after a warm-up, at 25 rows of
98304 (6 x 128^2) and of 393216 (6 x 256^2) values: dmh_start_mix reads init and writes out (8 bytes per element), the three
launches write eps, read init and write K, read K and eps and write out (24 bytes per element).  Writes profiles/start_from.json
and prints the same JSON line.  A measurement tool: nothing gates on it, and it says nothing about sample quality.  Not bench.py:
that is the project's yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

STRENGTHS = (None, 0.25, 0.5, 0.75, 1.0)                     # None: sample()
SAMPLERS = ('ddim', 'dpmpp_2m')
ROWS = (98304, 393216)


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


def _rate(bytes_per_elem, elems, us):
    return round(bytes_per_elem * elems / (us * 1e-6) / 1e12, 3)


def launches_alone(dev, reps, bs):
    from dmhomo_amd import ops
    rows = []
    ca, cb = 0.6, 0.8
    for n in ROWS:
        init = torch.rand((bs, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        ids = torch.arange(bs, dtype=torch.int64, device=dev)
        state = torch.tensor([99, 0, 0, 0], dtype=torch.int64, device=dev)
        out = torch.empty_like(init)
        ca_t, cb_t = torch.full((bs,), ca, device=dev), torch.full((bs,), cb, device=dev)
        elems = bs * n

        def three():                                         # what a caller without the entry launches (allocations included)
            eps = ops.rng_indexed((bs, n), ids, state, 0)
            return ops.q_sample(ops.affine(init, 2., -1.), eps, ca_t, cb_t)
        state[1] = 0
        want = three()
        state[1] = 0
        assert torch.equal(ops.start_mix(init, ca, cb, sample_ids=ids, state=state, out=out), want)      # the same bits
        us_m, mm_m = _timed(lambda: ops.start_mix(init, ca, cb, sample_ids=ids, state=state, out=out), reps)
        us_3, mm_3 = _timed(three, reps)
        us_r, mm_r = _timed(lambda: ops.rng_indexed((bs, n), ids, state, 0), reps)
        noise = torch.randn_like(init)
        us_g, mm_g = _timed(lambda: ops.start_mix(init, ca, cb, noise=noise, out=out), reps)
        rows.append({'B': bs, 'per_sample': n, 'calls_per_batch': reps,
                     'start_mix_keyed_us_per_call': round(us_m, 2), 'start_mix_keyed_us_min_max': mm_m,
                     'start_mix_keyed_bytes_per_element': 8, 'start_mix_keyed_tbytes_per_s': _rate(8, elems, us_m),
                     'three_launches_us_per_call': round(us_3, 2), 'three_launches_us_min_max': mm_3,
                     'three_launches_bytes_per_element': 24, 'three_launches_tbytes_per_s': _rate(24, elems, us_3),
                     'rng_indexed_alone_us_per_call': round(us_r, 2), 'rng_indexed_alone_us_min_max': mm_r,
                     'start_mix_given_noise_us_per_call': round(us_g, 2), 'start_mix_given_noise_us_min_max': mm_g,
                     'start_mix_given_noise_bytes_per_element': 12, 'start_mix_given_noise_tbytes_per_s': _rate(12, elems, us_g),
                     'saved_us_per_call': round(us_3 - us_m, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'start_from.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_start.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    from dmhomo_amd.schedule import start_entry
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    init = torch.rand((a.bs, 6, a.image_size, a.image_size), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    runs = []
    for name in SAMPLERS:                                    # (one diffusion object per sampler: the strengths share its captures)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.hip_graph, d.graph_cache_size = name, True, len(STRENGTHS)
        d.rng.key_by_sample(99, range(a.bs), dev)
        for s in STRENGTHS:
            runs.append((name, s, d, []))

    def call(d, s):
        t0 = time.perf_counter()
        if s is None:
            img, _, _ = d.sample(classes, rgb_flow, flow, mask)
        else:
            img, _, _ = d.sample_from(init, s, classes, rgb_flow, flow, mask)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(img).all())
        return dt
    for _, s, d, _ in runs:                                  # warm-up: capture (where the setting has one of its own) + a replayed call
        call(d, s), call(d, s)
    for _ in range(a.rounds):
        for _, s, d, times in runs:
            times.append(call(d, s))
    res = {'tool': 'bench_start', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True,
           'clip_mode': 'static', 'generator': 'keyed', 'weights': 'random (no checkpoint): nothing here is about quality',
           'rounds': a.rounds, 'order': 'interleaved round-robin in one process', 'device': torch.cuda.get_device_name(0),
           'settings': []}
    for name, s, d, times in runs:
        med = statistics.median(times)
        entries = a.s_step if s is None else a.s_step - start_entry(a.s_step, s)
        res['settings'].append({'sampler': name, 'call': 'sample' if s is None else 'sample_from', 'strength': s, 'entries': entries,
                                'images_per_s': round(a.bs / med, 3), 'ms_per_call': round(med * 1e3, 3),
                                'ms_per_entry': round(med * 1e3 / entries, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'ms_per_call_spread_percent': round((max(times) - min(times)) / med * 100., 2),
                                'graph_captures_of_the_sampler': d.graph_captures})
    by = {(r['sampler'], r['strength']): r for r in res['settings']}
    for r in res['settings']:
        off = by[(r['sampler'], None)]
        r['call_time_over_sample'] = round(r['ms_per_call'] / off['ms_per_call'], 4)
        r['entries_over_S'] = round(r['entries'] / a.s_step, 4)
        r['entry_time_over_sample'] = round(r['ms_per_entry'] / off['ms_per_entry'], 4)
    res['launches_alone'] = launches_alone(dev, a.reps, a.bs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
