"""Conditional sampler: sample() against sample_known() (the source image kept), in ms per denoise entry, and the launches of
the feature (dmh_known_blend's one, dmh_known_error's two) alone, beside dmh_pag_shift in the same run.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, cond_scale 3, cfg_mode 'streams', the captured step, noise
keyed by sample id, random weights, the static clamp — for five settings: {ddim, dpmpp_2m} x {off, 'source' kept at
known_resample 1}, and ddim with 'source' kept at known_resample 2 (twice the entries: the per-entry time is the figure).  They
run interleaved in one process (round-robin, --rounds times, after a warm-up call each that also captures), each call timed with
a host clock around work that ends in a device synchronise; the median per setting is reported with the spread.  Then the
launches alone, by HIP events around --reps back-to-back calls after a warm-up, at 25 rows of 98304 (6 x 128^2) and of 393216
(6 x 256^2) values on N(0, 1.5) logits with the source half kept: bytes moved per element are 17 with a null pass (cond, null,
known, out: 4 each, the mask 1) and 13 without, dmh_pag_shift's 20 resp. 12.  Writes profiles/known_pixels.json and prints the
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

# (sampler, keep, known_resample)
SETTINGS = (('ddim', None, 1), ('ddim', 'source', 1), ('ddim', 'source', 2), ('dpmpp_2m', None, 1), ('dpmpp_2m', 'source', 1))
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
    for n in ROWS:
        gen = torch.Generator(device=dev).manual_seed(1)
        cond, null, pert = (torch.randn((bs, n), device=dev, generator=gen) * 1.5 for _ in range(3))
        K = torch.rand((bs, n), device=dev, generator=gen) * 2. - 1.
        kmask = torch.zeros((bs, n), device=dev, dtype=torch.uint8)
        kmask[:, :n // 2] = 1
        out = torch.empty_like(cond)
        elems = bs * n
        us_b, mm_b = _timed(lambda: ops.known_blend(cond, null, None, 3., K, kmask, out=out), reps)
        us_c, mm_c = _timed(lambda: ops.known_blend(cond, None, None, 1., K, kmask, out=out), reps)
        us_i, mm_i = _timed(lambda: ops.known_blend(out, None, None, 1., K, kmask), reps)       # in place: the write-back form
        ws, err = ops.known_error_workspace(cond), torch.empty((bs,), device=dev, dtype=torch.float64)
        us_e, mm_e = _timed(lambda: ops.known_error(cond, null, None, 3., K, kmask, ws=ws, out=err), reps)
        c2, n2 = cond.clone(), null.clone()
        us_p, mm_p = _timed(lambda: ops.pag_shift(c2, n2, pert, 0.001), reps)                   # (a small scale: 60 in-place shifts stay finite)
        us_q, mm_q = _timed(lambda: ops.pag_shift(c2, None, pert, 0.001), reps)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(err).all()) and bool(torch.isfinite(c2).all())
        rows.append({'B': bs, 'per_row': n, 'kept_fraction': 0.5, 'calls_per_batch': reps,
                     'blend_us_per_call': round(us_b, 2), 'blend_us_min_max': mm_b, 'blend_bytes_per_element': 17,
                     'blend_tbytes_per_s': _rate(17, elems, us_b),
                     'blend_cond_only_us_per_call': round(us_c, 2), 'blend_cond_only_us_min_max': mm_c,
                     'blend_cond_only_bytes_per_element': 13, 'blend_cond_only_tbytes_per_s': _rate(13, elems, us_c),
                     'blend_in_place_us_per_call': round(us_i, 2), 'blend_in_place_us_min_max': mm_i,
                     'blend_in_place_tbytes_per_s': _rate(13, elems, us_i),
                     'error_us_per_call': round(us_e, 2), 'error_us_min_max': mm_e, 'error_launches': 2,
                     'pag_shift_us_per_call': round(us_p, 2), 'pag_shift_us_min_max': mm_p, 'pag_shift_bytes_per_element': 20,
                     'pag_shift_tbytes_per_s': _rate(20, elems, us_p),
                     'pag_shift_cond_only_us_per_call': round(us_q, 2), 'pag_shift_cond_only_us_min_max': mm_q,
                     'pag_shift_cond_only_bytes_per_element': 12, 'pag_shift_cond_only_tbytes_per_s': _rate(12, elems, us_q)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'known_pixels.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_known.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'streams'
    runs = []
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    known = torch.rand((a.bs, 6, a.image_size, a.image_size), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    for name, keep, r in SETTINGS:                           # (one diffusion object per setting: each keeps its capture)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.hip_graph, d.known_resample = name, True, r
        d.rng.key_by_sample(99, range(a.bs), dev)
        runs.append((name, keep, r, d, []))

    def call(d, keep):
        t0 = time.perf_counter()
        if keep is None:
            img, _, _ = d.sample(classes, rgb_flow, flow, mask)
        else:
            img, _, _ = d.sample_known(known, keep, classes, rgb_flow, flow, mask)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(img).all())
        if keep == 'source':
            assert torch.equal(img[:, :3], known[:, :3])
        return dt
    for _, keep, _, d, _ in runs:                            # warm-up: capture + one replayed call
        call(d, keep), call(d, keep)
    for _ in range(a.rounds):
        for _, keep, _, d, times in runs:
            times.append(call(d, keep))
    res = {'tool': 'bench_known', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cond_scale': 3.0, 'cfg_mode': 'streams', 'hip_graph': True,
           'clip_mode': 'static', 'generator': 'keyed', 'weights': 'random (no checkpoint): nothing here is about quality',
           'rounds': a.rounds, 'order': 'interleaved round-robin in one process', 'device': torch.cuda.get_device_name(0),
           'settings': []}
    for name, keep, r, d, times in runs:
        med = statistics.median(times)
        entries = a.s_step * r
        res['settings'].append({'sampler': name, 'keep': keep, 'known_resample': r, 'entries': entries,
                                'images_per_s': round(a.bs / med, 3), 'ms_per_call': round(med * 1e3, 3),
                                'ms_per_entry': round(med * 1e3 / entries, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'graph_captures': d.graph_captures})
    by = {(r['sampler'], r['keep'], r['known_resample']): r for r in res['settings']}
    for name, keep, r in SETTINGS:
        if keep is not None:
            off, on = by[(name, None, 1)], by[(name, keep, r)]
            on['ms_per_entry_over_off'] = round(on['ms_per_entry'] - off['ms_per_entry'], 4)
            on['entry_time_over_off'] = round(on['ms_per_entry'] / off['ms_per_entry'], 4)
    res['launches_alone'] = launches_alone(dev, a.reps, a.bs)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
