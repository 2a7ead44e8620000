"""Conditional sampler: the loop as it is against perturbed-attention guidance (``pag_scale``), in ms per denoise step, the shift
launch (dmh_pag_shift) alone next to dmh_flow_guidance_shift, and the attention core with perturbed rows (dmh_attention_pag) next
to dmh_attention.

bench.py's geometry — cfg.Unet(dim=64) at 128x128, batch 25, S = 32, the captured step, noise keyed by sample id, random weights,
the static clamp — with cfg_mode 'batched' (the mode the switch runs in; off is measured in the same mode) for sixteen settings:
{ddim, dpmpp_2m} x cond_scale {3, 1} x dedup_dropped_rows {off, on} x pag_scale {off, 2.5}.  At cond_scale 3 the switch makes 2B
UNet rows 3B, at cond_scale 1 B rows 2B.  The settings run interleaved in one process (round-robin, --rounds times, after a warm-up
call each that also captures), each call timed with a host clock around work that ends in a device synchronise; the median per
setting is reported with the spread between its calls.  Then the launches alone, by HIP events around --reps back-to-back calls
after a warm-up: the two shifts at (25, 98304) and (25, 393216) on N(0, 1.5) logits, with a null pass (5 x 4 bytes per element:
three reads, two writes) and without (3 x 4 bytes), against the 8 TB/s HBM peak; the attention cores at B = 75 (three passes of 25)
and n = 256 / 1024, with no row, the last third and every row perturbed.  Writes profiles/pag.json and prints the same JSON line.
A measurement tool: nothing gates on it, and it says nothing about sample quality.  Not bench.py: that is the project's
yardstick."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SCALE = 2.5
ATTN_B, ATTN_NS = 75, (256, 1024)
SETTINGS = tuple(itertools.product(('ddim', 'dpmpp_2m'), (3., 1.), (False, True), (None, SCALE)))
SHAPES = ((25, 98304), (25, 393216))
HBM_PEAK = 8e12                                              # bytes per second


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


def launch_alone(dev, reps):
    from dmhomo_amd import ops
    rows = []
    for B, n in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        cond, null, third = (torch.randn((B, n), device=dev, generator=gen) * 1.5 for _ in range(3))
        for entry, shift in (('dmh_pag_shift', ops.pag_shift), ('dmh_flow_guidance_shift', ops.flow_guidance_shift)):
            for with_null in (True, False):
                # a scale of 0 keeps the in-place values where they are over the repeated calls (e is a zero: the same loads
                # and stores)
                us, mm = _timed(lambda: shift(cond, null if with_null else None, third, 0.), reps)
                assert bool(torch.isfinite(cond).all())
                moved = (5 if with_null else 3) * B * n * 4
                rows.append({'entry': entry, 'B': B, 'n': n, 'null_pass': with_null, 'bytes_per_element': 20 if with_null else 12,
                             'us_per_call': round(us, 2), 'us_min_max': mm, 'launches': 1,
                             'gb_per_s': round(moved / us * 1e-3, 1), 'of_hbm_peak': round(moved / (us * 1e-6) / HBM_PEAK, 4),
                             'calls_per_batch': reps})
    return rows


def attention_alone(dev, reps):
    from dmhomo_amd import ops
    rows = []
    for n in ATTN_NS:
        gen = torch.Generator(device=dev).manual_seed(2)
        qkv = torch.randn((ATTN_B, n, 1, 384), device=dev, generator=gen)
        for entry, pert_lo in (('dmh_attention', None), ('dmh_attention_pag', ATTN_B), ('dmh_attention_pag', 2 * ATTN_B // 3),
                               ('dmh_attention_pag', 0)):
            us, mm = _timed(lambda: ops.attention_core(qkv, 32 ** -0.5, pert_lo=pert_lo), reps)
            rows.append({'entry': entry, 'B': ATTN_B, 'n': n, 'pert_lo': pert_lo,
                         'perturbed_rows': 0 if pert_lo is None else ATTN_B - pert_lo, 'us_per_call': round(us, 2),
                         'us_min_max': mm, 'calls_per_batch': reps, 'includes': 'the allocation of out by the wrapper'})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pag.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pag.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import cfg, ddpm
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = cfg.Unet(dim=a.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = 'batched'
    runs = []
    data, classes = next(ddpm.SyntheticConditions(a.image_size, a.bs, seed=1000, device=dev))
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()
    for sampler, cs, dedup, pg in SETTINGS:                  # (one diffusion object per setting: each keeps its capture)
        d = cfg.GaussianDiffusion(model, image_size=a.image_size, timesteps=1000, sampling_timesteps=a.s_step, loss_type='l1',
                                  objective='pred_x0').to(dev)
        d.sampler, d.hip_graph, d.pag_scale = sampler, True, pg
        d.rng.key_by_sample(99, range(a.bs), dev)
        runs.append((sampler, cs, dedup, pg, d, []))

    def call(d, cs, dedup):
        model.dedup_dropped_rows = dedup
        t0 = time.perf_counter()
        img, _, _ = d.sample(classes, rgb_flow, flow, mask, cond_scale=cs)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(img).all())
        return time.perf_counter() - t0
    for _, cs, dedup, _, d, _ in runs:                       # warm-up: capture + one replayed call
        call(d, cs, dedup), call(d, cs, dedup)
    for _ in range(a.rounds):
        for _, cs, dedup, _, d, times in runs:
            times.append(call(d, cs, dedup))
    res = {'tool': 'bench_pag', 'unet': {'dim': a.dim, 'dim_mults': [1, 2, 4, 8], 'channels': 6}, 'bs': a.bs,
           'image_size': a.image_size, 'sampling_timesteps': a.s_step, 'cfg_mode': 'batched', 'hip_graph': True,
           'clip_mode': 'static', 'generator': 'keyed', 'rounds': a.rounds, 'order': 'interleaved round-robin in one process',
           'device': torch.cuda.get_device_name(0), 'settings': []}
    for sampler, cs, dedup, pg, d, times in runs:
        med = statistics.median(times)
        res['settings'].append({'sampler': sampler, 'cond_scale': cs, 'dedup_dropped_rows': dedup, 'pag_scale': pg,
                                'images_per_s': round(a.bs / med, 3), 'ms_per_call': round(med * 1e3, 3),
                                'ms_per_step': round(med * 1e3 / a.s_step, 4),
                                'ms_per_call_min_max': [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
                                'spread_of_median': round((max(times) - min(times)) / med, 4),
                                'graph_captures': d.graph_captures})
    by = {(r['sampler'], r['cond_scale'], r['dedup_dropped_rows'], r['pag_scale']): r for r in res['settings']}
    for sampler, cs, dedup, pg in SETTINGS:
        if pg is not None:
            off, on = by[(sampler, cs, dedup, None)], by[(sampler, cs, dedup, pg)]
            on['ms_per_step_over_off'] = round(on['ms_per_step'] - off['ms_per_step'], 4)
            on['step_time_over_off'] = round(on['ms_per_step'] / off['ms_per_step'], 4)
    res['launch_alone'] = launch_alone(dev, a.reps)
    res['attention_alone'] = attention_alone(dev, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
