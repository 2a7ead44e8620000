#!/usr/bin/env python3
"""Time dmh_hem_batch (csrc/hem_data.hip) at the shapes HEM trains on: B = 32 sampled 128 x 128 pairs -> ori_size 360 x 640,
crop 320 x 576.  Pre-allocated outputs, warm-up, then --runs runs of --per-run back-to-back launches, one HIP event pair around
each run (so the host's enqueue latency is not inside every sample); the median over the runs of the time per launch (500
launches by default) is reported with the spread, as microseconds and as the fraction of the 8 TB/s HBM peak that the bytes the launch has
to write (48 B per output pixel + 24 B per patch pixel; the 6 B per source pixel it reads are listed beside them) amount to.
A record, not a gate.

    python tools/bench_hem_batch.py [--out profiles/hem_batch.json] [--runs 25] [--per-run 20] [--bs 32]

The figure is copied into docs/EXPERIMENTS.md by hand.
"""
import argparse
import json
import os
import random
import statistics
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hem_batch.json'))
    ap.add_argument('--runs', type=int, default=25, help='timed runs (the median is over these)')
    ap.add_argument('--per-run', type=int, default=20, help='back-to-back launches inside one event pair')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--bs', type=int, default=32)
    a = ap.parse_args()
    assert a.runs * a.per_run >= 20
    from dmhomo_amd import ops
    from dmhomo_amd.hem_data import DGMTrainData, homo_scale
    assert torch.cuda.is_available(), 'the measurement needs the MI355X'
    dev = torch.device('cuda', 0)
    B, (h, w), (H, W), (ph, pw), rho = a.bs, (128, 128), (360, 640), (320, 576), 16
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, size=(B, 6, h, w), dtype=np.uint8)).to(dev)
    fwd = np.stack([homo_scale(h, w, np.eye(3) + np.array([[.03, -.02, 6.], [.02, .04, -5.], [2e-4, -1e-4, 0.]])
                               * rng.uniform(-1, 1, (3, 3)), H, W) for _ in range(B)])
    homo = torch.from_numpy(fwd).to(dev)
    homo_inv = torch.from_numpy(np.stack([np.linalg.inv(m) for m in fwd])).to(dev)
    r = random.Random(0)
    start = torch.tensor([[r.randint(rho, W - rho - pw), r.randint(rho, H - rho - ph)] for _ in range(B)],
                         dtype=torch.int32, device=dev)
    ds = DGMTrainData(types.SimpleNamespace(crop_size=(ph, pw), ori_size=(H, W), rho=rho), npy_path=())
    C = ops.C
    m3, s3 = (C.c_double * 3)(*ds.mean_I.ravel()), (C.c_double * 3)(*ds.std_I.ravel())
    outs = [torch.empty((B, c, hh, ww), device=dev, dtype=torch.float32)
            for c, hh, ww in ((2, H, W), (6, H, W), (4, H, W), (2, ph, pw), (4, ph, pw))]

    def launch():
        ops.call('dmh_hem_batch', ops.ptr(imgs, torch.uint8), ops.ptr(homo, torch.float64), ops.ptr(homo_inv, torch.float64),
                 ops.ptr(start, torch.int32), C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), B, h, w, H, W, ph, pw,
                 *[ops.ptr(t) for t in outs])

    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    # one event pair around a back-to-back run of launches: the queue is full after the first, so the host's enqueue latency
    # (Python + ctypes, several microseconds) is outside all but the first launch of a run
    times = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.per_run):
            launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / a.per_run)      # microseconds per launch
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    written = B * (48 * H * W + 24 * ph * pw)
    read = B * 6 * h * w
    med = statistics.median(times)
    res = {'kernel': 'dmh_hem_batch', 'B': B, 'source': [h, w], 'ori_size': [H, W], 'crop_size': [ph, pw],
           'runs': a.runs, 'launches_per_run': a.per_run, 'warmup': a.warmup,
           'timer': 'one HIP event pair around each run of back-to-back launches, divided by the launches of the run; '
                    'us_* are per launch, median / spread over the runs',
           'us_median': round(med, 2), 'us_min': round(min(times), 2), 'us_max': round(max(times), 2),
           'us_p10': round(sorted(times)[len(times) // 10], 2), 'us_p90': round(sorted(times)[(9 * len(times)) // 10], 2),
           'bytes_written': written, 'bytes_read_source': read,
           'written_TBps_at_median': round(written / (med * 1e-6) / 1e12, 3),
           'fraction_of_8TBps_hbm_peak': round(written / (med * 1e-6) / HBM_PEAK, 4),
           'bound': 'HBM writes (48 B per output pixel + 24 B per patch pixel); the uint8 source stays in cache',
           'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
