"""Re-labelling a batch: the one launch (dmh_relabel_batch, ops.relabel_batch) against what it stands for — ops.homography_flow +
ops.homography_warp + the where / cat that assemble the 12-channel batch — allocations included on both sides.

Batches of 25 at 128 x 128 and 256 x 256.  The stand-in is handed the labels and the validity mask the fused launch wrote, so
neither the host-side draw nor a validity pass the fused launch also replaces is charged to it: its five launches are the
flow, the copy of img1 the warp's layout asks for, the warp, the where and the cat.  The four settings
(two sizes x {fused, three launches}) run interleaved in one process: --rounds times round-robin, each turn --reps back-to-back
calls between HIP events after a warm-up; the median per setting is reported with the spread of its turns.  Both sides are checked
to give the same bits before anything is timed.  Bytes: the fused launch reads img1 (3 planes, plus the warp's taps, which hit
the same lines), img2 only where the warp has no source pixel (counted in full: an upper bound) and the mask, and writes 12
planes + 1 byte per pixel; counted as (3 + 3 + 1 + 12) * 4 + 1 = 77 bytes per pixel.  Writes profiles/relabel.json and prints the
same JSON line.  A measurement tool: nothing gates on it, and it says nothing about sample quality.  Not bench.py: that is the
project's yardstick."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SIZES = (128, 256)
SEED = 7


def _turn(fn, reps):
    """us per call of one turn: ``reps`` back-to-back calls between HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=25)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'relabel.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_relabel.py measures on the GPU: none found (no fallback)')
    from dmhomo_amd import ops
    dev = torch.device('cuda', 0)
    settings = []
    for S in SIZES:
        gen = torch.Generator(device=dev).manual_seed(S)
        data = torch.rand((a.bs, 12, S, S), device=dev, generator=gen)
        ids = torch.arange(a.bs, dtype=torch.int64, device=dev)
        _, homos, valid = ops.relabel_batch(data, ids, SEED)
        homos, ok = homos.clone(), valid.bool().unsqueeze(1).clone()

        def fused(data=data, ids=ids):
            return ops.relabel_batch(data, ids, SEED)

        def three(data=data, homos=homos, ok=ok, S=S):       # what a caller without the entry launches
            flow, rgb = ops.homography_flow(homos, S, S, 256.)
            warp = ops.homography_warp(data[:, :3].contiguous(), homos, (S, S))
            target = torch.where(ok, warp, data[:, 3:6])
            return torch.cat([data[:, :3], target, data[:, 6:7], rgb, flow], dim=1)
        assert torch.equal(three(), fused()[0])              # the same bits
        settings.append({'image_size': S, 'what': 'dmh_relabel_batch', 'launches': 1, 'fn': fused, 'turns': []})
        settings.append({'image_size': S, 'what': 'homography_flow + homography_warp + contiguous + where + cat', 'launches': 5,
                         'fn': three, 'turns': []})
    for s in settings:                                       # warm-up
        for _ in range(20):
            s['fn']()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for s in settings:
            s['turns'].append(_turn(s['fn'], a.reps))
    res = {'tool': 'bench_relabel', 'bs': a.bs, 'rounds': a.rounds, 'calls_per_turn': a.reps,
           'order': 'interleaved round-robin in one process', 'device': torch.cuda.get_device_name(0),
           'timing': 'HIP events around back-to-back calls, allocations included', 'settings': []}
    for s in settings:
        med = statistics.median(s['turns'])
        px = a.bs * s['image_size'] ** 2
        row = {'image_size': s['image_size'], 'what': s['what'], 'launches': s['launches'], 'us_per_call': round(med, 2),
               'us_min_max': [round(min(s['turns']), 2), round(max(s['turns']), 2)]}
        if s['launches'] == 1:
            row['bytes_per_pixel'] = 77
            row['tbytes_per_s'] = round(77 * px / (med * 1e-6) / 1e12, 3)
        res['settings'].append(row)
    for S in SIZES:
        f, t = (r for r in res['settings'] if r['image_size'] == S)
        f['time_over_the_launches_it_replaces'] = round(f['us_per_call'] / t['us_per_call'], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
