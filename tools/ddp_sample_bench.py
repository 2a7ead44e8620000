"""Unconditional sampler: eager loop vs the replayed captured step (ddpm.GaussianDiffusion.hip_graph).

A DDP Unet(dim=64, channels=6) with random weights at 128x128, batch 16: ddim_sample at S = 32 and p_sample_loop at T =
--timesteps (the reference's 1000 by default), eager and graphed, self-conditioning off and on, keyed device generator.
Timed with HIP events after warm-up.  Prints one JSON line: images/s and ms per denoise step of every run, the eager /
graph ratio, launches per replayed step (node count of the captured step), and the fused step kernel's time per launch
against its byte count (model output + img read, img written, padded next input written; 8 TB/s HBM).  Not bench.py:
that is the project's yardstick for the conditional sampler."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_BPS = 8e12


def graph_nodes(body):
    """node count of one capture of ``body`` (kept as a graph, not instantiated, never replayed)"""
    hip = ctypes.CDLL('libamdhip64.so')
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        body()
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n))
    del g
    return int(n.value) if rc == 0 else None


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--ddim-steps', type=int, default=32)
    ap.add_argument('--timesteps', type=int, default=1000, help='T of the ancestral p_sample_loop run')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--kernel-reps', type=int, default=200)
    a = ap.parse_args()
    from dmhomo_amd import cfg, ddpm, ops
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    mults, channels = (1, 2, 4, 8), 6
    B, S = a.batch, a.size
    res = {'tool': 'ddp_sample_bench', 'unet': {'dim': a.dim, 'dim_mults': list(mults), 'channels': channels},
           'batch': B, 'image_size': S, 'ddim_steps': a.ddim_steps, 'timesteps': a.timesteps, 'generator': 'keyed',
           'runs': {}}
    for sc in (False, True):
        model = ddpm.Unet(dim=a.dim, dim_mults=mults, channels=channels, self_condition=sc).to(dev)
        for kind in ('ddim', 'ddpm'):
            if kind == 'ddim':
                d = ddpm.GaussianDiffusion(model, image_size=S, timesteps=1000, sampling_timesteps=a.ddim_steps).to(dev)
                nsteps = a.ddim_steps
            else:
                d = ddpm.GaussianDiffusion(model, image_size=S, timesteps=a.timesteps).to(dev)
                nsteps = a.timesteps
            d.rng = cfg.DeviceRng().key_by_sample(1, range(B), dev)
            row = {'steps': nsteps}
            for graph in (False, True):
                d.hip_graph = graph
                for _ in range(a.warmup):
                    d.sample(batch_size=B)
                torch.cuda.synchronize()
                ms = timed(lambda: d.sample(batch_size=B), a.reps)
                tag = 'graph' if graph else 'eager'
                row[f'{tag}_images_per_s'] = round(B * 1e3 / ms, 3)
                row[f'{tag}_ms_per_step'] = round(ms / nsteps, 4)
            row['eager_ms_over_graph_ms'] = round(row['graph_images_per_s'] / row['eager_images_per_s'], 4)
            st = d.__dict__['_graph_state']
            row['launches_per_step'] = graph_nodes(st['mid'])
            key = f"{kind}_{'sc' if sc else 'nosc'}"
            res['runs'][key] = row
            if kind == 'ddim':
                # the fused step alone, on the captured state's buffers (a mid-loop DDIM entry, drawing noise)
                ops.sampler_seek(st['cursor'], 0, st['table'], st['times'], st['cur'], st['tcond'])
                mo = torch.randn_like(st['img'])
                img = st['img'].clone()
                xin = st['xin'].clone()
                state = d.rng.state.clone()
                ids = d.rng.ids_for(B)

                def step():
                    ops.sampler_step_ddp_dev(st['cur'], st['cursor'], st['draws'], mo, img, None, ids, state, xin=xin,
                                             self_cond=sc)
                step()
                us = 1e3 * timed(step, a.kernel_reps)
                n = img.numel()
                nbytes = 4 * (3 * n + xin.numel())          # model output + img read, img written, padded input written
                res[f'fused_step_{"sc" if sc else "nosc"}'] = {
                    'us_per_launch': round(us, 3), 'bytes': nbytes, 'TB_per_s': round(nbytes / us / 1e6, 3),
                    'fraction_of_8TBps': round(nbytes / us / 1e6 / (HBM_BPS / 1e12), 4),
                    'cpad': int(xin.shape[3]), 'noise': 'drawn in-kernel (keyed), not read'}
                img = xin = mo = None
            d = None
        model = None
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
