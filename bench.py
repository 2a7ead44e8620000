#!/usr/bin/env python3
"""Headline benchmark: sampled images/sec of the DGM denoising hot path (BASELINE.json).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

Workload (BASELINE.json configs[1], README inference config at 128x128): CFG Unet dim=64,
dim_mults (1,2,4,8), channels=6, GaussianDiffusion(image_size=128, timesteps=1000,
sampling_timesteps=32, objective='pred_x0'), cond_scale=3 (2 UNet forwards per denoise step,
run as one 2B batch), bs=25 per GPU.  One "step" = one pass of the hot path over one batch:
sample() (32 denoise steps) + the uint8 / homography record of Trainer.sample + (N>1) the
gather to rank 0.  Inputs (conditions, weights) are resident in HBM before the timed region;
weights are seeded random init (the trained DGM.pt is not available offline; speed is weight
independent), noise comes from the sample-indexed device generator (dmh_rng_indexed: row i of an N-rank run is row i
of the 1-GPU run).  Samples shard across ranks with no
data-path collective -> "scaling": "weak" (25 samples per GPU).

N > 1 without a torchrun environment: this process only LAUNCHES (it never touches the GPU): it starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child, relays rank 0's JSON line and exits
with the child's code — the counterpart of the reference's N hand-started processes (README:14,
DGM/dgm_sample.py:13-18).

Prints ONE JSON line on rank 0.  A plain run does only what the headline needs: it sets up, warms up, times the K steps,
writes its outputs (--dump-outputs) and prints the line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step`, `config`, ...).  With --full it also measures and checks the rest, all of it outside the timed region
(each leg can be left out with its --no-* flag):
  phases       the per-rank / per-phase diagnosis of an N-rank line
  variants     dedup_dropped_rows (the opt-in row de-duplication, timed in extra steps) and, N = 1, exact_fp32 (a fresh
               child process under DMH_CONV3_VARIANT=6); config.measured_rel_error: the canonical conv against fp64
  roofline     the dominant kernel (stride-1 3x3 conv, conv_f16x3_kernel<3,3,1,0,...>: implicit GEMM on the fp16
               matrix cores, every fp32 product carried by three fp16 MFMAs under block scaling).
               achieved = ALGORITHMIC FLOPs (2*9*Cin*Cout*H*W*B) of its launches / their HIP-event
               durations;  peak = the dense fp16 MFMA peak of MI355X (2.5 PFLOP/s, MI355X_MICROARCH.md) / 3 executed
               FLOPs per algorithmic FLOP = 833 algorithmic TFLOP/s: the ceiling of this arithmetic on the pipe it
               runs on;  frac = achieved / peak (= executed fp16-MFMA FLOP/s / 2.5 PFLOP/s).  Beside it
               `hbm_frac_canonical`: the north_star's yardstick, algorithmic bytes of the canonical fused
               conv3x3+GN+SiLU 64->64 @128^2 launch / its time / 8 TB/s (target >= 0.30), and `vs_fp32_mfma_peak`
               (what an exact-fp32 MFMA kernel could reach at most).  HIP events sit on the launch stream around
               every dmh_conv2d of ONE EXTRA untimed step in batched mode (exclusive per-launch durations: in the
               default 'streams' mode the two CFG passes overlap); the timed region itself carries no events.
               traffic = HBM bytes per launch of that kernel, MEASURED BY THIS RUN (round 5): two child runs of this script
               under `rocprofv3 --pmc` (FETCH_SIZE x2, WRITE_SIZE: separate passes) after the timed region; the committed
               figure of profiles/ stays beside it (`traffic_committed`, `traffic_vs_committed`); `--no-traffic`, N > 1 or a
               failing profiler fall back to the committed figure, tagged with its source file
  cpu_baseline the oracle (a port of the reference's CPU path, bit-equal to it on the build host)
               timed on this box's host cores on a bounded sample (bs=2, s_step=4, same network).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_FP32_MFMA_TFLOPS = 157.3     # dense fp32 MFMA = fp32 vector peak (MI355X_MICROARCH.md)
PEAK_FP16_MFMA_TFLOPS = 2500.0    # dense fp16 / bf16 MFMA peak (same guide); the pipe conv_f16x3_kernel executes on
PEAK_HBM_TBS = 8.0                # HBM3E peak (same guide)
F16X3_TERMS = 3                   # executed fp16 MFMA FLOPs per algorithmic FLOP (h2*g1s + h1*g2 + h1*g1)


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a torchrun environment: start the N ranks as a child process tree and relay
    rank 0's JSON line.  This parent makes no HIP / torch.cuda call (it does not even import torch) and never
    re-execs itself; it exits non-zero when any rank failed."""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC: what RCCL needs on this pool
    env.setdefault('OMP_NUM_THREADS', '8')
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = None
    for out in proc.stdout:
        if out.startswith('{') and '"metric"' in out:
            line = out.strip()
        else:
            sys.stdout.write(out)
    rc = proc.wait()
    if line is not None:
        print(line, flush=True)
    if rc != 0 or line is None:
        print(f'bench.py: the {n}-rank child run failed (exit code {rc}, JSON line {"present" if line else "missing"})',
              file=sys.stderr)
        sys.exit(rc if rc != 0 else 1)


_RDZV_VARS = ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'GROUP_RANK', 'ROLE_RANK', 'ROLE_NAME',
              'ROLE_WORLD_SIZE', 'GROUP_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')


def child_env(**extra):
    """environment of a measurement child (a FRESH process: never a re-exec of this one): the rendezvous variables of a
    torchrun parent are removed — a one-rank child must not join, or collide with, the parent's still-live process group"""
    env = {k: v for k, v in os.environ.items() if k not in _RDZV_VARS and not k.startswith('TORCHELASTIC_')}
    env.update(extra)
    return env


def run_child(cmd, timeout, env=None, cwd=None):
    """subprocess.run(capture_output=True) for a child that has children of its own (rocprofv3 -> python): the child leads a
    new session, and on a timeout the whole process GROUP is killed — killing rocprofv3 alone would leave its python child on
    the GPU holding the pipes, and the read that follows the kill would block for good.  -> (returncode, stdout, stderr);
    raises subprocess.TimeoutExpired after the group is gone."""
    import signal
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=cwd,
                            start_new_session=True)
    try:
        out, err = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        try:
            proc.communicate(timeout=15)
        except subprocess.TimeoutExpired:
            pass                                             # (a grandchild that left the group still holds a pipe: give up on it)
        raise
    return proc.returncode, out, err


def under_profiler():
    """True when this process runs under rocprofv3 / a rocprofiler-sdk tool preload (every process of such a tree has the GPU
    initialised before main(): it must not start programs that exec again — shebang scripts, env, sh -c)"""
    return 'rocprof' in os.environ.get('LD_PRELOAD', '').lower() or any(
        k.startswith(('ROCPROF', 'ROCP_TOOL', 'ROCPROFILER')) for k in os.environ)


def smi_sample(device_index):
    """ONE `rocm-smi --json` call for this rank's GPU (no sampling thread): the SMU's own running averages of clock and
    socket power, read right before and right after the timed region — on an 8-GPU chassis a throttled GPU (this workload
    sits on the power limit) shows here.  rocm-smi does not initialise HIP.  -> {field: value} or {'error': ...}"""
    import re
    import shutil
    if under_profiler():
        # rocm-smi is a `#!/usr/bin/env python3` script: under rocprofv3 the preloaded tool library initialises the GPU in
        # `env` before it execs python3 — the exec-after-GPU-init this pool forbids (seen once, refused by the box, round 6)
        return {'skipped': 'running under a profiler preload: no child programs are started'}
    exe = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    try:
        r = subprocess.run([exe, '-d', str(device_index), '--showclocks', '--showpower', '--showtemp', '--json'],
                           capture_output=True, text=True, timeout=20)
        cards = json.loads(r.stdout.strip().splitlines()[-1])
        card = next(v for k, v in sorted(cards.items()) if k.startswith('card'))
        keep = {}
        for k, v in card.items():
            if re.search(r'sclk|power|junction', k, re.I):
                m = re.search(r'-?[0-9]+(\.[0-9]+)?', str(v))
                keep[k.strip(' :')] = float(m.group(0)) if m else v
        return keep
    except Exception as e:                                   # (no rocm-smi, another JSON shape): reported, never fatal
        return {'error': f'{type(e).__name__}: {str(e)[:120]}'}


def conv_error(image_size, dev):
    """the measured error of THIS process's convolution arithmetic (fp16 pieces by default, the exact-fp32 kernels under
    DMH_CONV3_VARIANT=6) on the canonical shape: one row of a weight-standardised 3x3 conv 64 -> 64 at image_size^2 on N(0,1)
    activations (CFG:114-128) against an fp64 F.conv2d on the host; max |y - y64| / max |y64|."""
    import torch
    import torch.nn.functional as F
    from dmhomo_amd import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn((1, 64, image_size, image_size), generator=g)
    w = torch.randn((64, 64, 3, 3), generator=g)
    b = torch.randn((64,), generator=g)
    wd = w.double()
    mean = wd.mean(dim=(1, 2, 3), keepdim=True)
    var = wd.var(dim=(1, 2, 3), unbiased=False, keepdim=True)
    ws = (wd - mean) * (var + 1e-5).rsqrt()
    ref = F.conv2d(x.double(), ws, b.double(), padding=1)
    pc = ops.PackedConv(ws.float().contiguous().to(dev), b.to(dev), 64)
    y = ops.conv2d(pc, x.permute(0, 2, 3, 1).contiguous().to(dev)).permute(0, 3, 1, 2).double().cpu()
    return float((y - ref).abs().max() / ref.abs().max())


def exact_fp32_variant(args, timeout=420):
    """`variants.exact_fp32`: the same command in a FRESH child process under DMH_CONV3_VARIANT=6 (read once per process:
    every 3x3 conv on the exact-fp32 Winograd kernel, the other convs on the fp32-MFMA implicit GEMM) — what the precision /
    throughput trade of `config.arithmetic` buys on THIS box.  -> dict for the JSON line (an 'error' entry when it failed)."""
    cmd = [sys.executable, os.path.abspath(__file__), '--steps', '3', '--warmup', '1', '--bs', str(args.bs), '--s_step',
           str(args.s_step), '--image_size', str(args.image_size), '--dim', str(args.dim), '--cfg-mode', args.cfg_mode,
           '--full', '--no-variants', '--no-traffic', '--no-cpu-baseline', '--no-roofline', '--no-phases'] + (
               ['--no-graph'] if args.no_graph else [])
    try:
        rc, out, err = run_child(cmd, timeout, env=child_env(DMH_CONV3_VARIANT='6'), cwd=ROOT)
        lines = [l for l in out.splitlines() if l.startswith('{') and '"metric"' in l]
        if rc != 0 or not lines:
            return {'error': f'child exit code {rc}: {err[-300:]}'}
        d = json.loads(lines[-1])
        return {'value': d['value'], 'unit': 'images/s', 'ms_per_step': d['ms_per_step'],
                'ms_per_denoise_step': d['ms_per_denoise_step'], 'steps': d['steps'],
                'measured_rel_error': d['config'].get('measured_rel_error'),
                'how': 'a fresh child process of this script under DMH_CONV3_VARIANT=6, after the timed region',
                'arithmetic': 'every conv in exact fp32: 3x3 = Winograd F(2x2,3x3) on fp32 MFMA (conv_wino.hip), the rest = '
                              'fp32-MFMA implicit GEMM (conv.hip); attention projections unchanged'}
    except subprocess.TimeoutExpired:
        return {'error': f'the child did not finish in {timeout} s (its process group was killed)'}
    except Exception as e:
        return {'error': f'{type(e).__name__}: {str(e)[:200]}'}


def cpu_model():
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def physical_cores():
    """distinct (physical id, core id) pairs of /proc/cpuinfo (SMT siblings counted once); None when it cannot be read"""
    try:
        cores, phys, cid = set(), None, None
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('physical id'):
                    phys = line.split(':', 1)[1].strip()
                elif line.startswith('core id'):
                    cid = line.split(':', 1)[1].strip()
                elif not line.strip():
                    if cid is not None:
                        cores.add((phys, cid))
                    phys = cid = None
        if cid is not None:
            cores.add((phys, cid))
        return len(cores) or None
    except OSError:
        return None


def _oracle_forward_setup(dim, image_size, conds=None):
    import torch
    from oracle import unet as OU
    from detweights import det_state_dict, shapes_of
    from dmhomo_amd import cfg
    m = cfg.Unet(dim=dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    sd = det_state_dict(shapes_of(m))
    B = 2
    g = torch.Generator().manual_seed(1)
    if conds is not None and conds[0].shape[0] >= B:
        rgb, mask = conds[0][:B].contiguous(), conds[2][:B].contiguous()
    else:
        rgb = torch.rand((B, 3, image_size, image_size), generator=g)
        mask = (torch.rand((B, 1, image_size, image_size), generator=g) > 0.5).float()
    x = torch.randn((B, 6, image_size, image_size), generator=g)
    tt = torch.full((B,), 500, dtype=torch.long)
    classes = torch.zeros(B, dtype=torch.long)

    def forward():
        with torch.no_grad():
            OU.cfg_unet_forward(sd, x, tt, classes, rgb, mask, None)
    return forward


def cpu_probe(args):
    """child-process mode (`bench.py --cpu-probe N`): median seconds of 3 oracle UNet forwards (bs=2) at N threads, after one
    warm-up — the all-cores point of `cpu_baseline`, run apart so that the parent can bound it with a timeout"""
    import torch
    torch.set_num_threads(args.cpu_probe)
    fwd = _oracle_forward_setup(args.dim, args.image_size)
    fwd()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fwd()
        ts.append(time.perf_counter() - t0)
    print(json.dumps({'threads': args.cpu_probe, 'median_s': sorted(ts)[1], 'all_s': ts}))


def cpu_baseline(dim, image_size, seconds=12.0, slice_bs=0, conds=None):
    """oracle (kind 'port') on the host cores: bs=2, s_step=4 passes of the same network, reported as
    images/s at s_step=32 (cost per denoise step is constant, so x 4/32).  conds: (rgb_flow01, flow, mask) CPU tensors —
    rows of the synthetic conditions the GPU leg ran on.
    Thread count: oneDNN over-threads this bs=2 workload on a many-core host (8 threads 0.24 s, 16: 0.13 s, 32: 0.26 s,
    128: 1.24 s, 256: 104 s per UNet forward on the round-1 / round-4 boxes), so a sweep picks it — on the MEDIAN of three
    forwards per count (round 4 picked on one: a 1 % difference moved `value` by 25 % between runs), near-ties (< 3 %) going
    to the larger count — and the real sample is then timed at the best TWO counts; both are reported, `value` is the
    faster.  The all-physical-cores point SURVEY 8d asks for is measured in a child process under a timeout."""
    import torch
    from oracle import diffusion as OD
    from detweights import det_state_dict, shapes_of
    from dmhomo_amd import cfg
    m = cfg.Unet(dim=dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    sd = det_state_dict(shapes_of(m))
    buf = OD.schedule_buffers(1000, 'cosine')
    B, S = 2, 4
    g = torch.Generator().manual_seed(1)

    def conditions(n):
        if conds is not None and conds[0].shape[0] >= n:
            return tuple(t[:n].contiguous() for t in conds)
        return (torch.rand((n, 3, image_size, image_size), generator=g),
                torch.zeros((n, 2, image_size, image_size)),
                (torch.rand((n, 1, image_size, image_size), generator=g) > 0.5).float())
    rgb, flow, mask = conditions(B)
    classes = torch.zeros(B, dtype=torch.long)
    ncpu = os.cpu_count() or 1
    nphys = physical_cores() or ncpu
    fwd = _oracle_forward_setup(dim, image_size, conds)
    tried = {}
    for nt in sorted({n for n in (8, 16, 32, 64) if n <= ncpu} or {ncpu}):
        torch.set_num_threads(nt)
        fwd()                                            # warm-up at this count (oneDNN primitive caches, thread pool)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fwd()
            ts.append(time.perf_counter() - t0)
        tried[nt] = round(sorted(ts)[1], 4)
        if tried[nt] > 1.5 * min(tried.values()):
            break                                            # (past the optimum: the wider settings only get slower)
    best = min(tried.values())
    ranked = sorted(tried, key=lambda n: (tried[n] > 1.03 * best, tried[n] if tried[n] > 1.03 * best else -n))
    picks = ranked[:2]

    def sample_rate(nt):
        torch.set_num_threads(nt)

        def one():
            with torch.no_grad():
                OD.cfg_sample(sd, buf, classes, rgb, flow, mask, image_size=image_size, channels=6,
                              sampling_timesteps=S, objective='pred_x0')
        one()                                               # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            one()
            n += 1
            el = time.perf_counter() - t0
            if el >= seconds / len(picks) or n >= 4:
                break
        return el / n, n
    timed = {nt: sample_rate(nt) for nt in picks}
    cores = min(timed, key=lambda n: timed[n][0])
    per_pass, n = timed[cores]
    torch.set_num_threads(cores)
    # the all-physical-cores point, bounded: a child process, killed after 90 s
    allc = {'threads': nphys}
    if nphys in tried:
        allc['forward_s'] = tried[nphys]
    else:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpu-probe', str(nphys), '--dim', str(dim),
                                '--image_size', str(image_size)], capture_output=True, text=True, timeout=90)
            allc['forward_s'] = json.loads(r.stdout.strip().splitlines()[-1])['median_s'] if r.returncode == 0 else None
            if r.returncode != 0:
                allc['error'] = r.stderr[-300:]
        except subprocess.TimeoutExpired:
            allc['forward_s'] = None
            allc['note'] = 'more than 90 s for warm-up + 3 forwards: over-threaded (the child was killed)'
    res = {'value': B * (S / 32.0) / per_pass, 'unit': 'images/s (s_step=32 equivalent)', 'cores': cores,
           'kind': 'port', 'cpu_model': cpu_model(), 'host_cores': ncpu, 'physical_cores': nphys,
           'threads_tried': {str(k): v for k, v in tried.items()},
           'threads_note': 'MEDIAN seconds of 3 oracle UNet forwards (bs=2) per thread count; the best two counts (ties < 3 % '
                           'to the larger) then run the real sample: `at_threads`; `cores` / `value` = the faster of them',
           'at_threads': {str(k): {'value': B * (S / 32.0) / v[0], 's_per_pass': round(v[0], 3), 'passes': v[1]}
                          for k, v in timed.items()},
           'all_physical_cores': allc,
           'conditions': 'synthetic homography conditions of the GPU leg (SURVEY 8d)' if conds is not None else 'torch.rand',
           'sample': f'oracle cfg_sample bs={B} s_step={S} {image_size}x{image_size} dim={dim}, {n} passes, '
                     f'{per_pass:.2f} s/pass = {per_pass / S * 1000:.0f} ms per denoise step (bs={B}); '
                     f'images/s scaled by 4/32 to s_step=32'}
    if allc.get('forward_s'):
        # one denoise step = 2 forwards; the sample's other work is < 1 % of it
        allc['value_estimate'] = B / (2 * allc['forward_s']) / 32.0
        allc['estimate_note'] = 'images/s (s_step=32 equivalent) from the forward time alone: bs / (2 forwards x 32 steps)'
    if slice_bs:
        # SURVEY 8d's second CPU row: a slice of the headline configuration itself (bs = 25, s_step = 2), extrapolated x16
        Bs, Ss = slice_bs, 2
        rgb2, flow2, mask2 = conditions(Bs)
        t1 = time.perf_counter()
        with torch.no_grad():
            OD.cfg_sample(sd, buf, torch.zeros(Bs, dtype=torch.long), rgb2, flow2,
                          mask2, image_size=image_size, channels=6, sampling_timesteps=Ss, objective='pred_x0')
        el2 = time.perf_counter() - t1
        res['slice'] = {'value': Bs * (Ss / 32.0) / el2, 'unit': 'images/s (s_step=32 equivalent)', 'cores': cores,
                        'sample': f'oracle cfg_sample bs={Bs} s_step={Ss} (one pass, {el2:.1f} s), EXTRAPOLATED x16 to '
                                  f's_step=32: the cost per denoise step is constant'}
    return res


def assemble_phases(mine, rank, world, broadcast_ms, broadcast_first_ms):
    """every rank hands in its own figures (`mine`); rank 0 gets the `phases` object of the JSON line, the others None.
    How to read it: `value` is global images / the barrier-to-barrier MAXIMUM; a sub-linear N-rank
    line is then explained by per_rank_ms (one slow rank = `straggler_rank`: look at its smi clocks / power — throttling),
    by gather_ms (transport of the records to rank 0) or by neither (launch jitter: per_rank_ms_max well under ms_per_step);
    broadcast_ms is start-up cost outside the timed region."""
    import torch.distributed as dist
    every = [mine]
    if world > 1:
        every = [None] * world
        dist.all_gather_object(every, mine)
    if rank != 0:
        return None
    per = [e['ms_per_step'] for e in every]
    return {
        'per_rank_ms': per, 'per_rank_ms_min': min(per), 'per_rank_ms_max': max(per),
        'per_rank_ms_mean': sum(per) / len(per), 'straggler_rank': per.index(max(per)),
        'broadcast_ms': broadcast_ms, 'broadcast_first_ms': broadcast_first_ms,
        'local_ms': [e['local_ms'] for e in every], 'gather_ms': [e['gather_ms'] for e in every],
        'smi': [{'rank': e['rank'], 'device': e['device'], 'host': e['host'], 'before': e['smi_before'],
                 'after': e['smi_after']} for e in every],
        'note': 'per_rank_ms: each rank\'s own wall time per timed step up to ITS last kernel (the line\'s ms_per_step is '
                'the barrier-to-barrier maximum); broadcast_ms: the weight payload (scatter + all-gather) repeated once '
                'the communicator exists, broadcast_first_ms: the first call; local_ms / gather_ms: sample + record, '
                'then — after a barrier — the gather to rank 0, of ONE instrumented step after the timed region; smi: '
                'one rocm-smi --json call per rank right before / right after the timed loop (the SMU\'s averages)'}


def plumbing_only(args):
    """tests/test_distributed_cpu.py only: the N > 1 plumbing of this script (launcher -> ranks -> process group ->
    weight payload -> shards -> gather -> max-over-ranks timing -> ONE JSON line) on gloo / CPU, with the sampling
    step left out — there is no CPU path for it.  Refuses to run outside that test."""
    if os.environ.get('DMH_BENCH_PLUMBING_TEST') != '1':
        raise RuntimeError('bench.py --device cpu is a test-only plumbing mode (tests/test_distributed_cpu.py); the '
                           'benchmark itself needs MI355X GPUs — there is no CPU path')
    import torch
    import torch.distributed as dist
    from dmhomo_amd import cfg
    from dmhomo_amd import distributed as D
    rank, world, device = D.init_from_env('gloo')
    assert world == args.gpus and device.type == 'cpu'
    torch.manual_seed(rank)                               # different weights per rank before the payload
    model = cfg.Unet(dim=8, dim_mults=(1, 2), channels=6, num_classes=1)
    diffusion = cfg.GaussianDiffusion(model, image_size=16, timesteps=50, sampling_timesteps=4, objective='pred_x0')
    dist.barrier()
    tb = time.perf_counter()
    D.broadcast_module_(diffusion, src=0)
    dist.barrier()
    broadcast_first_ms = broadcast_ms = (time.perf_counter() - tb) * 1e3
    if not args.no_phases:
        tb = time.perf_counter()
        D.broadcast_module_(diffusion, src=0)
        dist.barrier()
        broadcast_ms = (time.perf_counter() - tb) * 1e3
    digest = torch.tensor([float(sum(p.double().sum() for p in diffusion.state_dict().values()))], dtype=torch.float64)
    lo, hi = D.shard_bounds(args.bs * world, rank, world)
    imgs = torch.arange(lo, hi, dtype=torch.uint8).reshape(-1, 1, 1, 1).expand(-1, 6, 4, 4).contiguous()
    homos = torch.arange(lo, hi, dtype=torch.float64).reshape(-1, 1, 1).expand(-1, 3, 3).contiguous()
    smi_before = smi_sample(0) if not args.no_phases else None
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gi, gh = D.gather_records(imgs, homos, dst=0)
    elapsed_local = time.perf_counter() - t0
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    phases = None
    if not args.no_phases:
        tg = time.perf_counter()
        D.gather_records(imgs, homos, dst=0)
        phases = assemble_phases({'rank': rank, 'ms_per_step': elapsed_local / max(args.steps, 1) * 1e3, 'local_ms': 0.0,
                                  'gather_ms': (time.perf_counter() - tg) * 1e3, 'smi_before': smi_before,
                                  'smi_after': smi_sample(0), 'host': socket.gethostname(), 'device': str(device)},
                                 rank, world, broadcast_ms, broadcast_first_ms)
    ranks = torch.ones(1)
    dist.all_reduce(ranks)
    dmin, dmax = digest.clone(), digest.clone()
    dist.all_reduce(dmin, op=dist.ReduceOp.MIN)
    dist.all_reduce(dmax, op=dist.ReduceOp.MAX)
    if rank == 0:
        ok = (gi[:, 0, 0, 0].tolist() == list(range(args.bs * world)) and gh[:, 0, 0].tolist() ==
              [float(i) for i in range(args.bs * world)] and float(dmin) == float(dmax))
        res = {'metric': 'plumbing only (no sampling: CPU test mode)', 'value': None, 'n_gpus': world,
               'steps': args.steps, 'warmup': args.warmup, 'rccl_ranks': int(ranks.item()),
               'backend': dist.get_backend(), 'plumbing_only': True, 'records_in_rank_order': bool(ok),
               'global_batch': args.bs * world, 'elapsed_s': float(t.item())}
        if phases is not None:
            res['phases'] = phases
        print(json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def parse_args(argv=None):
    """the command line; without --full every leg beside the headline is switched off (the --no-* flags then say so)"""
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--bs', type=int, default=25, help='samples per GPU')
    ap.add_argument('--s_step', type=int, default=32)
    ap.add_argument('--image_size', type=int, default=128)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--full', action='store_true',
                    help='also measure and check everything beside the headline, outside the timed region: `phases`, '
                         '`roofline` (with its rocprofv3 traffic passes), `variants` (dedup_dropped_rows, exact_fp32), '
                         '`config.measured_rel_error` and `cpu_baseline`; the --no-* flags below leave out one of them. '
                         'Without it a run sets up, warms up, times the steps, dumps its outputs if asked and prints the line')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU oracle baseline')
    ap.add_argument('--cfg-mode', default='streams', choices=['batched', 'streams'])
    ap.add_argument('--stream-splits', type=int, default=1, help="row sub-batches per CFG pass in 'streams' mode")
    ap.add_argument('--no-graph', action='store_true', help="launch every kernel from Python instead of replaying the "
                    "HIP graph of the sampling loop (cfg.GaussianDiffusion.hip_graph)")
    ap.add_argument('--no-roofline', action='store_true', help='with --full: skip the extra untimed step that carries the '
                    'HIP events')
    ap.add_argument('--no-traffic', action='store_true',
                    help='with --full: quote roofline.traffic from the committed PMC profile instead of measuring it (two '
                         'child runs under rocprofv3 --pmc, ~40 s, after the timed region; single-GPU runs only)')
    ap.add_argument('--no-variants', action='store_true',
                    help='with --full: skip the extra steps (after the timed region) that time cfg.Unet.dedup_dropped_rows '
                         'and the exact-fp32 child run, reported under "variants" (the headline `value` never includes them)')
    ap.add_argument('--no-phases', action='store_true',
                    help='with --full: skip the per-rank / per-phase diagnosis (weight payload, local step, gather, rocm-smi '
                         'samples: all outside the timed region) reported under "phases"')
    ap.add_argument('--dedup', action='store_true',
                    help='development / profiling: run the TIMED loop itself with cfg.Unet.dedup_dropped_rows (the line is then '
                         'labelled as that variant and is not the headline)')
    ap.add_argument('--workload', default='sample', choices=['sample', 'train'],
                    help="'train': the optimiser step of BASELINE configs[3] (16 images per GPU, gradients averaged over "
                         "RCCL) instead of the headline sampling loop; same launch contract, see tools/train_bench.py")
    ap.add_argument('--cpu-probe', type=int, default=0, help='internal: the child-process mode of cpu_baseline (see cpu_probe)')
    ap.add_argument('--device', default='cuda', choices=['cuda', 'cpu'],
                    help="'cpu' is the test-only plumbing mode of tests/test_distributed_cpu.py (raises elsewhere)")
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step returned (rank 0\'s gathered records: '
                         'imgs as float32, homos as float64) to DIR/<name>.npy, at most 64 MB in all (see dump_outputs)')
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    if args.dump_outputs and (args.workload != 'sample' or args.device != 'cuda'):
        ap.error('--dump-outputs covers the sampling workload on the GPU only')
    if not args.full:
        args.no_cpu_baseline = args.no_roofline = args.no_traffic = args.no_variants = args.no_phases = True
    return args


def main():
    args = parse_args()
    if args.cpu_probe:
        return cpu_probe(args)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return launch_ranks(args.gpus, sys.argv[1:])       # before anything touches torch / the GPU
    if args.device == 'cpu':
        return plumbing_only(args)
    if args.workload == 'train':
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        import train_bench
        ns = argparse.Namespace(bs=16 if args.bs == 25 else args.bs, size=args.image_size, dim=args.dim, steps=args.steps,
                                warmup=args.warmup, accum=1, torch=False)
        line = train_bench.run(ns)
        if line is not None:
            print(json.dumps(line))
        return

    import torch
    import torch.distributed as dist
    from dmhomo_amd import cfg, ddpm, ops
    from dmhomo_amd import distributed as D

    rank, world, device = D.init_from_env()
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'
    assert device.type == 'cuda', 'bench.py needs MI355X GPUs (no CPU path)'

    # ---- model: seeded init on every rank, then rank 0's weights win (one scatter+all-gather payload)
    torch.manual_seed(0)
    model = cfg.Unet(dim=args.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1)
    model.cfg_mode = args.cfg_mode
    model.stream_splits = args.stream_splits
    model.dedup_dropped_rows = bool(args.dedup)
    diffusion = cfg.GaussianDiffusion(model, image_size=args.image_size, timesteps=1000,
                                      sampling_timesteps=args.s_step, loss_type='l1', objective='pred_x0').to(device)
    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # the weight payload (scatter + all-gather, distributed.py); for `phases` timed twice: the first call also builds the
    # communicator
    fence()
    tb = time.perf_counter()
    D.broadcast_module_(diffusion, src=0)
    fence()
    broadcast_first_ms = broadcast_ms = (time.perf_counter() - tb) * 1e3
    if not args.no_phases:
        tb = time.perf_counter()
        D.broadcast_module_(diffusion, src=0)
        fence()
        broadcast_ms = (time.perf_counter() - tb) * 1e3
    # (ONE denoise step is captured and replayed s_step times: any depth, the 250-step stress configuration included)
    use_graph = not args.no_graph
    diffusion.hip_graph = use_graph
    # ---- synthetic conditions of this rank's shard, resident in HBM
    lo, hi = D.shard_bounds(args.bs * world, rank, world)
    # noise keyed by GLOBAL sample index (dmh_rng_indexed inside the captured denoise step): row i of the N-rank job is
    # row i of the 1-GPU job, whatever N is (the reference's N hand-started processes each draw their own, unseeded stream)
    D.key_noise_by_sample(diffusion, 99, args.bs * world, device=device)
    conds = ddpm.SyntheticConditions(args.image_size, hi - lo, seed=1000 + lo, device=device)
    data, classes = next(conds)
    rgb_flow, flow, mask = data[:, -5:-2].contiguous(), data[:, -2:].contiguous(), data[:, -6:-5].contiguous()

    def step():
        img, _, fl = diffusion.sample(classes, rgb_flow, flow, mask)          # cond_scale=3 (CFG:714)
        imgs_u8 = ops.to_uint8(img)
        homos = ops.dlt_homography(fl)
        return D.gather_records(imgs_u8, homos, dst=0)

    for _ in range(args.warmup):
        step()
    fence()
    smi_before = smi_sample(device.index or 0) if not args.no_phases else None
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    elapsed_local = time.perf_counter() - t0             # this rank's own finish line (before it waits for the others)
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)             # (outside the timed region, before the untimed extra steps)
    # ---- phases (N-rank diagnosis; all of it OUTSIDE the timed region): the SMU's averages right after the loop, then one
    # instrumented step with the local work (sample + record) and the gather timed apart, a barrier between them so that the
    # gather's time is the transport, not the wait for the slowest rank
    phases = None
    if not args.no_phases:
        smi_after = smi_sample(device.index or 0)
        fence()
        tl = time.perf_counter()
        img_, _, fl_ = diffusion.sample(classes, rgb_flow, flow, mask)
        u8_, hm_ = ops.to_uint8(img_), ops.dlt_homography(fl_)
        torch.cuda.synchronize()
        local_ms = (time.perf_counter() - tl) * 1e3
        fence()
        tg = time.perf_counter()
        D.gather_records(u8_, hm_, dst=0)
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - tg) * 1e3
        mine = {'rank': rank, 'ms_per_step': elapsed_local / max(args.steps, 1) * 1e3, 'local_ms': local_ms, 'gather_ms': gather_ms,
                'smi_before': smi_before, 'smi_after': smi_after, 'host': socket.gethostname(), 'device': str(device)}
        phases = assemble_phases(mine, rank, world, broadcast_ms, broadcast_first_ms)
    # ---- roofline leg: HIP events on the launch stream around every dmh_conv2d of ONE EXTRA untimed step with the
    # cond + null rows in one launch sequence (exclusive per-launch durations; same kernels, same shapes)
    log = None
    if not args.no_roofline and rank == 0:
        diffusion.hip_graph = False                      # (per-launch HIP events need eager launches)
        model.cfg_mode = 'batched'
        step_local = lambda: diffusion.sample(classes, rgb_flow, flow, mask)   # no collective: rank 0 only
        step_local()
        torch.cuda.synchronize()
        ops.CONV_LOG = []
        step_local()
        torch.cuda.synchronize()
        log, ops.CONV_LOG = ops.CONV_LOG, None
        model.cfg_mode = args.cfg_mode
    # ---- variants: reported beside the headline, never as it: the opt-in de-duplication of the conditional pass's
    # dropped rows (cfg.Unet.dedup_dropped_rows: identical samples, B + kept rows per denoise step instead of 2B), in the
    # headline's own configuration (captured step, cfg_mode as above), timed after the timed region
    dedup_elapsed, dedup_rows, dedup_steps = 0.0, None, max(2, min(args.steps, 5))
    if not args.no_variants:
        diffusion.hip_graph = use_graph
        model.dedup_dropped_rows = True
        step()                                           # (captures the de-duplicating step)
        fence()
        base_draw = int(diffusion.rng.state[1].item())
        t1 = time.perf_counter()
        for _ in range(dedup_steps):
            step()
        fence()
        dedup_elapsed = (time.perf_counter() - t1) / dedup_steps
        model.dedup_dropped_rows = bool(args.dedup)
        # the UNet rows those steps computed: the keep masks are a pure function of (seed, sample id, draw index) — a
        # sample() call makes 2 * s_step draws, the mask of denoise step k is draw 1 + 2k of the call
        st_, kept = diffusion.rng.state.clone(), 0
        for c_ in range(dedup_steps):
            for k_ in range(args.s_step):
                st_[1] = base_draw + c_ * 2 * args.s_step + 1 + 2 * k_
                kept += int(ops.rng_keep_mask(diffusion.rng.sample_ids, st_, 1 - model.cond_drop_prob).sum().item())
        dedup_rows = (hi - lo) + kept / (dedup_steps * args.s_step)
    rccl_ranks = 1
    if world > 1:
        t = torch.tensor([elapsed, dedup_elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, dedup_elapsed = float(t[0].item()), float(t[1].item())
        ones = torch.ones(1, device=device)
        dist.all_reduce(ones)                             # every rank took part in an RCCL collective
        rccl_ranks = int(ones.item())
        assert rccl_ranks == dist.get_world_size()

    if rank == 0:
        images = args.bs * world * args.steps
        res = {
            'metric': f'sampled images/sec ({args.image_size}x{args.image_size}, s_step={args.s_step})' + (
                ' [--dedup: the dedup_dropped_rows VARIANT, not the headline]' if args.dedup else ''),
            'value': images / elapsed, 'unit': 'images/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': elapsed / args.steps * 1e3,
            'ms_per_denoise_step': elapsed / args.steps / args.s_step * 1e3,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'rccl_ranks': rccl_ranks, 'backend': (dist.get_backend() if world > 1 else None),
            'config': {'workload': f'DGM CFG-Unet dim={args.dim} {args.image_size}x{args.image_size} '
                                   f'bs={args.bs}/GPU s_step={args.s_step} cond_scale=3 ' + (
                                       '(BASELINE configs[1])' if (args.dim, args.image_size, args.bs, args.s_step) ==
                                       (64, 128, 25, 32) else '(BASELINE configs[4], stress; NOT the headline)' if
                                       (args.dim, args.image_size, args.bs, args.s_step) == (128, 256, 8, 250) else
                                       '(README / DGM/dgm_sample.py:28-38 geometry image_size=256; NOT the headline)' if
                                       (args.dim, args.image_size, args.bs, args.s_step) == (64, 256, 25, 32) else
                                       '(non-BASELINE configuration)'),
                       'global_batch': args.bs * world, 'sharding': f'samples x{world}, no data-path collective',
                       'cfg_mode': args.cfg_mode, 'hip_graph': use_graph,
                       'weights': 'seeded random init',
                       'noise': 'Philox4x32-10 keyed by (seed, global sample id, draw, element): dmh_rng_indexed, rows invariant to N',
                       'arithmetic': 'fp32 tensors; 3x3 / 1x1 convolutions and the attention projections multiply block-scaled '
                                     'fp16 pieces of the fp32 operands on the matrix cores (3 MFMAs per product block, '
                                     'fp32 accumulate, error at the fp32-accumulation level: DESIGN.md 3.1); '
                                     'DMH_CONV3_VARIANT=6 selects the exact-fp32 kernels'},
        }
        if not args.no_variants:
            res['variants'] = {'dedup_dropped_rows': {
                'value': args.bs * world / dedup_elapsed, 'unit': 'images/s', 'ms_per_step': dedup_elapsed * 1e3,
                'speedup_vs_value': (args.bs * world / dedup_elapsed) / (images / elapsed), 'steps': dedup_steps,
                'hip_graph': use_graph, 'cfg_mode': args.cfg_mode,
                'unet_rows_per_denoise_step': dedup_rows, 'unet_rows_per_denoise_step_full': 2 * (hi - lo),
                'rows_note': 'rank 0: its null-pass rows + the mean number of conditional rows kept per denoise step',
                'note': 'NOT the headline (`value` computes all 2B rows): opt-in cfg.Unet.dedup_dropped_rows — rows of the '
                        'conditional pass whose class was dropped (p = 0.5, CFG:404,415-425) equal their null-pass rows and '
                        'are not computed; the keep mask stays on the device (row subsets of include/dmhomo_hip.h) inside the '
                        'captured step; bitwise identical samples (tests/test_gpu_dedup.py)'}}
        if phases is not None:
            res['phases'] = phases
        # the measured error of this process's conv arithmetic on the canonical shape (fp64 host reference), and — beside the
        # headline, from a fresh child process — what the exact-fp32 kernels deliver on this box, with their error
        own = 'f16x3' if os.environ.get('DMH_CONV3_VARIANT', '9') == '9' else f"DMH_CONV3_VARIANT={os.environ['DMH_CONV3_VARIANT']}"
        if args.full:
            try:
                res['config']['measured_rel_error'] = {own: conv_error(args.image_size, device)}
            except Exception as e:
                res['config']['measured_rel_error'] = {'error': f'{type(e).__name__}: {str(e)[:160]}'}
            res['config']['measured_rel_error_note'] = ('max |y - y64| / max |y64| of one row of the canonical weight-standardised '
                                                        '3x3 conv 64->64 at image_size^2 on N(0,1) input against an fp64 host '
                                                        'convolution')
        if not args.no_variants and world == 1 and own == 'f16x3':
            torch.cuda.synchronize()
            ex = exact_fp32_variant(args)
            res['variants']['exact_fp32'] = ex
            if ex.get('value'):
                ex['speedup_vs_value'] = ex['value'] / (images / elapsed)
            if isinstance(ex.get('measured_rel_error'), dict):
                res['config']['measured_rel_error']['exact_fp32'] = next(iter(ex['measured_rel_error'].values()), None)
        if log:
            args.measure_traffic = (world == 1 and not args.no_traffic and
                                    (args.dim, args.image_size, args.bs) == (64, 128, 25))   # (the committed figure's workload)
            res['roofline'] = roofline(log, args)
        if not args.no_cpu_baseline:         # rank 0's host cores, whatever N is (the other ranks wait at the barrier)
            big = args.dim * args.image_size > 64 * 128
            torch.cuda.synchronize()
            res['cpu_baseline'] = cpu_baseline(args.dim, args.image_size, seconds=4.0 if big else 12.0,
                                               slice_bs=0 if big else args.bs,
                                               conds=(rgb_flow.cpu(), flow.cpu(), mask.cpu()))
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, records):
    """--dump-outputs: the gathered records of the last timed step, as a caller of step() receives them, for comparing two
    builds output for output.  DIR/imgs.npy = the uint8 image pairs as float32 (N, 6, S, S), DIR/homos.npy = the float64
    homographies (N, 3, 3).  When the images exceed the 64 MB budget, a fixed sample of whole rows (numpy seed 0, sorted) is
    written instead, and DIR/imgs_rows.npy (float64) holds the row indices it took."""
    import numpy as np
    imgs, homos = records
    imgs = imgs.cpu().numpy().astype(np.float32)
    homos = homos.cpu().numpy().astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    n = imgs.shape[0]
    fit = max(1, (DUMP_LIMIT_BYTES - homos.nbytes - 8 * n) // max(imgs[:1].nbytes, 1))
    if fit < n:
        rows = np.sort(np.random.default_rng(0).choice(n, size=fit, replace=False))
        imgs = imgs[rows]
        np.save(os.path.join(out_dir, 'imgs_rows.npy'), rows.astype(np.float64))
    elif os.path.exists(os.path.join(out_dir, 'imgs_rows.npy')):
        os.remove(os.path.join(out_dir, 'imgs_rows.npy'))     # (left by an earlier, larger run into the same DIR)
    np.save(os.path.join(out_dir, 'imgs.npy'), imgs)
    np.save(os.path.join(out_dir, 'homos.npy'), homos)


def measure_traffic(timeout=240):
    """HBM bytes per stride-1 3x3 launch, measured NOW: two child runs of this script under `rocprofv3 --pmc` (FETCH_SIZE, then
    WRITE_SIZE: separate passes, as MI355X_MICROARCH.md prescribes; --kernel-trace only), on the workload tools/profile_round6.sh
    uses for the committed figure (one eager batched step at s_step = 2: same launches, same shapes).  Units / corrections as
    tools/pmc_traffic.py: counters in KiB, FETCH_SIZE doubled on gfx950.  -> (bytes per launch, launches) or raises."""
    import csv
    import glob
    import shutil
    import tempfile
    if shutil.which('rocprofv3') is None:
        raise RuntimeError('rocprofv3 not on PATH')
    kernel = 'conv_f16x3_kernel<3, 3, 1, 0'
    out = {}
    env = child_env(TMPDIR='/tmp')       # (no RANK / MASTER_*: the child is a one-rank job of its own)
    for counter in ('FETCH_SIZE', 'WRITE_SIZE'):
        d = tempfile.mkdtemp(prefix='dmh_pmc_', dir='/tmp')
        try:
            cmd = ['rocprofv3', '--kernel-trace', '--pmc', counter, '--output-format', 'csv', '-d', d, '-o', 't', '--',
                   sys.executable, os.path.abspath(__file__), '--steps', '1', '--warmup', '1', '--s_step', '2', '--cfg-mode',
                   'batched', '--no-variants', '--no-cpu-baseline', '--no-roofline', '--no-graph', '--no-phases']
            # (rocprofv3 leads its own session: a timeout kills the profiler AND the python under it — run_child)
            rc, _, err = run_child(cmd, timeout, env=env, cwd='/tmp')
            files = glob.glob(d + '/**/*counter_collection.csv', recursive=True)
            if rc != 0 or not files:
                raise RuntimeError(f'rocprofv3 --pmc {counter} failed (rc {rc}): {err[-200:]}')
            vals = [float(row['Counter_Value']) for row in csv.DictReader(open(files[0]))
                    if row['Counter_Name'] == counter and kernel in row['Kernel_Name']]
            if not vals:
                raise RuntimeError(f'no {counter} rows for {kernel}')
            out[counter] = (sum(vals) / len(vals), len(vals))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return 2 * out['FETCH_SIZE'][0] * 1024 + out['WRITE_SIZE'][0] * 1024, out['FETCH_SIZE'][1]


def newest_committed_traffic():
    """profiles/rNN_pmc_traffic.json with the highest NN (what tools/check_traffic.py resolves for a directory argument)"""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_pmc_traffic.json')))
    return files[-1] if files else None


def roofline(log, args):
    """the `roofline` object of the JSON line from the HIP-event log of one batched step (see the module docstring)."""
    fl3 = ms3 = n3 = by3 = 0.0      # stride-1 3x3 launches (the dominant kernel): 3 executed fp16 FLOPs per algorithmic one
    flc = msc = nc = 0.0            # of those, the canonical 64->64 @ image_size^2 with the GN+SiLU prologue
    flu = msu = 0.0                 # sub-pixel Upsample convs (16 of every 36 taps executed): reported, not in `frac`
    flq = msq = nq = 0.0            # the same shape WITHOUT the prologue (block 1 of a ResnetBlock): reported beside it
    for e0, e1, k, stride, B, ho, wo, cin, cout, ups, pro in log:
        if k != 3:
            continue
        ms = e0.elapsed_time(e1)
        fl = 2.0 * 9 * cin * cout * ho * wo * B
        if ups == 2:
            flu, msu = flu + fl, msu + ms
            continue
        fl3, ms3, n3 = fl3 + fl, ms3 + ms, n3 + 1
        by3 += 4.0 * B * ho * wo * (cin + cout) + 4 * (9 * cin * cout + 3 * cout) + 8 * B * cout     # SURVEY 8d, per launch
        if (cin, cout, ho) == (64, 64, args.image_size):
            if pro:
                flc, msc, nc = flc + fl, msc + ms, nc + 1
            else:
                flq, msq, nq = flq + fl, msq + ms, nq + 1
    if not ms3:                      # (a configuration without a stride-1 3x3 launch in the log)
        return {'bound': 'mfma', 'achieved': None, 'peak': PEAK_FP16_MFMA_TFLOPS / F16X3_TERMS, 'unit': 'TFLOP/s',
                'frac': None, 'traffic': None, 'note': 'no stride-1 3x3 conv launch was logged'}
    ach = fl3 / (ms3 * 1e-3) / 1e12
    peak = PEAK_FP16_MFMA_TFLOPS / F16X3_TERMS
    rows = 2 * args.bs
    canon_bytes = 4.0 * rows * args.image_size ** 2 * (64 + 64) + 4 * (9 * 64 * 64 + 3 * 64) + 8 * rows * 64
    canon_us = msc / max(nc, 1) * 1e3
    traffic, traffic_src = None, None
    tpath = newest_committed_traffic()
    if tpath:                           # FETCH_SIZE / WRITE_SIZE passes of rocprofv3 (tools/profile_round6.sh)
        with open(tpath) as f:
            traffic = json.load(f).get('hbm_bytes_per_launch')
        traffic_src = 'profiles/' + os.path.basename(tpath)
    traffic_note = ('HBM bytes per launch (rocprofv3 PMC FETCH_SIZE x2 + WRITE_SIZE, separate passes, averaged over the 3x3 '
                    'launches of a batched step); from the committed profile, not measured by this run')
    committed = traffic
    if getattr(args, 'measure_traffic', False):
        # measured by THIS run (two child processes under rocprofv3 --pmc, after the timed region); the committed figure stays
        # beside it, with the deviation — a traffic regression now shows in the driver's own line
        try:
            t0 = time.perf_counter()
            traffic, nl = measure_traffic()
            traffic_src = 'measured by this run: 2 x rocprofv3 --pmc child passes of bench.py (batched, eager, s_step 2)'
            traffic_note = (f'HBM bytes per launch: FETCH_SIZE x2 + WRITE_SIZE (separate passes), averaged over {nl} stride-1 3x3 '
                            f'launches; {time.perf_counter() - t0:.0f} s for the two passes')
        except Exception as e:                       # (no profiler on the box, a refused counter, a timeout): quote the file
            traffic_note += f' [live measurement failed: {str(e)[:160]}]'
    return {
        'kernel': 'conv_f16x3_kernel<3,3,1,0,...> (stride-1 3x3 conv, implicit GEMM, 3 x v_mfma_f32_16x16x32_f16 per fp32 '
                  'product block, fp32 accumulate)',
        'bound': 'mfma', 'achieved': ach, 'peak': peak, 'unit': 'TFLOP/s', 'frac': ach / peak,
        'peak_note': 'algorithmic TFLOP/s; peak = 2500 dense fp16 MFMA TFLOP/s / 3 executed FLOPs per algorithmic FLOP',
        'executed': {'pipe': 'fp16 MFMA', 'TFLOP/s': ach * F16X3_TERMS, 'peak': PEAK_FP16_MFMA_TFLOPS,
                     'frac': ach * F16X3_TERMS / PEAK_FP16_MFMA_TFLOPS},
        'vs_fp32_mfma_peak': ach / PEAK_FP32_MFMA_TFLOPS,
        'traffic': traffic, 'traffic_source': traffic_src, 'traffic_note': traffic_note,
        'traffic_committed': committed,
        'traffic_vs_committed': (traffic / committed) if (traffic and committed) else None,
        'algorithmic_bytes_per_launch_avg': by3 / max(n3, 1),
        'traffic_vs_algorithmic_note': 'the canonical launch alone moves 1.02x its algorithmic bytes (profiles/r05_pmc_canonical.json); the '
                                       'average over ALL stride-1 3x3 launches sits ~1.24x above the SURVEY 8d sum because of the <= 32^2 levels. '
                                       'Since round 6 the cout tiles of one pixel tile run on the SAME XCD there (DMH_CONV_XCD_DEEP=32): a launch '
                                       'fetches its input once per XCD instead of once per cout tile, and every XCD streams the whole weight image '
                                       '(9.4 MB at 512->512@16^2 through a 4 MB L2: re-fetched from the Infinity Cache) — FETCH_SIZE of those '
                                       'launches went UP by a third, of 256->256@32^2 down by a quarter, +2 % on this average, and the step got '
                                       '0.24-0.29 % FASTER (tight A/B on three boxes, profiles/r06_ab_xcd.txt): these launches move < 1 TB/s, '
                                       'their bytes cost no time (DESIGN 3.1); DMH_CONV_XCD_DEEP=0 restores 242 MB',
        'measured_in': 'one extra untimed step, cfg_mode=batched, HIP events on the launch stream',
        'launches': int(n3), 'avg_launch_us': ms3 / max(n3, 1) * 1e3,
        'algorithmic_flop_per_launch': fl3 / max(n3, 1),
        'same_shape_without_prologue': {'launches': int(nq), 'avg_launch_us': (msq / nq * 1e3) if nq else None},
        'canonical_64to64_128sq': {'launches': int(nc), 'avg_launch_us': canon_us,
                                   'what': 'conv3x3 64->64 at image_size^2 WITH the fused GroupNorm+SiLU prologue (block 2 of '
                                           'a ResnetBlock) and the GroupNorm partials in the epilogue',
                                   'TFLOP/s': (flc / (msc * 1e-3) / 1e12) if msc else None,
                                   'algorithmic_bytes_per_launch': canon_bytes,
                                   'GB/s_algorithmic': (canon_bytes / (canon_us * 1e-6) / 1e9) if msc else None},
        'hbm_frac_canonical': (canon_bytes / (canon_us * 1e-6) / 1e12 / PEAK_HBM_TBS) if msc else None,
        'subpixel_upsample_convs': {'TFLOP/s_algorithmic': (flu / (msu * 1e-3) / 1e12) if msu else None,
                                    'note': 'Upsample+conv3x3 in sub-pixel form executes 16 of every 36 taps; kept out of frac'},
    }


if __name__ == '__main__':
    main()
