"""Shared by tests/test_threshold_host.py and tests/test_gpu_threshold.py: the case list of the row-quantile selector
(dmh_row_quantile_abs) and the float64 references of dynamic thresholding — the quantile (numpy sort of the fp32 |x| taken as
float64; rank, k, frac as include/dmhomo_hip.h states them) and one denoise step with a threshold per row (the ``_statement``
of tests/test_gpu_solver.py restated with the threshold, a DDIM update added).  No GPU, no dmhomo_amd import."""
import math

import numpy as np
import torch

KINDS = ('normal', 'equal', 'zeros', 'two', 'lowbits', 'range', 'signs', 'inf', 'nan')
SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 1536, 9600)       # 1536 = 6 * 16^2, 9600 = 6 * 40^2
BIG = (98304, 25)                                                   # the workload's row (6 * 128^2) at its batch, once
HUGE = (393216, 2)                                                  # 6 * 256^2
P_WORKLOAD = 0.995


def rank_of(p, n):
    """(k, frac): rank = p * (n - 1) in double, k = floor(rank), frac = float32(rank - k)"""
    rank = float(p) * (n - 1)
    k = int(math.floor(rank))
    frac = float(np.float32(rank - k))
    if frac >= 1.:
        k, frac = k + 1, 0.
    return k, frac


def percentiles(n):
    """k = 0 with frac != 0 (n > 1), the median, 0.9, the workload's, the maximum, and 0.25 (an integral rank where n = 4j + 1,
    as 0.5 gives one for every odd n and 1.0 for every n)"""
    return (0.5 / n, 0.25, 0.5, 0.9, P_WORKLOAD, 1.0)


def make_row(kind, n, k, seed):
    """one row of n fp32 values of the given kind; k: the rank the case selects (the 'two' kind meets there)"""
    gen = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n, generator=gen)
    if kind == 'normal':
        return torch.randn(n, generator=gen) * 1.5
    if kind == 'equal':
        return torch.full((n,), -0.7)
    if kind == 'zeros':                                       # every key is 0: +0.0 and -0.0 mixed
        x = torch.zeros(n)
        x[1::2] = -0.0
        return x
    if kind == 'two':                                         # sorted: k + 1 values 0.25, then 0.75: v[k] != v[k+1] exactly here
        x = torch.full((n,), 0.75)
        x[:k + 1] = 0.25
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1., 1.)
        return (x * sign)[perm]
    if kind == 'lowbits':                                     # 1.0 + j ulps, j < 1024: only the last radix digit differs
        bits = 0x3f800000 + torch.randint(0, 1024, (n,), generator=gen, dtype=torch.int32)
        return bits.view(torch.float32)
    if kind == 'range':                                       # 1e-45 (denormals; some round to 0) .. 1e30 in one row
        e = torch.rand(n, generator=gen, dtype=torch.float64) * 75. - 45.
        return (10. ** e).float() * torch.where(torch.rand(n, generator=gen) < 0.5, -1., 1.)
    if kind == 'signs':                                       # magnitudes 1 .. n, signs alternating
        x = torch.arange(1, n + 1, dtype=torch.float32) * 0.37
        x[::2] = -x[::2]
        return x[perm]
    x = torch.randn(n, generator=gen) * 1.5
    x[int(perm[0])] = float('inf') if kind == 'inf' else float('nan')
    return x


def selector_cases():
    """[(name, x (B, n) fp32, p, the rows' kinds)]: every size x percentile at B = 1 and B = 3, the kinds rotating so that each
    row of a batch is of another kind and every kind meets every size; then the two large ones"""
    cases, c = [], 0
    for n in SIZES:
        for p in percentiles(n):
            k, _ = rank_of(p, n)
            for B in (1, 3):
                kinds = [KINDS[(c + 4 * j) % len(KINDS)] for j in range(B)]
                x = torch.stack([make_row(kd, n, k, 1000 * c + j) for j, kd in enumerate(kinds)])
                cases.append((f'n{n}-p{p:.6g}-' + '+'.join(kinds), x, p, tuple(kinds)))
                c += 1
    n, B = BIG
    k, _ = rank_of(P_WORKLOAD, n)
    kinds = [KINDS[j % len(KINDS)] for j in range(B)]
    cases.append((f'n{n}-B{B}', torch.stack([make_row(kd, n, k, 77 + j) for j, kd in enumerate(kinds)]), P_WORKLOAD,
                  tuple(kinds)))
    n, B = HUGE
    k, _ = rank_of(P_WORKLOAD, n)
    kinds = ('normal', 'lowbits')
    cases.append((f'n{n}-B{B}', torch.stack([make_row(kd, n, k, 99 + j) for j, kd in enumerate(kinds)]), P_WORKLOAD, kinds))
    return cases


def quantile_ref(row, p):
    """float64 reference for one fp32 row without NaN -> (k, frac, a, b, q): a = v[k], b = v[k+1] (a where frac == 0: never
    looked at), q = a + (b - a) * frac, exact in float64 up to one rounding"""
    v = np.sort(np.abs(row.detach().cpu().numpy().astype(np.float32)).astype(np.float64))
    assert not np.isnan(v).any()
    k, frac = rank_of(p, v.shape[0])
    a = float(v[k])
    if frac == 0.:
        return k, frac, a, a, a
    b = float(v[k + 1])
    q = b if (math.isinf(b) or a == b) else a + (b - a) * frac
    return k, frac, a, b, q


def threshold_ref(x0_raw, p):
    """per row of a (B, ...) tensor: (raw quantile q, thr = max(1, q)) as float64 tensors"""
    q = torch.tensor([quantile_ref(r.reshape(-1), p)[4] for r in x0_raw], dtype=torch.float64)
    return q, q.clamp(min=1.)


def apply_threshold(x0_raw, thr):
    """float64: clamp(x0_raw, -thr, thr) / thr per row; a NaN thr makes its row NaN"""
    t = thr.double().reshape(-1, *([1] * (x0_raw.dim() - 1)))
    x = x0_raw.double()
    out = torch.minimum(torch.maximum(x, -t), t) / t
    return torch.where(torch.isnan(t), torch.full_like(x, float('nan')), out)


def statement(step, mc, mn, keep, x, noise, hist, thr):
    """float64: guided blend (CFG:410, a dropped row's logits are the null logits), objective branch, the threshold where the
    entry clips, pred_noise re-derived, update (mode 0 DDIM, 1 last, 3 multistep) -> (img, x_start)"""
    f = lambda name: float(getattr(step, name))              # (the fp32 values the kernel reads)
    mc, x = mc.double(), x.double()
    if mn is not None:
        nl = mn.double()
        mo = mc if keep is None else torch.where(keep.bool().reshape(-1, 1, 1, 1), mc, nl)
        mo = nl + (mo - nl) * f('cond_scale')
    else:
        mo = mc
    if step.objective == 0:
        x0 = f('sqrt_recip_ac') * x - f('sqrt_recipm1_ac') * mo
    elif step.objective == 1:
        x0 = mo
    else:
        x0 = f('sqrt_ac') * x - f('sqrt_1m_ac') * mo
    if step.clip:
        x0 = apply_threshold(x0, thr)
    pn = mo if step.objective == 0 else (f('sqrt_recip_ac') * x - x0) / f('sqrt_recipm1_ac')
    if step.mode == 1:
        return x0, x0
    if step.mode == 0:
        return x0 * f('c0') + f('c1') * pn + f('c2') * noise.double(), x0
    o = f('c0') * x0 + f('c1') * x
    if step.c2 != 0.:
        o = o + f('c2') * hist.double()
    return o, x0
