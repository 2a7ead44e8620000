"""Shared by tests/test_guidance_host.py and tests/test_gpu_guidance.py: the case list of the guidance-rescale factor
(dmh_guidance_factor) and the float64 references of rescaled classifier-free guidance (Lin et al. 2024, 3.4) as
include/dmhomo_hip.h defines it.  Per row b of n values:

    mo_c = cond, or null where keep[b] == 0;   cfg = null + (mo_c - null) * cond_scale   (fp32, op by op, no contraction)
    ratio = std(mo_c) / std(cfg) (population; float64 here), 1 where std(cfg) == 0;   g[b] = 1 + phi * (ratio - 1)

and one denoise step on cfg * g[b] (the ``statement`` of tests/threshold_cases.py extended by the factor, the threshold
optional).  No GPU, no dmhomo_amd import."""
import numpy as np
import torch

import threshold_cases as TC

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 1536, 9600)     # 1536 = 6 * 16^2, 9600 = 6 * 40^2
BATCHES = (1, 3)
BIG = (98304, 25)                                                          # the workload's row (6 * 128^2) at its batch, once
RAGGED_CANDIDATES = tuple(range(4097, 40000, 1231))                        # odd and even sizes above one workgroup's share
KINDS = ('normal', 'keep', 'equal', 'keep0', 'pow2', 'const', 'huge', 'nan', 'inf', 'phi1')
CS, PHI = 3., 0.7
GATE = 2. ** -23      # of g: one fp32 ulp.  g is an fp64 value rounded to fp32 ONCE (2^-24 of it); the fp64 moments behind it
#                       carry a relative error of about n * 2^-53 * (1 + mean^2 / var) <= 1e-9 for every case here (the offset
#                       case: 98304 * 1.1e-16 * 1e6 * a few), which can move that one rounding by at most one ulp


def ragged_size(splits_of, B):
    """the first candidate n for which a row of a B-row launch is cut into >= 2 splits with a shorter last one; splits_of(B,
    n) is the library's dmh_guidance_splits"""
    for n in RAGGED_CANDIDATES:
        s = splits_of(B, n)
        if s >= 2 and n % (4 * s) != 0:                      # (a split is a multiple of 4 elements long)
            return n, s
    raise AssertionError('no candidate size is split raggedly')


def blend32(cond, null, keep, cs):
    """(mo_c, cfg) of (B, n) fp32 logits, in fp32 exactly as guided_logit evaluates them"""
    cond, null = cond.float(), null.float()
    mo = cond if keep is None else torch.where(keep.bool().reshape(-1, 1), cond, null)
    cfg = null + (mo - null) * torch.tensor(cs, dtype=torch.float32)
    return mo, cfg


def factor_ref(cond, null, keep, cs, phi):
    """float64 g (B,): the blend in fp32, two-pass moments in float64; a row that holds a NaN or an infinity answers NaN"""
    B = cond.shape[0]
    mo, cfg = blend32(cond.reshape(B, -1), null.reshape(B, -1), keep, cs)
    vc = mo.double().var(dim=1, unbiased=False)
    vg = cfg.double().var(dim=1, unbiased=False)
    ratio = torch.where(vg == 0., torch.ones_like(vg), vc.sqrt() / vg.sqrt())
    g = 1. + float(np.float32(phi)) * (ratio - 1.)
    bad = ~(torch.isfinite(mo).all(dim=1) & torch.isfinite(cfg).all(dim=1))
    return torch.where(bad, torch.full_like(g, float('nan')), g)


def _randn(shape, gen, scale=1.5):
    return torch.randn(shape, generator=gen) * scale


def make_case(kind, B, n, seed):
    """-> dict(cond, null (B, n) fp32, keep (B,) uint8 or None, cs, phi, expect): expect 'ref' (against factor_ref within
    GATE), a float (that value exactly in every row), or ('nan', row) (that row NaN, the others bitwise those of ``clean``)"""
    gen = torch.Generator().manual_seed(seed)
    cond, null = _randn((B, n), gen), _randn((B, n), gen)
    case = dict(kind=kind, cond=cond, null=null, keep=None, cs=CS, phi=PHI, expect='ref')
    if kind == 'keep':                                        # rows mixed: the middle row of three is dropped
        case['keep'] = torch.tensor([1, 0, 1][:B] if B > 1 else [1], dtype=torch.uint8)
    elif kind == 'equal':                                     # cond bitwise equal to null
        case.update(cond=null.clone(), expect=1.)
    elif kind == 'keep0':                                     # every row dropped: cond is never read (NaN would show)
        case.update(cond=torch.full((B, n), float('nan')), keep=torch.zeros(B, dtype=torch.uint8), expect=1.)
    elif kind == 'pow2':                                      # cfg = 4 * cond exactly: ratio 1/4, g = 1 + 0.5 * (-0.75)
        case.update(null=torch.zeros((B, n)), cs=4., phi=0.5, expect=0.625 if n > 1 else 1.)
    elif kind == 'const':                                     # constant rows: nothing to rescale
        case.update(cond=torch.full((B, n), 0.3) * torch.arange(1, B + 1).reshape(B, 1),
                    null=torch.full((B, n), -1.7) * torch.arange(1, B + 1).reshape(B, 1), expect=1.)
    elif kind == 'huge':                                      # squares overflow fp32, not fp64
        case.update(cond=cond * 1e18, null=null * 0.5e18)
    elif kind in ('nan', 'inf'):                              # one broken row between finite rows (the only row at B = 1)
        row, col = B // 2, int(torch.randint(0, n, (1,), generator=gen))
        clean = dict(case)
        cond = cond.clone()
        cond[row, col] = float('nan') if kind == 'nan' else float('-inf')
        case.update(cond=cond, expect=('nan', row), clean=clean)
    elif kind == 'phi1':                                      # phi = 1: std(cfg * g) == std(cond)
        case['phi'] = 1.
    elif kind == 'offset':                                    # |mean| / std = 1e3: a one-pass fp32 E[x^2] - mean^2 loses it
        case.update(cond=cond / 1.5 + 1000., null=null / 1.5 + 1000.)
    else:
        assert kind == 'normal', kind
    return case


def factor_cases(ragged=()):
    """[(name, case)]: every kind at every size and batch, the ragged multi-split sizes the caller chose with ragged_size,
    then the workload's shape: normal with a keep mask, and the offset rows (kind (e) of the issue, at n = 98304 only)"""
    out, c = [], 0
    for n in tuple(SIZES) + tuple(ragged):
        for B in BATCHES:
            for kind in KINDS:
                out.append((f'{kind}-n{n}-B{B}', make_case(kind, B, n, 100 + c)))
                c += 1
    n, B = BIG
    big = make_case('normal', B, n, 7)
    big['keep'] = (torch.arange(B) % 3 != 1).to(torch.uint8)
    out.append((f'normal+keep-n{n}-B{B}', big))
    for B in BATCHES:
        out.append((f'offset-n{n}-B{B}', make_case('offset', B, n, 8 + B)))
    return out


def one_pass_fp32_variance_ratio(cond, null, keep, cs):
    """what the issue warns of: var = E[x^2] - mean^2 accumulated in fp32 -> var(mo_c) / var(cfg) per row"""
    mo, cfg = blend32(cond, null, keep, cs)
    out = []
    for x in (mo, cfg):
        n = x.shape[1]
        s1, s2 = x.sum(dim=1, dtype=torch.float32), (x * x).sum(dim=1, dtype=torch.float32)
        out.append(s2 / n - (s1 / n) * (s1 / n))
    return out[0] / out[1]


def statement(step, mc, mn, keep, x, noise, hist, thr, gfac):
    """float64: guided blend (CFG:410, a dropped row's logits are the null logits) times the row's factor, objective branch,
    the static clamp (thr None) or the threshold where the entry clips, pred_noise re-derived, update (mode 0 DDIM, 1 last, 3
    multistep) -> (img, x_start, raw x_start before any clamp)"""
    f = lambda name: float(getattr(step, name))              # (the fp32 values the kernel reads)
    mc, x = mc.double(), x.double()
    rows = (-1,) + (1,) * (x.dim() - 1)
    if mn is not None:
        nl = mn.double()
        mo = mc if keep is None else torch.where(keep.bool().reshape(rows), mc, nl)
        mo = nl + (mo - nl) * f('cond_scale')
    else:
        mo = mc
    mo = mo * gfac.double().reshape(rows)
    if step.objective == 0:
        x0 = f('sqrt_recip_ac') * x - f('sqrt_recipm1_ac') * mo
    elif step.objective == 1:
        x0 = mo
    else:
        x0 = f('sqrt_ac') * x - f('sqrt_1m_ac') * mo
    raw = x0
    if step.clip:
        x0 = TC.apply_threshold(x0, torch.ones(x.shape[0], dtype=torch.float64) if thr is None else thr)
    pn = mo if step.objective == 0 else (f('sqrt_recip_ac') * x - x0) / f('sqrt_recipm1_ac')
    if step.mode == 1:
        return x0, x0, raw
    if step.mode == 0:
        return x0 * f('c0') + f('c1') * pn + f('c2') * noise.double(), x0, raw
    o = f('c0') * x0 + f('c1') * x
    if step.c2 != 0.:
        o = o + f('c2') * hist.double()
    return o, x0, raw
