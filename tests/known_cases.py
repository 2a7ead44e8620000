"""The statements behind sampling around known pixels (cfg.GaussianDiffusion.sample_known; include/dmhomo_hip_known.h has the
definition), on the CPU: the fp32 blend restated with torch ops in the kernel's order and the select over it — what
dmh_known_blend must give bit for bit —, the score of dmh_known_error in exact rational arithmetic, the stay coefficients of
known_resample in float64 from the closed form, a float64 loop that takes recorded network outputs, and the case table of
the kernel tests."""
from fractions import Fraction
import math

import numpy as np
import torch

import guidance_cases as GC

F32 = torch.float32
PER_ROW = (1, 3, 4, 5, 24, 210, 1536)      # below a vector, straddling head and tail, odd, 6 * 16 * 16
BATCHES = (1, 3)
OFFSETS = (0, 1, 2, 3)                     # floats past a 16-byte boundary at which the output starts
FORMS = ('cond', 'cond+null', 'cond+null+keep')
MASKS = ('zero', 'all', 'source', 'target', 'random', 'one')
CS = 3.


# ------------------------------------------------------------------------------------------ the statement
def blend32(cond, null, keep, cs):
    """the logits a step works on, in fp32 exactly as guided_logit evaluates them, rows flat or not: cond, or null + (c - null)
    * cs with c = null in the rows where keep == 0"""
    cond = cond.to(F32)
    if null is None:
        return cond
    null = null.to(F32)
    rows = (-1,) + (1,) * (cond.dim() - 1)
    c = cond if keep is None else torch.where(keep.bool().reshape(rows), cond, null)
    return null + (c - null) * torch.tensor(cs, dtype=F32)


def select(x, K, mask):
    """K on the kept elements (mask != 0), x elsewhere: no arithmetic joins the two"""
    return torch.where(mask.reshape(x.shape) != 0, K.to(x.dtype), x)


def blend_ref(cond, null, keep, cs, K, mask):
    return select(blend32(cond, null, keep, cs), K, mask)


def error_ref(x, K, mask):
    """per row, sum m * (x - K)^2 / max(1, sum m) over the kept elements, m = (mask != 0): x and K are taken as given (fp32
    or float64 values), the arithmetic is exact (rationals), the result rounded to float64 once -> ((B,) float64, kept count
    per row)"""
    B = x.shape[0]
    x, K, m = x.reshape(B, -1).double(), K.reshape(B, -1).double(), mask.reshape(B, -1) != 0
    out, cnt = [], []
    for b in range(B):
        xs, ks = x[b][m[b]].tolist(), K[b][m[b]].tolist()
        total = sum(((Fraction(a) - Fraction(k)) ** 2 for a, k in zip(xs, ks)), Fraction(0))
        out.append(float(total / max(1, len(xs))))
        cnt.append(len(xs))
    return torch.tensor(out, dtype=torch.float64), cnt


def stay_ref(abar, t, t_next, eta):
    """(c0, c1, c2) of the stay entry t -> t in front of the entry t -> t_next (t_next < 0: the entry that returns x_0), float64,
    from the closed form: a = abar[t], a' = abar[t_next] or 1, sigma^2 = eta^2 (1 - a / a') (1 - a') / (1 - a), c^2 = 1 - a' -
    sigma^2.  abar: float64 values of the fp32 buffer"""
    a = float(abar[t])
    a1 = 1. if t_next < 0 else float(abar[t_next])
    s2 = 0. if t_next < 0 else eta * eta * (1. - a / a1) * (1. - a1) / (1. - a)
    c_sq = max(1. - a1 - s2, 0.)
    return math.sqrt(a), math.sqrt(a / a1 * c_sq), math.sqrt(a / a1 * s2 + 1. - a / a1)


def ddim_ref(abar, t, t_next, eta):
    """(c0, c1, c2) of the DDIM entry t -> t_next itself, float64: sqrt(a'), c, sigma"""
    a, a1 = float(abar[t]), float(abar[t_next])
    s2 = eta * eta * (1. - a / a1) * (1. - a1) / (1. - a)
    return math.sqrt(a1), math.sqrt(max(1. - a1 - s2, 0.)), math.sqrt(s2)


def reference_loop(steps, nets, draws, K, mask, cs, correct=None):
    """the loop of sample_known in float64 on recorded network outputs and noise: the blend in fp32 as the kernels read it,
    ``correct(step, x)`` (photo guidance: float64) where given, the select, the step of guidance_cases.statement in float64 ->
    per entry (the logits before the overwrite, x_start, img).  K: the fp32 values 2 * known - 1."""
    cpu = lambda t: None if t is None else t.cpu()
    img, ni, out = draws[0].cpu().double(), 1, []
    hist = None
    ones = torch.ones(img.shape[0])
    for (time, step, _), (cond, null, keep) in zip(steps, nets):
        x = blend32(cpu(cond), cpu(null), cpu(keep), cs)
        x = x.double() if correct is None else correct(step, x)
        y = select(x, K.double(), mask)
        noise = None
        if step.mode == 0:
            noise, ni = draws[ni].cpu(), ni + 1
        img, x0, _ = GC.statement(step, y, None, None, img, noise, hist, None, ones)
        hist = x0
        out.append((x, x0, img))
    assert ni == len(draws)
    return out


# ------------------------------------------------------------------------------------------ the kernel cases
def make_mask(kind, B, n, gen):
    m = torch.zeros((B, n), dtype=torch.uint8)
    if kind == 'all':
        m[:] = 1
    elif kind == 'source':
        m[:, :n // 2] = 1
    elif kind == 'target':
        m[:, n // 2:] = 1
    elif kind == 'random':
        m = (torch.rand((B, n), generator=gen) < 0.5).to(torch.uint8) * 255       # (any nonzero byte keeps)
        m[m != 0] = torch.randint(1, 256, (int((m != 0).sum()),), generator=gen).to(torch.uint8)
    elif kind == 'one':
        m[B - 1, n - 1] = 7
    else:
        assert kind == 'zero'
    return m


def make_case(B, n, form, mask_kind, seed, nan_kept=True):
    """cond, null, keep (the row B // 2 dropped: its conditional logits are NaN, never to be read), K, mask; NaN logits under a
    kept element and under one that is not, where the row has both"""
    gen = torch.Generator().manual_seed(seed)
    cond = torch.randn((B, n), generator=gen) * 1.5
    null = torch.randn((B, n), generator=gen) * 1.5 if form != 'cond' else None
    keep = None
    mask = make_mask(mask_kind, B, n, gen)
    for b in range(B):
        kept, free = torch.nonzero(mask[b] != 0).flatten(), torch.nonzero(mask[b] == 0).flatten()
        if len(kept) and nan_kept:
            cond[b, kept[len(kept) // 2]] = float('nan')
        if len(free) > 1:
            cond[b, free[len(free) // 2]] = float('nan')
    if form == 'cond+null+keep':
        keep = torch.ones((B,), dtype=torch.uint8)
        keep[B // 2] = 0
        cond[B // 2] = float('nan')
    K = torch.rand((B, n), generator=gen) * 2. - 1.
    return {'B': B, 'n': n, 'cond': cond, 'null': null, 'keep': keep, 'K': K, 'mask': mask, 'form': form, 'mask_kind': mask_kind}


def cases(per_row=PER_ROW, batches=BATCHES, forms=FORMS, masks=MASKS):
    out, seed = [], 100
    for n in per_row:
        for B in batches:
            for form in forms:
                for mk in masks:
                    seed += 1
                    out.append((f'{form}-{mk}-{B}x{n}', make_case(B, n, form, mk, seed)))
    return out


def bytes_of(img01):
    """saveTrainPair's truncation (dmh_to_uint8): uint8(img * 255), fp32"""
    return (img01.to(F32) * torch.tensor(255., dtype=F32)).to(torch.uint8)


def all_bytes():
    """the 256 values k = n / 255 in fp32"""
    return torch.tensor(np.arange(256, dtype=np.float32) / np.float32(255.))
