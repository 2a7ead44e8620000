"""Shared by tests/test_apg_host.py and tests/test_gpu_apg.py: the case table of the adaptive-projected-guidance kernels
(dmh_apg_coef, dmh_apg_apply) and the float64 statement of APG (Sadat, Hilliges, Weber 2024, Algorithm 1) as
include/dmhomo_hip.h defines it.  Per row b of n values:

    c = cond, or null where keep[b] == 0;   d = c - null (fp32);   beta != 0: d <- run = d + beta * run_prev (fp32, op by op)
    Sdd = sum d^2, Sdc = sum d*c, Scc = sum c^2 (float64);   s = 1 if rho == 0 or Sdd == 0, else min(1, rho / sqrt(Sdd))
    p = 0 if Scc == 0, else Sdc / Scc;   A = 1 - (w - 1) * s * (1 - eta) * p,  Cc = (w - 1) * s;   guided = A * c + Cc * d

A row whose sums are not all finite answers A = Cc = NaN.  No GPU, no dmhomo_amd import (the library's modules are handed to
``check_einval`` by its callers)."""
import ctypes
import math

import numpy as np
import torch

import guidance_cases as GC

SIZES = GC.SIZES                                             # 1, 2, 3, 63 .. 1025, 1536, 9600
BATCHES = (1, 3)
BIG = (98304, 25)                                            # the workload's row (6 * 128^2) at its batch, once
KINDS = ('normal', 'keep', 'equal', 'czero', 'rho_bind', 'rho_loose', 'momentum', 'nan')
CS = 3.
# (floats past a 16-byte boundary of cond, null, run): the vector path, the vector path behind a scalar head, the word path
# twice (cond against null out of phase), and — cases with a running average only — run alone out of phase
PHASES = ((0, 0, 0), (1, 1, 1), (3, 2, 2), (0, 1, 1), (0, 0, 2))
ULPS = 2.    # gate of a coefficient, in fp32 ulps of the reference value: one for the single rounding of the fp64 value to fp32,
#              one for the fp64 sums behind it: their relative error is about n * 2^-53 (<= 1.1e-11 at n = 98304) where the terms
#              of a sum do not cancel — Sdd and Scc never do, Sdc under the condition ``cancellation`` checks (>= 1e-3: the error
#              stays below 1.1e-8 of Sdc, 0.1 ulp) — and A = 1 - X carries it times |X / A|, a factor below 10 in every case here


def ragged_size(splits_of, B):
    """the first candidate n for which a row of a B-row launch is cut into >= 2 splits with a shorter last one; splits_of(B, n)
    is the library's dmh_apg_splits"""
    return GC.ragged_size(splits_of, B)


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def update32(cond, null, keep, beta=0., run_prev=None):
    """(c, d) of (B, n) fp32 logits in fp32, op by op as the kernels evaluate them; with beta != 0, d is the new running average"""
    cond, null = cond.float(), null.float()
    c = cond if keep is None else torch.where(keep.bool().reshape(-1, *([1] * (cond.dim() - 1))), cond, null)
    d = c - null
    if beta != 0.:
        d = d + f32(beta) * run_prev
    return c, d


def sums(c, d):
    """float64 (Sdd, Sdc, Scc) per row"""
    B = c.shape[0]
    cd, dd = c.reshape(B, -1).double(), d.reshape(B, -1).double()
    return (dd * dd).sum(dim=1), (dd * cd).sum(dim=1), (cd * cd).sum(dim=1)


def cancellation(c, d):
    """|sum d*c| / sum |d*c| per row (1 where the denominator is 0): the condition the ulp gate assumes is >= 1e-3"""
    B = c.shape[0]
    prod = d.reshape(B, -1).double() * c.reshape(B, -1).double()
    den = prod.abs().sum(dim=1)
    return torch.where(den == 0., torch.ones_like(den), prod.sum(dim=1).abs() / den)


def coef_ref(c, d, cs, eta, rho):
    """float64 (B, 2): (A, Cc) from fp32 c and d; cs, eta, rho enter as the fp32 values the kernel receives -> also s and p"""
    w, eta, rho = (float(np.float32(v)) for v in (cs, eta, rho))
    sdd, sdc, scc = sums(c, d)
    one = torch.ones_like(sdd)
    s = one if rho == 0. else torch.where(sdd == 0., one, torch.minimum(one, rho / sdd.sqrt()))
    p = torch.where(scc == 0., torch.zeros_like(scc), sdc / scc)
    cc = (w - 1.) * s
    a = 1. - cc * (1. - eta) * p
    bad = ~(torch.isfinite(sdd) & torch.isfinite(sdc) & torch.isfinite(scc))
    nan = torch.full_like(a, float('nan'))
    return torch.stack([torch.where(bad, nan, a), torch.where(bad, nan, cc)], dim=1), s, p


def guided_ref(c, d, coef):
    """float64 guided logits from float64 coefficients (B, 2)"""
    rows = (-1,) + (1,) * (c.dim() - 1)
    return coef[:, 0].double().reshape(rows) * c.double() + coef[:, 1].double().reshape(rows) * d.double()


def guided32(c, d, coef):
    """what dmh_apg_apply must write, bit for bit: (A * c) + (Cc * d) in fp32, two products and one add"""
    rows = (-1,) + (1,) * (c.dim() - 1)
    return coef[:, 0].float().reshape(rows) * c + coef[:, 1].float().reshape(rows) * d


def ulps(got, ref):
    """|got - ref| in fp32 ulps of ref (float64 tensors in; NaN where either is NaN)"""
    spacing = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))
    return (got.double() - ref).abs() / spacing


def _randn(shape, gen, scale=1.5):
    return torch.randn(shape, generator=gen) * scale


def make_case(kind, B, n, seed):
    """-> dict(kind, calls [(cond, null)] (B, n) fp32 — three consecutive calls on one running average for 'momentum', else one —
    keep (B,) uint8 or None, cs, eta, rho, beta, nan_row)"""
    gen = torch.Generator().manual_seed(seed)
    calls = [(_randn((B, n), gen), _randn((B, n), gen)) for _ in range(3 if kind == 'momentum' else 1)]
    case = dict(kind=kind, calls=calls, keep=None, cs=CS, eta=0.25, rho=0., beta=0., nan_row=None)
    cond, null = calls[0]
    if kind == 'keep':                                        # rows mixed: the middle row of three is dropped
        case['keep'] = torch.tensor([1, 0, 1][:B] if B > 1 else [0], dtype=torch.uint8)
        if B == 1:                                            # (the dropped row's cond is never read: NaN would show)
            case['calls'] = [(torch.full((B, n), float('nan')), null)]
    elif kind == 'equal':                                     # cond bitwise equal to null: A == 1, Cc == w - 1, guided == c
        case['calls'] = [(null.clone(), null)]
    elif kind == 'czero':                                     # c == 0: nothing to project on, p = 0, A == 1
        case['calls'] = [(torch.zeros((B, n)), null)]
        case['rho'] = 0.5 * math.sqrt(n)                      # (|d| is about 1.5 sqrt(n): Cc is not trivial either)
    elif kind == 'rho_bind':                                  # |d| is about 2.1 sqrt(n): the cap binds
        case['rho'] = 1.0 * math.sqrt(n)
    elif kind == 'rho_loose':                                 # ... and does not
        case['rho'] = 10. * math.sqrt(n) + 10.
    elif kind == 'momentum':
        case.update(beta=-0.5, rho=2.0 * math.sqrt(n), eta=0.)
        if B > 1:
            case['keep'] = torch.tensor([1, 1, 0][:B], dtype=torch.uint8)
    elif kind == 'nan':                                       # one NaN in one row (the only row at B = 1)
        row, col = B // 2, int(torch.randint(0, n, (1,), generator=gen))
        dirty = cond.clone()
        dirty[row, col] = float('nan')
        case.update(calls=[(dirty, null)], clean=[(cond, null)], nan_row=row)
    else:
        assert kind == 'normal', kind
    return case


def cases(ragged=()):
    """[(name, case)]: every kind at every size and batch, the ragged multi-split sizes the caller chose with ragged_size (one per
    batch, each at its own batch), then the workload's row once: three calls with momentum, a cap and a keep mask"""
    out, c = [], 0
    for n in SIZES:
        for B in BATCHES:
            for kind in KINDS:
                out.append((f'{kind}-n{n}-B{B}', make_case(kind, B, n, 300 + c)))
                c += 1
    for B, n in zip(BATCHES, ragged):
        for kind in KINDS:
            out.append((f'{kind}-n{n}-B{B}', make_case(kind, B, n, 300 + c)))
            c += 1
    n, B = BIG
    big = make_case('momentum', B, n, 17)
    big['keep'] = (torch.arange(B) % 3 != 1).to(torch.uint8)
    out.append((f'momentum+keep-n{n}-B{B}', big))
    return out


def reference(case, which='calls'):
    """the float64 statement over the case's calls -> per call dict(c, d (fp32: d is the new running average with beta != 0),
    coef (B, 2) float64, s, p, cancel)"""
    out, run = [], None
    for cond, null in case[which]:
        if case['beta'] != 0. and run is None:
            run = torch.zeros_like(null)
        c, d = update32(cond, null, case['keep'], case['beta'], run)
        if case['beta'] != 0.:
            run = d
        coef, s, p = coef_ref(c, d, case['cs'], case['eta'], case['rho'])
        out.append(dict(c=c, d=d, coef=coef, s=s, p=p, cancel=cancellation(c, d)))
    return out


def check_einval(_lib, ops):
    """every DMH_EINVAL of dmh_apg_splits, dmh_apg_coef[_dev] and dmh_apg_apply: -1 with a message that names the entry point,
    before anything is launched (the pointers are host memory nobody reads) -> the number of refusals seen"""
    lib = _lib.lib()
    buf = ctypes.cast((ctypes.c_char * 256)(), ctypes.c_void_p)
    step = ctypes.byref(_lib.DmhStep(objective=1, clip=1, mode=ops.MODE_LAST, cond_scale=3.))
    seen = 0

    def refused(name, args, word):
        nonlocal seen
        assert getattr(lib, name)(*args, None) == -1, (name, args)
        msg = lib.dmh_last_error().decode()
        assert name + ':' in msg and word in msg, (name, word, msg)
        seen += 1
    for B, n in ((0, 4), (-1, 4), (1, 0), (1, 2 ** 31)):
        assert lib.dmh_apg_splits(B, n) == -1 and b'dmh_apg_splits:' in lib.dmh_last_error(), (B, n)
        seen += 1
    for name, s in (('dmh_apg_coef', step), ('dmh_apg_coef_dev', buf)):
        #       s  cond null keep  eta  rho beta  run   ws  coef B  n
        good = [s, buf, buf, None, 0.5, 0., 0., None, buf, buf, 2, 8]
        for i, word in ((0, 'null pointer'), (1, 'null pointer'), (8, 'null pointer'), (9, 'null pointer'), (2, 'model_null')):
            refused(name, good[:i] + [None] + good[i + 1:], word)
        refused(name, [s, buf, None, buf] + good[4:], 'keep needs model_null')
        for B, n, word in ((0, 8, 'B=0'), (-3, 8, 'B=-3'), (2, 0, 'n=0'), (2, -5, 'n=-5'), (2, 2 ** 31, '2^31')):
            refused(name, good[:10] + [B, n], word)
        for eta in (-0.1, 1.5, float('nan'), float('inf')):
            refused(name, good[:4] + [eta] + good[5:], 'eta')
        for rho in (-1., float('nan'), float('inf')):
            refused(name, good[:5] + [rho] + good[6:], 'rho')
        for beta in (-1., 1., 1.5, -2., float('nan'), float('inf')):
            refused(name, good[:6] + [beta, buf] + good[8:], 'beta')
        refused(name, good[:6] + [0., buf] + good[8:], 'run is given')          # a running average without momentum
        refused(name, good[:6] + [-0.5, None] + good[8:], 'run is NULL')        # momentum without one
    #       cond null keep  run  coef guided B  n
    other = ctypes.cast((ctypes.c_char * 256)(), ctypes.c_void_p)
    good = [buf, buf, None, None, buf, other, 2, 8]
    for i, word in ((0, 'null pointer'), (4, 'null pointer'), (5, 'null pointer'), (1, 'model_null')):
        refused('dmh_apg_apply', good[:i] + [None] + good[i + 1:], word)
    refused('dmh_apg_apply', [buf, None, buf] + good[3:], 'keep needs model_null')
    for B, n, word in ((0, 8, 'B=0'), (2, 0, 'n=0'), (2, 2 ** 31, '2^31')):
        refused('dmh_apg_apply', good[:6] + [B, n], word)
    far = ctypes.cast((ctypes.c_char * 256)(), ctypes.c_void_p)
    inside = ctypes.c_void_p(other.value + 32)                # 2 * 8 floats = 64 bytes: half a tensor in
    for args in ([other, buf, None, None, buf, other, 2, 8], [buf, other, None, None, buf, inside, 2, 8],
                 [buf, far, None, inside, buf, other, 2, 8]):
        refused('dmh_apg_apply', args, 'overlaps')
    return seen
