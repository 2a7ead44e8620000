"""The statement of guidance on the flow condition (``flow_guidance``; include/dmhomo_hip.h has the definition) in fp32 torch ops
on the CPU — what dmh_flow_guidance_shift must give bit for bit —, its float64 form, dmh_affine_rows_keep's statement, the case
table of the kernel tests and the argument checks of the two entries.  No GPU is used here."""
import ctypes
import itertools

import torch

SIZES = (1, 3, 4, 5, 255, 1536, 4099)                          # elements per row
BATCHES = (1, 3, 5)
PHASES = ((0, 0, 0), (1, 1, 1), (1, 2, 3), (0, 0, 2))           # floats off a 16-byte boundary: cond, null, uncond
BIG = (25, 98304)                                               # the workload: 25 samples of 6 x 128 x 128
WS = (1., -1., 0.5, 2.5)                                        # w = flow_guidance - 1


def shift32(cond, null, uncond, w, keep=None):
    """fp32, one rounding per operation: e = w * (b - u), b = null (case A) or cond (case B); -> (cond', null' or None).  Rows
    with keep == 0 keep their cond bits (the kernel neither reads nor writes them)."""
    w32 = torch.tensor(w, dtype=torch.float32)
    b = cond if null is None else null
    d = b - uncond
    e = w32 * d
    if null is None:
        assert keep is None
        return b + e, None
    new_cond = cond + e
    if keep is not None:
        rows = keep.bool().reshape((-1,) + (1,) * (cond.dim() - 1))
        new_cond = torch.where(rows, new_cond, cond)
        # (torch.where hands a NaN's payload on unchanged: the dropped rows compare bitwise)
    return new_cond, b + e


def shift64(cond, null, uncond, w, keep=None):
    """the same in float64 on the fp32 inputs (w as the fp32 value the kernel receives) -> (cond', null' or None, e)"""
    w64 = float(torch.tensor(w, dtype=torch.float32))
    c, u = cond.double(), uncond.double()
    b = c if null is None else null.double()
    e = w64 * (b - u)
    if null is None:
        return b + e, None, e
    new_cond = c + e
    if keep is not None:
        rows = keep.bool().reshape((-1,) + (1,) * (cond.dim() - 1))
        new_cond = torch.where(rows, new_cond, c)
    return new_cond, b + e, e


def affine_keep32(x, scale, shift, keep):
    """dmh_affine's expression (the product rounded, then the sum) on kept rows, +0.0 on dropped rows"""
    y = x * torch.tensor(scale, dtype=torch.float32) + torch.tensor(shift, dtype=torch.float32)
    rows = keep.bool().reshape((-1,) + (1,) * (x.dim() - 1))
    return torch.where(rows, y, torch.zeros_like(y))


def keeps_for(B):
    """the keep masks of a case with a null pass: None, mixed (at B == 1: the one row kept), all zero"""
    mixed = torch.tensor([1, 0, 1, 1, 0][:B], dtype=torch.uint8)
    return {'none': None, 'mixed': mixed, 'zero': torch.zeros(B, dtype=torch.uint8)}


def inputs(B, n, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn((B, n), generator=gen) * 1.5
    return r(), r(), r()


def cases():
    """[(name, dict(cond, null or None, uncond, keep or None, w))]: every size x batch, with and without a null pass, keep None /
    mixed / all zero; the rows of cond with keep == 0 are NaN (they were never computed)"""
    out = []
    for k, (n, B) in enumerate(itertools.product(SIZES, BATCHES)):
        cond, null, uncond = inputs(B, n, 100 + k)
        w = WS[k % len(WS)]
        out.append((f'n{n}-B{B}-caseB', dict(cond=cond, null=None, uncond=uncond, keep=None, w=w)))
        for kind, keep in keeps_for(B).items():
            c = cond.clone()
            if keep is not None:
                c[~keep.bool()] = float('nan')
            out.append((f'n{n}-B{B}-caseA-keep-{kind}', dict(cond=c, null=null, uncond=uncond, keep=keep, w=w)))
    return out


def check_einval(_lib):
    """every DMH_EINVAL of the two entries: -1 with a message that names the entry point, before anything is launched (the
    pointers are host memory nobody reads) -> the number of refusals seen"""
    lib = _lib.lib()
    mem = lambda: ctypes.cast((ctypes.c_char * 256)(), ctypes.c_void_p)
    a, b, c = mem(), mem(), mem()
    seen = 0

    def refused(name, args, word):
        nonlocal seen
        assert getattr(lib, name)(*args, None) == -1, (name, args)
        msg = lib.dmh_last_error().decode()
        assert name + ':' in msg and word in msg, (name, word, msg)
        seen += 1
    name = 'dmh_flow_guidance_shift'
    #       cond null uncond keep  w  B  n
    good = [a, b, c, None, 1., 2, 8]
    refused(name, [None] + good[1:], 'null pointer')
    refused(name, good[:2] + [None] + good[3:], 'null pointer')
    refused(name, [a, None, c, b, 1., 2, 8], 'keep needs model_null')
    for B, n, word in ((0, 8, 'B=0'), (-3, 8, 'B=-3'), (2, 0, 'n=0'), (2, -5, 'n=-5'), (2, 2 ** 31, '2^31')):
        refused(name, good[:5] + [B, n], word)
    for w in (float('nan'), float('inf'), float('-inf')):
        refused(name, good[:4] + [w] + good[5:], 'not finite')
    odd = ctypes.c_void_p(c.value + 2)
    refused(name, [a, b, odd, None, 1., 2, 8], '4-byte aligned')
    inside = ctypes.c_void_p(a.value + 32)                      # 2 * 8 floats = 64 bytes: half a tensor in
    refused(name, [a, b, a, None, 1., 2, 8], 'uncond overlaps')
    refused(name, [a, b, inside, None, 1., 2, 8], 'uncond overlaps')
    refused(name, [a, b, b, None, 1., 2, 8], 'uncond overlaps')
    refused(name, [a, None, inside, None, 1., 2, 8], 'uncond overlaps')
    refused(name, [a, inside, c, None, 1., 2, 8], 'model_cond overlaps model_null')
    name = 'dmh_affine_rows_keep'
    #       x  y  scale shift keep B  n
    good = [a, b, 2., -1., c, 2, 8]
    for i in (0, 1, 4):
        refused(name, good[:i] + [None] + good[i + 1:], 'null pointer')
    for B, n, word in ((0, 8, 'B=0'), (-3, 8, 'B=-3'), (2, 0, 'n=0'), (2, -5, 'n=-5'), (2, 2 ** 31, '2^31')):
        refused(name, good[:5] + [B, n], word)
    refused(name, [ctypes.c_void_p(a.value + 1)] + good[1:], '4-byte aligned')
    refused(name, [a, inside] + good[2:], 'y overlaps x')
    refused(name, [a, a] + good[2:], 'y overlaps x')
    return seen


N_EINVAL = (3 + 5 + 3 + 1 + 5) + (3 + 5 + 1 + 2)
