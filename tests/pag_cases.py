"""The statement of perturbed-attention guidance (``pag_scale``; include/dmhomo_hip.h has the definition) in fp32 torch ops on the
CPU — what dmh_pag_shift must give bit for bit —, its float64 form, the statement of the identity arm of dmh_attention_pag, the
case tables of the kernel tests and the argument checks of the two entries.  The sizes and pointer phases are those of
tests/flowg_cases.py.  No GPU is used here."""
import ctypes
import itertools

import torch

import flowg_cases as FC

SIZES, BATCHES, PHASES, BIG = FC.SIZES, FC.BATCHES, FC.PHASES, FC.BIG
SCALES = (0., 0.5, 3.)                                          # s = pag_scale
ATTN_B = 3
ATTN_NS = (1, 31, 32, 33, 64, 65, 256)                          # the query / key tile edges of K4, and the 128^2 bottleneck
ATTN_ROWS = (None, (0, 2))                                      # every row, or a list that leaves physical row 1 out


def _rows(keep, like):
    return keep.bool().reshape((-1,) + (1,) * (like.dim() - 1))


def shift32(cond, null, pert, s, keep=None):
    """fp32, one rounding per operation: c = cond where the row was computed, else null; d = c - p; e = s * d; case A (null is
    not None): null' = null + e, cond' = cond + e on computed rows; case B: cond' = c + e.  -> (cond', null' or None).  Rows with
    keep == 0 keep their cond bits (the kernel neither reads nor writes them)."""
    s32 = torch.tensor(s, dtype=torch.float32)
    if null is None:
        assert keep is None
        return cond + s32 * (cond - pert), None
    c = cond if keep is None else torch.where(_rows(keep, cond), cond, null)
    e = s32 * (c - pert)
    new_cond = cond + e
    if keep is not None:
        new_cond = torch.where(_rows(keep, cond), new_cond, cond)      # (torch.where hands a NaN's payload on unchanged)
    return new_cond, null + e


def shift64(cond, null, pert, s, keep=None):
    """the same in float64 on the fp32 inputs (s as the fp32 value the kernel receives) -> (cond', null' or None, e)"""
    s64 = float(torch.tensor(s, dtype=torch.float32))
    c0, p = cond.double(), pert.double()
    if null is None:
        e = s64 * (c0 - p)
        return c0 + e, None, e
    n = null.double()
    c = c0 if keep is None else torch.where(_rows(keep, cond), c0, n)
    e = s64 * (c - p)
    new_cond = c0 + e
    if keep is not None:
        new_cond = torch.where(_rows(keep, cond), new_cond, c0)
    return new_cond, n + e, e


def cases():
    """[(name, dict(cond, null or None, pert, keep or None, s))]: every size x batch, with and without a null pass, keep None /
    mixed / all zero; the rows of cond with keep == 0 are NaN (they were never computed); s walks SCALES"""
    out = []
    for k, (n, B) in enumerate(itertools.product(SIZES, BATCHES)):
        cond, null, pert = FC.inputs(B, n, 300 + k)
        s = SCALES[k % len(SCALES)]
        out.append((f'n{n}-B{B}-caseB', dict(cond=cond, null=None, pert=pert, keep=None, s=s)))
        for j, (kind, keep) in enumerate(FC.keeps_for(B).items()):
            c = cond.clone()
            if keep is not None:
                c[~keep.bool()] = float('nan')
            out.append((f'n{n}-B{B}-caseA-keep-{kind}', dict(cond=c, null=null, pert=pert, keep=keep,
                                                             s=SCALES[(k + j) % len(SCALES)])))
    return out


def attention_identity(qkv):
    """the identity arm: the attention core's output is v itself, out[b][pix][h*32 + e] = qkv[b][pix][256 + h*32 + e]"""
    return qkv[..., 256:384]


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
    name = 'dmh_pag_shift'
    #       cond null pert keep  s  B  n
    good = [a, b, c, None, 1., 2, 8]
    refused(name, [None] + good[1:], 'null pointer')
    refused(name, good[:2] + [None] + good[3:], 'null pointer')
    refused(name, [a, None, c, b, 1., 2, 8], 'keep needs model_null')
    for B, n, word in ((0, 8, 'B=0'), (-3, 8, 'B=-3'), (2, 0, 'n=0'), (2, -5, 'n=-5'), (2, 2 ** 31, '2^31')):
        refused(name, good[:5] + [B, n], word)
    for s in (float('nan'), float('inf'), float('-inf'), -1., -1e-30):
        refused(name, good[:4] + [s] + good[5:], 'finite number >= 0')
    odd = ctypes.c_void_p(c.value + 2)
    refused(name, [a, b, odd, None, 1., 2, 8], '4-byte aligned')
    inside = ctypes.c_void_p(a.value + 32)                      # 2 * 8 floats = 64 bytes: half a tensor in
    refused(name, [a, b, a, None, 1., 2, 8], 'pert overlaps')
    refused(name, [a, b, inside, None, 1., 2, 8], 'pert overlaps')
    refused(name, [a, b, b, None, 1., 2, 8], 'pert overlaps')
    refused(name, [a, None, inside, None, 1., 2, 8], 'pert overlaps')
    refused(name, [a, inside, c, None, 1., 2, 8], 'model_cond overlaps model_null')
    name = 'dmh_attention_pag'
    #       qkv out B  n  scale rows pert_lo
    good = [a, b, 3, 4, 0.5, None, 1]
    refused(name, [None] + good[1:], 'bad arguments')
    refused(name, [a, None] + good[2:], 'bad arguments')
    refused(name, [a, b, 0] + good[3:], 'bad arguments')
    refused(name, [a, b, 3, 0] + good[4:], 'bad arguments')
    for lo in (-1, 4, 2 ** 31 - 1):
        refused(name, good[:6] + [lo], 'pert_lo')
    return seen


N_EINVAL = (3 + 5 + 5 + 1 + 5) + (4 + 3)
