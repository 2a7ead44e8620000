"""Case tables, inputs and float64 references shared by tests/test_attn_core_host.py (no GPU) and
tests/test_gpu_attn_core.py (-m gpu): the kernels of csrc/attention.hip (linattn_context / merge / apply, attention_kernel)
and the seven launches of csrc/attention_backward.hip (dmh_linattn_backward), each alone, at the smallest pixel counts that
reach every split, chunk and tile boundary of their launch plan.

Layout: qkv is (B, n, 384), channel = part * 128 + head * 32 + d (part 0 q, 1 k, 2 v), outputs (B, n, 128), channel =
head * 32 + e — what the kernels see.  Reference: the plain mathematics (autograd for the gradients) in float64 from the same
fp32 inputs.  Yardstick: the same plain operation in float32 torch on the CPU; e32 = its error against float64, measured as
the kernel's error is measured: max abs error over the reference's max abs per (batch row, head) — per (row, split, head)
for the pass-1 partials — never over a whole tensor.  Gate of a kernel output: `plain` keeps the bounds of the older
whole-tensor tests of these kernels, FWD = 1e-5 forward and GRAD = 2e-5 for gradients; every other kind gets
max(that, 10 * e32).  tests/test_attn_core_host.py caps every e32 at CAP, so no gate exceeds 10 * CAP."""
import collections
import functools
import math

import numpy as np
import torch

from gpu_util import rand
from linattn_fused_cases import cdiv, ctx_err, unit_err
from norm_bwd_cases import ulp32  # noqa: F401  (one fp32 unit in the last place, for the known answers)

SCALE = float(np.float32(32 ** -0.5))      # the fp32 value the kernels receive
FWD = 1e-5
GRAD = 2e-5
CAP = 1e-3

# ------------------------------------------------------------------ the launch plan, restated from the two kernel files
LA_NS = 128             # pixels per split of linattn_context_kernel
LA_PART = 32 + 32 + 1024
LA_TILES = 4            # 32-pixel tiles per workgroup of linattn_apply_kernel
LAB_TILES = 4           # ... of linattn_bwd_q_kernel / linattn_bwd_kv_kernel
LAB_NS = 128            # pixels per split of pixel_outer_kernel
COLSUM_CHUNK = 256      # pixels per chunk of colsum128_kernel
ATT_TILE = 32           # queries per wave and keys per step of attention_kernel


def splits(n):
    return cdiv(n, LA_NS)


def partial_floats(B, n):
    """forward partials [b][split][head][LA_PART]"""
    return B * splits(n) * 4 * LA_PART


def bwd_regions(B, n):
    """the five regions of the backward workspace in their order: name -> (offset, floats).  The two partial regions are
    [split or chunk][b][...] — the batch row is the INNER index there, unlike the forward partials."""
    sizes = [('qs', B * n * 128), ('dctx_part', cdiv(n, LAB_NS) * B * 4 * 1024), ('dctx', B * 4 * 1024),
             ('t_part', cdiv(n, COLSUM_CHUNK) * B * 128), ('t', B * 128)]
    out, off = collections.OrderedDict(), 0
    for name, size in sizes:
        out[name] = (off, size)
        off += size
    return out


def bwd_workspace_floats(B, n):
    return sum(size for _, size in bwd_regions(B, n).values())


def row(n):
    """(context / outer-product splits, pixels in the last split, colsum128 chunks, pixels in the last chunk, key tiles,
    keys in the last tile)"""
    ns, nc, nt = cdiv(n, LA_NS), cdiv(n, COLSUM_CHUNK), cdiv(n, ATT_TILE)
    return ns, n - (ns - 1) * LA_NS, nc, n - (nc - 1) * COLSUM_CHUNK, nt, n - (nt - 1) * ATT_TILE


# ------------------------------------------------------------------ the tables
Case = collections.namedtuple('Case', 'n B kind')

LA_N = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1000)
ATT_N = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025)
LA_KIND_N = (33, 257, 1000)
ATT_KIND_N = (33, 257, 1025)
LA_KINDS = ['plain', 'sharp_k', 'sharp_q', 'rising', 'falling', 'offset90', 'v_outlier']
ATT_KINDS = ['plain', 'big_logits', 'rising', 'falling', 'last_key', 'first_key', 'v_outlier']
DOMINANT = ('last_key', 'first_key')


def _table(ns, kind_n, kinds):
    t = [Case(n, 2, 'plain') for n in ns] + [Case(257, 1, 'plain'), Case(257, 3, 'plain')]
    return t + [Case(n, 2, k) for k in kinds[1:] for n in kind_n]


LA_CASES = _table(LA_N, LA_KIND_N, LA_KINDS)
ATT_CASES = _table(ATT_N, ATT_KIND_N, ATT_KINDS)


def case_id(c):
    return f'n{c.n}-B{c.B}-{c.kind}'


# ------------------------------------------------------------------ inputs
RAMP = 12.0             # rising / falling: k moves by RAMP per 128 pixels
SHARP = 30.0
OFFSET = 90.0
BIG = 12.0
DOMINATE = 25.0
V_OUTLIER = 4096.0
V_OUTLIER_AT = 5        # pixel of every 128 that carries the large v


def _ramp(n):
    return RAMP * torch.arange(n, dtype=torch.float32) / 128.0


def _v_outlier(qkv):
    qkv[:, V_OUTLIER_AT::128, 256:] *= V_OUTLIER


def la_inputs(case):
    """fp32 qkv (B, n, 384) and dout (B, n, 128) of a LinearAttention case"""
    n, B, kind = case
    seed = 9000 + 17 * n + 1000 * B
    qkv = rand((B, n, 384), seed) * 1.5
    dout = rand((B, n, 128), seed + 1)
    if kind == 'sharp_k':
        qkv[..., 128:256] *= SHARP
    elif kind == 'sharp_q':
        qkv[..., :128] *= SHARP
    elif kind == 'rising':
        qkv[..., 128:256] += _ramp(n)[None, :, None]
    elif kind == 'falling':
        qkv[..., 128:256] -= _ramp(n)[None, :, None]
    elif kind == 'offset90':     # softmax is shift invariant on both axes; without the max subtraction exp(90) overflows
        qkv[..., 128:256] += OFFSET
        qkv[..., :128] -= OFFSET
    elif kind == 'v_outlier':
        _v_outlier(qkv)
    else:
        assert kind == 'plain', kind
    return dict(qkv=qkv.contiguous(), dout=dout.contiguous())


def dominant_key(case):
    return {'last_key': case.n - 1, 'first_key': 0}[case.kind]


def att_inputs(case):
    """fp32 qkv (B, n, 384) of an attention case"""
    n, B, kind = case
    seed = 9500 + 17 * n + 1000 * B
    qkv = rand((B, n, 384), seed) * 1.5
    if kind == 'big_logits':
        qkv[..., :256] *= BIG
    elif kind == 'rising':       # a query whose channels sum to a positive number meets a larger logit at every key tile
        qkv[..., 128:256] += _ramp(n)[None, :, None]
    elif kind == 'falling':
        qkv[..., 128:256] -= _ramp(n)[None, :, None]
    elif kind in DOMINANT:       # one key x 25, every q sign-aligned to it (as test_attention_online_softmax_rescale)
        j = dominant_key(case)
        qkv[:, j, 128:256] *= DOMINATE
        qkv[..., :128] = qkv[:, j:j + 1, 128:256].sign() * qkv[..., :128].abs()
    elif kind == 'v_outlier':
        _v_outlier(qkv)
    else:
        assert kind == 'plain', kind
    return dict(qkv=qkv.contiguous())


# ------------------------------------------------------------------ references
def heads(qkv):
    """(B, n, 384) -> q, k, v (B, 4, 32, n)"""
    B, n, _ = qkv.shape
    return [t.reshape(B, n, 4, 32).permute(0, 2, 3, 1) for t in qkv.split(128, dim=-1)]


def la_autograd(qkv, dout, dtype):
    """the LinearAttention core and its gradients by torch autograd in dtype.  -> k, v (B, 4, 32, n) logits / values,
    ctx (B, 4, 32, 32) [d][e], M, S (B, 4, 32) = max and sum exp(k - M) of k over the pixels, out (B, n, 128),
    dqkv (B, n, 384), dctx (B, 4, 32, 32) = d loss / d ctx, t (B, 4, 32) = sum_n k' dk'"""
    x = qkv.detach().to(dtype).requires_grad_(True)
    n = x.shape[1]
    q, k, v = heads(x)
    qs = q.softmax(dim=2) * SCALE
    ks = k.softmax(dim=3)
    ks.retain_grad()
    ctx = torch.einsum('bhdn,bhen->bhde', ks, v) / n
    ctx.retain_grad()
    out = torch.einsum('bhde,bhdn->bnhe', ctx, qs).reshape(x.shape[0], n, 128)
    out.backward(dout.to(dtype))
    kd = k.detach()
    M = kd.amax(3)
    return dict(k=kd, v=v.detach(), ctx=ctx.detach(), M=M, S=(kd - M[..., None]).exp().sum(3), out=out.detach(),
                dqkv=x.grad, dctx=ctx.grad, t=(ks.detach() * ks.grad).sum(3))


def la_formulas(qkv, ctx, M, S, dout, drop_last_split=False, drop_last_chunk=False):
    """the backward as the header of csrc/attention_backward.hip states it, in the dtype of the arguments, from a given
    ctx and (M, S) as the kernel takes them.  -> dqkv (B, n, 384), dctx (B, 4, 32, 32), t (B, 4, 32).
    drop_last_split / drop_last_chunk: the two mutations tests/test_attn_core_host.py shows the gates to reject — a dctx
    without the last LAB_NS-pixel split, a t without the last COLSUM_CHUNK-pixel chunk."""
    B, n, _ = qkv.shape
    q, k, v = heads(qkv)
    dO = dout.reshape(B, n, 4, 32).permute(0, 2, 3, 1)                   # [e, n]
    s = q.softmax(dim=2)
    qs = s * SCALE
    kp = (k - M[..., None]).exp() / S[..., None]
    n_d = (cdiv(n, LAB_NS) - 1) * LAB_NS if drop_last_split else n
    dctx = torch.einsum('bhdn,bhen->bhde', qs[..., :n_d], dO[..., :n_d])
    ds = torch.einsum('bhde,bhen->bhdn', ctx, dO) * SCALE
    dq = s * (ds - (ds * s).sum(2, keepdim=True))
    dkp = torch.einsum('bhde,bhen->bhdn', dctx, v) / n
    dv = torch.einsum('bhde,bhdn->bhen', dctx, kp) / n
    n_t = (cdiv(n, COLSUM_CHUNK) - 1) * COLSUM_CHUNK if drop_last_chunk else n
    t = (kp * dkp)[..., :n_t].sum(3)
    dk = kp * (dkp - t[..., None])
    dqkv = torch.cat([g.permute(0, 3, 1, 2).reshape(B, n, 128) for g in (dq, dk, dv)], dim=2)
    return dict(dqkv=dqkv, dctx=dctx, t=t)


def split_pad(k, v, L=LA_NS):
    """k, v (B, 4, 32, n) -> (B, 4, 32, ns, L), padded with -inf / 0 as the kernel masks"""
    B, n = k.shape[0], k.shape[3]
    ns = cdiv(n, L)
    pad = ns * L - n
    kp = torch.cat([k, k.new_full((B, 4, 32, pad), -math.inf)], 3).reshape(B, 4, 32, ns, L)
    vp = torch.cat([v, v.new_zeros((B, 4, 32, pad))], 3).reshape(B, 4, 32, ns, L)
    return kp, vp


def split_units(k, v):
    """per (b, split, head): lse (B, ns, 4, 32) = logsumexp of k[d] over the split's pixels, wm (B, ns, 4, 32, 32) [d][e] =
    the softmax-weighted mean of v[e] over them, m (B, ns, 4, 32) = the split's maximum of k[d]"""
    kp, vp = split_pad(k, v)
    lse = torch.logsumexp(kp, 4).permute(0, 3, 1, 2).contiguous()
    wm = torch.einsum('bhdsl,bhesl->bshde', kp.softmax(4), vp).contiguous()
    return lse, wm, kp.amax(4).permute(0, 3, 1, 2).contiguous()


def merge_splits(m, s, c, n, weights=True):
    """the merge of csrc/attention.hip in the dtype of its arguments: m, s (B, ns, 4, 32), c (B, ns, 4, 32, 32) ->
    ctx (B, 4, 32, 32), M, S (B, 4, 32).  weights=False: the mutation without exp(m - M)."""
    M = m.amax(1)
    w = (m - M[:, None]).exp() if weights else torch.ones_like(m)
    S = (s * w).sum(1)
    return (c * w[..., None]).sum(1) / S[..., None] / n, M, S


def att_forward(qkv, dtype):
    """softmax_j((q * scale) . k) v -> out (B, n, 128), and P (B, 4, n, n)"""
    x = qkv.to(dtype)
    B, n, _ = x.shape
    q, k, v = heads(x)
    sim = torch.einsum('bhdi,bhdj->bhij', q * SCALE, k)
    p = sim.softmax(dim=-1)
    return torch.einsum('bhij,bhdj->bihd', p, v).reshape(B, n, 128), p


def att_online(qkv, dtype, rescale=True):
    """the key-tile loop of attention_kernel in dtype on the CPU: running maximum, running sum and accumulator over tiles
    of ATT_TILE keys.  rescale=False: the mutation whose accumulator is not multiplied by alpha when the maximum rises."""
    x = qkv.to(dtype)
    B, n, _ = x.shape
    q, k, v = heads(x)
    qs = q * SCALE
    mrun = x.new_full((B, 4, n), -math.inf)
    lrun = x.new_zeros((B, 4, n))
    acc = x.new_zeros((B, 4, n, 32))
    for k0 in range(0, n, ATT_TILE):
        sim = torch.einsum('bhdi,bhdj->bhij', qs, k[..., k0:k0 + ATT_TILE])
        mnew = torch.maximum(mrun, sim.amax(3))
        alpha = (mrun - mnew).exp()
        p = (sim - mnew[..., None]).exp()
        lrun = lrun * alpha + p.sum(3)
        if rescale:
            acc = acc * alpha[..., None]
        acc = acc + torch.einsum('bhij,bhdj->bhid', p, v[..., k0:k0 + ATT_TILE])
        mrun = mnew
    return (acc / lrun[..., None]).permute(0, 2, 1, 3).reshape(B, n, 128)


# ------------------------------------------------------------------ error measures (float64, on the CPU)
def _amax(t, dims):
    return t.abs().amax(dims)


def bh_err(got, ref):
    """(B, n, 128) -> (B, 4): max |err| over a (row, head)'s pixels and channels, over max |ref| there"""
    B, n, _ = ref.shape
    g, r = got.double().cpu().reshape(B, n, 4, 32), ref.double().reshape(B, n, 4, 32)
    return _amax(g - r, (1, 3)) / _amax(r, (1, 3)).clamp_min(1e-300)


def vec_err(got, ref):
    """(B, 4, 32) -> (B, 4)"""
    g, r = got.double().cpu().reshape(ref.shape), ref.double()
    return _amax(g - r, (2,)) / _amax(r, (2,)).clamp_min(1e-300)


def dqkv_err(got, ref, scales=None):
    """(B, n, 384) -> {dq, dk, dv: (B, 4)}.  scales: {dq, dk: (B, 4)} to measure against instead of max |ref| (`cancel_scales`)"""
    g, r = got.double().cpu().reshape(ref.shape), ref.double()
    out = {}
    for i, name in enumerate(('dq', 'dk', 'dv')):
        gi, ri = g[..., 128 * i:128 * i + 128], r[..., 128 * i:128 * i + 128]
        out[name] = bh_err(gi, ri)
        if scales is not None and name in scales:
            B, n, _ = ri.shape
            out[name] = _amax((gi - ri).reshape(B, n, 4, 32), (1, 3)) / scales[name]
    return out


def cancel_scales(qkv, ctx, dctx, dout):
    """n = 1 only: the softmax over one pixel is the constant 1 and the context does not depend on d, so dq = s (ds - sum ds s)
    and dk = k' (dk' - t) are mathematically ZERO — there is no reference scale to measure an error against.  Their errors
    are measured against the terms that cancel instead: max |s ds| and max |k' dk'| per (row, head), (B, 4) each."""
    B, n, _ = qkv.shape
    q, k, v = heads(qkv)
    dO = dout.reshape(B, n, 4, 32).permute(0, 2, 3, 1)
    ds = torch.einsum('bhde,bhen->bhdn', ctx, dO) * SCALE
    dkp = torch.einsum('bhde,bhen->bhdn', dctx, v) / n
    return dict(dq=_amax(q.softmax(2) * ds, (2, 3)), dk=_amax(k.softmax(3) * dkp, (2, 3)))


def gate(kind, e32, floor):
    """tensor of gates for a tensor of e32"""
    e32 = torch.as_tensor(e32, dtype=torch.float64)
    if kind == 'plain':
        return torch.full_like(e32, floor)
    return (10.0 * e32).clamp_min(floor)


def worst(kind, err, e32, floor):
    """-> (err, e32, gate, err / gate) of the unit that comes closest to (or goes furthest over) its gate"""
    err, e32 = torch.as_tensor(err, dtype=torch.float64).flatten(), torch.as_tensor(e32, dtype=torch.float64).flatten()
    g = gate(kind, e32, floor)
    ratio = torch.where(torch.isfinite(err), err / g, torch.full_like(err, math.inf))
    i = int(ratio.argmax())
    return err[i].item(), e32[i].item(), g[i].item(), ratio[i].item()


def check(name, kind, err, e32, floor):
    """print the [parity] line of one kernel output (its worst unit) and hold every unit to its gate"""
    e, y, g, ratio = worst(kind, err, e32, floor)
    print(f'[parity] {name}: err={e:.3e} e32={y:.3e} gate={g:.3e} '
          f'(worst of {torch.as_tensor(err).numel()} units, max e32 {float(torch.as_tensor(e32).max()):.3e})')
    assert ratio <= 1.0, f'{name}: error {e:.3e} of the reference scale, plain fp32 on the CPU has {y:.3e}, gate {g:.3e}'
    return e, y


# ------------------------------------------------------------------ references per case
@functools.lru_cache(maxsize=None)
def la_reference(case):
    """-> inp, r64 / r32 (la_autograd), zero_scale (n = 1: cancel_scales, else None), the pass-1 units lse / wm (float64)
    and m32 (bitwise: a maximum is exact in any order), M32, kmax, and e32 of every compared quantity"""
    case = Case(*case)
    inp = la_inputs(case)
    r64 = la_autograd(inp['qkv'], inp['dout'], torch.float64)
    r32 = la_autograd(inp['qkv'], inp['dout'], torch.float32)
    lse64, wm64, _ = split_units(r64['k'], r64['v'])
    lse32, wm32, m32 = split_units(r32['k'], r32['v'])
    kmax = max(1.0, r64['k'].abs().max().item())
    zs = cancel_scales(inp['qkv'].double(), r64['ctx'], r64['dctx'], inp['dout'].double()) if case.n == 1 else None
    e32 = dict(lse_abs=(lse32.double() - lse64).abs().amax(3) / kmax, wm=unit_err(wm32, wm64),
               ctx=ctx_err(r32['ctx'], r64['ctx']), S=vec_err(r32['S'], r64['S']), out=bh_err(r32['out'], r64['out']),
               dctx=ctx_err(r32['dctx'], r64['dctx']), t=vec_err(r32['t'], r64['t']), **dqkv_err(r32['dqkv'], r64['dqkv'], zs))
    return dict(zero_scale=zs, case=case, inp=inp, r64=r64, r32=r32, lse=lse64, wm=wm64, m32=m32, M32=r32['M'], kmax=kmax,
                e32=e32)


@functools.lru_cache(maxsize=None)
def att_reference(case):
    """-> inp, out (float64), e32 (B, 4), and for the dominant-key kinds the smallest fp32 softmax weight of that key"""
    case = Case(*case)
    inp = att_inputs(case)
    out64, _ = att_forward(inp['qkv'], torch.float64)
    out32, p32 = att_forward(inp['qkv'], torch.float32)
    res = dict(case=case, inp=inp, out=out64, e32=dict(out=bh_err(out32, out64)))
    if case.kind in DOMINANT:
        res['dominant_weight'] = p32[..., dominant_key(case)].min().item()
    return res


# known answers of dmh_attention -----------------------------------------------------------------------------------------
def att_constant_v(n, equal_keys, B=2):
    """plain q, v the same at every pixel (128 different channel values): out = v at every query.
    equal_keys: every key is the same vector too, and v lies on a grid of 2^-8 below 8.  Then every logit of a query is the
    same fp32 number, every weight exp(0) = 1, the row sum is the integer n and the accumulator v * n (11 + 11 bits) — all
    exact in fp32 — and out = (v n) * (1 / n) carries the rounding of the reciprocal and of the product only: at most
    2^-23 |v| < 2 ulps.  With plain keys the two sums of n rounded weights each carry up to (n - 1) 2^-24 of their own
    (plain fp32 torch on the CPU is 5 ... 20 ulps off at the n of the table): `constant_v_gate`."""
    qkv = att_inputs(Case(n, B, 'plain'))['qkv'].clone()
    v = rand((128,), 9901) * 1.5
    if equal_keys:
        qkv[..., 128:256] = rand((128,), 9902) * 1.5
        v = (v * 256).round().clamp(-2047, 2047) / 256
        v[v == 0] = 2.0 ** -8
    qkv[..., 256:] = v
    return qkv.contiguous()


def constant_v_bound(n):
    """relative error of out = (sum_j p_j v) / (sum_j p_j) in fp32 for ANY order of the additions: n products and n - 1
    additions above, n - 1 additions below (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, to first
    order), the reciprocal and the final product"""
    return (2 * n + 2) * 2.0 ** -24


def constant_v_rel(out, qkv):
    """max over the elements of |out - v| / |v|"""
    v = qkv[:, :1, 256:].double()
    return ((out.double().cpu() - v).abs() / v.abs()).max().item()


def constant_v_gate(qkv):
    """the gate of the plain-key form, per element and relative to |v|: 10 x e32 (the project's rule), e32 = the same measure of
    plain fp32 torch on the CPU, not below the 4 ulps (2^-22 |v|) of the exact form and never above the worst-case
    summation bound.  -> (gate, e32)"""
    e32 = constant_v_rel(att_forward(qkv, torch.float32)[0], qkv)
    return min(constant_v_bound(qkv.shape[1]), max(10.0 * e32, 2.0 ** -22)), e32


def att_equal_keys(n, B=2):
    """every key the same vector: the softmax is uniform, out = the mean of v over the pixels.  v has mean 3 in every channel,
    so that the answer is not a cancelling sum (a mean near zero would measure the order of n additions, not the kernel)."""
    qkv = att_inputs(Case(n, B, 'plain'))['qkv'].clone()
    qkv[..., 128:256] = rand((128,), 9902) * 1.5
    qkv[..., 256:] += 3.0
    return qkv.contiguous()


# what the host test asks of the inputs ----------------------------------------------------------------------------------
def neighbour_weight(k):
    """(B, 4, 32, n) -> (B, 4, 32): the smallest exp(-|m_sp - m_sp+1|) over neighbouring splits (1 where there is one split)"""
    m = split_pad(k, k)[0].amax(4)                                       # (B, 4, 32, ns)
    if m.shape[3] < 2:
        return k.new_ones(k.shape[:3])
    return (-(m[..., 1:] - m[..., :-1]).abs()).exp().amin(3)


def underflow_fraction(k):
    """the fraction of pixels whose exp argument is below the smallest normal fp32 exponent in some (head, d) column"""
    return (k - k.amax(3, keepdim=True) < -126 * math.log(2)).flatten(1, 2).any(1).double().mean().item()
