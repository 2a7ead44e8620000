"""Case tables, inputs and the fp64 reference shared by tests/test_linattn_fused_host.py (no GPU) and
tests/test_gpu_linattn_fused.py (-m gpu): the two fused LinearAttention passes of csrc/linattn_fused.hip and the merge
between them, each alone and together, at the pixel counts where a workgroup owns several 64-pixel sub-tiles.

Layout: activations are (B, n, C) — the kernels see [B][n][C], so the GPU tests run them as images with H = 1, W = n.
Reference (`reference`): the unfused mathematics in float64 from the same fp32 inputs.  Yardstick: the same function in
float32 on the CPU; e32 = its error against float64, measured exactly as the kernel's error is measured (`head_err`,
`ctx_err`, `unit_err`, `y_err`).  Gate of a kernel output: 2e-5 for the `plain` kind (the bound the parity tests of these
kernels in tests/test_gpu_kernels.py have always used, here per head), max(2e-5, 10 * e32) for every other kind — the rule
of tests/norm_bwd_cases.py.  tests/test_linattn_fused_host.py caps every e32 at CAP, so that no gate exceeds 10 * CAP."""
import collections
import functools
import math

import torch

from gpu_util import rand

EPS = 1e-5
SCALE = 32 ** -0.5
FLOOR = 2e-5
CAP = 1e-3
TP = 64                 # pixels per sub-tile (csrc/linattn_fused.hip)
LA_PART = 32 + 32 + 1024

Case = collections.namedtuple('Case', 'n C B kind')


def cdiv(a, b):
    return -(-a // b)


def plan(n):
    """the launch plan of csrc/linattn_fused.hip (`fused_tiles`, `dmh_linattn_fused_splits`) restated: sub-tiles per
    workgroup, workgroups (splits) per sample, sub-tiles of the last split, valid pixels of the last sub-tile"""
    nt = cdiv(n, TP)
    tiles = min(max(nt // 32, 1), 8)
    ns = cdiv(nt, tiles)
    return dict(nt=nt, tiles=tiles, ns=ns, last_tiles=nt - (ns - 1) * tiles, last_pixels=n - (nt - 1) * TP)


# ------------------------------------------------------------------ the table
KINDS = ['plain', 'sharp_k', 'sharp_q', 'rising', 'falling', 'gain_outlier', 'one_hot_pixel', 'tiny_head', 'v_outlier',
         'constant_image', 'zero_v']
ZERO_KINDS = ('constant_image', 'zero_v')      # the attention output is exactly zero
WIDTHS = (64, 128, 256)
ODD_WIDTHS = (32, 96)                          # one chunk / an odd chunk count: accepted by the C ABI, in no UNet
KIND_N = (65, 4160)                            # tiles = 1 with a one-pixel second split / tiles = 2 with a short 33rd split
SMALL_N = (1, 4, 63, 64, 65)                   # tiles = 1, one or two splits
MID_N = (4095, 4096, 4097, 6150)               # tiles = 2, 2, 2 (+ a 33rd split of one pixel), 3
BIG_N = (16384, 16512)                         # tiles = 8; 16512: 33 splits, the last one of 2 sub-tiles


def _table():
    t = [Case(n, C, 2, 'plain') for n in SMALL_N + MID_N + (4160,) for C in WIDTHS]
    t += [Case(4097, 64, 1, 'plain'), Case(4097, 128, 3, 'plain')]
    t += [Case(n, C, 1, k) for n in BIG_N for C in WIDTHS for k in ('plain', 'rising')]
    t += [Case(n, C, 2, 'plain') for n in KIND_N for C in ODD_WIDTHS]
    t += [Case(n, C, 2, k) for k in KINDS[1:] for n in KIND_N for C in WIDTHS]
    return t


CASES = _table()


def case_id(c):
    return f'n{c.n}-C{c.C}-B{c.B}-{c.kind}'


# ------------------------------------------------------------------ reference
def layernorm(t, gain, dim=-1):
    m = t.mean(dim, keepdim=True)
    v = t.var(dim, unbiased=False, keepdim=True)
    return (t - m) / (v + EPS).sqrt() * gain


def reference(x, g, w_qkv, w_out=None, b_out=None, g_out=None):
    """x (B, n, C), g (C,), w_qkv (384, C) [, w_out (64, 128), b_out (64,), g_out (64,)], all of one dtype (float64 for
    the reference, float32 for the yardstick).  -> dict: k, v (B, 4, 32, n) the projected logits / values, ctx (B, 4, 32, 32)
    [d][e], out (B, n, 128) channel = head * 32 + e, and for the block r = LN(to_out(out) + b) * g_out, y = x + r."""
    B, n, C = x.shape
    qkv = layernorm(x, g) @ w_qkv.t()                                   # (B, n, 384)
    q, k, v = [t.reshape(B, n, 4, 32).permute(0, 2, 3, 1) for t in qkv.split(128, dim=-1)]   # (B, 4, 32, n)
    qs = q.softmax(dim=2) * SCALE
    ks = k.softmax(dim=3)
    ctx = torch.einsum('bhdn,bhen->bhde', ks, v) / n
    out = torch.einsum('bhde,bhdn->bnhe', ctx, qs).reshape(B, n, 128)
    res = dict(k=k, v=v, ctx=ctx, out=out)
    if w_out is not None:
        res['t'] = out @ w_out.t()
        res['r'] = layernorm(res['t'] + b_out, g_out)
        res['y'] = x + res['r']
    return res


def split_units(k, v, n):
    """per (b, split, head) of the launch plan of n, from the logits k, v (B, 4, 32, n):
    lse (B, ns, 4, 32) = logsumexp of k[d] over the split's pixels, wm (B, ns, 4, 32, 32) [d][e] = the softmax-weighted mean
    of v[e] over them — the two forms of a context partial that do not depend on the maximum a split happens to store"""
    p = plan(n)
    B = k.shape[0]
    L = p['tiles'] * TP
    pad = p['ns'] * L - n
    kp = torch.cat([k, k.new_full((B, 4, 32, pad), -math.inf)], 3).reshape(B, 4, 32, p['ns'], L)
    vp = torch.cat([v, v.new_zeros((B, 4, 32, pad))], 3).reshape(B, 4, 32, p['ns'], L)
    lse = torch.logsumexp(kp, 4).permute(0, 3, 1, 2).contiguous()
    wm = torch.einsum('bhdsl,bhesl->bshde', kp.softmax(4), vp).contiguous()
    return lse, wm


def partials_from(k, v, n, offsets):
    """context partials (B, ns, 4, LA_PART) as pass 1 lays them out — m[32], s[32], ctx[32][32] — from float64 logits, the
    stored maximum of split sp moved off the true one by offsets[sp]"""
    p = plan(n)
    B = k.shape[0]
    L = p['tiles'] * TP
    pad = p['ns'] * L - n
    kp = torch.cat([k, k.new_full((B, 4, 32, pad), -math.inf)], 3).reshape(B, 4, 32, p['ns'], L)
    vp = torch.cat([v, v.new_zeros((B, 4, 32, pad))], 3).reshape(B, 4, 32, p['ns'], L)
    m = kp.amax(4) + offsets.to(k.dtype)[None, None, None, :]           # (B, 4, 32, ns)
    w = (kp - m[..., None]).exp()
    s = w.sum(4)
    c = torch.einsum('bhdsl,bhesl->bshde', w, vp)
    return torch.cat([m.permute(0, 3, 1, 2), s.permute(0, 3, 1, 2), c.reshape(B, p['ns'], 4, 1024)], 3).contiguous()


def merge_formula(partial, n):
    """the merge of the splits in partial's dtype: M = max m, S = sum s exp(m - M), ctx = sum ctx exp(m - M) / S / n"""
    B, ns = partial.shape[:2]
    m, s, c = partial[..., :32], partial[..., 32:64], partial[..., 64:].reshape(B, ns, 4, 32, 32)
    w = (m - m.amax(1, keepdim=True)).exp()
    return (c * w[..., None]).sum(1) / (s * w).sum(1)[..., None] / n


def merge_offsets(ns):
    """a different offset for neighbouring splits, in [-3, 3]"""
    return torch.tensor([((7 * sp) % 5 - 2) * 1.5 for sp in range(ns)], dtype=torch.float64)


# ------------------------------------------------------------------ error measures (float64, on the CPU)
def _amax(t, dims):
    return t.abs().amax(dims)


def head_err(got, ref):
    """(B, n, 128) -> (4,): max |err| over a head's channels, all rows and pixels, over max |ref| there"""
    B, n, _ = ref.shape
    g, r = got.double().cpu().reshape(B, n, 4, 32), ref.double().reshape(B, n, 4, 32)
    return _amax(g - r, (0, 1, 3)) / _amax(r, (0, 1, 3)).clamp_min(1e-300)


def ctx_err(got, ref):
    """(B, 4, 32, 32) -> (B, 4)"""
    g, r = got.double().cpu().reshape(ref.shape), ref.double()
    return _amax(g - r, (2, 3)) / _amax(r, (2, 3)).clamp_min(1e-300)


def unit_err(got, ref):
    """(B, ns, 4, 32, 32) -> (B, ns, 4)"""
    g, r = got.double().cpu(), ref.double()
    return _amax(g - r, (3, 4)) / _amax(r, (3, 4)).clamp_min(1e-300)


def y_err(got, ref_y, ref_r):
    """(B, n, 64) -> (B,).  y = x + r with r = LN(to_out(core) + b) * g_out of order one, so the error of r is measured
    against max |r| of the sample; the final addition rounds y once more, at most half an ulp of |y| — one whole fp32 ulp
    (2^-23 |y|) is taken off every element's error first, which matters only where |x| is far above |r| (the one-hot
    pixels at 1e4)."""
    g = got.double().cpu().reshape(ref_y.shape)
    e = ((g - ref_y).abs() - 2.0 ** -23 * ref_y.abs()).clamp_min(0.0)
    return e.amax((1, 2)) / _amax(ref_r, (1, 2)).clamp_min(1e-300)


def gate(kind, e32):
    """tensor of gates for a tensor of e32"""
    e32 = torch.as_tensor(e32, dtype=torch.float64)
    if kind == 'plain':
        return torch.full_like(e32, FLOOR)
    return (10.0 * e32).clamp_min(FLOOR)


def check(name, kind, err, e32):
    """print the [parity] line of one kernel output (its worst unit) and hold every unit to its gate; -> (err, e32) there"""
    err, e32 = torch.as_tensor(err, dtype=torch.float64).flatten(), torch.as_tensor(e32, dtype=torch.float64).flatten()
    g = gate(kind, e32)
    i = int((err / g).argmax())
    print(f'[parity] {name}: err={err[i].item():.3e} e32={e32[i].item():.3e} gate={g[i].item():.3e} '
          f'(worst of {err.numel()} units, max e32 {e32.max().item():.3e})')
    assert bool(torch.isfinite(err).all()), f'{name}: not finite'
    assert bool((err <= g).all()), f'{name}: error {err[i].item():.3e} of the reference scale, plain fp32 on the CPU has ' \
                                   f'{e32[i].item():.3e}, gate {g[i].item():.3e}'
    return err[i].item(), e32[i].item()


# ------------------------------------------------------------------ inputs
RISE = 40.0             # rising / falling: alpha runs from 0 to RISE over the pixels
# ... and the k rows are as sharp as in sharp_k: |k| <= |w_row| sqrt(C) max|g| whatever x is, about 8 at C = 64 with unit
# rows, and a linear ramp gives a workgroup 1/32 of the whole rise — unit rows cannot move a column's maximum by the 7 nats
# (exp < 1e-3) inside a workgroup that the host test asks for; x 30 does, for every column (test_linattn_fused_host.py)
RISE_K = 30.0
HOT = 1.0e4
V_OUTLIER_AT = 17       # pixel of every sub-tile that carries the large v
V_SMALL = 2.0 ** -23    # scale of the other pixels: their variance is far below eps, LN(x) ~ x / sqrt(eps)


def hot_pixels(n):
    return sorted({0, n // 3, n // 2, n - 2, n - 1} & set(range(n)))


def inputs(case):
    """fp32 inputs of a case: x (B, n, C), g, w (384, C), and for C == 64 the block's wo (64, 128), bo, go"""
    n, C, B, kind = case
    seed = 7000 + 13 * n + C + 1000 * B
    x = rand((B, n, C), seed) * 1.7 + 0.3
    x[..., :C // 2] *= 4.0                                   # two channel halves with different maxima
    g = 1 + 0.2 * rand((C,), seed + 1)
    w = rand((384, C), seed + 2, C ** -0.5)
    # the core output is O(0.03 / n) (the context carries 1 / n): scale to_out so that its result is of order one and not
    # buried under the bias — otherwise LN(to_out(core) + b) barely depends on the attention (`t_rms`, checked on the host)
    wo = rand((64, 128), seed + 3, 128 ** -0.5) * 30.0 * n
    bo = rand((64,), seed + 4, 0.1)
    go = 1 + 0.2 * rand((64,), seed + 5)
    if kind == 'sharp_k':
        w[128:256] *= 30.0
    elif kind == 'sharp_q':
        w[:128] *= 30.0
    elif kind in ('rising', 'falling'):
        u = w[128:256].mean(0)
        u = u / u.norm()
        alpha = torch.linspace(0.0, RISE, n) if n > 1 else torch.zeros(1)
        if kind == 'falling':
            alpha = alpha.flip(0)
        x = x + alpha[None, :, None] * u[None, None, :]
        w[128:256] *= RISE_K
    elif kind == 'gain_outlier':
        g[C // 3] *= 1024.0
    elif kind == 'one_hot_pixel':
        j = int(g.abs().argmax())
        for p in hot_pixels(n):
            x[:, p, :] = 0.0
            x[:, p, j] = HOT
    elif kind == 'tiny_head':
        w[256 + 96:384] /= 4096.0
        wo[:, 96:128] *= 4096.0
    elif kind == 'v_outlier':
        x = x * V_SMALL
        for p in range(V_OUTLIER_AT, n, TP):
            row = w[256 + p % 128]
            x[:, p, :] = row / row.norm()
    elif kind == 'constant_image':
        x = x[..., :1].expand(B, n, C)
        bo = torch.full((64,), 0.25)                         # LN(to_out(0) + b) is exactly 0 only for a constant b
    elif kind == 'zero_v':
        w[256:384] = 0.0
    else:
        assert kind == 'plain', kind
    d = dict(x=x.contiguous(), g=g, w=w.contiguous())
    if C == 64:
        d.update(wo=wo.contiguous(), bo=bo, go=go)
    return d


def _run(inp, dtype, wo=None):
    blk = [t.to(dtype) for t in ((inp['wo'] if wo is None else wo), inp['bo'], inp['go'])] if 'wo' in inp else []
    return reference(inp['x'].to(dtype), inp['g'].to(dtype), inp['w'].to(dtype), *blk)


def wo_without_head3(wo):
    w = wo.clone()
    w[:, 96:128] = 0.0
    return w


@functools.lru_cache(maxsize=2)
def case_reference(case):
    """-> inp, plan, the float64 reference (without the logits: what is needed of them is formed here), the pass-1 units
    lse / wm, the merge inputs, and e32 of every compared quantity.  Cached for the case at hand only: the GPU tests visit
    the table case by case."""
    case = Case(*case)
    inp = inputs(case)
    p = plan(case.n)
    r64, r32 = _run(inp, torch.float64), _run(inp, torch.float32)
    lse64, wm64 = split_units(r64['k'], r64['v'], case.n)
    lse32, wm32 = split_units(r32['k'], r32['v'], case.n)
    kmax = max(1.0, r64['k'].abs().max().item())
    part = partials_from(r64['k'], r64['v'], case.n, merge_offsets(p['ns'])).float()
    zero = case.kind in ZERO_KINDS
    out = dict(case=case, inp=inp, plan=p, kmax=kmax, zero=zero, ctx=r64['ctx'], out=r64['out'], lse=lse64, wm=wm64,
               partial=part, merged=merge_formula(part.double(), case.n),
               stats=dict(k=_col_stats(r64['k'], case.n), vmax=r64['v'].abs().amax((0, 2, 3)),
                          ctxmax=r64['ctx'].abs().amax((0, 2, 3)), v_pix=r64['v'].abs().amax((1, 2))))
    # (constant_image: torch's fp32 mean of C equal numbers is not exact, the kernels' is — power-of-two butterflies — so
    #  their k is exactly 0 and lse = log(pixels of the split): no yardstick, the floor alone)
    e32 = dict(lse_abs=(lse32.double() - lse64).abs().amax(3) / kmax * (case.kind != 'constant_image'))
    if not zero:
        e32.update(wm=unit_err(wm32, wm64), ctx=ctx_err(r32['ctx'], r64['ctx']), out=head_err(r32['out'], r64['out']),
                   merged=ctx_err(merge_formula(part, case.n), out['merged']))
    if 'wo' in inp:
        out.update(y=r64['y'], r=r64['r'], t_rms=r64['t'].pow(2).mean().sqrt().item())
        if case.kind != 'constant_image':     # (zero_v: y = x + LN(b) * g_out, not zero)
            e32['y'] = _amax(r32['r'].double() - r64['r'], (1, 2)) / _amax(r64['r'], (1, 2))
        if case.kind == 'tiny_head':          # head 3's own contribution to y
            wz = wo_without_head3(inp['wo'])
            z64, z32 = _run(inp, torch.float64, wz), _run(inp, torch.float32, wz)
            out['d3'] = r64['y'] - z64['y']
            out['y_without3'] = z64['y']
            d32 = (r32['r'] - z32['r']).double()
            e32['d3'] = _amax(d32 - (r64['r'] - z64['r']), (1, 2)) / _amax(out['d3'], (1, 2))
    out['e32'] = e32
    return out


def _col_stats(k, n):
    """what the host test asks of the k logits (B, 4, 32, n): per column the smallest exp(m_first_subtile - m_final) over
    the workgroups that own at least two sub-tiles, the same for the last sub-tile, and the fraction of pixels whose
    exp2 argument is below the smallest normal fp32 exponent"""
    p = plan(n)
    B = k.shape[0]
    pad = p['nt'] * TP - n
    mt = torch.cat([k, k.new_full((B, 4, 32, pad), -math.inf)], 3).reshape(B, 4, 32, p['nt'], TP).amax(4)   # per sub-tile
    first, last = k.new_ones((B, 4, 32)), k.new_ones((B, 4, 32))
    for sp in range(p['ns']):
        t0, t1 = sp * p['tiles'], min((sp + 1) * p['tiles'], p['nt'])
        if t1 - t0 < 2:
            continue
        fin = mt[..., t0:t1].amax(3)
        first = torch.minimum(first, (mt[..., t0] - fin).exp())
        last = torch.minimum(last, (mt[..., t1 - 1] - fin).exp())
    under = (k - k.amax(3, keepdim=True) < -126 * math.log(2)).flatten(1, 2).any(1).double().mean().item()
    return dict(first=first, last=last, under=under)
