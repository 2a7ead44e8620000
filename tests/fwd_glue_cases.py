"""Case tables, inputs and CPU references shared by tests/test_fwd_glue_host.py (no GPU) and tests/test_gpu_fwd_glue.py
(-m gpu): the forward-path glue between the matrix-core kernels, each kernel alone — the channel LayerNorm, its per-pixel
statistics and GroupNorm+SiLU+residual of csrc/norm.hip, the final 1x1 convolution, input assembly, loss means, per-sample
affine combinations, uint8 export and step-table seek of csrc/sampler.hip, and the embeddings of csrc/embed.hip.

Reference: the plain operation in float64 torch on the CPU, from the same fp32 inputs.
Yardstick: the same plain formula in fp32 torch on the CPU; e32 = its error against the float64 reference, max abs error over
the reference's max abs (`rel` of tests/norm_bwd_cases.py, with its SCALE_FLOOR).
Gate of a float64-compared output: max(FLOOR, 10 * e32) — FLOOR, CAP and the 10x rule are those of tests/norm_bwd_cases.py
(DESIGN.md section 4); the host file holds every e32 under CAP.  dmh_final_conv_nchw, dmh_diff_mean and dmh_loss_combine are
checked per element against bounds from the standard error analysis (`fc_reference`, `dm_reference`, `lc_reference`); the
elementwise kernels of csrc/sampler.hip (compiled with contraction off), input assembly, the uint8 export and the table
gathers are bit-exact against fp32 torch / numpy in the same op order; the embeddings keep the atol of test_embeddings."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from gpu_util import rand
from norm_bwd_cases import CAP, EPS, FLOOR, SCALE_FLOOR, U, check, gate, rel   # noqa: F401  (re-exported to the two test files)

EMBED_ATOL = 2e-6      # the gate test_embeddings (tests/test_gpu_kernels.py) already uses


def hw_id(bhw):
    B, H, W = bhw
    return f'{B}x{H * W}px'


# ------------------------------------------------------------------ channel LayerNorm / per-pixel statistics
# C/4 lanes' worth of quads -> the <LPP, NV> arm of dmh_chan_layernorm (csrc/norm.hip); dmh_pixel_stats has no <2,1> / <4,1>
# arm: its ladder starts at <8,1>.  Restated here, with no export to read it from, as tests/test_norm_backward_host.py does
# for the backward ladder.
LN_LADDER = ((2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8))
PS_LADDER = LN_LADDER[2:]
LN_BLOCK_CAP = 16384     # launch_ln / launch_ps: at most this many 256-thread blocks, then the grid-stride loop
GS_BLOCK_CAP = 8192      # dmh_gn_silu_residual(_stats)


def arm(C, ladder=LN_LADDER):
    """-> (LPP, NV, ragged): the arm C dispatches to, and whether C/4 leaves lanes of a pixel's group (or part of the last
    NV round) without a quad"""
    c4 = C // 4
    for lpp, nv in ladder:
        if c4 <= lpp * nv:
            return lpp, nv, c4 < lpp * nv
    raise ValueError(C)


LN_WIDTHS = [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048]
LN_PIX = [(1, 1, 1), (1, 5, 7), (3, 7, 9)]     # 1, 35 and 189 pixels (odd: the 32-lane arm ends in half a wave)
LN_KINDS = ['unit', 'offset30', 'scale1e-4', 'scale1e4', 'const']
LN_KIND_WIDTHS = [12, 64, 132, 516]
LN_CASES = [(C, p, 'unit') for C in LN_WIDTHS for p in LN_PIX] + \
           [(C, LN_PIX[2], k) for C in LN_KIND_WIDTHS for k in LN_KINDS[1:]]
# the smallest launch that loops: C = 132 -> <64,1>, 4 pixels per block, 16384 blocks cover 65536 pixels; 3 more
LN_LOOP_CASE = (132, (1, 65536 + 3, 1), 'unit')


def ln_id(case):
    C, bhw, kind = case
    lpp, nv, ragged = arm(C)
    return f'C{C}-ln{lpp}x{nv}{"r" if ragged else ""}-ps{"x".join(map(str, arm(C, PS_LADDER)[:2]))}-{hw_id(bhw)}-{kind}'


def ln_formula(x, g, res=None, eps=EPS):
    """x (..., C), g (C,) -> (out, mean, rstd) in x's dtype: two-pass, biased variance, gain only (CFG:137-141)"""
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    out = (x - mean) * rstd * g
    if res is not None:
        out = out + res
    return out, mean[..., 0], rstd[..., 0]


def ln_inputs(case):
    """NHWC fp32.  unit: x * 2 + 0.7, as test_chan_layernorm; the kinds move the whole tensor"""
    C, (B, H, W), kind = case
    seed = 11000 + 7 * C + B * H * W % 1000
    shape = (B, H, W, C)
    if kind == 'const':
        x = torch.full(shape, 2.5)
    else:
        x = rand(shape, seed) * 2 + 0.7
        if kind == 'offset30':         # mean at 30 standard deviations
            x = x - 0.7 + 60.0
        elif kind == 'scale1e-4':      # variance (4e-8) below eps
            x = x * 1e-4
        elif kind == 'scale1e4':
            x = x * 1e4
        else:
            assert kind == 'unit', kind
    return dict(x=x.contiguous(), g=1 + 0.2 * rand((C,), seed + 1), res=rand(shape, seed + 2))


def _ln_reference(case):
    inp = ln_inputs(case)
    out = dict(inp=inp)
    for name, dt in (('ref64', torch.float64), ('ref32', torch.float32)):
        x, g, res = (inp[k].to(dt) for k in ('x', 'g', 'res'))
        o, mean, rstd = ln_formula(x, g)
        out[name] = dict(out=o, out_res=o + res, mean=mean, rstd=rstd)
    return out


@functools.lru_cache(maxsize=None)
def ln_reference(case):
    """-> inp {x, g, res}, ref64 / ref32 {out, out_res, mean, rstd}"""
    return _ln_reference(case)


def ln_loop_reference():
    """the grid-stride case (35 MB per fp32 tensor): not cached"""
    return _ln_reference(LN_LOOP_CASE)


# ------------------------------------------------------------------ SiLU(a * y + b) + res, and the statistics of the result
GS_WIDTHS = [4, 12, 64, 128, 256, 516]
GS_STATS_ARM = {64: 16, 128: 32, 256: 64}      # dmh_gn_silu_residual_stats: gn_silu_residual_kernel<LPP>
GS_PIX = [(1, 1, 1), (3, 5, 7), (2, 9, 21)]    # (B, HW) = (1, 1), (3, 35), (2, 189)
GS_KINDS = ['unit', 'saturated']
GS_CASES = [(C, p, 'unit', r) for C in GS_WIDTHS for p in GS_PIX for r in (False, True)] + \
           [(C, GS_PIX[2], 'saturated', r) for C in GS_WIDTHS for r in (False, True)]
# past the 8192-block cap: 131077 pixels x 16 quads = 8192.3 blocks of 256 quads
GS_LOOP_CASE = (64, (1, 131072 + 5, 1), 'unit', True)
GS_SATURATED_AT = 95.0


def gs_id(case):
    C, bhw, kind, with_res = case
    a = f'k0+k{GS_STATS_ARM[C]}' if C in GS_STATS_ARM else 'k0'
    return f'C{C}-{a}-{hw_id(bhw)}-{kind}-{"res" if with_res else "nores"}'


def gs_formula(y, coef, res=None, eps=EPS):
    """y (B, H, W, C), coef (B, 2, C) -> (out, mean, rstd, z): out = SiLU(z) + res with z = a * y + b, and the channel
    LayerNorm statistics of every pixel of out (what dmh_gn_silu_residual_stats hands to the LinearAttention behind it)"""
    z = coef[:, 0, None, None, :] * y + coef[:, 1, None, None, :]
    out = F.silu(z)
    if res is not None:
        out = out + res
    mean = out.mean(-1)
    rstd = (out.var(-1, unbiased=False) + eps).rsqrt()
    return out, mean, rstd, z


def gs_inputs(case):
    C, (B, H, W), kind, with_res = case
    seed = 12000 + 7 * C + B * H * W % 1000
    y = rand((B, H, W, C), seed)
    coef = torch.stack([1 + 0.2 * rand((B, C), seed + 1), 0.3 * rand((B, C), seed + 2)], 1).contiguous()
    if kind == 'saturated':      # |z| reaches 95 on both sides: exp(-z) overflows fp32 above 88.7
        z = gs_formula(y.double(), coef.double())[3]
        coef = coef * (GS_SATURATED_AT / min(z.max().item(), -z.min().item()))
    else:
        assert kind == 'unit', kind
    return dict(y=y, coef=coef.contiguous(), res=rand((B, H, W, C), seed + 3) if with_res else None)


def _gs_reference(case):
    inp = gs_inputs(case)
    out = dict(inp=inp)
    for name, dt in (('ref64', torch.float64), ('ref32', torch.float32)):
        o, mean, rstd, z = gs_formula(inp['y'].to(dt), inp['coef'].to(dt), None if inp['res'] is None else inp['res'].to(dt))
        out[name] = dict(out=o, mean=mean, rstd=rstd)
        if dt == torch.float64:
            out['z'] = z
    return out


@functools.lru_cache(maxsize=None)
def gs_reference(case):
    """-> inp {y, coef, res}, ref64 / ref32 {out, mean, rstd}, z (float64 pre-activations)"""
    return _gs_reference(case)


def gs_loop_reference():
    return _gs_reference(GS_LOOP_CASE)


# ------------------------------------------------------------------ dmh_final_conv_nchw
FC_COUTS = [1, 2, 3, 4, 6, 8, 12, 16]
FC_WIDTHS = [4, 32, 60, 64, 68, 128, 320]       # C <= 64: a lane owns one quad (C < 64: lanes without one); above: the loop
FC_PIX = [(1, 1, 1), (3, 5, 7), (2, 9, 21)]     # 1, 105 and 378 pixels: off 16 and off 64, a row boundary inside a 16-pixel block
# the thinned cross product: every Cout at C = 64 and 128 (both code paths), every C at Cout = 6 and 16
FC_PAIRS = sorted({(C, co) for C in (64, 128) for co in FC_COUTS} | {(C, co) for C in FC_WIDTHS for co in (6, 16)})


def fc_id(pair):
    C, cout = pair
    return f'C{C}-{"one" if C <= 64 else "loop"}-Cout{cout}'


def fc_inputs(C, cout, bhw):
    R, H, W = bhw
    seed = 13000 + 11 * C + cout + R * H * W % 1000
    return dict(x=rand((R, H, W, C), seed), w=rand((cout, C), seed + 1, C ** -0.5), bias=rand((cout,), seed + 2))


def fc_reference(x, w, bias):
    """x (R, H, W, C) NHWC, w (Cout, C), bias (Cout,) or None, fp32 -> (ref, bound) float64 (R, Cout, H, W): a dot product of
    C terms accumulated in ANY order is within C u sum |x||w| (Higham, Accuracy and Stability of Numerical Algorithms,
    section 3.1; the form `bgemm_reference` of tests/norm_bwd_cases.py uses); + 2 for the bias addition and its own term"""
    C = x.shape[-1]
    xd, wd = x.double(), w.double()
    ref = torch.einsum('rhwc,oc->rohw', xd, wd)
    mag = torch.einsum('rhwc,oc->rohw', xd.abs(), wd.abs())
    if bias is not None:
        ref = ref + bias.double()[None, :, None, None]
        mag = mag + bias.double().abs()[None, :, None, None]
    return ref, (C + 2) * U * mag


def fc_fp32(x, w, bias):
    return F.linear(x, w, bias).permute(0, 3, 1, 2)


# ------------------------------------------------------------------ dmh_assemble_input
AS_CPADS = [4, 8, 12, 16, 20, 24]     # Cpad / 4 = 1 .. 4: assemble_input_pix_kernel<1 .. 4>; above: assemble_input_kernel


def as_id(cpad):
    return f'Cpad{cpad}-{"pix" + str(cpad // 4) if cpad <= 16 else "generic"}'


def as_splits(cpad):
    """(Ca, Cb): Ca + Cb == Cpad, Ca + Cb < Cpad, and Cb = 0 (b is None)"""
    return [(cpad - 3, 3), (cpad - 3, 1), (cpad - 1, 0)]


AS_REPS = [1, 3]
AS_HW = [(1, 1), (9, 11)]     # HW = 1 and 99
AS_B = 2


def as_inputs(cpad, ca, cb, hw):
    H, W = hw
    seed = 14000 + 13 * cpad + ca + H * W
    return dict(a=rand((AS_B, ca, H, W), seed), b=rand((AS_B, cb, H, W), seed + 1) if cb else None,
                m=torch.rand((AS_B, 1, H, W), generator=torch.Generator().manual_seed(seed + 2)))


def as_reference(a, b, m, reps, cpad):
    """-> NHWC (reps * B, H, W, cpad): cat(a, b * m) zero padded, the batch repeated"""
    B, ca, H, W = a.shape
    parts = [a]
    if b is not None:
        parts.append(b * m if m is not None else b)
    used = sum(p.shape[1] for p in parts)
    parts.append(torch.zeros((B, cpad - used, H, W)))
    return torch.cat(parts, 1).repeat(reps, 1, 1, 1).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ dmh_diff_mean / dmh_loss_combine
# C * HW = 1, 255, 16384 (one element per thread of the 64 x 256), 16385 and 6 * 40 * 56; with fewer than 16129 elements some
# of a sample's 64 partial blocks own none
DM_SHAPES = [(1, 1, 1), (3, 5, 17), (4, 64, 64), (5, 29, 113), (6, 40, 56)]
DM_B = [3, 70]            # 70: two blocks of diff_final_kernel
DM_FACTOR = 6.0           # rounding of the difference (1), of the square (2 + 1), of the mask product (1), of the result (1)
LC_B = [1, 3, 70]
LC_FACTOR = 3.0


def dm_id(case):
    (C, H, W), B = case
    return f'{C}x{H * W}={C * H * W}-B{B}'


DM_CASES = [(s, B) for s in DM_SHAPES for B in DM_B]


def dm_inputs(case):
    (C, H, W), B = case
    seed = 15000 + C * H * W % 977 + B
    gen = torch.Generator().manual_seed(seed + 2)
    # mask values in (0.25, 1.25) with a third of them zero: a mask read at the wrong pixel changes the mean
    m = (torch.rand((B, 1, H, W), generator=gen) + 0.25) * (torch.rand((B, 1, H, W), generator=gen) > 1 / 3)
    return dict(a=rand((B, C, H, W), seed), b=rand((B, C, H, W), seed + 1), m=m.contiguous())


def dm_terms(a, b, m, squared):
    d = a - b
    v = d * d if squared else d.abs()
    return v if m is None else m * v


def dm_reference(a, b, m, squared):
    """-> (ref, bound) float64 (B,): the per-sample mean of m * |a - b| (or m * (a - b)^2) over (C, H, W).  Every term is
    non-negative, so the relative roundings of the terms carry over to the sum; the kernel accumulates in f64 and rounds once"""
    ref = dm_terms(a.double(), b.double(), None if m is None else m.double(), squared).mean((1, 2, 3))
    return ref, DM_FACTOR * U * ref


def dm_fp32(a, b, m, squared, mask_index_wraps=False):
    """the kernel's statement in torch: the terms in fp32, their sum in float64, one rounding.
    mask_index_wraps: the WRONG kernel whose mask is indexed by the element i instead of the pixel i % HW"""
    B, C, H, W = a.shape
    if mask_index_wraps and m is not None:
        flat = m.reshape(-1)
        idx = (torch.arange(B)[:, None] * H * W + torch.arange(C * H * W)[None, :]) % flat.numel()
        m = flat[idx].reshape(B, C, H, W)
    return (dm_terms(a, b, m, squared).double().sum((1, 2, 3)) / (C * H * W)).float()


def lc_inputs(B):
    """per-sample losses, photometric terms and weights: all positive, as the loss terms they stand for"""
    gen = torch.Generator().manual_seed(16000 + B)
    return tuple(torch.rand((B,), generator=gen) + 0.05 for _ in range(3))


def lc_reference(l, ph, w):
    """-> (ref, bound): mean(l) + mean(w * ph); the kernel rounds each product, each mean and the sum once in fp32"""
    a, p = l.double().mean(), (w.double() * ph.double()).mean()
    return a + p, LC_FACTOR * U * (a.abs() + p.abs())


def lc_fp32(l, ph, w):
    return (l.double().mean().float() + (w * ph).double().mean().float())


# ------------------------------------------------------------------ elementwise kernels
EW_B = 3
EW_PER = [1, 255, 257]
EW_COMBOS = [(y, d, c) for y in (False, True) for d in (False, True) for c in (False, True)]


def ew_inputs(per):
    """x, y spread over both sides of +-1; per-sample coefficients with no special value"""
    seed = 17000 + per
    gen = torch.Generator().manual_seed(seed + 2)
    co = lambda: (torch.rand((EW_B,), generator=gen) * 0.9 + 0.3)
    return dict(x=rand((EW_B, per), seed, 1.5), y=rand((EW_B, per), seed + 1, 1.5), ca=co(), cb=co(), dv=co())


def lincomb_fp32(x, ca, y=None, cb=None, dv=None, clamp=False):
    """rows_lincomb_kernel's op order: two rounded products, one add, one divide, the clamp"""
    v = ca[:, None] * x
    if y is not None:
        v = v + cb[:, None] * y
    if dv is not None:
        v = v / dv[:, None]
    return v.clamp(-1.0, 1.0) if clamp else v


def u8_table():
    """fp32: every k / 255 with its two fp32 neighbours (768 values), and the two edge values of test_affine_uint8_qsample
    that are not among them (0.5 -> 127.5, 0.999999): 770 distinct entries"""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    tab = np.concatenate([np.nextafter(k, np.float32(-np.inf)), k, np.nextafter(k, np.float32(np.inf)),
                          np.array([0.5, 0.999999], dtype=np.float32)])
    assert tab.dtype == np.float32
    return tab


def u8_reference(tab, nearest=False):
    """numpy's fp32 product truncated to uint8 (nearest: the WRONG export that rounds)"""
    p = tab * np.float32(255)
    assert p.dtype == np.float32
    return (np.rint(p) if nearest else p).astype(np.uint8)


# ------------------------------------------------------------------ embeddings
SIN_DIMS = [2, 6, 64, 130]
FOURIER_HALVES = [1, 8, 16, 33]
EMB_ROWS = [1, 5, 37]


def emb_times(R):
    """int64 (R,): starts with 123456, 0, 1, 999, then timesteps below 1000"""
    rest = torch.randint(0, 1000, (R,), generator=torch.Generator().manual_seed(18000 + R)).tolist()
    return torch.tensor(([123456, 0, 1, 999] + rest)[:R], dtype=torch.int64)


def sin_freq(dim):
    half = dim // 2
    return torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / max(half - 1, 1)))


def sin_reference(t, freq):
    """float64 sin / cos of the fp32 argument fl(t) * f  -> (R, dim)"""
    arg = (t.float()[:, None] * freq[None, :]).double()
    return torch.cat([arg.sin(), arg.cos()], 1)


def fourier_reference(t, w):
    """-> (R, 2 * half + 1) float64: (fl(t), sin, cos) of the fp32 argument ((t * w) * 2) * pi"""
    tf = t.float()
    arg = (((tf[:, None] * w[None, :]) * torch.tensor(2.0)) * torch.tensor(math.pi, dtype=torch.float32)).double()
    return torch.cat([tf.double()[:, None], arg.sin(), arg.cos()], 1)


SSG_N = [4, 1020, 1028]     # one thread, 255 and 257 quads: the second block of a row has one thread at work
