"""Case tables, inputs and CPU references shared by tests/test_conv_fwd_host.py (no GPU) and tests/test_gpu_conv_fwd.py
(-m gpu): every kernel instance dmh_conv2d dispatches to (csrc/conv.hip, csrc/conv_f16x3.hip), each alone.

Reference: the plain operation in float64 torch on the CPU, from the same fp32 inputs — nearest x2 upsample where asked,
SiLU(a*x+b) on source 0 where in_coef is given (zero padding applies to the ACTIVATED tensor), F.conv2d with the pad rule of
`ref_conv` (tests/test_gpu_kernels.py), + bias, + res or + SiLU(ra*res+rb).
Yardstick: the same formula in fp32 torch on the CPU.  The affine a*x+b of the prologue and of the residual is one fused
multiply-add there, as the kernels document theirs (fmaf): a GroupNorm folded into (a, b) cancels in a*x+b, and a product
rounded on its own would make the yardstick of the 'offset mean' construction 1e3 times worse than any of the kernels.
Both are measured PER OUTPUT CHANNEL (the weight scale is per output channel; a global maximum hides a small-scale channel):
e32_c = max |ref32 - ref64| over channel c / max |ref64| over channel c (floored at SCALE_FLOOR), err_c likewise;
gate: err_c <= max(FLOOR, 10 * e32_c) — FLOOR, CAP and the 10x rule are those of tests/norm_bwd_cases.py;
the host file holds every e32_c under CAP, and every channel well enough conditioned to have a scale (`host_condition`: a
channel whose few outputs all cancel gets another draw of its weight row, decided on the CPU by the references alone).
GroupNorm partials are checked per 8 x 16 stat tile against `stat_reference`.

Data contract (header of csrc/conv_f16x3.hip): an operand keeps 22 significant bits while it is within 2^18 of the running
block maximum of its workgroup; smaller values lose bits in proportion.  The kinds below scale whole 32-channel chunks, so a
value that falls below that window sits next to one 2^18 larger in the same dot product and does not matter to the output."""
import functools
import zlib

import torch
import torch.nn.functional as F

from gpu_util import rand
from norm_bwd_cases import CAP, FLOOR, SCALE_FLOOR, U, gate, gn_coef, rel   # noqa: F401  (re-exported to the two test files)

KC = 32                # input channels per chunk (csrc/conv_f16x3.hip)
STAT_TH, STAT_TW = 8, 16     # stat tile of every default instance (EpilogueRows::write_stats_grid, the stride-2 igemm tiles)
PRO_GROUPS = 4         # GroupNorm groups of the prologue cases (divides every C0 used with a prologue)

# id -> k, stride, upsample2 as handed to PackedConv, subpixel, workgroup tile (TH, TW) in output pixels (up2: on the low-
# resolution grid).  Restated here as LN_LADDER (tests/fwd_glue_cases.py) restates its ladder: there is no export to read.
INSTANCES = {
    '3x3n': dict(k=3, s=1, ups=0, sub=True, tile=(16, 16)),     # conv_f16x3_kernel<3,3,1,0,16,16,4,1> (PACKPW)
    '3x3w': dict(k=3, s=1, ups=0, sub=True, tile=(8, 16)),      # <3,3,1,0,8,16,2,2>
    'up1n': dict(k=3, s=1, ups=1, sub=False, tile=(16, 16)),    # <3,3,1,1,16,16,4,1>
    'up1w': dict(k=3, s=1, ups=1, sub=False, tile=(8, 16)),     # <3,3,1,1,8,16,2,2>
    'up2': dict(k=3, s=1, ups=1, sub=True, tile=(4, 16)),       # <2,2,1,3,4,16,4,1>: four parities
    '1x1n': dict(k=1, s=1, ups=0, sub=True, tile=(16, 16)),     # <1,1,1,0,16,16,4,1> (FIN epilogue)
    '1x1w': dict(k=1, s=1, ups=0, sub=True, tile=(8, 16)),      # <1,1,1,0,8,16,2,2>
    's2dn': dict(k=4, s=2, ups=0, sub=True, tile=(16, 16)),     # <2,2,1,2,16,16,4,1> over the space-to-depth view
    's2dw': dict(k=4, s=2, ups=0, sub=True, tile=(8, 16)),      # <2,2,1,2,8,16,2,2>
    '4x4i': dict(k=4, s=2, ups=0, sub=True, tile=(8, 16)),      # conv_igemm_kernel<4,4,2,0,16,8,16>
    '2x2i': dict(k=2, s=2, ups=0, sub=True, tile=(8, 16)),      # conv_igemm_kernel<2,2,2,0,16,8,16>
    '7x7p': dict(k=7, s=1, ups=0, sub=True, tile=(16, 16)),     # conv_f16x3_kernel<7,7,1,4,16,16,4,1>: two taps per K slice
    '7x7': dict(k=7, s=1, ups=0, sub=True, tile=(16, 16)),      # <7,7,1,0,16,16,4,1>
}
F16 = [i for i in INSTANCES if not i.endswith('i')]      # the eleven conv_f16x3_kernel instances
NO_STATS = ('up2',)
NO_CONCAT = ('up2', 's2dn', 's2dw', '7x7p')               # (a second source sends s2d shapes to 4x4i and 7x7p shapes to 7x7)
NO_PROLOGUE = ('s2dn', 's2dw')


def instance_of(k, s, ups, sub, C0, C1, Cout):
    """the dispatch of dmh_conv2d / dmh_f16x3_launch / PackedConv under the default DMH_CONV3_VARIANT, restated"""
    wide = Cout % 128 == 0
    if k == 3 and ups:
        return 'up2' if (sub and C1 == 0 and Cout % 64 == 0 and C0 % 4 == 0) else ('up1w' if wide else 'up1n')
    if k == 3:
        return '3x3w' if wide else '3x3n'
    if k == 1:
        return '1x1w' if wide else '1x1n'
    if k == 4:
        return ('s2dw' if wide else 's2dn') if (C0 % 32 == 0 and C1 == 0) else '4x4i'
    if k == 2:
        return '2x2i'
    assert k == 7, k
    return '7x7p' if (C0 <= 16 and C1 == 0) else '7x7'


def out_hw(inst, H, W):
    d = INSTANCES[inst]
    if d['ups']:
        return 2 * H, 2 * W
    return (H // 2, W // 2) if d['s'] == 2 else (H, W)


# ------------------------------------------------------------------ the case table
# a case: (instance, B, H, W, C0, C1, Cout, options, kind) with H, W the INPUT size; options a '+'-joined subset of OPTION_WORDS
OPTION_WORDS = ('nobias', 'res', 'rescoef', 'stats', 'incoef', 'inbound', 'inboundinf')
KINDS = ('unit', 'perchan', 'grow', 'shrink', 'jump01', 'jump10', 'zero-chunk', 'zero-sample', 'outlier', 'tiny', 'huge',
         'pro-huge', 'pro-offset', 'pro-outlier')


def base_channels(inst):
    """(C0, C1, Cout) of the geometry, option and row-subset rows: two chunks (one ragged), two cout tiles where the
    instance can have them"""
    wide = INSTANCES[inst]['tile'] == (8, 16) and inst not in ('4x4i', '2x2i')
    c0 = {'s2dn': 32, 's2dw': 32, '7x7p': 12, '7x7': 20}.get(inst, 36)
    return c0, 0, 256 if wide else (128 if inst == 'up2' else 68)


def geometries(inst):
    """name -> input (H, W): one output pixel, a ragged sub-tile, exactly one workgroup tile, one tile + 1 both ways, the two
    strips across two tiles, and a 2 x 3-tile grid (B = 1: 12 workgroups with two cout tiles, >= 8 and no multiple of 8)"""
    d = INSTANCES[inst]
    TH, TW = d['tile']
    if inst == 'up2':                        # tiles on the low-resolution grid = the input
        g = dict(px=(1, 1), ragged=(3, 7), tile=(TH, TW), tile1=(TH + 1, TW + 1), stripH=(TH + 1, 1), stripW=(1, TW + 1),
                 deal=(TH + 1, 2 * TW + 1))
    elif d['ups']:                           # output = 2 x input: the smallest output is 2 x 2
        g = dict(px=(1, 1), ragged=(3, 7), tile=(TH // 2, TW // 2), tile1=(TH // 2 + 1, TW // 2 + 1), stripH=(TH // 2 + 1, 1),
                 stripW=(1, TW // 2 + 1), deal=(TH // 2 + 1, TW + 1))
    elif d['s'] == 2:
        g = dict(px=(2, 2), ragged=(10, 14), tile=(2 * TH, 2 * TW), tile1=(2 * TH + 2, 2 * TW + 2), stripH=(2 * TH + 2, 2),
                 stripW=(2, 2 * TW + 2), deal=(2 * TH + 2, 4 * TW + 2))
        if d['k'] == 4:                      # odd sizes: the last input row / column is read by no tap
            g.update(px3=(3, 3), ragged_odd=(11, 15))
    else:
        g = dict(px=(1, 1), ragged=(5, 7), tile=(TH, TW), tile1=(TH + 1, TW + 1), stripH=(TH + 1, 1), stripW=(1, TW + 1),
                 deal=(TH + 1, 2 * TW + 1))
    return g


def channel_rows(inst):
    """(C0, C1, Cout): one ragged chunk, one full, full + ragged, three (odd chunk counts: the mxslot ping-pong and the load_b
    clamp past the last chunk); the concats; every Cout tiling"""
    _, _, co = base_channels(inst)
    if inst in ('s2dn', 's2dw'):
        rows = [(32, 0, co), (96, 0, co)] + [(32, 0, c) for c in ((4, 64, 132) if inst == 's2dn' else (128,))]
    elif inst == '7x7p':
        rows = [(c, 0, co) for c in (4, 12, 16)] + [(12, 0, c) for c in (4, 64, 132)]
    elif inst == '7x7':
        rows = [(20, 0, co), (36, 0, co), (8, 8, co)] + [(20, 0, c) for c in (4, 64, 132)]
    else:
        c0s = (4, 36) if inst == '4x4i' else (4, 32, 36, 96)      # (4x4 / s2 with C0 % 32 == 0 and one source is s2d)
        rows = [(c, 0, co) for c in c0s]
        if inst not in NO_CONCAT:
            rows += [(4, 4, co), (36, 20, co), (32, 64, co)]
        if inst == 'up2':
            rows += [(36, 0, 64), (36, 0, 256)]
        elif co == 256:
            rows += [(36, 0, 128)]
        else:
            rows += [(36, 0, c) for c in (4, 64, 132)]
    return rows


def options(inst):
    """every option set dmh_conv2d accepts for the instance; the last is prologue + res_coef + stats together"""
    st = [] if inst in NO_STATS else ['stats']
    opts = ['nobias', '', 'res', 'rescoef'] + st + ['+'.join(['res'] + st), '+'.join(['rescoef'] + st)]
    if inst not in NO_PROLOGUE:
        opts += ['incoef', 'incoef+inbound', 'incoef+inboundinf', '+'.join(['incoef', 'inbound', 'rescoef'] + st)]
    return list(dict.fromkeys(opts))


def kinds(inst):
    """(kind, C0, C1, Cout): the dynamic-range kinds on >= 2 chunks (s2d: the four parities of 32 channels are its chunks)"""
    _, _, co = base_channels(inst)
    if inst == '7x7p':                       # one chunk: nothing for a running maximum to do
        return [(k, 12, 0, co) for k in ('perchan', 'zero-sample', 'outlier', 'tiny', 'huge')]
    c0 = {'s2dn': 32, 's2dw': 32, '7x7': 36, '4x4i': 68}.get(inst, 96)
    out = [(k, c0, 0, co) for k in ('perchan', 'grow', 'shrink', 'zero-chunk', 'zero-sample', 'outlier', 'tiny', 'huge')]
    if inst not in NO_CONCAT:
        cc = (8, 8) if inst == '7x7' else (36, 20)
        out += [(k, cc[0], cc[1], co) for k in ('jump01', 'jump10')]
    if inst in ('3x3n', '3x3w', '1x1n', '1x1w', 'up1n', 'up1w'):
        out += [(k, 36, 0, co) for k in ('pro-huge', 'pro-offset', 'pro-outlier')]
    return out


def _cases():
    cs = []
    for inst in INSTANCES:
        c0, c1, co = base_channels(inst)
        geo = geometries(inst)
        st = '' if inst in NO_STATS else 'stats'
        for name, (H, W) in geo.items():
            for B in ((1,) if name == 'deal' else (1, 3)):
                cs.append((inst, B, H, W, c0, c1, co, st, 'unit'))
        H, W = geo['tile1']
        for (a, b, c) in channel_rows(inst):
            cs.append((inst, 3, H, W, a, b, c, st, 'unit'))
        for o in options(inst):
            cs.append((inst, 3, H, W, c0, c1, co, o, 'unit'))
        for (k, a, b, c) in kinds(inst):
            o = '' if (k in ('tiny', 'huge') or not st) else st
            if k.startswith('pro-'):
                o = 'incoef+inbound'
            cs.append((inst, 3, H, W, a, b, c, o, k))
    # Hout == 33 (34 behind an upsample) with >= 2 cout tiles: xcd == 1 with gridDim.y > 1 (launch_f16x3)
    cs += [('3x3n', 1, 33, 16, 36, 0, 132, 'stats', 'unit'), ('3x3w', 1, 33, 16, 96, 0, 256, 'stats', 'unit'),
           ('1x1n', 1, 33, 16, 36, 0, 132, 'stats', 'unit'), ('1x1w', 1, 33, 16, 96, 0, 256, 'stats', 'unit'),
           ('up1n', 1, 17, 8, 36, 0, 132, 'stats', 'unit'), ('up1w', 1, 17, 8, 96, 0, 256, 'stats', 'unit'),
           ('up2', 1, 17, 8, 36, 0, 128, '', 'unit'),
           ('s2dn', 1, 66, 32, 32, 0, 132, 'stats', 'unit'), ('s2dw', 1, 66, 32, 32, 0, 256, 'stats', 'unit'),
           ('7x7p', 1, 33, 16, 12, 0, 132, 'stats', 'unit'), ('7x7', 1, 33, 16, 20, 0, 132, 'stats', 'unit')]
    return list(dict.fromkeys(cs))


CASES = _cases()
# the PACKPW limit: the second tile row has the full 18-row halo, so the packed relative offset reaches 17 * Win + 17 = 65518
PACKPW_CASE = ('3x3n', 1, 33, 3853, 4, 0, 4, 'stats', 'unit')


def case_id(case):
    inst, B, H, W, C0, C1, Cout, opt, kind = case
    cin = f'{C0}+{C1}' if C1 else f'{C0}'
    return f'{inst}-B{B}-{H}x{W}-{cin}to{Cout}-{opt or "bias"}-{kind}'


def opt_set(case):
    return frozenset(w for w in case[7].split('+') if w)


def workgroups(case):
    """(workgroups of the launch, cout tiles) of an f16x3 case"""
    inst, B, H, W, C0, C1, Cout = case[:7]
    TH, TW = INSTANCES[inst]['tile']
    ho, wo = (H, W) if inst == 'up2' else out_hw(inst, H, W)
    ct = -(-Cout // (128 if (TH, TW) == (8, 16) else 64))
    return B * -(-ho // TH) * -(-wo // TW) * ct, ct


# ------------------------------------------------------------------ inputs
REDRAWN_SEEDS = (2, 5, 6, 7, 8)     # weight, bias, res, res_coef: what a redraw of an output channel replaces


def _seed(case, salt=0, attempt=0):
    return (zlib.crc32(case_id(case).encode()) + 7919 * salt + 104729 * attempt) % (2 ** 31)


def chunk_scales(kind, n0, n1):
    """per-chunk activation scale of source 0 (n0 chunks) and source 1 (n1)"""
    n = n0 + n1
    if kind in ('grow', 'shrink'):
        s = [10.0 ** (-4 + 7 * i / max(n - 1, 1)) for i in range(n)]      # 1e-4 .. 1e3: every chunk raises the maximum
        s = s if kind == 'grow' else s[::-1]
    elif kind in ('jump01', 'jump10'):       # the rescale falls on the source boundary
        lo, hi = (1e-3, 1e3) if kind == 'jump01' else (1e3, 1e-3)
        s = [lo] * n0 + [hi] * n1
    elif kind == 'zero-chunk':
        s = [1.0] * n
        s[n // 2] = 0.0
    else:
        s = [{'tiny': 1e-18, 'huge': 1e18}.get(kind, 1.0)] * n
    return s[:n0], s[n0:]


def _scaled(x, scales, inst):
    """x (B, C, H, W) times its chunk's scale; s2d: chunk = (pixel parity, 32 channels), parity (py, px) = ((y+1)&1, (x+1)&1)
    of the shifted space-to-depth view (header of csrc/conv_f16x3.hip)"""
    B, C, H, W = x.shape
    if inst in ('s2dn', 's2dw'):
        per = C // KC
        ys, xs, cs = (torch.arange(H) + 1) % 2, (torch.arange(W) + 1) % 2, torch.arange(C) // KC
        idx = (ys[:, None, None] * 2 + xs[None, :, None]) * per + cs[None, None, :]            # (H, W, C)
        return x * torch.tensor(scales, dtype=torch.float32)[idx].permute(2, 0, 1)[None]
    sc = torch.tensor(scales, dtype=torch.float32).repeat_interleave(KC)[:C]
    return x * sc[None, :, None, None]


def fma32(a, x, b):
    """fl32(a * x + b) with one rounding (fmaf): the product of two fp32 numbers is exact in float64"""
    return (a.double() * x.double() + b.double()).float()


def conv_inputs(case, attempt=0):
    """fp32 CPU tensors, activations NCHW: x0, x1, w (Cout, C0 + C1, k, k), bias, res, res_coef (B, 2, Cout), in_coef
    (B, 2, C0), gamma / beta (the GroupNorm whose fold in_coef is) — None where the case has none.
    attempt: another draw of everything that belongs to one output channel (weight row, bias, residual), the activations
    staying what they are: `conv_reference` gives every channel its first draw that meets the host conditions"""
    inst, B, H, W, C0, C1, Cout, _, kind = case
    d, o = INSTANCES[inst], opt_set(case)
    k = d['k']
    ho, wo = out_hw(inst, H, W)
    sd = lambda i: _seed(case, i, attempt if i in REDRAWN_SEEDS else 0)
    n0 = 4 * C0 // KC if inst in ('s2dn', 's2dw') else -(-C0 // KC)
    s0, s1 = chunk_scales(kind, n0, -(-C1 // KC))
    x0 = _scaled(rand((B, C0, H, W), sd(0)), s0, inst)
    x1 = _scaled(rand((B, C1, H, W), sd(1)), s1, inst) if C1 else None
    amax = max(s0 + s1)
    if kind == 'zero-sample':
        x0[1] = 0
        if x1 is not None:
            x1[1] = 0
    elif kind == 'outlier':                  # the + 1 pixel: inside the last tile, in the halo of its three neighbours
        x0[0, 1, H - 1, W - 1] = 1e4
    elif kind == 'pro-huge':
        x0 = x0 * 1e12 + 3e11
    elif kind == 'pro-offset':               # |mean| >> sigma: the producer declines to bound (+inf)
        x0 = x0 * 0.01 + 300.0
    elif kind == 'pro-outlier':
        x0[0, 3, min(5, H - 1), min(7, W - 1)] = 4.0e4
        x0[B - 1, C0 - 1, H - 1, W - 1] = -9.0e3
    w = rand((Cout, C0 + C1, k, k), sd(2), ((C0 + C1) * k * k) ** -0.5)
    wsc = torch.ones(Cout)
    if kind == 'perchan':
        wsc = 10.0 ** (torch.arange(Cout) % 9 - 4).float()
        w = w * wsc[:, None, None, None]
    inp = dict(x0=x0.contiguous(), x1=x1, w=w.contiguous(), bias=None, res=None, res_coef=None, in_coef=None, gamma=None, beta=None)
    oscale = amax
    if 'incoef' in o:                        # the fold of a real GroupNorm (gn_coef): a*x+b is of order one whatever x is,
        g, be = 1 + 0.3 * rand((C0,), sd(3)), 0.2 * rand((C0,), sd(4))       # and dmh_gn_finalize_bound can bound it
        c = gn_coef(x0, g, be, None, PRO_GROUPS)
        inp.update(in_coef=torch.stack([c['a'], c['c']], 1).contiguous(), gamma=g, beta=be)
        oscale = 1.0
    if 'nobias' not in o:
        inp['bias'] = 0.1 * rand((Cout,), sd(5)) * oscale * wsc
    if 'res' in o or 'rescoef' in o:
        inp['res'] = rand((B, Cout, ho, wo), sd(6)) * oscale * wsc[None, :, None, None]
    if 'rescoef' in o:
        inp['res_coef'] = torch.stack([1 + 0.2 * rand((B, Cout), sd(7)), 0.3 * rand((B, Cout), sd(8))], 1).contiguous()
    return inp


# ------------------------------------------------------------------ references
def conv_formula(inp, inst, dt, magnitude=False):
    """the reference (dt = float64) or the yardstick (float32): -> (B, Cout, Hout, Wout).
    magnitude: the sum of the absolute values of all terms of every output instead (|x| * |w|, |bias|, |residual term|)"""
    d = INSTANCES[inst]
    k, s = d['k'], d['s']
    aff = (lambda a, x, b: a * x + b) if dt == torch.float64 else fma32
    x0 = inp['x0'].to(dt)
    if inp['in_coef'] is not None:
        c = inp['in_coef'].to(dt)
        x0 = F.silu(aff(c[:, 0, :, None, None], x0, c[:, 1, :, None, None]))
    x = x0 if inp['x1'] is None else torch.cat([x0, inp['x1'].to(dt)], 1)
    if d['ups']:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    pad = k // 2 if s == 1 else (1 if k == 4 else 0)
    ab = (lambda t: t.abs()) if magnitude else (lambda t: t)
    y = F.conv2d(ab(x), ab(inp['w'].to(dt)), None if inp['bias'] is None else ab(inp['bias'].to(dt)), s, pad)
    if inp['res'] is not None:
        r = inp['res'].to(dt)
        if inp['res_coef'] is not None:
            rc = inp['res_coef'].to(dt)
            r = F.silu(aff(rc[:, 0, :, None, None], r, rc[:, 1, :, None, None]))
        y = y + ab(r)
    return y


def conv_plain(inp, inst, dt):
    """conv_formula restated without F.conv2d / F.interpolate / F.silu: the activation written out, the upsample as a
    repeat, the zero border of the ACTIVATED tensor as a copy into zeros (k // 2 at stride 1, 1 for 4x4 / s2, 0 for
    2x2 / s2), the convolution as a sum over taps of strided windows"""
    d = INSTANCES[inst]
    k, s = d['k'], d['s']
    silu = lambda z: z / (1 + torch.exp(-z))
    aff = (lambda a, x, b: a * x + b) if dt == torch.float64 else fma32
    x0 = inp['x0'].to(dt)
    if inp['in_coef'] is not None:
        c = inp['in_coef'].to(dt)
        x0 = silu(aff(c[:, 0, :, None, None], x0, c[:, 1, :, None, None]))
    x = x0 if inp['x1'] is None else torch.cat([x0, inp['x1'].to(dt)], 1)
    if d['ups']:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    pad = {1: k // 2, 2: 1 if k == 4 else 0}[s]
    B, C, H, W = x.shape
    xp = torch.zeros((B, C, H + 2 * pad, W + 2 * pad), dtype=dt)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    ho, wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    w = inp['w'].to(dt)
    y = torch.zeros((B, w.shape[0], ho, wo), dtype=dt)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s]
            y += torch.einsum('bchw,oc->bohw', win, w[:, :, ky, kx])
    if inp['bias'] is not None:
        y = y + inp['bias'].to(dt)[None, :, None, None]
    if inp['res'] is not None:
        r = inp['res'].to(dt)
        if inp['res_coef'] is not None:
            rc = inp['res_coef'].to(dt)
            r = silu(aff(rc[:, 0, :, None, None], r, rc[:, 1, :, None, None]))
        y = y + r
    return y


def chan_scale(ref64):
    return ref64.abs().amax((0, 2, 3)).clamp_min(SCALE_FLOOR)


def chan_rel(got, ref64):
    """(Cout,): max |got - ref| over max |ref|, per output channel, in float64 (`rel` of tests/norm_bwd_cases.py per channel)"""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    return (got - ref64).abs().amax((0, 2, 3)) / chan_scale(ref64)


MAX_ATTEMPTS = 48
KAPPA_MARGIN = 8.0


def channel_kappa(mag64, ref64):
    """(Cout,): the largest sum of |terms| of any output of the channel over the channel's largest |output|"""
    return mag64.amax((0, 2, 3)) / chan_scale(ref64)


def _measure(inp, inst):
    ref64, ref32 = conv_formula(inp, inst, torch.float64), conv_formula(inp, inst, torch.float32)
    e32 = chan_rel(ref32, ref64)
    g = e32.mul(10.0).clamp_min(FLOOR)
    kappa = channel_kappa(conv_formula(inp, inst, torch.float64, magnitude=True), ref64)
    return dict(inp=inp, ref64=ref64, ref32=ref32, e32=e32, gate=g, kappa=kappa)


def host_condition(m):
    """(Cout,) bool.  The two conditions on the INPUTS of a case, decided on the CPU by the references alone:
      e32_c < CAP                       (tests/norm_bwd_cases.py; CAP / 2 while drawing)
      KAPPA_MARGIN * kappa_c * U <= gate_c
    The second is the contract every fp32-accumulating kernel has: a channel's error is measured against the channel's largest
    |output| S_c, but ONE rounding of a term of an output already costs up to u * sum |terms| = u * kappa_c * S_c.  A channel
    with few outputs that all cancel (one output pixel, one sample: kappa in the hundreds for one channel in a hundred) has no
    scale to be measured against — whatever the order of accumulation, the fp32 yardstick's own included, whose e32 is one
    sample of that order.  Such a channel gets another draw of its weight row, bias and residual."""
    return (m['e32'] < CAP / 2) & (KAPPA_MARGIN * m['kappa'] * U <= m['gate'])


def _reference(case):
    inst = case[0]
    m = _measure(conv_inputs(case, 0), inst)
    need = ~host_condition(m)
    draw = torch.zeros_like(need, dtype=torch.int64)
    if bool(need.any()):
        inp = {k: (None if v is None else v.clone()) for k, v in m['inp'].items()}
        for attempt in range(1, MAX_ATTEMPTS):
            alt = _measure(conv_inputs(case, attempt), inst)
            take = need & host_condition(alt)
            inp['w'][take] = alt['inp']['w'][take]
            if inp['bias'] is not None:
                inp['bias'][take] = alt['inp']['bias'][take]
            if inp['res'] is not None:
                inp['res'][:, take] = alt['inp']['res'][:, take]
            if inp['res_coef'] is not None:
                inp['res_coef'][:, :, take] = alt['inp']['res_coef'][:, :, take]
            draw[take] = attempt
            need = need & ~take
            if not bool(need.any()):
                break
        m = _measure(inp, inst)
    m['draw'] = draw
    return m


@functools.lru_cache(maxsize=None)
def conv_reference(case):
    """-> inp, ref64, ref32 (B, Cout, Hout, Wout), e32 and gate (Cout,)"""
    return _reference(case)


def packpw_reference():
    """the Win = 3853 case (2 MB per tensor): not cached"""
    return _reference(PACKPW_CASE)


def stat_reference(ref64, g, th=STAT_TH):
    """ref64 (B, Cout, Ho, Wo), g (Cout,) the channels' gates -> (ref, bound) float64 (B, tiles, Cout, 2), tile =
    srow * tilesX + tx over th x 16 stat tiles: the sum and the sum of squares of the reference over the tile's n valid pixels.
    Bound: every output within g_c S_c of the reference (S_c the channel maximum) and an fp32 sum of m = n + 8 terms in any
    order (the kernel adds a lane's 8 rows, 4 row groups, 2 waves; gamma_m = m U / (1 - m U): Higham, Accuracy and Stability
    of Numerical Algorithms, section 4.2):
      |d sum|   <= n g S + gamma_m sum |ref|          |d sumsq| <= 2 n g S^2 (1 + g) + gamma_m sum ref^2"""
    B, Cc, ho, wo = ref64.shape
    ty, tx = -(-ho // th), -(-wo // STAT_TW)
    S = chan_scale(ref64)
    ref = torch.zeros((B, ty * tx, Cc, 2), dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for r in range(ty):
        for c in range(tx):
            t = ref64[:, :, r * th:(r + 1) * th, c * STAT_TW:(c + 1) * STAT_TW]
            n = t.shape[2] * t.shape[3]
            m = n + 8
            gm = m * U / (1 - m * U)
            ref[:, r * tx + c, :, 0] = t.sum((2, 3))
            ref[:, r * tx + c, :, 1] = (t * t).sum((2, 3))
            bound[:, r * tx + c, :, 0] = n * g * S + gm * t.abs().sum((2, 3))
            bound[:, r * tx + c, :, 1] = 2 * n * g * S * S * (1 + g) + gm * (t * t).sum((2, 3))
    return ref, bound


# ------------------------------------------------------------------ known answers
# tap probes: weight = one 1.0 at tap (ky, kx) with o == c, fp16-representable input -> the output is the (upsampled) input
# shifted with zero padding, bit for bit: every product is exact and every other term an exact zero
PROBE_INSTANCES = ('3x3n', '3x3w', 'up1n', 'up1w', 'up2', '7x7p', '7x7', 's2dn', 's2dw', '4x4i')


def probe_channels(inst):
    """C = Cout == Cin of the probe (a multiple of 4 that lands on the instance)"""
    return {'3x3n': 4, '3x3w': 128, 'up1n': 4, 'up1w': 128, 'up2': 64, '7x7p': 4, '7x7': 20, 's2dn': 32, 's2dw': 128, '4x4i': 4}[inst]


def probe_input(inst, B=2):
    """(B, C, H, W) at the one-tile-plus-one shape: small integers / 8, no zero among them"""
    C = probe_channels(inst)
    H, W = geometries(inst)['tile1']
    v = torch.randint(1, 256, (B, C, H, W), generator=torch.Generator().manual_seed(4200 + C)).float()
    sign = torch.randint(0, 2, (B, C, H, W), generator=torch.Generator().manual_seed(4300 + C)).float() * 2 - 1
    return v * sign / 8


def probe_weight(inst, ky, kx):
    C, k = probe_channels(inst), INSTANCES[inst]['k']
    w = torch.zeros((C, C, k, k))
    w[torch.arange(C), torch.arange(C), ky, kx] = 1.0
    return w


def probe_expected(inst, x, ky, kx):
    """out[y][x] = X[s*y + ky - pad][s*x + kx - pad] (zero outside), X the nearest-upsampled input where the instance upsamples"""
    d = INSTANCES[inst]
    k, s = d['k'], d['s']
    X = x.repeat_interleave(2, 2).repeat_interleave(2, 3) if d['ups'] else x
    pad = k // 2 if s == 1 else (1 if k == 4 else 0)
    B, C, H, W = X.shape
    ho, wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    out = torch.zeros((B, C, ho, wo), dtype=x.dtype)
    for oy in range(ho):
        iy = s * oy + ky - pad
        if 0 <= iy < H:
            ix = s * torch.arange(wo) + kx - pad
            ok = (ix >= 0) & (ix < W)
            out[:, :, oy, ok] = X[:, :, iy, ix[ok]]
    return out
