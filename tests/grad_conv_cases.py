"""Case table, inputs and CPU references shared by tests/test_grad_conv_host.py (no GPU) and tests/test_gpu_grad_conv.py
(-m gpu): every weight-gradient kernel of csrc/conv_backward.hip alone, at the shapes where its index branches are decided.

    dW[o][c][ky][kx] = sum_{b,y,x} dy[b][y][x][o] * X[b][y + ky - pad][x + kx - pad][c]          db[o] = sum_{b,y,x} dy[b][y][x][o]

with X the input as the convolution saw it: cat(src0, src1), SiLU(a*src0 + b) where in_coef is given, the nearest x2 repeat
of the stored input for `ups`, the stored (H+1) x (W+1) tensor of the 2x2 'valid' form, the pixel-unshuffled view (channel
c*4 + py*2 + px of pixel (y, x) is x[2y+py][2x+px][c]) for dmh_conv_unshuffle_wgrad.

Reference: that formula written out in float64 torch on the CPU from the same fp32 inputs (a sum over taps of einsums of
shifted windows; tests/test_grad_conv_host.py holds it to float64 autograd of F.conv2d).  Yardstick: the same in fp32, the
affine a*x + b of the prologue as ONE fused multiply-add (`fma32` of tests/conv_fwd_cases.py), as the kernels have it.

Unit of measurement, after each kernel's accuracy contract:
  w1, w7, wu (exact fp32 MFMA, fp32 accumulation: every product is right to one rounding, whatever the scale of its row or
      column): every output-channel ROW of dW (all c, all taps) against the row's own maximum AND every input-channel COLUMN
      (all o, all taps) against the column's own maximum;
  w3, w2 (fp16 pieces with ONE block scale per workgroup: dY over its 64 output channels, X over its 32 input channels):
      every (64-o tile, 32-c block, tap) against that block's own maximum; where the reference block is exactly zero (a tap
      that only meets padding) the kernel's is too;
  db: per channel against the channel's sum of |dy| — what the rounding error of a sum is proportional to (Higham, Accuracy
      and Stability of Numerical Algorithms, section 4.2); the sum itself may cancel to nothing.
Gate of a unit: err <= max(FLOOR, 10 * e32_unit), FLOOR, CAP and U those of tests/norm_bwd_cases.py;
the host file holds every e32_unit of every case under CAP.  Per-(o, c)-pair units are NOT used: a pair's few taps cancel
(e32 up to 1e-2)."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from conv_fwd_cases import fma32
from gpu_util import rand
from norm_bwd_cases import CAP, FLOOR, SCALE_FLOOR, U, gn_coef   # noqa: F401  (re-exported to the two test files)

TH, TW = 4, 16          # the item: pixels of dy a workgroup stages at a time (csrc/conv_backward.hip)
OT, CB = 64, 32         # output channels per workgroup; input channels per fp16-piece workgroup (NCBW = 2 blocks of 16)
PRO_GROUPS = 4          # GroupNorm groups of the coef cases (divides every C0 used with a prologue)

# id -> taps per axis, padding, kernel family, input channels per partial-block column tile (wgrad_cw), modes
INSTANCES = {
    'w3': dict(k=3, pad=1, family='f16', cw=64, modes=('plain', 'concat', 'coef', 'ups')),   # conv_wgrad_f16x3_kernel<3,1,2> + reduce_v2
    'w2': dict(k=2, pad=0, family='f16', cw=64, modes=('plain',)),                           # conv_wgrad_f16x3_kernel<2,0,2> + reduce_v2
    'w1': dict(k=1, pad=0, family='fp32', cw=64, modes=('plain', 'concat', 'coef')),         # conv_wgrad_kernel<1,4,0> + reduce<false>
    'w7': dict(k=7, pad=3, family='fp32', cw=16, modes=('plain', 'concat', 'coef')),         # conv_wgrad_kernel<7,1,3> + reduce<false>
    'wu': dict(k=1, pad=0, family='fp32', cw=64, modes=('plain',)),                          # conv_wgrad_kernel<1,4,0,true> + reduce<true>
}
F16 = ('w3', 'w2')
FP32 = ('w1', 'w7', 'wu')


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the dispatch and the split plan, restated
def wgrad_splits(nitems, npairs):
    return max(1, min(512 // max(npairs, 1), nitems))


def wgrad_splits_f16(nitems, npairs):
    s = 512 // (2 * max(npairs, 1))
    if s >= 8:
        s = s // 8 * 8
    return max(1, min(s, nitems))


def instance_of(entry, k):
    """the dispatch of dmh_conv_wgrad (KH = 2, 3: the fp16-piece kernel; 1, 7: the exact-fp32 kernel) / the unshuffle entry"""
    if entry == 'dmh_conv_unshuffle_wgrad':
        return 'wu'
    assert entry == 'dmh_conv_wgrad'
    return {1: 'w1', 2: 'w2', 3: 'w3', 7: 'w7'}[k]


def cin_of(case):
    """input channels as the kernel sees them (wu: the 4C of the unshuffled view)"""
    return 4 * case[5] if case[0] == 'wu' else case[5] + case[6]


def plan(case):
    """grid, splits, items per split and workspace floats of the case's launch"""
    inst, _, B, H, W, C0, C1, Cout = case[:8]
    d = INSTANCES[inst]
    k, cin = d['k'], cin_of(case)
    otiles, ctiles = cdiv(Cout, OT), cdiv(cin, d['cw'])
    npairs = otiles * ctiles
    nitems = B * cdiv(H, TH) * cdiv(W, TW)
    s32, s16 = wgrad_splits(nitems, npairs), wgrad_splits_f16(nitems, npairs)
    f16 = d['family'] == 'f16'
    nsplit = s16 if f16 else s32
    ns_ws = s32 if inst == 'wu' else (max(s32, s16) if k <= 3 else s32)      # (the size function does not know the branch)
    per = cdiv(nitems, nsplit)
    # fp16-piece: two workgroups of 32 channels per (pair, split); the second returns at once where its block starts past Cin
    idle = sum(1 for ct in range(ctiles) if ct * 64 + 32 >= cin) * otiles * nsplit if f16 else 0
    return dict(family=d['family'], otiles=otiles, ctiles=ctiles, npairs=npairs, nitems=nitems, nsplit=nsplit, per=per,
                grid=(nsplit, npairs * (2 if f16 else 1)), idle=idle,
                part_w=nsplit * npairs * 64 * 64 * k * k, part_b=nsplit * otiles * 64,
                workspace=ns_ws * npairs * 64 * 64 * k * k + ns_ws * otiles * 64)


# ------------------------------------------------------------------ the case table
# a case: (instance, mode, B, H, W, C0, C1, Cout, kind, db, seed) — H, W the size of dy; C0 / C1 the two sources' channels
# (wu: C0 = C of the stored x (B, 2H, 2W, C)); db: False = the entry gets db = NULL; seed: another draw of the inputs
GEOMETRIES = [(1, 1), (3, 7), (4, 16), (5, 17), (5, 1), (1, 17), (9, 33)]
UPS_GEOMETRIES = [(2, 2), (4, 16), (6, 18), (6, 2), (2, 18)]
CH_HW, CH_B = (5, 17), 3                     # the channel and kind rows: one item + 1 both ways, three samples
CONCATS = [(4, 4), (36, 20), (32, 64), (60, 8)]
KINDS = ('unit', 'ochan', 'cchan', 'otile', 'cblock', 'cblockw', 'jump')


def base_channels(inst):
    """(C0, Cout) of the geometry rows: two input-channel blocks with a ragged second, two output tiles with a ragged second"""
    return {'w7': 20, 'wu': 20}.get(inst, 36), 68


def _cases():
    cs = []
    add = lambda inst, mode, B, hw, c0, c1, co, kind='unit', db=True, seed=0: cs.append(
        (inst, mode, B, hw[0], hw[1], c0, c1, co, kind, db, seed))
    for inst in INSTANCES:
        c0, co = base_channels(inst)
        for hw in GEOMETRIES:
            for B in (1, 3):
                add(inst, 'plain', B, hw, c0, 0, co)
        if inst == 'w3':
            for hw in UPS_GEOMETRIES:
                for B in (1, 3):
                    add(inst, 'ups', B, hw, c0, 0, co)
            for c in (4, 68):
                add(inst, 'ups', CH_B, (6, 18), c, 0, co)
        # channels
        if inst in ('w3', 'w2', 'w1'):
            for c in (4, 16, 32, 36, 64, 68, 132):
                add(inst, 'plain', CH_B, CH_HW, c, 0, 68)
            for o in (4, 64, 132):
                add(inst, 'plain', CH_B, CH_HW, 36, 0, o)
            if inst != 'w2':
                for (a, b) in CONCATS:
                    add(inst, 'concat', CH_B, CH_HW, a, b, 68)
        elif inst == 'w7':
            for c in (4, 12, 16, 20, 36):
                add(inst, 'plain', CH_B, CH_HW, c, 0, 68)
            for o in (4, 132):
                add(inst, 'plain', CH_B, CH_HW, 20, 0, o)
            add(inst, 'concat', CH_B, CH_HW, 8, 8, 68)
        else:
            for c in (4, 8, 16, 20, 36):
                for o in (4, 68, 132):
                    add(inst, 'plain', CH_B, CH_HW, c, 0, o)
        if 'coef' in INSTANCES[inst]['modes']:
            for c in (4, 36, 68):
                add(inst, 'coef', CH_B, CH_HW, c, 0, 68)
        add(inst, 'plain', CH_B, CH_HW, c0, 0, co, db=False)
        # kinds
        if inst in FP32:
            for kind in ('ochan', 'cchan'):
                add(inst, 'plain', CH_B, CH_HW, c0, 0, co, kind)
        else:
            for kind in ('otile', 'cblock', 'cblockw'):
                add(inst, 'plain', CH_B, CH_HW, 68, 0, 132, kind)
        if inst == 'w3':
            for (a, b) in ((32, 64), (36, 20)):          # the source boundary on / inside a 32-channel block
                add(inst, 'concat', CH_B, CH_HW, a, b, 68, 'jump')
    return list(dict.fromkeys(cs))


CASES = _cases()


def case_id(case):
    inst, mode, B, H, W, C0, C1, Cout, kind, db, seed = case
    cin = f'{C0}+{C1}' if C1 else f'{C0}'
    return f'{inst}-{mode}-B{B}-{H}x{W}-{cin}to{Cout}-{kind}' + ('' if db else '-nodb') + (f'-s{seed}' if seed else '')


def stored_hw(case):
    """size of the stored input src0 / src1 / x for a dy of H x W"""
    inst, mode, _, H, W = case[:5]
    if inst == 'wu':
        return 2 * H, 2 * W
    if inst == 'w2':
        return H + 1, W + 1
    if mode == 'ups':
        assert H % 2 == 0 and W % 2 == 0
        return H // 2, W // 2
    return H, W


# ------------------------------------------------------------------ inputs
def _seed(case, salt):
    return (zlib.crc32(case_id(case).encode()) + 7919 * salt) % (2 ** 31)


def chan_decades(n):
    """10^(i % 9 - 4) for channel i"""
    return 10.0 ** (torch.arange(n) % 9 - 4).float()


def wgrad_inputs(case):
    """fp32 CPU tensors, NHWC: dy (B, H, W, Cout), x0 (B, Hin, Win, C0), x1 or None, in_coef (B, 2, C0) or None"""
    inst, mode, B, H, W, C0, C1, Cout, kind, _, _ = case
    hin, win = stored_hw(case)
    dy = rand((B, H, W, Cout), _seed(case, 0))
    x0 = rand((B, hin, win, C0), _seed(case, 1))
    x1 = rand((B, hin, win, C1), _seed(case, 2)) if C1 else None
    if kind == 'ochan':
        dy = dy * chan_decades(Cout)
    elif kind == 'cchan':
        assert x1 is None
        x0 = x0 * chan_decades(C0)
    elif kind == 'otile':                    # one scale per workgroup's 64 output channels
        dy = dy * torch.tensor([1.0, 1e-3, 1e3]).repeat_interleave(OT)[:Cout]
    elif kind in ('cblock', 'cblockw'):      # one scale per workgroup's 32 input channels; 'cblockw': wide enough that ONE
        assert x1 is None                    # scale for all channels would miss the gate (tests/test_grad_conv_host.py)
        sc = [1e3, 1.0, 1e-3] if kind == 'cblock' else [1e4, 1.0, 1e-4]
        x0 = x0 * torch.tensor(sc).repeat_interleave(CB)[:C0]
    elif kind == 'jump':
        x1 = x1 * 1e3
    else:
        assert kind == 'unit', kind
    coef = None
    if mode == 'coef':                       # the fold of a real GroupNorm, as in tests/conv_fwd_cases.py
        g, be = 1 + 0.3 * rand((C0,), _seed(case, 3)), 0.2 * rand((C0,), _seed(case, 4))
        c = gn_coef(x0.permute(0, 3, 1, 2), g, be, None, PRO_GROUPS)
        coef = torch.stack([c['a'], c['c']], 1).contiguous()
    return dict(dy=dy.contiguous(), x0=x0.contiguous(), x1=x1, in_coef=coef)


# ------------------------------------------------------------------ references
def unshuffled(x, order='py*2+px'):
    """(B, 2H, 2W, C) -> (B, H, W, 4C), channel c*4 + py*2 + px of pixel (y, x) = x[2y+py][2x+px][c]"""
    B, H2, W2, C = x.shape
    v = x.reshape(B, H2 // 2, 2, W2 // 2, 2, C)                      # b y py x px c
    perm = (0, 1, 3, 5, 2, 4) if order == 'py*2+px' else (0, 1, 3, 5, 4, 2)
    return v.permute(*perm).reshape(B, H2 // 2, W2 // 2, 4 * C)


def conv_input(inp, case, dt, order='py*2+px'):
    """X as the convolution saw it, NHWC, unpadded"""
    inst, mode = case[:2]
    x0 = inp['x0'].to(dt)
    if inp['in_coef'] is not None:
        c = inp['in_coef'].to(dt)
        a, b = c[:, 0, None, None, :], c[:, 1, None, None, :]
        x0 = F.silu(a * x0 + b if dt == torch.float64 else fma32(a, x0, b))
    x = x0 if inp['x1'] is None else torch.cat([x0, inp['x1'].to(dt)], 3)
    if mode == 'ups':
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    if inst == 'wu':
        x = unshuffled(x, order)
    return x


def wgrad_formula(inp, case, dt, dy=None, order='py*2+px'):
    """-> dW (Cout, Cin, k, k), db (Cout,) in dt; dy: another output gradient than inp's (the mutations)"""
    d = INSTANCES[case[0]]
    k, pad = d['k'], d['pad']
    X = conv_input(inp, case, dt, order)
    dy = (inp['dy'] if dy is None else dy).to(dt)
    B, H, W, Cout = dy.shape
    Xp = F.pad(X, (0, 0, pad, pad, pad, pad))
    assert Xp.shape[1] == H + k - 1 and Xp.shape[2] == W + k - 1, (tuple(Xp.shape), H, W, k)
    dw = torch.zeros((Cout, X.shape[3], k, k), dtype=dt)
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = torch.einsum('bhwo,bhwc->oc', dy, Xp[:, ky:ky + H, kx:kx + W])
    return dw, dy.sum((0, 1, 2))


def block_amax(t):
    """(Cout, Cin, k, k) -> (o tiles, c blocks, taps): max |t| over each workgroup block of the fp16-piece kernels"""
    co, ci, k, _ = t.shape
    ot, cb = cdiv(co, OT), cdiv(ci, CB)
    p = torch.zeros((ot * OT, cb * CB, k * k), dtype=t.dtype)
    p[:co, :ci] = t.reshape(co, ci, k * k).abs()
    return p.view(ot, OT, cb, CB, k * k).amax((1, 3))


def unit_errors(inst, dw, db, dw64, db64, dysum):
    """-> {unit name: errors of (dw, db) against the float64 (dw64, db64), one per unit, each over its unit's scale}"""
    dw = dw.detach().double().cpu()
    assert dw.shape == dw64.shape, (tuple(dw.shape), tuple(dw64.shape))
    dwd = (dw - dw64).abs()
    out = {}
    if inst in FP32:
        out['rows'] = dwd.amax((1, 2, 3)) / dw64.abs().amax((1, 2, 3)).clamp_min(SCALE_FLOOR)
        out['cols'] = dwd.amax((0, 2, 3)) / dw64.abs().amax((0, 2, 3)).clamp_min(SCALE_FLOOR)
    else:
        out['blocks'] = (block_amax(dwd) / block_amax(dw64).clamp_min(SCALE_FLOOR)).reshape(-1)
    if db is not None:
        out['db'] = (db.detach().double().cpu() - db64).abs() / dysum.clamp_min(SCALE_FLOOR)
    return out


def _measure(case):
    inp = wgrad_inputs(case)
    dw64, db64 = wgrad_formula(inp, case, torch.float64)
    dw32, db32 = wgrad_formula(inp, case, torch.float32)
    dysum = inp['dy'].double().abs().sum((0, 1, 2))
    e32 = unit_errors(case[0], dw32, db32, dw64, db64, dysum)
    gates = {u: e.mul(10.0).clamp_min(FLOOR) for u, e in e32.items()}
    return dict(inp=inp, dw64=dw64, db64=db64, dw32=dw32, db32=db32, dysum=dysum, e32=e32, gate=gates)


@functools.lru_cache(maxsize=None)
def wgrad_reference(case):
    """-> inp, dw64, db64, dw32, db32, e32 and gate per unit name (one entry per unit)"""
    return _measure(case)


def worst(case, r, dw, db):
    """-> (worst err / gate over every unit, description of where) of a kernel's (dw, db); inf where something is not
    finite or a block whose reference is exactly zero is not"""
    inst = case[0]
    if not bool(torch.isfinite(dw).all()) or (db is not None and not bool(torch.isfinite(db).all())):
        return float('inf'), 'not finite (never written?)'
    if inst in F16:
        zero = block_amax(r['dw64']) == 0
        if bool((block_amax(dw.detach().double().cpu())[zero] != 0).any()):
            return float('inf'), 'a block whose reference is exactly zero is not'
    errs = unit_errors(inst, dw, db if case[9] else None, r['dw64'], r['db64'], r['dysum'])
    best = (-1.0, '')
    for u, e in errs.items():
        ratio = e / r['gate'][u]
        i = int(ratio.argmax())
        if ratio[i].item() > best[0]:
            best = (ratio[i].item(), f'{u}[{i}]: err={e[i].item():.3e} e32={r["e32"][u][i].item():.3e} gate={r["gate"][u][i].item():.3e}')
    return best


def worst_e32(r):
    return {u: e.max().item() for u, e in r['e32'].items()}


# ------------------------------------------------------------------ known answers
def onehot_positions(H, W):
    """the first and the last pixel, and at 5 x 17 the pixels on either side of the item corner"""
    pos = [(0, 0), (H - 1, W - 1)]
    if (H, W) == (5, 17):
        pos += [(3, 15), (4, 16)]
    return list(dict.fromkeys(pos))


def eighths(shape, seed):
    """non-zero fp16-representable values k / 8, |k| <= 255"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(1, 256, shape, generator=g).float()
    return v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) / 8


def onehot_expected(case, x, b, y0, x0, o0):
    """dW (Cout, Cin, k, k) for dy = one 1.0 at (b, y0, x0, o0): row o0 is the k x k window of the input as the convolution
    saw it around that pixel (zeros where it leaves the image), every other row 0 — written with indices, not with
    wgrad_formula"""
    inst, mode, _, H, W, _, _, Cout = case[:8]
    d = INSTANCES[inst]
    k, pad = d['k'], d['pad']
    cin = cin_of(case)
    dw = torch.zeros((Cout, cin, k, k))
    if inst == 'wu':
        C = x.shape[3]
        for c in range(C):
            for py in (0, 1):
                for px in (0, 1):
                    dw[o0, c * 4 + py * 2 + px, 0, 0] = x[b, 2 * y0 + py, 2 * x0 + px, c]
        return dw
    hv, wv = (H + 1, W + 1) if inst == 'w2' else (H, W)
    for ky in range(k):
        for kx in range(k):
            y, xx = y0 + ky - pad, x0 + kx - pad
            if 0 <= y < hv and 0 <= xx < wv:
                dw[o0, :, ky, kx] = x[b, y // 2, xx // 2] if mode == 'ups' else x[b, y, xx]
    return dw


# ------------------------------------------------------------------ the two-piece fp16 split, emulated
def split2_product(dy, X, sd_exp, sx_exp):
    """float64 arrays: sum over the first axis of d*x as the fp16-piece kernels form it — d1 = fp16(d sd), d2 = fp16(d sd - d1),
    likewise x; d1 x1 + d2 x1 + d1 x2 exactly, unscaled.  dy (n, O), X (n, C); sd_exp / sx_exp: exponents of the block maxima,
    broadcastable to (O,) / (C,)  (scale = 2^(14 - exponent), header of the fp16-piece kernel)"""
    def pieces(v, e):
        s = np.ldexp(1.0, 14 - e)
        v = np.float32(v * s).astype(np.float64)
        h1 = v.astype(np.float16).astype(np.float64)
        h2 = (v - h1).astype(np.float32).astype(np.float16).astype(np.float64)
        return h1, h2, s
    d1, d2, sd = pieces(dy, sd_exp)
    x1, x2, sx = pieces(X, sx_exp)
    acc = d1.T @ x1 + d2.T @ x1 + d1.T @ x2
    return acc / (np.reshape(sd, (-1, 1)) * np.reshape(sx, (1, -1)))


def max_exponent(a):
    """floor(log2(max |a|))"""
    return int(np.floor(np.log2(np.abs(a).max())))


# ------------------------------------------------------------------ composites at their smallest shapes
# (name, B, H, W, C, Cout): H, W the size of x
def _composites():
    cs = []
    for B in (1, 3):
        for C in (4, 36):
            for co in (4, 68):
                for hw in ((2, 2), (4, 4), (10, 14), (34, 34)):
                    cs += [('down', B, hw[0], hw[1], C, co), ('unshuffle', B, hw[0], hw[1], C, co)]
                for hw in ((1, 1), (3, 7), (9, 17)):
                    cs.append(('up', B, hw[0], hw[1], C, co))
    return cs


COMPOSITES = _composites()


def composite_id(c):
    return f'{c[0]}-B{c[1]}-{c[2]}x{c[3]}-{c[4]}to{c[5]}'


def composite_op(name, x, w, b):
    """NCHW"""
    if name == 'down':                       # Downsample: conv 4x4 / stride 2 / pad 1
        return F.conv2d(x, w, b, 2, 1)
    if name == 'up':                         # Upsample: nearest x2 -> conv 3x3
        return F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, b, 1, 1)
    assert name == 'unshuffle'               # DDP Downsample: pixel-unshuffle (channel c*4 + py*2 + px) -> 1x1
    return F.conv2d(F.pixel_unshuffle(x, 2), w, b)


def composite_inputs(c):
    name, B, H, W, C, co = c
    sd = lambda i: (zlib.crc32(composite_id(c).encode()) + 7919 * i) % (2 ** 31)
    wshape = {'down': (co, C, 4, 4), 'up': (co, C, 3, 3), 'unshuffle': (co, 4 * C, 1, 1)}[name]
    x = rand((B, C, H, W), sd(0))
    w = rand(wshape, sd(1), (wshape[1] * wshape[2] * wshape[3]) ** -0.5)
    b = rand((co,), sd(2), 0.1)
    ho, wo = {'down': (H // 2, W // 2), 'up': (2 * H, 2 * W), 'unshuffle': (H // 2, W // 2)}[name]
    dy = rand((B, co, ho, wo), sd(3))
    return dict(x=x, w=w, b=b, dy=dy)


def _grads(name, inp, dt):
    x, w, b = (inp[n].to(dt).requires_grad_(True) for n in ('x', 'w', 'b'))
    return torch.autograd.grad(composite_op(name, x, w, b), (x, w, b), inp['dy'].to(dt))


def composite_errors(got, ref64, dysum):
    """got, ref64: (dx NCHW, dw OIHW, db) -> {dx: per input channel, dw: per output channel, db: per channel over sum |dy|}"""
    dx, dw, db = (g.detach().double().cpu() for g in got)
    rx, rw, rb = ref64
    assert dx.shape == rx.shape and dw.shape == rw.shape and db.shape == rb.shape
    return dict(dx=(dx - rx).abs().amax((0, 2, 3)) / rx.abs().amax((0, 2, 3)).clamp_min(SCALE_FLOOR),
                dw=(dw - rw).abs().amax((1, 2, 3)) / rw.abs().amax((1, 2, 3)).clamp_min(SCALE_FLOOR),
                db=(db - rb).abs() / dysum.clamp_min(SCALE_FLOOR))


@functools.lru_cache(maxsize=None)
def composite_reference(c):
    inp = composite_inputs(c)
    ref64, ref32 = _grads(c[0], inp, torch.float64), _grads(c[0], inp, torch.float32)
    dysum = inp['dy'].double().abs().sum((0, 2, 3))
    e32 = composite_errors(ref32, ref64, dysum)
    return dict(inp=inp, ref64=ref64, ref32=ref32, dysum=dysum, e32=e32,
                gate={u: e.mul(10.0).clamp_min(FLOOR) for u, e in e32.items()})
