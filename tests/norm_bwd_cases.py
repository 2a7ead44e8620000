"""Case tables, inputs and CPU references shared by tests/test_norm_backward_host.py (no GPU) and
tests/test_gpu_norm_backward.py (-m gpu): the normalisation-backward, small-GEMM and row-softmax kernels, each alone.

Reference: torch autograd of the plain operation on the CPU in float64, from the same fp32 inputs.
Yardstick: the same plain operation through torch autograd on the CPU in float32; e32 = its error against the float64
reference, max abs error over the reference's max abs (as `_rel` of tests/test_gpu_backward.py).
Gate of a kernel output: error against float64 <= max(FLOOR, 10 * e32) — 10x is the project's rule,
FLOOR is the gate tests/test_gpu_backward.py gives dmh_chan_layernorm_backward.  CAP bounds e32 on the host, so that no
gate can exceed 10 * CAP.  dmh_sum_over_batch and dmh_bgemm are checked per element against bounds derived from the
standard summation / dot-product error analysis instead (`sum_over_batch_bound`, `bgemm_reference`)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from gpu_util import rand

EPS = 1e-5
FLOOR = 5e-6
CAP = 2e-5
U = 2.0 ** -24          # fp32 unit roundoff


SCALE_FLOOR = 1e-30    # a reference smaller than this everywhere (the fp32 yardstick of it is exactly zero) is measured against it


def rel(got, ref):
    """max |got - ref| over max |ref|, in float64; max |ref| is floored at SCALE_FLOOR (`check` says when that happens)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(SCALE_FLOOR)).item()


def gate(e32):
    return max(FLOOR, 10.0 * e32)


def check(name, got, ref64, ref32):
    """print the [parity] line of one kernel output and hold it to its gate; -> (error, e32, gate)"""
    e32 = rel(ref32, ref64)
    err = rel(got, ref64) if bool(torch.isfinite(got).all()) else float('inf')
    g = gate(e32)
    floored = ref64.abs().max().item() < SCALE_FLOOR
    print(f'[parity] {name}: err={err:.3e} e32={e32:.3e} gate={g:.3e} ref_absmax={ref64.abs().max().item():.3e}' +
          (f' (reference below {SCALE_FLOOR:.0e}: err, e32 and gate are absolute, in units of {SCALE_FLOOR:.0e})' if floored else ''))
    assert err <= g, f'{name}: error {err:.3e} of the reference scale, fp32 autograd on the CPU has {e32:.3e}, gate {g:.3e}'
    return err, e32, g


def _autograd(fn, leaves, dout, dtype):
    """gradients of fn(*leaves) in dtype (None leaves are passed through and get None back)"""
    xs = [None if t is None else t.detach().to(dtype).requires_grad_(True) for t in leaves]
    out = fn(*xs)
    gs = iter(torch.autograd.grad(out, [x for x in xs if x is not None], dout.to(dtype)))
    return [None if x is None else next(gs) for x in xs]


# ------------------------------------------------------------------ GroupNorm -> (scale + 1, shift) -> SiLU
GN_SHAPES = [  # B, C, groups, H, W
    (2, 64, 8, 16, 16),     # HW = 256: exactly one chunk
    (3, 64, 8, 19, 23),     # HW = 437: ragged second chunk; B = 3 for the batch sum
    (1, 24, 8, 3, 3),       # C/4 = 6: 252 active threads, fewer pixels than pixel lanes
    (2, 48, 8, 17, 16),     # C/4 = 12
    (1, 512, 8, 4, 4),      # two pixel lanes
    (1, 1024, 8, 3, 3),     # C/4 = 256, 128 channels per group: the finalize wave strides
    (1, 2048, 8, 2, 3),     # the quad loop of the reduce kernel runs twice
    (2, 8, 8, 5, 7),        # one channel per group
]
GN_KIND_SHAPE = (3, 64, 8, 19, 23)
GN_KINDS = ['unit', 'offset30', 'scale1e-4', 'scale1e4', 'saturated']
GN_CASES = [(s, 'unit', ss) for s in GN_SHAPES for ss in (False, True)] + \
           [(GN_KIND_SHAPE, k, ss) for k in GN_KINDS[1:] for ss in (False, True)]
GN_FINALIZE_CASES = [((3, 64, 8, 19, 23), 1, False), ((3, 64, 8, 19, 23), 5, True),
                     ((1, 1024, 8, 3, 3), 1, True), ((1, 1024, 8, 3, 3), 5, False)]   # shape, tiles, with ss


def gn_id(case):
    (B, C, G, H, W), kind, ss = case
    return f'{B}x{C}g{G}x{H}x{W}-{kind}-{"ss" if ss else "noss"}'


def gn_op(y, gamma, beta, ss, groups):
    h = F.group_norm(y, groups, gamma, beta, EPS)
    if ss is not None:
        c = y.shape[1]
        h = h * (ss[:, :c, None, None] + 1) + ss[:, c:, None, None]
    return F.silu(h)


def gn_coef(y, gamma, beta, ss, groups):
    """what dmh_gn_finalize folds (the comment at the top of csrc/norm_backward.hip), in y's dtype:
    a = rstd*gamma*(s+1), c = (beta - mean*rstd*gamma)*(s+1) + t, and (mean, rstd) per (sample, group)"""
    B, C = y.shape[:2]
    yg = y.reshape(B, groups, -1)
    mean = yg.mean(2)
    rstd = (yg.var(2, unbiased=False) + EPS).rsqrt()
    mc, rc = mean.repeat_interleave(C // groups, 1), rstd.repeat_interleave(C // groups, 1)
    sp1 = ss[:, :C] + 1 if ss is not None else torch.ones_like(mc)
    t = ss[:, C:] if ss is not None else torch.zeros_like(mc)
    return dict(a=rc * gamma * sp1, c=(beta - mc * rc * gamma) * sp1 + t, mean=mean, rstd=rstd)


def gn_inputs(case):
    """fp32 NCHW inputs.  Channels differ in scale and samples / channels in mean (all of order one), so that a group's
    (mean, rstd) is its own; the kinds then move the whole tensor."""
    (B, C, G, H, W), kind, with_ss = case
    seed = 1000 + 7 * GN_SHAPES.index((B, C, G, H, W))
    sc = 0.75 + 0.75 * torch.rand((1, C, 1, 1), generator=torch.Generator().manual_seed(seed))
    y = rand((B, C, H, W), seed + 1) * sc + 0.5 * rand((B, C, 1, 1), seed + 2)
    gamma, beta = 1 + 0.2 * rand((C,), seed + 3), 0.2 * rand((C,), seed + 4)
    ss = 0.3 * rand((B, 2 * C), seed + 5) if with_ss else None
    dout = rand((B, C, H, W), seed + 6)
    if kind == 'offset30':
        y = y + 30.0 * y.std()
    elif kind == 'scale1e-4':      # variance below eps
        y = y * 1e-4
    elif kind == 'scale1e4':
        y = y * 1e4
    elif kind == 'saturated':      # |z| reaches 95 on both sides: exp(-z) overflows fp32 above 88.7
        z = F.group_norm(y.double(), G, gamma.double(), None, EPS)
        gamma = gamma * (95.0 / min(z.max().item(), -z.min().item()))
    else:
        assert kind == 'unit', kind
    return dict(y=y.contiguous(), gamma=gamma, beta=beta, ss=ss, dout=dout, groups=G)


@functools.lru_cache(maxsize=None)
def gn_reference(case):
    """-> inputs, ref64 / ref32 {dy, dgamma, dbeta, dss}, and coef (B,2,C) / mr (B,groups,2): the float64 formula rounded to
    fp32, so that the backward kernels are tested alone"""
    inp = gn_inputs(case)
    G = inp['groups']
    leaves = (inp['y'], inp['gamma'], inp['beta'], inp['ss'])
    fn = lambda y, g, b, s: gn_op(y, g, b, s, G)
    names = ('dy', 'dgamma', 'dbeta', 'dss')
    ref64 = dict(zip(names, _autograd(fn, leaves, inp['dout'], torch.float64)))
    ref32 = dict(zip(names, _autograd(fn, leaves, inp['dout'], torch.float32)))
    dbl = [None if t is None else t.double() for t in leaves]
    co = gn_coef(*dbl, G)
    coef = torch.stack([co['a'], co['c']], 1).float().contiguous()
    mr = torch.stack([co['mean'], co['rstd']], 2).float().contiguous()
    z = coef[:, 0, :, None, None].double() * dbl[0] + coef[:, 1, :, None, None].double()
    return dict(inp=inp, ref64=ref64, ref32=ref32, coef=coef, mr=mr, zmin=z.min().item(), zmax=z.max().item())


@functools.lru_cache(maxsize=None)
def gn_finalize_reference(fcase):
    """-> the unit-kind gn_reference of the shape, stats (B, tiles, C, 2) = per-tile (sum y, sum y^2) in float64 rounded to
    fp32, and the finalize outputs {a, c, mean, rstd} by the float64 formula (ref64) and by the same formula in fp32 (ref32)"""
    shape, tiles, with_ss = fcase
    r = gn_reference((shape, 'unit', with_ss))
    inp = r['inp']
    B, C = inp['y'].shape[:2]
    yd = inp['y'].double().reshape(B, C, -1)
    parts = torch.tensor_split(yd, tiles, dim=2)
    stats = torch.stack([torch.stack([p.sum(2), (p * p).sum(2)], 2) for p in parts], 1).float().contiguous()
    args = (inp['y'], inp['gamma'], inp['beta'], inp['ss'])
    ref64 = gn_coef(*[None if t is None else t.double() for t in args], inp['groups'])
    ref32 = gn_coef(*args, inp['groups'])
    return dict(back=r, stats=stats, ref64=ref64, ref32=ref32, hw=yd.shape[2])


# ------------------------------------------------------------------ weight standardisation
# OIHW: K = 576, 7, 257, 4608, 588.  (512, 512, 3, 3) is 2.4 M floats, far more than any other case here: it is the widest
# production weight and the one shape at which a thread of ws_backward_kernel walks 18 strided rounds — keep it.
WS_SHAPES = [(64, 64, 3, 3), (3, 7, 1, 1), (5, 257, 1, 1), (512, 512, 3, 3), (8, 12, 7, 7)]
WS_KINDS = ['unit', 'offset30', 'scale1e-6', 'const_row']
WS_CASES = [(s, k) for s in WS_SHAPES for k in WS_KINDS]


def ws_id(case):
    (o, i, kh, kw), kind = case
    return f'{o}x{i * kh * kw}-{kind}'


def ws_op(w):
    m = w.mean(dim=(1, 2, 3), keepdim=True)
    v = w.var(dim=(1, 2, 3), unbiased=False, keepdim=True)
    return (w - m) * (v + EPS).rsqrt()


def ws_inputs(case):
    shape, kind = case
    seed = 2000 + 7 * WS_SHAPES.index(shape)
    o = shape[0]
    w = rand(shape, seed) * (0.5 + torch.rand((o, 1, 1, 1), generator=torch.Generator().manual_seed(seed + 1))) + \
        0.3 * rand((o, 1, 1, 1), seed + 2)
    dwh = rand(shape, seed + 3)
    if kind == 'offset30':
        w = w + 30.0 * w.std()
    elif kind == 'scale1e-6':      # variance far below eps
        w = w * 1e-6
    elif kind == 'const_row':      # var = 0 exactly in one row
        w[o // 2] = 0.37
    else:
        assert kind == 'unit', kind
    return dict(w=w.contiguous(), dwh=dwh)


@functools.lru_cache(maxsize=None)
def ws_reference(case):
    inp = ws_inputs(case)
    (r64,) = _autograd(ws_op, (inp['w'],), inp['dwh'], torch.float64)
    (r32,) = _autograd(ws_op, (inp['w'],), inp['dwh'], torch.float32)
    return dict(inp=inp, ref64=dict(dw=r64), ref32=dict(dw=r32))


# ------------------------------------------------------------------ channel LayerNorm
LN_CASES = [  # C, (B, H, W), kind — what the four cases of test_chan_layernorm_backward do not reach
    (256, (2, 5, 7), 'unit'),       # <64,1>
    (1024, (1, 3, 3), 'unit'),      # <64,4>
    (40, (2, 5, 7), 'unit'),        # ragged in <16,1>
    (260, (1, 4, 5), 'unit'),       # ragged in <64,2>
    (516, (1, 3, 3), 'unit'),       # ragged in <64,4>
    (64, (1, 1, 1), 'unit'),        # a single pixel
    (64, (2, 48, 48), 'unit'),      # 4608 pixels > 256 blocks x 16: the grid-stride loop runs
    (8, (2, 72, 72), 'unit'),       # 10368 pixels > 256 blocks x 32
    (256, (2, 5, 7), 'offset30'),
]


def ln_id(case):
    C, (B, H, W), kind = case
    return f'C{C}-{B}x{H}x{W}-{kind}'


def ln_op(x, g):
    m = x.mean(1, keepdim=True)
    v = x.var(1, unbiased=False, keepdim=True)
    return (x - m) * (v + EPS).rsqrt() * g[None, :, None, None]


def ln_inputs(case):
    C, (B, H, W), kind = case
    seed = 3000 + C + H
    x = rand((B, C, H, W), seed) * 1.5 + 0.3
    if kind == 'offset30':
        x = x + 30 * 1.5
    return dict(x=x, g=1 + 0.2 * rand((C,), seed + 1), dout=rand((B, C, H, W), seed + 2))


@functools.lru_cache(maxsize=None)
def ln_reference(case):
    inp = ln_inputs(case)
    leaves = (inp['x'], inp['g'])
    return dict(inp=inp, ref64=dict(zip(('dx', 'dg'), _autograd(ln_op, leaves, inp['dout'], torch.float64))),
                ref32=dict(zip(('dx', 'dg'), _autograd(ln_op, leaves, inp['dout'], torch.float32))))


# ------------------------------------------------------------------ row softmax
SM_SHAPES = [(1, 1), (5, 63), (7, 64), (3, 65), (9, 1024), (2, 1000)]   # rows, n
SM_KINDS = ['unit', 'spread80', 'equal', 'one_hot200']
SM_CASES = [(s, k) for s in SM_SHAPES for k in SM_KINDS]


def sm_grad_is_zero(case):
    """n = 1 (softmax is the constant 1) and one_hot200 with n > 1 (P is exact 0s and one 1 per row in fp32, the float64
    gradient of the order exp(-200)): dS = P * (dP - sum dP P) is exactly zero in fp32, whatever the order of the sum"""
    (rows, n), kind = case
    return n == 1 or kind == 'one_hot200'


def sm_id(case):
    (rows, n), kind = case
    return f'{rows}x{n}-{kind}'


def sm_inputs(case):
    (rows, n), kind = case
    seed = 4000 + 3 * n + rows
    gen = torch.Generator().manual_seed(seed)
    if kind == 'unit':
        s = rand((rows, n), seed + 1)
    elif kind == 'spread80':       # the max subtraction matters
        s = (torch.rand((rows, n), generator=gen) * 2 - 1) * 80
    elif kind == 'equal':
        s = torch.full((rows, n), 0.7)
    else:                          # one logit 200 above the rest: the others underflow to exactly 0 in fp32
        assert kind == 'one_hot200', kind
        s = rand((rows, n), seed + 1)
        s[torch.arange(rows), torch.randint(0, n, (rows,), generator=gen)] += 200.0
    return dict(s=s.contiguous(), dp=rand((rows, n), seed + 2))


@functools.lru_cache(maxsize=None)
def sm_reference(case):
    """-> P and dS by float64 (ref64) and float32 (ref32) autograd of softmax(S); p32 = the float64 P rounded to fp32, what
    the backward kernel is given"""
    inp = sm_inputs(case)
    out = {}
    for name, dt in (('ref64', torch.float64), ('ref32', torch.float32)):
        s = inp['s'].to(dt).requires_grad_(True)
        p = s.softmax(dim=-1)
        (ds,) = torch.autograd.grad(p, (s,), inp['dp'].to(dt))
        out[name] = dict(p=p.detach(), ds=ds)
    return dict(inp=inp, p32=out['ref64']['p'].float().contiguous(), **out)


# ------------------------------------------------------------------ derived elementwise bounds
SOB_B = [1, 15, 16, 17, 48, 49, 64, 65, 113, 1024]
SOB_PER = [1, 15, 16, 17, 256]


def sum_over_batch_bound(x):
    """|fl(sum_b x[b][i]) - sum| <= (B - 1) u sum_b |x[b][i]| for ANY order of the B - 1 fp32 additions (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2, to first order); the bound used is B u sum |x|.  -> (ref, bound), float64"""
    xd = x.double()
    return xd.sum(0), x.shape[0] * U * xd.abs().sum(0)


BGEMM_SHAPES = [(1, 1, 1, 1, 1), (33, 31, 7, 2, 3), (64, 32, 63, 1, 4), (5, 70, 2, 3, 1), (32, 32, 33, 1, 1)]  # M N K nbo nbi
BGEMM_ALPHAS = [1.0, -0.37]


def ulp32(x):
    """one fp32 unit in the last place of |x| (float64 tensor; 0 -> 0)"""
    _, e = torch.frexp(x.abs().float())
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), (e - 24).to(torch.int32)))


def bgemm_reference(a, b, alpha):
    """a (.., M, K), b (.., K, N) fp32 -> (ref, bound) in float64 for C = alpha * a @ b computed in fp32: a dot product of K
    terms accumulated in any order is within K u sum |a||b| (Higham, section 3.1); K + 1 leaves room for the rounding of
    the products, the factor 2 for the matrix instruction's internal pairing of the two k it takes at once; the final
    multiplication by alpha (the fp32 value the kernel receives) rounds once more: one fp32 ulp of the reference"""
    K = a.shape[-1]
    al = float(np.float32(alpha))
    ref = al * (a.double() @ b.double())
    bound = 2.0 * (K + 1) * U * abs(al) * (a.double().abs() @ b.double().abs()) + ulp32(ref)
    return ref, bound


def bgemm_inputs(shape):
    M, N, K, nbo, nbi = shape
    seed = 5000 + M + 3 * N + 5 * K
    return rand((nbo, nbi, M, K), seed), rand((nbo, nbi, K, N), seed + 1)
