"""Case tables, inputs, float64 statements and fp32 yardsticks shared by tests/test_aux_host.py (no GPU) and
tests/test_gpu_aux.py (-m gpu): the loss-gradient kernels (dmh_loss_backward, dmh_loss_backward_ddp), the layout helpers
(dmh_s2d_shift, dmh_d2s, dmh_sumpool2), the dataset kernels (dmh_resize_bilinear_u8, dmh_mask_open_nearest), the geometry
helpers (dmh_pixel_grid, dmh_norm_grid, dmh_homography_flow_points, dmh_homography_flow, dmh_flow_to_image) and the
single-tensor optimiser entries (dmh_sumsq, dmh_gradnorm_finalize, dmh_adam, dmh_ema), each alone.

FLOOR, CAP, rel, gate and check are those of tests/norm_bwd_cases.py: a float64-compared output is held to
max(FLOOR, 10 * e32), e32 = the error of the same formula in fp32 torch on the CPU; the host file
holds every e32 under CAP.  Permutations, fixed-order sums and formulas the kernels keep in the reference's op order are
compared bit for bit with the fp32 statement instead."""
import functools

import numpy as np
import torch

from gpu_util import rand
from norm_bwd_cases import FLOOR, CAP, U, rel, gate, check  # noqa: F401  (re-exported to the two test files)
from oracle import dataset as OD
from oracle import geometry as OG


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ 1. dmh_loss_backward
LB_SHAPES = [       # B, H, W
    (1, 2, 2),      # smallest legal
    (2, 3, 5),      # part of a block
    (3, 16, 16),    # exactly 256 pixels
    (2, 17, 15),    # 255 pixels
    (2, 9, 29),     # 261 pixels: one block and five pixels
]
LB_KINDS = ['zero', 'frac', 'int', 'fold', 'far']
LB_MASKS = ['random', 'ones', 'zeros']
LB_CASES = [(s, k) for s in LB_SHAPES for k in LB_KINDS]
LB_EXACT_SHAPES = [(2, 5, 9), (1, 17, 17)]     # H - 1 and W - 1 powers of two: zero flow gives exact integer coordinates
LB_ABAR = [0.9995, 0.004, 0.31]                # near 1, near 0, in between; rotated by the shape's index


def lb_id(case):
    (B, H, W), kind = case
    return f'{B}x{H}x{W}-{kind}'


def lb_flow(shape, kind, seed):
    B, H, W = shape
    if kind == 'zero':
        return torch.zeros((B, 2, H, W))
    if kind == 'frac':       # leaves the image on every side
        return (torch.rand((B, 2, H, W), generator=_gen(seed)) * 2 - 1) * 6.0
    if kind == 'int':
        return torch.round((torch.rand((B, 2, H, W), generator=_gen(seed)) * 2 - 1) * 3.0)
    if kind == 'far':        # every pixel lands on the last row / column corner: x1ok and y1ok false
        return torch.full((B, 2, H, W), 1000.0)
    assert kind == 'fold', kind     # every pixel is sent to one interior point with fractional parts (0.25, 0.5)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    tx, ty = (W - 1) // 2 + 0.25, (H - 1) // 2 + 0.5
    if ty > H - 1:           # H = 2: the half point between the two rows
        ty = 0.5
    return torch.stack([tx - xs, ty - ys], 1).contiguous()


def lb_mask(shape, mkind, seed):
    B, H, W = shape
    if mkind == 'random':
        return (torch.rand((B, 1, H, W), generator=_gen(seed)) < 0.6).float()
    return torch.full((B, 1, H, W), 1.0 if mkind == 'ones' else 0.0)


def lb_inputs(shape, kind, mkind='random', plant_zeros=False):
    """fp32 inputs of dmh_loss_backward.  ``warped`` is an INPUT of the kernel: it is the oracle's fp32 flow_warp here and is
    taken as given by every statement below.  plant_zeros: every 7th element of ``target`` is ``out``'s and every 5th of
    ``warped`` is ``out[:, :3]``'s, so that the L1 derivative is exactly 0 there."""
    B, H, W = shape
    si = (LB_SHAPES + LB_EXACT_SHAPES).index(shape)
    seed = 7000 + 40 * si + 5 * LB_KINDS.index(kind)
    out, target = rand((B, 6, H, W), seed), rand((B, 6, H, W), seed + 1)
    flow = lb_flow(shape, kind, seed + 2)
    mask = lb_mask(shape, mkind, seed + 3)
    abar = torch.tensor([LB_ABAR[(si + b) % 3] for b in range(B)])
    warped = OG.flow_warp(out[:, 3:].contiguous(), flow)
    if plant_zeros:
        t, o = target.view(-1), out.view(-1)
        t[::7] = o[::7]
        wv, im1 = warped.view(-1), out[:, :3].reshape(-1)
        wv[::5] = im1[::5]
    return dict(out=out, target=target, warped=warped.contiguous(), mask=mask, flow=flow, abar=abar)


def lb_taps(flow):
    """corner indices and the four weights of the warp, from oracle.geometry.warp_coords: fp32 coordinates in the
    reference's op order.  -> x0, y0 (int64), x1ok, y1ok (bool), w, e, n, s (fp32), each (B, H, W)"""
    B, _, H, W = flow.shape
    ix, iy, x0, y0 = OG.warp_coords(flow)
    fx0, fy0 = x0.to(torch.float32), y0.to(torch.float32)
    w, e, n, s = ix - fx0, (fx0 + 1) - ix, iy - fy0, (fy0 + 1) - iy
    x0, y0 = x0.long(), y0.long()
    return dict(x0=x0, y0=y0, x1ok=x0 + 1 <= W - 1, y1ok=y0 + 1 <= H - 1, w=w, e=e, n=n, s=s)


LB_MUTATIONS = ['swap_sw_ne', 'x1ok_dropped', 'x1ok_strict', 'gD_added', 'norm6']


def lb_scatter(gD, taps, mutate=None):
    """transpose of the warp's gather, in gD's dtype: out[b][c][corner] += gD[b][c][p] * weight; a corner one past the last
    row / column is dropped.  Mutations (restated wrong kernels, host file): 'swap_sw_ne' exchanges the s*w and n*e
    weights; 'x1ok_dropped' adds the x0 + 1 tap without its guard, at the flat index y0 * W + x0 + 1 (the first pixel of the
    next row; the one index past the plane is dropped); 'x1ok_strict' drops the last column's valid tap (x0 + 1 < W - 1)"""
    B, Cc, H, W = gD.shape
    dt = gD.dtype
    w, e, n, s = (taps[k].to(dt) for k in 'wens')
    x0, y0, x1ok, y1ok = taps['x0'], taps['y0'], taps['x1ok'], taps['y1ok']
    wne, wsw = (n * e, s * w) if mutate == 'swap_sw_ne' else (s * w, n * e)
    if mutate == 'x1ok_strict':
        x1ok = x0 + 1 < W - 1
    corners = [(y0 * W + x0, s * e, torch.ones_like(x1ok)), (y0 * W + x0 + 1, wne, x1ok),
               ((y0 + 1) * W + x0, wsw, y1ok), ((y0 + 1) * W + x0 + 1, n * w, x1ok & y1ok)]
    if mutate == 'x1ok_dropped':
        corners[1] = (corners[1][0], wne, corners[1][0] < H * W)
    out = torch.zeros((B, Cc, H * W), dtype=dt)
    g = gD.reshape(B, Cc, H * W)
    for idx, wt, ok in corners:
        idx = torch.where(ok, idx, torch.zeros_like(idx)).reshape(B, 1, H * W).expand(B, Cc, H * W)
        wt = torch.where(ok, wt, torch.zeros_like(wt)).reshape(B, 1, H * W)
        out.scatter_add_(2, idx, g * wt)
    return out.reshape(B, Cc, H, W)


def lb_statement(inp, squared, dtype, mutate=None, warped=None):
    """d loss / d out of p_losses (CFG:796-806), loss = mean l(out - target) + mean_b abar_b mean mask l(warped - out[:, :3]),
    in ``dtype`` from the fp32 inputs, ``warped`` taken as given:
        g  = l'(out - target) / (6 B HW),   gD = abar_b mask l'(warped - out[:, :3]) / (3 B HW),   l' = 2 d or sign d
        dout[:, :3] = g - gD,   dout[:, 3:] = g + scatter(gD)
    -> dict(dout, g, gD, scat)"""
    out, target, mask, abar = (inp[k].to(dtype) for k in ('out', 'target', 'mask', 'abar'))
    warped = (inp['warped'] if warped is None else warped).to(dtype)
    B, _, H, W = out.shape
    lp = (lambda d: 2.0 * d) if squared else torch.sign
    g = lp(out - target) / (6.0 * B * H * W)
    gD = abar.view(B, 1, 1, 1) * mask * lp(warped - out[:, :3]) / ((6.0 if mutate == 'norm6' else 3.0) * B * H * W)
    scat = lb_scatter(gD, lb_taps(inp['flow']), mutate)
    dout = g.clone()
    dout[:, :3] = dout[:, :3] + gD if mutate == 'gD_added' else dout[:, :3] - gD
    dout[:, 3:] += scat
    return dict(dout=dout, g=g, gD=gD, scat=scat)


def lb_direct32(inp, squared):
    """g and gD in fp32 torch in the op order of loss_bwd_direct_kernel (products and one division only, so contraction has
    nothing to fuse): n1 = 1 / (B * 6 * HW), g = (2 d) n1 or +-n1; n2 = abar mask / (B * 3 * HW), gD = (2 D) n2 or +-n2"""
    out, target, warped, mask, abar = (inp[k] for k in ('out', 'target', 'warped', 'mask', 'abar'))
    B, _, H, W = out.shape
    one = torch.ones((), dtype=torch.float32)
    n1 = one / torch.tensor(float(B) * 6.0 * float(H * W), dtype=torch.float32)
    n2 = abar.view(B, 1, 1, 1) * mask / torch.tensor(float(B) * 3.0 * float(H * W), dtype=torch.float32)
    d, D = out - target, warped - out[:, :3]
    if squared:
        return 2.0 * d * n1, 2.0 * D * n2
    return torch.sign(d) * n1, torch.sign(D) * n2


@functools.lru_cache(maxsize=None)
def lb_reference(shape, kind, mkind, squared, plant_zeros=False):
    inp = lb_inputs(shape, kind, mkind, plant_zeros)
    return dict(inp=inp, ref64=lb_statement(inp, squared, torch.float64), ref32=lb_statement(inp, squared, torch.float32),
                taps=lb_taps(inp['flow']))


def lb_adjoint(scat, gD, x, wx):
    """both sides of <scatter(gD), x> = <gD, flow_warp(x)> in float64, and the scale sum |gD| |flow_warp(x)| the difference
    is measured against"""
    lhs = (scat.double() * x.double()).sum().item()
    rhs = (gD.double() * wx.double()).sum().item()
    return lhs, rhs, (gD.double().abs() * wx.double().abs()).sum().item()


# ------------------------------------------------------------------ 2. dmh_loss_backward_ddp
DDP_CASES = [(B, per) for B in (1, 3) for per in (1, 255, 256, 257)]
DDP_BLOCK_CAP = 8192                                # blocks of 256 threads dmh_loss_backward_ddp launches at most
DDP_LOOP_CASE = (2, DDP_BLOCK_CAP * 128 + 3)        # total = 8192 * 256 + 6: the smallest launch with a second trip
DDP_SCALES = [1.0, 0.25]


def ddp_inputs(B, per):
    seed = 7600 + B + per % 1000
    out, target = rand((B, per), seed), rand((B, per), seed + 1)
    t, o = target.view(-1), out.view(-1)
    t[::7] = o[::7]                                  # planted exact zeros of the difference
    w = torch.tensor([0.75, 1.5, 0.3125][:B]) + 0.01 * torch.rand((B,), generator=_gen(seed + 2))   # distinct per row
    return dict(out=out, target=target, w=w)


def ddp_statement32(inp, squared, scale):
    """fp32 torch in the op order of ddp_loss_bwd_kernel: inv = 1 / ((float)B * (float)per), n = (scale * w_b) * inv,
    dout = (2 d) n or +-n (sign 0 = 0).  Products only: the kernel is expected to match bit for bit."""
    out, target, w = inp['out'], inp['target'], inp['w']
    B, per = out.shape
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    inv = f(1.0) / (f(B) * f(per))
    n = ((f(scale) * w) * inv).view(B, 1)
    d = out - target
    return 2.0 * d * n if squared else torch.sign(d) * n


# ------------------------------------------------------------------ 3. dmh_s2d_shift, dmh_d2s, dmh_sumpool2
LAYOUT_B = [1, 3]
LAYOUT_HW = [(2, 2), (2, 6), (6, 4), (10, 14)]
LAYOUT_C = [4, 12, 36, 64]      # float4 counts below, at and above one block over the (H, W) above; C / 4 odd and even


def iota(shape):
    """the element's own flat index as a float (exact below 2^24): a misplaced element names itself"""
    n = int(np.prod(shape))
    assert n < 2 ** 24
    return torch.arange(n, dtype=torch.float32).reshape(shape)


def s2d_shift_ref(x):
    """x (B, H, W, C), H and W even -> X (B, H/2 + 1, W/2 + 1, 4C): X[b][cy][cx][(py*2+px)*C + c] =
    x[b][2cy-1+py][2cx-1+px][c], +0.0 outside"""
    B, H, W, C = x.shape
    xp = torch.zeros((B, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    return xp.view(B, H // 2 + 1, 2, W // 2 + 1, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2 + 1, W // 2 + 1, 4 * C)


def d2s_ref(a):
    """a (B, H, W, 4C) -> (B, 2H, 2W, C): out[b][2m+ry][2l+rx][c] = a[b][m][l][(ry*2+rx)*C + c]"""
    B, H, W, C4 = a.shape
    C = C4 // 4
    return a.view(B, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, C)


def sumpool2_ref(a):
    """a (B, 2H, 2W, C) -> (B, H, W, C): (a[2m][2l] + a[2m][2l+1]) + (a[2m+1][2l] + a[2m+1][2l+1]) in a's dtype"""
    B, H2, W2, C = a.shape
    v = a.view(B, H2 // 2, 2, W2 // 2, 2, C)
    return (v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])


def down_weight_as_2x2(w):
    """the 4x4 / stride 2 weight (Cout, C, 4, 4) as the 2x2 weight over the shifted space-to-depth view, (Cout, 4C, 2, 2)
    with channels (py, px, c) and ky = 2 dy + py: the inverse of the reshape at the end of ops.conv_down_backward"""
    cout, c = w.shape[:2]
    return w.view(cout, c, 2, 2, 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(cout, 4 * c, 2, 2)


# ------------------------------------------------------------------ 4. dmh_resize_bilinear_u8, dmh_mask_open_nearest
RESIZE_SIZES = [            # (Hs, Ws), (Hd, Wd)
    ((7, 9), (7, 9)),       # scale 1: the result is src / div exactly
    ((8, 12), (4, 6)),      # exact x2
    ((37, 53), (16, 16)),   # non-integer ratio, down
    ((5, 7), (16, 16)),     # up: both clamp branches on both axes
    ((1, 9), (4, 4)),       # one-pixel source axis
    ((9, 1), (4, 4)),
    ((6, 6), (1, 1)),       # one-pixel destination
]
RESIZE_C = [1, 3, 4]
RESIZE_B = [1, 3]
RESIZE_DIV = [255.0, 1.0]
PLANES, PLANE0, MASK_PLANE = 12, 2, 6      # the (B, 12, Hd, Wd) batch; resize writes planes 2 .. 2 + C, the mask plane 6
MASK_SIZES = RESIZE_SIZES + [((13, 9), (1, 7)), ((13, 9), (7, 1))]     # the 3x3 windows collapse
MASK_KINDS = ['binary', 'floats', 'ones', 'single0', 'single1', 'block3']


def resize_src(B, hs, ws, C, kind='random'):
    if kind == 'random':
        g = np.random.default_rng(7700 + 13 * hs + ws + 3 * C + B)
        return g.integers(0, 256, size=(B, hs, ws, C), dtype=np.uint8)
    return np.full((B, hs, ws, C), 0 if kind == 'zeros' else 255, dtype=np.uint8)


def resize_oracle(src, hd, wd, div):
    """oracle.dataset.resize_linear of src / div (fp32 IEEE division, as the kernel's) per image -> (B, C, hd, wd) fp32"""
    x = src.astype(np.float32) / np.float32(div)
    return np.stack([OD.resize_linear(im, hd, wd).transpose(2, 0, 1) for im in x]).astype(np.float32)


RESIZE_MUTATIONS = ['no_half', 'clamp_at_n', 'fractions_swapped']


def _taps(nd, ns, mutate=None):
    """source index pair and fraction of lin_tap (csrc/dataset.hip), the fraction in fp32; mutations as named"""
    scale = float(ns) / nd
    d = np.arange(nd, dtype=np.float64)
    f = (d * scale if mutate == 'no_half' else (d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo = s < 0
    f[lo], s[lo] = 0.0, 0
    hi = s >= (ns if mutate == 'clamp_at_n' else ns - 1)
    f[hi], s[hi] = 0.0, ns - 1
    s = np.minimum(s, ns - 1)
    return s, np.minimum(s + 1, ns - 1), f


def resize_plain(src, hd, wd, div, dtype=np.float64, mutate=None):
    """plain bilinear interpolation from the kernel's taps, in ``dtype``: (B, C, hd, wd).  float64: the independent
    statement the kernel is held to within 8 * 2^-24 * (255 / div); float32 with a mutation: a restated wrong kernel"""
    B, hs, ws, C = src.shape
    x = (src.astype(np.float32) / np.float32(div)).astype(dtype)
    x0, x1, fx = _taps(wd, ws, mutate)
    y0, y1, fy = _taps(hd, hs, mutate)
    if mutate == 'fractions_swapped':      # (needs hd == wd)
        fx, fy = fy, fx
    fx, fy = fx.astype(dtype), fy.astype(dtype)
    one = dtype(1.0)
    rows = x[:, :, x0] * (one - fx)[None, None, :, None] + x[:, :, x1] * fx[None, None, :, None]
    out = rows[:, y0] * (one - fy)[None, :, None, None] + rows[:, y1] * fy[None, :, None, None]
    return out.transpose(0, 3, 1, 2).astype(dtype)


def resize_bound(div):
    """one rounding in the division and three in each pass, on values no larger than 255 / div"""
    return 8.0 * U * (255.0 / div)


def mask_src(kind, B, hs, ws):
    g = np.random.default_rng(7800 + 17 * hs + ws + B)
    if kind == 'binary':
        return (g.random((B, hs, ws)) < 0.7).astype(np.float32)
    if kind == 'floats':           # min / max are exact on any floats
        return g.standard_normal((B, hs, ws)).astype(np.float32)
    m = np.ones((B, hs, ws), dtype=np.float32)
    if kind == 'ones':             # stays all ones: pixels outside the image are ignored
        return m
    cy, cx = hs // 2, ws // 2
    if kind == 'single0':
        m[:, cy, cx] = 0.0
        return m
    m[:] = 0.0
    if kind == 'single1':          # the opening removes it
        m[:, cy, cx] = 1.0
    else:                          # a 3x3 block of ones (clipped by a small image) survives
        assert kind == 'block3', kind
        m[:, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = 1.0
    return m


def mask_oracle(m, hd, wd):
    return np.stack([OD.dilate3(OD.erode3(OD.resize_nearest(p, hd, wd))) for p in m]).astype(np.float32)


def mask_scipy(m, hd, wd):
    """the same opening by scipy.ndimage on the oracle's nearest resize: an independent statement of the morphology"""
    from scipy import ndimage
    out = []
    for p in m:
        r = OD.resize_nearest(p, hd, wd).astype(np.float64)
        er = ndimage.grey_erosion(r, size=(3, 3), mode='constant', cval=np.inf)
        out.append(ndimage.grey_dilation(er, size=(3, 3), mode='constant', cval=-np.inf))
    return np.stack(out).astype(np.float32)


# ------------------------------------------------------------------ 5. geometry helpers
GRID_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 16), (1, 17, 16)]     # B, H, W
GRID_STARTS = [0.0, 3.0, -0.5]


def pixel_grid_ref(B, H, W, start):
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W) + torch.tensor(start, dtype=torch.float32)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W) + torch.tensor(start, dtype=torch.float32)
    return torch.stack([xs, ys], 1).contiguous()


def norm_grid_ref(v):
    """norm_grid DDP:1292-1299 in fp32 torch: (B, 2, H, W) -> (B, H, W, 2); H = 1 or W = 1 divides by zero as torch does"""
    B, _, H, W = v.shape
    return torch.stack([2.0 * v[:, 0] / (W - 1) - 1.0, 2.0 * v[:, 1] / (H - 1) - 1.0], -1).contiguous()


FLOW_POINTS_CASES = [       # B, divide, Bi, H, W
    (3, 3, 3, 20, 13),      # band height 6: rows 18 and 19 clamp to the last band; 260 points
    (3, 3, 1, 20, 13),
    (3, 3, 3, 3, 85),       # H = divide; 255 points
    (1, 1, 1, 16, 16),      # 256
    (3, 2, 1, 9, 29),       # 261; band height 4, row 8 clamps
    (3, 2, 3, 2, 128),      # H = divide; 256
    (1, 3, 1, 3, 87),       # 261
]


def homographies(shape, seed):
    """float64 homographies near the identity, each its own"""
    g = np.random.default_rng(seed)
    base = np.array([[.02, -.01, 1.5], [.015, -.02, -1.0], [2e-4, -1e-4, 0.]])
    return np.eye(3) + base * g.uniform(-1, 1, tuple(shape) + (3, 3))


def flow_points_inputs(case):
    B, divide, Bi, H, W = case
    seed = 7900 + 11 * H + W + divide
    g = np.random.default_rng(seed)
    idx = np.stack([g.uniform(-3, W + 3, (Bi, H, W)), g.uniform(-3, H + 3, (Bi, H, W)),
                    g.uniform(0.8, 1.25, (Bi, H, W))], 1)             # not a pixel grid; third coordinate != 1
    return homographies((B, divide), seed + 1), idx


def flow_points_ref(Hm, idx):
    """get_flow_np DDP:927-969 in numpy float64: row y uses the homography of band min(y // (H // divide), divide - 1);
    w' += 1e-6 unconditionally"""
    B, divide = Hm.shape[:2]
    Bi, _, H, W = idx.shape
    band = np.minimum(np.arange(H) // (H // divide), divide - 1)
    h = Hm[:, band]                                                    # (B, H, 3, 3)
    x, y, o = (np.broadcast_to(idx[:, k], (B, H, W)) for k in range(3))
    q = [h[:, :, r, 0][:, :, None] * x + h[:, :, r, 1][:, :, None] * y + h[:, :, r, 2][:, :, None] * o for r in range(3)]
    qw = q[2] + 1e-6
    return np.stack([q[0] / qw - x, q[1] / qw - y], 1)


HFLOW_CASES = [(1, 1, 1), (2, 5, 7), (3, 16, 16), (2, 9, 29)]         # B, H, W of dmh_homography_flow
MAX_FLOWS = [256.0, 1.0]


def int_grid(H, W):
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.stack([xs, ys, np.ones_like(xs)], 0)[None]


def edge_flows(max_flow):
    """(N, 2) fp32 flows at the edges of flow_to_image: zero flow with every sign of zero (atan2(0, 0), ss == 0: grey 1);
    flows along +-x and +-y with both signs of the zero component (hue 0, 1/4, 1/2, 3/4); the diagonals; magnitudes at
    max_flow / 8 exactly (saturation 1), one fp32 step below, 1e6 above (the clamp), a generic 0.37 of it, and 1e-30 (its
    square underflows: magnitude 0)"""
    sat = np.float32(max_flow / 8.0)
    mags = [sat, np.nextafter(sat, np.float32(0)), np.float32(sat * 1e6), np.float32(sat * 0.37), np.float32(1e-30)]
    pz, nz = np.float32(0.0), np.float32(-0.0)
    rows = [(pz, pz), (pz, nz), (nz, pz), (nz, nz)]
    for m in mags:
        rows += [(m, pz), (m, nz), (-m, pz), (-m, nz), (pz, m), (nz, m), (pz, -m), (nz, -m),
                 (m, m), (-m, m), (-m, -m), (m, -m)]
    return np.array(rows, dtype=np.float32)


def flow_image_oracle(flow, max_flow):
    """oracle.geometry.flow_to_image per image: flow (B, 2, H, W) fp32 numpy -> (B, 3, H, W) fp32"""
    return np.stack([OG.flow_to_image(f.transpose(1, 2, 0), max_flow).transpose(2, 0, 1) for f in flow]).astype(np.float32)


# ------------------------------------------------------------------ 6. single-tensor optimiser entries
OPT_SIZES = [1, 255, 256, 257, 65536 + 1]      # the last: the first dmh_sumsq launch whose threads take a second element
OPT_STEPS = 3
OPT_MAX_NORMS = [1e6, 1e-3]                     # above and below the norm of every gradient of opt_tensors (host file)
ADAM = dict(lr=1e-3, b1=0.9, b2=0.99, eps=1e-8)
ADAM_ULPS = dict(p=40, m=8, v=12)              # the bars of test_clip_adam_multi_vs_fp64 (tests/test_gpu_wgrad_splits.py)
NORM_REL = 1.5e-7                              # its bar on the norm and the clip coefficient
EMA_DECAYS = [0.9, 0.995, 0.9999]
EMA_ULPS = 2.0          # one rounding each in the difference, the product and the sum; contraction can only remove one


def ulp32_spacing(a):
    """spacing of fp32 numbers at |a| (fp64 tensor); 2^-149 below the normal range"""
    a = a.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def f32(v):
    """the Python float as the fp32 value the C ABI receives"""
    return float(torch.tensor(v, dtype=torch.float32))


def adam_step64(p, m, v, g, coef, step, lr, b1, b2, eps):
    """one torch.optim.Adam step in float64 on the gradient g * coef, with the fp32 betas the C ABI takes ->
    (p, m, v) after the step and the scale of each update, whose fp32 ulp the error is counted in:
    max(|b1 m|, |(1 - b1) g|) for m, likewise for v, max(|p|, |step|) for p (the sums cancel where the terms have opposite
    signs)"""
    f1, f2 = f32(b1), f32(b2)
    bc1, bc2 = 1 - f1 ** step, 1 - f2 ** step
    gd = g.double() * coef
    sm = torch.maximum((f1 * m).abs(), ((1 - f1) * gd).abs())
    sv = torch.maximum(f2 * v, (1 - f2) * gd * gd)
    m = f1 * m + (1 - f1) * gd
    v = f2 * v + (1 - f2) * gd * gd
    upd = (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
    sp = torch.maximum(p.abs(), upd.abs())
    return (p - upd, m, v), (sp, sm, sv)


def opt_tensors(n):
    g = _gen(8000 + n % 977)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.05 * step for step in range(1, OPT_STEPS + 1)]
    return p0, grads


def norm_coef64(g, max_norm):
    nrm = float(torch.sqrt((g.double() ** 2).sum()))
    return nrm, min(1.0, f32(max_norm) / (nrm + 1e-6))


def ema_ref64(ema, p, decay):
    """ema + (1 - decay) (p - ema) in float64 with the fp32 decay (1 - decay is exact in fp32 for decay >= 0.5)"""
    return ema.double() + (1.0 - f32(decay)) * (p.double() - ema.double())
