"""Photometric-consistency guidance (include/dmhomo_hip.h, "Photometric-consistency guidance"), restated in float64, and the
case table of its tests.  No GPU and no library here: torch on the CPU only.

The one thing taken over in fp32 is what the definition takes over from dmh_flow_warp: the sample point, its four taps and
their bilinear weights (``taps32``: flow_warp_taps of csrc/geometry_dev.h, one rounding per operation).  Everything behind
them — the warp, the residual, the transposed warp, s, the step and the energy — is float64 on a dense (H*W, H*W) matrix
W[p, q] = w_p(q), which is small at the shapes of the tests."""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
SHAPES = ((2, 2), (5, 7), (16, 16), (33, 47))   # 33 x 47 = 1551 pixels: seven workgroups of 256 per sample, a ragged last one
BATCHES = (1, 3)
FLOWS = ('zero', 'shift', 'subpixel', 'far', 'fold', 'homography')
MASKS = ('zero', 'one', 'binary', 'fraction')
LAMBDAS = (0.25, 1.)


# ------------------------------------------------------------------------------------------ the taps, as dmh_flow_warp has them
def taps32(flow):
    """flow (2, H, W) fp32 -> (x0, y0, x1ok, y1ok int64 / bool (H, W); wnw, wne, wsw, wse fp32 (H, W))"""
    _, H, W = flow.shape
    flow = flow.to(F32)
    t = lambda v: torch.full((H, W), float(v), dtype=F32)
    xi = torch.arange(W, dtype=F32).reshape(1, W).expand(H, W)
    yi = torch.arange(H, dtype=F32).reshape(H, 1).expand(H, W)
    vx, vy = xi + flow[0], yi + flow[1]
    gx = t(2.) * vx / t(W - 1) - t(1.)
    gy = t(2.) * vy / t(H - 1) - t(1.)
    ix = (gx + t(1.)) * (t(W - 1) / t(2.))
    iy = (gy + t(1.)) * (t(H - 1) / t(2.))
    ix = torch.minimum(t(W - 1), torch.maximum(ix, t(0.)))
    iy = torch.minimum(t(H - 1), torch.maximum(iy, t(0.)))
    fx0, fy0 = ix.floor(), iy.floor()
    w, e, n, s = ix - fx0, (fx0 + t(1.)) - ix, iy - fy0, (fy0 + t(1.)) - iy
    x0, y0 = fx0.long(), fy0.long()
    return x0, y0, x0 + 1 <= W - 1, y0 + 1 <= H - 1, s * e, s * w, n * e, n * w


def warp_matrix(flow):
    """flow (2, H, W) -> W (H*W, H*W) float64, W[p, q] = w_p(q): a tap one past the last row / column is dropped"""
    _, H, Wd = flow.shape
    x0, y0, x1ok, y1ok, wnw, wne, wsw, wse = taps32(flow)
    hw = H * Wd
    M = torch.zeros((hw, hw), dtype=F64)
    p = torch.arange(hw)
    for dy, dx, wt, ok in ((0, 0, wnw, torch.ones_like(x1ok)), (0, 1, wne, x1ok), (1, 0, wsw, y1ok), (1, 1, wse, x1ok & y1ok)):
        ok = ok.reshape(-1)
        q = ((y0 + dy) * Wd + (x0 + dx)).reshape(-1)
        M.index_put_((p[ok], q[ok]), wt.reshape(-1).double()[ok], accumulate=True)
    return M


# ------------------------------------------------------------------------------------------ the statement
def blend32(cond, null, keep, cs):
    """the logits a step works on, in fp32 exactly as guided_logit evaluates them: cond, or null + (c - null) * cs with c = null
    in the rows where keep == 0"""
    cond = cond.to(F32)
    if null is None:
        return cond
    null = null.to(F32)
    c = cond if keep is None else torch.where(keep.bool().reshape(-1, 1, 1, 1), cond, null)
    return null + (c - null) * torch.tensor(cs, dtype=F32)


def lam32(w, sqrt_ac):
    """lambda = w * (sqrt_ac * sqrt_ac) as the kernels form it: fp32, two roundings"""
    return float(np.float32(w) * (np.float32(sqrt_ac) * np.float32(sqrt_ac)))


def matrices(flow):
    """the warp matrix of every sample: what the functions below take as ``mats`` where a test calls several of them on one flow"""
    return [warp_matrix(flow[b]) for b in range(flow.shape[0])]


def weights_ref(flow, mask, mats=None):
    """s (B, H, W) float64 = sum_p mask[p] * w_p(q)"""
    B, _, H, W = flow.shape
    mats = matrices(flow) if mats is None else mats
    return torch.stack([mats[b].T @ mask[b].reshape(-1).double() for b in range(B)]).reshape(B, H, W)


def energy_ref(x, flow, mask, mats=None):
    """E (B,) float64 of x (B, 6, H, W), any float dtype"""
    B, _, H, W = x.shape
    mats = matrices(flow) if mats is None else mats
    out = []
    for b in range(B):
        M = mats[b]
        x1, x2 = x[b, :3].reshape(3, -1).double(), x[b, 3:].reshape(3, -1).double()
        d = x2 @ M.T - x1
        out.append((mask[b].reshape(1, -1).double() * d * d).sum() / (3. * H * W))
    return torch.stack(out)


def guide_ref(x, flow, mask, lam, precondition=True, mats=None):
    """one correction of the blend x (B, 6, H, W) -> y (B, 6, H, W) float64.  lam: a float or one per sample.
    precondition=False: the plain gradient step without the division by max(1, s) (what the division is there to prevent)"""
    B, _, H, W = x.shape
    lam = [float(lam)] * B if not hasattr(lam, '__len__') else [float(v) for v in lam]
    y = torch.empty((B, 6, H, W), dtype=F64)
    mats = matrices(flow) if mats is None else mats
    for b in range(B):
        M = mats[b]
        m = mask[b].reshape(-1).double()
        x1, x2 = x[b, :3].reshape(3, -1).double(), x[b, 3:].reshape(3, -1).double()
        r = m * (x2 @ M.T - x1)
        s = M.T @ m
        den = torch.clamp(s, min=1.) if precondition else torch.ones_like(s)
        y[b, :3] = (x1 + 0.5 * lam[b] * r).reshape(3, H, W)
        y[b, 3:] = (x2 - 0.5 * lam[b] * (r @ M) / den).reshape(3, H, W)
    return y


def energy_scale(x, flow, mask, mats=None):
    """(B,) float64: E with |u| + |x| in place of u - x — what the rounding errors of a float64 evaluation of E are relative to"""
    B, _, H, W = x.shape
    mats = matrices(flow) if mats is None else mats
    out = []
    for b in range(B):
        M = mats[b]
        x1, x2 = x[b, :3].reshape(3, -1).double().abs(), x[b, 3:].reshape(3, -1).double().abs()
        d = x2 @ M.T + x1
        out.append((mask[b].reshape(1, -1).double().abs() * d * d).sum() / (3. * H * W))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------ the case table
def make_flow(kind, B, H, W, gen):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing='ij')
    f = torch.zeros((B, 2, H, W), dtype=F64)
    if kind == 'shift':                                       # whole pixels, another shift per sample, some of it off the image
        for b in range(B):
            f[b, 0], f[b, 1] = 1 + b, -1 - (b % 2)
    elif kind == 'subpixel':
        f = torch.randn((B, 2, H, W), generator=gen, dtype=F64) * 1.5
    elif kind == 'far':                                       # every sample point clamped to a border: whole rows / columns
        f = torch.where(torch.rand((B, 2, H, W), generator=gen) < 0.5, -1000., 1000.).double()       # land on single targets
    elif kind == 'fold':                                      # flow_x = -0.9 x: ten source columns fold onto one target column
        f[:, 0] = -0.9 * xs
        f[:, 1] = 0.25
    elif kind == 'homography':                                # a small projective map around the identity
        for b in range(B):
            h = torch.eye(3, dtype=F64) + torch.tensor([[0.03, -0.02, 0.7], [0.015, -0.025, -0.4], [2e-4, -1e-4, 0.]]) * (1 + b)
            den = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
            f[b, 0] = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) / den - xs
            f[b, 1] = (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) / den - ys
    else:
        assert kind == 'zero', kind
    return f.to(F32)


def make_mask(kind, B, H, W, gen):
    if kind == 'zero':
        return torch.zeros((B, 1, H, W), dtype=F32)
    if kind == 'one':
        return torch.ones((B, 1, H, W), dtype=F32)
    u = torch.rand((B, 1, H, W), generator=gen)
    return (u > 0.4).float() if kind == 'binary' else u.to(F32)


def cases(shapes=SHAPES, batches=BATCHES, flows=FLOWS, masks=MASKS):
    """[(name, dict(B, H, W, flow_kind, mask_kind, flow (B, 2, H, W), mask (B, 1, H, W), cond, null (B, 6, H, W) fp32, keep (B,)
    uint8 with a dropped row))]"""
    out = []
    for (H, W) in shapes:
        for B in batches:
            for fk in flows:
                for mk in masks:
                    gen = torch.Generator().manual_seed(1000 * H + 10 * W + B + 7 * FLOWS.index(fk) + 31 * MASKS.index(mk))
                    keep = torch.ones((B,), dtype=torch.uint8)
                    keep[B // 2] = 0
                    out.append((f'{fk}-{mk}-{B}x{H}x{W}',
                                dict(B=B, H=H, W=W, flow_kind=fk, mask_kind=mk, flow=make_flow(fk, B, H, W, gen),
                                     mask=make_mask(mk, B, H, W, gen), cond=torch.randn((B, 6, H, W), generator=gen) * 0.8,
                                     null=torch.randn((B, 6, H, W), generator=gen) * 0.8, keep=keep)))
    return out


VARIANTS = ('cond', 'cond+null', 'cond+null+keep')


def variant(case, which):
    """-> (cond, null or None, keep or None) of one of VARIANTS"""
    if which == 'cond':
        return case['cond'], None, None
    return case['cond'], case['null'], (case['keep'] if which == 'cond+null+keep' else None)


def is_identity(flow):
    """whether every sample's warp matrix is the identity bit for bit (zero flow at a size where the fp32 taps land on the pixel)"""
    return all(torch.equal(warp_matrix(flow[b]), torch.eye(flow.shape[2] * flow.shape[3], dtype=F64)) for b in range(flow.shape[0]))
