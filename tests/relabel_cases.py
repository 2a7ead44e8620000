"""What the tests of relabel_batch share (include/dmhomo_hip_relabel.h has the definition): a float64 numpy statement of the draw
— Philox through oracle/rng.py, u01 in fp32, the closed-form scaling, the base product, one rounding per operation — the source
coordinates the validity is defined on, the shapes of the kernel tests and their inputs."""
import numpy as np
import torch

from oracle import rng as ORNG

# (B, H, W): one partial workgroup; exactly one; a partial second one with W % 4 != 0; H != W; the real size once
SHAPES = ((1, 8, 8), (3, 16, 16), (3, 20, 20), (2, 12, 20), (2, 128, 128))
SEEDS = (0, 1, 2, 3)
RANGES = (.03, 8., 3e-5)                                      # the defaults: SyntheticConditions' constants
DRAW = 0xFFFFFFFF                                             # the draw word of the label's two Philox blocks
# every scaling exact: ranges that are powers of two at a size where s = (W / 640, H / 360, 1) = (2^-5, 2^-3, 1) — the entries
# of H_new then ARE the uniforms up to powers of two, so the uniforms can be read back from the output bit for bit
EXACT_SHAPE, EXACT_RANGES = (2, 45, 20), (0.125, 8., 2. ** -12)
NEAR = 1e-9                                                   # a coordinate this close to a bound may fall on either side


def words(seed, sample_ids):
    """(B, 8) uint32: blocks q = 0, 1 of counter {q, 0xFFFFFFFF, id lo, id hi}, key (seed lo, seed hi)"""
    return ORNG.words(int(seed), [int(i) for i in sample_ids], DRAW, 8)


def uniforms(w):
    """u = 2.0 * (double)u01(w) - 1.0, u01 in fp32 (a rounded multiply and a rounded add)"""
    u01 = ORNG._u01(np.asarray(w, dtype=np.uint32))
    assert u01.dtype == np.float32
    d = 2.0 * u01.astype(np.float64)
    return d - 1.0


def perturbation(u, ranges=RANGES):
    """P0 in the 360 x 640 frame from the eight uniforms of a sample"""
    a, t, p = (float(v) for v in ranges)
    u = [float(v) for v in u]
    return np.array([[1.0 + u[0] * a, u[1] * a, u[2] * t],
                     [u[3] * a, 1.0 + u[4] * a, u[5] * t],
                     [u[6] * p, u[7] * p, 1.0]], dtype=np.float64)


def to_frame(P0, H, W):
    """P[i][j] = (P0[i][j] * s_i) / s_j, s = (W / 640, H / 360, 1)"""
    s = np.array([W / 640.0, H / 360.0, 1.0], dtype=np.float64)
    return (P0 * s[:, None]) / s[None, :]


def compose(P, Hb):
    """(P . Hb) / (P . Hb)[2][2], the sum as (p0 h0 + p1 h1) + p2 h2"""
    Hb = np.asarray(Hb, dtype=np.float64).reshape(3, 3)
    M = np.empty((3, 3), dtype=np.float64)
    for i in range(3):
        for j in range(3):
            M[i, j] = (P[i, 0] * Hb[0, j] + P[i, 1] * Hb[1, j]) + P[i, 2] * Hb[2, j]
    return M / M[2, 2]


def homographies(seed, sample_ids, H, W, ranges=RANGES, base=None):
    """(B, 3, 3) float64: H_new of every sample id (base: None or (B, 3, 3))"""
    u = uniforms(words(seed, sample_ids))
    out = []
    for b in range(len(u)):
        P = to_frame(perturbation(u[b], ranges), H, W)
        out.append(P if base is None else compose(P, base[b]))
    return np.stack(out)


def inverse(m):
    """adjugate times 1 / determinant, in dmh_homography_warp's operation order"""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).reshape(9)]
    a = [m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
    det = m[0] * a[0] + m[1] * a[3] + m[2] * a[6]
    idet = 1.0 / det if det != 0.0 else 0.0
    return np.array([v * idet for v in a], dtype=np.float64)


def source_coordinates(m, H, W):
    """(sx, sy), each (H, W) float64: m^-1 . (x, y, 1) per destination pixel, in the kernel's operation order"""
    inv = inverse(m)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    qx = inv[0] * x + inv[1] * y + inv[2]
    qy = inv[3] * x + inv[4] * y + inv[5]
    qw = inv[6] * x + inv[7] * y + inv[8]
    with np.errstate(divide='ignore', invalid='ignore'):
        sx = np.where(qw != 0.0, qx / qw, 0.0)
        sy = np.where(qw != 0.0, qy / qw, 0.0)
    return sx, sy


def valid_of(m, H, W):
    """-> (valid (H, W) bool: the source coordinate in the closed [0, W - 1] x [0, H - 1]; near (H, W) bool: within NEAR of a bound)"""
    sx, sy = source_coordinates(m, H, W)
    ok = (sx >= 0.0) & (sx <= W - 1.0) & (sy >= 0.0) & (sy <= H - 1.0)
    near = np.zeros((H, W), dtype=bool)
    for v, hi in ((sx, W - 1.0), (sy, H - 1.0)):
        near |= (np.abs(v) <= NEAR) | (np.abs(v - hi) <= NEAR)
    return ok, near


def base_homographies(B, H, W, seed=7):
    """(B, 3, 3) float64: mild homographies of the H x W frame for the batch's own labels (a generator of its own, not the draw)"""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        P0 = np.eye(3) + np.array([[.02, -.01, 5.], [.015, -.02, -4.], [2e-5, -1e-5, 0.]]) * g.uniform(-1, 1, (3, 3))
        out.append(to_frame(P0, H, W))
    return np.stack(out)


def batch_inputs(B, H, W, seed):
    """(B, 12, H, W) fp32: images in [0, 1] with both ends among their values, a binary mask, and condition channels that are
    NOT what the relabelled batch must hold (so a kernel that copied them would be seen)"""
    gen = torch.Generator().manual_seed(seed)
    data = torch.rand((B, 12, H, W), generator=gen)
    data[:, 6] = (data[:, 6] > 0.4).float()
    data[:, 10:] = torch.randn((B, 2, H, W), generator=gen)
    data[0, 0, 0, 0], data[0, 0, 0, 1] = 0., 1.
    return data
