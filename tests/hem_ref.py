"""Tests only: the numpy restatement of what dmh_hem_batch / dmh_hem_flow compute (dmhomo_amd/csrc/hem_data.hip), i.e. of
DGMTrainData's item arithmetic (HEM/dataset/data_loader.py:121-255).  The product never imports this file.

Pinned to the reference by tests/golden/hem.npz (tests/golden/make_golden_hem.py ran the reference's homo_scale,
homo_convert_to_flow and DGMTrainData.data_aug): test_hem_data_host.py.  The 8-bit bilinear resize has NO reference-made
vector — OpenCV is not in the build image — and is written from OpenCV's published algorithm (resize.cpp, the 8-bit
INTER_LINEAR path); the kernel is checked against this restatement alone and parity with cv2 itself is UNPINNED."""
import numpy as np

MEAN_I = np.array([118.93, 113.97, 102.60]).reshape(1, 1, 3)          # data_loader.py:103-104
STD_I = np.array([69.85, 68.81, 72.45]).reshape(1, 1, 3)
F32 = np.float32


def _to_unit(h, w, inverse=False):
    """pixel coordinates of an (h, w) image <-> the square [-1, 1]^2: x = (w/2) u + w/2, y = (h/2) v + h/2; the inverse written
    out (u = 2x/w - 1), not computed"""
    if inverse:
        return np.array([[2.0 / w, 0., -1.], [0., 2.0 / h, -1.], [0., 0., 1.]])
    return np.array([[w / 2.0, 0., w / 2.0], [0., h / 2.0, h / 2.0], [0., 0., 1.]])


def homo_scale(h0, w0, H, h1, w1):
    """the homography H of an (h0, w0) image for the image resized to (h1, w1): through the unit square and back"""
    unit = _to_unit(h0, w0, inverse=True) @ np.asarray(H, dtype=np.float64) @ _to_unit(h0, w0)
    return _to_unit(h1, w1) @ unit @ _to_unit(h1, w1, inverse=True)


def _taps(n_src, n_dst, clamp_fraction):
    """source index and the two short coefficients (11 fractional bits, round half to even) of every output coordinate"""
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * float(n_src) / float(n_dst) - 0.5).astype(F32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = f - fl                                                        # float32
    if clamp_fraction:
        lo, hi = s < 0, s >= n_src - 1
        s = np.where(lo, 0, np.where(hi, n_src - 1, s))
        f = np.where(lo | hi, F32(0), f).astype(F32)
    c0 = np.rint((F32(1) - f) * F32(2048)).astype(np.int64)
    c1 = np.rint(f * F32(2048)).astype(np.int64)
    return s, c0, c1


def resize_u8(img, H, W):
    """cv2.resize(img, (W, H)) of a uint8 (..., h, w) plane stack with INTER_LINEAR's 8-bit arithmetic; as is when the size fits"""
    h, w = img.shape[-2:]
    if (h, w) == (H, W):
        return img.copy()
    sx, a0, a1 = _taps(w, W, True)
    sy, b0, b1 = _taps(h, H, False)                                   # the vertical fraction is not clamped: only the rows are
    sx1 = np.minimum(sx + 1, w - 1)
    sy0, sy1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    src = img.astype(np.int64)
    S = src[..., sx] * a0 + src[..., sx1] * a1                        # (..., h, W) horizontal pass
    S0, S1 = S[..., sy0, :] >> 4, S[..., sy1, :] >> 4
    out = (((b0[:, None] * S0) >> 16) + ((b1[:, None] * S1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def gray(u8_hwc):
    """(H, W, 3) uint8 -> (H, W) fp32: the float64 normalisation and np.mean over the channels (data_loader.py:240-250)"""
    g = (u8_hwc.astype(np.float64) - MEAN_I) / STD_I
    return (((g[..., 0] + g[..., 1]) + g[..., 2]) / 3.0).astype(F32)


def mapping(Hm, H, W):
    """fp32 mapping (2, H, W) of homography Hm in float64 with epsilon 1e-8, products summed left to right without FMA"""
    Hm = np.asarray(Hm, dtype=np.float64).reshape(3, 3)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    wq = (Hm[2, 0] * x + Hm[2, 1] * y) + Hm[2, 2]
    mx = ((Hm[0, 0] * x + Hm[0, 1] * y) + Hm[0, 2]) / (wq + 1e-8)
    my = ((Hm[1, 0] * x + Hm[1, 1] * y) + Hm[1, 2]) / (wq + 1e-8)
    return np.stack([mx, my]).astype(F32)


def flow(Hm, H, W):
    """homo_convert_to_flow (data_loader.py:42-52): (2, H, W) fp32 = mapping - grid, subtracted in fp32"""
    y, x = np.mgrid[0:H, 0:W].astype(F32)
    return mapping(Hm, H, W) - np.stack([x, y])


def batch(img12, homos, starts, ori_size, crop_size):
    """img12 uint8 (B,6,h,w), homos (B,3,3) f64 at (h, w), starts B x (x, y) -> the dict of numpy arrays dmh_hem_batch's
    caller (DGMTrainData.from_pairs) returns"""
    B, _, h, w = img12.shape
    (H, W), (ph, pw) = ori_size, crop_size
    out = {k: [] for k in ('imgs_gray_full', 'imgs_gray_patch', 'flow_gt_full', 'flow_gt_patch', 'imgs_rgb_full')}
    for b in range(B):
        Hf = np.asarray(homos[b], dtype=np.float64)
        if (h, w) != (H, W):
            Hf = homo_scale(h, w, Hf, H, W)
        Hb = np.linalg.inv(Hf)
        u8 = resize_u8(img12[b], H, W)
        g = np.stack([gray(u8[:3].transpose(1, 2, 0)), gray(u8[3:].transpose(1, 2, 0))])
        fl = np.concatenate([flow(Hb, H, W), flow(Hf, H, W)])
        x, y = starts[b]
        out['imgs_rgb_full'].append(u8.astype(F32) / F32(255))
        out['imgs_gray_full'].append(g)
        out['flow_gt_full'].append(fl)
        out['imgs_gray_patch'].append(g[:, y:y + ph, x:x + pw])
        out['flow_gt_patch'].append(fl[:, y:y + ph, x:x + pw])
    out = {k: np.stack(v) for k, v in out.items()}
    out['start'] = np.asarray(starts, dtype=F32).reshape(B, 2, 1, 1)
    return out


def flow_tol(flow_ref):
    """per element, one fp32 ulp of the mapped coordinate (or of the flow where that is the larger number): what a float64
    mapping that differs in its last bits — a BLAS np.dot with FMA against products summed one by one — can move the fp32
    flow by.  Never above 2^-14, the ulp below 1024; the caller's coordinates stay below that."""
    B_, two, H, W = (1,) * (4 - flow_ref.ndim) + flow_ref.shape
    assert two % 2 == 0
    y, x = np.mgrid[0:H, 0:W].astype(F32)
    grid = np.tile(np.stack([x, y]), (two // 2, 1, 1))
    big = np.maximum(np.abs(flow_ref + grid), np.abs(flow_ref)).astype(F32)
    assert big.max() < 1024
    return np.spacing(big)


def assert_flow_close(name, got, ref):
    got, ref = np.asarray(got, dtype=F32), np.asarray(ref, dtype=F32)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, tol = np.abs(got.astype(np.float64) - ref.astype(np.float64)), flow_tol(ref)
    print(f'[parity] {name}: max_abs={err.max():.3e} worst err/ulp={(err / tol).max():.2f} mismatching={int((err > 0).sum())}')
    assert (err <= tol).all() and tol.max() <= 2.0 ** -14, name
