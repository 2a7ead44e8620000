"""Sample preview sheets: the host side of DDP:1489-1555 (visulize_flow, postProcess, postProcess_cv2, make_gif), a stand-in
for torchvision.utils.save_image / make_grid (package not installed here; its published layout restated) with a PNG writer on
the standard library, and the fused path ``save_preview_sheets`` — (img, mask, flow) -> two PNG files through ONE kernel
(dmh_preview_sheet: panels, BGR swap, grid, quantisation) and one device-to-host copy per sheet.

Panel values come from libdmhomo_hip.so (preview.hip); there is no CPU path for them.  Grid assembly of an already finished
float tensor (``make_grid`` / ``save_image``) and file encoding are host plumbing, as in torchvision.
"""
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import ops

CV2_DSIZE = (256, 256)          # DDP:1527 hard-codes the canvas of the homography warp


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError('dmhomo_amd preview kernels need a GPU; there is no CPU path')
    return torch.device('cuda', torch.cuda.current_device())


def _on_gpu(t):
    t = torch.as_tensor(t)
    return t if t.is_cuda else t.to(_dev())


# ------------------------------------------------------------------ files
def write_png(array, path):
    """(H, W, 3) uint8 -> an 8-bit RGB PNG (one IDAT, filter 0 on every row), standard library only."""
    a = np.ascontiguousarray(np.asarray(array))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f'write_png takes an (H, W, 3) uint8 array, got {a.dtype} {a.shape}')
    h, w, _ = a.shape
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)          # filter byte 0 + the row
    rows[:, 1:] = a.reshape(h, 3 * w)

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)

    png = (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
           chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b''))
    with open(os.fspath(path), 'wb') as f:
        f.write(png)


def make_grid(tensor, nrow=8, padding=2):
    """torchvision.utils.make_grid(tensor, nrow, padding, pad_value=0) for a (B, C, H, W) batch (or one (C, H, W) image):
    xmaps = min(nrow, B), ymaps = ceil(B / xmaps), image k at row (k // xmaps)(H+p)+p, column (k % xmaps)(W+p)+p of a
    (C, ymaps (H+p)+p, xmaps (W+p)+p) sheet; B == 1: the image alone.  Single-channel images are repeated to 3 channels.
    Host numpy: a layout of finished values."""
    a = tensor.detach().cpu().numpy() if torch.is_tensor(tensor) else np.asarray(tensor)
    if a.ndim == 2:
        a = a[None]
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4:
        raise ValueError(f'make_grid takes (B, C, H, W) or (C, H, W), got {a.shape}')
    if a.shape[1] == 1:
        a = np.repeat(a, 3, axis=1)
    B, C, H, W = a.shape
    if B == 1:
        return a[0].copy()
    Hs, Ws, xmaps = ops.grid_shape(B, H, W, nrow, padding)
    grid = np.zeros((C, Hs, Ws), dtype=a.dtype)
    for k in range(B):
        y, x = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        grid[:, y:y + H, x:x + W] = a[k]
    return grid


def save_image(tensor, path, nrow=8, padding=2):
    """stand-in for torchvision.utils.save_image(tensor, path, nrow=..., padding=...): make_grid, then
    mul(255).add_(0.5).clamp_(0, 255) truncated to uint8 (two fp32 roundings, as torch does them), written as a PNG."""
    grid = make_grid(tensor, nrow=nrow, padding=padding).astype(np.float32)
    q = np.clip(grid * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)
    write_png(q.transpose(1, 2, 0), path)


def make_gif(img1, img2, name):
    """DDP:1543-1555: the two image files as a two-frame GIF sample_gif_results/{name}.gif, 0.5 s per frame, loop 0.  Written
    with PIL when it imports (the reference uses imageio + cv2, not installed here); without PIL one line is printed and
    nothing is written — nothing else depends on it."""
    try:
        from PIL import Image
    except ImportError:
        print(f'make_gif: PIL is not available, sample_gif_results/{name}.gif not written')
        return
    if not os.path.exists('sample_gif_results'):
        os.mkdir('sample_gif_results')
    frames = [Image.open(p).convert('RGB') for p in (img1, img2)]
    frames[0].save(f'sample_gif_results/{name}.gif', save_all=True, append_images=frames[1:], duration=500, loop=0)


# ------------------------------------------------------------------ panels
def visulize_flow(all_images):
    """DDP:1489-1502: flows (B,2,H,W) -> the HSV flow image (B,3,H,W) fp32, max_flow 256, returned on the host as the
    reference returns it (dmh_flow_to_image)."""
    flow = _on_gpu(all_images.detach()).to(torch.float32).contiguous()
    return ops.flow_to_image(flow, 256.).cpu()


def _preview_inputs(torch_tensor, mask, flows):
    img = _on_gpu(torch_tensor.detach())[:, :6].to(torch.float32).contiguous()
    return img, _on_gpu(mask.detach()).to(torch.float32).contiguous(), _on_gpu(flows.detach()).to(torch.float32).contiguous()


def postProcess(torch_tensor, mask, flows):
    """DDP:1505-1517: buf1 = [img1 | img1 | mask x3 | flow_vis], buf2 = [img2 | flow_warp(img2, flows) | mask x3 | flow_vis],
    each (B,3,H,4W), on the inputs' device (one launch: dmh_post_process)."""
    buf1, buf2 = ops.post_process(*_preview_inputs(torch_tensor, mask, flows))
    return buf1.to(torch_tensor.device), buf2.to(torch_tensor.device)


def postProcess_cv2(imgs, homos, rank):
    """DDP:1520-1540 on a saveTrainPair record: imgs uint8 (B,6,H,W), homos float64 (B,3,3) ->
    buf1 = [img1 | warpPerspective(img1, H, (256, 256))], buf2 = [img2 | img2] on device ``rank``.  The canvas is (256, 256)
    whatever the record's size (DDP:1527), so — as in the reference — the panels only line up for records 256 pixels high.

    Deliberate deviation: cv2 is not installed, and its warpPerspective interpolates with fixed-point coefficient tables that
    quantise the fraction to 1/32; dmh_homography_warp gives the EXACT bilinear result (float64 inverse, coordinates and
    weights, constant border 0 per neighbour)."""
    dev = torch.device('cuda', rank) if isinstance(rank, int) else torch.device(rank)
    imgs = np.asarray(imgs)
    if imgs.shape[2] != CV2_DSIZE[1]:
        raise ValueError(f'postProcess_cv2 warps onto a {CV2_DSIZE} canvas (DDP:1527) and puts it beside the record: records '
                         f'must be {CV2_DSIZE[1]} pixels high, got {imgs.shape[2]}')
    img1s = torch.from_numpy(imgs[:, :3].astype(np.float32) / 255.).to(dev)
    img2s = torch.from_numpy(imgs[:, 3:6].astype(np.float32) / 255.).to(dev)
    Hm = torch.from_numpy(np.ascontiguousarray(np.asarray(homos, dtype=np.float64).reshape(-1, 3, 3))).to(dev)
    with torch.cuda.device(dev):
        warp_img2s = ops.homography_warp(img1s.contiguous(), Hm, CV2_DSIZE)
    return torch.concat([img1s, warp_img2s], -1), torch.concat([img2s, img2s], -1)


# ------------------------------------------------------------------ the fused path
def save_preview_sheets(img, mask, flows, source_path, target_path, nrow, padding=2, bgr=True):
    """what ``postProcess`` -> ``[:, [2,1,0]]`` -> ``utils.save_image(..., nrow=nrow)`` writes for both buffers
    (DDP:1912-1929), fused: one dmh_preview_sheet launch produces both uint8 sheets, each is copied to the host once and
    encoded.  Per pixel and sample the kernel reads 9 floats and writes 24 bytes."""
    s1, s2 = ops.preview_sheet(*_preview_inputs(img, mask, flows), nrow=nrow, padding=padding, bgr=bgr)
    write_png(s1.cpu().numpy(), source_path)
    write_png(s2.cpu().numpy(), target_path)


def num_to_groups(num, divisor):
    """DDP:66-72: num as full groups of ``divisor`` and the remainder"""
    groups, remainder = divmod(num, divisor)
    return [divisor] * groups + ([remainder] if remainder > 0 else [])


def square_rows(n):
    """DDP:1973-1975: the largest square number of samples, at most 16, that a batch of n offers"""
    s = min(math.floor(math.sqrt(n)), 4)
    return s * s
