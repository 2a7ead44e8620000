"""CPU: the host side of the sample preview sheets — the binding of the three preview kernels, the reference's names and
signatures (tests/golden/make_golden_preview.py -> surface_preview.json), the PNG writer decoded with zlib here, and the grid
layout against a numpy restatement of torchvision's make_grid carried by this file."""
import inspect
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('dmh_post_process', 'dmh_preview_sheet', 'dmh_homography_warp')


def test_header_and_binding_hold_the_preview_kernels():
    from dmhomo_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'dmhomo_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(dmh_[a-z0-9_]+)\s*\(', src))
    for name in KERNELS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and args[-1] is _lib.C.c_void_p          # status code; the stream goes last
    assert _lib.ABI_VERSION == 500                                          # additive: the version stays


def test_preview_kernels_refuse_bad_arguments():
    """NULL pointers, 0 / negative sizes and sizes whose product overflows answer through the error channel (every case here
    is refused by the validator: nothing is launched, with or without a GPU)"""
    import ctypes as C
    from dmhomo_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * 64)()
    hp = C.cast(buf, C.c_void_p)
    for name in KERNELS:
        _, argtypes = _lib.SIGNATURES[name]
        for ival, p in ((4, None), (0, hp), (-1, hp), (2 ** 30, hp), (2 ** 16, hp)):
            args = [ival if t is _lib.c_int else p for t in argtypes]
            assert getattr(lib, name)(*args) == -1, (name, ival, p)
            assert name.encode() in lib.dmh_last_error()
    # an unaligned sheet pointer (the kernel stores dwords)
    odd = C.c_void_p(hp.value + 1)
    assert lib.dmh_preview_sheet(hp, hp, hp, odd, hp, 2, 4, 4, 2, 2, 1, None) == -1 and b'aligned' in lib.dmh_last_error()


def test_alias_module_offers_the_reference_preview_surface(golden_dir):
    from dmhomo_amd.denoising_diffusion_models import denoising_diffusion_pytorch as ddp
    with open(os.path.join(golden_dir, 'surface_preview.json')) as f:
        want = json.load(f)
    assert sorted(want) == ['make_gif', 'postProcess', 'postProcess_cv2', 'visulize_flow']
    for name, sig in want.items():
        assert str(inspect.signature(getattr(ddp, name))) == sig, name
    assert ddp.Trainer.preview is False
    with open(os.path.join(golden_dir, 'surface.json')) as f:
        surface = json.load(f)
    assert str(inspect.signature(ddp.Trainer.__init__)) == surface['denoising_diffusion_pytorch']['Trainer']['__init__']


def decode_png(path):
    """an 8-bit RGB, non-interlaced PNG whose rows all use filter 0 -> (H, W, 3) uint8; checks signature, chunk CRCs, IHDR"""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    w, h, depth, colour, comp, filt, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b''.join(body for kind, body in chunks if kind == b'IDAT'))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()                                             # filter type 0 on every row
    return rows[:, 1:].reshape(h, w, 3)


def test_png_writer(tmp_path):
    from dmhomo_amd import preview
    a = np.random.default_rng(37).integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    path = str(tmp_path / 'a.png')
    preview.write_png(a, path)
    got = decode_png(path)
    assert got.shape == a.shape and got.tobytes() == a.tobytes()
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.array(Image.open(path)), a)


def make_grid_np(a, nrow, padding):
    """torchvision.utils.make_grid(tensor, nrow, padding, pad_value=0) as published, on a (B, C, H, W) array"""
    B, C, H, W = a.shape
    if B == 1:
        return a[0]
    xmaps = min(nrow, B)
    ymaps = int(np.ceil(B / xmaps))
    height, width = H + padding, W + padding
    grid = np.zeros((C, height * ymaps + padding, width * xmaps + padding), dtype=a.dtype)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= B:
                break
            grid[:, y * height + padding:y * height + padding + H, x * width + padding:x * width + padding + W] = a[k]
            k += 1
    return grid


def quantise_np(grid):
    """save_image: mul(255).add_(0.5).clamp_(0, 255) -> uint8, HWC"""
    g = grid.astype(np.float32) * np.float32(255)
    g = g + np.float32(0.5)
    return np.clip(g, 0, 255).astype(np.uint8).transpose(1, 2, 0)


@pytest.mark.parametrize('B', [1, 4, 9, 10])
@pytest.mark.parametrize('nrow', [1, 3, 8])
def test_grid_geometry_and_save_image(tmp_path, B, nrow):
    from dmhomo_amd import preview, ops
    H, W, pad = 5, 7, 2
    a = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(B * 10 + nrow)) * 1.2 - 0.1   # some values clamp
    want = make_grid_np(a.numpy(), nrow, pad)
    got = preview.make_grid(a, nrow=nrow, padding=pad)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert ops.grid_shape(B, H, W, nrow, pad)[:2] == want.shape[1:]
    path = str(tmp_path / 'g.png')
    preview.save_image(a, path, nrow=nrow, padding=pad)
    assert np.array_equal(decode_png(path), quantise_np(want))
    if B > 1:                                                # the default padding of save_image is 2
        preview.save_image(a, path, nrow=nrow)
        assert np.array_equal(decode_png(path), quantise_np(want))


def test_num_to_groups_and_square_rows():
    from dmhomo_amd import preview
    assert preview.num_to_groups(9, 4) == [4, 4, 1] and preview.num_to_groups(4, 2) == [2, 2] and preview.num_to_groups(3, 8) == [3]
    assert [preview.square_rows(n) for n in (1, 2, 4, 8, 9, 25, 80)] == [1, 1, 4, 4, 9, 16, 16]
