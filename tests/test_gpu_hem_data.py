"""-m gpu: HEM training batches built on the device (dmhomo_amd/hem_data.py over dmh_hem_batch / dmh_hem_flow,
csrc/hem_data.hip) against tests/hem_ref.py — the numpy restatement that test_hem_data_host.py pins to the reference's own
outputs — and against the reference's golden vectors directly where one exists (tests/golden/hem.npz).

What is compared how: ``imgs_rgb_full`` and ``imgs_gray_full`` bit for bit (integer resize, IEEE float64 normalisation);
``flow_gt_full`` within one fp32 ulp of the mapped coordinate (hem_ref.assert_flow_close; the kernel and the restatement share
the operation order, so 0 mismatching elements is the expected print); the patch tensors ``torch.equal`` to windows of the full
ones.  The 8-bit resize is checked against the restatement alone: parity with cv2 itself is UNPINNED (no OpenCV here)."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import hem_ref
from gpu_util import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(ori, crop, rho):
    return types.SimpleNamespace(crop_size=crop, ori_size=ori, rho=rho)


def make_record(B, h, w, seed):
    """a saveTrainPair-shaped record: smooth + noisy uint8 pairs (the bilinear taps matter) and homographies of the (h, w) image
    with a perspective row"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    imgs = np.empty((B, 6, h, w), np.uint8)
    for b in range(B):
        for c in range(6):
            base = 127 + 100 * np.sin(xx / (3.0 + c) + rng.random() * 6) * np.cos(yy / (2.5 + b))
            imgs[b, c] = np.clip(base + rng.integers(-25, 25, size=(h, w)), 0, 255).astype(np.uint8)
    imgs[0, :, 0, :] = 255                                            # extremes on the rows / columns whose taps are clipped
    imgs[0, :, -1, :] = 0
    imgs[-1, :, :, 0] = 0
    imgs[-1, :, :, -1] = 255
    homos = np.stack([np.eye(3) + np.array([[.03, -.02, .06 * w], [.02, .04, -.05 * h], [.02 / w, -.015 / h, 0.]])
                      * rng.uniform(-1, 1, (3, 3)) for _ in range(B)])
    return imgs, homos


def check_batch(name, got, imgs, homos, starts, ori, crop):
    """one batch dict from the device against the restatement"""
    ref = hem_ref.batch(imgs, homos, starts, ori, crop)
    B, (H, W), (ph, pw) = len(imgs), ori, crop
    g = {k: v.cpu() for k, v in got.items()}
    assert set(g) == {'imgs_gray_full', 'imgs_gray_patch', 'flow_gt_full', 'flow_gt_patch', 'start', 'imgs_rgb_full'}
    for k, shape in (('imgs_gray_full', (B, 2, H, W)), ('imgs_rgb_full', (B, 6, H, W)), ('flow_gt_full', (B, 4, H, W)),
                     ('imgs_gray_patch', (B, 2, ph, pw)), ('flow_gt_patch', (B, 4, ph, pw)), ('start', (B, 2, 1, 1))):
        assert g[k].shape == shape and g[k].dtype == torch.float32 and got[k].is_cuda, (name, k, g[k].shape)
    rgb = g['imgs_rgb_full'].numpy()
    u8 = np.rint(rgb * 255).astype(np.int64)
    print(f'[parity] {name}: resized uint8 differing from the restatement: '
          f'{int((u8 != np.rint(ref["imgs_rgb_full"] * 255)).sum())} of {u8.size}; '
          f'grey elements differing: {int((g["imgs_gray_full"].numpy() != ref["imgs_gray_full"]).sum())}')
    assert np.array_equal(rgb, ref['imgs_rgb_full']), f'{name}: imgs_rgb_full (the integer resize)'
    assert np.array_equal(g['imgs_gray_full'].numpy(), ref['imgs_gray_full']), f'{name}: imgs_gray_full'
    hem_ref.assert_flow_close(f'{name} flow_gt_full', g['flow_gt_full'].numpy(), ref['flow_gt_full'])
    for b, (x, y) in enumerate(starts):
        assert torch.equal(g['imgs_gray_patch'][b], g['imgs_gray_full'][b, :, y:y + ph, x:x + pw]), (name, b)
        assert torch.equal(g['flow_gt_patch'][b], g['flow_gt_full'][b, :, y:y + ph, x:x + pw]), (name, b)
    assert np.array_equal(g['start'].numpy(), ref['start'])
    return g


# (22, 38): W % 4 != 0, every row ends in a partial group of two pixels and rows are not 16-byte aligned; (24, 40): the
# all-vector path.  Starts at both extremes of [rho, W - rho - pw] x [rho, H - rho - ph] and one in between; in the first case
# the patch columns start at x = 2, 12, 7: offsets 2, 0 and 3 mod 4 against the threads' groups of four.
SMALL = [((22, 38), [(2, 2), (12, 4), (7, 3)]), ((24, 40), [(2, 2), (14, 6), (7, 3)])]


@pytest.mark.parametrize('ori,starts', SMALL, ids=['22x38-tail', '24x40-vector'])
def test_small_shapes_against_the_restatement(ori, starts):
    from dmhomo_amd.hem_data import DGMTrainData
    crop, rho = (16, 24), 2
    imgs, homos = make_record(3, 16, 16, seed=ori[1])
    ds = DGMTrainData(params(ori, crop, rho), npy_path=(), device=dev(), seed=0)
    for x, y in starts:
        assert rho <= x <= ori[1] - rho - crop[1] and rho <= y <= ori[0] - rho - crop[0]
    check_batch(f'16x16->{ori[0]}x{ori[1]}', ds.from_pairs(imgs, homos, starts), imgs, homos, starts, ori, crop)
    # drawn crops: the dataset's generator, x then y per item, recorded in ``start``
    ds2 = DGMTrainData(params(ori, crop, rho), npy_path=(), device=dev(), seed=7)
    want = DGMTrainData(params(ori, crop, rho), npy_path=(), seed=7).draw_starts(3)
    got = ds2.from_pairs(imgs, homos)
    assert got['start'].reshape(3, 2).tolist() == [[float(x), float(y)] for x, y in want]
    check_batch('drawn crops', got, imgs, homos, want, ori, crop)


def test_record_at_ori_size_is_not_resized():
    """the reference raises UnboundLocalError here (homo_gt_inv is only bound in the resize branch); the inverse is always formed"""
    from dmhomo_amd.hem_data import DGMTrainData
    ori, crop, starts = (22, 38), (16, 24), [(12, 4), (3, 2)]
    imgs, homos = make_record(2, *ori, seed=5)
    ds = DGMTrainData(params(ori, crop, 2), npy_path=(), device=dev(), seed=0)
    g = check_batch('no resize', ds.from_pairs(imgs, homos, starts), imgs, homos, starts, ori, crop)
    assert np.array_equal((g['imgs_rgb_full'] * 255).numpy(), imgs.astype(np.float32))


def test_vertical_fraction_is_not_clamped():
    """the pixel of test_hem_data_host.py::test_ref_resize_properties that tells the two readings of the vertical pass apart,
    from the kernel: rows [0, 1] of a 2 x 2 source -> 4 x 3; pixel (0, 1) is 0 with the fraction kept, 1 with it clamped"""
    from dmhomo_amd.hem_data import DGMTrainData
    imgs = np.tile(np.array([[0, 1], [0, 1]], np.uint8), (1, 6, 1, 1))
    ds = DGMTrainData(params((4, 3), (4, 3), 0), npy_path=(), device=dev(), seed=0)
    g = check_batch('2x2->4x3', ds.from_pairs(imgs, np.eye(3)[None], [(0, 0)]), imgs, np.eye(3)[None], [(0, 0)], (4, 3), (4, 3))
    u8 = np.rint(g['imgs_rgb_full'].numpy() * 255).astype(int)
    assert u8[0, :, 0].tolist() == [[0, 0, 1]] * 6


def test_real_geometry_once():
    """128 x 128 samples -> 360 x 640, crop 320 x 576, rho 16: the shapes HEM trains on"""
    from dmhomo_amd.hem_data import DGMTrainData
    ori, crop, rho = (360, 640), (320, 576), 16
    imgs, homos = make_record(2, 128, 128, seed=9)
    starts = [(16, 16), (48, 24)]                                    # the extremes of [16, 48] x [16, 24]
    ds = DGMTrainData(params(ori, crop, rho), npy_path=(), device=dev(), seed=0)
    check_batch('128x128->360x640', ds.from_pairs(imgs, homos, starts), imgs, homos, starts, ori, crop)


def test_three_doors_one_result(tmp_path):
    """per-sample files (the format scripts/generate_nyps_to_single_case.py writes) read item by item, as a batch, and the
    same arrays handed over directly — as numpy and as a device tensor — give the same bits"""
    from dmhomo_amd.hem_data import DGMTrainData, DGMBatchLoader
    spec = importlib.util.spec_from_file_location('gen_split_hem', os.path.join(ROOT, 'scripts', 'generate_nyps_to_single_case.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ori, crop, rho = (22, 38), (16, 24), 2
    imgs, homos = make_record(4, 16, 16, seed=21)
    np.save(str(tmp_path / 'rec.npy'), [{'imgs': imgs[:3], 'homos': homos[:3]}, {'imgs': imgs[3:], 'homos': homos[3:]}],
            allow_pickle=True)
    assert gen.split_records([str(tmp_path / 'rec.npy')], str(tmp_path / 'samples'), verbose=False) == 4
    ds = DGMTrainData(params(ori, crop, rho), npy_path=str(tmp_path / 'samples'), device=dev(), seed=3)
    assert len(ds) == 4 and [os.path.basename(p) for p in ds.npy_path] == ['1.npy', '2.npy', '3.npy', '4.npy']
    twin = DGMTrainData(params(ori, crop, rho), npy_path=(), seed=3)
    for i in (2, 0):
        (x, y), = twin.draw_starts(1)
        item = ds[i]                                                  # draws from ds's generator: the same crop
        assert item['start'].shape == (2, 1, 1) and item['start'].flatten().tolist() == [x, y]
        row = ds.batch([i], starts=[(x, y)])
        direct = ds.from_pairs(imgs[i:i + 1], homos[i:i + 1], starts=[(x, y)])
        on_dev = ds.from_pairs(torch.from_numpy(imgs[i:i + 1]).to(dev()), homos[i:i + 1], starts=[(x, y)])
        for k in item:
            assert item[k].is_cuda and torch.equal(item[k], row[k][0]), (i, k)
            assert torch.equal(row[k], direct[k]) and torch.equal(direct[k], on_dev[k]), (i, k)
    starts = [(2, 2), (12, 4), (7, 3), (5, 2)]
    check_batch('from files', ds.batch([0, 1, 2, 3], starts), imgs, homos, starts, ori, crop)
    # the loader end to end: batches of 3 out of 4 files, the short batch dropped, every batch drawn and built on the device
    dl = DGMBatchLoader(ds, 3, seed=1)
    for _ in range(3):
        b = next(dl)
        assert b['imgs_gray_patch'].shape == (3, 2) + crop and b['start'].shape == (3, 2, 1, 1) and b['flow_gt_full'].is_cuda
        assert bool(torch.isfinite(b['flow_gt_patch']).all())


def test_homo_convert_to_flow_against_the_reference(golden_dir):
    from dmhomo_amd.hem_data import homo_convert_to_flow
    gd = np.load(os.path.join(golden_dir, 'hem.npz'))
    for k in range(3):
        f = homo_convert_to_flow(gd['homo_scale'][k], (24, 40))
        assert f.shape == (1, 2, 24, 40) and f.dtype == torch.float32 and not f.is_cuda and not f.requires_grad
        hem_ref.assert_flow_close(f'homo_convert_to_flow[{k}] vs reference', f[0].numpy(), gd['flows'][k])
    f = homo_convert_to_flow(gd['homo_scale'][0], (22, 38))          # rows that are not 16-byte aligned
    hem_ref.assert_flow_close('homo_convert_to_flow 22x38', f[0].numpy(), hem_ref.flow(gd['homo_scale'][0], 22, 38))


def test_data_aug_against_the_reference(golden_dir):
    """the reference's data_aug outputs themselves (fixed start, and random.seed(7) -> [7, 3]) from the device"""
    from dmhomo_amd.hem_data import DGMTrainData
    gd = np.load(os.path.join(golden_dir, 'hem.npz'))
    names = ('img1', 'img2', 'img1_patch', 'img2_patch', 'flow_gt_b', 'flow_gt_f', 'flow_gt_b_patch', 'flow_gt_f_patch')
    for tag, start in (('fixed', [5, 2]), ('seeded', None)):
        ds = DGMTrainData(params((24, 40), (16, 24), 2), npy_path=(), device=dev(), seed=7)
        Hm = gd[f'{tag}.homo']
        out = ds.data_aug(gd['img1_u8'], gd['img2_u8'], Hm, np.linalg.inv(Hm), start=start)
        assert len(out) == 9 and out[8] == [int(v) for v in gd[f'{tag}.start']]
        for name, t in zip(names, out[:8]):
            want = gd[f'{tag}.{name}']
            assert t.is_cuda and tuple(t.shape) == want.shape, (tag, name, t.shape, want.shape)
            if name.startswith('img'):
                assert np.array_equal(t.cpu().numpy(), want), (tag, name)
            else:
                hem_ref.assert_flow_close(f'data_aug {tag}.{name} vs reference', t.cpu().numpy()[0], want[0])


def test_geometric_sense():
    """the reference's unit_test idea (data_loader.py:167): flow_warp(img2, flow_gt_f) lands on img1.  img2 is built from a smooth
    img1 with the package's flow_warp and the restatement's flow of the inverse homography, quantised to uint8 as a record is.
    No tolerance fixed in advance: the same comparison is measured with the restatement's tensors in place of the kernel's
    outputs, and the kernel's figure is gated at twice that (room for fp32 rounding in flow_warp)."""
    from dmhomo_amd import ops
    from dmhomo_amd.hem_data import DGMTrainData
    H, W, m = 48, 64, 8
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img1 = np.stack([127 + 90 * np.sin(xx / (9. + c) + c) * np.cos(yy / (7. + c)) for c in range(3)]).astype(np.float32)
    Hm = np.array([[1.02, .015, 1.8], [-.01, .99, -1.2], [1e-4, -8e-5, 1.]])
    flow_b = torch.from_numpy(hem_ref.flow(np.linalg.inv(Hm), H, W))[None].to(dev())
    img2 = ops.flow_warp(torch.from_numpy(img1)[None].to(dev()), flow_b)[0].cpu().numpy()       # img2(q) = img1(H^-1 q)
    rec = np.concatenate([np.rint(img1), np.rint(img2)]).astype(np.uint8)[None]
    ds = DGMTrainData(params((H, W), (32, 48), 4), npy_path=(), device=dev(), seed=0)
    got = ds.from_pairs(rec, Hm[None], starts=[(4, 4)])
    ref = hem_ref.batch(rec, Hm[None], [(4, 4)], (H, W), (32, 48))

    def misfit(gray, flow):
        """max |flow_warp(img2_gray, flow_gt_f) - img1_gray| away from the border"""
        back = ops.flow_warp(gray[:, 1:2].contiguous(), flow[:, 2:4].contiguous())
        return float((back - gray[:, 0:1])[:, :, m:H - m, m:W - m].abs().max())

    e_ref = misfit(torch.from_numpy(ref['imgs_gray_full']).to(dev()), torch.from_numpy(ref['flow_gt_full']).to(dev()))
    e_got = misfit(got['imgs_gray_full'], got['flow_gt_full'])
    scale = float(got['imgs_gray_full'].abs().max())
    print(f'[parity] geometric sense: max |warp(img2_gray, flow_gt_f) - img1_gray| on the interior: kernel {e_got:.3e}, '
          f'restatement {e_ref:.3e} (grey range +-{scale:.2f}); gate = 2 x restatement')
    assert 0 < e_ref < 0.1 * scale                                   # the construction itself makes sense
    assert e_got <= 2 * e_ref
    # and the other direction's sign: the backward flow moves img1 onto img2
    fwd = ops.flow_warp(got['imgs_gray_full'][:, 0:1].contiguous(), got['flow_gt_full'][:, 0:2].contiguous())
    assert float((fwd - got['imgs_gray_full'][:, 1:2])[:, :, m:H - m, m:W - m].abs().max()) < 0.1 * scale


@pytest.mark.parametrize('bad', [(15, 2), (2, 7), (-1, 2), (2, -3), (2 ** 31 - 1, -2 ** 31)], ids=str)
def test_out_of_range_start_poisons_that_sample_only(bad):
    """a start outside [0, W - pw] x [0, H - ph] is device data: NaN patches for that sample, everything else unchanged — a
    validation path, nothing is read or written out of bounds"""
    from dmhomo_amd.hem_data import DGMTrainData
    ori, crop = (22, 38), (16, 24)
    imgs, homos = make_record(3, 16, 16, seed=2)
    ds = DGMTrainData(params(ori, crop, 2), npy_path=(), device=dev(), seed=0)
    good = [(2, 2), (14, 6), (7, 3)]                                 # (14, 6): the last start that fits (rho is the caller's margin)
    want = ds.from_pairs(imgs, homos, good)
    starts = [good[0], bad, good[2]]
    got = ds.from_pairs(imgs, homos, starts)
    for k in ('imgs_gray_full', 'imgs_rgb_full', 'flow_gt_full'):
        assert torch.equal(got[k], want[k]), k
    for k in ('imgs_gray_patch', 'flow_gt_patch'):
        assert bool(torch.isnan(got[k][1]).all()), k
        assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][2], want[k][2]), k
        assert bool(torch.isfinite(want[k]).all()), k
