"""CPU: the host side of the HEM training-batch path (dmhomo_amd/hem_data.py, csrc/hem_data.hip).

 * tests/hem_ref.py — the numpy restatement the GPU tests compare the kernel with — against tests/golden/hem.npz, the
   reference's own homo_scale / homo_convert_to_flow / DGMTrainData.data_aug outputs (tests/golden/make_golden_hem.py).
   The 8-bit resize is the one piece without a reference-made vector (no OpenCV in the build image): parity with cv2 UNPINNED.
 * the reference's names and signatures (surface_hem.json), the crop draws, the loader's epochs, the binding's refusals."""
import ctypes as C
import inspect
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import hem_ref

ORI, CROP, RHO, REC = (24, 40), (16, 24), 2, (16, 16)
KERNELS = ('dmh_hem_batch', 'dmh_hem_flow')


@pytest.fixture(scope='module')
def gd(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'hem.npz')))


def params(ori=ORI, crop=CROP, rho=RHO):
    return types.SimpleNamespace(crop_size=crop, ori_size=ori, rho=rho)


# ------------------------------------------------------------------ the restatement against the reference's outputs
def test_ref_homo_scale_matches_the_reference(gd):
    from dmhomo_amd import hem_data
    for fn in (hem_ref.homo_scale, hem_data.homo_scale):
        got = np.stack([fn(REC[0], REC[1], Hm, ORI[0], ORI[1]) for Hm in gd['homos']])
        assert got.dtype == np.float64
        assert np.allclose(got, gd['homo_scale'], rtol=1e-12, atol=0)          # same numpy calls; BLAS builds may differ in the last bits


def test_ref_flow_matches_the_reference(gd):
    assert (np.abs(gd['homos'][:, 2, :2]) > 1e-5).all()                        # the perspective row is exercised
    for k in range(3):
        hem_ref.assert_flow_close(f'hem_ref.flow[{k}] vs reference', hem_ref.flow(gd['homo_scale'][k], *ORI), gd['flows'][k])


@pytest.mark.parametrize('tag', ['fixed', 'seeded'])
def test_ref_batch_matches_the_reference_data_aug(gd, tag):
    """every output of the reference's data_aug from the restatement: grey tensors bit-equal (pure IEEE float64), flows within
    one fp32 ulp of the mapped coordinate, patches the reference's windows"""
    img12 = np.concatenate([gd['img1_u8'], gd['img2_u8']], axis=2).transpose(2, 0, 1)[None]
    start = [int(v) for v in gd[f'{tag}.start']]
    ds = None
    if tag == 'seeded':                                                        # random.Random(7) draws what random.seed(7) drew
        from dmhomo_amd.hem_data import DGMTrainData
        ds = DGMTrainData(params(), npy_path=(), seed=7)
        assert ds.draw_starts(1) == [start] == [[7, 3]]
    got = hem_ref.batch(img12, gd[f'{tag}.homo'][None], [start], ORI, CROP)
    for i, name in enumerate(('img1', 'img2')):
        assert np.array_equal(got['imgs_gray_full'][0, i], gd[f'{tag}.{name}'][:, :, 0]), name
        assert np.array_equal(got['imgs_gray_patch'][0, i], gd[f'{tag}.{name}_patch'][:, :, 0]), name
    for i, name in enumerate(('flow_gt_b', 'flow_gt_f')):
        hem_ref.assert_flow_close(f'{tag}.{name}', got['flow_gt_full'][0, 2 * i:2 * i + 2], gd[f'{tag}.{name}'][0])
        hem_ref.assert_flow_close(f'{tag}.{name}_patch', got['flow_gt_patch'][0, 2 * i:2 * i + 2], gd[f'{tag}.{name}_patch'][0])
    assert got['start'].reshape(2).tolist() == gd[f'{tag}.start'].tolist()
    assert got['imgs_gray_patch'].shape == (1, 2) + CROP and got['flow_gt_patch'].shape == (1, 4) + CROP


def test_ref_resize_properties():
    """no reference vector exists for the 8-bit resize; what can be said without one: identity at equal size, constants stay
    constant, the clamped edge columns see their own source column only, and two pixels worked out by hand (one of them on the
    top row, where the vertical fraction is kept and only the row indices are clipped)"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(6, 16, 16), dtype=np.uint8)
    assert np.array_equal(hem_ref.resize_u8(a, 16, 16), a)
    for v in (0, 1, 127, 255):
        assert (hem_ref.resize_u8(np.full((1, 5, 7), v, np.uint8), 22, 38) == v).all()
    up = hem_ref.resize_u8(a, 22, 38)
    assert up.shape == (6, 22, 38) and up.dtype == np.uint8
    # left / right columns: fraction clamped with the index -> the source's edge columns resized vertically only
    col = hem_ref.resize_u8(a[:, :, :1].repeat(2, axis=2), 22, 2)
    assert np.array_equal(up[:, :, 0], col[:, :, 0])
    # two pixels by hand, 2 x 2 -> 4 x 4.  (dy, dx) = (0, 1): fx = 0.25 -> a = (1536, 512); fy = -0.25 -> sy = -1, fraction 0.75
    # kept (b = (512, 1536)), both rows clipped to row 0: S = 255 * 512, S >> 4 = 8160, (512 * 8160 >> 16) + (1536 * 8160 >> 16)
    # = 63 + 191, (254 + 2) >> 2 = 64.  (1, 1): b = (1536, 512), S0 >> 4 = 8160, S1 >> 4 = 24480: 191 + 191, (382 + 2) >> 2 = 96.
    t = hem_ref.resize_u8(np.array([[[0, 255], [255, 0]]], np.uint8), 4, 4)[0]
    assert t[0, 1] == 64 and t[1, 1] == 96 and t[0, 0] == 0 and t[0, 3] == 255 and np.array_equal(t, t.T)
    # a pixel that tells the unclamped vertical fraction from a clamped one, 2 x 2 -> 4 x 3 of rows [0, 1]: dx = 1 has fx = 0.5,
    # a = (1024, 1024), S = 1024, S >> 4 = 64 on both (clipped) rows.  dy = 0: sy = -1 with the fraction 0.75 KEPT, b = (512, 1536):
    # (512 * 64 >> 16) + (1536 * 64 >> 16) = 0 + 1, (1 + 2) >> 2 = 0.  Clamping the fraction with the index (b = (2048, 0)) would
    # give (2048 * 64 >> 16) = 2, (2 + 2) >> 2 = 1.
    t = hem_ref.resize_u8(np.array([[[0, 1], [0, 1]]], np.uint8), 4, 3)[0]
    assert t[0, 1] == 0 and t[0].tolist() == [0, 0, 1]


# ------------------------------------------------------------------ the public surface
def test_signatures_match_the_reference(golden_dir):
    from dmhomo_amd import hem_data
    with open(os.path.join(golden_dir, 'surface_hem.json')) as f:
        want = json.load(f)
    assert sorted(want) == ['DGMTrainData.__init__', 'DGMTrainData.data_aug', 'homo_convert_to_flow', 'homo_scale']
    assert str(inspect.signature(hem_data.homo_scale)) == want['homo_scale']
    assert str(inspect.signature(hem_data.homo_convert_to_flow)) == want['homo_convert_to_flow']
    assert str(inspect.signature(hem_data.DGMTrainData.data_aug)) == want['DGMTrainData.data_aug']
    # the constructor: the reference's parameters, then keyword-only additions (npy_path, device, seed)
    sig = inspect.signature(hem_data.DGMTrainData.__init__)
    extra = [p for p in sig.parameters.values() if p.kind is p.KEYWORD_ONLY]
    assert [p.name for p in extra] == ['npy_path', 'device', 'seed'] and all(p.default is None for p in extra)
    base = sig.replace(parameters=[p for p in sig.parameters.values() if p.kind is not p.KEYWORD_ONLY])
    assert str(base) == want['DGMTrainData.__init__']


def test_dataset_constants_and_file_list(tmp_path):
    from dmhomo_amd.hem_data import DGMTrainData, REFERENCE_GLOB
    for i in (3, 1, 2):
        np.save(str(tmp_path / f'{i}.npy'), {'img12': np.zeros((6, 4, 4), np.uint8), 'homo12': np.eye(3)})
    (tmp_path / 'notes.txt').write_text('x')
    ds = DGMTrainData(params(), npy_path=str(tmp_path))
    assert len(ds) == 3 and [os.path.basename(p) for p in ds.npy_path] == ['1.npy', '2.npy', '3.npy']
    assert len(DGMTrainData(params(), npy_path=str(tmp_path / '[12].npy'))) == 2          # a glob
    assert REFERENCE_GLOB.endswith('traindata/samples/*npy*')
    assert ds.mean_I.shape == ds.std_I.shape == (1, 1, 3)
    assert ds.mean_I.ravel().tolist() == [118.93, 113.97, 102.60] and ds.std_I.ravel().tolist() == [69.85, 68.81, 72.45]
    assert (ds.crop_size, ds.ori_h, ds.ori_w, ds.rho) == (CROP, 24, 40, 2)
    img12, homo = ds._load(1)
    assert img12.shape == (6, 4, 4) and img12.dtype == np.uint8 and homo.dtype == np.float64


def test_dataset_without_files_and_explicit_file_list(tmp_path):
    from dmhomo_amd.hem_data import DGMTrainData, DGMBatchLoader
    ds = DGMTrainData(params(), npy_path=())
    assert len(ds) == 0 and ds.npy_path == []
    with pytest.raises(ValueError):
        DGMBatchLoader(ds, 1)
    with pytest.raises(ValueError):
        DGMTrainData(params(), phase='train2')
    files = []
    for i in (2, 1):
        files.append(str(tmp_path / f'{i}.npy'))
        np.save(files[-1], {'img12': np.full((6, 4, 4), i, np.uint8), 'homo12': np.eye(3) * i})
    ds = DGMTrainData(params(), npy_path=files)                   # a sequence keeps its order
    assert len(ds) == 2 and ds.npy_path == files and ds._pool is None
    got = [f.result() for f in ds.load_async([0, 1])]
    assert [int(g[0][0, 0, 0]) for g in got] == [2, 1] and ds._pool is not None
    ds.close()
    assert ds._pool is None
    assert int(ds.load_async([1])[0].result()[1][0, 0]) == 1      # a later read starts new worker threads
    ds.close()


def test_crop_draws_follow_the_reference_order_and_bounds():
    """per item x = randint(rho, W - rho - pw), then y = randint(rho, H - rho - ph), from the dataset's own generator"""
    from dmhomo_amd.hem_data import DGMTrainData
    for ori, crop, rho, seed in ((ORI, CROP, 2, 7), ((360, 640), (320, 576), 16, 0), ((22, 38), (16, 24), 2, 11)):
        ds = DGMTrainData(params(ori, crop, rho), npy_path=(), seed=seed)
        r = random.Random(seed)
        want = []
        for _ in range(64):
            x = r.randint(rho, ori[1] - rho - crop[1])
            want.append([x, r.randint(rho, ori[0] - rho - crop[0])])
        got = ds.draw_starts(40) + ds.draw_starts(24)
        assert got == want
        xs, ys = np.array(got).T
        assert xs.min() >= rho and xs.max() <= ori[1] - rho - crop[1] and ys.min() >= rho and ys.max() <= ori[0] - rho - crop[0]
    random.seed(5)
    state = random.getstate()
    DGMTrainData(params(), npy_path=(), seed=1).draw_starts(3)
    assert random.getstate() == state                                        # the process-wide generator is left alone


class _FakeDs:
    """what DGMBatchLoader needs of a dataset, without files or a device"""

    def __init__(self, n):
        self.n, self.loaded = n, []

    def __len__(self):
        return self.n

    def load_async(self, indices):
        self.loaded.append(list(indices))
        return [types.SimpleNamespace(result=lambda i=i: i) for i in indices]

    def assemble(self, items):
        return list(items)


def test_loader_epochs_permutation_and_drop_last():
    from dmhomo_amd.hem_data import DGMBatchLoader
    ds = _FakeDs(7)
    dl = DGMBatchLoader(ds, 3, shuffle=True, drop_last=True, seed=1)
    batches = [next(dl) for _ in range(6)]
    assert all(len(b) == 3 for b in batches)                                  # the short last batch never shows
    e0, e1, e2 = (batches[0] + batches[1], batches[2] + batches[3], batches[4] + batches[5])
    for e in (e0, e1, e2):
        assert len(set(e)) == 6 and set(e) <= set(range(7))                   # six different samples of one permutation
    g = torch.Generator().manual_seed(1)
    assert e0 == torch.randperm(7, generator=g).tolist()[:6] and e1 == torch.randperm(7, generator=g).tolist()[:6]
    assert e0 != e1                                                           # a new permutation per epoch
    assert ds.loaded[:len(batches) + 1][-1] is not None and len(ds.loaded) == len(batches) + 1   # one batch read ahead
    # drop_last=False keeps the short batch; shuffle=False keeps file order
    dl = DGMBatchLoader(_FakeDs(7), 3, shuffle=False, drop_last=False)
    assert [next(dl) for _ in range(4)] == [[0, 1, 2], [3, 4, 5], [6], [0, 1, 2]]
    dl = DGMBatchLoader(_FakeDs(6), 3, shuffle=False)
    assert [next(dl) for _ in range(3)] == [[0, 1, 2], [3, 4, 5], [0, 1, 2]]
    with pytest.raises(ValueError):
        DGMBatchLoader(_FakeDs(2), 3)
    with pytest.raises(ValueError):
        DGMBatchLoader(_FakeDs(0), 3, drop_last=False)
    assert str(inspect.signature(DGMBatchLoader.__init__)) == '(self, ds, batch_size, shuffle=True, drop_last=True, seed=0)'


# ------------------------------------------------------------------ the binding
def test_header_and_binding_hold_the_hem_kernels():
    import re
    from dmhomo_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'dmhomo_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(dmh_[a-z0-9_]+)\s*\(', src))
    lib = _lib.lib()
    for name in KERNELS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and args[-1] is C.c_void_p                  # status code; the stream goes last
    assert _lib.ABI_VERSION == 500 == lib.dmh_version()                      # additive: the version stays


def test_cpu_tensors_are_refused():
    from dmhomo_amd import ops, _lib
    from dmhomo_amd.hem_data import DGMTrainData
    img = torch.zeros((1, 6, 8, 8), dtype=torch.uint8)
    Hm = torch.eye(3, dtype=torch.float64)[None]
    with pytest.raises(_lib.DmhError):
        ops.hem_batch(img, Hm, Hm, torch.zeros((1, 2), dtype=torch.int32), [1., 1., 1.], [1., 1., 1.], (8, 8), (4, 4))
    with pytest.raises(_lib.DmhError):
        ops.hem_flow(Hm, 8, 8)
    ds = DGMTrainData(params((8, 8), (4, 4), 1), npy_path=(), seed=0)
    with pytest.raises(_lib.DmhError):
        ds.from_pairs(img, np.eye(3)[None])
    with pytest.raises(_lib.DmhError):
        ds.from_pairs(np.zeros((1, 6, 8, 8), np.float32), np.eye(3)[None])  # a record is uint8
    with pytest.raises(NotImplementedError):
        ds.data_aug(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), np.eye(3), np.eye(3), gray=False)


def _hem_batch_args(lib_types, p, B=2, h=16, w=16, H=22, W=38, ph=16, pw=24):
    ints = iter((B, h, w, H, W, ph, pw))
    return [next(ints) if t is lib_types.c_int else p for t in lib_types.SIGNATURES['dmh_hem_batch'][1]]


def test_hem_kernels_refuse_bad_arguments():
    """NULL pointers, zero / negative / overflowing sizes, a crop larger than the output and an unaligned output answer through
    the error channel (every case is refused by the validator: nothing is launched, with or without a GPU)"""
    from dmhomo_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * 256)()
    hp = C.c_void_p((C.addressof(buf) + 15) & ~15)
    for name in KERNELS:
        _, argtypes = _lib.SIGNATURES[name]
        for ival, p in ((4, None), (0, hp), (-1, hp), (2 ** 30, hp), (2 ** 16, hp)):
            args = [ival if t is _lib.c_int else p for t in argtypes]
            assert getattr(lib, name)(*args) == -1, (name, ival, p)
            assert name.encode() in lib.dmh_last_error()
    # each pointer of dmh_hem_batch on its own
    argtypes = _lib.SIGNATURES['dmh_hem_batch'][1]
    for k, t in enumerate(argtypes[:-1]):
        if t is _lib.c_int:
            continue
        args = _hem_batch_args(_lib, hp)
        args[k] = None
        assert lib.dmh_hem_batch(*args) == -1 and b'null pointer' in lib.dmh_last_error(), k
    # each size of it at zero, and the crop against the output
    for kw in (dict(B=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(ph=0), dict(pw=0), dict(B=65536)):
        assert lib.dmh_hem_batch(*_hem_batch_args(_lib, hp, **kw)) == -1, kw
    for kw in (dict(ph=23), dict(pw=39), dict(ph=23, pw=39)):
        assert lib.dmh_hem_batch(*_hem_batch_args(_lib, hp, **kw)) == -1 and b'crop' in lib.dmh_last_error(), kw
    assert lib.dmh_hem_batch(*_hem_batch_args(_lib, hp, B=1 << 10, H=1 << 10, W=1 << 10)) == -1     # B*6*H*W >= 2^31
    odd = C.c_void_p(hp.value + 4)
    args = _hem_batch_args(_lib, hp)
    args[14] = odd                                                           # imgs_rgb_full
    assert lib.dmh_hem_batch(*args) == -1 and b'aligned' in lib.dmh_last_error()
    assert lib.dmh_hem_flow(hp, 1, 4, 4, odd, None) == -1 and b'aligned' in lib.dmh_last_error()
    assert lib.dmh_hem_flow(None, 1, 4, 4, hp, None) == -1 and lib.dmh_hem_flow(hp, 1, 4, 4, None, None) == -1
