"""HEM training batches from sampled pairs: ``DGMTrainData`` of the reference's
``HEM/dataset/data_loader.py:97-255`` re-hosted for the MI355X — the reader of the per-sample ``{"img12", "homo12"}`` files
that ``scripts/generate_nyps_to_single_case.py`` writes, and of a ``saveTrainPair`` record straight from ``Trainer.sample``.

The reference builds every item in DataLoader workers with OpenCV and float64 numpy: two ``cv2.resize`` to ``ori_size``, the
mean / std normalisation, the grey conversion, two full-resolution homography flows and a random crop — about 16 MB of
float32 per item in six tensors.  Here the host keeps what is nine numbers per sample (``homo_scale`` and ``np.linalg.inv`` in
float64, bit for bit the reference's calls, and the crop draws of ``random.randint``) and one launch of ``dmh_hem_batch``
(csrc/hem_data.hip) writes the whole collated batch on the device from the uint8 record: 1 byte per source pixel-channel of
H2D when the record comes from files, none when it is a sampled batch.

    ds = DGMTrainData(params, npy_path='traindata/samples')      # params: crop_size, ori_size, rho
    for batch in DGMBatchLoader(ds, 32): ...                      # the dict of the reference's collated batch, device tensors
    batch = ds.from_pairs(record['imgs'], record['homos'])        # no disk in between

Deliberate deviations from the reference, also listed in INTEGRATION.md:
  * a record that already has ``ori_size`` raises ``UnboundLocalError`` there (``homo_gt_inv`` is bound only inside the resize
    branch, data_loader.py:138-140); here the inverse is always formed, which is the evident intent;
  * the file list is sorted (``glob`` order is the file system's), ``__len__`` does not print, and the crop draws come from the
    dataset's own ``random.Random(seed)`` instead of the process-wide generator (same draws for the same seed);
  * ``HomoTestData`` and ``fetch_dataloader`` are not built: they need ``cv2.imread`` and the evaluation set.
There is no CPU path: CPU tensors and a missing library raise, as everywhere in the package.
"""
import glob
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from ._lib import DmhError
from .ddpm import adapt_homography_to_preprocessing_v3

REFERENCE_GLOB = '/root/test/0521_lr5e-4_bs128/traindata/samples/*npy*'       # data_loader.py:112
KEYS = ('imgs_gray_full', 'imgs_gray_patch', 'flow_gt_full', 'flow_gt_patch', 'start', 'imgs_rgb_full')


def homo_scale(h0, w0, H, h1, w1):
    """data_loader.py:29-39 under the reference's name: the homography H of an (h0, w0) image expressed for the image resized
    to (h1, w1).  It is the function DDP:978-988 states too, so the package's one host restatement serves both (float64)."""
    return adapt_homography_to_preprocessing_v3(h0, w0, H, h1, w1)


def _device(device=None):
    return torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())


def homo_convert_to_flow(H, size=(360, 640)):
    """data_loader.py:42-52: the flow of homography H on a ``size`` = (h, w) grid, (1, 2, h, w) fp32 on the CPU as the
    reference returns it; computed by dmh_hem_flow."""
    Hm = torch.from_numpy(np.ascontiguousarray(np.asarray(H, dtype=np.float64).reshape(1, 3, 3))).to(_device())
    return ops.hem_flow(Hm, int(size[0]), int(size[1])).cpu().requires_grad_(False)


class DGMTrainData:
    """data_loader.py:97-255.  ``ds[i]`` -> the reference's item dict (device tensors, ``start`` float (2, 1, 1));
    ``ds.batch(indices)`` / ``ds.from_pairs(imgs, homos)`` -> the same dict with a leading batch dimension, one launch."""

    def __init__(self, params, phase='train', *, npy_path=None, device=None, seed=None):
        """``npy_path``: None (the reference's hard-coded glob), a directory, a glob pattern, or a sequence of file names —
        an empty one gives a dataset without files, for ``from_pairs`` / ``data_aug`` alone."""
        if phase not in ('train', 'val', 'test'):
            raise ValueError(f'phase {phase!r}: expected train, val or test')
        self.params, self.rho = params, params.rho
        self.crop_size = params.crop_size
        self.ori_h, self.ori_w = params.ori_size[:2]
        self.mean_I = np.array([118.93, 113.97, 102.60]).reshape(1, 1, 3)      # data_loader.py:103-104
        self.std_I = np.array([69.85, 68.81, 72.45]).reshape(1, 1, 3)
        if npy_path is None or isinstance(npy_path, (str, os.PathLike)):
            pattern = REFERENCE_GLOB if npy_path is None else \
                os.path.join(str(npy_path), '*npy*') if os.path.isdir(str(npy_path)) else str(npy_path)
            self.npy_path = sorted(glob.glob(pattern))
        else:
            self.npy_path = [str(f) for f in npy_path]
        self._device = device
        self.random = random.Random(seed)
        self._pool = None                      # worker threads of load_async, started on first use, ended by close()

    def close(self):
        """end the worker threads (a later ``batch`` starts new ones)"""
        pool, self._pool = getattr(self, '_pool', None), None
        if pool is not None:
            pool.shutdown(wait=True)

    def __del__(self):
        self.close()

    @property
    def device(self):
        return _device(self._device)

    def __len__(self):
        return len(self.npy_path)

    # ---- host side: the file of one sample (data_loader.py:123-128), the crop draws (224-225), the 3x3 algebra (139-140)
    def _load(self, idx):
        buf = np.load(self.npy_path[idx], allow_pickle=True).item()
        return np.asarray(buf['img12']), np.asarray(buf['homo12'], dtype=np.float64)

    def load_async(self, indices):
        """start reading the files of ``indices`` on the worker threads -> futures for ``assemble``"""
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=8)
        return [self._pool.submit(self._load, i) for i in indices]

    def draw_starts(self, n, size=None):
        """n crops as the reference draws them, item by item: x = randint(rho, W - rho - pw), then y (data_loader.py:224-225)"""
        H, W = size if size is not None else (self.ori_h, self.ori_w)
        ph, pw = self.crop_size
        out = []
        for _ in range(n):
            x = self.random.randint(self.rho, W - self.rho - pw)
            y = self.random.randint(self.rho, H - self.rho - ph)
            out.append([x, y])
        return out

    def _homographies(self, homos, h, w):
        """(B,3,3) f64 at the record's size -> (2,B,3,3): forward at ori_size, and its inverse (always formed: module docstring)"""
        fwd = [np.asarray(Hm, dtype=np.float64).reshape(3, 3) for Hm in homos]
        if h != self.ori_h or w != self.ori_w:
            fwd = [homo_scale(h, w, Hm, self.ori_h, self.ori_w) for Hm in fwd]
        return np.stack([np.stack(fwd), np.stack([np.linalg.inv(Hm) for Hm in fwd])])

    def _launch(self, imgs, both, starts, size):
        """imgs uint8 (B,6,h,w) numpy / device tensor, both (2,B,3,3) f64 numpy, starts B x (x, y) -> the batch dict"""
        if isinstance(imgs, np.ndarray):
            if imgs.dtype != np.uint8:
                raise DmhError(f'img12 must be uint8 as saveTrainPair writes it, got {imgs.dtype}')
            imgs = torch.from_numpy(np.ascontiguousarray(imgs)).to(self.device)
        elif not imgs.is_cuda:
            raise DmhError('a tensor record must live on the GPU (host records are numpy arrays); there is no CPU path')
        imgs, dev = imgs.contiguous(), imgs.device
        B = imgs.shape[0]
        st = np.asarray(starts, dtype=np.int64).reshape(B, 2)
        hh = torch.from_numpy(np.ascontiguousarray(both)).to(dev)
        s32 = torch.from_numpy(st.astype(np.int32)).to(dev)
        gray, rgb, flow, gray_p, flow_p = ops.hem_batch(imgs, hh[0], hh[1], s32, self.mean_I.ravel(), self.std_I.ravel(),
                                                        size, self.crop_size)
        start = torch.from_numpy(st.astype(np.float32).reshape(B, 2, 1, 1)).to(dev)
        return {'imgs_gray_full': gray, 'imgs_gray_patch': gray_p, 'flow_gt_full': flow, 'flow_gt_patch': flow_p,
                'start': start, 'imgs_rgb_full': rgb}

    def from_pairs(self, imgs, homos, starts=None):
        """a ``saveTrainPair`` record — imgs uint8 (B,6,h,w), numpy or a device tensor; homos (B,3,3) f64 at that size — as
        one training batch.  ``starts``: B crops (x, y) instead of drawing them."""
        if imgs.ndim != 4 or imgs.shape[1] != 6 or len(homos) != imgs.shape[0]:
            raise ValueError(f'imgs {tuple(imgs.shape)} / homos {np.shape(homos)}: expected (B,6,h,w) and (B,3,3)')
        if torch.is_tensor(homos):
            homos = homos.detach().cpu().numpy()
        B, _, h, w = imgs.shape
        both = self._homographies(homos, h, w)
        if starts is None:
            starts = self.draw_starts(B)
        return self._launch(imgs, both, starts, (self.ori_h, self.ori_w))

    def assemble(self, items, starts=None):
        """loaded (img12, homo12) items -> the batch dict; the records of one batch must share a size"""
        shapes = {it[0].shape for it in items}
        if len(shapes) != 1:
            raise ValueError(f'records of different sizes in one batch: {sorted(shapes)}')
        return self.from_pairs(np.stack([it[0] for it in items]), np.stack([it[1] for it in items]), starts)

    def batch(self, indices, starts=None):
        return self.assemble([f.result() for f in self.load_async(indices)], starts)

    def __getitem__(self, idx):
        return {k: v[0] for k, v in self.batch([idx]).items()}

    def data_aug(self, img1, img2, homo_gt, homo_gt_inv, start=None, normalize=True, gray=True):
        """data_loader.py:217-255 on uint8 (H, W, 3) images that already have their final size -> the reference's 9-tuple
        (img1, img2, img1_patch, img2_patch as (·,·,1) grey; flow_gt_b, flow_gt_f and their patches as (1,2,·,·); start),
        device tensors.  The kernel builds the normalised grey item, the one form ``__getitem__`` uses."""
        if not (normalize and gray):
            raise NotImplementedError('dmh_hem_batch builds the normalised grey item only (normalize=True, gray=True)')
        img1, img2 = np.asarray(img1), np.asarray(img2)
        if img1.dtype != np.uint8 or img2.dtype != np.uint8 or img1.shape != img2.shape or img1.shape[2:] != (3,):
            raise DmhError(f'data_aug takes two uint8 (H, W, 3) images, got {img1.dtype} {img1.shape} / {img2.dtype} {img2.shape}')
        height, width = img1.shape[:2]
        if start is None:
            start = self.draw_starts(1, (height, width))[0]
        img12 = np.concatenate((img1, img2), axis=2).transpose(2, 0, 1)[None]
        both = np.stack([np.asarray(homo_gt, dtype=np.float64).reshape(1, 3, 3),
                         np.asarray(homo_gt_inv, dtype=np.float64).reshape(1, 3, 3)])
        d = self._launch(img12, both, [start], (height, width))
        g, gp, f, fp = d['imgs_gray_full'][0], d['imgs_gray_patch'][0], d['flow_gt_full'], d['flow_gt_patch']
        return (g[0, :, :, None], g[1, :, :, None], gp[0, :, :, None], gp[1, :, :, None], f[:, 0:2], f[:, 2:4], fp[:, 0:2],
                fp[:, 2:4], [int(start[0]), int(start[1])])


class DGMBatchLoader:
    """endless batches like ``cycle(DataLoader(ds, batch_size, shuffle=True, drop_last=True))`` (fetch_dataloader,
    data_loader.py:378-387): a new permutation per epoch, the short last batch dropped (``drop_last=False`` keeps it); the
    files of the next batch are read by the dataset's worker threads while the current batch is in use."""

    def __init__(self, ds, batch_size, shuffle=True, drop_last=True, seed=0):
        if drop_last and len(ds) < batch_size:
            raise ValueError(f'{len(ds)} samples cannot fill a batch of {batch_size} (drop_last=True)')
        if len(ds) == 0:
            raise ValueError('the dataset is empty')
        self.ds, self.batch_size, self.shuffle, self.drop_last = ds, batch_size, shuffle, drop_last
        self.gen = torch.Generator().manual_seed(seed)
        self._order, self._pos = [], 0
        self._pending = None

    def _next_indices(self):
        left = len(self._order) - self._pos
        if left <= 0 or (self.drop_last and left < self.batch_size):
            n = len(self.ds)
            self._order = torch.randperm(n, generator=self.gen).tolist() if self.shuffle else list(range(n))
            self._pos = 0
        idx = self._order[self._pos:self._pos + self.batch_size]
        self._pos += self.batch_size
        return idx

    def __iter__(self):
        return self

    def __next__(self):
        cur = self._pending if self._pending is not None else self.ds.load_async(self._next_indices())
        self._pending = self.ds.load_async(self._next_indices())      # read while the caller trains on ``cur``
        return self.ds.assemble([f.result() for f in cur])
