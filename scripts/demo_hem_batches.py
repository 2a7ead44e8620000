#!/usr/bin/env python3
"""The last link of the chain: sample one batch of pairs with ``Trainer.sample`` (as scripts/dgm_sample.py does) and serve the
record as one HEM training batch with ``DGMTrainData.from_pairs`` — no file in between.

    python scripts/demo_hem_batches.py [-c DGM] [--bs 4] [--image_size 128] [--s_step 8] [--dim 64] [--seed 0]

Prints the shape of every tensor of the batch (the dict HEM/train.py's loop reads from its DataLoader: ``ori_size`` (360, 640),
``crop_size`` (320, 576), ``rho`` 16) and the statistics of ``flow_gt_patch``.  Without results/model-<c>.pt the seeded random
initialisation is sampled: the images are noise-like, the homographies and everything built from them are not.
"""
import argparse
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmhomo_amd.denoising_diffusion_models.denoising_diffusion_pytorch import Trainer  # noqa: E402
from dmhomo_amd.denoising_diffusion_models.classifier_free_guidance import Unet, GaussianDiffusion  # noqa: E402
from dmhomo_amd.hem_data import DGMTrainData  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('-c', type=str, default='None')
parser.add_argument('--bs', type=int, default=4)
parser.add_argument('--image_size', type=int, default=128)
parser.add_argument('--s_step', type=int, default=8)
parser.add_argument('--dim', type=int, default=64)
parser.add_argument('--seed', type=int, default=0)
args = parser.parse_args()


def main():
    device = torch.device('cuda', 0)
    torch.manual_seed(args.seed)
    model = Unet(dim=args.dim, dim_mults=(1, 2, 4, 8), channels=6, num_classes=1).to(device)
    diffusion = GaussianDiffusion(model, image_size=args.image_size, timesteps=1000, sampling_timesteps=args.s_step,
                                  loss_type='l1', objective='pred_x0').to(device)
    trainer = Trainer(diffusion, 'DGM_Conditions', train_batch_size=args.bs, train_num_steps=1, results_folder='results',
                      augment_horizontal_flip=False, num_worker=0, shuffle=False, split_batches=False)
    if os.path.exists(os.path.join('results', f'model-{args.c}.pt')):
        trainer.load(args.c)
    else:
        print(f'results/model-{args.c}.pt not found: sampling from the seeded random initialisation')
    record = trainer.sample(0, device)                     # {"imgs": uint8 (B,6,S,S), "homos": float64 (B,3,3)}
    print(f'record: imgs {record["imgs"].dtype} {record["imgs"].shape}, homos {record["homos"].dtype} {record["homos"].shape}')

    params = types.SimpleNamespace(crop_size=(320, 576), ori_size=(360, 640), rho=16)
    ds = DGMTrainData(params, npy_path=(), device=device, seed=args.seed)
    batch = ds.from_pairs(record['imgs'], record['homos'].reshape(-1, 3, 3))
    for k, v in batch.items():
        print(f'{k:16s} {tuple(v.shape)} {v.dtype} {v.device}')
    print('start (x, y):', batch['start'].reshape(-1, 2).tolist())
    fp = batch['flow_gt_patch']
    for name, sl in (('backward (homo_inv)', fp[:, 0:2]), ('forward  (homo)', fp[:, 2:4])):
        print(f'flow_gt_patch {name}: mean {float(sl.mean()):+.3f} std {float(sl.std()):.3f} '
              f'min {float(sl.min()):+.3f} max {float(sl.max()):+.3f} px, finite {bool(torch.isfinite(sl).all())}')


if __name__ == '__main__':
    main()
