#!/usr/bin/env python3
"""Golden fixture of the UNCONDITIONAL class's training step (ddpm.GaussianDiffusion, DDP:481-820): run the reference.

Run in the build container only (needs /root/reference, read-only):
    python tests/golden/make_golden_ddp_train.py
Same stubs / deterministic weights as make_golden.py (seed 1, as tests/test_gpu_unet.py make_ddp).  What is recorded
(data only), for two objective / loss configurations (pred_noise / l1 and pred_v / l2, both with p2_loss_weight_gamma
0.5) and three self-conditioning cases ('nosc': self_condition=False; 'sc0' / 'sc1': self_condition=True with the
`random() < 0.5` draw of DDP:785 failing / firing):

  ddp_train_step.npz
    img, t, noise                          one (3, 3, 16, 16) image batch in [0, 1] + the draws of forward / p_losses
    <cfg>.<case>.loss                      p_losses value (DDP:772-811) on normalize(img)
    <cfg>.<case>.gnorm                     || d loss / d parameter ||_2 of each whole tensor (named_parameters order),
                                           from loss.backward()
    <cfg>.<case>.grad                      SAMPLE elements of each of those gradients (all of them for smaller tensors),
                                           concatenated in the same order (the file stays small: every element of every
                                           gradient is checked against autograd by the GPU tests)
    gidx.<nosc|sc>, goff.<nosc|sc>         their flat indices within each tensor (int32, a seeded draw per tensor,
                                           concatenated) and the offsets of each tensor's run: one set per model layout
    <cfg>.<case>.grad_norm                 what clip_grad_norm_(parameters, 1.0) returns (DDP:1852)
    <cfg>.<case>.traj.loss                 loss of 4 consecutive optimiser steps (accumulate 2, clip 1.0,
                                           Adam(lr=1e-3, betas=(0.9, 0.99))) on that batch, draws held fixed
    <cfg>.<case>.traj.param_l2             || parameters ||_2 after each of those steps
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, load_det, npz  # noqa: E402

CONFIGS = (('pred_noise', 'l1'), ('pred_v', 'l2'))
CASES = (('nosc', False, 0.9), ('sc0', True, 0.9), ('sc1', True, 0.1))
SAMPLE = 32


def main():
    _, ddp = import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(171)
    B = 3
    img = torch.rand(B, 3, 16, 16, generator=g)
    tt = torch.tensor([17, 803, 440])
    nz = torch.randn(B, 3, 16, 16, generator=g)
    arrays = {'img': img, 't': tt, 'noise': nz}
    x_start = img * 2 - 1                                        # normalize_to_neg_one_to_one, DDP:819
    for obj, lt in CONFIGS:
        for case, sc, draw in CASES:
            key = f'{obj}.{lt}.{case}'
            m = ddp.Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=3, self_condition=sc)
            load_det(m, seed=1)
            d = ddp.GaussianDiffusion(m, image_size=16, timesteps=1000, objective=obj, loss_type=lt,
                                      p2_loss_weight_gamma=0.5)
            ddp.random = lambda draw=draw: draw                  # the module-level `random()` of DDP:785

            def loss_fn():
                return d.p_losses(x_start, tt, noise=nz)

            loss = loss_fn()
            loss.backward()
            arrays[key + '.loss'] = loss.detach()
            norms, vals, idxs, offs = [], [], [], [0]
            for i, (k, p) in enumerate(m.named_parameters()):
                gr = torch.zeros_like(p) if p.grad is None else p.grad.clone()
                norms.append(gr.double().norm())
                idx = torch.arange(gr.numel())
                if gr.numel() > SAMPLE:
                    idx = torch.randperm(gr.numel(), generator=torch.Generator().manual_seed(1000 + i))[:SAMPLE].sort().values
                vals.append(gr.reshape(-1)[idx])
                idxs.append(idx)
                offs.append(offs[-1] + len(idx))
            arrays[key + '.gnorm'] = torch.stack(norms)
            arrays[key + '.grad'] = torch.cat(vals)
            tag = 'sc' if sc else 'nosc'
            arrays['gidx.' + tag] = torch.cat(idxs).to(torch.int32)
            arrays['goff.' + tag] = torch.tensor(offs, dtype=torch.int32)
            arrays[key + '.grad_norm'] = torch.nn.utils.clip_grad_norm_(d.parameters(), 1.0)
            m.zero_grad()
            opt = torch.optim.Adam(d.parameters(), lr=1e-3, betas=(0.9, 0.99))
            losses, pl2 = [], []
            for _ in range(4):
                total = 0.
                for _ in range(2):
                    loss = loss_fn() / 2
                    total += loss.item()
                    loss.backward()
                torch.nn.utils.clip_grad_norm_(d.parameters(), 1.0)
                opt.step()
                opt.zero_grad()
                losses.append(total)
                pl2.append(float(torch.sqrt(sum((p.detach().double() ** 2).sum() for p in m.parameters()))))
            arrays[key + '.traj.loss'] = torch.tensor(losses, dtype=torch.float64)
            arrays[key + '.traj.param_l2'] = torch.tensor(pl2, dtype=torch.float64)
            print(key, 'loss', float(arrays[key + '.loss']), 'grad_norm', float(arrays[key + '.grad_norm']), 'traj', losses)
    npz('ddp_train_step', **arrays)


if __name__ == '__main__':
    main()
