#!/usr/bin/env python3
"""Drop-in counterpart of the reference's DGM/dgm_sample.py on dmhomo_amd (same CLI flags, same output format).

    python scripts/dgm_sample.py -c DGM --s_step 32 --bs 25 --exp run0 [--image_size 256] [--batches 2] [--preview] [--sampler dpmpp_2m] [--clip_mode dynamic] [--guidance_rescale 0.7] [--guidance_interval 0.25 0.75] [--apg_eta 0 --apg_norm_threshold 15 --apg_momentum -0.5] [--photo_guidance 0.5] [--flow_guidance 2] [--pag_scale 3] [--keep source --known_resample 2] [--strength 0.5] [--relabel identity --relabel_seed 1 --relabel_ranges .03 8 3e-5]

Differences from the reference script (DGM/dgm_sample.py:11-101), all forced by what is available offline:
  * conditions come from dmhomo_amd.ddpm.SyntheticConditions (the CA-Homo dataset of DDP:1058-1066 is not
    shipped) unless --conditions points at a .pt file holding an iterable of (12-channel batch, classes);
  * -c names results/model-<c>.pt like the reference; when the file does not exist the seeded random
    initialisation is used (the trained DGM.pt lives on HuggingFace, README:8);
  * the loop stops after --batches batches instead of running until killed (SAMPLE:62);
  * --sampler dpmpp_2m replaces the DDIM update with the second-order multistep solver (an addition: the reference has
    DDIM only); the default, ddim, is the reference's loop;
  * --clip_mode dynamic replaces the clamp of every step's x_start to [-1, 1] by dynamic thresholding at the
    --dynamic_threshold_percentile-th percentile of each sample's |x_start| (an addition: the reference clamps); the default,
    static, is the reference's clamp;
  * --guidance_rescale PHI in (0, 1] rescales every step's guided blend towards the standard deviation of its conditional
    output (rescaled classifier-free guidance, Lin et al. 2024; an addition); the default, 0, is the reference's blend;
  * --guidance_interval LO HI applies the guidance only at the entries whose normalised time t / (T - 1) lies in [LO, HI]; the
    others run the conditional pass alone, at half the UNet rows (limited-interval guidance, Kynkaanniemi et al. 2024; an
    addition); the default, off, guides every entry as the reference does;
  * --apg_eta ETA in [0, 1] replaces the guided blend by adaptive projected guidance (Sadat et al. 2024; an addition): the part of
    cond - null parallel to the conditional output is weighted by ETA, --apg_norm_threshold RHO > 0 caps the update's norm per
    sample and --apg_momentum BETA in (-1, 1) averages it over the steps; the default, off, is the reference's blend.  Not
    together with --guidance_rescale or --guidance_interval;
  * --photo_guidance W in (0, 1] moves every step's predicted pair down the gradient of the photometric term of the training
    loss, mask * (flow_warp(im2, flow) - im1) ** 2, by W * alpha_bar_t (photometric-consistency guidance; an addition), and
    prints each batch's mean dmhomo_amd.ddpm.photometric_error; the default, off, is the reference's sampler, which ignores the
    flow.  Not together with --guidance_rescale, --guidance_interval or --apg_eta;
  * --flow_guidance S >= 0 guides on the homography condition itself (classifier-free guidance with two scales, as InstructPix2Pix;
    an addition): every step also runs the network without rgb_flow and moves the logits by (S - 1) times the difference; 1 is
    the unguided sampler at the cost of the extra pass, the default, off, is the reference's sampler.  It asks for a checkpoint
    trained with demo.py --flow_drop_prob (otherwise the no-flow pass is out of distribution).  Not together with
    --guidance_interval; the passes then run as one batched launch sequence (cfg_mode = 'batched');
  * --pag_scale S >= 0 turns on perturbed-attention guidance (Ahn et al. 2024; an addition): every step also runs the network
    with the bottleneck self-attention map replaced by the identity and moves the logits by S times the difference to that
    structurally degraded prediction; it needs no label and no retraining, so it works on any existing checkpoint; 0 is the
    unguided sampler at the cost of the extra pass, the default, off, is the reference's sampler.  Not together with
    --flow_guidance or --guidance_interval; the passes then run as one batched launch sequence (cfg_mode = 'batched');
  * --keep source|target keeps that image of every batch's own pair (channels 0-5 of a dataset batch) and generates only the
    other one around it (GaussianDiffusion.sample_known; an addition): the kept image's bytes in the record are the batch's;
    --known_resample R >= 1 runs every entry of the time list R times (RePaint's harmonisation with jump length 1, Lugmayr et
    al. 2022; R times the UNet passes); each batch's mean known-pixel score — how far the model's final prediction is from the
    pixels it was told to keep — is printed.  With SyntheticConditions, whose image channels are zeros, the switch pins a black
    image: it is meant for --conditions / a dataset folder.  Not together with --clip_mode dynamic or --guidance_rescale, and
    --known_resample > 1 not with --sampler dpmpp_2m; the default, off, is the reference's sampler;
  * --strength F in (0, 1] starts every batch from its own pair (channels 0-5 of a dataset batch) noised to an intermediate time
    instead of from pure noise, and runs only the last floor(s_step * F) entries of the time list (GaussianDiffusion.sample_from —
    SDEdit, Meng et al. 2022; an addition): the real scene, re-labelled under the batch's homography condition, at F times the
    UNet passes; 1 runs every entry.  Together with --keep the kept image stays the batch's and the other one starts from the
    batch's.  With SyntheticConditions, whose image channels are zeros, the start is a noised black pair: the flag is meant for
    --conditions / a dataset folder.  A strength below 1 / s_step runs no entry and is refused; the default, off, is the
    reference's sampler;
  * --relabel identity|batch replaces every batch, directly behind the loader, by the same real source images under NEW homography
    labels drawn on the device (dmhomo_amd.ddpm.relabel_batch, one launch; an addition): per sample a perturbation in
    SyntheticConditions' parameterisation — --relabel_ranges A T P bound its affine entries, its shift in pixels of the 360 x 640
    frame and its perspective entries, default .03 8 3e-5 — taken as the label itself (identity) or applied on top of the batch's
    own homography (batch), with its flow and flow image, and the source warped by it in place of the batch's target.  The draw
    is keyed by --relabel_seed (default: --seed) and the global sample index, like the noise, so a job's labels do not depend on
    the number of ranks.  With --keep source --strength F the record holds the real source and a target generated under the
    fresh label, started from the warped source, at F times the UNet passes: finite real scenes yield unlimited labels.  Not
    together with --keep target (the batch's target belongs to the old label).  With SyntheticConditions, whose image channels
    are zeros, the images are black: the flag is meant for --conditions / a dataset folder.  Sample quality with trained weights:
    not measured.  The default, off, leaves every batch as the loader dealt it;
  * --preview turns on the flow-remap and homography-warp sheets the reference always writes under
    generate_training_pairs/ when its step counter is a multiple of 100 (DDP:1972-2019); off by default;
  * multi-GPU: launch with torch.distributed.run instead of N hand-started processes (--gpu_nums / -i are
    still accepted and select the data slice exactly as the reference's unused arguments did: not at all); rank 0
    alone reads the checkpoint and broadcasts the online + EMA weights over RCCL (the reference's N processes each
    load the file, SAMPLE:54); sampling replays one captured denoise step from a HIP graph, with the conditional pass's
    dropped rows not computed (cfg.Unet.dedup_dropped_rows: the same samples bit for bit); noise is keyed by --seed and
    the global sample index (dmh_rng_indexed).  With the synthetic conditions sample g of the job is also BUILT from
    g (ddpm.SyntheticConditions), so N processes write, between them, exactly the records one process writes in N times
    as many batches (tests/test_gpu_distributed.py).  With a dataset folder the loader deals rows to ranks in strides
    (dataset.ConditionLoader, as accelerate's sharded DataLoader does) while noise ids are contiguous per rank: the
    records are reproducible for a given N, but which noise meets which image depends on N.
Output: traindata/<exp>/dataset/idx_<i>_rank_<r>_part_<p>_dm_cahomo_<k>k.npy — a pickled list of
{"imgs": uint8 (B,6,H,W), "homos": float64 (B,3,3)} every 2 batches (SAMPLE:73-77), the format
HEM/dataset/data_loader.py:123-131 consumes.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmhomo_amd.denoising_diffusion_models.denoising_diffusion_pytorch import Trainer  # noqa: E402
from dmhomo_amd.denoising_diffusion_models.classifier_free_guidance import Unet, GaussianDiffusion  # noqa: E402
from dmhomo_amd import distributed as D  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('-c', type=str, default='None')
parser.add_argument('--gpu_nums', type=int, default=0)
parser.add_argument('--s_step', type=int, default=0)
parser.add_argument('--part', type=int, default=0)
parser.add_argument('--bs', type=int, default=80)
parser.add_argument('--exp', type=str, default='exp')
parser.add_argument('-i', type=int, default=0)
parser.add_argument('--image_size', type=int, default=256)        # SAMPLE:32 hard-codes 256
parser.add_argument('--batches', type=int, default=2)
parser.add_argument('--conditions', type=str, default=None)
parser.add_argument('--preview', action='store_true', help='write preview sheets when the step counter is a multiple of 100')
parser.add_argument('--seed', type=int, default=0, help='noise seed (every value is keyed by seed and global sample index)')
parser.add_argument('--sampler', choices=('ddim', 'dpmpp_2m'), default='ddim',
                    help="the update over the --s_step time list: the reference's DDIM, or the second-order multistep solver "
                         "DPM-Solver++ 2M (deterministic, not in the reference; ScheduleHost.sampler)")
parser.add_argument('--clip_mode', choices=('static', 'dynamic'), default='static',
                    help="what a step does to x_start: the reference's clamp to [-1, 1], or dynamic thresholding (Saharia et al. "
                         "2022; not in the reference; ScheduleHost.clip_mode)")
parser.add_argument('--dynamic_threshold_percentile', type=float, default=0.995,
                    help='the percentile of |x_start| per sample that --clip_mode dynamic clamps at, in (0, 1]')
parser.add_argument('--guidance_rescale', type=float, default=0.,
                    help='phi of rescaled classifier-free guidance in [0, 1] (Lin et al. 2024 use 0.7; not in the reference; '
                         'ScheduleHost.guidance_rescale); 0: off')
parser.add_argument('--guidance_interval', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                    help='guide only where LO <= t / (T - 1) <= HI, 0 <= LO <= HI <= 1 (Kynkaanniemi et al. 2024; not in the '
                         'reference; ScheduleHost.guidance_interval); default: every entry')
parser.add_argument('--apg_eta', type=float, default=None,
                    help='weight in [0, 1] of the part of the guidance update parallel to the conditional output: adaptive projected '
                         'guidance (Sadat et al. 2024 use 0; not in the reference; GaussianDiffusion.apg_eta); default: off')
parser.add_argument('--apg_norm_threshold', type=float, default=0.,
                    help='with --apg_eta: cap of the norm of the guidance update per sample, >= 0; 0: no cap')
parser.add_argument('--apg_momentum', type=float, default=0.,
                    help='with --apg_eta: momentum in (-1, 1) of the running average of the update (the paper uses -0.5); 0: none')
parser.add_argument('--photo_guidance', type=float, default=None,
                    help='weight in (0, 1] of photometric-consistency guidance: every step moves its predicted pair towards '
                         'flow_warp(im2, flow) == im1 under the mask (not in the reference; GaussianDiffusion.photo_guidance); '
                         'default: off')
parser.add_argument('--flow_guidance', type=float, default=None,
                    help='scale >= 0 of classifier-free guidance on the flow condition: every step also runs a pass without '
                         'rgb_flow (not in the reference; GaussianDiffusion.flow_guidance); default: off')
parser.add_argument('--pag_scale', type=float, default=None,
                    help='scale >= 0 of perturbed-attention guidance: every step also runs a pass whose bottleneck self-attention '
                         'map is the identity (not in the reference; GaussianDiffusion.pag_scale); default: off')
parser.add_argument('--keep', choices=('source', 'target'), default=None,
                    help="keep this image of every batch's own pair and generate the other one around it (not in the reference; "
                         "GaussianDiffusion.sample_known, Trainer.keep); default: off")
parser.add_argument('--known_resample', type=int, default=1,
                    help='with --keep: run every entry of the time list this many times (RePaint, jump length 1; '
                         'ScheduleHost.known_resample); 1: none')
parser.add_argument('--strength', type=float, default=None,
                    help="start every batch from its own pair noised to an intermediate time and run the last floor(s_step * "
                         "STRENGTH) entries only, STRENGTH in (0, 1] (SDEdit; not in the reference; GaussianDiffusion.sample_from, "
                         "Trainer.strength); default: off")
parser.add_argument('--relabel', choices=('identity', 'batch'), default=None,
                    help="draw a new homography label per sample on the device and sample every batch under it: the label is the "
                         "drawn perturbation (identity) or the perturbation on top of the batch's own homography (batch); meant "
                         "for --conditions / a dataset folder — with SyntheticConditions the images are black (not in the "
                         "reference; ddpm.relabel_batch, Trainer.relabel); default: off")
parser.add_argument('--relabel_seed', type=int, default=None, help='with --relabel: seed of the label draw; default: --seed')
parser.add_argument('--relabel_ranges', type=float, nargs=3, default=None, metavar=('A', 'T', 'P'),
                    help='with --relabel: bounds of the affine entries (< 0.25), the shift in pixels of the 360 x 640 frame and the '
                         'perspective entries (< 5e-4) of the drawn perturbation; default: .03 8 3e-5')
args = parser.parse_args()

num_classes = 1


def main():
    rank, world, device = D.init_from_env()
    torch.manual_seed(args.seed)         # (the initialisation used when no checkpoint is found; torch seeds its CPU generator at random)
    model = Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=6, num_classes=num_classes).to(device)
    model.cfg_mode = 'streams'
    diffusion = GaussianDiffusion(model, image_size=args.image_size, timesteps=1000, sampling_timesteps=args.s_step,
                                  loss_type='l1', objective='pred_x0').to(device)
    folder = torch.load(args.conditions) if args.conditions else 'DGM_Conditions'
    trainer = Trainer(diffusion, folder, train_batch_size=args.bs, train_lr=1e-4, train_num_steps=200000,
                      gradient_accumulate_every=2, ema_decay=0.995, amp=False, results_folder='results',
                      save_and_sample_every=2000, num_samples=4, augment_horizontal_flip=False, num_worker=0,
                      total_data_slice_idx=args.gpu_nums, data_slice_idx=args.i, shuffle=False,
                      split_batches=False)     # --bs is PER PROCESS, as for the reference's hand-started processes (SAMPLE:13-18)
    trainer.preview = args.preview
    # rank 0 alone reads the checkpoint; the online and the EMA copy reach the other ranks as one RCCL payload each
    have = os.path.exists(os.path.join('results', f'model-{args.c}.pt')) if rank == 0 else None
    if not D.load_on_rank0_and_broadcast(trainer, args.c if have else None):
        if rank == 0:
            print(f'results/model-{args.c}.pt not found: sampling from the seeded random initialisation')
    sampler = trainer.ema.ema_model                        # what Trainer.sample draws from (DDP:1960)
    sampler.model.cfg_mode = 'streams'
    sampler.hip_graph = True                               # one captured denoise step replayed s_step times
    sampler.sampler = args.sampler
    sampler.clip_mode, sampler.dynamic_threshold_percentile = args.clip_mode, args.dynamic_threshold_percentile
    sampler.guidance_rescale = args.guidance_rescale
    sampler.guidance_interval = None if args.guidance_interval is None else tuple(args.guidance_interval)
    sampler.apg_eta, sampler.apg_norm_threshold, sampler.apg_momentum = args.apg_eta, args.apg_norm_threshold, args.apg_momentum
    sampler.photo_guidance = args.photo_guidance
    sampler.flow_guidance = args.flow_guidance
    if args.flow_guidance is not None:
        sampler.model.cfg_mode = 'batched'                 # the third pass rides in the one batched launch sequence
    sampler.pag_scale = args.pag_scale
    if args.pag_scale is not None:
        sampler.model.cfg_mode = 'batched'                 # the perturbed pass rides in the one batched launch sequence
    trainer.score_photometric = args.photo_guidance is not None
    trainer.keep, sampler.known_resample = args.keep, args.known_resample
    trainer.score_known = args.keep is not None
    trainer.strength = args.strength
    trainer.relabel = args.relabel
    trainer.relabel_seed = args.seed if args.relabel_seed is None else args.relabel_seed
    if args.relabel_ranges is not None:
        trainer.relabel_ranges = tuple(args.relabel_ranges)
    sampler.model.dedup_dropped_rows = True                # CFG:404,415-425: dropped conditional rows == null rows, not computed
    out_dir = f'traindata/{args.exp}/dataset/'
    os.makedirs(out_dir, exist_ok=True)
    train_list, part = [], args.part
    for b in range(args.batches):
        # noise keyed by (seed, GLOBAL sample index): rank r of N draws rows [b*bs*N + r*bs, +bs) of the job's noise, so
        # the noise of a sample does not depend on how many processes made the job (the reference's N hand-started
        # processes, SAMPLE:13-18, each draw from their own default generator: torch seeds it at random per process)
        # (a loader that ends on a short batch — dataset.ConditionLoader keeps it, like the reference's DataLoader — draws
        #  the first rows' ids: cfg.DeviceRng.ids_for)
        D.key_noise_by_sample(sampler, args.seed, args.bs * world, first_id=b * args.bs * world, device=device)
        ret = trainer.sample(args.i, device, step=len(train_list))
        train_list.append(ret)
        print(f'length of trainList {len(train_list)}')
        if trainer.score_photometric:
            print(f'rank {rank}: mean photometric error of batch {b}: {float(trainer.last_photometric_error.mean()):.6e}')
        if trainer.score_known:
            print(f'rank {rank}: mean known-pixel error of batch {b}: {float(trainer.last_known_error.mean()):.6e}')
        if len(train_list) % 2 == 0:
            np.save(f'{out_dir}idx_{args.i}_rank_{rank}_part_{part}_dm_cahomo_{len(train_list) * args.bs / 1000}k.npy',
                    np.array(train_list, dtype=object), allow_pickle=True)
            train_list.clear()
            part += 1
    # (captured denoise steps live in an LRU keyed by batch shape: a loader whose epochs end on a short batch captures twice per
    #  job, not twice per epoch)
    print(f'rank {rank}: graph captures {sampler.graph_captures}')


if __name__ == '__main__':
    main()
