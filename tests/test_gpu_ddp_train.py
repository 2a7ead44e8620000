"""-m gpu: training the unconditional class (ddpm.GaussianDiffusion / ddpm.Unet, DDP:315-820) on the HIP backward kernels.

1. the DDP Downsample's weight gradient (dmh_conv_unshuffle_wgrad) and data gradient against fp64 autograd;
2. the loss gradient (dmh_loss_backward_ddp) against autograd;
3. the whole ddpm.Unet backward against autograd through the oracle's functional forward;
4. DDPTrainStep against the reference's own loss.backward() / clip / Adam (tests/golden/make_golden_ddp_train.py);
5. the user's loop: loss = d(img); loss.backward(); clip_grad_norm_; torch.optim.Adam.step();
6. the optimiser state_dict round trip.
Gates are <= 10x the error measured on MI355X; the measured worst is printed."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from detweights import det_state_dict, shapes_of
from gpu_util import dev, nhwc, nchw, rand, ReplayDeviceRng

pytestmark = pytest.mark.gpu

CONFIGS = (('pred_noise', 'l1'), ('pred_v', 'l2'))
CASES = ('nosc', 'sc0', 'sc1')
LOOP_CASE = 'pred_noise.l1.sc1'           # the user-loop test's configuration


def g(x):
    return x.to(dev())


def _rel(got, ref):
    ref = ref.double().cpu()
    return ((got.double().cpu().reshape(ref.shape) - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def make_ddp(dim, sc, channels=3, seed=1):
    from dmhomo_amd import ddpm
    m = ddpm.Unet(dim=dim, dim_mults=(1, 2, 4, 8), channels=channels, self_condition=sc)
    sd = det_state_dict(shapes_of(m), seed)
    m.load_state_dict(sd)
    return m.to(dev()), sd


def load(golden_dir):
    return {k: v for k, v in np.load(os.path.join(golden_dir, 'ddp_train_step.npz')).items()}


# ----------------------------------------------------------------------------------- 1. Downsample backward
# (C, Cout, H): the three Downsamples of the dim-64 model at 128x128, and C values off the MFMA tile (the dim-8 model)
UNSHUFFLE = [(64, 64, 128), (64, 128, 64), (128, 256, 32), (8, 8, 16), (16, 16, 8), (24, 32, 8)]


@pytest.mark.parametrize('B', [1, 3, 16])
@pytest.mark.parametrize('C,Cout,H', UNSHUFFLE, ids=[f'{c}to{o}@{h}' for c, o, h in UNSHUFFLE])
def test_unshuffle_backward_vs_fp64(C, Cout, H, B):
    """pixel-unshuffle + 1x1 (DDP:110-113): dW, db from the in-place kernel and dx through the permuted 1x1 + dmh_d2s,
    against fp64 autograd of F.conv2d over the unshuffled view (oracle.unet._downsample); two runs bitwise equal"""
    from dmhomo_amd import ops
    from oracle import unet as OU
    x = rand((B, C, H, H), 900 + C)
    w = rand((Cout, 4 * C, 1, 1), 901, (4 * C) ** -0.5)
    b = rand((Cout,), 902)
    dy = rand((B, Cout, H // 2, H // 2), 903)
    xd, wd, bd = (v.double().requires_grad_(True) for v in (x, w, b))
    out = OU._downsample({'1.weight': wd, '1.bias': bd}, xd)
    rdx, rdw, rdb = torch.autograd.grad(out, [xd, wd, bd], dy.double())
    dx, dw, db = ops.conv_unshuffle_backward(nhwc(dy), nhwc(x), g(w))
    assert dw.shape == w.shape and db.shape == b.shape
    ew, eb, ex = _rel(dw, rdw), _rel(db, rdb), _rel(nchw(dx), rdx)
    print(f'[parity] unshuffle bwd {C}->{Cout} @{H} B={B}: dW {ew:.2e} db {eb:.2e} dx {ex:.2e} (rel_to_max)')
    assert ew < 2e-6 and eb < 2e-6, (ew, eb)        # exact fp32 MFMA, fp32 accumulation
    assert ex < 4e-6, ex                            # the 1x1 conv kernel's operand split
    dw2, db2 = ops.conv_unshuffle_wgrad(nhwc(dy), nhwc(x))
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


# ----------------------------------------------------------------------------------- 2. loss gradient
@pytest.mark.parametrize('squared', [False, True], ids=['l1', 'l2'])
def test_loss_backward_ddp_vs_autograd(squared):
    """DDP:804-811: mean_b(p2_weight[t_b] * mean_chw l(out - target)), scaled by 1/accum; exact zeros of out - target
    get a zero L1 gradient, as torch's sign does"""
    from dmhomo_amd import ops
    B, C, H, W = 3, 3, 24, 40
    out, target = rand((B, C, H, W), 910), rand((B, C, H, W), 911)
    target.view(-1)[::7] = out.view(-1)[::7]
    w = torch.tensor([0.5, 1.7, 0.03])
    o = out.double().requires_grad_(True)
    lf = F.mse_loss if squared else F.l1_loss
    loss = (lf(o, target.double(), reduction='none').reshape(B, -1).mean(1) * w.double()).mean() * 0.5
    ref, = torch.autograd.grad(loss, [o])
    got = ops.loss_backward_ddp(g(out), g(target), g(w), squared, 0.5).cpu()
    r = _rel(got, ref)
    print(f'[parity] ddp loss bwd {"l2" if squared else "l1"}: rel_to_max={r:.2e}')
    assert r < 1e-6, r
    if not squared:
        assert (got.view(-1)[::7] == 0).all()


# ----------------------------------------------------------------------------------- 3. whole UNet backward
def _unet_backward(dim, sc, channels, B, S, gate, seed, dscale):
    from dmhomo_amd import train
    from oracle import unet as OU
    m, sd = make_ddp(dim, sc, channels)
    x = rand((B, channels, S, S), seed)
    xs = rand((B, channels, S, S), seed + 1) if sc else None
    t = torch.tensor([17, 803, 440, 999][:B])
    dout = rand((B, channels, S, S), seed + 2) * dscale
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    # (fp32 on purpose: the reference's weight standardisation switches to eps = 1e-3 for any other dtype, DDP:125)
    sdd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    out_ref = OU.ddp_unet_forward(sdd, x, t, xs, sc)
    pnames = [k for k, _ in m.named_parameters()]
    ref = dict(zip(pnames, torch.autograd.grad(out_ref, [sdd[k] for k in pnames], dout, allow_unused=True)))
    ut = train.UnetTrain(m)
    assert ut.uncond
    out, saved = ut.forward_uncond(g(x), g(t), None if xs is None else g(xs))
    assert _rel(out, out_ref.detach()) < 2e-4
    got = ut.backward(saved, g(dout))
    missing = [k for k in pnames if k not in got]
    assert not missing, missing
    worst, wk = 0.0, None
    for k in pnames:
        if ref[k] is None:
            continue
        if ref[k].abs().max() < 1e-4 * dscale:   # a conv bias in front of a GroupNorm: its true gradient is 0
            assert got[k].abs().max().item() < 1e-3 * dscale, k
            continue
        r = _rel(got[k], ref[k])
        if r > worst:
            worst, wk = r, k
    print(f'[parity] ddp unet dim={dim} @{S} sc={sc} channels={channels} (input pad {ut.cin_pad}) bwd: '
          f'{len(pnames)} parameter gradients, worst rel_to_max={worst:.3e} ({wk})')
    assert worst < gate, (worst, wk)


@pytest.mark.parametrize('sc,channels', [(False, 3), (True, 3), (True, 6)], ids=['pad4', 'pad8', 'pad12'])
def test_ddp_unet_backward_vs_autograd(sc, channels):
    """ddpm.Unet (DDP:315-447) at dim 8, 16x16: every parameter's gradient; input paddings 4, 8, 12"""
    _unet_backward(8, sc, channels, 3, 16, 3e-5, 920, 1.0)            # measured 3.2e-6 .. 5.2e-6


def test_ddp_unet_backward_dim64_vs_autograd():
    """the configuration the unconditional sampler is benched at: dim 64, 128x128 (B = 2), self-conditioning"""
    _unet_backward(64, True, 3, 2, 128, 1e-4, 930, 1.0 / (3 * 128 * 128))   # d(mean loss)/d(out) scale; measured 1.2e-5


# ----------------------------------------------------------------------------------- 4. against the reference
def _setup(gd, obj, lt, case, lr=1e-3, accum=1):
    from dmhomo_amd import ddpm, train
    m, _ = make_ddp(8, case != 'nosc')
    d = ddpm.GaussianDiffusion(m, image_size=16, timesteps=1000, sampling_timesteps=4, objective=obj, loss_type=lt,
                               p2_loss_weight_gamma=0.5).to(dev())
    ts = train.DDPTrainStep(d, lr=lr, betas=(0.9, 0.99), accum=accum)
    draws = dict(t=g(torch.from_numpy(gd['t'])), noise=g(torch.from_numpy(gd['noise'])), use_self_cond=case == 'sc1')
    return m, d, ts, g(torch.from_numpy(gd['img'])), draws


def _grad_errors(gd, key, m, grads):
    """-> (worst error of the recorded elements relative to the largest of them, worst relative error of a whole
    tensor's L2 norm), each with the parameter it was found at"""
    tag = 'nosc' if key.endswith('nosc') else 'sc'
    idx, off = torch.from_numpy(gd['gidx.' + tag]).long(), gd['goff.' + tag]
    refs, norms = torch.from_numpy(gd[key + '.grad']).double(), gd[key + '.gnorm']
    names = [k for k, _ in m.named_parameters()]
    assert len(names) + 1 == len(off) == len(norms) + 1
    worst, wk, nworst, nk = 0.0, None, 0.0, None
    for i, k in enumerate(names):
        full = grads[k].detach().double().cpu().reshape(-1)
        ref, got = refs[off[i]:off[i + 1]], full[idx[off[i]:off[i + 1]]]
        if norms[i] < 1e-5:                       # conv biases in front of a GroupNorm: true gradient 0
            assert full.abs().max().item() < 1e-4, k
            continue
        r = ((got - ref).abs().max() / ref.abs().max()).item()
        n = abs(full.norm().item() - float(norms[i])) / float(norms[i])
        if r > worst:
            worst, wk = r, k
        if n > nworst:
            nworst, nk = n, k
    return (worst, wk), (nworst, nk)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('obj,lt', CONFIGS, ids=['pred_noise-l1', 'pred_v-l2'])
def test_ddp_train_step_vs_reference(golden_dir, obj, lt, case):
    """loss_and_grads against the reference's p_losses + loss.backward() + clip_grad_norm_; then 4 optimiser steps
    (accumulate 2, Adam lr 1e-3) against the reference's own loop: loss and || params ||"""
    gd = load(golden_dir)
    key = f'{obj}.{lt}.{case}'
    m, d, ts, img, draws = _setup(gd, obj, lt, case)
    loss, grads = ts.loss_and_grads(img, **draws)
    want = float(gd[key + '.loss'])
    (worst, wk), (nworst, nk) = _grad_errors(gd, key, m, grads)
    clip = ts.apply(grads)
    print(f'[parity] ddp train {key}: loss {float(loss):.7f} want {want:.7f}; worst gradient rel_to_max={worst:.3e} ({wk}); '
          f'worst tensor-norm error {nworst:.3e} ({nk}); grad norm {clip[0].item():.6f} want {float(gd[key + ".grad_norm"]):.6f}')
    assert abs(float(loss) - want) <= 2e-5 * abs(want)
    assert worst < 6e-5, (worst, wk)
    assert nworst < 3e-5, (nworst, nk)           # measured <= 3.0e-6
    assert abs(clip[0].item() - float(gd[key + '.grad_norm'])) <= 1e-4 * float(gd[key + '.grad_norm'])
    m, d, ts, img, draws = _setup(gd, obj, lt, case, accum=2)
    for i in range(4):
        total = ts.step([img, img], draws=[draws, draws])
        pl2 = float(torch.sqrt(sum((p.detach().double() ** 2).sum() for p in m.parameters())))
        want, wl2 = float(gd[key + '.traj.loss'][i]), float(gd[key + '.traj.param_l2'][i])
        print(f'[parity] ddp train {key} step {i}: loss {float(total):.6f} want {want:.6f}   |params| {pl2:.6f} want {wl2:.6f}')
        assert abs(float(total) - want) <= (2e-5 if i == 0 else 1e-4) * want
        assert abs(pl2 - wl2) <= 1e-4 * wl2


# ----------------------------------------------------------------------------------- 5. the user's loop
def test_ddp_loss_backward_adam_user_loop(golden_dir, monkeypatch):
    """the reference's idiom for this class: loss = diffusion(img); loss.backward(); clip_grad_norm_; Adam.step() — with
    t, noise and the self-conditioning draw replayed.  Fails without the feature (the loss has no grad_fn)."""
    from dmhomo_amd import ddpm
    gd = load(golden_dir)
    m, d, _, img, draws = _setup(gd, 'pred_noise', 'l1', 'sc1')
    monkeypatch.setattr(torch, 'randint', lambda *a, **k: draws['t'].clone())      # DDP:817
    d._random = lambda: 0.1                                                        # DDP:785: fires
    noise = draws['noise']

    def sample(diff):
        diff.rng = ReplayDeviceRng([rand((2, 3, 16, 16), 940 + i) for i in range(8)])
        return diff.ddim_sample((2, 3, 16, 16))
    before = sample(d)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.99))
    losses = []
    for i in range(3):
        d.rng = ReplayDeviceRng([noise.cpu()])
        loss = d(img)
        assert loss.grad_fn is not None and loss.ndim == 0
        loss.backward()
        if i == 0:
            missing = [k for k, p in m.named_parameters() if p.grad is None]
            assert not missing, missing
            (worst, wk), (nworst, nk) = _grad_errors(gd, LOOP_CASE, m, {k: p.grad for k, p in m.named_parameters()})
            print(f'[parity] ddp user loop: first-step gradients vs the reference, worst rel_to_max={worst:.3e} ({wk}), '
                  f'worst tensor-norm error {nworst:.3e} ({nk})')
            assert worst < 6e-5 and nworst < 3e-5, (worst, wk, nworst, nk)
            assert abs(float(loss) - float(gd[LOOP_CASE + '.loss'])) <= 2e-5 * float(gd[LOOP_CASE + '.loss'])
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        opt.zero_grad()
        losses.append(float(loss))
    print(f'[parity] ddp user loop losses: {losses}')
    assert losses[0] > losses[1] > losses[2], losses
    d.rng = ReplayDeviceRng([noise.cpu()])
    with torch.no_grad():
        val = d(img)
    assert val.grad_fn is None and not val.requires_grad and bool(torch.isfinite(val))
    after = sample(d)
    assert not torch.equal(before, after)
    m2, _ = make_ddp(8, True)
    m2.load_state_dict(m.state_dict())
    d2 = ddpm.GaussianDiffusion(m2, image_size=16, timesteps=1000, sampling_timesteps=4, objective='pred_noise',
                                loss_type='l1', p2_loss_weight_gamma=0.5).to(dev())
    assert torch.equal(after, sample(d2))


# ----------------------------------------------------------------------------------- 6. checkpoint round trip
def test_ddp_optimizer_state_dict_round_trip(golden_dir):
    """two steps, the Adam state_dict (torch.optim.Adam's layout) and the weights into a fresh DDPTrainStep, two more
    steps: the same trajectory as the uninterrupted run and the reference's"""
    gd = load(golden_dir)
    key = 'pred_v.l2.sc1'
    m, d, ts, img, draws = _setup(gd, 'pred_v', 'l2', 'sc1', accum=2)
    for _ in range(2):
        ts.step([img, img], draws=[draws, draws])
    osd = ts.state_dict()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.99))
    opt.load_state_dict(osd)                                        # the layout torch.optim.Adam reads
    assert len(opt.state) == len(list(m.parameters()))
    m2, d2, ts2, _, _ = _setup(gd, 'pred_v', 'l2', 'sc1', accum=2)
    m2.load_state_dict(m.state_dict())
    ts2.load_state_dict(osd)
    assert ts2.opt_step == 2
    for i in (2, 3):
        a = ts.step([img, img], draws=[draws, draws])
        b = ts2.step([img, img], draws=[draws, draws])
        want = float(gd[key + '.traj.loss'][i])
        print(f'[parity] ddp resume step {i}: {float(a):.6f} / resumed {float(b):.6f} want {want:.6f}')
        assert abs(float(a) - float(b)) <= 1e-5 * abs(float(a))
        assert abs(float(b) - want) <= 1e-4 * want
    for (k, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert (p - q).abs().max().item() <= 1e-5 * max(p.abs().max().item(), 1e-3), k
