"""-m gpu: the sample preview path — dmh_post_process against the reference's postProcess buffers (tests/golden/preview.npz,
made by tests/golden/make_golden_preview.py) and against the composition of the stand-alone kernels, dmh_preview_sheet against
a numpy restatement of make_grid + save_image's quantisation, dmh_homography_warp against a float64 numpy restatement of the
exact bilinear warp, and the Trainer wiring (train at a milestone, sample at every 100th step)."""
import os

import numpy as np
import pytest
import torch

from gpu_util import dev, report
from test_preview_host import decode_png, make_grid_np, quantise_np

pytestmark = pytest.mark.gpu

ULP1 = 1.2e-7          # one fp32 ulp of 1.0: values are in [0, 1] and the kernel's only fp32 rounding is the last one


@pytest.fixture(scope='module')
def gd(golden_dir):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, 'preview.npz')).items()}


def panels(buf):
    W = buf.shape[-1] // 4
    return [buf[..., i * W:(i + 1) * W] for i in range(4)]


def test_post_process_against_the_reference(gd):
    from dmhomo_amd import ops
    from dmhomo_amd.denoising_diffusion_models import denoising_diffusion_pytorch as ddp
    img, mask, flow = (gd[k].to(dev()) for k in ('img', 'mask', 'flow'))
    buf1, buf2 = ddp.postProcess(img, mask, flow)
    assert buf1.device == img.device and buf1.dtype == torch.float32
    assert buf1.shape == buf2.shape == gd['buf1'].shape == (5, 3, 16, 96)
    for name, got, want in (('buf1', buf1.cpu(), gd['buf1']), ('buf2', buf2.cpu(), gd['buf2'])):
        g, w = panels(got), panels(want)
        for i, panel in enumerate(('image', 'warp', 'mask')):
            assert torch.equal(g[i], w[i]), f'{name}: {panel} panel'
        err, _ = report(f'{name} flow panel', g[3], w[3])
        assert err <= 2e-5                                   # the gate of test_gpu_geometry.py on flow_to_image
    # the composition of the stand-alone kernels, bit for bit
    warp, vis, m3 = ops.flow_warp(img[:, 3:6].contiguous(), flow), ops.flow_to_image(flow, 256.), mask.repeat(1, 3, 1, 1)
    assert torch.equal(buf1, torch.cat([img[:, :3], img[:, :3], m3, vis], -1))
    assert torch.equal(buf2, torch.cat([img[:, 3:6], warp, m3, vis], -1))
    assert torch.equal(ddp.visulize_flow(flow), vis.cpu())
    # host inputs come back on the host
    h1, h2 = ddp.postProcess(gd['img'], gd['mask'], gd['flow'])
    assert not h1.is_cuda and torch.equal(h1, buf1.cpu()) and torch.equal(h2, buf2.cpu())


def sheet_np(buf, nrow, bgr, padding=2):
    a = buf.cpu().numpy()
    return quantise_np(make_grid_np(a[:, ::-1] if bgr else a, nrow, padding))


@pytest.mark.parametrize('bgr', [True, False])
@pytest.mark.parametrize('B,nrow', [(5, 1), (5, 2), (5, 5), (1, 2)])
def test_preview_sheet_against_make_grid_and_quantise(gd, B, nrow, bgr):
    from dmhomo_amd import ops
    img, mask, flow = (gd[k][:B].to(dev()).contiguous() for k in ('img', 'mask', 'flow'))
    buf1, buf2 = ops.post_process(img, mask, flow)
    s1, s2 = ops.preview_sheet(img, mask, flow, nrow=nrow, padding=2, bgr=bgr)
    assert s1.dtype == torch.uint8 and s1.shape == s2.shape
    for name, s, own, ref in (('source', s1, buf1, gd['buf1'][:B]), ('target', s2, buf2, gd['buf2'][:B])):
        got = s.cpu().numpy()
        want = sheet_np(own, nrow, bgr)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(got, want), f'{name}: {int((got != want).sum())} bytes differ from make_grid + quantise'
        # against the reference's buffers: everything but the flow panel bytewise, the flow panel within one level
        # (2e-5 * 255 cannot move a value by more than one)
        want_ref = sheet_np(ref, nrow, bgr)
        ind = np.zeros(tuple(ref.shape), dtype=np.float32)
        ind[..., 3 * (ref.shape[-1] // 4):] = 1.
        in_flow = make_grid_np(ind, nrow, 2).transpose(1, 2, 0) > 0
        assert np.array_equal(got[~in_flow], want_ref[~in_flow]), name
        d = np.abs(got[in_flow].astype(np.int32) - want_ref[in_flow].astype(np.int32))
        print(f'[parity] sheet {name} B={B} nrow={nrow} bgr={bgr}: flow panel max level difference {int(d.max())}, '
              f'{int((d > 0).sum())} of {d.size} bytes differ')
        assert d.max() <= 1


def test_preview_sheet_with_another_padding_and_save_preview_sheets(gd, tmp_path):
    """padding 0 and 3, and the file path: save_preview_sheets writes what postProcess -> [:, [2,1,0]] -> save_image writes"""
    from dmhomo_amd import ops, preview
    img, mask, flow = (gd[k].to(dev()) for k in ('img', 'mask', 'flow'))
    buf1, buf2 = ops.post_process(img, mask, flow)
    for padding in (0, 3):
        s1, s2 = ops.preview_sheet(img, mask, flow, nrow=3, padding=padding, bgr=True)
        assert np.array_equal(s1.cpu().numpy(), sheet_np(buf1, 3, True, padding))
        assert np.array_equal(s2.cpu().numpy(), sheet_np(buf2, 3, True, padding))
    src, tgt = str(tmp_path / 's.png'), str(tmp_path / 't.png')
    preview.save_preview_sheets(img, mask, flow, src, tgt, nrow=2)
    assert np.array_equal(decode_png(src), sheet_np(buf1, 2, True)) and np.array_equal(decode_png(tgt), sheet_np(buf2, 2, True))
    unfused = str(tmp_path / 'u.png')
    preview.save_image(buf2[:, [2, 1, 0]], unfused, nrow=2)
    assert np.array_equal(decode_png(unfused), decode_png(tgt))


def warp_np(src, M, Hd, Wd):
    """cv2.warpPerspective(src, M, (Wd, Hd)) without the inverse-map flag as EXACT bilinear interpolation in float64:
    dst(x, y) = src(M^-1 (x, y, 1)), constant border 0 per neighbour.  src (C, H, W) -> (C, Hd, Wd) float64."""
    C, H, W = src.shape
    Mi = np.linalg.inv(np.asarray(M, dtype=np.float64))
    ys, xs = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing='ij')
    qx = Mi[0, 0] * xs + Mi[0, 1] * ys + Mi[0, 2]
    qy = Mi[1, 0] * xs + Mi[1, 1] * ys + Mi[1, 2]
    qw = Mi[2, 0] * xs + Mi[2, 1] * ys + Mi[2, 2]
    sx, sy = qx / qw, qy / qw
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    s64 = src.astype(np.float64)

    def tap(yi, xi):
        ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
        v = s64[:, np.clip(yi, 0, H - 1).astype(np.int64), np.clip(xi, 0, W - 1).astype(np.int64)]
        return np.where(ok[None], v, 0.0)
    top = (1 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)
    bot = (1 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)
    return (1 - fy) * top + fy * bot


def test_homography_warp():
    from dmhomo_amd import ops, ddpm
    g = torch.Generator().manual_seed(1527)
    src = torch.rand(3, 3, 64, 64, generator=g)
    Hd, Wd = 72, 80
    # identity: the source inside the image, 0 on the rest of the larger canvas; an integer translation: the shifted image
    eye = torch.eye(3, dtype=torch.float64)
    shift = torch.tensor([[1., 0., 5.], [0., 1., -3.], [0., 0., 1.]], dtype=torch.float64)
    out = ops.homography_warp(src[:2].to(dev()).contiguous(), torch.stack([eye, shift]).to(dev()), (Wd, Hd)).cpu()
    assert out.shape == (2, 3, Hd, Wd) and out.dtype == torch.float32
    assert torch.equal(out[0, :, :64, :64], src[0]) and not out[0, :, 64:].any() and not out[0, :, :, 64:].any()
    want = torch.zeros(3, Hd, Wd)
    want[:, :61, 5:69] = src[1][:, 3:, :]                     # dst(x, y) = src(x - 5, y + 3)
    assert torch.equal(out[1], want)
    # homographies of SyntheticConditions strength
    cond = ddpm.SyntheticConditions(64, 1)
    Hs = np.stack([cond._homography(torch.Generator().manual_seed(2000 + i)) for i in range(3)])
    out = ops.homography_warp(src.to(dev()), torch.from_numpy(Hs).to(dev()), (Wd, Hd)).cpu().numpy()
    for i in range(3):
        want = warp_np(src[i].numpy(), Hs[i], Hd, Wd).astype(np.float32)
        err = float(np.abs(out[i].astype(np.float64) - want.astype(np.float64)).max())
        print(f'[parity] homography warp {i}: max |hip - f64 restatement| = {err:.3e}, mean value {want.mean():.3f}')
        assert want.mean() > 0.2                               # the warp lands on the canvas: the comparison sees the image
        assert err <= ULP1


def test_post_process_cv2_on_a_train_pair_record():
    from dmhomo_amd import ddpm
    from dmhomo_amd.denoising_diffusion_models import denoising_diffusion_pytorch as ddp
    S, B = 256, 2
    cond = ddpm.SyntheticConditions(S, B, seed=31)
    data, _ = next(cond)
    pair = torch.rand(B, 6, S, S, generator=torch.Generator().manual_seed(8)).to(dev())
    rec = ddpm.saveTrainPair(pair, data[:, 6:7], data[:, -2:].contiguous())
    assert rec['imgs'].shape == (B, 6, S, S) and rec['imgs'].dtype == np.uint8 and rec['homos'].shape == (B, 3, 3)
    buf1, buf2 = ddp.postProcess_cv2(rec['imgs'], rec['homos'], 0)
    assert buf1.shape == buf2.shape == (B, 3, S, 2 * S) and buf1.dtype == buf2.dtype == torch.float32 and buf1.is_cuda
    img1 = rec['imgs'][:, :3].astype(np.float32) / 255.
    img2 = rec['imgs'][:, 3:6].astype(np.float32) / 255.
    assert np.array_equal(buf2.cpu().numpy(), np.concatenate([img2, img2], -1))
    assert np.array_equal(buf1[..., :S].cpu().numpy(), img1)
    for i in range(B):
        want = warp_np(img1[i], rec['homos'][i], 256, 256).astype(np.float32)
        err = float(np.abs(buf1[i, :, :, S:].cpu().numpy().astype(np.float64) - want).max())
        print(f'[parity] postProcess_cv2 warp {i}: max |hip - f64 restatement| = {err:.3e}')
        assert err <= ULP1
    with pytest.raises(ValueError):
        ddp.postProcess_cv2(rec['imgs'][:, :, :32, :32], rec['homos'], 0)


def _tiny_trainer(tmp, preview, steps=2):
    from test_gpu_unet import make_cfg
    from dmhomo_amd import cfg, ddpm
    torch.manual_seed(1871)                                   # the training noise stream: the same for both runs
    m, _ = make_cfg(8)
    d = cfg.GaussianDiffusion(m, image_size=32, timesteps=1000, sampling_timesteps=2, objective='pred_x0').to(dev())
    tr = ddpm.Trainer(d, 'DGM_Conditions', train_batch_size=2, gradient_accumulate_every=2, train_lr=1e-3,
                      train_num_steps=steps, results_folder=str(tmp), save_and_sample_every=2, num_samples=4,
                      ema_update_every=1)
    tr.preview = preview
    return tr, m


def _same(a, b, path):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], f'{path}.{k}')
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f'{path}[{i}]')
    elif torch.is_tensor(a):
        assert torch.equal(a.cpu(), b.cpu()), path
    else:
        assert a == b, path


def _training_state(tr):
    """everything a checkpoint holds plus the generators the next training step draws from, copied to the host"""
    import copy

    def host(v):
        if torch.is_tensor(v):
            return v.detach().cpu().clone()
        if isinstance(v, dict):
            return {k: host(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [host(x) for x in v]
        return copy.deepcopy(v)
    return {'checkpoint': host({'step': tr.step, 'model': tr.model.state_dict(), 'opt': tr._ts.state_dict(),
                                'ema': tr.ema.state_dict(), 'scaler': None, 'version': None}),
            'cpu_rng': torch.get_rng_state().clone(), 'cuda_rng': torch.cuda.get_rng_state(dev()).clone()}


def test_trainer_train_writes_sample_sheets_and_leaves_training_alone(tmp_path, monkeypatch):
    """Trainer.train with preview (DDP:1871-1935) on the tiny model of test_trainer_train_loop_and_checkpoint: the sheets
    exist, have make_grid's size for 4 images of (32, 128) with nrow 2 and repeat the source image in the second panel; with
    preview off no PNG is written.

    Sampling must not disturb the training state.  Two training runs cannot be compared bit for bit for that: the
    batch-reduction kernels of the backward pass are not bitwise reproducible run to run (test_gpu_backward.py,
    test_train_step_follows_moved_parameter_storage) — measured here on the MI355X: two runs of this 2-step job, whose one
    preview comes AFTER the last optimiser step and so cannot reach the weights, already differ in the last bits of
    null_classes_emb, and three runs WITHOUT previews differ from each other in 198 and 205 of the 282 tensors.  The same property is therefore pinned inside ONE run, bit for bit: model, optimiser moments, EMA copy,
    step counter and both torch generators (the training noise stream) are captured right before the preview and must be
    identical right after it, and the checkpoint written after the preview must hold exactly the state captured before it —
    what the run without previews would have saved at that point."""
    monkeypatch.chdir(tmp_path)                               # make_gif writes sample_gif_results/ under the working directory
    on, off = tmp_path / 'on', tmp_path / 'off'
    tr_on, m_on = _tiny_trainer(on, True)
    seen = {}
    inner = tr_on._preview_milestone

    def watched(data, milestone, device):
        seen['before'] = _training_state(tr_on)
        inner(data, milestone, device)
        seen['after'] = _training_state(tr_on)
    tr_on._preview_milestone = watched
    tr_on.train()
    assert tr_on.step == 2 and set(seen) == {'before', 'after'}
    _same(seen['before'], seen['after'], 'state')
    ck = torch.load(str(on / 'model-1.pt'), map_location='cpu')
    assert set(ck) == {'step', 'model', 'opt', 'ema', 'scaler', 'version'}
    want = dict(seen['before']['checkpoint'], version=ck['version'])
    _same(ck, want, 'checkpoint')
    tr_off, m_off = _tiny_trainer(off, False)
    tr_off.train()
    assert not list(off.glob('*.png')) and (off / 'model-1.pt').exists() and not (tmp_path / 'generate_training_pairs').exists()
    src, tgt = decode_png(str(on / 'sample-1-source.png')), decode_png(str(on / 'sample-1-target.png'))
    assert src.shape == tgt.shape == (2 * (32 + 2) + 2, 2 * (128 + 2) + 2, 3)
    for k in range(4):
        y, x = (k // 2) * 34 + 2, (k % 2) * 130 + 2
        assert np.array_equal(src[y:y + 32, x:x + 32], src[y:y + 32, x + 32:x + 64])         # [img1 | img1 | ...]
        assert np.array_equal(src[y:y + 32, x + 64:x + 128], tgt[y:y + 32, x + 64:x + 128])   # mask and flow panels agree
    assert not src[:2].any() and not src[:, :2].any()          # padding
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert (tmp_path / 'sample_gif_results' / '1.gif').exists()


def test_preview_milestone_puts_the_generators_back(tmp_path, monkeypatch):
    """the sampler of a preview draws from torch's generators (or the sampler's keyed state): all of them are put back, so
    the training noise after a milestone does not depend on ``preview``"""
    monkeypatch.chdir(tmp_path)
    from dmhomo_amd import cfg
    tr, m = _tiny_trainer(tmp_path / 'r', True)
    data = next(tr.dl)
    for keyed in (False, True):
        rng = tr.ema.ema_model.rng
        if keyed:
            rng.key_by_sample(3, range(2), dev())
        torch.manual_seed(5)
        cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
        st0 = rng.state.clone() if keyed else None
        tr._preview_milestone(data, 7, dev())
        assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(dev()), dev0)
        assert not keyed or torch.equal(rng.state, st0)
        assert (tmp_path / 'r' / 'sample-7-source.png').exists()
    assert isinstance(tr.ema.ema_model.rng, cfg.DeviceRng)


def test_trainer_sample_writes_the_four_sheets_and_returns_the_same_record(tmp_path, monkeypatch):
    """Trainer.sample(0, 0, step=100) with preview (DDP:1972-2019): the flow-remap and homography-warp sheets under
    generate_training_pairs/, and the record of the same call with step=1"""
    monkeypatch.chdir(tmp_path)
    from test_gpu_unet import make_cfg
    from dmhomo_amd import cfg, ddpm

    def record(step, preview):
        m, _ = make_cfg(8)
        d = cfg.GaussianDiffusion(m, image_size=256, timesteps=1000, sampling_timesteps=2, objective='pred_x0').to(dev())
        tr = ddpm.Trainer(d, 'DGM_Conditions', train_batch_size=5, results_folder=str(tmp_path / 'results'))
        tr.preview = preview
        d.rng.key_by_sample(11, range(5), dev())               # the same noise for both calls
        return tr.sample(0, 0, step=step)
    r100 = record(100, True)
    names = [f'generate_training_pairs/idx_0_step_100_rank_0_sample-{k}_{kind}.png'
             for kind in ('flowRemap', 'homoWarp') for k in ('source', 'target')]
    for n in names:
        assert (tmp_path / n).exists(), n
    # 5 samples -> the largest square, 4, in 2 rows (DDP:1973-1975)
    assert decode_png(str(tmp_path / names[0])).shape == (2 * (256 + 2) + 2, 2 * (4 * 256 + 2) + 2, 3)
    assert decode_png(str(tmp_path / names[2])).shape == (2 * (256 + 2) + 2, 2 * (2 * 256 + 2) + 2, 3)
    # the homoWarp target sheet is [img2 | img2] of the record, BGR
    tgt = decode_png(str(tmp_path / names[3]))
    assert np.array_equal(tgt[2:258, 2:258], tgt[2:258, 258:514])
    assert np.array_equal(tgt[2:258, 2:258], r100['imgs'][0, 3:6][::-1].transpose(1, 2, 0))
    before = sorted(os.listdir(tmp_path / 'generate_training_pairs'))
    r1 = record(1, True)
    assert sorted(os.listdir(tmp_path / 'generate_training_pairs')) == before          # step 1: nothing written
    assert np.array_equal(r1['imgs'], r100['imgs']) and np.array_equal(r1['homos'], r100['homos'])
    r100_off = record(100, False)
    assert sorted(os.listdir(tmp_path / 'generate_training_pairs')) == before          # preview off: nothing written
    assert np.array_equal(r100_off['imgs'], r100['imgs'])
    tr_small = ddpm.Trainer(cfg.GaussianDiffusion(make_cfg(8)[0], image_size=32, timesteps=1000, sampling_timesteps=2,
                                                  objective='pred_x0').to(dev()), 'DGM_Conditions', train_batch_size=2)
    tr_small.preview = True
    with pytest.raises(ValueError):
        tr_small.sample(0, 0, step=100)
