"""-m gpu: the weight-gradient kernels (dmh_conv_wgrad) the way training runs them — a workgroup walking SEVERAL pixel
tiles ("items") — against an fp64 reference, plus the small training kernels at their production sizes.

dmh_conv_wgrad splits the B * ceil(H/4) * ceil(W/16) items (item = (b * tilesY + ty) * tilesX + tx) into ``nsplit``
contiguous ranges of ``per`` items, one range per workgroup.  Only a second item reaches the running-maximum rescale of
the fp16-piece kernel's accumulators, its parity slots, the prefetch of the next item and the exact-fp32 kernel's item
loop; ragged last splits and splits without any item are further edges.  ``split_plan`` restates the host's split rule
(wgrad_splits / wgrad_splits_f16, csrc/conv_backward.hip) so that every case below says what it covers;
tests/test_wgrad_splits_host.py checks the restatement against the library and the coverage of the cases on the CPU.

Reference: dW[o, c, ky, kx] = sum over pixels of dy * (shifted input), one fp64 GEMM per tap over the zero-padded (or
nearest-x2-upsampled, or stride-2) input, in torch on the GPU; ``test_reference_matches_autograd`` checks it once
against CPU F.conv2d autograd.  Gates: rel-to-max per tensor, per (tap, 64x64 (o, c) block) against the block's own
maximum, db against the fp64 sum, and two calls bitwise equal (the reduction order is fixed by design)."""
import os

import pytest
import torch
import torch.nn.functional as F

from aux_cases import adam_step64, ulp32_spacing as _ulp32     # shared with the single-tensor entries (tests/test_gpu_aux.py)

pytestmark = pytest.mark.gpu

TH, TW = 4, 16                  # pixels of an item (a 4 x 16 tile of dy)


def cdiv(a, b):
    return -(-a // b)


def wgrad_family(k):
    """'f16': the fp16-piece kernel (k = 2, 3); 'fp32': the exact-fp32 kernel (k = 1, 7)"""
    return 'f16' if k in (2, 3) else 'fp32'


def wgrad_npairs(cin, cout, k):
    return cdiv(cout, 64) * cdiv(cin, 16 if k == 7 else 64)


def wgrad_splits(nitems, npairs):
    return min(max(512 // max(npairs, 1), 1), nitems)


def wgrad_splits_f16(nitems, npairs):
    s = 512 // (2 * max(npairs, 1))
    if s >= 8:
        s = s // 8 * 8
    return min(max(s, 1), nitems)


def split_plan(B, H, W, cin, cout, k):
    """B, H, W: the size of dy (the conv's output); cin: the input channels the kernel sees"""
    nitems = B * cdiv(H, TH) * cdiv(W, TW)
    npairs = wgrad_npairs(cin, cout, k)
    ns = (wgrad_splits_f16 if wgrad_family(k) == 'f16' else wgrad_splits)(nitems, npairs)
    per = cdiv(nitems, ns)
    used = cdiv(nitems, per)
    return dict(family=wgrad_family(k), nitems=nitems, npairs=npairs, nsplit=ns, per=per, used=used,
                empty=ns - used, ragged=nitems % per != 0)


# (name, B, H, W, C0, C1, Cout, k, mode): H, W the size of dy; C0 the first source's channels as the kernel sees them
# (mode 'down': 4C of the space-to-depth view of x (B, 2H, 2W, C)); mode: plain | concat | coef (GroupNorm+SiLU
# prologue) | ups (nearest x2 of a stored H/2 x W/2 input) | down (4x4 / stride 2 through ops.conv_down_backward)
CASES = [
    ('f16 3x3 2/wg 112 empty', 3, 64, 96, 64, 0, 64, 3, 'plain'),
    ('f16 3x3 40->72 3/wg ragged', 2, 133, 49, 40, 0, 72, 3, 'plain'),
    ('f16 3x3 concat 64+32->96 2/wg ragged', 1, 89, 33, 64, 32, 96, 3, 'concat'),
    ('f16 3x3 prologue 48->80 3/wg ragged', 2, 133, 49, 48, 0, 80, 3, 'coef'),
    ('f16 3x3 ups 64->48 2/wg ragged', 3, 114, 34, 64, 0, 48, 3, 'ups'),
    ('f16 down 4*32->48 2/wg ragged', 3, 57, 33, 128, 0, 48, 2, 'down'),
    ('fp32 1x1 concat 40+24->200 3/wg ragged', 2, 133, 49, 40, 24, 200, 1, 'concat'),
    ('fp32 7x7 12->64 2/wg ragged', 3, 137, 65, 12, 0, 64, 7, 'plain'),
]

# every distinct weight-gradient call of one dim-64 training step at 128x128 (CFG UNet, DDP UNet with and without
# self-conditioning): (k, ups, C0, C1, Cout, H, W, prologue), H, W the size of dy.  Recorded by
# test_training_wgrad_shapes_are_listed, which fails when the model starts passing a shape this list lacks.
TRAIN_SHAPES = [
    (1, 0, 64, 0, 384, 64, 64, 0), (1, 0, 64, 0, 384, 128, 128, 0), (1, 0, 64, 64, 64, 128, 128, 0), (1, 0, 128, 0, 64, 64, 64, 0),
    (1, 0, 128, 0, 64, 128, 128, 0), (1, 0, 128, 0, 128, 32, 32, 0), (1, 0, 128, 0, 128, 64, 64, 0), (1, 0, 128, 0, 256, 16, 16, 0),
    (1, 0, 128, 0, 256, 32, 32, 0), (1, 0, 128, 0, 384, 32, 32, 0), (1, 0, 128, 0, 384, 64, 64, 0), (1, 0, 128, 0, 512, 16, 16, 0),
    (1, 0, 128, 64, 128, 64, 64, 0), (1, 0, 256, 0, 384, 16, 16, 0), (1, 0, 256, 0, 384, 32, 32, 0), (1, 0, 256, 128, 256, 32, 32, 0),
    (1, 0, 512, 0, 384, 16, 16, 0), (1, 0, 512, 256, 512, 16, 16, 0), (2, 0, 256, 0, 64, 64, 64, 0), (2, 0, 256, 0, 128, 32, 32, 0),
    (2, 0, 512, 0, 256, 16, 16, 0), (3, 0, 64, 0, 64, 64, 64, 0), (3, 0, 64, 0, 64, 64, 64, 1), (3, 0, 64, 0, 64, 128, 128, 0),
    (3, 0, 64, 0, 64, 128, 128, 1), (3, 0, 64, 64, 64, 128, 128, 0), (3, 0, 128, 0, 128, 32, 32, 0), (3, 0, 128, 0, 128, 32, 32, 1),
    (3, 0, 128, 0, 128, 64, 64, 1), (3, 0, 128, 64, 128, 64, 64, 0), (3, 0, 256, 0, 256, 16, 16, 0), (3, 0, 256, 0, 256, 16, 16, 1),
    (3, 0, 256, 0, 256, 32, 32, 1), (3, 0, 256, 0, 512, 16, 16, 0), (3, 0, 256, 128, 256, 32, 32, 0), (3, 0, 512, 0, 512, 16, 16, 0),
    (3, 0, 512, 0, 512, 16, 16, 1), (3, 0, 512, 256, 512, 16, 16, 0), (3, 1, 128, 0, 64, 128, 128, 0), (3, 1, 256, 0, 128, 64, 64, 0),
    (3, 1, 512, 0, 256, 32, 32, 0), (7, 0, 4, 0, 64, 128, 128, 0), (7, 0, 8, 0, 64, 128, 128, 0), (7, 0, 12, 0, 64, 128, 128, 0),
]
TRAIN_B = 16


def train_case(s):
    k, ups, c0, c1, cout, H, W, pro = s
    mode = 'down' if k == 2 else 'ups' if ups else 'coef' if pro else 'concat' if c1 else 'plain'
    return (f'{k}x{k} {mode} {c0}+{c1}->{cout} @{H}x{W}', TRAIN_B, H, W, c0, c1, cout, k, mode)


def case_plan(case):
    _, B, H, W, c0, c1, cout, k, _ = case
    return split_plan(B, H, W, c0 + c1, cout, k)


# ------------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope='module')
def ops():
    from dmhomo_amd import ops as _ops
    _ops.lib()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return _ops


def _dev():
    return torch.device('cuda', 0)


def ref_wgrad(dy, src0, src1=None, k=3, coef=None, ups=0, down=False):
    """fp64 (dW OIHW, db) of the conv whose output gradient is dy (B, H, W, Cout) NHWC and whose input is cat(src0,
    src1) (after SiLU(a * src0 + b) with coef (B, 2, C0); after a nearest x2 upsampling with ups): one GEMM per tap.
    down: the 4x4 / stride 2 / pad 1 conv of src0 (B, 2H, 2W, C)."""
    x = src0.double()
    if coef is not None:
        x = F.silu(coef[:, 0].double()[:, None, None, :] * x + coef[:, 1].double()[:, None, None, :])
    if src1 is not None:
        x = torch.cat([x, src1.double()], 3)
    if ups:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    d = dy.double()
    B, H, W, cout = d.shape
    cin = x.shape[3]
    d2 = d.reshape(-1, cout).t()
    kk, st, p = (4, 2, 1) if down else (k, 1, k // 2)
    xp = F.pad(x, (0, 0, p, p, p, p))
    dw = torch.empty((cout, cin, kk, kk), dtype=torch.float64, device=d.device)
    for ky in range(kk):
        for kx in range(kk):
            tap = xp[:, ky:ky + st * (H - 1) + 1:st, kx:kx + st * (W - 1) + 1:st, :]
            dw[:, :, ky, kx] = d2 @ tap.reshape(-1, cin)
    return dw, d.reshape(-1, cout).sum(0)


def block_rel(got, ref):
    """worst over (64-block of o, 64-block of c, tap) of max|err| / max|ref| of that block"""
    o, c = ref.shape[:2]
    t = ref[0, 0].numel()
    err = (got.double() - ref).abs().reshape(o, c, t)
    ref = ref.abs().reshape(o, c, t)
    po, pc = cdiv(o, 64) * 64 - o, cdiv(c, 64) * 64 - c
    err, ref = (F.pad(v, (0, 0, 0, pc, 0, po)).reshape(cdiv(o, 64), 64, cdiv(c, 64), 64, t).amax((1, 3))
                for v in (err, ref))
    r = torch.where(ref > 0, err / ref.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))
    return r.max().item()


def rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def make_inputs(case, seed):
    _, B, H, W, c0, c1, cout, k, mode = case
    g = torch.Generator(device=_dev()).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device=_dev())
    dy = rn(B, H, W, cout)
    if mode == 'down':
        return dict(dy=dy, x=rn(B, 2 * H, 2 * W, c0 // 4), w=rn(cout, c0 // 4, 4, 4) * 0.05)
    hin, win = (H // 2, W // 2) if mode == 'ups' else (H, W)
    a = dict(dy=dy, src0=rn(B, hin, win, c0), src1=rn(B, hin, win, c1) if c1 else None, coef=None)
    if mode == 'coef':
        a['coef'] = torch.stack([1 + 0.3 * rn(B, c0), 0.5 * rn(B, c0)], 1).contiguous()
    return a


def run_wgrad(ops, case, a):
    k, mode = case[7], case[8]
    if mode == 'down':
        _, dw, db = ops.conv_down_backward(a['dy'], a['x'], a['w'])
        return dw, db
    return ops.conv_wgrad(a['dy'], a['src0'], a['src1'], k=k, in_coef=a['coef'], ups=int(mode == 'ups'))


def reference(case, a):
    k, mode = case[7], case[8]
    if mode == 'down':
        return ref_wgrad(a['dy'], a['x'], down=True)
    return ref_wgrad(a['dy'], a['src0'], a['src1'], k=k, coef=a['coef'], ups=int(mode == 'ups'))


# gates (<= 10x the error measured on MI355X): rel-to-max of the tensor, worst (tap, 64x64 block), db
# (measured: CASES f16 1.5-1.8e-7 / 2.1-2.6e-7 / 0.9-1.6e-7, fp32 2.4-3.1e-7 / 2.4-4.0e-7 / 1.2-2.2e-7; training shapes
#  f16 1.9e-7-1.1e-6 / 2.7e-7-1.4e-6 / 1.0-2.6e-7, fp32 1.9-9.8e-7 / 2.7e-7-1.2e-6 / 1.2-5.5e-7)
GATES = {'f16': (1.5e-6, 2e-6, 8e-7), 'fp32': (2.4e-6, 2.4e-6, 1.2e-6)}
TRAIN_GATES = {'f16': (1.8e-6, 2.6e-6, 9e-7), 'fp32': (1.9e-6, 2.7e-6, 1.2e-6)}


def check_case(ops, case, a, gates):
    name = case[0]
    p = case_plan(case)
    dw, db = run_wgrad(ops, case, a)
    dw2, db2 = run_wgrad(ops, case, a)
    torch.cuda.synchronize()
    rw, rb = reference(case, a)
    e_w, e_blk, e_b = rel(dw, rw), block_rel(dw, rw), rel(db, rb)
    print(f'[parity] wgrad {name} ({p["family"]}, {p["nitems"]} items / {p["nsplit"]} splits: {p["per"]} per workgroup, '
          f'{p["empty"]} empty, ragged={p["ragged"]}): dW rel_to_max={e_w:.3e} worst block={e_blk:.3e} db={e_b:.3e}')
    gw, gblk, gb = gates
    assert e_w <= gw and e_blk <= gblk and e_b <= gb, (name, e_w, e_blk, e_b)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), f'{name}: two calls differ'


# ------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_wgrad_multi_item_splits(ops, case):
    check_case(ops, case, make_inputs(case, 1000 + CASES.index(case)), GATES[case_plan(case)['family']])


@pytest.mark.parametrize('shape', TRAIN_SHAPES, ids=[train_case(s)[0] for s in TRAIN_SHAPES])
def test_wgrad_training_shapes_b16(ops, shape):
    """every weight-gradient shape of the dim-64 training steps, at the batch a GPU trains (16 images of 128x128)"""
    case = train_case(shape)
    check_case(ops, case, make_inputs(case, 2000 + TRAIN_SHAPES.index(shape)), TRAIN_GATES[case_plan(case)['family']])


def _item_positions(case):
    """(B, H, W) tensors on the device: each pixel's item's position inside its split, and whether it is the split's
    last item"""
    _, B, H, W, c0, c1, cout, k, _ = case
    p = case_plan(case)
    ty, tx = cdiv(H, TH), cdiv(W, TW)
    item = torch.arange(B * ty * tx, device=_dev()).reshape(B, ty, tx)
    item = item.repeat_interleave(TH, 1).repeat_interleave(TW, 2)[:, :H, :W]
    pos = item % p['per']
    last = (pos == p['per'] - 1) | (item == p['nitems'] - 1)
    return pos, last


DYN_CASE = ('f16 3x3 128->128 3/wg', 2, 48, 96, 128, 0, 128, 3, 'plain')
DYN_GATES = {'rising': (1.3e-6, 1.7e-6, 1.3e-6), 'falling': (2e-6, 2.5e-6, 2e-6),      # measured 1.3 / 1.7 / 1.4e-7,
             'zero_first': (1.8e-6, 2.2e-6, 1e-6), 'outlier_last': (1.7e-6, 2.5e-6, 1.1e-6)}  # 2.2 / 2.7 / 2.5e-7, ...


@pytest.mark.parametrize('pattern', list(DYN_GATES))
def test_wgrad_dynamic_range_along_a_split(ops, pattern):
    """magnitudes placed by an item's position inside its split (3 items per workgroup): rising by 2^6 per item (the
    running maxima rise at every item, so the accumulators are rescaled at every item and both parity slots are
    reused), falling by 2^-6 per item, a first item of exact zeros (dy and x) before non-zero items, and one isolated
    outlier in each split's last item"""
    case = DYN_CASE
    p = case_plan(case)
    assert p['per'] >= 3
    pos, last = _item_positions(case)
    a = make_inputs(case, 3000)
    dy, x = a['dy'], a['src0']
    if pattern == 'rising':
        dy *= torch.exp2(6.0 * pos)[..., None]
    elif pattern == 'falling':
        dy *= torch.exp2(-6.0 * pos)[..., None]
    elif pattern == 'zero_first':
        dy *= (pos > 0)[..., None]
        x *= (pos > 0)[..., None]
    else:
        g = torch.Generator().manual_seed(3001)
        sel = torch.nonzero(last.flatten()).flatten()
        pick = sel[torch.randperm(sel.numel(), generator=g)[:16].to(sel.device)]
        o = torch.randint(0, dy.shape[3], (pick.numel(),), generator=g).to(_dev())
        dy.view(-1, dy.shape[3])[pick, o] = 3.0e4
    check_case(ops, (f'dynamic range {pattern}',) + case[1:], a, DYN_GATES[pattern])


def test_reference_matches_autograd():
    """ref_wgrad (on the CPU here) against F.conv2d autograd in fp64 at a small shape, every mode"""
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    B, H, W = 2, 6, 10
    for k, mode in ((3, 'plain'), (3, 'concat'), (3, 'coef'), (3, 'ups'), (1, 'concat'), (7, 'plain'), (4, 'down')):
        c0, c1, cout = 5, (3 if mode == 'concat' else 0), 4
        h, w_ = (H // 2, W // 2) if mode == 'ups' else (2 * H, 2 * W) if mode == 'down' else (H, W)
        s0, s1 = rn(B, h, w_, c0), rn(B, h, w_, c1) if c1 else None
        coef = torch.stack([1 + 0.3 * rn(B, c0), 0.5 * rn(B, c0)], 1) if mode == 'coef' else None
        dy = rn(B, H, W, cout)
        x = s0
        if coef is not None:
            x = F.silu(coef[:, 0, None, None, :] * x + coef[:, 1, None, None, :])
        if s1 is not None:
            x = torch.cat([x, s1], 3)
        x = nchw(x)
        if mode == 'ups':
            x = F.interpolate(x, scale_factor=2, mode='nearest')
        wt = torch.zeros((cout, c0 + c1, k, k), dtype=torch.float64, requires_grad=True)
        bt = torch.zeros((cout,), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, wt, bt, 2, 1) if mode == 'down' else F.conv2d(x, wt, bt, 1, k // 2)
        gw, gb = torch.autograd.grad(y, (wt, bt), nchw(dy))
        rw, rb = ref_wgrad(dy, s0, s1, k=k, coef=coef, ups=int(mode == 'ups'), down=mode == 'down')
        assert torch.allclose(rw, gw, rtol=1e-12, atol=1e-12) and torch.allclose(rb, gb, rtol=1e-12, atol=1e-12), (k, mode)


def test_training_wgrad_shapes_are_listed(ops, monkeypatch):
    """wrap ops.conv_wgrad while one dim-64 UnetTrain forward + backward runs at 128x128 (CFG, DDP with and without
    self-conditioning): every shape it passes must be in TRAIN_SHAPES (and every listed shape must still occur)"""
    from test_gpu_unet import make_cfg, make_ddp, _cond_inputs
    from dmhomo_amd import train
    from gpu_util import rand
    seen = set()
    orig = ops.conv_wgrad

    def rec(dy, src0, src1=None, k=3, in_coef=None, want_bias=True, ups=0):
        B, H, W, cout = dy.shape
        seen.add((k, int(ups), src0.shape[3], 0 if src1 is None else src1.shape[3], cout, H, W, int(in_coef is not None)))
        return orig(dy, src0, src1, k=k, in_coef=in_coef, want_bias=want_bias, ups=ups)
    monkeypatch.setattr(ops, 'conv_wgrad', rec)
    B, S = 2, 128
    d = _dev()
    m, _ = make_cfg(64)
    x, rf, mk = _cond_inputs(B, S, 40)
    ut = train.UnetTrain(m)
    out, saved = ut.forward(x.to(d), torch.tensor([5, 900], device=d), torch.zeros(B, dtype=torch.long, device=d),
                            rf.to(d), mk.to(d), torch.tensor([True, False], device=d))
    ut.backward(saved, rand(tuple(out.shape), 41).to(d))
    del m, ut, saved
    for sc in (False, True):
        m, _ = make_ddp(64, sc)
        ut = train.UnetTrain(m)
        xs = rand((B, 3, S, S), 43).to(d) if sc else None
        out, saved = ut.forward_uncond(rand((B, 3, S, S), 42).to(d), torch.tensor([5, 900], device=d), xs)
        ut.backward(saved, rand(tuple(out.shape), 44).to(d))
        del m, ut, saved
    torch.cuda.synchronize()
    print('[parity] recorded weight-gradient shapes:', sorted(seen))
    assert seen - set(TRAIN_SHAPES) == set(), sorted(seen - set(TRAIN_SHAPES))
    assert set(TRAIN_SHAPES) - seen == set(), sorted(set(TRAIN_SHAPES) - seen)


# ------------------------------------------------------------------------------------------ class embedding backward
def _class_embed_bwd(ops, d, classes, keep, dtable, dnull, nc):
    ops.call('dmh_class_embed_backward', ops.ptr(d), ops.ptr(classes, torch.int64), ops.ptr(keep, torch.uint8),
             ops.ptr(dtable), ops.ptr(dnull), d.shape[0], d.shape[1], nc)


def _class_embed_bwd_ref(d, classes, keep, nc):
    """sequential fp32 sums in row order (the kernel's order): kept rows with an id in [0, nc) into their table row,
    dropped rows into the null row, kept rows with any other id nowhere"""
    D = d.shape[1]
    tab = torch.zeros((nc, D), dtype=torch.float32)
    null = torch.zeros((D,), dtype=torch.float32)
    for b in range(d.shape[0]):
        c = int(classes[b])
        if not keep[b]:
            null += d[b]
        elif 0 <= c < nc:
            tab[c] += d[b]
    return tab, null


@pytest.mark.parametrize('B,D,nc,keep', [(16, 100, 5, 'random'), (16, 256, 3, 'none'), (16, 64, 4, 'all'),
                                         (1, 70, 1, 'all'), (1, 33, 2, 'none'), (37, 200, 9, 'random')])
def test_class_embed_backward_bitwise(ops, B, D, nc, keep):
    """dmh_class_embed_backward == sequential fp32 row-order sums, bitwise: repeated ids, every row dropped / none
    dropped, B = 1, D not a multiple of 64"""
    g = torch.Generator().manual_seed(B * 1000 + D)
    d = torch.randn((B, D), generator=g)
    classes = torch.randint(0, nc, (B,), generator=g)
    k = {'random': torch.rand((B,), generator=g) > 0.3, 'none': torch.zeros(B, dtype=torch.bool),
         'all': torch.ones(B, dtype=torch.bool)}[keep].to(torch.uint8)
    dt, dn = torch.full((nc, D), 7.0, device=_dev()), torch.full((D,), 7.0, device=_dev())
    _class_embed_bwd(ops, d.to(_dev()), classes.to(_dev()), k.to(_dev()), dt, dn, nc)
    rt, rn = _class_embed_bwd_ref(d, classes, k, nc)
    assert torch.equal(dt.cpu(), rt) and torch.equal(dn.cpu(), rn)


def test_class_embed_backward_ignores_out_of_range_ids(ops):
    """kept rows with the ids -1 and num_classes (their forward row is NaN) add to no table row: the gradient table is
    the middle of a sentinel-filled allocation, so a stray write lands in a canary row this test reads"""
    B, D, nc = 12, 100, 4
    g = torch.Generator().manual_seed(77)
    d = torch.randn((B, D), generator=g)
    classes = torch.tensor([-1, nc] * (B // 2))
    k = torch.tensor([1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1], dtype=torch.uint8)
    buf = torch.full((nc + 2, D), 1234.5, device=_dev())
    dn = torch.empty((D,), device=_dev())
    _class_embed_bwd(ops, d.to(_dev()), classes.to(_dev()), k.to(_dev()), buf[1:nc + 1], dn, nc)
    out = buf.cpu()
    assert (out[0] == 1234.5).all() and (out[nc + 1] == 1234.5).all(), 'a write outside the gradient table'
    rt, rn = _class_embed_bwd_ref(d, classes, k, nc)
    assert torch.equal(out[1:nc + 1], rt) and torch.equal(dn.cpu(), rn)


# ------------------------------------------------------------------------------------- small training kernels
@pytest.mark.parametrize('cout,cin', [(8064, 512), (8064, 256), (256, 256), (256, 64)],
                         ids=['stacked-mlp-cfg', 'stacked-mlp-ddp', 'time_mlp.3', 'time_mlp.1'])
@pytest.mark.parametrize('Bn', [1, 16])
def test_linear_backward_vs_fp64(ops, cout, cin, Bn):
    """ops.linear_backward: the split-K branch (cout >= 1024, % 128: the stacked ResnetBlock MLP of the dim-64 models)
    and the direct branch"""
    g = torch.Generator(device=_dev()).manual_seed(cout + cin + Bn)
    x = torch.randn((Bn, cin), generator=g, device=_dev())
    w = torch.randn((cout, cin), generator=g, device=_dev()) * cin ** -0.5
    dy = torch.randn((Bn, cout), generator=g, device=_dev())
    dx, dw, db = ops.linear_backward(x, w, dy)
    rx, rw, rb = dy.double() @ w.double(), dy.double().t() @ x.double(), dy.double().sum(0)
    e = (rel(dx, rx), rel(dw, rw), rel(db, rb))
    print(f'[parity] linear_backward {cout}x{cin} Bn={Bn}: dx={e[0]:.3e} dw={e[1]:.3e} db={e[2]:.3e}')
    if Bn == 1:                        # measured dx 2.2-7.2e-7, dw 2.4-3.9e-8; db is dy itself
        assert e[0] <= 2e-6 and e[1] <= 2.4e-7 and torch.equal(db, dy[0]), e
    else:                              # measured dx 2.2-7.5e-7, dw 1.2-2.0e-7, db 5.7-9.8e-8
        assert e[0] <= 2e-6 and e[1] <= 1.2e-6 and e[2] <= 5e-7, e


def _act_inputs():
    x = torch.cat([torch.linspace(-100, 100, 200001), torch.linspace(-95, -80, 3001), torch.linspace(-16, 4, 4001),
                   torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1e-38, -1.1e-38, 2.0 ** -126, -2.0 ** -126,
                                 1e-30, -1e-30, 100.0, -100.0])])
    return x.float()


# measured 2.71, 3.92, 3.95, 9.54 ulp
ACT_GATES = {('silu', 'forward'): 4.0, ('silu', 'backward'): 6.0, ('gelu', 'forward'): 6.0, ('gelu', 'backward'): 16.0}


def test_act_forward_backward_ulps(ops):
    """ops.act SiLU / GELU forward and backward (dy = 1 and random dy) over |x| <= 100, signed zeros, subnormals.
    Reference in fp64 at the fp32 arguments the kernel forms (x * -1/sqrt2, -x/2 * x).  Forward: ulps of the result;
    backward: ulps of the operation's own scale, |dy| * the largest term of f' (f' has a root where its terms cancel)"""
    x = _act_inputs()
    g = torch.Generator().manual_seed(11)
    dy = torch.randn(x.shape, generator=g)
    xd = x.double()
    t = (x * -0.70710678118654752440).double()                       # fp32 product, as the kernel forms it
    e = ((-0.5 * x) * x).double()
    sg = torch.sigmoid(xd)
    phi = 0.5 * torch.special.erfc(t)
    xg = xd * 0.3989422804014327 * torch.exp(e)
    ref = {'silu': (xd * sg, sg * (1 + xd * (1 - sg)), sg * torch.maximum(torch.ones_like(xd), (xd * (1 - sg)).abs())),
           'gelu': (xd * phi, phi + xg, torch.maximum(phi, xg.abs()))}
    xdev = x.to(_dev())
    worst = {}
    for mode, (f, fp, scale) in ref.items():
        out = ops.act(xdev, mode).cpu().double()
        worst[(mode, 'forward')] = ((out - f).abs() / _ulp32(f)).max().item()
        ub = 0.0
        for dyv in (torch.ones_like(x), dy):
            gb = ops.act(xdev, mode, dy=dyv.to(_dev())).cpu().double()
            ub = max(ub, ((gb - dyv.double() * fp).abs() / _ulp32(dyv.double().abs() * scale)).max().item())
        worst[(mode, 'backward')] = ub
    print('[parity] act: ' + ', '.join(f'{m} {d} {v:.2f} ulp' for (m, d), v in worst.items()))
    for k, v in worst.items():
        assert v <= ACT_GATES[k], (k, v)


@pytest.mark.parametrize('B,S', [(2, 128), (16, 64)])
def test_linear_attention_core_backward_production_sizes(ops, B, S):
    """the LinearAttention core backward at n = 128^2 (128 pixel splits) and at B = 16, n = 64^2, vs fp64 autograd"""
    n = S * S
    g = torch.Generator(device=_dev()).manual_seed(S + B)
    qkv = torch.randn((B, S, S, 384), generator=g, device=_dev()) * 1.5
    dout = torch.randn((B, S, S, 128), generator=g, device=_dev())
    qd = qkv.double().requires_grad_(True)
    q, k, v = [t.reshape(B, n, 4, 32).permute(0, 2, 3, 1) for t in qd.split(128, dim=3)]
    q = q.softmax(dim=-2) * 32 ** -0.5
    k = k.softmax(dim=-1)
    ctx = torch.einsum('bhdn,bhen->bhde', k, v / n)
    out = torch.einsum('bhde,bhdn->bhen', ctx, q).permute(0, 3, 1, 2).reshape(B, S, S, 128)
    (gq,) = torch.autograd.grad(out, (qd,), dout.double())
    o, sv = ops.linear_attention_core_train(qkv, 32 ** -0.5)
    dq = ops.linear_attention_core_backward(sv, dout)
    ef = rel(o, out.detach())
    e = [rel(dq[..., sl], gq[..., sl]) for sl in (slice(0, 128), slice(128, 256), slice(256, 384))]
    print(f'[parity] linattn core B={B} n={S}^2: fwd={ef:.3e} dq={e[0]:.3e} dk={e[1]:.3e} dv={e[2]:.3e}')
    assert ef <= 5e-6 and max(e) <= 2.5e-6, (ef, e)        # measured fwd 5.6-7.5e-7, grads 2.7-8.7e-7


def test_resnet_block_backward_b16(ops):
    """one ResnetBlockTrain forward + backward at the training batch: B = 16, 64x64, 128 -> 128 channels, against the
    fp64 autograd reference of test_gpu_backward.test_resnet_block_backward"""
    from test_gpu_backward import _ref_block
    from gpu_util import rand
    from dmhomo_amd import train
    B, c, H = 16, 128, 64
    P = dict(w1=rand((c, c, 3, 3), 80, (1.0 / (c * 9)) ** 0.5) + 0.01, b1=rand((c,), 81, 0.1),
             g1=1 + 0.2 * rand((c,), 82), be1=0.2 * rand((c,), 83),
             w2=rand((c, c, 3, 3), 84, (1.0 / (c * 9)) ** 0.5) + 0.01, b2=rand((c,), 85, 0.1),
             g2=1 + 0.2 * rand((c,), 86), be2=0.2 * rand((c,), 87))
    x = rand((B, c, H, H), 90)
    ss = 0.3 * rand((B, 2 * c), 91)
    dout = rand((B, c, H, H), 92)
    D = {k: v.double().requires_grad_(True) for k, v in P.items()}
    xd, ssd = x.double().requires_grad_(True), ss.double().requires_grad_(True)
    h = _ref_block(xd, D['w1'], D['b1'], D['g1'], D['be1'], ssd)
    out = _ref_block(h, D['w2'], D['b2'], D['g2'], D['be2'], None) + xd
    names = list(D)
    ref = dict(zip(['x', 'ss'] + names, torch.autograd.grad(out, [xd, ssd] + [D[k] for k in names], dout.double())))
    blk = train.ResnetBlockTrain({k: v.to(_dev()) for k, v in P.items()}, c, 0)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(_dev())
    o, saved = blk.forward(nhwc(x), None, ss.to(_dev()).contiguous())
    dx, gr = blk.backward(saved, nhwc(dout))
    errs = {'out': rel(o.permute(0, 3, 1, 2).cpu(), out.detach()), 'x': rel(dx.permute(0, 3, 1, 2).cpu(), ref['x']),
            'ss': rel(gr['ss'].cpu(), ref['ss'])}
    errs.update({k: rel(gr[k].reshape(ref[k].shape).cpu(), ref[k]) for k in names})
    print('[parity] resnet block B=16 64x64 128ch: ' + ' '.join(f'{k}={v:.2e}' for k, v in errs.items()))
    gates = dict(out=9e-6, x=5e-6, ss=1e-5, w1=7e-6, b1=1.4e-5, g1=1.8e-5, be1=3.7e-5, w2=7e-6, b2=3.6e-6, g2=6e-6,
                 be2=4e-6)                                  # 10x measured, rounded down
    assert all(errs[k] <= v for k, v in gates.items()), errs


@pytest.mark.parametrize('max_norm', [1.0, 1e6], ids=['clipped', 'unclipped'])
def test_clip_adam_multi_vs_fp64(ops, max_norm):
    """ops.clip_adam_multi_ over 53 tensors (two launches: MT_MAX = 48) of 1, 4095, 4096, 4097 and 3 * 4096 + 5
    elements, 3 steps, against clip_grad_norm_ + torch.optim.Adam arithmetic in fp64 (with the fp32 betas the C ABI
    takes).  Errors in ulps of each update's own scale: max(|b1 m|, |(1 - b1) g|) for m, likewise for v, and
    max(|p|, |step|) for p (the sums cancel where the terms have opposite signs)"""
    sizes = [1, 4095, 4096, 4097, 3 * 4096 + 5] * 10 + [4097, 1, 4096]
    lr, b1, b2, eps = 1e-3, 0.9, 0.99, 1e-8
    g = torch.Generator().manual_seed(123)
    p0 = [torch.randn(n, generator=g) for n in sizes]
    P = [t.to(_dev()) for t in p0]
    M = [torch.zeros_like(t) for t in P]
    V = [torch.zeros_like(t) for t in P]
    rp, rm, rv = [t.double() for t in p0], [torch.zeros(n, dtype=torch.float64) for n in sizes], \
        [torch.zeros(n, dtype=torch.float64) for n in sizes]
    worst = dict(norm=0.0, p=0.0, m=0.0, v=0.0)
    for step in range(1, 4):
        gs = [torch.randn(n, generator=g) * 0.05 * step for n in sizes]
        clip = ops.clip_adam_multi_(P, [t.to(_dev()) for t in gs], M, V, max_norm, lr, b1, b2, eps, step)
        nrm = torch.sqrt(sum((t.double() ** 2).sum() for t in gs))
        coef = min(1.0, max_norm / (nrm.item() + 1e-6))
        assert (coef < 1.0) == (max_norm == 1.0)
        c = clip.cpu().double()
        worst['norm'] = max(worst['norm'], abs(c[0].item() - nrm.item()) / nrm.item(), abs(c[1].item() - coef) / coef)
        for i, gr in enumerate(gs):
            (rp[i], rm[i], rv[i]), (sp, sm, sv) = adam_step64(rp[i], rm[i], rv[i], gr, c[1].item(), step, lr, b1, b2, eps)
            for key, got, want, sc in (('p', P[i], rp[i], sp), ('m', M[i], rm[i], sm), ('v', V[i], rv[i], sv)):
                worst[key] = max(worst[key], ((got.cpu().double() - want).abs() / _ulp32(sc)).max().item())
            rp[i], rm[i], rv[i] = P[i].cpu().double(), M[i].cpu().double(), V[i].cpu().double()   # next step from the kernel's state
    print(f'[parity] clip_adam_multi ({max_norm}): norm/coef rel={worst["norm"]:.2e}, ulps p={worst["p"]:.2f} '
          f'm={worst["m"]:.2f} v={worst["v"]:.2f}')
    # measured: norm 1.6e-8 / 6.1e-8, p 9.5 / 14.9 ulp (the kernel forms the bias corrections in fp32), m 2.0 / 2.7,
    # v 2.7 / 3.7 (unclipped / clipped)
    assert worst['norm'] <= 1.5e-7 and worst['p'] <= 40 and worst['m'] <= 8 and worst['v'] <= 12, worst
