"""CPU half of tests/test_gpu_aux.py: the statements, yardsticks and bounds of tests/aux_cases.py hold on their own.

Every float64-gated output has its fp32 yardstick e32 computed here and held under CAP = 2e-5 ([yardstick] lines); the
loss-gradient statement is the float64 autograd gradient of p_losses; the layout, resize, morphology and geometry statements
agree with independent float64 / torch / scipy forms of the same operation; and wrong kernels restated on the CPU miss their
gates, each by the factor its [mutation] line prints."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_cases as ax
from gpu_util import rand
from oracle import dataset as OD
from oracle import geometry as OG


# ------------------------------------------------------------------ 1. dmh_loss_backward
@pytest.mark.parametrize('case', ax.LB_CASES, ids=ax.lb_id)
def test_loss_backward_yardstick(case):
    """e32 of both halves of dout for every mask and both losses, under CAP; and what each flow kind is there for"""
    shape, kind = case
    B, H, W = shape
    for mkind in ax.LB_MASKS:
        for squared in (False, True):
            r = ax.lb_reference(shape, kind, mkind, squared)
            for name, sl in (('dout[:, :3]', slice(0, 3)), ('dout[:, 3:]', slice(3, 6))):
                r64, r32 = r['ref64']['dout'][:, sl], r['ref32']['dout'][:, sl]
                assert bool(torch.isfinite(r64).all()) and r64.abs().max().item() > 0
                e32 = ax.rel(r32, r64)
                print(f'[yardstick] loss_backward {ax.lb_id(case)} {mkind} {"l2" if squared else "l1"} {name}: '
                      f'e32={e32:.3e} gate={ax.gate(e32):.3e} ref_absmax={r64.abs().max().item():.3e}')
                assert e32 <= ax.CAP
    t = ax.lb_reference(shape, kind, 'random', True)['taps']
    flat = (t['y0'] * W + t['x0']).reshape(B, -1)
    if kind == 'far':
        assert not t['x1ok'].any() and not t['y1ok'].any() and bool((flat == H * W - 1).all())
    if kind == 'fold':
        assert all(len(set(row.tolist())) == 1 for row in flat)          # (the fractions up to the rounding of 2 x / (W - 1))
        assert bool(((t['w'] - 0.25).abs() < 1e-5).all()) and bool(((t['n'] - 0.5).abs() < 1e-5).all())
    if kind == 'zero':     # (W - 1 = 15: 2 x / 15 rounds, a coordinate may come out one fp32 step below its pixel, w = 1 - 2^-20)
        near = (t['w'] < 1e-5) | (t['w'] > 1 - 1e-5)
        assert bool(near.all()) and bool(((flat - torch.arange(H * W)).abs() <= W + 1).all())
    if kind == 'frac' and H * W >= 15:
        ix, iy, _, _ = OG.warp_coords(ax.lb_inputs(shape, kind)['flow'])
        assert ix.min() == 0 and ix.max() == W - 1 and iy.min() == 0 and iy.max() == H - 1      # leaves on every side


def _ref_flow_warp(x, flow):
    """the reference's flow_warp (DDP:1262-1280) as the torch op it calls"""
    B, _, H, W = x.shape
    xs = torch.arange(W, dtype=x.dtype).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, dtype=x.dtype).view(1, H, 1).expand(B, H, W)
    gx = 2.0 * (xs + flow[:, 0]) / (W - 1) - 1.0
    gy = 2.0 * (ys + flow[:, 1]) / (H - 1) - 1.0
    return F.grid_sample(x, torch.stack([gx, gy], -1), mode='bilinear', padding_mode='border', align_corners=True)


@pytest.mark.parametrize('case', ax.LB_CASES, ids=ax.lb_id)
def test_loss_backward_statement_is_the_gradient_of_p_losses(case):
    """with the float64 warp as ``warped`` and every |warped - im1| > 1e-3 (so that no L1 sign hangs on the warp's rounding)
    the statement agrees with float64 autograd of the full loss through F.grid_sample within 1e-5 of the gradient's maximum;
    what is left is the fp32 versus float64 coordinates of the taps"""
    shape, kind = case
    B, H, W = shape
    for mkind in ('random', 'ones'):
        inp = dict(ax.lb_inputs(shape, kind, mkind))
        out = inp['out'].clone()
        w64 = _ref_flow_warp(out[:, 3:].double(), inp['flow'].double())
        near = (w64 - out[:, :3].double()).abs() < 2e-3
        out[:, :3] = torch.where(near, out[:, :3] + 0.01, out[:, :3])           # (the warp reads out[:, 3:] only)
        inp['out'] = out
        assert (w64 - out[:, :3].double()).abs().min().item() > 1e-3
        for squared in (False, True):
            od = out.double().requires_grad_(True)
            fn = F.mse_loss if squared else F.l1_loss
            wr = _ref_flow_warp(od[:, 3:], inp['flow'].double())
            loss = fn(od, inp['target'].double(), reduction='none').reshape(B, -1).mean() + \
                (inp['abar'].double()[:, None] *
                 (inp['mask'].double() * fn(wr, od[:, :3], reduction='none')).reshape(B, -1)).mean()
            gref, = torch.autograd.grad(loss, od)
            st = ax.lb_statement(inp, squared, torch.float64, warped=w64)['dout']
            e = ax.rel(st, gref)
            print(f'[yardstick] loss_backward statement vs float64 autograd {ax.lb_id(case)} {mkind} '
                  f'{"l2" if squared else "l1"}: {e:.3e}')
            assert e <= 1e-5


def test_loss_backward_l1_sign_needs_warped_as_input():
    """the reason ``warped`` is taken as given: where |warped - im1| is below the warp's rounding, a reference that warps in
    float64 takes another sign and is n2 or 2 n2 away, O(1) of the gradient.  Shown on a plane of planted ties."""
    shape, kind = (3, 16, 16), 'frac'
    inp = dict(ax.lb_inputs(shape, kind, 'ones'))
    w64 = _ref_flow_warp(inp['out'][:, 3:].double(), inp['flow'].double())
    out = inp['out'].clone()
    out[1, 0] = inp['warped'][1, 0]              # im1 = the fp32 warp on one plane: sign 0 there, +-1 by the float64 warp
    inp['out'] = out
    a = ax.lb_statement(inp, False, torch.float64)['dout']
    b = ax.lb_statement(inp, False, torch.float64, warped=w64.clone())['dout']
    flips = int((torch.sign(inp['warped'].double() - out[:, :3].double()) != torch.sign(w64 - out[:, :3].double())).sum())
    e = ax.rel(b, a)
    print(f'[yardstick] loss_backward l1: {flips} sign(s) differ between the fp32 and the float64 warp, statement moves {e:.3e}')
    assert flips >= 1 and e > 0.1


@pytest.mark.parametrize('mutate', ax.LB_MUTATIONS)
def test_loss_backward_mutations_miss(mutate):
    """restated wrong kernels against the gate of the case they are worst at.  'x1ok_dropped' is the exception and is held to
    be INVISIBLE: the coordinate is clipped to W - 1 before the floor, so x0 = W - 1 only where ix = W - 1 exactly and the
    weight w = ix - x0 of the tap one past the row is exactly 0 (likewise y1ok) — the guard keeps an address inside the
    plane, not a value out of the sum.  No value test can see it; 'x1ok_strict' (the guard one column too early) is the
    neighbouring mistake that a value test does see."""
    worst, where = 0.0, None
    for shape, kind in ax.LB_CASES:
        for squared in (False, True):
            r = ax.lb_reference(shape, kind, 'ones', squared)
            bad = ax.lb_statement(r['inp'], squared, torch.float32, mutate=mutate)['dout']
            for sl in (slice(0, 3), slice(3, 6)):
                r64, r32 = r['ref64']['dout'][:, sl], r['ref32']['dout'][:, sl]
                f = ax.rel(bad[:, sl], r64) / ax.gate(ax.rel(r32, r64))
                if f > worst:
                    worst, where = f, (ax.lb_id((shape, kind)), 'l2' if squared else 'l1', sl.start)
    print(f'[mutation] loss_backward {mutate}: misses its gate {worst:.3g}x at {where}')
    if mutate == 'x1ok_dropped':
        assert worst <= 1.0, worst
        t = ax.lb_taps(ax.lb_inputs((2, 9, 29), 'frac')['flow'])
        assert bool((t['w'][~t['x1ok']] == 0).all()) and bool((t['n'][~t['y1ok']] == 0).all()) and int((~t['x1ok']).sum()) > 0
    else:
        assert worst >= 10.0, worst


def test_loss_backward_exact_shapes_and_adjoint_yardstick():
    """zero flow at (5, 9) and (17, 17): integer coordinates, weights exactly 1 and 0, so the fp32 statement of dout[:, 3:]
    is fl32(g + gD) bit for bit; and the adjoint identity <scatter(gD), x> = <gD, flow_warp(x)> holds for the fp32 statement
    and the oracle's fp32 warp far inside the floor of the gate"""
    for shape in ax.LB_EXACT_SHAPES:
        for squared in (False, True):
            inp = ax.lb_inputs(shape, 'zero', 'random')
            t = ax.lb_taps(inp['flow'])
            assert bool((t['s'] * t['e'] == 1).all()) and bool((t['w'] == 0).all()) and bool((t['n'] == 0).all())
            g, gD = ax.lb_direct32(inp, squared)
            st = ax.lb_statement(inp, squared, torch.float32)
            assert torch.equal(st['scat'], st['gD'])
            assert ax.rel(g, st['g'].double()) <= 2 * ax.U and ax.rel(gD, st['gD'].double()) <= 4 * ax.U
    worst = 0.0
    for shape, kind in ax.LB_CASES:
        r = ax.lb_reference(shape, kind, 'random', True)
        x = rand(r['inp']['warped'].shape, 7500)
        wx = OG.flow_warp(x, r['inp']['flow'])
        lhs, rhs, scale = ax.lb_adjoint(r['ref32']['scat'], r['ref64']['gD'], x, wx)
        worst = max(worst, abs(lhs - rhs) / scale)
    print(f'[yardstick] loss_backward adjoint identity, fp32 statement and fp32 warp: e32={worst:.3e} of sum |gD||warp(x)|')
    assert worst <= ax.CAP and ax.gate(worst) == ax.FLOOR


# ------------------------------------------------------------------ 2. dmh_loss_backward_ddp
def test_loss_backward_ddp_statement():
    """the fp32 statement is within 3 roundings of the float64 gradient of mean_b w_b mean l(out - target) * scale, its
    planted zeros are exact, and the loop case is the smallest with a second trip"""
    for (B, per) in ax.DDP_CASES + [(2, 4099)]:
        inp = ax.ddp_inputs(B, per)
        assert len(set(inp['w'].tolist())) == B
        for squared in (False, True):
            for scale in ax.DDP_SCALES:
                od = inp['out'].double().requires_grad_(True)
                fn = F.mse_loss if squared else F.l1_loss
                loss = scale * (inp['w'].double() * fn(od, inp['target'].double(), reduction='none').mean(1)).mean()
                gref, = torch.autograd.grad(loss, od)
                st = ax.ddp_statement32(inp, squared, scale)
                e = ax.rel(st, gref)
                print(f'[yardstick] loss_backward_ddp B={B} per={per} {"l2" if squared else "l1"} scale={scale}: e32={e:.3e}')
                assert e <= 4 * ax.U
                assert not st.view(-1)[::7].any()
    B, per = ax.DDP_LOOP_CASE
    total, cap = B * per, ax.DDP_BLOCK_CAP * 256
    assert cap < total <= cap + 256 and total - 6 == cap and float(np.float32(per)) == per


# ------------------------------------------------------------------ 3. layout helpers
def test_layout_statements():
    """d2s is the inverse of the channel order conv_down_dgrad_pack documents; sumpool2 is the backward of nearest x2
    upsampling; s2d_shift followed by the 2x2 valid convolution with the weight reshaped as conv_down_backward does is the
    4x4 / stride 2 / pad 1 convolution — in float64"""
    for B in ax.LAYOUT_B:
        for (H, W) in ax.LAYOUT_HW:
            C = 12
            dx = rand((B, 2 * H, 2 * W, C), 7300 + H).double()
            packed = torch.empty((B, H, W, 4 * C), dtype=torch.float64)
            for ry in (0, 1):
                for rx in (0, 1):           # out[m][l][(ry*2+rx)*C + c] = dx[2m+ry][2l+rx][c]
                    packed[..., (ry * 2 + rx) * C:(ry * 2 + rx + 1) * C] = dx[:, ry::2, rx::2]
            assert torch.equal(ax.d2s_ref(packed), dx)
            xs = rand((B, C, H, W), 7301 + W).double().requires_grad_(True)
            gup = rand((B, C, 2 * H, 2 * W), 7302).double()
            (gx,) = torch.autograd.grad(F.interpolate(xs, scale_factor=2, mode='nearest'), xs, gup)
            mine = ax.sumpool2_ref(gup.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
            assert ax.rel(mine, gx) <= 1e-15
            x = rand((B, H, W, C), 7303).double()
            w = rand((5, C, 4, 4), 7304).double()
            X = ax.s2d_shift_ref(x)
            a = F.conv2d(X.permute(0, 3, 1, 2), ax.down_weight_as_2x2(w))
            b = F.conv2d(x.permute(0, 3, 1, 2), w, stride=2, padding=1)
            assert a.shape == b.shape and ax.rel(a, b) <= 1e-14
    x = ax.iota((1, 2, 2, 4))
    X = ax.s2d_shift_ref(x)
    assert X.shape == (1, 2, 2, 16) and X[0, 0, 0, 12:].tolist() == [0., 1., 2., 3.] and not X[0, 0, 0, :12].any()
    assert int(np.signbit(X.numpy()).sum()) == 0                                    # the border is +0.0
    quads = sorted({B * (H // 2 + 1) * (W // 2 + 1) * C for B in ax.LAYOUT_B for H, W in ax.LAYOUT_HW for C in ax.LAYOUT_C})
    assert quads[0] < 256 < quads[-1] and any(q % 256 for q in quads)               # below and above one block, ragged


def test_layout_mutations_miss():
    """exchanged parities and a transposed pixel each move elements: the index-valued input names them"""
    x = ax.iota((1, 6, 4, 4))
    good = ax.s2d_shift_ref(x)
    bad = good.view(1, 4, 3, 2, 2, 4).transpose(3, 4).reshape(good.shape)          # (py, px) exchanged
    n = int((bad != good).sum())
    print(f'[mutation] s2d_shift with py and px exchanged: {n} of {good.numel()} elements differ bitwise, allowed 0')
    assert n > 0
    a = ax.iota((1, 2, 3, 16))
    good = ax.d2s_ref(a)
    bad = a.view(1, 2, 3, 2, 2, 4).permute(0, 1, 4, 2, 3, 5).reshape(good.shape)   # ry and rx exchanged
    n = int((bad != good).sum())
    print(f'[mutation] d2s with ry and rx exchanged: {n} of {good.numel()} elements differ bitwise, allowed 0')
    assert n > 0
    r = rand((1, 4, 6, 4), 7310)
    good = ax.sumpool2_ref(r)
    v = r.view(1, 2, 2, 3, 2, 4)
    bad = ((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + v[:, :, 1, :, 0]) + v[:, :, 1, :, 1]      # a left-to-right sum
    n = int((bad != good).sum())
    print(f'[mutation] sumpool2 summed left to right: {n} of {good.numel()} elements differ bitwise, allowed 0')
    assert n > 0


# ------------------------------------------------------------------ 4. dataset kernels
@pytest.mark.parametrize('sizes', ax.RESIZE_SIZES, ids=lambda s: f'{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}')
def test_resize_statements(sizes):
    """the fp32 restatement of the kernel's taps is oracle.dataset.resize_linear bit for bit (so the mutations below are
    mutations of the oracle), the oracle is within the derived bound of plain float64 interpolation, scale 1 is src / div
    exactly, and the up case takes both clamp branches on both axes"""
    (hs, ws), (hd, wd) = sizes
    for C in ax.RESIZE_C:
        for div in ax.RESIZE_DIV:
            for kind in ('random', 'zeros', 'full'):
                src = ax.resize_src(3, hs, ws, C, kind)
                want = ax.resize_oracle(src, hd, wd, div)
                assert np.array_equal(ax.resize_plain(src, hd, wd, div, np.float32).view(np.int32), want.view(np.int32))
                e = np.abs(want.astype(np.float64) - ax.resize_plain(src, hd, wd, div)).max()
                assert e <= ax.resize_bound(div), (e, ax.resize_bound(div))
                if (hs, ws) == (hd, wd):
                    assert np.array_equal(want, (src.astype(np.float32) / np.float32(div)).transpose(0, 3, 1, 2))
                if kind == 'full':
                    assert np.array_equal(want, np.full_like(want, np.float32(255.0) / np.float32(div)))
    print(f'[yardstick] resize {hs}x{ws} -> {hd}x{wd}: oracle within {ax.resize_bound(255.0):.3e} (div 255) of float64')
    if (hs, ws) == (5, 7):
        for nd, ns in ((hd, hs), (wd, ws)):
            f = ((np.arange(nd) + 0.5) * (ns / nd) - 0.5).astype(np.float32)
            assert np.floor(f).min() < 0 and np.floor(f).max() >= ns - 1


@pytest.mark.parametrize('mutate', ax.RESIZE_MUTATIONS)
def test_resize_mutations_miss(mutate):
    """the gate of the resize is bitwise: a restated wrong kernel misses it by its count of differing elements; the factor
    over the float64 bound is printed beside it.  'clamp_at_n' keeps the fraction where the tap pair collapses onto the last
    pixel, v (1 - f) + v f: a rounding apart from v at most, which only the bitwise comparison sees."""
    worst_n, worst_f = 0, 0.0
    for (hs, ws), (hd, wd) in ax.RESIZE_SIZES:
        if mutate == 'fractions_swapped' and hd != wd:
            continue
        src = ax.resize_src(3, hs, ws, 3)
        want = ax.resize_oracle(src, hd, wd, 255.0)
        bad = ax.resize_plain(src, hd, wd, 255.0, np.float32, mutate)
        worst_n = max(worst_n, int((bad.view(np.int32) != want.view(np.int32)).sum()))
        worst_f = max(worst_f, np.abs(bad.astype(np.float64) - ax.resize_plain(src, hd, wd, 255.0)).max() / ax.resize_bound(255.0))
    print(f'[mutation] resize {mutate}: up to {worst_n} elements differ bitwise from the oracle (allowed 0), '
          f'{worst_f:.3g}x the float64 bound')
    assert worst_n > 0
    if mutate != 'clamp_at_n':
        assert worst_f >= 10.0


@pytest.mark.parametrize('sizes', ax.MASK_SIZES, ids=lambda s: f'{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}')
def test_mask_open_statements(sizes):
    """oracle.dataset's nearest resize + opening equals scipy.ndimage's grey erosion / dilation with outside pixels ignored,
    for every input kind; all ones stays all ones; a single one is removed; a 3x3 block survives at scale 1"""
    (hs, ws), (hd, wd) = sizes
    for kind in ax.MASK_KINDS:
        m = ax.mask_src(kind, 3, hs, ws)
        a, b = ax.mask_oracle(m, hd, wd), ax.mask_scipy(m, hd, wd)
        assert a.shape == (3, hd, wd) and np.array_equal(a, b), (kind, sizes)
        if kind == 'ones':
            assert bool((a == 1).all())
        if (hs, ws) == (hd, wd) == (7, 9):
            if kind == 'single1':
                assert not a.any()
            if kind == 'block3':
                assert np.array_equal(a, m)
            if kind == 'single0':
                assert int((a == 0).sum()) == 3 and not a[:, 3, 4].any()      # the dilation closes the eroded hole up to its centre


def test_mask_open_mutation_misses():
    """an opening that counts outside pixels as 0 empties the border; a closing instead of an opening keeps the single one"""
    m = ax.mask_src('ones', 1, 7, 9)
    p = np.pad(OD.resize_nearest(m[0], 7, 9), 1)
    er = np.min([p[dy:dy + 7, dx:dx + 9] for dy in range(3) for dx in range(3)], axis=0)
    n = int((er != ax.mask_oracle(m, 7, 9)[0]).sum())
    print(f'[mutation] mask opening with a zero border: {n} of 63 elements differ, allowed 0')
    assert n == 63 - 5 * 7
    m = ax.mask_src('single1', 1, 7, 9)
    closed = OD.erode3(OD.dilate3(m[0]))
    n = int((closed != ax.mask_oracle(m, 7, 9)[0]).sum())
    print(f'[mutation] mask closing instead of opening: {n} of 63 elements differ, allowed 0')
    assert n == 1


# ------------------------------------------------------------------ 5. geometry helpers
def test_geometry_statements():
    """the grid statements are the oracle's mesh and normalisation; the band rule of the points statement against a per-row
    loop; the integer-grid points statement rounded to fp32 is oracle.geometry.homo_to_flow"""
    for (B, H, W) in ax.GRID_SHAPES:
        g = ax.pixel_grid_ref(B, H, W, 0.0)
        assert g.shape == (B, 2, H, W) and g[0, 0, 0].tolist() == list(range(W)) and g[0, 1, :, 0].tolist() == list(range(H))
        if H > 1 and W > 1:
            ix, iy, _, _ = OG.warp_coords(torch.zeros((B, 2, H, W)))
            ng = ax.norm_grid_ref(g)
            assert ng.shape == (B, H, W, 2)
            assert torch.equal(((ng[..., 0] + 1) * torch.tensor((W - 1) / 2, dtype=torch.float32)).clamp(0, W - 1), ix)
    ng = ax.norm_grid_ref(ax.pixel_grid_ref(1, 1, 1, 0.0))
    assert bool(torch.isnan(ng).all())                                  # 0 / 0 on both axes
    for case in ax.FLOW_POINTS_CASES:
        B, divide, Bi, H, W = case
        Hm, idx = ax.flow_points_inputs(case)
        ref = ax.flow_points_ref(Hm, idx)
        assert ref.shape == (B, 2, H, W)
        for b in range(B):
            for y in range(H):
                h = Hm[b, min(y // (H // divide), divide - 1)]
                p = idx[b if Bi > 1 else 0, :, y]                      # (3, W)
                q = h @ p
                want = np.stack([q[0] / (q[2] + 1e-6) - p[0], q[1] / (q[2] + 1e-6) - p[1]])
                assert np.abs(ref[b, :, y] - want).max() <= 1e-12
    assert {H * W for _, _, _, H, W in ax.FLOW_POINTS_CASES} >= {255, 256, 261}
    for (B, H, W) in ax.HFLOW_CASES:
        Hm = ax.homographies((B,), 7950 + H)
        pts = ax.flow_points_ref(Hm[:, None], ax.int_grid(H, W)).astype(np.float32)
        for b in range(B):
            assert np.array_equal(pts[b].transpose(1, 2, 0), OG.homo_to_flow(Hm[b], H, W))


def test_flow_image_edge_field():
    """the edge field holds what it names, and the oracle gives the colours derived by hand there"""
    for mf in ax.MAX_FLOWS:
        fl = ax.edge_flows(mf)
        n = fl.shape[0]
        img = ax.flow_image_oracle(fl.T.reshape(1, 2, 1, n), mf)[0, :, 0].T          # (n, 3)
        assert bool(np.isfinite(img).all()) and img.min() >= 0 and img.max() <= 1
        assert np.array_equal(img[:4], np.ones((4, 3), np.float32))                    # zero flow, every sign of zero: grey 1
        tiny = np.abs(fl).max(1) == np.float32(1e-30)
        assert tiny.sum() == 12 and np.array_equal(img[tiny], np.ones((12, 3), np.float32))
        sat = np.float32(mf / 8.0)
        axis = {(1, 0): (1, 0, 0), (-1, 0): (0, 1, 1), (0, 1): (0.5, 1, 0), (0, -1): (0.5, 0, 1)}  # hue 0, 1/2, 1/4, 3/4
        seen = 0
        for i in range(n):
            u, v = fl[i]
            if max(abs(u), abs(v)) >= sat and (u == 0 or v == 0):
                want = axis[(int(np.sign(u)), int(np.sign(v)))]
                assert np.abs(img[i] - np.array(want)).max() <= 2e-6, (fl[i], img[i])
                seen += 1
        assert seen == 16 and int(np.signbit(fl).sum()) > 20


def test_flow_image_mutation_misses():
    """a saturation that is not clamped, and a hue taken without the + 1 (negative angles wrap wrongly), against 2e-5"""
    fl = ax.edge_flows(256.0)
    want = ax.flow_image_oracle(fl.T.reshape(1, 2, 1, -1), 256.0)
    scaled = ax.flow_image_oracle((fl * np.float32(0.5)).T.reshape(1, 2, 1, -1), 256.0)     # as if max_flow were doubled
    f = np.abs(scaled - want).max() / 2e-5
    print(f'[mutation] flow_to_image at half the saturation: misses 2e-5 by {f:.3g}x')
    assert f >= 10
    flipped = ax.flow_image_oracle((fl * np.float32([1, -1])).T.reshape(1, 2, 1, -1), 256.0)  # v negated: hue mirrored
    f = np.abs(flipped - want).max() / 2e-5
    print(f'[mutation] flow_to_image with v negated: misses 2e-5 by {f:.3g}x')
    assert f >= 10


# ------------------------------------------------------------------ 6. optimiser
def test_optimiser_statements():
    """the shared float64 Adam step is torch.optim.Adam (float64) on the scaled gradient; the fp32 statement of the EMA is
    inside the derived 2 ulp; the sizes reach the second trip of dmh_sumsq"""
    n = 257
    p0, grads = ax.opt_tensors(n)
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=ax.ADAM['lr'], betas=(ax.f32(ax.ADAM['b1']), ax.f32(ax.ADAM['b2'])), eps=ax.ADAM['eps'])
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step, g in enumerate(grads, 1):
        ref.grad = g.double() * 0.5
        opt.step()
        (p, m, v), _ = ax.adam_step64(p, m, v, g, 0.5, step, **ax.ADAM)
        assert ax.rel(p, ref.detach()) <= 1e-13
    worst = 0.0
    for decay in ax.EMA_DECAYS:
        assert float(np.float32(1) - np.float32(decay)) == 1.0 - ax.f32(decay)
        ema, pp = rand((65537,), 8100), rand((65537,), 8101)
        st = ema + (1 - torch.tensor(decay, dtype=torch.float32)) * (pp - ema)
        ulps = ((st.double() - ax.ema_ref64(ema, pp, decay)).abs() / ax.ulp32_spacing(torch.maximum(ema.abs(), pp.abs()).double())).max()
        worst = max(worst, ulps.item())
    print(f'[yardstick] ema fp32 statement: {worst:.2f} ulp of max(|ema|, |p|), bound {ax.EMA_ULPS}')
    assert worst <= ax.EMA_ULPS
    assert ax.OPT_SIZES[-1] == 256 * 256 + 1
    for n in ax.OPT_SIZES:
        for g in ax.opt_tensors(n)[1]:
            assert [ax.norm_coef64(g, mx)[1] < 1.0 for mx in ax.OPT_MAX_NORMS] == [False, True]
