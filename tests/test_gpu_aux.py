"""-m gpu: the loss-gradient, layout, dataset, geometry and single-tensor optimiser kernels, each ALONE through the C ABI —
dmh_loss_backward and dmh_loss_backward_ddp, dmh_sumsq / dmh_gradnorm_finalize / dmh_adam / dmh_ema of csrc/train_misc.hip;
dmh_s2d_shift, dmh_d2s and dmh_sumpool2 of csrc/conv_backward.hip; dmh_resize_bilinear_u8 and dmh_mask_open_nearest of
csrc/dataset.hip; dmh_pixel_grid, dmh_norm_grid, dmh_homography_flow_points, dmh_homography_flow and dmh_flow_to_image of
csrc/geometry.hip — against a float64 statement of the operation on the CPU, or bit for bit against fp32 torch / numpy where
the kernel keeps that op order.  Cases, statements and gates: tests/aux_cases.py (its yardsticks, cross-checks and mutations
are held on the CPU by tests/test_aux_host.py).  Every output is the interior of a NaN-filled buffer with guard bands: an
element never written fails, a write outside fails, and the inputs are bitwise unchanged after the launch.  Every assertion
prints a [parity] line."""
import ctypes as C

import numpy as np
import pytest
import torch

import aux_cases as ax
from gpu_util import dev, rand

pytestmark = pytest.mark.gpu

GUARD = 64          # elements on each side of an output (256 bytes of fp32: the interior keeps its 16-byte alignment)
_INT = {4: torch.int32, 8: torch.int64, 1: torch.uint8}


@pytest.fixture(scope='module')
def ops():
    from dmhomo_amd import ops as _ops
    _ops.lib()
    return _ops


def _d(t):
    return None if t is None else torch.as_tensor(t).to(dev()).contiguous()


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _poisoned(shape, dtype=torch.float32):
    """-> (whole NaN-filled buffer, its interior viewed as ``shape``)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev(), dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_untouched(buf):
    nan = _bits(torch.full((1,), float('nan'), dtype=buf.dtype))[0].item()
    b = _bits(buf)
    return bool((b[:GUARD] == nan).all()) and bool((b[-GUARD:] == nan).all())


def _bitwise(name, got, want):
    """got == want bit for bit (NaN == NaN, -0.0 != +0.0: compared as integers), printing the mismatch count and the first
    mismatch"""
    got, want = torch.as_tensor(got).cpu().contiguous(), torch.as_tensor(want).cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    ne = _bits(got) != _bits(want)
    bad = int(ne.sum())
    first = ''
    if bad:
        i = tuple(ne.nonzero()[0].tolist())
        first = f'; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}'
    print(f'[parity] {name}: {bad} of {got.numel()} elements differ bitwise, allowed 0{first}')
    assert bad == 0, name + first


def _unchanged(name, pairs):
    for k, (d, h) in pairs.items():
        assert torch.equal(_bits(d.cpu()), _bits(torch.as_tensor(h))), f'{name}: the launch changed its input {k}'


# ------------------------------------------------------------------ 1. dmh_loss_backward
def _lb_run(ops, inp, squared):
    """-> dout (B, 6, H, W), gD (B, 3, H, W) on the CPU, from poisoned buffers"""
    B, _, H, W = inp['out'].shape
    d = {k: _d(v) for k, v in inp.items()}
    dbuf, dout = _poisoned((B, 6, H, W))
    gbuf, gD = _poisoned((B, 3, H, W))
    ops.call('dmh_loss_backward', ops.ptr(d['out']), ops.ptr(d['target']), ops.ptr(d['warped']), ops.ptr(d['mask']),
             ops.ptr(d['flow']), ops.ptr(d['abar']), ops.ptr(dout), ops.ptr(gD), B, H, W, int(squared))
    torch.cuda.synchronize()
    assert _guards_untouched(dbuf) and _guards_untouched(gbuf), 'dmh_loss_backward wrote outside dout / gD'
    _unchanged('dmh_loss_backward', {k: (d[k], inp[k]) for k in inp})
    return dout.cpu(), gD.cpu()


@pytest.mark.parametrize('case', ax.LB_CASES, ids=ax.lb_id)
def test_loss_backward_vs_statement(ops, case):
    """both halves of dout within max(5e-6, 10 * e32) of the float64 statement that takes the fp32 ``warped`` as given, for
    three masks and both losses; gD likewise; the forward's corner indices (and its output) are those the statement scatters
    to; and the kernel's scatter is the transpose of the forward warp: <scatter(gD), x> = <gD, flow_warp(x)>.
    (No run-to-run equality here: 'fold', 'far' and 'frac' collide, and the float atomics are the one free summation order
    in the library.)"""
    shape, kind = case
    tag = ax.lb_id(case)
    for mkind in ax.LB_MASKS:
        for squared in (False, True):
            r = ax.lb_reference(shape, kind, mkind, squared)
            dout, gD = _lb_run(ops, r['inp'], squared)
            name = f'loss_backward {tag} {mkind} {"l2" if squared else "l1"}'
            for half, sl in (('dout[:, :3]', slice(0, 3)), ('dout[:, 3:]', slice(3, 6))):
                ax.check(f'{name} {half}', dout[:, sl], r['ref64']['dout'][:, sl], r['ref32']['dout'][:, sl])
            if mkind != 'zeros':
                ax.check(f'{name} gD', gD, r['ref64']['gD'], r['ref32']['gD'])
    r = ax.lb_reference(shape, kind, 'random', True)
    inp, taps = r['inp'], r['taps']
    flow = _d(inp['flow'])
    wbuf, wout = _poisoned(inp['warped'].shape)
    B, _, H, W = inp['out'].shape
    x0 = torch.full((B, H, W), -7, device=dev(), dtype=torch.int32)
    y0 = torch.full((B, H, W), -7, device=dev(), dtype=torch.int32)
    im2 = _d(inp['out'][:, 3:])
    ops.call('dmh_flow_warp', ops.ptr(im2), ops.ptr(flow), ops.ptr(wout), ops.ptr(x0, torch.int32),
             ops.ptr(y0, torch.int32), B, 3, H, W, 0, 0)
    assert _guards_untouched(wbuf)
    nx, ny = int((x0.cpu().long() != taps['x0']).sum()), int((y0.cpu().long() != taps['y0']).sum())
    print(f'[parity] flow_warp {tag} corner indices vs the statement: {nx} x0 and {ny} y0 of {B * H * W} differ, allowed 0')
    assert nx == 0 and ny == 0
    _bitwise(f'flow_warp {tag} output vs the oracle (the ``warped`` the cases are given)', wout, inp['warped'])
    dout, gD = _lb_run(ops, inp, True)
    g32, _ = ax.lb_direct32(inp, True)
    x = rand(inp['warped'].shape, 7500)
    wx = ops.flow_warp(_d(x), flow).cpu()
    lhs, rhs, scale = ax.lb_adjoint(dout[:, 3:].double() - g32[:, 3:].double(), r['ref64']['gD'], x, wx)
    err = abs(lhs - rhs) / scale
    print(f'[parity] loss_backward {tag} adjoint: <scatter(gD), x> = {lhs:.9e}, <gD, flow_warp(x)> = {rhs:.9e}, '
          f'|difference| = {err:.3e} of sum |gD||flow_warp(x)|, gate {ax.FLOOR:.1e}')
    assert err <= ax.FLOOR         # (e32 of the identity is 9e-8 on the CPU, tests/test_aux_host.py: the gate is the floor)


@pytest.mark.parametrize('shape', ax.LB_EXACT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_loss_backward_known_answers(ops, shape):
    """zero flow at H - 1 and W - 1 powers of two: every coordinate is an exact integer, each pixel makes one contribution
    of weight 1 and the zero-weight ones add signed zeros, so dout[:, 3:] = fl32(g + gD) bit for bit, gD is the fp32
    statement bit for bit, and two runs are bitwise equal.  All-zero mask (any flow): dout is the direct term bit for bit."""
    for mkind in ('random', 'ones'):
        for squared in (False, True):
            inp = ax.lb_inputs(shape, 'zero', mkind)
            g32, gD32 = ax.lb_direct32(inp, squared)
            dout, gD = _lb_run(ops, inp, squared)
            name = f'loss_backward known answer {shape} {mkind} {"l2" if squared else "l1"}'
            _bitwise(f'{name} gD', gD, gD32)
            _bitwise(f'{name} dout[:, 3:] vs fl32(g + gD)', dout[:, 3:], g32[:, 3:] + gD32)
            again, _ = _lb_run(ops, inp, squared)
            _bitwise(f'{name} second run', again, dout)
    for kind in ('frac', 'fold'):
        for squared in (False, True):
            inp = ax.lb_inputs(shape, kind, 'zeros')
            g32, _ = ax.lb_direct32(inp, squared)
            dout, gD = _lb_run(ops, inp, squared)
            _bitwise(f'loss_backward {shape} {kind} mask 0 {"l2" if squared else "l1"}: dout vs the direct term', dout, g32)
            assert not gD.any()


def test_loss_backward_l1_exact_zeros(ops):
    """every 7th element of target is out's and every 5th of warped is out[:, :3]'s: the direct term is exactly 0 at the
    first set (seen under a zero mask, where dout is the direct term) and gD exactly 0 at the second"""
    for shape in ((2, 9, 29), (3, 16, 16)):
        inp = ax.lb_inputs(shape, 'frac', 'zeros', plant_zeros=True)
        dout, _ = _lb_run(ops, inp, False)
        n1 = int(dout.view(-1)[::7].count_nonzero())
        inp = ax.lb_inputs(shape, 'frac', 'ones', plant_zeros=True)
        dout, gD = _lb_run(ops, inp, False)
        n2 = int(gD.view(-1)[::5].count_nonzero())
        both = (inp['out'] == inp['target'])[:, :3] & (inp['warped'] == inp['out'][:, :3])
        n3 = int(dout[:, :3][both].count_nonzero())
        print(f'[parity] loss_backward l1 {shape}: {n1} planted direct terms and {n2} planted gD not exactly 0, {n3} of '
              f'{int(both.sum())} elements planted in both; allowed 0')
        assert n1 == 0 and n2 == 0 and n3 == 0 and int(both.sum()) > 0
        assert int(gD.count_nonzero()) > gD.numel() // 2
        r = ax.lb_reference(shape, 'frac', 'ones', False, True)
        for half, sl in (('dout[:, :3]', slice(0, 3)), ('dout[:, 3:]', slice(3, 6))):
            ax.check(f'loss_backward l1 planted zeros {shape} {half}', dout[:, sl], r['ref64']['dout'][:, sl],
                     r['ref32']['dout'][:, sl])


# ------------------------------------------------------------------ 2. dmh_loss_backward_ddp
def _ddp_run(ops, inp, squared, scale):
    B, per = inp['out'].shape
    d = {k: _d(v) for k, v in inp.items()}
    buf, dout = _poisoned((B, per))
    ops.call('dmh_loss_backward_ddp', ops.ptr(d['out']), ops.ptr(d['target']), ops.ptr(d['w']), ops.ptr(dout), B, per,
             int(squared), float(scale))
    torch.cuda.synchronize()
    assert _guards_untouched(buf), 'dmh_loss_backward_ddp wrote outside dout'
    _unchanged('dmh_loss_backward_ddp', {k: (d[k], inp[k]) for k in inp})
    return dout.cpu()


@pytest.mark.parametrize('B,per', ax.DDP_CASES)
def test_loss_backward_ddp_bitwise(ops, B, per):
    """products only: bit for bit the fp32 statement n = (scale * w_b) * inv, dout = (2 d) n or +-n, with exact zeros where
    out == target"""
    inp = ax.ddp_inputs(B, per)
    for squared in (False, True):
        for scale in ax.DDP_SCALES:
            got = _ddp_run(ops, inp, squared, scale)
            _bitwise(f'loss_backward_ddp B={B} per={per} {"l2" if squared else "l1"} scale={scale}', got,
                     ax.ddp_statement32(inp, squared, scale))
            assert not got.view(-1)[::7].any()


def test_loss_backward_ddp_grid_stride(ops):
    """B = 2, per = 8192 * 128 + 3: the block cap is reached and the first six threads take a second trip.  Bitwise as above;
    under L1 every element is +-n of its row, so the row index i / per is read off on both sides of the row boundary and of
    the 8192-block boundary"""
    B, per = ax.DDP_LOOP_CASE
    inp = ax.ddp_inputs(B, per)
    for squared in (True, False):
        got = _ddp_run(ops, inp, squared, 0.25)
        want = ax.ddp_statement32(inp, squared, 0.25)
        _bitwise(f'loss_backward_ddp loop case B={B} per={per} {"l2" if squared else "l1"}', got, want)
    n = want.abs().max(dim=1).values          # L1 (the last pass): |dout| is n_b wherever out != target
    assert n[0] != n[1]
    flat, cap = got.view(-1), ax.DDP_BLOCK_CAP * 256
    for i in (per - 2, per - 1, per, per + 1, cap - 2, cap - 1, cap, cap + 1, cap + 5, B * per - 1):
        row = i // per
        if inp['out'].view(-1)[i] != inp['target'].view(-1)[i]:
            assert flat[i].abs() == n[row], (i, row, flat[i].item(), n.tolist())
    print(f'[parity] loss_backward_ddp loop case: row index right at i = {per - 1} | {per} and {cap - 1} | {cap}')


# ------------------------------------------------------------------ 3. dmh_s2d_shift, dmh_d2s, dmh_sumpool2
LAYOUT = [(B, hw) for B in ax.LAYOUT_B for hw in ax.LAYOUT_HW]


def _layout_run(ops, entry, x, out_shape, B, H, W, Cc):
    xd = _d(x)
    buf, out = _poisoned(out_shape)
    ops.call(entry, ops.ptr(xd), ops.ptr(out), B, H, W, Cc)
    torch.cuda.synchronize()
    assert _guards_untouched(buf), f'{entry} wrote outside its output'
    _unchanged(entry, dict(x=(xd, x)))
    return out.cpu()


@pytest.mark.parametrize('B,hw', LAYOUT, ids=lambda v: str(v).replace(' ', ''))
def test_s2d_shift_bitwise(ops, B, hw):
    """the input holds each element's own flat index; the border taps are written as +0.0, not left as poison"""
    H, W = hw
    for Cc in ax.LAYOUT_C:
        x = ax.iota((B, H, W, Cc)) + 1.0             # (no zero inside: a zero in the output is a border tap)
        want = ax.s2d_shift_ref(x)
        got = _layout_run(ops, 'dmh_s2d_shift', x, want.shape, B, H, W, Cc)
        _bitwise(f's2d_shift B={B} {H}x{W} C={Cc}', got, want)
        assert int((got == 0).sum()) == B * Cc * (2 * (H // 2 + 1) * 2 + 2 * (W // 2 + 1) * 2 - 4)


@pytest.mark.parametrize('B,hw', LAYOUT, ids=lambda v: str(v).replace(' ', ''))
def test_d2s_bitwise(ops, B, hw):
    H, W = hw
    for Cc in ax.LAYOUT_C:
        a = ax.iota((B, H, W, 4 * Cc))
        want = ax.d2s_ref(a)
        _bitwise(f'd2s B={B} {H}x{W} C={Cc}', _layout_run(ops, 'dmh_d2s', a, want.shape, B, H, W, Cc), want)


@pytest.mark.parametrize('B,hw', LAYOUT, ids=lambda v: str(v).replace(' ', ''))
def test_sumpool2_bitwise(ops, B, hw):
    """random data against (a + b) + (c + d) in fp32 torch, and the index-valued input (every sum exact) for the placement"""
    H, W = hw
    for Cc in ax.LAYOUT_C:
        for name, a in (('random', rand((B, 2 * H, 2 * W, Cc), 7400 + H + Cc)), ('index', ax.iota((B, 2 * H, 2 * W, Cc)))):
            want = ax.sumpool2_ref(a)
            _bitwise(f'sumpool2 B={B} {H}x{W} C={Cc} {name}', _layout_run(ops, 'dmh_sumpool2', a, want.shape, B, H, W, Cc), want)


def test_layout_refusals(ops):
    """odd H or W for dmh_s2d_shift, C % 4 != 0 for all three: refused before anything is launched"""
    from dmhomo_amd._lib import DmhError
    x = torch.zeros(4096, device=dev())
    buf, out = _poisoned((4096,))
    for entry, args in (('dmh_s2d_shift', (1, 3, 4, 4)), ('dmh_s2d_shift', (1, 4, 5, 4)), ('dmh_s2d_shift', (1, 4, 4, 6)),
                        ('dmh_d2s', (1, 4, 4, 6)), ('dmh_sumpool2', (1, 4, 4, 2))):
        with pytest.raises(DmhError):
            ops.call(entry, ops.ptr(x), ops.ptr(out), *args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------ 4. dmh_resize_bilinear_u8, dmh_mask_open_nearest
def _plane_ptr(batch, plane):
    B, P, Hd, Wd = batch.shape
    return C.c_void_p(batch.data_ptr() + plane * Hd * Wd * 4)


def _planes_check(name, buf, batch, lo, hi):
    assert _guards_untouched(buf), f'{name} wrote outside the batch'
    other = torch.cat([batch[:, :lo], batch[:, hi:]], 1)
    assert bool(torch.isnan(other).all()), f'{name} wrote to a plane that is not its own'


_size_id = lambda s: f'{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}'


@pytest.mark.parametrize('sizes', ax.RESIZE_SIZES, ids=_size_id)
def test_resize_bilinear_u8(ops, sizes):
    """planes 2 .. 2 + C of a poisoned (B, 12, Hd, Wd) batch, bit for bit oracle.dataset.resize_linear of src / div (the
    kernel body is compiled with contraction off and mirrors its op order), and within 8 * 2^-24 * (255 / div) of plain
    bilinear interpolation in float64 from the same taps; the other planes stay poison"""
    (hs, ws), (hd, wd) = sizes
    worst = 0.0
    for B in ax.RESIZE_B:
        for Cc in ax.RESIZE_C:
            for div in ax.RESIZE_DIV:
                for kind in (('random', 'zeros', 'full') if (B, div) == (3, 255.0) else ('random',)):
                    src = ax.resize_src(B, hs, ws, Cc, kind)
                    sd = _d(src)
                    buf, batch = _poisoned((B, ax.PLANES, hd, wd))
                    ops.call('dmh_resize_bilinear_u8', ops.ptr(sd, torch.uint8), _plane_ptr(batch, ax.PLANE0), B, hs, ws, Cc, hd,
                             wd, ax.PLANES * hd * wd, float(div))
                    torch.cuda.synchronize()
                    name = f'resize {hs}x{ws}->{hd}x{wd} B={B} C={Cc} div={div:g} {kind}'
                    _planes_check(name, buf, batch, ax.PLANE0, ax.PLANE0 + Cc)
                    assert np.array_equal(sd.cpu().numpy(), src)
                    got = batch[:, ax.PLANE0:ax.PLANE0 + Cc].cpu()
                    _bitwise(name, got, torch.from_numpy(ax.resize_oracle(src, hd, wd, div)))
                    e = np.abs(got.numpy().astype(np.float64) - ax.resize_plain(src, hd, wd, div)).max() / ax.resize_bound(div)
                    worst = max(worst, e)
    print(f'[parity] resize {hs}x{ws}->{hd}x{wd}: worst |err| / bound against float64 interpolation = {worst:.3e}, allowed 1')
    assert worst <= 1.0


@pytest.mark.parametrize('sizes', ax.MASK_SIZES, ids=_size_id)
def test_mask_open_nearest(ops, sizes):
    """plane 6 of a poisoned (B, 12, Hd, Wd) batch, exactly oracle.dataset's resize_nearest -> erode3 -> dilate3 and exactly
    scipy.ndimage's grey opening of the nearest-resized mask, for binary, float, all-ones, single-0, single-1 and 3x3-block
    inputs"""
    (hs, ws), (hd, wd) = sizes
    for B in (1, 3):
        for kind in ax.MASK_KINDS:
            m = ax.mask_src(kind, B, hs, ws)
            md = _d(m)
            buf, batch = _poisoned((B, ax.PLANES, hd, wd))
            ops.call('dmh_mask_open_nearest', ops.ptr(md), _plane_ptr(batch, ax.MASK_PLANE), B, hs, ws, hd, wd,
                     ax.PLANES * hd * wd)
            torch.cuda.synchronize()
            name = f'mask_open {hs}x{ws}->{hd}x{wd} B={B} {kind}'
            _planes_check(name, buf, batch, ax.MASK_PLANE, ax.MASK_PLANE + 1)
            assert np.array_equal(md.cpu().numpy(), m)
            got = batch[:, ax.MASK_PLANE].cpu()
            _bitwise(name + ' vs oracle', got, torch.from_numpy(ax.mask_oracle(m, hd, wd)))
            _bitwise(name + ' vs scipy', got, torch.from_numpy(ax.mask_scipy(m, hd, wd)))
            if kind == 'ones':
                assert bool((got == 1).all())


# ------------------------------------------------------------------ 5. geometry helpers
@pytest.mark.parametrize('shape', ax.GRID_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pixel_grid_and_norm_grid_bitwise(ops, shape):
    """dmh_pixel_grid against arange + start and dmh_norm_grid against 2.0 * v / (W - 1) - 1.0, fp32 torch, bit for bit; at
    H = 1 or W = 1 the division by zero gives what torch gives (NaN where torch has NaN, the same bits elsewhere)"""
    B, H, W = shape
    for start in ax.GRID_STARTS:
        buf, out = _poisoned((B, 2, H, W))
        ops.call('dmh_pixel_grid', ops.ptr(out), B, H, W, float(start))
        torch.cuda.synchronize()
        assert _guards_untouched(buf)
        _bitwise(f'pixel_grid {shape} start={start}', out, ax.pixel_grid_ref(B, H, W, start))
    v = rand((B, 2, H, W), 7850 + H) * 10.0
    v[0, :, 0, 0] = 0.0                                      # 0 / 0 where the axis has one pixel
    vd = _d(v)
    buf, out = _poisoned((B, H, W, 2))
    out.fill_(123.0)                                         # (NaN is a legitimate output here: poison the interior otherwise)
    ops.call('dmh_norm_grid', ops.ptr(vd), ops.ptr(out), B, H, W)
    torch.cuda.synchronize()
    assert _guards_untouched(buf) and torch.equal(vd.cpu(), v)
    want, got = ax.norm_grid_ref(v), out.cpu()
    assert not bool((got == 123.0).any())
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and (bool(nan.any()) == (H == 1 or W == 1))
    _bitwise(f'norm_grid {shape}', torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))


@pytest.mark.parametrize('case', ax.FLOW_POINTS_CASES, ids=lambda c: 'B{}d{}Bi{}-{}x{}'.format(*c))
def test_homography_flow_points(ops, case):
    """get_flow_np on points that are no pixel grid (third coordinate != 1), band by band, against the numpy float64
    formula within 1e-12 absolute (the bar of tests/test_gpu_surface.py)"""
    B, divide, Bi, H, W = case
    Hm, idx = ax.flow_points_inputs(case)
    hd, idd = _d(Hm), _d(idx)
    buf, out = _poisoned((B, 2, H, W), torch.float64)
    ops.call('dmh_homography_flow_points', ops.ptr(hd, torch.float64), ops.ptr(idd, torch.float64), ops.ptr(out, torch.float64),
             B, divide, Bi, H, W)
    torch.cuda.synchronize()
    assert _guards_untouched(buf) and np.array_equal(hd.cpu().numpy(), Hm) and np.array_equal(idd.cpu().numpy(), idx)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - ax.flow_points_ref(Hm, idx)).max()
    print(f'[parity] homography_flow_points {case}: max_abs={err:.3e}, allowed 1e-12')
    assert err <= 1e-12


def _homography_flow(ops, Hm, H, W, max_flow, want_flow=True, want_rgb=True):
    B = Hm.shape[0]
    hd = _d(Hm)
    fbuf, flow = _poisoned((B, 2, H, W))
    rbuf, rgb = _poisoned((B, 3, H, W))
    ops.call('dmh_homography_flow', ops.ptr(hd, torch.float64), ops.ptr(flow if want_flow else None),
             ops.ptr(rgb if want_rgb else None), B, H, W, float(max_flow))
    torch.cuda.synchronize()
    assert _guards_untouched(fbuf) and _guards_untouched(rbuf) and np.array_equal(hd.cpu().numpy(), Hm)
    assert want_flow or bool(torch.isnan(flow).all())
    assert want_rgb or bool(torch.isnan(rgb).all())
    return flow, rgb


def _flow_to_image(ops, flow, max_flow):
    B, _, H, W = flow.shape
    buf, rgb = _poisoned((B, 3, H, W))
    before = flow.clone()
    ops.call('dmh_flow_to_image', ops.ptr(flow), ops.ptr(rgb), B, H * W, float(max_flow))
    torch.cuda.synchronize()
    assert _guards_untouched(buf) and torch.equal(_bits(flow), _bits(before))
    return rgb


@pytest.mark.parametrize('shape', ax.HFLOW_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_homography_flow(ops, shape):
    """the flow half is the points kernel on the integer grid rounded to fp32 (held to one fp32 ulp, against the kernel and
    against the numpy statement); the rgb half is oracle.geometry.flow_to_image of that flow within 2e-5 and bit for bit
    dmh_flow_to_image on it (they share flow_pixel_to_rgb); either output alone leaves the other untouched"""
    B, H, W = shape
    Hm = ax.homographies((B,), 7950 + H)
    Hm[0] = np.eye(3) + np.array([[0, 0, 2.5], [0, 0, 0], [0, 0, 0.]])              # a translation along x
    grid = ax.int_grid(H, W)
    buf, pts = _poisoned((B, 2, H, W), torch.float64)
    hd, gd = _d(Hm[:, None]), _d(grid)           # (held: a temporary would hand its memory to the next allocation before the launch)
    ops.call('dmh_homography_flow_points', ops.ptr(hd, torch.float64), ops.ptr(gd, torch.float64), ops.ptr(pts, torch.float64),
             B, 1, 1, H, W)
    torch.cuda.synchronize()
    assert _guards_untouched(buf)
    ref = torch.from_numpy(ax.flow_points_ref(Hm[:, None], grid))
    for mf in ax.MAX_FLOWS:
        flow, rgb = _homography_flow(ops, Hm, H, W, mf)
        for name, r64 in (('the points kernel', pts.cpu()), ('the numpy statement', ref)):
            ulps = ((flow.cpu().double() - r64.float().double()).abs() / ax.ulp32_spacing(r64)).max().item()
            nb = int((_bits(flow.cpu()) != _bits(r64.float())).sum())
            print(f'[parity] homography_flow {shape} flow vs {name} rounded to fp32: {ulps:.2f} ulp, {nb} of {flow.numel()} '
                  f'differ bitwise; allowed 1 ulp')
            assert ulps <= 1.0
        err = np.abs(rgb.cpu().numpy() - ax.flow_image_oracle(flow.cpu().numpy(), mf)).max()
        print(f'[parity] homography_flow {shape} max_flow={mf:g} rgb vs the oracle: max_abs={err:.3e}, allowed 2e-5')
        assert err <= 2e-5
        _bitwise(f'flow_to_image vs the rgb half of homography_flow {shape} max_flow={mf:g}', _flow_to_image(ops, flow, mf), rgb)
        f_only, _ = _homography_flow(ops, Hm, H, W, mf, want_rgb=False)
        _, r_only = _homography_flow(ops, Hm, H, W, mf, want_flow=False)
        _bitwise(f'homography_flow {shape} flow alone', f_only, flow)
        _bitwise(f'homography_flow {shape} rgb alone', r_only, rgb)


@pytest.mark.parametrize('max_flow', ax.MAX_FLOWS)
def test_flow_to_image_edge_field(ops, max_flow):
    """zero flow with every sign of zero, flows along +-x and +-y (v = -0.0 included: the hue sector boundaries), the
    diagonals, magnitudes at max_flow / 8 exactly, one step below and 1e6 above (the saturation clamp) and 1e-30, against
    oracle.geometry.flow_to_image within 2e-5; the second image holds the field in reverse order (the batch stride)"""
    fl = ax.edge_flows(max_flow)
    n = fl.shape[0]
    flow = np.stack([fl.T.reshape(2, 1, n), fl[::-1].T.reshape(2, 1, n)]).astype(np.float32)
    rgb = _flow_to_image(ops, _d(flow), max_flow).cpu().numpy()
    assert np.isfinite(rgb).all()
    want = ax.flow_image_oracle(flow, max_flow)
    err = np.abs(rgb - want)
    i = np.unravel_index(err.argmax(), err.shape)
    print(f'[parity] flow_to_image edge field max_flow={max_flow:g}: max_abs={err.max():.3e} at flow '
          f'{flow[i[0], :, 0, i[3]].tolist()}, allowed 2e-5')
    assert err.max() <= 2e-5
    assert np.array_equal(rgb[0, :, 0, :4], np.ones((3, 4), np.float32))              # zero flow: grey 1 exactly
    assert np.array_equal(rgb[0], rgb[1][:, :, ::-1])


# ------------------------------------------------------------------ 6. single-tensor optimiser entries
def _table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _norm_clip(ops, g, max_norm):
    """dmh_sumsq + dmh_gradnorm_finalize into poisoned buffers -> the (2,) device tensor [norm, coefficient]"""
    nb = ops.sumsq_blocks()
    pbuf, part = _poisoned((nb,), torch.float64)
    cbuf, clip = _poisoned((2,))
    ops.call('dmh_sumsq', ops.ptr(g), g.numel(), ops.ptr(part, torch.float64))
    ops.call('dmh_gradnorm_finalize', ops.ptr(part, torch.float64), nb, float(max_norm), ops.ptr(clip))
    torch.cuda.synchronize()
    assert _guards_untouched(pbuf) and _guards_untouched(cbuf) and bool(torch.isfinite(part).all())
    return clip


OPT_CASES = [(n, mx) for n in ax.OPT_SIZES for mx in [None] + ax.OPT_MAX_NORMS]


@pytest.mark.parametrize('n,max_norm', OPT_CASES, ids=lambda v: str(v))
def test_adam_single_vs_multi_and_fp64(ops, n, max_norm):
    """three steps of dmh_adam with gscale NULL (max_norm None) or the coefficient of dmh_sumsq + dmh_gradnorm_finalize
    (max_norm above and below the norm): the norm and the coefficient, and those of dmh_sumsq_multi on the same tensor,
    within 1.5e-7 of float64, p, m, v bit for bit
    dmh_adam_multi on the same tensor, and within the ulp bars of test_clip_adam_multi_vs_fp64 of the float64 Adam step"""
    p0, grads = ax.opt_tensors(n)
    bufs = [_poisoned((n,)) for _ in range(3)]
    P, M, V = (b[1] for b in bufs)
    P.copy_(p0)
    M.zero_()
    V.zero_()
    P2, M2, V2 = _d(p0), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    sizes = (C.c_int64 * 1)(n)
    h = ax.ADAM
    worst = dict(norm=0.0, p=0.0, m=0.0, v=0.0)
    for step, g in enumerate(grads, 1):
        gd = _d(g)
        clip, coef = None, 1.0
        if max_norm is not None:
            clip = _norm_clip(ops, gd, max_norm)
            c = clip.cpu().double()
            nrm, want = ax.norm_coef64(g, max_norm)
            assert (want < 1.0) == (max_norm == ax.OPT_MAX_NORMS[1])
            worst['norm'] = max(worst['norm'], abs(c[0].item() - nrm) / nrm, abs(c[1].item() - want) / want)
            coef = c[1].item()
            nbm = int(ops.lib().dmh_multi_blocks(sizes, 1))           # the multi-tensor sum of squares on the same tensor, alone
            mbuf, partm = _poisoned((nbm,), torch.float64)
            c2buf, clipm = _poisoned((2,))
            ops.call('dmh_sumsq_multi', _table([gd]), sizes, 1, ops.ptr(partm, torch.float64))
            ops.call('dmh_gradnorm_finalize', ops.ptr(partm, torch.float64), nbm, float(max_norm), ops.ptr(clipm))
            cm = clipm.cpu().double()
            assert _guards_untouched(mbuf) and _guards_untouched(c2buf) and nbm == -(-n // 4096)
            worst['norm'] = max(worst['norm'], abs(cm[0].item() - nrm) / nrm, abs(cm[1].item() - want) / want)
        rp, rm, rv = P.cpu().double(), M.cpu().double(), V.cpu().double()          # each step from the kernel's state
        ops.call('dmh_adam', ops.ptr(P), ops.ptr(gd), ops.ptr(M), ops.ptr(V), ops.ptr(clip), n, h['lr'], h['b1'], h['b2'],
                 h['eps'], step)
        ops.call('dmh_adam_multi', _table([P2]), _table([gd]), _table([M2]), _table([V2]), sizes, 1, ops.ptr(clip), h['lr'],
                 h['b1'], h['b2'], h['eps'], step)
        torch.cuda.synchronize()
        assert all(_guards_untouched(b[0]) for b in bufs) and torch.equal(gd.cpu(), g)
        for name, a, b in (('p', P, P2), ('m', M, M2), ('v', V, V2)):
            _bitwise(f'adam n={n} max_norm={max_norm} step {step} {name}: dmh_adam vs dmh_adam_multi', a, b)
        (wp, wm, wv), (sp, sm, sv) = ax.adam_step64(rp, rm, rv, g, coef, step, **h)
        for key, got, want, sc in (('p', P, wp, sp), ('m', M, wm, sm), ('v', V, wv, sv)):
            worst[key] = max(worst[key], ((got.cpu().double() - want).abs() / ax.ulp32_spacing(sc)).max().item())
    print(f'[parity] adam n={n} max_norm={max_norm}: norm/coef rel={worst["norm"]:.2e}, ulps p={worst["p"]:.2f} '
          f'm={worst["m"]:.2f} v={worst["v"]:.2f}; allowed {ax.NORM_REL:.1e}, {ax.ADAM_ULPS}')
    assert worst['norm'] <= ax.NORM_REL and all(worst[k] <= ax.ADAM_ULPS[k] for k in 'pmv'), worst


@pytest.mark.parametrize('n', ax.OPT_SIZES)
def test_ema_vs_fp64(ops, n):
    """ema + (1 - decay) (p - ema) in float64 within 2 ulp of max(|ema|, |p|); p unchanged"""
    for decay in ax.EMA_DECAYS:
        e0, p = rand((n,), 8100 + n % 97), rand((n,), 8101 + n % 97)
        buf, ema = _poisoned((n,))
        ema.copy_(e0)
        pd = _d(p)
        ops.call('dmh_ema', ops.ptr(ema), ops.ptr(pd), n, float(decay))
        torch.cuda.synchronize()
        assert _guards_untouched(buf) and torch.equal(pd.cpu(), p)
        ulps = ((ema.cpu().double() - ax.ema_ref64(e0, p, decay)).abs() /
                ax.ulp32_spacing(torch.maximum(e0.abs(), p.abs()).double())).max().item()
        print(f'[parity] ema n={n} decay={decay}: {ulps:.2f} ulp of max(|ema|, |p|), allowed {ax.EMA_ULPS}')
        assert ulps <= ax.EMA_ULPS
