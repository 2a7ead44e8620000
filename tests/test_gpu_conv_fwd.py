"""-m gpu: every kernel instance behind dmh_conv2d (csrc/conv.hip, csrc/conv_f16x3.hip) alone — the eleven instantiations of
conv_f16x3_kernel and the two of conv_igemm_kernel — against the float64 references of tests/conv_fwd_cases.py, PER OUTPUT
CHANNEL: err_c <= max(FLOOR, 10 * e32_c) (tests/test_conv_fwd_host.py holds every e32_c under CAP), and
every GroupNorm stat tile against the float64 sums of its own valid pixels (`stat_reference`).

Every launch goes through `launch` below: `out` and `stats` are interior slices of NaN-filled buffers, so an element or a
stat tile the kernel does not write fails the gate, the guard bands on both sides must stay bitwise NaN, and the inputs
bitwise what they were.  Known answers (zero input, a zero output channel, one-tap weights on fp16-representable data) and
row subsets are held bit for bit.  Under DMH_CONV3_VARIANT = 0 / 6 (a child process per variant) the instance table
collapses onto the exact-fp32 kernels: the unit-kind cases, the known answers and the row subsets run there with the same
gates, and what needs the fp16-piece kernels skips."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import conv_fwd_cases as cf
from gpu_util import dev

pytestmark = pytest.mark.gpu

GUARD = 4096                                   # floats of NaN before and after `out` and `stats`
NAN_BITS = 0x7fc00000


@pytest.fixture(scope='module')
def ops():
    from dmhomo_amd import ops as _ops
    _ops.lib()
    return _ops


def _d(t):
    return None if t is None else t.contiguous().to(dev())


def _nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(dev())


def _bits(t):
    return t.view(torch.int32)


def _poisoned(n):
    """-> (whole buffer, interior view of n floats)"""
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=dev())
    assert int(_bits(buf)[0]) == NAN_BITS
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf):
    b = _bits(buf)
    return bool((b[:GUARD] == NAN_BITS).all()) and bool((b[-GUARD:] == NAN_BITS).all())


def stat_th(ops, ho, wo, k, s):
    """height of a stat tile, from what dmh_conv_tiles implies (16 columns wide always)"""
    tiles, tx = ops.lib().dmh_conv_tiles(ho, wo, k, s), -(-wo // 16)
    assert tiles > 0 and tiles % tx == 0
    th = 8 if tiles // tx == -(-ho // 8) else 16
    assert tiles // tx == -(-ho // th)
    return th, tiles


def launch(ops, pc, x0, x1=None, in_coef=None, res=None, res_coef=None, want_stats=False, in_bound=None, rows=None,
           upsample2=None, force_src1=None):
    """dmh_conv2d as ops.conv2d drives it, into caller-owned poisoned buffers -> (out (B, Ho, Wo, Cout), stats or None).
    upsample2 / force_src1: a DmhConv the wrapper would not build (the refusals)"""
    B, H, W, _ = x0.shape
    ho, wo = ops.conv_out_hw(pc, H, W)
    obuf, oflat = _poisoned(B * ho * wo * pc.cout)
    out = oflat.view(B, ho, wo, pc.cout)
    sbuf = stats = None
    if want_stats:
        _, tiles = stat_th(ops, ho, wo, pc.k, pc.stride)
        sbuf, sflat = _poisoned(B * tiles * pc.cout * 2)
        stats = sflat.view(B, tiles, pc.cout, 2)
    src1 = x1 if force_src1 is None else force_src1
    ins = [t for t in (x0, src1, in_coef, res, res_coef, in_bound, pc.wpack, pc.bias) if t is not None]
    before = [_bits(t).clone() for t in ins]
    ptr = ops.ptr
    d = ops._lib.DmhConv(C.sizeof(ops._lib.DmhConv), ptr(x0), ptr(src1), ptr(pc.wpack), ptr(pc.bias), ptr(in_coef), ptr(res),
                         ptr(res_coef), ptr(out), ptr(stats), B, H, W, pc.c0, pc.c1 if force_src1 is None else force_src1.shape[3],
                         pc.cout, pc.k, pc.k, pc.stride, pc.upsample2 if upsample2 is None else upsample2,
                         ptr(in_bound), 0 if in_bound is None else in_bound.shape[1], 0, None, None, None, None, 1e-5,
                         None if rows is None else ptr(rows, torch.int32))
    ops.call('dmh_conv2d', C.byref(d))
    torch.cuda.synchronize()
    assert _guards_untouched(obuf), 'the guard bands of out were written'
    assert sbuf is None or _guards_untouched(sbuf), 'the guard bands of stats were written'
    for t, b in zip(ins, before):
        assert torch.equal(_bits(t), b), 'an input was written'
    return out, stats


def packed(ops, inst, w, bias, C0, C1):
    d = cf.INSTANCES[inst]
    pc = ops.PackedConv(_d(w), _d(bias), C0, C1, d['s'], d['ups'], subpixel=d['sub'])
    if ops.f16x3_default():
        assert (pc.upsample2 == 2) == (inst == 'up2'), (inst, pc.upsample2)
    return pc


def _skip_outside_default(ops, case):
    """under DMH_CONV3_VARIANT 0 / 6 (the child runs of test_exact_fp32_variants_in_child_process): the dynamic-range kinds
    belong to the fp16-piece kernels, and up2 / in_bound exist only there"""
    if ops.f16x3_default():
        return
    o = cf.opt_set(case)
    if case[8] != 'unit' or case[0] == 'up2' or 'inbound' in o or 'inboundinf' in o:
        pytest.skip('needs the fp16-piece kernels (DMH_CONV3_VARIANT unset)')


def run_case(ops, case, r):
    """launch the case, hold every output channel and every stat tile to its gate, print the [parity] lines"""
    inst, B, H, W, C0, C1, Cout, _, kind = case
    d, o, inp = cf.INSTANCES[inst], cf.opt_set(case), r['inp']
    name = cf.case_id(case)
    pc = packed(ops, inst, inp['w'], inp['bias'], C0, C1)
    x0, coef = _nhwc(inp['x0']), _d(inp['in_coef'])
    bound = None
    if 'inboundinf' in o:
        bound = torch.full((B, cf.PRO_GROUPS), float('inf'), device=dev())
    elif 'inbound' in o:      # as a producing conv would hand them over: one 'tile' holding the whole sample
        st = torch.stack([x0.sum((1, 2)), (x0 * x0).sum((1, 2))], -1).reshape(B, 1, C0, 2).contiguous()
        _, bound = ops.gn_finalize(st, _d(inp['gamma']), _d(inp['beta']), H * W, cf.PRO_GROUPS, want_bound=True)
        c64 = inp['in_coef'].double()
        z = (c64[:, 0, :, None, None] * inp['x0'].double() + c64[:, 1, :, None, None]).abs()
        zmax = z.reshape(B, cf.PRO_GROUPS, -1).amax(2)
        assert bool((bound.double().cpu() >= zmax).all()), (name, bound, zmax)
        assert bool(torch.isinf(bound).all()) == (kind == 'pro-offset'), (name, bound)
    out, stats = launch(ops, pc, x0, _nhwc(inp['x1']), coef, _nhwc(inp['res']), _d(inp['res_coef']), 'stats' in o, bound)
    got = out.permute(0, 3, 1, 2).cpu()
    assert bool(torch.isfinite(got).all()), f'{name}: {int((~torch.isfinite(got)).sum())} outputs not finite (never written?)'
    err = cf.chan_rel(got, r['ref64'])
    ratio = err / r['gate']
    c = int(ratio.argmax())
    print(f'[parity] conv_fwd {name}: worst err_c/gate_c={ratio[c].item():.3f} at channel {c}: err={err[c].item():.3e} '
          f'e32={r["e32"][c].item():.3e} gate={r["gate"][c].item():.3e}; worst e32_c={r["e32"].max().item():.3e}')
    assert bool((err <= r['gate']).all()), f'{name}: channel {c}: error {err[c].item():.3e} over its gate {r["gate"][c].item():.3e}'
    if stats is not None:
        th, _ = stat_th(ops, got.shape[2], got.shape[3], d['k'], d['s'])
        ref, bnd = cf.stat_reference(r['ref64'], r['gate'], th)
        gs = stats.cpu().double()
        assert gs.shape == ref.shape and bool(torch.isfinite(gs).all()), f'{name}: a stat tile was never written'
        sr = ((gs - ref).abs() / bnd.clamp_min(1e-300)).amax((0, 2))          # (tiles, 2)
        print(f'[parity] conv_fwd {name} stat tiles ({th}x16, {ref.shape[1]} per sample): worst |d sum|/bound='
              f'{sr[:, 0].max().item():.3f} (tile {int(sr[:, 0].argmax())}) |d sumsq|/bound={sr[:, 1].max().item():.3f} '
              f'(tile {int(sr[:, 1].argmax())})')
        assert bool(((gs - ref).abs() <= bnd).all()), f'{name}: stat tile off its bound'
    return got, stats


# ------------------------------------------------------------------ every case against float64
@pytest.mark.parametrize('case', cf.CASES, ids=cf.case_id)
def test_conv_fwd(ops, case):
    _skip_outside_default(ops, case)
    run_case(ops, case, cf.conv_reference(case))


def test_conv3x3_packpw_limit_nonzero(ops):
    """Win = 3853 with random data: the second tile row's packed 16-bit source offset reaches 17 * Win + 17 = 65518"""
    r = cf.packpw_reference()
    run_case(ops, cf.PACKPW_CASE, r)


# ------------------------------------------------------------------ known answers, bitwise
def _pow2_bias(Cout):
    return 2.0 ** (torch.arange(Cout) % 5 - 2).float() * (1 - 2 * (torch.arange(Cout) % 2)).float()


@pytest.mark.parametrize('inst', list(cf.INSTANCES))
def test_zero_input_gives_bias(ops, inst):
    """all-zero input, no prologue: out == bias exactly and every stat tile is exactly (n bias, n bias^2) (powers of two);
    with a residual out == bias + res in fp32"""
    if inst == 'up2' and not ops.f16x3_default():
        pytest.skip('needs the fp16-piece kernels (DMH_CONV3_VARIANT unset)')
    d = cf.INSTANCES[inst]
    C0, C1, Cout = cf.base_channels(inst)
    H, W = cf.geometries(inst)['tile1']
    B = 2
    bias = _pow2_bias(Cout)
    w = cf.rand((Cout, C0, d['k'], d['k']), 77, 0.1)
    pc = packed(ops, inst, w, bias, C0, 0)
    x0 = torch.zeros((B, H, W, C0), device=dev())
    ws = inst not in cf.NO_STATS
    out, stats = launch(ops, pc, x0, want_stats=ws)
    ho, wo = out.shape[1:3]
    assert torch.equal(out.cpu(), bias.expand(B, ho, wo, Cout)), inst
    if ws:
        th, _ = stat_th(ops, ho, wo, d['k'], d['s'])
        ones = torch.ones((B, Cout, ho, wo), dtype=torch.float64)
        n = cf.stat_reference(ones, torch.zeros(Cout, dtype=torch.float64), th)[0][..., 0]        # valid pixels per tile
        want = torch.stack([n * bias.double(), n * bias.double() ** 2], -1)
        assert torch.equal(stats.cpu().double(), want), inst
    res = cf.rand((B, ho, wo, Cout), 78)
    out, _ = launch(ops, pc, x0, res=res.to(dev()))
    assert torch.equal(out.cpu(), bias + res), inst
    print(f'[parity] conv_fwd {inst} zero input {B}x{H}x{W}: out == bias, stat tiles == n*bias, out == bias + res: bitwise')


@pytest.mark.parametrize('inst', list(cf.INSTANCES))
def test_zero_output_channel_is_bias(ops, inst):
    """an all-zero output channel among non-zero ones (its weight scale has nothing to normalise) equals bias[c] exactly"""
    if inst == 'up2' and not ops.f16x3_default():
        pytest.skip('needs the fp16-piece kernels (DMH_CONV3_VARIANT unset)')
    d = cf.INSTANCES[inst]
    C0, C1, Cout = cf.base_channels(inst)
    H, W = cf.geometries(inst)['tile1']
    w = cf.rand((Cout, C0, d['k'], d['k']), 79, 0.1)
    zc = [1, Cout - 2]
    w[zc] = 0
    bias = cf.rand((Cout,), 80)
    pc = packed(ops, inst, w, bias, C0, 0)
    out, _ = launch(ops, pc, cf.rand((2, H, W, C0), 81).to(dev()))
    got = out.cpu()
    for c in zc:
        assert bool((got[..., c] == bias[c]).all()), (inst, c)
    assert bool((got[..., 0] != bias[0]).any())
    print(f'[parity] conv_fwd {inst} zero output channels {zc}: == bias bitwise')


@pytest.mark.parametrize('inst', cf.PROBE_INSTANCES)
def test_tap_probes(ops, inst):
    """a single 1.0 at tap (ky, kx), o == c, on fp16-representable data: the output is the (upsampled) input shifted with zero
    padding, bit for bit — tap order, halo addressing, the column-major tap walk, the tap pairs of UPS = 4 and the parity
    re-indexing of UPS = 2 / 3, with no gate in between"""
    if inst == 'up2' and not ops.f16x3_default():
        pytest.skip('needs the fp16-piece kernels (DMH_CONV3_VARIANT unset)')
    k, Cc = cf.INSTANCES[inst]['k'], cf.probe_channels(inst)
    x = cf.probe_input(inst)
    x0 = _nhwc(x)
    bad = []
    for ky in range(k):
        for kx in range(k):
            pc = packed(ops, inst, cf.probe_weight(inst, ky, kx), None, Cc, 0)
            out, _ = launch(ops, pc, x0)
            want = cf.probe_expected(inst, x, ky, kx)
            if not torch.equal(out.permute(0, 3, 1, 2).cpu(), want):
                bad.append((ky, kx))
    print(f'[parity] conv_fwd {inst} tap probes at {tuple(x.shape)}: {k * k - len(bad)} of {k * k} taps bitwise; wrong: {bad}')
    assert not bad, (inst, bad)


# ------------------------------------------------------------------ row subsets
@pytest.mark.parametrize('inst', list(cf.INSTANCES))
def test_row_subsets_alone(ops, inst):
    """DmhConv.rows at a multi-tile shape, B = 3: the active rows of out and stats are bitwise those of the full launch, the
    inactive rows keep their NaN"""
    if inst == 'up2' and not ops.f16x3_default():
        pytest.skip('needs the fp16-piece kernels (DMH_CONV3_VARIANT unset)')
    case = next(c for c in cf.CASES if c[0] == inst and c[1] == 3 and c[7] == ('rescoef' if inst in cf.NO_STATS else 'rescoef+stats'))
    _, B, H, W, C0, C1, Cout = case[:7]
    inp = cf.conv_reference(case)['inp']
    pc = packed(ops, inst, inp['w'], inp['bias'], C0, C1)
    args = (_nhwc(inp['x0']), None, None, _nhwc(inp['res']), _d(inp['res_coef']), inst not in cf.NO_STATS)
    full, fstats = launch(ops, pc, *args)
    assert bool(torch.isfinite(full).all())
    for subset in ([1], [0, 2], []):
        keep = torch.zeros((B,), dtype=torch.uint8)
        keep[subset] = 1
        rows = ops.rows_from_keep(keep.to(dev()))
        out, stats = launch(ops, pc, *args, rows=rows)
        for b in range(B):
            for got, want in ((out, full), (stats, fstats)):
                if got is None:
                    continue
                if b in subset:
                    assert torch.equal(_bits(got[b]), _bits(want[b])), (inst, subset, b)
                else:
                    assert bool((_bits(got[b]) == NAN_BITS).all()), (inst, subset, b)
    print(f'[parity] conv_fwd {cf.case_id(case)} row subsets [1], [0, 2], []: active rows bitwise, inactive rows NaN')


# ------------------------------------------------------------------ refusals
def test_refusals(ops):
    from dmhomo_amd._lib import DmhError
    z = lambda *s: torch.zeros(s, device=dev())
    w = lambda co, ci, k: cf.rand((co, ci, k, k), 90, 0.1)
    pc = ops.PackedConv(_d(w(8, 8, 3)), None, 4, 4)
    with pytest.raises(DmhError, match='single source'):                 # in_coef with src1
        launch(ops, pc, z(1, 5, 5, 4), z(1, 5, 5, 4), in_coef=z(1, 2, 4))
    pc = ops.PackedConv(_d(w(8, 4, 2)), None, 4, 0, 2)
    for hw in ((5, 4), (4, 5)):
        with pytest.raises(DmhError, match='even input'):                # 2x2 with odd H or W
            launch(ops, pc, z(1, hw[0], hw[1], 4))
    if not ops.f16x3_default():
        return
    pc = ops.PackedConv(_d(w(64, 32, 4)), None, 32, 0, 2)
    with pytest.raises(DmhError, match='no GroupNorm prologue'):         # in_coef on the s2d path
        launch(ops, pc, z(1, 8, 8, 32), in_coef=z(1, 2, 32))
    pc = ops.PackedConv(_d(w(64, 32, 3)), None, 32, 0, 1, 1)
    assert pc.upsample2 == 2
    with pytest.raises(DmhError, match='sub-pixel'):                     # stats on up2
        launch(ops, pc, z(1, 4, 4, 32), want_stats=True)
    with pytest.raises(DmhError, match='sub-pixel'):                     # src1 on up2
        launch(ops, pc, z(1, 4, 4, 32), force_src1=z(1, 4, 4, 4))


# ------------------------------------------------------------------ final / pixel_stats at ragged shapes
@pytest.mark.parametrize('H,W', [(5, 7), (17, 17)])
def test_conv1x1_final_and_pixel_stats_ragged(ops, H, W):
    """test_conv1x1_fused_final_projection (tests/test_gpu_kernels.py) at a ragged sub-tile and at one tile + 1"""
    if not ops.f16x3_default():
        pytest.skip('needs the fp16-piece kernels (DMH_CONV3_VARIANT unset)')
    B, C0, C1, Co, n = 3, 36, 20, 64, 6
    x0, x1 = cf.rand((B, H, W, C0), 40).to(dev()), cf.rand((B, H, W, C1), 41).to(dev())
    pc = ops.PackedConv(cf.rand((Co, C0 + C1, 1, 1), 42, (C0 + C1) ** -0.5).to(dev()), cf.rand((Co,), 43, 0.1).to(dev()), C0, C1)
    res = cf.rand((B, H, W, Co), 44).to(dev())
    rcoef = torch.stack([1 + 0.2 * cf.rand((B, Co), 45), 0.3 * cf.rand((B, Co), 46)], 1).contiguous().to(dev())
    fw, fb = cf.rand((n, Co), 47, Co ** -0.5).to(dev()), cf.rand((n,), 48, 0.2).to(dev())
    out = ops.conv2d(pc, x0, x1, res=res, res_coef=rcoef)
    out2, y = ops.conv2d(pc, x0, x1, res=res, res_coef=rcoef, final=(fw, fb))
    assert torch.equal(out2, out) and torch.equal(y, ops.final_conv_nchw(out, fw, fb))
    none, y2 = ops.conv2d(pc, x0, x1, res=res, res_coef=rcoef, final=(fw, None), keep_out=False)
    assert none is None and torch.equal(y2, ops.final_conv_nchw(out, fw, None))
    out3, pst = ops.conv2d(pc, x0, x1, res=res, res_coef=rcoef, pixel_stats=True)
    want_st = torch.empty((B, H * W, 2), device=dev())
    ops.call('dmh_pixel_stats', ops.ptr(out), ops.ptr(want_st), B * H * W, Co, 1e-5, None, 0)
    assert torch.equal(out3, out) and torch.equal(pst, want_st)
    print(f'[parity] conv_fwd 1x1n final / keep_out=False / pixel_stats at {B}x{H}x{W}: bitwise the separate launches')


# ------------------------------------------------------------------ the exact-fp32 variants
@pytest.mark.parametrize('variant', ['0', '6'])
def test_exact_fp32_variants_in_child_process(variant):
    """DMH_CONV3_VARIANT = 0 (exact-fp32 implicit GEMM) / 6 (exact-fp32 Winograd for the 3x3) is read once per process: this
    file runs again in a fresh child under it — the unit kind, the known answers, the geometry and option matrix and the row
    subsets, with unchanged gates"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DMH_CONV3_VARIANT=variant)
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', '-rs',
                        os.path.abspath(__file__), '-k', 'not child_process'],
                       capture_output=True, text=True, env=env, cwd=root, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
