"""-m gpu: every weight-gradient kernel of csrc/conv_backward.hip alone — conv_wgrad_f16x3_kernel<3,1,2> / <2,0,2> with
conv_wgrad_reduce_v2_kernel, conv_wgrad_kernel<1,4,0> / <7,1,3> / <1,4,0,true> with conv_wgrad_reduce_kernel<false / true> —
through dmh_conv_wgrad and dmh_conv_unshuffle_wgrad, against the float64 references of tests/grad_conv_cases.py, per unit of
each kernel's accuracy contract: err <= max(FLOOR, 10 * e32_unit) (tests/test_grad_conv_host.py holds
every e32_unit under CAP).

Every launch goes through `launch` below: `dw`, `db` and the workspace are interior slices of NaN-filled buffers with guard
bands on both sides (an element never written fails its gate, a guard word written fails the launch), `dw` and `db` start
0-3 floats past a 16-byte boundary (they are written by scalar stores), the workspace has the size the library's own size
function gives, and the inputs are bitwise what they were.  Known answers (one-hot dy, integer dy on fp16-representable
input, zero inputs), workspace contents, repeats and db = NULL are held bit for bit; the composites ops.conv_down_backward,
ops.conv_up_backward and ops.conv_unshuffle_backward are held to float64 autograd at their smallest shapes."""
import zlib

import pytest
import torch

import grad_conv_cases as gc
from gpu_util import dev, nchw, nhwc

pytestmark = pytest.mark.gpu

GUARD = 4096                                   # floats of NaN before and after dw, db and the workspace
NAN_BITS = 0x7fc00000


@pytest.fixture(scope='module')
def ops():
    from dmhomo_amd import ops as _ops
    _ops.lib()
    return _ops


def _d(t):
    return None if t is None else t.contiguous().to(dev())


def _bits(t):
    return t.view(torch.int32)


def _poisoned(n, off=0, fill=float('nan')):
    """-> (whole NaN buffer, interior view of n floats that starts `off` floats past a 16-byte boundary, filled with `fill`)"""
    buf = torch.full((n + 2 * GUARD + 4,), float('nan'), device=dev())
    assert buf.data_ptr() % 16 == 0 and int(_bits(buf)[0]) == NAN_BITS
    view = buf[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == 4 * off
    if fill == fill:
        view.fill_(fill)
    return buf, view, (GUARD + off, GUARD + off + n)


def _guards_untouched(buf, span):
    b = _bits(buf)
    return bool((b[:span[0]] == NAN_BITS).all()) and bool((b[span[1]:] == NAN_BITS).all())


def launch(ops, inst, dy, x0, x1=None, coef=None, ups=0, want_db=True, dw_off=0, db_off=0, work_fill=float('nan'), k=None,
           dims=None):
    """dmh_conv_wgrad / dmh_conv_unshuffle_wgrad (inst 'wu') into caller-owned poisoned buffers -> (dw (Cout, Cin, k, k), db
    or None).  k / dims = (B, H, W, C0, C1, Cout): what the entry is told where it is not what the tensors say (the refusals)"""
    B, H, W, Cout = dy.shape
    C0, C1 = x0.shape[3], 0 if x1 is None else x1.shape[3]
    k = gc.INSTANCES[inst]['k'] if k is None else k
    lib = ops.lib()
    if inst == 'wu':
        cin = 4 * C0
        wsn = lib.dmh_conv_unshuffle_wgrad_workspace_floats(B, x0.shape[1], x0.shape[2], C0, Cout)
    else:
        cin = C0 + C1
        wsn = lib.dmh_conv_wgrad_workspace_floats(B, H, W, C0, C1, Cout, k if k in (1, 2, 3, 7) else 3)
    assert wsn > 0, wsn
    wbuf, dwf, wspan = _poisoned(Cout * cin * k * k, dw_off)
    bbuf, dbf, bspan = _poisoned(Cout, db_off)
    kbuf, work, kspan = _poisoned(wsn, 0, work_fill)
    ins = [t for t in (dy, x0, x1, coef) if t is not None]
    before = [_bits(t).clone() for t in ins]
    ptr = ops.ptr
    if inst == 'wu':
        b_, h_, w_, c_, _, co_ = dims or (B, x0.shape[1], x0.shape[2], C0, 0, Cout)
        ops.call('dmh_conv_unshuffle_wgrad', ptr(dy), ptr(x0), ptr(dwf), ptr(dbf) if want_db else None, ptr(work), b_, h_, w_, c_, co_)
    else:
        b_, h_, w_, c0_, c1_, co_ = dims or (B, H, W, C0, C1, Cout)
        ops.call('dmh_conv_wgrad', ptr(dy), ptr(x0), ptr(x1), ptr(coef), ptr(dwf), ptr(dbf) if want_db else None, ptr(work),
                 b_, h_, w_, c0_, c1_, co_, k, int(ups))
    torch.cuda.synchronize()
    assert _guards_untouched(wbuf, wspan), 'the guard bands of dw were written'
    assert _guards_untouched(bbuf, bspan), 'the guard bands of db were written'
    assert _guards_untouched(kbuf, kspan), 'the guard bands of the workspace were written'
    if not want_db:
        assert bool((_bits(dbf) == NAN_BITS).all()), 'db = NULL, yet the buffer next to it was written'
    for t, b in zip(ins, before):
        assert torch.equal(_bits(t), b), 'an input was written'
    return dwf.view(Cout, cin, k, k), (dbf if want_db else None)


def launch_case(ops, case, inp, **kw):
    inst, mode = case[:2]
    return launch(ops, inst, _d(inp['dy']), _d(inp['x0']), _d(inp['x1']), _d(inp['in_coef']), ups=int(mode == 'ups'), **kw)


def _offsets(case):
    h = zlib.crc32(gc.case_id(case).encode())
    return h % 4, (h >> 2) % 4


# ------------------------------------------------------------------ every case against float64
@pytest.mark.parametrize('case', gc.CASES, ids=gc.case_id)
def test_grad_conv(ops, case):
    r = gc.wgrad_reference(case)
    p = gc.plan(case)
    dw_off, db_off = _offsets(case)
    dw, db = launch_case(ops, case, r['inp'], want_db=case[9], dw_off=dw_off, db_off=db_off)
    dw, db = dw.cpu(), None if db is None else db.cpu()
    f, where = gc.worst(case, r, dw, db)
    e32 = gc.worst_e32(r)
    print(f'[parity] grad_conv {gc.case_id(case)} (grid {p["grid"]}, {p["idle"]} idle, dw +{dw_off} db +{db_off} floats): worst err/gate='
          f'{f:.3f} at {where}; worst e32 ' + ' '.join(f'{u}={e:.3e}' for u, e in e32.items()))
    assert f <= 1.0, f'{gc.case_id(case)}: {where}: {f:.3g} x its gate'


# ------------------------------------------------------------------ known answers, bitwise
def _onehot_cases(inst):
    c0, co = gc.base_channels(inst)
    out = [(inst, 'plain', 2, h, w, c0, 0, co, 'unit', True, 0) for (h, w) in ((1, 1), (5, 17), (9, 33))]
    if inst == 'w3':
        out += [(inst, 'ups', 2, h, w, c0, 0, co, 'unit', True, 0) for (h, w) in ((2, 2), (6, 18))]
    return out


@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_onehot_dy_gives_the_input_window(ops, inst):
    """dy = a single 1.0 at (b, y0, x0, o0) over non-zero fp16-representable input: row o0 of dW is the k x k window of the
    input as the convolution saw it around that pixel, every other row is 0, db is the one-hot — bit for bit"""
    n = bad = 0
    for case in _onehot_cases(inst):
        _, mode, B, H, W, C0, _, Cout = case[:8]
        hin, win = gc.stored_hw(case)
        x = gc.eighths((B, hin, win, C0), 5200 + H)
        xd = _d(x)
        for i, (y0, x0) in enumerate(gc.onehot_positions(H, W)):
            b, o0 = (B - 1, Cout - 1) if i % 2 else (0, 0)
            if (y0, x0) == (3, 15):
                o0 = 63                                      # the last channel of the first 64-tile
            dy = torch.zeros((B, H, W, Cout))
            dy[b, y0, x0, o0] = 1.0
            dw, db = launch(ops, inst, _d(dy), xd, ups=int(mode == 'ups'), dw_off=i % 4, db_off=(i + 1) % 4)
            ok = torch.equal(dw.cpu(), gc.onehot_expected(case, x, b, y0, x0, o0)) and torch.equal(db.cpu(), dy[b, y0, x0])
            n += 1
            bad += not ok
            assert ok, (gc.case_id(case), b, y0, x0, o0)
    print(f'[parity] grad_conv {inst} one-hot dy: {n} launches, {bad} mismatches (bitwise)')


@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_integer_dy_is_exact(ops, inst):
    """integer dy (|d| <= 8) on k/8 input (|k| <= 255): every product and every partial sum is exact in fp32 and in the fp16
    pieces, so db is bitwise the integer sum and dW bitwise the float64 sum, whatever the order of accumulation"""
    c0, co = gc.base_channels(inst)
    n = 0
    for mode, (H, W) in [('plain', (5, 17)), ('plain', (9, 33))] + ([('ups', (6, 18))] if inst == 'w3' else []):
        case = (inst, mode, 3, H, W, c0, 0, co, 'unit', True, 0)
        hin, win = gc.stored_hw(case)
        x = gc.eighths((3, hin, win, c0), 5300 + H)
        dy = torch.randint(-8, 9, (3, H, W, co), generator=torch.Generator().manual_seed(5301 + H)).float()
        dw64, db64 = gc.wgrad_formula(dict(dy=dy, x0=x, x1=None, in_coef=None), case, torch.float64)
        assert dw64.abs().max().item() * 8 < 2 ** 24
        dw, db = launch(ops, inst, _d(dy), _d(x), ups=int(mode == 'ups'), dw_off=1, db_off=3)
        assert torch.equal(db.cpu().double(), db64), gc.case_id(case)
        assert torch.equal(dw.cpu().double(), dw64), gc.case_id(case)
        n += 1
    print(f'[parity] grad_conv {inst} integer dy: db and dW bitwise the exact sums in {n} launches, 0 mismatches')


def _side_cases(inst):
    """the base case at one item + 1, the 27-item geometry, and the smallest channel counts (fp16-piece: Cin <= 32, where the
    second workgroup of a pair returns and the reduce reads a partial slice that nobody wrote)"""
    c0, co = gc.base_channels(inst)
    pick = lambda **kw: next(c for c in gc.CASES if c[0] == inst and c[8] == 'unit' and c[9] and
                             all(c[('inst', 'mode', 'B', 'H', 'W', 'C0', 'C1', 'Cout').index(k)] == v for k, v in kw.items()))
    out = [pick(mode='plain', B=3, H=5, W=17, C0=c0, Cout=co), pick(mode='plain', B=3, H=9, W=33),
           pick(mode='plain', B=3, H=5, W=17, C0=4), pick(mode='plain', B=1, H=1, W=1)]
    if inst == 'w3':
        out += [pick(mode='ups', B=3, H=6, W=18, C0=c0), pick(mode='coef', C0=36), pick(mode='concat', C0=36, C1=20)]
    return out


@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_zero_inputs(ops, inst):
    """dy = 0: dW = 0 and db = 0 exactly; x = 0: dW = 0 exactly and db bitwise what it is with non-zero x"""
    for case in _side_cases(inst):
        inp = gc.wgrad_reference(case)['inp']
        _, db_ref = launch_case(ops, case, inp)
        z = dict(inp, dy=torch.zeros_like(inp['dy']))
        dw, db = launch_case(ops, case, z)
        assert bool((_bits(dw) == 0).all()) and bool((_bits(db) == 0).all()), gc.case_id(case)
        if inp['in_coef'] is not None:          # SiLU(b) of a zero input is not zero: nothing to hold
            continue
        z = dict(inp, x0=torch.zeros_like(inp['x0']), x1=None if inp['x1'] is None else torch.zeros_like(inp['x1']))
        dw, db = launch_case(ops, case, z)
        assert bool((dw == 0).all()), gc.case_id(case)
        assert torch.equal(_bits(db), _bits(db_ref)), gc.case_id(case)
    print(f'[parity] grad_conv {inst} zero dy / zero x at {len(_side_cases(inst))} shapes: exact zeros, db bitwise, 0 mismatches')


@pytest.mark.parametrize('inst', list(gc.INSTANCES))
def test_workspace_contents_repeats_offsets_and_null_db(ops, inst):
    """a workspace prefilled with NaN, with zeros and with 1e30 gives the same bits; so do a second call, every start of dw
    and db 0-3 floats past a 16-byte boundary, and dW of the call with db = NULL"""
    n = 0
    for case in _side_cases(inst):
        inp = gc.wgrad_reference(case)['inp']
        dw0, db0 = launch_case(ops, case, inp)
        assert bool(torch.isfinite(dw0).all()) and bool(torch.isfinite(db0).all()), gc.case_id(case)
        runs = [dict(work_fill=0.0), dict(work_fill=1e30), dict()] + [dict(dw_off=o, db_off=(o + 2) % 4) for o in (1, 2, 3)]
        for kw in runs:
            dw, db = launch_case(ops, case, inp, **kw)
            assert torch.equal(_bits(dw), _bits(dw0)) and torch.equal(_bits(db), _bits(db0)), (gc.case_id(case), kw)
        dw, db = launch_case(ops, case, inp, want_db=False, dw_off=2)
        assert db is None and torch.equal(_bits(dw), _bits(dw0)), gc.case_id(case)
        n += len(runs) + 1
    print(f'[parity] grad_conv {inst} workspace NaN / 0 / 1e30, repeat, output offsets 1-3, db = NULL: {n} launches bitwise '
          f'the first, 0 mismatches')


# ------------------------------------------------------------------ refusals
def test_refusals(ops):
    from dmhomo_amd._lib import DmhError
    z = lambda *s: torch.zeros(s, device=dev())
    with pytest.raises(DmhError, match='bad shape'):                     # C0 % 4
        launch(ops, 'w3', z(1, 4, 4, 8), z(1, 4, 4, 8), dims=(1, 4, 4, 6, 0, 8))
    with pytest.raises(DmhError, match='bad shape'):                     # Cout % 4
        launch(ops, 'w1', z(1, 4, 4, 8), z(1, 4, 4, 8), dims=(1, 4, 4, 8, 0, 6))
    with pytest.raises(DmhError, match='not built'):                     # KH = 5
        launch(ops, 'w3', z(1, 4, 4, 8), z(1, 4, 4, 8), k=5)
    with pytest.raises(DmhError, match='single source'):                 # in_coef with src1
        launch(ops, 'w3', z(1, 4, 4, 8), z(1, 4, 4, 4), z(1, 4, 4, 4), coef=z(1, 2, 4))
    with pytest.raises(DmhError, match='ups needs'):                     # ups with KH != 3
        launch(ops, 'w1', z(1, 4, 4, 8), z(1, 4, 4, 8), ups=1)
    for hw in ((5, 4), (4, 5)):
        with pytest.raises(DmhError, match='ups needs'):                 # ups with an odd size
            launch(ops, 'w3', z(1, hw[0], hw[1], 8), z(1, 4, 4, 8), ups=1)
    with pytest.raises(DmhError, match='bad shape'):                     # the unshuffle entry with an odd H
        launch(ops, 'wu', z(1, 2, 2, 8), z(1, 6, 4, 4), dims=(1, 5, 4, 4, 0, 8))
    with pytest.raises(DmhError, match='bad shape'):                     # ... with C % 4
        launch(ops, 'wu', z(1, 2, 2, 8), z(1, 4, 4, 8), dims=(1, 4, 4, 6, 0, 8))


# ------------------------------------------------------------------ composites at their smallest shapes
@pytest.mark.parametrize('c', gc.COMPOSITES, ids=gc.composite_id)
def test_composite_backward(ops, c):
    """ops.conv_down_backward / conv_up_backward / conv_unshuffle_backward against float64 autograd: dx per input channel, dw
    per output channel, db per channel"""
    r = gc.composite_reference(c)
    inp = r['inp']
    fn = {'down': ops.conv_down_backward, 'up': ops.conv_up_backward, 'unshuffle': ops.conv_unshuffle_backward}[c[0]]
    dx, dw, db = fn(nhwc(inp['dy']), nhwc(inp['x']), _d(inp['w']))
    assert all(bool(torch.isfinite(t).all()) for t in (dx, dw, db)), gc.composite_id(c)
    errs = gc.composite_errors((nchw(dx), dw, db), r['ref64'], r['dysum'])
    line, ok = [], True
    for u, e in errs.items():
        ratio = e / r['gate'][u]
        i = int(ratio.argmax())
        line.append(f'{u} err/gate={ratio[i].item():.3f} (err={e[i].item():.3e} e32={r["e32"][u][i].item():.3e})')
        ok = ok and ratio[i].item() <= 1.0
    print(f'[parity] grad_conv composite {gc.composite_id(c)}: ' + '; '.join(line))
    assert ok, (gc.composite_id(c), line)


def test_conv_down_backward_refuses_an_odd_height(ops):
    from dmhomo_amd._lib import DmhError
    z = lambda *s: torch.zeros(s, device=dev())
    with pytest.raises(DmhError):
        ops.conv_down_backward(z(1, 2, 2, 4), z(1, 5, 4, 4), z(4, 4, 4, 4))
