"""-m gpu: the fp16-piece weight image (csrc/weight_image.h, csrc/conv_f16x3.hip) is ONE thing however it is made.

(a) route equality, device against device, bitwise: the image of a weight made alone (``ops.ws_standardize`` where the case
    standardises, then ``ops.PackedConv`` without a batch) against the one a ``ops.PackBatch`` table makes of it — the whole
    ``wpack`` buffer, per-channel ``oscale`` tail included, and the standardised weight where there is one.
(b) layout pin, host against device, bitwise: the documented element order and the two-plane split restated in numpy, on
    weights for which the host arithmetic is exact.
Nothing here compares by tolerance and no element or case is left out."""
import numpy as np
import pytest
import torch

from gpu_util import dev, rand

pytestmark = pytest.mark.gpu

CASES = [  # (Cout, C0, C1, k)
    (64, 64, 0, 3), (128, 64, 0, 3),
    (72, 48, 0, 3),                      # neither Cout % 64 nor C0 % 32 is zero
    (64, 64, 32, 3), (64, 48, 16, 3),    # fused concat: the second chunk group starts on a (padded) chunk of its own
    (384, 64, 0, 1), (64, 128, 0, 1), (8, 12, 0, 1),
]
MODES = ['plain', 'ws', 'tr', 'ws+tr']   # standardised first (ws) / the data-gradient image (tr: taps flipped, O and I exchanged)


@pytest.fixture(scope='module')
def ops():
    from dmhomo_amd import ops as _ops
    _ops.lib()
    return _ops


def _weight(case, zero=False):
    cout, c0, c1, k = case
    w = rand((cout, c0 + c1, k, k), 300 + CASES.index(case), (1.0 / ((c0 + c1) * k * k)) ** 0.5) + 0.01
    if zero:                             # an all-zero output channel of the plain image (5) and of the transposed one (3)
        w[5] = 0
        w[:, 3] = 0
    return w.to(dev())


_SINGLE = {}


def _single(ops, case, mode, zero=False):
    """(image, standardised weight or None) by the launches of a weight on its own; made once per (case, mode)"""
    key = (case, mode, zero)
    if key not in _SINGLE:
        cout, c0, c1, k = case
        w = _weight(case, zero)
        ws = ops.ws_standardize(w) if 'ws' in mode else None
        src = w if ws is None else ws
        if 'tr' in mode:                 # standardise first, then flip and transpose: conv_dgrad_pack(w1s, ...)
            pc = ops.PackedConv(src.flip(2, 3).transpose(0, 1).contiguous(), None, cout)
        else:
            pc = ops.PackedConv(src, None, c0, c1)
        _SINGLE[key] = (pc.wpack.clone(), ws)
    return _SINGLE[key]


def _register(ops, batch, case, mode, zero=False):
    """the same image as a job (or two) of ``batch``: (PackedConv, standardised-weight buffer or None)"""
    cout, c0, c1, k = case
    w = _weight(case, zero)
    buf = torch.empty_like(w) if 'ws' in mode else None
    if mode == 'plain':
        return ops.PackedConv(w, None, c0, c1, batch=batch), None
    if mode == 'ws':
        return ops.PackedConv(buf, None, c0, c1, batch=batch, ws_from=w), buf
    if mode == 'tr':
        return ops.conv_dgrad_pack(w, c0, batch=batch), None
    ops.PackedConv(buf, None, c0, c1, batch=batch, ws_from=w)          # 'ws+tr', as ResnetBlockTrain.build registers it
    return ops.conv_dgrad_pack(buf, c0, batch=batch), buf


def _check(ops, jobs):
    """jobs: [(case, mode, zero, PackedConv, buf)] of a batch that has run"""
    for case, mode, zero, pc, buf in jobs:
        ref, ws = _single(ops, case, mode, zero)
        assert pc.wpack.shape == ref.shape and torch.equal(pc.wpack, ref), (case, mode)
        if ws is not None:
            assert torch.equal(buf, ws), (case, mode, 'standardised weight')


def _modes(case):
    return MODES if case[2] == 0 else MODES[:2]


@pytest.mark.parametrize('case', CASES, ids=[str(c) for c in CASES])
def test_single_and_table_routes_make_the_same_image(ops, case):
    batch, jobs = ops.PackBatch(), []
    for mode in _modes(case):
        jobs.append((case, mode, False) + _register(ops, batch, case, mode))
    batch.run()
    _check(ops, jobs)


def _planes(wpack, case):
    """image as fp16 [nt][chunk][tap][nh][nb][plane][k group][o & 15][j] + the oscale tail"""
    cout, c0, c1, k = case
    nt, nch = (cout + 63) // 64, (c0 + 31) // 32 + (c1 + 31) // 32
    n = nt * nch * k * k * 2 * 2 * 2 * 64 * 8
    img = wpack.cpu().numpy()
    assert img.size == n // 2 + nt * 64
    return img[:n // 2].view(np.uint16).reshape(nt, nch, k * k, 2, 2, 2, 4, 16, 8), img[n // 2:]


def test_all_zero_channel_has_scale_one_and_zero_planes(ops):
    case = (72, 48, 0, 3)
    batch, jobs = ops.PackBatch(), []
    for mode in ('plain', 'tr'):
        jobs.append((case, mode, True) + _register(ops, batch, case, mode, zero=True))
    batch.run()
    _check(ops, jobs)
    for (_, mode, _, pc, _), (cs, o) in zip(jobs, (((72, 48, 0, 3), 5), ((48, 72, 0, 3), 3))):
        for wpack in (pc.wpack, _single(ops, case, mode, True)[0]):
            planes, osc = _planes(wpack, cs)
            assert osc[o] == 1.0 and osc[o + 1] != 1.0
            assert not planes[0, :, :, 0, 0, :, :, o, :].any()          # (+0.0 everywhere: no sign bit either)


def _mixed(n):
    """n jobs of mixed shapes; standardising and plain jobs alternate, every third one (where C1 == 0) is transposed"""
    out = []
    for i in range(n):
        case = CASES[(i * 3) % len(CASES)]
        mode = ('ws' if i % 2 else 'plain') if (i % 3 or case[2]) else 'tr'
        out.append((case, mode))
    return out


def test_more_jobs_than_one_table_holds(ops):
    """33 jobs = PM_MAX + 1: phases 1 and 2 need a second table, whose block offsets start again at 0"""
    batch, jobs = ops.PackBatch(), []
    for case, mode in _mixed(33):
        jobs.append((case, mode, False) + _register(ops, batch, case, mode))
    assert len(batch.jobs) == 33
    batch.run()
    _check(ops, jobs)


def test_standardising_jobs_interleaved_with_plain_ones(ops):
    """phase 0 skips the jobs that do not standardise: its table is denser than the one of phases 1 and 2"""
    order = [((72, 48, 0, 3), 'plain'), ((64, 48, 16, 3), 'ws'), ((8, 12, 0, 1), 'tr'), ((128, 64, 0, 3), 'ws+tr'),
             ((64, 128, 0, 1), 'plain'), ((384, 64, 0, 1), 'ws'), ((64, 64, 32, 3), 'plain'), ((72, 48, 0, 3), 'ws')]
    batch, jobs = ops.PackBatch(), []
    for case, mode in order:
        jobs.append((case, mode, False) + _register(ops, batch, case, mode))
    batch.run()
    _check(ops, jobs)


def _host_image(w, c0, c1):
    """the documented layout (csrc/weight_image.h, "fp16 element index") in numpy: uint16 planes and the oscale floats.
    fp16 element ((((((nt * nchunks + ch) * T + tap) * 2 + nh) * 2 + nb) * 2 + plane) * 64 + lane) * 8 + j holds plane
    (g1, g2) of w[o = nt*64 + nh*32 + nb*16 + (lane & 15)][c = chunk channel (lane >> 4)*8 + j][tap] / oscale[o]; a source's
    channels fill whole 32-channel chunks (zero beyond its width), oscale[o] = 2^(e - 15) with max |w[o]| = f * 2^e,
    f in [0.5, 1), and 1 for the padded channels."""
    cout, cin, k, _ = w.shape
    T, nt, n0, n1 = k * k, (cout + 63) // 64, (c0 + 31) // 32, (c1 + 31) // 32
    wp = np.zeros((nt * 64, (n0 + n1) * 32, T), np.float32)
    wp[:cout, :c0] = w[:, :c0].reshape(cout, c0, T)
    wp[:cout, n0 * 32:n0 * 32 + c1] = w[:, c0:].reshape(cout, c1, T)
    osc = np.ones((nt * 64,), np.float32)
    _, e = np.frexp(np.abs(w).reshape(cout, -1).max(1))
    osc[:cout] = np.ldexp(np.float32(1), e - 15)
    s = wp / osc[:, None, None]                                     # exact: a power of two
    g1 = s.astype(np.float16)
    g2 = (s - g1.astype(np.float32)).astype(np.float16)
    g = np.stack([g1, g2])                                          # [plane][o][c][tap]
    g = g.reshape(2, nt, 2, 2, 16, n0 + n1, 4, 8, T)                # [plane][nt][nh][nb][o & 15][chunk][k group][j][tap]
    g = g.transpose(1, 5, 8, 2, 3, 0, 6, 4, 7)                      # [nt][chunk][tap][nh][nb][plane][k group][o & 15][j]
    return np.ascontiguousarray(g).view(np.uint16), osc


@pytest.mark.parametrize('case', [(72, 48, 0, 3), (64, 48, 16, 3)], ids=str)
def test_image_layout_against_numpy(ops, case):
    """plain images only.  The weights are integer multiples of 2^-10 from [-4, 4] with at least one |w| >= 2 per channel:
    the scale is then 2^13 and every scaled value an integer multiple of 8 below 2^15 (2^12, 4 and at most 2^14 where the
    maximum is exactly 4), both planes are normal fp16 numbers or zero, the subtraction is exact, and both roundings are
    round-to-nearest-even on the host as on the device — no input on which numpy and the device may differ is left."""
    cout, c0, c1, k = case
    g = torch.Generator().manual_seed(77)
    w = torch.randint(-4096, 4097, (cout, c0 + c1, k, k), generator=g).float() / 1024
    w[:, 0, 0, 0] = torch.where(torch.arange(cout) % 3 == 0, 4.0, -2.5)     # (a maximum of exactly 4 on every third channel)
    assert w.abs().amax((1, 2, 3)).min() >= 2 and w.abs().max() <= 4
    host, osc = _host_image(w.numpy(), c0, c1)
    batch = ops.PackBatch()
    alone, in_table = ops.PackedConv(w.to(dev()), None, c0, c1), ops.PackedConv(w.to(dev()), None, c0, c1, batch=batch)
    batch.run()
    for pc in (alone, in_table):
        planes, tail = _planes(pc.wpack, case)
        assert np.array_equal(tail, osc)
        assert np.array_equal(planes, host)
