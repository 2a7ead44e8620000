"""CPU: the host side of re-labelling a batch (ddpm.relabel_batch, Trainer.relabel): the statement of tests/relabel_cases.py
against the numpy route it restates in closed form, the draw's words, the refusals, the Trainer's id rule, the binding of the
new entry point in a table of its own, its argument validation (before any launch: no GPU here), the CLI flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import relabel_cases as RC
from oracle import rng as ORNG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry -> the test file that launches it ALONE (the rule of tests/test_abi_coverage_host.py, for the table of
# include/dmhomo_hip_relabel.h)
ALONE = {'dmh_relabel_batch': ('test_gpu_relabel.py', 'ops.relabel_batch')}


# ------------------------------------------------------------------------------------------ the statement
SIZES = ((8, 8), (16, 16), (12, 20), (128, 128), (256, 256))


def test_closed_form_is_the_numpy_route():
    """P[i][j] = P0[i][j] s_i / s_j against adapt_homography_to_preprocessing_v3(360, 640, P0, H, W): within 1e-9 max|P| (measured:
    worst element-relative gap 1.1e-10 over 10 000 draws at five sizes)"""
    from dmhomo_amd.ddpm import adapt_homography_to_preprocessing_v3
    n, worst = 2000, 0.
    for k, (H, W) in enumerate(SIZES):
        u = RC.uniforms(RC.words(11 + k, range(n)))
        for b in range(n):
            P0 = RC.perturbation(u[b])
            P = RC.to_frame(P0, H, W)
            ref = adapt_homography_to_preprocessing_v3(360, 640, P0, H, W)
            gap = float(np.abs(P - ref).max()) / float(np.abs(P).max())
            worst = max(worst, gap)
    print(f'[relabel] closed form vs numpy route: worst gap / max|P| = {worst:.2e} over {n * len(SIZES)} draws (bound 1e-9)')
    assert worst <= 1e-9


def test_zero_ranges_give_the_identity_exactly():
    for H, W in SIZES:
        got = RC.homographies(3, range(5), H, W, ranges=(0., 0., 0.))
        assert np.array_equal(got, np.broadcast_to(np.eye(3), (5, 3, 3)))      # (u * 0 may be -0: equal to 0)


def test_uniforms_lie_in_the_closed_interval_and_are_exact():
    w = RC.words(1, range(4000))
    u = RC.uniforms(w)
    assert u.dtype == np.float64 and u.shape == (4000, 8) and float(u.min()) > -1. and float(u.max()) <= 1.
    assert abs(float(u.mean())) < 0.02
    assert np.array_equal(u * 2. ** 32, np.round(u * 2. ** 32))      # multiples of 2^-32: both double operations were exact
    lo, hi = RC.uniforms(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert lo == 2. ** -32 - 1. and hi == 1.


def test_another_seed_or_id_changes_the_words():
    base = RC.words(5, [7])
    assert base.shape == (1, 8) and base.dtype == np.uint32
    assert np.array_equal(base, RC.words(5, [7]))
    for other in (RC.words(6, [7]), RC.words(5, [8]), RC.words(5 + 2 ** 32, [7]), RC.words(5, [7 + 2 ** 32])):
        assert not (other == base).any()
    many = RC.words(0, range(64))
    assert len({tuple(r) for r in many.tolist()}) == 64
    assert np.array_equal(RC.words(0, [5, 6, 7]), many[5:8])         # a row depends on its own id alone


def test_the_draw_word_keeps_the_label_apart_from_the_noise():
    """the noise of the keyed generator counts its draws up from 0 in the same counter word"""
    for seed, sid in ((0, 0), (5, 41), (2 ** 40 + 3, 2 ** 33 + 1)):
        label = RC.words(seed, [sid])[0]
        assert np.array_equal(label, ORNG.words(seed, [sid], 0xFFFFFFFF, 8)[0])
        for draw in range(4):
            noise = ORNG.words(seed, [sid], draw, 8)[0]
            assert not (noise == label).any(), (seed, sid, draw)


def test_the_statement_alone_skips_no_pixel_and_keeps_half_of_every_sample():
    """with the default ranges at the shapes and seeds of the GPU test: no source coordinate within 1e-9 of a bound, and no sample
    with fewer than half its pixels valid (the minimum over 10 000 draws at 8 x 8 was 0.5625)"""
    lowest = 1.
    for B, H, W in RC.SHAPES:
        for seed in RC.SEEDS:
            for m in RC.homographies(seed, range(B), H, W):
                ok, near = RC.valid_of(m, H, W)
                assert not near.any(), (B, H, W, seed)
                lowest = min(lowest, float(ok.mean()))
    for m in RC.homographies(9, range(1000), 8, 8):
        lowest = min(lowest, float(RC.valid_of(m, 8, 8)[0].mean()))
    print(f'[relabel] lowest valid fraction of a sample: {lowest:.4f}')
    assert lowest >= 0.5


def test_identity_homography_has_every_pixel_valid():
    for B, H, W in RC.SHAPES:
        ok, near = RC.valid_of(np.eye(3), H, W)
        assert ok.all() and near.sum() == 2 * (H + W) - 4          # (the frame's border sits ON the bounds)


# ------------------------------------------------------------------------------------------ the refusals
BAD_RANGES = [(-.01, 8., 3e-5), (.03, -1., 3e-5), (.03, 8., -1e-6), (float('nan'), 8., 3e-5), (.03, float('inf'), 3e-5),
              (.03, 8., float('nan')), (.25, 8., 3e-5), (.3, 8., 3e-5), (.03, 8., 5e-4), (.03, 8., 1e-3), (.03, 8.), None, 'abc',
              (.03, 8., 3e-5, 1.)]


@pytest.mark.parametrize('bad', BAD_RANGES, ids=lambda v: str(v))
def test_ranges_are_refused(bad):
    from dmhomo_amd import ddpm, ops
    with pytest.raises(ValueError, match='relabel ranges'):
        ops.relabel_ranges(bad)
    data = torch.zeros(2, 12, 8, 8)                           # (a CPU tensor: a call that got as far as the kernel would say so)
    with pytest.raises(ValueError, match='relabel ranges'):
        ddpm.relabel_batch(data, [0, 1], ranges=bad)
    with pytest.raises(ValueError, match='relabel ranges'):
        ops.relabel_batch(data, torch.arange(2), ranges=bad)


def test_good_ranges_pass_and_other_arguments_are_refused():
    from dmhomo_amd import ddpm, ops
    assert ops.relabel_ranges((.03, 8, 3e-5)) == (.03, 8., 3e-5) == ops.RELABEL_RANGES
    assert ops.relabel_ranges([0, 0, 0]) == (0., 0., 0.)
    assert ops.relabel_ranges((0.2499, 1e6, 4.99e-4)) == (0.2499, 1e6, 4.99e-4)
    data = torch.zeros(2, 12, 8, 8)
    with pytest.raises(ValueError, match="base = 'other'"):
        ddpm.relabel_batch(data, [0, 1], base='other')
    with pytest.raises(ValueError, match='12'):
        ops.relabel_batch(torch.zeros(2, 6, 8, 8), torch.arange(2))
    with pytest.raises(ValueError, match='sample_ids'):
        ops.relabel_batch(data, torch.arange(3))
    with pytest.raises(ValueError, match='base'):
        ops.relabel_batch(data, torch.arange(2), base=torch.zeros(2, 9, dtype=torch.float64))
    import inspect
    sig = inspect.signature(ddpm.relabel_batch)
    assert list(sig.parameters) == ['data', 'sample_ids', 'seed', 'base', 'ranges', 'fill', 'max_flow']
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d['seed'], d['base'], d['ranges'], d['fill'], d['max_flow']) == (0, 'identity', (.03, 8., 3e-5), True, 256)


# ------------------------------------------------------------------------------------------ the Trainer
class _Sampler:
    """what Trainer.sample needs of a sampler, on the CPU"""
    image_size = 8

    def __init__(self, rng=None):
        self.calls = []
        if rng is not None:
            self.rng = rng

    def sample(self, classes, rgb_flow, flow, mask):
        self.calls.append((rgb_flow, flow, mask))
        return torch.zeros(flow.shape[0], 6, 8, 8), mask, flow


def _trainer(monkeypatch, sampler, batches):
    from dmhomo_amd import ddpm
    seen = []

    def fake_relabel(data, sample_ids, seed=0, base='identity', ranges=None, fill=True, max_flow=256):
        seen.append(dict(ids=[int(v) for v in sample_ids], seed=seed, base=base, ranges=ranges, rows=data.shape[0]))
        B = data.shape[0]
        return data + 1., torch.full((B, 3, 3), float(len(seen)), dtype=torch.float64), torch.ones(B, 1, 8, 8, dtype=torch.uint8)
    monkeypatch.setattr(ddpm, 'relabel_batch', fake_relabel)
    monkeypatch.setattr(ddpm, 'saveTrainPair', lambda imgs, mask, flows: {'flows': flows})
    return ddpm.Trainer(sampler, batches, train_batch_size=3), seen


def _batches(n, B=3):
    return [(torch.full((B, 12, 8, 8), float(k)), torch.zeros(B, dtype=torch.long)) for k in range(n)]


def test_trainer_defaults_are_inert(monkeypatch):
    from dmhomo_amd import ddpm
    T = ddpm.Trainer
    assert T.relabel is None and T.relabel_ranges == (.03, 8., 3e-5) and T.relabel_seed == 0 and T.relabel_first == 0
    assert T.last_relabel_homos is None and T.last_relabel_valid is None
    s = _Sampler()
    tr, seen = _trainer(monkeypatch, s, _batches(2))
    ret = tr.sample(0, 'cpu')
    assert not seen and tr.last_relabel_homos is None and float(ret['flows'].max()) == 0.     # the loader's batch, untouched


def test_trainer_ids_without_a_keyed_generator_count_the_rows_seen(monkeypatch):
    s = _Sampler()
    tr, seen = _trainer(monkeypatch, s, _batches(2) + _batches(1, B=2) + _batches(1))
    tr.relabel, tr.relabel_seed, tr.relabel_first, tr.relabel_ranges = 'batch', 17, 100, (.01, 2., 1e-5)
    ret = tr.sample(0, 'cpu')
    assert float(ret['flows'].min()) == 1.                    # everything below ran on the NEW batch
    assert float(s.calls[0][0].min()) == 1. and float(s.calls[0][2].min()) == 1.
    assert float(tr.last_relabel_homos[0, 0, 0]) == 1. and tr.last_relabel_valid.shape == (3, 1, 8, 8)
    tr.sample(0, 'cpu')
    tr.sample(0, 'cpu')                                       # a short batch
    tr.sample(0, 'cpu')
    assert [c['ids'] for c in seen] == [[100, 101, 102], [103, 104, 105], [106, 107], [108, 109, 110]]
    assert all((c['seed'], c['base'], c['ranges']) == (17, 'batch', (.01, 2., 1e-5)) for c in seen)
    assert float(tr.last_relabel_homos[0, 0, 0]) == 4.


def test_trainer_ids_are_the_keyed_generators(monkeypatch):
    from dmhomo_amd.sampling import DeviceRng
    rng = DeviceRng().key_by_sample(5, range(40, 43), 'cpu')
    s = _Sampler(rng)
    tr, seen = _trainer(monkeypatch, s, _batches(2) + _batches(1, B=2))
    tr.relabel, tr.relabel_first = 'identity', 1000
    tr.sample(0, 'cpu')
    rng.key_by_sample(5, range(46, 49), 'cpu')
    tr.sample(0, 'cpu')
    tr.sample(0, 'cpu')                                       # a short batch draws the first rows' ids, like the noise
    assert [c['ids'] for c in seen] == [[40, 41, 42], [46, 47, 48], [46, 47]]
    rng.unkey()                                               # back to counting: the rows of the keyed calls were seen too
    tr.dl = iter(_batches(1))
    tr.sample(0, 'cpu')
    assert seen[-1]['ids'] == [1008, 1009, 1010]


def test_trainer_refuses_the_target_and_what_is_no_base_before_it_draws_a_batch(monkeypatch):
    s = _Sampler()
    tr, seen = _trainer(monkeypatch, s, _batches(1))
    tr.relabel, tr.keep = 'identity', 'target'
    with pytest.raises(ValueError, match="keep = 'target'.*old label"):
        tr.sample(0, 'cpu')
    tr.keep, tr.relabel = None, 'homography'
    with pytest.raises(ValueError, match="Trainer.relabel = 'homography'"):
        tr.sample(0, 'cpu')
    tr.relabel, tr.relabel_ranges = 'identity', (.5, 8., 3e-5)
    with pytest.raises(ValueError, match='relabel ranges'):
        tr.sample(0, 'cpu')
    assert not seen and not s.calls
    tr.relabel_ranges = (.03, 8., 3e-5)
    tr.sample(0, 'cpu')                                       # the one batch is still there
    assert len(seen) == 1


# ------------------------------------------------------------------------------------------ the binding
def _header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def _header_functions(name):
    return sorted(set(re.findall(r'\b(dmh_[a-z0-9_]+)\s*\(', _header_source(name))))


def _ctype_of(param):
    param = param.strip()
    if '*' in param:
        return C.c_void_p
    for word, t in (('uint64_t', C.c_uint64), ('int64_t', C.c_int64), ('double', C.c_double), ('float', C.c_float),
                    ('int', C.c_int)):
        if re.search(r'\b' + word + r'\b', param):
            return t
    raise AssertionError(param)


def test_the_new_entry_has_a_header_and_a_table_of_its_own():
    from dmhomo_amd import _lib, ops
    names = _header_functions('dmhomo_hip_relabel.h')
    assert names == sorted(_lib.RELABEL_EXTENSIONS) == ['dmh_relabel_batch']
    for table in (_lib.SIGNATURES, _lib.EXTENSIONS, _lib.START_EXTENSIONS):
        assert not set(names) & set(table)
    for other in ('dmhomo_hip.h', 'dmhomo_hip_known.h', 'dmhomo_hip_start.h'):
        assert 'dmh_relabel' not in open(os.path.join(ROOT, 'include', other)).read()
    assert _lib.ABI_VERSION == 500
    h = C.CDLL(_lib.LIB_PATH)
    lib = _lib.lib()
    src = _header_source('dmhomo_hip_relabel.h')
    for name in names:
        assert hasattr(h, name), name
        res, args = _lib.RELABEL_EXTENSIONS[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args), name
        proto = re.search(r'\bint\s+' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert proto and res is C.c_int
        assert [_ctype_of(p) for p in proto.group(1).split(',')] == list(args), name      # the table against the prototype
    assert callable(ops.relabel_batch)
    assert "call('dmh_relabel_batch'" in open(os.path.join(ROOT, 'dmhomo_amd', 'ops.py')).read()


def test_the_new_entry_names_the_test_that_launches_it_alone():
    from dmhomo_amd import _lib
    assert sorted(ALONE) == sorted(_lib.RELABEL_EXTENSIONS)
    tests = os.path.dirname(os.path.abspath(__file__))
    for entry, (file, name) in ALONE.items():
        src = open(os.path.join(tests, file)).read()
        assert re.search(r'\b' + re.escape(name) + r'\s*\(', src), (entry, file)


def test_a_library_without_the_new_symbol_fails_loudly(monkeypatch):
    from dmhomo_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setitem(_lib.RELABEL_EXTENSIONS, 'dmh_relabel_missing', (C.c_int, []))
    with pytest.raises(AttributeError, match='dmh_relabel_missing'):
        _lib.lib()


def test_the_makefile_builds_the_new_source_with_its_header():
    mk = open(os.path.join(ROOT, 'dmhomo_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\brelabel\.hip\b', mk, flags=re.M)
    rules = [ln for ln in mk.splitlines() if re.match(r'^(asan/)?%\.o: %\.hip', ln)]
    assert len(rules) == 2 and all('include/dmhomo_hip_relabel.h' in ln for ln in rules)


def test_the_kernels_share_their_per_pixel_bodies():
    """the flow and the warp are one definition each, called from the stand-alone kernels and from the fused one"""
    csrc = os.path.join(ROOT, 'dmhomo_amd', 'csrc')
    read = lambda f: open(os.path.join(csrc, f)).read()
    dev = read('geometry_dev.h')
    for fn in ('homography_flow_pixel', 'homography_inverse', 'homography_warp_source', 'homography_warp_taps',
               'homography_warp_sample'):
        assert len(re.findall(r'__device__ __forceinline__ \w+ ' + fn + r'\(', dev)) == 1, fn
    assert 'homography_flow_pixel(' in read('geometry.hip') and 'homography_flow_pixel(' in read('relabel.hip')
    for fn in ('homography_inverse(', 'homography_warp_source(', 'homography_warp_taps(', 'homography_warp_sample('):
        assert fn in read('preview.hip') and fn in read('relabel.hip'), fn
    for f in ('geometry_dev.h', 'relabel.hip'):
        assert '#pragma clang fp contract(off)' in read(f)


def test_the_entry_validates_its_arguments():
    """DMH_EINVAL (-1) with a message, before anything is launched (no GPU here)"""
    from dmhomo_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * (16 * 8192))()
    base = (C.addressof(buf) + 15) & ~15
    p = lambda k=0, off=0: C.c_void_p(base + 8192 * k + off)  # disjoint host addresses: only ever compared, never read
    n = 0

    def refused(args, word):
        nonlocal n
        assert lib.dmh_relabel_batch(*args, None) == -1, (args, word)
        assert b'dmh_relabel_batch' in lib.dmh_last_error() and word.encode() in lib.dmh_last_error(), (word, lib.dmh_last_error())
        n += 1
    #       data  ids   seed a    t   p     maxf  base  fill out   Hm    valid B  H  W      (2 x 12 x 8 x 8 floats = 6144 bytes)
    good = [p(0), p(1), 5, .03, 8., 3e-5, 256., None, 1, p(3), p(4), p(5), 2, 8, 8]
    with_base = good[:7] + [p(2)] + good[8:]
    for g in (good, with_base):
        for i in (0, 1, 9, 10, 11):
            refused(g[:i] + [None] + g[i + 1:], 'null pointer')
        for B, H, W in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (2, 1, 8), (2, 8, 1), (2, 0, 8), (2, 8, -3), (2, 65537, 8),
                        (2, 8, 65537), (2, 65536, 65536), (65535, 64, 64)):
            refused(g[:12] + [B, H, W], 'B*12*H*W')
        for i in (3, 4, 5):
            for bad in (-1e-9, float('nan'), float('inf'), -float('inf')):
                refused(g[:i] + [bad] + g[i + 1:], 'finite number >= 0')
        refused(g[:3] + [.25] + g[4:], 'max_affine')
        refused(g[:3] + [1.] + g[4:], 'max_affine')
        refused(g[:5] + [5e-4] + g[6:], 'max_persp')
        for bad in (0., -1., float('nan'), float('inf')):
            refused(g[:6] + [bad] + g[7:], 'max_flow')
        refused([p(0, 2)] + g[1:], '4-byte')
        refused(g[:9] + [p(3, 1)] + g[10:], '4-byte')
        refused(g[:1] + [p(1, 4)] + g[2:], '8-byte')
        refused(g[:10] + [p(4, 4)] + g[11:], '8-byte')
        refused(g[:9] + [g[0]] + g[10:], 'out overlaps data')                     # out == data
        refused(g[:9] + [p(0, 6140)] + g[10:], 'out overlaps data')               # the last float of data
        refused([p(3, 6140)] + g[1:], 'out overlaps data')                        # data begins on the last float of out
    refused(with_base[:7] + [p(2, 4)] + with_base[8:], '8-byte')
    assert n == 2 * (5 + 11 + 12 + 3 + 4 + 4 + 3) + 1


# ------------------------------------------------------------------------------------------ the CLI
def test_cli_flags_parse_and_the_docstring_warns_about_synthetic_conditions():
    src = open(os.path.join(ROOT, 'scripts', 'dgm_sample.py')).read()
    doc = src.split('"""')[1]
    assert '[--relabel identity' in doc.split('\n\n')[1]      # the usage line
    para = [p for p in doc.split('  * ') if p.startswith('--relabel')]
    assert len(para) == 1 and 'SyntheticConditions' in para[0] and 'black' in para[0] and '--conditions' in para[0]
    assert 'not measured' in para[0]
    head = src[:src.index('args = parser.parse_args()')]
    head = head[head.index('parser = argparse.ArgumentParser()'):]
    ns = {}
    exec('import argparse\n' + head, ns)                     # the parser alone (the script's imports need the built package)
    p = ns['parser']
    off = p.parse_args([])
    assert off.relabel is None and off.relabel_seed is None and off.relabel_ranges is None      # off by default
    a = p.parse_args(['--relabel', 'batch', '--relabel_seed', '7', '--relabel_ranges', '.01', '4', '1e-5', '--keep', 'source',
                      '--strength', '0.5'])
    assert (a.relabel, a.relabel_seed, a.relabel_ranges, a.keep, a.strength) == ('batch', 7, [.01, 4., 1e-5], 'source', 0.5)
    assert p.parse_args(['--relabel', 'identity']).relabel == 'identity'
    for bad in (['--relabel'], ['--relabel', 'other'], ['--relabel_ranges', '1', '2'], ['--relabel_seed', 'x']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    help_ = [a for a in p._actions if a.dest == 'relabel'][0].help
    assert 'SyntheticConditions' in help_ and 'black' in help_ and '--conditions' in help_
    assert 'trainer.relabel = args.relabel' in src
    assert 'trainer.relabel_seed = args.seed if args.relabel_seed is None else args.relabel_seed' in src
