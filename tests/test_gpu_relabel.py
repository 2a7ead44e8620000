"""-m gpu: re-labelling a batch of real pairs (ddpm.relabel_batch, Trainer.relabel): the kernel (dmh_relabel_batch) alone and the
Trainer on top of it.

1. dmh_relabel_batch alone, into NaN-poisoned outputs between guard words: the homographies against the float64 statement of
   tests/relabel_cases.py, flow / flow image / warped source bit for bit the stand-alone kernels' on the homographies it wrote,
   the validity against the statement's coordinates, the fill, the copies, zero ranges, sharding, the refusals;
2. Trainer.sample with relabel on the smallest network of the sampler tests (tests/detweights.py, 16 x 16), eager and captured,
   keyed generator."""
import ctypes as C

import numpy as np
import pytest
import torch

import known_cases as KC
import relabel_cases as RC
from gpu_util import dev
from test_gpu_guidance import g, same
from test_gpu_solver import _cfg_diffusion, _cfg_model

pytestmark = pytest.mark.gpu

SEED = 3
GUARD = 24                                                    # words in front of and behind every output


# --------------------------------------------------------------------------------------------- 1. the kernel alone
def _guarded(shape, dtype, off=0):
    """an output of ``shape`` poisoned with NaN (0xAB for bytes) between guard words -> (view, buffer, lo)"""
    n = int(np.prod(shape))
    fill = 0xAB if dtype == torch.uint8 else float('nan')
    lo = GUARD + off
    buf = torch.full((n + lo + GUARD,), fill, device=dev(), dtype=dtype)
    return buf[lo:lo + n].view(shape), buf, lo


def _guards_hold(buf, lo, n):
    head, tail = buf[:lo], buf[lo + n:]
    if buf.dtype == torch.uint8:
        return bool((head == 0xAB).all()) and bool((tail == 0xAB).all())
    return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())


def _ids(B, first=0):
    return torch.arange(first, first + B, dtype=torch.int64, device=dev())


def _launch(data, ids, seed=SEED, ranges=RC.RANGES, base=None, fill=True, off=0):
    """one guarded ops.relabel_batch -> (out, homos, valid) with the guards checked and nothing left poisoned"""
    from dmhomo_amd import ops
    B, _, H, W = data.shape
    out, obuf, olo = _guarded((B, 12, H, W), torch.float32, off)
    hm, hbuf, hlo = _guarded((B, 3, 3), torch.float64, off)
    va, vbuf, vlo = _guarded((B, H, W), torch.uint8, off)
    before = data.clone()
    got = ops.relabel_batch(data, ids, seed, ranges, 256., base, fill, out=out, homos=hm, valid=va)
    assert got[0] is out and got[1] is hm and got[2] is va
    assert _guards_hold(obuf, olo, out.numel()) and _guards_hold(hbuf, hlo, hm.numel()) and _guards_hold(vbuf, vlo, va.numel())
    assert not torch.isnan(out).any() and not torch.isnan(hm).any() and bool((va <= 1).all())       # every word was written
    assert same(data, before)
    return out, hm, va


@pytest.fixture(scope='module')
def cases():
    """per shape: the batch (its flow channels a real homography flow, for the 'batch' base), its DLT homographies, and one
    launch per (base, fill) — computed once and left unchanged"""
    from dmhomo_amd import ops
    out = {}
    for i, (B, H, W) in enumerate(RC.SHAPES):
        data = g(RC.batch_inputs(B, H, W, 50 + i))
        hb = g(torch.from_numpy(RC.base_homographies(B, H, W)))
        flow, rgb = ops.homography_flow(hb, H, W, 256.)
        data[:, 7:10], data[:, 10:] = rgb, flow
        dlt = ops.dlt_homography(data[:, 10:].contiguous())
        c = {'data': data, 'dlt': dlt, 'ids': _ids(B, 10 * i)}
        c['identity'] = _launch(data, c['ids'])
        c['nofill'] = _launch(data, c['ids'], fill=False, off=1)
        c['batch'] = _launch(data, c['ids'], base=dlt)
        out[(B, H, W)] = c
    return out


def _rel_gap(got, want):
    """worst |got - want| / |want| over the entries (an entry that is exactly 0 in the statement must be 0)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = want == 0.
    assert (got[zero] == 0.).all()
    return float((np.abs(got - want)[~zero] / np.abs(want[~zero])).max())


def test_uniforms_are_bitwise():
    """at a size and ranges where every scaling is a power of two the entries ARE the uniforms: read back bit for bit"""
    B, H, W = RC.EXACT_SHAPE
    a, t, p = RC.EXACT_RANGES
    assert (W / 640., H / 360.) == (2. ** -5, 2. ** -3)
    ids = _ids(B, 123456789012)                               # (an id with a high word)
    _, hm, _ = _launch(g(RC.batch_inputs(B, H, W, 1)), ids, ranges=RC.EXACT_RANGES)
    hm = hm.cpu().numpy()
    u = RC.uniforms(RC.words(SEED, ids.tolist()))
    s0, s1 = W / 640., H / 360.
    back = np.stack([(hm[:, 0, 0] - 1.) / a, hm[:, 0, 1] * s1 / s0 / a, hm[:, 0, 2] / s0 / t,
                     hm[:, 1, 0] * s0 / s1 / a, (hm[:, 1, 1] - 1.) / a, hm[:, 1, 2] / s1 / t,
                     hm[:, 2, 0] * s0 / p, hm[:, 2, 1] * s1 / p], axis=1)
    assert np.array_equal(back.view(np.int64), u.view(np.int64))
    assert np.array_equal(hm, RC.homographies(SEED, ids.tolist(), H, W, RC.EXACT_RANGES)) and (hm[:, 2, 2] == 1.).all()


@pytest.mark.parametrize('shape', RC.SHAPES, ids=str)
def test_homographies_against_the_statement(cases, shape):
    """identity base: rtol 1e-13 (one multiply and one divide per entry); 'batch' base: rtol 1e-12 (five more operations and a
    divide), on the DLT homographies the device computed"""
    B, H, W = shape
    c = cases[shape]
    ids = c['ids'].tolist()
    want = RC.homographies(SEED, ids, H, W)
    gap = _rel_gap(c['identity'][1].cpu().numpy(), want)
    gap_b = _rel_gap(c['batch'][1].cpu().numpy(), RC.homographies(SEED, ids, H, W, base=c['dlt'].cpu().numpy()))
    print(f'[relabel] {shape}: worst relative gap of an entry of Hm: identity {gap:.2e} (gate 1e-13), batch {gap_b:.2e} (gate 1e-12)')
    assert gap <= 1e-13 and gap_b <= 1e-12
    assert same(c['nofill'][1], c['identity'][1])             # the label does not depend on the fill
    assert not np.array_equal(c['batch'][1].cpu().numpy(), c['identity'][1].cpu().numpy())
    assert float((c['batch'][1][:, 2, 2] - 1.).abs().max()) == 0.


@pytest.mark.parametrize('which', ['identity', 'nofill', 'batch'])
@pytest.mark.parametrize('shape', RC.SHAPES, ids=str)
def test_planes_are_the_stand_alone_kernels_on_the_homographies_written(cases, shape, which):
    from dmhomo_amd import ops
    B, H, W = shape
    c = cases[shape]
    data = c['data']
    out, hm, va = c[which]
    flow, rgb = ops.homography_flow(hm.contiguous(), H, W, 256.)
    assert same(out[:, 10:], flow) and same(out[:, 7:10], rgb)
    assert same(out[:, :3], data[:, :3]) and same(out[:, 6], data[:, 6])         # the copies
    warp = ops.homography_warp(data[:, :3].contiguous(), hm.contiguous(), (W, H))
    ok = va.bool().unsqueeze(1).expand(B, 3, H, W)
    if which == 'nofill':
        assert same(out[:, 3:6], warp)
    else:
        assert same(out[:, 3:6][ok], warp[ok])
        assert same(out[:, 3:6][~ok], data[:, 3:6][~ok])      # the batch's own target where the warp has no source pixel
    assert int((~ok).sum()) > 0                               # (both arms were seen)


@pytest.mark.parametrize('which', ['identity', 'batch'])
@pytest.mark.parametrize('shape', RC.SHAPES, ids=str)
def test_valid_against_the_statements_coordinates(cases, shape, which):
    """float64 coordinates from the homographies the kernel wrote, in its operation order; a pixel whose coordinate is within 1e-9
    of a bound may be skipped, at most one per case; under the identity base no sample has fewer than half its pixels valid"""
    B, H, W = shape
    _, hm, va = cases[shape][which]
    hm, va = hm.cpu().numpy(), va.cpu().numpy().astype(bool)
    skipped = 0
    for b in range(B):
        ok, near = RC.valid_of(hm[b], H, W)
        skipped += int(near.sum())
        assert np.array_equal(va[b][~near], ok[~near]), (shape, which, b)
        if which == 'identity':
            assert va[b].mean() >= 0.5, (shape, b, va[b].mean())
    assert skipped <= 1, skipped


@pytest.mark.parametrize('shape', RC.SHAPES, ids=str)
def test_zero_ranges_leave_the_source_where_it_is(cases, shape):
    B, H, W = shape
    data = cases[shape]['data']
    out, hm, va = _launch(data, cases[shape]['ids'], ranges=(0., 0., 0.))
    eye = torch.eye(3, dtype=torch.float64, device=dev()).expand(B, 3, 3)
    assert torch.equal(hm, eye) and bool((va == 1).all()) and same(out[:, 3:6], data[:, :3])


def test_rows_of_a_shard_are_the_rows_of_the_whole_job():
    B, H, W = 10, 16, 16
    data = g(RC.batch_inputs(B, H, W, 77))
    whole = _launch(data, _ids(B))
    again = _launch(data, _ids(B), off=3)
    part = _launch(data[5:8].contiguous(), _ids(3, 5))
    for w, a, p in zip(whole[:2], again[:2], part[:2]):
        assert same(w, a) and same(w[5:8], p)
    assert torch.equal(whole[2], again[2]) and torch.equal(whole[2][5:8], part[2])
    other = _launch(data, _ids(B), seed=SEED + 1)
    assert not same(other[1], whole[1]) and not same(other[0][:, 10:], whole[0][:, 10:])
    assert same(other[0][:, :3], whole[0][:, :3])
    assert len({tuple(h.flatten().tolist()) for h in whole[1]}) == B           # every id its own label


def test_public_call_is_the_kernel_behind_the_dlt(cases):
    from dmhomo_amd import ddpm
    shape = (3, 16, 16)
    c = cases[shape]
    ids = c['ids'].tolist()
    out, homos, valid = ddpm.relabel_batch(c['data'], ids, SEED)
    assert homos.shape == (3, 3, 3) and homos.dtype == torch.float64 and valid.shape == (3, 1, 16, 16) and valid.dtype == torch.uint8
    assert same(out, c['identity'][0]) and same(homos, c['identity'][1]) and torch.equal(valid[:, 0], c['identity'][2])
    out, homos, valid = ddpm.relabel_batch(c['data'], c['ids'], SEED, base='batch')
    assert same(out, c['batch'][0]) and same(homos, c['batch'][1]) and torch.equal(valid[:, 0], c['batch'][2])
    out, _, _ = ddpm.relabel_batch(c['data'], c['ids'], SEED, fill=False)
    assert same(out, c['nofill'][0])


def test_rejected_arguments_launch_nothing():
    """DMH_EINVAL with a message and every output word still poisoned: out == data, B = 0, H = 1, a null ids (no bad device
    pointer is passed: every pointer is a live allocation or NULL)"""
    from dmhomo_amd import _lib, ops
    B, H, W = 2, 8, 8
    data = g(RC.batch_inputs(B, H, W, 5))
    ids = _ids(B)
    out, obuf, _ = _guarded((B, 12, H, W), torch.float32)
    hm, hbuf, _ = _guarded((B, 3, 3), torch.float64)
    va, vbuf, _ = _guarded((B, H, W), torch.uint8)
    lib = _lib.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    good = [P(data), P(ids), SEED, .03, 8., 3e-5, 256., None, 1, P(out), P(hm), P(va), B, H, W]
    for args, word in ((good[:9] + [P(data)] + good[10:], 'out overlaps data'), (good[:12] + [0, H, W], 'B=0'),
                       (good[:12] + [B, 1, W], 'H=1'), (good[:1] + [None] + good[2:], 'null pointer')):
        assert lib.dmh_relabel_batch(*args, _lib.stream()) == -1, word
        assert word.encode() in lib.dmh_last_error(), (word, lib.dmh_last_error())
    with pytest.raises(_lib.DmhError, match='out overlaps data'):
        ops.relabel_batch(data, ids, out=data)
    with pytest.raises(ValueError, match='relabel ranges'):
        ops.relabel_batch(data, ids, ranges=(.3, 8., 3e-5), out=out, homos=hm, valid=va)
    torch.cuda.synchronize()
    assert bool(torch.isnan(obuf).all()) and bool(torch.isnan(hbuf).all()) and bool((vbuf == 0xAB).all())
    assert same(data, g(RC.batch_inputs(B, H, W, 5)))


# --------------------------------------------------------------------------------------------- 2. the Trainer
T_, S_, B_, SIZE = 100, 5, 4, 16
FIRST = 40


@pytest.fixture(scope='module')
def tiny():
    m, _ = _cfg_model()
    return m


def _diffusion(m, **attrs):
    from dmhomo_amd import cfg
    m.cfg_mode, m.dedup_dropped_rows = 'batched', False
    d = _cfg_diffusion(m, size=SIZE, T=T_, S=S_)
    d.rng = cfg.DeviceRng()
    for k, v in attrs.items():
        setattr(d, k, v)
    return d


def _batch():
    """a loader batch of B_ rows whose source images hold every byte value n / 255"""
    from dmhomo_amd import ddpm
    data, classes = next(ddpm.SyntheticConditions(SIZE, B_, seed=1000))
    data = data.clone()
    gen = torch.Generator().manual_seed(31)
    data[:, :6] = g(torch.rand((B_, 6, SIZE, SIZE), generator=gen))
    data[:, :3] = g(KC.all_bytes().repeat(3 * B_).reshape(B_, 3, SIZE, SIZE))
    return data, classes


def _trainer(d, batches, **attrs):
    from dmhomo_amd import ddpm
    tr = ddpm.Trainer(d, batches, train_batch_size=B_)
    assert tr.ema.ema_model is d
    for k, v in attrs.items():
        setattr(tr, k, v)
    return tr


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'captured'])
def test_trainer_samples_the_real_source_under_a_new_label(tiny, graph):
    from dmhomo_amd import ddpm, ops
    data, classes = _batch()
    d = _diffusion(tiny, hip_graph=graph)
    tr = _trainer(d, [(data, classes)] * 4, relabel='identity', relabel_seed=11, keep='source', strength=0.5)
    key = lambda dd, lo=FIRST, n=B_: dd.rng.key_by_sample(5, range(lo, lo + n), dev())
    key(d)
    ret = tr.sample(0, 0)
    homos, valid = tr.last_relabel_homos, tr.last_relabel_valid
    assert homos.shape == (B_, 3, 3) and valid.shape == (B_, 1, SIZE, SIZE) and 0 < int(valid.sum()) < valid.numel()
    # by hand: relabel_batch, then sample_from on its outputs
    new, h2, v2 = ddpm.relabel_batch(data, range(FIRST, FIRST + B_), 11)
    assert same(h2, homos) and torch.equal(v2, valid)
    key(d)
    pair = new[:, :6]
    imgs = d.sample_from(pair, 0.5, classes=classes, rgb_flow=new[:, -5:-2], flow=new[:, -2:].contiguous(), mask=new[:, -6:-5],
                         known=pair, known_mask='source')
    want = ddpm.saveTrainPair(imgs[0], mask=imgs[1], flows=imgs[2])
    assert sorted(ret) == sorted(want) == ['homos', 'imgs']
    assert np.array_equal(ret['imgs'], want['imgs']) and np.array_equal(ret['homos'], want['homos'])
    # the record: the batch's source bytes, the DLT of the NEW flow
    src = torch.arange(256, dtype=torch.uint8).repeat(B_, 3).reshape(B_, 3, SIZE, SIZE).numpy()
    assert (ret['imgs'][:, :3] == src).all()
    flow, _ = ops.homography_flow(homos.contiguous(), SIZE, SIZE, 256.)
    assert np.array_equal(ret['homos'], ddpm.homo_gen(flow).cpu().numpy().squeeze())
    assert not np.array_equal(ret['homos'], ddpm.homo_gen(data[:, -2:]).cpu().numpy().squeeze())      # not the old label
    # another relabel_seed: other labels, no new capture
    caps, cached = d.graph_captures, len(d.__dict__.get('_graph_states', {}))
    assert caps == (1 if graph else 0) and cached == caps
    tr.relabel_seed = 12
    key(d)
    other = tr.sample(0, 0)
    assert not same(tr.last_relabel_homos, homos) and not np.array_equal(other['homos'], ret['homos'])
    assert (other['imgs'][:, :3] == src).all()
    assert d.graph_captures == caps and len(d.__dict__.get('_graph_states', {})) == cached
    # the same labels from a second trainer whose loader deals the rows in two half batches keyed with their ids (built last: a
    # second sampler on the shared network replaces the engine signature the first one's captures are cached under)
    d2 = _diffusion(tiny, hip_graph=graph)
    half = B_ // 2
    tr2 = _trainer(d2, [(data[:half].contiguous(), classes[:half]), (data[half:].contiguous(), classes[half:])],
                   relabel='identity', relabel_seed=11, keep='source', strength=0.5)
    labels, records = [], []
    for k in range(2):
        key(d2, FIRST + k * half, half)
        records.append(tr2.sample(0, 0))
        labels.append(tr2.last_relabel_homos)
    assert same(torch.cat(labels), homos)
    assert np.array_equal(np.concatenate([r['homos'] for r in records]), ret['homos'])


def test_trainer_relabels_in_front_of_every_sampling_mode(tiny):
    """strength alone: sample_from starts from the new pair; neither: sample() under the new labels; keep = 'target': refused"""
    from dmhomo_amd import ddpm
    data, classes = _batch()
    d = _diffusion(tiny)
    tr = _trainer(d, [(data, classes)] * 4, relabel='batch', relabel_seed=2)
    ids = range(FIRST, FIRST + B_)
    new, homos, _ = ddpm.relabel_batch(data, ids, 2, base='batch')
    conds = dict(classes=classes, rgb_flow=new[:, -5:-2], flow=new[:, -2:].contiguous(), mask=new[:, -6:-5])
    d.rng.key_by_sample(5, ids, dev())
    ret = tr.sample(0, 0)
    assert same(tr.last_relabel_homos, homos)
    d.rng.key_by_sample(5, ids, dev())
    imgs = d.sample(**conds)
    assert np.array_equal(ret['imgs'], ddpm.saveTrainPair(imgs[0], mask=imgs[1], flows=imgs[2])['imgs'])
    tr.strength = 0.6
    d.rng.key_by_sample(5, ids, dev())
    ret = tr.sample(0, 0)
    d.rng.key_by_sample(5, ids, dev())
    imgs = d.sample_from(new[:, :6], 0.6, **conds)
    assert np.array_equal(ret['imgs'], ddpm.saveTrainPair(imgs[0], mask=imgs[1], flows=imgs[2])['imgs'])
    tr.keep = 'target'
    with pytest.raises(ValueError, match="keep = 'target'"):
        tr.sample(0, 0)
    # without a keyed generator: relabel_first + rows seen
    d.rng.unkey()
    tr.keep, tr.strength, tr.relabel, tr.relabel_first = None, None, 'identity', 500
    seen = tr._relabel_seen
    assert seen == 2 * B_
    torch.manual_seed(1)
    tr.sample(0, 0)
    _, want, _ = ddpm.relabel_batch(data, range(500 + seen, 500 + seen + B_), 2)
    assert same(tr.last_relabel_homos, want)
