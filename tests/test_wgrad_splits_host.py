"""CPU: the weight-gradient split rule that tests/test_gpu_wgrad_splits.py restates, against the library's own host
function (dmh_conv_wgrad_workspace_floats), and the coverage the GPU file's parametrization claims: if the split
heuristic changes, these fail instead of the GPU tests quietly losing their multi-item cases."""
import itertools

from dmhomo_amd import _lib
from test_gpu_wgrad_splits import (CASES, DYN_CASE, TRAIN_SHAPES, case_plan, cdiv, train_case, wgrad_npairs,
                                   wgrad_splits, wgrad_splits_f16)


def _expected_workspace(B, H, W, c0, c1, cout, k):
    npairs = wgrad_npairs(c0 + c1, cout, k)
    nitems = B * cdiv(H, 4) * cdiv(W, 16)
    ns = wgrad_splits(nitems, npairs)
    if k <= 3:
        ns = max(ns, wgrad_splits_f16(nitems, npairs))
    return ns * npairs * 64 * 64 * k * k + ns * cdiv(cout, 64) * 64


def _all_cases():
    return CASES + [DYN_CASE] + [train_case(s) for s in TRAIN_SHAPES]


def test_split_rule_matches_workspace_size():
    """partial blocks of the workspace = max(fp32 splits, fp16-piece splits) for k <= 3, the fp32 splits otherwise"""
    ws = _lib.lib().dmh_conv_wgrad_workspace_floats
    shapes = [(c[1], c[2], c[3], c[4], c[5], c[6], c[7]) for c in _all_cases()]
    shapes += [(B, H, W, c0, 0, cout, k) for B, H, W, c0, cout, k in itertools.product(
        (1, 3, 16), (4, 17, 128), (16, 33, 128), (8, 64, 200, 512), (24, 64, 384), (1, 2, 3, 7))]
    for s in shapes:
        assert ws(*s) == _expected_workspace(*s), s


def test_gpu_cases_cover_the_split_edges():
    plans = {c[0]: case_plan(c) for c in _all_cases()}
    for fam in ('f16', 'fp32'):
        ps = [p for p in plans.values() if p['family'] == fam]
        assert any(p['per'] == 2 for p in ps), fam
        assert any(p['per'] >= 3 for p in ps), fam
        assert any(p['ragged'] for p in ps), fam
        assert any(p['empty'] > 0 for p in ps), fam
    for c in CASES + [DYN_CASE]:                            # every targeted case reaches the multi-item code
        assert case_plan(c)['per'] >= 2, c
    assert case_plan(DYN_CASE)['per'] >= 3 and case_plan(DYN_CASE)['family'] == 'f16'
    assert case_plan(CASES[0])['empty'] == 112               # B=3, 64x96, 64->64: 288 items over 256 splits
    modes = {(c[7], c[8]) for c in CASES}
    assert {(3, 'plain'), (3, 'concat'), (3, 'coef'), (3, 'ups'), (2, 'down')} <= modes
    assert {1, 7} <= {c[7] for c in CASES}
    odd = [c for c in CASES if c[6] % 64 or (c[4] + c[5]) % 64]
    assert {case_plan(c)['family'] for c in odd} == {'f16', 'fp32'}


def test_training_shape_list_is_the_b16_training_step():
    """TRAIN_SHAPES: distinct, recorded at 128x128 (the dy of the finest level); at B = 16 the finest level's shapes
    give a workgroup several items (16 for the 64-channel 3x3 convs, 8 for the 7x7 init conv)"""
    assert len(TRAIN_SHAPES) == len(set(TRAIN_SHAPES)) > 0
    assert max(s[5] for s in TRAIN_SHAPES) == 128
    assert {s[0] for s in TRAIN_SHAPES} == {1, 2, 3, 7}
    plans = {s: case_plan(train_case(s)) for s in TRAIN_SHAPES}
    assert plans[(3, 0, 64, 0, 64, 128, 128, 0)]['per'] == 16 and plans[(7, 0, 12, 0, 64, 128, 128, 0)]['per'] == 8
    assert all(p['per'] >= 2 for s, p in plans.items() if s[5] >= 64)
