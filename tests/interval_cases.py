"""Shared by tests/test_interval_host.py and tests/test_gpu_interval.py: the guidance interval (``guidance_interval``,
limited-interval guidance of Kynkaanniemi et al. 2024) restated — which entries of a sampling loop are guided, and the row
lists dmh_rows_gated builds for them (include/dmhomo_hip.h, "Guidance interval").  No GPU, no dmhomo_amd import."""
import itertools

import torch

SENTINEL = -77          # what the row buffers hold before a launch: slots behind rows[0 .. n] must still hold it afterwards


def sample_times(T, S):
    """the time list of the sampling loops (CFG:674-677): S values from T - 1 down, the last step goes to -1"""
    ts = torch.linspace(-1, T - 1, steps=S + 1).int().tolist()
    return ts[:0:-1]


def guided_pattern(times, T, interval):
    """an entry at timestep t is guided iff lo <= t / (T - 1) <= hi, in float64; no interval: every entry"""
    if interval is None:
        return [True] * len(times)
    return [float(interval[0]) <= float(t) / float(max(T - 1, 1)) <= float(interval[1]) for t in times]


# (T, S, interval, the pattern written out by hand).  The first has an unguided -> guided and a guided -> unguided transition and
# an unguided last entry: times 99 82 65 49 32 15, u = 1.000 .828 .657 .495 .323 .152
PATTERNS = (
    (100, 6, (0.3, 0.7), [False, False, True, True, True, False]),
    (100, 6, (0., 1.), [True] * 6),
    (100, 6, (0.9, 0.95), [False] * 6),                      # contains no sampled time
    (100, 6, (0.5, 1.), [True, True, True, False, False, False]),
    (100, 6, (0., 0.2), [False] * 5 + [True]),
    (100, 6, (1., 1.), [True] + [False] * 5),                # closed at both ends: u = 99 / 99
    (1000, 4, (0.25, 0.75), [False, True, True, False]),     # times 999 749 499 249: u = 1 .7497 .4995 .2492
    (10, 10, (0.3, 0.3), [False] * 10),                      # times 9 .. 0: 3 / 9 is not 0.3
    (11, 11, (0.3, 0.3), [False] * 7 + [True] + [False] * 3),  # times 10 .. 0: 3 / 10 is
)
NOTHING = (0.9, 0.95)    # at T = 100, S = 6: guides no entry


def rows_ref(keep, B, extra, guided, null_side):
    """the contract of dmh_rows_gated -> [n, row_0 .. row_{n-1}].  keep: a list of B flags or None."""
    if not guided:
        return [0] if null_side else [B] + list(range(B))
    kept = [b for b in range(B) if null_side or keep is None or keep[b]]
    rows = kept + list(range(B, B + extra))
    return [len(rows)] + rows


def keep_masks(B):
    """all-0, all-1, mixed (where B allows one) and None"""
    out = [('zeros', [0] * B), ('ones', [1] * B), ('none', None)]
    if B > 1:
        out.append(('mixed', [(b + 1) % 2 if B == 3 else int(b in (1, 2)) for b in range(B)]))
    return out


def row_cases():
    """[(name, B, keep, extra, null_side)]: B in {1, 3, 5} x the masks x extra in {0, B} x both sides"""
    out = []
    for B in (1, 3, 5):
        for (kname, keep), extra, null_side in itertools.product(keep_masks(B), (0, B), (False, True)):
            out.append((f'B{B}-{kname}-extra{extra}-{"null" if null_side else "cond"}', B, keep, extra, null_side))
    return out
