"""What the tests of sample_from share (CPU statements; include/dmhomo_hip_start.h has the definition): the start image with
one fp32 operation per line, the strength -> first entry map restated independently of dmhomo_amd/schedule.py, the shapes of the
kernel tests and their inputs."""
import math
from fractions import Fraction

import torch

# (B, per_sample) of the kernel tests: per % 4 != 0 (the scalar path), the tiny model's row, 8 workgroups per sample each looping
# twice plus a tail quad ((16388 / 4 = 4097 quads over 8 * 256 threads), the B >= 512 arm (one workgroup per sample, looping)
SHAPES = ((1, 1), (3, 3), (3, 5), (3, 210), (3, 1536), (64, 16388), (600, 2052))
OFFSETS = (0, 1, 2, 3)                                       # floats past a 16-byte boundary


def f32(v):
    """the fp32 value of a Python float, as a 0-dim tensor"""
    return torch.tensor(float(v), dtype=torch.float32)


def mix32(init01, eps, ca, cb):
    """the start image on the CPU in fp32, one rounding per line (torch's CPU kernels do not contract across calls)"""
    x = init01.to(torch.float32)
    ca32, cb32 = f32(ca), f32(cb)
    k = x * 2
    k = k + (-1)
    a = ca32 * k
    b = cb32 * eps.to(torch.float32)
    return a + b


def entries_run(S, strength):
    """n of the definition, restated without a floor: the largest integer n <= S with n <= S * strength + 1e-9, the right side in
    the same double arithmetic, found by walking up from 0"""
    v = S * float(strength) + 1e-9
    n = 0
    while n + 1 <= S and n + 1 <= v:
        n += 1
    return n


def first_entry(S, strength):
    """k0 = S - n, or None where the call is refused (strength outside (0, 1], not finite, or n == 0)"""
    if isinstance(strength, bool) or not isinstance(strength, (int, float)):
        return None
    s = float(strength)
    if math.isnan(s) or not (0. < s <= 1.):
        return None
    n = entries_run(S, s)
    return None if n == 0 else S - n


def exact_multiple(k, S):
    """the double nearest k / S: the strength a user writes for 'k of S entries'"""
    return float(Fraction(k, S))


def kernel_inputs(B, per, seed):
    """init in [0, 1] with both ends among its values, noise ~ N(0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    init = torch.rand((B, per), generator=gen)
    init.view(-1)[0] = 0.
    init.view(-1)[-1] = 1.
    noise = torch.randn((B, per), generator=gen)
    return init, noise
