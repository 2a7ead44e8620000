"""Tensor-level wrappers of the C ABI (include/dmhomo_hip.h).

PyTorch is used here only to allocate device memory (``torch.empty``) and to carry
pointers; every value is produced by a kernel of libdmhomo_hip.so.  Activations
are NHWC fp32 tensors shaped (B, H, W, C).
"""
import ctypes as C
import math

import os

import torch

from . import _lib
from ._lib import call, ptr, lib

F32 = torch.float32


def _empty(shape, like, dtype=F32):
    return torch.empty(shape, device=like.device, dtype=dtype)


# ------------------------------------------------------------------ weight preparation
def ws_standardize(w, eps=1e-5, out=None):
    """N1: (w - mean_o) * rsqrt(var_o + eps) per output channel (CFG:123-126)."""
    w = w.detach().contiguous()
    out = torch.empty_like(w) if out is None else out
    cout = w.shape[0]
    call('dmh_ws_standardize', ptr(w), ptr(out), cout, w.numel() // cout, float(eps))
    return out


class PackBatch:
    """the weight images of many PackedConvs, made together by ``run()`` — now and again after every update of the weights
    (a training step re-packs after every optimiser step): ``pre`` (closures that assemble a weight from the parameters:
    padded, re-indexed, standardised), then ONE table for dmh_pack_conv_weights_multi (three kernel phases over all plain
    stride-1 1x1 / 3x3 images), then ``specials`` (the images that need launches of their own).  Buffers and source
    pointers are fixed when the batch is built; ``run()`` is graph-capturable."""

    def __init__(self):
        self.jobs, self.pre, self.specials, self._keep, self._arr = [], [], [], [], None

    def add(self, src, ws, wpack, cout, c0, c1, kh, transposed):
        self.jobs.append(_lib.DmhPackJob(ptr(src), ptr(ws), ptr(wpack), cout, c0, c1, kh, int(transposed)))
        self._keep.append((src, ws, wpack))
        self._arr = None

    def run(self, eps=1e-5):
        for f in self.pre:
            f()
        if self.jobs:
            if self._arr is None:
                self._arr = (_lib.DmhPackJob * len(self.jobs))(*self.jobs)
            call('dmh_pack_conv_weights_multi', C.cast(self._arr, C.c_void_p), len(self.jobs), float(eps))
        for f in self.specials:
            f()


def f16x3_default():
    """the fp16-piece kernels (DMH_CONV3_VARIANT unset or 9) serve the 1x1 / 3x3 convolutions"""
    return os.environ.get('DMH_CONV3_VARIANT', '9') == '9'


class PackedConv:
    """a conv weight in dmh_conv2d's tile-major layout + its geometry.  How the image is made is decided here and nowhere
    else; every route goes through a PackBatch (``batch``; a private one, run before the constructor returns, when None):
    the plain stride-1 1x1 / 3x3 images of the default kernels are jobs of its table, every other form (7x7, 4x4 and
    2x2 / stride 2, sub-pixel Upsample + 3x3, all of them under the exact-fp32 DMH_CONV3_VARIANT 0 / 6) registers ``repack``
    with it.  tests/test_gpu_weight_image.py pins the table's images to the single launches' and to the documented layout.
    With a ``batch`` the image exists after ``batch.run()``; ``w_oihw``'s storage must stay where it is.
    ws_from (the raw weight): the image is that of its standardised form, which the batch also writes into ``w_oihw``.
    transposed: ``w_oihw`` is the weight (c0, Cout, k, k) of a stride-1 conv and the image is that of its DATA-GRADIENT conv
    (taps flipped, O and I exchanged: by index arithmetic in the table's kernels, through a copy otherwise)."""
    __slots__ = ('wpack', 'bias', 'cout', 'c0', 'c1', 'k', 'stride', 'upsample2', '_w', '_up2')

    def __init__(self, w_oihw, bias, c0, c1=0, stride=1, upsample2=0, subpixel=True, batch=None, ws_from=None,
                 transposed=False):
        w = w_oihw.detach()
        assert w.is_contiguous()
        cout, cin, kh, kw = w.shape
        if transposed:
            cout, cin = cin, cout
        assert cin == c0 + c1 and kh == kw and not (transposed and (c1 or stride != 1 or upsample2)), (w.shape, c0, c1)
        self._w = w
        n_up2 = lib().dmh_conv_up2_pack_floats(cout, c0) if (upsample2 and kh == 3 and c1 == 0 and subpixel) else -1
        self._up2 = n_up2 > 0
        if self._up2:                     # Upsample + conv3x3 as four 2x2 sub-pixel convs (upsample2 = 2)
            self.wpack = _empty((n_up2,), w)
            upsample2 = 2
        else:
            self.wpack = _empty((lib().dmh_conv_pack_floats(cout, c0, c1, kh, kw),), w)
        self.bias = None if bias is None else bias.detach().contiguous()
        self.cout, self.c0, self.c1, self.k, self.stride, self.upsample2 = cout, c0, c1, kh, stride, upsample2
        own = batch is None
        if own:
            batch = PackBatch()
        src = None if ws_from is None else ws_from.detach()
        assert src is None or (src.is_contiguous() and src.shape == w.shape)
        if kh in (1, 3) and stride == 1 and not upsample2 and f16x3_default():
            batch.add(w if src is None else src, None if src is None else w, self.wpack, cout, c0, c1, kh, transposed)
        else:
            if src is not None:
                batch.pre.append(lambda: ws_standardize(src, out=w))
            if transposed:
                self._w = wt = _empty((cout, cin, kh, kw), w)
                batch.pre.append(lambda: wt.copy_(w.flip(2, 3).transpose(0, 1)))
            batch.specials.append(self.repack)
        if own:
            batch.run()

    def repack(self):
        """(re)make an image that has launches of its own from the weight tensor's current values"""
        if self._up2:
            call('dmh_pack_conv_weight_up2', ptr(self._w), ptr(self.wpack), self.cout, self.c0)
        else:
            call('dmh_pack_conv_weight', ptr(self._w), ptr(self.wpack), self.cout, self.c0, self.c1, self.k, self.k)


def conv_out_hw(pc, h, w):
    if pc.upsample2:
        return h * 2, w * 2
    if pc.stride == 2:
        return h // 2, w // 2
    return h, w


# launch timing of the conv kernels with HIP events on the launch stream (bench.py's roofline leg):
# when a list, every dmh_conv2d launch appends (start_event, end_event, k, stride, B, Hout, Wout, Cin, Cout, upsample2,
# has GroupNorm+SiLU prologue)
CONV_LOG = None


def rows_from_keep(keep, extra=0):
    """the active-row list of a classifier-free-guidance pass (include/dmhomo_hip.h, "Row subsets"): int32 (1 + B + extra,)
    = [n, the rows with keep != 0 ..., B .. B + extra - 1, (unused)]; every batched wrapper below takes it as ``rows=``."""
    B = keep.shape[0]
    rows = torch.empty((1 + B + extra,), device=keep.device, dtype=torch.int32)
    call('dmh_rows_from_keep', ptr(keep, torch.uint8), B, int(extra), ptr(rows, torch.int32))
    return rows


def _rows(rows):
    return ptr(rows, torch.int32)


def conv2d(pc, src0, src1=None, in_coef=None, res=None, res_coef=None, want_stats=False, in_bound=None, final=None,
           keep_out=True, pixel_stats=False, eps=1e-5, fin_out=None, rows=None):
    """K1/K2.  src0 (B,H,W,C0) [+ src1 (B,H,W,C1) = fused channel concat]. Returns out or (out, stats).
    in_bound (B, k), with in_coef: upper bounds of the prologue's |a*x+b| per sample (gn_finalize(want_bound=True)).
    final = (w (n, Cout), b (n,) or None), 1x1 convs with Cout <= 64 only: also apply that pointwise projection to every
    finished output pixel and return (out, y) with y (B, n, H, W) NCHW — ``final_conv_nchw(out, w, b)`` without the second
    pass over ``out`` (DmhConv.fin_*); keep_out=False: ``out`` itself is not stored (returned as None).
    fin_out: where y goes (a contiguous (B, n, H, W) tensor, e.g. a row slice of the caller's result) instead of a new tensor.
    pixel_stats (1x1 convs with Cout == 64): return (out, pstats) with pstats (B, H*W, 2) = the channel-LayerNorm (mean, rstd)
    of every output pixel, as ``dmh_pixel_stats(out)`` gives them, for ``linear_attention_fused(..., stats=)``."""
    B, H, W, c0 = src0.shape
    assert c0 == pc.c0 and (pc.c1 == 0) == (src1 is None), (src0.shape, pc.c0, pc.c1)
    if src1 is not None:
        assert src1.shape == (B, H, W, pc.c1), (src1.shape, pc.c1)
    ho, wo = conv_out_hw(pc, H, W)
    assert keep_out or final is not None
    out = _empty((B, ho, wo, pc.cout), src0) if keep_out else None
    fin_w = fin_b = None
    if final is not None:
        fin_w, fin_b = final
        assert fin_w.shape[1] == pc.cout and fin_w.is_contiguous() and not want_stats, (fin_w.shape, pc.cout)
        if fin_out is None:
            fin_out = _empty((B, fin_w.shape[0], ho, wo), src0)
        assert fin_out.shape == (B, fin_w.shape[0], ho, wo) and fin_out.is_contiguous() and fin_out.dtype == F32
    else:
        assert fin_out is None
    pst = None
    if pixel_stats:
        assert final is None and not want_stats and pc.cout == 64 and pc.k == 1, (pc.cout, pc.k)
        pst = _empty((B, ho * wo, 2), src0)
    stats = None
    if want_stats:
        tiles = lib().dmh_conv_tiles(ho, wo, pc.k, pc.stride)
        stats = _empty((B, tiles, pc.cout, 2), src0)
    if res is not None:
        assert res.shape == (B, ho, wo, pc.cout), (res.shape, (B, ho, wo, pc.cout))
    d = _lib.DmhConv(C.sizeof(_lib.DmhConv), ptr(src0), ptr(src1), ptr(pc.wpack), ptr(pc.bias), ptr(in_coef), ptr(res), ptr(res_coef),
                     ptr(out), ptr(stats), B, H, W, pc.c0, pc.c1, pc.cout, pc.k, pc.k, pc.stride, pc.upsample2,
                     ptr(in_bound), 0 if in_bound is None else in_bound.shape[1],
                     0 if fin_w is None else fin_w.shape[0], ptr(fin_w), ptr(fin_b), ptr(fin_out), ptr(pst), float(eps), _rows(rows))
    if CONV_LOG is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call('dmh_conv2d', C.byref(d))
        e1.record()
        CONV_LOG.append((e0, e1, pc.k, pc.stride, B, ho, wo, pc.c0 + pc.c1, pc.cout, pc.upsample2, in_coef is not None))
    else:
        call('dmh_conv2d', C.byref(d))
    if final is not None:
        return out, fin_out
    if pixel_stats:
        return out, pst
    return (out, stats) if want_stats else out


# ------------------------------------------------------------------ normalisation glue
def _ss_arg(ss, B, Cc):
    """(pointer, row stride) of the (scale, shift) rows: ss is None, or a (B, 2C) view with unit column stride"""
    if ss is None:
        return None, 0
    assert ss.stride(1) == 1 and ss.shape[0] == B and ss.shape[1] == 2 * Cc
    return C.c_void_p(ss.data_ptr()), ss.stride(0)


def gn_finalize(stats, gamma, beta, hw, groups, ss=None, eps=1e-5, want_bound=False, rows=None):
    """N2: stats (B,tiles,C,2) -> coef (B,2,C).  ss: (B, >=2C) view whose row b starts with (scale[C], shift[C]).
    want_bound: -> (coef, bound) with bound (B, groups) >= |a*x + b| over each (sample, group): ``conv2d(in_bound=)``."""
    B, tiles, Cc, _ = stats.shape
    coef = _empty((B, 2, Cc), stats)
    ss_ptr, ss_stride = _ss_arg(ss, B, Cc)
    if want_bound:
        bound = _empty((B, groups), stats)
        call('dmh_gn_finalize_bound', ptr(stats), tiles, ptr(gamma), ptr(beta), ss_ptr, ss_stride, ptr(coef), ptr(bound),
             B, Cc, groups, hw, float(eps), _rows(rows))
        return coef, bound
    call('dmh_gn_finalize', ptr(stats), tiles, ptr(gamma), ptr(beta), ss_ptr, ss_stride, ptr(coef), B, Cc, groups,
         hw, float(eps), _rows(rows))
    return coef


# widths whose ResnetBlock epilogue can hand the LayerNorm statistics to the LinearAttention behind it
PIXEL_STATS_FUSABLE = (64, 128, 256)


def gn_silu_residual(y, coef, res, pixel_stats=False, eps=1e-5, rows=None):
    """SiLU(a*y+b) + res.  pixel_stats: also return the (B, H*W, 2) per-pixel (mean, rstd) of the channel LayerNorm of the
    result — what ``dmh_pixel_stats`` would compute from it — for ``linear_attention_fused(..., stats=)``."""
    B, H, W, Cc = y.shape
    out = torch.empty_like(y)
    if pixel_stats:
        stats = _empty((B, H * W, 2), y)
        call('dmh_gn_silu_residual_stats', ptr(y), ptr(coef), ptr(res), ptr(out), ptr(stats), B, H * W, Cc, float(eps),
             _rows(rows))
        return out, stats
    call('dmh_gn_silu_residual', ptr(y), ptr(coef), ptr(res), ptr(out), B, H * W, Cc, _rows(rows))
    return out


def chan_layernorm(x, g, res=None, eps=1e-5, rows=None):
    """N4 (+ optional residual add)."""
    Cc = x.shape[-1]
    out = torch.empty_like(x)
    npix = x.numel() // Cc
    call('dmh_chan_layernorm', ptr(x), ptr(g), ptr(res), ptr(out), npix, Cc, float(eps), _rows(rows), npix // x.shape[0])
    return out


# ------------------------------------------------------------------ attention cores
def linear_attention_core(qkv, scale, rows=None):
    """K3.  qkv (B,H,W,384) -> (B,H,W,128)."""
    B, H, W, c = qkv.shape
    assert c == 384
    n = H * W
    partial = _empty((lib().dmh_linattn_partial_floats(B, n),), qkv)
    ctx = _empty((B, 4, 32, 32), qkv)
    out = _empty((B, H, W, 128), qkv)
    call('dmh_linattn_context', ptr(qkv), ptr(partial), B, n, _rows(rows))
    call('dmh_linattn_merge', ptr(partial), ptr(ctx), B, n, _rows(rows))
    call('dmh_linattn_apply', ptr(qkv), ptr(ctx), ptr(out), B, n, float(scale), _rows(rows))
    return out


class PackedLinAttn:
    """to_qkv weight of a LinearAttention (384, C, 1, 1) packed for the fused kernels (once per weight version)."""

    def __init__(self, w_qkv):
        c = w_qkv.shape[1]
        assert w_qkv.shape[0] == 384 and c % 32 == 0, w_qkv.shape
        w = w_qkv.detach().reshape(384, c).contiguous().float()
        self.c = c
        self.wpack = _empty((lib().dmh_linattn_fused_pack_floats(c),), w)
        call('dmh_linattn_fused_pack', ptr(w), ptr(self.wpack), c)


class PackedLinAttnOut:
    """to_out of a LinearAttention with dim 64: conv weight (64, 128, 1, 1) + bias + the gain of its LayerNorm, packed for
    the fully fused second pass."""

    def __init__(self, w_out, bias, ln_g):
        assert tuple(w_out.shape[:2]) == (64, 128), w_out.shape
        w = w_out.detach().reshape(64, 128).contiguous().float()
        self.wpack = _empty((lib().dmh_linattn_out_pack_floats(),), w)
        call('dmh_linattn_out_pack', ptr(w), ptr(self.wpack))
        self.bias = bias.detach().contiguous().float()
        self.ln_g = ln_g.detach().reshape(-1).contiguous().float()


def linear_attention_fused(x, ln_g, pla, scale, eps=1e-5, out=None, stats=None, rows=None):
    """K3f.  x (B,H,W,C) -> attention core output (B,H,W,128) of LinearAttention(PreNorm-LayerNorm(x)): LayerNorm,
    to_qkv and both attention passes in two kernels, q/k/v never stored.
    With ``out`` (PackedLinAttnOut, C == 64) the second pass also applies to_out, its LayerNorm and the residual:
    returns x + LN(to_out(core)) of shape (B,H,W,64) — the whole Residual(PreNorm(LinearAttention)) block."""
    B, H, W, c = x.shape
    assert c == pla.c
    n = H * W
    if stats is None:     # (the producer of x may have written them already: gn_silu_residual(pixel_stats=True))
        stats = _empty((B, n, 2), x)
        call('dmh_pixel_stats', ptr(x), ptr(stats), B * n, c, float(eps), _rows(rows), n)
    assert stats.shape == (B, n, 2)
    ns = lib().dmh_linattn_fused_splits(B, n)
    partial = _empty((B, ns, 4, 1088), x)
    ctx = _empty((B, 4, 32, 32), x)
    call('dmh_linattn_fused_context', ptr(x), ptr(stats), ptr(ln_g), ptr(pla.wpack), ptr(partial), B, n, c, _rows(rows))
    call('dmh_linattn_merge_n', ptr(partial), ptr(ctx), B, n, ns, _rows(rows))
    if out is not None:
        y = _empty((B, H, W, 64), x)
        call('dmh_linattn_fused_apply_out', ptr(x), ptr(stats), ptr(ln_g), ptr(pla.wpack), ptr(ctx), ptr(out.wpack),
             ptr(out.bias), ptr(out.ln_g), ptr(y), B, n, c, float(scale), float(eps), _rows(rows))
        return y
    o = _empty((B, H, W, 128), x)
    call('dmh_linattn_fused_apply', ptr(x), ptr(stats), ptr(ln_g), ptr(pla.wpack), ptr(ctx), ptr(o), B, n, c,
         float(scale), _rows(rows))
    return o


def attention_core(qkv, scale, rows=None, pert_lo=None):
    """K4.  qkv (B,H,W,384) -> (B,H,W,128).  pert_lo (perturbed-attention guidance, dmh_attention_pag): the physical rows
    >= pert_lo take the identity attention map, their output is v = qkv[..., 256:]; None is dmh_attention as it is."""
    B, H, W, c = qkv.shape
    assert c == 384
    out = _empty((B, H, W, 128), qkv)
    if pert_lo is None:
        call('dmh_attention', ptr(qkv), ptr(out), B, H * W, float(scale), _rows(rows))
        return out
    if isinstance(pert_lo, bool) or not isinstance(pert_lo, int) or not 0 <= pert_lo <= B:
        raise ValueError(f'attention_core: pert_lo = {pert_lo!r} for {B} rows (an int in [0, B])')
    call('dmh_attention_pag', ptr(qkv), ptr(out), B, H * W, float(scale), _rows(rows), pert_lo)
    return out


# ------------------------------------------------------------------ embeddings
ACT = {None: 0, 'silu': 1, 'gelu': 2}


def sinusoidal_embed(t, freq):
    R, dim = t.shape[0], freq.shape[0] * 2
    out = _empty((R, dim), freq)
    call('dmh_sinusoidal_embed', ptr(t, torch.int64), ptr(freq), ptr(out), R, dim)
    return out


def fourier_embed(t, weights):
    """RandomOrLearnedSinusoidalPosEmb CFG:185-190: (R,) int64, (half,) -> (R, 2*half + 1)"""
    R, half = t.shape[0], weights.shape[0]
    out = _empty((R, 2 * half + 1), weights)
    call('dmh_fourier_embed', ptr(t, torch.int64), ptr(weights), ptr(out), R, half)
    return out


def class_embed(classes, keep, table, null_emb):
    R, dim = classes.shape[0], table.shape[1]
    out = _empty((R, dim), table)
    call('dmh_class_embed', ptr(classes, torch.int64), ptr(keep, torch.uint8), ptr(table), ptr(null_emb), ptr(out), R,
         dim, table.shape[0])
    return out


def linear(x, wt, bias, act_in=None, act_out=None, out=None):
    """y = act_out(act_in(x) @ wt + bias); wt is W^T (in, out). x / out may be column slices (unit inner stride)."""
    R, in_dim = x.shape
    out_dim = wt.shape[1]
    assert wt.shape[0] == in_dim and x.stride(1) == 1
    if out is None:
        out = _empty((R, out_dim), wt)
    assert out.shape == (R, out_dim) and out.stride(1) == 1
    call('dmh_linear', C.c_void_p(x.data_ptr()), x.stride(0), ptr(wt), ptr(bias), C.c_void_p(out.data_ptr()),
         out.stride(0), R, in_dim, out_dim, ACT[act_in], ACT[act_out])
    return out


def ss_gather(T, Ct, bias, cursor, classes, keep, out=None):
    """(scale, shift) rows of a replayed denoise step from the tables of ``UnetEngine.ss_tables``:
    out[b] = (T[cursor] + Ct[keep[b] ? classes[b] : last row]) + bias — bitwise ``linear`` over the full embedding."""
    B, N = classes.shape[0], T.shape[1]
    if out is None:
        out = _empty((B, N), T)
    assert out.shape == (B, N) and out.is_contiguous() and Ct.shape[1] == N and bias.shape == (N,)
    call('dmh_ss_gather', ptr(T), ptr(Ct), ptr(bias), ptr(cursor, torch.int32), ptr(classes, torch.int64),
         ptr(keep, torch.uint8), Ct.shape[0] - 1, ptr(out), B, N, T.shape[0])
    return out


# ------------------------------------------------------------------ sampler glue
def assemble_input(a, b=None, m=None, reps=1, cpad=None, out=None):
    """(B,Ca,H,W) [+ (B,Cb,H,W) * (B,1,H,W)] NCHW -> NHWC (reps*B, H, W, cpad), zero padded (into ``out`` if given)."""
    B, ca, H, W = a.shape
    cb = 0 if b is None else b.shape[1]
    if cpad is None:
        cpad = (ca + cb + 3) // 4 * 4
    if out is None:
        out = _empty((reps * B, H, W, cpad), a)
    elif tuple(out.shape) != (reps * B, H, W, cpad):
        raise ValueError(f'assemble_input: out has shape {tuple(out.shape)}, expected {(reps * B, H, W, cpad)}')
    call('dmh_assemble_input', ptr(a), ca, ptr(b), cb, ptr(m), ptr(out), B, reps, H * W, cpad)
    return out


def uncond_input(x, x_self_cond, self_condition, cpad, out=None):
    """the network input of ddpm.Unet (DDP:408-411), NHWC: cat((x_self_cond, x)) when the model self-conditions — zeros for a
    self-condition that is not given — else x alone.  x: contiguous fp32 (B,C,H,W)."""
    if not self_condition:
        return assemble_input(x, None, None, cpad=cpad, out=out)
    sc = torch.zeros_like(x) if x_self_cond is None else x_self_cond.to(F32).contiguous()
    return assemble_input(sc, x, None, cpad=cpad, out=out)


def final_conv_nchw(x, w, bias):
    R, H, W, Cc = x.shape
    cout = w.shape[0]
    out = _empty((R, cout, H, W), x)
    call('dmh_final_conv_nchw', ptr(x), ptr(w), ptr(bias), ptr(out), R, H * W, Cc, cout)
    return out


OBJECTIVE = {'pred_noise': 0, 'pred_x0': 1, 'pred_v': 2}
MODE_DDIM, MODE_LAST, MODE_DDPM, MODE_MULTISTEP = 0, 1, 2, 3


def sampler_step(step, model_cond, model_null, x, noise, want_x_start=True, want_pred_noise=False, keep=None):
    """keep (B,) uint8, with model_null: rows with keep == 0 take model_null as their conditional logits (rows the conditional
    pass did not compute: Unet.dedup_dropped_rows)"""
    img = torch.empty_like(x)
    xs = torch.empty_like(x) if want_x_start else None
    pn = torch.empty_like(x) if want_pred_noise else None
    call('dmh_sampler_step', C.byref(step), ptr(model_cond), ptr(model_null), ptr(x), ptr(noise), ptr(img), ptr(xs),
         ptr(pn), x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img, xs, pn


def step_table(steps, times, device):
    """device tables of a replayed sampling loop: steps (list of DmhStep, host-computed) -> (uint8 tensor holding the
    packed structs, int64 times, int32 cursor, one-struct uint8 'current' buffer)."""
    n = len(steps)
    # the kernels read these entries from device memory and cannot validate them at launch: do it here
    if n < 1 or len(times) != n:
        raise ValueError(f'step_table: {n} steps, {len(times)} times')
    for i, st in enumerate(steps):
        if st.objective not in (0, 1, 2) or st.mode not in (MODE_DDIM, MODE_LAST, MODE_DDPM, MODE_MULTISTEP):
            raise ValueError(f'step_table: entry {i} has objective {st.objective} / mode {st.mode}')
        if (st.mode == MODE_LAST) != (i == n - 1) and st.mode != MODE_DDPM:
            raise ValueError(f'step_table: entry {i} of {n} has mode {st.mode}: MODE_LAST belongs to the last entry only')
    sz = C.sizeof(_lib.DmhStep)
    arr = (_lib.DmhStep * n)(*steps)
    raw = torch.frombuffer(bytearray(C.string_at(C.addressof(arr), n * sz)), dtype=torch.uint8).clone()
    table = raw.to(device)
    tt = torch.tensor(list(times), dtype=torch.int64).to(device)
    cursor = torch.zeros((1,), dtype=torch.int32, device=device)
    cur = torch.zeros((sz,), dtype=torch.uint8, device=device)
    return table, tt, cursor, cur


def sampler_seek(cursor, k, table, times, cur, tcond):
    """k >= 0: cursor = k; k < 0: cursor += 1 (clamped); cur = table[cursor]; tcond[:] = times[cursor]."""
    call('dmh_sampler_seek', ptr(cursor, torch.int32), int(k), ptr(table, torch.uint8), ptr(times, torch.int64),
         times.shape[0], ptr(cur, torch.uint8), ptr(tcond, torch.int64), tcond.shape[0])


def sampler_step_dev(cur, model_cond, model_null, x, noise, out=None, keep=None):
    """sampler_step with its DmhStep in device memory (``cur`` of step_table); out may be x (in place)."""
    img = torch.empty_like(x) if out is None else out
    call('dmh_sampler_step_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(x), ptr(noise), ptr(img),
         None, None, x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img


def sampler_step_ddp_dev(cur, cursor, draws, model_out, img, noise=None, sample_ids=None, state=None, x_start=None, xin=None,
                         self_cond=False):
    """the replayed step of the unconditional loop in one launch (dmh_sampler_step_ddp_dev), in place on img (B,C,H,W):
    entry ``cur`` of step_table, its noise from the keyed generator (sample_ids + state) or ``noise`` when draws[cursor] != 0,
    x_start (B,C,H,W) if given, and the next step's network input ``xin`` (B,H,W,cpad) — cat(x_start, img) with self_cond,
    img without — if given."""
    B, Cc, H, W = img.shape
    for t in (model_out, noise, x_start):
        if t is not None and tuple(t.shape) != (B, Cc, H, W):
            raise ValueError(f'sampler_step_ddp_dev: {tuple(t.shape)} against img {(B, Cc, H, W)}')
    cin = Cc * (2 if self_cond else 1)
    if xin is not None:
        if xin.dim() != 4 or tuple(xin.shape[:3]) != (B, H, W):
            raise ValueError(f'sampler_step_ddp_dev: xin {tuple(xin.shape)} against img {(B, Cc, H, W)}')
        cpad = xin.shape[3]
    else:
        cpad = (cin + 3) // 4 * 4
    if sample_ids is not None and sample_ids.shape[0] < B:
        raise ValueError(f'sampler_step_ddp_dev: {sample_ids.shape[0]} sample ids for {B} rows')
    call('dmh_sampler_step_ddp_dev', ptr(cur, torch.uint8), ptr(cursor, torch.int32), ptr(draws, torch.int32), ptr(model_out),
         ptr(img), ptr(noise), ptr(sample_ids, torch.int64), ptr(state, torch.int64), ptr(x_start), ptr(xin), B, Cc, H * W, cpad,
         int(bool(self_cond)))
    return img


def sampler_step_ms(step, model_cond, model_null, x, hist, out=None, want_x_start=False, keep=None):
    """one step of the multistep solver (dmh_sampler_step_ms): MODE_MULTISTEP or MODE_LAST, no noise; ``hist`` (x's shape) is
    the previous step's x_start, read when the entry's c2 != 0 and overwritten with this step's.  out may be x (in place).
    -> (img, x_start or None)"""
    if tuple(hist.shape) != tuple(x.shape):
        raise ValueError(f'sampler_step_ms: hist {tuple(hist.shape)} against x {tuple(x.shape)}')
    img = torch.empty_like(x) if out is None else out
    xs = torch.empty_like(x) if want_x_start else None
    call('dmh_sampler_step_ms', C.byref(step), ptr(model_cond), ptr(model_null), ptr(x), ptr(hist), ptr(img), ptr(xs),
         x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img, xs


def sampler_step_ms_dev(cur, model_cond, model_null, x, hist, out=None, x_start=None, keep=None):
    """sampler_step_ms with its DmhStep in device memory (``cur`` of step_table); out may be x (in place)."""
    if tuple(hist.shape) != tuple(x.shape):
        raise ValueError(f'sampler_step_ms_dev: hist {tuple(hist.shape)} against x {tuple(x.shape)}')
    img = torch.empty_like(x) if out is None else out
    call('dmh_sampler_step_ms_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(x), ptr(hist), ptr(img),
         ptr(x_start), x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img


def sampler_step_ddp_ms_dev(cur, cursor, model_out, img, hist, x_start=None, xin=None, self_cond=False):
    """the multistep solver's replayed step of the unconditional loop in one launch (dmh_sampler_step_ddp_ms_dev), in place on
    img (B,C,H,W): entry ``cur`` of step_table, ``hist`` as sampler_step_ms, x_start and the next step's network input ``xin``
    as sampler_step_ddp_dev."""
    B, Cc, H, W = img.shape
    for t in (model_out, hist, x_start):
        if t is not None and tuple(t.shape) != (B, Cc, H, W):
            raise ValueError(f'sampler_step_ddp_ms_dev: {tuple(t.shape)} against img {(B, Cc, H, W)}')
    cin = Cc * (2 if self_cond else 1)
    if xin is not None:
        if xin.dim() != 4 or tuple(xin.shape[:3]) != (B, H, W):
            raise ValueError(f'sampler_step_ddp_ms_dev: xin {tuple(xin.shape)} against img {(B, Cc, H, W)}')
        cpad = xin.shape[3]
    else:
        cpad = (cin + 3) // 4 * 4
    call('dmh_sampler_step_ddp_ms_dev', ptr(cur, torch.uint8), ptr(cursor, torch.int32), ptr(model_out), ptr(img), ptr(hist),
         ptr(x_start), ptr(xin), B, Cc, H * W, cpad, int(bool(self_cond)))
    return img


def row_quantile_abs(x, k, frac, floor=0., out=None):
    """(B, ...) fp32 -> (B,): max(floor, quantile of |x[b]| at rank k + frac, linearly interpolated) — an exact selection
    (dmh_row_quantile_abs); a row that holds a NaN answers NaN.  (k, frac): ScheduleHost._quantile_rank(p, n)."""
    B = x.shape[0]
    if out is None:
        out = _empty((B,), x)
    elif tuple(out.shape) != (B,):
        raise ValueError(f'row_quantile_abs: out {tuple(out.shape)} for {B} rows')
    call('dmh_row_quantile_abs', ptr(x), ptr(out), B, x.numel() // max(B, 1), int(k), float(frac), float(floor))
    return out


def _threshold_buffers(who, x, x0_raw, thr):
    x0_raw = torch.empty_like(x) if x0_raw is None else x0_raw
    thr = _empty((x.shape[0],), x) if thr is None else thr
    if tuple(x0_raw.shape) != tuple(x.shape) or tuple(thr.shape) != (x.shape[0],):
        raise ValueError(f'{who}: x0_raw {tuple(x0_raw.shape)} / thr {tuple(thr.shape)} against x {tuple(x.shape)}')
    return x0_raw, thr


def sampler_threshold(step, model_cond, model_null, x, k, frac, keep=None, x0_raw=None, thr=None):
    """the dynamic threshold of one denoise step (dmh_sampler_threshold): x0_raw = the step's x_start before any clamp (guided
    blend with ``keep`` as sampler_step, objective branch), thr[b] = max(1, quantile of |x0_raw[b]| at rank k + frac).
    -> (thr, x0_raw)"""
    x0_raw, thr = _threshold_buffers('sampler_threshold', x, x0_raw, thr)
    call('dmh_sampler_threshold', C.byref(step), ptr(model_cond), ptr(model_null), ptr(x), ptr(keep, torch.uint8), ptr(x0_raw),
         ptr(thr), x.shape[0], x.numel() // x.shape[0], int(k), float(frac))
    return thr, x0_raw


def sampler_threshold_dev(cur, model_cond, model_null, x, k, frac, keep=None, x0_raw=None, thr=None):
    """sampler_threshold with its DmhStep in device memory (``cur`` of step_table)"""
    x0_raw, thr = _threshold_buffers('sampler_threshold_dev', x, x0_raw, thr)
    call('dmh_sampler_threshold_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(x), ptr(keep, torch.uint8),
         ptr(x0_raw), ptr(thr), x.shape[0], x.numel() // x.shape[0], int(k), float(frac))
    return thr, x0_raw


def _step_thr_shapes(who, x, noise, hist, thr):
    for t in (noise, hist):
        if t is not None and tuple(t.shape) != tuple(x.shape):
            raise ValueError(f'{who}: {tuple(t.shape)} against x {tuple(x.shape)}')
    if tuple(thr.shape) != (x.shape[0],):
        raise ValueError(f'{who}: thr {tuple(thr.shape)} for {x.shape[0]} rows')


def sampler_step_thr(step, model_cond, model_null, x, noise, hist, thr, out=None, want_x_start=False, keep=None):
    """sampler_step / sampler_step_ms with a threshold per row (dmh_sampler_step_thr): where the entry clips, x_start =
    clamp(x0_raw, -thr[b], thr[b]) / thr[b].  ``noise`` for a DDIM entry, ``hist`` for a multistep entry (the other None).
    out may be x (in place).  -> (img, x_start or None)"""
    _step_thr_shapes('sampler_step_thr', x, noise, hist, thr)
    img = torch.empty_like(x) if out is None else out
    xs = torch.empty_like(x) if want_x_start else None
    call('dmh_sampler_step_thr', C.byref(step), ptr(model_cond), ptr(model_null), ptr(x), ptr(noise), ptr(hist), ptr(thr),
         ptr(img), ptr(xs), x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img, xs


def sampler_step_thr_dev(cur, model_cond, model_null, x, noise, hist, thr, out=None, x_start=None, keep=None):
    """sampler_step_thr with its DmhStep in device memory (``cur`` of step_table); out may be x (in place)."""
    _step_thr_shapes('sampler_step_thr_dev', x, noise, hist, thr)
    img = torch.empty_like(x) if out is None else out
    call('dmh_sampler_step_thr_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(x), ptr(noise), ptr(hist),
         ptr(thr), ptr(img), ptr(x_start), x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img


def guidance_splits(B, n):
    """workgroups per row of the guidance factor's first pass (dmh_guidance_splits): a pure function of (B, n)"""
    s = int(_lib.lib().dmh_guidance_splits(int(B), int(n)))
    if s < 1:
        raise ValueError(f'guidance_splits: B = {B} rows of n = {n} elements')
    return s


def guidance_workspace(x):
    """the fp64 workspace dmh_guidance_factor[_dev] asks for with logits of x's shape (B, ...): 4 doubles per (row, split)"""
    B = x.shape[0]
    return torch.empty((4 * B * guidance_splits(B, x.numel() // B),), device=x.device, dtype=torch.float64)


def _guidance_buffers(who, model_cond, model_null, ws, gfac):
    if model_null is None or tuple(model_null.shape) != tuple(model_cond.shape):
        raise ValueError(f'{who}: model_null {None if model_null is None else tuple(model_null.shape)} against model_cond '
                         f'{tuple(model_cond.shape)} (the factor needs the null pass)')
    B = model_cond.shape[0]
    ws = guidance_workspace(model_cond) if ws is None else ws
    gfac = _empty((B,), model_cond) if gfac is None else gfac
    need = 4 * B * guidance_splits(B, model_cond.numel() // B)
    if ws.numel() < need or tuple(gfac.shape) != (B,):
        raise ValueError(f'{who}: ws of {ws.numel()} doubles ({need} needed) / gfac {tuple(gfac.shape)} for {B} rows')
    return ws, gfac


def guidance_factor(step, model_cond, model_null, phi, keep=None, ws=None, gfac=None):
    """the guidance-rescale factor of one denoise step (dmh_guidance_factor): gfac[b] = 1 + phi * (std(cond[b]) / std(blend[b])
    - 1) with blend = null + (cond - null) * step.cond_scale and ``keep`` as sampler_step; fp64 moments, bitwise repeatable.
    ws: guidance_workspace(model_cond).  -> gfac (B,)"""
    ws, gfac = _guidance_buffers('guidance_factor', model_cond, model_null, ws, gfac)
    call('dmh_guidance_factor', C.byref(step), ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), float(phi),
         ptr(ws, torch.float64), ptr(gfac), model_cond.shape[0], model_cond.numel() // model_cond.shape[0])
    return gfac


def guidance_factor_dev(cur, model_cond, model_null, phi, keep=None, ws=None, gfac=None):
    """guidance_factor with its DmhStep in device memory (``cur`` of step_table)"""
    ws, gfac = _guidance_buffers('guidance_factor_dev', model_cond, model_null, ws, gfac)
    call('dmh_guidance_factor_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), float(phi),
         ptr(ws, torch.float64), ptr(gfac), model_cond.shape[0], model_cond.numel() // model_cond.shape[0])
    return gfac


def _gfac_shape(who, x, gfac):
    if tuple(gfac.shape) != (x.shape[0],):
        raise ValueError(f'{who}: gfac {tuple(gfac.shape)} for {x.shape[0]} rows')


def sampler_threshold_gr(step, model_cond, model_null, x, gfac, k, frac, keep=None, x0_raw=None, thr=None):
    """sampler_threshold on the rescaled blend (dmh_sampler_threshold_gr): gfac (B,) from guidance_factor.  -> (thr, x0_raw)"""
    x0_raw, thr = _threshold_buffers('sampler_threshold_gr', x, x0_raw, thr)
    _gfac_shape('sampler_threshold_gr', x, gfac)
    call('dmh_sampler_threshold_gr', C.byref(step), ptr(model_cond), ptr(model_null), ptr(x), ptr(keep, torch.uint8), ptr(gfac),
         ptr(x0_raw), ptr(thr), x.shape[0], x.numel() // x.shape[0], int(k), float(frac))
    return thr, x0_raw


def sampler_threshold_gr_dev(cur, model_cond, model_null, x, gfac, k, frac, keep=None, x0_raw=None, thr=None):
    """sampler_threshold_gr with its DmhStep in device memory (``cur`` of step_table)"""
    x0_raw, thr = _threshold_buffers('sampler_threshold_gr_dev', x, x0_raw, thr)
    _gfac_shape('sampler_threshold_gr_dev', x, gfac)
    call('dmh_sampler_threshold_gr_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(x), ptr(keep, torch.uint8),
         ptr(gfac), ptr(x0_raw), ptr(thr), x.shape[0], x.numel() // x.shape[0], int(k), float(frac))
    return thr, x0_raw


def _step_gr_shapes(who, x, noise, hist, thr, gfac):
    for t in (noise, hist):
        if t is not None and tuple(t.shape) != tuple(x.shape):
            raise ValueError(f'{who}: {tuple(t.shape)} against x {tuple(x.shape)}')
    if thr is not None and tuple(thr.shape) != (x.shape[0],):
        raise ValueError(f'{who}: thr {tuple(thr.shape)} for {x.shape[0]} rows')
    _gfac_shape(who, x, gfac)


def sampler_step_gr(step, model_cond, model_null, x, noise, hist, thr, gfac, out=None, want_x_start=False, keep=None):
    """sampler_step / sampler_step_ms / sampler_step_thr on the rescaled blend (dmh_sampler_step_gr): the guided logits of row b
    times gfac[b], the step behind them unchanged.  ``noise`` for a DDIM entry, ``hist`` for a multistep entry (the other
    None); ``thr`` None: the static clamp, else the threshold per row.  out may be x (in place).  -> (img, x_start or None)"""
    _step_gr_shapes('sampler_step_gr', x, noise, hist, thr, gfac)
    img = torch.empty_like(x) if out is None else out
    xs = torch.empty_like(x) if want_x_start else None
    call('dmh_sampler_step_gr', C.byref(step), ptr(model_cond), ptr(model_null), ptr(x), ptr(noise), ptr(hist), ptr(thr),
         ptr(gfac), ptr(img), ptr(xs), x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img, xs


def sampler_step_gr_dev(cur, model_cond, model_null, x, noise, hist, thr, gfac, out=None, x_start=None, keep=None):
    """sampler_step_gr with its DmhStep in device memory (``cur`` of step_table); out may be x (in place)."""
    _step_gr_shapes('sampler_step_gr_dev', x, noise, hist, thr, gfac)
    img = torch.empty_like(x) if out is None else out
    call('dmh_sampler_step_gr_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(x), ptr(noise), ptr(hist),
         ptr(thr), ptr(gfac), ptr(img), ptr(x_start), x.numel(), ptr(keep, torch.uint8), x.numel() // x.shape[0])
    return img


def _interval_tables(who, cursor, guided):
    if tuple(cursor.shape) != (1,) or guided.dim() != 1 or guided.shape[0] < 1:
        raise ValueError(f'{who}: cursor {tuple(cursor.shape)} / guided {tuple(guided.shape)} (one cursor, one flag per entry)')
    return ptr(cursor, torch.int32), ptr(guided, torch.uint8), guided.shape[0]


def rows_gated(keep, B, extra, cursor, guided, null_side=False, rows=None):
    """rows_from_keep behind the guidance interval's flag guided[cursor] (dmh_rows_gated; cursor, guided: device tensors of a
    replayed loop): int32 (1 + B + extra,).  A guided entry: the rows with keep != 0 (all B where keep is None, or on the
    null-only side), then B .. B + extra - 1; an unguided entry: all B rows and no extras, or — null_side — none.
    rows: the buffer to write (else a new one); the words behind rows[0 .. n] are left as they are."""
    B, extra = int(B), int(extra)
    if keep is not None and tuple(keep.shape) != (B,):
        raise ValueError(f'rows_gated: keep {tuple(keep.shape)} for {B} rows')
    pc, pg, S = _interval_tables('rows_gated', cursor, guided)
    if rows is None:
        rows = torch.empty((1 + max(B, 0) + max(extra, 0),), device=guided.device, dtype=torch.int32)
    elif tuple(rows.shape) != (1 + B + extra,):
        raise ValueError(f'rows_gated: rows {tuple(rows.shape)} for {B} rows and {extra} extras')
    call('dmh_rows_gated', ptr(keep, torch.uint8), B, extra, pc, pg, S, int(bool(null_side)), ptr(rows, torch.int32))
    return rows


def guidance_gate(cursor, guided, cond, null):
    """the gate behind the network of a replayed step under a guidance interval (dmh_guidance_gate): at an unguided entry
    (guided[cursor] == 0) null <- cond bit for bit, so that every step kernel behind it does the unguided step; at a guided
    entry nothing is touched.  -> null"""
    if tuple(null.shape) != tuple(cond.shape):
        raise ValueError(f'guidance_gate: null {tuple(null.shape)} against cond {tuple(cond.shape)}')
    pc, pg, S = _interval_tables('guidance_gate', cursor, guided)
    call('dmh_guidance_gate', pc, pg, S, ptr(cond), ptr(null), cond.numel())
    return null


def apg_splits(B, n):
    """workgroups per row of the first pass of the APG coefficients (dmh_apg_splits): a pure function of (B, n)"""
    s = int(_lib.lib().dmh_apg_splits(int(B), int(n)))
    if s < 1:
        raise ValueError(f'apg_splits: B = {B} rows of n = {n} elements')
    return s


def apg_workspace(x):
    """the fp64 workspace dmh_apg_coef[_dev] asks for with logits of x's shape (B, ...): 3 doubles per (row, split)"""
    B = x.shape[0]
    return torch.empty((3 * B * apg_splits(B, x.numel() // B),), device=x.device, dtype=torch.float64)


def _apg_shapes(who, model_cond, model_null, run):
    if model_null is None or tuple(model_null.shape) != tuple(model_cond.shape):
        raise ValueError(f'{who}: model_null {None if model_null is None else tuple(model_null.shape)} against model_cond '
                         f'{tuple(model_cond.shape)} (the projection needs the null pass)')
    if run is not None and tuple(run.shape) != tuple(model_cond.shape):
        raise ValueError(f'{who}: run {tuple(run.shape)} against model_cond {tuple(model_cond.shape)}')


def _apg_buffers(who, model_cond, model_null, beta, run, ws, coef):
    _apg_shapes(who, model_cond, model_null, run)
    if (run is not None) != (float(beta) != 0.):
        raise ValueError(f'{who}: run is {"given" if run is not None else "None"} with beta = {beta!r} (the running average goes '
                         f'with beta != 0, and only with it)')
    B = model_cond.shape[0]
    ws = apg_workspace(model_cond) if ws is None else ws
    coef = _empty((B, 2), model_cond) if coef is None else coef
    need = 3 * B * apg_splits(B, model_cond.numel() // B)
    if ws.numel() < need or tuple(coef.shape) != (B, 2):
        raise ValueError(f'{who}: ws of {ws.numel()} doubles ({need} needed) / coef {tuple(coef.shape)} for {B} rows')
    return ws, coef


def apg_coef(step, model_cond, model_null, eta, rho=0., beta=0., keep=None, run=None, ws=None, coef=None):
    """the coefficients of adaptive projected guidance for one denoise step (dmh_apg_coef; the definition: include/dmhomo_hip.h):
    coef[b] = (A, Cc) with guided = A * c + Cc * d, c the conditional logits (``keep`` as sampler_step), d = c - null, or — beta
    != 0 — the running average ``run`` (model_cond's shape, zero in front of the first step), overwritten in place with d + beta
    * run.  eta in [0, 1] weights the part of d parallel to c, rho >= 0 caps the update's norm per row (0: no cap); only
    step.cond_scale is read.  fp64 sums, bitwise repeatable.  ws: apg_workspace(model_cond).  -> coef (B, 2)"""
    ws, coef = _apg_buffers('apg_coef', model_cond, model_null, beta, run, ws, coef)
    call('dmh_apg_coef', C.byref(step), ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), float(eta), float(rho),
         float(beta), ptr(run), ptr(ws, torch.float64), ptr(coef), model_cond.shape[0], model_cond.numel() // model_cond.shape[0])
    return coef


def apg_coef_dev(cur, model_cond, model_null, eta, rho=0., beta=0., keep=None, run=None, ws=None, coef=None):
    """apg_coef with its DmhStep in device memory (``cur`` of step_table)"""
    ws, coef = _apg_buffers('apg_coef_dev', model_cond, model_null, beta, run, ws, coef)
    call('dmh_apg_coef_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), float(eta), float(rho),
         float(beta), ptr(run), ptr(ws, torch.float64), ptr(coef), model_cond.shape[0], model_cond.numel() // model_cond.shape[0])
    return coef


def apg_apply(model_cond, model_null, coef, keep=None, run=None, out=None):
    """the guided logits of adaptive projected guidance (dmh_apg_apply): A * c + Cc * d with coef (B, 2) of apg_coef and d = ``run``
    where the step keeps a running average (the one apg_coef just wrote), else c - null.  It reads no DmhStep: the same call
    serves the eager and the replayed loop.  out must not be one of the inputs.  The result goes to sampler_step / sampler_step_ms
    / sampler_threshold + sampler_step_thr as model_cond with model_null = None.  -> guided (model_cond's shape)"""
    _apg_shapes('apg_apply', model_cond, model_null, run)
    B = model_cond.shape[0]
    out = torch.empty_like(model_cond) if out is None else out
    if tuple(coef.shape) != (B, 2) or tuple(out.shape) != tuple(model_cond.shape):
        raise ValueError(f'apg_apply: coef {tuple(coef.shape)} / out {tuple(out.shape)} against model_cond {tuple(model_cond.shape)}')
    call('dmh_apg_apply', ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), ptr(run), ptr(coef), ptr(out), B,
         model_cond.numel() // B)
    return out


def _photo_dims(who, x, flow, mask):
    """(B, H, W) of logits (B, 6, H, W) with flow (B, 2, H, W) and mask (B, 1, H, W)"""
    if x.dim() != 4 or x.shape[1] != 6:
        raise ValueError(f'{who}: {tuple(x.shape)} (the image pair is (B, 6, H, W))')
    B, _, H, W = x.shape
    if tuple(flow.shape) != (B, 2, H, W) or tuple(mask.shape) != (B, 1, H, W):
        raise ValueError(f'{who}: flow {tuple(flow.shape)} / mask {tuple(mask.shape)} against {tuple(x.shape)}')
    return B, H, W


def photo_acc(B, H, W, device):
    """the zeroed Q31.32 accumulator of photo_weights / photo_guide for B samples of H x W pixels (dmh_photo_acc_words 64-bit
    words); every call that uses it leaves it zero"""
    n = int(_lib.lib().dmh_photo_acc_words(int(B), int(H), int(W)))
    if n < 1:
        raise ValueError(f'photo_acc: B = {B} samples of {H} x {W} pixels')
    return torch.zeros((n,), device=device, dtype=torch.int64)


def photo_weights(flow, mask, acc=None, out=None):
    """s[b, q] = sum_p mask[b, p] * w_p(q) (dmh_photo_weights): how much mask-weighted bilinear weight of flow_warp(., flow) lands
    on pixel q — the preconditioner of photo_guide, a function of flow (B, 2, H, W) and mask (B, 1, H, W) alone.  Integer
    fixed-point sums: bitwise repeatable.  -> s (B, H, W)"""
    if flow.dim() != 4 or flow.shape[1] != 2 or tuple(mask.shape) != (flow.shape[0], 1) + tuple(flow.shape[2:]):
        raise ValueError(f'photo_weights: flow {tuple(flow.shape)} / mask {tuple(mask.shape)}')
    B, _, H, W = flow.shape
    acc = photo_acc(B, H, W, flow.device) if acc is None else acc
    out = _empty((B, H, W), flow) if out is None else out
    if tuple(out.shape) != (B, H, W) or acc.numel() < B * H * W:
        raise ValueError(f'photo_weights: out {tuple(out.shape)} / acc of {acc.numel()} words for {B} x {H} x {W}')
    call('dmh_photo_weights', ptr(flow), ptr(mask), ptr(acc, torch.int64), ptr(out), B, H, W)
    return out


def _photo_guide_buffers(who, model_cond, model_null, flow, mask, s, acc, out):
    B, H, W = _photo_dims(who, model_cond, flow, mask)
    if model_null is not None and tuple(model_null.shape) != tuple(model_cond.shape):
        raise ValueError(f'{who}: model_null {tuple(model_null.shape)} against model_cond {tuple(model_cond.shape)}')
    out = torch.empty_like(model_cond) if out is None else out
    if tuple(s.shape) != (B, H, W) or tuple(out.shape) != tuple(model_cond.shape) or acc.numel() < 3 * B * H * W:
        raise ValueError(f'{who}: s {tuple(s.shape)} / out {tuple(out.shape)} / acc of {acc.numel()} words against model_cond '
                         f'{tuple(model_cond.shape)}')
    return B, H, W, out


def photo_guide(step, model_cond, model_null, keep, flow, mask, s, w, acc, out=None):
    """the logits of one denoise step after photometric-consistency guidance (dmh_photo_guide; the definition:
    include/dmhomo_hip.h): the guided blend of (model_cond, model_null, keep) as sampler_step reads it — model_null and keep may
    be None — with im1 = x[:, :3] moved towards flow_warp(im2, flow) and im2 = x[:, 3:] moved the transposed way, by lambda / 2
    = w * step.sqrt_ac ** 2 / 2 of the masked residual, the im2 side divided by max(1, s) (``s`` of photo_weights).  acc:
    photo_acc(...), zero before and after.  Only step.cond_scale and step.sqrt_ac are read.  Bitwise repeatable.  The result
    goes to sampler_step / sampler_step_ms / sampler_threshold + sampler_step_thr as model_cond with model_null = None.
    -> guided (model_cond's shape)"""
    B, H, W, out = _photo_guide_buffers('photo_guide', model_cond, model_null, flow, mask, s, acc, out)
    call('dmh_photo_guide', C.byref(step), ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), ptr(flow), ptr(mask), ptr(s),
         float(w), ptr(acc, torch.int64), ptr(out), B, H, W)
    return out


def photo_guide_dev(cur, model_cond, model_null, keep, flow, mask, s, w, acc, out=None):
    """photo_guide with its DmhStep in device memory (``cur`` of step_table)"""
    B, H, W, out = _photo_guide_buffers('photo_guide_dev', model_cond, model_null, flow, mask, s, acc, out)
    call('dmh_photo_guide_dev', ptr(cur, torch.uint8), ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), ptr(flow),
         ptr(mask), ptr(s), float(w), ptr(acc, torch.int64), ptr(out), B, H, W)
    return out


def photo_energy_splits(B, H, W):
    """workgroups per sample of the energy's first pass (dmh_photo_energy_splits): a pure function of (B, H, W)"""
    n = int(_lib.lib().dmh_photo_energy_splits(int(B), int(H), int(W)))
    if n < 1:
        raise ValueError(f'photo_energy_splits: B = {B} samples of {H} x {W} pixels')
    return n


def photo_energy_workspace(x):
    """the fp64 workspace dmh_photo_energy asks for with an image pair of x's shape (B, 6, H, W): one double per (sample, split)"""
    B, _, H, W = x.shape
    return torch.empty((B * photo_energy_splits(B, H, W),), device=x.device, dtype=torch.float64)


def photo_energy(x, flow, mask, ws=None, out=None):
    """the photometric energy per sample (dmh_photo_energy): E[b] = mean over (3, H, W) of mask * (flow_warp(x[:, 3:], flow) -
    x[:, :3]) ** 2, warp and sums in float64, a fixed summation order.  -> E (B,) float64"""
    B, H, W = _photo_dims('photo_energy', x, flow, mask)
    ws = photo_energy_workspace(x) if ws is None else ws
    out = _empty((B,), x, torch.float64) if out is None else out
    if tuple(out.shape) != (B,) or ws.numel() < B * photo_energy_splits(B, H, W):
        raise ValueError(f'photo_energy: out {tuple(out.shape)} / ws of {ws.numel()} doubles for {B} x {H} x {W}')
    call('dmh_photo_energy', ptr(x), ptr(flow), ptr(mask), ptr(ws, torch.float64), ptr(out, torch.float64), B, H, W)
    return out


def _keep_rows(who, keep, B):
    if keep is not None and (tuple(keep.shape) != (B,) or keep.dtype != torch.uint8):
        raise ValueError(f'{who}: keep {tuple(keep.shape)} {keep.dtype} for {B} rows (a (B,) uint8 mask)')


def flow_guidance_shift(cond, null, uncond, w, keep=None):
    """guidance on the flow condition, in place (dmh_flow_guidance_shift; the definition: include/dmhomo_hip.h): with the
    no-flow logits ``uncond`` and w = flow_guidance - 1, e = w * (b - uncond) with b = ``null`` where there is a null pass, else
    ``cond``; null += e and cond += e — but for the rows with keep == 0, which the conditional pass did not compute (``keep`` as
    sampler_step, with null only).  It reads no DmhStep: the same call serves the eager and the replayed loop.  -> (cond, null)"""
    B = cond.shape[0]
    if tuple(uncond.shape) != tuple(cond.shape) or (null is not None and tuple(null.shape) != tuple(cond.shape)):
        raise ValueError(f'flow_guidance_shift: uncond {tuple(uncond.shape)} / null {None if null is None else tuple(null.shape)} '
                         f'against cond {tuple(cond.shape)}')
    if keep is not None and null is None:
        raise ValueError('flow_guidance_shift: keep without null (without a null pass every row of cond was computed)')
    _keep_rows('flow_guidance_shift', keep, B)
    w = float(w)
    if not math.isfinite(w):
        raise ValueError(f'flow_guidance_shift: w = {w!r} is not finite')
    call('dmh_flow_guidance_shift', ptr(cond), ptr(null), ptr(uncond), ptr(keep, torch.uint8), w, B, cond.numel() // B)
    return cond, null


def pag_shift(cond, null, pert, s, keep=None):
    """perturbed-attention guidance, in place (dmh_pag_shift; the definition: include/dmhomo_hip.h): with the logits ``pert`` of
    the perturbed pass and s = pag_scale >= 0, e = s * (c - pert) with c = ``cond`` — on the rows with keep == 0, which the
    conditional pass did not compute, ``null`` (``keep`` as sampler_step, with null only); null += e and cond += e on the
    computed rows.  It reads no DmhStep: the same call serves the eager and the replayed loop.  -> (cond, null)"""
    B = cond.shape[0]
    if tuple(pert.shape) != tuple(cond.shape) or (null is not None and tuple(null.shape) != tuple(cond.shape)):
        raise ValueError(f'pag_shift: pert {tuple(pert.shape)} / null {None if null is None else tuple(null.shape)} '
                         f'against cond {tuple(cond.shape)}')
    if keep is not None and null is None:
        raise ValueError('pag_shift: keep without null (without a null pass every row of cond was computed)')
    _keep_rows('pag_shift', keep, B)
    s = float(s)
    if not (math.isfinite(s) and s >= 0.):
        raise ValueError(f'pag_shift: s = {s!r} is not a finite number >= 0')
    call('dmh_pag_shift', ptr(cond), ptr(null), ptr(pert), ptr(keep, torch.uint8), s, B, cond.numel() // B)
    return cond, null


def _known_shapes(who, model_cond, model_null, keep, known, kmask):
    """-> (B, per_row) of the known-pixel calls: known as model_cond, kmask one uint8 per element of it"""
    shape = tuple(model_cond.shape)
    if model_cond.dim() < 2 or (model_null is not None and tuple(model_null.shape) != shape) or tuple(known.shape) != shape:
        raise ValueError(f'{who}: known {tuple(known.shape)} / null {None if model_null is None else tuple(model_null.shape)} '
                         f'against model_cond {shape}')
    if kmask.dtype != torch.uint8 or kmask.numel() != model_cond.numel() or kmask.shape[0] != shape[0]:
        raise ValueError(f'{who}: kmask {tuple(kmask.shape)} {kmask.dtype} against model_cond {shape} (one uint8 per element, row '
                         f'by row)')
    if keep is not None and model_null is None:
        raise ValueError(f'{who}: keep without null (without a null pass every row of cond was computed)')
    _keep_rows(who, keep, shape[0])
    return shape[0], model_cond.numel() // shape[0]


def _aliases(a, b):
    return b is not None and a.data_ptr() < b.data_ptr() + b.numel() * b.element_size() and \
        b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()


def known_blend(model_cond, model_null, keep, cond_scale, known, kmask, out=None):
    """the logits of one denoise step with the known pixels in them (dmh_known_blend; the definition:
    include/dmhomo_hip_known.h): out = known where kmask != 0, else the guided blend of (model_cond, model_null, keep) as
    sampler_step reads it — model_null and keep may be None.  A select: a NaN logit under a kept element is gone.  kmask: uint8,
    one per element.  out None: model_cond itself, in place; out must not be model_null, known or kmask.  It reads no DmhStep: the
    same call serves the eager and the replayed loop, and — model_null None, cond_scale 1, in place on the unnormalised image
    with the caller's own values — the write-back behind the loop.  The result goes to sampler_step / sampler_step_ms /
    sampler_threshold + sampler_step_thr as model_cond with model_null = None.  -> out"""
    B, n = _known_shapes('known_blend', model_cond, model_null, keep, known, kmask)
    out = model_cond if out is None else out
    if tuple(out.shape) != tuple(model_cond.shape):
        raise ValueError(f'known_blend: out {tuple(out.shape)} against model_cond {tuple(model_cond.shape)}')
    if _aliases(out, model_null) or _aliases(out, known) or _aliases(out, kmask):
        raise ValueError('known_blend: out aliases model_null, known or kmask (in place means out is model_cond)')
    cs = float(cond_scale)
    if not math.isfinite(cs):
        raise ValueError(f'known_blend: cond_scale = {cs!r} is not finite')
    call('dmh_known_blend', ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), cs, ptr(known), ptr(kmask, torch.uint8),
         ptr(out), B, n)
    return out


def known_error_splits(B, n):
    """workgroups per row of the known-pixel score's first pass (dmh_known_error_splits): a pure function of (B, n)"""
    s = int(_lib.lib().dmh_known_error_splits(int(B), int(n)))
    if s < 1:
        raise ValueError(f'known_error_splits: B = {B} rows of n = {n} elements')
    return s


def known_error_workspace(x):
    """the fp64 workspace dmh_known_error asks for with logits of x's shape (B, ...): 2 doubles per (row, split)"""
    B = x.shape[0]
    return torch.empty((2 * B * known_error_splits(B, x.numel() // B),), device=x.device, dtype=torch.float64)


def known_error(model_cond, model_null, keep, cond_scale, known, kmask, ws=None, out=None):
    """how far logits are from the pixels they were told to keep (dmh_known_error): per row the mean over the kept elements
    (kmask != 0) of (x - known) ** 2, x the guided blend of (model_cond, model_null, keep) as known_blend reads it; float64, a
    fixed summation order; 0 for a row with nothing kept.  ws: known_error_workspace(model_cond).  -> (B,) float64"""
    B, n = _known_shapes('known_error', model_cond, model_null, keep, known, kmask)
    ws = known_error_workspace(model_cond) if ws is None else ws
    out = _empty((B,), model_cond, torch.float64) if out is None else out
    if tuple(out.shape) != (B,) or ws.numel() < 2 * B * known_error_splits(B, n) or _aliases(out, ws):
        raise ValueError(f'known_error: out {tuple(out.shape)} / ws of {ws.numel()} doubles for {B} rows of {n} (and out is not ws)')
    call('dmh_known_error', ptr(model_cond), ptr(model_null), ptr(keep, torch.uint8), float(cond_scale), ptr(known),
         ptr(kmask, torch.uint8), ptr(ws, torch.float64), ptr(out, torch.float64), B, n)
    return out


def affine_rows_keep(x, scale, shift, keep, out=None):
    """affine with a keep bit per row (dmh_affine_rows_keep): out[b] = scale * x[b] + shift where keep[b] != 0, else +0.0 — the
    normalisation of rgb_flow and the drop of ``flow_drop_prob`` in one launch.  keep: (B,) uint8."""
    x = x.contiguous()
    B = x.shape[0]
    if keep is None:
        raise ValueError('affine_rows_keep: keep is None (ops.affine is the call without a mask)')
    _keep_rows('affine_rows_keep', keep, B)
    y = torch.empty_like(x) if out is None else out
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError(f'affine_rows_keep: out {tuple(y.shape)} against x {tuple(x.shape)}')
    call('dmh_affine_rows_keep', ptr(x), ptr(y), float(scale), float(shift), ptr(keep, torch.uint8), B, x.numel() // B)
    return y


def rng_indexed(shape, sample_ids, state, kind=0):
    """one draw of the sample-indexed generator (dmh_rng_indexed): (B, *shape[1:]) fp32 whose row b is a pure function of
    (state[0] = seed, sample_ids[b], state[1] = draw index, element); the launch advances the draw index.
    kind 0: N(0,1) (CFG:679,705), 1: uniform [0,1) (CFG:90), 2: the raw Philox words (bit patterns; tests)."""
    B = int(shape[0])
    assert sample_ids.shape == (B,) and state.shape == (4,) and state.dtype == torch.int64
    out = torch.empty(tuple(shape), device=sample_ids.device, dtype=F32)
    call('dmh_rng_indexed', ptr(out), B, out.numel() // B, ptr(sample_ids, torch.int64), ptr(state, torch.int64), int(kind))
    return out


def start_mix(init01, ca, cb, *, noise=None, sample_ids=None, state=None, out=None):
    """the start image of sample_from in one launch (dmh_start_mix; the definition: include/dmhomo_hip_start.h): out = ca * (2 *
    init01 - 1) + cb * eps, every operation rounded separately — q_sample(affine(init01, 2, -1), eps) bit for bit.  eps: ``noise``,
    or the next draw of the keyed generator (``sample_ids``, ``state``; the launch advances the draw index as rng_indexed does and
    the noise never exists in memory); the entry refuses both or neither.  out may be ``noise`` itself.  -> out"""
    B = int(init01.shape[0])
    out = torch.empty_like(init01) if out is None else out
    if tuple(out.shape) != tuple(init01.shape) or (noise is not None and tuple(noise.shape) != tuple(init01.shape)):
        raise ValueError(f'start_mix: out {tuple(out.shape)} / noise {None if noise is None else tuple(noise.shape)} against '
                         f'init01 {tuple(init01.shape)}')
    if (sample_ids is not None and tuple(sample_ids.shape) != (B,)) or (state is not None and tuple(state.shape) != (4,)):
        raise ValueError(f'start_mix: sample_ids of {B} int64 (one per row) and state of 4 int64 expected')
    call('dmh_start_mix', ptr(init01), ptr(noise), ptr(sample_ids, torch.int64), ptr(state, torch.int64), float(ca), float(cb),
         ptr(out), B, init01.numel() // B)
    return out


RELABEL_RANGES = (.03, 8., 3e-5)          # (max_affine, max_shift, max_persp): the constants of ddpm.SyntheticConditions


def relabel_ranges(ranges):
    """(max_affine, max_shift, max_persp) as three floats, refused as include/dmhomo_hip_relabel.h says: negative or not finite,
    max_affine >= 0.25, max_persp >= 5e-4"""
    try:
        a, t, p = (float(v) for v in ranges)
    except (TypeError, ValueError):
        raise ValueError(f'relabel ranges = {ranges!r}: three numbers (max_affine, max_shift, max_persp)') from None
    if not all(math.isfinite(v) and v >= 0. for v in (a, t, p)):
        raise ValueError(f'relabel ranges = {ranges!r}: each must be a finite number >= 0')
    if a >= 0.25:
        raise ValueError(f'relabel ranges: max_affine = {a!r} must be below 0.25 (the linear part stays diagonally dominant)')
    if p >= 5e-4:
        raise ValueError(f"relabel ranges: max_persp = {p!r} must be below 5e-4 (w' stays >= 0.5 inside the frame)")
    return a, t, p


def relabel_batch(data, sample_ids, seed=0, ranges=RELABEL_RANGES, max_flow=256., base=None, fill=True, out=None, homos=None,
                  valid=None):
    """a batch re-labelled in one launch (dmh_relabel_batch; the definition: include/dmhomo_hip_relabel.h): data (B,12,H,W) fp32
    [img1 | img2 | mask | rgb_flow | flow], sample_ids (B,) int64 on the device, base (B,3,3) f64 or None -> (out (B,12,H,W),
    homos (B,3,3) f64, valid (B,H,W) uint8): a new homography per sample id, its flow and flow image, img1 warped by it as the
    target (the batch's img2 where the warp has no source pixel and ``fill``), img1 and mask copied."""
    if data.dim() != 4 or data.shape[1] != 12:
        raise ValueError(f'relabel_batch: data {tuple(data.shape)}: a (B, 12, H, W) batch expected')
    B, _, H, W = (int(v) for v in data.shape)
    a, t, p = relabel_ranges(ranges)
    if tuple(sample_ids.shape) != (B,):
        raise ValueError(f'relabel_batch: sample_ids {tuple(sample_ids.shape)}: {B} int64 (one per row) expected')
    if base is not None and tuple(base.shape) != (B, 3, 3):
        raise ValueError(f'relabel_batch: base {tuple(base.shape)}: ({B}, 3, 3) float64 expected')
    out = torch.empty_like(data) if out is None else out
    homos = torch.empty((B, 3, 3), device=data.device, dtype=torch.float64) if homos is None else homos
    valid = torch.empty((B, H, W), device=data.device, dtype=torch.uint8) if valid is None else valid
    if tuple(out.shape) != tuple(data.shape) or tuple(homos.shape) != (B, 3, 3) or tuple(valid.shape) != (B, H, W):
        raise ValueError(f'relabel_batch: out {tuple(out.shape)} / homos {tuple(homos.shape)} / valid {tuple(valid.shape)} against '
                         f'data {tuple(data.shape)}')
    call('dmh_relabel_batch', ptr(data), ptr(sample_ids, torch.int64), int(seed) & 0xFFFFFFFFFFFFFFFF, a, t, p, float(max_flow),
         ptr(base, torch.float64), int(bool(fill)), ptr(out), ptr(homos, torch.float64), ptr(valid, torch.uint8), B, H, W)
    return out, homos, valid


def rng_keep_mask(sample_ids, state, prob):
    """(B,) uint8: uniform draw of the indexed generator < prob (the class-dropout mask of CFG:84-90), one launch."""
    B = sample_ids.shape[0]
    out = torch.empty((B,), device=sample_ids.device, dtype=torch.uint8)
    call('dmh_rng_keep_mask', ptr(out, torch.uint8), B, ptr(sample_ids, torch.int64), ptr(state, torch.int64), float(prob))
    return out


def affine(x, scale, shift, out=None):
    x = x.contiguous()
    y = torch.empty_like(x) if out is None else out
    call('dmh_affine', ptr(x), ptr(y), float(scale), float(shift), x.numel())
    return y


def lerp(a, b, lam):
    """(1 - lam) * a + lam * b  (DDP:746) on the q_sample kernel."""
    B = a.shape[0]
    ca = torch.full((B,), 1.0 - lam, device=a.device, dtype=torch.float32)
    cb = torch.full((B,), lam, device=a.device, dtype=torch.float32)
    return q_sample(a.contiguous(), b.contiguous(), ca, cb)


def affine_tail_(x, c0, scale, shift):
    B, Cc, H, W = x.shape
    call('dmh_affine_tail', ptr(x), B, Cc, H * W, c0, float(scale), float(shift))
    return x


def q_sample(x_start, noise, ca, cb):
    out = torch.empty_like(x_start)
    B = x_start.shape[0]
    call('dmh_q_sample', ptr(x_start), ptr(noise), ptr(ca), ptr(cb), ptr(out), B, x_start.numel() // B)
    return out


def rows_lincomb(x, ca, y=None, cb=None, div=None, clamp=False):
    """out = ca[b] * x (+ cb[b] * y) (/ div[b]) (clamped to [-1, 1]); ca / cb / div: (B,) fp32 per-sample coefficients
    (``extract`` of a schedule buffer at a per-row timestep): D4 / D7 of SURVEY 8a in the reference's op order."""
    x = x.contiguous()
    B = x.shape[0]
    out = torch.empty_like(x)
    call('dmh_rows_lincomb', ptr(x), ptr(None if y is None else y.contiguous()), ptr(ca.contiguous()),
         ptr(None if cb is None else cb.contiguous()), ptr(None if div is None else div.contiguous()), ptr(out), B,
         x.numel() // B, int(bool(clamp)))
    return out


def diff_mean(a, b, mask=None, squared=False):
    """per-sample mean over (C,H,W) of mask * |a-b| (or (a-b)^2): the loss terms of p_losses (CFG:796-802)."""
    B, Cc, H, W = a.shape
    ws = torch.empty((B, 64), device=a.device, dtype=torch.float64)
    out = torch.empty((B,), device=a.device, dtype=F32)
    call('dmh_diff_mean', ptr(a), ptr(b), ptr(mask), int(bool(squared)), ptr(ws, torch.float64), ptr(out), B, Cc,
         H * W)
    return out


def loss_combine(l, photo, w):
    out = torch.empty((1,), device=l.device, dtype=F32)
    call('dmh_loss_combine', ptr(l), ptr(photo), ptr(w), ptr(out), l.shape[0])
    return out[0]


def to_uint8(img):
    out = torch.empty(img.shape, device=img.device, dtype=torch.uint8)
    call('dmh_to_uint8', ptr(img), ptr(out, torch.uint8), img.numel())
    return out


# ------------------------------------------------------------------ geometry
def homography_flow(Hm, H, W, max_flow=256., want_flow=True, want_rgb=True):
    """G2+G3.  Hm (B,3,3) f64 device -> flow (B,2,H,W), rgb (B,3,H,W)."""
    B = Hm.shape[0]
    flow = torch.empty((B, 2, H, W), device=Hm.device, dtype=F32) if want_flow else None
    rgb = torch.empty((B, 3, H, W), device=Hm.device, dtype=F32) if want_rgb else None
    call('dmh_homography_flow', ptr(Hm, torch.float64), ptr(flow), ptr(rgb), B, H, W, float(max_flow))
    return flow, rgb


def flow_to_image(flow, max_flow=256.):
    """G3: flow (B,2,H,W) -> rgb (B,3,H,W)."""
    B, _, H, W = flow.shape
    rgb = torch.empty((B, 3, H, W), device=flow.device, dtype=F32)
    call('dmh_flow_to_image', ptr(flow), ptr(rgb), B, H * W, float(max_flow))
    return rgb


FLOW_WARP_PAD = {'border': 0, 'zeros': 1, 'reflection': 2}
FLOW_WARP_MODE = {'bilinear': 0, 'nearest': 1, 'bicubic': 2}


def flow_warp(x, flow, want_indices=False, pad='border', mode='bilinear'):
    B, Cc, H, W = x.shape
    assert flow.shape == (B, 2, H, W)
    out = torch.empty_like(x)
    x0 = y0 = None
    if want_indices:
        x0 = torch.empty((B, H, W), device=x.device, dtype=torch.int32)
        y0 = torch.empty((B, H, W), device=x.device, dtype=torch.int32)
    call('dmh_flow_warp', ptr(x), ptr(flow), ptr(out), ptr(x0, torch.int32), ptr(y0, torch.int32), B, Cc, H, W,
         FLOW_WARP_PAD[pad], FLOW_WARP_MODE[mode])
    return (out, x0, y0) if want_indices else out


def pixel_grid(B, H, W, start, device):
    """get_grid DDP:1558-1574: (B,2,H,W) fp32 pixel coordinates (+ start)."""
    out = torch.empty((B, 2, H, W), device=device, dtype=F32)
    call('dmh_pixel_grid', ptr(out), B, H, W, float(start))
    return out


def norm_grid(v):
    """norm_grid DDP:1292-1299: (B,2,H,W) pixel coordinates -> (B,H,W,2) in [-1,1]."""
    B, two, H, W = v.shape
    assert two == 2
    out = torch.empty((B, H, W, 2), device=v.device, dtype=F32)
    call('dmh_norm_grid', ptr(v.contiguous()), ptr(out), B, H, W)
    return out


def homography_flow_points(Hm, idx):
    """get_flow_np DDP:927-969: Hm (B,divide,3,3) f64, idx (Bi,3,H,W) f64 -> flow (B,2,H,W) f64."""
    B, divide = Hm.shape[:2]
    Bi, three, H, W = idx.shape
    assert three == 3 and Hm.shape[2:] == (3, 3)
    out = torch.empty((B, 2, H, W), device=Hm.device, dtype=torch.float64)
    call('dmh_homography_flow_points', ptr(Hm.contiguous(), torch.float64), ptr(idx.contiguous(), torch.float64),
         ptr(out, torch.float64), B, divide, Bi, H, W)
    return out


def dlt_points(src, off):
    """DLT_solve DDP:1612-1643: src, off (N,P,2) f64 -> (N,3,3) f64 least-squares homographies."""
    N, P, two = src.shape
    assert two == 2 and off.shape == src.shape
    ws = torch.empty((N, _lib.DLT_BLOCKS, 44), device=src.device, dtype=torch.float64)
    out = torch.empty((N, 3, 3), device=src.device, dtype=torch.float64)
    call('dmh_dlt_points', ptr(src.contiguous(), torch.float64), ptr(off.contiguous(), torch.float64),
         ptr(ws, torch.float64), ptr(out, torch.float64), N, P)
    return out


def dlt_homography(flow):
    """G5: flow (B,2,H,W) fp32 -> (B,3,3) f64."""
    B, _, H, W = flow.shape
    ws = torch.empty((B, _lib.DLT_BLOCKS, 44), device=flow.device, dtype=torch.float64)
    out = torch.empty((B, 3, 3), device=flow.device, dtype=torch.float64)
    call('dmh_dlt_homography', ptr(flow), ptr(ws, torch.float64), ptr(out, torch.float64), B, H, W)
    return out


# ------------------------------------------------------------------ sample preview sheets (DDP:1489-1555)
def _preview_inputs(img, mask, flow):
    B, C6, H, W = img.shape
    assert C6 == 6 and mask.shape == (B, 1, H, W) and flow.shape == (B, 2, H, W), (img.shape, mask.shape, flow.shape)
    return B, H, W


def post_process(img, mask, flow):
    """postProcess DDP:1505-1517 in one launch: img (B,6,H,W), mask (B,1,H,W), flow (B,2,H,W) ->
    buf1 = [img1 | img1 | mask x3 | flow_vis], buf2 = [img2 | flow_warp(img2, flow) | mask x3 | flow_vis], (B,3,H,4W)."""
    B, H, W = _preview_inputs(img, mask, flow)
    buf1 = torch.empty((B, 3, H, 4 * W), device=img.device, dtype=F32)
    buf2 = torch.empty_like(buf1)
    call('dmh_post_process', ptr(img), ptr(mask), ptr(flow), ptr(buf1), ptr(buf2), B, H, W)
    return buf1, buf2


def grid_shape(B, H, W, nrow=8, padding=2):
    """torchvision's make_grid geometry for B images of (H, W): (sheet height, sheet width, xmaps); B == 1: the image alone"""
    if B == 1:
        return H, W, 1
    xmaps = min(int(nrow), B)
    ymaps = -(-B // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, xmaps


def preview_sheet(img, mask, flow, nrow=8, padding=2, bgr=True):
    """the panels of post_process + channel swap + make_grid + save_image's quantisation in one launch: two uint8 (Hs, Ws, 3)
    sheets on the device."""
    B, H, W = _preview_inputs(img, mask, flow)
    Hs, Ws, _ = grid_shape(B, H, 4 * W, nrow, padding)
    s1 = torch.empty((Hs, Ws, 3), device=img.device, dtype=torch.uint8)
    s2 = torch.empty_like(s1)
    call('dmh_preview_sheet', ptr(img), ptr(mask), ptr(flow), ptr(s1, torch.uint8), ptr(s2, torch.uint8), B, H, W, int(nrow),
         int(padding), int(bool(bgr)))
    return s1, s2


def homography_warp(src, homos, dsize):
    """cv2.warpPerspective(src, M, dsize) without the inverse-map flag, exact bilinear (float64 coordinates and weights):
    src (B,3,H,W) fp32, homos (B,3,3) f64, dsize = (width, height) as cv2 takes it -> (B,3,height,width)."""
    B, C3, H, W = src.shape
    assert C3 == 3 and homos.shape == (B, 3, 3), (src.shape, homos.shape)
    Wd, Hd = int(dsize[0]), int(dsize[1])
    dst = torch.empty((B, 3, Hd, Wd), device=src.device, dtype=F32)
    call('dmh_homography_warp', ptr(src), ptr(homos, torch.float64), ptr(dst), B, H, W, Hd, Wd)
    return dst


# ------------------------------------------------------------------ HEM training batches (HEM/dataset/data_loader.py:97-255)
def hem_batch(img12, homo, homo_inv, start, mean, std, ori_size, crop_size):
    """DGMTrainData's item arithmetic for a whole batch in one launch: img12 (B,6,h,w) uint8, homo / homo_inv (B,3,3) f64
    at ``ori_size``, start (B,2) int32 as (x, y) — all on the device; mean / std: three host floats each ->
    (imgs_gray_full, imgs_rgb_full, flow_gt_full, imgs_gray_patch, flow_gt_patch)."""
    B, six, h, w = img12.shape
    (H, W), (ph, pw) = ori_size, crop_size
    assert six == 6 and homo.shape == (B, 3, 3) and homo_inv.shape == (B, 3, 3) and start.shape == (B, 2), \
        (img12.shape, homo.shape, homo_inv.shape, start.shape)
    m3, s3 = (C.c_double * 3)(*[float(v) for v in mean]), (C.c_double * 3)(*[float(v) for v in std])
    pin, dev = ptr(img12, torch.uint8), img12.device          # (refuses a CPU tensor before anything is allocated)
    gray = torch.empty((B, 2, H, W), device=dev, dtype=F32)
    rgb = torch.empty((B, 6, H, W), device=dev, dtype=F32)
    flow = torch.empty((B, 4, H, W), device=dev, dtype=F32)
    gray_p = torch.empty((B, 2, ph, pw), device=dev, dtype=F32)
    flow_p = torch.empty((B, 4, ph, pw), device=dev, dtype=F32)
    call('dmh_hem_batch', pin, ptr(homo, torch.float64), ptr(homo_inv, torch.float64), ptr(start, torch.int32),
         C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), B, h, w, int(H), int(W), int(ph), int(pw), ptr(gray), ptr(rgb),
         ptr(flow), ptr(gray_p), ptr(flow_p))
    return gray, rgb, flow, gray_p, flow_p


def hem_flow(homo, H, W):
    """homo_convert_to_flow (data_loader.py:42-52): homo (B,3,3) f64 device -> flow (B,2,H,W) fp32."""
    B = homo.shape[0]
    assert homo.shape == (B, 3, 3), homo.shape
    ph = ptr(homo, torch.float64)
    flow = torch.empty((B, 2, int(H), int(W)), device=homo.device, dtype=F32)
    call('dmh_hem_flow', ph, B, int(H), int(W), ptr(flow))
    return flow


# ------------------------------------------------------------------ training (first pieces)
def conv_wgrad(dy, src0, src1=None, k=3, in_coef=None, want_bias=True, ups=0):
    """weight (and bias) gradient of the stride-1 kxk conv whose input was cat(src0, src1) (after the optional
    SiLU(a*src0+b) prologue; ups=1: after a nearest x2 upsampling; k=2: 'valid' conv over the space-to-depth view) and
    whose output gradient is dy.  NHWC in, OIHW (Cout, C0+C1, k, k) out."""
    B, H, W, cout = dy.shape
    c0 = src0.shape[3]
    c1 = 0 if src1 is None else src1.shape[3]
    dw = _empty((cout, c0 + c1, k, k), dy)
    db = _empty((cout,), dy) if want_bias else None
    work = _empty((lib().dmh_conv_wgrad_workspace_floats(B, H, W, c0, c1, cout, k),), dy)
    call('dmh_conv_wgrad', ptr(dy.contiguous()), ptr(src0), ptr(src1), ptr(in_coef), ptr(dw), ptr(db), ptr(work), B, H, W,
         c0, c1, cout, k, int(ups))
    return (dw, db) if want_bias else dw


def conv_dgrad_pack(w, c_in_total, batch=None):
    """PackedConv that computes the DATA gradient of a stride-1 conv with weight w (Cout, Cin, k, k): the same conv
    kernel on dy with the taps flipped and (Cout, Cin) transposed (no bias)."""
    assert w.shape[1] == c_in_total
    return PackedConv(w, None, w.shape[0], batch=batch, transposed=True)


def gn_finalize_train(stats, gamma, beta, hw, groups, ss=None, eps=1e-5):
    """gn_finalize that also returns mr (B, groups, 2) = (mean, rstd), saved for gn_silu_backward."""
    B, tiles, Cc, _ = stats.shape
    coef = _empty((B, 2, Cc), stats)
    mr = _empty((B, groups, 2), stats)
    ss_ptr, ss_stride = _ss_arg(ss, B, Cc)
    call('dmh_gn_finalize_train', ptr(stats), tiles, ptr(gamma), ptr(beta), ss_ptr, ss_stride, ptr(coef), ptr(mr), B, Cc,
         groups, hw, float(eps))
    return coef, mr


def gn_silu_backward(dout, y, coef, mr, gamma, beta, groups, ss=None):
    """backward of GroupNorm -> (scale+1, shift) -> SiLU: -> dy (B,H,W,C), dgamma (C,), dbeta (C,), dss (B, 2C) = the
    gradient wrt the (scale, shift) row of the ResnetBlock mlp (zeros are NOT returned when ss is None: dss = None)."""
    B, H, W, Cc = y.shape
    hw = H * W
    dy = _empty(y.shape, y)
    pg = _empty((B, 4, Cc), y)
    part = _empty((B, lib().dmh_gn_bwd_chunks(hw), Cc, 2), y)
    bcoef = _empty((B, 3, Cc), y)
    ss_ptr, ss_stride = _ss_arg(ss, B, Cc)
    call('dmh_gn_silu_backward', ptr(dout), ptr(y), ptr(coef), ptr(mr), ptr(gamma), ptr(beta), ss_ptr, ss_stride, ptr(dy),
         ptr(pg), ptr(part), ptr(bcoef), B, hw, Cc, groups)
    # pg is (B, 4, C): per sample (dgamma, dbeta, dscale, dshift) parts.  All four are summed over the batch in place (the
    # last two sums are not used: cheaper than a strided copy of the first two in front of the kernel), and the (scale, shift)
    # gradient goes back as a VIEW of pg — its one consumer copies it into its slice of the mlp output's gradient
    gb = _empty((4, Cc), y)
    call('dmh_sum_over_batch', ptr(pg), ptr(gb), B, 4 * Cc)
    dss = pg.reshape(B, 4 * Cc)[:, 2 * Cc:] if ss is not None else None
    return dy, gb[0], gb[1], dss


def ws_backward(w, dwh, eps=1e-5):
    """gradient wrt the raw weight from the gradient wrt the standardised one (CFG:120-126)."""
    cout = w.shape[0]
    w, dwh = w.contiguous(), dwh.contiguous()
    dw = torch.empty_like(w)
    call('dmh_ws_backward', ptr(w), ptr(dwh), ptr(dw), cout, w.numel() // cout, float(eps))
    return dw


def chan_layernorm_backward(x, g, dout, eps=1e-5):
    """backward of chan_layernorm (without its residual input, whose gradient is dout itself) -> dx, dg."""
    Cc = x.shape[-1]
    x, dout = x.contiguous(), dout.contiguous()
    dx = torch.empty_like(x)
    nb = lib().dmh_lnb_blocks()
    part = _empty((nb, Cc), x)
    call('dmh_chan_layernorm_backward', ptr(x), ptr(g), ptr(dout), ptr(dx), ptr(part), x.numel() // Cc, Cc, float(eps))
    dg = _empty((Cc,), x)
    call('dmh_sum_over_batch', ptr(part), ptr(dg), nb, Cc)
    return dx, dg


def linear_attention_core_train(qkv, scale):
    """linear_attention_core that also returns what its backward needs: (out, saved)."""
    B, H, W, c = qkv.shape
    assert c == 384
    n = H * W
    partial = _empty((lib().dmh_linattn_partial_floats(B, n),), qkv)
    ctx = _empty((B, 4, 32, 32), qkv)
    ms = _empty((B, 4, 32, 2), qkv)
    out = _empty((B, H, W, 128), qkv)
    call('dmh_linattn_context', ptr(qkv), ptr(partial), B, n, None)
    call('dmh_linattn_merge_ms', ptr(partial), ptr(ctx), ptr(ms), B, n)
    call('dmh_linattn_apply', ptr(qkv), ptr(ctx), ptr(out), B, n, float(scale), None)
    return out, dict(qkv=qkv, ctx=ctx, ms=ms, scale=float(scale))


def linear_attention_core_backward(sv, dout):
    """gradient wrt qkv (B,H,W,384) of the LinearAttention core from the gradient wrt its output (B,H,W,128)."""
    qkv = sv['qkv']
    B, H, W, _ = qkv.shape
    n = H * W
    dqkv = torch.empty_like(qkv)
    work = _empty((lib().dmh_linattn_bwd_workspace_floats(B, n),), qkv)
    call('dmh_linattn_backward', ptr(qkv), ptr(sv['ctx']), ptr(sv['ms']), ptr(dout.contiguous()), ptr(dqkv), ptr(work), B, n,
         sv['scale'])
    return dqkv


def _strides4(*v):
    return (C.c_int64 * 4)(*v)


def bgemm(a, sa, b, sb, c, sc, M, N, K, nbo, nbi, alpha=1.0):
    """c[bo][bi] = alpha * a[bo][bi] (MxK) @ b[bo][bi] (KxN); sa/sb/sc = (outer batch, inner batch, row, column) strides in
    floats; a, b, c: tensors or (tensor, float offset) pairs."""
    def base(t):
        if isinstance(t, tuple):
            return C.c_void_p(t[0].data_ptr() + 4 * t[1])
        return ptr(t)
    call('dmh_bgemm', base(a), _strides4(*sa), base(b), _strides4(*sb), base(c), _strides4(*sc), M, N, K, nbo, nbi,
         float(alpha))


def attention_core_train(qkv, scale):
    """bottleneck Attention core (CFG:287-295) on the small-GEMM kernels, keeping P = softmax(sim): (out (B,H,W,128), saved)."""
    B, H, W, c = qkv.shape
    assert c == 384
    n = H * W
    S = _empty((B, 4, n, n), qkv)
    # sim[i][j] = scale * sum_d q[i][d] k[j][d]
    bgemm(qkv, (n * 384, 32, 384, 1), (qkv, 128), (n * 384, 32, 1, 384), S, (4 * n * n, n * n, n, 1), n, n, 32, B, 4, scale)
    P = torch.empty_like(S)
    call('dmh_softmax_rows', ptr(S), ptr(P), B * 4 * n, n)
    out = _empty((B, H, W, 128), qkv)
    # out[i][h*32+d] = sum_j P[i][j] v[j][d]
    bgemm(P, (4 * n * n, n * n, n, 1), (qkv, 256), (n * 384, 32, 384, 1), out, (n * 128, 32, 128, 1), n, 32, n, B, 4)
    return out, dict(qkv=qkv, P=P, scale=float(scale))


def attention_core_backward(sv, dout):
    """gradient wrt qkv (B,H,W,384) of the Attention core from the gradient wrt its output (B,H,W,128)."""
    qkv, P, scale = sv['qkv'], sv['P'], sv['scale']
    B, H, W, _ = qkv.shape
    n = H * W
    dout = dout.contiguous()
    dqkv = torch.empty_like(qkv)
    sP, sQ, sO = (4 * n * n, n * n, n, 1), (n * 384, 32, 384, 1), (n * 128, 32, 128, 1)
    # dv[j][d] = sum_i P[i][j] dout[i][d]
    bgemm(P, (4 * n * n, n * n, 1, n), dout, sO, (dqkv, 256), sQ, n, 32, n, B, 4)
    # dP[i][j] = sum_d dout[i][d] v[j][d]
    dP = torch.empty_like(P)
    bgemm(dout, sO, (qkv, 256), (n * 384, 32, 1, 384), dP, sP, n, n, 32, B, 4)
    call('dmh_softmax_rows_backward', ptr(P), ptr(dP), B * 4 * n, n)          # dP <- dsim
    # dq[i][d] = scale * sum_j dsim[i][j] k[j][d] ;  dk[j][d] = scale * sum_i dsim[i][j] q[i][d]
    bgemm(dP, sP, (qkv, 128), sQ, dqkv, sQ, n, 32, n, B, 4, scale)
    bgemm(dP, (4 * n * n, n * n, 1, n), qkv, sQ, (dqkv, 128), sQ, n, 32, n, B, 4, scale)
    return dqkv


def conv_up_backward(dy, x, w, dpack=None):
    """backward of Upsample = nearest x2 -> conv3x3 (CFG:106-107): dy (B,2H,2W,Cout), x (B,H,W,C) -> dx, dw, db."""
    B, H, W, c = x.shape
    dpack = dpack or conv_dgrad_pack(w, c)
    gup = conv2d(dpack, dy)                                             # gradient wrt the upsampled tensor
    dx = torch.empty_like(x)
    call('dmh_sumpool2', ptr(gup), ptr(dx), B, H, W, c)
    dw, db = conv_wgrad(dy, x, k=3, ups=1)
    return dx, dw, db


# Downsample 4x4 / stride 2 / pad 1: for input row parity r the taps (ky, row offset a) that reach it
_DOWN_K = {0: {-1: 3, 0: 1}, 1: {0: 2, 1: 0}}


def conv_down_dgrad_pack(w, batch=None):
    """PackedConv of the 3x3 conv over dy that yields the data gradient of the 4x4/stride-2 conv in pixel-shuffle
    layout: out[m][l][(ry*2+rx)*C + c] = dx[2m+ry][2l+rx][c]."""
    cout, c = w.shape[0], w.shape[1]
    w3 = torch.zeros((4 * c, cout, 3, 3), device=w.device, dtype=torch.float32)

    def fill():                            # (the taps that no parity reaches stay zero)
        for ry in (0, 1):
            for rx in (0, 1):
                par = ry * 2 + rx
                for a, ky in _DOWN_K[ry].items():
                    for b, kx in _DOWN_K[rx].items():
                        w3[par * c:(par + 1) * c, :, a + 1, b + 1] = w[:, :, ky, kx].t()
    fill()
    if batch is not None:
        batch.pre.append(fill)
    return PackedConv(w3, None, cout, batch=batch)


def conv_down_backward(dy, x, w, dpack=None):
    """backward of Downsample = conv 4x4 / stride 2 / pad 1 (CFG:110-111): dy (B,H/2,W/2,Cout), x (B,H,W,C) -> dx, dw, db"""
    B, H, W, c = x.shape
    cout = dy.shape[3]
    dpack = dpack or conv_down_dgrad_pack(w)
    g4 = conv2d(dpack, dy)                                              # (B, H/2, W/2, 4C)
    dx = torch.empty_like(x)
    call('dmh_d2s', ptr(g4), ptr(dx), B, H // 2, W // 2, c)
    X = _empty((B, H // 2 + 1, W // 2 + 1, 4 * c), x)
    call('dmh_s2d_shift', ptr(x.contiguous()), ptr(X), B, H, W, c)
    dw2, db = conv_wgrad(dy, X, k=2)                                    # (Cout, 4C, 2, 2): [(py,px,c)][dy][dx]
    dw = dw2.view(cout, 2, 2, c, 2, 2).permute(0, 3, 4, 1, 5, 2).reshape(cout, c, 4, 4).contiguous()
    return dx, dw, db


def conv_unshuffle_wgrad(dy, x, want_bias=True):
    """weight (and bias) gradient of the DDP Downsample = pixel-unshuffle + 1x1 (DDP:110-113): dy (B,H/2,W/2,Cout),
    x (B,H,W,C) the stored input, read in place -> dw (Cout, 4C, 1, 1) in the reference's channel order c*4 + py*2 + px"""
    B, H, W, c = x.shape
    cout = dy.shape[3]
    assert tuple(dy.shape) == (B, H // 2, W // 2, cout), (dy.shape, x.shape)
    dw = _empty((cout, 4 * c, 1, 1), dy)
    db = _empty((cout,), dy) if want_bias else None
    work = _empty((lib().dmh_conv_unshuffle_wgrad_workspace_floats(B, H, W, c, cout),), dy)
    call('dmh_conv_unshuffle_wgrad', ptr(dy.contiguous()), ptr(x.contiguous()), ptr(dw), ptr(db), ptr(work), B, H, W, c, cout)
    return (dw, db) if want_bias else dw


def conv_unshuffle_dgrad_pack(w, batch=None):
    """PackedConv of the 1x1 conv over dy that yields the data gradient of the DDP Downsample (weight w (Cout, 4C, 1, 1))
    in pixel-shuffle layout: out[m][l][(py*2+px)*C + c] = dx[2m+py][2l+px][c] (then dmh_d2s).  The transposed, permuted
    weight is re-derived from w on every ``batch.run()``."""
    cout, c4 = w.shape[0], w.shape[1]
    c = c4 // 4
    wt = torch.empty((c4, cout, 1, 1), device=w.device, dtype=torch.float32)
    w_src = w.detach()

    def fill():                            # wt[(py*2+px)*C + c][o] = w[o][c*4 + py*2 + px]
        wt.view(4, c, cout).copy_(w_src.view(cout, c, 4).permute(2, 1, 0))
    fill()
    if batch is not None:
        batch.pre.append(fill)
    return PackedConv(wt, None, cout, batch=batch)


def conv_unshuffle_backward(dy, x, w, dpack=None):
    """backward of the DDP Downsample (DDP:110-113): dy (B,H/2,W/2,Cout), x (B,H,W,C), w (Cout, 4C, 1, 1) -> dx, dw, db"""
    B, H, W, c = x.shape
    dpack = dpack or conv_unshuffle_dgrad_pack(w)
    g4 = conv2d(dpack, dy)                                              # (B, H/2, W/2, 4C)
    dx = torch.empty_like(x)
    call('dmh_d2s', ptr(g4), ptr(dx), B, H // 2, W // 2, c)
    dw, db = conv_unshuffle_wgrad(dy, x)
    return dx, dw, db


def act(x, mode, dy=None):
    """mode 'silu' | 'gelu': f(x), or dy * f'(x) when dy is given."""
    x = x.contiguous()
    out = torch.empty_like(x)
    call('dmh_act', ptr(x), ptr(None if dy is None else dy.contiguous()), ptr(out), x.numel(), {'silu': 1, 'gelu': 2}[mode])
    return out


def add(a, b):
    """a + b (elementwise, same shape) on the q_sample kernel."""
    B = a.shape[0]
    one = torch.ones((B,), device=a.device, dtype=torch.float32)
    return q_sample(a.contiguous(), b.contiguous(), one, one)


def linear_backward(x, w, dy, want_bias=True):
    """y = x @ w.T (+ b), x (B,in), w (out,in), dy (B,out) -> dx (B,in), dw (out,in), db (out,)"""
    Bn, cin = x.shape
    cout = w.shape[0]
    x, dy, w = x.contiguous(), dy.contiguous(), w.contiguous()
    dx = _empty((Bn, cin), x)
    dw = _empty((cout, cin), x)
    if cout >= 1024 and cout % 128 == 0:       # long K (the stacked per-block MLPs): split it, add the parts in order
        nk = cout // 128
        part = _empty((nk, Bn, cin), x)
        bgemm(dy, (0, 128, cout, 1), w, (0, 128 * cin, cin, 1), part, (0, Bn * cin, cin, 1), Bn, cin, 128, 1, nk)
        call('dmh_sum_over_batch', ptr(part), ptr(dx), nk, Bn * cin)
    else:
        bgemm(dy, (0, 0, cout, 1), w, (0, 0, cin, 1), dx, (0, 0, cin, 1), Bn, cin, cout, 1, 1)
    bgemm(dy, (0, 0, 1, cout), x, (0, 0, cin, 1), dw, (0, 0, cin, 1), cout, cin, Bn, 1, 1)
    db = None
    if want_bias:
        db = _empty((cout,), x)
        call('dmh_sum_over_batch', ptr(dy), ptr(db), Bn, cout)
    return dx, dw, db


# ------------------------------------------------------------------ loss gradient + optimiser (training step)
def loss_backward(out, target, warped, mask, flow, abar, squared=False):
    """gradient of p_losses (CFG:796-806) wrt the UNet output (B,6,H,W); ``warped`` = flow_warp(out[:, 3:], flow)."""
    B, _, H, W = out.shape
    dout = torch.empty_like(out)
    gD = torch.empty((B, 3, H, W), device=out.device, dtype=F32)
    call('dmh_loss_backward', ptr(out), ptr(target.contiguous()), ptr(warped), ptr(mask.contiguous()),
         ptr(flow.contiguous()), ptr(abar.contiguous()), ptr(dout), ptr(gD), B, H, W, int(bool(squared)))
    return dout


def loss_backward_ddp(out, target, w, squared=False, scale=1.0):
    """gradient of the unconditional p_losses (DDP:804-811) wrt the UNet output (B,C,H,W): w (B,) = p2_loss_weight[t];
    ``scale`` folds in 1 / accum"""
    out = out.contiguous()
    B = out.shape[0]
    dout = torch.empty_like(out)
    call('dmh_loss_backward_ddp', ptr(out), ptr(target.contiguous()), ptr(w.to(F32).contiguous()), ptr(dout), B,
         out.numel() // B, int(bool(squared)), float(scale))
    return dout


def sumsq_blocks():
    return int(lib().dmh_sumsq_blocks())


def grad_norm_clip(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ (DDP:1852) as data: (2,) tensor [total L2 norm, min(1, max_norm/(norm+1e-6))];
    the gradients themselves are left alone — dmh_adam multiplies by the coefficient while reading them."""
    nb = sumsq_blocks()
    dev = grads[0].device
    part = torch.empty((len(grads) * nb,), device=dev, dtype=torch.float64)
    for i, gr in enumerate(grads):
        call('dmh_sumsq', ptr(gr), gr.numel(), ptr(part[i * nb:], torch.float64))
    out = torch.empty((2,), device=dev, dtype=F32)
    call('dmh_gradnorm_finalize', ptr(part, torch.float64), part.numel(), float(max_norm), ptr(out))
    return out


def adam_(p, g, m, v, gscale, lr, b1, b2, eps, step):
    """in-place torch.optim.Adam update (no weight decay, no amsgrad) of p with gradient g * gscale[1]."""
    call('dmh_adam', ptr(p), ptr(g), ptr(m), ptr(v), ptr(gscale), p.numel(), float(lr), float(b1), float(b2),
         float(eps), int(step))


def ema_(ema, p, decay):
    """ema <- ema * decay + p * (1 - decay), in place."""
    call('dmh_ema', ptr(ema), ptr(p), p.numel(), float(decay))


def _ptr_table(tensors):
    for t in tensors:
        assert t.is_cuda and t.dtype == F32 and t.is_contiguous()
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def clip_adam_multi_(params, grads, ms, vs, max_norm, lr, b1, b2, eps, step):
    """clip_grad_norm_ + Adam.step (DDP:1852-1857) over lists of tensors in a handful of launches (dmh_sumsq_multi,
    dmh_gradnorm_finalize, dmh_adam_multi).  -> (2,) tensor [total norm, clip coefficient]"""
    n = len(params)
    sizes = (C.c_int64 * n)(*[p.numel() for p in params])
    gt = _ptr_table(grads)
    nb = int(lib().dmh_multi_blocks(sizes, n))
    part = torch.empty((nb,), device=params[0].device, dtype=torch.float64)
    call('dmh_sumsq_multi', gt, sizes, n, ptr(part, torch.float64))
    clip = torch.empty((2,), device=params[0].device, dtype=F32)
    call('dmh_gradnorm_finalize', ptr(part, torch.float64), nb, float(max_norm), ptr(clip))
    call('dmh_adam_multi', _ptr_table(params), gt, _ptr_table(ms), _ptr_table(vs), sizes, n, ptr(clip), float(lr), float(b1),
         float(b2), float(eps), int(step))
    return clip
