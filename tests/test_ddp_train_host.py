"""CPU: the host side of the unconditional class's training kernels (dmh_conv_unshuffle_wgrad, the DDP Downsample's weight
gradient, and dmh_loss_backward_ddp, the gradient of its loss).  Every refusal happens in host-side validation, before a
launch, and answers through the error channel; the workspace size function answers -1 for sizes it cannot serve.  No GPU
is needed (host pointers: nothing here may pass validation)."""
import ctypes

from dmhomo_amd import _lib

BUF = (ctypes.c_char * 4096)()
P = ctypes.cast(BUF, ctypes.c_void_p)


def test_unshuffle_wgrad_workspace_size():
    lib = _lib.lib()
    ws = lib.dmh_conv_unshuffle_wgrad_workspace_floats
    # the 1x1 wgrad's layout: (splits x 64x64 partial blocks per (Cout, 4C) tile pair) + (splits x 64-channel bias rows)
    for B, H, C, cout in ((16, 128, 64, 64), (16, 64, 64, 128), (16, 32, 128, 256), (3, 16, 8, 8), (1, 4, 24, 32)):
        n = ws(B, H, H, C, cout)
        npairs = -(-cout // 64) * -(-4 * C // 64)
        per_split = npairs * 64 * 64 + -(-cout // 64) * 64
        assert n > 0 and n % per_split == 0, (B, H, C, cout, n)
        assert n // per_split <= B * -(-H // 2 // 4) * -(-H // 2 // 16)          # at most one split per pixel tile
    for bad in ((0, 16, 16, 8, 8), (2, 15, 16, 8, 8), (2, 16, 7, 8, 8), (2, 16, 16, 0, 8), (2, 16, 16, 8, -1),
                (2, 16, 16, 2 ** 19, 8), (2 ** 20, 2 ** 10, 2 ** 10, 8, 8), (2 ** 30, 16, 16, 8, 8)):
        assert ws(*bad) == -1, bad


def test_unshuffle_wgrad_rejects_bad_arguments():
    lib = _lib.lib()
    fn = lib.dmh_conv_unshuffle_wgrad

    def call(**kw):
        a = dict(dy=P, x=P, dw=P, db=None, work=P, B=2, H=16, W=16, C=8, Cout=8)
        a.update(kw)
        rc = fn(a['dy'], a['x'], a['dw'], a['db'], a['work'], a['B'], a['H'], a['W'], a['C'], a['Cout'], None)
        return rc, lib.dmh_last_error().decode()
    for null in ('dy', 'x', 'dw', 'work'):
        rc, msg = call(**{null: None})
        assert rc == -1 and 'dmh_conv_unshuffle_wgrad' in msg, null
    for bad in (dict(B=0), dict(B=-3), dict(H=0), dict(W=-2), dict(C=0), dict(Cout=0),
                dict(H=15), dict(W=17),                                          # odd input size
                dict(C=6), dict(Cout=10),                                        # not multiples of 4
                dict(C=2 ** 19 + 4),                                             # 4C beyond the size range
                dict(B=2 ** 12, H=2 ** 10, W=2 ** 10),                           # B*H*W overflows int
                dict(B=2 ** 30)):
        rc, msg = call(**bad)
        assert rc == -1 and 'dmh_conv_unshuffle_wgrad' in msg, (bad, rc, msg)


def test_loss_backward_ddp_rejects_bad_arguments():
    lib = _lib.lib()
    fn = lib.dmh_loss_backward_ddp

    def call(**kw):
        a = dict(out=P, target=P, w=P, dout=P, B=2, per=768, squared=0, scale=1.0)
        a.update(kw)
        rc = fn(a['out'], a['target'], a['w'], a['dout'], a['B'], a['per'], a['squared'], a['scale'], None)
        return rc, lib.dmh_last_error().decode()
    for null in ('out', 'target', 'w', 'dout'):
        rc, msg = call(**{null: None})
        assert rc == -1 and 'dmh_loss_backward_ddp' in msg, null
    for bad in (dict(B=0), dict(B=-1), dict(per=0), dict(per=-768), dict(squared=2), dict(squared=-1),
                dict(B=2 ** 30, per=2 ** 40), dict(B=3, per=2 ** 62)):          # B * per overflows
        rc, msg = call(**bad)
        assert rc == -1 and 'dmh_loss_backward_ddp' in msg, (bad, rc, msg)
