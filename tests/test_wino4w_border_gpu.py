"""GPU tests (pytest -m gpu) of the border handling of the F(4x4,3x3)-domain weight gradient (csrc/wino4w.hip): which of a lane's ten
DMA pieces a chunk on the image border fetches comes from per-lane bit masks built once and combined per chunk by class (first /
last / second-to-last column block, top / bottom tile row).  The shapes sit on the edges of every class and on the coincidences
(one column block, one tile row); tests/test_wino4_gpu.py keeps the general shapes.

Tolerance: that file's bar -- 1e-4 relative + 1e-4 of the gradient's scale against torch CPU fp32 autograd."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(a, b, rtol, atol, what=""):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max abs err {err.max():.3e}, max |ref| {np.abs(b).max():.3e}, " \
                               f"{int((~(err <= tol)).sum())} of {err.size} off, first at {np.argwhere(~(err <= tol))[0]}"
    return float(err.max())


@functools.lru_cache(maxsize=None)
def _case(n, cin, cout, h, w):
    """inputs and the torch CPU fp32 autograd gradients of one shape (computed once; nobody writes to them)"""
    gen = torch.Generator().manual_seed(77 + n * 1000 + cin + 3 * cout + 7 * h + 11 * w)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = (torch.randn(cout, cin, 3, 3, generator=gen) * 0.1).requires_grad_()
    b = torch.zeros(cout, requires_grad=True)
    gy = torch.randn(n, cout, h, w, generator=gen)
    F.conv2d(x, wt, b, padding=1).backward(gy)
    return x, gy, wt.grad.detach(), b.grad.detach()


def _wgrad(x, gy, cout, waves=None):
    """x, gy: device tensors (contiguous, possibly views into larger buffers)"""
    from probabilisticteacher_amd import _lib, ops
    lib = _lib.load()
    n, cin, h, w = x.shape
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV)
    if waves is None:
        ws = torch.empty(lib.ptmi_conv3x3_wino4_wgrad_ws_floats(n, cin, cout, h, w), device=DEV)
        _lib.call("ptmi_conv3x3_wino4_wgrad", ops._ptr(x), ops._ptr(gy), ops._ptr(dw), ops._ptr(db), ops._ptr(ws), n, cin, cout, h, w,
                  0, ops._stream())
    else:
        ws = torch.empty(lib.ptmi_conv3x3_wino4_wgrad_ws_floats_waves(n, cin, cout, h, w, waves), device=DEV)
        _lib.call("ptmi_conv3x3_wino4_wgrad_waves", ops._ptr(x), ops._ptr(gy), ops._ptr(dw), ops._ptr(db), ops._ptr(ws), n, cin, cout,
                  h, w, 0, waves, ops._stream())
    return dw, db


def _check(dw, db, dw_ref, db_ref):
    close(dw, dw_ref, 1e-4, 1e-4 * float(dw_ref.abs().max()), "dW")
    close(db, db_ref, 1e-4, 1e-4 * float(db_ref.abs().max()), "db")


# A chunk is 4 rows x 16 columns; its x patch is rows y0 - 1 .. y0 + 4, columns x0 - 4 .. x0 + 19.  W: 16 one whole block; 19 / 20 / 21,
# 35 / 36 / 37 both sides of `x0 + 20 <= W` with a last block of 3, 4, 5 columns (3: the second-to-last block's halo piece straddles
# the edge; W = 19: that block is also the first); 51, 83 the same with interior blocks.  H: 1, 2, 4 a single tile row with 1, 2, 4
# rows; 5, 6, 8, 9 both sides of `y0 + 5 <= H` and a last tile row of 1, 2, 4, 1 rows; 7 (with 37) the one of 3.
BORDER_SHAPES = [
    (1, 32, 64, 1, 16), (1, 40, 72, 4, 16), (2, 32, 64, 5, 16), (1, 32, 64, 9, 16),
    (1, 32, 64, 2, 19), (1, 40, 72, 8, 19), (2, 32, 64, 5, 19),
    (1, 32, 64, 1, 20), (1, 32, 64, 5, 20), (1, 40, 72, 9, 20),
    (1, 32, 64, 4, 21), (2, 40, 72, 6, 21),
    (1, 32, 64, 2, 35), (1, 64, 128, 9, 35),
    (1, 40, 72, 5, 36), (1, 32, 64, 8, 36),
    (1, 32, 64, 1, 37), (1, 40, 72, 6, 37), (1, 32, 64, 7, 37),
    (1, 32, 64, 4, 51), (1, 40, 72, 9, 51),
    (1, 32, 64, 2, 83), (1, 40, 72, 5, 83), (1, 64, 128, 8, 83),
    # 150 chunks (5 tile rows x 10 column blocks x 3 images) over 64 splits of 3: splits begin mid-row and mid-image, run across the
    # row and image ends, and the last splits are empty
    (3, 40, 72, 18, 150),
]


@pytest.mark.parametrize("n,cin,cout,h,w", BORDER_SHAPES)
def test_wino4w_border_classes(n, cin, cout, h, w):
    """dW, db at the edges of every border class against torch CPU fp32 autograd (1e-4 relative + 1e-4 of the gradient's scale)"""
    x, gy, dw_ref, db_ref = _case(n, cin, cout, h, w)
    dw, db = _wgrad(x.to(DEV), gy.to(DEV), cout)
    _check(dw, db, dw_ref, db_ref)


def _nan_framed(t, pad):
    """a contiguous device view of t's values in the middle of a buffer that is NaN on both sides"""
    buf = torch.full((pad + t.numel() + pad,), float("nan"), device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("n,cin,cout,h,w", [
    (2, 40, 72, 3, 13),       # a single tile row and a single column block: every class at once
    (2, 40, 72, 13, 51),      # all nine border positions and interior chunks; last block 3 columns wide
])
def test_wino4w_nothing_invalid_is_fetched(n, cin, cout, h, w):
    """x and dY as views into larger buffers whose surroundings are NaN: the first chunk's base (row -1, column -4 of the first
    channel) lies before the tensor and the last chunk's patch reaches past it.  A piece wrongly taken as valid there -- above the
    first channel, below the last one, or in the next plane's rows -- brings a NaN into dW or db."""
    x, gy, dw_ref, db_ref = _case(n, cin, cout, h, w)
    pad = (w + 8) * 6
    xbuf, xv = _nan_framed(x, pad)
    gbuf, gv = _nan_framed(gy, pad)
    dw, db = _wgrad(xv, gv, cout)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), "a fetch reached outside the tensors"
    _check(dw, db, dw_ref, db_ref)
    assert bool(torch.isnan(xbuf[:pad]).all() and torch.isnan(xbuf[-pad:]).all() and torch.isnan(gbuf[:pad]).all()
                and torch.isnan(gbuf[-pad:]).all())


def test_wino4w_border_bitwise_repeatable():
    """Two launches give the same bits; so do two launches of the `waves` entry point with 1 and with 3 fills of the chip"""
    n, cin, cout, h, w = 3, 40, 72, 9, 83
    x, gy, dw_ref, db_ref = _case(n, cin, cout, h, w)
    xd, gd = x.to(DEV), gy.to(DEV)
    for waves in (None, 1, 3):
        dw, db = _wgrad(xd, gd, cout, waves)
        dw2, db2 = _wgrad(xd, gd, cout, waves)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), f"waves {waves}: the result depends on the launch"
        _check(dw, db, dw_ref, db_ref)
