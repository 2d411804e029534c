"""GPU tests (pytest -m gpu) of the chunk set-up of the F(2x2,3x3)-domain weight gradient (csrc/wino.hip,
conv3x3_wino_wgrad_kernel<7 / 8>): patch origins stepped chunk by chunk, one offsets array rewritten on a class change, and
fix-up stores from per-lane LDS offsets built once.  ptmi_conv3x3_wino_wgrad is called directly (ops would route maps this
small elsewhere), with n = 3 so that a split's chunk range crosses image boundaries and row wraps.

Reference: torch CPU float64 autograd.  Tolerance, as tests/test_wino_gpu.py has it for this kernel: 1e-4 relative + 1e-4 of
the gradient's scale.  Every case is launched twice and must give the same bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n, cin, cout, H, W)
SHAPES = [
    (3, 64, 64, 5, 83),       # KSN = 7, three column blocks, last width 27 (one word to fix), odd H: both bottom-row cases
    (3, 64, 64, 4, 28),       # ONE column block, first and last at once, ends on a piece boundary: nothing to fix
    (3, 64, 64, 2, 29),       # last block of width 1: three words to fix
    (3, 64, 64, 3, 30),       # ... 2
    (3, 64, 64, 6, 31),       # ... 3
    (3, 64, 64, 1, 33),       # H = 1: the only tile row is top and bottom
    (3, 64, 64, 5, 61),       # KSN = 8 (16 tile pairs per row: 2 x 8 against 3 x 7), last block 29 wide
    (3, 70, 100, 5, 83),      # channel counts that are not multiples of 64: pieces of channels outside the tensor
]


def _wgrad(x, gy, cout):
    from probabilisticteacher_amd import _lib, ops
    n, cin, h, w = x.shape
    ws = torch.full((_lib.load().ptmi_conv3x3_wino_wgrad_ws_floats(n, cin, cout, h, w),), float("nan"), device=DEV)
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV)
    _lib.call("ptmi_conv3x3_wino_wgrad", ops._ptr(x), ops._ptr(gy), ops._ptr(dw), ops._ptr(db), ops._ptr(ws), n, cin, cout, h, w,
              0, ops._stream())
    return dw, db


def _close(a, b, rtol, atol, what):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    print(f"{what}: max abs err {err.max():.3e}, max |ref| {np.abs(b).max():.3e}")
    assert (err <= tol).all(), f"{what}: max abs err {err.max():.3e}, max |ref| {np.abs(b).max():.3e}, " \
                               f"{int((err > tol).sum())} of {err.size} off, first at {np.argwhere(err > tol)[0]}"


@pytest.mark.parametrize("n,cin,cout,h,w", SHAPES)
def test_wino_wgrad_setup(n, cin, cout, h, w):
    gen = torch.Generator().manual_seed(23 + n * 1000 + cin + cout + h + w)
    x = torch.randn(n, cin, h, w, generator=gen)
    gy = torch.randn(n, cout, h, w, generator=gen)
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wt, b, padding=1).backward(gy.double())
    xd, gd = x.to(DEV), gy.to(DEV)
    dw, db = _wgrad(xd, gd, cout)
    _close(dw, wt.grad, 1e-4, 1e-4 * float(wt.grad.abs().max()), "dW")
    _close(db, b.grad, 1e-4, 1e-4 * float(b.grad.abs().max()), "db")
    dw2, db2 = _wgrad(xd, gd, cout)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two launches differ"
