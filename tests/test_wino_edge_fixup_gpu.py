"""GPU tests (pytest -m gpu) of the patch fix-up of the F(4x4,3x3) forward / dgrad kernel (csrc/wino4p.hip): a 16-byte patch piece
that an image's right edge cuts is fetched whole and its words past the edge are zeroed in LDS at the chunk hand-over, from
per-tile state built in make_next.  Forward (epilogue 1, and 4 where H and W are even) and dgrad (epilogues 2, 3) through
ops.conv3x3_pack / ops.conv3x3_raw (epilogue 4: ops.conv3x3_relu_pool_nograd), under both tile schedules.

Reference: torch CPU.  Tolerance: the bar of tests/test_wino4_gpu.py -- 1e-4 relative + 1e-4 absolute on unit-scale outputs
(dgrad: + 2e-4).  Every launch is repeated and must give the same bits."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n, cin, cout, H, W): the smallest maps on which a 64-column tile straddles zero, one or several image edges and crosses an image
# boundary in the flat column walk
SHAPES = [
    (3, 64, 64, 9, 13),       # period 16: several image edges inside ONE 72-column patch; two bands, the second with one valid row; W & 3 = 1
    (2, 64, 64, 8, 62),       # period = tile width: the edge sits at the same patch column in every tile; W & 3 = 2
    (2, 64, 64, 17, 83),      # the conv5 width: W & 3 = 3; the last band has one row
    (1, 64, 64, 5, 166),      # the conv4 width
    (2, 64, 64, 8, 64),       # W & 3 = 0: the no-fix-up path
    (1, 64, 128, 4, 3),       # W < 4
]
_REF = {}


def _case(n, cin, cout, h, w):
    """inputs and torch CPU references of a shape, computed once"""
    key = (n, cin, cout, h, w)
    if key not in _REF:
        gen = torch.Generator().manual_seed(31 + n * 1000 + cin + cout + h + w)
        x = torch.randn(n, cin, h, w, generator=gen).requires_grad_()
        wt = torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cin))
        b = torch.randn(cout, generator=gen) * 0.1
        gy = torch.randn(n, cout, h, w, generator=gen)
        mask_src = torch.randn(n, cin, h, w, generator=gen)
        y = F.conv2d(x, wt, b, padding=1)
        y.backward(gy)
        _REF[key] = dict(x=x.detach(), wt=wt, b=b, gy=gy, mask=mask_src, relu=F.relu(y.detach()), dx=x.grad.clone())
    return _REF[key]


def _close(a, b, rtol, atol, what):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    print(f"{what}: max abs err {err.max():.3e}, max |ref| {np.abs(b).max():.3e}")
    assert (err <= tol).all(), f"{what}: max abs err {err.max():.3e}, max |ref| {np.abs(b).max():.3e}, " \
                               f"{int((err > tol).sum())} of {err.size} off, first at {np.argwhere(err > tol)[0]}"


@pytest.mark.parametrize("schedule", ["static", "dynamic"])
@pytest.mark.parametrize("n,cin,cout,h,w", SHAPES)
def test_wino4p_edge_fixup(n, cin, cout, h, w, schedule):
    from probabilisticteacher_amd import ops
    c = _case(n, cin, cout, h, w)
    assert ops._conv_kind(cin, cout, (h, w)) == "wino4" and ops._conv_kind(cout, cin, (h, w)) == "wino4" and ops._WINO4_FAMILY == "wino4p"
    x, wt, b, gy, mask = (c[k].to(DEV) for k in ("x", "wt", "b", "gy", "mask"))
    ops.set_tile_schedule(schedule)
    try:
        def twice(f, what):
            y1, y2 = f(), f()
            assert torch.equal(y1, y2), f"{what}: two launches differ"
            return y1

        wp = ops.conv3x3_pack(wt, 0, 1, (h, w))
        _close(twice(lambda: ops.conv3x3_raw(x, wp, b, None, cout, 1), "epilogue 1"), c["relu"], 1e-4, 1e-4, "epilogue 1 (bias + relu)")
        if h % 2 == 0 and w % 2 == 0:
            _close(twice(lambda: ops.conv3x3_relu_pool_nograd(x, wt, b), "epilogue 4"), F.max_pool2d(c["relu"], 2, 2), 1e-4, 1e-4,
                   "epilogue 4 (bias + relu + pool)")
        wd2 = ops.conv3x3_pack(wt, 1, 2, (h, w))
        _close(twice(lambda: ops.conv3x3_raw(gy, wd2, None, None, cin, 2), "epilogue 2"), c["dx"], 1e-4, 2e-4, "dgrad")
        wd3 = ops.conv3x3_pack(wt, 1, 3, (h, w))
        _close(twice(lambda: ops.conv3x3_raw(gy, wd3, None, mask, cin, 3), "epilogue 3"), c["dx"] * (c["mask"] > 0), 1e-4, 2e-4,
               "dgrad + relu mask")
    finally:
        ops.set_tile_schedule("static")
