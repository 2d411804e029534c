"""The chunk hand-over of the F(4x4,3x3) kernels (csrc/wino4p.hip forward / dgrad, csrc/wino4w.hip weight gradient): the counted
vmcnt wait, the fix-up of words past the image edge behind a wave-uniform branch, the drain and the barrier -- on shapes whose
chunks sit on the image border, follow an interior chunk, or cross tiles and images inside one persistent workgroup.

Reference: the direct kernels (ops.set_conv_algo("direct") / ptmi_conv3x3_wgrad) at the bars of tests/test_wino4_gpu.py.  Every
launch is repeated 20 times on the same inputs and every repeat must equal the first bit for bit: a hand-over that waits too little
shows as a rare difference of the numbers, not as a fault."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPEATS = 20


def g(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, rtol, atol, what=""):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max abs err {err.max():.3e}, max |ref| {np.abs(b).max():.3e}, " \
                               f"{int((err > tol).sum())} of {err.size} off, first at {np.argwhere(err > tol)[0]}"
    return float(err.max())


# (N, Cin, Cout, H, W)
FWD_SHAPES = [
    (2, 64, 64, 13, 21),      # every chunk borders an edge; fix-ups in every tile
    (2, 72, 96, 24, 70),      # interior chunks directly followed by last-column chunks; ragged Cout
    (1, 128, 64, 8, 131),     # W % 4 != 0, one band, many column tiles
    (3, 64, 128, 50, 83),     # a conv5-level map, three images: a persistent workgroup crosses tiles and images
]
FWD_EPILOGUES = (0, 1, 4)     # bias / bias + ReLU / bias + ReLU + 2x2 max pool
DGRAD_EPILOGUES = (2, 3)      # plain / through the producer's ReLU mask

_inputs = {}                  # shape -> device tensors
_direct = {}                  # (shape, epilogue) -> the direct kernel's output, computed once


def _fwd_inputs(shape):
    if shape not in _inputs:
        n, cin, cout, h, w = shape
        gen = g(sum(shape) + 1000 * n)
        _inputs[shape] = dict(
            x=torch.randn(n, cin, h, w, generator=gen).to(DEV),
            wt=(torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cin))).to(DEV),
            b=(torch.randn(cout, generator=gen) * 0.1).to(DEV),
            gy=torch.randn(n, cout, h, w, generator=gen).to(DEV),
            mask=torch.randn(n, cin, h, w, generator=gen).to(DEV))
    return _inputs[shape]


def _launch(shape, epi):
    """one launch of epilogue `epi` through ops under the conv algorithm / tile schedule in force"""
    from probabilisticteacher_amd import ops
    t = _fwd_inputs(shape)
    n, cin, cout, h, w = shape
    if epi == 4:
        return ops.conv3x3_relu_pool_nograd(t["x"], t["wt"], t["b"])
    if epi <= 1:
        return ops.conv3x3_raw(t["x"], ops.conv3x3_pack(t["wt"], 0, epi, (h, w)), t["b"], None, cout, epi)
    wp = ops.conv3x3_pack(t["wt"], 1, epi, (h, w))                     # dgrad: contracts over cout
    return ops.conv3x3_raw(t["gy"], wp, None, t["mask"] if epi == 3 else None, cin, epi)


def _direct_ref(shape, epi):
    from probabilisticteacher_amd import ops
    if (shape, epi) not in _direct:
        ops.set_conv_algo("direct")
        try:
            assert ops._conv_kind(shape[1], shape[2], shape[3:]) == "mfma"
            _direct[(shape, epi)] = _launch(shape, epi)
        finally:
            ops.set_conv_algo("auto")
    return _direct[(shape, epi)]


@pytest.mark.parametrize("schedule", ["static", "dynamic"])
@pytest.mark.parametrize("n,cin,cout,h,w", FWD_SHAPES)
def test_handover_forward_and_dgrad(n, cin, cout, h, w, schedule):
    from probabilisticteacher_amd import ops
    shape = (n, cin, cout, h, w)
    assert ops._conv_kind(cin, cout, (h, w)) == "wino4" and ops._conv_kind(cout, cin, (h, w)) == "wino4"
    ops.set_tile_schedule(schedule)
    try:
        for epi in FWD_EPILOGUES + DGRAD_EPILOGUES:
            ref = _direct_ref(shape, epi)
            first = _launch(shape, epi)
            err = close(first, ref, 1e-4, 1e-4, f"epilogue {epi} vs the direct kernel")
            print(f"{shape} {schedule} epilogue {epi}: max abs err {err:.2e}")
            for rep in range(1, REPEATS):
                assert torch.equal(_launch(shape, epi), first), f"epilogue {epi}: repeat {rep} differs from the first launch"
    finally:
        ops.set_tile_schedule("static")


WG_SHAPES = [
    (2, 32, 64, 9, 35),
    (2, 64, 64, 50, 83),      # (ops routes this map to the F(2x2,3x3)-domain kernel)
    (1, 96, 128, 24, 70),
    (4, 64, 64, 4, 16),       # one chunk per image: the prologue and the first hand-over
]
_wg = {}                      # shape -> (x, dy, dW, db of the direct split-K kernel)


def _wg_case(shape):
    from probabilisticteacher_amd import _lib, ops
    if shape not in _wg:
        n, cin, cout, h, w = shape
        gen = g(17 + sum(shape) + 1000 * n)
        x = torch.randn(n, cin, h, w, generator=gen).to(DEV)
        dy = torch.randn(n, cout, h, w, generator=gen).to(DEV)
        ws = torch.empty(_lib.load().ptmi_conv3x3_wgrad_ws_floats(n, cin, cout, h, w), device=DEV)
        dw, db = torch.empty(cout, cin, 3, 3, device=DEV), torch.empty(cout, device=DEV)
        _lib.call("ptmi_conv3x3_wgrad", ops._ptr(x), ops._ptr(dy), ops._ptr(dw), ops._ptr(db), ops._ptr(ws), n, cin, cout, h, w, 0,
                  ops._stream())
        _wg[shape] = (x, dy, dw, db)
    return _wg[shape]


def _wino4_wgrad(x, dy, cout, waves):
    """the F(4x4,3x3)-domain weight gradient: through ops.conv3x3_wgrad where ops routes the shape to it, else (maps below its fill
    bar, fewer than 64 channels) through ptmi_conv3x3_wino4_wgrad_waves itself"""
    from probabilisticteacher_amd import _lib, ops
    n, cin, h, w = x.shape
    if ops._wgrad_kind(cin, cout, h, w) == "wino4w":
        ops.set_wgrad_waves(waves)
        try:
            return ops.conv3x3_wgrad(x, dy, cout)
        finally:
            ops.set_wgrad_waves(1)
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
    db = torch.full((cout,), float("nan"), device=DEV)
    ws = torch.empty(_lib.load().ptmi_conv3x3_wino4_wgrad_ws_floats_waves(n, cin, cout, h, w, waves), device=DEV)
    _lib.call("ptmi_conv3x3_wino4_wgrad_waves", ops._ptr(x), ops._ptr(dy), ops._ptr(dw), ops._ptr(db), ops._ptr(ws), n, cin, cout,
              h, w, 0, waves, ops._stream())
    return dw, db


@pytest.mark.parametrize("waves", [1, 3])
@pytest.mark.parametrize("n,cin,cout,h,w", WG_SHAPES)
def test_handover_weight_gradient(n, cin, cout, h, w, waves):
    x, dy, dw_d, db_d = _wg_case((n, cin, cout, h, w))
    dw, db = _wino4_wgrad(x, dy, cout, waves)
    scale = float(dw_d.abs().max())
    e_w = close(dw, dw_d, 1e-4, 1e-4 * scale, "dW vs the direct split-K kernel")
    e_b = close(db, db_d, 1e-4, 1e-4 * float(db_d.abs().max()), "db vs the direct split-K kernel")
    print(f"{(n, cin, cout, h, w)} waves {waves}: dW max abs err {e_w:.2e} (scale {scale:.2e}), db {e_b:.2e}")
    for rep in range(1, REPEATS):
        dw2, db2 = _wino4_wgrad(x, dy, cout, waves)
        assert torch.equal(dw2, dw) and torch.equal(db2, db), f"repeat {rep} differs from the first launch"
