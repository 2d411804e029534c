"""GPU (pytest -m gpu): MODEL.ROI_BOX_HEAD.NUM_CONV / CONV_DIM / NORM -- the ROI-mosaic kernels (csrc/roi_mosaic.hip), one conv
layer and the whole box head on the mosaic, and the trainer on such a head.

References.  Layout: the index arithmetic of tests/box_head_ref.py (bit-equal).  Mosaic GroupNorm: torch.nn.functional.group_norm +
relu per ROI in float64 with the float32 CPU result as the yardstick of tests/losses_ref.py::check -- err(got) <= max(base_rtol,
4 * err(ref32)), the constants of tests/groupnorm_ref.py.  Convolutions and the head: D2's FastRCNNConvFCHead restated on torch
modules (tests/box_head_ref.py) in float64, at the bar tests/test_wino4_gpu.py holds the 3x3 kernels to, scale-aware as
tests/test_groupnorm_gpu.py::test_backbone_parity states it: |got - ref| <= 1e-4 * max |ref| + 1e-4 * |ref|, i.e.
rel(got) = max |got - ref| / (max |ref| + |ref|) <= 1e-4; the whole head is allowed max(1e-4, 4 * rel(yardstick)), the yardstick
being the same layers through ops.conv3x3 on the un-mosaicked (R, C, 7, 7) tensor with torch's fp32 group_norm between them."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import box_head_ref as br
from tests import groupnorm_ref as gr
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_BAR = 1e-4


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from probabilisticteacher_amd import ops as _ops
    return _ops


def _call(name, *args):
    from probabilisticteacher_amd import _lib
    return _lib.call(name, *args)


def rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f"{tuple(got.shape)} vs {tuple(ref.shape)}"
    return float(((got - ref).abs() / (ref.abs().max() + ref.abs())).max())


def _shifted(t, by=1):
    """a copy of `t` that starts 4 * by bytes behind a 16-byte boundary"""
    big = torch.zeros(t.numel() + 8, device=DEV)
    v = big[by:by + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * by
    return v


# ============================================================================ pack, unpack, mask
RS = (0, 1, 63, 64, 65, 130)


@pytest.mark.parametrize("pooled", [7, 3, 6], ids=["P7", "P3", "P6_scalar_rows"])
@pytest.mark.parametrize("c", [32, 64])
def test_pack_unpack_mask(ops, c, pooled):
    """data bit-equal to the restatement, every gutter and empty cell exactly 0.0, unpack(pack(x)) == x, the mask a copy with the
    gutters zeroed (NaNs included) that leaves its input alone; outputs between guard bands, every element of a canvas written;
    the same bits with the canvases 4 bytes off the 16-byte grid.  (P = 6: 63 x 63 canvases, the dword path.)"""
    p = ops._ptr
    assert ops.ROI_MOSAIC_GN_MAX_CELL == ops.roi_mosaic_gn_max_cell()
    for r in RS:
        gen = torch.Generator().manual_seed(100 * r + c + pooled)
        x = torch.randn(r, c, pooled, pooled, generator=gen)
        want = br.mosaic_pack(x)
        _, gx, s, ncv = br.mosaic_geometry(r, pooled)
        assert tuple(want.shape) == (ncv, c, s, s) and (pooled != 7 or (gx, s, ncv) == (8, 64, -(-r // 64)))
        if r == 0:
            cv = ops.roi_mosaic_pack(x.to(DEV))
            assert tuple(cv.shape) == (0, c, s, s) and tuple(ops.roi_mosaic_unpack(cv, 0, pooled).shape) == (0, c, pooled, pooled)
            assert tuple(ops.roi_mosaic_mask(cv, 0, pooled).shape) == (0, c, s, s)
            for name in ("ptmi_roi_mosaic_pack", "ptmi_roi_mosaic_unpack", "ptmi_roi_mosaic_mask"):
                _call(name, None, None, 0, c, pooled, ops._stream())         # nothing to do: no launch, null pointers are fine
            continue
        data = br.mosaic_data_mask(r, pooled).expand_as(want)
        xg = Guarded.of(x, device=DEV).snapshot()
        cvg = Guarded(want.shape, device=DEV)
        _call("ptmi_roi_mosaic_pack", p(xg.payload), p(cvg.payload), r, c, pooled, ops._stream())
        torch.cuda.synchronize()
        cvg.assert_guards_intact(f"pack r {r}")
        xg.assert_unchanged(f"pack r {r} x")
        assert cvg.unwritten() == 0, f"pack r {r}: {cvg.unwritten()} canvas elements not written"
        got = cvg.payload.cpu()
        assert torch.equal(got, want), f"pack r {r}"
        assert bool((got[~data] == 0).all()) and int(data.sum()) == x.numel()
        # unpack
        cvg.snapshot()
        backg = Guarded(x.shape, device=DEV)
        _call("ptmi_roi_mosaic_unpack", p(cvg.payload), p(backg.payload), r, c, pooled, ops._stream())
        torch.cuda.synchronize()
        backg.assert_guards_intact(f"unpack r {r}")
        cvg.assert_unchanged(f"unpack r {r} canvas")
        assert backg.unwritten() == 0 and torch.equal(backg.payload.cpu(), x), f"unpack(pack(x)) r {r}"
        # mask: a canvas with something in every gutter and empty cell, NaNs among it
        dirty = torch.where(data, want, torch.randn(want.shape, generator=gen) + 3.0)
        dirty[~data & (torch.rand(want.shape, generator=gen) < 0.05)] = float("nan")
        dg = Guarded.of(dirty, device=DEV).snapshot()
        mg = Guarded(want.shape, device=DEV)
        _call("ptmi_roi_mosaic_mask", p(dg.payload), p(mg.payload), r, c, pooled, ops._stream())
        torch.cuda.synchronize()
        mg.assert_guards_intact(f"mask r {r}")
        dg.assert_unchanged(f"mask r {r} input")
        assert mg.unwritten() == 0 and torch.equal(mg.payload.cpu(), want), f"mask r {r}"
        # the same through canvases 4 bytes off the 16-byte grid (dword accesses)
        cs = _shifted(torch.full(want.shape, 7.0, device=DEV))
        _call("ptmi_roi_mosaic_pack", p(xg.payload), p(cs), r, c, pooled, ops._stream())
        assert torch.equal(cs.cpu(), want), f"pack r {r}, canvas moved by 4 bytes"
        xs = _shifted(torch.full(x.shape, 7.0, device=DEV), 3)
        _call("ptmi_roi_mosaic_unpack", p(cs), p(xs), r, c, pooled, ops._stream())
        assert torch.equal(xs.cpu(), x), f"unpack r {r}, canvas moved by 4 bytes"
        ms = _shifted(torch.full(want.shape, 7.0, device=DEV), 2)
        _call("ptmi_roi_mosaic_mask", p(_shifted(dirty.to(DEV))), p(ms), r, c, pooled, ops._stream())
        assert torch.equal(ms.cpu(), want), f"mask r {r}, canvases moved"


def test_pack_unpack_mask_are_each_others_backward(ops):
    r, c, pooled = 70, 32, 7
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(r, c, pooled, pooled, generator=gen).to(DEV).requires_grad_()
    cv = ops.roi_mosaic_pack(x)
    up = torch.randn(cv.shape, generator=gen)                   # something in every gutter of the incoming gradient
    cv.backward(up.to(DEV))
    assert torch.equal(x.grad.cpu(), br.mosaic_unpack(up, r, pooled))
    cv2 = cv.detach().clone().requires_grad_()
    y = ops.roi_mosaic_unpack(ops.roi_mosaic_mask(cv2, r, pooled), r, pooled)
    assert torch.equal(y, x.detach())
    g = torch.randn(y.shape, generator=gen)
    y.backward(g.to(DEV))
    assert torch.equal(cv2.grad.cpu(), br.mosaic_pack(g)), "zeros in gutters and empty cells of the gradient"


def test_abi_argument_checks(ops):
    from probabilisticteacher_amd import _lib
    lib, p, s = _lib.load(), ops._ptr, ops._stream()
    x = torch.zeros(2, 32, 7, 7, device=DEV)
    cv = torch.full((1, 32, 64, 64), 7.0, device=DEV)
    st, dg, db = (torch.full((64,), 7.0, device=DEV) for _ in range(3))
    ws = ops._mosaic_gn_ws(2, 32, 7, 32, x.device)
    gn_fwd, gn_bwd = lib.ptmi_roi_mosaic_gn_relu_fwd, lib.ptmi_roi_mosaic_gn_relu_bwd
    for fn, what in ((lambda: lib.ptmi_roi_mosaic_pack(None, p(cv), 2, 32, 7, s), "roi_mosaic_pack"),
                     (lambda: lib.ptmi_roi_mosaic_pack(p(x), p(cv), -1, 32, 7, s), "roi_mosaic_pack"),
                     (lambda: lib.ptmi_roi_mosaic_unpack(p(cv), None, 2, 32, 7, s), "roi_mosaic_unpack"),
                     (lambda: lib.ptmi_roi_mosaic_unpack(p(cv), p(x), 2, 0, 7, s), "roi_mosaic_unpack"),
                     (lambda: lib.ptmi_roi_mosaic_mask(p(cv), p(cv), 2, 32, 7, s), "roi_mosaic_mask"),
                     (lambda: lib.ptmi_roi_mosaic_mask(p(cv), p(cv), 2, 32, 0, s), "roi_mosaic_mask"),
                     (lambda: gn_fwd(p(cv), p(dg), p(db), p(cv), p(st), 2, 48, 7, 32, gr.EPS, s), "roi_mosaic_gn_relu_fwd"),
                     (lambda: gn_fwd(p(cv), p(dg), p(db), None, p(st), 2, 32, 7, 32, gr.EPS, s), "roi_mosaic_gn_relu_fwd"),
                     (lambda: gn_fwd(p(cv), p(dg), p(db), p(cv), p(st), 2, 32, 63, 32, gr.EPS, s), "roi_mosaic_gn_relu_fwd"),
                     (lambda: gn_bwd(p(cv), p(cv), p(cv), p(dg), p(st), p(cv), p(dg), p(db), 2, 32, 7, 32, None, s), "roi_mosaic_gn_relu_bwd"),
                     (lambda: gn_bwd(p(cv), p(cv), p(cv), p(dg), p(st), p(cv), p(dg), p(db), 2, 32, 7, 5, p(ws), s), "roi_mosaic_gn_relu_bwd")):
        rc = fn()
        msg = lib.ptmi_last_error().decode()
        assert rc < 0 and msg.startswith(what + ":"), (what, rc, msg)
    assert lib.ptmi_roi_mosaic_gn_ws_bytes(2, 48, 7, 32) < 0 and lib.ptmi_roi_mosaic_gn_ws_bytes(2, 2048, 7, 32) < 0
    assert lib.ptmi_roi_mosaic_gn_relu_fwd(None, None, None, None, None, 0, 32, 7, 32, gr.EPS, s) == 0
    assert lib.ptmi_roi_mosaic_gn_relu_bwd(None, None, None, None, None, None, None, None, 0, 32, 7, 32, None, s) == 0
    torch.cuda.synchronize()
    for t in (cv, st, dg, db):
        assert bool((t == 7.0).all()), "nothing above may have written an output"
    with pytest.raises(ValueError):
        ops.roi_mosaic_unpack(torch.zeros(1, 32, 64, 60, device=DEV), 2, 7)
    with pytest.raises(ValueError):
        ops.roi_mosaic_gn_relu(torch.zeros(1, 48, 64, 64, device=DEV), torch.ones(48, device=DEV), torch.zeros(48, device=DEV), 2, 7)


# ============================================================================ mosaic GroupNorm + ReLU
GN_CASES, GN_SEED = br.GN_CASES, br.GN_SEED
_GN = {}


def _gn_case(c, r, pooled, offset):
    """ROI-layout inputs, the float64 / float32 CPU references on them, and canvases with something in every gutter: computed once"""
    key = (c, r, pooled, offset)
    if key not in _GN:
        ins = gr.inputs((r, c, pooled, pooled), offset, seed=GN_SEED)
        z, gamma, beta, dy = ins
        gen = torch.Generator().manual_seed(c + r + pooled)
        data = br.mosaic_data_mask(r, pooled)
        zc, dyc = br.mosaic_pack(z), br.mosaic_pack(dy)
        zc = torch.where(data.expand_as(zc), zc, torch.randn(zc.shape, generator=gen) * 5 + offset)
        dyc = torch.where(data.expand_as(dyc), dyc, torch.randn(dyc.shape, generator=gen) * 5)
        _GN[key] = (gr.reference(*ins, True, torch.float64), gr.reference(*ins, True, torch.float32), ins, zc, dyc, data)
    return _GN[key]


def _raw_gn(ops, zc, gamma, beta, dyc, r, pooled, bufs=None, ws=None):
    """ptmi_roi_mosaic_gn_relu_fwd + _bwd on device canvases -> {"y", "stats", "dz", "dgamma", "dbeta"}"""
    c = int(zc.shape[1])
    o = bufs or {"y": torch.empty_like(zc), "stats": torch.empty(r * gr.GROUPS * 2, device=DEV), "dz": torch.empty_like(zc),
                 "dgamma": torch.empty(c, device=DEV), "dbeta": torch.empty(c, device=DEV)}
    ws = ops._mosaic_gn_ws(r, c, pooled, gr.GROUPS, zc.device) if ws is None else ws
    p = ops._ptr
    _call("ptmi_roi_mosaic_gn_relu_fwd", p(zc), p(gamma), p(beta), p(o["y"]), p(o["stats"]), r, c, pooled, gr.GROUPS, gr.EPS, ops._stream())
    _call("ptmi_roi_mosaic_gn_relu_bwd", p(dyc), p(o["y"]), p(zc), p(gamma), p(o["stats"]), p(o["dz"]), p(o["dgamma"]), p(o["dbeta"]),
          r, c, pooled, gr.GROUPS, p(ws), ops._stream())
    return o


@pytest.mark.parametrize("offset", gr.OFFSETS)
@pytest.mark.parametrize("c,r,pooled", GN_CASES)
def test_mosaic_gn_parity(ops, c, r, pooled, offset):
    """ops.roi_mosaic_gn_relu through autograd: y, dz, dgamma, dbeta on the data pixels under the project's rule; gutters and
    empty cells of y and dz exactly 0.0 whatever z and dy hold there"""
    ref64, ref32, (z, gamma, beta, dy), zc, dyc, data = _gn_case(c, r, pooled, offset)
    zd, gd, bd = (t.to(DEV).requires_grad_() for t in (zc, gamma, beta))
    y = ops.roi_mosaic_gn_relu(zd, gd, bd, r, pooled, gr.GROUPS, gr.EPS)
    y.backward(dyc.to(DEV))
    yc, dzc = y.detach().cpu(), zd.grad.cpu()
    assert bool((yc[~data.expand_as(yc)] == 0).all()) and bool((dzc[~data.expand_as(dzc)] == 0).all())
    got = {"y": br.mosaic_unpack(yc, r, pooled), "dz": br.mosaic_unpack(dzc, r, pooled), "dgamma": gd.grad, "dbeta": bd.grad}
    errs = gr.check_all(got, ref64, ref32, f"C {c} R {r} P {pooled} offset {offset}")
    print(f"[box_head] mosaic gn C {c} R {r} P {pooled} offset {offset}: " +
          ", ".join(f"{k} {e:.2e} (fp32 cpu {e32:.2e})" for k, (e, e32) in errs.items()))
    assert 0.2 < float((got["y"] == 0).float().mean()) < 0.8


def test_mosaic_gn_statistics_of_a_large_mean(ops):
    """mean 1000, deviation 1.  The yardstick rule does not reach this regime (tests/groupnorm_ref.py: the fp32 CPU result is
    itself off by more than YARDSTICK_CAP there), so, as tests/test_groupnorm_gpu.py::test_statistics_of_a_large_mean does, mean and
    rstd are held against float64 -- 2e-7 and 1e-6 relative, its bounds: half an fp32 ulp of the mean is 6e-8, and the variance of
    the fp32 inputs over 98 values is exact to ~1e-6 -- and y to what an fp32 mean allows: z - mean is exact, the mean is within one
    ulp(1000) = 6.1e-5 of the true one, so |y - y64| <= 6.1e-5 * rstd * |gamma| + 1e-5 * |y64|."""
    r, c, pooled = 65, 64, 7
    gen = torch.Generator().manual_seed(9)
    z = torch.randn(r, c, pooled, pooled, generator=gen) + 1000.0
    gamma, beta = 1.0 + (torch.rand(c, generator=gen) - 0.5), torch.rand(c, generator=gen) - 0.5
    zc = br.mosaic_pack(z)
    o = _raw_gn(ops, zc.to(DEV), gamma.to(DEV), beta.to(DEV), torch.zeros(zc.shape, device=DEV), r, pooled)
    runs = z.double().view(r * gr.GROUPS, -1)
    mean, var = runs.mean(1), runs.var(1, unbiased=False)
    stats = o["stats"].view(-1, 2).cpu().double()
    e_mean = float(((stats[:, 0] - mean).abs() / mean).max())
    rstd = 1.0 / torch.sqrt(var + gr.EPS)
    e_rstd = float(((stats[:, 1] - rstd).abs() / rstd).max())
    y64 = F.relu(F.group_norm(z.double(), gr.GROUPS, gamma.double(), beta.double(), gr.EPS))
    y = br.mosaic_unpack(o["y"].cpu(), r, pooled).double()
    bound = 6.1e-5 * rstd.view(r, gr.GROUPS, 1, 1, 1) * gamma.double().abs().view(1, gr.GROUPS, c // gr.GROUPS, 1, 1) + \
        1e-5 * y64.view(r, gr.GROUPS, c // gr.GROUPS, pooled, pooled).abs()
    over = ((y - y64).abs().view_as(bound) / bound).max()
    print(f"[box_head] large mean: mean {e_mean:.2e}, rstd {e_rstd:.2e}, y at {float(over):.3f} of its bound")
    assert e_mean <= 2e-7 and e_rstd <= 1e-6 and float(over) <= 1.0


def test_mosaic_gn_same_bits_whatever_the_address(ops):
    """two launches; after an unrelated allocation; every canvas 4, 8, 12 bytes off the 16-byte grid"""
    for c, r, pooled in ((32, 65, 7), (256, 130, 7), (64, 65, 3), (32, 65, 6)):
        _, _, (_, gamma, beta, _), zc, dyc, _ = _gn_case(c, r, pooled, 3.0)
        zd, dyd, g, b = (t.to(DEV) for t in (zc, dyc, gamma, beta))
        first = {k: v.clone() for k, v in _raw_gn(ops, zd, g, b, dyd, r, pooled).items()}
        again = _raw_gn(ops, zd, g, b, dyd, r, pooled)
        assert all(torch.equal(first[k], again[k]) for k in first), "two launches"
        junk = torch.randn(123457, device=DEV)
        later = _raw_gn(ops, zd.clone(), g.clone(), b.clone(), dyd.clone(), r, pooled)
        assert all(torch.equal(first[k], later[k]) for k in first), "after an unrelated allocation"
        del junk
        for shift in (1, 2, 3):
            bufs = {"y": _shifted(torch.empty_like(zd), shift), "dz": _shifted(torch.empty_like(zd), (shift + 1) % 4),
                    "stats": torch.empty(r * gr.GROUPS * 2, device=DEV), "dgamma": torch.empty(c, device=DEV),
                    "dbeta": torch.empty(c, device=DEV)}
            o = _raw_gn(ops, _shifted(zd, shift), g, b, _shifted(dyd, shift), r, pooled, bufs)
            for k in first:
                assert torch.equal(first[k], o[k]), f"C {c} R {r} P {pooled}: {k} with the canvases moved by {4 * shift} bytes"


def test_mosaic_gn_guard_bands(ops):
    """y, dz, mean_rstd, dgamma, dbeta and the workspace between guard bands: every guard word intact, every element of the
    outputs written (gutters and empty cells included), the inputs unchanged"""
    from probabilisticteacher_amd import _lib
    for c, r, pooled in ((32, 1, 7), (64, 65, 7), (256, 130, 7), (64, 65, 3), (32, 65, 6)):
        _, _, (_, gamma, beta, _), zc, dyc, _ = _gn_case(c, r, pooled, 0.0)
        zg, gg, bg, dg = (Guarded.of(t, device=DEV).snapshot() for t in (zc, gamma, beta, dyc))
        bufs = {"y": Guarded(zc.shape, device=DEV), "dz": Guarded(zc.shape, device=DEV),
                "stats": Guarded((r * gr.GROUPS * 2,), device=DEV), "dgamma": Guarded((c,), device=DEV), "dbeta": Guarded((c,), device=DEV)}
        nbytes = int(_lib.load().ptmi_roi_mosaic_gn_ws_bytes(r, c, pooled, gr.GROUPS))
        assert nbytes > 0 and nbytes % 256 == 0
        ws = Guarded((nbytes,), torch.uint8, front=65536, back=65536, device=DEV)
        o = _raw_gn(ops, zg.payload, gg.payload, bg.payload, dg.payload, r, pooled, {k: v.payload for k, v in bufs.items()}, ws.payload)
        torch.cuda.synchronize()
        for k, v in bufs.items():
            v.assert_guards_intact(f"C {c} R {r} P {pooled} {k}")
            assert v.unwritten() == 0, f"C {c} R {r} P {pooled} {k}: {v.unwritten()} elements not written"
        ws.assert_guards_intact(f"C {c} R {r} P {pooled} workspace")
        for t, name in ((zg, "z"), (gg, "gamma"), (bg, "beta"), (dg, "dy")):
            t.assert_unchanged(f"C {c} R {r} P {pooled} {name}")
        plain = _raw_gn(ops, zc.to(DEV), gamma.to(DEV), beta.to(DEV), dyc.to(DEV), r, pooled)
        assert all(torch.equal(plain[k].reshape(-1), o[k].reshape(-1)) for k in plain)


# ============================================================================ one conv layer on the mosaic
def _close(got, ref, what, bar=CONV_BAR):
    e = rel(got, ref)
    print(f"[box_head] {what}: rel err {e:.3e} (bar {bar:.3e})")
    assert e <= bar, f"{what}: rel err {e:.3e} > {bar:.3e}"
    return e


@pytest.mark.parametrize("norm", ["", "GN"])
def test_one_conv_layer_on_the_mosaic(ops, norm):
    """pack -> ops.conv3x3 -> mask | mosaic GroupNorm -> unpack against conv2d (-> group_norm) -> relu per ROI in float64: output,
    dx, dW, db / dgamma, dbeta; the gutters of the layer's output are exactly zero (and were not before the mask)"""
    r, c, pooled = 70, 64, 7
    gen = torch.Generator().manual_seed(11)
    x = torch.relu(torch.randn(r, c, pooled, pooled, generator=gen))
    w = torch.randn(c, c, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * c))
    b = torch.zeros(c) if norm else torch.rand(c, generator=gen) - 0.5
    gamma, beta = 1.0 + (torch.rand(c, generator=gen) - 0.5), torch.rand(c, generator=gen) - 0.5
    up = torch.randn(r, c, pooled, pooled, generator=gen)
    x64, w64, b64, g64, be64 = (t.double().requires_grad_() for t in (x, w, b, gamma, beta))
    t64 = F.conv2d(x64, w64, b64, padding=1)
    out64 = F.relu(F.group_norm(t64, gr.GROUPS, g64, be64, gr.EPS) if norm else t64)
    (out64 * up.double()).sum().backward()
    xd, wd, bd, gd, bed = (t.to(DEV).requires_grad_() for t in (x, w, b, gamma, beta))
    cv = ops.roi_mosaic_pack(xd)
    data = br.mosaic_data_mask(r, pooled)
    if norm:
        t = ops.conv3x3(cv, wd, ops.zero_bias(c, DEV), False)
        m = ops.roi_mosaic_gn_relu(t, gd, bed, r, pooled, gr.GROUPS, gr.EPS)
    else:
        t = ops.conv3x3(cv, wd, bd, True)
        m = ops.roi_mosaic_mask(t, r, pooled)
    assert bool((t.detach().cpu()[~data.expand_as(t)] != 0).any()), "the convolution leaves something in the gutters"
    assert bool((m.detach().cpu()[~data.expand_as(m)] == 0).all()), "gutters and empty cells of the layer's output"
    out = ops.roi_mosaic_unpack(m, r, pooled)
    (out * up.to(DEV)).sum().backward()
    _close(out, out64, f"conv layer norm {norm!r} out")
    _close(xd.grad, x64.grad, f"conv layer norm {norm!r} dx")
    _close(wd.grad, w64.grad, f"conv layer norm {norm!r} dW")
    if norm:
        _close(gd.grad, g64.grad, "conv layer GN dgamma")
        _close(bed.grad, be64.grad, "conv layer GN dbeta")
    else:
        _close(bd.grad, b64.grad, "conv layer db")


# ============================================================================ the whole head
HEAD = ["MODEL.ROI_BOX_HEAD.NUM_CONV", 2, "MODEL.ROI_BOX_HEAD.CONV_DIM", 64, "MODEL.ROI_BOX_HEAD.NUM_FC", 1,
        "MODEL.ROI_BOX_HEAD.FC_DIM", 32]


def _cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "MODEL.ANCHOR_GENERATOR.NAME", "DifferentiableAnchorGenerator",
        "UNSUPNET.BURN_UP_STEP", 2, "SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEED", 0] + list(opts))


def _yardstick(ops, params, x, up, norm):
    """the same layers through ops.conv3x3 on the un-mosaicked (R, C, 7, 7) tensor, torch's fp32 group_norm between them, ops.linear
    behind: parent-commit code -> {"out", "dx", parameter name: gradient}"""
    leaves = {k: v.detach().clone().to(DEV).requires_grad_() for k, v in params.items()}
    xd = x.to(DEV).requires_grad_()
    t = xd
    for k in (1, 2):
        if norm:
            t = ops.conv3x3(t, leaves[f"conv{k}.weight"], ops.zero_bias(64, DEV), False)
            t = F.relu(F.group_norm(t, gr.GROUPS, leaves[f"conv{k}.norm.weight"], leaves[f"conv{k}.norm.bias"], gr.EPS))
        else:
            t = ops.conv3x3(t, leaves[f"conv{k}.weight"], leaves[f"conv{k}.bias"], True)
    out = ops.linear(t.flatten(1), leaves["fc1.weight"], leaves["fc1.bias"], True)
    (out * up.to(DEV)).sum().backward()
    res = {"out": out.detach(), "dx": xd.grad}
    res.update({k: v.grad for k, v in leaves.items()})
    return res


@pytest.mark.parametrize("norm", ["", "GN"])
def test_whole_head_against_float64(ops, norm):
    """FastRCNNConvFCHead (NUM_CONV 2, CONV_DIM 64, NUM_FC 1, FC_DIM 32) on 70 ROIs of 64 channels: output and every gradient
    against the float64 restatement, bar max(1e-4, 4 * the yardstick's own error) per tensor.

    Measured on an MI355X (rel err = max |got - ref| / (max |ref| + |ref|); mosaic / yardstick; every bar is 1e-4):
        NORM ""    out 9.39e-07 / 9.39e-07, dx 1.21e-06 / 1.21e-06, conv1.weight 9.25e-07 / 7.97e-07, conv1.bias 6.74e-07 / 6.42e-07,
                   conv2.weight 6.46e-07 / 5.67e-07, conv2.bias 1.23e-07 / 1.87e-07, fc1.weight 8.10e-07 / 8.10e-07,
                   fc1.bias 7.64e-08 / 7.64e-08
        NORM "GN"  out 8.75e-07 / 1.05e-06, dx 1.40e-06 / 1.36e-06, conv1.weight 1.15e-06 / 9.62e-07, conv1.norm.weight 2.01e-06 /
                   2.25e-06, conv1.norm.bias 1.79e-06 / 1.65e-06, conv2.weight 1.04e-06 / 6.86e-07, conv2.norm.weight 9.30e-07 /
                   8.19e-07, conv2.norm.bias 1.06e-07 / 1.37e-07, fc1.weight 1.16e-06 / 1.19e-06, fc1.bias 9.44e-08 / 9.44e-08"""
    from probabilisticteacher_amd.modeling.backbone import ShapeSpec
    from probabilisticteacher_amd.modeling.roi_heads import build_box_head
    r, c, pooled = 70, 64, 7
    torch.manual_seed(13)
    gen = torch.Generator().manual_seed(14)
    ref = br.RefHead(c, pooled, 2, 64, 1, 32, norm)
    br.perturb_(ref, gen)
    head = build_box_head(_cfg(*HEAD, "MODEL.ROI_BOX_HEAD.NORM", norm), ShapeSpec(channels=c, height=pooled, width=pooled))
    head.load_state_dict(ref.state_dict())
    head.to(DEV)
    x = torch.relu(torch.randn(r, c, pooled, pooled, generator=gen))
    up = torch.randn(r, 32, generator=gen)
    want = br.reference(ref, x, up, torch.float64)
    yard = _yardstick(ops, ref.state_dict(), x, up, norm)
    xd = x.to(DEV).requires_grad_()
    out = head(xd)
    assert tuple(out.shape) == (r, 32)
    (out * up.to(DEV)).sum().backward()
    got = {"out": out.detach(), "dx": xd.grad}
    got.update({n: p.grad for n, p in head.named_parameters()})
    assert set(got) == set(want) == set(yard)
    failed = []
    for k in want:
        e, ey = rel(got[k], want[k]), rel(yard[k], want[k])
        bar = max(CONV_BAR, 4 * ey)
        print(f"[box_head] whole head norm {norm!r} {k}: {e:.2e} / {ey:.2e} (bar {bar:.2e})")
        if not e <= bar:
            failed.append((k, e, bar))
    assert not failed, failed


def test_head_without_fc_and_without_rois(ops):
    """NUM_FC 0: the output stays (R, CONV_DIM, P, P); R = 0: empty tensors of the right shape, nothing launched"""
    from probabilisticteacher_amd import _lib
    from probabilisticteacher_amd.modeling.backbone import ShapeSpec
    from probabilisticteacher_amd.modeling.roi_heads import build_box_head
    torch.manual_seed(15)
    head = build_box_head(_cfg("MODEL.ROI_BOX_HEAD.NUM_CONV", 1, "MODEL.ROI_BOX_HEAD.CONV_DIM", 64, "MODEL.ROI_BOX_HEAD.NUM_FC", 0,
                               "MODEL.ROI_BOX_HEAD.NORM", "GN"), ShapeSpec(channels=64, height=7, width=7)).to(DEV)
    x = torch.relu(torch.randn(5, 64, 7, 7, generator=torch.Generator().manual_seed(16)))
    out = head(x.to(DEV))
    assert tuple(out.shape) == (5, 64, 7, 7) and head.output_size == 64 * 49
    t64 = F.conv2d(x.double(), head.conv1.weight.detach().cpu().double(), None, padding=1)
    _close(out, F.relu(F.group_norm(t64, 32, head.conv1.norm.weight.detach().cpu().double(),
                                    head.conv1.norm.bias.detach().cpu().double(), 1e-5)), "NUM_FC 0 head")
    calls, real = [], _lib.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    _lib.call = spy
    try:
        empty = head(torch.zeros(0, 64, 7, 7, device=DEV))
    finally:
        _lib.call = real
    assert tuple(empty.shape) == (0, 64, 7, 7) and calls == []
    with_fc = build_box_head(_cfg(*HEAD), ShapeSpec(channels=64, height=7, width=7)).to(DEV)
    assert tuple(with_fc(torch.zeros(0, 64, 7, 7, device=DEV)).shape) == (0, 32)


def test_more_rois_than_a_chunk(ops, monkeypatch):
    """the ROI list is cut into packs of ops.ROI_MOSAIC_CHUNK: with a chunk of 64 the 150 ROIs of this call go through three packs
    and give what one pack gives, bit for bit in forward (a ROI's result does not depend on its cell)"""
    from probabilisticteacher_amd.modeling.backbone import ShapeSpec
    from probabilisticteacher_amd.modeling.roi_heads import build_box_head
    assert ops.ROI_MOSAIC_CHUNK == 8192
    torch.manual_seed(17)
    head = build_box_head(_cfg(*HEAD, "MODEL.ROI_BOX_HEAD.NORM", "GN"), ShapeSpec(channels=64, height=7, width=7)).to(DEV)
    x = torch.relu(torch.randn(150, 64, 7, 7, generator=torch.Generator().manual_seed(18))).to(DEV)
    one = head(x)
    one.sum().backward()
    g_one = {n: p.grad.clone() for n, p in head.named_parameters()}
    head.zero_grad()
    monkeypatch.setattr(ops, "ROI_MOSAIC_CHUNK", 64)
    three = head(x)
    three.sum().backward()
    assert torch.equal(one, three)
    for n, p in head.named_parameters():
        _close(p.grad, g_one[n], f"chunked {n}")


# ============================================================================ the trainer
NEW_ENTRIES = ("ptmi_roi_mosaic_pack", "ptmi_roi_mosaic_unpack", "ptmi_roi_mosaic_gn_relu_fwd", "ptmi_roi_mosaic_gn_relu_bwd")
GN_HEAD = HEAD + ["MODEL.ROI_BOX_HEAD.NORM", "GN"]


def _spy_step(tr, batch):
    """one run_step with the library calls logged on tr.calls and what the optimiser tail saw on tr.seen"""
    from probabilisticteacher_amd import _lib
    real = tr._clip_and_step

    def recording(clip_norm):
        tr.seen = tuple(t.clone() for t in (tr.student.trainable(), tr.student.grad, tr.momentum_buf))
        return real(clip_norm)
    tr._clip_and_step = recording
    tr.calls, call = [], _lib.call

    def spy(name, *a):
        tr.calls.append(name)
        return call(name, *a)
    _lib.call = spy
    try:
        return dict(tr.run_step(batch))
    finally:
        _lib.call = call
        tr._clip_and_step = real


def _trainer(cfg):
    """A fresh trainer from SEED in a regime where the unsupervised losses are defined (tests/test_groupnorm_gpu.py::_trainer):
    the config's warm-up stays on and one foreground class starts with a logit bias of +1, so that the teacher calls proposals
    foreground by construction, not by luck."""
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    seed_all_rng(cfg.SEED)
    tr = PTrainer(cfg)
    with torch.no_grad():
        for model in (tr.model, tr.model_teacher):
            model.roi_heads.box_predictor.cls_score.bias[0] = 1.0
    return tr


def _strip(metrics):
    return {k: v for k, v in metrics.items() if k not in ("data_time", "time")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from bench import synth_records
    from probabilisticteacher_amd import checkpoint
    gen = torch.Generator().manual_seed(77)
    K = _cfg().MODEL.ROI_HEADS.NUM_CLASSES
    batches = [tuple(synth_records(gen, 2, 192, 256, K, DEV) for _ in range(4)) for _ in range(4)]
    out = {"batches": batches}
    a = _trainer(_cfg(*GN_HEAD))
    out["a"], out["a_metrics"], out["a_seen"], out["a_calls"] = a, [], [], []
    path = str(tmp_path_factory.mktemp("box_head") / "after3.pth")
    for i, batch in enumerate(batches):
        if i == 3:
            checkpoint.save_checkpoint(a, path)
            out["streams"] = (a._rng.getstate(), a._key_gen.get_state())
            out["ema"] = (a.student.flat.clone(), a.teacher.flat.clone())      # what the EMA of step 3 starts from
        out["a_metrics"].append(_spy_step(a, batch))
        out["a_seen"].append(a.seen)
        out["a_calls"].append(a.calls)
    out["teacher_after"] = a.teacher.flat.clone()
    torch.cuda.synchronize()
    b = _trainer(_cfg(*GN_HEAD))
    out["b"], out["b_metrics"] = b, [_spy_step(b, batch) for batch in batches]
    # a fresh trainer that resumes from the file written after three steps; the checkpoint does not hold the random streams
    # (shrink-paste ratio, sampling keys), so the test carries them over
    c = _trainer(_cfg(*GN_HEAD))
    checkpoint.load_checkpoint(c, path, resume=True)
    c._rng.setstate(out["streams"][0])
    c._key_gen.set_state(out["streams"][1])
    out["c"], out["c_metrics"] = c, _spy_step(c, batches[3])
    plain = _trainer(_cfg())
    out["plain"], out["plain_metrics"] = plain, _spy_step(plain, batches[0])
    torch.cuda.synchronize()
    return out


def test_trainer_losses_are_finite_and_the_new_entries_run(runs):
    a = runs["a"]
    assert a.iter == 4 and a.deterministic
    for i, m in enumerate(runs["a_metrics"]):
        losses = {k: v for k, v in m.items() if k.startswith("loss")}
        assert len(losses) >= 4 and (i < 2 or any(k.endswith("_unsup") for k in losses)), (i, sorted(m))
        assert all(math.isfinite(v) for v in m.values()), (i, m)
    for i, calls in enumerate(runs["a_calls"]):
        for name in NEW_ENTRIES:
            assert name in calls, (i, name)
        assert "ptmi_roi_mosaic_mask" not in calls, "the GN head has no mask pass"
        # a head pass: pack, two normalised layers, unpack; its backward: pack (of dy), two norm backwards, unpack (of dx)
        fwd, bwd = calls.count("ptmi_roi_mosaic_gn_relu_fwd"), calls.count("ptmi_roi_mosaic_gn_relu_bwd")
        assert fwd % 2 == 0 and bwd % 2 == 0 and bwd >= 2 and fwd >= bwd, (i, fwd, bwd)
        assert calls.count("ptmi_roi_mosaic_pack") == calls.count("ptmi_roi_mosaic_unpack") == (fwd + bwd) // 2, (i, fwd, bwd)
        assert calls[-2:] == ["ptmi_sumsq", "ptmi_clip_sgd_step_seg_wd"]


def test_trainer_teacher_head_parameters_follow_the_ema(runs):
    a = runs["a"]
    k = a.cfg.UNSUPNET.EMA_KEEP_RATE
    s, t = runs["ema"]
    want = s * float(1 - k) + t * float(k)
    names = [n for n in a.student.index if ".box_head.conv" in n]
    assert names == [f"roi_heads.box_head.conv{j}.{q}" for j in (1, 2) for q in ("weight", "norm.weight", "norm.bias")]
    moved = 0
    for n in names:
        off, cnt = a.student.index[n]
        got, w = runs["teacher_after"][off:off + cnt], want[off:off + cnt]
        assert bool(((got - w).abs() <= 1e-6 * w.abs()).all()), n
        moved += int((got != t[off:off + cnt]).sum())
    assert moved > 0, "the student's head parameters have moved away from the teacher's by step 3"


def test_trainer_head_norm_parameters_decay_at_weight_decay_norm(runs):
    """the momentum buffer after the first step IS s g + wd_seg p: WEIGHT_DECAY_NORM (0) for conv{k}.norm.*, WEIGHT_DECAY (1e-4)
    for conv{k}.weight -- at 1e-6 relative, and apart from the other kind's decay"""
    a = runs["a"]
    p0, g, buf0 = (t.cpu().double() for t in runs["a_seen"][0])
    assert not bool(buf0.any())
    s = 10.0 / max(float(g.norm()), 10.0)
    buf1 = runs["a_seen"][1][2].cpu().double()
    names = [m for m, q in a.student.params.items() if q.requires_grad]
    assert a.cfg.SOLVER.WEIGHT_DECAY_NORM == 0.0 and a.cfg.SOLVER.WEIGHT_DECAY == 1e-4
    for n, wd in (("roi_heads.box_head.conv1.norm.weight", 0.0), ("roi_heads.box_head.conv2.norm.bias", 0.0),
                  ("roi_heads.box_head.conv2.weight", 1e-4)):
        off, cnt = a.student.index[n]
        assert a.segment_wd[names.index(n)] == wd, n
        p, gg = p0[off:off + cnt], g[off:off + cnt]
        assert bool(gg.abs().max() > 0), f"{n} got a gradient"
        upd = s * gg + wd * p
        err_b = (buf1[off:off + cnt] - upd).abs()
        assert bool((err_b <= 1e-6 * ((s * gg).abs() + (wd * p).abs())).all()), f"{n} momentum: max err {float(err_b.max()):.3e}"
        if not n.endswith("norm.bias"):                                    # (norm.bias starts at 0: both decays give the same buffer)
            other = s * gg + (1e-4 - wd) * p
            assert not bool(((buf1[off:off + cnt] - other).abs() <= 1e-6 * ((s * gg).abs() + 1e-4 * p.abs())).all()), n


def test_trainer_is_reproducible(runs):
    a, b = runs["a"], runs["b"]
    for ma, mb in zip(runs["a_metrics"], runs["b_metrics"]):
        assert _strip(ma) == _strip(mb)
    assert torch.equal(a.student.flat, b.student.flat) and torch.equal(a.teacher.flat, b.teacher.flat)
    assert torch.equal(a.momentum_buf, b.momentum_buf)


def test_trainer_resume_continues_bit_for_bit(runs):
    a, c = runs["a"], runs["c"]
    assert c.iter == 4 and c.start_iter == 3
    assert _strip(runs["c_metrics"]) == _strip(runs["a_metrics"][3])
    assert torch.equal(a.student.flat, c.student.flat) and torch.equal(a.teacher.flat, c.teacher.flat)
    assert torch.equal(a.momentum_buf, c.momentum_buf)


def test_default_head_calls_none_of_the_new_entries(runs):
    plain = runs["plain"]
    assert [k for k in plain.model.state_dict() if k.startswith("roi_heads.box_head.")] == \
        [f"roi_heads.box_head.fc{k}.{s}" for k in (1, 2) for s in ("weight", "bias")]
    assert not [n for n in plain.calls if n.startswith("ptmi_roi_mosaic_")]
    assert plain.calls[-2:] == ["ptmi_sumsq", "ptmi_clip_sgd_step"]
    assert all(math.isfinite(v) for v in runs["plain_metrics"].values())
