"""numpy restatements of the ROI poolers detectron2's ROIPooler reaches (torchvision roi_align / roi_pool), the reference of
tests/test_roi_pooler_{cpu,gpu}.py.  Geometry and weights are fp32 in the order the definitions are written (SURVEY.md A.9 plus
`aligned` / `sampling_ratio`; ROIPool: roundf corners, floor / ceil bin edges clamped to the map); the backward passes accumulate the
same taps / the argmax scatter in float64.

The second half of the file is the float64 parity apparatus of tests/test_roi_dispatch_{cpu,gpu}.py: see the header there."""
import math
import os
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from tests.losses_ref import MARGIN

f32 = np.float32


def special_boxes(gen, n, fh, fw):
    """The box set of tests/test_ops_gpu.py::test_roi_align: random boxes, then one partly outside, one beyond the far border, a
    tiny one, the whole image and one many times the map.  -> rois (n, 5) torch fp32 with a random image index in {0, 1}."""
    h, w = fh * 16, fw * 16
    cx, cy = torch.rand(n, generator=gen) * w, torch.rand(n, generator=gen) * h
    bw = 4.0 + torch.rand(n, generator=gen) * w * 0.7
    bh = 4.0 + torch.rand(n, generator=gen) * h * 0.7
    boxes = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    boxes[0] = torch.tensor([-30.0, -20.0, 40.0, 35.0])
    boxes[1] = torch.tensor([fw * 16 - 96.0, fh * 16 - 100.0, fw * 16 + 24.0, fh * 16 + 20.0])
    boxes[2] = torch.tensor([10.0, 10.0, 10.5, 10.2])
    boxes[3] = torch.tensor([0.0, 0.0, fw * 16.0, fh * 16.0])
    boxes[4] = torch.tensor([-9000.0, -7000.0, 9500.0, 8000.0])
    return torch.cat([torch.randint(0, 2, (n, 1), generator=gen).float(), boxes], 1)


# ------------------------------------------------------------------------------------------------------------------ ROIAlign
def _align_geom(roi, P, scale, aligned, sampling_ratio):
    s = f32(scale)
    off = f32(0.5) if aligned else f32(0.0)
    sw, sh = f32(roi[1]) * s - off, f32(roi[2]) * s - off
    ew, eh = f32(roi[3]) * s - off, f32(roi[4]) * s - off
    rw, rh = ew - sw, eh - sh
    if not aligned:
        rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
    bh, bw = rh / f32(P), rw / f32(P)
    gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(rh / f32(P)))
    gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(rw / f32(P)))
    return int(roi[0]), sw, sh, bw, bh, gw, gh, max(gh * gw, 1)


def _axis_taps(start, bsz, pb, gn, L):
    """The valid samples of bin row / column `pb` along one axis, in sample order: (low cell, high cell, low weight l, high
    weight h) -- the validity test [-1, L], the clamp and the tap split of A.9 are the same along y and x."""
    if gn <= 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, f32), np.zeros(0, f32)
    i = np.arange(gn, dtype=f32)
    v = (start + f32(pb) * bsz) + ((i + f32(.5)) * bsz) / f32(gn)
    v = v[~((v < f32(-1.0)) | (v > f32(L)))]
    v = np.where(v <= 0, f32(0), v).astype(f32)
    lo = v.astype(np.int64)
    edge = lo >= L - 1
    lo = np.where(edge, L - 1, lo)
    hi = np.where(edge, L - 1, lo + 1)
    v = np.where(edge, lo.astype(f32), v).astype(f32)
    l = (v - lo.astype(f32)).astype(f32)
    return lo, hi, l, (f32(1) - l).astype(f32)


def roi_align(feat, rois, P, scale, aligned=True, sampling_ratio=0):
    """feat (N, C, H, W), rois (R, 5) numpy fp32 -> (R, C, P, P) fp32.  A bin's samples are visited iy outer, ix inner and added
    one by one in fp32 (np.cumsum is a sequential sum), each as w1 f(yl, xl) + w2 f(yl, xh) + w3 f(yh, xl) + w4 f(yh, xh)."""
    feat, rois = np.asarray(feat, f32), np.asarray(rois, f32)
    N, C, H, W = feat.shape
    out = np.zeros((len(rois), C, P, P), f32)
    for r, roi in enumerate(rois):
        b, sw, sh, bw, bh, gw, gh, count = _align_geom(roi, P, scale, aligned, sampling_ratio)
        xt = [_axis_taps(sw, bw, pw, gw, W) for pw in range(P)]
        for ph in range(P):
            yl, yh, ly, hy = _axis_taps(sh, bh, ph, gh, H)
            for pw in range(P):
                xl, xh, lx, hx = xt[pw]
                if len(yl) == 0 or len(xl) == 0:
                    continue
                f = feat[b]
                w1, w2 = hy[:, None] * hx[None, :], hy[:, None] * lx[None, :]
                w3, w4 = ly[:, None] * hx[None, :], ly[:, None] * lx[None, :]
                term = (w1 * f[:, yl[:, None], xl[None, :]] + w2 * f[:, yl[:, None], xh[None, :]]
                        + w3 * f[:, yh[:, None], xl[None, :]] + w4 * f[:, yh[:, None], xh[None, :]])
                acc = np.cumsum(term.reshape(C, -1), axis=1, dtype=f32)[:, -1]
                out[r, :, ph, pw] = acc / f32(count)
    return out


def roi_align_backward(dout, rois, shape, P, scale, aligned=True, sampling_ratio=0):
    """float64 accumulation of g w_k / count on the same taps -> (N, C, H, W) float64"""
    dout, rois = np.asarray(dout, np.float64), np.asarray(rois, f32)
    N, C, H, W = shape
    df = np.zeros(shape, np.float64)
    for r, roi in enumerate(rois):
        b, sw, sh, bw, bh, gw, gh, count = _align_geom(roi, P, scale, aligned, sampling_ratio)
        xt = [_axis_taps(sw, bw, pw, gw, W) for pw in range(P)]
        for ph in range(P):
            yl, yh, ly, hy = _axis_taps(sh, bh, ph, gh, H)
            for pw in range(P):
                xl, xh, lx, hx = xt[pw]
                if len(yl) == 0 or len(xl) == 0:
                    continue
                g = dout[r, :, ph, pw][:, None, None] / count
                for ya, wy in ((yl, hy), (yh, ly)):
                    for xa, wx in ((xl, hx), (xh, lx)):
                        w = (wy[:, None] * wx[None, :]).astype(np.float64)       # the fp32 tap weight
                        yy, xx = np.broadcast_arrays(ya[:, None], xa[None, :])
                        np.add.at(df[b], (slice(None), yy, xx), g * w[None])
    return df


# ------------------------------------------------------------------------------------------------------------------- ROIPool
def _roundf(v):
    """C roundf of an fp32 value: half away from zero (|v| + 0.5 is exact in float64)"""
    v = float(f32(v))
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def roi_pool_bins(roi, P, scale, H, W):
    """-> per bin row (hstart, hend) and per bin column (wstart, wend), clamped to the map"""
    s = f32(scale)
    rsw, rsh = _roundf(f32(roi[1]) * s), _roundf(f32(roi[2]) * s)
    rew, reh = _roundf(f32(roi[3]) * s), _roundf(f32(roi[4]) * s)
    rw, rh = max(rew - rsw + 1, 1), max(reh - rsh + 1, 1)
    bh, bw = f32(rh) / f32(P), f32(rw) / f32(P)
    clamp = lambda v, L: min(max(v, 0), L)
    hb = [(clamp(int(math.floor(f32(ph) * bh)) + rsh, H), clamp(int(math.ceil(f32(ph + 1) * bh)) + rsh, H)) for ph in range(P)]
    wb = [(clamp(int(math.floor(f32(pw) * bw)) + rsw, W), clamp(int(math.ceil(f32(pw + 1) * bw)) + rsw, W)) for pw in range(P)]
    return hb, wb


def roi_pool(feat, rois, P, scale):
    """-> (values (R, C, P, P) fp32, argmax (R, C, P, P) int32).  np.argmax returns the FIRST maximum of the bin's cells flattened
    h outer, w inner: the raster scan with a strict `>` from -FLT_MAX.  An empty bin: value 0, argmax -1."""
    feat, rois = np.asarray(feat, f32), np.asarray(rois, f32)
    N, C, H, W = feat.shape
    out = np.zeros((len(rois), C, P, P), f32)
    arg = np.full((len(rois), C, P, P), -1, np.int32)
    for r, roi in enumerate(rois):
        b = int(roi[0])
        hb, wb = roi_pool_bins(roi, P, scale, H, W)
        for ph, (hs, he) in enumerate(hb):
            for pw, (ws, we) in enumerate(wb):
                if he <= hs or we <= ws:
                    continue
                cells = feat[b, :, hs:he, ws:we].reshape(C, -1)
                k = np.argmax(cells, axis=1)
                out[r, :, ph, pw] = cells[np.arange(C), k]
                arg[r, :, ph, pw] = (hs + k // (we - ws)) * W + ws + k % (we - ws)
    return out, arg


def roi_pool_backward(dout, arg, rois, shape):
    """float64 scatter of dout through the argmax -> (N, C, H, W) float64"""
    dout = np.asarray(dout, np.float64)
    N, C, H, W = shape
    df = np.zeros((N, C, H * W), np.float64)
    for r, roi in enumerate(np.asarray(rois, f32)):
        b = int(roi[0])
        a = arg[r].reshape(C, -1)
        g = dout[r].reshape(C, -1)
        cc = np.broadcast_to(np.arange(C)[:, None], a.shape)
        ok = a >= 0
        np.add.at(df[b], (cc[ok], a[ok]), g[ok])
    return df.reshape(shape)


# ============================================================================ ROIAlign: float64 parity with an fp32 yardstick
# (tests/test_roi_dispatch_cpu.py, tests/test_roi_dispatch_gpu.py; the convention of tests/gemm_ref.py)
#
# Reference.  `roi_align64` / `roi_align_backward64`: geometry, index decisions and the 1-D tap weights l, h = 1 - l are the fp32
# values of _align_geom / _axis_taps (another precision there picks other cells than the kernels); from there on float64: a tap's
# weight is the exact product of its two 1-D weights, the sums run in float64, evaluated separably -- per ROI the (P, H) and (P, W)
# matrices of summed 1-D weights, value = Wy F Wx^T / count -- which is the same sum in another order at 2^-53.
# (`roi_align_backward` above rounds each tap weight to fp32 first: it differs from `roi_align_backward64` by at most one rounding
# per term, which tests/test_roi_dispatch_cpu.py asserts.)
#
# Yardsticks.  Forward: `roi_align` above (torchvision's order, every operation fp32).  Backward: `roi_align_backward32`, the
# atomic kernel's expression (g * w) / count added one tap at a time in ROI, bin, sample, tap order in float32.
#
# Error measure, scale-aware: err(x) = max |x - ref64| / S with the magnitude S = sum w |f| / count per output (forward) and
# S = sum |g| w / count per cell (backward): what every fp32 rounding of these sums is proportional to (all weights are >= 0).
# Where S == 0 the element must match exactly; a NaN is an infinite error.
#
# Hard bounds, per element, in units of u = 2^-24 times S, times 1.01 for the second-order terms (the largest count below is
# 2.2e5: (1 + u)^n - 1 <= 1.007 n u).  Counted as the number of roundings the contribution of one term (one tap) can pass through;
# gh x gw is the ROI's sampling grid, T = 4 gh gw its taps per bin.
#   forward, gather kernels (roi_align_fwd_body; the table-less branch of roi_align_fwd_bin_kernel): hy * hx, w * f, at most T
#       additions, the division by count (table-less branch: w / count, then one FMA per tap) -> at most T + 3;
#   forward, table kernels: a table entry is the sum of at most 2 gh (2 gw) 1-D weights: 2 gh + 2 gw roundings; 1 / count and its
#       product with the x entry: 2; wy[a] * wx[b]: 1; one FMA per cell over at most (gh + 1)(gw + 1) cells.  With gh, gw >= 1
#       both 2 gh + 2 gw and (gh + 1)(gw + 1) are <= 4 gh gw = T -> at most 2 T + 3.
#       Both are within `fwd_terms` = 2 T + 8 (this count leaves 5 to spare).
#   backward, atomic kernel (roi_align_bwd_body) and the yardstick: hy * hx, g * w, / count, then the K additions that meet in the
#       cell (K = taps landing on it, from all ROIs) -> at most K + 3: `bwd_terms_atomic`;
#   backward, band kernel: per ROI touching the cell the x table entry (2 gw sums, 1 / count, its product: 2 gw + 2), t[ph] = one
#       product and six FMAs over pw (7), the y table entry (2 gh), seven FMAs over ph into the cell (7): 2 (gh + gw) + 16; the
#       cell's running value then passes through the 7 FMAs of every later ROI touching it.  With n ROIs on the cell and
#       g = the largest 2 (gh + gw) among them -> at most g + 16 + 7 (n - 1): `bwd_terms_band`.
# Tight bound: err(got) <= MARGIN * err(yardstick), MARGIN = tests/losses_ref.MARGIN (4), the yardstick's err over the same case.
U24 = 2.0 ** -24


def _axis_matrix(start, bsz, gn, L, P):
    """-> (P, L) float64 sums of the fp32 1-D weights that bin row / column pb puts on each cell, (P, L) int64 taps per cell"""
    wm, cnt = np.zeros((P, L)), np.zeros((P, L), np.int64)
    for pb in range(P):
        lo, hi, l, h = _axis_taps(start, bsz, pb, gn, L)
        np.add.at(wm[pb], lo, h.astype(np.float64))
        np.add.at(wm[pb], hi, l.astype(np.float64))
        np.add.at(cnt[pb], lo, 1)
        np.add.at(cnt[pb], hi, 1)
    return wm, cnt


def roi_align64(feat, rois, P, scale, aligned=True, sampling_ratio=0):
    """-> value (R, C, P, P) float64, magnitude S = sum w |f| / count (R, C, P, P) float64, T = 4 gh gw (R, 1, P, P) int64"""
    f64 = np.asarray(feat, f32).astype(np.float64)
    fabs, rois = np.abs(f64), np.asarray(rois, f32)
    N, C, H, W = f64.shape
    val, S, T = np.zeros((len(rois), C, P, P)), np.zeros((len(rois), C, P, P)), np.zeros((len(rois), 1, P, P), np.int64)
    for r, roi in enumerate(rois):
        b, sw, sh, bw, bh, gw, gh, count = _align_geom(roi, P, scale, aligned, sampling_ratio)
        wy, _ = _axis_matrix(sh, bh, gh, H, P)
        wx, _ = _axis_matrix(sw, bw, gw, W, P)
        val[r] = np.matmul(np.matmul(wy, f64[b]), wx.T) / count
        S[r] = np.matmul(np.matmul(wy, fabs[b]), wx.T) / count
        T[r] = 4 * max(gh, 0) * max(gw, 0)
    return val, S, T


def fwd_terms(T):
    return 2 * T + 8


def roi_align_backward64(dout, rois, shape, P, scale, aligned=True, sampling_ratio=0):
    """-> namespace of (N, C, H, W) float64 `value` and magnitude `S` = sum |g| w / count, and per cell (N, 1, H, W) int64:
    `K` taps landing on it, `nroi` ROIs with a tap on it, `gmax` the largest 2 (gh + gw) among those"""
    d64, rois = np.asarray(dout, f32).astype(np.float64), np.asarray(rois, f32)
    N, C, H, W = shape
    o = SimpleNamespace(value=np.zeros(shape), S=np.zeros(shape), K=np.zeros((N, 1, H, W), np.int64),
                        nroi=np.zeros((N, 1, H, W), np.int64), gmax=np.zeros((N, 1, H, W), np.int64))
    for r, roi in enumerate(rois):
        b, sw, sh, bw, bh, gw, gh, count = _align_geom(roi, P, scale, aligned, sampling_ratio)
        wy, ny = _axis_matrix(sh, bh, gh, H, P)
        wx, nx = _axis_matrix(sw, bw, gw, W, P)
        g = d64[r] / count
        o.value[b] += np.matmul(np.matmul(wy.T, g), wx)
        o.S[b] += np.matmul(np.matmul(wy.T, np.abs(g)), wx)
        ty, tx = ny.sum(0), nx.sum(0)
        o.K[b, 0] += ty[:, None] * tx[None, :]
        on = (ty[:, None] > 0) & (tx[None, :] > 0)
        o.nroi[b, 0] += on
        o.gmax[b, 0] = np.maximum(o.gmax[b, 0], on * (2 * (gh + gw)))
    return o


def bwd_terms_atomic(b64):
    return b64.K + 3


def bwd_terms_band(b64):
    return b64.gmax + 16 + 7 * np.maximum(b64.nroi - 1, 0)


def roi_align_backward32(dout, rois, shape, P, scale, aligned=True, sampling_ratio=0):
    """the fp32 yardstick of the backward: cell += (g * w) / count, w = the fp32 product of the tap's 1-D weights, one tap at a time
    in ROI, bin (ph, pw), sample (iy, ix), tap ((yl, xl), (yl, xh), (yh, xl), (yh, xh)) order -> (N, C, H, W) float32"""
    dout, rois = np.asarray(dout, f32), np.asarray(rois, f32)
    N, C, H, W = shape
    df = np.zeros((N, C, H * W), f32)
    for r, roi in enumerate(rois):
        b, sw, sh, bw, bh, gw, gh, count = _align_geom(roi, P, scale, aligned, sampling_ratio)
        xt = [_axis_taps(sw, bw, pw, gw, W) for pw in range(P)]
        idx, vals = [], []
        for ph in range(P):
            yl, yh, ly, hy = _axis_taps(sh, bh, ph, gh, H)
            for pw in range(P):
                xl, xh, lx, hx = xt[pw]
                if len(yl) == 0 or len(xl) == 0:
                    continue
                w = np.stack([hy[:, None] * hx[None, :], hy[:, None] * lx[None, :], ly[:, None] * hx[None, :],
                              ly[:, None] * lx[None, :]], -1).astype(f32)
                cell = np.stack([yl[:, None] * W + xl[None, :], yl[:, None] * W + xh[None, :], yh[:, None] * W + xl[None, :],
                                 yh[:, None] * W + xh[None, :]], -1)
                idx.append(cell.reshape(-1))
                vals.append((dout[r, :, ph, pw][:, None] * w.reshape(1, -1)) / f32(count))
        if idx:
            idx, vals = np.concatenate(idx), np.concatenate(vals, 1)
            assert vals.dtype == f32
            for c in range(C):
                np.add.at(df[b, c], idx, vals[c])
    return df.reshape(shape)


def scaled_err(x, ref64, S):
    """elementwise |x - ref64| / S; 0 where x == ref64, inf where they differ at S == 0 or x is NaN"""
    x = np.asarray(x, np.float64)
    assert x.shape == ref64.shape == S.shape, f"shape {x.shape} vs {ref64.shape} vs {S.shape}"
    d = np.abs(x - ref64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(d == 0, 0.0, d / S)
    return np.where(np.isnan(e), np.inf, e)


def err(x, ref64, S):
    return float(scaled_err(x, ref64, S).max()) if ref64.size else 0.0


def check(got, ref64, S, bound_terms, err_seq32, margin=MARGIN, what=""):
    """both bounds of the header.  `bound_terms`: roundings per element (broadcast against the output); `err_seq32`: err() of the
    yardstick on the same case -> (err(got) / err(seq32), largest share of the hard bound)"""
    if not ref64.size:
        return 0.0, 0.0
    e = scaled_err(got, ref64, S)
    hard = np.broadcast_to(np.asarray(bound_terms, np.float64) * U24 * 1.01, e.shape)
    eg, frac = float(e.max()), float((e / hard).max())
    ratio = eg / err_seq32 if err_seq32 > 0 else (float("inf") if eg > 0 else 0.0)
    if os.environ.get("PTMI_TEST_VERBOSE"):
        print(f"[check] {what}: err(got) {eg / U24:.2f} err(seq32) {err_seq32 / U24:.2f} (units of 2^-24) ratio {ratio:.3f} "
              f"of hard bound {frac:.4f}")
    if frac > 1:
        at = np.unravel_index(int(np.argmax(e / hard)), e.shape)
        raise AssertionError(f"{what}: at {at} err {e[at]:.3e} = {e[at] / U24:.1f} x 2^-24 of S = {S[at]:.3e} is outside the hard "
                             f"bound of {hard[at] / U24 / 1.01:.0f} roundings (got {np.asarray(got)[at]!r}, reference {ref64[at]!r})")
    assert eg <= margin * err_seq32, f"{what}: err {eg:.3e} > {margin:g} * err(seq32) {err_seq32:.3e} (ratio {ratio:.2f})"
    return ratio, frac


# ---------------------------------------------------------------------------------------------- which path a ROI takes
def tab_stride(H, W):
    """floats per row of the forward kernel's per-bin weight table (roi_tab_stride)"""
    return ((max(H, W) + 1 + 6) // 7 + 1 + 1 + 3) & ~3


BANDS = 8                                    # row bands = waves of the band backward kernel


def classify(roi, H, W, P, scale, aligned=True, sampling_ratio=0):
    """where the grouped kernels send one ROI (P = 7) -> (path, windows, bands):
    path     "novalid" (no sample inside [-1, H] x [-1, W]: the backward header holds x1 = y1 = -1, every output is 0), "notable"
             (the forward header's sy < 0: a bin spans more cells than the table holds, or a fixed grid's samples descend: the
             sample-by-sample branch), "unrolled" (sy <= 4 and sx <= 4) or "generic";
    windows  16-column windows the band kernel slides over the ROI's columns [x0, x1] (0 for "novalid");
    bands    the row bands of ceil(H / 8) rows that its rows [y0, y1] touch."""
    assert P == 7
    b, sw, sh, bw, bh, gw, gh, count = _align_geom(roi, P, scale, aligned, sampling_ratio)
    ts, variant = tab_stride(H, W), not (aligned and sampling_ratio == 0)
    span, lohi = [], []
    for start, bsz, gn, L in ((sh, bh, gh, H), (sw, bw, gw, W)):
        worst, fits, lo_all, hi_all = 0, True, None, None
        for pb in range(P):
            lo, hi, _, _ = _axis_taps(start, bsz, pb, gn, L)
            n = 0
            for l, h2 in zip(lo.tolist(), hi.tolist()):
                ascends = not variant or l >= lo[0]
                n = h2 - int(lo[0]) + 1 if ascends and h2 - int(lo[0]) < ts else -(1 << 20)
            fits, worst = fits and n >= 0, max(worst, n)
            if len(lo):
                lo_all = int(lo.min()) if lo_all is None else min(lo_all, int(lo.min()))
                hi_all = int(hi.max()) if hi_all is None else max(hi_all, int(hi.max()))
        span.append(worst if fits else -1)
        lohi.append((lo_all, hi_all))
    (y0, y1), (x0, x1) = lohi
    if y0 is None or x0 is None:
        return "novalid", 0, frozenset()
    br = -(-H // BANDS)
    bands = frozenset(w for w in range(BANDS) if max(y0, w * br) <= min(y1, min(H, (w + 1) * br) - 1))
    path = "notable" if min(span) < 0 else "unrolled" if span[0] <= 4 and span[1] <= 4 else "generic"
    return path, -(-(x1 - x0 + 1) // 16), bands


def admitted_classes(H, W, sampling_ratio=0):
    """the classify classes a map of H x W cells can show at all.  A fixed grid of one sample a bin touches two cells a side: its
    table always fits and is never generic"""
    need = {"novalid", "unrolled", "windows1"}
    if sampling_ratio != 1:
        need.add("notable")
        if tab_stride(H, W) > 4:
            need.add("generic")
    if W >= 17:
        need.add("windows2")
    if W >= 33:
        need.add("windows3+")
    if H >= 2:
        need.add("skips a band")
    return need


def classes_present(rois, H, W, P, scale, aligned=True, sampling_ratio=0):
    have = set()
    owning = sum(1 for w in range(BANDS) if w * -(-H // BANDS) < H)
    for roi in np.asarray(rois, f32):
        path, windows, bands = classify(roi, H, W, P, scale, aligned, sampling_ratio)
        have.add(path)
        if path != "novalid":
            have.add("windows1" if windows == 1 else "windows2" if windows == 2 else "windows3+")
            if len(bands) < owning:
                have.add("skips a band")
    return have


# ---------------------------------------------------------------------------------------------- boxes, images, operands
def edge_boxes(fh, fw, scale):
    """(24, 4) fp32 boxes in image coordinates for a map of fh x fw cells at `scale`: the five specials of `special_boxes`, then the
    geometries that set lacks.  Written in cells (u = coordinate * scale; an aligned ROI starts sampling at u - 0.5):"""
    H, W = float(fh), float(fw)
    # a fixed grid of 2 puts a bin's two samples half a bin apart: with bins of 2 (TS + 2) cells the middle bin's samples are both
    # inside the map and further apart than the forward table holds -> no table, without a descending grid
    half = 3.5 * 2 * (tab_stride(fh, fw) + 2)
    wide = (W / 2 - half, 1, W / 2 + half, H - 1) if fw >= fh else (1, H / 2 - half, W - 1, H / 2 + half)
    cells = [
        (-30 / 16, -20 / 16, 40 / 16, 35 / 16),                  # 0 partly outside
        (W - 6, H - 6.25, W + 1.5, H + 1.25),                    # 1 beyond the far border
        (10 / 16, 10 / 16, 10.5 / 16, 10.2 / 16),                # 2 tiny
        (0, 0, W, H),                                            # 3 the whole image
        (-9000 / 16, -7000 / 16, 9500 / 16, 8000 / 16),          # 4 many times the map: no table
        (3, 2, 3, 6),                                            # 5 zero width
        (2, 3, 7, 3),                                            # 6 zero height
        (8, 2, 3, 6),                                            # 7 inverted in x  (a fixed grid's samples descend: no table)
        (2, 7, 6, 3),                                            # 8 inverted in y
        (8, 7, 2, 1),                                            # 9 inverted in both
        (W + 3, H + 2, W + 9, H + 8),                            # 10 no valid sample: beyond both far borders
        (-30, 1, -20, 4),                                        # 11 no valid sample in x alone
        (-1, -1, 6, 6),                                          # 12 aligned: exactly 7 cells, one sample a bin, the first ON -1.0
        (W - 6, H - 6, W + 1, H + 1),                            # 13 aligned: the last sample ON W and ON H (inclusive: valid)
        (1, 1, 15, 15),                                          # 14 exactly 14 cells: ceil(14 / 7) = 2 without a remainder
        (2, 3, 23, 10),                                          # 15 exactly 21 x 7 cells; 22 columns: two windows
        (W - 1.5, 1, W + 0.4, H - 0.5),                          # 16 on the last column: the l >= L - 1 clamp
        (1, 2, 27, 9),                                           # 17 26 cells wide: two 16-column windows
        (0.5, 1.5, 41, 6),                                       # 18 40.5 cells wide: three windows
        (2, 0.5, 9, 33),                                         # 19 32.5 cells high: bins of 5 sample rows (generic table)
        (4, 1, 6, 2.5),                                          # 20 a few cells inside one row band
        (-1.5, -1.5, 5.5, 5.5),                                  # 21 not aligned: exactly 7 cells, the first sample ON -1.0
        (W - 6.5, H - 6.5, W + 0.5, H + 0.5),                    # 22 not aligned: the last sample ON W and ON H
        wide,                                                    # 23 bins two tables wide along the longer axis (see above)
    ]
    return (np.asarray(cells, np.float64) / float(scale)).astype(f32)


def box_set(n, fh, fw, scale, seed):
    """`n` boxes: the edge boxes first, then seeded random ones with the size distribution of `special_boxes`"""
    e = edge_boxes(fh, fw, scale)
    gen = np.random.default_rng([seed, n, fh, fw])
    cx, cy = gen.random(max(n, 1)) * fw, gen.random(max(n, 1)) * fh
    bw, bh = 0.25 + gen.random(max(n, 1)) * fw * 0.7, 0.25 + gen.random(max(n, 1)) * fh * 0.7
    rnd = (np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1) / float(scale)).astype(f32)
    return np.concatenate([e, rnd])[:n]


def counts_to_rois(boxes, counts):
    """box i goes to the image that the per-image count list gives row i -> rois (R, 5) fp32 sorted by image, img_offsets (N + 1) int32"""
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    assert len(boxes) == offs[-1]
    img = np.repeat(np.arange(len(counts)), counts).astype(f32)
    return np.concatenate([img[:, None], np.asarray(boxes, f32)], 1), offs


def scaled_randn(gen, shape, plane_of_row=None, planes=None):
    """seeded randn (n, c, ...) with every (image, channel) plane multiplied by a power of two from 2^-10 .. 2^10.  For ROI rows:
    `plane_of_row` (the image of each row) and `planes` = number of images"""
    x = gen.standard_normal(shape, dtype=f32)
    n = shape[0] if plane_of_row is None else planes
    pw = np.exp2(gen.integers(-10, 11, size=(n, shape[1]))).astype(f32)
    pw = pw if plane_of_row is None else pw[np.asarray(plane_of_row, np.int64)]
    return x * pw.reshape(pw.shape + (1,) * (len(shape) - 2))


# ---------------------------------------------------------------------------------------------- the dispatch classes and the cases
# (C, H, W, forward planes per workgroup [0: the gather kernel], backward planes [0: the atomic kernel], backward LDS class in KB)
MAPS = [
    (9, 48, 100, 8, 3, 80),          # forward: 8 planes in exactly 150 KB, ragged 8 + 1; backward 3 + 3 + 3
    (5, 25, 31, 4, 4, 80),           # 4 planes, ragged 4 + 1, both ways
    (3, 25, 31, 3, 3, 80),           # 3 planes in the 4-plane kernel: the unused plane aliases plane 0
    (1, 5, 9, 1, 1, 80),             # bands of one row, three waves own none, the map narrower than a window
    (9, 50, 100, 3, 3, 80),          # 8 planes no longer fit 150 KB: 3 in 72 KB
    (5, 100, 120, 1, 1, 80),         # 1 plane each way
    (5, 128, 144, 1, 2, 160),        # forward: exactly 72 KB; backward: 2 planes in the 160 KB class (162,432 B)
    (5, 140, 140, 0, 1, 160),        # forward: gather fallback; backward 1 plane in 160 KB
    (5, 193, 193, 0, 0, 0),          # neither fits: gather forward, atomic backward
    (9, 256, 9, 8, 4, 80),           # bands of exactly 32 rows: served
    (9, 257, 9, 8, 0, 0),            # 33 rows a band: atomic fallback
]
COUNTS_LONG = [(0, 1, 2, 3, 0, 21, 0), (41,), (20, 19)]
COUNTS_SHORT = [(0, 3, 21)]
VARIANTS = [(0, 0), (0, 2), (1, 2), (1, 1)]


def fwd_planes(c, h, w, pooled):
    """the host rule of roi_fwd_planes, restated (for tests/test_roi_dispatch_cpu.py: it keeps MAPS honest; not a parity reference)"""
    plane = h * w * 4
    if pooled != 7 or plane > 72 * 1024:
        return 0
    if c >= 8 and 8 * plane <= 150 * 1024:
        return 8
    return min(72 * 1024 // plane, 4, c)


def bwd_plan(c, h, w, pooled):
    """the host rule of roi_bwd_grouped, restated -> (planes per workgroup [0: atomic kernel], LDS class in KB, bytes of LDS asked for)"""
    br, pitch = -(-h // BANDS), ((h * w + 47) // 64) * 64 + 16
    strips = BANDS * (64 * 4 + 4 * 52) * 4
    cls, cg = 80, (80 * 1024 - strips) // (pitch * 4)
    if cg < 1:
        cls, cg = 160, (160 * 1024 - strips) // (pitch * 4)
    cg = min(cg, 4, c)
    if pooled != 7 or br > 32 or cg < 1:
        return 0, 0, 0
    return cg, cls, cg * pitch * 4 + strips


@dataclass(frozen=True)
class Case:
    group: str
    C: int
    H: int
    W: int
    counts: tuple
    P: int = 7
    scale: float = 1 / 16
    aligned: int = 1
    ratio: int = 0

    @property
    def name(self):
        return (f"{self.C}x{self.H}x{self.W} counts {','.join(map(str, self.counts))} P{self.P} scale {self.scale:g} "
                f"aligned {self.aligned} ratio {self.ratio}")

    @property
    def fwd_served(self):
        return fwd_planes(self.C, self.H, self.W, self.P) > 0

    @property
    def bwd_served(self):
        return bwd_plan(self.C, self.H, self.W, self.P)[0] > 0


def all_cases():
    out = []
    for i, m in enumerate(MAPS):
        out += [Case("(1) map classes x ROI counts", *m[:3], counts) for counts in (COUNTS_LONG if i in (0, 1, 3) else COUNTS_SHORT)]
    for i in (0, 6):
        out += [Case("(2) variants", *MAPS[i][:3], COUNTS_SHORT[0], aligned=a, ratio=s) for a, s in VARIANTS]
    out += [Case("(3) scale", *MAPS[1][:3], COUNTS_SHORT[0], scale=s) for s in (1 / 8, 1.0)]
    out += [Case("(4) pooled size", *MAPS[1][:3], COUNTS_SHORT[0], P=p) for p in (1, 2, 5, 14)]
    return out


@lru_cache(maxsize=None)
def build(case):
    """operands, float64 references, yardsticks and their errors of one case (computed once per process, never modified)"""
    n, R = len(case.counts), sum(case.counts)
    shape = (n, case.C, case.H, case.W)
    rois, offs = counts_to_rois(box_set(R, case.H, case.W, case.scale, 7), case.counts)
    gen = np.random.default_rng([29, n, case.C, case.H, case.W, R, case.P])
    feat = scaled_randn(gen, shape)
    dout = scaled_randn(gen, (R, case.C, case.P, case.P), rois[:, 0], n)
    var = (case.P, case.scale, bool(case.aligned), case.ratio)
    f64, fS, fT = roi_align64(feat, rois, *var)
    f32y = roi_align(feat, rois, *var)
    b64 = roi_align_backward64(dout, rois, shape, *var)
    b32y = roi_align_backward32(dout, rois, shape, *var)
    o = SimpleNamespace(case=case, shape=shape, rois=rois, offs=offs, feat=feat, dout=dout, f64=f64, fS=fS, fT=fT, f32y=f32y, b64=b64,
                        b32y=b32y, fe32=err(f32y, f64, fS), be32=err(b32y, b64.value, b64.S))
    for a in (rois, offs, feat, dout, f64, fS, fT, f32y, b64.value, b64.S, b64.K, b64.nroi, b64.gmax, b32y):
        a.setflags(write=False)
    return o
