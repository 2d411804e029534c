"""numpy restatements of the ROI poolers detectron2's ROIPooler reaches (torchvision roi_align / roi_pool), the reference of
tests/test_roi_pooler_{cpu,gpu}.py.  Geometry and weights are fp32 in the order the definitions are written (SURVEY.md A.9 plus
`aligned` / `sampling_ratio`; ROIPool: roundf corners, floor / ceil bin edges clamped to the map); the backward passes accumulate the
same taps / the argmax scatter in float64."""
import math

import numpy as np
import torch

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
