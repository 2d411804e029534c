#!/usr/bin/env python
"""HIP-event time of the box head, forward + backward, at the train step's own ROI count:

    python tools/box_head_timing.py [--rois 8192] [--channels 512] [--baseline-rois 2048] [--repeat 5] [--out profiles/box_head_timing.txt]

Heads (FastRCNNConvFCHead on `--rois` pooled 7 x 7 ROIs of `--channels` channels; dx is computed too, as the ROI pooler's backward
needs it):

    2fc             NUM_FC 2, FC_DIM 1024: the shipped head
    4conv1fc        NUM_CONV 4, CONV_DIM 256, NUM_FC 1, FC_DIM 1024 on the ROI mosaic, conv + bias + ReLU + mask
    4conv1fc GN     the same with NORM "GN": conv, then the mosaic GroupNorm + ReLU

and, for what the mosaic is justified against, the four conv layers alone:

    convs mosaic    pack -> [ops.conv3x3 + mask] x 4 -> unpack at `--rois`
    convs per ROI   the same layers through ops.conv3x3 on the (R, C, 7, 7) tensor itself -- every ROI a 7 x 7 "image" -- at
                    `--baseline-rois`; compared per ROI

Then the mosaic's own kernels at (`--rois`, CONV_DIM 256): bytes are counted from the shapes -- pack / unpack move the ROI tensor and
the canvases once each, mask 2 canvas maps, GroupNorm forward 2 (z in, y out), backward 7 (dy, y, z twice: dgamma / dbeta and dz;
dz out) -- and "of HBM" is bytes / time over 6.29 TB/s, the rate a float4 copy reaches on an MI355X.  One untimed call, then
`--repeat` timed ones between HIP events on the kernels' stream; the MEDIAN is reported.  No threshold is set on any number."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
P = 7


def time_ms(fn, repeat):
    fn()
    out = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rois", type=int, default=8192)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--baseline-rois", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_head_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "box_head_timing needs the GPU: there is no CPU path to time"
    from probabilisticteacher_amd import _lib, ops
    from probabilisticteacher_amd.config import setup_cfg
    from probabilisticteacher_amd.modeling.backbone import ShapeSpec
    from probabilisticteacher_amd.modeling.roi_heads import build_box_head
    dev = torch.device("cuda", 0)
    R, C, RB = args.rois, args.channels, args.baseline_rois
    gen = torch.Generator(device=dev).manual_seed(1)

    def head(*opts):
        cfg = setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), ["MODEL.DEVICE", "cuda:0", "MODEL.VGG.PRETRAIN", ""] + list(opts))
        torch.manual_seed(2)
        return build_box_head(cfg, ShapeSpec(channels=C, height=P, width=P)).to(dev)

    conv4 = ["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.CONV_DIM", 256, "MODEL.ROI_BOX_HEAD.NUM_FC", 1]
    heads = [("2fc", head()), ("4conv1fc", head(*conv4)), ("4conv1fc GN", head(*conv4, "MODEL.ROI_BOX_HEAD.NORM", "GN"))]
    x = torch.relu(torch.randn(R, C, P, P, device=dev, generator=gen)).requires_grad_()
    up = torch.randn(R, 1024, device=dev, generator=gen)

    def step(fn, xin, upstream, params):
        def run():
            xin.grad = None
            for q in params:
                q.grad = None
            fn(xin).backward(upstream)
        return run

    lines = [f"# tools/box_head_timing.py --rois {R} --channels {C} --baseline-rois {RB} --repeat {args.repeat}",
             f"# {torch.cuda.get_device_name(0)}; median of {args.repeat} HIP-event timings, forward + backward (dx, dW, db); "
             f"HBM rate {HBM_BYTES_PER_S / 1e12:.2f} TB/s",
             f"{'head':16} {'ROIs':>6} {'ms':>9} {'us / ROI':>9}"]
    for name, h in heads:
        t = time_ms(step(h, x, up, list(h.parameters())), args.repeat)
        lines.append(f"{name:16} {R:6d} {t:9.3f} {1e3 * t / R:9.3f}")
    # the conv layers alone: on the mosaic, and as R separate 7 x 7 maps
    h4 = heads[1][1]
    convs = [getattr(h4, f"conv{k}") for k in range(1, 5)]
    params = [q for c in convs for q in (c.weight, c.bias)]
    upc = torch.randn(R, 256, P, P, device=dev, generator=gen)
    t_mosaic = time_ms(step(h4._convs, x, upc, params), args.repeat)

    def per_roi(t):
        for c in convs:
            t = ops.conv3x3(t, c.weight, c.bias, True)
        return t
    xb = x.detach()[:RB].clone().requires_grad_()
    t_base = time_ms(step(per_roi, xb, upc[:RB].clone(), params), args.repeat)
    lines += ["", f"{'conv layers':16} {'ROIs':>6} {'ms':>9} {'us / ROI':>9}",
              f"{'convs mosaic':16} {R:6d} {t_mosaic:9.3f} {1e3 * t_mosaic / R:9.3f}",
              f"{'convs per ROI':16} {RB:6d} {t_base:9.3f} {1e3 * t_base / RB:9.3f}",
              f"per-ROI time, 7 x 7 maps over mosaic: {(t_base / RB) / (t_mosaic / R):.2f}x"]
    del xb, upc, heads, h4, x, up
    # the mosaic's own kernels at CONV_DIM 256
    c, groups, eps = 256, 32, 1e-5
    p, s = ops._ptr, ops._stream()
    _, _, side, ncv = ops.roi_mosaic_geometry(R, P)
    rois = torch.randn(R, c, P, P, device=dev, generator=gen)
    back = torch.empty_like(rois)
    z = torch.randn(ncv, c, side, side, device=dev, generator=gen)
    dy = torch.randn(ncv, c, side, side, device=dev, generator=gen)
    y, dz = torch.empty_like(z), torch.empty_like(z)
    gamma, beta = torch.rand(c, device=dev, generator=gen) + 0.5, torch.rand(c, device=dev, generator=gen) - 0.5
    stats, dgamma, dbeta = torch.empty(R * groups * 2, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev)
    ws = ops._mosaic_gn_ws(R, c, P, groups, dev)
    roi_b, map_b = 4.0 * rois.numel(), 4.0 * z.numel()
    kernels = [("pack", roi_b + map_b, lambda: _lib.call("ptmi_roi_mosaic_pack", p(rois), p(y), R, c, P, s)),
               ("unpack", roi_b + map_b, lambda: _lib.call("ptmi_roi_mosaic_unpack", p(z), p(back), R, c, P, s)),
               ("mask", 2 * map_b, lambda: _lib.call("ptmi_roi_mosaic_mask", p(z), p(dz), R, c, P, s)),
               ("gn_relu_fwd", 2 * map_b, lambda: _lib.call("ptmi_roi_mosaic_gn_relu_fwd", p(z), p(gamma), p(beta), p(y), p(stats), R, c, P,
                                                            groups, eps, s)),
               ("gn_relu_bwd", 7 * map_b, lambda: _lib.call("ptmi_roi_mosaic_gn_relu_bwd", p(dy), p(y), p(z), p(gamma), p(stats), p(dz),
                                                            p(dgamma), p(dbeta), R, c, P, groups, p(ws), s))]
    lines += ["", f"{'mosaic kernel':16} {'R x c':>12} {'ms':>9} {'GB':>7} {'of HBM':>7}"]
    for name, nbytes, fn in kernels:
        t = time_ms(fn, args.repeat)
        lines.append(f"{name:16} {f'{R}x{c}':>12} {t:9.3f} {nbytes / 1e9:7.2f} {nbytes / (t * 1e-3) / HBM_BYTES_PER_S:7.1%}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
