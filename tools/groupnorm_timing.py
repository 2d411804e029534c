#!/usr/bin/env python
"""HIP-event time of the two GroupNorm entries (csrc/groupnorm.hip) at the train step's own layer shapes:

    python tools/groupnorm_timing.py [--images 16] [--height 800] [--width 1333] [--repeat 10] [--out profiles/groupnorm_timing.txt]

conv1_1 ... conv5_3 of VGG16 on `--images` maps of height x width (the pool halves both, rounding down).  For every layer: one untimed
call of ptmi_gn_relu_fwd and ptmi_gn_relu_bwd (ReLU on), then `--repeat` timed ones between HIP events on the kernels' stream; the
MEDIAN is reported.  Bytes moved are counted from the shapes: forward reads z twice (statistics, apply) and writes y = 3 maps;
backward reads dy, y, z twice (plane sums, apply) and writes dz = 7 maps; the parameter vectors, statistics and partial sums are
below 0.1 % of that and left out.  "of HBM" is bytes / time over 6.29 TB/s, the rate a float4 copy reaches on an MI355X.  A map
that fits the 256 MB Infinity Cache (conv5) can exceed it on its second read.  No threshold is set on any number."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
LAYERS = [("conv1_1", 64, 0), ("conv1_2", 64, 0), ("conv2_1", 128, 1), ("conv2_2", 128, 1), ("conv3_1", 256, 2), ("conv3_2", 256, 2),
          ("conv3_3", 256, 2), ("conv4_1", 512, 3), ("conv4_2", 512, 3), ("conv4_3", 512, 3), ("conv5_1", 512, 4), ("conv5_2", 512, 4),
          ("conv5_3", 512, 4)]


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
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupnorm_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "groupnorm_timing needs the GPU: there is no CPU path to time"
    from probabilisticteacher_amd import _lib, ops
    dev = torch.device("cuda", 0)
    p, groups, eps = ops._ptr, 32, 1e-5
    lines = [f"# tools/groupnorm_timing.py --images {args.images} --height {args.height} --width {args.width} --repeat {args.repeat}",
             f"# {torch.cuda.get_device_name(0)}; median of {args.repeat} HIP-event timings per entry, ReLU on; HBM rate {HBM_BYTES_PER_S / 1e12:.2f} TB/s",
             f"{'layer':8} {'n x c x h x w':>22} {'L':>9} {'fwd ms':>8} {'fwd GB':>7} {'of HBM':>7} {'bwd ms':>8} {'bwd GB':>7} {'of HBM':>7}"]
    tot = [0.0, 0.0, 0.0, 0.0]
    shape = None
    for name, c, pools in LAYERS:
        n, h, w = args.images, args.height >> pools, args.width >> pools
        if shape != (n, c, h, w):
            shape = (n, c, h, w)
            z = dy = y = dz = None                 # free the previous layer's maps first
            gen = torch.Generator(device=dev).manual_seed(c + h)
            z = torch.randn(shape, device=dev, generator=gen)
            dy = torch.randn(shape, device=dev, generator=gen)
            y, dz = torch.empty_like(z), torch.empty_like(z)
            gamma, beta = torch.rand(c, device=dev, generator=gen) + 0.5, torch.rand(c, device=dev, generator=gen) - 0.5
            stats, dgamma, dbeta = torch.empty(n * groups * 2, device=dev), torch.empty(c, device=dev), torch.empty(c, device=dev)
            ws = ops._gn_ws(n, c, h * w, groups, dev)
        s = ops._stream()

        def fwd():
            _lib.call("ptmi_gn_relu_fwd", p(z), p(gamma), p(beta), p(y), p(stats), n, c, h * w, groups, eps, 1, p(ws), s)

        def bwd():
            _lib.call("ptmi_gn_relu_bwd", p(dy), p(y), p(z), p(gamma), p(stats), p(dz), p(dgamma), p(dbeta), n, c, h * w, groups, 1,
                      p(ws), s)
        tf, tb = time_ms(fwd, args.repeat), time_ms(bwd, args.repeat)
        map_bytes = 4.0 * z.numel()
        bf, bb = 3 * map_bytes, 7 * map_bytes
        lines.append(f"{name:8} {'x'.join(str(v) for v in shape):>22} {(c // groups) * h * w:9d} {tf:8.3f} {bf / 1e9:7.2f} "
                     f"{bf / (tf * 1e-3) / HBM_BYTES_PER_S:7.1%} {tb:8.3f} {bb / 1e9:7.2f} {bb / (tb * 1e-3) / HBM_BYTES_PER_S:7.1%}")
        tot = [tot[0] + tf, tot[1] + bf, tot[2] + tb, tot[3] + bb]
    lines.append(f"{'all 13':8} {'':>22} {'':>9} {tot[0]:8.3f} {tot[1] / 1e9:7.2f} {tot[1] / (tot[0] * 1e-3) / HBM_BYTES_PER_S:7.1%} "
                 f"{tot[2]:8.3f} {tot[3] / 1e9:7.2f} {tot[3] / (tot[2] * 1e-3) / HBM_BYTES_PER_S:7.1%}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
