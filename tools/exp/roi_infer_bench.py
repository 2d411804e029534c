#!/usr/bin/env python
"""tools/exp/roi_infer_bench.py -- HIP-event time of GuassianFastRCNNOutputLayers.inference() (teacher pseudo-labelling, the
eval path) for 16 images x 2000 proposals at 800 x 1333, on the dense NMS path and on the per-(image, class) path:
K = 8 and K = 20 on both, K = 80 by class only (its dense bitmask would need 51 GB).  The time includes the call's one
device->host read.  Two score distributions: `flat` (randn * 2 logits: thousands of candidates per image) and `peaked` (a trained
teacher: a few hundred).  Also the row-per-thread classification losses at C = K + 1 columns, forward + gradient.
    python tools/exp/roi_infer_bench.py [--iters 5] [--out profiles/roi_infer_by_class.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from probabilisticteacher_amd import ops  # noqa: E402
from probabilisticteacher_amd.config import setup_cfg  # noqa: E402
from probabilisticteacher_amd.modeling.roi_heads import (GuassianFastRCNNOutputLayers, nms_ws_bytes_by_class,  # noqa: E402
                                                         nms_ws_bytes_dense)
from probabilisticteacher_amd.structures import Boxes, FreeInstances  # noqa: E402

DEV = "cuda:0"
N, PER, H, W = 16, 2000, 800, 1333


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def case(gen, K, peaked):
    R = N * PER
    scores = torch.randn(R, K + 1, generator=gen) * 2.0
    if peaked:
        scores *= 0.2
        scores[:, K] += 6.0
        idx = torch.randperm(R, generator=gen)[:N * 150]
        scores[idx, torch.randint(0, K, (N * 150,), generator=gen)] += 9.0
    deltas = torch.randn(R, 8 * K, generator=gen)
    deltas.view(R, K, 8)[..., :2] *= 2.0
    deltas.view(R, K, 8)[..., 2:4] *= 1.5
    props = []
    for _ in range(N):
        cx, cy = torch.rand(PER, generator=gen) * W, torch.rand(PER, generator=gen) * H
        bw, bh = 8 + torch.rand(PER, generator=gen) * W * 0.5, 8 + torch.rand(PER, generator=gen) * H * 0.5
        b = torch.stack([(cx - bw / 2).clamp(0, W), (cy - bh / 2).clamp(0, H), (cx + bw / 2).clamp(0, W),
                         (cy + bh / 2).clamp(0, H)], 1)
        p = FreeInstances((H, W))
        p.proposal_boxes = Boxes(b.to(DEV))
        props.append(p)
    return scores.to(DEV), deltas.to(DEV), props


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = [f"GuassianFastRCNNOutputLayers.inference(), {N} images x {PER} proposals, {H} x {W}, HIP-event ms per call "
             f"(mean of {a.iters} after one warm-up call), {torch.cuda.get_device_name(0)}",
             f"{'K':>3s} {'scores':>7s} {'path':>9s} {'ms':>9s} {'NMS mask MB':>12s} {'detections':>11s}"]
    for K in (8, 20, 80):
        cfg = setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"),
                        ["MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "MODEL.ROI_HEADS.NUM_CLASSES", K])
        layer = GuassianFastRCNNOutputLayers(cfg, 1024)
        for peaked in (False, True):
            scores, deltas, props = case(torch.Generator().manual_seed(K), K, peaked)
            for by_class in (False, True):
                if K == 80 and not by_class:
                    continue
                layer.nms_by_class = by_class
                det = sum(len(r) for r in layer.inference((scores, deltas), props)[0])
                ms = timeit(lambda: layer.inference((scores, deltas), props), a.iters)
                mb = (nms_ws_bytes_by_class if by_class else nms_ws_bytes_dense)(N, K, PER) / 1e6
                lines.append(f"{K:3d} {'peaked' if peaked else 'flat':>7s} {'by class' if by_class else 'dense':>9s} {ms:9.3f} "
                             f"{mb:12.1f} {det:11d}")
                print(lines[-1], flush=True)
            ops._WS.clear()                                 # the grow-only scratch: the next K starts without the last one's mask
            torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"classification losses, forward + gradient in one launch, R = {N * 512} rows, ms per call")
    lines.append(f"{'C':>3s} {'softmax_ce_mean':>16s} {'soft_ce_efl':>12s}")
    gen = torch.Generator().manual_seed(1)
    R = N * 512
    for K in (8, 20, 80):
        logits = (torch.randn(R, K + 1, generator=gen) * 2.0).to(DEV).requires_grad_()
        gt = torch.randint(0, K + 1, (R,), generator=gen).to(DEV)
        soft = torch.softmax(torch.randn(R, K + 1, generator=gen), -1).to(DEV)
        t0 = timeit(lambda: ops.softmax_ce_mean(logits, gt), a.iters * 4)
        t1 = timeit(lambda: ops.soft_ce_efl(soft, logits, 0.25, 0.5, True, 1.0 / R), a.iters * 4)
        lines.append(f"{K + 1:3d} {t0:16.4f} {t1:12.4f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
