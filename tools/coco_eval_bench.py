#!/usr/bin/env python
"""Time the COCO evaluator's three stages on a synthetic, seeded val2017-sized set:

    python tools/coco_eval_bench.py [--images 5000] [--classes 80] [--dets 100] [--gts 7] [--ref-images 100]

5000 images x 80 categories, 100 detections and about 7 ground-truth boxes per image with bench.py's box statistics
(log-uniform 32 .. 400 px sides on 1333 x 800).  Prints one JSON line: the matching kernel (HIP events around
ops.coco_match, median of 5), the literal Python restatement of pycocotools (tests/coco_eval_ref.py) on the first
--ref-images images scaled linearly to --images, and the host work around the kernel (packing, accumulate + summarize)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(n_img, K, n_dt, n_gt, seed=0, h=800, w=1333):
    rng = np.random.RandomState(seed)

    def boxes(n):
        bw = np.exp(rng.rand(n) * (math.log(400) - math.log(32)) + math.log(32))
        bh = np.exp(rng.rand(n) * (math.log(400) - math.log(32)) + math.log(32))
        cx, cy = rng.rand(n) * w, rng.rand(n) * h
        b = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
        b[:, 0::2] = b[:, 0::2].clip(0, w)
        b[:, 1::2] = b[:, 1::2].clip(0, h)
        return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)

    gt_img = np.repeat(np.arange(n_img), n_gt)
    gt = boxes(n_img * n_gt)
    gt_cat = rng.randint(0, K, n_img * n_gt)
    gt_crowd = (rng.rand(n_img * n_gt) < 0.03).astype(np.int32)
    # half of the detections are jittered copies of their image's ground truth (same class), half are anything
    dt_img = np.repeat(np.arange(n_img), n_dt)
    src = dt_img * n_gt + rng.randint(0, n_gt, n_img * n_dt)
    hit = rng.rand(n_img * n_dt) < 0.5
    dt = np.where(hit[:, None], gt[src] * (1 + 0.15 * rng.randn(n_img * n_dt, 4)), boxes(n_img * n_dt))
    dt[:, 2:] = np.abs(dt[:, 2:]) + 1.0
    dt = dt.astype(np.float32).astype(np.float64)
    dt_cat = np.where(hit, gt_cat[src], rng.randint(0, K, n_img * n_dt))
    dt_score = rng.rand(n_img * n_dt).astype(np.float32).astype(np.float64)
    return dict(dt_img=dt_img, dt_cat=dt_cat, dt_score=dt_score, dt_xywh=dt, gt_img=gt_img, gt_cat=gt_cat, gt_xywh=gt,
                gt_area=gt[:, 2] * gt[:, 3], gt_crowd=gt_crowd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=7)
    ap.add_argument("--ref-images", type=int, default=100)
    args = ap.parse_args()
    from probabilisticteacher_amd import evaluation, ops
    from tests import coco_eval_ref as ref
    dev = torch.device("cuda", 0)
    names = [f"c{k}" for k in range(args.classes)]
    data = synth(args.images, args.classes, args.dets, args.gts)
    t0 = time.perf_counter()
    packed = evaluation.coco_pack(args.images, args.classes, **data)
    t_pack = time.perf_counter() - t0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    a = [up(packed[k]) for k in ("dt_xywh", "dt_area")] + [torch.from_numpy(packed["dt_off"])] + \
        [up(packed[k]) for k in ("gt_xywh", "gt_area", "gt_crowd")] + [torch.from_numpy(packed["gt_off"])] + \
        [up(evaluation.COCO_IOU_THRS), up(evaluation.COCO_AREA_RNG)]
    ops.coco_match(*a)                                       # warm-up
    torch.cuda.synchronize()
    wall, kern = [], []
    for _ in range(5):
        ops.profile_start()
        t0 = time.perf_counter()
        out = ops.coco_match(*a)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        kern.append(ops.profile_stop()["coco_match"]["ms"] * 1e-3)
    tables = tuple(t.cpu().numpy() for t in out)
    t0 = time.perf_counter()
    res = evaluation.coco_summarize(*evaluation.coco_accumulate(packed, *tables), names)
    t_acc = time.perf_counter() - t0
    # the literal reference: computeIoU + evaluateImg over every (image, category) pair of the first --ref-images images
    n_ref = min(args.ref_images, args.images)
    segs = []
    for k in range(args.classes):
        for i in range(n_ref):
            s = k * args.images + i
            d, g = slice(packed["dt_off"][s], packed["dt_off"][s + 1]), slice(packed["gt_off"][s], packed["gt_off"][s + 1])
            segs.append({"dt_xywh": packed["dt_xywh"][d], "dt_score": packed["dt_score"][d], "dt_area": packed["dt_area"][d],
                         "gt_xywh": packed["gt_xywh"][g], "gt_area": packed["gt_area"][g], "gt_crowd": packed["gt_crowd"][g]})
    t0 = time.perf_counter()
    want = ref.match_tables(segs)
    t_ref = time.perf_counter() - t0
    same = True
    pos_d = pos_g = 0
    for k in range(args.classes):                            # the subset's tables against the kernel's, entry for entry
        s0, s1 = k * args.images, k * args.images + n_ref
        d, g = slice(packed["dt_off"][s0], packed["dt_off"][s1]), slice(packed["gt_off"][s0], packed["gt_off"][s1])
        nd, ng = d.stop - d.start, g.stop - g.start
        same &= bool(np.array_equal(tables[0][:, g], want[0][:, pos_g:pos_g + ng]) and
                     np.array_equal(tables[1][:, :, d], want[1][:, :, pos_d:pos_d + nd]) and
                     np.array_equal(tables[2][:, :, d], want[2][:, :, pos_d:pos_d + nd]))
        pos_d, pos_g = pos_d + nd, pos_g + ng
    print(json.dumps({
        "images": args.images, "classes": args.classes, "detections": int(len(packed["dt_score"])), "ground_truth": int(len(packed["gt_area"])),
        "segments": args.images * args.classes, "longest_gt_segment": int(np.diff(packed["gt_off"]).max()),
        "match_kernel_s": float(np.median(kern)), "match_call_s": float(np.median(wall)),
        "reference_match_s_scaled": t_ref * args.images / n_ref, "reference_match_s_measured": t_ref, "reference_images": n_ref,
        "host_pack_s": t_pack, "host_accumulate_s": t_acc, "tables_equal_on_subset": same, "AP": res["bbox"]["AP"],
        "AP50": res["bbox"]["AP50"]}), flush=True)


if __name__ == "__main__":
    main()
