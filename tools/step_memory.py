"""How much device memory does the train step itself need?  What is left of the HBM is what `--image-cache-gb` may take.

    python tools/step_memory.py [--amp] [--norm GN] [--per-gpu-batch 16] [--steps 4] [--height 800] [--width 1333]

The workload of bench.py (final_c2f.yaml, B labelled + B unlabelled synthetic images per step, teacher + student + EMA) WITHOUT
bench.py's allocator warm-up pool, which would be the peak itself.  Prints one JSON line: the peaks of
`torch.cuda.max_memory_allocated()` and `max_memory_reserved()` over the steps, weights and resident batches included."""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_records  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--amp", action="store_true")
    ap.add_argument("--norm", default="None", help="MODEL.VGG.NORM (GN keeps the pre-norm map z and the output y of every "
                                                   "trainable layer until backward)")
    ap.add_argument("--per-gpu-batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    args = ap.parse_args()
    from probabilisticteacher_amd.config import setup_cfg
    from probabilisticteacher_amd.engine import PTrainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = args.per_gpu_batch
    cfg = setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), [
        "MODEL.DEVICE", "cuda:0", "MODEL.VGG.PRETRAIN", "", "UNSUPNET.BURN_UP_STEP", 0, "SOLVER.IMG_PER_BATCH_LABEL", B,
        "SOLVER.IMG_PER_BATCH_UNLABEL", B, "SOLVER.AMP.ENABLED", bool(args.amp), "MODEL.VGG.NORM", args.norm])
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    torch.manual_seed(0)
    ratio_rng = random.Random(4321)
    trainer = PTrainer(cfg, ratio_fn=lambda: ratio_rng.uniform(0.5, 1.0))
    gen = torch.Generator().manual_seed(1234)
    batches = [tuple(synth_records(gen, B, args.height, args.width, K, dev) for _ in range(4)) for _ in range(2)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for i in range(args.steps):
        trainer.run_step(batches[i % 2])
    torch.cuda.synchronize()
    gb = 1e-9
    print(json.dumps({"amp": bool(args.amp), "norm": args.norm, "per_gpu_batch": B, "steps": args.steps, "image": [args.height, args.width],
                      "allocated_before_the_steps_gb": round(before * gb, 3),
                      "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() * gb, 3),
                      "max_memory_reserved_gb": round(torch.cuda.max_memory_reserved() * gb, 3),
                      "total_memory_gb": round(torch.cuda.get_device_properties(dev).total_memory * gb, 1)}))


if __name__ == "__main__":
    main()
