"""How many source images per second does the two-crop train loader deliver from files, with no model behind it?

    python tools/loader_bench.py [--root DIR] [--workers 0,2,4,8,16] [--records 200] [--min-seconds 2] [--warmup-batches 2] [--out FILE]
                                 [--image-cache-gb G]

Writes (once; an existing --root is reused) VOC-layout datasets of generated images with Pillow and a fixed seed -- PNG and
JPEG, at 2048x1024 (Cityscapes) and 1242x375 (KITTI) -- and times `build_detection_semisup_train_loader_two_crops` of
configs/pt/final_c2f.yaml (16 + 16 images per batch, MIN_SIZE_TRAIN 600) on each of them for every DATALOADER.NUM_WORKERS
asked for: records/s = source images (labelled + unlabelled) consumed per second over >= --records records and >= --min-seconds
after the warm-up batches, the device drained at both ends.  One JSON line per leg; the step needs 32 records per step time.
--image-cache-gb G adds, after every leg, the same leg through a DeviceImageCache (data/cache.py): a first pass fills the cache,
the second pass is the one timed, and the line says how many of its reads were hits."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from probabilisticteacher_amd.config import setup_cfg  # noqa: E402
from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops, datasets  # noqa: E402

CASES = (("png_2048x1024", "PNG", 1024, 2048), ("jpeg_2048x1024", "JPEG", 1024, 2048),
         ("png_1242x375", "PNG", 375, 1242), ("jpeg_1242x375", "JPEG", 375, 1242))
N_FILES = 24          # per dataset (labelled and unlabelled each)


def _image(rng, h, w):
    """street-scene-like statistics rather than noise: smooth gradients, a few flat rectangles, mild sensor noise (noise alone
    would make PNG's inflate and JPEG's entropy decoding unrepresentatively slow)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([96 + 64 * np.sin(x / rng.uniform(90, 400) + rng.uniform(0, 6)) + 40 * np.cos(y / rng.uniform(60, 300))
                    for _ in range(3)], axis=-1)
    boxes = []
    for _ in range(int(rng.randint(3, 9))):
        bw, bh = int(rng.randint(w // 16, w // 4)), int(rng.randint(h // 8, h // 2))
        x1, y1 = int(rng.randint(1, w - bw)), int(rng.randint(1, h - bh))
        img[y1:y1 + bh, x1:x1 + bw] = rng.randint(0, 256, 3)
        boxes.append((x1, y1, x1 + bw, y1 + bh))
    img += rng.normal(0.0, 3.0, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8), boxes


def write_dataset(root, fmt, h, w, seed):
    from PIL import Image
    for sub in ("JPEGImages", "Annotations", "ImageSets/Main"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    rng = np.random.RandomState(seed)
    ids = [f"{i:04d}" for i in range(N_FILES)]
    for fid in ids:
        img, boxes = _image(rng, h, w)
        # the reader opens JPEGImages/<id>.jpg; Pillow picks the decoder by content
        Image.fromarray(img).save(os.path.join(root, "JPEGImages", fid + ".jpg"), format=fmt, **({"quality": 92} if fmt == "JPEG" else {}))
        xml = f"<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size>" + "".join(
            f"<object><name>car</name><difficult>0</difficult><bndbox><xmin>{a}</xmin><ymin>{b}</ymin><xmax>{c}</xmax><ymax>{d}</ymax>"
            "</bndbox></object>" for a, b, c, d in boxes) + "</annotation>"
        with open(os.path.join(root, "Annotations", fid + ".xml"), "w") as f:
            f.write(xml)
    with open(os.path.join(root, "ImageSets", "Main", "train.txt"), "w") as f:
        f.write("\n".join(ids) + "\n")


def time_loader(case, workers, records, min_seconds, warmup_batches, device, cache_gb=0.0):
    """cache_gb > 0: the cached leg -- a first pass (not timed) runs until every file of both datasets is resident in a
    DeviceImageCache of that budget, or until 4 epochs' worth of records have gone by if the budget holds fewer; the timed
    pass that follows is the steady state"""
    cfg = setup_cfg("configs/pt/final_c2f.yaml", [
        "MODEL.DEVICE", device, "DATASETS.TRAIN_LABEL", (f"lb_{case}_label",), "DATASETS.TRAIN_UNLABEL", (f"lb_{case}_unlabel",),
        "DATALOADER.NUM_WORKERS", workers])
    per_batch = cfg.SOLVER.IMG_PER_BATCH_LABEL + cfg.SOLVER.IMG_PER_BATCH_UNLABEL
    need = -(-records // per_batch)
    cache = None
    if cache_gb > 0:
        from probabilisticteacher_amd.data import DeviceImageCache
        cache = DeviceImageCache(int(cache_gb * 1e9), device)
        loader = build_detection_semisup_train_loader_two_crops(cfg, seed=3, image_cache=cache)
        fill = 0
        while len(cache) < 2 * N_FILES and fill * per_batch < 4 * 2 * N_FILES:
            next(loader)
            fill += 1
    else:
        loader = build_detection_semisup_train_loader_two_crops(cfg, seed=3)
    for _ in range(warmup_batches):
        next(loader)
    torch.cuda.synchronize()
    hits0, misses0 = (cache.hits, cache.misses) if cache is not None else (0, 0)
    t0, c0 = time.perf_counter(), time.thread_time()
    batches = 0
    while batches < need or time.perf_counter() - t0 < min_seconds:
        next(loader)
        batches += 1
    c1 = time.thread_time()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    timed = (cache.hits - hits0, cache.misses - misses0) if cache is not None else None
    if hasattr(loader, "close"):
        loader.close()
    out = {"case": case, "workers": workers, "records": batches * per_batch, "seconds": round(dt, 4),
           "records_per_s": round(batches * per_batch / dt, 2), "ms_per_batch": round(1e3 * dt / batches, 2),
           "consumer_thread_cpu_ms_per_batch": round(1e3 * (c1 - c0) / batches, 2)}
    if cache is not None:
        out.update(image_cache_gb=cache_gb, cached_images=len(cache), cache_bytes_used=cache.bytes_used,
                   timed_pass_hits=timed[0], timed_pass_misses=timed[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="where the generated datasets live (default: a temporary directory)")
    ap.add_argument("--workers", default="0,2,4,8,16")
    ap.add_argument("--records", type=int, default=200)
    ap.add_argument("--min-seconds", type=float, default=2.0, help="keep a leg running at least this long")
    ap.add_argument("--warmup-batches", type=int, default=2)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--image-cache-gb", type=float, default=0.0,
                    help="> 0: after each leg, the same leg with a DeviceImageCache of this budget -- the first pass fills it, "
                         "the second is timed (48 files of 2048x1024 are 0.30 GB)")
    ap.add_argument("--write-only", action="store_true", help="write the missing datasets under --root and stop")
    args = ap.parse_args()
    tmp = None
    root = args.root
    if root is None:
        tmp = tempfile.TemporaryDirectory()
        root = tmp.name
    wanted = args.cases.split(",")
    missing = [(os.path.join(root, case, part), fmt, h, w, 100 + 2 * k + j) for k, (case, fmt, h, w) in enumerate(CASES)
               for j, part in enumerate(("label", "unlabel")) if case in wanted
               and not os.path.exists(os.path.join(root, case, part, "ImageSets", "Main", "train.txt"))]
    if args.write_only:
        for d, fmt, h, w, seed in missing:
            write_dataset(d, fmt, h, w, seed)
        return
    if missing:
        # in a child: the timed process is the same whether the files were there or not (generating 25 MB float arrays here
        # would leave the allocator in another state than a process that only reads has: +30 % on the serial 2048x1024 legs)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--write-only", "--root", root, "--cases", args.cases])
    for case in wanted:
        for part in ("label", "unlabel"):
            datasets.register_pascal_voc(f"lb_{case}_{part}", os.path.join(root, case, part), "train", ("car",))
    for case in wanted:
        for workers in (int(v) for v in args.workers.split(",")):
            for cache_gb in (0.0, args.image_cache_gb) if args.image_cache_gb > 0 else (0.0,):
                line = json.dumps(time_loader(case, workers, args.records, args.min_seconds, args.warmup_batches, args.device,
                                              cache_gb))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
