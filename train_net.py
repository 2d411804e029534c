#!/usr/bin/env python
"""train_net.py -- CLI equivalent of the reference's train_net.py / train.sh for the MI355X-native step.

    python train_net.py --num-gpus 1 --config configs/pt/final_c2f.yaml \
        MODEL.ANCHOR_GENERATOR.NAME DifferentiableAnchorGenerator UNSUPNET.TAU [0.5,0.5] MODEL.VGG.PRETRAIN ''
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_net.py --config ... --synthetic

Same flags as detectron2's default_argument_parser that the reference relies on (--config-file with argparse prefix
matching, --num-gpus, opts); process launch is torchrun-style (one process per GPU, RCCL).

Data: by default the datasets named by cfg.DATASETS.TRAIN_LABEL / TRAIN_UNLABEL / TEST (VOC-format directories registered
under $DETECTRON2_DATASETS as in pt/data/datasets/builtin.py, or ad hoc with --register NAME=DIR:SPLIT:CLASSES; COCO-format
jsons with --register-coco NAME=JSON:IMAGE_ROOT) go through
the host decoder + device two-crop mapper + aspect-ratio grouping (probabilisticteacher_amd/data, reference
pt/data/build.py:107-217); `--synthetic` feeds seeded synthetic two-crop batches in the same record format instead."""
import argparse
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def synthetic_loader(cfg, dev, rank, world):
    from bench import synth_records
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    bl, bu = cfg.SOLVER.IMG_PER_BATCH_LABEL // world, cfg.SOLVER.IMG_PER_BATCH_UNLABEL // world
    assert bl >= 1 and bu >= 1, "batch must be divisible by the world size (pt/data/build.py:174-187)"
    gen = torch.Generator().manual_seed(1234 + rank * 1000 + (cfg.SEED if cfg.SEED >= 0 else 0))
    h, w = 800, 1333
    while True:
        yield (synth_records(gen, bl, h, w, K, dev), synth_records(gen, bl, h, w, K, dev),
               synth_records(gen, bu, h, w, K, dev), synth_records(gen, bu, h, w, K, dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config-file", default="", metavar="FILE")
    ap.add_argument("--num-gpus", type=int, default=1)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--max-iter", type=int, default=None)
    ap.add_argument("--resume", action="store_true",
                    help="continue from MODEL.WEIGHTS (or OUTPUT_DIR/last_checkpoint): weights, optimiser state, iteration")
    ap.add_argument("--eval-only", action="store_true")
    ap.add_argument("--no-statistics", action="store_true",
                    help="log the losses only, without the rpn/ roi_head/ fast_rcnn/ statistics of a reference run's metrics.json")
    ap.add_argument("--detect-anomaly", action="store_true",
                    help="the reference's torch.autograd.set_detect_anomaly: check every activation and gradient for NaN / inf, stop "
                         "BEFORE the update of the first bad step; writes OUTPUT_DIR/anomaly.json and model_before_anomaly.pth")
    ap.add_argument("--register", action="append", default=[], metavar="NAME=DIR:SPLIT:CLS1,CLS2",
                    help="register a VOC-format directory as dataset NAME (Annotations/, JPEGImages/, ImageSets/Main/SPLIT.txt)")
    ap.add_argument("--register-coco", action="append", default=[], metavar="NAME=JSON:IMAGE_ROOT",
                    help="register a COCO-format json (images under IMAGE_ROOT) as dataset NAME")
    ap.add_argument("--image-cache-gb", type=float, default=0.0, metavar="G",
                    help="keep up to G GB of decoded images on this rank's device, so that every file is decoded once (the train "
                         "loader and all evaluations share the cache; nothing is evicted; 0 = off)")
    ap.add_argument("opts", nargs=argparse.REMAINDER)
    args = ap.parse_args()
    rank, local, world = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("LOCAL_RANK", 0), ("WORLD_SIZE", 1)))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from probabilisticteacher_amd.config import setup_cfg
    from probabilisticteacher_amd.engine import PTrainer
    cfg = setup_cfg(args.config_file, ["MODEL.DEVICE", f"cuda:{local}"] + args.opts)
    if cfg.UNSUPNET.Trainer != "pt":
        raise ValueError("Trainer Name is not found.")
    from probabilisticteacher_amd.data import datasets
    for spec in args.register:
        name, rest = spec.split("=", 1)
        dirname, split, classes = rest.split(":")
        datasets.register_pascal_voc(name, dirname, split, tuple(classes.split(",")))
    for spec in args.register_coco:
        name, rest = spec.split("=", 1)
        json_file, image_root = rest.split(":")
        datasets.register_coco_instances(name, json_file, image_root)
    from probabilisticteacher_amd.seeding import seed_all_rng
    seed_all_rng(None if cfg.SEED < 0 else cfg.SEED + rank)    # D2 default_setup
    if cfg.SEED < 0:
        torch.manual_seed(0)                                   # (without a SEED the initial weights stay those of seed 0)
    if args.image_cache_gb < 0:
        raise ValueError(f"--image-cache-gb must not be negative, got {args.image_cache_gb}")
    if args.image_cache_gb > 0 and not args.synthetic:
        from probabilisticteacher_amd.data import DeviceImageCache
        PTrainer.image_cache = DeviceImageCache(int(args.image_cache_gb * 1e9), cfg.MODEL.DEVICE)    # one per process = per rank
    if args.synthetic:
        loader = synthetic_loader(cfg, torch.device("cuda", local), rank, world)
    else:
        loader = PTrainer.build_train_loader(cfg)              # trainer.py:139-141 -> pt/data/build.py:107
    trainer = PTrainer(cfg, data_loader=loader, statistics=not args.no_statistics, detect_anomaly=args.detect_anomaly)
    inc = trainer.resume_or_load(resume=args.resume)          # trainer.py:466-496 (no-op without MODEL.WEIGHTS / checkpoint)
    if inc is not None and rank == 0:
        print(f"loaded {cfg.MODEL.WEIGHTS or 'last_checkpoint'}: start_iter {trainer.start_iter}, "
              f"missing {len(inc.missing_keys)}, unexpected {len(inc.unexpected_keys)}, wrong shape {len(inc.incorrect_shapes)}",
              flush=True)
    if args.eval_only and not args.synthetic:
        # reference train_net.py:60-75: evaluate the STUDENT of the loaded ensemble on cfg.DATASETS.TEST
        res = PTrainer.test(cfg, trainer.model)
        if cfg.TEST.AUG.ENABLED:                               # D2 tools/train_net.py: the TTA results ride along as *_TTA
            res_tta = PTrainer.test_with_TTA(cfg, trainer.model)
            if res is not None and res_tta is not None:
                res.update(res_tta)
        if rank == 0:
            print(res, flush=True)
        return
    if args.eval_only:
        n_batches = args.max_iter or 4
        loader = (next(trainer._data_iter)[1] for _ in range(n_batches))         # the weak labelled views
        names = [f"class{i}" for i in range(cfg.MODEL.ROI_HEADS.NUM_CLASSES)]
        ecfg = cfg.clone()
        ecfg.defrost()
        ecfg.TEST.EVALUATOR = "VOCeval"
        res = PTrainer.test(ecfg, trainer.model, loader, names)
        if rank == 0:
            print({k: v for k, v in res.items() if k == "bbox"}, flush=True)
        return
    # periodic checkpoints, metrics.json, model_final.pth; the student / teacher eval hooks run on cfg.DATASETS.TEST
    from probabilisticteacher_amd.anomaly import AnomalyError
    try:
        trainer.train(max_iter=args.max_iter, run_eval=not args.synthetic)
    except AnomalyError as e:
        # the step was stopped before its update: the weights on the device are the last good ones (iteration iter - 1)
        if rank == 0:
            from probabilisticteacher_amd import checkpoint
            os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
            with open(os.path.join(cfg.OUTPUT_DIR, "anomaly.json"), "w") as f:
                f.write(e.to_json() + "\n")
            checkpoint.save_checkpoint(trainer, os.path.join(cfg.OUTPUT_DIR, "model_before_anomaly.pth"),
                                       iteration=trainer.iter - 1, tag_last=False)
        sys.exit(f"AnomalyError: {e}")
    if PTrainer.image_cache is not None and rank == 0:
        print(PTrainer.image_cache, flush=True)               # images, bytes, hits and misses of rank 0's cache
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
