"""GPU (pytest -m gpu): the device image cache behind the train loader, the test loader and PTrainer.test, on six PNG files of
5x7, 33x17 and 64x48 pixels (two of each): the batches and the evaluation results are those of a run without the cache, a
resident file is never decoded again, and nothing ever writes to a cached tensor."""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_loader_workers_gpu import _same_record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(7, 5), (17, 33), (48, 64)] * 2          # (h, w) of file A0 .. A5
PASSES, BATCHES = 3, 8


def _write(tmp_path):
    """one VOC directory, three splits: label = A0 A1 A2, unlabel = A3 A4 A5 (one file of every size each), all = the six"""
    from PIL import Image
    from probabilisticteacher_amd.data import datasets
    root = str(tmp_path / "ic")
    for sub in ("JPEGImages", "Annotations", "ImageSets/Main"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    rng = np.random.RandomState(21)
    ids = [f"A{k}" for k in range(6)]
    for fid, (h, w) in zip(ids, SIZES):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, "JPEGImages", fid + ".jpg"), format="PNG")
        with open(os.path.join(root, "Annotations", fid + ".xml"), "w") as f:
            f.write(f"<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size><object><name>car</name>"
                    f"<difficult>0</difficult><bndbox><xmin>2</xmin><ymin>2</ymin><xmax>{w - 1}</xmax><ymax>{h - 1}</ymax></bndbox>"
                    "</object></annotation>")
    for split, part in (("label", ids[:3]), ("unlabel", ids[3:]), ("all", ids)):
        with open(os.path.join(root, "ImageSets", "Main", split + ".txt"), "w") as f:
            f.write("\n".join(part) + "\n")
        datasets.register_pascal_voc("ic_" + split, root, split, ("car",))
    return {os.path.realpath(os.path.join(root, "JPEGImages", fid + ".jpg")): 3 * h * w for fid, (h, w) in zip(ids, SIZES)}


def _cfg(tmp_path, *extra):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg("configs/pt/final_s2c.yaml", [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1,
        "DATASETS.TRAIN_LABEL", ("ic_label",), "DATASETS.TRAIN_UNLABEL", ("ic_unlabel",), "DATASETS.TEST", ("ic_all",),
        "INPUT.MIN_SIZE_TRAIN", (16, 24), "INPUT.MAX_SIZE_TRAIN", 64, "INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 320,
        "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0, "OUTPUT_DIR", str(tmp_path / "out"), "DATALOADER.NUM_WORKERS", 2, *extra])


def _count_decodes(monkeypatch):
    """every decode goes through datasets.read_image_hwc (the workers) or datasets.read_image (NUM_WORKERS 0)"""
    import threading
    from probabilisticteacher_amd.data import datasets
    lock, seen = threading.Lock(), []

    def wrap(fn):
        def f(file_name, *a):
            with lock:
                seen.append(os.path.realpath(file_name))
            return fn(file_name, *a)
        return f
    monkeypatch.setattr(datasets, "read_image_hwc", wrap(datasets.read_image_hwc))
    monkeypatch.setattr(datasets, "read_image", wrap(datasets.read_image))
    return seen


def _pass(cfg, cache):
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops
    loader = build_detection_semisup_train_loader_two_crops(cfg, seed=9, image_cache=cache)
    try:
        return [next(loader) for _ in range(BATCHES)]
    finally:
        loader.close()


@pytest.mark.parametrize("crop", [False, True])
def test_batches_are_byte_identical_and_resident_files_are_not_decoded(tmp_path, monkeypatch, crop):
    from probabilisticteacher_amd.data import DeviceImageCache, build_detection_test_loader, datasets, training_sampler
    size_of = _write(tmp_path)
    extra = ("INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "relative_range", "INPUT.CROP.SIZE", (0.6, 0.7)) if crop else ()
    cfg = _cfg(tmp_path, *extra)
    real_read = datasets.read_image
    ref = _pass(cfg, None)
    assert any(len(r["instances"].gt_boxes) for b in ref for r in b[0]) and all("instances" not in r for b in ref for r in b[2])
    # the two files the stream reads first (label, then unlabel, of seed 9) are what a budget of their two sizes holds
    first = [os.path.realpath(datasets.get_dataset_dicts([n])[next(training_sampler(3, s))]["file_name"])
             for n, s in (("ic_label", 9), ("ic_unlabel", 10))]
    ample, two = DeviceImageCache(1 << 20, DEV), DeviceImageCache(size_of[first[0]] + size_of[first[1]], DEV)
    seen = _count_decodes(monkeypatch)
    for cache, resident in ((ample, sorted(size_of)), (two, sorted(first))):
        for p in range(PASSES):
            del seen[:]
            misses = cache.misses
            got = _pass(cfg, cache)
            torch.cuda.synchronize()
            for i, (rb, gb) in enumerate(zip(ref, got)):
                for s, (rs, gs) in enumerate(zip(rb, gb)):
                    assert len(rs) == len(gs) == 1
                    _same_record(gs[0], rs[0], f"{len(resident)} resident, pass {p}, batch {i}, stream {s}")
            assert cache.bytes_used <= cache.budget_bytes and len(seen) <= cache.misses - misses
            assert not set(seen) & set(k[0] for k, _ in cache.items()) or p == 0, "a resident file was decoded"
            if p > 0:
                assert sorted(set(seen)) == sorted(set(size_of) - set(resident)), "exactly the files that are not resident"
        assert sorted(k[0] for k, _ in cache.items()) == resident and cache.hits > 0
        assert cache.bytes_used == sum(size_of[f] for f in resident)
        # one pass over the six files, each once (the test loader, which shares the cache): the count itself
        for workers in (2, 0):
            del seen[:]
            recs = list(build_detection_test_loader(_cfg(tmp_path, "DATALOADER.NUM_WORKERS", workers, *extra), "ic_all",
                                                    batch_size=4, image_cache=cache))
            assert sorted(seen) == sorted(set(size_of) - set(resident)) and [len(b) for b in recs] == [4, 2]
    # read-only: flips, crops, resizes and the strong augmentation have run over every cached tensor, three passes each
    torch.cuda.synchronize()
    for cache in (ample, two):
        for (path, _, _, bgr), img in cache.items():
            assert bgr is (cfg.INPUT.FORMAT == "BGR") and img.device == torch.device(DEV) and img.dtype == torch.uint8
            assert torch.equal(img.cpu(), real_read(path, cfg.INPUT.FORMAT)), f"{path}: the cached tensor was written to"


def _equal_results(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal_results(a[k], b[k]) for k in a)
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b


def test_second_evaluation_decodes_nothing_and_results_are_unchanged(tmp_path, monkeypatch):
    from probabilisticteacher_amd import modeling
    from probabilisticteacher_amd.data import DeviceImageCache
    from probabilisticteacher_amd.engine import PTrainer
    size_of = _write(tmp_path)
    cfg = _cfg(tmp_path)
    models = []
    for seed in (0, 1):                                           # "student", then "teacher"
        torch.manual_seed(seed)
        models.append(modeling.build_model(cfg).to(DEV))
    assert PTrainer.image_cache is None
    seen = _count_decodes(monkeypatch)
    off = [PTrainer.test(cfg, m) for m in models]
    assert len(seen) == 12, "without the cache both evaluations decode every file"
    assert all(np.isfinite(r["bbox"]["AP50"]) for r in off)
    cache = DeviceImageCache(1 << 20, DEV)
    monkeypatch.setattr(PTrainer, "image_cache", cache)
    on = []
    for k, m in enumerate(models):
        del seen[:]
        on.append(PTrainer.test(cfg, m))
        assert sorted(seen) == (sorted(size_of) if k == 0 else []), "the first evaluation decodes each file once, the second none"
    assert (len(cache), cache.misses, cache.hits) == (6, 6, 6) and cache.bytes_used == sum(size_of.values())
    for k in range(2):
        assert _equal_results(on[k], off[k]), (on[k], off[k])
