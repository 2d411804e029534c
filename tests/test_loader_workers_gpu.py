"""GPU (pytest -m gpu): DATALOADER.NUM_WORKERS on the device -- the ptmi_aug_unpack_hwc_batched kernel byte for byte against
numpy, and the worker path of the train / test loaders against the serial path (NUM_WORKERS 0) on files from disk."""
import os

import numpy as np
import pytest
import torch

from tests.test_host_logic import _write_voc_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_unpack_hwc_batch_is_byte_exact():
    """one launch over mixed sizes: widths with every row-tail length and odd row pitches (rows that start unaligned), a
    single row, a large image, and sources that start 1, 2 and 3 bytes off a dword boundary"""
    from probabilisticteacher_amd.data.augment import unpack_hwc_batch
    rng = np.random.RandomState(7)
    shapes = [(5, 1), (4, 3), (7, 5), (3, 127), (1, 64), (1, 1), (2, 1333), (9, 8), (6, 6), (300, 501), (1024, 2048)]
    arrs, srcs = [], []
    for h, w in shapes:
        arrs.append(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        srcs.append(torch.from_numpy(arrs[-1]).to(DEV))
    for off, (h, w) in ((1, (6, 16)), (2, (5, 127)), (3, (4, 1333)), (1, (3, 5)), (3, (1, 4))):
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        buf = torch.zeros(a.size + 8, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 4 == 0
        view = buf[off:off + a.size].view(h, w, 3)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 4 == off
        arrs.append(a)
        srcs.append(view)
    for bgr in (True, False):
        out = unpack_hwc_batch(srcs, bgr)
        torch.cuda.synchronize()
        assert len(out) == len(srcs)
        for a, o in zip(arrs, out):
            want = (a[:, :, ::-1] if bgr else a).transpose(2, 0, 1)
            assert o.dtype == torch.uint8 and tuple(o.shape) == want.shape and o.is_contiguous()
            assert np.array_equal(o.cpu().numpy(), want), f"{a.shape} bgr={bgr}"
    assert unpack_hwc_batch([], True) == []
    with pytest.raises(ValueError):
        unpack_hwc_batch([torch.zeros((3, 4, 5), dtype=torch.uint8, device=DEV)], True)


def _datasets(tmp_path):
    from probabilisticteacher_amd.data import datasets
    rng = np.random.RandomState(4)
    names = ("car",)
    for sub, n, (h, w) in (("label", 7, (160, 224)), ("unlabel", 5, (150, 231)), ("val", 5, (131, 203))):
        _write_voc_dir(str(tmp_path / sub), [f"{sub}{i}" for i in range(n)], names, rng, h=h, w=w)
        os.rename(tmp_path / sub / "ImageSets" / "Main" / "train.txt", tmp_path / sub / "ImageSets" / "Main" / "split.txt")
        datasets.register_pascal_voc("lw_" + sub, str(tmp_path / sub), "split", names)


def _cfg(tmp_path, workers, *extra):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg("configs/pt/final_s2c.yaml", [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "UNSUPNET.BURN_UP_STEP", 1, "SOLVER.IMG_PER_BATCH_LABEL", 2,
        "SOLVER.IMG_PER_BATCH_UNLABEL", 3, "DATASETS.TRAIN_LABEL", ("lw_label",), "DATASETS.TRAIN_UNLABEL", ("lw_unlabel",),
        "DATASETS.TEST", ("lw_val",), "INPUT.MIN_SIZE_TRAIN", (128, 160), "INPUT.MAX_SIZE_TRAIN", 320,
        "INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 320, "OUTPUT_DIR", str(tmp_path / "out"), "SOLVER.CHECKPOINT_PERIOD", 100,
        "DATALOADER.NUM_WORKERS", workers, *extra])


def _same_record(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "instances":
            assert a[k].image_size == b[k].image_size, what
            assert torch.equal(a[k].gt_boxes.tensor, b[k].gt_boxes.tensor), f"{what}: gt_boxes"
            assert torch.equal(a[k].gt_classes, b[k].gt_classes), f"{what}: gt_classes"
        elif isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].device == b[k].device and torch.equal(a[k], b[k]), f"{what}: {k}"
        else:
            assert a[k] == b[k], f"{what}: {k}"


@pytest.mark.parametrize("crop", [False, True])
def test_train_loader_batches_are_those_of_the_serial_path(tmp_path, crop):
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops
    _datasets(tmp_path)
    extra = ("INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "relative_range", "INPUT.CROP.SIZE", (0.6, 0.7)) if crop else ()
    runs = {}
    for workers in (0, 3):
        loader = build_detection_semisup_train_loader_two_crops(_cfg(tmp_path, workers, *extra), seed=9)
        runs[workers] = [next(loader) for _ in range(6)]
        loader.close()
    torch.cuda.synchronize()
    for i, (ref, got) in enumerate(zip(runs[0], runs[3])):
        assert [len(s) for s in got] == [2, 2, 3, 3]
        for s, (rs, gs) in enumerate(zip(ref, got)):
            for j, (r, g) in enumerate(zip(rs, gs)):
                assert g["image"].is_cuda and g["image"].dtype == torch.uint8
                assert (g["height"], g["width"]) == tuple(g["image"].shape[-2:])
                _same_record(g, r, f"batch {i} stream {s} record {j}")
    assert any("instances" in r and len(r["instances"].gt_boxes) for b in runs[3] for r in b[0])
    assert all("instances" not in r for b in runs[3] for r in b[2])


def test_test_loader_records_are_those_of_the_serial_path(tmp_path):
    from probabilisticteacher_amd.data import build_detection_test_loader
    _datasets(tmp_path)
    ref = list(build_detection_test_loader(_cfg(tmp_path, 0), "lw_val", batch_size=2))
    got = list(build_detection_test_loader(_cfg(tmp_path, 3), "lw_val", batch_size=2))
    torch.cuda.synchronize()
    assert [len(b) for b in got] == [len(b) for b in ref] == [2, 2, 1]
    for i, (rb, gb) in enumerate(zip(ref, got)):
        for j, (r, g) in enumerate(zip(rb, gb)):
            _same_record(g, r, f"batch {i} record {j}")
            assert torch.equal(g["instances"].difficult, r["instances"].difficult)


def test_two_train_iterations_from_files_with_workers(tmp_path):
    from probabilisticteacher_amd.engine import PTrainer
    _datasets(tmp_path)
    cfg = _cfg(tmp_path, 3, "SOLVER.IMG_PER_BATCH_UNLABEL", 2)
    torch.manual_seed(0)
    loader = PTrainer.build_train_loader(cfg)
    tr = PTrainer(cfg, data_loader=loader)
    m = tr.train(max_iter=2, log_period=1, run_eval=False)      # burn-in, then EMA copy + mutual learning
    losses = {k: v for k, v in m.items() if k[:4] == "loss" or k == "total_loss"}
    assert "total_loss" in losses and len(losses) > 1 and all(np.isfinite(v) for v in losses.values()), m
    assert tr.iter == 2
    loader.close()
