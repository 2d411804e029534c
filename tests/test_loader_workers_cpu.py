"""Host logic of DATALOADER.NUM_WORKERS (data/prefetch.py, data/build.py), no GPU: MODEL.DEVICE "cpu", a stub mapper with the
draw / __call__ signature of DeviceTwoCropMapper and a substituted `datasets.read_image_hwc`.

What is pinned here: the decodes really run in parallel; the mapper's rng is drawn per image in the order l0, u0, l1, u1, ...;
the batches do not depend on the number of workers or on which decode finishes first; the look-ahead is bounded by the named
constant; a decode error arrives at its sample with the file name; an abandoned iterator leaves no thread; bad values of the
key are rejected when the loader is built."""
import gc
import os
import random
import threading
import time

import numpy as np
import pytest
import torch

BL, BU = 2, 3


def _write_dataset(root, ids, sizes, rng):
    """VOC layout with PNG bytes under the .jpg names the reader expects (Pillow goes by content): image k is sizes[k] = (h, w)"""
    from PIL import Image
    for sub in ("JPEGImages", "Annotations", "ImageSets/Main"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for fid, (h, w) in zip(ids, sizes):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, "JPEGImages", fid + ".jpg"), format="PNG")
        open(os.path.join(root, "Annotations", fid + ".xml"), "w").write(
            f"<annotation><size><width>{w}</width><height>{h}</height><depth>3</depth></size><object><name>car</name>"
            f"<difficult>0</difficult><bndbox><xmin>2</xmin><ymin>3</ymin><xmax>{w - 1}</xmax><ymax>{h - 1}</ymax></bndbox></object>"
            "</annotation>")
    open(os.path.join(root, "ImageSets", "Main", "train.txt"), "w").write("\n".join(ids) + "\n")


@pytest.fixture
def files(tmp_path):
    """7 labelled + 5 unlabelled images, every one of its own size (so a shape names an image), landscape and portrait mixed"""
    from probabilisticteacher_amd.data import datasets
    rng = np.random.RandomState(11)
    lab = [(10 + k, 24 + k) if k % 3 else (24 + k, 10 + k) for k in range(7)]
    unl = [(40 + k, 60 + k) if k % 2 else (60 + k, 40 + k) for k in range(5)]
    _write_dataset(str(tmp_path / "lab"), [f"L{k}" for k in range(7)], lab, rng)
    _write_dataset(str(tmp_path / "unl"), [f"U{k}" for k in range(5)], unl, rng)
    datasets.register_pascal_voc("w_lab", str(tmp_path / "lab"), "train", ("car",))
    datasets.register_pascal_voc("w_unl", str(tmp_path / "unl"), "train", ("car",))
    return lab, unl


def _cfg(workers, bl=BL, bu=BU):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg("configs/pt/final_s2c.yaml", [
        "MODEL.DEVICE", "cpu", "SOLVER.IMG_PER_BATCH_LABEL", bl, "SOLVER.IMG_PER_BATCH_UNLABEL", bu,
        "DATASETS.TRAIN_LABEL", ("w_lab",), "DATASETS.TRAIN_UNLABEL", ("w_unl",), "DATASETS.TEST", ("w_lab",),
        "DATALOADER.NUM_WORKERS", workers])


class StubMapper:
    """DeviceTwoCropMapper's interface on the host: draw() consumes the one rng per image, __call__ takes explicit draws"""

    def __init__(self, seed=3):
        self.rng = random.Random(seed)
        self.drawn = []            # the shapes draw() really drew for, in order
        self.calls = []            # the batch size of every __call__

    def draw(self, shapes, params=None, flips=None, sizes=None, crops=None):
        n = len(shapes)
        crops = list(crops) if crops is not None else [None] * n
        sizes = list(sizes) if sizes is not None else [(h + self.rng.randint(0, 3), w) for h, w in shapes]
        if flips is None:
            self.drawn += [tuple(s) for s in shapes]
            flips = [self.rng.random() < 0.5 for _ in range(n)]
        params = list(params) if params is not None else [self.rng.randint(1, 200) for _ in range(n)]
        return crops, sizes, list(flips), params

    def __call__(self, dataset_dicts, params=None, flips=None, sizes=None, crops=None):
        self.calls.append(len(dataset_dicts))
        imgs = [d["image"] for d in dataset_dicts]
        crops, sizes, flips, params = self.draw([tuple(im.shape[-2:]) for im in imgs], params, flips, sizes, crops)
        out = []
        for d, im, f, p, sz in zip(dataset_dicts, imgs, flips, params, sizes):
            weak = im.flip(-1) if f else im.clone()
            strong = weak + p
            base = {k: v for k, v in d.items() if k != "image"}
            h, w = im.shape[-2:]
            out.append((dict(base, image=strong, height=h, width=w, size=sz), dict(base, image=weak, height=h, width=w, size=sz)))
        return out


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _batches(workers, n, mapper=None, seed=5):
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops
    mapper = mapper or StubMapper()
    loader = build_detection_semisup_train_loader_two_crops(_cfg(workers), mapper=mapper, seed=seed)
    try:
        return [next(loader) for _ in range(n)], mapper
    finally:
        loader.close()


def _decode_threads():
    from probabilisticteacher_amd.data import prefetch
    return [t for t in threading.enumerate() if t.name.startswith(prefetch.THREAD_NAME) and t.is_alive()]


def test_two_workers_decode_at_the_same_time(files, monkeypatch):
    """the first two decodes meet at a barrier: only two threads inside read_image_hwc at once get past it"""
    from probabilisticteacher_amd.data import datasets
    real = getattr(datasets, "read_image_hwc", None)
    barrier, lock, seen = threading.Barrier(2, timeout=20.0), threading.Lock(), []

    def decode(file_name):
        with lock:
            seen.append(file_name)
            first_two = len(seen) <= 2
        if first_two:
            barrier.wait()
        return real(file_name)
    monkeypatch.setattr(datasets, "read_image_hwc", decode, raising=False)
    got, _ = _batches(2, 1)
    assert len(got[0]) == 4 and len(got[0][0]) == BL and len(got[0][2]) == BU
    assert len(seen) >= 2 and not barrier.broken, "the decodes went through read_image_hwc, two at a time"


def test_draw_order_is_interleaved_and_batches_do_not_depend_on_workers(files, monkeypatch):
    from probabilisticteacher_amd.data import datasets, training_sampler
    lab, unl = files
    real = datasets.read_image_hwc
    ref, m0 = _batches(0, 6)
    assert set(m0.calls) == {1}, "NUM_WORKERS 0 maps image by image"
    sl, su = training_sampler(len(lab), 5), training_sampler(len(unl), 6)
    want = []
    for _ in range(len(m0.drawn) // 2):
        want += [lab[next(sl)], unl[next(su)]]
    assert m0.drawn == want, "serial path: l0, u0, l1, u1, ..."
    for workers, delay_seed in ((1, 0), (5, 1), (5, 2)):
        delays = random.Random(delay_seed)
        lock = threading.Lock()

        def decode(file_name):
            with lock:
                d = delays.choice((0.0, 0.002, 0.01, 0.03))
            time.sleep(d)                                   # later submissions overtake earlier ones
            return real(file_name)
        monkeypatch.setattr(datasets, "read_image_hwc", decode)
        got, m = _batches(workers, 6)
        assert m.drawn[:len(want)] == want, f"{workers} workers: one draw per image, in the serial order"
        assert len(m.drawn) % 2 == 0 and len(set(m.calls)) >= 1 and max(m.calls) == min(BL, BU), "mapped in chunks"
        assert _same(got, ref), f"{workers} workers: the batches of the serial path"


def test_look_ahead_is_bounded(files, monkeypatch):
    from probabilisticteacher_amd.data import datasets, prefetch
    real = datasets.read_image_hwc
    lock, state = threading.Lock(), {"running": 0, "max_running": 0}

    def decode(file_name):
        with lock:
            state["running"] += 1
            state["max_running"] = max(state["max_running"], state["running"])
        time.sleep(0.002)
        try:
            return real(file_name)
        finally:
            with lock:
                state["running"] -= 1
    monkeypatch.setattr(datasets, "read_image_hwc", decode)
    made, Real = [], prefetch.DecodeAhead

    class Watched(Real):
        def __init__(self, items, file_of, workers, in_flight, device):
            super().__init__(items, file_of, workers, in_flight, device)
            self.bound, self.most = in_flight, 0
            made.append(self)

        def _top_up(self):
            super()._top_up()
            self.most = max(self.most, len(self._pending) + self._held)
    monkeypatch.setattr(prefetch, "DecodeAhead", Watched)
    _batches(4, 8)
    assert prefetch.LOOKAHEAD_STEPS == 2 and len(made) == 1
    assert made[0].bound == prefetch.max_in_flight(BL + BU) == prefetch.LOOKAHEAD_STEPS * (BL + BU)
    assert 0 < made[0].most <= made[0].bound, "submitted and not yet handed back"
    assert state["max_running"] <= 4, "no more decodes at once than workers"

    # the object itself, with a slow consumer: what has started decoding and was not handed back stays within the bound
    started, handed, worst = [], [0], [0]

    def counting(file_name):
        with lock:
            started.append(file_name)
            worst[0] = max(worst[0], len(started) - handed[0])
        return real(file_name)
    monkeypatch.setattr(datasets, "read_image_hwc", counting)

    class Counted(Real):
        def release(self, tickets):
            with lock:
                handed[0] += len(tickets)
            super().release(tickets)
    names = [d["file_name"] for d in datasets.get_dataset_dicts(["w_lab"])] * 6
    ahead = Counted(names, lambda f: f, 4, prefetch.max_in_flight(3), "cpu")
    out = []
    while True:
        time.sleep(0.01)
        got = ahead.take_planar(3, True)
        if not got:
            break
        assert all(torch.equal(img, datasets.read_image(f)) for f, img in got)
        out += [f for f, _ in got]
    ahead.close()
    assert out == names and len(started) == len(names)
    assert 0 < worst[0] <= prefetch.max_in_flight(3) == 6


def test_decode_error_arrives_at_its_sample(files, monkeypatch):
    from probabilisticteacher_amd.data import datasets, training_sampler
    lab, _ = files
    order = [next(s) for s in [training_sampler(len(lab), 5)] for _ in range(12)]
    bad = f"L{order[7]}.jpg"                                  # first met as the 8th labelled sample (or earlier)
    real_hwc, real = datasets.read_image_hwc, datasets.read_image

    def failing(fn):
        def f(file_name, *a):
            if file_name.endswith(bad):
                raise OSError("truncated file")
            return fn(file_name, *a)
        return f
    monkeypatch.setattr(datasets, "read_image_hwc", failing(real_hwc))
    monkeypatch.setattr(datasets, "read_image", failing(real))

    def run(workers):
        from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops
        loader = build_detection_semisup_train_loader_two_crops(_cfg(workers), mapper=StubMapper(), seed=5)
        got = []
        with pytest.raises((OSError, RuntimeError)) as e:
            for _ in range(50):
                got.append(next(loader))
        return got, e.value
    ref, _ = run(0)
    got, err = run(3)
    assert bad in str(err) and "truncated file" in str(err)
    assert len(got) == len(ref) and _same(got, ref), "every batch in front of the bad sample still comes out"
    assert not _decode_threads(), "the pool is closed after the error"


def test_abandoned_iterator_leaves_no_thread(files, monkeypatch):
    from probabilisticteacher_amd.data import build as build_mod, build_detection_semisup_train_loader_two_crops, build_detection_test_loader
    monkeypatch.setattr(build_mod, "resize_batch", lambda imgs, sizes: [im.clone() for im in imgs])     # the device resize
    assert not _decode_threads()
    loader = build_detection_semisup_train_loader_two_crops(_cfg(3), mapper=StubMapper(), seed=5)
    next(loader)
    live = _decode_threads()
    assert len(live) == 3 and all(t.daemon for t in live), "NUM_WORKERS daemon threads"
    loader.close()
    assert not _decode_threads(), "close() stops the workers"
    loader = build_detection_semisup_train_loader_two_crops(_cfg(2), mapper=StubMapper(), seed=5)
    next(loader)
    assert len(_decode_threads()) == 2
    del loader
    gc.collect()
    assert not _decode_threads(), "dropping the iterator stops the workers"
    loader = build_detection_semisup_train_loader_two_crops(_cfg(2), mapper=StubMapper(), seed=5)
    with pytest.raises(ZeroDivisionError):
        for i, _ in enumerate(loader):
            1 // (1 - i)                                     # the train loop fails in its second iteration
    del loader
    gc.collect()
    assert not _decode_threads(), "a failed train loop does not keep them either"
    test = build_detection_test_loader(_cfg(2), "w_lab")
    next(test)
    assert len(_decode_threads()) == 2
    test.close()
    assert not _decode_threads()


def test_test_loader_records_do_not_depend_on_workers(files, monkeypatch):
    from probabilisticteacher_amd.data import build as build_mod, build_detection_test_loader
    monkeypatch.setattr(build_mod, "resize_batch", lambda imgs, sizes: [im.clone() for im in imgs])     # the device resize
    ref = list(build_detection_test_loader(_cfg(0), "w_lab", batch_size=2))
    assert [len(b) for b in ref] == [2, 2, 2, 1] and [r["image_id"] for b in ref for r in b] == [f"L{k}" for k in range(7)]
    for workers in (1, 4):
        got = list(build_detection_test_loader(_cfg(workers), "w_lab", batch_size=2))
        assert len(got) == len(ref)
        for bg, br in zip(got, ref):
            for g, r in zip(bg, br):
                assert g.keys() == r.keys() and torch.equal(g["image"], r["image"])
                assert all(g[k] == r[k] for k in ("height", "width", "image_id", "file_name"))
                assert torch.equal(g["instances"].gt_boxes.tensor, r["instances"].gt_boxes.tensor)
                assert torch.equal(g["instances"].gt_classes, r["instances"].gt_classes)
    assert not _decode_threads()


@pytest.mark.parametrize("value", [-1, 2.5, "4", None])
def test_bad_worker_count_is_rejected_when_the_loader_is_built(files, value):
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops, build_detection_test_loader
    cfg = _cfg(0)
    cfg.defrost()
    cfg.DATALOADER.NUM_WORKERS = value
    with pytest.raises(ValueError, match="DATALOADER.NUM_WORKERS"):
        build_detection_semisup_train_loader_two_crops(cfg, mapper=StubMapper())
    with pytest.raises(ValueError, match="DATALOADER.NUM_WORKERS"):
        build_detection_test_loader(cfg, "w_lab")
