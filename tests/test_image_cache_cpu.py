"""Host logic of the device image cache (data/cache.py) and of the loaders that use it, no GPU: MODEL.DEVICE "cpu", the stub
mapper of tests/test_loader_workers_cpu.py and a substituted decoder.

What is pinned here: the budget is never exceeded and nothing is evicted; a rewritten file is decoded afresh; with a cache the
loaders deliver the records of the cache-off run in the same order whatever is resident and whichever decode finishes first;
only misses are decoded; a decode error still arrives at its sample; a second serial pass decodes nothing."""
import os
import random
import threading
import time

import numpy as np
import pytest
import torch

from tests.test_loader_workers_cpu import StubMapper, _cfg, _decode_threads, _same, _write_dataset


@pytest.fixture
def files(tmp_path):
    """7 labelled + 5 unlabelled images, every one of its own size, landscape and portrait mixed"""
    from probabilisticteacher_amd.data import datasets
    rng = np.random.RandomState(11)
    lab = [(10 + k, 24 + k) if k % 3 else (24 + k, 10 + k) for k in range(7)]
    unl = [(40 + k, 60 + k) if k % 2 else (60 + k, 40 + k) for k in range(5)]
    _write_dataset(str(tmp_path / "lab"), [f"L{k}" for k in range(7)], lab, rng)
    _write_dataset(str(tmp_path / "unl"), [f"U{k}" for k in range(5)], unl, rng)
    datasets.register_pascal_voc("w_lab", str(tmp_path / "lab"), "train", ("car",))
    datasets.register_pascal_voc("w_unl", str(tmp_path / "unl"), "train", ("car",))
    return lab, unl


def _names(dataset):
    from probabilisticteacher_amd.data import datasets
    return [d["file_name"] for d in datasets.get_dataset_dicts([dataset])]


def _count_decodes(monkeypatch, delays_seed=None, fail=None):
    """substitute both decoders by counting ones; delays_seed: shuffled decode delays; fail: a file-name suffix that raises"""
    from probabilisticteacher_amd.data import datasets
    real_hwc, real = datasets.read_image_hwc, datasets.read_image
    lock, seen = threading.Lock(), []
    delays = random.Random(delays_seed)

    def wrap(fn):
        def f(file_name, *a):
            with lock:
                seen.append(file_name)
                d = delays.choice((0.0, 0.002, 0.01, 0.03)) if delays_seed is not None else 0.0
            time.sleep(d)
            if fail is not None and file_name.endswith(fail):
                raise OSError("truncated file")
            return fn(file_name, *a)
        return f
    monkeypatch.setattr(datasets, "read_image_hwc", wrap(real_hwc))
    monkeypatch.setattr(datasets, "read_image", wrap(real))
    return seen


def _drain(names, cache, workers=3, n=3, bgr=True, in_flight=6):
    from probabilisticteacher_amd.data import prefetch
    kw = {} if cache is None else {"cache": cache, "bgr": bgr}
    ahead = prefetch.DecodeAhead(names, lambda f: f, workers, in_flight, "cpu", **kw)
    out = []
    try:
        while True:
            got = ahead.take_planar(n, bgr)
            if not got:
                return out
            out += got
    finally:
        ahead.close()


def test_budget_fits_two_of_five_and_is_never_exceeded(tmp_path, monkeypatch):
    from probabilisticteacher_amd.data import datasets, prefetch
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    rng = np.random.RandomState(3)
    _write_dataset(str(tmp_path / "five"), [f"F{k}" for k in range(5)], [(9, 13)] * 5, rng)
    names = [str(tmp_path / "five" / "JPEGImages" / f"F{k}.jpg") for k in range(5)]
    one = 3 * 9 * 13
    cache = DeviceImageCache(2 * one, "cpu")
    seen = _count_decodes(monkeypatch)
    ahead = prefetch.DecodeAhead(names * 2, lambda f: f, 2, 4, "cpu", cache=cache, bgr=True)
    out = []
    while True:
        got = ahead.take_planar(1, True)
        assert cache.bytes_used <= cache.budget_bytes
        if not got:
            break
        out += got
    ahead.close()
    assert len(cache) == 2 and cache.bytes_used == 2 * one == cache.budget_bytes
    assert sorted(k[0] for k, _ in cache.items()) == [os.path.realpath(f) for f in names[:2]], "the first two that were inserted"
    assert [f for f, _ in out] == names * 2
    monkeypatch.undo()
    assert all(torch.equal(img, datasets.read_image(f)) for f, img in out)
    assert cache.hits + cache.misses == 10 and cache.misses == len(seen), "every miss was decoded, nothing else was"
    # F0 and F1 are inserted when they are taken, so their second reading hits unless it was submitted before that: with four
    # in flight, submission 5 (F0 again) follows the first take
    assert cache.hits == 2 and len(seen) == 8
    for k, img in cache.items():
        assert img.dtype == torch.uint8 and tuple(img.shape) == (3, 9, 13) and k[3] is True
    # what does not fit is refused, what is wrong is an error, and the state is inspectable
    assert cache.insert(("x", 1, 1, True), torch.zeros((3, 1, 1), dtype=torch.uint8)) is False
    assert len(cache) == 2 and cache.bytes_used == 2 * one
    big = DeviceImageCache(10 ** 6, "cpu")
    with pytest.raises(ValueError):
        big.insert(("x", 1, 1, True), torch.zeros((3, 2, 2), dtype=torch.float32))
    with pytest.raises(ValueError):
        big.insert(("x", 1, 1, True), torch.zeros((2, 2, 3), dtype=torch.uint8))
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            DeviceImageCache(bad, "cpu")
    assert (big.bytes_used, big.hits, big.misses, len(big)) == (0, 0, 0, 0)


def test_a_budget_of_zero_caches_nothing(files, monkeypatch):
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    names = _names("w_lab")
    cache = DeviceImageCache(0, "cpu")
    seen = _count_decodes(monkeypatch)
    ref = _drain(names, None)
    assert _same([i for _, i in _drain(names, cache)], [i for _, i in ref])
    assert _same([i for _, i in _drain(names, cache)], [i for _, i in ref])
    assert len(seen) == 3 * len(names) and len(cache) == 0 and cache.bytes_used == 0 and cache.misses == 2 * len(names)


def test_rewritten_file_is_a_miss_and_is_decoded_afresh(tmp_path, monkeypatch):
    from PIL import Image
    from probabilisticteacher_amd.data import datasets
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    rng = np.random.RandomState(5)
    _write_dataset(str(tmp_path / "d"), ["A", "B"], [(8, 12), (7, 9)], rng)
    a, b = (str(tmp_path / "d" / "JPEGImages" / f"{n}.jpg") for n in "AB")
    cache = DeviceImageCache(10 ** 6, "cpu")
    seen = _count_decodes(monkeypatch)
    first = _drain([a, b], cache)
    assert len(seen) == 2 and len(cache) == 2
    again = _drain([a, b], cache)
    assert len(seen) == 2 and cache.hits == 2, "unchanged files are hits"
    assert all(x is y for (_, x), (_, y) in zip(first, again)), "a hit is the resident tensor itself"
    # same size, new mtime: raw 8-bit RGB rows of the same shape compress to the same length only by accident, so write the
    # same pixels again and move the mtime
    st = os.stat(a)
    os.utime(a, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000))
    assert os.stat(a).st_size == st.st_size
    got = _drain([a, b], cache)
    assert [f for f in seen[2:]] == [a], "a new mtime alone invalidates; B is still a hit"
    assert got[0][1] is not first[0][1] and torch.equal(got[0][1], first[0][1])
    # new content and size
    Image.fromarray(rng.randint(0, 256, (5, 6, 3)).astype(np.uint8)).save(b, format="PNG")
    got = _drain([a, b], cache)
    assert seen[3:] == [b] and tuple(got[1][1].shape) == (3, 5, 6)
    monkeypatch.undo()
    assert torch.equal(got[1][1], datasets.read_image(b)) and not torch.equal(got[1][1][:, :5, :6], first[1][1][:, :5, :6])
    assert len(cache) == 4, "insert-only: the stale entries stay"
    # a symbolic link names the same entry; the other channel order is another one
    link = str(tmp_path / "link.jpg")
    os.symlink(a, link)
    hits = cache.hits
    assert _drain([link], cache)[0][1] is got[0][1] and cache.hits == hits + 1
    rgb = _drain([a], cache, bgr=False)[0][1]
    assert torch.equal(rgb, got[0][1].flip(0)) and len(cache) == 5
    # a file that is not there is a miss whose decode reports it
    with pytest.raises(RuntimeError, match="nowhere"):
        _drain([a, str(tmp_path / "nowhere.jpg")], cache, n=1)


def _train_batches(workers, n, cache, seed=5):
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops
    mapper = StubMapper()
    loader = build_detection_semisup_train_loader_two_crops(_cfg(workers), mapper=mapper, seed=seed, image_cache=cache)
    try:
        return [next(loader) for _ in range(n)], mapper
    finally:
        loader.close()


def test_order_with_mixed_hits_and_misses_is_the_cache_off_order(files, monkeypatch):
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    lab, unl = files
    ref, m0 = _train_batches(0, 8, None)
    ref5, _ = _train_batches(5, 8, None)
    assert _same(ref5, ref)
    sizes = sorted(3 * h * w for h, w in lab + unl)
    for budget, delay_seed in ((10 ** 7, 0), (sum(sizes[:6]), 1), (sizes[-1] + sizes[0], 2)):
        cache = DeviceImageCache(budget, "cpu")
        for rounds in range(2):                                  # the second loader starts with what the first one left
            seen = _count_decodes(monkeypatch, delays_seed=delay_seed + 10 * rounds)
            hits, misses = cache.hits, cache.misses
            got, m = _train_batches(5, 8, cache)
            monkeypatch.undo()
            assert m.drawn[:len(m0.drawn)] == m0.drawn, "one draw per image, in the serial order"
            assert _same(got, ref), f"budget {budget}, loader {rounds}: the batches of the cache-off run"
            assert cache.bytes_used <= budget
            # a miss that was submitted is decoded unless the loader was closed first: never more decodes than misses
            assert len(seen) <= cache.misses - misses
            assert (len(seen) == 0) == (budget == 10 ** 7 and rounds == 1), "only the full cache saves every decode"
            assert cache.hits > hits, "and some images came from the cache"
        assert len(cache) == 12 if budget == 10 ** 7 else 0 < len(cache) < 12
    assert not _decode_threads()


def test_decode_count_is_the_miss_count(files, monkeypatch):
    """a finite list through DecodeAhead, so that every submission is consumed: some files resident, some not, some twice"""
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    names = _names("w_lab") + _names("w_unl")
    order = random.Random(4).sample(names * 3, 36)
    ref = _drain(order, None, workers=4, n=5, in_flight=10)
    cache = DeviceImageCache(10 ** 7, "cpu")
    _drain(names[::2], cache)                                    # every second file is resident
    assert len(cache) == 6
    seen = _count_decodes(monkeypatch, delays_seed=7)
    hits, misses = cache.hits, cache.misses
    got = _drain(order, cache, workers=4, n=5, in_flight=10)
    assert [f for f, _ in got] == order and _same([i for _, i in got], [i for _, i in ref])
    assert len(seen) == cache.misses - misses and cache.hits - hits == len(order) - len(seen)
    assert not set(seen) & set(names[::2]), "a resident file is not decoded"
    assert len(cache) == 12
    del seen[:]
    assert _same([i for _, i in _drain(order, cache, workers=4, n=5, in_flight=10)], [i for _, i in ref]) and not seen


def test_decode_error_still_arrives_at_its_sample(files, monkeypatch):
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops, training_sampler
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    lab, _ = files
    order = [next(s) for s in [training_sampler(len(lab), 5)] for _ in range(12)]
    bad = f"L{order[7]}.jpg"
    good = [f for f in _names("w_lab") + _names("w_unl") if not f.endswith(bad)]

    def run(workers, cache):
        loader = build_detection_semisup_train_loader_two_crops(_cfg(workers), mapper=StubMapper(), seed=5, image_cache=cache)
        got = []
        with pytest.raises((OSError, RuntimeError)) as e:
            for _ in range(50):
                got.append(next(loader))
        return got, e.value

    full, half = DeviceImageCache(10 ** 7, "cpu"), DeviceImageCache(10 ** 7, "cpu")
    _drain(good, full)                                           # everything but the bad file is resident
    _drain(good[::2], half)
    _count_decodes(monkeypatch, delays_seed=3, fail=bad)
    ref, _ = run(0, None)
    for workers, cache in ((3, full), (3, half), (0, half), (3, DeviceImageCache(10 ** 7, "cpu"))):
        got, err = run(workers, cache)
        assert "truncated file" in str(err) and (bad in str(err) or workers == 0), "the decode pool adds the file name"
        assert len(got) == len(ref) and _same(got, ref), "every batch in front of the bad sample still comes out"
        assert not any(k[0].endswith(bad) for k, _ in cache.items())
    assert not _decode_threads(), "the pool is closed after the error"


def test_serial_second_pass_decodes_nothing(files, monkeypatch):
    from probabilisticteacher_amd.data import build as build_mod, build_detection_test_loader
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    ref, _ = _train_batches(0, 8, None)
    cache = DeviceImageCache(10 ** 7, "cpu")
    seen = _count_decodes(monkeypatch)
    first, _ = _train_batches(0, 8, cache)
    assert sorted(set(seen)) == sorted(_names("w_lab") + _names("w_unl")) and len(seen) == 12 == len(cache), "each file once"
    del seen[:]
    second, _ = _train_batches(0, 8, cache)
    assert not seen, "NUM_WORKERS 0: the second pass calls the decoder zero times"
    assert _same(first, ref) and _same(second, ref)
    assert not _decode_threads(), "and starts no thread"

    # the test loader shares the cache: the labelled files are resident already.  The stand-in resize returns its SOURCE, as
    # the device resize does for an image that has its test size: the record must still not be the cached tensor
    monkeypatch.setattr(build_mod, "resize_batch", lambda imgs, sizes: list(imgs))
    resident = {id(img) for _, img in cache.items()}
    plain = list(build_detection_test_loader(_cfg(0), "w_lab", batch_size=2))
    del seen[:]
    for workers in (0, 2):
        got = list(build_detection_test_loader(_cfg(workers), "w_lab", batch_size=2, image_cache=cache))
        assert not seen, f"NUM_WORKERS {workers}: evaluation after training decodes nothing"
        assert [len(b) for b in got] == [2, 2, 2, 1]
        for bg, bp in zip(got, plain):
            for g, p in zip(bg, bp):
                assert g.keys() == p.keys() and torch.equal(g["image"], p["image"]) and id(g["image"]) not in resident
                assert all(g[k] == p[k] for k in ("height", "width", "image_id", "file_name"))
                assert torch.equal(g["instances"].gt_boxes.tensor, p["instances"].gt_boxes.tensor)
                g["image"].zero_()                               # a consumer that writes to its record harms nobody
    for (path, _, _, bgr), img in cache.items():
        assert torch.equal(img, build_mod.datasets.read_image(path, "BGR" if bgr else "RGB")), "cached tensors were not written to"


def test_cache_on_another_device_is_rejected(files):
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops, build_detection_test_loader

    class Elsewhere:
        device = torch.device("meta")
    with pytest.raises(ValueError, match="image_cache"):
        build_detection_semisup_train_loader_two_crops(_cfg(2), mapper=StubMapper(), image_cache=Elsewhere())
    with pytest.raises(ValueError, match="image_cache"):
        build_detection_test_loader(_cfg(0), "w_lab", image_cache=Elsewhere())


def test_trainer_loaders_pass_the_class_cache_on(files, monkeypatch):
    from probabilisticteacher_amd.data import build as build_mod
    from probabilisticteacher_amd.data.cache import DeviceImageCache
    from probabilisticteacher_amd.engine import PTrainer
    assert PTrainer.image_cache is None, "off unless asked for"
    monkeypatch.setattr(build_mod, "resize_batch", lambda imgs, sizes: [im.clone() for im in imgs])
    cache = DeviceImageCache(10 ** 7, "cpu")
    monkeypatch.setattr(PTrainer, "image_cache", cache)
    seen = _count_decodes(monkeypatch)
    assert len(list(PTrainer.build_test_loader(_cfg(2), "w_lab"))) == 7 and len(seen) == 7 == len(cache)
    assert len(list(PTrainer.build_test_loader(_cfg(2), "w_lab"))) == 7 and len(seen) == 7, "the teacher's pass decodes nothing"
    assert cache.hits == 7
    import probabilisticteacher_amd.data as data_pkg
    passed = []
    monkeypatch.setattr(data_pkg, "build_detection_semisup_train_loader_two_crops", lambda cfg, **kw: passed.append(kw))
    PTrainer.build_train_loader(_cfg(2))
    assert passed == [{"image_cache": cache}]
