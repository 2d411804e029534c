"""The two-crop semi-supervised train loader and the test loader (reference pt/data/build.py:107-217, train_net.py:51-75).

Same structure as the reference -- an infinite, seeded, rank-sharded index stream per dataset (D2 TrainingSampler), the
two-crop mapper, aspect-ratio grouping of the labelled and the unlabelled stream in lock step, per-rank batch = total / world
(build.py:174-187) -- but the mapper is the device pipeline of data/mapper.py: the host only decodes the images.

cfg.DATALOADER.NUM_WORKERS (the reference's DataLoader worker processes, build.py:205-216) is the number of decode THREADS of
data/prefetch.py: 0 decodes and maps image by image on the consuming thread; n > 0 decodes ahead and maps a chunk of images
per call.  The record stream is the same for every value.

image_cache (data/cache.py, off by default): both loaders read a file that is resident on the device from there instead of
decoding it, and insert what they decode; the records are the same with and without it."""
import collections
import itertools
from typing import Iterable, Iterator, List, Optional

import torch
import torch.distributed as dist

from ..seeding import loader_seed
from ..structures import Boxes, FreeInstances
from . import datasets, prefetch
from .augment import resize_batch, resize_shortest_edge_size
from .mapper import AspectRatioGroupedSemiSupDatasetTwoCrop, DeviceTwoCropMapper


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def training_sampler(size: int, seed: int = 0, shuffle: bool = True) -> Iterator[int]:
    """D2 TrainingSampler: an infinite stream of indices -- a fresh seeded permutation per epoch, identical on all ranks --
    of which rank r takes elements r, r + world, r + 2 world, ..."""
    rank, world = _rank_world()

    def stream():
        g = torch.Generator().manual_seed(seed)
        while True:
            yield from (torch.randperm(size, generator=g) if shuffle else torch.arange(size)).tolist()
    return itertools.islice(stream(), rank, None, world)


def _cached_image(cache, file_name: str, fmt: str) -> torch.Tensor:
    """`datasets.read_image` on the cache's device through the cache (the serial path): a miss is decoded here and its
    host -> device copy -- the one the mapper would make -- is what the cache keeps"""
    key, img = cache.lookup(file_name, fmt == "BGR")
    if img is None:
        img = datasets.read_image(file_name, fmt).to(cache.device)
        cache.insert(key, img)
    return img


def _mapped_pairs(dicts: List[dict], sampler: Iterable[int], mapper: DeviceTwoCropMapper, fmt: str, labelled: bool,
                  image_cache=None):
    for i in sampler:
        img = None if image_cache is None else _cached_image(image_cache, dicts[i]["file_name"], fmt)
        d = datasets.to_mapper_input(dicts[i], fmt, image=img)
        if not labelled:                     # the unlabelled stream's annotations are never used (trainer.py:248-257)
            d = _drop_annotations(d)
        yield mapper([d])[0]


def _drop_annotations(d: dict) -> dict:
    return {k: v for k, v in d.items() if k not in ("boxes", "classes", "difficult")}


def _prefetched_pairs(label_dicts, unlabel_dicts, samp_l, samp_u, mapper, fmt: str, chunk: int, ahead_of):
    """The two `_mapped_pairs` streams with the decode on worker threads.  Returns (labelled stream, unlabelled stream,
    DecodeAhead).  The decodes are submitted in the order the lock-step zip consumes the streams (l0, u0, l1, u1, ...);
    `chunk` pairs at a time are unpacked with one launch and mapped with one mapper call per stream.  The mapper's one rng is
    drawn per image in that same interleaved order -- `mapper.draw` on this thread -- and the draws go to the batched call
    explicitly, so the records are those of the serial path."""
    def items():
        for il, iu in zip(samp_l, samp_u):
            yield label_dicts[il]
            yield unlabel_dicts[iu]
    ahead = ahead_of(items())
    queues = (collections.deque(), collections.deque())        # mapped pairs of the labelled / the unlabelled stream

    def fill():
        got = ahead.take_planar(2 * chunk, fmt == "BGR", multiple=2)
        inputs, draws = ([], []), ([], [])
        for k, (d, img) in enumerate(got):                     # k even: labelled, odd: unlabelled
            m = datasets.to_mapper_input(d, fmt, image=img)
            inputs[k % 2].append(m if k % 2 == 0 else _drop_annotations(m))
            draws[k % 2].append(mapper.draw([tuple(img.shape[-2:])]))
        for q, dd, dr in zip(queues, inputs, draws):
            crops, sizes, flips, params = ([x[j][0] for x in dr] for j in range(4))
            q.extend(mapper(dd, params=params, flips=flips, sizes=sizes, crops=crops))

    def stream(q):
        while True:
            if not q:
                fill()
            yield q.popleft()
    return stream(queues[0]), stream(queues[1]), ahead


def _closing(it, ahead):
    """`it`, and the decode threads stopped when the iterator is closed, dropped or fails"""
    try:
        yield from it
    finally:
        ahead.close()


def _decode_ahead(items, workers: int, in_flight: int, device, fmt: str, image_cache):
    if image_cache is None:
        return prefetch.DecodeAhead(items, lambda d: d["file_name"], workers, in_flight, device)
    return prefetch.DecodeAhead(items, lambda d: d["file_name"], workers, in_flight, device, cache=image_cache, bgr=fmt == "BGR")


def _check_cache_device(cfg, image_cache) -> None:
    if image_cache is None:
        return
    dev = torch.device(cfg.MODEL.DEVICE)
    if dev.type != image_cache.device.type or dev.index not in (None, image_cache.device.index):
        raise ValueError(f"image_cache is on {image_cache.device}, the loader works on MODEL.DEVICE {cfg.MODEL.DEVICE}")


def build_detection_semisup_train_loader_two_crops(cfg, mapper: Optional[DeviceTwoCropMapper] = None, seed: Optional[int] = None,
                                                   image_cache=None):
    """build.py:107-217: yields (label_strong, label_weak, unlabel_strong, unlabel_weak) lists of records forever.
    seed None: cfg.SEED when it is >= 0, else 0.  The index streams use the value itself on every rank (they are sharded by
    rank), the mapper adds its per-rank offset.  image_cache: a DeviceImageCache on MODEL.DEVICE, or None."""
    _check_cache_device(cfg, image_cache)
    rank, world = _rank_world()
    seed = loader_seed(cfg, seed)
    bl, bu = cfg.SOLVER.IMG_PER_BATCH_LABEL, cfg.SOLVER.IMG_PER_BATCH_UNLABEL
    assert bl > 0 and bl % world == 0, f"Total label batch size ({bl}) must be divisible by the number of gpus ({world})."
    assert bu > 0 and bu % world == 0, f"Total unlabel batch size ({bu}) must be divisible by the number of gpus ({world})."
    workers = prefetch.num_workers(cfg)
    label_dicts = datasets.get_dataset_dicts(cfg.DATASETS.TRAIN_LABEL, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)   # build.py:111
    unlabel_dicts = datasets.get_dataset_dicts(cfg.DATASETS.TRAIN_UNLABEL, filter_empty=False)
    mapper = mapper or DeviceTwoCropMapper.from_config(cfg, seed=seed + 17 * rank)
    fmt = cfg.INPUT.FORMAT
    samp_l, samp_u = training_sampler(len(label_dicts), seed), training_sampler(len(unlabel_dicts), seed + 1)
    bl, bu = bl // world, bu // world
    if workers == 0:
        lab = _mapped_pairs(label_dicts, samp_l, mapper, fmt, True, image_cache)
        unl = _mapped_pairs(unlabel_dicts, samp_u, mapper, fmt, False, image_cache)
        return iter(AspectRatioGroupedSemiSupDatasetTwoCrop((lab, unl), (bl, bu)))
    lab, unl, ahead = _prefetched_pairs(
        label_dicts, unlabel_dicts, samp_l, samp_u, mapper, fmt, min(bl, bu),
        lambda items: _decode_ahead(items, workers, prefetch.max_in_flight(bl + bu), cfg.MODEL.DEVICE, fmt, image_cache))
    return _closing(AspectRatioGroupedSemiSupDatasetTwoCrop((lab, unl), (bl, bu)), ahead)


def _test_record(cfg, d: dict, m: dict, dev, shared: bool = False) -> dict:
    """shared: m["image"] may live in an image cache, so the record must not be that tensor itself"""
    img = m["image"].to(dev)
    h, w = img.shape[-2:]
    nh, nw = resize_shortest_edge_size(h, w, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    out = resize_batch([img], [(nh, nw)])[0]
    if shared and out is img:                         # already at its test size: the resize hands its source back
        out = out.clone()
    rec = {"image": out, "height": h, "width": w, "image_id": d["image_id"], "file_name": d["file_name"]}
    if "boxes" in m:
        inst = FreeInstances((h, w))
        inst.gt_boxes, inst.gt_classes, inst.difficult = Boxes(m["boxes"]), m["classes"], m["difficult"]
        for k in ("iscrowd", "area"):                 # COCO-format datasets only (the COCO evaluator's dict-less path)
            if k in m:
                inst.set(k, m[k])
        rec["instances"] = inst
    return rec


def build_detection_test_loader(cfg, dataset_name: str, batch_size: int = 1, image_cache=None):
    """D2 build_detection_test_loader + DatasetMapper(is_train=False): ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST), no flip;
    records keep the ORIGINAL height / width (detector_postprocess scales the detections back) and carry the ground truth in
    original coordinates for the evaluator.  Rank r evaluates images r, r + world, ... (D2 InferenceSampler shards contiguously;
    the evaluator gathers the shards, so the split does not matter).  With DATALOADER.NUM_WORKERS > 0 the images are decoded
    ahead by that many threads (look-ahead: LOOKAHEAD_STEPS x max(batch_size, workers) images); the records are the same.
    image_cache: a DeviceImageCache on MODEL.DEVICE, or None; the one the train loader uses may be passed."""
    rank, world = _rank_world()
    _check_cache_device(cfg, image_cache)
    workers = prefetch.num_workers(cfg)
    dicts = datasets.get_dataset_dicts([dataset_name])
    dev = torch.device(cfg.MODEL.DEVICE)
    mine = dicts[rank::world]
    fmt = cfg.INPUT.FORMAT

    shared = image_cache is not None

    def serial():
        for s in range(0, len(mine), batch_size):
            yield [_test_record(cfg, d, datasets.to_mapper_input(
                d, fmt, image=_cached_image(image_cache, d["file_name"], fmt) if shared else None, is_train=False), dev, shared)
                for d in mine[s:s + batch_size]]

    def ahead_of_time():
        ahead = _decode_ahead(mine, workers, prefetch.max_in_flight(max(batch_size, workers)), dev, fmt, image_cache)
        try:
            while True:
                got = ahead.take_planar(batch_size, fmt == "BGR")
                if not got:
                    return
                yield [_test_record(cfg, d, datasets.to_mapper_input(d, fmt, image=img, is_train=False), dev, shared)
                       for d, img in got]
        finally:
            ahead.close()
    return serial() if workers == 0 else ahead_of_time()
