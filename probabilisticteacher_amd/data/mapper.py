"""Two-crop mapper and aspect-ratio grouping with the pixel work on the device.

Reference: pt/data/dataset_mapper.py:88-172 `DatasetMapperTwoCropSeparate.__call__` -- weak augmentation (D2
[RandomCrop +] ResizeShortestEdge + RandomFlip, dataset_mapper.py:50-62) -> `image_weak_aug`; strong augmentation of a copy -> the record pair
(strong, weak) in the a0 record format ("image" uint8 (3,H,W), "instances" FreeInstances{gt_boxes, gt_classes}, height,
width); pt/data/common.py:106-180 `AspectRatioGroupedSemiSupDatasetTwoCrop`.

Scope: image decoding stays on the host side of the boundary (the mapper takes the decoded uint8 image); the weak
augmentation ([RandomCrop,] ResizeShortestEdge = Pillow's antialiased bilinear resize, RandomFlip), the four strong
augmentations and the batching run here, for a whole step's images at once."""
import random
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from ..structures import Boxes, FreeInstances
from .augment import (CROP_TYPES, FLIP_MODES, StrongParams, Window, crop_size_range, flip_batch, hflip_batch,
                      resize_batch, resize_shortest_edge_size, sample_crop, sample_short_edge, sample_strong_params,
                      strong_augment_batch)


def weak_box_transform(boxes: torch.Tensor, crop: Optional[Window], src_size: Tuple[int, int], new_size: Tuple[int, int],
                       flip_mode: int, min_box_side: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """The weak augmentation's box arithmetic in D2's order, on any device: CropTransform (x -= x0, y -= y0), ResizeTransform
    (scale by new / cropped size; without a crop the divisor is `src_size`), HFlipTransform (flip_mode 1) or VFlipTransform
    (2), the clip to the image of transform_instance_annotations and the filter_empty_instances mask.  boxes: (M, 4) xyxy.
    Returns (fp32 boxes, keep mask).  A box the crop removes has no area left after the clip and fails the mask."""
    h, w = new_size
    b = boxes.float().clone()
    sh, sw = src_size
    if crop is not None:
        y0, x0, sh, sw = crop
        b[:, 0::2] -= x0
        b[:, 1::2] -= y0
    b[:, 0::2] *= w * 1.0 / sw                   # ResizeTransform.apply_coords
    b[:, 1::2] *= h * 1.0 / sh
    if flip_mode == 1:                           # HFlipTransform.apply_coords: x -> w - x, then re-order
        x1 = w - b[:, 2]
        x2 = w - b[:, 0]
        b[:, 0], b[:, 2] = x1, x2
    elif flip_mode == 2:                         # VFlipTransform.apply_coords: y -> h - y, then re-order
        y1 = h - b[:, 3]
        y2 = h - b[:, 1]
        b[:, 1], b[:, 3] = y1, y2
    b[:, 0::2].clamp_(0, w)                      # transform_instance_annotations clips to the image
    b[:, 1::2].clamp_(0, h)
    keep = ((b[:, 2] - b[:, 0]) > min_box_side) & ((b[:, 3] - b[:, 1]) > min_box_side)   # filter_empty_instances
    return b, keep


class DeviceTwoCropMapper:
    """dataset dicts {"image": uint8 (3,H,W) tensor (any device), "boxes": (M,4) xyxy abs, "classes": (M,), "height",
    "width"} -> list of (strong record, weak record) pairs, as DatasetMapperTwoCropSeparate returns per image.

    Weak augmentation = D2 build_augmentation: [RandomCrop] + ResizeShortestEdge + RandomFlip.  The crop is a window the
    resize (or, when it already has the target size, the flip / copy) reads in place.

    Random stream (`self.rng`; the reference draws from numpy's global state, so only the distributions can agree).  One call
    draws, in this order: for image 0, 1, ...: [crop enabled: u0, u1 ("relative_range") or the integers ch, cw
    ("absolute_range"), then y0, then x0], then the short edge (one `choice` / `randint`; nothing when min_size_train is
    empty); then one `random()` per image for the flip; then `sample_strong_params` per image.  Whatever the caller passes
    explicitly (`crops`, `sizes`, `flips`, `params`) is not drawn.  Without a crop and with "choice" sampling this is the
    stream of the mapper before crops existed."""

    def __init__(self, device, flip_prob: float = 0.5, seed: Optional[int] = None, min_box_side: float = 1e-5,
                 min_size_train: Sequence[int] = (), max_size_train: int = 1333, *, crop: Optional[Tuple[str, Sequence[float]]] = None,
                 flip: str = "horizontal", min_size_sampling: str = "choice"):
        """min_size_train / max_size_train / min_size_sampling = cfg.INPUT.MIN_SIZE_TRAIN / MAX_SIZE_TRAIN /
        MIN_SIZE_TRAIN_SAMPLING; empty min_size_train: the images already have their training resolution.
        crop = (cfg.INPUT.CROP.TYPE, cfg.INPUT.CROP.SIZE) or None; flip = cfg.INPUT.RANDOM_FLIP, the direction of a flip."""
        self.device = torch.device(device)
        self.flip_prob = flip_prob
        self.rng = random.Random(seed)
        self.min_box_side = min_box_side
        self.min_size_train, self.max_size_train = tuple(min_size_train), max_size_train
        if flip not in FLIP_MODES:                   # D2 RandomFlip raises when neither direction is set
            raise ValueError(f"INPUT.RANDOM_FLIP {flip!r}: one of {tuple(FLIP_MODES)}")
        self.flip = flip
        if min_size_sampling not in ("choice", "range"):
            raise ValueError(f"Unknown INPUT.MIN_SIZE_TRAIN_SAMPLING {min_size_sampling!r} ('choice' or 'range')")
        if min_size_sampling == "range" and len(self.min_size_train) != 2:
            raise ValueError(f"INPUT.MIN_SIZE_TRAIN_SAMPLING 'range' needs exactly two sizes, got {self.min_size_train}")
        self.min_size_sampling = min_size_sampling
        if crop is not None:
            ctype, csize = crop[0], tuple(crop[1])
            if ctype not in CROP_TYPES:
                raise ValueError(f"Unknown crop type {ctype!r} (INPUT.CROP.TYPE is one of {CROP_TYPES})")
            if len(csize) != 2:
                raise ValueError(f"INPUT.CROP.SIZE needs two values, got {csize}")
            if ctype == "absolute_range":
                crop_size_range(csize, 1, 1)         # SIZE[0] <= SIZE[1]
            crop = (ctype, csize)
        self.crop = crop

    @property
    def flip_mode(self) -> int:
        """what a flipped image gets: 0 nothing, 1 left-right, 2 top-bottom"""
        return FLIP_MODES[self.flip]

    @classmethod
    def from_config(cls, cfg, seed: Optional[int] = None):
        flip = cfg.INPUT.RANDOM_FLIP
        crop = (cfg.INPUT.CROP.TYPE, tuple(cfg.INPUT.CROP.SIZE)) if cfg.INPUT.CROP.ENABLED else None
        return cls(cfg.MODEL.DEVICE, flip_prob=0.0 if flip == "none" else 0.5, seed=seed,
                   min_size_train=cfg.INPUT.MIN_SIZE_TRAIN, max_size_train=cfg.INPUT.MAX_SIZE_TRAIN, crop=crop, flip=flip,
                   min_size_sampling=cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING)

    def draw(self, shapes: Sequence[Tuple[int, int]], params=None, flips=None, sizes=None, crops=None):
        """The host half of a call: every random decision for images of the given (h, w), in the documented order.
        Returns (crops, sizes, flips, params); touches no device."""
        n = len(shapes)
        draw_crops, draw_sizes = crops is None and self.crop is not None, sizes is None
        crops = list(crops) if crops is not None else [None] * n
        sizes = list(sizes) if sizes is not None else [None] * n
        for i, (h, w) in enumerate(shapes):
            if draw_crops:
                crops[i] = sample_crop(self.crop[0], self.crop[1], h, w, self.rng)
            if draw_sizes:
                ch, cw = (h, w) if crops[i] is None else crops[i][2:]
                sizes[i] = (resize_shortest_edge_size(ch, cw, sample_short_edge(self.min_size_train, self.min_size_sampling, self.rng),
                                                      self.max_size_train) if self.min_size_train else (ch, cw))
        flips = list(flips) if flips is not None else [self.rng.random() < self.flip_prob for _ in range(n)]
        params = list(params) if params is not None else [sample_strong_params(self.rng) for _ in range(n)]
        return crops, sizes, flips, params

    def _weak(self, imgs, crops, sizes, modes) -> List[torch.Tensor]:
        """crop -> resize -> flip.  A crop goes to the resize as its source window; one that already has the target size
        goes to the flip / copy launch instead.  Without crops and vertical flips these are the two launches of old."""
        if all(c is None for c in crops):
            res = resize_batch(imgs, sizes)
            if 2 not in modes:
                return hflip_batch(res, [m == 1 for m in modes])
            return flip_batch(res, modes)
        resized = [c is not None and tuple(c[2:]) != tuple(sz) for c, sz in zip(crops, sizes)]
        res = resize_batch(imgs, [sz if (r or c is None) else tuple(im.shape[-2:]) for im, c, sz, r in zip(imgs, crops, sizes, resized)],
                           [c if r else None for c, r in zip(crops, resized)])
        return flip_batch(res, modes, [None if (r or c is None) else c for c, r in zip(crops, resized)])

    def __call__(self, dataset_dicts: Sequence[Dict], params: Optional[Sequence[StrongParams]] = None,
                 flips: Optional[Sequence[bool]] = None, sizes: Optional[Sequence[Tuple[int, int]]] = None,
                 crops: Optional[Sequence[Optional[Window]]] = None) -> List[Tuple[Dict, Dict]]:
        """flips[i]: flip image i in the mapper's direction; sizes[i] = (new_h, new_w); crops[i] = (y0, x0, ch, cw) or None"""
        imgs = [d["image"].to(self.device, non_blocking=True) for d in dataset_dicts]
        crops, sizes, flips, params = self.draw([tuple(im.shape[-2:]) for im in imgs], params, flips, sizes, crops)
        modes = [self.flip_mode if f else 0 for f in flips]
        weak = self._weak(imgs, crops, sizes, modes)          # [T.RandomCrop], T.ResizeShortestEdge, T.RandomFlip
        strong = strong_augment_batch(weak, params)
        out = []
        for d, src, w_img, s_img, mode, crop in zip(dataset_dicts, imgs, weak, strong, modes, crops):
            h, w = w_img.shape[-2:]
            inst = None
            if "boxes" in d:
                b, keep = weak_box_transform(d["boxes"].to(self.device), crop, tuple(src.shape[-2:]), (h, w), mode, self.min_box_side)
                inst = FreeInstances((h, w))
                inst.gt_boxes = Boxes(b[keep])
                inst.gt_classes = d["classes"].to(self.device)[keep]
            base = {k: v for k, v in d.items() if k not in ("image", "boxes", "classes")}
            rec_s, rec_w = dict(base, image=s_img, height=h, width=w), dict(base, image=w_img, height=h, width=w)
            if inst is not None:
                rec_s["instances"], rec_w["instances"] = inst, inst      # the key record is a deepcopy in the reference
            out.append((rec_s, rec_w))
        return out


class _Stream:
    """one of the two record streams: two aspect-ratio buckets of (strong, weak) pairs and the bucket being filled"""

    def __init__(self, batch_size: int):
        self.batch_size = batch_size
        self.buckets = ([], [])            # index 0: landscape (w > h), 1: portrait / square
        self.current = self.buckets[0]

    def offer(self, pair) -> None:
        if len(self.current) == self.batch_size:       # a full batch is waiting for the other stream: drop the pair
            return
        strong = pair[0]
        self.current = self.buckets[0 if strong["width"] > strong["height"] else 1]
        self.current.append(pair)

    def ready(self) -> bool:
        return len(self.current) == self.batch_size

    def take(self):
        strong, weak = [p[0] for p in self.current], [p[1] for p in self.current]
        del self.current[:]
        return strong, weak


class AspectRatioGroupedSemiSupDatasetTwoCrop:
    """pt/data/common.py:106-180 (same name, same iteration contract): consumes a labelled and an unlabelled stream of
    (strong, weak) record pairs in lock step and yields (label_strong, label_weak, unlabel_strong, unlabel_weak) whenever
    BOTH streams have a full bucket; images with w > h and w <= h never share a batch (less padding).  As in the
    reference, a stream whose batch is already full ignores its incoming pairs until the other one catches up."""

    def __init__(self, dataset: Tuple[Iterable, Iterable], batch_size: Tuple[int, int]):
        self.label_dataset, self.unlabel_dataset = dataset
        self.batch_size_label, self.batch_size_unlabel = batch_size

    def __iter__(self):
        lab, unl = _Stream(self.batch_size_label), _Stream(self.batch_size_unlabel)
        for pair_l, pair_u in zip(self.label_dataset, self.unlabel_dataset):
            lab.offer(pair_l)
            unl.offer(pair_u)
            if lab.ready() and unl.ready():
                ls, lw = lab.take()
                us, uw = unl.take()
                yield ls, lw, us, uw
