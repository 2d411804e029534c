"""Test-time augmentation: the TEST.AUG node of detectron2 0.5 (GeneralizedRCNNWithTTA / DatasetMapperTTA), box branch.

D2 is not a dependency of this project; like every other D2-owned primitive this restates the 0.5 release ("parity by
restatement, not by execution").  Per record: every TEST.AUG.MIN_SIZES entry resizes the loader's image once more
(ResizeShortestEdge arithmetic, Pillow-bilinear on the device), optionally also flipped; the model runs on each; every
augmentation's detections are mapped back to the original image and merged by one plain batched NMS per image
(ops.tta_merge: two HIP kernels around the existing segmented sort and NMS, one device->host read per batch).

One departure from D2, on purpose: D2 runs the augmented images three at a time and zero-pads a batch of mixed sizes, so its
result depends on that memory knob.  Here one call holds the two images of one size (unflipped, flipped): no padding enters."""
from typing import List, NamedTuple, Sequence, Tuple

import torch
from torch import nn

from .. import ops
from ..data.augment import _f32, hflip_batch, resize_batch, resize_shortest_edge_size
from ..structures import Boxes, Instances


class TTAAug(NamedTuple):
    """One augmentation of a record.  The factors are fp32 values (formed in double, rounded once): D2 multiplies float32
    numpy arrays by Python floats, which numpy rounds to fp32 first."""
    size: Tuple[int, int]       # (h_s, w_s) of the augmented image
    flip: bool
    fx: float                   # fp32(w / w_s): back to the loader image
    fy: float                   # fp32(h / h_s)
    gx: float                   # fp32(W / w): back to the original image (1.0 and unused without a pre-transform)
    gy: float                   # fp32(H / h)
    pre: bool                   # (h, w) != (H, W): D2's pre_tfm exists


def check_tta_options(cfg) -> Tuple[Tuple[int, ...], int, bool]:
    """Validate TEST.AUG.MIN_SIZES / MAX_SIZE / FLIP -> (min_sizes, max_size, flip).  A ValueError names the key."""
    aug = cfg.TEST.AUG

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    sizes = aug.MIN_SIZES
    if not isinstance(sizes, (tuple, list)) or len(sizes) == 0 or not all(is_int(s) and s > 0 for s in sizes):
        raise ValueError(f"TEST.AUG.MIN_SIZES must be a non-empty sequence of positive integers, got {sizes!r}")
    if not is_int(aug.MAX_SIZE) or aug.MAX_SIZE <= 0:
        raise ValueError(f"TEST.AUG.MAX_SIZE must be a positive integer, got {aug.MAX_SIZE!r}")
    if not isinstance(aug.FLIP, bool):
        raise ValueError(f"TEST.AUG.FLIP must be True or False, got {aug.FLIP!r}")
    return tuple(sizes), aug.MAX_SIZE, aug.FLIP


def tta_plan(h: int, w: int, H: int, W: int, min_sizes: Sequence[int], max_size: int, flip: bool) -> List[TTAAug]:
    """DatasetMapperTTA for a loader image of (h, w) whose original is (H, W): the augmentations in D2's order -- s0, s0 + flip,
    s1, s1 + flip, ... -- each with the factors that take its boxes back.  Host only."""
    pre = (h, w) != (H, W)
    gx, gy = (_f32(W / w), _f32(H / h)) if pre else (1.0, 1.0)
    plan = []
    for s in min_sizes:
        hs, ws = resize_shortest_edge_size(h, w, s, max_size)
        for f in ((False, True) if flip else (False,)):
            plan.append(TTAAug((hs, ws), f, _f32(w / ws), _f32(h / hs), gx, gy, pre))
    return plan


class GeneralizedRCNNWithTTA(nn.Module):
    """`GeneralizedRCNNWithTTA(cfg, model)(batch)` -> [{"instances": Instances}] like the model itself, each Instances of the
    record's original (height, width) with pred_boxes, scores and pred_classes (scores_logists / boxes_sigma do not survive a
    merge, and empty boxes are not filtered: D2's TTA does not call detector_postprocess).  Inference runs record by record,
    one call per size; all records of the batch are merged in one set of launches."""

    def __init__(self, cfg, model):
        super().__init__()
        self.min_sizes, self.max_size, self.flip = check_tta_options(cfg)
        self.model = model
        self.nms_thresh = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        self.max_det = int(cfg.TEST.DETECTIONS_PER_IMAGE)

    def augmented_inputs(self, image: torch.Tensor, plan: Sequence[TTAAug]) -> List[List[dict]]:
        """The model inputs of one record, one batch per size: the loader image resized (a second resampling, as in D2),
        then its mirror image if the plan has one."""
        sizes = [a.size for a in plan if not a.flip]
        resized = resize_batch([image] * len(sizes), sizes)
        flipped = hflip_batch(resized, [True] * len(resized)) if self.flip else []
        return [[{"image": r}] + ([{"image": flipped[i]}] if self.flip else []) for i, r in enumerate(resized)]

    @torch.no_grad()
    def forward(self, batched_inputs: List[dict]):
        assert not self.model.training, "test-time augmentation runs the model in eval mode"
        if not batched_inputs:
            return []
        rows, counts, sizes, boxes, scores, classes = [], [], [], [], [], []
        for i, rec in enumerate(batched_inputs):
            image = rec["image"].to(self.model.device, non_blocking=True)
            h, w = int(image.shape[-2]), int(image.shape[-1])
            H, W = int(rec.get("height", h)), int(rec.get("width", w))
            sizes.append((H, W))
            plan = tta_plan(h, w, H, W, self.min_sizes, self.max_size, self.flip)
            results = [r for batch in self.augmented_inputs(image, plan) for r in self.model.inference(batch, do_postprocess=False)]
            for a, res in zip(plan, results):
                rows.append((i, a.flip, a.size[1], a.fx, a.fy, a.gx, a.gy, a.pre))
                counts.append(len(res.scores))
                boxes.append(res.pred_boxes.tensor)
                scores.append(res.scores)
                classes.append(res.pred_classes)
        merged = ops.tta_merge(torch.cat(boxes), torch.cat(scores), torch.cat(classes), rows, counts, sizes, self.nms_thresh,
                               self.max_det)
        out = []
        for size, (b, s, c) in zip(sizes, merged):
            out.append({"instances": Instances(size, pred_boxes=Boxes(b), scores=s, pred_classes=c)})
        return out
