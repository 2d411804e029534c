"""Meta-architecture: three-branch Gaussian Faster R-CNN (reference pt/modeling/meta_arch/rcnn.py:30-92) and the
teacher/student holder (pt/modeling/meta_arch/ts_ensemble.py:20-29)."""
from typing import List

import torch
from torch import nn

from .. import ops
from ..registry import META_ARCH_REGISTRY
from ..structures import ImageList
from .backbone import build_backbone
from .roi_heads import build_roi_heads
from .rpn import build_proposal_generator
from .statistics import StatisticsSink


@META_ARCH_REGISTRY.register()
class GuassianGeneralizedRCNN(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.backbone = build_backbone(cfg)
        self.proposal_generator = build_proposal_generator(cfg, self.backbone.output_shape())
        self.roi_heads = build_roi_heads(cfg, self.backbone.output_shape())
        self.input_format = cfg.INPUT.FORMAT
        self.register_buffer("pixel_mean", torch.tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1), False)
        self._mean = [float(v) for v in cfg.MODEL.PIXEL_MEAN]
        self._std = [float(v) for v in cfg.MODEL.PIXEL_STD]
        self.statistics = None
        self._frame_colours = {}

    def enable_statistics(self) -> StatisticsSink:
        """Count what the reference logs beside its losses (modeling/statistics.py): ONE sink, owned here and handed to the
        modules that count -- the RPN, the ROI head and its predictor.  Without this call their `statistics` stays None and they
        launch nothing."""
        self.statistics = StatisticsSink()
        for m in (self.proposal_generator, self.roi_heads, getattr(self.roi_heads, "box_predictor", None)):
            if m is not None:
                m.statistics = self.statistics
        return self.statistics

    @property
    def device(self):
        return self.pixel_mean.device

    def preprocess_image(self, batched_inputs: List[dict]) -> ImageList:
        """D2 GeneralizedRCNN.preprocess_image: normalise, then zero-pad to the batch max."""
        imgs = [x["image"].to(self.device, non_blocking=True) for x in batched_inputs]
        sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in imgs]
        return ImageList(ops.preprocess_images(imgs, self._mean, self._std), sizes)

    def frame_state(self, batched_inputs: List[dict], images: ImageList):
        """The ops.FrameState of a batch whose records carry "frame" = (x1, y1, dw, dh, colour) from PTrainer.resize: per image
        the canvas and the pasted rectangle, and what a frame pixel holds behind preprocess_image -- the normalisation kernel's
        own output for that colour, a constant of the model.  None: no record has one (weak views, the teacher), or the
        tile-list launch is off."""
        if not ops.frame_skip_active():
            return None
        frames = [x.get("frame") for x in batched_inputs]
        colours = {tuple(f[4]) for f in frames if f is not None}
        rings = ops.frame_rings([None if f is None else f[:4] for f in frames], images.image_sizes)
        if rings is None or len(colours) != 1:
            return None
        colour = colours.pop()
        pat = self._frame_colours.get(colour)
        if pat is None:
            probe = torch.tensor(colour, dtype=torch.uint8).view(3, 1, 1).expand(3, 8, 8).contiguous().to(self.device)
            pat = self._frame_colours[colour] = ops.preprocess_images([probe], self._mean, self._std)[0, :, :4, :4].contiguous()
        return ops.FrameState(rings, pat, ("image", colour, tuple(self._mean), tuple(self._std)))

    def inference(self, batched_inputs, do_postprocess: bool = True):
        """Eval-mode path (rcnn.py:33-34 -> D2 GeneralizedRCNN.inference + detector_postprocess):
        test-time RPN (6000 -> 1000 proposals), ROI inference, boxes rescaled to each record's height/width.
        do_postprocess=False (D2's keyword, used by modeling/tta.py): the list of Instances as the ROI heads return them, in
        the coordinates of the network input."""
        assert not self.training
        images = self.preprocess_image(batched_inputs)
        features = self.backbone(images.tensor)
        proposals, _ = self.proposal_generator(images, features, None)
        results, _ = self.roi_heads(images, features, proposals, None)
        if not do_postprocess:
            return results
        out = []
        for res, rec, size in zip(results, batched_inputs, images.image_sizes):
            out.append({"instances": detector_postprocess(res, rec.get("height", size[0]), rec.get("width", size[1]))})
        return out

    @staticmethod
    def _padded_size(batched_inputs):
        return (max(int(x["image"].shape[-2]) for x in batched_inputs), max(int(x["image"].shape[-1]) for x in batched_inputs))

    def can_run_jointly(self, sup_inputs, unsup_inputs) -> bool:
        """Both batches pad to the same canvas (then the padded region, the feature-map size and the anchor grid of each
        branch are what they would be in separate passes)."""
        return (self.training and len(sup_inputs) > 0 and len(unsup_inputs) > 0 and
                self._padded_size(sup_inputs) == self._padded_size(unsup_inputs))

    def forward_joint(self, sup_inputs, unsup_inputs, danchor=True):
        """`model(sup, branch="supervised")` and `model(unsup, branch="unsupervised", danchor=...)` (trainer.py:341,
        353-355) with ONE backbone + RPN-head pass over the concatenated images: the convolutions are per-image, so
        each branch sees exactly the activations of its separate pass; what changes is launch granularity (48 images
        per conv / wgrad launch instead of 32 + 16: fewer, fuller launches) and the summation order inside the weight
        gradients.  Returns (losses_sup, losses_unsup)."""
        assert self.can_run_jointly(sup_inputs, unsup_inputs)
        ns = len(sup_inputs)
        images = self.preprocess_image(list(sup_inputs) + list(unsup_inputs))
        # (anomaly mode: the shared backbone + RPN-head pass reports as branch "joint", each branch's heads under its own name)
        with ops.anomaly_branch("joint"):
            with ops.anomaly_scope("backbone"):
                features = self.backbone(images.tensor, self.frame_state(list(sup_inputs) + list(unsup_inputs), images))
            feats = [features[f] for f in self.proposal_generator.in_features]
            with ops.anomaly_scope("proposal_generator"):
                obj, deltas = self.proposal_generator.head_outputs(feats)
                all_props = self.proposal_generator.proposals_from_head(images, features, (obj, deltas))
        out = []
        for sl, inputs, branch, da in ((slice(0, ns), sup_inputs, "supervised", False),
                                       (slice(ns, None), unsup_inputs, "unsupervised", danchor)):
            img = ImageList(images.tensor[sl], images.image_sizes[sl])
            feat = {k: v[sl] for k, v in features.items()}
            head = ([o[sl] for o in obj], [d[sl] for d in deltas])
            gt = [x["instances"].to(self.device) for x in inputs]
            with ops.anomaly_branch(branch):
                with ops.anomaly_scope("proposal_generator"):
                    proposals, l_rpn = self.proposal_generator(img, feat, gt, branch=branch if branch == "unsupervised" else "",
                                                               danchor=da, head_out=head, proposals=all_props[sl])
                with ops.anomaly_scope("roi_heads"):
                    _, l_det = self.roi_heads(img, feat, proposals, gt, branch=branch)
            losses = {}
            losses.update(l_det)
            losses.update(l_rpn)
            out.append(losses)
        return out[0], out[1]

    def forward(self, batched_inputs, branch="supervised", danchor=False):
        if not self.training:
            return self.inference(batched_inputs)
        with ops.anomaly_branch(branch):
            return self._forward_train(batched_inputs, branch, danchor)

    def _forward_train(self, batched_inputs, branch, danchor):
        images = self.preprocess_image(batched_inputs)
        gt_instances = None
        if "instances" in batched_inputs[0]:
            gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
        with ops.anomaly_scope("backbone"):
            features = self.backbone(images.tensor, self.frame_state(batched_inputs, images))

        if branch == "supervised":
            with ops.anomaly_scope("proposal_generator"):
                proposals_rpn, proposal_losses = self.proposal_generator(images, features, gt_instances)
            with ops.anomaly_scope("roi_heads"):
                _, detector_losses = self.roi_heads(images, features, proposals_rpn, gt_instances, branch=branch)
            losses = {}
            losses.update(detector_losses)
            losses.update(proposal_losses)
            return losses, [], [], None
        if branch == "unsup_data_weak":
            with ops.anomaly_scope("proposal_generator"):
                proposals_rpn, _ = self.proposal_generator(images, features, None, compute_loss=False)
            with ops.anomaly_scope("roi_heads"):
                proposals_roih, roi_predictions = self.roi_heads(images, features, proposals_rpn, targets=None,
                                                                 compute_loss=False, branch=branch)
            return {}, proposals_rpn, proposals_roih, roi_predictions
        if branch == "unsupervised":
            with ops.anomaly_scope("proposal_generator"):
                proposals_rpn, proposal_losses = self.proposal_generator(images, features, gt_instances, branch=branch,
                                                                         danchor=danchor)
            with ops.anomaly_scope("roi_heads"):
                _, detector_losses = self.roi_heads(images, features, proposals_rpn, gt_instances, branch=branch)
            losses = {}
            losses.update(detector_losses)
            losses.update(proposal_losses)
            return losses, [], [], None
        raise ValueError(f"unknown branch {branch!r}")


def detector_postprocess(results, output_height: int, output_width: int):
    """D2 0.5 detector_postprocess: rescale the detections from the network input size to the requested output
    size, clip, drop empty boxes."""
    scale_x = output_width / results.image_size[1]
    scale_y = output_height / results.image_size[0]
    res = type(results)((int(output_height), int(output_width)), **results.get_fields())
    boxes = res.pred_boxes.clone() if res.has("pred_boxes") else res.proposal_boxes.clone()
    boxes.scale(scale_x, scale_y)
    boxes.clip(res.image_size)
    res.set("pred_boxes" if res.has("pred_boxes") else "proposal_boxes", boxes)
    return res[boxes.nonempty()]


class EnsembleTSModel(nn.Module):
    """Holder that fixes the checkpoint prefixes `modelTeacher.` / `modelStudent.` (ts_ensemble.py:20-29)."""

    def __init__(self, modelTeacher, modelStudent):
        super().__init__()
        if isinstance(modelTeacher, nn.parallel.DistributedDataParallel):
            modelTeacher = modelTeacher.module
        if isinstance(modelStudent, nn.parallel.DistributedDataParallel):
            modelStudent = modelStudent.module
        self.modelTeacher = modelTeacher
        self.modelStudent = modelStudent


def build_model(cfg):
    from .backbone import check_norm
    if check_norm(cfg.MODEL.VGG.NORM) and cfg.SOLVER.AMP.ENABLED:
        raise ValueError("MODEL.VGG.NORM='GN' with SOLVER.AMP.ENABLED=True is not implemented: the bf16-storage backbone has no "
                         "norm layer")
    if cfg.MODEL.ROI_BOX_HEAD.NUM_CONV > 0 and cfg.SOLVER.AMP.ENABLED:
        raise ValueError(f"MODEL.ROI_BOX_HEAD.NUM_CONV={cfg.MODEL.ROI_BOX_HEAD.NUM_CONV} with SOLVER.AMP.ENABLED=True is not "
                         "implemented: the bf16-storage stack has no box-head conv layers")
    model =META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
    model.to(torch.device(cfg.MODEL.DEVICE))
    return model
