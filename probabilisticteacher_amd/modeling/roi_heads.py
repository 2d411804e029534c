"""Gaussian ROI head on HIP kernels (reference pt/modeling/roi_heads/{roi_heads.py,fast_rcnn.py}).

ROIAlign, the FC box head (fp32 MFMA GEMMs with fused bias/ReLU), IoU matching, box codec, per-class NMS and all
losses (+gradients) are HIP kernels; torch gathers rows by index and carries the per-image containers.
Quirks kept: bbox_pred emits 8 numbers per class always; apply_deltas decodes the sigma
quadruples as boxes and they are dropped (fast_rcnn.py:63); teacher scores are multiplied by 1-mean(sigmoid(sigma))
(:101); per-class NMS uses torchvision's fp32 `boxes + cls*(max+1)` offset; unsup cls loss divides by R (NaN if 0)."""
import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import ops
from ..registry import ROI_BOX_HEAD_REGISTRY, ROI_HEADS_REGISTRY
from ..structures import Boxes, FreeInstances
from .box_regression import Box2BoxTransform, uncertainty_losses
from . import sampling

GT_LOGIT = math.log((1.0 - 1e-10) / (1 - (1.0 - 1e-10)))     # proposal_utils.py:207


class _LinearP(nn.Module):
    def __init__(self, nin, nout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(nout, nin))
        self.bias = nn.Parameter(torch.zeros(nout))


POOLER_TYPES = ("ROIAlignV2", "ROIAlign", "ROIPool")


class ROIPooler(nn.Module):
    """Single-level pooler (D2 ROIPooler; constructed at roi_heads.py:68-73): MODEL.ROI_BOX_HEAD.POOLER_TYPE
    "ROIAlignV2" (aligned), "ROIAlign" (detectron2's legacy, not aligned) -- both with POOLER_SAMPLING_RATIO 0 (adaptive grid) or
    > 0 (fixed grid) -- and "ROIPool" (max pooling; the sampling ratio is ignored, as in detectron2)."""

    def __init__(self, output_size, scales, sampling_ratio, pooler_type):
        super().__init__()
        if pooler_type not in POOLER_TYPES:
            raise ValueError(f"MODEL.ROI_BOX_HEAD.POOLER_TYPE: {pooler_type!r} is not supported (one of {', '.join(POOLER_TYPES)})")
        if int(sampling_ratio) != sampling_ratio or sampling_ratio < 0:
            raise ValueError(f"MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO: expected an integer >= 0, got {sampling_ratio!r}")
        if len(scales) != 1:
            raise ValueError(f"MODEL.ROI_HEADS.IN_FEATURES: {len(scales)} feature levels; multi-level (FPN) ROI pooling is not "
                             "supported, the pooler takes exactly one")
        self.output_size, self.scale = int(output_size), float(scales[0])
        self.pooler_type, self.sampling_ratio = pooler_type, int(sampling_ratio)
        # the operator is resolved once (as box_regression.uncertainty_losses does for the loss pair)
        if pooler_type == "ROIPool":
            self._pool = lambda feat, rois, img_offsets: ops.roi_pool(feat, rois, self.output_size, self.scale,
                                                                      img_offsets=img_offsets)
        else:
            aligned = pooler_type == "ROIAlignV2"
            self._pool = lambda feat, rois, img_offsets: ops.roi_align(feat, rois, self.output_size, self.scale, img_offsets,
                                                                       aligned, self.sampling_ratio)
        # the fused ROIAlign -> fc1 bf16 operand writer (SOLVER.AMP.ENABLED) exists for ROIAlignV2 with the adaptive grid only
        self.defers = pooler_type == "ROIAlignV2" and self.sampling_ratio == 0

    def forward(self, x: List[torch.Tensor], box_lists: List[Boxes]) -> torch.Tensor:
        dev = x[0].device
        counts = [len(b) for b in box_lists]
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + c)
        if not box_lists or offs[-1] == 0:
            rois = torch.zeros((0, 5), device=dev)
        else:
            # the image-index column in one repeat_interleave (a `full` + `cat` pair per image was 2 n tiny launches); only the n
            # counts travel from the host (a fixed-size pinned staging block: no host allocation in the step)
            img_col = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.float32, device=dev),
                                              ops.dev_i32(counts, dev).long(), output_size=offs[-1])
            rois = torch.cat([img_col.unsqueeze(1), torch.cat([b.tensor for b in box_lists], 0)], 1)
        # (ops.dev_i32: pinned + asynchronous -- torch.tensor(list, device=...) copies from pageable memory, which waits for the stream)
        img_offsets = ops.dev_i32(offs, dev) if len(box_lists) == x[0].shape[0] else None
        if (self.defers and img_offsets is not None and offs[-1] > 0 and ops._native_bf16() and x[0].is_cuda
                and ops.roi_align_p8m_fits(x[0].shape[1], x[0].shape[2], x[0].shape[3], self.output_size)):
            # SOLVER.AMP.ENABLED: the pooling is deferred to its consumer -- the box head's first Linear layer takes its bf16
            # operands straight from the ROIAlign kernel (p8._RoiAlignLinearP8)
            return DeferredROIAlign(x[0], rois.contiguous(), img_offsets, self.output_size, self.scale)
        # every other setting: the materialised fp32 tensor (the box head takes its ordinary ops.linear route)
        return self._pool(x[0], rois.contiguous(), img_offsets)


class DeferredROIAlign:
    """What ROIPooler hands to the box head in the bf16-storage mode: the ROIAlign call, not yet made."""

    def __init__(self, feat, rois, img_offsets, output_size, scale):
        self.feat, self.rois, self.img_offsets, self.output_size, self.scale = feat, rois, img_offsets, output_size, scale

    def materialize(self) -> torch.Tensor:
        return ops.roi_align(self.feat, self.rois, self.output_size, self.scale, self.img_offsets)


BOX_HEAD_NORM_KEY = "MODEL.ROI_BOX_HEAD.NORM"
BOX_HEAD_NORMS = ("", "GN")


class _HeadConvP(nn.Module):
    """`weight` (c2_msra_fill), `bias` (zeros; absent with a norm, D2 Conv2d(bias=not norm)) and the `norm` child of one 3x3 conv
    of the box head, registered in D2's order: weight, bias, norm.weight, norm.bias."""

    def __init__(self, cin, cout, norm):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")
        if norm:
            from .backbone import _GroupNormParams      # (solver.norm_parameter_names finds it: SOLVER.WEIGHT_DECAY_NORM applies)
            self.norm = _GroupNormParams(cout)
        else:
            self.bias = nn.Parameter(torch.zeros(cout))


@ROI_BOX_HEAD_REGISTRY.register()
class FastRCNNConvFCHead(nn.Module):
    """[conv3x3 -> norm -> ReLU] x NUM_CONV -> flatten -> [fc + ReLU] x NUM_FC: D2 0.5's FastRCNNConvFCHead
    restated literally -- D2 is not installed here, so parity is by restatement (tests/box_head_ref.py), as for TTA and COCOeval.

    conv{k}: 3x3, stride 1, padding 1, to CONV_DIM channels, bias = not NORM, norm child `conv{k}.norm`, c2_msra_fill init, bias 0;
    NORM "" or "GN" (GroupNorm(32, CONV_DIM), eps 1e-5, weight 1, bias 0).  fc{k}: c2_xavier_fill init.  Convs come before fcs in
    the state dict (D2's optimiser numbering).  With NUM_FC == 0 the output stays (R, CONV_DIM, P, P) and `output_size` is its
    element count.

    The conv layers run on the ROI mosaic (ops.roi_mosaic_*, csrc/roi_mosaic.hip): ROIs packed 64 to a 64 x 64 canvas at P = 7,
    ops.conv3x3 on the canvases, gutters re-zeroed by the mask (no norm) or by the mosaic GroupNorm.  NUM_CONV == 0 is the fc-only
    head, launch for launch what it was."""

    def __init__(self, cfg, input_shape):
        super().__init__()
        H = cfg.MODEL.ROI_BOX_HEAD
        self.num_conv, self.num_fc = int(H.NUM_CONV), H.NUM_FC
        self.norm = "" if H.NORM is None else H.NORM
        if self.norm not in BOX_HEAD_NORMS:
            raise ValueError(f"{BOX_HEAD_NORM_KEY}={H.NORM!r} is not implemented: accepted values are "
                             f"{', '.join(repr(v) for v in BOX_HEAD_NORMS)} (BN and SyncBN need running statistics this build does "
                             "not have)")
        channels, self.pooled = input_shape.channels, int(input_shape.height)
        if self.num_conv > 0:
            from .backbone import GN_GROUPS
            if input_shape.height != input_shape.width:
                raise ValueError(f"MODEL.ROI_BOX_HEAD.NUM_CONV={self.num_conv}: the ROI mosaic takes square pooled maps, got "
                                 f"{input_shape.height} x {input_shape.width}")
            if self.norm and H.CONV_DIM % GN_GROUPS:
                raise ValueError(f"{BOX_HEAD_NORM_KEY}='GN': MODEL.ROI_BOX_HEAD.CONV_DIM={H.CONV_DIM} channels do not divide into "
                                 f"{GN_GROUPS} groups")
            cell = (H.CONV_DIM // GN_GROUPS) * (self.pooled + 1) ** 2
            if self.norm and cell > ops.ROI_MOSAIC_GN_MAX_CELL:
                raise ValueError(f"{BOX_HEAD_NORM_KEY}='GN': a (ROI, group) cell of CONV_DIM / {GN_GROUPS} x (POOLER_RESOLUTION + 1)^2 = "
                                 f"{cell} floats exceeds the {ops.ROI_MOSAIC_GN_MAX_CELL} the mosaic GroupNorm holds in a wave")
        for k in range(self.num_conv):
            setattr(self, f"conv{k + 1}", _HeadConvP(channels, H.CONV_DIM, self.norm))
            channels = H.CONV_DIM
        self.conv_dim = channels
        dim = channels * input_shape.height * input_shape.width
        for k in range(H.NUM_FC):
            fc = _LinearP(dim, H.FC_DIM)
            nn.init.kaiming_uniform_(fc.weight, a=1)
            setattr(self, f"fc{k + 1}", fc)
            dim = H.FC_DIM
        self.output_size = dim

    accepts_deferred_roi_align = True      # forward() takes ROIPooler's DeferredROIAlign (SOLVER.AMP.ENABLED) as well as a tensor

    def _convs(self, x):
        """(R, C, P, P) -> (R, CONV_DIM, P, P) on the ROI mosaic, at most ops.ROI_MOSAIC_CHUNK ROIs per pack"""
        total, P = int(x.shape[0]), self.pooled
        if total == 0:
            return x.new_zeros((0, self.conv_dim, P, P))
        outs = []
        for a in range(0, total, ops.ROI_MOSAIC_CHUNK):
            xs = x[a:a + ops.ROI_MOSAIC_CHUNK]
            r = int(xs.shape[0])
            t = ops.roi_mosaic_pack(xs)
            for k in range(1, self.num_conv + 1):
                conv = getattr(self, f"conv{k}")
                with ops.anomaly_scope(f"conv{k}"):
                    if self.norm:
                        t = ops.conv3x3(t, conv.weight, ops.zero_bias(conv.weight.shape[0], t.device), False)
                        with ops.anomaly_scope("norm"):
                            t = ops.roi_mosaic_gn_relu(t, conv.norm.weight, conv.norm.bias, r, P, conv.norm.num_groups, conv.norm.eps)
                    else:
                        t = ops.conv3x3(t, conv.weight, conv.bias, True)
                        if k < self.num_conv:       # (the last layer's gutters are never read: unpack takes the data pixels, and its
                            t = ops.roi_mosaic_mask(t, r, P)        # backward, pack, writes the zeros of dy itself)
            outs.append(ops.roi_mosaic_unpack(t, r, P))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def forward(self, x):
        first = 0
        if self.num_conv > 0:
            if isinstance(x, DeferredROIAlign):
                x = x.materialize()
            x = self._convs(x)
            if self.num_fc == 0:
                return x
        if isinstance(x, DeferredROIAlign):
            from .. import p8
            if self.num_fc and self.fc1.weight.shape[1] >= p8.LINEAR_MIN_K:
                with ops.anomaly_scope("fc1"):        # (the fused node: box_pooler's ROIAlign + fc1)
                    x = p8.roi_align_linear(x.feat, x.rois, x.img_offsets, x.output_size, x.scale, self.fc1.weight, self.fc1.bias, True)
                first = 1
            else:
                x = x.materialize()
        if first == 0:
            x = x.flatten(1)
        for k in range(first, self.num_fc):
            fc = getattr(self, f"fc{k + 1}")
            with ops.anomaly_scope(f"fc{k + 1}"):
                x = ops.linear(x, fc.weight, fc.bias, True)
        return x


def build_box_head(cfg, input_shape):
    return ROI_BOX_HEAD_REGISTRY.get(cfg.MODEL.ROI_BOX_HEAD.NAME)(cfg, input_shape)


# ---- teacher inference: one NMS per image over all (roi, class) entries, or one per (image, class)
NMS_DENSE_AUTO_MAX = 16384      # entries per image the LDS segmented sort holds: the dense path's range when left on auto
NMS_SEGMENT_MAX = 524288        # boxes per NMS segment: the scan kernel keeps one row of the bitmask in LDS (64 KB)


def nms_ws_bytes_dense(nimg: int, num_classes: int, max_r: int) -> int:
    """bitmask workspace of the dense path: one segment of K * max R_i entries per image"""
    cap = num_classes * max_r
    return nimg * cap * ((cap + 63) // 64) * 8


def nms_ws_bytes_by_class(nimg: int, num_classes: int, max_r: int) -> int:
    """bitmask workspace of the by-class path: K segments of max R_i entries per image"""
    return nimg * num_classes * max_r * ((max_r + 63) // 64) * 8


def select_nms_by_class(num_classes: int, counts, nms_by_class: Optional[bool] = None) -> bool:
    """Which path `GuassianFastRCNNOutputLayers.inference` takes for a batch with counts[i] proposals in image i: True = NMS per
    (image, class) segment, False = one NMS per image over its dense K * R_i (roi, class) entries.  None decides by size: dense
    while K * max R_i <= 16 384 (every shipped config: K = 8 x 2000 proposals, K = 1), by class above; True / False force a
    path.  Raises ValueError for a segment the single-pass bitmask NMS cannot hold (524 288 boxes): K * max R_i on the dense
    path, max R_i on the by-class path."""
    max_r = max(counts) if len(counts) else 0
    cap = num_classes * max_r
    by_class = cap > NMS_DENSE_AUTO_MAX if nms_by_class is None else bool(nms_by_class)
    if not by_class and cap > NMS_SEGMENT_MAX:
        raise ValueError(f"ROI inference: {num_classes} classes x {max_r} proposals = {cap} NMS candidates per image exceed the "
                         f"{NMS_SEGMENT_MAX} the single-pass bitmask NMS holds; leave nms_by_class on None / True or lower "
                         "MODEL.RPN.POST_NMS_TOPK_TEST")
    if by_class and max_r > NMS_SEGMENT_MAX:
        raise ValueError(f"ROI inference: {max_r} proposals per image exceed the {NMS_SEGMENT_MAX} the single-pass bitmask NMS "
                         "holds per class; lower MODEL.RPN.POST_NMS_TOPK_TEST")
    return by_class


class GuassianFastRCNNOutputLayers(nn.Module):
    """cls_score (K+1) and bbox_pred (8K) + Gaussian / entropy-focal losses + teacher inference
    (fast_rcnn.py:145-409)."""

    def __init__(self, cfg, input_size: int):
        super().__init__()
        self.cfg = cfg
        self.num_classes = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        assert not cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG
        self.model_type = cfg.UNSUPNET.MODEL_TYPE
        self.nll_loss, self.kl_loss = uncertainty_losses(self.model_type)        # fast_rcnn.py:286-307, :238-257
        self.box2box_transform = Box2BoxTransform(weights=cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS)
        self.cls_score = _LinearP(input_size, self.num_classes + 1)
        self.bbox_pred = _LinearP(input_size, self.num_classes * 8)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        self.test_score_thresh = cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST
        self.test_nms_thresh = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
        self.test_topk_per_image = cfg.TEST.DETECTIONS_PER_IMAGE
        self.loss_weight = {"loss_cls": 1.0, "loss_box_reg": cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT}

    statistics = None       # the meta-architecture's StatisticsSink (modeling/statistics.py); None = nothing is counted
    nms_by_class: Optional[bool] = None     # inference(): None = by size (select_nms_by_class), True / False force a path

    def forward(self, x):
        if x.dim() > 2:         # a box head that ends in a conv layer (NUM_FC 0): D2's FastRCNNOutputLayers flattens too
            x = x.flatten(1)
        with ops.anomaly_scope("cls_score"):
            scores = ops.linear(x, self.cls_score.weight, self.cls_score.bias, False)
        with ops.anomaly_scope("bbox_pred"):
            return scores, ops.linear(x, self.bbox_pred.weight, self.bbox_pred.bias, False)

    # ---- supervised (D2 FastRCNNOutputLayers.losses + fast_rcnn.py:265-336)
    def losses(self, predictions, proposals: List[FreeInstances]):
        scores, deltas = predictions
        K = self.num_classes
        gt_classes = torch.cat([p.gt_classes for p in proposals], 0)
        pb = torch.cat([p.proposal_boxes.tensor for p in proposals], 0)
        gb = torch.cat([p.gt_boxes.tensor for p in proposals], 0)
        if self.statistics is not None:                     # D2 0.5 _log_classification_stats, as device counts
            self.statistics.put_classification(ops.cls_stats(scores, gt_classes), gt_classes.numel())
        with ops.anomaly_scope("loss_cls"):
            loss_cls = ops.softmax_ce_mean(scores, gt_classes)
        fg = torch.nonzero((gt_classes >= 0) & (gt_classes < K)).squeeze(1)
        d = deltas.view(-1, K, 8)[fg, gt_classes[fg]]
        with ops.anomaly_scope("loss_box_reg"):
            tgt = self.box2box_transform.get_deltas(pb[fg], gb[fg])
            loss_box = self.nll_loss(d, tgt, 1.0 / max(gt_classes.numel(), 1.0))
        out = {"loss_cls": loss_cls, "loss_box_reg": loss_box}
        return {k: v * self.loss_weight.get(k, 1.0) for k, v in out.items()}

    # ---- unsupervised (roi_heads.py:130-171 + fast_rcnn.py:179-263)
    def losses_unsupervised(self, predictions, proposals: List[FreeInstances]):
        scores, deltas = predictions
        K, U = self.num_classes, self.cfg.UNSUPNET
        T = torch.cat([p.soft_label for p in proposals]).detach().contiguous()
        r = T.shape[0]
        inv = 1.0 / r if r > 0 else float("nan")                      # fast_rcnn.py:209 divides by R
        with ops.anomaly_scope("loss_cls"):
            out = {"loss_cls": ops.soft_ce_efl(T, scores, U.TAU[0], U.EFL_LAMBDA[0], bool(U.EFL), inv)}
        if proposals[0].has("boxes_sigma"):
            with torch.no_grad():
                sig_p = torch.cat([p.boxes_sigma for p in proposals])
                pb = torch.cat([p.proposal_boxes.tensor for p in proposals])
                psb = torch.cat([p.pseudo_boxes.tensor for p in proposals])
                cls = T.max(-1)[1] if r > 0 else torch.zeros(0, dtype=torch.int64, device=T.device)
                rows = torch.nonzero(cls != K).squeeze(1)
                with ops.anomaly_scope("loss_box_reg"):
                    mu_p = self.box2box_transform.get_deltas(pb[rows], psb[rows])
                sig_sel = sig_p[rows].contiguous()
            q = deltas.view(-1, K, 8)[rows, cls[rows]]                 # one gather instead of the per-row loop (:159-161)
            with ops.anomaly_scope("loss_box_reg"):
                out["loss_box_reg"] = self.kl_loss(q, mu_p, sig_sel, None, U.TAU[1], U.EFL_LAMBDA[1], bool(U.EFL), 1, 1.0)
        return out

    # ---- teacher inference (fast_rcnn.py:338-409, :34-141)
    @torch.no_grad()
    def inference(self, predictions, proposals: List[FreeInstances]):
        """fast_rcnn.py:338-409 + fast_rcnn_inference(_single_image) :34-141 for the whole batch at once.
        `ptmi_roi_infer_prepare` does the per-ROI part (decode, finite filter, clip, score threshold, sigma rescoring,
        per-image candidate count / max coordinate) in one launch and leaves dense (roi, class) arrays; candidates are
        never compacted on the host: a segmented stable sort of the keys over the fixed (R_i * K)-entry segments puts
        each image's candidates first, in the order batched_nms visits them, and the NMS runs on the first count[i]
        entries (counts stay on the device).  With many classes (select_nms_by_class) the same entries go through NMS as one
        segment per (image, class) instead, and the kept ones are merged per image.  ONE device->host read per call (the
        kept-detection counts) on either path."""
        scores, deltas = predictions
        K = self.num_classes
        dev = scores.device
        n = len(proposals)
        counts = [len(p) for p in proposals]
        R = sum(counts)
        pb = torch.cat([p.proposal_boxes.tensor for p in proposals], 0).contiguous()
        probs = ops.softmax_rows(scores)
        roff = [0]
        for c in counts:
            roff.append(roff[-1] + c)
        roi_img = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), ops.dev_i32(counts, dev),
                                          output_size=R)
        hw = torch.tensor([[float(p.image_size[0]), float(p.image_size[1])] for p in proposals]).pin_memory().to(
            dev, non_blocking=True)
        boxes, keys, roi_valid, img_max, img_cnt, img_inv = ops.roi_infer_prepare(
            deltas.contiguous(), pb, probs, roi_img, hw, K, self.box2box_transform.weights,
            self.box2box_transform.scale_clamp, self.test_score_thresh)
        seg = ops.dev_i32([K * o for o in roff], dev)                     # dense (roi, class) segments per image
        # NMS capacity = the segment length (no host read to learn the candidate count), and the bitmask workspace is
        # segments * capacity * ceil(capacity / 64) * 8 bytes.  Two layouts, chosen by select_nms_by_class:
        #   dense     one segment of K * max R_i entries per image: 32 MB per image at K = 8, R = 2000 (the shipped configs,
        #             ~0.5 GB for 16 images), but 200 MB per image at K = 20 and 3.2 GB at K = 80 -- it grows with (K R)^2;
        #   by class  K segments of max R_i entries per image: 4 MB per (image, 8 classes) at R = 2000 -- 65 / 164 / 655 MB
        #             for 16 images at K = 8 / 20 / 80.  Pairs of different classes never suppress each other, so only this
        #             much of the dense mask was ever needed.
        # The scan kernel keeps one row of the mask in LDS, which caps a segment at 524 288 boxes.
        max_r = max(counts) if counts else 0
        cap = K * max_r
        lengths = [K * c for c in counts]
        det_max = self.test_topk_per_image
        if select_nms_by_class(K, counts, self.nms_by_class):
            # class-major keys, one sort + one NMS over the n * K (image, class) segments, kept entries back to the dense
            # array; its stable descending sort per image is batched_nms's order (score, then dense index roi * K + class)
            cseg_h = ops.roi_class_seg_offsets(counts, K)
            cseg = ops.dev_i32(cseg_h, dev)
            ckeys, ccnt = ops.roi_infer_class_keys(keys, cseg, n, K, max_r)
            csrt, corder = ops.segsort_desc(ckeys, cseg, max_len=max_r, lengths=[c for c in counts for _ in range(K)])
            nms_boxes = ops.roi_infer_class_nms_boxes(boxes, corder, cseg, img_max, img_cnt, n, K, max_r)
            # (no class contributes more than DETECTIONS_PER_IMAGE entries to the image's top-k)
            keep_c = max(min(max_r, det_max) if det_max >= 0 else max_r, 1)
            keep, kcnt = ops.nms_batched(nms_boxes, cseg, max_r, float(self.test_nms_thresh), int(keep_c), seg_counts=ccnt)
            kept_keys, img_kept = ops.roi_infer_class_collect(csrt, corder, keep, kcnt, cseg, n, K, max_r, R)
            srt, order = ops.segsort_desc(kept_keys.view(-1), seg, max_len=cap, topk=det_max if det_max > 0 else None,
                                          lengths=lengths)
            host = torch.cat([img_kept, img_inv]).cpu().tolist()          # the one sync
            kc, dropped = host[:n], host[n:]
            if det_max >= 0:
                kc = [min(k, det_max) for k in kc]
            first = seg[:-1].long()
            pos = torch.cat([first[i] + torch.arange(kc[i], device=dev) for i in range(n)], 0) if n else seg[:0].long()
        else:
            srt, order = ops.segsort_desc(keys.view(-1), seg, max_len=cap, lengths=lengths)
            nms_boxes = ops.roi_infer_nms_boxes(boxes, order, seg, img_max, cap, K)
            topk = det_max if det_max >= 0 else max(cap, 1)
            keep, kcnt = ops.nms_batched(nms_boxes, seg, cap, float(self.test_nms_thresh), int(max(topk, 1)),
                                         seg_counts=img_cnt)
            host = torch.cat([kcnt, img_inv]).cpu().tolist()              # the one sync
            kc, dropped = host[:n], host[n:]
            keep_g = keep.long() + seg[:-1].long().unsqueeze(1)            # (seg[i] = K * roff[i])
            pos = torch.cat([keep_g[i, :kc[i]] for i in range(n)], 0) if n else seg[:0].long()
        img_base = torch.repeat_interleave(seg[:-1].long(), ops.dev_i32(kc, dev).long(), output_size=sum(kc))
        dense = img_base + order[pos].long()                              # flat (roi, class) index of every detection
        roi, cls = torch.div(dense, K, rounding_mode="floor"), dense % K
        r_boxes, r_scores = boxes.view(-1, 4)[dense], srt[pos]
        r_sig = deltas.view(R, K, 8)[roi, cls, 4:]
        img_start = torch.div(img_base, K, rounding_mode="floor")        # first ROI row of the detection's image
        row = roi
        if any(dropped):
            # reference quirk (fast_rcnn.py:68-71,96,126): after the finite filter the kept ROIs are re-indexed by their
            # position in the FILTERED list, and `scores_logists` / the returned ROI indices use that position (the
            # logits are even read from the UNfiltered tensor at it)
            excl = torch.cumsum(roi_valid.long(), 0) - roi_valid.long()
            row = img_start + (excl[roi] - excl[img_start])
        r_logits = scores[row]
        results, kept_rows = [], []
        c0 = 0
        row_local = row - img_start                                        # ROI index within the image (img_start = roff[i])
        for i, prop in enumerate(proposals):
            k = kc[i]
            res = FreeInstances(prop.image_size)
            res.pred_boxes = Boxes(r_boxes[c0:c0 + k])
            res.scores = r_scores[c0:c0 + k]
            res.pred_classes = cls[c0:c0 + k]
            res.scores_logists = r_logits[c0:c0 + k]
            res.boxes_sigma = r_sig[c0:c0 + k]
            results.append(res)
            kept_rows.append(row_local[c0:c0 + k])
            c0 += k
        return results, kept_rows


@ROI_HEADS_REGISTRY.register()
class GuassianROIHead(nn.Module):
    def __init__(self, cfg, input_shape: Dict):
        super().__init__()
        self.cfg = cfg
        H = cfg.MODEL.ROI_HEADS
        self.num_classes = H.NUM_CLASSES
        self.batch_size_per_image = H.BATCH_SIZE_PER_IMAGE
        self.positive_fraction = H.POSITIVE_FRACTION
        self.proposal_append_gt = H.PROPOSAL_APPEND_GT
        self.iou_thresholds, self.iou_labels = list(H.IOU_THRESHOLDS), list(H.IOU_LABELS)
        self.box_in_features = H.IN_FEATURES
        B = cfg.MODEL.ROI_BOX_HEAD
        in_channels = input_shape[self.box_in_features[0]].channels
        scales = tuple(1.0 / input_shape[k].stride for k in self.box_in_features)
        self.box_pooler = ROIPooler(B.POOLER_RESOLUTION, scales, B.POOLER_SAMPLING_RATIO, B.POOLER_TYPE)
        from .backbone import ShapeSpec
        self.box_head = build_box_head(cfg, ShapeSpec(channels=in_channels, height=B.POOLER_RESOLUTION,
                                                      width=B.POOLER_RESOLUTION))
        self.box_predictor = GuassianFastRCNNOutputLayers(cfg, self.box_head.output_size)
        self.train_on_pred_boxes = B.TRAIN_ON_PRED_BOXES

    statistics = None       # the meta-architecture's StatisticsSink (modeling/statistics.py); None = nothing is recorded

    def forward(self, images, features, proposals, targets=None, compute_loss=True, branch=""):
        if self.training and compute_loss:
            assert targets
            proposals = self.label_and_sample_proposals(proposals, targets, branch=branch)
        feats = [features[f] for f in self.box_in_features]
        with ops.anomaly_scope("box_pooler"):
            box_features = self.box_pooler(feats, [x.proposal_boxes for x in proposals])
            if isinstance(box_features, DeferredROIAlign) and not getattr(self.box_head, "accepts_deferred_roi_align", False):
                box_features = box_features.materialize()       # any other head registered in ROI_BOX_HEAD_REGISTRY gets a tensor
        with ops.anomaly_scope("box_head"):
            box_features = self.box_head(box_features)
        with ops.anomaly_scope("box_predictor"):
            predictions = self.box_predictor(box_features)
        del box_features
        if branch == "unsupervised" and self.training:
            with ops.anomaly_scope("box_predictor"):
                return proposals, self.box_predictor.losses_unsupervised(predictions, proposals)
        if self.training and compute_loss:
            with ops.anomaly_scope("box_predictor"):
                return proposals, self.box_predictor.losses(predictions, proposals)
        pred_instances, _ = self.box_predictor.inference(predictions, proposals)
        return pred_instances, predictions

    @torch.no_grad()
    def label_and_sample_proposals(self, proposals, targets, branch=""):
        """roi_heads.py:192-255 (+ proposal_utils.py:157-224 GT append, D2 _sample_proposals A.12) and
        roi_heads.py:257-291 for the unsupervised branch."""
        K = self.num_classes
        out = []
        dev = proposals[0].proposal_boxes.tensor.device
        n = len(proposals)
        if branch == "unsupervised":
            # matched-label-1 proposals only (roi_heads.py:257-291): one IoU-match launch pair, one count read and one
            # nonzero for the whole batch instead of a kernel chain + host sync per image
            pcounts = [len(p.proposal_boxes) for p in proposals]
            gcounts = [len(t.pseudo_boxes) for t in targets]
            pb_all = torch.cat([t.pseudo_boxes.tensor for t in targets], 0)
            boxes_all = torch.cat([p.proposal_boxes.tensor for p in proposals], 0)
            midx, mlab, _, gt_off, box_off = ops.iou_match_batched(pb_all, gcounts, boxes_all, pcounts, self.iou_thresholds,
                                                                   self.iou_labels, False)
            hit = mlab == 1
            img_of = torch.repeat_interleave(torch.arange(n, device=dev), box_off[1:] - box_off[:-1],
                                             output_size=boxes_all.shape[0])
            counts = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, img_of, hit.long()).cpu().tolist()
            flat = torch.nonzero(hit).squeeze(1)
            glob = midx[flat] + gt_off[img_of[flat]].long()                 # rows of the concatenated pseudo labels
            sel_boxes = boxes_all[flat]
            has_sigma = targets[0].has("boxes_sigma")
            if pb_all.shape[0] > 0:
                sel_pb = pb_all[glob]
                sel_soft = torch.cat([t.scores_logists for t in targets], 0)[glob]
                sel_sig = torch.cat([t.boxes_sigma for t in targets], 0)[glob] if has_sigma else None
            c0 = 0
            for prop, tgt, cnt, gc in zip(proposals, targets, counts, gcounts):
                r = FreeInstances(prop.image_size)
                r.proposal_boxes = Boxes(sel_boxes[c0:c0 + cnt])
                if gc == 0:
                    r.pseudo_boxes, r.soft_label = tgt.pseudo_boxes, tgt.scores_logists
                    if has_sigma:
                        r.boxes_sigma = tgt.boxes_sigma
                else:
                    r.pseudo_boxes, r.soft_label = Boxes(sel_pb[c0:c0 + cnt]), sel_soft[c0:c0 + cnt]
                    if has_sigma:
                        r.boxes_sigma = sel_sig[c0:c0 + cnt]
                c0 += cnt
                out.append(r)
            if self.statistics is not None:                 # roi_heads.py:220-221: the reference appends zeros here
                self.statistics.put_scalar("roi_head/num_target_fg_samples_" + branch, 0.0)
                self.statistics.put_scalar("roi_head/num_target_bg_samples_" + branch, 0.0)
            return out
        # the whole batch at once.  Proposals (+ appended ground truth) of all images are
        # concatenated; labels come from one batched IoU match, the 512-per-image sample from one sampling launch
        # (random keys, see sampling.py); ONE device->host read (the sample sizes) for the batch.
        gcounts = [len(t.gt_boxes) for t in targets]
        gt_all = torch.cat([t.gt_boxes.tensor for t in targets], 0)
        total_gt = gt_all.shape[0]
        parts_b, parts_l, bcounts = [], [], []
        gt_logit = torch.full((total_gt,), GT_LOGIT, device=dev)
        g0 = 0
        for prop, tgt, gc in zip(proposals, targets, gcounts):
            parts_b.append(prop.proposal_boxes.tensor)
            parts_l.append(prop.objectness_logits)
            cnt = len(prop.proposal_boxes)
            if self.proposal_append_gt:
                parts_b.append(tgt.gt_boxes.tensor)
                parts_l.append(gt_logit[g0:g0 + gc])
                cnt += gc
            g0 += gc
            bcounts.append(cnt)
        boxes_all = torch.cat(parts_b, 0)
        logits_all = torch.cat(parts_l, 0)
        midx, mlab, _, gt_off, box_off = ops.iou_match_batched(gt_all, gcounts, boxes_all, bcounts, self.iou_thresholds,
                                                               self.iou_labels, False)
        total = boxes_all.shape[0]
        img_of = torch.repeat_interleave(torch.arange(n, device=dev), box_off[1:] - box_off[:-1], output_size=total)
        if total_gt > 0:
            gidx = (midx + gt_off[img_of].long()).clamp_(max=total_gt - 1)          # images without gt: masked below
            cls = torch.cat([t.gt_classes for t in targets], 0)[gidx]
            cls = torch.where(mlab == 0, torch.full_like(cls, K), cls)              # also covers images without gt
            cls = torch.where(mlab == -1, torch.full_like(cls, -1), cls)
        else:
            gidx = None
            cls = torch.full((total,), K, dtype=torch.int64, device=dev)
        keys = sampling.draw_keys(cls, bcounts, K)
        npos = int(self.batch_size_per_image * self.positive_fraction)
        fg, bg, cnt = ops.sample_by_keys(cls, keys, box_off, max(bcounts), self.batch_size_per_image, npos, K)
        cnt_h = cnt.cpu().tolist()                                                   # the one sync
        if self.statistics is not None:                     # roi_heads.py:243-253: np.mean over the images, from that read
            self.statistics.put_scalar("roi_head/num_target_fg_samples_" + branch, sum(nf for nf, _ in cnt_h) / len(cnt_h))
            self.statistics.put_scalar("roi_head/num_target_bg_samples_" + branch, sum(nb for _, nb in cnt_h) / len(cnt_h))
        fg = fg + box_off[:-1].long().unsqueeze(1)
        bg = bg + box_off[:-1].long().unsqueeze(1)
        sel = torch.cat([t for i, (nf, nb) in enumerate(cnt_h) for t in (fg[i, :nf], bg[i, :nb])], 0)
        sel_boxes, sel_logits, sel_cls = boxes_all[sel], logits_all[sel], cls[sel]
        if total_gt > 0:
            has_gt = torch.tensor([float(gc > 0) for gc in gcounts]).pin_memory().to(dev, non_blocking=True)
            sel_gt = gt_all[gidx[sel]] * has_gt[img_of[sel]].unsqueeze(1)            # zeros for images without gt
        else:
            sel_gt = boxes_all.new_zeros((sel.shape[0], 4))
        c0 = 0
        for prop, (nf, nb) in zip(proposals, cnt_h):
            k = nf + nb
            r = FreeInstances(prop.image_size)
            r.proposal_boxes = Boxes(sel_boxes[c0:c0 + k])
            r.objectness_logits = sel_logits[c0:c0 + k]
            r.gt_classes = sel_cls[c0:c0 + k]
            r.gt_boxes = Boxes(sel_gt[c0:c0 + k])
            c0 += k
            out.append(r)
        return out


def build_roi_heads(cfg, input_shape):
    return ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, input_shape)
