"""Torch restatements of what the logged statistics count, shared by tests/test_statistics_cpu.py and _gpu.py.

`cls_counts`: detectron2 0.5 `_log_classification_stats` (reached from `FastRCNNOutputLayers.losses`), restated from memory --
parity unpinned -- up to the four counts it divides.  `label_counts`: reference pt/modeling/proposal_generator/rpn.py:222-225."""
import torch


def cls_counts(scores: torch.Tensor, gt_classes: torch.Tensor):
    """(num_accurate, num_fg, fg_num_accurate, num_false_negative); on the CPU torch.argmax returns the first of equal maxima"""
    scores, gt_classes = scores.detach().cpu(), gt_classes.cpu()
    bg_class_ind = scores.shape[1] - 1
    if gt_classes.numel() == 0:
        return [0, 0, 0, 0]
    pred_classes = scores.argmax(dim=1)
    fg_inds = (gt_classes >= 0) & (gt_classes < bg_class_ind)
    num_fg = fg_inds.nonzero().numel()
    fg_gt_classes = gt_classes[fg_inds]
    fg_pred_classes = pred_classes[fg_inds]
    num_false_negative = (fg_pred_classes == bg_class_ind).nonzero().numel()
    num_accurate = (pred_classes == gt_classes).nonzero().numel()
    fg_num_accurate = (fg_pred_classes == fg_gt_classes).nonzero().numel()
    return [num_accurate, num_fg, fg_num_accurate, num_false_negative]


def cls_metrics(scores, gt_classes):
    """the `fast_rcnn/*` scalars D2 puts into its storage: nothing for no rows, the foreground ratios only with foreground"""
    num_instances = gt_classes.numel()
    if num_instances == 0:
        return {}
    num_accurate, num_fg, fg_num_accurate, num_false_negative = cls_counts(scores, gt_classes)
    m = {"fast_rcnn/cls_accuracy": num_accurate / num_instances}
    if num_fg > 0:
        m["fast_rcnn/fg_cls_accuracy"] = fg_num_accurate / num_fg
        m["fast_rcnn/false_negative"] = num_false_negative / num_fg
    return m


def label_counts(labels: torch.Tensor):
    """(num_pos_anchors, num_neg_anchors) before the division by the number of images"""
    labels = labels.cpu()
    return [int((labels == 1).sum().item()), int((labels == 0).sum().item())]


# the keys of `last_metrics` beside the losses, grad_norm and data_time
RPN_KEYS = {"rpn/num_pos_anchors", "rpn/num_neg_anchors"}
CLS_KEYS = {"fast_rcnn/cls_accuracy", "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative"}
SUP_KEYS = {"roi_head/num_target_fg_samples_supervised", "roi_head/num_target_bg_samples_supervised"}
UNSUP_KEYS = {"roi_head/num_target_fg_samples_unsupervised", "roi_head/num_target_bg_samples_unsupervised"}
