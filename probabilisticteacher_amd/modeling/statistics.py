"""The statistics a reference run logs beside its losses: `rpn/num_pos_anchors`, `rpn/num_neg_anchors`
(pt/modeling/proposal_generator/rpn.py:222-228), `roi_head/num_target_{fg,bg}_samples_<branch>`
(pt/modeling/roi_heads/roi_heads.py:202-253) and `fast_rcnn/cls_accuracy`, `fg_cls_accuracy`, `false_negative`
(detectron2 0.5 `_log_classification_stats`, restated from memory: parity unpinned).

The reference reads every one of them back with `.item()` where it is made.  Here the modules leave integer COUNTS on the
device (ops.label_counts, ops.cls_stats) in one sink owned by the meta-architecture; the trainer appends them to the packed
tensor its metrics writer reads back anyway, and the ratios -- and D2's omissions -- are formed on the host afterwards."""
from typing import Dict, Optional, Sequence

import torch

KEY = "statistics"            # the entry of a step's record under which the trainer hands the sink to `_write_metrics`
EXACT_IN_FP32 = 1 << 24       # the counts travel as fp32 beside the losses: exact below 2^24


class StatisticsSink:
    """What the supervised branch of ONE step counted.  `reset()` before the step, `put_*` from the modules, then
    `packed()` (device, N_COUNTS floats in a fixed layout whatever was recorded) and `metrics()` (host) from the writer."""
    N_COUNTS = 6              # labels == 1, labels == 0 | argmax == gt, foreground, foreground & argmax == gt, foreground & argmax == K

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.rpn_counts: Optional[torch.Tensor] = None
        self.rpn_images = 0
        self.cls_counts: Optional[torch.Tensor] = None
        self.cls_rows = 0
        self.host: Dict[str, float] = {}

    def put_rpn_labels(self, counts: torch.Tensor, num_images: int, num_labels: int) -> None:
        """counts = ops.label_counts of the (N, R) labels the supervised RPN loss trains on"""
        assert num_labels < EXACT_IN_FP32, f"{num_labels} anchor labels: their counts would not survive the fp32 readback"
        self.rpn_counts, self.rpn_images = counts, int(num_images)

    def put_classification(self, counts: torch.Tensor, rows: int) -> None:
        """counts = ops.cls_stats of the (R, K + 1) scores and (R,) classes the supervised classification loss trains on"""
        assert rows < EXACT_IN_FP32, f"{rows} sampled proposals: their counts would not survive the fp32 readback"
        self.cls_counts, self.cls_rows = counts, int(rows)

    def put_scalar(self, name: str, value: float) -> None:
        """a statistic whose value the host already holds"""
        self.host[name] = float(value)

    def packed(self, device) -> torch.Tensor:
        parts = [c if c is not None else torch.zeros(k, dtype=torch.int32, device=device)
                 for c, k in ((self.rpn_counts, 2), (self.cls_counts, 4))]
        return torch.cat(parts).float()

    def metrics(self, counts: Sequence[float]) -> Dict[str, float]:
        """`counts`: the N_COUNTS values of `packed()` after the readback"""
        pos, neg, accurate, fg, fg_accurate, false_negative = (int(v) for v in counts)
        m = dict(self.host)
        if self.rpn_images > 0:
            m["rpn/num_pos_anchors"] = pos / self.rpn_images
            m["rpn/num_neg_anchors"] = neg / self.rpn_images
        if self.cls_rows > 0:                       # D2 logs nothing for an empty batch of proposals ...
            m["fast_rcnn/cls_accuracy"] = accurate / self.cls_rows
            if fg > 0:                              # ... and the foreground ratios only where there is foreground
                m["fast_rcnn/fg_cls_accuracy"] = fg_accurate / fg
                m["fast_rcnn/false_negative"] = false_negative / fg
        return m
