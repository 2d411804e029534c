"""R-CNN box codec on HIP kernels (reference pt/modeling/box_regression.py:43-139)."""
import math
from typing import Tuple

import torch

from .. import ops

_DEFAULT_SCALE_CLAMP = math.log(1000.0 / 16)


class Box2BoxTransform:
    def __init__(self, weights: Tuple[float, float, float, float], scale_clamp: float = _DEFAULT_SCALE_CLAMP):
        self.weights = tuple(float(w) for w in weights)
        self.scale_clamp = scale_clamp

    def get_deltas(self, src_boxes: torch.Tensor, target_boxes: torch.Tensor) -> torch.Tensor:
        """(dx,dy,dw,dh) with the reference's `+1e-9` inside the logs (box_regression.py:94-95).  Differentiable
        w.r.t. src_boxes (the learnable anchors)."""
        return ops.get_deltas(src_boxes, target_boxes, self.weights)

    def apply_deltas(self, deltas: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
        """deltas (N, 4k) -> boxes (N, 4k); dw/dh clamped to log(1000/16) (box_regression.py:101-139)."""
        return ops.apply_deltas(deltas.contiguous(), boxes, self.weights, self.scale_clamp)


MODEL_TYPES = ("GUASSIAN", "LAPLACE")     # UNSUPNET.MODEL_TYPE (pt/config.py; the reference's spelling)


def uncertainty_losses(model_type: str):
    """UNSUPNET.MODEL_TYPE -> (nll_sum, kl_efl_loss): the box-uncertainty loss pair of the chosen model, resolved once when the
    model is built.  "GUASSIAN": ops.gaussian_nll_sum / ops.kl_efl_loss; "LAPLACE": ops.laplace_nll_sum /
    ops.laplace_kl_efl_loss (the same arguments).  Any other value raises ValueError (the reference's loss code has no branch
    for it and fails inside the step)."""
    if model_type == "GUASSIAN":
        return ops.gaussian_nll_sum, ops.kl_efl_loss
    if model_type == "LAPLACE":
        return ops.laplace_nll_sum, ops.laplace_kl_efl_loss
    raise ValueError(f"UNSUPNET.MODEL_TYPE {model_type!r} is not supported: expected one of {', '.join(MODEL_TYPES)}")
