"""CPU restatement of detectron2 0.5 test-time augmentation (DatasetMapperTTA, GeneralizedRCNNWithTTA._inverse_boxes and
_merge_detections), written the way D2 / fvcore write it: transforms as objects whose apply_box takes the four corners
through apply_coords and then min / max, numpy float32 arrays multiplied by factors that numpy rounds to float32, and the
merge as plain fast_rcnn_inference_single_image on top of oracle.d2.batched_nms.  D2 is not installed: parity by restatement.
Shares no code with probabilisticteacher_amd/modeling/tta.py or the HIP kernels."""
import numpy as np
import torch

from oracle import d2

SCORE_THRESH = 1e-8          # _merge_detections passes it to fast_rcnn_inference_single_image


# ---------------------------------------------------------------------------- fvcore transforms (what TTA uses of them)
class Transform:
    def apply_coords(self, coords):
        raise NotImplementedError

    def apply_box(self, box):
        """fvcore Transform.apply_box: the four corners through apply_coords, then the axis-aligned hull"""
        idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
        coords = np.asarray(box).reshape(-1, 4)[:, idxs].reshape(-1, 2)
        coords = self.apply_coords(coords).reshape((-1, 4, 2))
        minxy = coords.min(axis=1)
        maxxy = coords.max(axis=1)
        return np.concatenate((minxy, maxxy), axis=1)


class HFlipTransform(Transform):
    def __init__(self, width):
        self.width = width

    def apply_coords(self, coords):
        coords = coords.copy()
        coords[:, 0] = np.float32(self.width) - coords[:, 0]
        return coords

    def inverse(self):
        return self


class ResizeTransform(Transform):
    def __init__(self, h, w, new_h, new_w):
        self.h, self.w, self.new_h, self.new_w = h, w, new_h, new_w

    def apply_coords(self, coords):
        coords = coords.copy()
        # a float32 array times a Python float: numpy multiplies in float32, the factor rounded once
        coords[:, 0] = coords[:, 0] * np.float32(self.new_w * 1.0 / self.w)
        coords[:, 1] = coords[:, 1] * np.float32(self.new_h * 1.0 / self.h)
        return coords

    def inverse(self):
        return ResizeTransform(self.new_h, self.new_w, self.h, self.w)


class TransformList:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def apply_box(self, box):
        for t in self.transforms:
            box = t.apply_box(box)
        return box

    def inverse(self):
        return TransformList([t.inverse() for t in self.transforms[::-1]])


def shortest_edge_size(h, w, size, max_size):
    """D2 0.5 ResizeShortestEdge.get_transform"""
    scale = size * 1.0 / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh = newh * scale
        neww = neww * scale
    neww = int(neww + 0.5)
    newh = int(newh + 0.5)
    return newh, neww


# ---------------------------------------------------------------------------- DatasetMapperTTA
def augmentations(h, w, H, W, min_sizes, max_size, flip):
    """[(size (h_s, w_s), flipped, TransformList)] in D2's order.  (h, w): the loader's image, (H, W): the original."""
    pre = [ResizeTransform(H, W, h, w)] if (h, w) != (H, W) else []          # NoOpTransform otherwise: nothing to apply
    out = []
    for s in min_sizes:
        hs, ws = shortest_edge_size(h, w, s, max_size)
        resize = ResizeTransform(h, w, hs, ws)
        out.append(((hs, ws), False, TransformList(pre + [resize])))
        if flip:
            out.append(((hs, ws), True, TransformList(pre + [resize, HFlipTransform(ws)])))
    return out


def plan(h, w, H, W, min_sizes, max_size, flip):
    """The same list as numbers: (size, flipped, fx, fy, gx, gy, has pre-transform) with the factors as float32."""
    rows = []
    for size, flipped, tfms in augmentations(h, w, H, W, min_sizes, max_size, flip):
        inv = tfms.inverse().transforms
        resize_inv = inv[1] if flipped else inv[0]
        fx = np.float32(resize_inv.new_w * 1.0 / resize_inv.w)
        fy = np.float32(resize_inv.new_h * 1.0 / resize_inv.h)
        has_pre = (h, w) != (H, W)
        gx = np.float32(W * 1.0 / w) if has_pre else np.float32(1.0)
        gy = np.float32(H * 1.0 / h) if has_pre else np.float32(1.0)
        rows.append((size, flipped, fx, fy, gx, gy, has_pre))
    return rows


def inverse_boxes(boxes, tfms):
    """_inverse_boxes for one augmentation: float32 numpy boxes (n, 4) in augmented coordinates -> original coordinates"""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):                  # (the tests feed NaN / inf rows on purpose)
        out = tfms.inverse().apply_box(boxes)
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------------------- _merge_detections
def merge_single_image(boxes, scores, classes, image_shape, nms_thresh, topk_per_image, score_thresh=SCORE_THRESH):
    """D2 0.5 fast_rcnn_inference_single_image on class-agnostic boxes (n, 4) and the (n, K + 1) score matrix that holds each
    detection's score at its class -- here taken row by row, which is the order filter_mask.nonzero() gives, since a row has
    one entry.  Returns boxes, scores, classes of the kept detections plus what the device path exposes on the way:
    valid (the finite filter), candidate (valid and score > thresh), clipped boxes of the valid rows, max coordinate."""
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    scores = torch.as_tensor(scores, dtype=torch.float32).reshape(-1)
    classes = torch.as_tensor(classes, dtype=torch.int64).reshape(-1)
    valid = torch.isfinite(boxes).all(dim=1) & torch.isfinite(scores)
    vb, vs, vc = boxes[valid], scores[valid], classes[valid]
    vb = d2.Boxes(vb.clone())
    vb.clip(image_shape)
    vb = vb.tensor
    filter_mask = vs > score_thresh
    cb, cs, cc = vb[filter_mask], vs[filter_mask], vc[filter_mask]
    keep = d2.batched_nms(cb, cs, cc, nms_thresh)
    if topk_per_image >= 0:
        keep = keep[:topk_per_image]
    candidate = torch.zeros_like(valid)
    candidate[valid.nonzero().view(-1)[filter_mask]] = True
    info = {"valid": valid, "candidate": candidate, "clipped": vb, "cand_boxes": cb, "cand_scores": cs, "cand_classes": cc,
            "max_coordinate": cb.max() if cb.numel() else torch.tensor(0.0)}
    return cb[keep], cs[keep], cc[keep], info


def merge(per_aug, tfms, image_shape, nms_thresh, topk_per_image):
    """One image: per_aug[a] = (boxes (n_a, 4), scores (n_a,), classes (n_a,)) CPU tensors in augmented coordinates, tfms[a] its
    TransformList.  -> boxes, scores, classes, info of merge_single_image over the concatenation in augmentation order."""
    all_b = [torch.from_numpy(inverse_boxes(b.numpy(), t)) for (b, _, _), t in zip(per_aug, tfms)]
    all_b = torch.cat(all_b) if all_b else torch.zeros((0, 4))
    all_s = torch.cat([s for _, s, _ in per_aug]) if per_aug else torch.zeros(0)
    all_c = torch.cat([c for _, _, c in per_aug]) if per_aug else torch.zeros(0, dtype=torch.int64)
    return merge_single_image(all_b, all_s, all_c, image_shape, nms_thresh, topk_per_image) + (all_b,)
