"""Torch restatement of the RPN's anchor labelling with MODEL.RPN.BOUNDARY_THRESH, line by line after the reference's
`label_and_sample_anchors` (pt/modeling/proposal_generator/rpn.py:414-433) and the D2 0.5 functions it calls:

    pairwise_iou -> Matcher (thresholds, low-quality matches) -> Boxes.inside_box -> labels[~inside] = -1
                 -> subsample_labels (supervised)  |  labels == 1 (pseudo labels)

It shares no code with the product; tests/test_rpn_boundary_cpu.py and tests/test_rpn_boundary_gpu.py compare the product with
it.  Everything that decides a label is evaluated in float32, the dtype of the reference; the loss figures are evaluated in
float64 (tests/losses_ref.py) from the float32 inputs.  The fixed inputs of the GPU test (`case`) live here too, with the
conditions (`guards`) that make a pass impossible while the feature is missing."""
import torch

from tests import losses_ref

STRIDE = 16
GRID_HW = (20, 28)                                             # 20 * 28 * 9 = 5 040 anchors: no multiple of 64 or 256
IMAGE_SIZES = [(320, 448), (300, 400), (320, 437)]             # (h, w) on the 320 x 448 canvas
THRESHOLDS, LABELS = (0.3, 0.7), (0, -1, 1)


# ------------------------------------------------------------------------------------------------ D2 0.5, restated
def grid_anchors(table_wh, grid_hw=GRID_HW, stride=STRIDE):
    """anchor_generator.py:108-122: cell = (-w/2, -h/2, w/2, h/2) per (w, h) row; anchor (y, x, a) = shift (x, y) * stride + cell"""
    a = torch.as_tensor(table_wh, dtype=torch.float32)
    cell = torch.stack([-a[:, 0] / 2.0, -a[:, 1] / 2.0, a[:, 0] / 2.0, a[:, 1] / 2.0], -1)
    h, w = grid_hw
    sy, sx = torch.meshgrid(torch.arange(0, h * stride, stride, dtype=torch.float32),
                            torch.arange(0, w * stride, stride, dtype=torch.float32), indexing="ij")
    shifts = torch.stack([sx.reshape(-1), sy.reshape(-1), sx.reshape(-1), sy.reshape(-1)], 1)
    return (shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4)


def pairwise_iou(b1, b2):
    area1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    area2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])
    wh = wh.clamp(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


def matcher(quality, thresholds=THRESHOLDS, labels=LABELS, allow_low_quality=True):
    """D2 Matcher.__call__ on an (M, R) quality matrix -> (matched index int64 (R,), label int8 (R,)); among equal maxima the
    lowest ground-truth index is the match"""
    m, r = quality.shape
    if quality.numel() == 0:
        return torch.zeros(r, dtype=torch.int64), torch.full((r,), labels[0], dtype=torch.int8)
    vals = quality.max(dim=0).values
    rows = torch.arange(m).view(m, 1).expand(m, r)
    matches = torch.where(quality == vals.view(1, r), rows, torch.full_like(rows, m)).min(dim=0).values
    out = torch.full((r,), 1, dtype=torch.int8)
    bounds = [-float("inf")] + list(thresholds) + [float("inf")]
    for lab, low, high in zip(labels, bounds[:-1], bounds[1:]):
        out[(vals >= low) & (vals < high)] = lab
    if allow_low_quality:                                     # set_low_quality_matches_
        best = quality.max(dim=1).values
        out[(quality == best[:, None]).nonzero()[:, 1]] = 1
    return matches, out


def inside_box(boxes, box_size, boundary_threshold=0):
    """D2 0.5 Boxes.inside_box"""
    height, width = box_size
    return ((boxes[..., 0] >= -boundary_threshold) & (boxes[..., 1] >= -boundary_threshold)
            & (boxes[..., 2] < width + boundary_threshold) & (boxes[..., 3] < height + boundary_threshold))


def subsample_labels(labels, keys, num_samples, positive_fraction, bg_label=0):
    """D2 subsample_labels + RPN._subsample_labels; the two permutations are the ascending order of the candidates' keys (the
    project's injectable stand-in for the reference's two randperm draws)"""
    positive = ((labels != -1) & (labels != bg_label)).nonzero().squeeze(1)
    negative = (labels == bg_label).nonzero().squeeze(1)
    num_pos = min(positive.numel(), int(num_samples * positive_fraction))
    num_neg = min(negative.numel(), num_samples - num_pos)
    pos_idx = positive[torch.argsort(keys[positive], stable=True)[:num_pos]]
    neg_idx = negative[torch.argsort(keys[negative], stable=True)[:num_neg]]
    out = torch.full_like(labels, -1)
    out[pos_idx] = 1
    out[neg_idx] = 0
    return out


# ------------------------------------------------------------------------------------------------ rpn.py:414-433
def label_anchors(anchors, boxes, image_sizes, boundary_thresh):
    """rpn.py:414-425 per image -> (matched_idxs (N, R) int64, labels (N, R) int8, match quality of the match (N, R))"""
    midx, labs, ious = [], [], []
    for image_size_i, gt_boxes_i in zip(image_sizes, boxes):
        quality = pairwise_iou(gt_boxes_i, anchors)
        matched_idxs, gt_labels_i = matcher(quality)
        if boundary_thresh >= 0:
            anchors_inside_image = inside_box(anchors, image_size_i, boundary_thresh)
            gt_labels_i[~anchors_inside_image] = -1
        midx.append(matched_idxs)
        labs.append(gt_labels_i)
        ious.append(quality.max(dim=0).values if len(gt_boxes_i) else torch.zeros(anchors.shape[0]))
    return torch.stack(midx), torch.stack(labs), torch.stack(ious)


def labels_sup(anchors, boxes, image_sizes, boundary_thresh, keys, num_samples, positive_fraction):
    """-> (matched_idxs, sampled labels (N, R) int8)"""
    midx, labs, _ = label_anchors(anchors, boxes, image_sizes, boundary_thresh)
    return midx, torch.stack([subsample_labels(l, k, num_samples, positive_fraction) for l, k in zip(labs, keys)])


def positives_unsup(anchors, boxes, image_sizes, boundary_thresh):
    """rpn.py:426-428 -> (matched_idxs, flat positive rows i * R + j in ascending order)"""
    midx, labs, _ = label_anchors(anchors, boxes, image_sizes, boundary_thresh)
    return midx, (labs.reshape(-1) == 1).nonzero().squeeze(1)


# ------------------------------------------------------------------------------------------------ losses (float64)
def get_deltas(src, tgt, weights=(1.0, 1.0, 1.0, 1.0)):
    """box_regression.py:66-99"""
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    sx, sy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tx, ty = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return torch.stack((wx * (tx - sx) / sw, wy * (ty - sy) / sh, ww * torch.log(tw / sw + 1e-9), wh * torch.log(th / sh + 1e-9)), 1)


def losses_sup(anchors, logits, d8, boxes, midx, labels, num_samples):
    """rpn.py:191-255 with the Gaussian box term: BCE over labels >= 0, NLL over labels == 1, both / (num_samples * N)"""
    n, r = labels.shape
    inv = 1.0 / (num_samples * n)
    flat = (labels.reshape(-1) == 1).nonzero().squeeze(1)
    img, j = flat // r, flat % r
    gt_rows = torch.stack([boxes[i][midx[i, k]] for i, k in zip(img.tolist(), j.tolist())]) if flat.numel() else torch.zeros(0, 4)
    tgt = get_deltas(anchors[j].double(), gt_rows.double())
    return {"loss_rpn_cls": float(losses_ref.bce_logits_sum(logits.double(), labels, inv)),
            "loss_rpn_loc": float(losses_ref.gaussian_nll_sum(d8.reshape(-1, 8)[flat].double(), tgt, inv))}


def losses_unsup(anchors, logits, d8, boxes, soft, sigma, midx, flat, num_samples, tau, lam, efl):
    """rpn.py:257-361: soft objectness over the positives, KL over the positives the teacher calls foreground"""
    n, r = logits.shape
    inv = 1.0 / (num_samples * n)
    img, j = (flat // r).tolist(), (flat % r).tolist()
    sel = [(i, int(midx[i, k])) for i, k in zip(img, j)]
    T = torch.stack([soft[i][g] for i, g in sel]).double()
    sig = torch.stack([sigma[i][g] for i, g in sel]).double()
    tgt = torch.stack([boxes[i][g] for i, g in sel]).double()
    loss_cls, fg = losses_ref.rpn_soft_obj_loss(T, logits.reshape(-1)[flat].double(), tau[0], lam[0], efl, inv)
    mu_p = get_deltas(anchors[flat % r].double(), tgt)
    loss_loc = losses_ref.kl_efl_loss(d8.reshape(-1, 8)[flat].double(), mu_p, sig, fg, tau[1], lam[1], efl, 0, inv)
    return {"loss_rpn_cls": float(loss_cls), "loss_rpn_loc": float(loss_loc)}


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
def case(table_wh, num_classes=8, seed=11):
    """Three images of different sizes on one canvas over the shared 5 040 anchors; image 1 has no box.  The boxes are fixed by
    hand: some well inside (their best anchors are inside), some touching or crossing the border (their best anchors stick
    out), so that at BOUNDARY_THRESH 0 every image with boxes has positives on both sides of the test (`guards`)."""
    gen = torch.Generator().manual_seed(seed)
    anchors = grid_anchors(table_wh)
    boxes = [torch.tensor([[100.0, 96.0, 228.0, 224.0],          # a 128 x 128 anchor, exactly
                           [180.0, 60.0, 362.0, 152.0],          # close to a 181 x 90 anchor
                           [0.0, 0.0, 150.0, 130.0],             # touches the top-left corner
                           [330.0, 200.0, 448.0, 320.0],         # touches the bottom-right corner
                           [40.0, 150.0, 130.0, 318.0],
                           [250.0, 170.0, 300.0, 215.0]]),       # small: only a low-quality match
             torch.zeros(0, 4),
             torch.tensor([[150.0, 100.0, 280.0, 226.0],
                           [300.0, 10.0, 437.0, 200.0],          # touches the right border of this image only
                           [0.0, 200.0, 90.0, 320.0]])]
    n, r = len(boxes), anchors.shape[0]
    out = {"anchors": anchors, "boxes": boxes, "sizes": list(IMAGE_SIZES),
           "logits": torch.randn(n, r, generator=gen), "d8": torch.randn(n, r, 8, generator=gen) * 0.5,
           "keys": torch.rand(n, r, generator=gen),
           "soft": [torch.randn(len(b), num_classes + 1, generator=gen) * 2 for b in boxes],
           "sigma": [torch.randn(len(b), 4, generator=gen) for b in boxes]}
    return out


def guards(anchors, boxes, sizes, boundary_thresh=0):
    """Conditions on the inputs, not tolerances: per image with boxes, the Matcher's labels have >= 1 positive inside, >= 1 positive
    outside (turned to ignore), >= 1 negative inside and >= 1 negative outside; and some anchor is inside one image and outside
    another.  Without them a test could pass with the feature missing."""
    _, before, _ = label_anchors(anchors, boxes, sizes, -1)
    inside = torch.stack([inside_box(anchors, s, boundary_thresh) for s in sizes])
    for i, b in enumerate(boxes):
        if len(b) == 0:
            assert int((before[i] == 0).sum()) == anchors.shape[0]
            continue
        for lab, name in ((1, "positive"), (0, "negative")):
            assert int(((before[i] == lab) & inside[i]).sum()) >= 1, f"image {i}: no inside {name}"
            assert int(((before[i] == lab) & ~inside[i]).sum()) >= 1, f"image {i}: no outside {name}"
    assert bool((inside.any(0) & ~inside.all(0)).any()), "no anchor is inside one image and outside another"
    return before, inside
