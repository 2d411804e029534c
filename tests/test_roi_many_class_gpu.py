"""GPU (pytest -m gpu): teacher ROI inference with NMS per (image, class) segment -- the path for 20- and 80-class heads.

  1. each new kernel against a torch restatement, plain equality (the fp32 class-offset add included);
  2. the by-class path against the dense path on identical inputs, `torch.equal` on every output;
  3. K = 80 x 2000 proposals against oracle.pt.roi_inference, inside the by-class memory law;
  4. D2 0.5 batched_nms's 40 000-box rule (offset trick below, one NMS per class on unshifted boxes from there on);
  5. the shipped class count still launches what it launched, name for name;
  6. one mutual-learning step of a 20-class PTrainer, twice, bit for bit.

The oracle comparison is the one tests/test_functions_gpu.py::_check_inference applies: indices, classes and copied fields
exact, boxes rtol 1e-5 / atol 1e-4, scores rtol 1e-5 / atol 1e-7.  The oracle's >= 40 000 branch orders its result with an
unstable argsort, so the inputs of (3) and (4) are made to have pairwise distinct candidate scores per image, and that is
asserted."""
import contextlib
import math
import os

import pytest
import torch

from oracle import d2, pt as opt
from tests.helpers import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptmi_roi_infer_class_keys", "ptmi_roi_infer_class_nms_boxes", "ptmi_roi_infer_class_collect")


def _cfg(K, *opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"),
                     ["MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "MODEL.ROI_HEADS.NUM_CLASSES", K] + list(opts))


def _layer(K, *opts, by_class=None):
    from probabilisticteacher_amd.modeling.roi_heads import GuassianFastRCNNOutputLayers
    layer = GuassianFastRCNNOutputLayers(_cfg(K, *opts), 1024)
    layer.nms_by_class = by_class
    return layer


def _rand_boxes(gen, n, h, w, lo=8.0, hi=0.5):
    cx, cy = torch.rand(n, generator=gen) * w, torch.rand(n, generator=gen) * h
    bw = lo + torch.rand(n, generator=gen) * w * hi
    bh = lo + torch.rand(n, generator=gen) * h * hi
    return torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)


def _roi_case(gen, K, counts, sizes, scale=2.0):
    """(tests/test_functions_gpu.py::_roi_case) random logits / deltas and per-image proposals, for the HIP path and the oracle"""
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    R = sum(counts)
    scores = torch.randn(R, K + 1, generator=gen) * scale
    deltas = torch.randn(R, 8 * K, generator=gen)
    deltas.view(R, K, 8)[..., :2] *= 2.0                   # centre shifts of a few tenths of the box
    deltas.view(R, K, 8)[..., 2:4] *= 1.5                  # size changes
    props_g, props_o = [], []
    for c, (h, w) in zip(counts, sizes):
        b = _rand_boxes(gen, c, h, w)
        b[:, 0::2].clamp_(0, w)
        b[:, 1::2].clamp_(0, h)
        pg, po = FreeInstances((h, w)), opt.FreeInstances((h, w))
        pg.proposal_boxes, po.proposal_boxes = Boxes(b.to(DEV)), d2.Boxes(b.clone())
        props_g.append(pg)
        props_o.append(po)
    return scores, deltas, props_g, props_o


@contextlib.contextmanager
def _spy():
    from probabilisticteacher_amd import _lib
    names, real = [], _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def _prepare(layer, scores, deltas, props_g):
    """what inference() hands to either NMS path: ptmi_roi_infer_prepare's outputs"""
    from probabilisticteacher_amd import ops
    counts = [len(p) for p in props_g]
    pb = torch.cat([p.proposal_boxes.tensor for p in props_g], 0).contiguous()
    roi_img = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32, device=DEV), ops.dev_i32(counts, DEV),
                                      output_size=sum(counts))
    hw = torch.tensor([[float(p.image_size[0]), float(p.image_size[1])] for p in props_g], device=DEV)
    return ops.roi_infer_prepare(deltas.to(DEV).contiguous(), pb, ops.softmax_rows(scores.to(DEV)), roi_img, hw,
                                 layer.num_classes, layer.box2box_transform.weights, layer.box2box_transform.scale_clamp,
                                 layer.test_score_thresh)


def _duplicates(keys, counts):
    """(R, K) bool: candidate entries (key >= 0) whose key occurs more than once among their image's candidates"""
    out = torch.zeros_like(keys, dtype=torch.bool)
    r0 = 0
    for c in counts:
        k = keys[r0:r0 + c]
        _, inv, cnt = torch.unique(k.reshape(-1), return_inverse=True, return_counts=True)
        out[r0:r0 + c] = (cnt[inv] > 1).view_as(k) & (k >= 0)
        r0 += c
    return out


def _make_scores_distinct(layer, gen, scores, deltas, props_g, thresh):
    """Nudge the sigma logits of entries whose rescored score collides with another candidate's of the same image -- on the host's
    restatement of the score (fast_rcnn.py:85,101) and on the device's keys -- until no two candidates of an image share a
    score on either side.  A sigma quadruple belongs to one (roi, class) entry, so nothing else moves.  Returns the device keys."""
    K, counts = layer.num_classes, [len(p) for p in props_g]
    R = scores.shape[0]
    for _ in range(12):
        p = torch.softmax(scores, -1)[:, :K]
        host = p * (1 - torch.sigmoid(deltas.view(R, K, 8)[..., 4:]).sum(-1) / 4.0)
        host = torch.where(p > thresh, host, torch.full_like(host, -1.0))
        dev_keys = _prepare(layer, scores, deltas, props_g)[1].cpu()
        dup = _duplicates(host, counts) | _duplicates(dev_keys, counts)
        if not dup.any():
            return dev_keys
        idx = dup.nonzero()
        deltas.view(R, K, 8)[idx[:, 0], idx[:, 1], 4:] += torch.randn(idx.shape[0], 4, generator=gen) * 0.05
    raise AssertionError("candidate scores could not be made pairwise distinct")


def _check_vs_oracle(layer, ocfg, scores, deltas, props_g, props_o):
    got, got_rows = layer.inference((scores.to(DEV), deltas.to(DEV)), props_g)
    ref, ref_rows = opt.roi_inference(ocfg, scores, deltas, props_o)
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert len(a) == len(b), f"image {i}: {len(a)} vs {len(b)} detections"
        assert torch.equal(got_rows[i].cpu(), ref_rows[i]), f"image {i}: kept ROI indices / order"
        assert torch.equal(a.pred_classes.cpu(), b.pred_classes), f"image {i}: classes"
        close(a.pred_boxes.tensor.cpu(), b.pred_boxes.tensor, 1e-5, 1e-4, "detection boxes")
        close(a.scores.cpu(), b.scores, 1e-5, 1e-7, "detection scores")
        assert torch.allclose(a.scores_logists.cpu(), b.scores_logists, rtol=0, atol=0, equal_nan=True), \
            "scores_logists are copies of input rows"
        assert torch.equal(a.boxes_sigma.cpu(), b.boxes_sigma), "boxes_sigma are copies of input entries"
    return ref


# ============================================================================ 1. the kernels
def test_kernels_against_torch_restatement():
    """K = 21, counts [130, 0, 65, 1]: segments that cross a 64 boundary, an empty image, a one-ROI image, an odd class count"""
    from probabilisticteacher_amd import ops
    K, counts, sizes = 21, [130, 0, 65, 1], [(600, 800), (600, 800), (512, 640), (480, 640)]
    n, R, max_r = len(counts), sum(counts), max(counts)
    gen = torch.Generator().manual_seed(21)
    scores, deltas, pg, _ = _roi_case(gen, K, counts, sizes)
    layer = _layer(K)
    boxes, keys, _, img_max, img_cnt, _ = _prepare(layer, scores, deltas, pg)
    roff = [0]
    for c in counts:
        roff.append(roff[-1] + c)
    cseg_h = ops.roi_class_seg_offsets(counts, K)
    cseg = ops.dev_i32(cseg_h, DEV)
    keys_h, boxes_h, max_h = keys.cpu(), boxes.cpu(), img_max.cpu()
    assert int((keys_h >= 0).sum()) == int(img_cnt.sum()) > 200

    # ---- class-major keys + candidate counts
    ckeys, ccnt = ops.roi_infer_class_keys(keys, cseg, n, K, max_r)
    want_keys = torch.cat([keys_h[roff[i]:roff[i + 1]].t().reshape(-1) for i in range(n)])
    want_cnt = torch.cat([(keys_h[roff[i]:roff[i + 1]] >= 0).sum(0) for i in range(n)]).int()
    assert torch.equal(ckeys.cpu(), want_keys) and torch.equal(ccnt.cpu(), want_cnt)
    assert want_cnt.view(n, K).sum(1).tolist() == img_cnt.cpu().tolist()

    # ---- the existing segmented sort over the n * K segments: stable, descending
    seg_len = [c for c in counts for _ in range(K)]
    csrt, corder = ops.segsort_desc(ckeys, cseg, max_len=max_r, lengths=seg_len)
    csrt_h, corder_h = csrt.cpu(), corder.cpu().long()
    for s in range(n * K):
        b, e = cseg_h[s], cseg_h[s + 1]
        v, ix = torch.sort(want_keys[b:e], descending=True, stable=True)
        assert torch.equal(csrt_h[b:e], v) and torch.equal(corder_h[b:e], ix)

    # ---- NMS boxes: offset trick below 40 000 candidates per image, unshifted from there on
    def want_nms_boxes(cnt_h):
        out = torch.empty(R * K, 4)
        for s in range(n * K):
            i, c = divmod(s, K)
            b, e = cseg_h[s], cseg_h[s + 1]
            off = torch.tensor(float(c)) * (max_h[i] + torch.tensor(1.0)) if cnt_h[i] < 40000 else torch.tensor(0.0)
            out[b:e] = boxes_h[roff[i] + corder_h[b:e], c] + off              # fp32, one rounding per operation
        return out
    nb = ops.roi_infer_class_nms_boxes(boxes, corder, cseg, img_max, img_cnt, n, K, max_r)
    assert torch.equal(nb.cpu(), want_nms_boxes(img_cnt.cpu().tolist()))
    fake = [40000, 0, 39999, 50000]
    nb2 = ops.roi_infer_class_nms_boxes(boxes, corder, cseg, img_max, ops.dev_i32(fake, DEV), n, K, max_r)
    assert torch.equal(nb2.cpu(), want_nms_boxes(fake))
    # ... and below 40 000 the bits ptmi_roi_infer_nms_boxes gives the same (roi, class) entry on the dense path
    seg_h = [K * o for o in roff]
    seg = ops.dev_i32(seg_h, DEV)
    _, dorder = ops.segsort_desc(keys.view(-1), seg, max_len=K * max_r, lengths=[K * c for c in counts])
    dnb = ops.roi_infer_nms_boxes(boxes, dorder, seg, img_max, K * max_r, K).cpu()
    by_entry = torch.empty(R * K, 4)
    for i in range(n):
        b, e = seg_h[i], seg_h[i + 1]
        by_entry[b + dorder.cpu().long()[b:e]] = dnb[b:e]
    by_entry = by_entry.view(R, K, 4)
    nb_h = nb.cpu()
    for s in range(n * K):
        i, c = divmod(s, K)
        b, e = cseg_h[s], cseg_h[s + 1]
        assert torch.equal(nb_h[b:e], by_entry[roff[i] + corder_h[b:e], c])

    # ---- collect: kept entries back to the dense (R, K) keys, kept count per image
    max_keep = 100
    keep, kcnt = ops.nms_batched(nb, cseg, max_r, 0.5, max_keep, seg_counts=ccnt)
    dense, img_kept = ops.roi_infer_class_collect(csrt, corder, keep, kcnt, cseg, n, K, max_r, R)
    keep_h, kcnt_h = keep.cpu().long(), kcnt.cpu().tolist()
    want_dense, want_kept = torch.full((R, K), -1.0), [0] * n
    for s in range(n * K):
        i, c = divmod(s, K)
        b = cseg_h[s]
        p = keep_h[s, :kcnt_h[s]]
        want_dense[roff[i] + corder_h[b + p], c] = csrt_h[b + p]
        want_kept[i] += kcnt_h[s]
    assert 0 < sum(kcnt_h) < int(img_cnt.sum()), "NMS kept some candidates and suppressed some"
    assert torch.equal(dense.cpu(), want_dense) and img_kept.cpu().tolist() == want_kept


# ============================================================================ 2. by class == dense
def _variant(name, gen, K, scores, deltas):
    opts = []
    if name == "nonfinite":                                # the finite filter's re-indexing quirk is live
        deltas[3, 2] = float("inf")
        deltas[140, 1] = float("nan")
        scores[150, 0] = float("nan")
    elif name == "peaked":                                 # a trained teacher: few candidates, fewer than 100 detections
        scores *= 0.2
        scores[:, K] += 6.0
        idx = torch.randperm(scores.shape[0], generator=gen)[:40]
        scores[idx, torch.randint(0, K, (40,), generator=gen)] += 9.0
    elif name == "top10":                                  # the per-image cut falls inside the kept list
        opts = ["TEST.DETECTIONS_PER_IMAGE", 10]
    elif name == "all":
        opts = ["TEST.DETECTIONS_PER_IMAGE", -1]
    return opts


@pytest.mark.parametrize("variant", ["plain", "nonfinite", "peaked", "top10", "all"])
@pytest.mark.parametrize("K", [1, 8, 21])
def test_by_class_equals_dense(K, variant):
    counts, sizes = [130, 65, 0, 1], [(600, 800), (512, 640), (600, 800), (480, 640)]
    gen = torch.Generator().manual_seed(100 + K)
    scores, deltas, pg, _ = _roi_case(gen, K, counts, sizes)
    opts = _variant(variant, gen, K, scores, deltas)
    sd, dd = scores.to(DEV), deltas.to(DEV)
    with _spy() as names:
        a, a_rows = _layer(K, *opts, by_class=True).inference((sd, dd), pg)
    assert all(s in names for s in NEW) and "ptmi_roi_infer_nms_boxes" not in names
    with _spy() as names:
        b, b_rows = _layer(K, *opts, by_class=False).inference((sd, dd), pg)
    assert "ptmi_roi_infer_nms_boxes" in names and not [s for s in NEW if s in names]
    lens = [len(x) for x in b]
    print(f"[by-class vs dense] K={K} {variant}: detections {lens}")
    assert lens[2] == 0 and sum(lens) > 0
    if variant == "peaked":
        assert all(x < 100 for x in lens)
    if variant == "top10" and K > 1:
        assert lens[0] == 10
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), f"image {i}: {len(x)} vs {len(y)} detections"
        assert torch.equal(a_rows[i], b_rows[i]), f"image {i}: kept rows"
        assert torch.equal(x.pred_boxes.tensor, y.pred_boxes.tensor), f"image {i}: pred_boxes"
        assert torch.equal(x.scores, y.scores), f"image {i}: scores"
        assert torch.equal(x.pred_classes, y.pred_classes), f"image {i}: pred_classes"
        assert torch.allclose(x.scores_logists, y.scores_logists, rtol=0, atol=0, equal_nan=True), f"image {i}: scores_logists"
        assert torch.equal(x.boxes_sigma, y.boxes_sigma), f"image {i}: boxes_sigma"


# ============================================================================ 3. K = 80 at full size
def test_k80_full_size_against_oracle_within_the_memory_law():
    from probabilisticteacher_amd.modeling.roi_heads import nms_ws_bytes_by_class, nms_ws_bytes_dense
    K, counts, sizes = 80, [2000, 1873], [(800, 1333), (800, 1200)]
    gen = torch.Generator().manual_seed(80)
    scores, deltas, pg, po = _roi_case(gen, K, counts, sizes, scale=2.0)
    layer = _layer(K)
    assert layer.nms_by_class is None and layer.test_score_thresh == 0.05
    keys = _make_scores_distinct(layer, gen, scores, deltas, pg, 0.05)
    assert not _duplicates(keys, counts).any()
    cand = [int((keys[:2000] >= 0).sum()), int((keys[2000:] >= 0).sum())]
    print(f"[K=80] candidates per image {cand}")
    assert all(5000 < c < 40000 for c in cand)
    sd, dd = scores.to(DEV), deltas.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with _spy() as names:
        layer.inference((sd, dd), pg)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"[K=80] peak device memory rise over inference(): {rise / 1e6:.1f} MB")
    assert all(s in names for s in NEW) and "ptmi_roi_infer_nms_boxes" not in names
    # between the two derived numbers: the by-class mask (82 MB) and the dense mask alone (6.4 GB)
    assert nms_ws_bytes_by_class(2, K, 2000) == 81_920_000 < 1e9 < nms_ws_bytes_dense(2, K, 2000) == 6_400_000_000
    assert rise < 1e9
    ref = _check_vs_oracle(layer, opt.Cfg(num_classes=K), scores, deltas, pg, po)
    assert all(len(r) == 100 for r in ref)


# ============================================================================ 4. the 40 000 rule
def test_40000_candidates_switch_to_unshifted_boxes():
    K, counts, sizes = 80, [2000, 400], [(800, 1333), (800, 1200)]
    gen = torch.Generator().manual_seed(40000)
    scores, deltas, pg, po = _roi_case(gen, K, counts, sizes, scale=0.1)
    layer = _layer(K, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.001)
    ocfg = opt.Cfg(num_classes=K, roi_score_thresh_test=0.001)
    keys = _make_scores_distinct(layer, gen, scores, deltas, pg, 0.001)
    assert not _duplicates(keys, counts).any()
    assert int((keys[:2000] >= 0).sum()) == 160000 and int((keys[2000:] >= 0).sum()) == 32000, "one image on each branch"
    with _spy() as names:
        ref = _check_vs_oracle(layer, ocfg, scores, deltas, pg, po)
    assert all(s in names for s in NEW)
    assert all(len(r) == 100 for r in ref)


# ============================================================================ 5. the shipped class count
def test_k8_default_launches_what_it_launched():
    K, counts, sizes = 8, [2000, 1873], [(800, 1333), (800, 1200)]
    gen = torch.Generator().manual_seed(7)
    scores, deltas, pg, _ = _roi_case(gen, K, counts, sizes)
    layer = _layer(K)
    with _spy() as names:
        got, _ = layer.inference((scores.to(DEV), deltas.to(DEV)), pg)
    assert names == ["ptmi_softmax_rows", "ptmi_roi_infer_prepare", "ptmi_segsort_topk_desc", "ptmi_roi_infer_nms_boxes",
                     "ptmi_nms_batched"], names
    assert all(len(g) == 100 for g in got)


# ============================================================================ 6. a 20-class mutual-learning step
def test_20_class_mutual_learning_step_twice(monkeypatch):
    from bench import synth_records
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.modeling.roi_heads import GuassianFastRCNNOutputLayers
    from probabilisticteacher_amd.seeding import seed_all_rng
    K = 20
    cfg = _cfg(K, "MODEL.ANCHOR_GENERATOR.NAME", "DifferentiableAnchorGenerator", "UNSUPNET.BURN_UP_STEP", 0,
               "SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1, "SEED", 0)
    # a 192 x 256 image yields a few hundred proposals, fewer than the 820 at which 20 classes leave the dense path on their
    # own: the path is forced, for the teacher and the student alike
    monkeypatch.setattr(GuassianFastRCNNOutputLayers, "nms_by_class", True)
    from probabilisticteacher_amd.modeling import roi_heads
    seen, rule = [], roi_heads.select_nms_by_class
    monkeypatch.setattr(roi_heads, "select_nms_by_class", lambda k, counts, flag=None: seen.append((k, list(counts), flag)) or
                        rule(k, counts, flag))
    gen = torch.Generator().manual_seed(20)
    batch = tuple(synth_records(gen, 1, 192, 256, K, DEV) for _ in range(4))
    runs = []
    for _ in range(2):
        seed_all_rng(0)
        tr = PTrainer(cfg)
        with _spy() as names:
            m = dict(tr.run_step(batch))
        torch.cuda.synchronize()
        m.pop("data_time", None)
        assert all(s in names for s in NEW) and "ptmi_roi_infer_nms_boxes" not in names, "by-class path taken"
        print(f"[20-class step] teacher inference: (K, proposals per image, forced) = {seen[-1]}")
        assert seen[-1][0] == K and seen[-1][2] is True
        losses = {k: v for k, v in m.items() if "loss" in k}
        assert len(losses) >= 4 and any(k.endswith("_unsup") for k in losses) and all(math.isfinite(v) for v in losses.values()), m
        runs.append((tr, m))
    (ta, ma), (tb, mb) = runs
    assert ma.keys() == mb.keys() and not {k: (ma[k], mb[k]) for k in ma if not (ma[k] == mb[k])}
    assert torch.equal(ta.student.flat, tb.student.flat) and torch.equal(ta.teacher.flat, tb.teacher.flat)
