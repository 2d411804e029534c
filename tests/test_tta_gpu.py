"""GPU (pytest -m gpu): test-time augmentation (TEST.AUG) -- the two HIP kernels of csrc/tta.hip, ops.tta_merge, the
GeneralizedRCNNWithTTA wrapper and PTrainer.test_with_TTA -- against tests/tta_ref.py, the literal CPU restatement of
detectron2 0.5's DatasetMapperTTA / _inverse_boxes / _merge_detections.  Every comparison is exact (torch.equal)."""
import os

import numpy as np
import pytest
import torch

from tests import tta_ref
from tests.test_host_logic import _write_voc_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
SIZES_18 = (80, 96, 101, 115, 128, 141, 160, 200, 230)          # x flip = 18 augmentations


# ---------------------------------------------------------------------------- shared builders
def _rows_of(img, plan):
    """ops' per-augmentation rows from the restatement's plan (float32 factors -> Python floats, exactly)"""
    return [(img, flipped, float(size[1]), float(fx), float(fy), float(gx), float(gy), pre)
            for size, flipped, fx, fy, gx, gy, pre in plan]


def _random_boxes(rng, n, hs, ws):
    """boxes in the augmented image's coordinates, partly outside it on every side"""
    x1 = rng.uniform(-0.2 * ws, 1.0 * ws, n)
    y1 = rng.uniform(-0.2 * hs, 1.0 * hs, n)
    bw = rng.uniform(1.0, 0.5 * ws, n)
    bh = rng.uniform(1.0, 0.5 * hs, n)
    return np.stack([x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32)


def _special_rows(boxes, scores):
    """the rows the finite filter, the strict threshold and the per-step min / max exist for (an augmentation of 100 rows)"""
    boxes[3, 1] = np.nan
    scores[5] = np.inf
    scores[7] = np.float32(1e-8)                 # == the threshold as fp32: dropped, the comparison is strict
    boxes[9, 2] = np.inf
    scores[11] = 0.0
    boxes[13] = boxes[13][[2, 1, 0, 3]]          # x1 > x2: apply_box's min / max puts it right
    boxes[15, 2] = 3e38                          # finite, but a factor > 1 takes it to inf
    scores[17] = np.nan
    boxes[19, 0] = -np.inf


def _reference(images, per_image_augs, thr, topk):
    """per image: tta_ref.merge over its augmentations -> kept (boxes, scores, classes), info, mapped boxes before the filters"""
    out = []
    for (h, w, H, W), augs in zip(images, per_image_augs):
        per_aug = [(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(c)) for _, b, s, c in augs]
        out.append(tta_ref.merge(per_aug, [t for t, _, _, _ in augs], (H, W), thr, topk))
    return out


def _flatten(images, per_image_augs, plans):
    rows, counts, boxes, scores, classes = [], [], [], [], []
    for i, (augs, plan) in enumerate(zip(per_image_augs, plans)):
        rows += _rows_of(i, plan)
        for _, b, s, c in augs:
            counts.append(len(s))
            boxes.append(torch.from_numpy(b))
            scores.append(torch.from_numpy(s))
            classes.append(torch.from_numpy(c))
    sizes = [(H, W) for _, _, H, W in images]
    return rows, counts, torch.cat(boxes).to(DEV), torch.cat(scores).to(DEV), torch.cat(classes).to(DEV), sizes


# ---------------------------------------------------------------------------- a. mapping bits
GEOM_PRE = [(112, 160, 224, 320), (160, 224, 171, 240), (224, 160, 448, 320)]      # the second: no factor is an fp32 number
GEOM_SAME = [(160, 224, 160, 224), (101, 141, 101, 141), (224, 160, 224, 160)]
COUNT_CYCLES = [[100, 0, 1], [0, 0, 0], [1, 100, 0]]            # image 1: every augmentation empty


@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("naug", [1, 2, 18])
@pytest.mark.parametrize("nimg", [1, 3])
def test_map_boxes_bits(nimg, naug, pre):
    from probabilisticteacher_amd import ops
    rng = np.random.RandomState(100 * nimg + naug + (7 if pre else 0))
    min_sizes, flip = {1: ((101,), False), 2: ((101,), True), 18: (SIZES_18, True)}[naug]
    images = (GEOM_PRE if pre else GEOM_SAME)[:nimg]
    plans, per_image_augs = [], []
    for i, (h, w, H, W) in enumerate(images):
        augs = tta_ref.augmentations(h, w, H, W, min_sizes, 4000, flip)
        plans.append(tta_ref.plan(h, w, H, W, min_sizes, 4000, flip))
        cyc = COUNT_CYCLES[i] if nimg == 3 else [100, 0, 1]
        mine = []
        for a, ((hs, ws), _, tfms) in enumerate(augs):
            n = cyc[a % 3]
            b = _random_boxes(rng, n, hs, ws)
            s = rng.uniform(0.01, 1.0, n).astype(np.float32)
            if n == 100:
                _special_rows(b, s)
            mine.append((tfms, b, s, rng.randint(0, 8, n).astype(np.int64)))
        per_image_augs.append(mine)
    assert len(plans[0]) == naug
    ref = _reference(images, per_image_augs, 0.5, 100)
    rows, counts, boxes, scores, classes, sizes = _flatten(images, per_image_augs, plans)
    assert 0 in counts or (nimg, naug) == (1, 1), "an empty augmentation is part of every larger case"
    got_b, got_k, got_max, got_cnt = ops.tta_map_boxes(boxes, scores, rows, counts, sizes)
    torch.cuda.synchronize()
    exp_b, exp_k, exp_max, exp_cnt, nspecial = [], [], [], [], 0
    for (_, _, _, info, mapped), augs in zip(ref, per_image_augs):
        valid, cand = info["valid"], info["candidate"]
        sc = torch.cat([torch.from_numpy(s) for _, _, s, _ in augs])
        eb = torch.zeros((len(valid), 4))
        eb[valid] = info["clipped"]                              # (a row the finite filter drops comes back as zeros)
        exp_b.append(eb)
        exp_k.append(torch.where(cand, sc, torch.full_like(sc, NINF)))
        exp_max.append(float(info["max_coordinate"]))
        exp_cnt.append(int(cand.sum()))
        nspecial += int((~valid).sum())
        if len(valid) >= 100:
            assert not torch.equal(mapped[valid], info["clipped"]), "the clip acts on some box"
    assert torch.equal(got_b.cpu(), torch.cat(exp_b)), "mapped + clipped boxes, bit for bit"
    assert torch.equal(got_k.cpu(), torch.cat(exp_k)), "sort keys: score of a candidate, -inf otherwise"
    assert got_cnt.cpu().tolist() == exp_cnt
    assert torch.equal(got_max.cpu(), torch.tensor(exp_max, dtype=torch.float32)), "max coordinate over the candidates"
    if nimg == 3:
        assert exp_cnt[1] == 0 and exp_max[1] == 0.0
    if 100 in counts:
        assert nspecial >= 6, "NaN / inf rows were part of the input"


def test_map_boxes_is_repeatable_and_empty_input_launches_nothing_but_the_clears():
    from probabilisticteacher_amd import ops
    rng = np.random.RandomState(5)
    plan = tta_ref.plan(112, 160, 224, 320, (96, 128), 4000, True)
    counts = [100, 100, 100, 100]
    boxes = torch.from_numpy(np.concatenate([_random_boxes(rng, 100, s[0], s[1]) for s, *_ in plan])).to(DEV)
    scores = torch.from_numpy(rng.uniform(0.01, 1, 400).astype(np.float32)).to(DEV)
    a = ops.tta_map_boxes(boxes, scores, _rows_of(0, plan), counts, [(224, 320)])
    b = ops.tta_map_boxes(boxes, scores, _rows_of(0, plan), counts, [(224, 320)])
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "integer atomics only: the same bits on every run"
    e = ops.tta_map_boxes(boxes[:0], scores[:0], _rows_of(0, plan), [0, 0, 0, 0], [(224, 320)])
    assert e[0].shape == (0, 4) and e[2].tolist() == [0.0] and e[3].tolist() == [0]
    with pytest.raises(ValueError, match="grouped by image"):
        ops.tta_map_boxes(boxes, scores, _rows_of(1, plan[:2]) + _rows_of(0, plan[2:]), counts, [(224, 320)] * 2)
    with pytest.raises(ValueError, match="400"):
        ops.tta_map_boxes(boxes, scores, _rows_of(0, plan), [100, 100, 100, 99], [(224, 320)])


# ---------------------------------------------------------------------------- b. merge
def _iou64(b):
    b = b.double()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt, rb = torch.max(b[:, None, :2], b[None, :, :2]), torch.min(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area[:, None] + area[None, :] - inter
    return torch.where(union > 0, inter / union, torch.zeros_like(inter))


def _inputs_are_decidable(info, thr, margin, unique_scores=True):
    """the condition under which an exact comparison is fair, checked on the CPU in float64 before the GPU is touched: no
    same-class pair of candidates with an IoU within `margin` of the threshold (the fp32 IoU of shifted boxes may differ from it
    in the last bits), and no two candidates of the image with one score"""
    b, s, c = info["cand_boxes"], info["cand_scores"], info["cand_classes"]
    if len(s) < 2:
        return True
    iou = _iou64(b)
    same = (c[:, None] == c[None, :]) & ~torch.eye(len(c), dtype=torch.bool)
    if bool(((iou - thr).abs() <= margin)[same].any()):
        return False
    return not unique_scores or len(torch.unique(s)) == len(s)


MERGE_GEOM = [(112, 160, 224, 320), (160, 224, 160, 224)]


def _merge_inputs(seed, k, per_aug=40, min_sizes=(96, 128)):
    """two images x four augmentations: jittered copies of a few seed boxes per image (as the flipped twin of a detection is
    in practice), drawn in original coordinates and taken into each augmentation's own coordinates.  A copy has its seed's
    class -- most of the time: at 80 classes mostly not, so that more than 100 detections survive the NMS"""
    rng = np.random.RandomState(seed)
    p_seed_class = 0.85 if k < 80 else 0.2
    plans, per_image_augs = [], []
    for h, w, H, W in MERGE_GEOM:
        augs = tta_ref.augmentations(h, w, H, W, min_sizes, 4000, True)
        plan = tta_ref.plan(h, w, H, W, min_sizes, 4000, True)
        nseed = 6
        sx1, sy1 = rng.uniform(0, 0.6 * W, nseed), rng.uniform(0, 0.6 * H, nseed)
        seeds = np.stack([sx1, sy1, sx1 + rng.uniform(0.15 * W, 0.4 * W, nseed), sy1 + rng.uniform(0.15 * H, 0.4 * H, nseed)], 1)
        seed_cls = rng.randint(0, k, nseed)
        mine = []
        for ((hs, ws), flipped, tfms), (_, _, fx, fy, gx, gy, _) in zip(augs, plan):
            which = rng.randint(0, nseed, per_aug)
            b = seeds[which] + rng.uniform(-8, 8, (per_aug, 4))
            b[:, 0::2] /= float(fx) * float(gx)
            b[:, 1::2] /= float(fy) * float(gy)
            if flipped:
                b[:, 0::2] = ws - b[:, [2, 0]]
            cls = np.where(rng.rand(per_aug) < p_seed_class, seed_cls[which], rng.randint(0, k, per_aug)).astype(np.int64)
            s = rng.uniform(0.05, 0.98, per_aug).astype(np.float32)
            s[1], s[2] = 0.0, np.float32(1e-8)                     # non-candidates sit among the candidates
            b = b.astype(np.float32)
            b[4, 3] = np.nan
            mine.append((tfms, b, s, cls))
        plans.append(plan)
        per_image_augs.append(mine)
    return plans, per_image_augs


def _decidable_merge_inputs(k, thr, unique_scores=True, edit=None):
    for seed in range(5):
        plans, augs = _merge_inputs(1000 * k + seed, k)
        if edit is not None:
            edit(augs)
        ref = _reference(MERGE_GEOM, augs, thr, -1)
        if all(_inputs_are_decidable(r[3], thr, 1e-5, unique_scores) for r in ref):
            return plans, augs
    pytest.fail("five seeds in a row gave an IoU within 1e-5 of the threshold or a repeated score")


def _run_merge(plans, augs, thr, det):
    from probabilisticteacher_amd import ops
    rows, counts, boxes, scores, classes, sizes = _flatten(MERGE_GEOM, augs, plans)
    return ops.tta_merge(boxes, scores, classes, rows, counts, sizes, thr, det)


@pytest.mark.parametrize("det", [100, 5, -1])
@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("k", [1, 8, 80])
def test_merge_matches_the_restatement(k, thr, det):
    plans, augs = _decidable_merge_inputs(k, thr)
    ref = _reference(MERGE_GEOM, augs, thr, det)
    got = _run_merge(plans, augs, thr, det)
    assert len(got) == len(ref) == 2
    for (gb, gs, gc), (rb, rs, rc, info, _) in zip(got, ref):
        print(f"k={k} thr={thr} det={det}: {int(info['candidate'].sum())} candidates of {len(info['candidate'])}, kept {len(rs)}")
        assert len(rs) > 0 and len(rs) < int(info["candidate"].sum()), "the NMS or the cap removed something"
        assert gc.dtype == torch.int64
        assert torch.equal(gb.cpu(), rb) and torch.equal(gs.cpu(), rs) and torch.equal(gc.cpu(), rc)
    if det == 5 and k > 1:
        assert all(len(g[1]) == 5 for g in got), "the cap of 5 acts"
    if det == 100 and k == 80:
        assert all(len(g[1]) == 100 for g in got) and all(len(r[1]) > 100 for r in _reference(MERGE_GEOM, augs, thr, -1)), \
            "the cap of 100 acts"


def test_merge_of_a_long_segment_takes_the_radix_sort():
    """an image with more than 16 384 detections over its augmentations (nearly all of them below the score threshold): the
    segmented sort leaves its LDS kernel for rocPRIM's; the merge is the same"""
    from probabilisticteacher_amd import _lib

    def edit(per_image_augs):
        tfms, b, s, c = per_image_augs[1][3]
        rng = np.random.RandomState(9)
        n = 16400
        per_image_augs[1][3] = (tfms, np.concatenate([_random_boxes(rng, n, 128, 179), b]),
                                np.concatenate([np.zeros(n, dtype=np.float32), s]),
                                np.concatenate([rng.randint(0, 8, n).astype(np.int64), c]))
    plans, augs = _decidable_merge_inputs(8, 0.5, edit=edit)
    ref = _reference(MERGE_GEOM, augs, 0.5, 100)
    names, call = [], _lib.call

    def spy(name, *a):
        names.append(name)
        return call(name, *a)
    _lib.call = spy
    try:
        got = _run_merge(plans, augs, 0.5, 100)
    finally:
        _lib.call = call
    assert names == ["ptmi_tta_map_boxes", "ptmi_segsort_desc", "ptmi_tta_nms_boxes", "ptmi_nms_batched"]
    for (gb, gs, gc), (rb, rs, rc, info, _) in zip(got, ref):
        assert len(rs) > 0 and torch.equal(gb.cpu(), rb) and torch.equal(gs.cpu(), rs) and torch.equal(gc.cpu(), rc)
    assert len(ref[1][3]["candidate"]) > 16384


def test_merge_breaks_score_ties_by_position():
    """the one case with repeated scores: identical boxes (IoU 1, far from the threshold) with one score -- of one class (the
    first stays) and of two classes (both stay); the rest of the input is the decidable cluster set"""
    def edit(per_image_augs):
        _, b, s, c = per_image_augs[0][1]
        b[10] = b[11] = b[12] = np.array([20, 10, 60, 40], dtype=np.float32)
        s[10] = s[11] = s[12] = np.float32(0.99)
        c[10], c[11], c[12] = 3, 3, 5
        _, b2, s2, c2 = per_image_augs[0][3]                   # the same score again in a later augmentation, elsewhere
        b2[10], s2[10], c2[10] = np.array([5, 30, 25, 50], dtype=np.float32), np.float32(0.99), 3
    plans, augs = _decidable_merge_inputs(8, 0.5, unique_scores=False, edit=edit)
    ref = _reference(MERGE_GEOM, augs, 0.5, 100)
    got = _run_merge(plans, augs, 0.5, 100)
    for (gb, gs, gc), (rb, rs, rc, _, _) in zip(got, ref):
        assert torch.equal(gb.cpu(), rb) and torch.equal(gs.cpu(), rs) and torch.equal(gc.cpu(), rc)
    top = got[0][1].cpu() == np.float32(0.99)
    assert int(top.sum()) == 3 and got[0][2].cpu()[top].tolist() == [3, 5, 3], "first of class 3, class 5, then the later one"


def test_merge_launch_count_does_not_grow():
    """the merged batch is four entry points and one host read whatever the number of augmentations or detections"""
    from probabilisticteacher_amd import _lib
    seen = []
    for min_sizes, per_aug in (((96,), 20), (SIZES_18, 40)):
        rng_plans, augs = _merge_inputs(3, 8, per_aug=per_aug, min_sizes=min_sizes)
        names, call = [], _lib.call

        def spy(name, *a):
            names.append(name)
            return call(name, *a)
        _lib.call = spy
        try:
            _run_merge(rng_plans, augs, 0.5, 100)
        finally:
            _lib.call = call
        seen.append(names)
    assert seen[0] == seen[1] == ["ptmi_tta_map_boxes", "ptmi_segsort_topk_desc", "ptmi_tta_nms_boxes", "ptmi_nms_batched"]


def test_merge_of_nothing():
    from probabilisticteacher_amd import ops
    plan = tta_ref.plan(160, 224, 160, 224, (96,), 4000, True)
    z = torch.zeros((0, 4), device=DEV)
    out = ops.tta_merge(z, z[:, 0], torch.zeros(0, dtype=torch.int64, device=DEV), _rows_of(0, plan), [0, 0], [(160, 224)], 0.5, 100)
    assert len(out) == 1 and out[0][0].shape == (0, 4) and out[0][1].shape == (0,) and out[0][2].dtype == torch.int64
    # detections, but no candidate: every score at or below the threshold
    b = torch.tensor([[1.0, 1.0, 9.0, 9.0]] * 2, device=DEV)
    out = ops.tta_merge(b, torch.zeros(2, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), _rows_of(0, plan), [1, 1],
                        [(160, 224)], 0.5, 100)
    assert out[0][0].shape == (0, 4) and out[0][1].shape == (0,)


# ---------------------------------------------------------------------------- the model
def _model_cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg("configs/pt/final_s2c.yaml", ["MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", ""] + list(opts))


@pytest.fixture(scope="module")
def model():
    from probabilisticteacher_amd import modeling
    torch.manual_seed(0)
    return modeling.build_model(_model_cfg()).eval()


def _image(seed, h, w):
    return torch.randint(0, 256, (3, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).to(DEV)


def _fields(inst):
    return inst.pred_boxes.tensor.cpu(), inst.scores.cpu(), inst.pred_classes.cpu()


# ---------------------------------------------------------------------------- c. identity
def test_one_unflipped_augmentation_of_the_same_size_is_plain_inference(model):
    from probabilisticteacher_amd.modeling.tta import GeneralizedRCNNWithTTA
    cfg = _model_cfg("TEST.AUG.MIN_SIZES", (160,), "TEST.AUG.FLIP", False)
    thr = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
    tta = GeneralizedRCNNWithTTA(cfg, model)
    for seed in range(5):
        rec = {"image": _image(seed, 160, 224), "height": 160, "width": 224}
        with torch.no_grad():
            plain = model.inference([rec])[0]["instances"]
        pb, ps, pc = _fields(plain)
        assert len(ps) > 1
        iou = _iou64(pb)
        same = (pc[:, None] == pc[None, :]) & ~torch.eye(len(pc), dtype=torch.bool)
        if bool(((iou - thr).abs() <= 1e-4)[same].any()):
            continue                      # the class offset differs between the two NMS passes: such a pair may go either way
        out = tta([rec])[0]["instances"]
        assert out.image_size == (160, 224) and set(out.get_fields()) == {"pred_boxes", "scores", "pred_classes"}
        out = out[out.pred_boxes.nonempty()]                     # plain inference's non-empty filter
        tb, ts, tc = _fields(out)
        assert torch.equal(tb, pb) and torch.equal(ts, ps) and torch.equal(tc, pc)
        return
    pytest.fail("five seeds in a row kept a same-class pair with an IoU within 1e-4 of NMS_THRESH_TEST")


# ---------------------------------------------------------------------------- d. orchestration
def _by_hand(model, rec, min_sizes, thr, det):
    """the wrapper's work spelled out: resize_batch / hflip_batch, one inference call per size, tta_ref on the CPU"""
    from probabilisticteacher_amd.data.augment import hflip_batch, resize_batch
    img = rec["image"]
    h, w = img.shape[-2:]
    H, W = rec["height"], rec["width"]
    augs = tta_ref.augmentations(h, w, H, W, min_sizes, 4000, True)
    per_aug = []
    for s in min_sizes:
        size = tta_ref.shortest_edge_size(h, w, s, 4000)
        resized = resize_batch([img], [size])[0]
        flipped = hflip_batch([resized], [True])[0]
        assert tuple(resized.shape[-2:]) == size
        with torch.no_grad():
            for res in model.inference([{"image": resized}, {"image": flipped}], do_postprocess=False):
                assert res.image_size == size, "augmented-image coordinates"
                per_aug.append(_fields(res))
    assert [a[0] for a in augs] == [tta_ref.shortest_edge_size(h, w, s, 4000) for s in min_sizes for _ in range(2)]
    return tta_ref.merge(per_aug, [t for _, _, t in augs], (H, W), thr, det)


def test_wrapper_equals_the_steps_by_hand(model):
    from probabilisticteacher_amd.modeling.tta import GeneralizedRCNNWithTTA
    cfg = _model_cfg("TEST.AUG.MIN_SIZES", (96, 128), "TEST.AUG.FLIP", True)
    tta = GeneralizedRCNNWithTTA(cfg, model)
    thr, det = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, cfg.TEST.DETECTIONS_PER_IMAGE
    rec = {"image": _image(11, 112, 160), "height": 224, "width": 320}
    rb, rs, rc, info, _ = _by_hand(model, rec, (96, 128), thr, det)
    out = tta([rec])[0]["instances"]
    gb, gs, gc = _fields(out)
    print(f"orchestration: {len(info['candidate'])} detections over 4 augmentations, {len(rs)} kept")
    assert out.image_size == (224, 320) and len(rs) > 0
    assert torch.equal(gb, rb) and torch.equal(gs, rs) and torch.equal(gc, rc)
    # a batch of two records of different sizes: each record's result is its single-record result
    rec2 = {"image": _image(12, 160, 224), "height": 160, "width": 224}
    both = tta([rec, rec2])
    single2 = tta([rec2])[0]["instances"]
    assert both[1]["instances"].image_size == (160, 224)
    for got, want in ((both[0]["instances"], out), (both[1]["instances"], single2)):
        assert all(torch.equal(a, b) for a, b in zip(_fields(got), _fields(want)))
    rb2, rs2, rc2, _, _ = _by_hand(model, rec2, (96, 128), thr, det)
    assert all(torch.equal(a, b) for a, b in zip(_fields(single2), (rb2, rs2, rc2)))


# ---------------------------------------------------------------------------- e. end to end
def _spy_test(cfg, model):
    from probabilisticteacher_amd import _lib
    from probabilisticteacher_amd.engine import PTrainer
    names, call = [], _lib.call

    def spy(name, *a):
        names.append(name)
        return call(name, *a)
    _lib.call = spy
    try:
        res = PTrainer.test(cfg, model)
    finally:
        _lib.call = call
    return names, res


def test_test_with_tta_end_to_end(tmp_path, model):
    from probabilisticteacher_amd.data import datasets
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.modeling.meta_arch import detector_postprocess
    _write_voc_dir(str(tmp_path / "val"), [f"val{i}" for i in range(3)], ("car",), np.random.RandomState(4), h=160, w=224)
    os.rename(tmp_path / "val" / "ImageSets" / "Main" / "train.txt", tmp_path / "val" / "ImageSets" / "Main" / "split.txt")
    datasets.register_pascal_voc("tta_val", str(tmp_path / "val"), "split", ("car",))
    base = ["DATASETS.TEST", ("tta_val",), "INPUT.MIN_SIZE_TEST", 128, "INPUT.MAX_SIZE_TEST", 320, "DATALOADER.NUM_WORKERS", 0]
    cfg = _model_cfg(*base, "TEST.AUG.ENABLED", True, "TEST.AUG.MIN_SIZES", (96, 128), "TEST.AUG.MAX_SIZE", 320)
    for mode in (True, False):
        model.train(mode)
        res = PTrainer.test_with_TTA(cfg, model)
        assert model.training is mode, "the model's mode is restored"
        assert set(res) == {"bbox_TTA", "per_class_AP50_TTA"}, "every top-level key of the evaluator's results, suffixed"
        assert set(res["bbox_TTA"]) == {"AP", "AP50", "AP75"} and set(res["per_class_AP50_TTA"]) == {"car"}
        assert all(0.0 <= v <= 100.0 for v in res["bbox_TTA"].values()), res
    # TEST.AUG.ENABLED False: PTrainer.test launches what it launches on a config whose TEST.AUG node nobody touched
    off = _model_cfg(*base, "TEST.AUG.ENABLED", False, "TEST.AUG.MIN_SIZES", (96, 128), "TEST.AUG.FLIP", False)
    names_off, res_off = _spy_test(off, model)
    names_plain, res_plain = _spy_test(_model_cfg(*base), model)
    assert names_off == names_plain and len(names_plain) > 0 and res_off == res_plain
    assert set(res) == {k + "_TTA" for k in res_plain}
    assert not [n for n in names_plain if "tta" in n]
    # ... and with ENABLED the plain evaluation is still the plain evaluation
    names_on, res_on = _spy_test(cfg, model)
    assert names_on == names_plain and res_on == res_plain
    # model.inference(batch) without the new keyword: do_postprocess=False followed by detector_postprocess
    model.eval()
    rec = {"image": _image(21, 112, 160), "height": 224, "width": 320}
    with torch.no_grad():
        plain = model.inference([rec])[0]["instances"]
        raw = model.inference([rec], do_postprocess=False)
    assert isinstance(raw, list) and len(raw) == 1 and raw[0].image_size == (112, 160)
    post = detector_postprocess(raw[0], 224, 320)
    assert plain.image_size == (224, 320) and len(plain.scores) > 0
    assert all(torch.equal(a, b) for a, b in zip(_fields(plain), _fields(post)))
    assert torch.equal(plain.boxes_sigma, post.boxes_sigma) and torch.equal(plain.scores_logists, post.scores_logists)
