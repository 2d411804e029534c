"""CPU: the COCO-format reader and the host half of the COCO evaluator (packing, accumulate, summarize) against the literal
restatement of pycocotools in tests/coco_eval_ref.py.  The matching kernel itself is tests/test_coco_eval_gpu.py's; here the
evaluator is fed the reference's match tables, so no GPU is needed."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import coco_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(image_id, gt_xywh, gt_cls, crowd=None, area=None, h=480, w=640):
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    g = np.asarray(gt_xywh, dtype=np.float64).reshape(-1, 4)
    inst = FreeInstances((h, w))
    inst.gt_boxes = Boxes(torch.tensor(np.stack([g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]], 1), dtype=torch.float32))
    inst.gt_classes = torch.tensor(gt_cls, dtype=torch.int64)
    if crowd is not None:
        inst.set("iscrowd", torch.tensor(crowd, dtype=torch.int32))
    if area is not None:
        inst.set("area", torch.tensor(area, dtype=torch.float64))
    return {"image_id": image_id, "height": h, "width": w, "instances": inst}


def _output(dt_xywh, scores, classes, h=480, w=640):
    from probabilisticteacher_amd.structures import Boxes, Instances
    d = np.asarray(dt_xywh, dtype=np.float64).reshape(-1, 4)
    inst = Instances((h, w))
    inst.pred_boxes = Boxes(torch.tensor(np.stack([d[:, 0], d[:, 1], d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]], 1), dtype=torch.float32))
    inst.scores = torch.tensor(scores, dtype=torch.float32)
    inst.pred_classes = torch.tensor(classes, dtype=torch.int64)
    return {"instances": inst}


def _ref_tables(packed, segments):
    """the reference's match tables in the evaluator's segment order (segment = category * n_img + image)"""
    n_img, n_cat = packed["n_img"], packed["n_cat"]
    return ref.match_tables([segments.get((i, k)) for k in range(n_cat) for i in range(n_img)])


# ------------------------------------------------------------------------------------------------------------------ reader
def _write_coco_json(path, with_annotations=True):
    data = {"images": [{"id": 30, "file_name": "c.jpg", "height": 100, "width": 200},
                       {"id": 7, "file_name": "a.jpg", "height": 120, "width": 160},
                       {"id": 19, "file_name": "b.jpg", "height": 90, "width": 110}],
            "categories": [{"id": 90, "name": "toothbrush"}, {"id": 3, "name": "car"}, {"id": 17, "name": "cat"}]}
    if with_annotations:
        data["annotations"] = [
            {"id": 1, "image_id": 7, "category_id": 17, "bbox": [10.5, 20.25, 30.0, 40.5], "area": 600.0, "iscrowd": 0},
            {"id": 2, "image_id": 7, "category_id": 3, "bbox": [1.0, 2.0, 100.0, 50.0], "area": 4000.0, "iscrowd": 1},
            {"id": 3, "image_id": 30, "category_id": 90, "bbox": [0.0, 0.0, 8.0, 8.0], "iscrowd": 0},
        ]                                                     # image 19 has no annotation; annotation 3 has no area
    with open(path, "w") as f:
        json.dump(data, f)


def test_coco_json_reader_registration_and_mapper_input(tmp_path):
    from probabilisticteacher_amd.data import datasets
    jf = str(tmp_path / "instances.json")
    _write_coco_json(jf)
    datasets.register_coco_instances("cc_tiny", jf, str(tmp_path / "img"))
    dicts = datasets.get_dataset_dicts(["cc_tiny"])
    assert [d["image_id"] for d in dicts] == [7, 19, 30], "images sorted by id"
    assert dicts[0]["file_name"] == os.path.join(str(tmp_path / "img"), "a.jpg") and (dicts[0]["height"], dicts[0]["width"]) == (120, 160)
    meta = datasets.metadata("cc_tiny")
    assert meta["thing_classes"] == ["car", "cat", "toothbrush"]
    assert meta["thing_dataset_id_to_contiguous_id"] == {3: 0, 17: 1, 90: 2}
    assert meta["evaluator_type"] == "coco" and meta["json_file"] == jf and meta["image_root"] == str(tmp_path / "img")
    a0, a1 = dicts[0]["annotations"]
    assert a0 == {"category_id": 1, "bbox": [10.5, 20.25, 40.5, 60.75], "bbox_xywh": [10.5, 20.25, 30.0, 40.5], "iscrowd": 0,
                  "area": 600.0}
    assert a1["category_id"] == 0 and a1["iscrowd"] == 1 and a1["bbox"] == [1.0, 2.0, 101.0, 52.0] and a1["area"] == 4000.0
    assert dicts[1]["annotations"] == []
    assert dicts[2]["annotations"][0]["category_id"] == 2 and dicts[2]["annotations"][0]["area"] == 64.0
    assert len(datasets.get_dataset_dicts(["cc_tiny"], filter_empty=True)) == 2
    img = torch.zeros((3, 120, 160), dtype=torch.uint8)
    train = datasets.to_mapper_input(dicts[0], image=img)
    assert train["boxes"].tolist() == [[10.5, 20.25, 40.5, 60.75]] and train["classes"].tolist() == [1], "the crowd box is dropped"
    assert "iscrowd" not in train and "area" not in train and train["difficult"].tolist() == [False]
    test = datasets.to_mapper_input(dicts[0], image=img, is_train=False)
    assert test["classes"].tolist() == [1, 0] and test["iscrowd"].tolist() == [0, 1] and test["area"].tolist() == [600.0, 4000.0]
    # a json without `annotations` (the reference's coco_2017_unlabel): records without the key
    jf2 = str(tmp_path / "image_info.json")
    _write_coco_json(jf2, with_annotations=False)
    unl = datasets.load_coco_json(jf2, "root")
    assert len(unl) == 3 and all("annotations" not in d for d in unl)
    assert "boxes" not in datasets.to_mapper_input(unl[0], image=img)
    # the reference's two COCO-format splits are registered under $DETECTRON2_DATASETS
    assert {"coco_2017_unlabel", "coco_2017_for_voc20"} <= set(datasets._DATASETS)
    assert datasets._METADATA["coco_2017_unlabel"]["json_file"].endswith("coco/annotations/image_info_unlabeled2017.json")


def test_voc_mapper_input_is_unchanged_for_test_records(tmp_path):
    from probabilisticteacher_amd.data import datasets
    d = {"file_name": "x.jpg", "image_id": "x", "annotations": [{"category_id": 0, "bbox": [1.0, 2.0, 3.0, 4.0], "difficult": 1}]}
    img = torch.zeros((3, 8, 8), dtype=torch.uint8)
    a, b = datasets.to_mapper_input(d, image=img), datasets.to_mapper_input(d, image=img, is_train=False)
    assert set(a) == set(b) == {"image", "image_id", "file_name", "boxes", "classes", "difficult"}
    assert all(torch.equal(a[k], b[k]) for k in ("boxes", "classes", "difficult"))


# ------------------------------------------------------------------------------------------------------------ known answer
def test_known_answer_one_image_one_category():
    """two small GT, three detections: 0.9 hits the first GT exactly, 0.8 hits nothing, 0.7 overlaps the second GT with IoU
    exactly 0.5 -- a match at t = 0.5 (0.5 < 0.5 is false) and at no higher threshold."""
    from probabilisticteacher_amd.evaluation import COCODetectionEvaluator
    gt = [[0, 0, 10, 10], [20, 20, 10, 10]]
    dt = [[0, 0, 10, 10], [100, 100, 10, 10], [20, 20, 10, 5]]
    sc = [0.9, 0.8, 0.7]
    seg = {"dt_xywh": dt, "dt_score": [float(np.float32(s)) for s in sc], "dt_area": [100.0, 100.0, 50.0],
           "gt_xywh": gt, "gt_area": [100.0, 100.0], "gt_crowd": [0, 0]}
    assert ref.bb_iou(dt, gt, [0, 0])[2][1] == 0.5
    ap50, ap75 = (51 + 50 * 2 / 3) / 101, 51 / 101
    ap = (ap50 + 9 * 51 / 101) / 10
    # ... on the literal reference
    e = ref.evaluate_img(seg, ref.AREA_RNG[0], 100)
    assert e["dtMatchPos"][:, 0].tolist() == [0] * 10 and e["dtMatchPos"][:, 1].tolist() == [-1] * 10
    assert e["dtMatchPos"][:, 2].tolist() == [1] + [-1] * 9
    want = ref.derive_results(*ref.accumulate({(0, 0): seg}, 1, 1), ["thing"])
    for k, v in (("AP", ap), ("AP50", ap50), ("AP75", ap75), ("APs", ap), ("AP-thing", ap)):
        assert math.isclose(want["bbox"][k], 100 * v, rel_tol=0, abs_tol=1e-12), k
    assert math.isnan(want["bbox"]["APm"]) and math.isnan(want["bbox"]["APl"])
    # ... and on the evaluator's pack / accumulate / summarize, fed with the reference's match tables
    ev = COCODetectionEvaluator(["thing"])
    ev.process([_record(5, gt, [0, 0])], [_output(dt, sc, [0, 0, 0])])
    packed = ev.pack()
    assert packed["dt_off"].tolist() == [0, 3] and packed["gt_off"].tolist() == [0, 2]
    assert packed["dt_area"].tolist() == [100.0, 100.0, 50.0] and packed["gt_area"].tolist() == [100.0, 100.0]
    got = ev.results_from_tables(packed, *_ref_tables(packed, {(0, 0): seg}))
    assert list(got["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-thing"]
    assert list(got["bbox_recall"]) == ["AR@1", "AR@10", "AR@100", "ARs", "ARm", "ARl"]
    for k, v in (("AP", ap), ("AP50", ap50), ("AP75", ap75), ("APs", ap), ("AP-thing", ap)):
        assert math.isclose(got["bbox"][k], 100 * v, rel_tol=0, abs_tol=1e-12), k
    assert math.isnan(got["bbox"]["APm"]) and math.isnan(got["bbox"]["APl"])
    assert math.isclose(got["bbox_recall"]["AR@1"], 100 * 0.5, abs_tol=1e-12)          # the best detection alone: one of two GT
    assert math.isclose(got["bbox_recall"]["AR@100"], 100 * (1.0 + 9 * 0.5) / 10, abs_tol=1e-12)


# -------------------------------------------------------------------------------- accumulate / summarize vs the reference
SIDES = (4, 8, 16, 32, 40, 120)


def _random_evaluation(seed=11, n_img=6, n_cat=3):
    """crowd GT, GT in every area range (16 .. 14400 px^2, the 32^2 boundary included), images with GT but no detections and
    the reverse, pairs with neither, and scores from a five-value set so that the stable order decides among ties"""
    rng = np.random.RandomState(seed)
    box = lambda: [int(rng.randint(0, 12)) * 4, int(rng.randint(0, 12)) * 4, SIDES[rng.randint(len(SIDES))], SIDES[rng.randint(len(SIDES))]]
    records, outputs, segments = [], [], {}
    for i in range(n_img):
        gts, gcls, crowd, dts, dcls, scores = [], [], [], [], [], []
        for k in range(n_cat):
            ng = 0 if (i == 1 or (i + k) % 4 == 0) else int(rng.randint(1, 6))        # image 1: detections only
            nd = 0 if (i == 2 or (i + 2 * k) % 5 == 0) else int(rng.randint(1, 9))    # image 2: ground truth only
            g = [box() for _ in range(ng)]
            d = [g[rng.randint(ng)][:] if ng and rng.rand() < 0.6 else box() for _ in range(nd)]
            for b in d:
                if rng.rand() < 0.5:
                    b[2 + rng.randint(2)] = SIDES[rng.randint(len(SIDES))]
            gts += g
            gcls += [k] * ng
            crowd += [int(rng.rand() < 0.25) for _ in range(ng)]
            dts += d
            dcls += [k] * nd
            scores += [float(np.float32(rng.choice([0.9, 0.75, 0.6, 0.45, 0.3]))) for _ in range(nd)]
        perm = rng.permutation(len(dts))                       # detections arrive in the model's order, classes interleaved
        dts, dcls, scores = [dts[j] for j in perm], [dcls[j] for j in perm], [scores[j] for j in perm]
        area = [float(b[2] * b[3]) * (1.0 if rng.rand() < 0.7 else 0.5) for b in gts]       # (segmentation area <= box area)
        records.append(_record(100 - i, gts, gcls, crowd, area))       # descending ids: the evaluator sorts the images
        outputs.append(_output(dts, scores, dcls))
        for k in range(n_cat):
            gsel, dsel = [j for j, c in enumerate(gcls) if c == k], [j for j, c in enumerate(dcls) if c == k]
            if gsel or dsel:
                segments[(n_img - 1 - i, k)] = {
                    "dt_xywh": [dts[j] for j in dsel], "dt_score": [scores[j] for j in dsel],
                    "dt_area": [float(dts[j][2] * dts[j][3]) for j in dsel], "gt_xywh": [gts[j] for j in gsel],
                    "gt_area": [area[j] for j in gsel], "gt_crowd": [crowd[j] for j in gsel]}
    return records, outputs, segments


def test_accumulate_and_summarize_equal_the_literal_reference():
    from probabilisticteacher_amd.evaluation import COCODetectionEvaluator, coco_accumulate
    n_img, n_cat = 6, 3
    names = ["a", "b", "c"]
    records, outputs, segments = _random_evaluation(n_img=n_img, n_cat=n_cat)
    assert any(sum(s["gt_crowd"]) for s in segments.values())
    assert any(len(s["dt_score"]) != len(set(s["dt_score"])) for s in segments.values()), "score ties inside a segment"
    for lo, hi in ref.AREA_RNG[1:]:
        assert any(lo <= a <= hi for s in segments.values() for a in s["gt_area"])
    ev = COCODetectionEvaluator(names)
    for r, o in zip(records, outputs):
        ev.process([r], [o])
    packed = ev.pack()
    assert packed["image_ids"] == sorted(r["image_id"] for r in records)
    tables = _ref_tables(packed, segments)
    assert tables[1].shape == (4, 10, len(packed["dt_score"])) and tables[0].shape == (4, len(packed["gt_area"]))
    want_p, want_r = ref.accumulate(segments, n_img, n_cat)
    got_p, got_r = coco_accumulate(packed, *tables)
    assert got_p.shape == want_p.shape == (10, 101, n_cat, 4, 3) and got_r.shape == want_r.shape
    assert (want_p > -1).any() and (want_p == -1).any()
    assert np.array_equal(got_p == -1, want_p == -1) and np.array_equal(got_r == -1, want_r == -1)
    assert np.abs(got_p - want_p).max() <= 1e-12 and np.abs(got_r - want_r).max() <= 1e-12
    want = ref.derive_results(want_p, want_r, names)
    got = ev.results_from_tables(packed, *tables)
    for part in ("bbox", "bbox_recall"):
        assert list(got[part]) == list(want[part])
        for k, v in want[part].items():
            assert (math.isnan(v) and math.isnan(got[part][k])) or abs(got[part][k] - v) <= 1e-12, (part, k, got[part][k], v)
    assert all(np.isfinite(got["bbox"][k]) for k in ("AP", "AP50", "AP75", "APs", "APm", "APl"))


def test_ground_truth_from_dataset_dicts_and_results_file(tmp_path):
    """GT from the dataset dicts (bbox_xywh / XYXY, default iscrowd and area, images that were never processed) gives the
    same packing as the same GT carried by the records; rank 0 writes coco_instances_results.json in D2's format"""
    from probabilisticteacher_amd.evaluation import COCODetectionEvaluator
    records, outputs, _ = _random_evaluation(seed=3, n_img=3, n_cat=2)
    dicts = []
    for r in records:
        inst = r["instances"]
        b = inst.gt_boxes.tensor.double().tolist()
        dicts.append({"image_id": r["image_id"], "annotations": [
            {"category_id": int(c), "bbox": bb, "iscrowd": int(cr), "area": float(ar)} if j % 2 else
            {"category_id": int(c), "bbox": [0, 0, 0, 0], "bbox_xywh": [bb[0], bb[1], bb[2] - bb[0], bb[3] - bb[1]], "iscrowd": int(cr),
             "area": float(ar)}
            for j, (c, bb, cr, ar) in enumerate(zip(inst.gt_classes.tolist(), b, inst.iscrowd.tolist(), inst.area.tolist()))]})
    dicts.append({"image_id": 1000, "annotations": [{"category_id": 1, "bbox": [2.0, 4.0, 10.0, 20.0]}]})       # never processed
    by_dict = COCODetectionEvaluator(["a", "b"], dataset_dicts=dicts, output_dir=str(tmp_path / "inference"))
    by_rec = COCODetectionEvaluator(["a", "b"])
    for r, o in zip(records, outputs):
        by_dict.process([{k: v for k, v in r.items() if k != "instances"}], [o])
        by_rec.process([r], [o])
    by_rec.process([_record(1000, [[2, 4, 8, 16]], [1])], [_output(np.zeros((0, 4)), [], [])])
    p, q = by_dict.pack(), by_rec.pack()
    assert p["image_ids"] == q["image_ids"] and p["image_ids"][-1] == 1000
    for k in ("dt_off", "gt_off", "dt_xywh", "dt_score", "dt_area", "dt_rank", "gt_xywh", "gt_area", "gt_crowd"):
        assert np.array_equal(p[k], q[k]), k
    assert p["gt_area"][p["gt_off"][-1] - 1] == 8.0 * 16.0 and p["gt_crowd"].dtype == np.int32
    by_dict._write_results()
    rows = json.load(open(tmp_path / "inference" / "coco_instances_results.json"))
    n = sum(len(o["instances"].scores) for o in outputs)
    assert len(rows) == n and set(rows[0]) == {"image_id", "category_id", "bbox", "score"} and len(rows[0]["bbox"]) == 4


def test_only_the_first_hundred_detections_per_image_and_category_are_packed():
    from probabilisticteacher_amd.evaluation import COCODetectionEvaluator
    rng = np.random.RandomState(0)
    n = 130
    sc = np.float32(rng.choice(np.linspace(0.05, 0.95, 19), n))
    dt = np.stack([np.arange(n), np.arange(n), np.full(n, 8), np.full(n, 8)], 1)
    ev = COCODetectionEvaluator(["a", "b"])
    ev.process([_record(1, [[0, 0, 8, 8]], [0])], [_output(dt, sc, [0] * n)])
    packed = ev.pack()
    order = np.argsort(-sc.astype(np.float64), kind="mergesort")[:100]
    assert packed["dt_off"].tolist() == [0, 100, 100] and packed["dt_rank"].tolist() == list(range(100))
    assert np.array_equal(packed["dt_xywh"][:, 0], order.astype(np.float64)) and np.array_equal(packed["dt_score"], sc[order].astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ wiring
def test_build_evaluator_returns_the_coco_evaluator():
    from probabilisticteacher_amd.config import setup_cfg
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.evaluation import COCODetectionEvaluator, PascalVOCDetectionEvaluator
    cfg = setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), ["TEST.EVALUATOR", "COCOeval"])
    ev = PTrainer.build_evaluator(cfg, ["a", "b"])
    assert isinstance(ev, COCODetectionEvaluator) and ev._dict_gt is None
    ev = PTrainer.build_evaluator(cfg, ["a", "b"], dataset_dicts=[{"image_id": 1, "annotations": []}], output_dir="out")
    assert isinstance(ev, COCODetectionEvaluator) and list(ev._dict_gt) == [1] and ev._output_dir == "out"
    cfg = setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), ["TEST.EVALUATOR", "VOCeval"])
    assert isinstance(PTrainer.build_evaluator(cfg, ["a"], True), PascalVOCDetectionEvaluator)
    cfg = setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), ["TEST.EVALUATOR", "nope"])
    with pytest.raises(ValueError, match="Unknown test evaluator"):
        PTrainer.build_evaluator(cfg, ["a"])
