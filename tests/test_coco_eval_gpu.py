"""GPU (pytest -m gpu): ptmi_coco_match (csrc/coco_eval.hip) against the literal restatement of pycocotools in
tests/coco_eval_ref.py -- every table entry of every segment exactly equal -- its argument checks, and TEST.EVALUATOR = COCOeval
end to end through PTrainer.test on a COCO json and on a VOC-format directory."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import coco_eval_ref as ref
from tests.test_host_logic import _write_voc_dir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (4, 8, 16, 40, 120)


def _box(rng):
    return [int(rng.randint(0, 40)) * 4, int(rng.randint(0, 40)) * 4, SIDES[rng.randint(len(SIDES))], SIDES[rng.randint(len(SIDES))]]


def _near(rng, g):
    """a detection derived from ground-truth box g on the integer grid: the same box, one side swapped for another of SIDES,
    or the box moved by a quarter / third / half of a side -- overlaps of 1/2, 3/5, 3/4 (of a crowd box) and 1 among them"""
    x, y, w, h = g
    mode = rng.randint(4)
    if mode == 1:
        if rng.rand() < 0.5:
            w = SIDES[rng.randint(len(SIDES))]
        else:
            h = SIDES[rng.randint(len(SIDES))]
    elif mode >= 2:
        div = (4, 3, 2)[rng.randint(3)]
        if rng.rand() < 0.5:
            x += w // div
        else:
            y += h // div
    return [x, y, w, h]


def _segment(rng, D, G, crowd_p=0.2, near_p=0.7):
    gt = [_box(rng) for _ in range(G)]
    for j in range(1, G):                                    # clusters: several GT compete for the same detections
        if rng.rand() < 0.4:
            gt[j] = _near(rng, gt[rng.randint(j)])
    dt = [_near(rng, gt[rng.randint(G)]) if G and rng.rand() < near_p else _box(rng) for _ in range(D)]
    return {"dt_xywh": dt, "dt_score": [1.0 - 0.005 * d for d in range(D)], "dt_area": [float(b[2] * b[3]) for b in dt],
            "gt_xywh": gt, "gt_area": [float(b[2] * b[3]) * (1.0 if rng.rand() < 0.8 else 0.5) for b in gt],
            "gt_crowd": [int(rng.rand() < crowd_p) for _ in range(G)]}


def _segments():
    rng = np.random.RandomState(2017)
    segs = [_segment(rng, 1, 3)]                             # odd lengths first: later segments start at odd offsets
    for rep in range(3):
        for D in (0, 1, 2, 7, 100):
            for G in (0, 1, 3, 12):
                if rep == 2 and D == 100 and G == 12:
                    continue
                segs.append(_segment(rng, D, G, crowd_p=(0.2, 0.0, 0.5)[rep]))
    # every GT a crowd box: matched again and again, every match ignored
    s = _segment(rng, 7, 3)
    s["gt_crowd"] = [1, 1, 1]
    segs.append(s)
    # one crowd GT under five detections, all of which it matches
    segs.append({"dt_xywh": [[8, 8, 16, 16], [12, 8, 16, 16], [8, 12, 16, 16], [8, 8, 8, 16], [16, 16, 8, 8]],
                 "dt_score": [0.9, 0.8, 0.7, 0.6, 0.5], "dt_area": [256.0, 256.0, 256.0, 128.0, 64.0],
                 "gt_xywh": [[8, 8, 16, 16]], "gt_area": [256.0], "gt_crowd": [1]})
    # GT 0 is large (ignored in "medium"), GT 1 medium; the detection overlaps GT 0 fully and GT 1 by exactly 1/2: where GT 0
    # is ignored the later, non-ignored GT 1 is visited first and keeps the match at t = 0.5; above it GT 0 takes it, ignored
    segs.append({"dt_xywh": [[0, 0, 120, 120]], "dt_score": [0.9], "dt_area": [14400.0],
                 "gt_xywh": [[0, 0, 120, 120], [0, 0, 120, 60]], "gt_area": [14400.0, 7200.0], "gt_crowd": [0, 0]})
    # a long ground-truth list
    big = _segment(rng, 7, 1024, crowd_p=0.1)
    big["dt_xywh"][1] = list(big["gt_xywh"][1000])
    big["dt_area"][1] = float(big["dt_xywh"][1][2] * big["dt_xywh"][1][3])
    segs.append(big)
    segs.append(_segment(rng, 7, 12))
    return segs


_CACHE = {}


def _case():
    """the segments, their packed arrays and the reference's tables: computed once, shared, never modified"""
    if not _CACHE:
        segs = _segments()
        cat = lambda k, shape, dtype: np.concatenate([np.asarray(s[k], dtype=dtype).reshape(shape) for s in segs])
        _CACHE.update(
            segs=segs, dt_off=np.cumsum([0] + [len(s["dt_score"]) for s in segs]), gt_off=np.cumsum([0] + [len(s["gt_crowd"]) for s in segs]),
            dt_xywh=cat("dt_xywh", (-1, 4), np.float64), dt_area=cat("dt_area", (-1,), np.float64),
            gt_xywh=cat("gt_xywh", (-1, 4), np.float64), gt_area=cat("gt_area", (-1,), np.float64),
            gt_crowd=cat("gt_crowd", (-1,), np.int32), tables=ref.match_tables(segs))
    return _CACHE


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _match(c, **kw):
    from probabilisticteacher_amd import ops
    return ops.coco_match(_dev(c["dt_xywh"]), _dev(c["dt_area"]), _dev(c["dt_off"], torch.int64), _dev(c["gt_xywh"]), _dev(c["gt_area"]),
                          _dev(c["gt_crowd"]), _dev(c["gt_off"], torch.int64), _dev(ref.IOU_THRS),
                          _dev(np.asarray(ref.AREA_RNG, dtype=np.float64)), **kw)


def test_the_cases_cover_what_they_claim():
    """(CPU arithmetic only) ties at the thresholds, crowd re-matching, the ignored-GT order, area ignores, odd offsets"""
    c = _case()
    segs, (gi, dm, di) = c["segs"], c["tables"]
    assert 55 <= len(segs) <= 70
    assert {(len(s["dt_score"]), len(s["gt_crowd"])) for s in segs} >= {(D, G) for D in (0, 1, 2, 7, 100) for G in (0, 1, 3, 12)}
    assert max(len(s["gt_crowd"]) for s in segs) == 1024
    loops = sum(4 * 10 * len(s["dt_score"]) * len(s["gt_crowd"]) for s in segs)
    assert loops < 3e6, loops
    thr = set(ref.IOU_THRS.tolist())
    tied = sum(any(v in thr for row in ref.compute_iou(s) for v in row) for s in segs)
    assert 3 * tied >= len(segs), f"{tied} of {len(segs)} segments hold an IoU equal to a threshold"
    assert any(o % 2 for o in c["dt_off"][1:-1]) and any(o % 4 for o in c["dt_off"][1:-1])
    assert any(o % 2 for o in c["gt_off"][1:-1]) and any(o % 4 for o in c["gt_off"][1:-1])
    # a crowd GT matched by several detections
    k = next(i for i, s in enumerate(segs) if s["gt_crowd"] == [1] and len(s["dt_score"]) == 5)
    d0 = c["dt_off"][k]
    assert dm[0, 0, d0:d0 + 5].tolist() == [0, 0, 0, 0, 0] and di[0, 0, d0:d0 + 5].tolist() == [1] * 5
    # the later non-ignored GT wins over the earlier ignored one ("medium"), the earlier one where both count ("all")
    k = next(i for i, s in enumerate(segs) if s["gt_area"] == [14400.0, 7200.0])
    d0 = c["dt_off"][k]
    assert dm[0, 0, d0] == 0 and dm[2, 0, d0] == 1 and di[2, 0, d0] == 0 and dm[2, 1, d0] == 0 and di[2, 1, d0] == 1
    # unmatched detections outside each of the small / medium / large ranges
    for a in (1, 2, 3):
        assert ((dm[a] == -1) & (di[a] == 1)).any() and ((dm[a] == -1) & (di[a] == 0)).any()
    assert (gi[0] != gi[1]).any() and (gi[1] != gi[2]).any() and (gi[2] != gi[3]).any()


def test_coco_match_equals_the_literal_reference():
    c = _case()
    gi, dm, di = (t.cpu().numpy() for t in _match(c))
    want_gi, want_dm, want_di = c["tables"]
    assert gi.dtype == dm.dtype == di.dtype == np.int32
    assert gi.shape == want_gi.shape and dm.shape == want_dm.shape == di.shape == want_di.shape
    bad = []
    for k in range(len(c["segs"])):                          # every segment, so that a failure names its shape
        d = slice(c["dt_off"][k], c["dt_off"][k + 1])
        g = slice(c["gt_off"][k], c["gt_off"][k + 1])
        if not (np.array_equal(gi[:, g], want_gi[:, g]) and np.array_equal(dm[:, :, d], want_dm[:, :, d])
                and np.array_equal(di[:, :, d], want_di[:, :, d])):
            bad.append((k, len(c["segs"][k]["dt_score"]), len(c["segs"][k]["gt_crowd"])))
    assert not bad, f"segments (index, D, G) that differ: {bad}"
    assert np.array_equal(gi, want_gi) and np.array_equal(dm, want_dm) and np.array_equal(di, want_di)


def test_fewer_thresholds_and_ranges_and_empty_sides():
    """T = 16 thresholds (the widest wave: 4 x 16 lanes), A = 1, and arrays with no detections / no ground truth at all"""
    from probabilisticteacher_amd import ops
    c = _case()
    segs = c["segs"][:25]
    thr = np.linspace(0.2, 0.95, 16)
    want = ref.match_tables(segs, iou_thrs=thr)
    nd, ng = c["dt_off"][25], c["gt_off"][25]
    got = ops.coco_match(_dev(c["dt_xywh"][:nd]), _dev(c["dt_area"][:nd]), _dev(c["dt_off"][:26], torch.int64), _dev(c["gt_xywh"][:ng]),
                         _dev(c["gt_area"][:ng]), _dev(c["gt_crowd"][:ng]), _dev(c["gt_off"][:26], torch.int64), _dev(thr),
                         _dev(np.asarray(ref.AREA_RNG, dtype=np.float64)))
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    one = ops.coco_match(_dev(c["dt_xywh"][:nd]), _dev(c["dt_area"][:nd]), _dev(c["dt_off"][:26], torch.int64), _dev(c["gt_xywh"][:ng]),
                         _dev(c["gt_area"][:ng]), _dev(c["gt_crowd"][:ng]), _dev(c["gt_off"][:26], torch.int64), _dev(ref.IOU_THRS[:1]),
                         _dev(np.asarray(ref.AREA_RNG[2:3], dtype=np.float64)))
    w = ref.match_tables(segs, iou_thrs=ref.IOU_THRS[:1], area_rng=ref.AREA_RNG[2:3])
    assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(one, w))
    z4, z1, zi = torch.zeros((0, 4), dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV), \
        torch.zeros(0, dtype=torch.int32, device=DEV)
    zoff = torch.zeros(4, dtype=torch.int64)
    gi, dm, di = ops.coco_match(z4, z1, zoff, _dev(c["gt_xywh"][:3]), _dev(c["gt_area"][:3]), _dev(c["gt_crowd"][:3]),
                                torch.tensor([0, 1, 1, 3]), _dev(ref.IOU_THRS), _dev(np.asarray(ref.AREA_RNG, dtype=np.float64)))
    assert dm.shape == (4, 10, 0) and np.array_equal(gi.cpu().numpy(), c["tables"][0][:, :3])
    gi, dm, di = ops.coco_match(_dev(c["dt_xywh"][:3]), _dev(c["dt_area"][:3]), torch.tensor([0, 2, 2, 3]), z4, z1, zi, zoff,
                                _dev(ref.IOU_THRS), _dev(np.asarray(ref.AREA_RNG, dtype=np.float64)))
    assert gi.shape == (4, 0) and (dm.cpu().numpy() == -1).all()
    area = c["dt_area"][:3]
    want_di = np.stack([np.repeat(((area < lo) | (area > hi))[None], 10, 0) for lo, hi in ref.AREA_RNG]).astype(np.int32)
    assert np.array_equal(di.cpu().numpy(), want_di)


def test_argument_checks_refuse_before_any_launch():
    """one detection too many, G above the limit, T = 17, A = 5, tables that do not tile the arrays, a null pointer: an error
    each, and the prefilled outputs keep their sentinel"""
    from probabilisticteacher_amd import _lib, ops
    lim = ops.coco_match_max_gt()
    assert lim >= 1024
    thr, rng_ = _dev(ref.IOU_THRS), _dev(np.asarray(ref.AREA_RNG, dtype=np.float64))

    def arrays(nd, ng):
        return (torch.ones((nd, 4), dtype=torch.float64, device=DEV), torch.ones(nd, dtype=torch.float64, device=DEV),
                torch.ones((ng, 4), dtype=torch.float64, device=DEV), torch.ones(ng, dtype=torch.float64, device=DEV),
                torch.zeros(ng, dtype=torch.int32, device=DEV))

    def sentinel(nd, ng, T=10, A=4):
        return (torch.full((A, ng), -7, dtype=torch.int32, device=DEV), torch.full((A, T, nd), -7, dtype=torch.int32, device=DEV),
                torch.full((A, T, nd), -7, dtype=torch.int32, device=DEV))

    def untouched(out):
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in out)

    dx, da, gx, ga, gc = arrays(101, 2)
    out = sentinel(101, 2)
    with pytest.raises(ValueError, match="101 detections"):
        ops.coco_match(dx, da, torch.tensor([0, 101]), gx, ga, gc, torch.tensor([0, 2]), thr, rng_, out=out)
    assert untouched(out)
    ops.coco_match(dx[:100], da[:100], torch.tensor([0, 100]), gx, ga, gc, torch.tensor([0, 2]), thr, rng_)      # 100 are served
    dx, da, gx, ga, gc = arrays(2, lim + 1)
    out = sentinel(2, lim + 1)
    with pytest.raises(ValueError, match="ground-truth boxes"):
        ops.coco_match(dx, da, torch.tensor([0, 2]), gx, ga, gc, torch.tensor([0, lim + 1]), thr, rng_, out=out)
    assert untouched(out)
    dx, da, gx, ga, gc = arrays(2, 3)
    out = sentinel(2, 3, T=17)
    with pytest.raises(ValueError, match="17 IoU thresholds"):
        ops.coco_match(dx, da, torch.tensor([0, 2]), gx, ga, gc, torch.tensor([0, 3]), _dev(np.linspace(0.1, 0.9, 17)), rng_, out=out)
    assert untouched(out)
    out = sentinel(2, 3, A=5)
    with pytest.raises(ValueError, match="5 area ranges"):
        ops.coco_match(dx, da, torch.tensor([0, 2]), gx, ga, gc, torch.tensor([0, 3]), thr, _dev(np.tile([0.0, 1e10], (5, 1))), out=out)
    assert untouched(out)
    out = sentinel(2, 3)
    with pytest.raises(ValueError, match="does not tile"):
        ops.coco_match(dx, da, torch.tensor([0, 1]), gx, ga, gc, torch.tensor([0, 3]), thr, rng_, out=out)
    with pytest.raises(ValueError, match="does not tile"):
        ops.coco_match(dx, da, torch.tensor([0, 3, 2]), gx, ga, gc, torch.tensor([0, 1, 3]), thr, rng_, out=out)
    assert untouched(out)
    with pytest.raises(_lib.PtmiError, match="ROCm device tensor"):
        ops.coco_match(dx.cpu(), da, torch.tensor([0, 2]), gx, ga, gc, torch.tensor([0, 3]), thr, rng_, out=out)
    # the C entry point itself: the same limits, and a null pointer
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    doff, goff = torch.tensor([0, 2], device=DEV), torch.tensor([0, 3], device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(dt_xywh=p(dx), dt_area=p(da), dt_off=p(doff), gt_xywh=p(gx), gt_area=p(ga), gt_crowd=p(gc), gt_off=p(goff), nseg=1,
                 nd=2, ng=3, max_dt=2, max_gt=3, thr=p(thr), nthr=10, rng=p(rng_), narea=4, gi=p(out[0]), dm=p(out[1]), di=p(out[2]))
        a.update(kw)
        return lib.ptmi_coco_match(*a.values(), stream), lib.ptmi_last_error().decode()

    for kw, msg in ((dict(max_dt=101), "101 detections"), (dict(max_gt=lim + 1), "ground-truth boxes"), (dict(nthr=17), "17 IoU thresholds"),
                    (dict(narea=5), "5 area ranges"), (dict(dt_xywh=None), "detection arrays missing"), (dict(gi=None), "ground-truth arrays missing"),
                    (dict(gt_off=None), "offset tables missing"), (dict(thr=None), "missing"), (dict(dm=None), "detection arrays missing")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched(out)
    rc, err = call()
    assert rc == 0, err
    torch.cuda.synchronize()
    assert not bool((out[1] == -7).any()) and not bool((out[0] == -7).any()) and not bool((out[2] == -7).any())


# ------------------------------------------------------------------------------------------------------------- end to end
def _small_cfg(extra):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "INPUT.MIN_SIZE_TEST", 160, "INPUT.MAX_SIZE_TEST", 320,
        "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0, "TEST.EVALUATOR", "COCOeval"] + extra)


def _ref_results(ev, n_cat, names):
    """the literal reference on the evaluator's stored predictions and ground truth"""
    gts = ev._dict_gt if ev._dict_gt is not None else ev._gt
    ids = sorted(gts)
    segments = {}
    for i, iid in enumerate(ids):
        xywh, cls, crowd, area = gts[iid]
        for k in range(n_cat):
            sel = [j for j in range(len(cls)) if cls[j] == k]
            if sel:
                segments[(i, k)] = {"gt_xywh": [xywh[j].tolist() for j in sel], "gt_area": [float(area[j]) for j in sel],
                                    "gt_crowd": [int(crowd[j]) for j in sel]}
    for iid, xywh, scores, classes in ev._predictions:
        for k in range(n_cat):
            sel = [j for j in range(len(classes)) if classes[j] == k]
            if sel:
                seg = segments.setdefault((ids.index(iid), k), {})
                seg.update(dt_xywh=[xywh[j].tolist() for j in sel], dt_score=[scores[j] for j in sel],
                           dt_area=[float(xywh[j][2]) * float(xywh[j][3]) for j in sel])
    return ref.derive_results(*ref.accumulate(segments, len(ids), n_cat), names)


def test_cocoeval_end_to_end_on_a_coco_json_and_a_voc_directory(tmp_path, monkeypatch):
    from PIL import Image
    from probabilisticteacher_amd import evaluation, modeling
    from probabilisticteacher_amd.data import datasets
    from probabilisticteacher_amd.engine import PTrainer
    rng = np.random.RandomState(5)
    names = ["car", "person", "bus"]
    os.makedirs(tmp_path / "img")
    images, anns = [], []
    for i in range(4):
        h, w = 160, 224
        img = rng.randint(0, 96, (h, w, 3)).astype(np.uint8)
        for _ in range(int(rng.randint(1, 4)) if i != 2 else 0):          # image 2 has no annotation
            bw, bh = int(rng.randint(24, 120)), int(rng.randint(20, 100))
            x1, y1 = int(rng.randint(1, w - bw)), int(rng.randint(1, h - bh))
            img[y1:y1 + bh, x1:x1 + bw] += 120
            anns.append({"id": len(anns) + 1, "image_id": 10 + i, "category_id": (2, 5, 9)[rng.randint(3)],
                         "bbox": [x1 + 0.5, y1 + 0.25, float(bw), float(bh)], "area": 0.8 * bw * bh, "iscrowd": int(len(anns) == 1)})
        Image.fromarray(img).save(str(tmp_path / "img" / f"{i}.jpg"), quality=95)
        images.append({"id": 10 + i, "file_name": f"{i}.jpg", "height": h, "width": w})
    with open(tmp_path / "inst.json", "w") as f:
        json.dump({"images": images[::-1], "annotations": anns,
                   "categories": [{"id": 9, "name": "bus"}, {"id": 2, "name": "car"}, {"id": 5, "name": "person"}]}, f)
    datasets.register_coco_instances("cc_val", str(tmp_path / "inst.json"), str(tmp_path / "img"))
    cfg = _small_cfg(["MODEL.ROI_HEADS.NUM_CLASSES", 3, "DATASETS.TEST", ("cc_val",)])
    torch.manual_seed(0)
    model = modeling.build_model(cfg).to(DEV)
    built = []
    orig = PTrainer.build_evaluator.__func__
    monkeypatch.setattr(PTrainer, "build_evaluator", classmethod(lambda cls, *a, **k: built.append(orig(cls, *a, **k)) or built[-1]))
    res = PTrainer.test(cfg, model)
    ev = built[-1]
    assert isinstance(ev, evaluation.COCODetectionEvaluator) and ev._dict_gt is not None and list(ev._dict_gt) == [10, 11, 12, 13]
    assert list(res["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-car", "AP-person", "AP-bus"]
    assert sum(len(p[2]) for p in ev._predictions) > 0, "the untrained model still proposes boxes at SCORE_THRESH_TEST 0"
    want = _ref_results(ev, 3, names)
    for part in ("bbox", "bbox_recall"):
        for k, v in want[part].items():
            got = res[part][k]
            print(part, k, got, v)
            assert (math.isnan(v) and math.isnan(got)) or abs(got - v) <= 1e-12, (part, k, got, v)
    assert all(math.isnan(v) or 0.0 <= v <= 100.0 for v in res["bbox"].values())
    # the same evaluator on a VOC-format directory through an explicit loader: ground truth from the records
    _write_voc_dir(str(tmp_path / "voc"), [f"v{i}" for i in range(3)], ("car", "person", "bus"), rng, h=160, w=224)
    datasets.register_pascal_voc("cc_voc", str(tmp_path / "voc"), "train", ("car", "person", "bus"))
    res2 = PTrainer.test(cfg, model, data_loader=PTrainer.build_test_loader(cfg, "cc_voc"), class_names=names)
    ev2 = built[-1]
    assert ev2._dict_gt is None and len(ev2._gt) == 3
    assert np.isfinite(res2["bbox"]["AP50"]) and 0.0 <= res2["bbox"]["AP50"] <= 100.0
    want2 = _ref_results(ev2, 3, names)
    assert abs(res2["bbox"]["AP50"] - want2["bbox"]["AP50"]) <= 1e-12 and abs(res2["bbox"]["AP"] - want2["bbox"]["AP"]) <= 1e-12
    # and through cfg.DATASETS.TEST (the dataset's dicts): VOC dicts carry neither iscrowd nor area
    cfg.defrost()
    cfg.DATASETS.TEST = ("cc_voc",)
    res3 = PTrainer.test(cfg, model)
    assert built[-1]._dict_gt is not None and np.isfinite(res3["bbox"]["AP50"])
    assert abs(res3["bbox"]["AP50"] - _ref_results(built[-1], 3, names)["bbox"]["AP50"]) <= 1e-12
