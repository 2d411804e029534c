"""Detection evaluation: the Pascal-VOC protocol and, further down, the COCO protocol.

Reference: pt/engine/trainer.py:127-137 `build_evaluator` (TEST.EVALUATOR == "VOCeval" ->
detectron2.evaluation.PascalVOCDetectionEvaluator), driven from the eval hooks at trainer.py:529-542; the README's
mAP50 tables are this evaluator's "AP50".  detectron2 is not vendored under /root/reference: the protocol below restates
D2 0.5's pascal_voc_evaluation.py (itself the official VOCdevkit / py-faster-rcnn `voc_eval`): detections are written as
text with 3 (score) / 1 (coordinates) decimals and 1-based corners, matched greedily in descending score order against
the ground truth of their class with the `+ 1` pixel-inclusive IoU, "difficult" objects neither count nor punish, AP by
the VOC2010+ area rule or the VOC2007 11-point rule, for IoU thresholds 0.50:0.05:0.95.

Ground truth comes from the records themselves ("instances".gt_boxes / gt_classes [+ "difficult"]) instead of the
VOC XML files D2 parses: D2 subtracts 1 from xmin/ymin when it builds a training record, so the XML box is
[x1 + 1, y1 + 1, x2, y2] of the record's box."""
from collections import OrderedDict, defaultdict
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch


def voc_ap(rec: np.ndarray, prec: np.ndarray, use_07_metric: bool = False) -> float:
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.0
        return float(ap)
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def voc_eval(dets: List[tuple], gts: Dict[object, dict], ovthresh: float = 0.5, use_07_metric: bool = False):
    """dets: [(image_id, score, x1, y1, x2, y2)] of ONE class; gts: image_id -> {"bbox": (M,4), "difficult": (M,) bool}.
    Returns (rec, prec, ap)."""
    class_recs, npos = {}, 0
    for iid, g in gts.items():
        diff = np.asarray(g["difficult"], dtype=bool)
        class_recs[iid] = {"bbox": np.asarray(g["bbox"], dtype=float).reshape(-1, 4), "difficult": diff,
                           "det": [False] * len(diff)}
        npos += int(np.sum(~diff))
    image_ids = [d[0] for d in dets]
    confidence = np.array([float(d[1]) for d in dets])
    BB = np.array([[float(z) for z in d[2:]] for d in dets]).reshape(-1, 4)
    order = np.argsort(-confidence)
    BB = BB[order, :]
    image_ids = [image_ids[x] for x in order]
    nd = len(image_ids)
    tp, fp = np.zeros(nd), np.zeros(nd)
    for d in range(nd):
        R = class_recs.get(image_ids[d], {"bbox": np.zeros((0, 4)), "difficult": np.zeros(0, bool), "det": []})
        bb = BB[d, :].astype(float)
        ovmax = -np.inf
        BBGT = R["bbox"].astype(float)
        if BBGT.size > 0:
            ixmin = np.maximum(BBGT[:, 0], bb[0])
            iymin = np.maximum(BBGT[:, 1], bb[1])
            ixmax = np.minimum(BBGT[:, 2], bb[2])
            iymax = np.minimum(BBGT[:, 3], bb[3])
            iw = np.maximum(ixmax - ixmin + 1.0, 0.0)
            ih = np.maximum(iymax - iymin + 1.0, 0.0)
            inters = iw * ih
            uni = ((bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0)
                   + (BBGT[:, 2] - BBGT[:, 0] + 1.0) * (BBGT[:, 3] - BBGT[:, 1] + 1.0) - inters)
            overlaps = inters / uni
            ovmax = np.max(overlaps)
            jmax = int(np.argmax(overlaps))
        if ovmax > ovthresh:
            if not R["difficult"][jmax]:
                if not R["det"][jmax]:
                    tp[d] = 1.0
                    R["det"][jmax] = True
                else:
                    fp[d] = 1.0
        else:
            fp[d] = 1.0
    fp = np.cumsum(fp)
    tp = np.cumsum(tp)
    rec = tp / float(npos) if npos > 0 else tp * 0.0
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


class PascalVOCDetectionEvaluator:
    """process(inputs, outputs) per batch, evaluate() -> OrderedDict(bbox={"AP", "AP50", "AP75"}) (values in percent)."""

    def __init__(self, class_names: Sequence[str], is_2007: bool = False):
        self._class_names = list(class_names)
        self._is_2007 = bool(is_2007)
        self.reset()

    def reset(self):
        self._predictions = defaultdict(list)         # class id -> [(image_id, score, x1, y1, x2, y2)]
        self._gt = {}                                 # image_id -> (boxes (M,4) in XML convention, classes, difficult)

    def process(self, inputs: Iterable[dict], outputs: Iterable[dict]):
        for inp, out in zip(inputs, outputs):
            image_id = inp.get("image_id", len(self._gt))
            if "instances" in inp and inp["instances"].has("gt_boxes"):
                gt = inp["instances"]
                b = gt.gt_boxes.tensor.detach().cpu().numpy().astype(float).copy()
                b[:, 0] += 1.0
                b[:, 1] += 1.0
                diff = gt.difficult.cpu().numpy().astype(bool) if gt.has("difficult") else np.zeros(len(b), bool)
                self._gt[image_id] = (b, gt.gt_classes.cpu().numpy(), diff)
            else:
                self._gt.setdefault(image_id, (np.zeros((0, 4)), np.zeros(0, np.int64), np.zeros(0, bool)))
            inst = out["instances"]
            boxes = inst.pred_boxes.tensor.detach().cpu().numpy()
            scores = inst.scores.detach().cpu().tolist()
            classes = inst.pred_classes.detach().cpu().tolist()
            for box, score, cls in zip(boxes, scores, classes):
                xmin, ymin, xmax, ymax = box
                # the (matlab) VOC toolkit takes 1-based corners, written with fixed precision (D2 keeps the text round trip)
                line = f"{score:.3f} {xmin + 1:.1f} {ymin + 1:.1f} {xmax:.1f} {ymax:.1f}".split(" ")
                self._predictions[cls].append((image_id,) + tuple(float(v) for v in line))

    def _gather(self):
        """D2's evaluator gathers every rank's predictions on rank 0 before scoring (comm.gather of the pickled lists); the
        ground truth of the images a rank processed travels with them.  Non-zero ranks return None from evaluate()."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return True
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, (dict(self._predictions), self._gt))
        if dist.get_rank() != 0:
            return False
        self._predictions, self._gt = defaultdict(list), {}
        for preds, gt in parts:
            for c, lines in preds.items():
                self._predictions[c].extend(lines)
            self._gt.update(gt)
        return True

    def evaluate(self) -> "Optional[OrderedDict[str, dict]]":
        if not self._gather():
            return None
        aps = defaultdict(list)                       # iou threshold (percent) -> per-class APs
        for cls_id, _ in enumerate(self._class_names):
            dets = self._predictions.get(cls_id, [])
            gts = {iid: {"bbox": b[c == cls_id], "difficult": d[c == cls_id]} for iid, (b, c, d) in self._gt.items()}
            for thresh in range(50, 100, 5):
                _, _, ap = voc_eval(dets, gts, ovthresh=thresh / 100.0, use_07_metric=self._is_2007)
                aps[thresh].append(ap * 100)
        ret = OrderedDict()
        mAP = {iou: float(np.mean(x)) for iou, x in aps.items()}
        ret["bbox"] = {"AP": float(np.mean(list(mAP.values()))), "AP50": mAP[50], "AP75": mAP[75]}
        ret["per_class_AP50"] = {n: aps[50][i] for i, n in enumerate(self._class_names)}
        return ret


# ---------------------------------------------------------------------------------------------------------------------------
# COCO protocol (TEST.EVALUATOR = "COCOeval", the reference's default: pt/config.py, pt/engine/trainer.py:132-133 ->
# detectron2 COCOEvaluator -> pycocotools COCOeval, iouType "bbox").  pycocotools is not a dependency: the protocol is
# restated here (parity by restatement against tests/coco_eval_ref.py, not by running pycocotools).  The greedy matching
# (computeIoU + evaluateImg: every (image, category) pair x 10 IoU thresholds x 4 area ranges) is ONE launch of
# ptmi_coco_match (csrc/coco_eval.hip); packing the segments and `accumulate` are vectorised host work around it.
COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_MAX_DETS = (1, 10, 100)
COCO_AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)


def _segment_offsets(seg: np.ndarray, nseg: int) -> np.ndarray:
    off = np.zeros(nseg + 1, dtype=np.int64)
    np.cumsum(np.bincount(seg, minlength=nseg), out=off[1:])
    return off


def coco_pack(n_img: int, n_cat: int, dt_img, dt_cat, dt_score, dt_xywh, gt_img, gt_cat, gt_xywh, gt_area, gt_crowd) -> dict:
    """Flat detection / ground-truth lists -> the segment layout of ops.coco_match.  Segment s = category * n_img + image.
    Detections: per segment in stable descending score order (np.argsort(-s, kind="mergesort") of computeIoU / evaluateImg),
    the first maxDets[-1] = 100; area = w * h in double (pycocotools loadRes).  Ground truth: dataset order."""
    dt_img, dt_cat = np.asarray(dt_img, dtype=np.int64).reshape(-1), np.asarray(dt_cat, dtype=np.int64).reshape(-1)
    dt_score = np.asarray(dt_score, dtype=np.float64).reshape(-1)
    dt_xywh = np.asarray(dt_xywh, dtype=np.float64).reshape(-1, 4)
    gt_img, gt_cat = np.asarray(gt_img, dtype=np.int64).reshape(-1), np.asarray(gt_cat, dtype=np.int64).reshape(-1)
    gt_xywh = np.asarray(gt_xywh, dtype=np.float64).reshape(-1, 4)
    nseg = n_img * n_cat
    ok = (dt_cat >= 0) & (dt_cat < n_cat)               # (a class the dataset does not list has no category to be scored in)
    dt_img, dt_cat, dt_score, dt_xywh = dt_img[ok], dt_cat[ok], dt_score[ok], dt_xywh[ok]
    seg = dt_cat * n_img + dt_img
    order = np.lexsort((-dt_score, seg))                # stable: equal scores keep their order of arrival
    seg = seg[order]
    start = _segment_offsets(seg, nseg)
    rank = np.arange(len(seg), dtype=np.int64) - start[seg]
    keep = rank < COCO_MAX_DETS[-1]
    order, seg, rank = order[keep], seg[keep], rank[keep]
    xywh = np.ascontiguousarray(dt_xywh[order])
    gseg = gt_cat * n_img + gt_img
    gorder = np.argsort(gseg, kind="mergesort")
    gseg = gseg[gorder]
    return {"n_img": n_img, "n_cat": n_cat, "dt_off": _segment_offsets(seg, nseg), "dt_seg": seg, "dt_rank": rank,
            "dt_score": dt_score[order], "dt_xywh": xywh, "dt_area": xywh[:, 2] * xywh[:, 3],
            "gt_off": _segment_offsets(gseg, nseg), "gt_seg": gseg, "gt_xywh": np.ascontiguousarray(gt_xywh[gorder]),
            "gt_area": np.asarray(gt_area, dtype=np.float64).reshape(-1)[gorder],
            "gt_crowd": np.asarray(gt_crowd, dtype=np.int32).reshape(-1)[gorder]}


def coco_match_on_device(packed: dict, device, iou_thrs=COCO_IOU_THRS, area_rng=COCO_AREA_RNG):
    """one ops.coco_match call over every segment -> gt_ignore (A, NG), dt_match (A, T, ND), dt_ignore (A, T, ND) as numpy"""
    from . import ops
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = ops.coco_match(up(packed["dt_xywh"]), up(packed["dt_area"]), torch.from_numpy(packed["dt_off"]),
                         up(packed["gt_xywh"]), up(packed["gt_area"]), up(packed["gt_crowd"]), torch.from_numpy(packed["gt_off"]),
                         up(np.asarray(iou_thrs, dtype=np.float64)), up(np.asarray(area_rng, dtype=np.float64)))
    return tuple(t.cpu().numpy() for t in out)


def coco_accumulate(packed: dict, gt_ignore, dt_match, dt_ignore, rec_thrs=COCO_REC_THRS, max_dets=COCO_MAX_DETS):
    """pycocotools COCOeval.accumulate over the match tables: precision (T, R, K, A, M) and recall (T, K, A, M), -1 where a
    (category, area range) has no non-ignored ground truth.  Per category, area range and maxDet: each image's first maxDet
    detections, merged by a stable descending score sort; tp / fp cumulative sums without the ignored detections;
    rc = tp / npig, pr = tp / (tp + fp + spacing(1)) made non-increasing from the right; precision sampled at the first
    position whose recall reaches each recall threshold (0 beyond the last recall reached); recall = rc[-1]."""
    n_img, K = packed["n_img"], packed["n_cat"]
    A, T = dt_match.shape[0], dt_match.shape[1]
    R, M = len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    if n_img == 0:
        return precision, recall
    dt_lo, gt_lo = packed["dt_off"][::n_img], packed["gt_off"][::n_img]       # category k owns segments [k n_img, (k+1) n_img)
    for k in range(K):
        d0, d1, g0, g1 = dt_lo[k], dt_lo[k + 1], gt_lo[k], gt_lo[k + 1]
        score, rank = packed["dt_score"][d0:d1], packed["dt_rank"][d0:d1]
        npigs = (gt_ignore[:, g0:g1] == 0).sum(axis=1)
        for m, max_det in enumerate(max_dets):
            sel = np.nonzero(rank < max_det)[0]
            sel = sel[np.argsort(-score[sel], kind="mergesort")]
            for a in range(A):
                npig = int(npigs[a])
                if npig == 0:
                    continue
                dtm = dt_match[a, :, d0:d1][:, sel] >= 0
                keepd = dt_ignore[a, :, d0:d1][:, sel] == 0
                tp = np.cumsum(dtm & keepd, axis=1).astype(np.float64)
                fp = np.cumsum(~dtm & keepd, axis=1).astype(np.float64)
                nd = tp.shape[1]
                if nd == 0:
                    recall[:, k, a, m] = 0
                    precision[:, :, k, a, m] = 0
                    continue
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                recall[:, k, a, m] = rc[:, -1]
                for t in range(T):
                    inds = np.searchsorted(rc[t], rec_thrs, side="left")
                    precision[t, :, k, a, m] = np.where(inds < nd, pr[t][np.minimum(inds, nd - 1)], 0.0)
    return precision, recall


def coco_summarize(precision, recall, class_names: Sequence[str], iou_thrs=COCO_IOU_THRS) -> "OrderedDict[str, dict]":
    """pycocotools summarize + detectron2 _derive_coco_results: percent; nan where no entry is > -1.  bbox: AP (IoU .50:.95),
    AP50, AP75, APs / APm / APl (all at maxDets 100) and AP-<class>; bbox_recall: AR@1 / AR@10 / AR@100 and ARs / ARm / ARl."""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s) * 100) if s.size else float("nan")

    at = lambda v: np.where(v == iou_thrs)[0]
    bbox = OrderedDict()
    bbox["AP"] = mean(precision[:, :, :, 0, -1])
    bbox["AP50"] = mean(precision[at(.5), :, :, 0, -1])
    bbox["AP75"] = mean(precision[at(.75), :, :, 0, -1])
    for a, n in ((1, "APs"), (2, "APm"), (3, "APl")):
        bbox[n] = mean(precision[:, :, :, a, -1])
    for k, name in enumerate(class_names):
        bbox["AP-" + name] = mean(precision[:, :, k, 0, -1])
    rec = OrderedDict()
    for m, n in enumerate(("AR@1", "AR@10", "AR@100")):
        rec[n] = mean(recall[:, :, 0, m])
    for a, n in ((1, "ARs"), (2, "ARm"), (3, "ARl")):
        rec[n] = mean(recall[:, :, a, -1])
    return OrderedDict(bbox=bbox, bbox_recall=rec)


def _gt_from_dict(d: dict):
    """ground truth of one dataset dict, in double as D2 reads / writes the json (convert_to_coco_json for box-only data):
    bbox_xywh if the reader kept it, else XYXY -> XYWH; iscrowd defaults to 0; area defaults to w * h"""
    xywh, cats, crowd, area = [], [], [], []
    for a in d.get("annotations", []):
        if "bbox_xywh" in a:
            x, y, w, h = (float(v) for v in a["bbox_xywh"])
        else:
            x1, y1, x2, y2 = (float(v) for v in a["bbox"])
            x, y, w, h = x1, y1, x2 - x1, y2 - y1
        xywh.append((x, y, w, h))
        cats.append(int(a["category_id"]))
        crowd.append(int(a.get("iscrowd", 0)))
        area.append(float(a["area"]) if "area" in a else w * h)
    return (np.asarray(xywh, dtype=np.float64).reshape(-1, 4), np.asarray(cats, dtype=np.int64), np.asarray(crowd, dtype=np.int32),
            np.asarray(area, dtype=np.float64))


class COCODetectionEvaluator:
    """detectron2 COCOEvaluator (tasks = bbox) with the interface of PascalVOCDetectionEvaluator: process(inputs, outputs) per
    batch, evaluate() -> OrderedDict(bbox={"AP", "AP50", "AP75", "APs", "APm", "APl", "AP-<class>"...}, bbox_recall={...}),
    values in percent (None on ranks other than 0).

    dataset_dicts: the registered dataset's dicts -- ground truth is read from them in double, for every image of the dataset,
    as pycocotools reads the json.  None: ground truth comes from the records ("instances".gt_boxes / gt_classes, optional
    iscrowd / area), for the images that were processed.  Works on VOC-format datasets as well (no crowd, area = w * h).
    output_dir: rank 0 writes coco_instances_results.json (D2's format; category_id is the dataset's own id when
    `dataset_id_map`, contiguous id -> dataset id, is given).  device: where the matching kernel runs (default: the current
    ROCm device)."""

    def __init__(self, class_names: Sequence[str], dataset_dicts: Optional[List[dict]] = None, output_dir: Optional[str] = None,
                 device=None, dataset_id_map: Optional[Dict[int, int]] = None):
        self._class_names = list(class_names)
        self._output_dir = output_dir
        self._device = device
        self._dataset_id_map = dataset_id_map
        self._dict_gt = None
        if dataset_dicts is not None:
            self._dict_gt = OrderedDict((d["image_id"], _gt_from_dict(d)) for d in dataset_dicts)
        self.reset()

    def reset(self):
        self._predictions = []                        # per processed image: (image_id, xywh (n,4) f64, scores [float], classes [int])
        self._gt = OrderedDict()                      # image_id -> (xywh, classes, crowd, area) from the records

    def process(self, inputs: Iterable[dict], outputs: Iterable[dict]):
        for inp, out in zip(inputs, outputs):
            image_id = inp.get("image_id", len(self._predictions))
            if self._dict_gt is None:
                if "instances" in inp and inp["instances"].has("gt_boxes"):
                    gt = inp["instances"]
                    b = gt.gt_boxes.tensor.detach().cpu().numpy().astype(np.float64).reshape(-1, 4)
                    xywh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)
                    crowd = gt.iscrowd.cpu().numpy().astype(np.int32) if gt.has("iscrowd") else np.zeros(len(b), np.int32)
                    area = gt.area.cpu().numpy().astype(np.float64) if gt.has("area") else xywh[:, 2] * xywh[:, 3]
                    self._gt[image_id] = (xywh, gt.gt_classes.cpu().numpy().astype(np.int64), crowd, area)
                else:
                    self._gt.setdefault(image_id, (np.zeros((0, 4)), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0)))
            inst = out["instances"]
            # D2 instances_to_coco_json: XYXY -> XYWH on the fp32 boxes, then Python floats
            b = inst.pred_boxes.tensor.detach().cpu().to(torch.float32).reshape(-1, 4).clone()
            b[:, 2] -= b[:, 0]
            b[:, 3] -= b[:, 1]
            self._predictions.append((image_id, b.numpy().astype(np.float64), inst.scores.detach().cpu().tolist(),
                                      inst.pred_classes.detach().cpu().tolist()))

    def _gather(self):
        """as PascalVOCDetectionEvaluator._gather: every rank's predictions (and record ground truth) meet on rank 0"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return True
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, (self._predictions, self._gt))
        if dist.get_rank() != 0:
            return False
        self._predictions, self._gt = [], OrderedDict()
        for preds, gt in parts:
            self._predictions.extend(preds)
            self._gt.update(gt)
        return True

    def pack(self) -> dict:
        """the processed predictions and the ground truth as coco_pack's segment layout; images in sorted id order (pycocotools
        params.imgIds), in order of arrival where the ids do not compare"""
        gts = self._dict_gt if self._dict_gt is not None else self._gt
        ids = list(gts)
        ids += [p[0] for p in self._predictions if p[0] not in gts]
        ids = list(OrderedDict.fromkeys(ids))
        try:
            ids = sorted(ids)
        except TypeError:
            pass
        index = {iid: i for i, iid in enumerate(ids)}
        n = [len(p[2]) for p in self._predictions]
        dt_img = np.repeat(np.asarray([index[p[0]] for p in self._predictions], dtype=np.int64), n)
        cat = lambda parts, shape, dtype: (np.concatenate(parts) if parts else np.zeros(shape)).astype(dtype).reshape(shape)
        dt_xywh = cat([p[1] for p in self._predictions], (-1, 4), np.float64)
        dt_score = cat([np.asarray(p[2], dtype=np.float64) for p in self._predictions], (-1,), np.float64)
        dt_cat = cat([np.asarray(p[3], dtype=np.int64) for p in self._predictions], (-1,), np.int64)
        gt_img = np.repeat(np.asarray([index[i] for i in gts], dtype=np.int64), [len(g[1]) for g in gts.values()])
        g = list(gts.values())
        packed = coco_pack(len(ids), len(self._class_names), dt_img, dt_cat, dt_score, dt_xywh, gt_img,
                           cat([v[1] for v in g], (-1,), np.int64), cat([v[0] for v in g], (-1, 4), np.float64),
                           cat([v[3] for v in g], (-1,), np.float64), cat([v[2] for v in g], (-1,), np.int32))
        packed["image_ids"] = ids
        return packed

    def results_from_tables(self, packed: dict, gt_ignore, dt_match, dt_ignore) -> "OrderedDict[str, dict]":
        """accumulate + summarize over the match tables of `packed` (whoever computed them)"""
        precision, recall = coco_accumulate(packed, gt_ignore, dt_match, dt_ignore)
        return coco_summarize(precision, recall, self._class_names)

    def _write_results(self):
        import json
        import os
        os.makedirs(self._output_dir, exist_ok=True)
        rows = []
        for image_id, xywh, scores, classes in self._predictions:
            for box, s, c in zip(xywh.tolist(), scores, classes):
                c = self._dataset_id_map[c] if self._dataset_id_map is not None else c
                rows.append({"image_id": image_id, "category_id": c, "bbox": box, "score": s})
        with open(os.path.join(self._output_dir, "coco_instances_results.json"), "w") as f:
            f.write(json.dumps(rows))
            f.flush()

    def evaluate(self) -> "Optional[OrderedDict[str, dict]]":
        if not self._gather():
            return None
        if self._output_dir:
            self._write_results()
        packed = self.pack()
        device = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
        return self.results_from_tables(packed, *coco_match_on_device(packed, device))


@torch.no_grad()
def inference_on_dataset(model, data_loader: Iterable[List[dict]],
                         evaluator: "Union[PascalVOCDetectionEvaluator, COCODetectionEvaluator]"):
    """D2 inference_on_dataset: eval mode, `model(batched_inputs)` (rcnn.py:33-34 -> inference + detector_postprocess),
    evaluator.process per batch; the model's previous mode is restored."""
    was_training = model.training
    model.eval()
    evaluator.reset()
    try:
        for batch in data_loader:
            evaluator.process(batch, model(batch))
    finally:
        model.train(was_training)
    return evaluator.evaluate()
