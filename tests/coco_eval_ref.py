"""A literal, loop-for-loop restatement of the COCO detection protocol: pycocotools `COCOeval.computeIoU`, `evaluateImg`,
`accumulate`, `summarize` and `maskApi.c: bbIou`, plus detectron2's `_derive_coco_results`, for boxes.  pycocotools cannot be
installed here, so parity with it is by restatement, not by execution.  Written on its own: it shares no code with
probabilisticteacher_amd/evaluation.py or csrc/coco_eval.hip, and stands to them as tests/roi_pooler_ref.py and
tests/statistics_ref.py stand to their kernels.  Plain Python floats (IEEE doubles) throughout.

An evaluation is described by `segments`: {(image index, category index): segment}, a segment being a dict of
  dt_xywh (D, 4), dt_score (D), dt_area (D)      detections in ANY order (sorted here, as pycocotools does)
  gt_xywh (G, 4), gt_area (G), gt_crowd (G)      ground truth in dataset order
Missing keys / absent pairs mean "none"."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]


def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou: o[d][g]"""
    o = [[0.0] * len(gt) for _ in dt]
    for g in range(len(gt)):
        G = [float(v) for v in gt[g]]
        ga = G[2] * G[3]
        crowd = bool(iscrowd[g])
        for d in range(len(dt)):
            T = [float(v) for v in dt[d]]
            da = T[2] * T[3]
            o[d][g] = 0.0
            w = min(T[2] + T[0], G[2] + G[0]) - max(T[0], G[0])
            if w <= 0:
                continue
            h = min(T[3] + T[1], G[3] + G[1]) - max(T[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d][g] = i / u
    return o


def _seg(seg):
    seg = seg or {}
    get = lambda k, shape: np.asarray(seg.get(k, []), dtype=np.float64).reshape(shape)
    return (get("dt_xywh", (-1, 4)), get("dt_score", (-1,)), get("dt_area", (-1,)), get("gt_xywh", (-1, 4)),
            get("gt_area", (-1,)), np.asarray(seg.get("gt_crowd", np.zeros(0)), dtype=np.int64).reshape(-1))


def compute_iou(seg, max_det=MAX_DETS[-1]):
    """COCOeval.computeIoU: detections by descending score (stable), the first maxDets[-1]; ious[d][g], g in dataset order"""
    dt_xywh, dt_score, _, gt_xywh, _, gt_crowd = _seg(seg)
    if len(gt_xywh) == 0 and len(dt_xywh) == 0:
        return []
    inds = np.argsort([-s for s in dt_score], kind="mergesort")
    dt = [dt_xywh[i] for i in inds]
    if len(dt) > max_det:
        dt = dt[0:max_det]
    if len(dt) == 0 or len(gt_xywh) == 0:
        return []
    return bb_iou(dt, gt_xywh, gt_crowd)


def evaluate_img(seg, a_rng, max_det, iou_thrs=IOU_THRS, ious=None):
    """COCOeval.evaluateImg for one (image, category) and one area range.  None when both sides are empty.  Beside
    pycocotools' fields (dtScores, dtMatches as booleans, dtIgnore, gtIgnore in VISITING order) the result names the matched
    ground truth by its position in dataset order (dtMatchPos, -1 = none), the ignore flags in dataset order (gtIgnoreDataset)
    and the detection order (dtOrder)."""
    dt_xywh, dt_score, dt_area, gt_xywh, gt_area, gt_crowd = _seg(seg)
    if len(gt_xywh) == 0 and len(dt_xywh) == 0:
        return None
    ignore = [1 if (gt_crowd[g] or (gt_area[g] < a_rng[0] or gt_area[g] > a_rng[1])) else 0 for g in range(len(gt_xywh))]
    gtind = np.argsort(ignore, kind="mergesort")
    dtind = np.argsort([-s for s in dt_score], kind="mergesort")[0:max_det]
    iscrowd = [int(gt_crowd[g]) for g in gtind]
    ious = compute_iou(seg) if ious is None else ious          # (self.ious[imgId, catId]: computed once per pair)
    ious = [[row[g] for g in gtind] for row in ious] if len(ious) > 0 else ious
    T, G, D = len(iou_thrs), len(gtind), len(dtind)
    gtm = np.zeros((T, G))
    dtm = -np.ones((T, D), dtype=np.int64)
    gt_ig = np.array([ignore[g] for g in gtind], dtype=np.int64)
    dt_ig = np.zeros((T, D))
    if not len(ious) == 0:
        for tind, t in enumerate(iou_thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind][gind] < iou:
                        continue
                    iou = ious[dind][gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = m
                gtm[tind, m] = 1
    a = np.array([dt_area[d] < a_rng[0] or dt_area[d] > a_rng[1] for d in dtind]).reshape((1, D))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == -1, np.repeat(a, T, 0)))
    pos = np.where(dtm >= 0, np.asarray(gtind, dtype=np.int64)[np.maximum(dtm, 0)] if G else -1, -1)
    return {"dtScores": [dt_score[d] for d in dtind], "dtMatches": dtm >= 0, "dtIgnore": dt_ig, "gtIgnore": gt_ig,
            "dtMatchPos": pos, "gtIgnoreDataset": np.asarray(ignore, dtype=np.int64), "dtOrder": np.asarray(dtind)}


def accumulate(segments, n_img, n_cat, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS, area_rng=AREA_RNG):
    """COCOeval.evaluate + accumulate: precision (T, R, K, A, M), recall (T, K, A, M), -1 where nothing was evaluated"""
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), n_cat, len(area_rng), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    ious = {(i, k): compute_iou(segments.get((i, k)), max_dets[-1]) for k in range(K) for i in range(n_img)}
    eval_imgs = {(k, a, i): evaluate_img(segments.get((i, k)), area_rng[a], max_dets[-1], iou_thrs, ious[i, k])
                 for k in range(K) for a in range(A) for i in range(n_img)}
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [eval_imgs[k, a, i] for i in range(n_img)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    if nd:
                        recall[t, k, a, m] = rc[-1]
                    else:
                        recall[t, k, a, m] = 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def _summarize(precision, recall, ap, iou_thr=None, area="all", max_det=100, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
    mind = [i for i, md in enumerate(max_dets) if md == max_det]
    if ap == 1:
        s = precision
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind]
    else:
        s = recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, aind, mind]
    return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])


def summarize(precision, recall):
    """COCOeval.summarize's twelve numbers (before x 100; -1 = nothing evaluated)"""
    st = lambda *a, **k: _summarize(precision, recall, *a, **k)
    return [st(1), st(1, iou_thr=.5), st(1, iou_thr=.75), st(1, area="small"), st(1, area="medium"), st(1, area="large"),
            st(0, max_det=1), st(0, max_det=10), st(0, max_det=100), st(0, area="small"), st(0, area="medium"),
            st(0, area="large")]


def derive_results(precision, recall, class_names):
    """detectron2 COCOEvaluator._derive_coco_results (+ the recall half of summarize): percent, nan where nothing was evaluated"""
    stats = summarize(precision, recall)
    pct = lambda v: float(v * 100 if v >= 0 else "nan")
    bbox = {n: pct(stats[i]) for i, n in enumerate(["AP", "AP50", "AP75", "APs", "APm", "APl"])}
    for idx, name in enumerate(class_names):
        p = precision[:, :, idx, 0, -1]
        p = p[p > -1]
        bbox["AP-" + name] = float(np.mean(p) * 100) if p.size else float("nan")
    rec = {n: pct(stats[6 + i]) for i, n in enumerate(["AR@1", "AR@10", "AR@100", "ARs", "ARm", "ARl"])}
    return {"bbox": bbox, "bbox_recall": rec}


def match_tables(seg_list, iou_thrs=IOU_THRS, area_rng=AREA_RNG, max_det=MAX_DETS[-1]):
    """the three tables of ptmi_coco_match for a LIST of segments laid out one after the other (detections in visiting
    order): gt_ignore (A, NG), dt_match (A, T, ND), dt_ignore (A, T, ND)"""
    A, T = len(area_rng), len(iou_thrs)
    gi, dm, di = [[] for _ in range(A)], [[] for _ in range(A)], [[] for _ in range(A)]
    for seg in seg_list:
        ious = compute_iou(seg, max_det)
        for a in range(A):
            e = evaluate_img(seg, area_rng[a], max_det, iou_thrs, ious)
            if e is None:
                continue
            gi[a].append(e["gtIgnoreDataset"])
            dm[a].append(e["dtMatchPos"])
            di[a].append(e["dtIgnore"].astype(np.int64))
    cat = lambda parts, ax, empty: np.concatenate(parts, axis=ax) if parts else np.zeros(empty, dtype=np.int64)
    return (np.stack([cat(gi[a], 0, (0,)) for a in range(A)]).astype(np.int32),
            np.stack([cat(dm[a], 1, (T, 0)) for a in range(A)]).astype(np.int32),
            np.stack([cat(di[a], 1, (T, 0)) for a in range(A)]).astype(np.int32))
