"""CPU: the logged statistics (modeling/statistics.py) from raw counts to `last_metrics` -- the host half of
PTrainer(statistics=True).  `_write_metrics` is driven on a stand-in object, as tests/test_distributed_cpu.py drives it."""
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import statistics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_KEYS = {"loss_cls", "loss_rpn_loc", "total_loss", "grad_norm", "data_time"}


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def _write(rec, world=1):
    from probabilisticteacher_amd.engine.trainer import PTrainer
    me = SimpleNamespace(world_size=world, METRIC_KEYS=PTrainer.METRIC_KEYS, last_metrics={})
    PTrainer._write_metrics(me, rec, 0.5, torch.tensor([9.0]))
    return me.last_metrics


def _losses():
    return {"loss_cls": torch.tensor(1.5), "loss_rpn_loc": torch.tensor(0.25)}


def _sink(rpn=(30, 100), images=4, cls=(300, 40, 10, 25), rows=512):
    from probabilisticteacher_amd.modeling.statistics import StatisticsSink
    s = StatisticsSink()
    s.put_rpn_labels(_i32(*rpn), images, 4000)
    s.put_classification(_i32(*cls), rows)
    s.put_scalar("roi_head/num_target_fg_samples_supervised", 37.5)
    s.put_scalar("roi_head/num_target_bg_samples_supervised", 474.5)
    return s


def test_single_rank_ratios_from_raw_counts():
    from probabilisticteacher_amd.modeling import statistics
    m = _write(dict(_losses(), **{statistics.KEY: _sink()}))
    assert set(m) == OLD_KEYS | ref.RPN_KEYS | ref.CLS_KEYS | ref.SUP_KEYS
    assert m["loss_cls"] == 1.5 and m["total_loss"] == 1.75 and m["grad_norm"] == 3.0 and m["data_time"] == 0.5
    assert m["rpn/num_pos_anchors"] == 30 / 4 and m["rpn/num_neg_anchors"] == 100 / 4
    assert m["fast_rcnn/cls_accuracy"] == 300 / 512
    assert m["fast_rcnn/fg_cls_accuracy"] == 10 / 40 and m["fast_rcnn/false_negative"] == 25 / 40
    assert m["roi_head/num_target_fg_samples_supervised"] == 37.5 and m["roi_head/num_target_bg_samples_supervised"] == 474.5


def test_foreground_ratios_absent_without_foreground():
    from probabilisticteacher_amd.modeling import statistics
    m = _write(dict(_losses(), **{statistics.KEY: _sink(cls=(500, 0, 0, 0))}))
    assert set(m) == OLD_KEYS | ref.RPN_KEYS | ref.SUP_KEYS | {"fast_rcnn/cls_accuracy"}
    assert m["fast_rcnn/cls_accuracy"] == 500 / 512


def test_no_classifier_keys_without_rows():
    from probabilisticteacher_amd.modeling import statistics
    m = _write(dict(_losses(), **{statistics.KEY: _sink(cls=(0, 0, 0, 0), rows=0)}))
    assert set(m) == OLD_KEYS | ref.RPN_KEYS | ref.SUP_KEYS


def test_without_statistics_the_key_set_is_the_old_one():
    assert set(_write(_losses())) == OLD_KEYS


def test_mutual_learning_step_adds_the_unsupervised_zeros():
    from probabilisticteacher_amd.modeling import statistics
    s = _sink()
    s.put_scalar("roi_head/num_target_fg_samples_unsupervised", 0.0)
    s.put_scalar("roi_head/num_target_bg_samples_unsupervised", 0.0)
    m = _write({"loss_cls_sup": torch.tensor(1.0), "loss_cls_unsup": torch.tensor(2.0), statistics.KEY: s})
    assert set(m) == ({"loss_cls_sup", "loss_cls_unsup", "total_loss", "grad_norm", "data_time"} | ref.RPN_KEYS | ref.CLS_KEYS |
                      ref.SUP_KEYS | ref.UNSUP_KEYS)
    assert m["roi_head/num_target_fg_samples_unsupervised"] == 0.0 and m["roi_head/num_target_bg_samples_unsupervised"] == 0.0
    s.reset()
    assert s.metrics([0] * s.N_COUNTS) == {} and s.packed("cpu").tolist() == [0.0] * s.N_COUNTS


def test_counts_beyond_fp32_exactness_are_refused():
    from probabilisticteacher_amd.modeling.statistics import StatisticsSink
    s = StatisticsSink()
    s.put_rpn_labels(_i32(1, 2), 1, (1 << 24) - 1)
    s.put_classification(_i32(1, 1, 1, 0), (1 << 24) - 1)
    with pytest.raises(AssertionError):
        s.put_rpn_labels(_i32(1, 2), 1, 1 << 24)
    with pytest.raises(AssertionError):
        s.put_classification(_i32(1, 1, 1, 0), 1 << 24)
    # the largest count that passes survives the fp32 trip
    s.put_classification(_i32((1 << 24) - 1, 3, 2, 1), (1 << 24) - 1)
    assert s.packed("cpu").tolist()[2] == float((1 << 24) - 1)


# ------------------------------------------------------------------------------------------------ two gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from probabilisticteacher_amd.modeling import statistics
    if rank == 0:
        rec = {"loss_cls": torch.tensor(1.0), "loss_rpn_loc": torch.tensor(3.0)}
        sink = _sink()
    else:
        rec = {"loss_cls": torch.tensor(2.0)}
        sink = _sink(rpn=(8, 248), images=2, cls=(100, 0, 0, 0), rows=256)
    rec[statistics.KEY] = sink
    q.put((rank, _write(rec, world)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_average_the_losses_and_keep_their_own_statistics():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):                                          # the losses: rank 0's keys, averaged over both ranks, as before
        assert out[r]["loss_cls"] == 1.5 and out[r]["loss_rpn_loc"] == 1.5 and out[r]["total_loss"] == 3.0
        assert out[r]["grad_norm"] == 3.0 and out[r]["data_time"] == 0.5
    assert set(out[0]) == OLD_KEYS | ref.RPN_KEYS | ref.CLS_KEYS | ref.SUP_KEYS
    assert out[0]["rpn/num_pos_anchors"] == 7.5 and out[0]["rpn/num_neg_anchors"] == 25.0
    assert out[0]["fast_rcnn/cls_accuracy"] == 300 / 512 and out[0]["fast_rcnn/fg_cls_accuracy"] == 0.25
    assert set(out[1]) == OLD_KEYS | ref.RPN_KEYS | ref.SUP_KEYS | {"fast_rcnn/cls_accuracy"}      # no foreground on rank 1
    assert out[1]["rpn/num_pos_anchors"] == 4.0 and out[1]["rpn/num_neg_anchors"] == 124.0
    assert out[1]["fast_rcnn/cls_accuracy"] == 100 / 256


# ------------------------------------------------------------------------------------------------ the restatements, by hand
def test_restatements_on_a_hand_made_case():
    K = 3
    scores = torch.tensor([[1.0, 5.0, 2.0, 0.0],     # gt 1: right
                           [3.0, 3.0, 1.0, 0.0],     # gt 0: two equal maxima, the first one wins: right
                           [3.0, 3.0, 1.0, 0.0],     # gt 1: the same tie: wrong
                           [0.0, 0.0, 0.0, 0.0],     # gt K (background): four equal maxima -> class 0: wrong
                           [0.0, 1.0, 2.0, 9.0],     # gt 2: predicted background: a false negative
                           [0.0, 1.0, 2.0, 9.0],     # gt K: right, not foreground
                           [2.0, 1.0, 0.0, 0.0],     # gt -1 (ignored): neither accurate nor foreground
                           [0.0, 0.0, 7.0, 7.0]])    # gt 2: tie between class 2 and background -> class 2: right
    gt = torch.tensor([1, 0, 1, K, 2, K, -1, 2])
    assert ref.cls_counts(scores, gt) == [4, 5, 3, 1]
    assert ref.cls_metrics(scores, gt) == {"fast_rcnn/cls_accuracy": 4 / 8, "fast_rcnn/fg_cls_accuracy": 3 / 5,
                                           "fast_rcnn/false_negative": 1 / 5}
    bg = torch.full((3,), K)
    assert ref.cls_counts(scores[:3], bg) == [0, 0, 0, 0] and ref.cls_metrics(scores[:3], bg) == {"fast_rcnn/cls_accuracy": 0.0}
    assert ref.cls_counts(scores[:0], gt[:0]) == [0, 0, 0, 0] and ref.cls_metrics(scores[:0], gt[:0]) == {}
    labels = torch.tensor([[1, 0, -1, 0], [-1, -1, 1, 1]], dtype=torch.int8)
    assert ref.label_counts(labels) == [3, 2] and ref.label_counts(labels[:0]) == [0, 0]
    # the sink turns exactly these counts into exactly these scalars
    from probabilisticteacher_amd.modeling.statistics import StatisticsSink
    s = StatisticsSink()
    s.put_classification(_i32(*ref.cls_counts(scores, gt)), gt.numel())
    s.put_rpn_labels(_i32(*ref.label_counts(labels)), labels.shape[0], labels.numel())
    assert s.metrics(s.packed("cpu").tolist()) == dict(ref.cls_metrics(scores, gt), **{"rpn/num_pos_anchors": 1.5,
                                                                                     "rpn/num_neg_anchors": 1.0})


# ------------------------------------------------------------------------------------------------ statistics=False launches nothing
def _cfg(tmp_path):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), ["MODEL.DEVICE", "cpu", "MODEL.VGG.PRETRAIN", "",
                                                                       "OUTPUT_DIR", str(tmp_path)])


def _run_supervised_losses(model, monkeypatch):
    """the two supervised loss methods on the CPU, their HIP operators replaced by torch stand-ins; `ops.cls_stats` and
    `ops.label_counts` raise"""
    from probabilisticteacher_amd import ops
    from probabilisticteacher_amd.structures import Boxes, FreeInstances

    def boom(*a, **k):
        raise AssertionError("a counting kernel was reached")
    monkeypatch.setattr(ops, "cls_stats", boom)
    monkeypatch.setattr(ops, "label_counts", boom)
    monkeypatch.setattr(ops, "softmax_ce_mean", lambda s, t: torch.nn.functional.cross_entropy(s, t))
    monkeypatch.setattr(ops, "get_deltas", lambda src, tgt, w: tgt - src)
    monkeypatch.setattr(ops, "bce_logits_sum", lambda x, lab, inv: x.sum() * inv)
    n, r, K = 2, 40, model.roi_heads.num_classes
    lab = torch.full((n, r), -1, dtype=torch.int8)
    lab[:, :5], lab[:, 5:30] = 1, 0
    monkeypatch.setattr(ops, "iou_match_batched", lambda gt, counts, boxes, bc, thr, labels, low: (
        torch.zeros((n, r), dtype=torch.int64), lab.clone(), None, torch.tensor([0, 1, 2], dtype=torch.int32), None))
    rpn, pred = model.proposal_generator, model.roi_heads.box_predictor
    monkeypatch.setattr(rpn, "nll_loss", lambda d, t, inv: d.sum() * inv)
    monkeypatch.setattr(pred, "nll_loss", lambda d, t, inv: d.sum() * inv)
    g = torch.Generator().manual_seed(0)
    gts = []
    for _ in range(n):
        inst = FreeInstances((64, 64))
        inst.gt_boxes = Boxes(torch.tensor([[4.0, 4.0, 40.0, 40.0]]))
        gts.append(inst)
    out = rpn._losses_sup(torch.rand(r, 4, generator=g), torch.randn(n, r, generator=g), torch.randn(n, r, 8, generator=g), gts)
    props = []
    for _ in range(n):
        p = FreeInstances((64, 64))
        p.proposal_boxes, p.gt_boxes = Boxes(torch.rand(6, 4, generator=g)), Boxes(torch.rand(6, 4, generator=g))
        p.gt_classes = torch.tensor([0, 1, K, K, K, 2])
        props.append(p)
    out.update(pred.losses((torch.randn(12, K + 1, generator=g), torch.randn(12, K * 8, generator=g)), props))
    return out


def test_statistics_off_never_reaches_the_counting_kernels(tmp_path, monkeypatch):
    from probabilisticteacher_amd.engine import PTrainer
    tr = PTrainer(_cfg(tmp_path))
    m = tr.model
    assert tr._statistics is None and m.statistics is None
    assert m.proposal_generator.statistics is None and m.roi_heads.statistics is None and m.roi_heads.box_predictor.statistics is None
    assert set(_run_supervised_losses(m, monkeypatch)) == {"loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg"}
    # ... and the same call does reach them once a sink is installed (the student only: the teacher computes no loss)
    on = PTrainer(_cfg(tmp_path), statistics=True)
    sink = on.model.statistics
    assert sink is not None and on._statistics is sink and on.model_teacher.statistics is None
    assert on.model.proposal_generator.statistics is sink and on.model.roi_heads.statistics is sink
    assert on.model.roi_heads.box_predictor.statistics is sink
    with pytest.raises(AssertionError, match="a counting kernel was reached"):
        _run_supervised_losses(on.model, monkeypatch)
