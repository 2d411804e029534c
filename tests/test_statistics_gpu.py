"""GPU: the two counting kernels (ops.cls_stats, ops.label_counts) against their torch restatements, integer-exact, and
PTrainer(statistics=True) end to end: every logged statistic recomputed in torch from what the supervised losses saw, the same
bits with and without statistics under SEED 0, no further host read, and the keys in metrics.json."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests import statistics_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc")
GRID_ROWS = 1024 * 256          # rows / labels one pass of the counting kernels' largest grid covers


# ------------------------------------------------------------------------------------------------ kernels
def _cls_case(R, C, seed, all_background=False):
    """gt holds -1, every foreground class and K; a third of the rows carry two equal maxima, another third three (where
    K + 1 allows), placed at random columns -- the background column included"""
    g = torch.Generator().manual_seed(seed)
    K = C - 1
    scores = torch.randn(R, C, generator=g)
    for i in range(R):
        ties = (i % 3) + 1                        # 1, 2 or 3 columns share the maximum
        if ties > 1:
            cols = torch.randperm(C, generator=g)[:min(ties, C)]
            scores[i, cols] = scores[i].max() + 1.0
    if all_background:
        return scores, torch.full((R,), K)
    gt = torch.randint(-1, K + 1, (R,), generator=g)
    if R >= 3:
        gt[:3] = torch.tensor([-1, 0, K])
    return scores, gt


@pytest.mark.parametrize("C", [2, 9, 21, 81])
@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 257, 4099])
def test_cls_stats_is_integer_exact(R, C):
    from probabilisticteacher_amd import ops
    scores, gt = _cls_case(R, C, 1000 * C + R)
    if R >= 3:
        assert {-1, 0, C - 1} <= set(gt.tolist())
    got = ops.cls_stats(scores.to(DEV), gt.to(DEV))
    assert got.dtype == torch.int32 and got.shape == (4,) and got.is_cuda
    want = ref.cls_counts(scores, gt)
    print(f"cls_stats R={R} C={C}: kernel {got.tolist()} torch {want}")
    assert got.tolist() == want


def test_cls_stats_all_background_and_past_one_grid():
    from probabilisticteacher_amd import ops
    scores, gt = _cls_case(257, 9, 5, all_background=True)
    got = ops.cls_stats(scores.to(DEV), gt.to(DEV)).tolist()
    assert got == ref.cls_counts(scores, gt) and got[1:] == [0, 0, 0]
    # more rows than one pass of the largest grid: the grid-stride loop takes a second turn
    g = torch.Generator().manual_seed(6)
    scores = torch.randint(0, 3, (GRID_ROWS + 3, 2), generator=g).float()          # every other row a tie
    gt = torch.randint(-1, 2, (GRID_ROWS + 3,), generator=g)
    assert ops.cls_stats(scores.to(DEV), gt.to(DEV)).tolist() == ref.cls_counts(scores, gt)


@pytest.mark.parametrize("shape", [(1, 1), (2, 256), (3, 4097), (0, 5), (1, GRID_ROWS + 5)])
def test_label_counts_is_integer_exact(shape):
    from probabilisticteacher_amd import ops
    g = torch.Generator().manual_seed(shape[0] * 7 + shape[1])
    labels = torch.randint(-1, 2, shape, generator=g, dtype=torch.int8)
    got = ops.label_counts(labels.to(DEV))
    assert got.dtype == torch.int32 and got.shape == (2,) and got.is_cuda
    print(f"label_counts {shape}: kernel {got.tolist()} torch {ref.label_counts(labels)}")
    assert got.tolist() == ref.label_counts(labels)


# ------------------------------------------------------------------------------------------------ the step
def _cfg(*opts):
    """the small step of tests/test_deterministic_gpu.py: final_c2f, 2 + 2 images"""
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2] + list(opts))


def _batches(cfg, steps, seed=77):
    from bench import synth_records
    gen = torch.Generator().manual_seed(seed)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    return [tuple(synth_records(gen, 2, 256, 384, K, DEV) for _ in range(4)) for _ in range(steps)]


def _capture(tr):
    """wrap the two supervised loss methods of the student: what they saw lands in the returned dict"""
    from probabilisticteacher_amd.modeling import sampling
    seen = {}
    rpn, pred = tr.model.proposal_generator, tr.model.roi_heads.box_predictor
    rpn_losses, cls_losses, relabel = rpn._losses_sup, pred.losses, sampling.keyed_relabel

    def losses_sup(anchors, logits, d8, gt_instances):
        def keep(*a, **k):
            seen["labels"] = relabel(*a, **k)
            return seen["labels"]
        sampling.keyed_relabel = keep
        try:
            return rpn_losses(anchors, logits, d8, gt_instances)
        finally:
            sampling.keyed_relabel = relabel

    def losses(predictions, proposals):
        seen["scores"] = predictions[0].detach().clone()
        seen["gt"] = [p.gt_classes.clone() for p in proposals]
        return cls_losses(predictions, proposals)
    rpn._losses_sup, pred.losses = losses_sup, losses
    return seen


def _expected(seen, K, mutual):
    labels, gt = seen["labels"], torch.cat(seen["gt"]).cpu()
    n = labels.shape[0]
    pos, neg = ref.label_counts(labels)
    want = {"rpn/num_pos_anchors": pos / n, "rpn/num_neg_anchors": neg / n}
    want.update(ref.cls_metrics(seen["scores"], gt))
    bg = [int((g == K).sum()) for g in seen["gt"]]                         # roi_heads.py:243-244
    fg = [g.numel() - b for g, b in zip(seen["gt"], bg)]
    want["roi_head/num_target_fg_samples_supervised"] = sum(fg) / len(fg)
    want["roi_head/num_target_bg_samples_supervised"] = sum(bg) / len(bg)
    if mutual:
        want["roi_head/num_target_fg_samples_unsupervised"] = want["roi_head/num_target_bg_samples_unsupervised"] = 0.0
    counts = {"rpn/num_pos_anchors": (pos, n), "rpn/num_neg_anchors": (neg, n)}
    acc, nfg, fg_acc, fn = ref.cls_counts(seen["scores"], gt)
    counts.update({"fast_rcnn/cls_accuracy": (acc, gt.numel()), "fast_rcnn/fg_cls_accuracy": (fg_acc, nfg),
                   "fast_rcnn/false_negative": (fn, nfg)})
    return want, counts


@pytest.mark.parametrize("joint", [True, False])
def test_step_statistics_equal_their_torch_restatement(joint):
    from probabilisticteacher_amd.engine import PTrainer
    cfg = _cfg("UNSUPNET.BURN_UP_STEP", 1)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    torch.manual_seed(3)
    tr = PTrainer(cfg, ratio_fn=lambda: 0.8, statistics=True)
    tr.joint_student_pass = joint
    joint_calls = []
    fj = tr.model.forward_joint
    tr.model.forward_joint = lambda *a, **k: (joint_calls.append(1), fj(*a, **k))[1]
    seen = _capture(tr)
    for step, batch in enumerate(_batches(cfg, 2)):
        mutual = step == 1
        seen.clear()
        m = tr.run_step(batch)
        assert seen["labels"].dtype == torch.int8 and seen["labels"].dim() == 2 and seen["scores"].shape[1] == K + 1
        want, counts = _expected(seen, K, mutual)
        names = [k + "_sup" for k in LOSSES] + [k + "_unsup" for k in LOSSES] if mutual else list(LOSSES)
        assert {k for k in m if "/" not in k} == set(names) | {"total_loss", "grad_norm", "data_time"}, sorted(m)
        assert {k for k in m if "/" in k} == set(want), sorted(m)
        assert set(want) >= ref.RPN_KEYS | ref.SUP_KEYS | {"fast_rcnn/cls_accuracy"}
        assert (set(want) >= ref.UNSUP_KEYS) == mutual
        for k, v in want.items():
            print(f"step {step} joint={joint} {k}: logged {m[k]!r} torch {v!r}")
            assert abs(m[k] - v) <= 1e-6, (k, m[k], v)
            if k in counts and counts[k][1] > 0:
                assert round(m[k] * counts[k][1]) == counts[k][0], (k, m[k], counts[k])
    assert len(joint_calls) == (1 if joint else 0)


def _count_host_reads(fn):
    """run fn() and count the calls of Tensor.cpu / .item / .tolist it makes"""
    n = {"cpu": 0, "item": 0, "tolist": 0}
    real = {k: getattr(torch.Tensor, k) for k in n}

    def counting(k):
        def f(self, *a, **kw):
            n[k] += 1
            return real[k](self, *a, **kw)
        return f
    for k in n:
        setattr(torch.Tensor, k, counting(k))
    try:
        out = fn()
    finally:
        for k in n:
            setattr(torch.Tensor, k, real[k])
    return out, n


@pytest.fixture(scope="module")
def seed0_pair():
    """two SEED 0 trainers on the same batches, statistics off and on: 2 burn-in + 2 mutual-learning steps each"""
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    cfg = _cfg("SEED", 0, "UNSUPNET.BURN_UP_STEP", 2)
    batches = _batches(cfg, 4)
    runs = {}
    for on in (False, True):
        seed_all_rng(0)
        tr = PTrainer(cfg, statistics=on)
        metrics, reads = [], []
        for b in batches:
            m, n = _count_host_reads(lambda: dict(tr.run_step(b)))
            metrics.append(m)
            reads.append(n)
        torch.cuda.synchronize()
        runs[on] = SimpleNamespace(trainer=tr, metrics=metrics, reads=reads)
    return runs


def test_statistics_leave_a_seeded_run_bit_identical(seed0_pair):
    off, on = seed0_pair[False], seed0_pair[True]
    assert off.trainer.deterministic and off.trainer.iter == on.trainer.iter == 4
    assert torch.equal(off.trainer.student.flat, on.trainer.student.flat), "student parameters differ"
    assert torch.equal(off.trainer.teacher.flat, on.trainer.teacher.flat), "teacher parameters differ"
    for step, (a, b) in enumerate(zip(off.metrics, on.metrics)):
        assert not [k for k in a if "/" in k] and set(b) - set(a) >= ref.RPN_KEYS | ref.SUP_KEYS
        assert set(a) <= set(b) and any(k.endswith("_unsup") for k in a) == (step >= 2)
        for k in a:
            if k != "data_time":
                assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), f"step {step}: {k} {a[k]!r} (off) vs {b[k]!r} (on)"


def test_statistics_add_no_host_read(seed0_pair):
    off, on = seed0_pair[False], seed0_pair[True]
    for step, (a, b) in enumerate(zip(off.reads, on.reads)):
        print(f"step {step}: host reads off {a} on {b}")
        assert a == b and a["cpu"] >= 1, f"step {step}: host reads {a} without statistics, {b} with"


@pytest.mark.parametrize("statistics", [True, False])
def test_train_writes_the_statistics_into_metrics_json(tmp_path, monkeypatch, statistics):
    from probabilisticteacher_amd import checkpoint
    from probabilisticteacher_amd.engine import PTrainer
    # (the periodic checkpointer would write the two models at the last iteration: not what this test is about)
    monkeypatch.setattr(checkpoint, "PeriodicCheckpointer", lambda *a, **k: SimpleNamespace(step=lambda it: None))
    cfg = _cfg("UNSUPNET.BURN_UP_STEP", 1, "OUTPUT_DIR", str(tmp_path))
    torch.manual_seed(4)
    tr = PTrainer(cfg, data_loader=iter(_batches(cfg, 2, seed=78)), statistics=statistics)
    tr.train(max_iter=2, log_period=1, run_eval=False)
    lines = [json.loads(l) for l in open(tmp_path / "metrics.json")]
    assert [l["iteration"] for l in lines] == [0, 1]
    for it, line in enumerate(lines):
        slashed = {k for k in line if "/" in k}
        if not statistics:
            assert not slashed, slashed
            continue
        assert slashed >= ref.RPN_KEYS | ref.SUP_KEYS | {"fast_rcnn/cls_accuracy"}
        assert slashed <= ref.RPN_KEYS | ref.SUP_KEYS | ref.CLS_KEYS | ref.UNSUP_KEYS
        assert (slashed >= ref.UNSUP_KEYS) == (it == 1) and ("loss_cls_unsup" in line) == (it == 1)
        assert 0.0 <= line["fast_rcnn/cls_accuracy"] <= 1.0
        assert 0 < line["rpn/num_pos_anchors"] + line["rpn/num_neg_anchors"] <= cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE
