"""GPU: MODEL.RPN.BOUNDARY_THRESH from the kernel up to the trainer, against the restatement of rpn.py:414-433 in
tests/rpn_boundary_ref.py.

Shapes: stride 16, the nine reference anchors on a 20 x 28 map (5 040 anchors per image: 20 workgroups of 256, the last one
partly filled), three images of sizes (320, 448), (300, 400), (320, 437) on one canvas, 6 / 0 / 3 boxes.  Labels, indices and row
lists are compared exactly; the two losses at the project's loss tolerance (tests/test_model_gpu.py: rtol 1e-4, atol 1e-6) against
float64 figures.  The inputs meet `rpn_boundary_ref.guards`: per image with boxes there are positives and negatives on both sides of
the inside test, so no assertion below can hold while the key is ignored."""
import ctypes
import math

import pytest
import torch

from tests import rpn_boundary_ref as ref
from tests.helpers import close
from tests.test_deterministic_gpu import _assert_same_run, _batches, _cfg as _trainer_cfg, _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR, LAB = [0.3, 0.7], [0, -1, 1]


def _cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg("configs/pt/final_c2f.yaml", ["MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", ""] + list(opts))


@pytest.fixture(scope="module")
def case():
    c = ref.case(_cfg().MODEL.ANCHOR_GENERATOR.ANCHOR[0])
    assert c["anchors"].shape == (5040, 4) and [len(b) for b in c["boxes"]] == [6, 0, 3]
    before, inside = ref.guards(c["anchors"], c["boxes"], c["sizes"], 0)
    for i in (0, 2):         # the guards once more, in the open: conditions on the inputs at t = 0
        assert int(((before[i] == 1) & inside[i]).sum()) >= 1 and int(((before[i] == 1) & ~inside[i]).sum()) >= 1
        assert int(((before[i] == 0) & inside[i]).sum()) >= 1 and int(((before[i] == 0) & ~inside[i]).sum()) >= 1
    ref.guards(c["anchors"], c["boxes"], c["sizes"], 16)
    c["gt_all"], c["counts"] = torch.cat(c["boxes"]).to(DEV), [len(b) for b in c["boxes"]]
    return c


class _Spy:
    """records the names `_lib.call` is asked for (as tests/test_deterministic_gpu.py does)"""

    def __enter__(self):
        from probabilisticteacher_amd import _lib
        self.lib, self.real, self.names = _lib, _lib.call, []

        def spy(name, *a):
            self.names.append(name)
            return self.real(name, *a)
        _lib.call = spy
        return self.names

    def __exit__(self, *exc):
        self.lib.call = self.real


def _todays_entry(gt_all, counts, anchors):
    """ptmi_iou_match_batched called directly, past the wrapper"""
    from probabilisticteacher_amd import _lib, ops
    n, r = len(counts), anchors.shape[0]
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    gt_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    midx = torch.empty((n, r), dtype=torch.int64, device=DEV)
    mlab = torch.empty((n, r), dtype=torch.int8, device=DEV)
    miou = torch.empty((n, r), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(off[-1], 1), dtype=torch.float32, device=DEV)
    _lib.call("ptmi_iou_match_batched", ops._ptr(gt_all), ops._ptr(gt_off), ops._ptr(anchors), None, n, r, off[-1],
              (ctypes.c_float * 2)(*THR), (ctypes.c_int * 3)(*LAB), 2, 1, ops._ptr(midx), ops._ptr(mlab), ops._ptr(miou), ops._ptr(ws),
              ops._stream())
    torch.cuda.synchronize()
    return midx, mlab, miou, gt_off, ws


# ------------------------------------------------------------------------------------------------ 1. the operator
def test_operator_equals_the_restatement_and_leaves_the_match_alone(case):
    from probabilisticteacher_amd import _lib, ops
    anchors, sizes = case["anchors"].to(DEV), case["sizes"]
    midx0, mlab0, miou0, gt_off, ws = _todays_entry(case["gt_all"], case["counts"], anchors)
    _, off_labels, _ = ref.label_anchors(case["anchors"], case["boxes"], sizes, -1)
    assert torch.equal(mlab0.cpu(), off_labels)                                             # today's entry, for the record
    for t in (0, 16):
        with _Spy() as names:
            midx, mlab, miou, _, box_off = ops.iou_match_batched(case["gt_all"], case["counts"], anchors, None, THR, LAB, True, sizes, t)
        assert names == ["ptmi_iou_match_batched_bounds"] and box_off is None
        want_idx, want, _ = ref.label_anchors(case["anchors"], case["boxes"], sizes, t)
        assert mlab.dtype == torch.int8 and torch.equal(mlab.cpu(), want), f"t = {t}: labels"
        assert torch.equal(midx, midx0) and torch.equal(miou, miou0), f"t = {t}: matched_idx / matched_iou are not today's bits"
        assert torch.equal(midx.cpu()[want == 1], want_idx[want == 1])
        assert int((mlab != mlab0).sum()) > 0
        # the sizes as a device tensor: the same call
        dev_sizes = ops.dev_sizes_hw(sizes, DEV)
        assert dev_sizes.shape == (3, 2) and dev_sizes.tolist() == [[float(h), float(w)] for h, w in sizes]
        assert torch.equal(ops.iou_match_batched(case["gt_all"], case["counts"], anchors, None, THR, LAB, True, dev_sizes, t)[1], mlab)
    # off: the existing entry alone, whatever else is handed in, and today's bits
    for extra in ((), (sizes, -1), (None, -5)):
        with _Spy() as names:
            midx, mlab, miou, _, _ = ops.iou_match_batched(case["gt_all"], case["counts"], anchors, None, THR, LAB, True, *extra)
        assert names == ["ptmi_iou_match_batched"]
        assert torch.equal(mlab, mlab0) and torch.equal(midx, midx0) and torch.equal(miou, miou0)
    # a NaN coordinate is outside (a value test: the anchor buffer keeps its size).  The other anchors keep the labels today's
    # entry gives them on the same buffer, relabelled by the restatement's inside test.
    bad = case["anchors"].clone()
    bad[77, 2] = float("nan")
    bad[4001, 1] = float("nan")
    _, lab_nan, _, _, _ = _todays_entry(case["gt_all"], case["counts"], bad.to(DEV))
    inside = torch.stack([ref.inside_box(bad, s, 16) for s in sizes])
    assert not bool(inside[:, [77, 4001]].any())
    got = ops.iou_match_batched(case["gt_all"], case["counts"], bad.to(DEV), None, THR, LAB, True, sizes, 16)[1].cpu()
    assert torch.equal(got, torch.where(inside, lab_nan.cpu(), torch.tensor(-1, dtype=torch.int8))) and bool((got[:, [77, 4001]] == -1).all())
    # argument errors, before any launch
    with pytest.raises(_lib.PtmiError, match="shared box set"):
        ops.iou_match_batched(case["gt_all"], case["counts"], anchors.repeat(3, 1), [5040] * 3, THR, LAB, True, sizes, 0)
    with pytest.raises(_lib.PtmiError, match="image_sizes_hw"):
        ops.iou_match_batched(case["gt_all"], case["counts"], anchors, None, THR, LAB, True, None, 0)
    with pytest.raises(_lib.PtmiError, match="image_sizes_hw"):
        ops.iou_match_batched(case["gt_all"], case["counts"], anchors, None, THR, LAB, True, sizes[:2], 0)
    with pytest.raises(TypeError, match="BOUNDARY_THRESH"):
        ops.iou_match_batched(case["gt_all"], case["counts"], anchors, None, THR, LAB, True, sizes, 0.0)
    n, r = 3, anchors.shape[0]
    out = [torch.empty((n, r), dtype=d, device=DEV) for d in (torch.int64, torch.int8, torch.float32)]
    dev_sizes = ops.dev_sizes_hw(sizes, DEV)

    def raw(box_off, sizes_ptr, t):
        _lib.call("ptmi_iou_match_batched_bounds", ops._ptr(case["gt_all"]), ops._ptr(gt_off), ops._ptr(anchors), box_off, n, r,
                  int(case["gt_all"].shape[0]), (ctypes.c_float * 2)(*THR), (ctypes.c_int * 3)(*LAB), 2, 1, ops._ptr(out[0]),
                  ops._ptr(out[1]), ops._ptr(out[2]), ops._ptr(ws), sizes_ptr, t, ops._stream())
    with pytest.raises(_lib.PtmiError, match="box_off must be NULL"):
        raw(ops._ptr(gt_off), ops._ptr(dev_sizes), 0.0)
    with pytest.raises(_lib.PtmiError, match="boundary_thresh"):
        raw(None, ops._ptr(dev_sizes), -1.0)
    with pytest.raises(_lib.PtmiError, match="sizes_hw"):
        raw(None, None, 0.0)
    with pytest.raises(_lib.PtmiError, match="boundary_thresh"):
        raw(None, ops._ptr(dev_sizes), float("nan"))


# ------------------------------------------------------------------------------------------------ 2. / 3. the two loss methods
def _rpn(t, num):
    from probabilisticteacher_amd.modeling.backbone import ShapeSpec
    from probabilisticteacher_amd.modeling.rpn import GuassianRPN
    cfg = _cfg("MODEL.RPN.BOUNDARY_THRESH", t, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", num)
    return cfg, GuassianRPN(cfg, {"vgg_block5": ShapeSpec(channels=8, stride=16)}).to(DEV)


def _instances(case, pseudo):
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    out = []
    for size, b, soft, sig in zip(case["sizes"], case["boxes"], case["soft"], case["sigma"]):
        inst = FreeInstances(size)
        if pseudo:
            inst.pseudo_boxes, inst.scores_logists, inst.boxes_sigma = Boxes(b.to(DEV)), soft.to(DEV), sig.to(DEV)
        else:
            inst.gt_boxes = Boxes(b.to(DEV))
        out.append(inst)
    return out


def _sup(case, t, num, statistics=False):
    """-> (losses as floats, the sampled labels the classification loss was handed, names of the entries called, the statistics)"""
    from probabilisticteacher_amd import ops
    from probabilisticteacher_amd.modeling import sampling
    from probabilisticteacher_amd.modeling.statistics import StatisticsSink
    _, rpn = _rpn(t, num)
    sink = rpn.statistics = StatisticsSink() if statistics else None
    seen, real = {}, ops.bce_logits_sum

    def bce(x, lab, inv):
        seen["labels"] = lab.clone()
        return real(x, lab, inv)
    sampling.set_key_source(lambda lab, s, bg: case["keys"].to(lab.device))
    ops.bce_logits_sum = bce
    try:
        with _Spy() as names:
            out = rpn._losses_sup(case["anchors"].to(DEV), case["logits"].to(DEV), case["d8"].to(DEV), _instances(case, False))
    finally:
        ops.bce_logits_sum = real
        sampling.set_key_source(None)
    stats = sink.metrics(sink.packed(DEV).tolist()) if statistics else None
    return {k: float(v) for k, v in out.items()}, seen["labels"].cpu(), names, stats


@pytest.mark.parametrize("num", [64, 256])          # 64 @ 25 %: the positive quota bites too (image 0 has 39 inside positives)
def test_supervised_labels_and_losses_end_to_end(case, num):
    got, labels, names, stats = _sup(case, 0, num, statistics=True)
    assert "ptmi_iou_match_batched_bounds" in names and "ptmi_iou_match_batched" not in names
    midx, want = ref.labels_sup(case["anchors"], case["boxes"], case["sizes"], 0, case["keys"], num, 0.25)
    assert torch.equal(labels, want), "sampled labels"
    inside = torch.stack([ref.inside_box(case["anchors"], s, 0) for s in case["sizes"]])
    assert bool((labels[~inside] == -1).all()) and int((labels >= 0).sum()) == 3 * num
    # the statistics count the labels after relabel and subsampling (rpn.py:222-228)
    assert stats == {"rpn/num_pos_anchors": int((want == 1).sum()) / 3, "rpn/num_neg_anchors": int((want == 0).sum()) / 3}
    assert stats["rpn/num_pos_anchors"] + stats["rpn/num_neg_anchors"] <= num
    figures = ref.losses_sup(case["anchors"], case["logits"], case["d8"], case["boxes"], midx, want, num)
    off, off_labels, off_names, _ = _sup(case, -1, num)
    assert "ptmi_iou_match_batched" in off_names and "ptmi_iou_match_batched_bounds" not in off_names
    midx_off, want_off = ref.labels_sup(case["anchors"], case["boxes"], case["sizes"], -1, case["keys"], num, 0.25)
    figures_off = ref.losses_sup(case["anchors"], case["logits"], case["d8"], case["boxes"], midx_off, want_off, num)
    print(f"[boundary] sup num={num} t=0 {got} restated {figures} | t=-1 {off} restated {figures_off}")
    assert torch.equal(off_labels, want_off)
    for k in ("loss_rpn_cls", "loss_rpn_loc"):
        close(got[k], figures[k], 1e-4, 1e-6, f"t = 0 {k}")
        close(off[k], figures_off[k], 1e-4, 1e-6, f"t = -1 {k}")
        assert got[k] != off[k] and abs(figures[k] - figures_off[k]) > 10 * (1e-4 * abs(figures[k]) + 1e-6), \
            f"{k} does not depend on BOUNDARY_THRESH"


def _unsup(case, t, logits=None):
    from probabilisticteacher_amd import ops
    logits = case["logits"] if logits is None else logits
    _, rpn = _rpn(t, 256)
    seen, real = {}, ops.rpn_soft_obj_loss

    def soft(T, x, *a):
        seen["x"] = x.detach().clone()
        return real(T, x, *a)
    ops.rpn_soft_obj_loss = soft
    try:
        with _Spy() as names:
            out = rpn._losses_unsup(case["anchors"].to(DEV), logits.to(DEV), case["d8"].to(DEV), _instances(case, True))
    finally:
        ops.rpn_soft_obj_loss = real
    return {k: float(v) for k, v in out.items()}, seen["x"].cpu(), names


def test_unsupervised_branch_positive_rows_and_losses(case):
    cfg = _cfg()
    U = cfg.UNSUPNET
    index = torch.arange(case["logits"].numel(), dtype=torch.float32).view_as(case["logits"])     # exact in fp32: a row's logit is its index
    res = {}
    for t in (0, -1):
        got, x, names = _unsup(case, t)
        assert ("ptmi_iou_match_batched_bounds" in names) == (t >= 0) and ("ptmi_iou_match_batched" in names) == (t < 0)
        midx, flat = ref.positives_unsup(case["anchors"], case["boxes"], case["sizes"], t)
        assert torch.equal(_unsup(case, t, index)[1].long(), flat), f"t = {t}: positive rows"
        assert torch.equal(x, case["logits"].reshape(-1)[flat])
        figures = ref.losses_unsup(case["anchors"], case["logits"], case["d8"], case["boxes"], case["soft"], case["sigma"], midx, flat,
                                   256, U.TAU, U.EFL_LAMBDA, U.EFL)
        print(f"[boundary] unsup t={t} rows {flat.numel()} {got} restated {figures}")
        for k in ("loss_rpn_cls", "loss_rpn_loc"):
            close(got[k], figures[k], 1e-4, 1e-6, f"t = {t} {k}")
        res[t] = (got, figures, flat)
    assert res[0][2].numel() < res[-1][2].numel()
    for k in ("loss_rpn_cls", "loss_rpn_loc"):
        assert res[0][0][k] != res[-1][0][k] and abs(res[0][1][k] - res[-1][1][k]) > 10 * (1e-4 * abs(res[0][1][k]) + 1e-6), \
            f"{k} does not depend on BOUNDARY_THRESH"


# ------------------------------------------------------------------------------------------------ 4. / 5. the trainer
def test_trainer_trains_with_the_key_and_stays_deterministic():
    cfg = _trainer_cfg("SEED", 3, "MODEL.RPN.BOUNDARY_THRESH", 0)
    batches = _batches(cfg, steps=4)                          # two burn-in steps, two mutual-learning steps (the joint student pass)
    with _Spy() as names:
        a = _run(cfg, batches, statistics=True)
    assert "ptmi_iou_match_batched_bounds" in names and a[0].iter == 4 and any(k.endswith("_unsup") for k in a[1][-1])
    for m in a[1]:
        assert all(math.isfinite(v) for v in m.values()), m
        assert 0 < m["rpn/num_pos_anchors"] + m["rpn/num_neg_anchors"] <= cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE
    b = _run(cfg, batches, statistics=True)
    _assert_same_run(a, b, "SEED 3, BOUNDARY_THRESH 0")
    off = _run(_trainer_cfg("SEED", 3, "MODEL.RPN.BOUNDARY_THRESH", -1), batches[:1], statistics=True)
    assert a[1][0]["loss_rpn_cls"] != off[1][0]["loss_rpn_cls"], "the first step's loss_rpn_cls does not depend on BOUNDARY_THRESH"


def test_off_is_off():
    batches = _batches(_trainer_cfg("SEED", 3), steps=2)
    with _Spy() as names:
        off = _run(_trainer_cfg("SEED", 3, "MODEL.RPN.BOUNDARY_THRESH", -1), batches)
    assert "ptmi_iou_match_batched" in names and not [n for n in names if n.endswith("_bounds")]
    plain = _run(_trainer_cfg("SEED", 3), batches)            # a config that does not mention the key
    _assert_same_run(off, plain, "BOUNDARY_THRESH -1 against no key")


def test_joint_student_pass_hands_each_branch_its_own_sizes():
    """one mutual-learning step whose two student branches share a canvas and differ in image sizes: the supervised call gets the
    sizes of the labelled images' instances, the unsupervised call those of the pseudo-label instances"""
    from bench import synth_records
    from probabilisticteacher_amd import ops
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    cfg = _trainer_cfg("SEED", 3, "MODEL.RPN.BOUNDARY_THRESH", 0, "UNSUPNET.BURN_UP_STEP", 0)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    gen = torch.Generator().manual_seed(5)
    sup, unsup = [(256, 384), (240, 384)], [(256, 384), (256, 352)]

    def recs(sizes):
        return [synth_records(gen, 1, h, w, K, DEV)[0] for h, w in sizes]
    batch = (recs(sup), recs(sup), recs(unsup), recs(unsup))
    seed_all_rng(3)
    tr = PTrainer(cfg)
    seen, joint, real, real_joint = [], [], ops.iou_match_batched, tr.model.forward_joint

    def match(gt_all, counts, boxes, box_counts, *rest):
        if box_counts is None:
            seen.append((list(counts), [tuple(s) for s in rest[3]], rest[4]))
        return real(gt_all, counts, boxes, box_counts, *rest)

    def forward_joint(*a, **k):
        joint.append(1)
        return real_joint(*a, **k)
    ops.iou_match_batched, tr.model.forward_joint = match, forward_joint
    try:
        m = tr.run_step(batch)
    finally:
        ops.iou_match_batched = real
    assert joint == [1] and all(math.isfinite(v) for v in m.values())
    assert [s[1] for s in seen] == [sup + sup, unsup] and [s[2] for s in seen] == [0, 0], seen
    assert seen[0][0] == [len(r["instances"]) for r in batch[0] + batch[1]]
