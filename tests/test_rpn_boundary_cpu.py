"""MODEL.RPN.BOUNDARY_THRESH on the CPU: the config key, Boxes.inside_box against the oracle's D2 statement, and the torch form
of the relabel (sampling.boundary_relabel, then sampling.keyed_relabel or the positive mask) against the restatement of
rpn.py:414-433 in tests/rpn_boundary_ref.py -- labels and positive index lists exactly equal.  The RPN's two loss methods run here
with their HIP operators replaced by torch stand-ins (the matcher's by the oracle's pairwise_iou + Matcher, a second witness
beside the restatement's own)."""
import os

import pytest
import torch

from oracle import d2
from tests import rpn_boundary_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/pt/final_c2f.yaml")


def _cfg(*opts, file=YAML):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(file, ["MODEL.DEVICE", "cpu", "MODEL.VGG.PRETRAIN", ""] + list(opts))


# ------------------------------------------------------------------------------------------------ config
def test_config_key_default_overrides_and_type_rule(tmp_path):
    assert _cfg().MODEL.RPN.BOUNDARY_THRESH == -1
    for v in (0, 16):
        assert _cfg("MODEL.RPN.BOUNDARY_THRESH", v).MODEL.RPN.BOUNDARY_THRESH == v
        assert _cfg("MODEL.RPN.BOUNDARY_THRESH", str(v)).MODEL.RPN.BOUNDARY_THRESH == v          # as the command line hands it over
        y = tmp_path / f"t{v}.yaml"
        y.write_text(f'_BASE_: "{YAML}"\nMODEL:\n  RPN: {{BOUNDARY_THRESH: {v}}}\n')
        got = _cfg(file=str(y)).MODEL.RPN.BOUNDARY_THRESH
        assert got == v and type(got) is int
    for bad in (0.5, "16.0", True):
        with pytest.raises(ValueError, match="Type mismatch"):
            _cfg("MODEL.RPN.BOUNDARY_THRESH", bad)
    y = tmp_path / "float.yaml"
    y.write_text(f'_BASE_: "{YAML}"\nMODEL:\n  RPN: {{BOUNDARY_THRESH: 0.0}}\n')
    with pytest.raises(ValueError, match="Type mismatch"):
        _cfg(file=str(y))


def _rpn(cfg):
    from probabilisticteacher_amd.modeling.backbone import ShapeSpec
    from probabilisticteacher_amd.modeling.rpn import GuassianRPN
    return GuassianRPN(cfg, {"vgg_block5": ShapeSpec(channels=8, stride=16)})


def test_rpn_reads_the_key_and_wants_an_integer():
    from probabilisticteacher_amd import ops
    assert _rpn(_cfg()).anchor_boundary_thresh == -1
    assert _rpn(_cfg("MODEL.RPN.BOUNDARY_THRESH", 16)).anchor_boundary_thresh == 16
    assert _rpn(_cfg("MODEL.RPN.BOUNDARY_THRESH", -7)).anchor_boundary_thresh == -7              # any negative value: off
    for bad in (0.0, 16.5, True, "0", None):
        with pytest.raises(TypeError, match="BOUNDARY_THRESH"):
            ops.check_boundary_thresh(bad)
    hand = _cfg().clone()
    hand.MODEL.RPN.BOUNDARY_THRESH = 0.0                     # a config built by hand, past the type rule
    with pytest.raises(TypeError, match="BOUNDARY_THRESH"):
        _rpn(hand)


# ------------------------------------------------------------------------------------------------ Boxes.inside_box
@pytest.mark.parametrize("t", [0, 16])
def test_inside_box_equals_the_oracle_on_hand_made_boxes(t):
    from probabilisticteacher_amd.structures import Boxes
    h, w = 300, 400
    nan = float("nan")
    rows = [([-t, -t, w + t - 0.5, h + t - 0.5], True),        # x1 == -t, y1 == -t: inside; x2 == w + t - 0.5: inside
            ([10.0, 10.0, w + t, 100.0], False),               # x2 == w + t: outside (strict)
            ([10.0, 10.0, 100.0, h + t], False),               # y2 == h + t: outside (strict)
            ([10.0, 10.0, w + t - 0.5, 100.0], True),
            ([-t - 0.5, 10.0, 100.0, 100.0], False),
            ([10.0, -t - 0.5, 100.0, 100.0], False),
            ([10.0, 10.0, 100.0, 100.0], True),
            ([nan, 10.0, 100.0, 100.0], False), ([10.0, nan, 100.0, 100.0], False),
            ([10.0, 10.0, nan, 100.0], False), ([10.0, 10.0, 100.0, nan], False),
            ([10.0, 10.0, float("inf"), 100.0], False), ([-float("inf"), 10.0, 100.0, 100.0], False)]
    x = torch.tensor([r for r, _ in rows], dtype=torch.float32)
    want = torch.tensor([v for _, v in rows])
    got = Boxes(x).inside_box((h, w), t)
    assert got.dtype == torch.bool and torch.equal(got, want)
    assert torch.equal(got, d2.Boxes(x).inside_box((h, w), t)) and torch.equal(got, ref.inside_box(x, (h, w), t))
    assert torch.equal(Boxes(x).inside_box((h, w)), d2.Boxes(x).inside_box((h, w)))              # the default threshold, 0
    assert Boxes(torch.zeros(0, 4)).inside_box((h, w), t).shape == (0,)


# ------------------------------------------------------------------------------------------------ the relabel chain
@pytest.fixture(scope="module")
def case():
    return ref.case(_cfg().MODEL.ANCHOR_GENERATOR.ANCHOR[0])


def _oracle_match(boxes, anchors):
    """the Matcher's output for the batch from the ORACLE's D2 functions (not the restatement's)"""
    m = d2.Matcher([0.3, 0.7], [0, -1, 1], allow_low_quality_matches=True)
    out = [m(d2.pairwise_iou(d2.Boxes(b), d2.Boxes(anchors))) for b in boxes]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out]).to(torch.int8)


def test_the_inputs_meet_their_guards(case):
    for t in (0, 16):
        ref.guards(case["anchors"], case["boxes"], case["sizes"], t)
    # the restatement's Matcher and the oracle's agree on these inputs (two witnesses for everything before the relabel)
    midx, lab, _ = ref.label_anchors(case["anchors"], case["boxes"], case["sizes"], -1)
    omidx, olab = _oracle_match(case["boxes"], case["anchors"])
    assert torch.equal(lab, olab) and torch.equal(midx[lab == 1], omidx[lab == 1])


@pytest.mark.parametrize("t", [0, 16, -1])
def test_torch_relabel_equals_the_restatement(case, t):
    from probabilisticteacher_amd.modeling import sampling
    anchors, boxes, sizes, keys = case["anchors"], case["boxes"], case["sizes"], case["keys"]
    _, matched = _oracle_match(boxes, anchors)
    got = sampling.boundary_relabel(matched.clone(), anchors, sizes, t)
    _, want, _ = ref.label_anchors(anchors, boxes, sizes, t)
    assert got.dtype == torch.int8 and torch.equal(got, want)
    if t < 0:
        assert torch.equal(got, matched)
    else:
        assert int((got != matched).sum()) > 0 and bool(((got == matched) | (got == -1)).all())
    # supervised: injected keys, 64 @ 25 % (both quotas bite on image 0) and the shipped 256 @ 25 %
    for num, frac in ((64, 0.25), (256, 0.25)):
        sampling.set_key_source(lambda lab, s, bg: keys)
        try:
            sampled = sampling.keyed_relabel(got, num, frac, 0)
        finally:
            sampling.set_key_source(None)
        _, want_s = ref.labels_sup(anchors, boxes, sizes, t, keys, num, frac)
        assert torch.equal(sampled, want_s)
        assert torch.equal(torch.nonzero(sampled.view(-1) == 1).squeeze(1), torch.nonzero(want_s.view(-1) == 1).squeeze(1))
        assert bool((sampled[got == -1] == -1).all()), "an ignored anchor was sampled"
    # unsupervised: the positive row list
    _, want_flat = ref.positives_unsup(anchors, boxes, sizes, t)
    assert torch.equal(torch.nonzero(got.view(-1) == 1).squeeze(1), want_flat)


def _instances(case, pseudo):
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    out = []
    for size, b, soft, sig in zip(case["sizes"], case["boxes"], case["soft"], case["sigma"]):
        inst = FreeInstances(size)
        if pseudo:
            inst.pseudo_boxes, inst.scores_logists, inst.boxes_sigma = Boxes(b), soft, sig
        else:
            inst.gt_boxes = Boxes(b)
        out.append(inst)
    return out


def _run_losses(case, t, monkeypatch, num=64):
    """GuassianRPN._losses_sup / _losses_unsup on CPU tensors; every HIP operator is a torch stand-in that records what the loss
    would see: the sampled labels, and the positive rows (logits and the first delta column hold their own flat index)"""
    from probabilisticteacher_amd import ops
    from probabilisticteacher_amd.modeling import sampling
    anchors, boxes, keys = case["anchors"], case["boxes"], case["keys"]
    n, r = len(boxes), anchors.shape[0]
    rpn = _rpn(_cfg("MODEL.RPN.BOUNDARY_THRESH", t, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", num))
    seen = {}

    def match(gt_all, counts, anc, box_counts, thr, labels, low):          # exactly the existing wrapper's arguments
        assert box_counts is None and list(thr) == [0.3, 0.7] and list(labels) == [0, -1, 1] and low is True
        midx, lab = _oracle_match(torch.split(gt_all, list(counts)), anc)
        off = torch.tensor([0] + list(counts)).cumsum(0).to(torch.int32)
        return midx, lab, None, off, None
    monkeypatch.setattr(ops, "iou_match_batched", match)
    monkeypatch.setattr(ops, "bce_logits_sum", lambda x, lab, inv: seen.setdefault("labels", lab.clone()).sum() * 0.0 + x.sum() * inv)
    monkeypatch.setattr(ops, "get_deltas", lambda src, tgt, w: tgt - src)
    monkeypatch.setattr(ops, "rpn_soft_obj_loss", lambda T, x, tau, lam, efl, inv: (
        seen.setdefault("unsup_rows", x.detach().long().clone()).sum() * 0.0 + x.sum() * inv, torch.ones(x.shape[0], dtype=torch.uint8)))
    monkeypatch.setattr(rpn, "nll_loss", lambda d, tg, inv: seen.setdefault("sup_rows", d[:, 0].detach().long().clone()).sum() * 0.0 + d.sum() * inv)
    monkeypatch.setattr(rpn, "kl_loss", lambda q, mu, sig, fg, tau, lam, efl, red, inv: q.sum() * inv)
    logits = torch.arange(n * r, dtype=torch.float32).view(n, r)
    d8 = torch.zeros(n, r, 8)
    d8[..., 0] = logits
    sampling.set_key_source(lambda lab, s, bg: keys)
    try:
        out_s = rpn._losses_sup(anchors, logits, d8, _instances(case, False))
    finally:
        sampling.set_key_source(None)
    out_u = rpn._losses_unsup(anchors, logits, d8, _instances(case, True))
    assert set(out_s) == set(out_u) == {"loss_rpn_cls", "loss_rpn_loc"}
    return seen


@pytest.mark.parametrize("t", [0, 16, -1])
def test_rpn_loss_methods_relabel_before_sampling_and_before_the_positive_mask(case, t, monkeypatch):
    seen = _run_losses(case, t, monkeypatch)
    _, want = ref.labels_sup(case["anchors"], case["boxes"], case["sizes"], t, case["keys"], 64, 0.25)
    assert torch.equal(seen["labels"], want)
    assert torch.equal(seen["sup_rows"], torch.nonzero(want.view(-1) == 1).squeeze(1))
    _, flat = ref.positives_unsup(case["anchors"], case["boxes"], case["sizes"], t)
    assert torch.equal(seen["unsup_rows"], flat)
    if t >= 0:           # ... and the key changes what the losses see (on the parent commit it does not)
        _, off = ref.labels_sup(case["anchors"], case["boxes"], case["sizes"], -1, case["keys"], 64, 0.25)
        assert not torch.equal(seen["labels"], off)
        assert not torch.equal(flat, ref.positives_unsup(case["anchors"], case["boxes"], case["sizes"], -1)[1])


def test_image_size_is_the_instances_own_not_the_canvas(case, monkeypatch):
    """the three images share one canvas and differ in size: an anchor inside (320, 448) and outside (300, 400) is ignored in image 1
    only -- visible in the image WITHOUT boxes, whose inside anchors are its only negatives"""
    seen = _run_losses(case, 0, monkeypatch, num=100000)             # a quota nothing reaches: no subsampling
    inside = torch.stack([ref.inside_box(case["anchors"], s, 0) for s in case["sizes"]])
    assert torch.equal(seen["labels"][1] == 0, inside[1]) and int(inside[1].sum()) < int(inside[0].sum())
