"""GPU (pytest -m gpu): the ROI pooler variants -- MODEL.ROI_BOX_HEAD.POOLER_TYPE in {ROIAlignV2, ROIAlign, ROIPool} and
POOLER_SAMPLING_RATIO >= 0 -- against the numpy restatements of tests/roi_pooler_ref.py (pinned to oracle.d2.roi_align by
tests/test_roi_pooler_cpu.py), on the maps and the box set of tests/test_ops_gpu.py::test_roi_align.

Tolerances: ROIAlign forward rtol 1e-5 / atol 1e-5 and backward rtol 1e-4 / atol 1e-4 (those of test_ops_gpu.py::test_roi_align);
ROIPool forward values and argmax EXACT, backward 1e-4 / 1e-4; model level 1e-4."""
import math

import numpy as np
import pytest
import torch

from oracle import pt as opt
from tests import roi_pooler_ref as ref
from tests.helpers import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAPS = [(25, 31), (70, 27), (83, 83)]
VARIANTS = [(0, 0), (0, 2), (1, 2), (1, 1)]           # (aligned, sampling_ratio)


def _inputs(fh, fw, seed=23):
    gen = torch.Generator().manual_seed(seed)
    feat = torch.randn(2, 18, fh, fw, generator=gen)
    rois = ref.special_boxes(gen, 40, fh, fw)
    assert float((rois[:, 3] - rois[:, 1]).min()) < 16.0            # exercises the non-aligned max(., 1) clamp
    gy = torch.randn(40, 18, 7, 7, generator=gen)
    return feat, rois, gy


def _grouped(rois):
    order = torch.argsort(rois[:, 0], stable=True)
    rs = rois[order]
    offs = torch.tensor([0, int((rs[:, 0] == 0).sum()), len(rs)], dtype=torch.int32, device=DEV)
    return order, rs, offs


# ============================================================================ ROIAlign variants
@pytest.mark.parametrize("aligned,ratio", VARIANTS)
@pytest.mark.parametrize("fh,fw", MAPS)
def test_roi_align_variants_forward_and_backward(fh, fw, aligned, ratio):
    from probabilisticteacher_amd import ops
    feat, rois, gy = _inputs(fh, fw)
    want = ref.roi_align(feat.numpy(), rois.numpy(), 7, 1 / 16, bool(aligned), ratio)
    want_g = ref.roi_align_backward(gy.numpy(), rois.numpy(), feat.shape, 7, 1 / 16, bool(aligned), ratio)
    # ungrouped: gather kernel + atomic scatter
    fd = feat.to(DEV).requires_grad_()
    out = ops.roi_align(fd, rois.to(DEV), 7, 1 / 16, None, bool(aligned), ratio)
    close(out.detach().cpu().numpy(), want, 1e-5, 1e-5, f"roi_align fwd aligned={aligned} ratio={ratio}")
    out.backward(gy.to(DEV))
    close(fd.grad.cpu().numpy(), want_g, 1e-4, 1e-4, f"roi_align bwd aligned={aligned} ratio={ratio}")
    empty = ops.roi_align(fd, torch.zeros((0, 5), device=DEV), 7, 1 / 16, None, bool(aligned), ratio)
    assert empty.shape == (0, 18, 7, 7)
    # grouped by image: LDS-plane forward with the per-ROI tables, band backward without atomics
    order, rs, offs = _grouped(rois)
    fd2 = feat.to(DEV).requires_grad_()
    out2 = ops.roi_align(fd2, rs.to(DEV), 7, 1 / 16, offs, bool(aligned), ratio)
    close(out2.detach().cpu().numpy(), want[order.numpy()], 1e-5, 1e-5, f"grouped fwd aligned={aligned} ratio={ratio}")
    assert torch.equal(ops.roi_align(fd2, rs.to(DEV), 7, 1 / 16, offs, bool(aligned), ratio), out2), "grouped forward repeatable"
    out2.backward(gy[order].to(DEV))
    close(fd2.grad.cpu().numpy(), want_g, 1e-4, 1e-4, f"grouped bwd aligned={aligned} ratio={ratio}")
    fd3 = feat.to(DEV).requires_grad_()
    ops.roi_align(fd3, rs.to(DEV), 7, 1 / 16, offs, bool(aligned), ratio).backward(gy[order].to(DEV))
    assert torch.equal(fd3.grad, fd2.grad), "grouped backward is atomic-free: bitwise repeatable"


def test_roi_align_ex_rejects_bad_variant_arguments():
    from probabilisticteacher_amd import _lib, ops
    feat, rois, _ = _inputs(25, 31)
    fd, rd = feat.to(DEV), rois.to(DEV)
    out = torch.empty((40, 18, 7, 7), device=DEV)
    for aligned, ratio in ((2, 0), (-1, 0), (1, -1)):
        with pytest.raises(_lib.PtmiError, match="sampling_ratio"):
            _lib.call("ptmi_roi_align_fwd_ex", ops._ptr(fd), ops._ptr(rd), ops._ptr(out), 2, 18, 25, 31, 40, 7, 1 / 16, ops._stream(),
                      aligned, ratio)
    with pytest.raises(ValueError, match="sampling_ratio"):
        ops.roi_align(fd, rd, 7, 1 / 16, None, True, -3)


# ============================================================================ ROIPool
@pytest.mark.parametrize("fh,fw", MAPS)
def test_roi_pool_forward_exact_and_backward(fh, fw):
    from probabilisticteacher_amd import ops
    feat, rois, gy = _inputs(fh, fw)
    rois[:, 0] = 1.0                                   # image 0 has no ROI: its gradient rows must be exactly zero
    want, want_arg = ref.roi_pool(feat.numpy(), rois.numpy(), 7, 1 / 16)
    assert (want_arg == -1).any() and (want_arg >= 0).any()          # empty bins (the boxes over the border) and real ones
    fd = feat.to(DEV).requires_grad_()
    out, arg = ops.roi_pool(fd, rois.to(DEV), 7, 1 / 16, return_argmax=True)
    assert arg.dtype == torch.int32 and not arg.requires_grad
    assert np.array_equal(arg.cpu().numpy(), want_arg), "ROIPool argmax must equal the restatement"
    assert np.array_equal(out.detach().cpu().numpy(), want), "ROIPool values must equal the restatement bit for bit"
    out.backward(gy.to(DEV))
    want_g = ref.roi_pool_backward(gy.numpy(), want_arg, rois.numpy(), feat.shape)
    close(fd.grad.cpu().numpy(), want_g, 1e-4, 1e-4, "roi_pool bwd")
    assert not fd.grad[0].any(), "an image without ROIs gets an exactly zero gradient"
    # both images used
    feat, rois, gy = _inputs(fh, fw, seed=31)
    want, want_arg = ref.roi_pool(feat.numpy(), rois.numpy(), 7, 1 / 16)
    fd = feat.to(DEV).requires_grad_()
    out, arg = ops.roi_pool(fd, rois.to(DEV), 7, 1 / 16, return_argmax=True)
    assert np.array_equal(arg.cpu().numpy(), want_arg) and np.array_equal(out.detach().cpu().numpy(), want)
    out.backward(gy.to(DEV))
    close(fd.grad.cpu().numpy(), ref.roi_pool_backward(gy.numpy(), want_arg, rois.numpy(), feat.shape), 1e-4, 1e-4, "roi_pool bwd")


def test_roi_pool_plateau_first_maximum_and_empty_r():
    from probabilisticteacher_amd import ops
    feat = torch.zeros(1, 3, 12, 12)
    feat[0, :, 4:8, 4:8] = 7.0                         # a plateau over several bins: the first cell in raster order wins
    feat[0, 1] = 2.5                                   # a constant plane: every bin's argmax is its first cell
    rois = torch.tensor([[0.0, 0.0, 0.0, 11.0, 11.0], [0.0, 3.0, 2.0, 9.0, 10.0], [0.0, 5.0, 5.0, 6.0, 6.0]])
    want, want_arg = ref.roi_pool(feat.numpy(), rois.numpy(), 3, 1.0)
    assert want_arg[0, 0, 1, 1] == 4 * 12 + 4 and want[0, 0, 1, 1] == 7.0          # bin rows / cols 4..7: first cell (4, 4)
    out, arg = ops.roi_pool(feat.to(DEV), rois.to(DEV), 3, 1.0, return_argmax=True)
    assert np.array_equal(arg.cpu().numpy(), want_arg) and np.array_equal(out.cpu().numpy(), want)
    # R = 0: zeros of shape (0, C, P, P), a zero gradient
    fd = feat.to(DEV).requires_grad_()
    e = ops.roi_pool(fd, torch.zeros((0, 5), device=DEV), 3, 1.0)
    assert e.shape == (0, 3, 3, 3)
    e.sum().backward()
    assert fd.grad.shape == feat.shape and not fd.grad.any()


# ============================================================================ the default is untouched
def test_default_pooler_is_the_direct_roi_align_call():
    from probabilisticteacher_amd import ops
    from probabilisticteacher_amd.modeling.roi_heads import ROIPooler
    from probabilisticteacher_amd.structures import Boxes
    feat, rois, gy = _inputs(25, 31)
    order, rs, offs = _grouped(rois)
    n0 = int(offs[1])
    pooler = ROIPooler(7, (1 / 16,), 0, "ROIAlignV2")
    f1 = feat.to(DEV).requires_grad_()
    got = pooler([f1], [Boxes(rs[:n0, 1:].to(DEV)), Boxes(rs[n0:, 1:].to(DEV))])
    assert isinstance(got, torch.Tensor)
    got.backward(gy[order].to(DEV))
    f2 = feat.to(DEV).requires_grad_()
    direct = ops.roi_align(f2, rs.to(DEV), 7, 1 / 16, offs)
    direct.backward(gy[order].to(DEV))
    assert torch.equal(got, direct) and torch.equal(f1.grad, f2.grad)
    f3 = feat.to(DEV).requires_grad_()
    kw = ops.roi_align(f3, rs.to(DEV), 7, 1 / 16, offs, aligned=True, sampling_ratio=0)
    kw.backward(gy[order].to(DEV))
    assert torch.equal(kw, direct) and torch.equal(f3.grad, f2.grad)
    # ungrouped too
    assert torch.equal(ops.roi_align(f2, rois.to(DEV), 7, 1 / 16, aligned=True, sampling_ratio=0), ops.roi_align(f2, rois.to(DEV), 7, 1 / 16))
    # the variants go through the same pooler class
    for ptype, ratio, fn in (("ROIAlign", 2, lambda f, r: ops.roi_align(f, r, 7, 1 / 16, offs, False, 2)),
                             ("ROIPool", 0, lambda f, r: ops.roi_pool(f, r, 7, 1 / 16))):
        p = ROIPooler(7, (1 / 16,), ratio, ptype)
        a = p([feat.to(DEV)], [Boxes(rs[:n0, 1:].to(DEV)), Boxes(rs[n0:, 1:].to(DEV))])
        assert torch.equal(a, fn(feat.to(DEV), rs.to(DEV))) and not torch.equal(a, direct)


# ============================================================================ model level
K, ANCHOR = 8, "DifferentiableAnchorGenerator"
SETTINGS = [("ROIPool", 0), ("ROIAlign", 2)]


def _cfg(ptype, ratio, amp=False):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg("configs/pt/final_c2f.yaml", [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "MODEL.ROI_HEADS.NUM_CLASSES", K, "UNSUPNET.BURN_UP_STEP", 0,
        "MODEL.ANCHOR_GENERATOR.NAME", ANCHOR,
        "MODEL.ROI_BOX_HEAD.POOLER_TYPE", ptype, "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", ratio,
        "SOLVER.AMP.ENABLED", bool(amp)])


def _load_params(model, params):
    sd = model.state_dict()
    assert set(sd) == set(params), set(sd) ^ set(params)
    with torch.no_grad():
        for k, v in params.items():
            sd[k].copy_(v)


def _records(seed, n, h=128, w=176):
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    g = torch.Generator().manual_seed(seed)
    boxes = torch.tensor([[10.0, 20.0, 90.0, 100.0], [60.0, 30.0, 170.0, 120.0], [5.0, 5.0, 60.0, 50.0]])
    recs = []
    for _ in range(n):
        img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        inst = FreeInstances((h, w))
        inst.gt_boxes, inst.gt_classes = Boxes(boxes.clone()), torch.tensor([0, 3, 7])
        recs.append({"image": img, "height": h, "width": w, "instances": inst})
    return recs


@pytest.mark.parametrize("ptype,ratio", SETTINGS)
def test_model_supervised_branch_uses_the_configured_pooler(ptype, ratio):
    """roi_heads' predictions on the supervised branch against a manual composition: the restatement's pooled features for the
    same sampled proposals through the model's own box head and predictor."""
    from probabilisticteacher_amd import modeling
    from probabilisticteacher_amd.modeling import sampling
    model = modeling.build_model(_cfg(ptype, ratio)).train()
    _load_params(model, opt.golden_params(opt.Cfg(num_classes=K, anchor_generator=ANCHOR), 1))
    seen = {}
    h1 = model.roi_heads.box_pooler.register_forward_hook(
        lambda m, inp, out: seen.update(feat=inp[0][0].detach(), boxes=[b.tensor.detach() for b in inp[1]], pooled=out))
    h2 = model.roi_heads.box_predictor.register_forward_hook(lambda m, inp, out: seen.update(pred=out))
    sampling.set_key_source(sampling.perm_key_source(opt.SeededPerm(5)))
    try:
        losses, _, _, _ = model(_records(0, 2), branch="supervised")
    finally:
        sampling.set_key_source(None)
        h1.remove()
        h2.remove()
    assert all(math.isfinite(float(v)) for v in losses.values()), losses
    assert isinstance(seen["pooled"], torch.Tensor) and seen["pooled"].dtype == torch.float32
    rois = torch.cat([torch.cat([torch.full((len(b), 1), float(i)), b.cpu()], 1) for i, b in enumerate(seen["boxes"])], 0).numpy()
    assert len(rois) > 100
    feat = seen["feat"].cpu().numpy()
    if ptype == "ROIPool":
        pooled, _ = ref.roi_pool(feat, rois, 7, 1 / 16)
    else:
        pooled = ref.roi_align(feat, rois, 7, 1 / 16, aligned=False, sampling_ratio=ratio)
    close(seen["pooled"].detach().cpu().numpy(), pooled, 1e-4, 1e-4, "pooled features")
    with torch.no_grad():
        scores, deltas = model.roi_heads.box_predictor(model.roi_heads.box_head(torch.from_numpy(pooled).to(DEV)))
    close(seen["pred"][0].detach().cpu().numpy(), scores.cpu().numpy(), 1e-4, 1e-4, "cls_score vs manual composition")
    close(seen["pred"][1].detach().cpu().numpy(), deltas.cpu().numpy(), 1e-4, 1e-4, "bbox_pred vs manual composition")
    # the teacher (inference) path goes through the same pooler
    seen.clear()
    h1 = model.roi_heads.box_pooler.register_forward_hook(lambda m, inp, out: seen.update(pooled=out, n=sum(len(b) for b in inp[1])))
    try:
        with torch.no_grad():
            model(_records(0, 2), branch="unsup_data_weak")
    finally:
        h1.remove()
    assert isinstance(seen["pooled"], torch.Tensor) and seen["pooled"].shape == (seen["n"], 512, 7, 7)


def _mutual_step(ptype, ratio, amp=False):
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.modeling import sampling
    from probabilisticteacher_amd.modeling.roi_heads import DeferredROIAlign
    tr = PTrainer(_cfg(ptype, ratio, amp), ratio_fn=lambda: 0.9)
    assert tr.operand_rounding == ("bf16" if amp else None)
    params = opt.golden_params(opt.Cfg(num_classes=K, anchor_generator=ANCHOR), 1)
    _load_params(tr.model, params)
    _load_params(tr.model_teacher, params)
    kinds = []
    for m in (tr.model, tr.model_teacher):
        m.roi_heads.box_pooler.register_forward_hook(lambda mod, inp, out: kinds.append(type(out)))
    lab, unl = _records(0, 2), _records(1, 1)
    sampling.set_key_source(sampling.perm_key_source(opt.SeededPerm(9)))
    try:
        m = tr.run_step(([lab[0]], [lab[1]], [dict(unl[0])], [dict(unl[0])]))
    finally:
        sampling.set_key_source(None)
    deferred = any(issubclass(k, DeferredROIAlign) for k in kinds)
    assert len(kinds) >= 3                             # teacher, supervised, unsupervised
    del tr
    return dict(m), deferred


LOSS_KEYS = [k + s for s in ("_sup", "_unsup") for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc")]


def test_trainer_mutual_learning_step_follows_the_pooler_setting():
    base, _ = _mutual_step("ROIAlignV2", 0)
    assert all(math.isfinite(base[k]) for k in LOSS_KEYS), base
    for ptype, ratio in SETTINGS:
        m, deferred = _mutual_step(ptype, ratio)
        print(f"\n[{ptype} ratio {ratio}] " + ", ".join(f"{k} {m[k]:.6f}" for k in LOSS_KEYS))
        assert all(math.isfinite(m[k]) for k in LOSS_KEYS), (ptype, m)
        assert not deferred
        assert m["loss_cls_sup"] != base["loss_cls_sup"], f"{ptype}: the setting did not reach the step"


def test_amp_step_with_roi_pool_gets_a_tensor_from_the_pooler():
    from probabilisticteacher_amd import ops
    try:
        base, deferred = _mutual_step("ROIAlignV2", 0, amp=True)
        assert deferred, "ROIAlignV2 / ratio 0 keeps the fused bf16 hand-over under SOLVER.AMP.ENABLED"
        m, deferred = _mutual_step("ROIPool", 0, amp=True)
    finally:
        ops.set_operand_rounding(None)
    assert not deferred, "ROIPool must hand the box head the materialised tensor"
    assert all(math.isfinite(m[k]) for k in LOSS_KEYS), m
    assert m["loss_cls_sup"] != base["loss_cls_sup"]
