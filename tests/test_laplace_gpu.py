"""GPU (pytest -m gpu): the Laplace uncertainty model (UNSUPNET.MODEL_TYPE LAPLACE).

(1) ptmi_laplace_nll_sum / ptmi_laplace_kl_efl_loss against a float64 torch restatement of the reference expressions
    (box_regression.py:38-40, rpn.py:319-344, fast_rcnn.py:238-257) differentiated by autograd;
(2) the model's three branches against the reference's own Laplace fixtures (tools/gen_golden_laplace.py);
(3) three real PTrainer.run_step iterations against the reference's;
(4) the joint student pass against the separate passes, and (5) the SOLVER.AMP.ENABLED path, both under LAPLACE.

Tolerances are those of the Gaussian tests (tests/test_model_gpu.py): losses 1e-4, gradient norms 2e-3; op parity: loss rtol
1e-5, gradients rtol 1e-4 with an absolute floor of 1e-5 of the median nonzero reference gradient."""
import math

import numpy as np
import pytest
import torch

from oracle import pt as opt
from tests.helpers import close, keyed_perm_source, load, match_detections, perm_key_source, records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(K, anchor, tau, burn=4000, model_type="LAPLACE"):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg("configs/pt/final_c2f.yaml", [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "MODEL.ANCHOR_GENERATOR.NAME", anchor,
        "MODEL.ROI_HEADS.NUM_CLASSES", K, "UNSUPNET.TAU", list(tau), "UNSUPNET.BURN_UP_STEP", burn,
        "UNSUPNET.MODEL_TYPE", model_type])


def _load_params(model, params):
    sd = model.state_dict()
    assert set(sd) == set(params), set(sd) ^ set(params)
    with torch.no_grad():
        for k, v in params.items():
            sd[k].copy_(v)


def _gpu_records(z, prefix, n):
    from probabilisticteacher_amd.structures import FreeInstances
    return records(z, prefix, n, make_instances=FreeInstances)


def _grad_check(z, prefix, named, tol=2e-3):
    checked = 0
    for k, p in named.items():
        key = f"{prefix}_norm_{k}"
        if key not in z.files:
            continue
        g = p.grad
        nrm = float(z[key])
        close(g.double().norm().cpu(), z[key], tol, 1e-7, key)
        close(g.flatten()[:32].cpu(), z[f"{prefix}_head_{k}"], 5e-3, 2e-4 * nrm + 1e-8, f"{prefix}_head_{k}")
        checked += 1
    assert checked >= 4


# ============================================================================ (1) op parity vs float64 autograd
LOSS_RTOL, GRAD_RTOL, GRAD_FLOOR = 1e-5, 1e-4, 1e-5


def _grad_close(got, ref, what):
    ref = ref.detach().double().cpu()
    nz = ref.abs()[ref != 0]
    floor = GRAD_FLOOR * float(nz.median()) if nz.numel() else 0.0
    close(got.detach().cpu(), ref, GRAD_RTOL, floor + 1e-12, what)


def _ref_laplace_nll(d, t, inv_norm):
    """-log(laplace_dist_pdf(mu, t, sigmoid(s)) + 1e-9).sum() * inv_norm, as box_regression.py:38-40,177-183 writes it"""
    mu, var = d[:, :4], torch.sigmoid(d[:, 4:])
    pdf = torch.exp(-torch.abs(mu - t) / torch.sqrt(var + 1e-9)) / torch.sqrt(4.0 * (var + 0.3))
    return -torch.log(pdf + 1e-9).sum() * inv_norm


def _ref_laplace_kl(q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
    """rpn.py:319-344 (reduction 0: sum over the fg rows * inv_norm) / fast_rcnn.py:238-257 (reduction 1: mean)"""
    sigma_p = torch.sigmoid(slog_p)
    weight = (1 - (1 + 0.5 * torch.log(4 * sigma_p)) / (1 + math.log(2))) ** lam if efl else torch.ones_like(sigma_p)
    sigma_p = sigma_p * tau
    sigma_q, mean_q = torch.sigmoid(q[:, 4:]), q[:, :4]
    kl = (torch.sqrt(sigma_p) * torch.exp(-(torch.abs(mean_q - mu_p) / torch.sqrt(sigma_p))) / torch.sqrt(sigma_q)
          + torch.abs(mean_q - mu_p) / torch.sqrt(sigma_q) + 0.5 * torch.log(sigma_q / sigma_p) - 1) * weight
    if fg is not None:
        kl = kl[fg.bool()]
    return kl.sum() * inv_norm if reduction == 0 else kl.mean()


def _nll_inputs(rows, seed):
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(rows, 8, generator=gen)
    d[:, :4] *= 0.5
    t = d[:, :4] + torch.randn(rows, 4, generator=gen) * 0.3
    if rows >= 8:
        t[0::8] = d[0::8, :4]                    # Delta = 0 exactly
        d[1::8, 4:] = -6.0                       # var = 0.0025 ...
        t[1::8] = d[1::8, :4] + 50.0             # ... and |Delta| / sqrt(var) = 1000: pdf underflows to 0
    return d, t


@pytest.mark.parametrize("rows", [0, 1, 37, 300, 70000])      # 70000 rows = 280 000 elements > 256 x 1024: grid-stride loop
def test_laplace_nll_sum_matches_float64_autograd(rows):
    from probabilisticteacher_amd import ops
    d, t = _nll_inputs(rows, 11 + rows)
    inv = 1.0 / 512.0
    dr, tr = d.double().requires_grad_(), t.double().requires_grad_()
    ref = _ref_laplace_nll(dr, tr, inv)
    ref.backward()
    # dt requested
    dd, td = d.to(DEV).requires_grad_(), t.to(DEV).requires_grad_()
    got = ops.laplace_nll_sum(dd, td, inv)
    close(got.detach().cpu(), ref.detach(), LOSS_RTOL, 1e-12, f"laplace nll ({rows} rows)")
    (got * 2.0).backward()
    _grad_close(dd.grad, 2 * dr.grad, f"laplace nll dd ({rows} rows)")
    _grad_close(td.grad, 2 * tr.grad, f"laplace nll dt ({rows} rows)")
    # dt not requested (NULL): the same loss and dd, bit for bit
    dd2 = d.to(DEV).requires_grad_()
    got2 = ops.laplace_nll_sum(dd2, t.to(DEV), inv)
    assert got2.item() == got.item() or (math.isnan(got2.item()) and math.isnan(got.item()))
    (got2 * 2.0).backward()
    assert torch.equal(dd2.grad, dd.grad)
    if rows == 0:
        assert got.item() == 0.0
    else:
        # the underflow rows contribute -log(1e-9) each and no gradient
        if rows >= 8:
            assert not dd.grad[1::8].any() and not td.grad[1::8].any()
            assert not dd.grad[0::8, :4].any()            # sign(0) = 0


def _kl_inputs(rows, seed):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(rows, 8, generator=gen)
    q[:, :4] *= 0.5
    mu_p = q[:, :4] + torch.randn(rows, 4, generator=gen) * 0.3
    slog_p = torch.randn(rows, 4, generator=gen)
    fg = (torch.rand(rows, generator=gen) < 0.7).to(torch.uint8)
    if rows:
        fg[0] = 1                                # at least one selected row (an empty mean is NaN on both sides)
    if rows >= 8:
        mu_p[0::8] = q[0::8, :4]                 # Delta = 0 exactly
        mu_p[1::8] = q[1::8, :4] - 100.0         # exp(-|Delta| / sqrt(vp)) underflows to 0
        fg[2] = 0
    return q, mu_p, slog_p, fg


@pytest.mark.parametrize("rows", [0, 1, 37, 300, 70000])
@pytest.mark.parametrize("reduction,use_fg", [(0, True), (1, False), (1, True)])
@pytest.mark.parametrize("efl", [True, False])
def test_laplace_kl_efl_loss_matches_float64_autograd(rows, reduction, use_fg, efl):
    from probabilisticteacher_amd import ops
    q, mu_p, slog_p, fg = _kl_inputs(rows, 23 + rows)
    tau, lam, inv = 0.5, 0.5, 1.0 / 768.0
    fg = fg if use_fg else None
    qr, mr = q.double().requires_grad_(), mu_p.double().requires_grad_()
    ref = _ref_laplace_kl(qr, mr, slog_p.double(), fg, tau, lam, efl, reduction, inv)
    fgd = fg.to(DEV) if fg is not None else None
    # dmu_p requested (the RPN's differentiable anchors)
    qd, md = q.to(DEV).requires_grad_(), mu_p.to(DEV).requires_grad_()
    got = ops.laplace_kl_efl_loss(qd, md, slog_p.to(DEV), fgd, tau, lam, efl, reduction, inv)
    if rows == 0:
        assert (math.isnan(got.item()) if reduction == 1 else got.item() == 0.0), got.item()
        return
    close(got.detach().cpu(), ref.detach(), LOSS_RTOL, 1e-12, f"laplace kl ({rows} rows)")
    ref.backward()
    (got * 2.0).backward()
    _grad_close(qd.grad, 2 * qr.grad, f"laplace kl dq ({rows} rows)")
    _grad_close(md.grad, 2 * mr.grad, f"laplace kl dmu_p ({rows} rows)")
    # dmu_p not requested (NULL; fast_rcnn.py detaches mu_p): same loss and dq, bit for bit
    qd2 = q.to(DEV).requires_grad_()
    got2 = ops.laplace_kl_efl_loss(qd2, mu_p.to(DEV), slog_p.to(DEV), fgd, tau, lam, efl, reduction, inv)
    assert got2.item() == got.item()
    (got2 * 2.0).backward()
    assert torch.equal(qd2.grad, qd.grad)
    if fg is not None:
        assert not qd.grad[fg.to(DEV) == 0].any()
    if rows >= 8:
        assert not qd.grad[0, :4].any()                 # sign(0) = 0


# ============================================================================ (2) model branches vs the reference's fixture
@pytest.mark.parametrize("anchor,tag", [("DefaultAnchorGenerator", "default_anchor"),
                                        ("DifferentiableAnchorGenerator", "diff_anchor")])
def test_laplace_model_branches_match_reference_goldens(anchor, tag):
    from probabilisticteacher_amd import modeling
    from probabilisticteacher_amd.modeling import sampling
    from probabilisticteacher_amd.engine.flat import FlatParams
    z = load("model_laplace_" + tag)
    # guard: the fixture really is the Laplace model (a fixture generated with the Gaussian setting would match it)
    zg = load("model_" + tag)
    assert abs(float(z["sup_loss_box_reg"]) - float(zg["sup_loss_box_reg"])) > 0.1 * abs(float(zg["sup_loss_box_reg"]))
    K, tau = int(z["K"]), tuple(float(v) for v in z["tau"])
    cfg = _cfg(K, anchor, tau)
    ocfg = opt.Cfg(num_classes=K, anchor_generator=anchor, tau=tau)
    model = modeling.build_model(cfg)
    model.train()
    _load_params(model, opt.golden_params(ocfg, int(z["seed"])))
    flat = FlatParams(model)
    named = dict(model.named_parameters())

    # ---- supervised branch: losses + gradients vs the reference
    perm = opt.SeededPerm(77)
    sampling.set_key_source(perm_key_source(perm))
    try:
        flat.zero_grad()
        losses, _, _, _ = model(_gpu_records(z, "sup", 2), branch="supervised")
        assert perm.log == list(z["sup_perm_log"]), f"label counts differ: {perm.log} vs {list(z['sup_perm_log'])}"
        for k, v in losses.items():
            close(v.detach().cpu(), z["sup_" + k], 1e-4, 1e-6, "sup " + k)
        sum(losses.values()).backward()
        _grad_check(z, "supgrad", named)

        # ---- teacher branch (no loss: the model type does not enter it)
        sampling.set_key_source(perm_key_source(opt.SeededPerm(78)))
        with torch.no_grad():
            _, prop_rpn, prop_roih, pred = model(_gpu_records(z, "weak", 2), branch="unsup_data_weak")
        for i in range(2):
            ref_b = z[f"t_rpn{i}_proposal_boxes"]
            assert abs(len(prop_rpn[i]) - len(ref_b)) <= 2, f"proposal count {len(prop_rpn[i])} vs {len(ref_b)}"
            zero = np.zeros(len(prop_rpn[i]), np.int64)
            frac, idx = match_detections(prop_rpn[i].proposal_boxes.tensor.cpu(), zero, ref_b, np.zeros(len(ref_b), np.int64))
            assert frac >= 0.97, f"rpn proposals matched {frac:.3f}"
            ok = idx >= 0
            close(prop_rpn[i].objectness_logits.cpu()[idx[ok]], z[f"t_rpn{i}_objectness_logits"][ok], 5e-4, 1e-5, "rpn scores")
            frac, idx = match_detections(prop_roih[i].pred_boxes.tensor.cpu(), prop_roih[i].pred_classes.cpu(),
                                         z[f"t_roih{i}_pred_boxes"], z[f"t_roih{i}_pred_classes"])
            assert len(prop_roih[i]) == len(z[f"t_roih{i}_scores"]) and frac >= 0.97, f"matched {frac:.3f}"
            ok = idx >= 0
            mine = idx[ok]
            close(prop_roih[i].scores.cpu()[mine], z[f"t_roih{i}_scores"][ok], 5e-4, 1e-6, "det scores")
            close(prop_roih[i].scores_logists.cpu()[mine], z[f"t_roih{i}_scores_logists"][ok], 1e-3, 5e-4, "det logits")
            close(prop_roih[i].boxes_sigma.cpu()[mine], z[f"t_roih{i}_boxes_sigma"][ok], 1e-3, 5e-4, "det sigma")
        assert pred[0].shape == z["t_pred_scores"].shape or abs(pred[0].shape[0] - z["t_pred_scores"].shape[0]) <= 4

        # ---- unsupervised branch fed with the REFERENCE's pseudo labels (the fixture's teacher outputs)
        from probabilisticteacher_amd.structures import Boxes, FreeInstances
        strong = _gpu_records(z, "strong", 2)
        for i, r in enumerate(strong):
            h, w = r["image"].shape[-2:]
            inst = FreeInstances((h, w))
            inst.pseudo_boxes = Boxes(torch.from_numpy(z[f"t_roih{i}_pred_boxes"]))
            inst.scores_logists = torch.from_numpy(z[f"t_roih{i}_scores_logists"])
            inst.boxes_sigma = torch.from_numpy(z[f"t_roih{i}_boxes_sigma"])
            r["instances"] = inst
        flat.zero_grad()
        sampling.set_key_source(perm_key_source(opt.SeededPerm(79)))
        losses_u, _, _, _ = model(strong, branch="unsupervised", danchor=True)
        for k, v in losses_u.items():
            close(v.detach().cpu(), z["unsup_" + k], 1e-4, 1e-6, "unsup " + k)
        sum(losses_u.values()).backward()
        _grad_check(z, "unsupgrad", named)
    finally:
        sampling.set_key_source(None)


# ============================================================================ (3) PTrainer.run_step vs the reference's
def test_laplace_run_step_matches_reference_golden():
    """Three real reference PTrainer.run_step iterations under LAPLACE (burn-in, EMA copy + mutual, EMA + mutual) replayed on the
    HIP trainer: metrics and parameter probes, at the bars of the Gaussian replay."""
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.modeling import sampling
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    z = load("run_step_laplace")
    K, tau, B = int(z["K"]), tuple(float(v) for v in z["tau"]), int(z["B"])
    cfg = _cfg(K, "DifferentiableAnchorGenerator", tau, burn=1)
    ocfg = opt.Cfg(num_classes=K, anchor_generator="DifferentiableAnchorGenerator", tau=tau, burn_up_step=1)
    ratios = []

    class ReplayTrainer(PTrainer):
        """Records the teacher's pseudo labels and hands the student the REFERENCE's (from the fixture)."""
        override = None
        mine = None

        def process_pseudo_label(self, proposals, proposal_type, psedo_label_method=""):
            out, n = super().process_pseudo_label(proposals, proposal_type, psedo_label_method)
            self.mine = out
            return (self.override, n) if self.override is not None else (out, n)

    tr = ReplayTrainer(cfg, ratio_fn=lambda: ratios.pop(0))
    _load_params(tr.model, opt.golden_params(ocfg, int(z["seed"])))
    _load_params(tr.model_teacher, opt.golden_params(ocfg, int(z["teacher_seed"])))
    probes = sorted({k.split("_s_sum_")[1] for k in z.files if "_s_sum_" in k})
    try:
        for it in range(3):
            data = tuple(_gpu_records(z, f"it{it}_{nm}", B) for nm in ("lq", "lk", "uq", "uk"))
            ratios[:] = [float(v) for v in z[f"it{it}_ratios"]]
            tr.override = None
            if f"it{it}_pseudo0_pseudo_boxes" in z.files:
                ov = []
                for i in range(B):
                    h, w = data[3][i]["image"].shape[-2:]
                    inst = FreeInstances((h, w))
                    inst.pseudo_boxes = Boxes(torch.from_numpy(z[f"it{it}_pseudo{i}_pseudo_boxes"]).to(DEV))
                    inst.scores_logists = torch.from_numpy(z[f"it{it}_pseudo{i}_scores_logists"]).to(DEV)
                    inst.boxes_sigma = torch.from_numpy(z[f"it{it}_pseudo{i}_boxes_sigma"]).to(DEV)
                    ov.append(inst)
                tr.override = ov
            sampling.set_key_source(perm_key_source(opt.SeededPerm(500 + it)))
            m = tr.run_step(data)
            if tr.override is not None:
                for mine, ref in zip(tr.mine, tr.override):
                    assert len(mine) == len(ref)
                    ca = mine.scores_logists[:, :-1].argmax(1).cpu() * 0      # class-agnostic match on boxes
                    frac, idx = match_detections(mine.pseudo_boxes.tensor.cpu(), ca, ref.pseudo_boxes.tensor.cpu(),
                                                 ca, box_tol=5e-2)
                    assert frac >= 0.95, f"pseudo boxes matched {frac:.3f}"
            for k in z.files:
                if k.startswith(f"it{it}_m_"):
                    close(torch.tensor(m[k[len(f"it{it}_m_"):]]), z[k], 1e-4 if it == 0 else 1e-3, 1e-6, k)
            ssd, tsd = tr.model.state_dict(), tr.model_teacher.state_dict()
            sum_atol = 2e-4 if it == 0 else 1e-3
            for k in probes:
                close(ssd[k].double().sum().cpu(), z[f"it{it}_s_sum_{k}"], 1e-5, sum_atol, f"student sum {k}")
                close(ssd[k].flatten()[:16].cpu(), z[f"it{it}_s_head_{k}"], 1e-4, 1e-6, f"student head {k}")
                close(tsd[k].double().sum().cpu(), z[f"it{it}_t_sum_{k}"], 1e-5, sum_atol, f"teacher sum {k}")
                close(tsd[k].flatten()[:16].cpu(), z[f"it{it}_t_head_{k}"], 1e-4, 1e-6, f"teacher head {k}")
    finally:
        sampling.set_key_source(None)


# ============================================================================ (4) joint pass == separate passes
def _joint_inputs(K):
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    g = torch.Generator().manual_seed(8)
    sup, un = [], []
    for i in range(3):
        img = torch.randint(0, 256, (3, 112, 144), generator=g, dtype=torch.uint8)
        m = 1 + i
        xy = torch.rand(m, 2, generator=g) * torch.tensor([80.0, 60.0])
        a = FreeInstances((112, 144))
        a.gt_boxes = Boxes(torch.cat([xy, xy + 25 + torch.rand(m, 2, generator=g) * 30], 1))
        a.gt_classes = torch.randint(0, K, (m,), generator=g)
        sup.append({"image": img, "instances": a})
    for i in range(2):
        img = torch.randint(0, 256, (3, 112, 144), generator=g, dtype=torch.uint8)
        a = FreeInstances((112, 144))
        a.pseudo_boxes = Boxes(torch.tensor([[20.0, 30.0, 90.0, 100.0], [60.0, 10.0, 140.0, 90.0]])[: 2 - i])
        a.scores_logists = torch.randn(2 - i, K + 1, generator=g)
        a.boxes_sigma = torch.randn(2 - i, 4, generator=g)
        un.append({"image": img, "instances": a})
    return sup, un


def test_laplace_joint_student_pass_equals_separate_passes():
    """forward_joint under LAPLACE against the two separate `model(...)` calls on the same inputs and sampler keys: identical
    losses, matching gradients; and the Laplace losses are not the Gaussian model's."""
    from probabilisticteacher_amd import modeling
    from probabilisticteacher_amd.engine.flat import FlatParams
    from probabilisticteacher_amd.modeling import sampling
    K = 8
    ocfg = opt.Cfg(num_classes=K, anchor_generator="DifferentiableAnchorGenerator")
    params = opt.golden_params(ocfg, 13)
    sup, un = _joint_inputs(K)

    def run(model_type, joint):
        model = modeling.build_model(_cfg(K, "DifferentiableAnchorGenerator", (0.5, 0.5), model_type=model_type)).train()
        _load_params(model, params)
        flat = FlatParams(model)
        assert model.can_run_jointly(sup, un)
        sampling.set_key_source(keyed_perm_source(opt.KeyedPerm(5)))
        flat.zero_grad()
        try:
            if joint:
                ls, lu = model.forward_joint(sup, un, danchor=True)
            else:
                ls, _, _, _ = model(sup, branch="supervised")
                lu, _, _, _ = model(un, branch="unsupervised", danchor=True)
        finally:
            sampling.set_key_source(None)
        (sum(ls.values()) + sum(lu.values())).backward()
        return ({k: float(v) for k, v in ls.items()}, {k: float(v) for k, v in lu.items()}, flat.grad.clone())

    s1, u1, g1 = run("LAPLACE", False)
    s2, u2, g2 = run("LAPLACE", True)
    for a, b in ((s1, s2), (u1, u2)):
        assert a.keys() == b.keys()
        for k in a:
            close(b[k], a[k], 1e-6, 1e-7, "joint vs separate " + k)
    close(g2.cpu(), g1.cpu(), 1e-4, 1e-5 * float(g1.abs().max()), "joint vs separate gradients")
    sg, ug, _ = run("GUASSIAN", True)
    assert abs(sg["loss_rpn_loc"] - s2["loss_rpn_loc"]) > 1e-3 * abs(sg["loss_rpn_loc"])
    assert abs(sg["loss_box_reg"] - s2["loss_box_reg"]) > 1e-3 * abs(sg["loss_box_reg"])
    assert abs(ug["loss_rpn_loc"] - u2["loss_rpn_loc"]) > 1e-3 * abs(ug["loss_rpn_loc"])


# ============================================================================ (5) SOLVER.AMP.ENABLED routes too
def test_laplace_amp_unsupervised_branch_dispatches():
    """Routing check, not parity: the SOLVER.AMP.ENABLED student (bf16 operands, fp32 loss heads) on the unsupervised branch
    gives finite losses under LAPLACE, and its box-regression loss is not the Gaussian one on the same inputs."""
    from probabilisticteacher_amd import ops
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.modeling import sampling
    from probabilisticteacher_amd.structures import Boxes, FreeInstances
    z = load("model_laplace_diff_anchor")
    K, tau = int(z["K"]), tuple(float(v) for v in z["tau"])
    ocfg = opt.Cfg(num_classes=K, anchor_generator="DifferentiableAnchorGenerator", tau=tau)
    params = opt.golden_params(ocfg, int(z["seed"]))
    out = {}
    for model_type in ("LAPLACE", "GUASSIAN"):
        cfg = _cfg(K, "DifferentiableAnchorGenerator", tau, model_type=model_type)
        cfg.defrost() if hasattr(cfg, "defrost") else None
        cfg.SOLVER.AMP.ENABLED = True
        tr = PTrainer(cfg)
        assert tr.operand_rounding == "bf16"
        _load_params(tr.model, params)
        strong = _gpu_records(z, "strong", 2)
        for i, r in enumerate(strong):
            h, w = r["image"].shape[-2:]
            inst = FreeInstances((h, w))
            inst.pseudo_boxes = Boxes(torch.from_numpy(z[f"t_roih{i}_pred_boxes"]))
            inst.scores_logists = torch.from_numpy(z[f"t_roih{i}_scores_logists"])
            inst.boxes_sigma = torch.from_numpy(z[f"t_roih{i}_boxes_sigma"])
            r["instances"] = inst
        sampling.set_key_source(perm_key_source(opt.SeededPerm(79)))
        try:
            with ops.operand_rounding(tr.operand_rounding):
                losses, _, _, _ = tr.model(strong, branch="unsupervised", danchor=True)
                sum(losses.values()).backward()
        finally:
            sampling.set_key_source(None)
        out[model_type] = {k: float(v) for k, v in losses.items()}
        del tr
    lap, gau = out["LAPLACE"], out["GUASSIAN"]
    assert set(lap) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}, set(lap)
    assert all(math.isfinite(v) for v in lap.values()), lap
    assert abs(lap["loss_box_reg"] - gau["loss_box_reg"]) > 0.1 * abs(gau["loss_box_reg"]), (lap, gau)
    assert abs(lap["loss_rpn_loc"] - gau["loss_rpn_loc"]) > 1e-3 * abs(gau["loss_rpn_loc"]), (lap, gau)
