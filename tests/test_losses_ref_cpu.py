"""CPU: tests/losses_ref.py is a sound reference for tests/test_losses_gpu.py.

(1) its float32 restatements agree, on the plain regimes, with what the suite already trusts: oracle.pt.gaussian_dist_pdf and
    rpn_losses_unsup (as tests/test_ops_gpu.py::test_unsup_losses uses them), F.binary_cross_entropy_with_logits, F.cross_entropy,
    F.softmax / F.log_softmax;
(2) every regime's float32 reference is finite;
(3) every regime keeps the float32 yardstick within 1e-2 of float64 for every checked quantity (a condition on the inputs);
(4) the float64 references of the saturated-weight rows are finite."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pt as opt
from tests import losses_ref as lr
from tests.helpers import close

F32, F64 = torch.float32, torch.float64
REGIMES = lr.regimes()
VARIANTS = [(f"{r.name}-{tag}" if tag else r.name, v) for r in REGIMES for tag, v in lr.variants(r)]


def _rclose(got, ref, what):
    close(got.detach(), ref.detach(), 1e-6, 1e-30, what)


# ============================================================================ (1) the restatements are the trusted expressions
def test_bce_restatement_is_binary_cross_entropy_with_logits():
    """... and that is the expression csrc/losses.hip::bce_kernel writes out; rows with label -1 count for nothing"""
    r = lr.bce_plain()
    x, lab = r.inputs["x"].clone().requires_grad_(), r.inputs["lab"]
    got = lr.bce_logits_sum(x, lab, lr.INV_NORM)
    valid = lab >= 0
    v, t = r.inputs["x"][valid], lab[valid].float()
    _rclose(got, F.binary_cross_entropy_with_logits(v, t, reduction="sum") * lr.INV_NORM, "bce")
    mx = torch.clamp(-v, min=0)
    _rclose(got, ((1 - t) * v + mx + torch.log(torch.exp(-mx) + torch.exp(-v - mx))).sum() * lr.INV_NORM, "bce, written out")
    got.backward()
    assert not x.grad[~valid].any()
    close(x.grad[valid], (torch.sigmoid(v) - t) * lr.INV_NORM, 1e-6, 1e-30, "bce grad")


def test_gaussian_nll_restatement_is_the_oracle_pdf():
    r = lr.gnll_plain()
    d, t = r.inputs["d"], r.inputs["t"]
    var = torch.sigmoid(d[:, 4:])
    _rclose(lr.gaussian_dist_pdf(d[:, :4], t, var), opt.gaussian_dist_pdf(d[:, :4], t, var), "gaussian pdf")
    ref = -torch.log(opt.gaussian_dist_pdf(d[:, :4], t, var) + 1e-9).sum() * lr.INV_NORM
    _rclose(lr.gaussian_nll_sum(d, t, lr.INV_NORM), ref, "gaussian nll")


@pytest.mark.parametrize("C", lr.CLASSES)
def test_softmax_restatements_are_torch_functional(C):
    r = lr.softmax_plain(C)
    x, tgt = r.inputs["x"], r.inputs["tgt"]
    a, b = x.clone().requires_grad_(), x.clone().requires_grad_()
    got, ref = lr.softmax_ce_mean(a, tgt), F.cross_entropy(b, tgt)
    _rclose(got, ref, "ce")
    got.backward(), ref.backward()
    close(a.grad, b.grad, 1e-6, 1e-9, "ce grad")
    _rclose(lr.softmax_rows(x), F.softmax(x, -1), "softmax")
    # ... and both are what csrc/losses.hip writes out: the row maximum subtracted, then exp, sum, log
    z = x - x.max(-1, keepdim=True)[0]
    e = torch.exp(z)
    _rclose(lr.softmax_rows(x), e / e.sum(-1, keepdim=True), "softmax, written out")
    _rclose(got, -(z - torch.log(e.sum(-1, keepdim=True))).gather(1, tgt.view(-1, 1)).mean(), "ce, written out")
    assert float(lr.softmax_ce_mean(torch.zeros(0, C), torch.zeros(0, dtype=torch.int64))) == 0.0


def test_soft_ce_restatement_is_the_expression_of_test_unsup_losses():
    r = lr.soft_ce_plain()
    T, S = r.inputs["T"], r.inputs["S"]
    C = T.shape[1]
    p = F.softmax(T, -1)
    ent = -(p * torch.log(p)).sum(-1)
    q = F.softmax(T / lr.TAU, -1) * ((1 - ent / math.log(C)) ** lr.LAM).unsqueeze(-1)
    _rclose(lr.soft_ce_efl(T, S, lr.TAU, lr.LAM, True, lr.INV_NORM), torch.sum(q * -F.log_softmax(S, -1)) * lr.INV_NORM, "soft ce")
    ref = torch.sum(F.softmax(T / lr.TAU, -1) * -F.log_softmax(S, -1)) * lr.INV_NORM
    _rclose(lr.soft_ce_efl(T, S, lr.TAU, lr.LAM, False, lr.INV_NORM), ref, "soft ce, efl off")


def _rand_boxes(gen, n, h, w, lo):
    xy = torch.rand(n, 2, generator=gen) * torch.tensor([w * 0.7, h * 0.7])
    wh = lo + torch.rand(n, 2, generator=gen) * torch.tensor([w * 0.3 - lo, h * 0.3 - lo])
    return torch.cat([xy, xy + wh], 1)


def test_rpn_restatements_are_the_oracle_rpn_losses_unsup():
    """one synthetic image whose selected anchors are the plain RPN and KL regimes' rows (tau and lambda of both heads 0.5)"""
    rp, kp = lr.rpn_plain(), lr.kl_plain()
    K = rp.inputs["T"].shape[1] - 1
    cfg = opt.Cfg(tau=(lr.TAU, lr.TAU), efl_lambda=(lr.LAM, lr.LAM))
    gen = torch.Generator().manual_seed(5)
    A = 200
    mask = torch.zeros(A, dtype=torch.bool)
    mask[torch.randperm(A, generator=gen)[:lr.ROWS]] = True
    anchors, matched = _rand_boxes(gen, A, 300, 400, 16.0), _rand_boxes(gen, A, 300, 400, 16.0)
    obj = torch.randn(1, A, generator=gen)
    obj[0, mask] = rp.inputs["x"]
    deltas = torch.randn(1, A, 8, generator=gen)
    deltas[0, mask] = kp.inputs["q"]
    ref = opt.rpn_losses_unsup(cfg, anchors, obj, deltas, [rp.inputs["T"]], [mask], [matched], [kp.inputs["slog_p"]], True)
    inv = 1.0 / cfg.rpn_batch_size_per_image
    got_cls, fg = lr.rpn_soft_obj_loss(rp.inputs["T"], rp.inputs["x"], lr.TAU, lr.LAM, True, inv)
    _rclose(got_cls, ref["loss_rpn_cls"], "rpn soft obj")
    assert torch.equal(fg.bool(), rp.inputs["T"].max(-1)[1] != K)          # no ties in the plain regime
    mu_p = opt.get_deltas(anchors, matched, cfg.rpn_bbox_reg_weights)[mask]
    got_loc = lr.kl_efl_loss(kp.inputs["q"], mu_p, kp.inputs["slog_p"], fg, lr.TAU, lr.LAM, True, 0, inv)
    _rclose(got_loc, ref["loss_rpn_loc"], "rpn kl")


def test_fg_is_the_lowest_index_among_equal_maxima():
    r = lr.rpn_ties()
    fg = lr.rpn_fg(r.inputs["T"])
    assert fg.all()                                   # a foreground class ties with, or beats, the last class on every row
    assert not lr.rpn_fg(torch.tensor([[0.0, 1.0, 1.0 + 1e-6]])).any()
    assert lr.rpn_fg(torch.tensor([[3.0, 3.0]])).all()


def test_teacher_rows_have_the_spread_exactly():
    for C in lr.CLASSES:
        for s in lr.SPREADS + lr.DENORMAL_SPREADS:
            T = lr.teacher_rows(lr.ROWS, C, s, torch.Generator().manual_seed(1))
            assert torch.equal(T.max(-1)[0] - T.min(-1)[0], torch.full((lr.ROWS,), s)) and float(T.min()) == 0.0


# ============================================================================ (2), (3) conditions on the regimes
def test_regime_names_are_unique():
    names = [n for n, _ in VARIANTS]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("name,reg", VARIANTS, ids=[n for n, _ in VARIANTS])
def test_regime_fp32_reference_is_finite_and_a_fair_yardstick(name, reg):
    r32, r64 = lr.reference(reg, F32), lr.reference(reg, F64)
    fl = lr.floors(reg)
    for k in lr.OUTPUTS[reg.op]:
        assert bool(torch.isfinite(r32[k]).all()), f"{name}: fp32 {k} not finite"
        assert bool(torch.isfinite(r64[k]).all()), f"{name}: fp64 {k} not finite"
        e32 = lr.err(r32[k], r64[k], fl[k])
        assert e32 <= lr.YARDSTICK_CAP, f"{name}: fp32 {k} is off by {e32:.3e}: move the regime"


def test_check_accepts_the_yardstick_and_rejects_a_wrong_sign():
    reg = lr.kl_teacher_sigma()
    r32, r64 = lr.reference(reg, F32), lr.reference(reg, F64)
    fl = lr.floors(reg)
    for k in lr.OUTPUTS[reg.op]:
        lr.check(r32[k], r64[k], r32[k], lr.rtol_of(k), fl[k], k)
        with pytest.raises(AssertionError):
            lr.check(-r32[k], r64[k], r32[k], lr.rtol_of(k), fl[k], k)
        with pytest.raises(AssertionError):
            lr.check(r32[k] * 1.05, r64[k], r32[k], lr.rtol_of(k), fl[k], k)


def test_beyond_the_denormal_band_the_fp32_reference_is_nan():
    for reg in lr.beyond_denormal():
        assert math.isnan(float(lr.reference(reg, F32)["loss"])), reg.name
        assert math.isfinite(float(lr.reference(reg.with_kw(efl=False), F32)["loss"])), reg.name


# ============================================================================ (4) saturated-weight rows
@pytest.mark.parametrize("op", ["kl_efl", "laplace_kl_efl"])
def test_saturated_sigma_float64_reference_is_finite(op):
    weight = lr.kl_weight if op == "kl_efl" else lr.laplace_kl_weight
    for values in [lr.SATURATED_SLOG_P] + [[v] for v in lr.BAND_SLOG_P]:
        reg = lr.saturated_sigma(op, values)
        w = weight(reg.inputs["slog_p"].double(), lr.LAM)
        assert bool(torch.isfinite(w).all()) and float(w.max()) < 2e-3, (values, float(w.max()))
        for tag, v in lr.variants(reg):
            r64 = lr.reference(v, F64)
            assert all(bool(torch.isfinite(r64[k]).all()) for k in lr.OUTPUTS[op]), (values, tag)
        # what the issue measured: fp32 torch gives a base of exactly 0 at and above 17
        if values is lr.SATURATED_SLOG_P:
            assert not weight(reg.inputs["slog_p"], lr.LAM).any()


@pytest.mark.parametrize("op", ["soft_ce_efl", "rpn_soft_obj"])
@pytest.mark.parametrize("C", [2, 9])
def test_near_uniform_teacher_float64_weight_is_tiny(op, C):
    reg = lr.uniform_teacher(op, C, 1e-4)
    w = lr.efl_weight(reg.inputs["T"].double(), lr.LAM)
    assert bool(torch.isfinite(w).all()) and float(w.max()) < 1e-4
    r64 = lr.reference(reg, F64)
    assert all(bool(torch.isfinite(r64[k]).all()) for k in lr.OUTPUTS[op])
    T0 = lr.uniform_teacher(op, C, 0.0).inputs["T"]
    assert torch.equal(T0.max(-1)[0], T0.min(-1)[0])
