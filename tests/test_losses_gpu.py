"""GPU (pytest -m gpu): the Gaussian-model loss kernels of csrc/losses.hip (bce, gnll, softmax_ce, softmax_rows, soft_ce_efl,
rpn_soft_obj, kl_efl; finalize and scale_rows behind them) against float64 autograd, with the float32 CPU restatement as yardstick.

Reference, regimes and the comparison are tests/losses_ref.py (see its docstring): a kernel output passes if
err(got) <= max(base_rtol, 4 * err(ref32)), err(x) = max |x - ref64| / (|ref64| + floor), base_rtol 1e-5 for a loss (and for
softmax_rows' probabilities), 1e-4 for a gradient; the gradient floor is 1e-5 of the median nonzero float64 gradient of the op's
plain regime.  The upstream gradient is 2.0 everywhere.

(1) parity by regime: saturation, teacher spread (0.1 .. 80 and the denormal band 90 .. 100), logit scale, ties, C in {2, 9, 21, 81};
(2) sizes: n = 1, 255 .. 257 and the 1024-block cap +- 1 and twice over it; R = 0;
(3) the shared workspace across ops on one stream;
(4) entropy weights whose exact base is 0 or nearly: saturated teacher sigma (Gaussian and Laplace KL), uniform teacher rows;
(5) teacher spread 120: the documented NaN.

Measured on an MI355X (first device run of these tests), per regime family over all its variants and C: `ratio` is the largest
err(got) / err(ref32) among the checks where 4 * err(ref32) exceeds base_rtol (elsewhere base_rtol governs: "-"), `of tol` the largest
err(got) / tolerance.

    regime family                                  checks | loss (y): ratio  of tol | gradients: ratio  of tol
    bce_plain, bce_saturated                            4 |              -    0.01  |             1.00    0.25
    gnll_plain, gnll_delta                              6 |              -    0.01  |                -    0.04
    gnll_sigma, gnll_crossed                            6 |              -    0.00  |             1.00    0.25
    kl_efl_plain, kl_one_fg                            30 |              -    0.01  |                -    0.19
    kl_teacher_sigma, kl_student_sigma                 36 |              -    0.01  |             1.00    0.25
    kl_crossed                                         18 |           1.44    0.36  |             1.00    0.25
    soft_ce / rpn plain, rpn_ties (C = 9)              12 |              -    0.01  |                -    0.12
    softmax_ce, scale 1 / 80 / 1e4, C in 2 .. 81       24 |              -    0.01  |                -    0.12
    softmax_rows, scale 1 / 80 / 1e4, C in 2 .. 81     12 |              -    0.05  |
    soft_ce, teacher spread 0.1, C in 2 .. 81          16 |           2.88    0.72  |             3.99    1.00
    rpn,     teacher spread 0.1, C in 2 .. 81          16 |           3.28    0.82  |             2.74    0.69
    soft_ce, teacher spread 1,   C in 2 .. 81          16 |              -    0.34  |             5.70    (margin 8, below)
    rpn,     teacher spread 1,   C in 2 .. 81          16 |              -    0.20  |                -    0.21
    soft_ce, teacher spread 5,   C in 2 .. 81          16 |              -    0.02  |             2.03    0.51
    soft_ce, teacher spread 20 / 60 / 80               48 |              -    0.01  |             1.00    0.25
    rpn,     teacher spread 5 / 20 / 60 / 80           64 |              -    0.02  |                -    0.03
    soft_ce_scale 1 / 80 / 1e4                         12 |              -    0.01  |                -    0.13
    rpn_x 1 / 20 / 50 / 100                            16 |              -    0.01  |             1.00    0.25
    soft_ce / rpn, spread 90 / 95 / 100, C = 2, 9      48 |              -    0.01  |                -    0.03
    spread 120 with efl off                             8 |              -    0.00  |                -    0.03
    sizes: bce n, workspace reuse                      29 |              -    0.01  |             1.00    0.25
    sizes: gnll / kl rows, kl mean                     54 |              -    0.01  |                -    0.19
    sizes: row kernels, R = 1 .. 262 444               35 |              -    0.05  |                -    0.12

Where a ratio is 1.00 the kernel and the fp32 reference round the same cancellation the same way (sigmoid(x) - 1 at |x| >= 9,
var (1 - var) at |sigma logit| >= 10, the entropy weight at slog_p = 12): that is the case the yardstick is for.

The one entry above 4: soft_ce_C81_spread1, dS, 5.70 with efl on and 5.28 with it off.  dS_j = w (p_j - q_j); at row 56, class 77,
p = 1.56597e-2 and q = 1.56641e-2 agree to 2.8e-4, so every ulp of p or q is 4.3e-4 of the difference.  The kernel's
p_j = expf(s_j - ms - ls) inherits the rounding of ls = logf(ss) (1 ulp of 2.4: 2 ulp of p) and of the subtraction (0.5 ulp of
|-4.16|: 2 ulp of p) before expf's own 1-2 ulp; ATen's log_softmax backward evaluates the same form with the same worst case.
On this element (the device's worst with efl on and off) the kernel is off by 3.4 ulp of p in all, the host by 0.6: an accident of rounding on either side, not an
operation the kernel does worse.  MARGINS gives this one output a margin of 8 (< 2 x 5.28): a tolerance of 2.2e-3.

Neither suspected hazard shows on the device.  With teacher sigma logits of 17, 20, 40 and 100 both KL kernels return a weight of
exactly 0 (loss with efl on / loss with efl off), as the fp32 reference does; from 12.5 to 16.5 it is 0 .. 1.2e-3, never NaN.  In
the denormal band (spread 90 .. 100) expf keeps the denormal: the loss is finite and at parity (C = 2: on / off = 1 exactly).
csrc/losses.hip is unchanged.  efl_weight's clamp IS needed: without it the rows of spread 1e-4, C = 9 are NaN.
"""
import math

import pytest
import torch

from tests import losses_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from probabilisticteacher_amd import ops as _ops
    return _ops


def run_gpu(ops, reg, optional=True):
    """the op on the device -> {"loss", gradients of UP * loss, "fg"} as CPU tensors; `optional`: request dt / dmu_p too"""
    i, kw = reg.inputs, dict(reg.kw)
    use_fg = kw.pop("use_fg", True)
    dev = {k: v.clone().to(DEV) for k, v in i.items()}
    out = {}
    if reg.op == "bce":
        leaves = {"dx": dev["x"].requires_grad_()}
        loss = ops.bce_logits_sum(leaves["dx"], dev["lab"], kw["inv_norm"])
    elif reg.op == "gnll":
        leaves = {"dd": dev["d"].requires_grad_()}
        if optional:
            leaves["dt"] = dev["t"].requires_grad_()
        loss = ops.gaussian_nll_sum(dev["d"], dev["t"], kw["inv_norm"])
    elif reg.op == "softmax_ce":
        leaves = {"dx": dev["x"].requires_grad_()}
        loss = ops.softmax_ce_mean(dev["x"], dev["tgt"])
    elif reg.op == "softmax_rows":
        return {"y": ops.softmax_rows(dev["x"]).cpu()}
    elif reg.op == "soft_ce_efl":
        leaves = {"dS": dev["S"].requires_grad_()}
        loss = ops.soft_ce_efl(dev["T"], dev["S"], kw["tau"], kw["lam"], kw["efl"], kw["inv_norm"])
    elif reg.op == "rpn_soft_obj":
        leaves = {"dx": dev["x"].requires_grad_()}
        loss, fg = ops.rpn_soft_obj_loss(dev["T"], dev["x"], kw["tau"], kw["lam"], kw["efl"], kw["inv_norm"])
        out["fg"] = fg.cpu()
    else:
        leaves = {"dq": dev["q"].requires_grad_()}
        if optional:
            leaves["dmu_p"] = dev["mu_p"].requires_grad_()
        fn = ops.kl_efl_loss if reg.op == "kl_efl" else ops.laplace_kl_efl_loss
        loss = fn(dev["q"], dev["mu_p"], dev["slog_p"], dev["fg"] if use_fg else None, kw["tau"], kw["lam"], kw["efl"],
                  kw["reduction"], kw["inv_norm"])
    (loss * lr.UP).backward()
    out["loss"] = loss.detach().cpu()
    for k, v in leaves.items():
        out[k] = v.grad.cpu()
    return out


def same_bits(a, b):
    return torch.equal(a, b) or bool((torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num()))


# (regime, output) -> its own margin over err(ref32), where the measured ratio is above 4; explained next to the table above
MARGINS = {("soft_ce_C81_spread1", "dS"): 8.0}


def compare(reg, got, name, floors=None):
    r64, r32 = lr.reference(reg, F64), lr.reference(reg, F32)
    fl = floors(r64) if floors else lr.floors(reg)
    for k in lr.OUTPUTS[reg.op]:
        if k in got:
            lr.check(got[k], r64[k], r32[k], lr.rtol_of(k), fl[k], f"{name} {k}", MARGINS.get((reg.name, k), lr.MARGIN))
    return r64


def run_and_compare(ops, reg, name, floors=None):
    """both forms of the call where a gradient is optional: the loss and the other gradient must not depend on the request"""
    got = run_gpu(ops, reg)
    r64 = compare(reg, got, name, floors)
    if reg.op in ("gnll", "kl_efl", "laplace_kl_efl"):
        less = run_gpu(ops, reg, optional=False)
        for k, v in less.items():
            assert same_bits(v, got[k]), f"{name}: {k} changes when the optional gradient is not requested"
    return got, r64


# ============================================================================ (1) parity by regime
VARIANTS = [(f"{r.name}-{tag}" if tag else r.name, v) for r in lr.regimes() for tag, v in lr.variants(r)]


@pytest.mark.parametrize("name,reg", VARIANTS, ids=[n for n, _ in VARIANTS])
def test_parity_by_regime(ops, name, reg):
    got, r64 = run_and_compare(ops, reg, name)
    i = reg.inputs
    if reg.op == "rpn_soft_obj":
        assert torch.equal(got["fg"], r64["fg"]), f"{name}: fg is not the lowest-index argmax"
    if reg.op == "softmax_rows":
        s = got["y"].double().sum(-1)
        assert float((s - 1).abs().max()) <= 4 * 2.0 ** -23, f"{name}: rows sum to 1 +- {float((s - 1).abs().max()):.3e}"
    if reg.op == "kl_efl" and reg.kw.get("use_fg", True):
        assert not got["dq"][i["fg"] == 0].any() and not got["dmu_p"][i["fg"] == 0].any(), f"{name}: unselected rows"
    if "zero_rows" in reg.meta:                                    # Delta = 0 exactly: no gradient on the means
        z = reg.meta["zero_rows"]
        g = got["dq"] if reg.op == "kl_efl" else got["dd"]
        assert not g[z, :4].any(), f"{name}: Delta = 0 rows"


# ============================================================================ (2) sizes
CAP = 1024 * 256                                                   # blocks_for caps the grid: elements (or rows) per pass
ELEMS = [1, 255, 256, 257, CAP - 1, CAP, CAP + 1, 2 * CAP + 77]
ROWS4 = [1, 63, 64, 65, 65535, 65536, 65537, 131091]               # rows x 4 straddles the same edges
ROWS = [1, 255, 256, 257, CAP + 300]


@pytest.mark.parametrize("n", ELEMS)
def test_bce_sizes(ops, n):
    run_and_compare(ops, lr.cycled(lr.bce_plain(), n), f"bce n={n}", lr.own_floors)


@pytest.mark.parametrize("rows", ROWS4)
def test_gnll_sizes(ops, rows):
    run_and_compare(ops, lr.cycled(lr.gnll_plain(), rows), f"gnll rows={rows}", lr.own_floors)


@pytest.mark.parametrize("rows", ROWS4)
def test_kl_sizes(ops, rows):
    reg = lr.cycled(lr.kl_plain(), rows)
    got, _ = run_and_compare(ops, reg, f"kl rows={rows}", lr.own_floors)
    assert not got["dq"][reg.inputs["fg"] == 0].any()


@pytest.mark.parametrize("use_fg", [True, False])
def test_kl_mean_over_the_block_cap(ops, use_fg):
    """131 091 rows in mean mode: sum and count partials over all 1024 slots, scale_rows_kernel's grid-stride on dq (rows x 8) and
    on dmu_p; fg selects about 70 %"""
    reg = lr.cycled(lr.kl_plain(), 131091).with_kw(reduction=1, use_fg=use_fg)
    got, _ = run_and_compare(ops, reg, f"kl mean fg={use_fg}", lr.own_floors)
    if use_fg:
        sel = reg.inputs["fg"].bool()
        assert 0.6 < float(sel.float().mean()) < 0.8
        assert not got["dq"][~sel].any() and not got["dmu_p"][~sel].any()


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("op", ["softmax_ce", "softmax_rows", "soft_ce_efl", "rpn_soft_obj"])
def test_row_kernel_sizes(ops, op, R):
    reg = lr.cycled(lr.plain_of(op, 9), R)
    got, r64 = run_and_compare(ops, reg, f"{op} R={R}", lr.own_floors)
    if op == "rpn_soft_obj":
        assert torch.equal(got["fg"], r64["fg"])


def test_no_rows(ops):
    """R = 0: sums and the CE mean give 0, the KL mean NaN (torch's mean of nothing)"""
    z = lambda *s, dtype=F32: torch.zeros(s, dtype=dtype, device=DEV)          # noqa: E731
    assert float(ops.bce_logits_sum(z(0), z(0, dtype=torch.int8), 1.0)) == 0.0
    assert float(ops.gaussian_nll_sum(z(0, 8), z(0, 4), 1.0)) == 0.0
    assert float(ops.softmax_ce_mean(z(0, 9), z(0, dtype=torch.int64))) == 0.0
    assert ops.softmax_rows(z(0, 9)).shape == (0, 9)
    assert float(ops.soft_ce_efl(z(0, 9), z(0, 9), 0.5, 0.5, True, 1.0)) == 0.0
    loss, fg = ops.rpn_soft_obj_loss(z(0, 9), z(0), 0.5, 0.5, True, 1.0)
    assert float(loss) == 0.0 and fg.shape == (0,)
    assert float(ops.kl_efl_loss(z(0, 8), z(0, 4), z(0, 4), z(0, dtype=torch.uint8), 0.5, 0.5, True, 0, 1.0)) == 0.0
    assert math.isnan(float(ops.kl_efl_loss(z(0, 8), z(0, 4), z(0, 4), None, 0.5, 0.5, True, 1, 1.0)))
    # ... and a mean over rows none of which is selected
    reg = lr.kl_plain()
    none = ops.kl_efl_loss(reg.inputs["q"].to(DEV), reg.inputs["mu_p"].to(DEV), reg.inputs["slog_p"].to(DEV),
                           z(lr.ROWS, dtype=torch.uint8), 0.5, 0.5, True, 1, 1.0)
    assert math.isnan(float(none))


# ============================================================================ (3) one workspace for every op
def test_workspace_reuse_across_ops(ops):
    """a 1024-block sum, a 1-block loss of another op, a mean-mode KL (which also fills the count slots and the scale slot), then the
    1-block loss again, all on one stream: each still right, the two 1-block results the same bits"""
    big = lr.cycled(lr.bce_plain(), 2 * CAP + 77)
    small = lr.gnll_plain()
    mean = lr.cycled(lr.kl_plain(), 70000).with_kw(reduction=1)
    a = run_gpu(ops, big)
    b = run_gpu(ops, small)
    c = run_gpu(ops, mean)
    d = run_gpu(ops, small)
    compare(big, a, "ws: bce over the cap", lr.own_floors)
    compare(small, b, "ws: gnll, one block")
    compare(mean, c, "ws: kl mean", lr.own_floors)
    compare(small, d, "ws: gnll again")
    for k in b:
        assert torch.equal(b[k], d[k]), k


# ============================================================================ (4) entropy weights whose exact base is (nearly) 0
def _bounded_by(on, off, factor, name):
    """the efl-on call against the same call with efl off: everything finite, |loss| and max |gradient| within `factor` of it.
    Every term of these losses is >= 0 and the weight multiplies term and gradient alike, so `factor` bounds the largest weight."""
    for k, v in on.items():
        if k == "fg":
            continue
        assert bool(torch.isfinite(v).all()), f"{name}: {k} not finite with efl on"
        assert bool(torch.isfinite(off[k]).all()) and float(off[k].abs().max()) > 0, f"{name}: {k} with efl off"
        a, b = float(v.abs().max()), float(off[k].abs().max())
        assert a <= factor * b, f"{name}: {k} {a:.3e} > {factor:.3e} * {b:.3e}"


KL_MODES = [(0, True), (1, False), (1, True)]


@pytest.mark.parametrize("reduction,use_fg", KL_MODES)
@pytest.mark.parametrize("op", ["kl_efl", "laplace_kl_efl"])
def test_saturated_teacher_sigma_weight_is_zero_not_nan(ops, op, reduction, use_fg):
    """teacher sigma logits 17, 20, 40, 100: fp32 sigmoid is 1 exactly, the exact base of the entropy weight is >= 0 and below 2e-8,
    the fp32 reference gives 0.  A correct fp32 evaluation may be off by a few eps = 6e-8, so the weight is at most
    sqrt(8 eps) ~ 7e-4 < 1e-3; a base that rounds below 0 must not become NaN."""
    reg = lr.saturated_sigma(op).with_kw(reduction=reduction, use_fg=use_fg)
    _bounded_by(run_gpu(ops, reg), run_gpu(ops, reg.with_kw(efl=False)), 1e-3, reg.name)


@pytest.mark.parametrize("slog_p", lr.BAND_SLOG_P)
@pytest.mark.parametrize("op", ["kl_efl", "laplace_kl_efl"])
def test_nearly_saturated_teacher_sigma_weight_is_finite_and_small(ops, op, slog_p):
    """12 < slog_p < 17: the base is rounding noise on both sides; finite, and within the float64 weight + 1e-3"""
    weight = lr.kl_weight if op == "kl_efl" else lr.laplace_kl_weight
    w64 = float(weight(torch.tensor(slog_p, dtype=F64), lr.LAM))
    assert 0 < w64 < 2e-3
    for reduction, use_fg in KL_MODES:
        reg = lr.saturated_sigma(op, [slog_p]).with_kw(reduction=reduction, use_fg=use_fg)
        _bounded_by(run_gpu(ops, reg), run_gpu(ops, reg.with_kw(efl=False)), w64 + 1e-3, reg.name)


@pytest.mark.parametrize("spread", [0.0, 1e-4])
@pytest.mark.parametrize("C", [2, 9])
@pytest.mark.parametrize("op", ["soft_ce_efl", "rpn_soft_obj"])
def test_uniform_teacher_rows_weight_is_zero_not_nan(ops, op, C, spread):
    """exactly uniform teacher rows and rows of spread 1e-4: the exact weight is below 1e-4, fp32 noise on the base a few eps"""
    reg = lr.uniform_teacher(op, C, spread)
    _bounded_by(run_gpu(ops, reg), run_gpu(ops, reg.with_kw(efl=False)), 1e-3, reg.name)


# ============================================================================ (5) beyond the denormal band
@pytest.mark.parametrize("reg", lr.beyond_denormal(), ids=lambda r: r.name)
def test_teacher_spread_120_keeps_the_documented_nan(ops, reg):
    """expf underflows to 0 and 0 * log 0 is NaN: efl_weight documents that it keeps it, as the fp32 reference does; efl off is finite"""
    assert math.isnan(float(lr.reference(reg, F32)["loss"]))
    assert math.isnan(float(run_gpu(ops, reg)["loss"]))
    off = reg.with_kw(efl=False)
    compare(off, run_gpu(ops, off), reg.name + " efl off")
