"""dtype-generic torch restatements of the loss terms csrc/losses.hip fuses with their gradients, the named input regimes they are
tested at and the comparison both tests/test_losses_ref_cpu.py and tests/test_losses_gpu.py use.

Restatements: every function below runs unchanged in float32 and in float64 and is differentiated by autograd.  They are written as
the kernel header cites the reference (box_regression.py:33-35, rpn.py:242-246,285-304,321-355, fast_rcnn.py:179-263), `+ 1e-9` terms,
`sigmoid(1 - x)` and `var + 0.3` included.  Where the reference calls torch.nn.functional (binary_cross_entropy_with_logits,
cross_entropy, softmax, log_softmax) so do they: the backward of those calls is the fp32 arithmetic the kernels mirror, and its error is
the yardstick below.  `fg` and every argmax are the LOWEST index among equal maxima (numpy.argmax).

Regimes: 64 seeded CPU rows that vary one cause of trouble (saturation, teacher spread, logit scale, ties) and draw the rest from
randn scaled as tests/test_laplace_gpu.py::_kl_inputs does.  Teacher rows have an exactly controlled max - min spread: one entry 0,
one entry `spread`, the others uniform between.

Comparison: `check(got, ref64, ref32, base_rtol, floor)`.  err(x) = max |x - ref64| / (|ref64| + floor); the kernel passes if
err(got) <= max(base_rtol, 4 * err(ref32)).  The float32 CPU restatement is the yardstick: near saturation the fp32 expressions lose
digits to cancellation themselves, and err(ref32) says how many.  The factor 4 covers the device's expf / logf / powf (1-2 ulp where
the host's are <= 1 ulp) and a different operation order.  A regime may use the yardstick only while err(ref32) <= 1e-2 (YARDSTICK_CAP):
the tolerance then never exceeds 4e-2, and a wrong weight, a missing term or a wrong sign is off by far more."""
import math
import os
from dataclasses import dataclass, field, replace

import numpy as np
import torch
import torch.nn.functional as F

LOSS_RTOL, GRAD_RTOL, GRAD_FLOOR = 1e-5, 1e-4, 1e-5        # the project's own, tests/test_laplace_gpu.py
LOSS_FLOOR = 1e-12
MARGIN = 4.0
YARDSTICK_CAP = 1e-2
UP = 2.0                                                    # upstream gradient of every comparison
ROWS = 64
TAU, LAM, INV_NORM = 0.5, 0.5, 1.0 / 512.0


# ================================================================================================ restatements
def bce_logits_sum(x, lab, inv_norm):
    """rpn.py:242-246: the reference's own call (its backward is sigmoid(x) - t, not the derivative of the log-sum-exp form, which
    cancels badly in fp32)"""
    valid = lab >= 0
    return F.binary_cross_entropy_with_logits(x[valid], lab[valid].to(x.dtype), reduction="sum") * inv_norm


def gaussian_dist_pdf(val, mean, var):
    """box_regression.py:33-35"""
    return torch.exp(-(val - mean) ** 2.0 / (var + 1e-9) / 2.0) / torch.sqrt(2.0 * np.pi * (var + 0.3))


def gaussian_nll_sum(d, t, inv_norm):
    """box_regression.py:165-176, fast_rcnn.py:286-296: d = (mu | sigma logits), (rows, 8)"""
    return -torch.log(gaussian_dist_pdf(d[:, :4], t, torch.sigmoid(d[:, 4:])) + 1e-9).sum() * inv_norm


def softmax_rows(x):
    return F.softmax(x, -1)


def softmax_ce_mean(x, tgt):
    """the reference's own call, cross_entropy(x, tgt, reduction="mean"); no rows -> 0 (D2's cross_entropy wrapper).  Its backward,
    softmax - onehot from exp(log_softmax), is the form the kernel evaluates; a restatement that subtracts the row maximum inside
    the autograd graph is NOT a yardstick: the gradient it routes through the max cancels the target's term exactly."""
    if x.shape[0] == 0:
        return x.sum() * 0.0
    return F.cross_entropy(x, tgt)


def efl_weight(T, lam):
    """fast_rcnn.py:199-200, rpn.py:288-290: (1 - H(softmax T) / log C) ** lambda, one weight per row"""
    p = F.softmax(T, -1)
    ent = -(p * torch.log(p)).sum(-1)
    return (1 - ent / math.log(T.shape[-1])) ** lam


def soft_ce_efl(T, S, tau, lam, efl, inv_norm):
    """fast_rcnn.py:179-213"""
    q = F.softmax(T / tau, -1)
    if efl:
        q = q * efl_weight(T, lam).unsqueeze(-1)
    return torch.sum(q * -F.log_softmax(S, -1)) * inv_norm


def rpn_fg(T):
    """rpn.py:292: the teacher's argmax is not the last (background) class; lowest index among equal maxima"""
    a = np.argmax(T.detach().cpu().numpy(), axis=-1)
    return torch.from_numpy((a != T.shape[-1] - 1).astype(np.uint8))


def rpn_soft_obj_loss(T, x, tau, lam, efl, inv_norm):
    """rpn.py:285-304, the sigmoid(1 - x) of :299 kept -> (loss, fg)"""
    q = F.softmax(T / tau, -1)
    q2 = torch.stack([q[:, -1], q[:, :-1].sum(-1)], -1)
    nl = -torch.log(torch.sigmoid(torch.stack([1 - x, x], -1)) + 1e-9)
    if efl:
        q2 = q2 * efl_weight(T, lam).unsqueeze(-1)
    return torch.sum(q2 * nl) * inv_norm, rpn_fg(T)


def kl_weight(slog_p, lam):
    """rpn.py:327-329, fast_rcnn.py:226-228: the Gaussian entropy weight of the teacher's variance"""
    ent = 0.5 * torch.log(2 * np.pi * np.e * torch.sigmoid(slog_p))
    return (1 - ent / (0.5 * math.log(2 * np.pi * np.e))) ** lam


def laplace_kl_weight(slog_p, lam):
    """rpn.py:319-321 (LAPLACE)"""
    return (1 - (1 + 0.5 * torch.log(4 * torch.sigmoid(slog_p))) / (1 + math.log(2))) ** lam


def _reduce(kl, fg, reduction, inv_norm):
    if fg is not None:
        kl = kl[fg.bool()]
    return kl.sum() * inv_norm if reduction == 0 else kl.mean()


def kl_efl_loss(q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
    """rpn.py:321-355 (reduction 0: sum over the fg rows * inv_norm), fast_rcnn.py:215-263 (reduction 1: mean over them)"""
    var_p = torch.sigmoid(slog_p) * tau
    var_q, mu_q = torch.sigmoid(q[:, 4:]), q[:, :4]
    kl = 0.5 * torch.log(var_q / var_p) - 0.5 + (var_p + (mu_q - mu_p) ** 2) / (2 * var_q)
    if efl:
        kl = kl * kl_weight(slog_p, lam)
    return _reduce(kl, fg, reduction, inv_norm)


def laplace_kl_efl_loss(q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
    """rpn.py:319-344, fast_rcnn.py:238-257 (LAPLACE), as tests/test_laplace_gpu.py restates it"""
    sp = torch.sigmoid(slog_p) * tau
    sq, mq = torch.sigmoid(q[:, 4:]), q[:, :4]
    ad = torch.abs(mq - mu_p)
    kl = torch.sqrt(sp) * torch.exp(-(ad / torch.sqrt(sp))) / torch.sqrt(sq) + ad / torch.sqrt(sq) + 0.5 * torch.log(sq / sp) - 1
    if efl:
        kl = kl * laplace_kl_weight(slog_p, lam)
    return _reduce(kl, fg, reduction, inv_norm)


# ================================================================================================ regimes
@dataclass(frozen=True)
class Regime:
    name: str
    op: str                 # bce | gnll | softmax_ce | softmax_rows | soft_ce_efl | rpn_soft_obj | kl_efl | laplace_kl_efl
    inputs: dict            # CPU tensors, float32 / int8 / int64 / uint8
    kw: dict = field(default_factory=dict)
    meta: dict = field(default_factory=dict)

    def with_kw(self, **kw):
        return replace(self, kw={**self.kw, **kw})

    def with_inputs(self, **inputs):
        return replace(self, inputs={**self.inputs, **inputs})


OUTPUTS = {"bce": ("loss", "dx"), "gnll": ("loss", "dd", "dt"), "softmax_ce": ("loss", "dx"), "softmax_rows": ("y",),
           "soft_ce_efl": ("loss", "dS"), "rpn_soft_obj": ("loss", "dx"), "kl_efl": ("loss", "dq", "dmu_p"),
           "laplace_kl_efl": ("loss", "dq", "dmu_p")}
_SUM_KW = {"inv_norm": INV_NORM}
_EFL_KW = {"tau": TAU, "lam": LAM, "efl": True, "inv_norm": INV_NORM}
_KL_KW = {"tau": TAU, "lam": LAM, "efl": True, "reduction": 0, "inv_norm": INV_NORM}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cycle(values, rows=ROWS):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.arange(rows) % len(values)]


def teacher_rows(rows, C, spread, gen):
    """rows of C teacher logits whose max - min is `spread` exactly: one entry 0, one entry `spread`, the rest uniform between"""
    T = torch.rand(rows, C, generator=gen) * spread
    for r in range(rows):
        p = torch.randperm(C, generator=gen)
        T[r, p[0]] = 0.0
        T[r, p[1]] = spread
    return T


# ---- plain regimes: randn only (the floor of every gradient comparison comes from these)
def bce_plain(seed=61):
    gen = _g(seed)
    x, lab = torch.randn(ROWS, generator=gen) * 3, torch.randint(-1, 2, (ROWS,), generator=gen).to(torch.int8)
    lab[0] = 1                                               # a single-element call still has a term
    return Regime("bce_plain", "bce", {"x": x, "lab": lab}, dict(_SUM_KW))


def gnll_plain(seed=62):
    gen = _g(seed)
    d = torch.randn(ROWS, 8, generator=gen)
    d[:, :4] *= 0.5
    return Regime("gnll_plain", "gnll", {"d": d, "t": d[:, :4] + torch.randn(ROWS, 4, generator=gen) * 0.3}, dict(_SUM_KW))


def softmax_plain(C=9, seed=63, op="softmax_ce"):
    gen = _g(seed + C)
    return Regime(f"{op}_plain_C{C}", op, {"x": torch.randn(ROWS, C, generator=gen) * 2,
                                           "tgt": torch.randint(0, C, (ROWS,), generator=gen)})


def soft_ce_plain(C=9, seed=64):
    gen = _g(seed + C)
    return Regime(f"soft_ce_plain_C{C}", "soft_ce_efl", {"T": torch.randn(ROWS, C, generator=gen) * 2,
                                                         "S": torch.randn(ROWS, C, generator=gen)}, dict(_EFL_KW))


def rpn_plain(C=9, seed=65):
    gen = _g(seed + C)
    return Regime(f"rpn_plain_C{C}", "rpn_soft_obj", {"T": torch.randn(ROWS, C, generator=gen) * 2,
                                                      "x": torch.randn(ROWS, generator=gen)}, dict(_EFL_KW))


def kl_plain(seed=66, op="kl_efl"):
    gen = _g(seed)
    q = torch.randn(ROWS, 8, generator=gen)
    q[:, :4] *= 0.5
    mu_p = q[:, :4] + torch.randn(ROWS, 4, generator=gen) * 0.3
    slog_p = torch.randn(ROWS, 4, generator=gen)
    fg = (torch.rand(ROWS, generator=gen) < 0.7).to(torch.uint8)
    fg[0] = 1                                                # an empty mean is NaN on both sides
    return Regime(f"{op}_plain", op, {"q": q, "mu_p": mu_p, "slog_p": slog_p, "fg": fg}, dict(_KL_KW))


def plain_of(op, C=9):
    if op == "bce":
        return bce_plain()
    if op == "gnll":
        return gnll_plain()
    if op in ("softmax_ce", "softmax_rows"):
        return softmax_plain(C, op=op)
    if op == "soft_ce_efl":
        return soft_ce_plain(C)
    if op == "rpn_soft_obj":
        return rpn_plain(C)
    return kl_plain(op=op)


# ---- saturation and edges
BCE_X = [0.0, 1e-4, -1e-4, 20.0, -20.0, 50.0, -50.0, 88.0, -88.0, 100.0, -100.0, 1000.0, -1000.0]
GNLL_SLOG = [-100.0, -30.0, -20.0, -10.0, 10.0, 20.0, 100.0]
GNLL_DELTA = [0.0, 1e-5, 1e-3, 0.1, 3.0, 50.0]
KL_SLOG_P = [-30.0, -10.0, 0.0, 6.0, 8.0, 10.0, 12.0]
KL_SLOG_Q = [-30.0, -20.0, 0.0, 20.0, 30.0]
SPREADS = [0.1, 1.0, 5.0, 20.0, 60.0, 80.0]
CLASSES = [2, 9, 21, 81]
SCALES = [1.0, 80.0, 1e4]
RPN_X_SCALES = [1.0, 20.0, 50.0, 100.0]
DENORMAL_SPREADS = [90.0, 95.0, 100.0]
SATURATED_SLOG_P = [17.0, 20.0, 40.0, 100.0]
BAND_SLOG_P = [12.5, 13.0, 14.0, 15.0, 16.0, 16.5]


def bce_saturated():
    """every x of BCE_X with every label of (-1, 0, 1): 39 entries, the rest plain"""
    r = bce_plain(71)
    x, lab = r.inputs["x"].clone(), r.inputs["lab"].clone()
    k = 0
    for v in BCE_X:
        for l in (-1, 0, 1):
            x[k], lab[k] = v, l
            k += 1
    return Regime("bce_saturated", "bce", {"x": x, "lab": lab}, dict(_SUM_KW))


def _set_delta(d, t, rows, mags):
    sign = torch.where(torch.arange(4) % 2 == 0, 1.0, -1.0)
    for r, m in zip(rows, mags):
        t[r] = d[r, :4] - sign * m if m else d[r, :4]


def gnll_sigma():
    r = gnll_plain(72)
    d = r.inputs["d"].clone()
    d[:, 4:] = _cycle(GNLL_SLOG).unsqueeze(1)
    return Regime("gnll_sigma", "gnll", {"d": d, "t": r.inputs["t"]}, dict(_SUM_KW))


def gnll_delta():
    """|mu - t| of GNLL_DELTA, signs alternating over the four coordinates; 0 is exact, 50 underflows the pdf (-log 1e-9, no gradient)"""
    r = gnll_plain(73)
    d, t = r.inputs["d"], r.inputs["t"].clone()
    _set_delta(d, t, range(ROWS), [GNLL_DELTA[i % len(GNLL_DELTA)] for i in range(ROWS)])
    return Regime("gnll_delta", "gnll", {"d": d, "t": t}, dict(_SUM_KW), {"zero_rows": list(range(0, ROWS, len(GNLL_DELTA)))})


def gnll_crossed():
    """GNLL_SLOG x GNLL_DELTA on the first 42 rows, the rest plain"""
    r = gnll_plain(74)
    d, t = r.inputs["d"].clone(), r.inputs["t"].clone()
    k = 0
    for s in GNLL_SLOG:
        for m in GNLL_DELTA:
            d[k, 4:] = s
            _set_delta(d, t, [k], [m])
            k += 1
    return Regime("gnll_crossed", "gnll", {"d": d, "t": t}, dict(_SUM_KW))


def _kl_special(i):
    """as test_laplace_gpu._kl_inputs: Delta = 0 exactly on every 8th row, and row 2 unselected"""
    i = {k: v.clone() for k, v in i.items()}
    i["mu_p"][0::8] = i["q"][0::8, :4]
    i["fg"][2] = 0
    return i, {"zero_rows": list(range(0, ROWS, 8))}


def kl_teacher_sigma():
    i, meta = _kl_special(kl_plain(75).inputs)
    i["slog_p"] = _cycle(KL_SLOG_P).unsqueeze(1).repeat(1, 4)
    return Regime("kl_teacher_sigma", "kl_efl", i, dict(_KL_KW), meta)


def kl_student_sigma():
    i, meta = _kl_special(kl_plain(76).inputs)
    i["q"][:, 4:] = _cycle(KL_SLOG_Q).unsqueeze(1)
    return Regime("kl_student_sigma", "kl_efl", i, dict(_KL_KW), meta)


def kl_crossed():
    """KL_SLOG_P x KL_SLOG_Q on the first 35 rows, the rest plain"""
    i, meta = _kl_special(kl_plain(77).inputs)
    k = 0
    for sp in KL_SLOG_P:
        for sq in KL_SLOG_Q:
            i["slog_p"][k] = sp
            i["q"][k, 4:] = sq
            k += 1
    return Regime("kl_crossed", "kl_efl", i, dict(_KL_KW), meta)


def kl_one_fg():
    i = {k: v.clone() for k, v in kl_plain(78).inputs.items()}
    i["fg"].zero_()
    i["fg"][17] = 1
    return Regime("kl_one_fg", "kl_efl", i, dict(_KL_KW), {"fg_only": True})


def _with_targets(r, C):
    x, tgt = r.inputs["x"], r.inputs["tgt"].clone()
    tgt[0], tgt[1] = 0, C - 1
    tgt[2], tgt[3] = int(np.argmax(x[2].numpy())), int(np.argmin(x[3].numpy()))
    return tgt


def softmax_scaled(op, C, scale):
    """plain or student logits of the given scale; targets include class 0, class C - 1, the row's argmax and its argmin.
    A condition on the inputs: where the target is the row's maximum and leads the runner-up by a gap of 8 .. 30, the gradient
    softmax - 1 = -e^-gap is a cancellation that ANY fp32 evaluation gets wrong by about 6e-8 e^gap (1e-2 at a gap of 12) while it is
    still above the floor.  Such a row's maximum is raised by 30: the true gradient is then below the floor."""
    r = softmax_plain(C, seed=80 + int(math.log10(scale) * 3), op=op)
    x = r.inputs["x"] / 2 * scale
    tgt = _with_targets(r.with_inputs(x=x), C)
    top = x.topk(2, dim=-1)
    gap = top.values[:, 0] - top.values[:, 1]
    for k in torch.nonzero((top.indices[:, 0] == tgt) & (gap > 8) & (gap < 30)).flatten().tolist():
        x[k, tgt[k]] += 30.0
    return Regime(f"{op}_C{C}_scale{scale:g}", op, {"x": x, "tgt": tgt})


def soft_ce_spread(C, spread):
    gen = _g(90 + C)
    return Regime(f"soft_ce_C{C}_spread{spread:g}", "soft_ce_efl",
                  {"T": teacher_rows(ROWS, C, spread, gen), "S": torch.randn(ROWS, C, generator=gen)}, dict(_EFL_KW))


def soft_ce_scaled(scale):
    """student logits of the given scale.  The teacher is mild here (randn / 2, so softmax(T / tau) stays away from 1): a saturated
    student against a saturated teacher is a second cause of trouble, p - q with both within 1e-4 of 1, whose fp32 error is 0, 1 or
    2 units of 6e-8 / (p - q) on either side by accident of rounding -- nothing a factor between two evaluations describes."""
    r = soft_ce_plain(9, seed=91)
    return Regime(f"soft_ce_scale{scale:g}", "soft_ce_efl", {"T": r.inputs["T"] / 4, "S": r.inputs["S"] * scale}, dict(_EFL_KW))


def rpn_spread(C, spread):
    gen = _g(92 + C)
    return Regime(f"rpn_C{C}_spread{spread:g}", "rpn_soft_obj",
                  {"T": teacher_rows(ROWS, C, spread, gen), "x": torch.randn(ROWS, generator=gen)}, dict(_EFL_KW))


def rpn_x_scaled(scale):
    r = rpn_plain(9, seed=93)
    return Regime(f"rpn_x{scale:g}", "rpn_soft_obj", {"T": r.inputs["T"], "x": r.inputs["x"] * scale}, dict(_EFL_KW))


def rpn_ties(C=9):
    """rows 0-31: the maximum tied between one foreground class and the last class (fg = 1: the lower index wins); rows 32-63: tied
    among two or three foreground classes only"""
    r = rpn_plain(C, seed=94)
    T = r.inputs["T"].clone()
    gen = _g(95)
    for k in range(ROWS):
        m = float(T[k].max()) + 1.0
        p = torch.randperm(C - 1, generator=gen)
        T[k, p[0]] = m
        if k < ROWS // 2:
            T[k, C - 1] = m
        else:
            T[k, p[1]] = m
            if k % 2:
                T[k, p[2]] = m
    return Regime(f"rpn_ties_C{C}", "rpn_soft_obj", {"T": T, "x": r.inputs["x"]}, dict(_EFL_KW))


def regimes():
    """every regime that goes through `check` (the plain ones included)"""
    out = [bce_plain(), bce_saturated(), gnll_plain(), gnll_sigma(), gnll_delta(), gnll_crossed(),
           kl_plain(), kl_teacher_sigma(), kl_student_sigma(), kl_crossed(), kl_one_fg(),
           soft_ce_plain(), rpn_plain(), rpn_ties()]
    for C in CLASSES:
        for s in SCALES:
            out.append(softmax_scaled("softmax_ce", C, s))
            out.append(softmax_scaled("softmax_rows", C, s))
        for s in SPREADS:
            out.append(soft_ce_spread(C, s))
            out.append(rpn_spread(C, s))
    out += [soft_ce_scaled(s) for s in SCALES] + [rpn_x_scaled(s) for s in RPN_X_SCALES]
    out += denormal_band()
    return out


def denormal_band():
    """teacher spread 90, 95, 100: softmax(T)'s smallest entry is an fp32 denormal; the fp32 reference keeps it and gives weight 1"""
    return [f(C, s) for C in (2, 9) for s in DENORMAL_SPREADS for f in (soft_ce_spread, rpn_spread)]


def beyond_denormal():
    """spread 120: exp underflows to 0 and 0 * log 0 makes the fp32 weight, and with it the loss, NaN (the kernel keeps it)"""
    return [f(C, 120.0) for C in (2, 9) for f in (soft_ce_spread, rpn_spread)]


def saturated_sigma(op, values=SATURATED_SLOG_P):
    """teacher sigma logits at which fp32 sigmoid is 1 exactly and the entropy weight's base 0: `values` cycled over the rows"""
    i = {k: v.clone() for k, v in kl_plain(96, op).inputs.items()}
    i["slog_p"] = _cycle(values).unsqueeze(1).repeat(1, 4)
    return Regime(f"{op}_slog_p_{'_'.join(f'{v:g}' for v in values)}", op, i, dict(_KL_KW))


def uniform_teacher(op, C, spread):
    """teacher rows that are uniform exactly (spread 0) or nearly (1e-4): the exact weight is below 1e-4"""
    f = soft_ce_spread if op == "soft_ce_efl" else rpn_spread
    r = f(C, spread if spread else 1.0)
    if not spread:
        T = torch.randn(ROWS, 1, generator=_g(97)).repeat(1, C)
    else:
        T = r.inputs["T"]
    return Regime(f"{op}_uniform_C{C}_spread{spread:g}", op, {**r.inputs, "T": T}, dict(_EFL_KW))


def variants(reg):
    """the settings each regime is checked under: efl on and off; for the KL both reductions, fg and None"""
    if reg.op in ("soft_ce_efl", "rpn_soft_obj"):
        return [(f"efl{int(e)}", reg.with_kw(efl=e)) for e in (True, False)]
    if reg.op in ("kl_efl", "laplace_kl_efl"):
        out = []
        for red, use_fg in ((0, True), (1, False), (1, True)):
            if reg.meta.get("fg_only") and not use_fg:
                continue
            for e in (True, False):
                out.append((f"red{red}_fg{int(use_fg)}_efl{int(e)}", reg.with_kw(reduction=red, efl=e, use_fg=use_fg)))
        return out
    return [("", reg)]


def cycled(reg, rows):
    """the regime's rows repeated to `rows` rows"""
    idx = torch.arange(rows) % ROWS
    return replace(reg, name=f"{reg.name}_x{rows}", inputs={k: v[idx].contiguous() for k, v in reg.inputs.items()})


# ================================================================================================ evaluation
def reference(reg, dtype):
    """the restatement in `dtype` on the CPU -> {"loss": ..., gradient name: ...} as float64 tensors; gradients of UP * loss"""
    i, kw = reg.inputs, dict(reg.kw)
    use_fg = kw.pop("use_fg", True)

    def leaf(name):
        return i[name].to(dtype).clone().requires_grad_()

    extra = {}
    if reg.op == "bce":
        leaves = {"dx": leaf("x")}
        loss = bce_logits_sum(leaves["dx"], i["lab"], **kw)
    elif reg.op == "gnll":
        leaves = {"dd": leaf("d"), "dt": leaf("t")}
        loss = gaussian_nll_sum(leaves["dd"], leaves["dt"], **kw)
    elif reg.op == "softmax_ce":
        leaves = {"dx": leaf("x")}
        loss = softmax_ce_mean(leaves["dx"], i["tgt"])
    elif reg.op == "softmax_rows":
        return {"y": softmax_rows(i["x"].to(dtype)).double()}
    elif reg.op == "soft_ce_efl":
        leaves = {"dS": leaf("S")}
        loss = soft_ce_efl(i["T"].to(dtype), leaves["dS"], **kw)
    elif reg.op == "rpn_soft_obj":
        leaves = {"dx": leaf("x")}
        loss, extra["fg"] = rpn_soft_obj_loss(i["T"].to(dtype), leaves["dx"], **kw)
    else:
        leaves = {"dq": leaf("q"), "dmu_p": leaf("mu_p")}
        fn = kl_efl_loss if reg.op == "kl_efl" else laplace_kl_efl_loss
        loss = fn(leaves["dq"], leaves["dmu_p"], i["slog_p"].to(dtype), i["fg"] if use_fg else None, **kw)
    (loss * UP).backward()
    out = {"loss": loss.detach().double()}
    for k, v in leaves.items():
        out[k] = v.grad.double()
    out.update(extra)
    return out


_floor_cache = {}


def floors(reg):
    """{output: floor}: 1e-12 for the loss; for a gradient (or softmax_rows' y) 1e-5 of the median nonzero |float64 value| of the
    op's PLAIN regime under the same settings -- never of the regime under test, where most true gradients may be ~1e-9"""
    C = next((v.shape[-1] for k, v in reg.inputs.items() if k in ("T", "x") and v.dim() == 2), 9)
    key = (reg.op, C, tuple(sorted(reg.kw.items())))
    if key not in _floor_cache:
        ref = reference(replace(plain_of(reg.op, C), kw=reg.kw), torch.float64)
        fl = {}
        for k in OUTPUTS[reg.op]:
            if k == "loss":
                fl[k] = LOSS_FLOOR
            else:
                nz = ref[k].abs()[ref[k] != 0]
                fl[k] = GRAD_FLOOR * float(nz.median())
        _floor_cache[key] = fl
    return _floor_cache[key]


def own_floors(ref64):
    """floors from the call's own float64 result: only for plain-regime inputs cycled to another length (the size tests)"""
    out = {}
    for k, v in ref64.items():
        if k == "loss":
            out[k] = LOSS_FLOOR
        elif k != "fg":
            nz = v.abs()[v != 0]
            out[k] = GRAD_FLOOR * float(nz.median()) if nz.numel() else 0.0
    return out


def rtol_of(output):
    return LOSS_RTOL if output in ("loss", "y") else GRAD_RTOL


def err(x, ref64, floor):
    x = np.asarray(x, dtype=np.float64)
    r = np.asarray(ref64, dtype=np.float64)
    assert x.shape == r.shape, f"shape {x.shape} vs {r.shape}"
    if not r.size:
        return 0.0
    d = np.abs(x - r)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(d == 0, 0.0, d / (np.abs(r) + floor))                 # an exact match is no error even where the floor is 0
    return float(np.max(np.where(np.isnan(e), np.inf, e)))


def check(got, ref64, ref32, base_rtol, floor, what="", margin=MARGIN):
    """err(got) <= max(base_rtol, margin * err(ref32)), and the yardstick itself within YARDSTICK_CAP; -> (err(got), err(ref32))"""
    eg, e32 = err(got, ref64, floor), err(ref32, ref64, floor)
    tol = max(base_rtol, margin * e32)
    if os.environ.get("PTMI_TEST_VERBOSE"):
        ratio = eg / e32 if e32 > 0 else float("inf") if eg > 0 else 0.0
        print(f"[check] {what}: err(got) {eg:.3e} err(ref32) {e32:.3e} ratio {ratio:.3f} tol-ratio {eg / tol:.3f}")
    assert e32 <= YARDSTICK_CAP, f"{what}: the fp32 yardstick is off by {e32:.3e} > {YARDSTICK_CAP:g}: move the regime"
    assert eg <= tol, f"{what}: err {eg:.3e} > max({base_rtol:g}, {margin:g} * {e32:.3e})"
    return eg, e32
