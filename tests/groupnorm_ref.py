"""Restatements for MODEL.VGG.NORM "GN" and SOLVER.WEIGHT_DECAY_NORM, shared by tests/test_groupnorm_cpu.py and
tests/test_groupnorm_gpu.py.

Layer: D2 get_norm("GN", C) is torch.nn.GroupNorm(32, C) (eps 1e-5, affine), D2's Conv2d computes norm(conv(x) + b) and
VGGBlock.forward applies F.relu_ (vgg.py:52,65-72).  `gn_relu` is that through torch.nn.functional.group_norm + relu, the primitive
D2 itself calls, differentiated by autograd; it runs unchanged in float32 and float64.

Comparison: tests/losses_ref.py::check -- err(got) <= max(base_rtol, 4 * err(ref32)) against float64, the fp32 CPU result being the
yardstick, valid while err(ref32) <= YARDSTICK_CAP = 1e-2; base_rtol LOSS_RTOL = 1e-5 for y and GRAD_RTOL = 1e-4 for gradients;
floor 1e-3 * max |ref64| per tensor.

Optimiser: `sgd_step64` restates one torch.optim.SGD(momentum, weight_decay) step behind the global clip and the per-parameter
clip of D2's maybe_add_gradient_clipping in float64, with one weight decay per segment (D2 get_default_optimizer_params:
SOLVER.WEIGHT_DECAY_NORM for norm parameters)."""
import math

import torch
import torch.nn.functional as F

from tests.losses_ref import GRAD_RTOL, LOSS_RTOL, YARDSTICK_CAP, check, err        # noqa: F401  (re-exported)

GROUPS, EPS = 32, 1e-5
FLOOR_SHARE = 1e-3
OFFSETS = (0.0, 3.0)

# (n, c, h, w): L = (c / 32) * h * w
SHAPES = [(2, 64, 5, 7),            # L 70: less than two waves, odd plane
          (1, 64, 37, 53),          # L 3922: not a multiple of 4, group starts off the 16-byte grid
          (2, 256, 1, 1),           # L 8
          (1, 64, 3, 1366),         # L 8196: long rows
          (3, 128, 64, 96),         # L 24576: n > 1, several pieces
          (1, 512, 50, 83),         # L 66400: conv5's real map
          (1, 64, 200, 336)]        # L 134400: many pieces


def chunk_plus_one_shape(chunk: int):
    """a shape whose groups hold chunk + 1 floats: c = 32 (one channel per group), h * w = chunk + 1"""
    n = chunk + 1
    h = next(d for d in range(int(math.isqrt(n)), 0, -1) if n % d == 0)
    return (1, 32, h, n // h)


def inputs(shape, offset, seed=0):
    """z = randn + offset, gamma ~ 1 +- 0.5, beta ~ +-0.5, upstream gradient randn: float32 CPU tensors"""
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(1000 * seed + c + h * w + int(offset))
    z = torch.randn(n, c, h, w, generator=gen) + offset
    gamma = 1.0 + (torch.rand(c, generator=gen) - 0.5)
    beta = torch.rand(c, generator=gen) - 0.5
    dy = torch.randn(n, c, h, w, generator=gen)
    return z, gamma, beta, dy


def gn_relu(z, gamma, beta, groups=GROUPS, eps=EPS, relu=True):
    y = F.group_norm(z, groups, gamma, beta, eps)
    return F.relu(y) if relu else y


def reference(z, gamma, beta, dy, relu, dtype, groups=GROUPS, eps=EPS):
    """{"y", "dz", "dgamma", "dbeta"} of the restatement in `dtype` on the CPU, as float64 tensors"""
    zz, gg, bb = (t.to(dtype).clone().requires_grad_() for t in (z, gamma, beta))
    y = gn_relu(zz, gg, bb, groups, eps, relu)
    y.backward(dy.to(dtype))
    return {"y": y.detach().double(), "dz": zz.grad.double(), "dgamma": gg.grad.double(), "dbeta": bb.grad.double()}


_REF = {}


def references(shape, offset, relu):
    """(ref64, ref32, inputs) of one case: computed once, shared by the tests, never written"""
    key = (tuple(shape), float(offset), bool(relu))
    if key not in _REF:
        ins = inputs(shape, offset)
        _REF[key] = (reference(*ins, relu, torch.float64), reference(*ins, relu, torch.float32), ins)
    return _REF[key]


def rtol_of(name):
    return LOSS_RTOL if name == "y" else GRAD_RTOL


def floor_of(ref64_tensor):
    return FLOOR_SHARE * float(ref64_tensor.abs().max())


def check_all(got, ref64, ref32, what):
    """every output of `got` ({"y", "dz", "dgamma", "dbeta"}) under the rule above -> {name: (err(got), err(ref32))}"""
    out = {}
    for k in ("y", "dz", "dgamma", "dbeta"):
        out[k] = check(got[k].detach().cpu().double().numpy(), ref64[k].numpy(), ref32[k].numpy(), rtol_of(k), floor_of(ref64[k]),
                       f"{what} {k}")
    return out


# ------------------------------------------------------------------------------------------------ optimiser
def d2_param_groups(model, base_lr, weight_decay, weight_decay_norm, norm_types):
    """D2 0.5 get_default_optimizer_params, restated for what this project accepts (BIAS_LR_FACTOR 1, WEIGHT_DECAY_BIAS ==
    WEIGHT_DECAY): modules in pre-order, named_parameters(recurse=False) of each, one group per trainable parameter seen for the
    first time; parameters of norm modules get weight_decay_norm.  -> ([group dict], [parameter name])"""
    groups, names, seen = [], [], set()
    for mod_name, mod in model.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            if not p.requires_grad or p in seen:
                continue
            seen.add(p)
            wd = weight_decay_norm if isinstance(mod, norm_types) else weight_decay
            groups.append({"params": [p], "lr": base_lr, "weight_decay": wd})
            names.append(f"{mod_name}.{pname}" if mod_name else pname)
    return groups, names


def sgd_step64(p, g, buf, offs, seg_wd, sumsq, clip_norm, clip_type, clip_value, inf_norm, lr, mu, first):
    """one fused step in float64 on CPU tensors -> (p', buf'): s = clip_norm / max(sqrt(sumsq), clip_norm); per segment
    g' = clip(g s) + wd_seg p; buf' = g' (first) or mu buf + g'; p' = p - lr buf'"""
    p, g, buf = p.double(), g.double(), buf.double()
    s = clip_norm / max(math.sqrt(float(sumsq)), clip_norm)
    pn, bn = p.clone(), buf.clone()
    for (a, b), wd in zip(zip(offs[:-1], offs[1:]), seg_wd):
        gs = g[a:b] * s
        if clip_type == "value":
            gs = gs.clamp(-clip_value, clip_value)
        elif clip_type == "norm" and b > a:
            nrm = float(gs.abs().max()) if inf_norm else float(gs.norm())
            gs = gs * min(clip_value / (nrm + 1e-6), 1.0)
        gs = gs + float(wd) * p[a:b]
        bn[a:b] = gs if first else mu * buf[a:b] + gs
        pn[a:b] = p[a:b] - lr * bn[a:b]
    return pn, bn
