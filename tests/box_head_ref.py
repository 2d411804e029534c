"""Literal restatement of detectron2 0.5's FastRCNNConvFCHead (modeling/roi_heads/box_head.py) on plain torch modules, shared by
tests/test_box_head_cpu.py and tests/test_box_head_gpu.py.  D2 is not installed here: parity is by restatement.

    Conv2d          D2's layers/wrappers.py Conv2d: nn.Conv2d with a `norm` child and an `activation`, forward conv -> norm -> act
    get_norm        D2's layers/batch_norm.py get_norm for the values this project accepts: "" -> None, "GN" -> nn.GroupNorm(32, C)
    RefHead         the nn.Sequential D2 builds: conv{k} = Conv2d(3x3, padding 1, bias=not norm, norm, ReLU), `flatten`, fc{k} =
                    nn.Linear + fc_relu{k}; c2_msra_fill on the convs, c2_xavier_fill on the fcs

It runs unchanged in float32 and float64.  `reference` differentiates it by autograd; `mosaic_*` restate the ROI-mosaic layout
(csrc/roi_mosaic.hip) by index arithmetic."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

GROUPS, EPS = 32, 1e-5

# (C, R, P): the issue's grid at P = 7 -- C = 32 has L = 49, odd and off the 16-byte grid -- and one shape per other path: P = 3
# (quads, 256 ROIs a canvas) and P = 6 (63 x 63 canvases: single floats)
GN_CASES = [(c, r, 7) for c in (32, 64, 256) for r in (1, 65, 130)] + [(64, 65, 3), (32, 65, 6)]
GN_SEED = 1         # of tests/groupnorm_ref.py::inputs.  Seed 0 puts one pre-ReLU value of (C 256, R 130, offset 3) within fp32 rounding
                    # of zero: float32 and float64 then take different sides of the ReLU and the fp32 CPU yardstick is off by 58 in
                    # dz.  tests/test_box_head_cpu.py holds the yardstick of every case to YARDSTICK_CAP under this seed.


def get_norm(norm, channels):
    if not norm:
        return None
    return {"GN": lambda c: nn.GroupNorm(GROUPS, c)}[norm](channels)


class Conv2d(nn.Conv2d):
    def __init__(self, *args, norm=None, activation=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.norm, self.activation = norm, activation

    def forward(self, x):
        x = F.conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)
        if self.norm is not None:
            x = self.norm(x)
        if self.activation is not None:
            x = self.activation(x)
        return x


class RefHead(nn.Sequential):
    def __init__(self, channels, pooled, num_conv, conv_dim, num_fc, fc_dim, norm=""):
        super().__init__()
        self._output_size = (channels, pooled, pooled)
        for k in range(num_conv):
            conv = Conv2d(self._output_size[0], conv_dim, kernel_size=3, padding=1, bias=not norm, norm=get_norm(norm, conv_dim),
                          activation=nn.ReLU())
            self.add_module(f"conv{k + 1}", conv)
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")        # c2_msra_fill
            if conv.bias is not None:
                nn.init.constant_(conv.bias, 0)
            self._output_size = (conv_dim, pooled, pooled)
        for k in range(num_fc):
            if k == 0:
                self.add_module("flatten", nn.Flatten())
            fc = nn.Linear(int(np.prod(self._output_size)), fc_dim)
            self.add_module(f"fc{k + 1}", fc)
            self.add_module(f"fc_relu{k + 1}", nn.ReLU())
            nn.init.kaiming_uniform_(fc.weight, a=1)                                          # c2_xavier_fill
            nn.init.constant_(fc.bias, 0)
            self._output_size = fc_dim

    @property
    def output_size(self):
        return int(np.prod(self._output_size))


def perturb_(module, gen):
    """norm weights to 1 +- 0.5, every bias to +-0.5: away from the init values a wrong wiring would hide behind"""
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(1.0 + (torch.rand(p.shape, generator=gen) - 0.5))
            elif n.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)


def reference(ref_head, x, up, dtype):
    """{"out", "dx", name: gradient of every parameter} of sum(head(x) * up) in `dtype` on the CPU, as float64 tensors"""
    import copy
    head = copy.deepcopy(ref_head).to(dtype)
    xx = x.to(dtype).clone().requires_grad_()
    out = head(xx)
    (out * up.to(dtype)).sum().backward()
    res = {"out": out.detach().double(), "dx": xx.grad.double()}
    res.update({n: p.grad.double() for n, p in head.named_parameters()})
    return res


# ------------------------------------------------------------------------------------------------ the mosaic layout
def mosaic_geometry(r, pooled):
    p = pooled + 1
    gx = max(1, 64 // p)
    return p, gx, gx * p, -(-r // (gx * gx))


def mosaic_index(r, pooled):
    """(canvas, y, x) int64 tensors of shape (r, pooled, pooled): where pixel (iy, ix) of ROI i sits"""
    p, gx, _, _ = mosaic_geometry(r, pooled)
    i = torch.arange(r).view(r, 1, 1)
    cell = i % (gx * gx)
    iy, ix = torch.arange(pooled).view(1, pooled, 1), torch.arange(pooled).view(1, 1, pooled)
    cv = (i // (gx * gx)).expand(r, pooled, pooled)
    return cv, ((cell // gx) * p + iy).expand(r, pooled, pooled), ((cell % gx) * p + ix).expand(r, pooled, pooled)


def mosaic_pack(x):
    """(R, C, P, P) -> (canvases, C, S, S) with zeros in gutters and empty cells"""
    r, c, pooled, _ = x.shape
    _, _, s, ncv = mosaic_geometry(r, pooled)
    out = torch.zeros(ncv, c, s, s, dtype=x.dtype)
    if r:
        cv, yy, xx = mosaic_index(r, pooled)
        out[cv, :, yy, xx] = x.permute(0, 2, 3, 1)
    return out


def mosaic_unpack(canvas, r, pooled):
    if r == 0:
        return canvas.new_zeros((0, canvas.shape[1], pooled, pooled))
    cv, yy, xx = mosaic_index(r, pooled)
    return canvas[cv, :, yy, xx].permute(0, 3, 1, 2).contiguous()


def mosaic_data_mask(r, pooled):
    """bool (canvases, 1, S, S): True on data pixels"""
    _, _, s, ncv = mosaic_geometry(r, pooled)
    m = torch.zeros(ncv, 1, s, s, dtype=torch.bool)
    if r:
        cv, yy, xx = mosaic_index(r, pooled)
        m[cv, 0, yy, xx] = True
    return m
