"""VGG16 conv backbone on the MFMA conv kernels (reference pt/modeling/backbone/vgg.py).

Parameter names match the reference (`vgg_block{b}.0.conv{k}.{weight,bias}`, vgg.py:44,55,89-92) so its
checkpoints / the vgg16_caffe.pth key map (vgg.py:130-145) apply unchanged.  Blocks 1..FREEZE_AT are frozen
(vgg.py:175-180): they run without recording autograd state, so their activations are never kept.

MODEL.VGG.NORM (vgg.py:52,194 -> D2 get_norm): "None" (or "") builds the modules above; "GN" gives every convolution a `norm`
child, torch.nn.GroupNorm(32, C) as D2 builds it (eps 1e-5, weight 1, bias 0), with the reference's state-dict layout
`...conv{k}.weight, .bias, .norm.weight, .norm.bias`.  A layer is then relu(GN(conv(x) + b)) and the block runs layer by layer
(ops.conv3x3 without ReLU, ops.group_norm_relu, ops.maxpool2x2): the statistics need the whole map, so the fused block node, the
conv + pool epilogue and the frame skip belong to "None" only.  Every other value ("BN", "FrozenBN", "SyncBN", ...) raises."""
import os
from collections import namedtuple

import torch
from torch import nn

from .. import ops
from ..registry import BACKBONE_REGISTRY

ShapeSpec = namedtuple("ShapeSpec", ["channels", "height", "width", "stride"], defaults=[None, None, None, None])

VGG_CFGS = {
    11: [64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    13: [64, 64, "M", 128, 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    16: [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"],
    19: [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"],
}
_TORCHVISION_FEATURE_IDX = {16: [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]}


NORM_KEY = "MODEL.VGG.NORM"
NORMS = ("None", "GN")          # accepted values ("" counts as "None", as D2's get_norm treats it)
GN_GROUPS, GN_EPS = 32, 1e-5    # D2 get_norm("GN", C) = nn.GroupNorm(32, C)


def check_norm(norm) -> str:
    """MODEL.VGG.NORM -> "" (no norm layer) or "GN"; anything else raises"""
    if norm in ("", "None", None):
        return ""
    if norm == "GN":
        return "GN"
    raise ValueError(f"{NORM_KEY}={norm!r} is not implemented: accepted values are {', '.join(repr(v) for v in NORMS)} "
                     "(BN, FrozenBN and SyncBN need running statistics this build does not have)")


class _GroupNormParams(nn.Module):
    """`weight` / `bias` of a conv's GroupNorm(32, C) child (ones / zeros, torch.nn.GroupNorm's own init)."""

    def __init__(self, channels, groups=GN_GROUPS, eps=GN_EPS):
        super().__init__()
        if channels % groups:
            raise ValueError(f"{NORM_KEY}='GN': {channels} channels do not divide into {groups} groups")
        self.num_groups, self.num_channels, self.eps = groups, channels, eps
        self.weight = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))


class _ConvParams(nn.Module):
    """Holds `weight` / `bias` of one 3x3 conv (c2_msra_fill init, vgg.py:61-63) and, with a norm, its `norm` child -- set after
    the conv's own parameters, as D2's Conv2d does, so that it follows them in the state dict and in the optimiser's numbering."""

    def __init__(self, cin, cout, norm=""):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")
        self.out_channels = cout
        if norm:
            self.norm = _GroupNormParams(cout)


class VGGBlock(nn.Module):
    """[conv3x3 + bias + ReLU] x k, then MaxPool(2,2) unless it is the last block (vgg.py:36-72)."""

    def __init__(self, in_channels, channel_cfg, pool=True, norm=""):
        super().__init__()
        self.pool = pool
        self.norm = check_norm(norm)
        self.num_convs = len(channel_cfg)
        for i, cout in enumerate(channel_cfg):
            setattr(self, f"conv{i + 1}", _ConvParams(in_channels, cout, self.norm))
            in_channels = cout
        self.out_channels = in_channels
        self.stride = 2

    def conv_params(self):
        """[w1, b1, w2, b2, ...]: what ops.vgg_block, p8.block and ops.frozen_block take"""
        convs = [getattr(self, f"conv{i + 1}") for i in range(self.num_convs)]
        return [p for c in convs for p in (c.weight, c.bias)]

    def forward(self, x, frame=None):
        """frame: the batch's ops.FrameState at the block's input (shrink-pasted images), advanced layer by layer"""
        if self.norm:
            return self._forward_norm(x, frame)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return ops.vgg_block(x, self.pool, self.conv_params(), frame)     # one autograd node, fused backward chain
        return ops.frozen_block(ops.NCHW, x, *x.shape, self.pool, self.conv_params(), frame)     # layer by layer

    def _forward_norm(self, x, frame=None):
        """MODEL.VGG.NORM "GN": relu(GN(conv(x) + b)) layer by layer, then the pool.  The group statistics run over the whole
        map: no constant frame survives them, so the FrameState ends here.  A frozen block (it runs under no_grad) normalises
        with its per-sample statistics like any other: D2's freeze converts BatchNorm only."""
        ops._frame_end(frame)
        for i in range(self.num_convs):
            c = getattr(self, f"conv{i + 1}")
            with ops.anomaly_scope(f"conv{i + 1}"):
                x = ops.conv3x3(x, c.weight, c.bias, False)
                with ops.anomaly_scope("norm"):
                    x = ops.group_norm_relu(x, c.norm.weight, c.norm.bias, c.norm.num_groups, c.norm.eps, True)
        return ops.maxpool2x2(x) if self.pool else x

    def freeze(self):
        for p in self.parameters():         # (the norm children's parameters included, as CNNBlockBase.freeze)
            p.requires_grad = False
        return self


class VGG(nn.Module):
    def __init__(self, stages, out_features=None, pretrain=""):
        super().__init__()
        self._names = []
        stride = 1
        self._out_feature_strides, self._out_feature_channels = {}, {}
        for i, block in enumerate(stages):
            name = f"vgg_block{i + 1}"
            self.add_module(name, nn.Sequential(block))
            self._names.append(name)
            if name == "vgg_block5":
                self._out_feature_strides[name] = self._out_feature_strides["vgg_block4"]
            else:
                stride *= block.stride
                self._out_feature_strides[name] = stride
            self._out_feature_channels[name] = block.out_channels
        self._out_features = out_features or [self._names[-1]]
        if pretrain:
            self._load_pretrained(pretrain)

    def _load_pretrained(self, path):
        """vgg.py:127-152: torchvision `features.N` keys -> `vgg_block{b}.0.conv{k}`."""
        if not os.path.exists(path):
            raise FileNotFoundError(f"MODEL.VGG.PRETRAIN={path!r} not found (set it to '' for random init)")
        sd = torch.load(path, map_location="cpu")
        names = [f"{n}.0.conv{k + 1}" for n in self._names for k in range(getattr(self, n)[0].num_convs)]
        own = self.state_dict()
        for idx, name in zip(_TORCHVISION_FEATURE_IDX[16], names):
            for suffix in ("weight", "bias"):
                if f"{name}.{suffix}" in own:           # (conv weights only: norm parameters keep their init, vgg.py:150 strict=False)
                    own[f"{name}.{suffix}"].copy_(sd[f"features.{idx}.{suffix}"])

    @property
    def size_divisibility(self):
        return 0

    def _forward_p8(self, x):
        """SOLVER.AMP.ENABLED: the whole stack on bf16-storage (P8) tensors -- the image is converted once (3 channels padded to
        one 16-channel chunk), every layer reads and writes bf16 (probabilisticteacher_amd/p8.py), and each requested feature map
        is converted back to fp32 NCHW once (its gradient re-enters the stack through the same conversion)."""
        from .. import p8
        n, c, h, w = x.shape
        t = p8.from_nchw(ops._chk(x.contiguous(), name="image batch"))
        outputs = {}
        for name in self._names:
            blk = getattr(self, name)[0]
            params = blk.conv_params()
            trainable = torch.is_grad_enabled() and any(p.requires_grad for p in params)
            if trainable or t.requires_grad:
                with ops.anomaly_scope(name + ".0"):
                    t = p8.block(t, n, c, h, w, blk.pool, params)
            else:
                with torch.no_grad():       # (so the last convolution pools in its epilogue)
                    t = ops.frozen_block(p8.P8, t, n, c, h, w, blk.pool, params)
            c = blk.out_channels
            if blk.pool:
                h, w = h // 2, w // 2
            if name in self._out_features:
                with ops.anomaly_scope(name):
                    outputs[name] = p8._ToNCHW.apply(t, n, c, h, w)
        return outputs

    def forward(self, x, frame=None):
        """frame: ops.FrameState of a batch with shrink-pasted images (meta_arch.preprocess_image), or None"""
        if ops._native_bf16():
            if any(getattr(self, name)[0].norm for name in self._names):
                raise ValueError(f"{NORM_KEY}='GN' with SOLVER.AMP.ENABLED: the bf16-storage stack has no norm layer")
            return self._forward_p8(x)
        outputs = {}
        for name in self._names:
            block = getattr(self, name)[0]
            frozen = not any(p.requires_grad for p in block.parameters())
            if frame is not None and not frame.alive:
                frame = None
            with ops.anomaly_scope(name + ".0"):          # (the state-dict path of the block's module: vgg_block{b}.0.conv{k})
                if frozen and not x.requires_grad:
                    with torch.no_grad():
                        x = block(x, frame)
                else:
                    x = block(x, frame)
            if name in self._out_features:
                outputs[name] = x
        return outputs

    def output_shape(self):
        return {n: ShapeSpec(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n])
                for n in self._out_features}

    def freeze(self, freeze_at=0):
        for idx, name in enumerate(self._names, start=1):
            if freeze_at >= idx:
                getattr(self, name)[0].freeze()
        return self


@BACKBONE_REGISTRY.register()
def build_vgg_backbone(cfg, input_shape):
    depth = cfg.MODEL.VGG.DEPTH
    norm = check_norm(cfg.MODEL.VGG.NORM)
    out_features = cfg.MODEL.VGG.OUT_FEATURES
    layout = VGG_CFGS[depth]
    max_stage = max({"vgg_block1": 1, "vgg_block2": 2, "vgg_block3": 3, "vgg_block4": 4, "vgg_block5": 5}[f]
                    for f in out_features)
    pools = [i for i, v in enumerate(layout) if v == "M"]
    stages, start, cin = [], 0, input_shape.channels
    for s in range(max_stage):
        chans = layout[start:pools[s]]
        stages.append(VGGBlock(cin, chans, pool=(s + 1 != 5), norm=norm))
        cin, start = chans[-1], pools[s] + 1
    pretrain = cfg.MODEL.VGG.PRETRAIN if cfg.MODEL.VGG.PRETRAIN else ""
    return VGG(stages, out_features=out_features, pretrain=pretrain).freeze(cfg.MODEL.BACKBONE.FREEZE_AT)


def build_backbone(cfg, input_shape=None):
    if input_shape is None:
        input_shape = ShapeSpec(channels=len(cfg.MODEL.PIXEL_MEAN))
    return BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, input_shape)
