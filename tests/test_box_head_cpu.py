"""CPU: MODEL.ROI_BOX_HEAD.NUM_CONV / CONV_DIM / NORM -- what is decided on the host (no kernel runs here).

The module layout of FastRCNNConvFCHead against D2 0.5's, restated on plain torch modules (tests/box_head_ref.py): state-dict keys
and their order (they fix D2's optimiser numbering in checkpoints), shapes, init values, the values that raise, the norm
parameters' weight decay, and the index arithmetic of the ROI-mosaic restatement the GPU tests compare the kernels with."""
import os

import pytest
import torch

from tests import box_head_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["MODEL.ROI_BOX_HEAD.NUM_CONV", 2, "MODEL.ROI_BOX_HEAD.CONV_DIM", 64, "MODEL.ROI_BOX_HEAD.NUM_FC", 1]


def _cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), ["MODEL.DEVICE", "cpu", "MODEL.VGG.PRETRAIN", ""] + list(opts))


def _head(*opts, channels=96):
    from probabilisticteacher_amd.modeling.backbone import ShapeSpec
    from probabilisticteacher_amd.modeling.roi_heads import build_box_head
    return build_box_head(_cfg(*opts), ShapeSpec(channels=channels, height=7, width=7))


def _keys(norm, num_conv=2, num_fc=1):
    per_conv = ("weight", "norm.weight", "norm.bias") if norm else ("weight", "bias")
    return ([f"conv{k}.{s}" for k in range(1, num_conv + 1) for s in per_conv] +
            [f"fc{k}.{s}" for k in range(1, num_fc + 1) for s in ("weight", "bias")])


@pytest.mark.parametrize("norm", ["", "GN"])
def test_conv_head_has_the_reference_layout(norm):
    torch.manual_seed(3)
    head = _head(*HEAD, "MODEL.ROI_BOX_HEAD.NORM", norm)
    ref = br.RefHead(96, 7, 2, 64, 1, 1024, norm)
    sd, rsd = head.state_dict(), ref.state_dict()
    assert list(sd.keys()) == _keys(norm) == list(rsd.keys())
    assert [n for n, _ in head.named_parameters()] == _keys(norm)
    assert not list(head.named_buffers())
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    assert tuple(sd["conv1.weight"].shape) == (64, 96, 3, 3) and tuple(sd["conv2.weight"].shape) == (64, 64, 3, 3)
    assert tuple(sd["fc1.weight"].shape) == (1024, 64 * 49) and head.output_size == ref.output_size == 1024
    for k in (1, 2):
        w = sd[f"conv{k}.weight"]
        # c2_msra_fill: kaiming normal, fan_out, relu -> std sqrt(2 / (9 * cout)); 36864+ samples: the estimate is within 2 %
        assert abs(float(w.std()) / (2.0 / (9 * 64)) ** 0.5 - 1.0) < 0.02 and abs(float(w.mean())) < 1e-3
        if norm:
            assert f"conv{k}.bias" not in sd
            assert bool((sd[f"conv{k}.norm.weight"] == 1).all()) and bool((sd[f"conv{k}.norm.bias"] == 0).all())
            n = getattr(head, f"conv{k}").norm
            assert (n.num_groups, n.num_channels, n.eps) == (32, 64, 1e-5)
        else:
            assert bool((sd[f"conv{k}.bias"] == 0).all())
    # c2_xavier_fill: kaiming uniform with a = 1 -> bound sqrt(3 / fan_in)
    bound = (3.0 / (64 * 49)) ** 0.5
    assert float(sd["fc1.weight"].abs().max()) <= bound and float(sd["fc1.weight"].abs().max()) > 0.99 * bound
    assert bool((sd["fc1.bias"] == 0).all())


def test_norm_parameters_get_the_norm_weight_decay():
    from probabilisticteacher_amd.modeling import build_model
    from probabilisticteacher_amd.solver import norm_parameter_names, segment_weight_decay
    cfg = _cfg(*HEAD, "MODEL.ROI_BOX_HEAD.NORM", "GN", "SOLVER.WEIGHT_DECAY_NORM", 0.0)
    model = build_model(cfg)
    keys = [k for k in model.state_dict() if k.startswith("roi_heads.box_head.")]
    assert keys == ["roi_heads.box_head." + k for k in _keys("GN")]
    want = {f"roi_heads.box_head.conv{k}.norm.{s}" for k in (1, 2) for s in ("weight", "bias")}
    assert norm_parameter_names(model) == want
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    wd = dict(zip(names, segment_weight_decay(cfg, model, names)))
    assert all(wd[n] == 0.0 for n in want) and wd["roi_heads.box_head.conv1.weight"] == cfg.SOLVER.WEIGHT_DECAY == 1e-4
    assert tuple(model.roi_heads.box_predictor.cls_score.weight.shape) == (cfg.MODEL.ROI_HEADS.NUM_CLASSES + 1, 1024)


@pytest.mark.parametrize("norm", ["", "GN"])
def test_a_head_without_fc_layers_keeps_the_map(norm):
    head = _head("MODEL.ROI_BOX_HEAD.NUM_CONV", 1, "MODEL.ROI_BOX_HEAD.CONV_DIM", 64, "MODEL.ROI_BOX_HEAD.NUM_FC", 0,
                 "MODEL.ROI_BOX_HEAD.NORM", norm)
    assert head.output_size == 64 * 49 == br.RefHead(96, 7, 1, 64, 0, 1024, norm).output_size
    assert list(head.state_dict().keys()) == _keys(norm, 1, 0)


@pytest.mark.parametrize("value", ["BN", "SyncBN", "gn"])
def test_other_norms_raise(value):
    with pytest.raises(ValueError, match="MODEL.ROI_BOX_HEAD.NORM"):
        _head(*HEAD, "MODEL.ROI_BOX_HEAD.NORM", value)
    from probabilisticteacher_amd.modeling import build_model
    with pytest.raises(ValueError, match="MODEL.ROI_BOX_HEAD.NORM"):
        build_model(_cfg(*HEAD, "MODEL.ROI_BOX_HEAD.NORM", value))


def test_channels_that_do_not_divide_raise():
    with pytest.raises(ValueError, match="MODEL.ROI_BOX_HEAD.NORM.*CONV_DIM"):
        _head("MODEL.ROI_BOX_HEAD.NUM_CONV", 2, "MODEL.ROI_BOX_HEAD.CONV_DIM", 48, "MODEL.ROI_BOX_HEAD.NORM", "GN")
    _head("MODEL.ROI_BOX_HEAD.NUM_CONV", 2, "MODEL.ROI_BOX_HEAD.CONV_DIM", 48)          # (without a norm 48 channels are fine)


def test_conv_head_with_amp_raises():
    from probabilisticteacher_amd.modeling import build_model
    with pytest.raises(ValueError, match="MODEL.ROI_BOX_HEAD.NUM_CONV.*SOLVER.AMP.ENABLED"):
        build_model(_cfg(*HEAD, "SOLVER.AMP.ENABLED", True))
    build_model(_cfg("SOLVER.AMP.ENABLED", True))                                         # (AMP alone still builds)


def test_default_head_is_what_it_was():
    from probabilisticteacher_amd.modeling import build_model
    model = build_model(_cfg())
    keys = [k for k in model.state_dict() if k.startswith("roi_heads.box_head.")]
    assert keys == [f"roi_heads.box_head.fc{k}.{s}" for k in (1, 2) for s in ("weight", "bias")]
    head = model.roi_heads.box_head
    assert head.num_conv == 0 and head.output_size == 1024 and tuple(head.fc1.weight.shape) == (1024, 512 * 49)
    assert [n for n, _ in head.named_modules() if n] == ["fc1", "fc2"]


def test_mosaic_restatement_places_the_rois():
    """ROI r -> canvas r // 64, cell ((r % 64) // 8, r % 8) at pitch 8 for P = 7; 256 ROIs a canvas at pitch 4 for P = 3"""
    assert br.mosaic_geometry(130, 7) == (8, 8, 64, 3) and br.mosaic_geometry(130, 3) == (4, 16, 64, 1)
    assert br.mosaic_geometry(5, 14) == (15, 4, 60, 1) and br.mosaic_geometry(0, 7)[3] == 0
    from probabilisticteacher_amd import ops
    for r, pooled in ((130, 7), (130, 3), (5, 14), (0, 7), (3, 70)):
        assert ops.roi_mosaic_geometry(r, pooled) == br.mosaic_geometry(r, pooled)
    x = torch.arange(130 * 2 * 49, dtype=torch.float32).view(130, 2, 7, 7) + 1.0
    cv = br.mosaic_pack(x)
    assert tuple(cv.shape) == (3, 2, 64, 64)
    assert torch.equal(cv[1, :, 16:23, 40:47], x[64 + 2 * 8 + 5]) and torch.equal(cv[2, :, 0:7, 8:15], x[129])
    assert int((cv != 0).sum()) == x.numel() and bool((cv[:, :, 7::8, :] == 0).all()) and bool((cv[:, :, :, 7::8] == 0).all())
    assert bool((cv[2, :, 8:, :] == 0).all()) and bool((cv[2, :, :8, 16:] == 0).all())
    assert torch.equal(br.mosaic_unpack(cv, 130, 7), x)
    assert torch.equal(br.mosaic_data_mask(130, 7).expand_as(cv), cv != 0)


def test_the_fp32_yardstick_of_the_mosaic_groupnorm_cases_is_sound():
    """every case tests/test_box_head_gpu.py compares under tests/losses_ref.py::check has an fp32 CPU result within YARDSTICK_CAP of
    float64, and far inside it: no pre-ReLU value sits where float32 and float64 take different sides of the ReLU"""
    from tests import groupnorm_ref as gr
    worst = 0.0
    for c, r, pooled in br.GN_CASES:
        for offset in gr.OFFSETS:
            ins = gr.inputs((r, c, pooled, pooled), offset, seed=br.GN_SEED)
            r64, r32 = gr.reference(*ins, True, torch.float64), gr.reference(*ins, True, torch.float32)
            worst = max(worst, max(gr.err(r32[k].numpy(), r64[k].numpy(), gr.floor_of(r64[k])) for k in r64))
    assert worst <= 0.1 * gr.YARDSTICK_CAP, worst
