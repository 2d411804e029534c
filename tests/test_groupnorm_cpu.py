"""CPU: MODEL.VGG.NORM "GN" and SOLVER.WEIGHT_DECAY_NORM -- what is decided on the host (no kernel runs here).

Accepted values and the values that raise, the reference's state-dict layout of a GN backbone, the per-segment weight-decay table,
the optimiser state against a real torch.optim.SGD built by D2's get_default_optimizer_params rule (tests/groupnorm_ref.py), and
the soundness of the fp32 yardstick tests/test_groupnorm_gpu.py compares the kernels with."""
import os

import pytest
import torch

from tests import groupnorm_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), ["MODEL.DEVICE", "cpu", "MODEL.VGG.PRETRAIN", ""] + list(opts))


def _backbone(*opts):
    from probabilisticteacher_amd.modeling.backbone import build_backbone
    return build_backbone(_cfg(*opts))


def _cpu_trainer(tmp_path, extra=()):
    """as tests/test_host_logic.py::_cpu_trainer"""
    from probabilisticteacher_amd.engine import PTrainer
    cfg = _cfg("MODEL.ANCHOR_GENERATOR.NAME", "DifferentiableAnchorGenerator", "OUTPUT_DIR", str(tmp_path), *extra)
    return cfg, PTrainer(cfg)


CONVS = [(1, 1, 64), (1, 2, 64), (2, 1, 128), (2, 2, 128), (3, 1, 256), (3, 2, 256), (3, 3, 256), (4, 1, 512), (4, 2, 512), (4, 3, 512),
         (5, 1, 512), (5, 2, 512), (5, 3, 512)]


def test_gn_builds_with_the_reference_layout():
    bb = _backbone("MODEL.VGG.NORM", "GN")
    want = [f"vgg_block{b}.0.conv{k}.{s}" for b, k, _ in CONVS for s in ("weight", "bias", "norm.weight", "norm.bias")]
    assert list(bb.state_dict().keys()) == want
    assert [n for n, _ in bb.named_parameters()] == want
    assert not list(bb.named_buffers()), "GroupNorm has no running statistics"
    sd = bb.state_dict()
    for b, k, c in CONVS:
        w, bias = sd[f"vgg_block{b}.0.conv{k}.norm.weight"], sd[f"vgg_block{b}.0.conv{k}.norm.bias"]
        assert w.shape == bias.shape == (c,) and bool((w == 1).all()) and bool((bias == 0).all())
        norm = getattr(getattr(bb, f"vgg_block{b}")[0], f"conv{k}").norm
        assert (norm.num_groups, norm.eps) == (32, 1e-5)


def test_none_keeps_the_modules_it_had():
    for value in ("None", ""):
        bb = _backbone("MODEL.VGG.NORM", value)
        assert list(bb.state_dict().keys()) == [f"vgg_block{b}.0.conv{k}.{s}" for b, k, _ in CONVS for s in ("weight", "bias")]
        assert not [n for n, _ in bb.named_modules() if n.endswith("norm")]


@pytest.mark.parametrize("value", ["BN", "FrozenBN", "SyncBN", "gn"])
def test_other_norms_raise(value):
    with pytest.raises(ValueError, match="MODEL.VGG.NORM"):
        _backbone("MODEL.VGG.NORM", value)
    from probabilisticteacher_amd.modeling import build_model
    with pytest.raises(ValueError, match="MODEL.VGG.NORM"):
        build_model(_cfg("MODEL.VGG.NORM", value))


def test_gn_with_amp_raises():
    from probabilisticteacher_amd.modeling import build_model
    with pytest.raises(ValueError, match="MODEL.VGG.NORM"):
        build_model(_cfg("MODEL.VGG.NORM", "GN", "SOLVER.AMP.ENABLED", True))
    build_model(_cfg("MODEL.VGG.NORM", "None", "SOLVER.AMP.ENABLED", True))       # (AMP alone still builds)


def test_channels_that_do_not_divide_raise():
    from probabilisticteacher_amd.modeling.backbone import VGGBlock
    with pytest.raises(ValueError, match="MODEL.VGG.NORM"):
        VGGBlock(3, [48], norm="GN")


def test_freeze_covers_the_norm_parameters():
    bb = _backbone("MODEL.VGG.NORM", "GN", "MODEL.BACKBONE.FREEZE_AT", 2)
    for n, p in bb.named_parameters():
        assert p.requires_grad == (n.split(".")[0] not in ("vgg_block1", "vgg_block2")), n


@pytest.mark.parametrize("value", [-1e-4, float("nan"), float("inf")])
def test_weight_decay_norm_must_be_finite_and_non_negative(value):
    from probabilisticteacher_amd.solver import check_optimizer_options
    with pytest.raises(ValueError, match="WEIGHT_DECAY_NORM"):
        check_optimizer_options(_cfg("SOLVER.WEIGHT_DECAY_NORM", value))
    check_optimizer_options(_cfg("SOLVER.WEIGHT_DECAY_NORM", 0.0))
    check_optimizer_options(_cfg("SOLVER.WEIGHT_DECAY_NORM", 0.5))


@pytest.fixture(scope="module")
def gn_trainer(tmp_path_factory):
    return _cpu_trainer(tmp_path_factory.mktemp("gn"), ["MODEL.VGG.NORM", "GN"])


def test_trainer_state_dict_order(gn_trainer):
    _, tr = gn_trainer
    keys = [k for k in tr.ensem_ts_model.state_dict().keys() if k.startswith("modelStudent.backbone.")]
    want = [f"modelStudent.backbone.vgg_block{b}.0.conv{k}.{s}" for b, k, _ in CONVS for s in ("weight", "bias", "norm.weight", "norm.bias")]
    assert keys == want
    assert [k.replace("modelTeacher.", "modelStudent.") for k in tr.ensem_ts_model.state_dict().keys()
            if k.startswith("modelTeacher.backbone.")] == want


def test_weight_decay_table(gn_trainer):
    from probabilisticteacher_amd.engine.flat import segment_offsets
    cfg, tr = gn_trainer
    names = [n for n, p in tr.student.params.items() if p.requires_grad]
    offs = segment_offsets(tr.student)
    assert len(tr.segment_wd) == len(names) == len(offs) - 1
    n_norm = 0
    for n, wd, a, b in zip(names, tr.segment_wd, offs[:-1], offs[1:]):
        assert (a, b - a) == tr.student.index[n]
        assert wd == (0.0 if ".norm." in n else cfg.SOLVER.WEIGHT_DECAY), n
        n_norm += ".norm." in n
    assert n_norm == 2 * len([c for c in CONVS if c[0] > cfg.MODEL.BACKBONE.FREEZE_AT]) > 0
    assert tr._seg_wd is not None and tr._seg_wd.tolist() == [float(torch.tensor(w, dtype=torch.float32)) for w in tr.segment_wd]
    assert tr._wd_segments.S == len(names)


def test_equal_decays_keep_the_plain_step(tmp_path):
    _, tr = _cpu_trainer(tmp_path, ["MODEL.VGG.NORM", "GN", "SOLVER.WEIGHT_DECAY_NORM", 0.0001])
    assert tr._seg_wd is None and tr._wd_segments is None and tr._segments is None
    _, tr = _cpu_trainer(tmp_path)
    assert tr._seg_wd is None and tr._wd_segments is None and tr._segments is None


def _torch_sgd(cfg, tr):
    from probabilisticteacher_amd.modeling.backbone import _GroupNormParams
    S = cfg.SOLVER
    groups, names = gr.d2_param_groups(tr.model, S.BASE_LR, S.WEIGHT_DECAY, S.WEIGHT_DECAY_NORM, (_GroupNormParams,))
    return torch.optim.SGD(groups, lr=S.BASE_LR, momentum=S.MOMENTUM), names


def test_optimizer_state_round_trip_with_torch_sgd(gn_trainer):
    from probabilisticteacher_amd import checkpoint
    cfg, tr = gn_trainer
    sgd, names = _torch_sgd(cfg, tr)
    assert names == checkpoint._trainable_names(tr)
    k = names.index("backbone.vgg_block3.0.conv1.weight")
    assert names[k:k + 4] == [f"backbone.vgg_block3.0.conv1.{s}" for s in ("weight", "bias", "norm.weight", "norm.bias")]
    gen = torch.Generator().manual_seed(3)
    tr.momentum_buf.copy_(torch.randn(tr.momentum_buf.shape, generator=gen))
    tr._first_step = False
    osd = checkpoint.optimizer_state_dict(tr)
    for g, n in zip(osd["param_groups"], names):
        assert g["weight_decay"] == (cfg.SOLVER.WEIGHT_DECAY_NORM if ".norm." in n else cfg.SOLVER.WEIGHT_DECAY), n
    assert {g["weight_decay"] for g in osd["param_groups"]} == {0.0, cfg.SOLVER.WEIGHT_DECAY}
    sgd.load_state_dict(osd)                                          # a real torch optimiser takes the file ...
    for g, n in zip(sgd.param_groups, names):
        assert g["weight_decay"] == (0.0 if ".norm." in n else cfg.SOLVER.WEIGHT_DECAY)
        off, cnt = tr.student.index[n]
        assert torch.equal(sgd.state[g["params"][0]]["momentum_buffer"].reshape(-1), tr.momentum_buf[off:off + cnt])
    back = sgd.state_dict()                                           # ... and what it writes loads back
    keep = tr.momentum_buf.clone()
    tr.momentum_buf.zero_()
    checkpoint.load_optimizer_state_dict(tr, back)
    assert torch.equal(tr.momentum_buf, keep) and not tr._first_step


def test_checkpoints_between_none_and_gn(gn_trainer, tmp_path):
    """D2's IncompatibleKeys: a "None" file in a GN model misses the norm keys, a GN file in a "None" model has them left over"""
    from probabilisticteacher_amd import checkpoint
    _, gn = gn_trainer
    _, plain = _cpu_trainer(tmp_path)
    a = checkpoint.save_checkpoint(plain, str(tmp_path / "plain.pth"), iteration=0)
    b = checkpoint.save_checkpoint(gn, str(tmp_path / "gn.pth"), iteration=0)
    inc = checkpoint.load_checkpoint(gn, a, resume=False)
    assert inc.missing_keys and all(".norm." in k for k in inc.missing_keys) and not inc.unexpected_keys
    assert len(inc.missing_keys) == 2 * 2 * len(CONVS)
    inc = checkpoint.load_checkpoint(plain, b, resume=False)
    assert inc.unexpected_keys and all(".norm." in k for k in inc.unexpected_keys) and not inc.missing_keys
    inc = checkpoint.load_checkpoint(gn, b, resume=True)
    assert not inc.missing_keys and not inc.unexpected_keys and not inc.incorrect_shapes


def test_pretrained_weights_leave_the_norm_parameters(tmp_path):
    from probabilisticteacher_amd.modeling.backbone import _TORCHVISION_FEATURE_IDX
    gen = torch.Generator().manual_seed(4)
    sd = {}
    for idx, (_, _, c), cin in zip(_TORCHVISION_FEATURE_IDX[16], CONVS, [3] + [c for _, _, c in CONVS[:-1]]):
        sd[f"features.{idx}.weight"] = torch.randn(c, cin, 3, 3, generator=gen)
        sd[f"features.{idx}.bias"] = torch.randn(c, generator=gen)
    path = str(tmp_path / "vgg16.pth")
    torch.save(sd, path)
    own = _backbone("MODEL.VGG.NORM", "GN", "MODEL.VGG.PRETRAIN", path).state_dict()
    assert torch.equal(own["vgg_block3.0.conv2.weight"], sd["features.12.weight"])
    assert torch.equal(own["vgg_block1.0.conv1.bias"], sd["features.0.bias"])
    assert bool((own["vgg_block3.0.conv2.norm.weight"] == 1).all()) and bool((own["vgg_block3.0.conv2.norm.bias"] == 0).all())


def test_sgd_step_restatement_is_torch_sgd():
    """tests/groupnorm_ref.py::sgd_step64 against torch.optim.SGD in float64 with per-group weight decay, two steps"""
    offs, wds = [0, 5, 69, 70], [1e-4, 0.0, 1e-4]
    gen = torch.Generator().manual_seed(5)
    p0, g = torch.randn(70, generator=gen, dtype=torch.float64), torch.randn(70, generator=gen, dtype=torch.float64) * 3
    params = [p0[a:b].clone().requires_grad_() for a, b in zip(offs[:-1], offs[1:])]
    sgd = torch.optim.SGD([{"params": [q], "weight_decay": w} for q, w in zip(params, wds)], lr=0.01, momentum=0.9)
    p, buf = p0.clone(), torch.zeros(70, dtype=torch.float64)
    ss = float((g * g).sum())
    s = 10.0 / max(ss ** 0.5, 10.0)
    assert s < 1.0
    for step in range(2):
        for q, (a, b) in zip(params, zip(offs[:-1], offs[1:])):
            q.grad = (g[a:b] * s).clone()
        sgd.step()
        p, buf = gr.sgd_step64(p, g, buf, offs, wds, ss, 10.0, "none", 0.0, False, 0.01, 0.9, step == 0)
        assert torch.allclose(p, torch.cat([q.detach() for q in params]), rtol=1e-13, atol=0)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("offset", gr.OFFSETS)
def test_yardstick_stays_within_the_cap(offset, relu):
    """the fp32 CPU restatement, which the GPU test measures the kernels with, is itself within YARDSTICK_CAP of float64 for
    every shape of the GPU test (the piece size does not matter here: 4097 stands for the chunk + 1 shape)"""
    worst = 0.0
    for shape in gr.SHAPES + [gr.chunk_plus_one_shape(4096)]:
        ref64, ref32, _ = gr.references(shape, offset, relu)
        for k in ("y", "dz", "dgamma", "dbeta"):
            e = gr.err(ref32[k].numpy(), ref64[k].numpy(), gr.floor_of(ref64[k]))
            worst = max(worst, e)
            assert e <= gr.YARDSTICK_CAP, f"{shape} offset {offset} relu {relu} {k}: yardstick off by {e:.3e}"
    print(f"[groupnorm] offset {offset} relu {relu}: worst yardstick error {worst:.3e}")
