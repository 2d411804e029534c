"""CPU: SOLVER.CLIP_GRADIENTS -- the config keys (detectron2 0.5 defaults), their validation in solver.check_optimizer_options
and the host-side segment / chunk tables of the per-parameter clipping kernels."""
import math

import pytest
import torch
from torch import nn

from probabilisticteacher_amd.config import setup_cfg
from probabilisticteacher_amd.engine.flat import FlatParams, segment_chunks, segment_offsets
from probabilisticteacher_amd.solver import check_optimizer_options, clip_gradients_options

KEY = "SOLVER.CLIP_GRADIENTS."


def test_defaults_are_those_of_detectron2():
    G = setup_cfg().SOLVER.CLIP_GRADIENTS
    assert G.ENABLED is False and G.CLIP_TYPE == "value" and G.CLIP_VALUE == 1.0 and G.NORM_TYPE == 2.0
    assert isinstance(G.CLIP_VALUE, float) and isinstance(G.NORM_TYPE, float)
    assert clip_gradients_options(setup_cfg()) is None


def test_keys_load_from_yaml_and_overrides(tmp_path):
    path = tmp_path / "clip.yaml"
    path.write_text("SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    CLIP_TYPE: norm\n    CLIP_VALUE: 0.5\n    NORM_TYPE: inf\n")
    cfg = setup_cfg(str(path))
    G = cfg.SOLVER.CLIP_GRADIENTS
    assert G.ENABLED is True and G.CLIP_TYPE == "norm" and G.CLIP_VALUE == 0.5 and G.NORM_TYPE == math.inf
    check_optimizer_options(cfg)
    assert clip_gradients_options(cfg) == ("norm", 0.5, True)
    path.write_text("SOLVER:\n  CLIP_GRADIENTS:\n    ENABLED: True\n    NORM_TYPE: .inf\n    CLIP_VALUE: 2\n")
    assert clip_gradients_options(setup_cfg(str(path))) == ("value", 2.0, True)
    # command-line overrides: typed values and the strings a shell delivers
    cfg = setup_cfg("", [KEY + "ENABLED", True, KEY + "CLIP_TYPE", "norm", KEY + "CLIP_VALUE", 0.25, KEY + "NORM_TYPE", 2.0])
    assert clip_gradients_options(cfg) == ("norm", 0.25, False)
    cfg = setup_cfg("", [KEY + "ENABLED", "True", KEY + "CLIP_TYPE", "norm", KEY + "CLIP_VALUE", "3", KEY + "NORM_TYPE", "inf"])
    assert cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE == math.inf and clip_gradients_options(cfg) == ("norm", 3.0, True)
    # the YAML file wins over the defaults, an override over the file
    cfg = setup_cfg(str(path), [KEY + "CLIP_VALUE", 0.125])
    assert clip_gradients_options(cfg) == ("value", 0.125, True)
    # a string that is no number is still a type error for a float key
    with pytest.raises(ValueError, match="Type mismatch"):
        setup_cfg("", [KEY + "CLIP_VALUE", "large"])


BAD = [("CLIP_TYPE", "full_model"), ("CLIP_VALUE", 0), ("NORM_TYPE", 1.0)]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_raise_only_when_enabled(key, value):
    with pytest.raises(ValueError, match="CLIP_GRADIENTS." + key):
        check_optimizer_options(setup_cfg("", [KEY + "ENABLED", True, KEY + key, value]))
    check_optimizer_options(setup_cfg("", [KEY + "ENABLED", False, KEY + key, value]))     # D2 does not look at them then
    check_optimizer_options(setup_cfg("", [KEY + key, value]))


def test_more_bad_values_and_the_untouched_rejections():
    for key, value in (("CLIP_VALUE", -1.0), ("NORM_TYPE", 0.0), ("NORM_TYPE", "-inf"), ("CLIP_TYPE", "")):
        with pytest.raises(ValueError, match="CLIP_GRADIENTS." + key):
            check_optimizer_options(setup_cfg("", [KEY + "ENABLED", True, KEY + key, value]))
    with pytest.raises(ValueError, match="NESTEROV"):
        check_optimizer_options(setup_cfg("", ["SOLVER.NESTEROV", True, KEY + "ENABLED", True]))


class _Net(nn.Module):
    """frozen and trainable parameters of 18, 64, 3*3*3*64 and 1 elements, declared in an order the flat layout reorders"""

    def __init__(self):
        super().__init__()
        self.frozen_w = nn.Parameter(torch.randn(64, 3, 3, 3), requires_grad=False)
        self.bias = nn.Parameter(torch.randn(64))
        self.weight = nn.Parameter(torch.randn(64, 3, 3, 3))
        self.frozen_b = nn.Parameter(torch.randn(64), requires_grad=False)
        self.scale = nn.Parameter(torch.randn(1))
        self.anchor_generator = nn.Module()
        self.anchor_generator.anchor_0 = nn.Parameter(torch.randn(9, 2))
        self.frozen_s = nn.Parameter(torch.randn(1), requires_grad=False)


def test_segment_table_of_a_small_module():
    fp = FlatParams(_Net())
    offs = segment_offsets(fp)
    sizes = [18, 64, 3 * 3 * 3 * 64, 1]
    assert fp.n_trainable == sum(sizes)
    assert offs[0] == 0 and offs[-1] == fp.n_trainable and len(offs) == len(sizes) + 1
    assert [b - a for a, b in zip(offs[:-1], offs[1:])] == sizes          # contiguous, in the order of FlatParams.index
    trainable = [n for n, p in fp.params.items() if p.requires_grad]
    assert trainable == ["anchor_generator.anchor_0", "bias", "weight", "scale"] == list(fp.index)[:4]
    assert [fp.index[n] for n in trainable] == [(a, b - a) for a, b in zip(offs[:-1], offs[1:])]
    # chunks: every segment cut on its own, ascending, nothing shared between two segments, everything covered once
    chunks, first = segment_chunks(offs, 512)
    assert first == [0, 1, 2, 6, 7] and len(chunks) == 7
    assert chunks == [(0, 0), (18, 1), (82, 2), (594, 2), (1106, 2), (1618, 2), (1810, 3)]
    covered = []
    for start, seg in chunks:
        covered.extend(range(start, min(start + 512, offs[seg + 1])))
    assert covered == list(range(fp.n_trainable))
    # an empty segment owns no chunk; a non-ascending table is refused
    assert segment_chunks([0, 4, 4, 9], 4) == ([(0, 0), (4, 2), (8, 2)], [0, 1, 1, 3])
    assert segment_chunks([0], 4) == ([], [0])
    with pytest.raises(ValueError):
        segment_chunks([0, 5, 3], 4)
