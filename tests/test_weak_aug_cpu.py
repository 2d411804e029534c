"""CPU: the host half of the weak augmentation -- the INPUT.CROP / MIN_SIZE_TRAIN_SAMPLING / RANDOM_FLIP config surface, the
crop and short-edge geometry (detectron2 0.5's RandomCrop / ResizeShortestEdge / RandomFlip written out), the box transform
crop -> resize -> flip -> clip -> filter, and the mapper's random stream."""
import random

import numpy as np
import pytest
import torch

from probabilisticteacher_amd.config import setup_cfg
from probabilisticteacher_amd.data import DeviceTwoCropMapper, crop_size, sample_crop, sample_short_edge, sample_strong_params
from probabilisticteacher_amd.data.augment import resize_shortest_edge_size
from probabilisticteacher_amd.data.mapper import weak_box_transform


def _cfg(*opts):
    return setup_cfg(opts=["MODEL.DEVICE", "cpu", *opts])


def test_config_keys_load_with_d2_defaults():
    c = _cfg()
    assert c.INPUT.CROP.ENABLED is False and c.INPUT.CROP.TYPE == "relative_range" and list(c.INPUT.CROP.SIZE) == [0.9, 0.9]
    assert c.INPUT.MIN_SIZE_TRAIN_SAMPLING == "choice"
    c = setup_cfg(opts=["INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "absolute", "INPUT.CROP.SIZE", "[512, 1024]"])
    assert c.INPUT.CROP.ENABLED is True and c.INPUT.CROP.TYPE == "absolute" and list(c.INPUT.CROP.SIZE) == [512, 1024]
    c = setup_cfg(opts=["INPUT.MIN_SIZE_TRAIN_SAMPLING", "range"])
    assert c.INPUT.MIN_SIZE_TRAIN_SAMPLING == "range"


def test_from_config_rejects_what_d2_rejects():
    with pytest.raises(ValueError):
        DeviceTwoCropMapper.from_config(_cfg("INPUT.RANDOM_FLIP", "diagonal"))
    with pytest.raises(ValueError):
        DeviceTwoCropMapper.from_config(_cfg("INPUT.MIN_SIZE_TRAIN_SAMPLING", "range", "INPUT.MIN_SIZE_TRAIN", "(480, 640, 800)"))
    with pytest.raises(ValueError):
        DeviceTwoCropMapper.from_config(_cfg("INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "diagonal_range"))
    with pytest.raises(ValueError):
        DeviceTwoCropMapper.from_config(_cfg("INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "absolute_range", "INPUT.CROP.SIZE", "[300, 200]"))
    # a disabled crop is not looked at, as in D2's build_augmentation
    assert DeviceTwoCropMapper.from_config(_cfg("INPUT.CROP.TYPE", "diagonal_range")).crop is None


def test_from_config_fills_flip_crop_and_sampling():
    m = DeviceTwoCropMapper.from_config(_cfg("INPUT.RANDOM_FLIP", "vertical"))
    assert m.flip == "vertical" and m.flip_mode == 2 and m.flip_prob == 0.5
    m = DeviceTwoCropMapper.from_config(_cfg("INPUT.RANDOM_FLIP", "none"))
    assert m.flip_mode == 0 and m.flip_prob == 0.0
    m = DeviceTwoCropMapper.from_config(_cfg())
    assert m.flip_mode == 1 and m.flip_prob == 0.5 and m.crop is None and m.min_size_sampling == "choice"
    m = DeviceTwoCropMapper.from_config(_cfg("INPUT.CROP.ENABLED", "True", "INPUT.MIN_SIZE_TRAIN_SAMPLING", "range",
                                             "INPUT.MIN_SIZE_TRAIN", "(480, 800)"))
    assert m.crop == ("relative_range", (0.9, 0.9)) and m.min_size_sampling == "range" and m.min_size_train == (480, 800)


def test_crop_size_hand_computed():
    # relative: int(x + 0.5)
    assert crop_size("relative", (0.5, 0.5), 101, 203) == (51, 102)            # 50.5 -> 51, 101.5 -> 102
    assert crop_size("relative", (0.3, 0.7), 10, 10) == (3, 7)
    assert crop_size("relative", (0.34, 0.35), 10, 10) == (3, 4)               # 3.4 -> 3, 3.5 -> 4
    assert crop_size("relative", (1.0, 1.0), 37, 41) == (37, 41)
    # relative_range: SIZE is held in float32
    h, w, u = 1024, 2048, (0.5, 0.25)
    s = np.float32(0.9)
    f = [float(s) + ui * float(np.float32(1) - s) for ui in u]
    want = (int(h * f[0] + 0.5), int(w * f[1] + 0.5))
    assert crop_size("relative_range", [0.9, 0.9], h, w, u) == want == (973, 1894)
    assert crop_size("relative_range", (0.9, 0.9), 1000, 1000, (0.0, 0.0)) == (900, 900)
    # float32(0.3) = 0.300000011920929: 0.3 * 10^8 + 0.5 would give 30000000, the float32 value gives 30000001
    assert crop_size("relative_range", (0.3, 0.3), 10 ** 8, 10, (0.0, 0.0)) == (int(10 ** 8 * float(np.float32(0.3)) + 0.5), 3) == (30000001, 3)
    # absolute: min(s, h) clamps
    assert crop_size("absolute", (512, 1024), 1024, 2048) == (512, 1024)
    assert crop_size("absolute", (512, 1024), 300, 2048) == (300, 1024)
    assert crop_size("absolute", (512, 1024), 600, 700) == (512, 700)
    # absolute_range: the drawn integers, inside [min(h, s0), min(h, s1)] x [min(w, s0), min(w, s1)]
    assert crop_size("absolute_range", (100, 200), 150, 400, (150, 200)) == (150, 200)
    assert crop_size("absolute_range", (100, 200), 150, 400, (100, 100)) == (100, 100)
    with pytest.raises(ValueError):
        crop_size("absolute_range", (100, 200), 150, 400, (151, 200))
    with pytest.raises(ValueError):
        crop_size("absolute_range", (200, 100), 150, 400, (100, 100))
    with pytest.raises(ValueError):
        crop_size("relative", (1.2, 1.0), 100, 100)
    with pytest.raises(ValueError):
        crop_size("relative_range", (1.2, 1.2), 100, 100, (0.5, 0.5))
    with pytest.raises(ValueError):
        crop_size("diagonal", (0.5, 0.5), 100, 100)


@pytest.mark.parametrize("ctype,size", [("relative", (0.75, 0.6)), ("relative_range", (0.9, 0.9)), ("absolute", (30, 45)),
                                        ("absolute_range", (10, 30))])
def test_sampled_crops_stay_inside_and_reach_both_ends(ctype, size):
    h, w = 40, 60
    rng = random.Random(2024)
    crops = [sample_crop(ctype, size, h, w, rng) for _ in range(10000)]
    for y0, x0, ch, cw in crops:
        assert 1 <= ch <= h and 1 <= cw <= w and 0 <= y0 <= h - ch and 0 <= x0 <= w - cw
    assert any(y0 == 0 for y0, _, _, _ in crops) and any(y0 == h - ch for y0, _, ch, _ in crops if ch < h)
    assert any(x0 == 0 for _, x0, _, _ in crops) and any(x0 == w - cw for _, x0, _, cw in crops if cw < w)
    chs, cws = {c[2] for c in crops}, {c[3] for c in crops}
    if ctype == "relative":
        assert chs == {30} and cws == {36}
    elif ctype == "relative_range":                       # f in [0.9, 1): int(40 f + 0.5) in 36 .. 40, int(60 f + 0.5) in 54 .. 60
        assert chs == set(range(36, 41)) and cws == set(range(54, 61))
    elif ctype == "absolute":
        assert chs == {30} and cws == {45}
    else:
        assert chs == set(range(10, 31)) and cws == set(range(10, 31))


def test_range_short_edge_sampling():
    rng = random.Random(5)
    got = [sample_short_edge((480, 800), "range", rng) for _ in range(10000)]
    assert min(got) == 480 and max(got) == 800 and all(isinstance(g, int) for g in got)
    assert {sample_short_edge((800, 480), "range", rng) for _ in range(10000)} <= set(range(480, 801))
    assert {sample_short_edge((480, 600, 800), "choice", rng) for _ in range(200)} == {480, 600, 800}
    with pytest.raises(ValueError):
        sample_short_edge((480, 600, 800), "range", rng)
    with pytest.raises(ValueError):
        sample_short_edge((480, 800), "nearest", rng)


def np_weak_boxes(boxes, crop, src_size, new_size, flip_mode, min_side=1e-5):
    """numpy restatement of D2's CropTransform -> ResizeTransform -> H/VFlipTransform -> clip -> filter_empty_instances in
    fp32 (tests/test_weak_aug_gpu.py uses it too)"""
    f32 = np.float32
    h, w = new_size
    b = np.asarray(boxes, dtype=f32).copy()
    sh, sw = src_size
    if crop is not None:
        y0, x0, sh, sw = crop
        b[:, 0::2] -= f32(x0)
        b[:, 1::2] -= f32(y0)
    b[:, 0::2] *= f32(w * 1.0 / sw)
    b[:, 1::2] *= f32(h * 1.0 / sh)
    if flip_mode == 1:
        b[:, 0], b[:, 2] = f32(w) - b[:, 2], f32(w) - b[:, 0]
    elif flip_mode == 2:
        b[:, 1], b[:, 3] = f32(h) - b[:, 3], f32(h) - b[:, 1]
    b[:, 0::2] = np.clip(b[:, 0::2], f32(0), f32(w))
    b[:, 1::2] = np.clip(b[:, 1::2], f32(0), f32(h))
    keep = ((b[:, 2] - b[:, 0]) > f32(min_side)) & ((b[:, 3] - b[:, 1]) > f32(min_side))
    return b, keep


BOXES = [[30.0, 20.0, 80.0, 60.0],        # inside the crop below
         [5.5, 3.25, 50.0, 40.0],         # straddles its top-left corner
         [90.0, 50.0, 140.0, 99.0],       # straddles its bottom-right corner
         [0.0, 0.0, 15.0, 9.0],           # outside (above / left)
         [125.0, 10.0, 150.0, 30.0],      # outside (right)
         [20.0, 12.0, 120.0, 75.0],       # exactly the crop
         [40.0, 30.0, 40.0, 50.0]]        # no width


@pytest.mark.parametrize("flip_mode", [0, 1, 2])
@pytest.mark.parametrize("crop,new_size", [((12, 20, 63, 100), (63, 100)), ((12, 20, 63, 100), (95, 151)), ((12, 20, 63, 100), (37, 59)),
                                           (None, (77, 123)), ((0, 0, 100, 160), (100, 160))])
def test_box_transform_equals_the_numpy_restatement(crop, new_size, flip_mode):
    src = (100, 160)
    got, keep = weak_box_transform(torch.tensor(BOXES), crop, src, new_size, flip_mode)
    want, wkeep = np_weak_boxes(BOXES, crop, src, new_size, flip_mode)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want), (got, want)
    assert keep.tolist() == wkeep.tolist()
    if crop == (12, 20, 63, 100):
        assert keep.tolist() == [True, True, True, False, False, True, False]
        if new_size == (63, 100):                 # (scaled, the crop's own box lands on the image within fp32 rounding only)
            assert np.array_equal(got.numpy()[5], np.array([0, 0, 100, 63], dtype=np.float32))


def test_seed_compatibility_without_crop():
    """crop disabled, "choice", "horizontal": the stream of the mapper before crops existed -- rng.choice per image, then
    rng.random() per image, then sample_strong_params per image"""
    shapes = [(96 + 8 * i, 128 - 4 * i) for i in range(8)]
    sizes_in = (64, 80, 96)
    mp = DeviceTwoCropMapper("cpu", seed=123, min_size_train=sizes_in, max_size_train=120)
    crops, sizes, flips, params = mp.draw(shapes)
    rng = random.Random(123)
    want_sizes = [resize_shortest_edge_size(h, w, rng.choice(sizes_in), 120) for h, w in shapes]
    want_flips = [rng.random() < 0.5 for _ in shapes]
    want_params = [sample_strong_params(rng) for _ in shapes]
    assert crops == [None] * 8 and sizes == want_sizes and flips == want_flips and params == want_params
    assert mp.rng.random() == rng.random()                                     # and nothing more was consumed
    # no MIN_SIZE_TRAIN: no size draw at all
    mp, rng = DeviceTwoCropMapper("cpu", seed=123), random.Random(123)
    _, sizes, flips, params = mp.draw(shapes)
    assert sizes == shapes and flips == [rng.random() < 0.5 for _ in shapes] and params == [sample_strong_params(rng) for _ in shapes]


def test_draw_order_with_crop():
    """per image: u0, u1, y0, x0, then the short edge; then the flips; then the strong parameters"""
    shapes = [(100, 160), (90, 70)]
    mp = DeviceTwoCropMapper("cpu", seed=9, min_size_train=(48, 64), max_size_train=100, crop=("relative_range", (0.5, 0.5)),
                             flip="vertical", min_size_sampling="range")
    crops, sizes, flips, params = mp.draw(shapes)
    rng = random.Random(9)
    for (h, w), crop, size in zip(shapes, crops, sizes):
        u = (rng.random(), rng.random())
        ch, cw = crop_size("relative_range", (0.5, 0.5), h, w, u)
        y0 = rng.randint(0, h - ch)
        x0 = rng.randint(0, w - cw)
        assert crop == (y0, x0, ch, cw)
        assert size == resize_shortest_edge_size(ch, cw, rng.randint(48, 64), 100)
    assert flips == [rng.random() < 0.5 for _ in shapes] and params == [sample_strong_params(rng) for _ in shapes]
    # explicit crops are not drawn
    mp2 = DeviceTwoCropMapper("cpu", seed=9, crop=("absolute", (10, 10)))
    rng = random.Random(9)
    c2, s2, f2, _ = mp2.draw(shapes, crops=[(1, 2, 30, 40), None])
    assert c2 == [(1, 2, 30, 40), None] and s2 == [(30, 40), (90, 70)] and f2 == [rng.random() < 0.5 for _ in shapes]
