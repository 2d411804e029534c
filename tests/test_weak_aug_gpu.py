"""GPU (pytest -m gpu): the windowed resize / flip kernels of csrc/augment.hip (INPUT.CROP without a cropped copy, vertical
flip) against Pillow and numpy, and the two-crop mapper with crop, range size sampling and both flip directions.
Every pixel comparison is BIT-EXACT."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_host_logic import _write_voc_dir
from tests.test_weak_aug_cpu import np_weak_boxes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _eq(a, b, what):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    assert bool((a == b).all()), f"{what}: {int((a != b).sum())} of {a.numel()} bytes differ"


def _img(rs, h, w, smooth=False):
    x = rs.randint(0, 256, (3, h, w))
    if smooth:
        x = np.cumsum(rs.randint(-3, 4, (3, h, w)), axis=2) % 256
    return torch.from_numpy(x.astype(np.uint8))


def pil_crop_resize(img, win, nh, nw):
    """Image.fromarray(img[y0:y0+ch, x0:x0+cw]).resize((nw, nh), Image.BILINEAR) per plane (Pillow resamples bands independently)"""
    a = img.numpy()
    if win is not None:
        y0, x0, ch, cw = win
        a = a[:, y0:y0 + ch, x0:x0 + cw]
    return torch.from_numpy(np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(p)).resize((nw, nh), Image.BILINEAR)) for p in a]))


def test_pil_helper_is_the_rgb_resize():
    """the per-plane helper above is what Pillow does to an RGB image"""
    rs = np.random.RandomState(0)
    im = _img(rs, 37, 53)
    hwc = np.ascontiguousarray(im.numpy().transpose(1, 2, 0))
    want = np.asarray(Image.fromarray(hwc[5:30, 7:47]).resize((61, 17), Image.BILINEAR)).transpose(2, 0, 1)
    assert np.array_equal(pil_crop_resize(im, (5, 7, 25, 40), 17, 61).numpy(), want)


def test_windowed_resize_matches_pillow_on_the_crop():
    from probabilisticteacher_amd.data import resize_batch
    rs = np.random.RandomState(21)
    a, b, big = _img(rs, 97, 131), _img(rs, 64, 80, smooth=True), _img(rs, 1024, 2048, smooth=True)
    cases = [  # (image, (y0, x0, ch, cw), (nh, nw))
        (a, (0, 0, 50, 70), (31, 43)),            # top-left corner, down-scale, both passes
        (a, (0, 61, 50, 70), (80, 111)),          # top-right corner, up-scale, odd origin
        (a, (47, 0, 50, 70), (50, 35)),           # bottom-left, x pass only
        (a, (47, 61, 50, 70), (25, 70)),          # bottom-right, y pass only
        (a, (13, 17, 41, 53), (29, 37)),          # interior, odd origin and odd width (the byte path)
        (a, (13, 18, 41, 53), (67, 90)),          # even origin, odd width
        (a, (1, 3, 95, 127), (95, 127)),          # the crop already has its size: copied out
        (a, (0, 0, 97, 131), (60, 81)),           # the whole image
        (b, (8, 16, 40, 48), (20, 24)),           # everything a multiple of four (the dword path)
        (b, (8, 16, 40, 48), (57, 48)),           # y pass only, aligned
        (b, None, (32, 40)),                      # an image without a window in a windowed batch
        (big, (51, 103, 922, 1843), (600, 1199)),  # Cityscapes -> relative crop -> short edge 600
        (big, (0, 0, 1024, 2048), (600, 1200)),
    ]
    outs = resize_batch([im.to(DEV) for im, _, _ in cases], [sz for _, _, sz in cases], [wn for _, wn, _ in cases])
    for (im, wn, (nh, nw)), o in zip(cases, outs):
        _eq(o, pil_crop_resize(im, wn, nh, nw), f"resize {tuple(im.shape)} window {wn} -> {(nh, nw)}")
    # a window equal to the whole image is the resize without windows
    plain = resize_batch([a.to(DEV), big.to(DEV)], [(60, 81), (600, 1200)])
    _eq(outs[7], plain[0], "whole-image window vs no window")
    _eq(outs[12], plain[1], "whole-image window vs no window (2048 x 1024)")
    with pytest.raises(ValueError):
        resize_batch([a.to(DEV)], [(30, 40)], [(0, 100, 50, 70)])              # window leaves the image
    with pytest.raises(ValueError):
        resize_batch([big.to(DEV)], [(20, 40)], [(0, 0, 1000, 2000)])          # beyond the 32-tap window


def test_flip_batch_modes_and_windows():
    from probabilisticteacher_amd.data import flip_batch, hflip_batch
    rs = np.random.RandomState(22)
    a, b, c = _img(rs, 40, 67), _img(rs, 32, 64), _img(rs, 5, 3)
    dense = [(a, 0), (a, 1), (a, 2), (b, 0), (b, 1), (b, 2), (c, 1), (c, 2)]
    outs = flip_batch([im.to(DEV) for im, _ in dense], [m for _, m in dense])
    for (im, m), o in zip(dense, outs):
        _eq(o, im if m == 0 else im.flip(-1) if m == 1 else im.flip(-2), f"flip mode {m} of {tuple(im.shape)}")
    _eq(outs[1], hflip_batch([a.to(DEV)], [True])[0], "mode 1 vs hflip_batch")
    _eq(outs[4], hflip_batch([b.to(DEV)], [True])[0], "mode 1 vs hflip_batch (aligned)")
    wins = [(a, (3, 5, 30, 41)), (a, (0, 0, 40, 67)), (a, (10, 64, 30, 3)), (b, (4, 8, 16, 32)), (b, (1, 2, 31, 62)), (a, (39, 0, 1, 67))]
    for m in (0, 1, 2):
        outs = flip_batch([im.to(DEV) for im, _ in wins], [m] * len(wins), [wn for _, wn in wins])
        for (im, (y0, x0, ch, cw)), o in zip(wins, outs):
            crop = im[:, y0:y0 + ch, x0:x0 + cw]
            _eq(o, crop if m == 0 else crop.flip(-1) if m == 1 else crop.flip(-2), f"flip mode {m} of window {(y0, x0, ch, cw)}")
    with pytest.raises(ValueError):
        flip_batch([a.to(DEV)], [3])
    with pytest.raises(ValueError):
        flip_batch([a.to(DEV)], [0], [(0, 0, 41, 67)])


def test_filter_support_is_clamped_to_the_window():
    """the crop is a constant 100 in an image of 255: a tap outside the window would show in the output"""
    from probabilisticteacher_amd.data import resize_batch
    cases = []
    for (y0, x0, ch, cw), size in [((7, 9, 40, 52), (17, 23)), ((7, 9, 40, 52), (90, 111)), ((8, 12, 40, 52), (13, 52)),
                                   ((1, 1, 30, 31), (30, 11)), ((20, 30, 44, 66), (5, 7))]:
        im = torch.full((3, 64, 96), 255, dtype=torch.uint8)
        im[:, y0:y0 + ch, x0:x0 + cw] = 100
        cases.append((im, (y0, x0, ch, cw), size))
    outs = resize_batch([im.to(DEV) for im, _, _ in cases], [sz for _, _, sz in cases], [wn for _, wn, _ in cases])
    for (_, wn, size), o in zip(cases, outs):
        assert tuple(o.shape) == (3,) + size
        assert bool((o == 100).all()), f"window {wn} -> {size}: {int((o != 100).sum())} bytes are not 100"


def test_mapper_crop_resize_flip_end_to_end():
    from probabilisticteacher_amd.data import DeviceTwoCropMapper, StrongParams, strong_augment_batch
    rs = np.random.RandomState(23)
    imgs = [_img(rs, 100, 160, smooth=True), _img(rs, 90, 70), _img(rs, 64, 96, smooth=True), _img(rs, 50, 60)]
    boxes = torch.tensor([[30.0, 20.0, 80.0, 60.0], [5.5, 3.25, 50.0, 40.0], [0.0, 0.0, 15.0, 9.0], [40.0, 30.0, 40.0, 50.0], [2.0, 1.0, 69.0, 89.0]])
    classes = torch.tensor([1, 2, 3, 4, 5])
    dd = [{"image": im, "boxes": boxes.clone(), "classes": classes.clone(), "file_name": f"{i}.png"} for i, im in enumerate(imgs)]
    crops = [(12, 20, 63, 100), (10, 5, 70, 51), None, (3, 7, 40, 44)]
    sizes = [(76, 120), (70, 51), (48, 72), (40, 44)]      # resized; the crop has its size already; no crop; ditto, not flipped
    flips = [True, True, False, False]
    params = [StrongParams(solarize=128), StrongParams(gray=True), StrongParams(blur_sigma=1.1), StrongParams()]
    for direction, transpose in (("vertical", Image.FLIP_TOP_BOTTOM), ("horizontal", Image.FLIP_LEFT_RIGHT), ("none", None)):
        mp = DeviceTwoCropMapper(DEV, seed=3, flip=direction)
        pairs = mp(dd, params=params, flips=flips, sizes=sizes, crops=crops)
        weak_ref = []
        for im, wn, (nh, nw), f in zip(imgs, crops, sizes, flips):
            y0, x0, ch, cw = wn if wn is not None else (0, 0) + tuple(im.shape[-2:])
            pil = Image.fromarray(np.ascontiguousarray(im.numpy().transpose(1, 2, 0)[y0:y0 + ch, x0:x0 + cw]))     # crop
            pil = pil.resize((nw, nh), Image.BILINEAR)                                                             # resize
            if f and transpose is not None:
                pil = pil.transpose(transpose)                                                                     # flip
            weak_ref.append(torch.from_numpy(np.ascontiguousarray(np.asarray(pil).transpose(2, 0, 1))))
        strong_ref = strong_augment_batch([w.to(DEV) for w in weak_ref], params)
        for i, ((s, w), wr, sr) in enumerate(zip(pairs, weak_ref, strong_ref)):
            _eq(w["image"], wr, f"{direction}: weak image {i}")
            _eq(s["image"], sr, f"{direction}: strong image {i}")
            assert (s["height"], s["width"]) == (w["height"], w["width"]) == tuple(wr.shape[-2:]) == sizes[i]
            assert s["instances"].image_size == sizes[i] and s["file_name"] == f"{i}.png"
            mode = {"vertical": 2, "horizontal": 1, "none": 0}[direction] if flips[i] else 0
            want, keep = np_weak_boxes(boxes.numpy(), crops[i], tuple(imgs[i].shape[-2:]), sizes[i], mode)
            assert np.array_equal(s["instances"].gt_boxes.tensor.cpu().numpy(), want[keep]), f"{direction}: boxes of image {i}"
            assert s["instances"].gt_classes.cpu().tolist() == classes.numpy()[keep].tolist()
            assert w["instances"].gt_boxes.tensor.shape == s["instances"].gt_boxes.tensor.shape


def test_train_loader_with_crop_and_range_sampling(tmp_path):
    from probabilisticteacher_amd.config import setup_cfg
    from probabilisticteacher_amd.data import build_detection_semisup_train_loader_two_crops, datasets
    rng = np.random.RandomState(24)
    names = ("car", "person")
    for sub, n in (("label", 5), ("unlabel", 5)):
        _write_voc_dir(str(tmp_path / sub), [f"{sub}{i}" for i in range(n)], names, rng, h=96, w=128)
        datasets.register_pascal_voc("weakaug_" + sub, str(tmp_path / sub), "train", names)
    cfg = setup_cfg(opts=["MODEL.DEVICE", DEV, "SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2,
                          "DATASETS.TRAIN_LABEL", ("weakaug_label",), "DATASETS.TRAIN_UNLABEL", ("weakaug_unlabel",),
                          "INPUT.MIN_SIZE_TRAIN", (60, 90), "INPUT.MAX_SIZE_TRAIN", 110, "INPUT.MIN_SIZE_TRAIN_SAMPLING", "range",
                          "INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "relative_range", "INPUT.CROP.SIZE", [0.6, 0.7],
                          "INPUT.RANDOM_FLIP", "vertical"])
    loader = build_detection_semisup_train_loader_two_crops(cfg, seed=5)
    seen = set()
    for _ in range(3):
        ls, lw, us, uw = next(loader)
        assert len(ls) == len(lw) == len(us) == len(uw) == 2
        for s, w in zip(ls + us, lw + uw):
            assert s["image"].shape == w["image"].shape == (3, s["height"], s["width"]) and s["image"].dtype == torch.uint8
            assert (s["height"], s["width"]) == (w["height"], w["width"])
            h, wd = s["height"], s["width"]
            assert max(h, wd) <= 110 and (60 <= min(h, wd) <= 90 or max(h, wd) == 110)
            seen.add((h, wd))
        for s in ls:
            b = s["instances"].gt_boxes.tensor.cpu()
            assert s["instances"].image_size == (s["height"], s["width"])
            assert bool((b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= s["width"]).all() and (b[:, 3] <= s["height"]).all())
            assert bool(((b[:, 2] - b[:, 0]) > 0).all() and ((b[:, 3] - b[:, 1]) > 0).all())
        assert all("instances" not in u for u in us)
    assert len(seen) > 1, "range sampling and random crops give more than one image size"
