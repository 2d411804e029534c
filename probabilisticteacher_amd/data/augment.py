"""Strong augmentation of the two-crop mapper ON THE DEVICE.

Reference: pt/data/detection_utils.py:38-60 `build_strong_augmentation`
    RandomApply([ColorJitter(0.4, 0.4, 0.4, 0.1)], p=0.8); RandomGrayscale(p=0.2);
    RandomApply([GaussianBlur([0.1, 2.0])], p=0.5); RandomApply([Solarize(threshold=0.5)], p=0.2)
run per image on a PIL copy inside DataLoader workers (pt/data/dataset_mapper.py:151-159).  At ~45 img/s per GPU x 2
strong crops that is ~100 PIL pipelines per second per GPU; here the whole batch of a step is augmented by a handful of
HBM-bound launches (csrc/augment.hip), byte-exact with Pillow for given parameters.

The random PARAMETERS are drawn on the host (`sample_strong_params`, same distributions as torchvision 0.8.2 /
augmentation_impl.py); the pixels never leave the device."""
import math
import random
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..ops import _chk, _image_desc, _ptr, _stream

OP_COPY, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_GRAY, OP_SOLARIZE = range(7)


@dataclass
class StrongParams:
    """one image's draw: `jitter` = the ColorJitter ops in application order [(op, factor), ...] (empty: not applied)"""
    jitter: List[Tuple[int, float]] = field(default_factory=list)
    gray: bool = False
    blur_sigma: Optional[float] = None
    solarize: Optional[int] = None          # threshold (round(0.5 * 256) = 128 in the reference) or None


def sample_strong_params(rng: random.Random) -> StrongParams:
    """Same distributions as the reference's pipeline (torchvision 0.8.2 ColorJitter.get_params: uniform factors in
    [max(0, 1 - v), 1 + v], hue in [-0.1, 0.1], shuffled order; RandomApply / RandomGrayscale coin flips;
    augmentation_impl.py:36 sigma ~ U(0.1, 2.0); :43 threshold = round(0.5 * 256))."""
    p = StrongParams()
    if rng.random() < 0.8:
        ops = [(OP_BRIGHTNESS, rng.uniform(0.6, 1.4)), (OP_CONTRAST, rng.uniform(0.6, 1.4)),
               (OP_SATURATION, rng.uniform(0.6, 1.4)), (OP_HUE, rng.uniform(-0.1, 0.1))]
        rng.shuffle(ops)
        p.jitter = ops
    p.gray = rng.random() < 0.2
    if rng.random() < 0.5:
        p.blur_sigma = rng.uniform(0.1, 2.0)
    if rng.random() < 0.2:
        p.solarize = round(0.5 * 256)
    return p


def _f32_bits(x: float) -> int:
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


def hue_shift(hue_factor: float) -> int:
    """`np.uint8(hue_factor * 255)` (torchvision adjust_hue): C float -> uint8 conversion, truncation then modulo 256"""
    return int(hue_factor * 255) & 0xFF


def box_blur_weights(sigma: float) -> Tuple[int, int, int]:
    """ImageFilter.GaussianBlur(radius=sigma) -> Pillow's ImagingGaussianBlur (3 box passes): integer box radius and the
    24-bit fixed-point weights ww (inner taps) / fw (the two fractional end taps), evaluated in fp32 / fp64 as BoxBlur.c does."""
    import numpy as np
    f32 = np.float32
    passes = 3
    sigma2 = f32(f32(f32(sigma) * f32(sigma)) / f32(passes))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    fr = f32(l + f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1)))))))
    radius = int(fr)
    ww = int(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1)))
    fw = ((1 << 24) - (radius * 2 + 1) * ww) // 2
    return radius, ww, fw


def _launch(name: str, rows, dev, max_elems: int, *extra):
    desc = _image_desc(rows, dev)
    _lib.call(name, _ptr(desc), len(rows), int(max_elems), *extra, _stream())


def strong_augment_batch(images: Sequence[torch.Tensor], params: Sequence[StrongParams]) -> List[torch.Tensor]:
    """images: uint8 (3, H, W) device tensors (channel order as in the record; PIL is told "RGB", dataset_mapper.py:155).
    Returns new tensors; the inputs are not modified.  Launches per BATCH: <= 4 colour rounds (+ a grey-level sum before a
    round in which some image applies contrast), grayscale, 6 box-blur passes, solarize."""
    n = len(images)
    if n == 0:
        return []
    dev = images[0].device
    cur = [_chk(im.contiguous(), torch.uint8, "image").clone() for im in images]        # colour ops run in place on the copy
    hw = [int(im.shape[-2] * im.shape[-1]) for im in cur]
    sums = torch.zeros(n, dtype=torch.int64, device=dev)

    def color_round(items):
        """items: [(image index, op, float factor, int parameter)]"""
        if not items:
            return
        if any(op == OP_CONTRAST for _, op, _, _ in items):
            rows = [[cur[i].data_ptr(), 0, cur[i].shape[-2], cur[i].shape[-1], 0, 0, 0, 0] for i, _, _, _ in items]
            desc = _image_desc(rows, dev)
            part = torch.empty(len(items), dtype=torch.int64, device=dev)
            _lib.call("ptmi_aug_gray_sum_batched", _ptr(desc), len(rows), max(hw[i] for i, _, _, _ in items), _ptr(part), _stream())
        else:
            part = sums
        rows = [[cur[i].data_ptr(), cur[i].data_ptr(), cur[i].shape[-2], cur[i].shape[-1], op, _f32_bits(f), ip, 0]
                for i, op, f, ip in items]
        _launch("ptmi_aug_color_batched", rows, dev, max(hw[i] for i, _, _, _ in items), _ptr(part))

    for k in range(4):
        items = []
        for i, p in enumerate(params):
            if len(p.jitter) > k:
                op, f = p.jitter[k]
                items.append((i, op, f if op != OP_HUE else 0.0, hue_shift(f) if op == OP_HUE else 0))
        color_round(items)
    color_round([(i, OP_GRAY, 0.0, 0) for i, p in enumerate(params) if p.gray])
    blur = [i for i, p in enumerate(params) if p.blur_sigma is not None]
    if blur:
        tmp = {i: torch.empty_like(cur[i]) for i in blur}
        dst = {i: torch.empty_like(cur[i]) for i in blur}
        wts = {i: box_blur_weights(params[i].blur_sigma) for i in blur}
        seq = [(cur, tmp), (tmp, dst), (dst, tmp), (tmp, dst), (dst, tmp), (tmp, dst)]       # H H H V V V, ends in dst
        for ps, (a, b) in enumerate(seq):
            rows = [[a[i].data_ptr(), b[i].data_ptr(), cur[i].shape[-2], cur[i].shape[-1], int(ps >= 3), *wts[i]] for i in blur]
            _launch("ptmi_aug_box_blur_batched", rows, dev, max(3 * hw[i] for i in blur))
        for i in blur:
            cur[i] = dst[i]
    color_round([(i, OP_SOLARIZE, 0.0, int(p.solarize)) for i, p in enumerate(params) if p.solarize is not None])
    return cur


def hflip_batch(images: Sequence[torch.Tensor], flips: Sequence[bool]) -> List[torch.Tensor]:
    """D2 RandomFlip(horizontal) -> HFlipTransform on planar uint8 images; one launch for the batch."""
    if not images:
        return []
    dev = images[0].device
    images = [_chk(im.contiguous(), torch.uint8, "image") for im in images]
    out = [torch.empty_like(im) for im in images]
    rows = [[im.data_ptr(), o.data_ptr(), im.shape[-2], im.shape[-1], int(bool(f)), 0, 0, 0] for im, o, f in zip(images, out, flips)]
    _launch("ptmi_aug_hflip_batched", rows, dev, max(im.numel() for im in images))
    return out


def unpack_hwc_batch(srcs: Sequence[torch.Tensor], bgr: bool) -> List[torch.Tensor]:
    """Decoded images as Pillow delivers them -- packed uint8 (H, W, 3) RGB device tensors, starting at any byte address -- to
    the planar (3, H, W) record format: `arr[:, :, ::-1].transpose(2, 0, 1)` of `datasets.read_image` (bgr) or the
    channel-preserving `arr.transpose(2, 0, 1)`.  One launch for the batch, whatever the image sizes."""
    if not srcs:
        return []
    dev = srcs[0].device
    for im in srcs:
        _chk(im, torch.uint8, "image")
        if im.dim() != 3 or im.shape[2] != 3 or im.numel() == 0:
            raise ValueError(f"unpack_hwc_batch: expected a non-empty (H, W, 3) image, got {tuple(im.shape)}")
    out = [torch.empty((3, im.shape[0], im.shape[1]), dtype=torch.uint8, device=dev) for im in srcs]
    rows = [[im.data_ptr(), o.data_ptr(), im.shape[0], im.shape[1], int(bool(bgr)), 0, 0, 0] for im, o in zip(srcs, out)]
    _launch("ptmi_aug_unpack_hwc_batched", rows, dev, max(im.shape[0] * im.shape[1] for im in srcs))
    return out


def resize_shortest_edge_size(h: int, w: int, short_edge: int, max_size: int) -> Tuple[int, int]:
    """D2 ResizeShortestEdge.get_transform: scale the short side to `short_edge`, cap the long side at `max_size`, round
    half up.  Returns (new_h, new_w)."""
    scale = short_edge * 1.0 / min(h, w)
    newh, neww = (short_edge, scale * w) if h < w else (scale * h, short_edge)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


CROP_TYPES = ("relative_range", "relative", "absolute", "absolute_range")
FLIP_MODES = {"none": 0, "horizontal": 1, "vertical": 2}          # p8 of ptmi_aug_flip_window_batched
Window = Tuple[int, int, int, int]                                 # (y0, x0, ch, cw)


def _f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def crop_size(crop_type: str, size: Sequence[float], h: int, w: int, u: Optional[Sequence[float]] = None) -> Tuple[int, int]:
    """D2 0.5 RandomCrop.get_crop_size for an (h, w) image -> (ch, cw).  `size` = INPUT.CROP.SIZE.
    "relative": fractions of the image, rounded half up.  "relative_range": `u` = two uniform draws in [0, 1); D2 holds SIZE
    as a float32 array, so f_i = float32(s_i) + u_i * (float32(1) - float32(s_i)) evaluated in double, then as "relative".
    "absolute": (s0, s1) clamped to the image.  "absolute_range": `u` = the two integers drawn from
    [min(h, s0), min(h, s1)] and [min(w, s0), min(w, s1)] (both ends inclusive; `crop_size_range`).
    D2 asserts that the crop fits the image: a result larger than the image (relative sizes above 1) is a ValueError."""
    s0, s1 = size
    if crop_type == "relative":
        ch, cw = int(h * s0 + 0.5), int(w * s1 + 0.5)
    elif crop_type == "relative_range":
        f0, f1 = (_f32(s) + float(ui) * _f32(1.0 - _f32(s)) for s, ui in zip((s0, s1), u))
        ch, cw = int(h * f0 + 0.5), int(w * f1 + 0.5)
    elif crop_type == "absolute":
        ch, cw = min(int(s0), h), min(int(s1), w)
    elif crop_type == "absolute_range":
        (hlo, hhi), (wlo, whi) = crop_size_range(size, h, w)
        ch, cw = int(u[0]), int(u[1])
        if not (hlo <= ch <= hhi and wlo <= cw <= whi):
            raise ValueError(f"absolute_range crop {ch}x{cw} outside [{hlo}, {hhi}] x [{wlo}, {whi}]")
    else:
        raise ValueError(f"Unknown crop type {crop_type!r} (INPUT.CROP.TYPE is one of {CROP_TYPES})")
    if ch > h or cw > w or ch < 1 or cw < 1:
        raise ValueError(f"{crop_type} crop {tuple(size)} of a {h}x{w} image gives {ch}x{cw}: the crop must fit the image")
    return ch, cw


def crop_size_range(size: Sequence[float], h: int, w: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """the inclusive integer ranges "absolute_range" draws ch and cw from"""
    s0, s1 = int(size[0]), int(size[1])
    if s0 > s1:
        raise ValueError(f"absolute_range crop needs SIZE[0] <= SIZE[1], got {tuple(size)}")
    return (min(h, s0), min(h, s1)), (min(w, s0), min(w, s1))


def sample_crop(crop_type: str, size: Sequence[float], h: int, w: int, rng: random.Random) -> Window:
    """D2 RandomCrop.get_transform -> (y0, x0, ch, cw).  Draw order: u0, u1 ("relative_range") or the two integers
    ("absolute_range"; the other types draw nothing), then y0 in [0, h - ch], then x0 in [0, w - cw]."""
    u = None
    if crop_type == "relative_range":
        u = (rng.random(), rng.random())
    elif crop_type == "absolute_range":
        hr, wr = crop_size_range(size, h, w)
        u = (rng.randint(*hr), rng.randint(*wr))
    ch, cw = crop_size(crop_type, size, h, w, u)
    y0 = rng.randint(0, h - ch)
    x0 = rng.randint(0, w - cw)
    return y0, x0, ch, cw


def sample_short_edge(min_size_train: Sequence[int], sampling: str, rng: random.Random) -> int:
    """D2 ResizeShortestEdge: "choice" picks one of the sizes, "range" a uniform integer in [min, max], both ends included"""
    if sampling == "choice":
        return rng.choice(min_size_train)
    if sampling == "range":
        if len(min_size_train) != 2:
            raise ValueError(f"INPUT.MIN_SIZE_TRAIN_SAMPLING 'range' needs exactly two sizes, got {tuple(min_size_train)}")
        return rng.randint(min(min_size_train), max(min_size_train))
    raise ValueError(f"Unknown INPUT.MIN_SIZE_TRAIN_SAMPLING {sampling!r} ('choice' or 'range')")


def _window_row(im: torch.Tensor, window: Optional[Window], dst: torch.Tensor, p8: int, p9: int) -> List[int]:
    """one 16-word descriptor row of the windowed kernels; the kernels trust it, so the window is checked here"""
    h, w = im.shape[-2:]
    y0, x0, ch, cw = (0, 0, h, w) if window is None else (int(v) for v in window)
    if not (0 <= y0 and 0 <= x0 and ch >= 1 and cw >= 1 and y0 + ch <= h and x0 + cw <= w):
        raise ValueError(f"window (y0, x0, ch, cw) = {(y0, x0, ch, cw)} is not inside the {h}x{w} image")
    return [im.data_ptr(), dst.data_ptr(), w, h * w, x0, y0, ch, cw, p8, p9, 0, 0, 0, 0, 0, 0]


def flip_batch(images: Sequence[torch.Tensor], modes: Sequence[int],
               windows: Optional[Sequence[Optional[Window]]] = None) -> List[torch.Tensor]:
    """Copy (mode 0), D2 HFlipTransform (1) or VFlipTransform (2) of planar uint8 images, or of a window (y0, x0, ch, cw) of
    each: a crop that needs no resize is taken here, by the launch that flips / copies anyway.  One launch for the batch."""
    if not images:
        return []
    dev = images[0].device
    images = [_chk(im.contiguous(), torch.uint8, "image") for im in images]
    windows = list(windows) if windows is not None else [None] * len(images)
    rows, out = [], []
    for im, m, win in zip(images, modes, windows):
        if int(m) not in (0, 1, 2):
            raise ValueError(f"flip mode {m}: 0 copy, 1 left-right, 2 top-bottom")
        o = torch.empty((3,) + (tuple(im.shape[-2:]) if win is None else (int(win[2]), int(win[3]))), dtype=torch.uint8, device=dev)
        rows.append(_window_row(im, win, o, int(m), 0))
        out.append(o)
    _launch("ptmi_aug_flip_window_batched", rows, dev, max(o.numel() for o in out))
    return out


def resize_batch(images: Sequence[torch.Tensor], sizes: Sequence[Tuple[int, int]],
                 windows: Optional[Sequence[Optional[Window]]] = None) -> List[torch.Tensor]:
    """Image.resize((new_w, new_h), Image.BILINEAR) of D2's ResizeTransform for a batch of planar uint8 images: the x pass
    of all images in one launch, then the y pass (a pass that does not change the size is skipped, as in Pillow).
    windows[i] = (y0, x0, ch, cw): image i is the resize of that crop of images[i] (D2 RandomCrop before the resize).  The
    crop is not copied out: the first pass that runs for the image reads the window in place, with the filter clamped to it."""
    if not images:
        return []
    if windows is not None and any(win is not None for win in windows):
        return _resize_windows(images, sizes, list(windows))
    dev = images[0].device
    cur = [_chk(im.contiguous(), torch.uint8, "image") for im in images]
    for vertical in (0, 1):
        rows, outs, idx = [], [], []
        for i, (im, (nh, nw)) in enumerate(zip(cur, sizes)):
            h, w = im.shape[-2:]
            new = nh if vertical else nw
            if new == (h if vertical else w):
                continue
            if math.ceil(max((h if vertical else w) / new, 1.0)) * 2 + 1 > 32:
                raise ValueError(f"resize {h}x{w} -> {nh}x{nw}: down-scaling factor beyond the kernel's 32-tap window")
            o = torch.empty((3, new, w) if vertical else (3, h, new), dtype=torch.uint8, device=dev)
            rows.append([im.data_ptr(), o.data_ptr(), h, w, new, vertical, 0, 0])
            outs.append(o)
            idx.append(i)
        if rows:
            _launch("ptmi_aug_resize_pass_batched", rows, dev, max(o.numel() for o in outs))
            for i, o in zip(idx, outs):
                cur[i] = o
    return cur


def _resize_windows(images, sizes, windows) -> List[torch.Tensor]:
    """resize_batch with at least one window: every pass is one launch of the windowed kernel for the whole batch (an image
    without a window, and the dense intermediate of a second pass, is the window that covers all of it)."""
    dev = images[0].device
    cur = [_chk(im.contiguous(), torch.uint8, "image") for im in images]
    win = list(windows)
    for vertical in (0, 1):
        rows, outs, idx = [], [], []
        for i, (im, (nh, nw)) in enumerate(zip(cur, sizes)):
            h, w = im.shape[-2:] if win[i] is None else (int(win[i][2]), int(win[i][3]))
            new = nh if vertical else nw
            if new == (h if vertical else w):
                continue
            if math.ceil(max((h if vertical else w) / new, 1.0)) * 2 + 1 > 32:
                raise ValueError(f"resize {h}x{w} -> {nh}x{nw}: down-scaling factor beyond the kernel's 32-tap window")
            o = torch.empty((3, new, w) if vertical else (3, h, new), dtype=torch.uint8, device=dev)
            rows.append(_window_row(im, win[i], o, new, vertical))
            outs.append(o)
            idx.append(i)
        if rows:
            _launch("ptmi_aug_resize_window_pass_batched", rows, dev, max(o.numel() for o in outs))
            for i, o in zip(idx, outs):
                cur[i], win[i] = o, None
    left = [i for i, wn in enumerate(win) if wn is not None]         # a window that already has its target size: copy it out
    if left:
        for i, o in zip(left, flip_batch([cur[i] for i in left], [0] * len(left), [win[i] for i in left])):
            cur[i] = o
    return cur
