"""CPU: the skip geometry of csrc/frame_skip.h (through its host-only C ABI) against a brute-force NumPy reference.

The reference knows nothing of rectangles: it keeps, per image, a boolean mask "this input pixel holds the pattern", erodes it by
3x3 for every convolution by a direct kernel (outside the image counts as unknown: the zero padding is not the pattern), keeps
only the whole pure tiles behind a convolution by the F(4x4, 3x3) kernels (a tile's roundoff depends on its whole window), pools
it by 2x2 (all four known), and calls a 4x4 tile pure iff its whole 6x6 window is inside the image and known.  A pixel tile (64
flat columns x 8 rows of the concatenated strips) may be skipped iff all of its 32 tiles are pure.

Zero tolerance: nothing the reference calls impure may ever be skipped.  For chains of convolutions the rectangles are exact, so
the skipped set must EQUAL the reference's; behind a pool the header may only be more careful.

So that the test cannot pass trivially, the reference itself must yield, for every shape, pixel tiles of three classes:
  whole     -- a pixel tile inside ONE strip, all 32 tiles pure (it is skipped);
  partial   -- a pixel tile inside one strip with some, not all, tiles pure (it must be kept);
  straddle  -- a pixel tile that spans two strips and holds pure tiles (it must be kept: every strip ends in a tile that touches
               columns >= W and starts with one whose window leaves the image, so such a pixel tile is never pure as a whole).
"""
import ctypes

import numpy as np
import pytest

from probabilisticteacher_amd import _lib, build_ext

SHAPES = [(40, 150), (24, 333), (50, 83)]
# the middle image's pasted rectangle (x0, y0, x1, y1): odd offsets, placed so that the three classes occur (checked below)
INNER = {(40, 150): (85, 21, 120, 37), (24, 333): (201, 3, 290, 22), (50, 83): (31, 31, 60, 47)}


@pytest.fixture(scope="module")
def lib():
    build_ext.build()
    return _lib.load()


def _rings(h, w, inner, scale=1, odd=0):
    """n = 3: no ring / a ring / a ring too thin for any 6x6 window; at `scale` times the resolution (+ odd: canvas not even)"""
    H, W = h * scale + odd, w * scale + odd
    x0, y0, x1, y1 = (v * scale + odd for v in inner)
    return (H, W), np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                             [0, 0, W, H, x0, y0, x1, y1],
                             [0, 0, W, H, 5, 5, W - 5, H - 5]], dtype=np.int32)


def _mask(H, W, ring):
    m = np.zeros((H, W), dtype=bool)
    ox0, oy0, ox1, oy1, ix0, iy0, ix1, iy1 = (int(v) for v in ring)
    if ox1 > ox0 and oy1 > oy0:
        m[max(oy0, 0):oy1, max(ox0, 0):ox1] = True
        m[max(iy0, 0):max(iy1, 0), max(ix0, 0):max(ix1, 0)] = False
    return m


def _erode(m):
    p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), dtype=bool)
    p[1:-1, 1:-1] = m
    out = np.ones_like(m)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def _pool(m):
    H, W = m.shape[0] // 2, m.shape[1] // 2
    return m[:2 * H, :2 * W].reshape(H, 2, W, 2).all(axis=(1, 3))


def _tiles(m):
    """behind the F(4x4, 3x3) kernels: the outputs of the aligned tiles whose whole window is known, and nothing else"""
    out = np.zeros_like(m)
    for py in range(0, m.shape[0] - 3, 4):
        for px in range(0, m.shape[1] - 3, 4):
            if _pure(m, py, px):
                out[py:py + 4, px:px + 4] = True
    return out


def _pure(m, py, px):
    H, W = m.shape
    if py - 1 < 0 or px - 1 < 0 or py + 5 > H or px + 5 > W:
        return False
    return bool(m[py - 1:py + 5, px - 1:px + 5].all())


def _walk(lib, rings, shape, ops):
    """rings and masks after the chain `ops` (0: conv3x3 direct, 1: pool, 2: conv3x3 F(4x4, 3x3)) -> (H, W), rings, masks"""
    H, W = shape
    masks = [_mask(H, W, r) for r in rings]
    rings = rings.copy()
    for op in ops:
        nxt = np.empty_like(rings)
        assert lib.ptmi_frame_ring_next(rings.ctypes.data, nxt.ctypes.data, len(rings), op, H, W) == 0
        rings = nxt
        masks = [(_erode, _pool, _tiles)[op](m) for m in masks]
        if op == 1:
            H, W = H // 2, W // 2
    return (H, W), rings, masks


def _reference_tiles(masks, H, W):
    """per pixel tile: (number of pure tiles, spans two strips)"""
    n, bands, period = len(masks), -(-H // 8), (W + 4) & ~3
    n_pix = -(-(n * bands * period) // 64)
    pure = np.zeros(n_pix, dtype=np.int32)
    for pix in range(n_pix):
        for t in range(32):
            u = pix * 64 + 4 * (t & 15)
            sf = u // period
            px, sn = u - sf * period, sf // bands
            py = (sf - sn * bands) * 8 + 4 * (t >> 4)
            if sn < n and px < W and py < H and _pure(masks[sn], py, px):
                pure[pix] += 1
    straddle = np.array([(p * 64) // period != (p * 64 + 63) // period for p in range(n_pix)])
    return pure, straddle


def _lists(lib, rings, H, W):
    n_pix = lib.ptmi_frame_pixel_tiles(len(rings), H, W)
    keep, skip = np.full(n_pix, -1, np.int32), np.full(n_pix, -1, np.int32)
    counts = np.zeros(2, np.int32)
    assert lib.ptmi_frame_skip_lists(rings.ctypes.data, len(rings), H, W, keep.ctypes.data, skip.ctypes.data,
                                     counts.ctypes.data) == 0
    return n_pix, keep[:counts[0]], skip[:counts[1]]


CHAINS = [((), 1, 0, True), ((0,), 1, 0, True), ((0, 0), 1, 0, True), ((0, 0, 1), 2, 1, False), ((0, 0, 1, 0), 2, 0, False),
          ((0, 1, 0, 0, 1, 0), 4, 3, False), ((2,), 1, 0, True), ((0, 2), 1, 0, True), ((0, 2, 1), 2, 1, True), ((0, 2, 1, 2), 2, 0, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: "in" + "".join("cpw"[o] for o in c[0]))
def test_predicate_and_lists_against_brute_force(lib, shape, chain):
    ops, scale, odd, exact = chain
    start, rings0 = _rings(shape[0], shape[1], INNER[shape], scale, odd)
    (H, W), rings, masks = _walk(lib, rings0, start, ops)
    assert (H, W) == shape
    # per 4x4 tile, every aligned tile of every image -- and a few unaligned / outside ones, which are never skippable
    for sn, (ring, m) in enumerate(zip(rings, masks)):
        ring = np.ascontiguousarray(ring)
        for py in range(-4, H + 4, 4):
            for px in range(-4, W + 4, 4):
                got = bool(lib.ptmi_frame_tile_skippable(ring.ctypes.data, H, W, py, px))
                want = 0 <= py and py + 4 <= H and 0 <= px and px + 4 <= W and _pure(m, py, px)
                assert not (got and not want), f"image {sn}: impure tile ({py}, {px}) skipped"
                if exact:
                    assert got == want, f"image {sn}: tile ({py}, {px}): header {got}, reference {want}"
    pure, straddle = _reference_tiles(masks, H, W)
    n_pix, keep, skip = _lists(lib, rings, H, W)
    assert n_pix == len(pure)
    assert sorted(np.concatenate([keep, skip]).tolist()) == list(range(n_pix))            # a partition, each list ascending
    assert (np.diff(keep) > 0).all() and (np.diff(skip) > 0).all()
    assert all(pure[p] == 32 for p in skip), "a pixel tile with an impure tile is skipped"
    for p in range(n_pix):                                                                  # the list builder and THE predicate agree
        assert bool(lib.ptmi_frame_pixel_tile_skippable(rings.ctypes.data, len(rings), H, W, p)) == (p in set(skip.tolist()))
    if exact:
        assert skip.tolist() == np.nonzero(pure == 32)[0].tolist()
    if not ops:
        whole = (pure == 32) & ~straddle
        partial = (pure > 0) & (pure < 32) & ~straddle
        assert whole.any() and partial.any() and ((pure > 0) & straddle).any(), (whole.sum(), partial.sum())
        assert not ((pure == 32) & straddle).any()
        # only the middle image contributes: the first has no ring, the third's is too thin
        bands, period = -(-H // 8), (W + 4) & ~3
        assert all(bands * period <= p * 64 and p * 64 + 63 < 2 * bands * period for p in np.nonzero(pure == 32)[0])
        assert len(skip) > 0


def test_ring_propagation_is_conservative_on_odd_canvases(lib):
    """pool of odd rectangles at odd sizes: every pixel the propagated ring calls known is known to the brute-force mask"""
    rng = np.random.RandomState(7)
    for _ in range(40):
        H, W = int(rng.randint(30, 90)), int(rng.randint(30, 90))
        x0, y0 = int(rng.randint(1, W // 2)), int(rng.randint(1, H // 2))
        rings = np.array([[0, 0, W, H, x0, y0, x0 + int(rng.randint(3, W // 2)), y0 + int(rng.randint(3, H // 2))]], np.int32)
        ops = [int(v) for v in rng.randint(0, 2, size=4)]
        (h, w), out, masks = _walk(lib, rings, (H, W), ops)
        if h == 0 or w == 0:
            continue
        assert not (_mask(h, w, out[0]) & ~masks[0]).any(), (H, W, ops)
