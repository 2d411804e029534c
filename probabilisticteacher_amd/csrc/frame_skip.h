// frame_skip.h -- geometry of the constant frame around a shrink-pasted image, over the tile walk of the fused F(4x4, 3x3) kernels
// (wino4_common.h).  The ONE source of that geometry: the tile-list builder, the fill kernel (frame_skip.hip) and the tests
// (through ptmi_frame_*) all evaluate the functions below, on the host and on the device alike.
//
// PTrainer.resize pastes every strong view, shrunk, into the middle of a canvas filled with one colour.  Per image a RING describes
// where a layer's INPUT is known in advance: every input pixel inside `outer` and outside `inner` (half-open rectangles, in that
// layer's input resolution) holds pattern[c][y & 3][x & 3].  outer.x1 <= outer.x0: the image has no ring.
//   * a 3x3 convolution (pad 1) by a DIRECT kernel maps a ring to the ring of its output pixel by pixel: an output pixel is known
//     iff its 3x3 window is -- outer shrinks by one pixel, inner grows by one;
//   * a 3x3 convolution by the F(4x4, 3x3) kernels maps it TILE by tile: the sixteen outputs of a tile come out of transforms of
//     its whole 6x6 window, so their roundoff -- not their value -- depends on all of it.  Only the outputs of tiles whose window
//     is all pattern are the pattern bit for bit: outer shrinks to the outermost such tiles, inner grows to whole tiles;
//   * a 2x2 / 2 max pool (floor mode): a pooled pixel is known iff its four inputs are -- outer: ceil / floor, inner: floor / ceil.
// A 4x4 output tile at (py, px) reads the 6x6 window (py - 1 .. py + 4, px - 1 .. px + 4): with the whole window inside the ring and
// the tile aligned to 4 in both directions (strips start at column 0, bands at multiples of 8), its inputs -- and, the kernel's
// arithmetic being the same for every tile, its outputs -- are the same bits as any other such tile's.  A pixel tile (64 flat
// columns x 8 rows = 32 tiles, possibly of two strips or two images) is skippable iff all of its 32 tiles are.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FS_HD __host__ __device__ inline
#else
#define FS_HD inline
#endif

constexpr int FS_TH = 8, FS_TW = 64;          // a pixel tile of wino4_common.h: XTH rows x XTW flat columns
constexpr int FS_RING_INTS = 8;               // a ring in memory: ox0, oy0, ox1, oy1, ix0, iy0, ix1, iy1 (int32)

struct fs_ring {
    int ox0, oy0, ox1, oy1;                   // outer: inside it (and outside inner) the input holds the pattern
    int ix0, iy0, ix1, iy1;                   // inner: the pasted image, grown by what the layers before have smeared
};

FS_HD fs_ring fs_ring_load(const int32_t* p)
{
    fs_ring r;
    r.ox0 = p[0]; r.oy0 = p[1]; r.ox1 = p[2]; r.oy1 = p[3];
    r.ix0 = p[4]; r.iy0 = p[5]; r.ix1 = p[6]; r.iy1 = p[7];
    return r;
}
FS_HD void fs_ring_store(const fs_ring& r, int32_t* p)
{
    p[0] = r.ox0; p[1] = r.oy0; p[2] = r.ox1; p[3] = r.oy1;
    p[4] = r.ix0; p[5] = r.iy0; p[6] = r.ix1; p[7] = r.iy1;
}
FS_HD bool fs_ring_present(const fs_ring& r) { return r.ox1 > r.ox0 && r.oy1 > r.oy0; }

// (arithmetic shifts: floor / ceil of a possibly negative coordinate)
FS_HD int fs_floor2(int v) { return v >> 1; }
FS_HD int fs_ceil2(int v) { return (v + 1) >> 1; }

// the ring of a 3x3 / pad 1 convolution's output, from the ring of its input
FS_HD fs_ring fs_ring_conv3x3(fs_ring r)
{
    if (!fs_ring_present(r)) return r;
    r.ox0 += 1; r.oy0 += 1; r.ox1 -= 1; r.oy1 -= 1;
    r.ix0 -= 1; r.iy0 -= 1; r.ix1 += 1; r.iy1 += 1;
    return r;
}
// the ring of the output of a 3x3 / pad 1 convolution by the F(4x4, 3x3) kernels on an H x W map: the union of the 4-aligned
// tiles t with fs_tile_skippable(r, H, W, t) -- exactly the outputs that are the pattern bit for bit
FS_HD int fs_up4(int v) { return (v + 3) & ~3; }
FS_HD fs_ring fs_ring_conv3x3_tiles(fs_ring r, int H, int W)
{
    if (!fs_ring_present(r)) return r;
    const int ox0 = r.ox0 < 0 ? 0 : r.ox0, oy0 = r.oy0 < 0 ? 0 : r.oy0, ox1 = r.ox1 > W ? W : r.ox1, oy1 = r.oy1 > H ? H : r.oy1;
    const int lx = ox1 - 5 < W - 4 ? ox1 - 5 : W - 4, ly = oy1 - 5 < H - 4 ? oy1 - 5 : H - 4;     // the last tile origin inside
    r.ox0 = fs_up4(ox0 + 1); r.oy0 = fs_up4(oy0 + 1);
    r.ox1 = (lx & ~3) + 4; r.oy1 = (ly & ~3) + 4;
    if (r.ix1 > r.ix0 && r.iy1 > r.iy0) {                 // tiles with px + 5 > ix0 and px - 1 < ix1 read the pasted image
        r.ix0 = fs_up4(r.ix0 - 4); r.iy0 = fs_up4(r.iy0 - 4);
        r.ix1 = (r.ix1 & ~3) + 4; r.iy1 = (r.iy1 & ~3) + 4;
    }
    return r;
}
// the ring of a 2x2 / 2 max pool's output
FS_HD fs_ring fs_ring_pool2x2(fs_ring r)
{
    if (!fs_ring_present(r)) return r;
    r.ox0 = fs_ceil2(r.ox0); r.oy0 = fs_ceil2(r.oy0); r.ox1 = fs_floor2(r.ox1); r.oy1 = fs_floor2(r.oy1);
    r.ix0 = fs_floor2(r.ix0); r.iy0 = fs_floor2(r.iy0); r.ix1 = fs_ceil2(r.ix1); r.iy1 = fs_ceil2(r.iy1);
    return r;
}

FS_HD int fs_bands(int H) { return (H + FS_TH - 1) / FS_TH; }
FS_HD int fs_period(int W) { return (W + 4) & ~3; }
FS_HD int64_t fs_pixel_tiles(int N, int H, int W) { return ((int64_t)N * fs_bands(H) * fs_period(W) + FS_TW - 1) / FS_TW; }

// THE predicate: the 4x4 tile at (py, px) of an H x W image with ring r reads nothing but the pattern, and lies inside the image
FS_HD bool fs_tile_skippable(const fs_ring& r, int H, int W, int py, int px)
{
    if (!fs_ring_present(r)) return false;
    if (py < 0 || px < 0 || py + 4 > H || px + 4 > W) return false;                      // never a tile that touches rows >= H / columns >= W
    const int ox0 = r.ox0 < 0 ? 0 : r.ox0, oy0 = r.oy0 < 0 ? 0 : r.oy0;                  // (a ring never reaches beyond the image)
    const int ox1 = r.ox1 > W ? W : r.ox1, oy1 = r.oy1 > H ? H : r.oy1;
    if (px - 1 < ox0 || py - 1 < oy0 || px + 5 > ox1 || py + 5 > oy1) return false;      // the 6x6 window inside outer
    if (r.ix1 <= r.ix0 || r.iy1 <= r.iy0) return true;                                   // (nothing pasted)
    return px + 5 <= r.ix0 || px - 1 >= r.ix1 || py + 5 <= r.iy0 || py - 1 >= r.iy1;     // ... and clear of inner
}

// tile t (0 .. 31: tile row t >> 4, tile column t & 15) of pixel tile pix -> (image, row, column) of its first pixel; false: the
// tile lies in a strip's padding columns or behind the last image (as tile_geometry of the kernels)
FS_HD bool fs_tile_of(int pix, int t, int N, int H, int W, int& sn, int& py, int& px)
{
    const int bands = fs_bands(H), period = fs_period(W);
    const int64_t u = (int64_t)pix * FS_TW + 4 * (t & 15);
    const int64_t sf = u / period;
    px = (int)(u - sf * period);
    sn = (int)(sf / bands);
    py = (int)(sf - (int64_t)sn * bands) * FS_TH + 4 * (t >> 4);
    return sn < N && px < W && py < H;
}

// a pixel tile is skippable iff every one of its 32 tiles is (rings: N x FS_RING_INTS, this layer's input resolution)
FS_HD bool fs_pixel_tile_skippable(const int32_t* rings, int N, int H, int W, int pix)
{
    for (int t = 0; t < 32; ++t) {
        int sn, py, px;
        if (!fs_tile_of(pix, t, N, H, W, sn, py, px)) return false;
        if (!fs_tile_skippable(fs_ring_load(rings + (int64_t)sn * FS_RING_INTS), H, W, py, px)) return false;
    }
    return true;
}
