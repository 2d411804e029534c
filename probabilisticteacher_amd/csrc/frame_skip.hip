// frame_skip.hip -- what goes with the tile-list launch of the fused F(4x4, 3x3) forward kernel (ptmi_conv3x3_wino4p_fwd_list):
// the host-side ring propagation and tile lists, and the kernel that writes the outputs of the tiles the list leaves out.
// Geometry and predicate: frame_skip.h, and nothing else.
#include "common.h"
#include "frame_skip.h"

#include <vector>

namespace {

typedef float fs_f32x4 __attribute__((ext_vector_type(4)));
typedef float fs_f32x2 __attribute__((ext_vector_type(2)));
// 16-byte / 8-byte stores to rows that are only 4-byte aligned (W need not be a multiple of 4): global_store_dwordx4 / x2
typedef fs_f32x4 __attribute__((aligned(4))) fs_f32x4_u;
typedef fs_f32x2 __attribute__((aligned(4))) fs_f32x2_u;

// One workgroup = one skipped pixel tile x 64 output channels.
// Full resolution (pooled = 0): thread = (channel group t >> 5 of 8, tile t & 31): per channel four 16-byte row stores of
// pattern[c][a][0 .. 3] (tiles are aligned to 4 in y and x).
// Pooled (epilogue 4, pooled = 1): the tile's 4x4 outputs are 2x2 pooled ones at (py / 2, px / 2); thread = (channel group t >> 4 of
// 16, tile pair t & 15): the two tiles of a pair are neighbours in a strip, except where the pair straddles a strip end -- one
// 16-byte store per pooled row, or two 8-byte ones.  pattern is indexed in OUTPUT coordinates either way: [c][y & 3][x & 3].
// Every tile is tested with the header's predicate again before anything is stored: a list that disagrees with the rings leaves
// a hole (caught by the tests), never a write outside the image.
__global__ __launch_bounds__(256) void frame_fill_kernel(const int* __restrict__ skip, const int* __restrict__ rings,
                                                         const float* __restrict__ pat, float* __restrict__ y, int N, int Cout,
                                                         int H, int W, int pooled)
{
    const int pix = skip[blockIdx.x];
    const int t = threadIdx.x;
    const int c0 = blockIdx.y * 64;
    if (!pooled) {
        int sn, py, px;
        if (!fs_tile_of(pix, t & 31, N, H, W, sn, py, px)) return;
        if (!fs_tile_skippable(fs_ring_load(rings + (int64_t)sn * FS_RING_INTS), H, W, py, px)) return;
        const int64_t HW = (int64_t)H * W;
#pragma unroll 2
        for (int c = c0 + (t >> 5); c < c0 + 64 && c < Cout; c += 8) {
            float* o = y + ((int64_t)sn * Cout + c) * HW + (int64_t)py * W + px;
            const fs_f32x4* p = (const fs_f32x4*)(pat + (int64_t)c * 16);
#pragma unroll
            for (int a = 0; a < 4; ++a) *(fs_f32x4_u*)(o + (int64_t)a * W) = p[a];
        }
        return;
    }
    const int pr = t & 15, t0 = (pr >> 3) * 16 + (pr & 7) * 2;         // tile row pr >> 3, tile columns 2 (pr & 7), + 1
    int sn[2], py[2], px[2];
    bool ok[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        ok[k] = fs_tile_of(pix, t0 + k, N, H, W, sn[k], py[k], px[k]);
        ok[k] = ok[k] && fs_tile_skippable(fs_ring_load(rings + (int64_t)sn[k] * FS_RING_INTS), H, W, py[k], px[k]);
    }
    const int OH = H >> 1, OW = W >> 1;
    const int64_t OHW = (int64_t)OH * OW;
    const bool pair = ok[0] && ok[1] && sn[0] == sn[1] && py[0] == py[1] && px[1] == px[0] + 4;
    for (int c = c0 + (t >> 4); c < c0 + 64 && c < Cout; c += 16) {
        const float* pc = pat + (int64_t)c * 16;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            fs_f32x2 v[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int oy = (py[k] >> 1) + a, ox = px[k] >> 1;        // ox is even: the pattern row's half (ox & 2)
                v[k] = *(const fs_f32x2*)(pc + (oy & 3) * 4 + (ox & 2));
            }
            if (pair) {
                float* o = y + ((int64_t)sn[0] * Cout + c) * OHW + (int64_t)((py[0] >> 1) + a) * OW + (px[0] >> 1);
                *(fs_f32x4_u*)o = (fs_f32x4){v[0][0], v[0][1], v[1][0], v[1][1]};
            } else {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!ok[k]) continue;
                    float* o = y + ((int64_t)sn[k] * Cout + c) * OHW + (int64_t)((py[k] >> 1) + a) * OW + (px[k] >> 1);
                    *(fs_f32x2_u*)o = v[k];
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int ptmi_frame_ring_next(const int32_t* rings_in, int32_t* rings_out, int n, int op, int h, int w)
{
    PTMI_CHECK_ARG(rings_in && rings_out && n > 0 && op >= 0 && op <= 2 && h > 0 && w > 0, "frame_ring_next: bad args");
    for (int i = 0; i < n; ++i) {
        const fs_ring r = fs_ring_load(rings_in + (int64_t)i * FS_RING_INTS);
        fs_ring_store(op == 0 ? fs_ring_conv3x3(r) : op == 1 ? fs_ring_pool2x2(r) : fs_ring_conv3x3_tiles(r, h, w),
                      rings_out + (int64_t)i * FS_RING_INTS);
    }
    return 0;
}

int64_t ptmi_frame_pixel_tiles(int n, int h, int w) { return n > 0 && h > 0 && w > 0 ? fs_pixel_tiles(n, h, w) : 0; }

int ptmi_frame_tile_skippable(const int32_t* ring, int h, int w, int py, int px)
{
    return ring && fs_tile_skippable(fs_ring_load(ring), h, w, py, px) ? 1 : 0;
}

int ptmi_frame_pixel_tile_skippable(const int32_t* rings, int n, int h, int w, int pix)
{
    return rings && n > 0 && h > 0 && w > 0 && pix >= 0 && pix < fs_pixel_tiles(n, h, w) &&
           fs_pixel_tile_skippable(rings, n, h, w, pix) ? 1 : 0;
}

// keep / skip: room for ptmi_frame_pixel_tiles(n, h, w) ints each; counts[0] / counts[1] = how many were written.  Both lists
// ascend.  Per strip the skippable tile columns are at most two intervals (the predicate is a product of a row and a column
// condition); a pixel tile is skippable iff sixteen skippable tile columns (of both tile rows) fall into it.
int ptmi_frame_skip_lists(const int32_t* rings, int n, int h, int w, int32_t* keep, int32_t* skip, int32_t* counts)
{
    PTMI_CHECK_ARG(rings && keep && skip && counts && n > 0 && h > 0 && w > 0, "frame_skip_lists: bad args");
    const int bands = fs_bands(h), period = fs_period(w);
    const int64_t nPix = fs_pixel_tiles(n, h, w);
    PTMI_CHECK_ARG(nPix * FS_TW < (1ll << 31), "frame_skip_lists: too many tiles");
    std::vector<unsigned char> cnt((size_t)nPix, 0);
    auto emit = [&](int64_t base, int a, int b) {                    // skippable tile columns [a, b) of the strip at flat column base
        if (a >= b) return;
        const int64_t ua = base + a, ub = base + b;
        for (int64_t p = ua / FS_TW; p <= (ub - 1) / FS_TW; ++p) {
            const int64_t lo = ua > p * FS_TW ? ua : p * FS_TW, hi = ub < (p + 1) * FS_TW ? ub : (p + 1) * FS_TW;
            cnt[(size_t)p] += (unsigned char)((hi - lo) / 4);
        }
    };
    for (int sn = 0; sn < n; ++sn) {
        const fs_ring r = fs_ring_load(rings + (int64_t)sn * FS_RING_INTS);
        if (!fs_ring_present(r)) continue;
        const int ox0 = r.ox0 < 0 ? 0 : r.ox0, oy0 = r.oy0 < 0 ? 0 : r.oy0, ox1 = r.ox1 > w ? w : r.ox1, oy1 = r.oy1 > h ? h : r.oy1;
        const bool inner = r.ix1 > r.ix0 && r.iy1 > r.iy0;
        const int pa = fs_up4(ox0 + 1);
        const int last = (ox1 - 5 < w - 4 ? ox1 - 5 : w - 4);       // the last column a skippable tile may start at
        if (last < pa) continue;
        const int pb = (last & ~3) + 4;
        for (int band = 0; band < bands; ++band) {
            bool rows_in = true, rows_out = true;
            for (int k = 0; k < 2; ++k) {
                const int py = band * FS_TH + 4 * k;
                rows_in = rows_in && py + 4 <= h && py - 1 >= oy0 && py + 5 <= oy1;
                rows_out = rows_out && (!inner || py + 5 <= r.iy0 || py - 1 >= r.iy1);
            }
            if (!rows_in) continue;
            const int64_t base = ((int64_t)sn * bands + band) * period;
            if (rows_out) {
                emit(base, pa, pb);
            } else {                                                 // columns px with px + 5 > ix0 and px - 1 < ix1 are blocked
                const int ba = fs_up4(r.ix0 - 4), bb = (r.ix1 & ~3) + 4;
                emit(base, pa, pb < ba ? pb : ba);
                emit(base, pa > bb ? pa : bb, pb);
            }
        }
    }
    int nk = 0, ns = 0;
    for (int64_t p = 0; p < nPix; ++p) {
        if (cnt[(size_t)p] == 16) skip[ns++] = (int32_t)p;
        else keep[nk++] = (int32_t)p;
    }
    counts[0] = nk;
    counts[1] = ns;
    return 0;
}

int ptmi_frame_fill(const int32_t* skip_list, int n_skip, const int32_t* rings, const float* pattern, float* y, int n, int cout,
                    int h, int w, int pooled, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(n_skip >= 0 && n > 0 && cout > 0 && h > 0 && w > 0 && (pooled == 0 || pooled == 1), "frame_fill: bad args");
    if (n_skip == 0) return 0;
    PTMI_CHECK_ARG(skip_list && rings && pattern && y, "frame_fill: bad args");
    PTMI_CHECK_ARG(n_skip <= fs_pixel_tiles(n, h, w) && cdiv(cout, 64) < 65536, "frame_fill: bad list length");
    hipLaunchKernelGGL(frame_fill_kernel, dim3((unsigned)n_skip, (unsigned)cdiv(cout, 64)), dim3(256), 0, (hipStream_t)s,
                       (const int*)skip_list, (const int*)rings, pattern, y, n, cout, h, w, pooled);
    PTMI_LAUNCH_CHECK("frame_fill");
    return 0;
}

}  // extern "C"
