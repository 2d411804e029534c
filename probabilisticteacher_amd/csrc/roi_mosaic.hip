// roi_mosaic.hip -- the ROI mosaic: pooled ROIs packed into canvases, so that the conv layers of the box head
// (MODEL.ROI_BOX_HEAD.NUM_CONV > 0, D2 FastRCNNConvFCHead) run on the tuned 3x3 kernels as ordinary maps.  gfx950 only.
//
// Layout.  A pooled ROI is a (C, P, P) map.  A cell is p x p pixels, p = P + 1; a canvas holds gx x gx cells, gx = max(1, 64 / p),
// and is a (C, S, S) map, S = gx * p (P = 7: 64 ROIs on a 64 x 64 canvas).  ROI r sits in canvas r / gx^2, cell row
// (r % gx^2) / gx, cell column r % gx; its data are the first P rows and columns of the cell.  Row P and column P of every cell
// (the gutter) and the cells past R are exactly 0.0 in every tensor a convolution reads: each ROI then sees a zero ring, from
// the gutter or from the convolution's own padding, and the convolution of the canvas is the per-ROI convolution on the data.
//
//   mosaic_copy_kernel      pack (ROIs -> canvases, zeros written to gutters and empty cells), unpack (its backward: data pixels
//                           only) and mask (canvas -> canvas with gutters and empty cells zeroed).  A workgroup owns one cell row
//                           of one canvas for 16 channels: canvas rows are read / written as whole lines (16-byte vectors where
//                           S % 4 == 0 and the canvas sits on a 16-byte boundary, dwords otherwise), the ROI side as runs of
//                           16 channels x P x P contiguous floats per ROI.
//   mosaic_gn_fwd_kernel    relu(GroupNorm(z)) per (ROI, group) over the data pixels: one wave per run, the run's cell (C / G
//                           channels x p x p, gutter included, at most 2048 floats) in registers: sum -> mean, corrected by the
//                           residual sum about it, then M2 about the mean -- a large mean does not cancel.  Lanes are combined
//                           by a butterfly, so every lane holds the same bits.  Gutters and empty cells of y are written as 0.
//   mosaic_gn_bwd_kernel    dz = rstd * (gamma * g - (s1 + xhat * s2) / L), g = dy * [y > 0], same wave <-> run assignment.
//   mosaic_gn_dgb_kernel    per (canvas, channel) plane: A = sum g, B = sum g * xhat over the canvas's ROIs (a fixed block of gx^2
//                           ROIs, fixed thread <-> pixel assignment, fixed tree) into the workspace;
//   mosaic_gn_dgb_final     canvases in canvas order, in double -> dbeta, dgamma.  No atomics anywhere.
//
// The lane <-> element assignment depends on the shape alone (quads where p % 4 == 0, single floats otherwise); the address only
// decides whether a quad is moved by one 16-byte access or by four dwords.  The bits are the same at any address.
#include "common.h"

namespace {

struct Mosaic {
    int P, p, gx, S, cells;
    int64_t ncv;        // canvases
};

inline Mosaic mosaic_of(int r, int pooled)
{
    Mosaic m;
    m.P = pooled, m.p = pooled + 1;
    m.gx = 64 / m.p < 1 ? 1 : 64 / m.p;
    m.S = m.gx * m.p;
    m.cells = m.gx * m.gx;
    m.ncv = cdiv64(r, m.cells);
    return m;
}

inline bool mosaic_dims_ok(int r, int c, int pooled) { return r >= 0 && c > 0 && pooled > 0 && pooled <= 4096; }

constexpr int64_t MZ_MAX_GRID = 0x7FFFFFFFll;
constexpr int MZ_CG = 16;           // channels a workgroup of the copy kernels moves
constexpr int MZ_GN_MAX_RUN = PTMI_ROI_MOSAIC_GN_MAX_CELL;

enum { MZ_PACK = 0, MZ_UNPACK = 1, MZ_MASK = 2 };

template <int V>
__device__ __forceinline__ void mz_load(const float* __restrict__ p, bool vec, float v[V])
{
    if (V == 4 && vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = p[k];
    }
}

template <int V>
__device__ __forceinline__ void mz_store(float* __restrict__ p, bool vec, const float v[V])
{
    if (V == 4 && vec) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) p[k] = v[k];
    }
}

// rois: (R, C, P, P); canvas: (ncv, C, S, S).  PACK rois -> canvas, UNPACK canvas -> rois, MASK canvas (src) -> canvas (dst).
template <int MODE, int V>
__global__ __launch_bounds__(256) void mosaic_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C, int P,
                                                          int p, int gx, int S, int ncg, int vec)
{
    const unsigned b = blockIdx.x;
    const int cg = (int)(b % (unsigned)ncg);
    const unsigned cell_row = b / (unsigned)ncg;
    const int cy = (int)(cell_row % (unsigned)gx);
    const int64_t cv = cell_row / (unsigned)gx;
    const int c0 = cg * MZ_CG;
    const int nc = C - c0 < MZ_CG ? C - c0 : MZ_CG;
    const int rowv = S / V;                 // vectors per canvas row
    const int per_c = p * rowv;             // ... per channel of the cell row
    const int total = nc * per_c;
    const int64_t r_row = (cv * gx + cy) * (int64_t)gx;       // the cell row's first ROI
    for (int i = threadIdx.x; i < total; i += 256) {
        const int cl = i / per_c, rem = i - cl * per_c;
        const int iy = rem / rowv, x = (rem - iy * rowv) * V;
        const int c = c0 + cl;
        const int64_t coff = ((cv * C + c) * S + (int64_t)cy * p + iy) * S + x;
        float v[V];
        if (MODE != MZ_PACK) mz_load<V>(src + coff, vec != 0, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int X = x + k, cx = X / p, ix = X - cx * p;
            const int64_t r = r_row + cx;
            const bool data = iy < P && ix < P && r < R;
            const int64_t roff = ((r * C + c) * P + iy) * P + ix;
            if (MODE == MZ_PACK) v[k] = data ? src[roff] : 0.f;
            if (MODE == MZ_MASK) v[k] = data ? v[k] : 0.f;
            if (MODE == MZ_UNPACK && data) dst[roff] = v[k];
        }
        if (MODE != MZ_UNPACK) mz_store<V>(dst + coff, vec != 0, v);
    }
}

// all-lane wave64 sum: a butterfly, every lane ends with the same bits
__device__ __forceinline__ float wave_allsum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// what a wave of the GroupNorm kernels works on: the cell of ROI `r` for the cpg channels of group g
struct MzRun {
    int64_t r, base;        // ROI (= cell index over all canvases), element offset of the cell's first pixel in channel g * cpg
    int g;
    bool live;              // false: beyond the runs of the launch
};

__device__ __forceinline__ MzRun mz_run(int C, int G, int p, int gx, int S, int64_t ncells)
{
    MzRun w;
    const int64_t run = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    w.live = run < ncells * G;
    w.r = run / G;
    w.g = (int)(run - w.r * G);
    const int cells = gx * gx;
    const int64_t cv = w.r / cells;
    const int ci = (int)(w.r - cv * cells);
    const int cy = ci / gx, cx = ci - cy * gx;
    w.base = ((cv * C + (int64_t)w.g * (C / G)) * S + (int64_t)cy * p) * S + (int64_t)cx * p;
    return w;
}

// element e of a run's cell -> channel within the group, row, column; its offset from the run's base
struct MzElem {
    int cl, iy, ix, off;
};

__device__ __forceinline__ MzElem mz_elem(int e, int p, int S)
{
    MzElem m;
    const int pp = p * p;
    m.cl = e / pp;
    const int rem = e - m.cl * pp;
    m.iy = rem / p;
    m.ix = rem - m.iy * p;
    m.off = m.cl * S * S + m.iy * S + m.ix;
    return m;
}

template <int V, int NS>
__global__ __launch_bounds__(256) void mosaic_gn_fwd_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            float* __restrict__ mean_rstd, int R, int C, int G, int P, int p, int gx,
                                                            int S, int64_t ncells, float eps, int vec)
{
    const MzRun w = mz_run(C, G, p, gx, S, ncells);
    if (!w.live) return;                                 // (wave-uniform; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    const int cpg = C / G, J = cpg * p * p;
    const float* zp = z + w.base;
    float* yp = y + w.base;
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    if (w.r >= R) {                                      // an empty cell of the last canvas
        for (int e = lane * V; e < J; e += 64 * V) mz_store<V>(yp + mz_elem(e, p, S).off, vec != 0, zero);
        return;
    }
    float v[NS][V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = (lane + 64 * i) * V;
        const MzElem m = mz_elem(e, p, S);
        const bool row = e < J && m.iy < P;
#pragma unroll
        for (int k = 0; k < V; ++k) v[i][k] = 0.f;
        if (row) mz_load<V>(zp + m.off, vec != 0, v[i]);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (!(row && m.ix + k < P)) v[i][k] = 0.f;
            s += v[i][k];
        }
    }
    const float L = (float)(cpg * P * P);
    const float m0 = wave_allsum(s) / L;
    float d1 = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = (lane + 64 * i) * V;
        const MzElem m = mz_elem(e, p, S);
        const bool row = e < J && m.iy < P;
#pragma unroll
        for (int k = 0; k < V; ++k) d1 += row && m.ix + k < P ? v[i][k] - m0 : 0.f;
    }
    const float mean = m0 + wave_allsum(d1) / L;         // the sum's own rounding, taken back out
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = (lane + 64 * i) * V;
        const MzElem m = mz_elem(e, p, S);
        const bool row = e < J && m.iy < P;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float d = v[i][k] - mean;
            q += row && m.ix + k < P ? d * d : 0.f;
        }
    }
    const float rstd = 1.f / sqrtf(wave_allsum(q) / L + eps);
    if (lane == 0) {
        mean_rstd[2 * (w.r * G + w.g)] = mean;
        mean_rstd[2 * (w.r * G + w.g) + 1] = rstd;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = (lane + 64 * i) * V;
        if (e >= J) continue;
        const MzElem m = mz_elem(e, p, S);
        const int ch = w.g * cpg + m.cl;
        const float ga = gamma[ch], be = beta[ch];
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float t = (v[i][k] - mean) * rstd * ga + be;
            o[k] = m.iy < P && m.ix + k < P ? (t < 0.f ? 0.f : t) : 0.f;        // (a NaN stays a NaN, as torch.relu keeps it)
        }
        mz_store<V>(yp + m.off, vec != 0, o);
    }
}

template <int V, int NS>
__global__ __launch_bounds__(256) void mosaic_gn_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ z, const float* __restrict__ gamma,
                                                            const float* __restrict__ mean_rstd, float* __restrict__ dz, int R,
                                                            int C, int G, int P, int p, int gx, int S, int64_t ncells, int vec)
{
    const MzRun w = mz_run(C, G, p, gx, S, ncells);
    if (!w.live) return;
    const int lane = threadIdx.x & 63;
    const int cpg = C / G, J = cpg * p * p;
    float* op = dz + w.base;
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    if (w.r >= R) {
        for (int e = lane * V; e < J; e += 64 * V) mz_store<V>(op + mz_elem(e, p, S).off, vec != 0, zero);
        return;
    }
    const float mean = mean_rstd[2 * (w.r * G + w.g)], rstd = mean_rstd[2 * (w.r * G + w.g) + 1];
    float gv[NS][V], xh[NS][V];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = (lane + 64 * i) * V;
        const MzElem m = mz_elem(e, p, S);
        const bool row = e < J && m.iy < P;
        float d4[V], y4[V], z4[V];
#pragma unroll
        for (int k = 0; k < V; ++k) d4[k] = y4[k] = z4[k] = 0.f;
        if (row) {
            mz_load<V>(dy + w.base + m.off, vec != 0, d4);
            mz_load<V>(y + w.base + m.off, vec != 0, y4);
            mz_load<V>(z + w.base + m.off, vec != 0, z4);
        }
        const float ga = row ? gamma[w.g * cpg + m.cl] : 0.f;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool data = row && m.ix + k < P;
            gv[i][k] = data && y4[k] > 0.f ? d4[k] : 0.f;
            xh[i][k] = data ? (z4[k] - mean) * rstd : 0.f;
            s1 += ga * gv[i][k];
            s2 += ga * gv[i][k] * xh[i][k];
        }
    }
    const float L = (float)(cpg * P * P);
    s1 = wave_allsum(s1) / L;
    s2 = wave_allsum(s2) / L;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int e = (lane + 64 * i) * V;
        if (e >= J) continue;
        const MzElem m = mz_elem(e, p, S);
        const float ga = gamma[w.g * cpg + m.cl];
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k)
            o[k] = m.iy < P && m.ix + k < P ? rstd * (gv[i][k] * ga - (s1 + xh[i][k] * s2)) : 0.f;
        mz_store<V>(op + m.off, vec != 0, o);
    }
}

// one (canvas, channel) plane: A = sum g, B = sum g * xhat over the data pixels of the canvas's ROIs
template <int V>
__global__ __launch_bounds__(256) void mosaic_gn_dgb_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ z, const float* __restrict__ mean_rstd,
                                                            int R, int C, int G, int P, int p, int gx, int S,
                                                            float2* __restrict__ part, int vec)
{
    __shared__ float sm[4];
    const int ch = (int)(blockIdx.x % (unsigned)C);
    const int64_t cv = blockIdx.x / (unsigned)C;
    const int g = ch / (C / G);
    const int64_t plane = (cv * C + ch) * (int64_t)S * S;
    const int n = S * S;
    float a = 0.f, b = 0.f;
    for (int e = threadIdx.x * V; e < n; e += 256 * V) {
        const int Y = e / S, X0 = e - Y * S;
        const int cy = Y / p, iy = Y - cy * p;
        if (iy >= P) continue;
        float d4[V], y4[V], z4[V];
        mz_load<V>(dy + plane + e, vec != 0, d4);
        mz_load<V>(y + plane + e, vec != 0, y4);
        mz_load<V>(z + plane + e, vec != 0, z4);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int X = X0 + k, cx = X / p, ix = X - cx * p;
            const int64_t r = (cv * gx + cy) * (int64_t)gx + cx;
            if (ix < P && r < R) {
                const float mean = mean_rstd[2 * (r * G + g)], rstd = mean_rstd[2 * (r * G + g) + 1];
                const float gg = y4[k] > 0.f ? d4[k] : 0.f;
                a += gg;
                b += gg * ((z4[k] - mean) * rstd);
            }
        }
    }
    const float at = block_sum_256(a, sm);
    const float bt = block_sum_256(b, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = make_float2(at, bt);
}

__global__ __launch_bounds__(64) void mosaic_gn_dgb_final(const float2* __restrict__ part, int64_t ncv, int C,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= C) return;
    double a = 0.0, b = 0.0;
    for (int64_t cv = 0; cv < ncv; ++cv) {
        const float2 v = part[cv * C + ch];
        a += (double)v.x;
        b += (double)v.y;
    }
    dbeta[ch] = (float)a;
    dgamma[ch] = (float)b;
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr)
{
    return ((((uintptr_t)a | (uintptr_t)b) | ((uintptr_t)c | (uintptr_t)d)) & 15) == 0;
}

template <int MODE>
int mosaic_copy(const char* name, const float* src, float* dst, int r, int c, int pooled, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(mosaic_dims_ok(r, c, pooled), "%s: bad shape r %d c %d pooled %d", name, r, c, pooled);
    if (r == 0) return 0;
    PTMI_CHECK_ARG(src && dst, "%s: null pointer", name);
    PTMI_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "%s: misaligned tensor (4 bytes)", name);
    PTMI_CHECK_ARG(MODE != MZ_MASK || src != dst, "%s: in place", name);
    const Mosaic m = mosaic_of(r, pooled);
    const int ncg = cdiv(c, MZ_CG);
    const int64_t grid = m.ncv * m.gx * ncg;
    PTMI_CHECK_ARG(grid <= MZ_MAX_GRID, "%s: too many ROIs for one launch", name);
    const float* canvas_a = MODE == MZ_PACK ? dst : src;
    const float* canvas_b = MODE == MZ_MASK ? dst : canvas_a;
    if (m.S % 4 == 0)
        hipLaunchKernelGGL((mosaic_copy_kernel<MODE, 4>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, src, dst, r, c, m.P, m.p,
                           m.gx, m.S, ncg, (int)aligned16(canvas_a, canvas_b));
    else
        hipLaunchKernelGGL((mosaic_copy_kernel<MODE, 1>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, src, dst, r, c, m.P, m.p,
                           m.gx, m.S, ncg, 0);
    PTMI_LAUNCH_CHECK(name);
    return 0;
}

inline bool mosaic_gn_dims_ok(int r, int c, int pooled, int groups)
{
    return mosaic_dims_ok(r, c, pooled) && groups > 0 && c % groups == 0 &&
           (int64_t)(c / groups) * (pooled + 1) * (pooled + 1) <= MZ_GN_MAX_RUN;
}

inline int64_t al256(int64_t b) { return (b + 255) / 256 * 256; }

// slots a lane holds: the run's cell in vectors of V over 64 lanes, rounded up to a power of two
inline int mosaic_gn_slots(int c, int groups, int p, int V)
{
    const int need = cdiv(cdiv((c / groups) * p * p, V), 64);
    int ns = 1;
    while (ns < need) ns *= 2;
    return ns;
}

#define MZ_GN_LAUNCH(KERNEL, V, NS, ...) \
    hipLaunchKernelGGL((KERNEL<V, NS>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, __VA_ARGS__)
#define MZ_GN_DISPATCH(KERNEL, ...)                                        \
    do {                                                                   \
        if (V == 4) {                                                      \
            switch (ns) {                                                  \
            case 1: MZ_GN_LAUNCH(KERNEL, 4, 1, __VA_ARGS__); break;        \
            case 2: MZ_GN_LAUNCH(KERNEL, 4, 2, __VA_ARGS__); break;        \
            case 4: MZ_GN_LAUNCH(KERNEL, 4, 4, __VA_ARGS__); break;        \
            default: MZ_GN_LAUNCH(KERNEL, 4, 8, __VA_ARGS__); break;       \
            }                                                              \
        } else {                                                           \
            switch (ns) {                                                  \
            case 1: MZ_GN_LAUNCH(KERNEL, 1, 1, __VA_ARGS__); break;        \
            case 2: MZ_GN_LAUNCH(KERNEL, 1, 2, __VA_ARGS__); break;        \
            case 4: MZ_GN_LAUNCH(KERNEL, 1, 4, __VA_ARGS__); break;        \
            case 8: MZ_GN_LAUNCH(KERNEL, 1, 8, __VA_ARGS__); break;        \
            case 16: MZ_GN_LAUNCH(KERNEL, 1, 16, __VA_ARGS__); break;      \
            default: MZ_GN_LAUNCH(KERNEL, 1, 32, __VA_ARGS__); break;      \
            }                                                              \
        }                                                                  \
    } while (0)

}  // namespace

extern "C" {

int ptmi_roi_mosaic_gn_max_cell(void) { return MZ_GN_MAX_RUN; }

int ptmi_roi_mosaic_pack(const float* x, float* canvas, int r, int c, int pooled, ptmi_stream_t s)
{
    return mosaic_copy<MZ_PACK>("roi_mosaic_pack", x, canvas, r, c, pooled, s);
}

int ptmi_roi_mosaic_unpack(const float* canvas, float* x, int r, int c, int pooled, ptmi_stream_t s)
{
    return mosaic_copy<MZ_UNPACK>("roi_mosaic_unpack", canvas, x, r, c, pooled, s);
}

int ptmi_roi_mosaic_mask(const float* in, float* out, int r, int c, int pooled, ptmi_stream_t s)
{
    return mosaic_copy<MZ_MASK>("roi_mosaic_mask", in, out, r, c, pooled, s);
}

int64_t ptmi_roi_mosaic_gn_ws_bytes(int r, int c, int pooled, int groups)
{
    if (!mosaic_gn_dims_ok(r, c, pooled, groups)) {
        ptmi_set_error("roi_mosaic_gn_ws_bytes: bad shape r %d c %d pooled %d groups %d (c a multiple of groups, at most %d floats "
                       "per (ROI, group) cell)", r, c, pooled, groups, MZ_GN_MAX_RUN);
        return -1;
    }
    if (r == 0) return 256;
    return al256(8 * mosaic_of(r, pooled).ncv * c);
}

int ptmi_roi_mosaic_gn_relu_fwd(const float* z, const float* gamma, const float* beta, float* y, float* mean_rstd, int r, int c,
                                int pooled, int groups, float eps, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(mosaic_gn_dims_ok(r, c, pooled, groups), "roi_mosaic_gn_relu_fwd: bad shape r %d c %d pooled %d groups %d (c a "
                   "multiple of groups, at most %d floats per (ROI, group) cell)", r, c, pooled, groups, MZ_GN_MAX_RUN);
    if (r == 0) return 0;
    PTMI_CHECK_ARG(z && gamma && beta && y && mean_rstd, "roi_mosaic_gn_relu_fwd: null pointer");
    PTMI_CHECK_ARG((((uintptr_t)z | (uintptr_t)y | (uintptr_t)mean_rstd) & 3) == 0, "roi_mosaic_gn_relu_fwd: misaligned tensor (4 bytes)");
    PTMI_CHECK_ARG(eps > 0.f, "roi_mosaic_gn_relu_fwd: eps must be positive");
    const Mosaic m = mosaic_of(r, pooled);
    const int64_t ncells = m.ncv * m.cells;
    const int64_t grid = cdiv64(ncells * groups, 4);
    PTMI_CHECK_ARG(grid <= MZ_MAX_GRID, "roi_mosaic_gn_relu_fwd: too many ROIs for one launch");
    const int V = m.p % 4 == 0 ? 4 : 1, ns = mosaic_gn_slots(c, groups, m.p, V);
    const int vec = V == 4 && aligned16(z, y);
    MZ_GN_DISPATCH(mosaic_gn_fwd_kernel, z, gamma, beta, y, mean_rstd, r, c, groups, m.P, m.p, m.gx, m.S, ncells, eps, vec);
    PTMI_LAUNCH_CHECK("roi_mosaic_gn_fwd");
    return 0;
}

int ptmi_roi_mosaic_gn_relu_bwd(const float* dy, const float* y, const float* z, const float* gamma, const float* mean_rstd,
                                float* dz, float* dgamma, float* dbeta, int r, int c, int pooled, int groups, void* ws,
                                ptmi_stream_t s)
{
    PTMI_CHECK_ARG(mosaic_gn_dims_ok(r, c, pooled, groups), "roi_mosaic_gn_relu_bwd: bad shape r %d c %d pooled %d groups %d (c a "
                   "multiple of groups, at most %d floats per (ROI, group) cell)", r, c, pooled, groups, MZ_GN_MAX_RUN);
    if (r == 0) return 0;
    PTMI_CHECK_ARG(dy && y && z && gamma && mean_rstd && dz && dgamma && dbeta && ws, "roi_mosaic_gn_relu_bwd: null pointer");
    PTMI_CHECK_ARG(((uintptr_t)ws & 255) == 0 && (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)z | (uintptr_t)dz) & 3) == 0,
                   "roi_mosaic_gn_relu_bwd: misaligned workspace (256 bytes) or tensor (4 bytes)");
    const Mosaic m = mosaic_of(r, pooled);
    const int64_t ncells = m.ncv * m.cells;
    const int64_t grid = cdiv64(ncells * groups, 4);
    PTMI_CHECK_ARG(grid <= MZ_MAX_GRID && m.ncv * c <= MZ_MAX_GRID, "roi_mosaic_gn_relu_bwd: too many ROIs for one launch");
    const int V = m.p % 4 == 0 ? 4 : 1, ns = mosaic_gn_slots(c, groups, m.p, V);
    const int vec = V == 4 && aligned16(dy, y, z, dz);
    float2* part = reinterpret_cast<float2*>(ws);
    const dim3 planes((unsigned)(m.ncv * c));
    if (m.S % 4 == 0)
        hipLaunchKernelGGL(mosaic_gn_dgb_kernel<4>, planes, dim3(256), 0, (hipStream_t)s, dy, y, z, mean_rstd, r, c, groups, m.P, m.p,
                           m.gx, m.S, part, (int)aligned16(dy, y, z));
    else
        hipLaunchKernelGGL(mosaic_gn_dgb_kernel<1>, planes, dim3(256), 0, (hipStream_t)s, dy, y, z, mean_rstd, r, c, groups, m.P, m.p,
                           m.gx, m.S, part, 0);
    PTMI_LAUNCH_CHECK("roi_mosaic_gn_dgb");
    hipLaunchKernelGGL(mosaic_gn_dgb_final, dim3((unsigned)cdiv(c, 64)), dim3(64), 0, (hipStream_t)s, part, m.ncv, c, dgamma, dbeta);
    PTMI_LAUNCH_CHECK("roi_mosaic_gn_dgb_final");
    MZ_GN_DISPATCH(mosaic_gn_bwd_kernel, dy, y, z, gamma, mean_rstd, dz, r, c, groups, m.P, m.p, m.gx, m.S, ncells, vec);
    PTMI_LAUNCH_CHECK("roi_mosaic_gn_bwd");
    return 0;
}

}  // extern "C"
