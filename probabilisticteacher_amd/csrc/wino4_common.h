// wino4_common.h -- what the two fused Winograd F(4x4, 3x3) forward / dgrad families share: wino4.hip (round 5: a wave owns all 36
// positions of 32 channels) and wino4p.hip (round 6, the default: the positions split over the two waves of a tile row).  Included
// by those two files and by nothing else.
//
// Shared: the tile geometry and the LDS stages, the transform constants and 1-D transforms, the accumulating MFMA wrappers, the
// DMA slots of the chunk schedule, G g G^T of the weight pack, and the whole host side (packed size, the 32-bit-offset predicate,
// argument checks + grid + launch).  Per family: which wave computes what -- the slab layout inside a chunk (XUC / XUH, the
// destination index of the pack), the slots of the A reads, window reads, transform FMAs and the hand-over, the C = 0 MFMAs,
// and the kernels.
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4 xlds_f32x4_t;
typedef __attribute__((address_space(3))) float xlds_f32_t;
typedef __attribute__((address_space(3))) void xlds_void_t;

constexpr int XKC = 4;                  // input channels per chunk = K of one MFMA
constexpr int XBM = 64;                 // output channels per workgroup
constexpr int XTH = 8, XTW = 64;        // output pixels per workgroup: 8 rows x 64 flat columns = 2 x 16 tiles of 4x4
constexpr int XPP = 72;                 // patch row pitch in floats: 18 pieces, LDS column c <-> flat column u0 - 4 + c
constexpr int XPR = XTH + 2;            // patch rows (image rows y0-1 .. y0+8)
constexpr int XPL = XPR * XPP;          // floats per channel plane (720)
constexpr int XUS = XKC * 9 * XBM * 4;  // U floats per chunk: 4 ci x 36 positions x 64 co = 9216 (36 KB); the order inside a channel: per family
constexpr int XPS = XKC * XPL;          // patch floats per chunk: 2880 = 720 pieces
constexpr int XPSP = 3072;              // ... padded to 3 DMA instructions per lane (pieces 720 .. 767 carry offset 0xFFFFFFFF)
constexpr int XNT = 256;
constexpr int XUI = XUS / 4 / XNT;      // 9 U DMA instructions per lane and chunk
constexpr int XPI = XPSP / 4 / XNT;     // 3 patch DMA instructions per lane and chunk
constexpr int XDI = XUI + XPI;          // 12
constexpr int XNU = 3, XNP = 4;         // stages
constexpr int XRUN = 32;                // dynamic schedule: pixel tiles per channel-tile run of a queue (= the workgroups of one XCD)
constexpr int XLDS = XNU * XUS + XNP * XPSP;   // 39936 floats = 159744 B

// transform constants (a = 3/4, b = 3/2)
constexpr float XA = 0.75f, XB = 1.5f, XA2 = 0.5625f, XB2 = 2.25f, XA3 = 0.421875f, XB3 = 3.375f;
constexpr float XA2B2 = 1.265625f, XS2 = 2.8125f;      // a^2 b^2, a^2 + b^2

// r = c * x + y / r = -c * x + y: explicit FMAs (the files are built with -fno-slp-vectorize: the SLP vectoriser otherwise builds
// v_pk_fma_f32 out of register shuffles -- slower than two scalar FMAs next to MFMAs on this part; inline-asm FMAs cost a
// compiler-inserted s_nop after every dependent pair)
__device__ __forceinline__ float xfma(float c, float x, float y) { return __builtin_fmaf(c, x, y); }
__device__ __forceinline__ float xfnma(float c, float x, float y) { return __builtin_fmaf(-c, x, y); }
__device__ __forceinline__ float xadd(float x, float y) { return x + y; }
__device__ __forceinline__ float xsub(float x, float y) { return x - y; }
__device__ __forceinline__ float xmul(float c, float x) { return c * x; }

// 1-D input transform t = B^T d: operation k of 12 (so that a slot can carry any sub-range of them).  E[] are the four
// intermediates (even / odd parts at +-a and +-b).
// operations 0 .. 5 are independent of each other, 6 .. 11 depend only on 0 .. 5: no back-to-back dependent FMAs
template <int K>
__device__ __forceinline__ void xin_op(const float (&d)[6], float (&t)[6], float (&E)[4])
{
    if constexpr (K == 0) t[0] = xfnma(XS2, d[2], d[4]);
    if constexpr (K == 1) t[5] = xfnma(XS2, d[3], d[5]);
    if constexpr (K == 2) E[0] = xfnma(XB2, d[2], d[4]);        // even part at +-a
    if constexpr (K == 3) E[1] = xfnma(XB2, d[1], d[3]);        // odd part at +-a (before the factor a)
    if constexpr (K == 4) E[2] = xfnma(XA2, d[2], d[4]);
    if constexpr (K == 5) E[3] = xfnma(XA2, d[1], d[3]);
    if constexpr (K == 6) t[0] = xfma(XA2B2, d[0], t[0]);
    if constexpr (K == 7) t[5] = xfma(XA2B2, d[1], t[5]);
    if constexpr (K == 8) t[1] = xfma(XA, E[1], E[0]);
    if constexpr (K == 9) t[2] = xfnma(XA, E[1], E[0]);
    if constexpr (K == 10) t[3] = xfma(XB, E[3], E[2]);
    if constexpr (K == 11) t[4] = xfnma(XB, E[3], E[2]);
}

// 1-D output transform y = A^T m (12 operations): y_k = sum_i p_i^k m_i (+ m_5 for k = 3)
__device__ __forceinline__ void xout(const float (&m)[6], float (&y)[4])
{
    const float s1 = xadd(m[1], m[2]), d1 = xsub(m[1], m[2]), s2 = xadd(m[3], m[4]), d2 = xsub(m[3], m[4]);
    y[0] = xadd(xadd(m[0], s1), s2);
    y[1] = xfma(XB, d2, xmul(XA, d1));
    y[2] = xfma(XB2, s2, xmul(XA2, s1));
    y[3] = xfma(XB3, d2, xfma(XA3, d1, m[5]));
}

// the MFMAs: accumulator tile in AGPRs ("a") or VGPRs ("v")
__device__ __forceinline__ void xmfma_a(f32x4& c, float a, float b) { asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b)); }
__device__ __forceinline__ void xmfma_v(f32x4& c, float a, float b) { asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b)); }

template <int... I, class F>
__device__ __forceinline__ void xfor(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }

// ---- the chunk schedule, shared part: a chunk is 72 slots, one MFMA each.  DMA instruction i sits in slot 5 + 6 i: the twelve
// pieces of a chunk spread EVENLY over its 72 slots -- the L2 -> LDS path moves a chunk's 48 KB in ~1570 cycles (DMA-only
// variant of tools/exp/make_wino4_variant.py: 30 B/clk/CU), two thirds of the chunk's MFMA time, and a burst (round 5's first
// version: 12 instructions in 24 slots) stalls the issuing wave behind its own queue
__host__ __device__ constexpr bool x_is_dma(int s) { return s % 6 == 5; }
__host__ __device__ constexpr int x_dma_at(int s) { return x_is_dma(s) ? s / 6 : -1; }
__host__ __device__ constexpr int x_dma_before(int s) { return (s + 0) / 6; }   // DMA instructions of this chunk issued before slot s

// ---- weight pack: U = G g G^T (6x6 per filter), evaluated in double and rounded once.  A thread owns one (output channel, input
// channel) pair, i.e. 36 floats of the 9 * XBM * 4 = 2304 that an input channel has in a chunk's slab; index(col, i, j) = where
// in those 2304 the family keeps U[i][j] of output channel col of the channel tile.  first / stride: the kernel's grid-stride walk
// (taken by the kernel itself: the block size folds to a constant only there).
// mode as ptmi_conv3x3_pack_weights (1: dgrad -- transposed channels, flipped taps).
template <class Index>
__device__ __forceinline__ void x_pack_weights(const float* __restrict__ w, float* __restrict__ wp, int wCout, int wCin, int mode,
                                               int coTiles, int nChunks, int64_t first, int64_t stride, Index index)
{
    const int64_t total = (int64_t)coTiles * nChunks * XKC * XBM;
    const int convCout = mode ? wCin : wCout, convCin = mode ? wCout : wCin;
    const double G[6][3] = {{64.0 / 81.0, 0.0, 0.0},
                            {-128.0 / 243.0, -32.0 / 81.0, -8.0 / 27.0},
                            {-128.0 / 243.0, 32.0 / 81.0, -8.0 / 27.0},
                            {32.0 / 243.0, 16.0 / 81.0, 8.0 / 27.0},
                            {32.0 / 243.0, -16.0 / 81.0, 8.0 / 27.0},
                            {0.0, 0.0, 1.0}};
    for (int64_t idx = first; idx < total; idx += stride) {
        int64_t t = idx;
        const int col = t % XBM; t /= XBM;
        const int cil = t % XKC; t /= XKC;
        const int chunk = t % nChunks;
        const int cot = t / nChunks;
        const int co = cot * XBM + col, ci = chunk * XKC + cil;
        double g[3][3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                float v = 0.f;
                if (co < convCout && ci < convCin)
                    v = mode == 0 ? w[((size_t)co * wCin + ci) * 9 + ky * 3 + kx]
                                  : w[((size_t)ci * wCin + co) * 9 + (2 - ky) * 3 + (2 - kx)];
                g[ky][kx] = (double)v;
            }
        }
        double rr[6][3];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) rr[i][kx] = G[i][0] * g[0][kx] + G[i][1] * g[1][kx] + G[i][2] * g[2][kx];
        }
        float* dst = wp + ((size_t)(cot * nChunks + chunk) * XKC + cil) * (9 * XBM * 4);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j < 6; ++j)
                dst[index(col, i, j)] = (float)(rr[i][0] * G[j][0] + rr[i][1] * G[j][1] + rr[i][2] * G[j][2]);
        }
    }
}

// ---- host side.  `name` is the entry point's name in error strings ("conv3x3_wino4_fwd", "conv3x3_wino4p_pack_weights", ...).
typedef void (*x_pack_kernel_t)(const float*, float*, int, int, int, int, int);
typedef void (*x_fwd_kernel_t)(const float*, const float*, const float*, const float*, float*, int, int, int, int, int, int, int, int,
                               int, int, int, int, int, int*);

inline int64_t x_packed_floats(int cin, int cout) { return (int64_t)cdiv(cout, XBM) * cdiv(cin, XKC) * XUS; }

inline int x_pack_weights_launch(const char* name, x_pack_kernel_t kernel, const float* w, float* wp, int w_cout, int w_cin, int mode,
                                 ptmi_stream_t s)
{
    PTMI_CHECK_ARG(w && wp && w_cout > 0 && w_cin > 0, "%s: bad args", name);
    const int convCout = mode ? w_cin : w_cout, convCin = mode ? w_cout : w_cin;
    const int coTiles = cdiv(convCout, XBM), nChunks = cdiv(convCin, XKC);
    const int64_t total = (int64_t)coTiles * nChunks * XKC * XBM;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, wp, w_cout, w_cin, mode, coTiles, nChunks);
    PTMI_LAUNCH_CHECK(name);
    return 0;
}

inline int x_fwd_fits(int cin, int cout, int h, int w)
{
    if (cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || (cin & 7)) return 0;       // chunks of 4 channels, walked in pairs
    // a workgroup's 64 flat columns may reach into the strips of later images: per-lane offsets are relative to the first one
    const int64_t img_span = XTW / ((w + 4) & ~3) + 2;
    return (img_span * cin + XKC) * h * w * 4 < (1ll << 32) && (img_span * cout + XBM) * h * w * 4 < (1ll << 32);
}

// dyn / stat: the family's kernel with / without the dynamic tile schedule
inline int x_fwd_sched(const char* name, x_fwd_kernel_t dyn, x_fwd_kernel_t stat, const float* x, const float* wp, const float* bias,
                       const float* mask_ref, float* y, int n, int cin, int cout, int h, int w, int epilogue, int32_t* sched,
                       ptmi_stream_t s)
{
    PTMI_CHECK_ARG(x && wp && y && n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "%s: bad args", name);
    PTMI_CHECK_ARG(epilogue >= 0 && epilogue <= 4, "%s: bad epilogue %d", name, epilogue);
    PTMI_CHECK_ARG(!(cin & 7), "%s: cin %d is not a multiple of 8 (use ptmi_conv3x3_wino_fwd)", name, cin);
    PTMI_CHECK_ARG(x_fwd_fits(cin, cout, h, w), "%s: image too large for 32-bit buffer offsets (n=%d cin=%d cout=%d h=%d w=%d)",
                   name, n, cin, cout, h, w);
    PTMI_CHECK_ARG(epilogue > 1 || bias, "%s: bias required for epilogue %d", name, epilogue);
    PTMI_CHECK_ARG(epilogue != 4 || bias, "%s: bias required for epilogue 4", name);
    PTMI_CHECK_ARG(epilogue != 3 || mask_ref, "%s: mask_ref required for epilogue 3", name);
    const int bands = cdiv(h, XTH), coTiles = cdiv(cout, XBM), nChunks = cin / XKC;
    const int period = (w + 1 + 3) & ~3;                     // strip length: W + at least one zero column, a multiple of 4
    const int64_t nPix = cdiv64((int64_t)n * bands * period, XTW);
    PTMI_CHECK_ARG(nPix * XTW < (1ll << 31), "%s: too many tiles", name);
    const int colocate = coTiles <= 4;
    const int64_t nWg = colocate ? cdiv64(nPix, 8) * 8 * coTiles : nPix * coTiles;      // tile ids (colocate: some beyond nPix -- the end)
    PTMI_CHECK_ARG(nWg < (1ll << 31) - 4096, "%s: too many tiles", name);
    // persistent workgroups: one per CU (a multiple of 8: a tile stays on the XCD of its id mod 8)
    const int cus = ptmi_device_cus();
    const int64_t grid = nWg < (cus / 8) * 8 ? nWg : (cus / 8) * 8;
    const bool use_dyn = sched && nChunks >= 4;   // (fewer chunks per tile than the schedule's LDS hand-offs assume: the static walk)
    hipLaunchKernelGGL(use_dyn ? dyn : stat, dim3((unsigned)grid), dim3(XNT), 0, (hipStream_t)s, x, wp, bias, mask_ref, y, n, cin, cout,
                       h, w, nChunks, epilogue, coTiles, bands, period, (int)nPix, colocate, (int)nWg, use_dyn ? (int*)sched : (int*)nullptr);
    PTMI_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace
