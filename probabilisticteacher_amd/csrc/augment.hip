// augment.hip -- weak (crop window, resize, flip) and strong augmentation of the two-crop mapper on the device (gfx950),
// byte-exact with Pillow.
//
// Replaces the PIL / torchvision CPU work the reference does per image in its DataLoader workers:
// pt/data/detection_utils.py:38-60 build_strong_augmentation [RandomApply(ColorJitter(0.4, 0.4, 0.4, 0.1), p=0.8),
// RandomGrayscale(p=0.2), RandomApply(GaussianBlur([0.1, 2.0]), p=0.5), RandomApply(Solarize(0.5), p=0.2)], applied at
// pt/data/dataset_mapper.py:151-159; GaussianBlur / Solarize are pt/data/transforms/augmentation_impl.py:21-53.
// The pixel arithmetic is Pillow's (libImaging Blend.c, Convert.c L24 / rgb2hsv / hsv2rgb, BoxBlur.c), restated in
// oracle/csrc/ref_aug.c, which is pinned against the real Pillow exhaustively over all 2^24 colours.
//
// All kernels are HBM-bound byte kernels over planar uint8 (3, H, W) images (the record format of SURVEY.md 8-a0), batched
// over images through a device descriptor table: blockIdx.y = image, 8 int64 words per image (include/ptmi355.h).
// Compiled with -ffp-contract=off; float / double expression trees mirror the C sources operation for operation.
#include "common.h"

namespace {

__device__ __forceinline__ uint8_t clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : (uint8_t)v); }

__device__ __forceinline__ uint8_t luma(uint8_t r, uint8_t g, uint8_t b)
{
    return (uint8_t)(((uint32_t)r * 19595u + (uint32_t)g * 38470u + (uint32_t)b * 7471u + 0x8000u) >> 16);
}

__device__ __forceinline__ uint8_t blend(uint8_t in1, uint8_t in2, float alpha)
{
    if (alpha >= 0.f && alpha <= 1.0f) return (uint8_t)((int)in1 + alpha * ((int)in2 - (int)in1));
    const float t = (float)((int)in1 + alpha * ((int)in2 - (int)in1));
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (uint8_t)t;
}

__device__ __forceinline__ void rgb2hsv(uint8_t r, uint8_t g, uint8_t b, uint8_t& oh, uint8_t& os, uint8_t& ov)
{
    const uint8_t maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const uint8_t minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    ov = maxc;
    if (minc == maxc) { oh = 0; os = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = ((float)(maxc - r)) / cr, gc = ((float)(maxc - g)) / cr, bc = ((float)(maxc - b)) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + rc - bc);
    else h = (float)(4.0 + gc - rc);
    h = (float)fmod((h / 6.0 + 1.0), 1.0);
    oh = clip8((int)(h * 255.0));
    os = clip8((int)(s * 255.0));
}

__device__ __forceinline__ void hsv2rgb(uint8_t h, uint8_t s, uint8_t v, uint8_t& r, uint8_t& g, uint8_t& b)
{
    if (s == 0) { r = g = b = v; return; }
    const int i = (int)floor((float)h * 6.0 / 255.0);
    const float f = (float)((float)h * 6.0 / 255.0 - (float)i);
    const float fs = (float)(((float)s) / 255.0);
    const int p = (int)round((float)v * (1.0 - fs));
    const int q = (int)round((float)v * (1.0 - fs * f));
    const int t = (int)round((float)v * (1.0 - fs * (1.0 - f)));
    const uint8_t up = clip8(p), uq = clip8(q), ut = clip8(t);
    switch (i % 6) {
        case 0: r = v; g = ut; b = up; break;
        case 1: r = uq; g = v; b = up; break;
        case 2: r = up; g = v; b = ut; break;
        case 3: r = up; g = uq; b = v; break;
        case 4: r = ut; g = up; b = v; break;
        default: r = v; g = up; b = uq; break;
    }
}

// desc words: [0] src, [1] dst, [2] h, [3] w, [4] op, [5] float parameter (bits), [6] integer parameter, [7] unused
// sum of the grey levels of every image (ImageStat of convert("L")): one 64-bit atomic per workgroup
__global__ __launch_bounds__(256) void aug_gray_sum_kernel(const int64_t* __restrict__ desc,
                                                           unsigned long long* __restrict__ sums)
{
    const int64_t* d = desc + 8 * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    const int64_t hw = d[2] * d[3];
    unsigned long long s = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x)
        s += luma(src[i], src[hw + i], src[2 * hw + i]);
    // integer sums: the order of the additions does not matter
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + blockIdx.y, part[0] + part[1] + part[2] + part[3]);
}

enum { OP_COPY = 0, OP_BRIGHTNESS = 1, OP_CONTRAST = 2, OP_SATURATION = 3, OP_HUE = 4, OP_GRAY = 5, OP_SOLARIZE = 6 };

__global__ __launch_bounds__(256) void aug_color_kernel(const int64_t* __restrict__ desc,
                                                        const unsigned long long* __restrict__ sums)
{
    const int64_t* d = desc + 8 * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    uint8_t* dst = (uint8_t*)d[1];
    const int64_t hw = d[2] * d[3];
    const int op = (int)d[4];
    const float f = __int_as_float((int)d[5]);
    int ip = (int)d[6];
    if (op == OP_CONTRAST)      // int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5)
        ip = (int)((double)sums[blockIdx.y] / (double)hw + 0.5);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) {
        uint8_t r = src[i], g = src[hw + i], b = src[2 * hw + i];
        switch (op) {
            case OP_BRIGHTNESS: r = blend(0, r, f); g = blend(0, g, f); b = blend(0, b, f); break;
            case OP_CONTRAST: { const uint8_t m = (uint8_t)ip; r = blend(m, r, f); g = blend(m, g, f); b = blend(m, b, f); break; }
            case OP_SATURATION: { const uint8_t l = luma(r, g, b); r = blend(l, r, f); g = blend(l, g, f); b = blend(l, b, f); break; }
            case OP_HUE: { uint8_t h, s, v; rgb2hsv(r, g, b, h, s, v); h = (uint8_t)(h + (uint8_t)ip); hsv2rgb(h, s, v, r, g, b); break; }
            case OP_GRAY: { const uint8_t l = luma(r, g, b); r = g = b = l; break; }
            case OP_SOLARIZE: r = r < ip ? r : (uint8_t)(255 - r); g = g < ip ? g : (uint8_t)(255 - g); b = b < ip ? b : (uint8_t)(255 - b); break;
            default: break;
        }
        dst[i] = r; dst[hw + i] = g; dst[2 * hw + i] = b;
    }
}

// One pass of Pillow's extended box blur (BoxBlur.c ImagingLineBoxBlur8) along x (vertical = 0) or y (vertical = 1):
//   out[x] = (sum_{|d| <= radius} in[clamp(x + d)] * ww + (in[clamp(x - radius - 1)] + in[clamp(x + radius + 1)]) * fw + 2^23) >> 24
// desc: [4] vertical, [5] radius, [6] ww, [7] fw.  (GaussianBlur sigma in [0.1, 2] gives radius 0 or 1: <= 5 taps.)
__global__ __launch_bounds__(256) void aug_box_blur_kernel(const int64_t* __restrict__ desc)
{
    const int64_t* d = desc + 8 * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    uint8_t* dst = (uint8_t*)d[1];
    const int h = (int)d[2], w = (int)d[3], vertical = (int)d[4], radius = (int)d[5];
    const uint32_t ww = (uint32_t)d[6], fw = (uint32_t)d[7];
    const int64_t hw = (int64_t)h * w, total = 3 * hw;
    const int n = vertical ? h : w, st = vertical ? w : 1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w);
        const int y = (int)((i / w) % h);
        const int pos = vertical ? y : x;
        const uint8_t* line = src + (i - (int64_t)pos * st);
        uint32_t acc = 0;
        for (int k = -radius; k <= radius; ++k) {
            int q = pos + k;
            q = q < 0 ? 0 : (q > n - 1 ? n - 1 : q);
            acc += line[(int64_t)q * st];
        }
        int l = pos - radius - 1, r = pos + radius + 1;
        l = l < 0 ? 0 : l;
        r = r > n - 1 ? n - 1 : r;
        const uint32_t bulk = acc * ww + ((uint32_t)line[(int64_t)l * st] + (uint32_t)line[(int64_t)r * st]) * fw;
        dst[i] = (uint8_t)((bulk + (1u << 23)) >> 24);
    }
}

// horizontal flip (D2 RandomFlip -> HFlipTransform: image[:, ::-1]) of planar images; desc [4] = 1 to flip, 0 to copy
__global__ __launch_bounds__(256) void aug_hflip_kernel(const int64_t* __restrict__ desc)
{
    const int64_t* d = desc + 8 * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    uint8_t* dst = (uint8_t*)d[1];
    const int h = (int)d[2], w = (int)d[3], flip = (int)d[4];
    const int64_t total = 3ll * h * w;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w);
        dst[i] = flip ? src[i - x + (w - 1 - x)] : src[i];
    }
}

// One pass of Pillow's Image.resize(..., BILINEAR) (Resample.c; D2 ResizeTransform of the weak augmentation,
// dataset_mapper.py:107-109) along x (p5 = 0: (3,h,w) -> (3,h,p4)) or y (p5 = 1: (3,h,w) -> (3,p4,w)): triangle filter whose
// support grows with the down-scaling factor, coefficients normalised in double and rounded to 22-bit fixed point, integer
// accumulation from 2^21, >> 22, saturate.  Every thread recomputes the few coefficients of its output column / row with the
// exact double expression tree of precompute_coeffs() (a table kernel would save ALU work nobody is waiting for).
constexpr int RS_PRECISION_BITS = 32 - 8 - 2;
constexpr int RS_MAX_TAPS = 32;             // ksize = 2 * ceil(scale) + 1: down-scaling factors up to 15

__global__ __launch_bounds__(256) void aug_resize_pass_kernel(const int64_t* __restrict__ desc)
{
    const int64_t* d = desc + 8 * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    uint8_t* dst = (uint8_t*)d[1];
    const int h = (int)d[2], w = (int)d[3], outSize = (int)d[4], vertical = (int)d[5];
    const int inSize = vertical ? h : w;
    const int oh = vertical ? outSize : h, ow = vertical ? w : outSize;
    const int64_t total = 3ll * oh * ow;
    double scale = (double)inSize / outSize, filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    const double ss = 1.0 / filterscale;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % ow);
        const int oy = (int)((i / ow) % oh);
        const int c = (int)(i / ((int64_t)ow * oh));
        const int xx = vertical ? oy : ox;
        const double center = 0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > inSize) xmax = inSize;
        xmax -= xmin;
        if (xmax > RS_MAX_TAPS) xmax = RS_MAX_TAPS;        // (rejected on the host)
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            ww += t < 1.0 ? 1.0 - t : 0.0;
        }
        const uint8_t* p = vertical ? src + ((int64_t)c * h + xmin) * w + ox : src + ((int64_t)c * h + oy) * w + xmin;
        const int64_t st = vertical ? w : 1;
        int acc = 1 << (RS_PRECISION_BITS - 1);
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            double v = t < 1.0 ? 1.0 - t : 0.0;
            if (ww != 0.0) v /= ww;
            const int k = v < 0 ? (int)(-0.5 + v * (1 << RS_PRECISION_BITS)) : (int)(0.5 + v * (1 << RS_PRECISION_BITS));
            acc += (int)p[x * st] * k;
        }
        acc >>= RS_PRECISION_BITS;
        dst[i] = acc < 0 ? 0 : (acc > 255 ? 255 : (uint8_t)acc);
    }
}

// ---------------------------------------------------------------- windowed sources: INPUT.CROP of the weak augmentation
// D2 RandomCrop in front of ResizeShortestEdge / RandomFlip (dataset_mapper.py:53-60).  The crop is never materialised: the
// first kernel that touches an image reads a WINDOW of it.  wdesc: 16 int64 words per image (include/ptmi355.h):
//   [0] src = element (0, 0, 0) of the underlying planar image, [1] dst (dense), [2] row pitch, [3] plane pitch (bytes),
//   [4] x0, [5] y0 (window origin), [6] ch, [7] cw (window size), [8] p8, [9] p9, [10..15] unused.
// Both kernels hand every thread four consecutive output bytes of one row (a "quad"; the last quad of a row may be short),
// so a wave writes 256 contiguous bytes; a quad moves as one dword where its address is 4-byte aligned and byte by byte
// where it is not (odd window origins / widths).  The choice is the same for every quad of a row.
enum { WD_WORDS = 16 };

__device__ __forceinline__ uint32_t load_quad(const uint8_t* p, bool wide)
{
    if (wide) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ void store_quad(uint8_t* o, uint32_t v, int n)
{
    if (n == 4 && ((uintptr_t)o & 3) == 0) { *reinterpret_cast<uint32_t*>(o) = v; return; }
    for (int j = 0; j < n; ++j) o[j] = (uint8_t)(v >> (8 * j));
}

// copy (p8 = 0), left-right flip (1: HFlipTransform) or top-bottom flip (2: VFlipTransform) of a window -> dense (3, ch, cw)
__global__ __launch_bounds__(256) void aug_flip_window_kernel(const int64_t* __restrict__ desc)
{
    const int64_t* d = desc + WD_WORDS * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    uint8_t* dst = (uint8_t*)d[1];
    const int64_t pitch = d[2], plane = d[3];
    const int x0 = (int)d[4], y0 = (int)d[5], ch = (int)d[6], cw = (int)d[7], mode = (int)d[8];
    const int qpr = (cw + 3) >> 2;                      // quads per output row
    const int64_t total = 3ll * ch * qpr;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(q % qpr) * 4;
        const int64_t r = q / qpr;                      // output row over the three planes
        const int oy = (int)(r % ch), c = (int)(r / ch);
        const int n = cw - ox < 4 ? cw - ox : 4;
        const int sy = mode == 2 ? ch - 1 - oy : oy;
        const uint8_t* row = src + c * plane + (int64_t)(y0 + sy) * pitch + x0;
        uint32_t v = 0;
        if (n == 4) {
            const uint8_t* p = mode == 1 ? row + (cw - 4 - ox) : row + ox;
            v = load_quad(p, ((uintptr_t)p & 3) == 0);
            if (mode == 1) v = __builtin_bswap32(v);
        } else {
            for (int j = 0; j < n; ++j) v |= (uint32_t)(mode == 1 ? row[cw - 1 - ox - j] : row[ox + j]) << (8 * j);
        }
        store_quad(dst + r * cw + ox, v, n);
    }
}

// Pillow's precompute_coeffs() for output position xx, as aug_resize_pass_kernel evaluates it: the support [xmin, xmin + xmax)
// is clamped to [0, inSize) -- for a window that is the WINDOW's extent, so a resized crop sees no pixel outside the crop --
// and ww is the sum of the triangle weights over it.
struct RsTaps { double center, ww; int xmin, xmax; };

__device__ __forceinline__ RsTaps rs_taps(int xx, double scale, double support, double ss, int inSize)
{
    RsTaps t;
    t.center = 0 + (xx + 0.5) * scale;
    t.xmin = (int)(t.center - support + 0.5);
    if (t.xmin < 0) t.xmin = 0;
    t.xmax = (int)(t.center + support + 0.5);
    if (t.xmax > inSize) t.xmax = inSize;
    t.xmax -= t.xmin;
    if (t.xmax > RS_MAX_TAPS) t.xmax = RS_MAX_TAPS;        // (rejected on the host)
    t.ww = 0.0;
    for (int x = 0; x < t.xmax; ++x) {
        double u = (x + t.xmin - t.center + 0.5) * ss;
        if (u < 0.0) u = -u;
        t.ww += u < 1.0 ? 1.0 - u : 0.0;
    }
    return t;
}

__device__ __forceinline__ int rs_coeff(const RsTaps& t, int x, double ss)
{
    double u = (x + t.xmin - t.center + 0.5) * ss;
    if (u < 0.0) u = -u;
    double v = u < 1.0 ? 1.0 - u : 0.0;
    if (t.ww != 0.0) v /= t.ww;
    return v < 0 ? (int)(-0.5 + v * (1 << RS_PRECISION_BITS)) : (int)(0.5 + v * (1 << RS_PRECISION_BITS));
}

// clip8(acc >> RS_PRECISION_BITS) as a byte to be OR-ed into a quad.  Written as an unsigned shift of max(acc, 0): for the signed
// shift-and-clamp form hipcc pairs two results into one v_ashr_pk_u8_i32 and ORs bytes 2 and 3 onto its result as if the
// upper half were zero; on an MI355X stale bits showed up in byte 2 of the quad (a host build of the same code was exact).
__device__ __forceinline__ uint32_t rs_round(int acc)
{
    const uint32_t u = (uint32_t)(acc < 0 ? 0 : acc) >> RS_PRECISION_BITS;
    return u > 255u ? 255u : u;
}

// aug_resize_pass_kernel's arithmetic on a window: (ch, cw) -> (ch, p8) along x (p9 = 0) or (p8, cw) along y (p9 = 1).  In the
// y pass the four outputs of a quad share their coefficients (one evaluation of the double expression tree per quad) and each
// tap is one dword of the source row where that is aligned; in the x pass every output has its own coefficients and its taps
// are consecutive source bytes that the neighbouring lanes read too.
__global__ __launch_bounds__(256) void aug_resize_window_pass_kernel(const int64_t* __restrict__ desc)
{
    const int64_t* d = desc + WD_WORDS * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    uint8_t* dst = (uint8_t*)d[1];
    const int64_t pitch = d[2], plane = d[3];
    const int x0 = (int)d[4], y0 = (int)d[5], h = (int)d[6], w = (int)d[7], outSize = (int)d[8], vertical = (int)d[9];
    const int inSize = vertical ? h : w;
    const int oh = vertical ? outSize : h, ow = vertical ? w : outSize;
    const int qpr = (ow + 3) >> 2;
    const int64_t total = 3ll * oh * qpr;
    double scale = (double)inSize / outSize, filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    const double ss = 1.0 / filterscale;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(q % qpr) * 4;
        const int64_t r = q / qpr;
        const int oy = (int)(r % oh), c = (int)(r / oh);
        const int n = ow - ox < 4 ? ow - ox : 4;
        const uint8_t* win = src + c * plane + (int64_t)y0 * pitch + x0;       // element (c, 0, 0) of the window
        uint32_t out = 0;
        if (vertical) {
            const RsTaps t = rs_taps(oy, scale, support, ss, inSize);
            const uint8_t* p = win + (int64_t)t.xmin * pitch + ox;
            const bool wide = n == 4 && ((((uintptr_t)p) | (uintptr_t)pitch) & 3) == 0;
            int acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = 1 << (RS_PRECISION_BITS - 1);
            for (int x = 0; x < t.xmax; ++x, p += pitch) {
                const int k = rs_coeff(t, x, ss);
                uint32_t v = 0;
                if (n == 4) v = load_quad(p, wide);
                else for (int j = 0; j < n; ++j) v |= (uint32_t)p[j] << (8 * j);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += (int)((v >> (8 * j)) & 255u) * k;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) out |= rs_round(acc[j]) << (8 * j);
        } else {
            const uint8_t* line = win + (int64_t)oy * pitch;
            for (int j = 0; j < n; ++j) {
                const RsTaps t = rs_taps(ox + j, scale, support, ss, inSize);
                const uint8_t* p = line + t.xmin;
                int acc = 1 << (RS_PRECISION_BITS - 1);
                for (int x = 0; x < t.xmax; ++x) acc += (int)p[x] * rs_coeff(t, x, ss);
                out |= rs_round(acc) << (8 * j);
            }
        }
        store_quad(dst + r * ow + ox, out, n);
    }
}

// ---------------------------------------------------------------- decoded image -> record format
// Pillow hands a decoded image over as packed (H, W, 3) RGB bytes; the records are planar (3, H, W), BGR by default
// (data/datasets.py read_image: arr[:, :, ::-1].transpose(2, 0, 1)).  desc: 8 int64 words per image,
//   [0] src packed (h, w, 3), [1] dst planar (3, h, w), [2] h, [3] w, [4] 0 keeps the channel order / 1 reverses it.
// A thread owns four consecutive pixels of one row: 12 source bytes, as three dwords where the address is 4-byte aligned
// (a wave then reads 768 contiguous bytes) and byte by byte where not or in a row's short last quad, and one quad per plane
// (store_quad: a dword where aligned).  6 bytes of traffic per pixel, no reuse, no LDS.
__global__ __launch_bounds__(256) void aug_unpack_hwc_kernel(const int64_t* __restrict__ desc)
{
    const int64_t* d = desc + 8 * (int64_t)blockIdx.y;
    const uint8_t* src = (const uint8_t*)d[0];
    uint8_t* dst = (uint8_t*)d[1];
    const int h = (int)d[2], w = (int)d[3], reverse = (int)d[4];
    const int qpr = (w + 3) >> 2;                       // quads per row
    const int64_t total = (int64_t)h * qpr, plane = (int64_t)h * w;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(q % qpr) * 4;
        const int64_t y = q / qpr;
        const int n = w - ox < 4 ? w - ox : 4;
        const int64_t pix = y * w + ox;
        const uint8_t* p = src + 3 * pix;
        uint32_t a0 = 0, a1 = 0, a2 = 0;                // source bytes 0..3, 4..7, 8..11
        if (n == 4 && ((uintptr_t)p & 3) == 0) {
            const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
            a0 = p4[0]; a1 = p4[1]; a2 = p4[2];
        } else {
            for (int j = 0; j < 3 * n; ++j) {
                const uint32_t b = (uint32_t)p[j] << (8 * (j & 3));
                if (j < 4) a0 |= b; else if (j < 8) a1 |= b; else a2 |= b;
            }
        }
        const uint32_t c0 = (a0 & 255u) | ((a0 >> 24) << 8) | (((a1 >> 16) & 255u) << 16) | (((a2 >> 8) & 255u) << 24);
        const uint32_t c1 = ((a0 >> 8) & 255u) | ((a1 & 255u) << 8) | ((a1 >> 24) << 16) | (((a2 >> 16) & 255u) << 24);
        const uint32_t c2 = ((a0 >> 16) & 255u) | (((a1 >> 8) & 255u) << 8) | ((a2 & 255u) << 16) | ((a2 >> 24) << 24);
        uint8_t* o = dst + pix;
        store_quad(o, reverse ? c2 : c0, n);
        store_quad(o + plane, c1, n);
        store_quad(o + 2 * plane, reverse ? c0 : c2, n);
    }
}

inline dim3 grid_for(int n, int64_t max_elems)
{
    int64_t bx = (max_elems + 1023) / 1024;
    if (bx > 2048) bx = 2048;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)n);
}

}  // namespace

extern "C" {

int ptmi_aug_gray_sum_batched(const int64_t* desc, int n, int64_t max_hw, uint64_t* sums_out, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(desc && sums_out && n > 0 && n < 65536 && max_hw > 0, "aug_gray_sum_batched: bad args");
    hipStream_t st = (hipStream_t)s;
    hipError_t e = hipMemsetAsync(sums_out, 0, sizeof(uint64_t) * (size_t)n, st);
    if (e != hipSuccess) { ptmi_set_error("aug_gray_sum_batched: memset failed"); return -2; }
    hipLaunchKernelGGL(aug_gray_sum_kernel, grid_for(n, max_hw), dim3(256), 0, st, desc,
                       reinterpret_cast<unsigned long long*>(sums_out));
    PTMI_LAUNCH_CHECK("aug_gray_sum_batched");
    return 0;
}

int ptmi_aug_color_batched(const int64_t* desc, int n, int64_t max_hw, const uint64_t* gray_sums, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(desc && n > 0 && n < 65536 && max_hw > 0, "aug_color_batched: bad args");
    hipLaunchKernelGGL(aug_color_kernel, grid_for(n, max_hw), dim3(256), 0, (hipStream_t)s, desc,
                       reinterpret_cast<const unsigned long long*>(gray_sums));
    PTMI_LAUNCH_CHECK("aug_color_batched");
    return 0;
}

int ptmi_aug_box_blur_batched(const int64_t* desc, int n, int64_t max_elems, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(desc && n > 0 && n < 65536 && max_elems > 0, "aug_box_blur_batched: bad args");
    hipLaunchKernelGGL(aug_box_blur_kernel, grid_for(n, max_elems), dim3(256), 0, (hipStream_t)s, desc);
    PTMI_LAUNCH_CHECK("aug_box_blur_batched");
    return 0;
}

int ptmi_aug_hflip_batched(const int64_t* desc, int n, int64_t max_elems, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(desc && n > 0 && n < 65536 && max_elems > 0, "aug_hflip_batched: bad args");
    hipLaunchKernelGGL(aug_hflip_kernel, grid_for(n, max_elems), dim3(256), 0, (hipStream_t)s, desc);
    PTMI_LAUNCH_CHECK("aug_hflip_batched");
    return 0;
}

int ptmi_aug_resize_pass_batched(const int64_t* desc, int n, int64_t max_out_elems, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(desc && n > 0 && n < 65536 && max_out_elems > 0, "aug_resize_pass_batched: bad args");
    hipLaunchKernelGGL(aug_resize_pass_kernel, grid_for(n, max_out_elems), dim3(256), 0, (hipStream_t)s, desc);
    PTMI_LAUNCH_CHECK("aug_resize_pass_batched");
    return 0;
}

int ptmi_aug_resize_window_pass_batched(const int64_t* wdesc, int n, int64_t max_out_elems, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(wdesc && n > 0 && n < 65536 && max_out_elems > 0, "aug_resize_window_pass_batched: bad args");
    hipLaunchKernelGGL(aug_resize_window_pass_kernel, grid_for(n, max_out_elems), dim3(256), 0, (hipStream_t)s, wdesc);
    PTMI_LAUNCH_CHECK("aug_resize_window_pass_batched");
    return 0;
}

int ptmi_aug_flip_window_batched(const int64_t* wdesc, int n, int64_t max_elems, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(wdesc && n > 0 && n < 65536 && max_elems > 0, "aug_flip_window_batched: bad args");
    hipLaunchKernelGGL(aug_flip_window_kernel, grid_for(n, max_elems), dim3(256), 0, (hipStream_t)s, wdesc);
    PTMI_LAUNCH_CHECK("aug_flip_window_batched");
    return 0;
}

int ptmi_aug_unpack_hwc_batched(const int64_t* desc, int n, int64_t max_pixels, ptmi_stream_t s)
{
    if (n == 0) return 0;
    PTMI_CHECK_ARG(desc && n > 0 && n < 65536 && max_pixels > 0, "aug_unpack_hwc_batched: bad args");
    hipLaunchKernelGGL(aug_unpack_hwc_kernel, grid_for(n, max_pixels), dim3(256), 0, (hipStream_t)s, desc);
    PTMI_LAUNCH_CHECK("aug_unpack_hwc_batched");
    return 0;
}

}  // extern "C"
