// groupnorm.hip -- GroupNorm (+ ReLU) forward and backward for MODEL.VGG.NORM "GN" (D2 get_norm("GN", C) =
// torch.nn.GroupNorm(32, C), eps 1e-5, affine; VGGBlock.forward: relu(norm(conv(x) + b))).  gfx950 only.
//
// NCHW fp32: group (i, g) is ONE contiguous run of L = (C / groups) * HW floats, channel plane (i, ch) one run of HW floats.
// Every kernel is a bandwidth-bound pass; the sums are two-stage with a fixed tree and no atomics:
//
//   forward   gn_stats_chunk_kernel   z -> (mean, M2) of every piece of GN_CHUNK floats of a run.  The piece sits in registers
//                                     (16 floats per thread): sum -> mean, then sum (x - mean)^2 about THAT mean -- no digits
//                                     are lost to a large mean, as sum / sumsq in fp32 would lose them.
//             gn_stats_final_kernel   pieces of a run in piece order, (count, mean, M2) by the parallel-variance formula in
//                                     double (n * groups * pieces numbers) -> mean_rstd.
//             gn_apply_fwd_kernel     y = max((z - mean) * rstd * gamma + beta, 0), one pass.
//   backward  gn_bwd_partial_kernel   per piece of a plane: A = sum g, B = sum g * xhat,  g = dy * (y > 0).
//             gn_bwd_plane_kernel     pieces of a plane in piece order, in double.
//             gn_bwd_final_kernel     dbeta, dgamma (planes in image order), s1 / L, s2 / L per group (channels in order).
//             gn_bwd_apply_kernel     dz = rstd * (g * gamma - (s1 + xhat * s2) / L), one pass.
//
// Lane <-> element assignment of the reducing kernels: element j of a piece goes to thread (j / 4) % 256, slot j / 1024, lane
// component j % 4 -- by a 16-byte load where the piece starts on a 16-byte boundary and the quad is whole, by dwords otherwise
// (a run starts 4-byte aligned only when L is odd).  The assignment, and with it every bit of the result, does not depend on
// the address.  The elementwise kernels take a dword head up to the first 16-byte boundary, 16-byte vectors, a dword tail.
// No lane touches a byte outside its piece.
#include "common.h"

namespace {

constexpr int GN_CHUNK = PTMI_GN_CHUNK;
constexpr int GN_SLOTS = GN_CHUNK / 1024;          // quads per thread
static_assert(GN_CHUNK % 1024 == 0, "a piece is a whole number of 256 x 4 quads");

__device__ __forceinline__ void gn_load4(const float* __restrict__ p, int e, int len, bool vec, float v[4])
{
    if (vec && e + 3 < len) {
        const float4 q = *reinterpret_cast<const float4*>(p + e);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = e + k < len ? p[e + k] : 0.f;
    }
}

__device__ __forceinline__ int gn_piece_len(int64_t total, int piece)
{
    const int64_t left = total - (int64_t)piece * GN_CHUNK;
    return left < GN_CHUNK ? (int)left : GN_CHUNK;
}

__global__ __launch_bounds__(256) void gn_stats_chunk_kernel(const float* __restrict__ z, int64_t L, int pieces,
                                                             float2* __restrict__ part)
{
    __shared__ float sm[4];
    __shared__ float sm_mean;
    const int64_t run = blockIdx.x / (unsigned)pieces;
    const int pc = (int)(blockIdx.x % (unsigned)pieces);
    const float* p = z + run * L + (int64_t)pc * GN_CHUNK;
    const int len = gn_piece_len(L, pc);
    const bool vec = ((uintptr_t)p & 15) == 0;
    float v[GN_SLOTS][4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < GN_SLOTS; ++i) {
        gn_load4(p, 1024 * i + 4 * (int)threadIdx.x, len, vec, v[i]);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float tot = block_sum_256(s, sm);
    if (threadIdx.x == 0) sm_mean = tot / (float)len;
    __syncthreads();
    const float m = sm_mean;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < GN_SLOTS; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = v[i][k] - m;
            q += 1024 * i + 4 * (int)threadIdx.x + k < len ? d * d : 0.f;
        }
    const float m2 = block_sum_256(q, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = make_float2(m, m2);
}

__global__ __launch_bounds__(64) void gn_stats_final_kernel(const float2* __restrict__ part, int64_t L, int pieces,
                                                            int runs, float eps, float* __restrict__ mean_rstd)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= runs) return;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int j = 0; j < pieces; ++j) {
        const float2 pm = part[(int64_t)r * pieces + j];
        const double nb = (double)gn_piece_len(L, j);
        const double d = (double)pm.x - mean, tot = cnt + nb;
        mean += d * (nb / tot);
        m2 += (double)pm.y + d * d * (cnt * nb / tot);
        cnt = tot;
    }
    mean_rstd[2 * (int64_t)r] = (float)mean;
    mean_rstd[2 * (int64_t)r + 1] = (float)(1.0 / sqrt(m2 / (double)L + (double)eps));
}

// what a workgroup of the plane-wise kernels works on: piece `pc` of plane (i, ch), the plane's group statistics
struct GnPiece {
    int64_t off;        // element offset of the piece in the map
    int len, ch;
    int64_t grp;
};

__device__ __forceinline__ GnPiece gn_plane_piece(int C, int cpg, int64_t hw, int pieces)
{
    GnPiece r;
    const int64_t plane = blockIdx.x / (unsigned)pieces;
    const int pc = (int)(blockIdx.x % (unsigned)pieces);
    r.ch = (int)(plane % C);
    r.grp = (plane / C) * (C / cpg) + r.ch / cpg;
    r.off = plane * hw + (int64_t)pc * GN_CHUNK;
    r.len = gn_piece_len(hw, pc);
    return r;
}

// dword head up to the first 16-byte boundary and the number of 16-byte vectors behind it, if every pointer sits at the same
// offset within 16 bytes; else everything is head
__device__ __forceinline__ void gn_split(uintptr_t a, uintptr_t diff, int len, int& head, int& nv)
{
    head = len, nv = 0;
    if ((diff & 15) == 0) {
        head = (int)(((16 - (a & 15)) & 15) >> 2);
        if (head > len) head = len;
        nv = (len - head) >> 2;
    }
}

template <int RELU>
__device__ __forceinline__ float gn_fwd_elem(float z, float mean, float rstd, float ga, float be)
{
    const float y = (z - mean) * rstd * ga + be;
    return RELU ? (y < 0.f ? 0.f : y) : y;       // (a NaN stays a NaN, as torch.relu keeps it: anomaly mode names this layer)
}

template <int RELU>
__global__ __launch_bounds__(256) void gn_apply_fwd_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ mean_rstd, float* __restrict__ y,
                                                           int C, int cpg, int64_t hw, int pieces)
{
    const GnPiece w = gn_plane_piece(C, cpg, hw, pieces);
    const float mean = mean_rstd[2 * w.grp], rstd = mean_rstd[2 * w.grp + 1];
    const float ga = gamma[w.ch], be = beta[w.ch];
    const float* zp = z + w.off;
    float* yp = y + w.off;
    int head, nv;
    gn_split((uintptr_t)zp, (uintptr_t)zp ^ (uintptr_t)yp, w.len, head, nv);
    for (int i = threadIdx.x; i < head; i += 256) yp[i] = gn_fwd_elem<RELU>(zp[i], mean, rstd, ga, be);
    const float4* z4 = reinterpret_cast<const float4*>(zp + head);
    float4* y4 = reinterpret_cast<float4*>(yp + head);
    for (int i = threadIdx.x; i < nv; i += 256) {
        const float4 a = z4[i];
        float4 o;
        o.x = gn_fwd_elem<RELU>(a.x, mean, rstd, ga, be);
        o.y = gn_fwd_elem<RELU>(a.y, mean, rstd, ga, be);
        o.z = gn_fwd_elem<RELU>(a.z, mean, rstd, ga, be);
        o.w = gn_fwd_elem<RELU>(a.w, mean, rstd, ga, be);
        y4[i] = o;
    }
    for (int i = head + 4 * nv + threadIdx.x; i < w.len; i += 256) yp[i] = gn_fwd_elem<RELU>(zp[i], mean, rstd, ga, be);
}

template <int RELU>
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                             const float* __restrict__ z,
                                                             const float* __restrict__ mean_rstd, int C, int cpg,
                                                             int64_t hw, int pieces, float2* __restrict__ part)
{
    __shared__ float sm[4];
    const GnPiece w = gn_plane_piece(C, cpg, hw, pieces);
    const float mean = mean_rstd[2 * w.grp], rstd = mean_rstd[2 * w.grp + 1];
    const float* dp = dy + w.off;
    const float* zp = z + w.off;
    const float* yp = RELU ? y + w.off : nullptr;
    const bool vec = ((((uintptr_t)dp | (uintptr_t)zp) | (RELU ? (uintptr_t)yp : 0)) & 15) == 0;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < GN_SLOTS; ++i) {
        const int e = 1024 * i + 4 * (int)threadIdx.x;
        float d4[4], z4[4], y4[4];
        gn_load4(dp, e, w.len, vec, d4);
        gn_load4(zp, e, w.len, vec, z4);
        if (RELU) gn_load4(yp, e, w.len, vec, y4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = RELU ? (y4[k] > 0.f ? d4[k] : 0.f) : d4[k];
            const float xh = (z4[k] - mean) * rstd;
            a += g;
            b += e + k < w.len ? g * xh : 0.f;
        }
    }
    const float at = block_sum_256(a, sm);
    const float bt = block_sum_256(b, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = make_float2(at, bt);
}

__global__ __launch_bounds__(64) void gn_bwd_plane_kernel(const float2* __restrict__ part, int pieces, int planes,
                                                          double2* __restrict__ ab)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= planes) return;
    double a = 0.0, b = 0.0;
    for (int j = 0; j < pieces; ++j) {
        const float2 v = part[(int64_t)p * pieces + j];
        a += (double)v.x;
        b += (double)v.y;
    }
    ab[p] = make_double2(a, b);
}

// threads [0, C): dbeta / dgamma of a channel (images ascending); threads [C, C + n * G): s1 / L, s2 / L of a group (channels
// ascending)
__global__ __launch_bounds__(64) void gn_bwd_final_kernel(const double2* __restrict__ ab, const float* __restrict__ gamma,
                                                          int n, int C, int cpg, int64_t hw, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, float2* __restrict__ s12)
{
    const int G = C / cpg;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < C) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < n; ++i) {
            const double2 v = ab[(int64_t)i * C + t];
            a += v.x;
            b += v.y;
        }
        dbeta[t] = (float)a;
        dgamma[t] = (float)b;
    } else if (t < C + n * G) {
        const int ng = t - C, i = ng / G, g = ng % G;
        double s1 = 0.0, s2 = 0.0;
        for (int ch = g * cpg; ch < (g + 1) * cpg; ++ch) {
            const double2 v = ab[(int64_t)i * C + ch];
            const double ga = (double)gamma[ch];
            s1 += ga * v.x;
            s2 += ga * v.y;
        }
        const double L = (double)cpg * (double)hw;
        s12[ng] = make_float2((float)(s1 / L), (float)(s2 / L));
    }
}

template <int RELU>
__device__ __forceinline__ float gn_bwd_elem(float dy, float y, float z, float mean, float rstd, float ga, float s1, float s2)
{
    const float g = RELU ? (y > 0.f ? dy : 0.f) : dy;
    const float xh = (z - mean) * rstd;
    return rstd * (g * ga - (s1 + xh * s2));
}

template <int RELU>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ z, const float* __restrict__ gamma,
                                                           const float* __restrict__ mean_rstd,
                                                           const float2* __restrict__ s12, float* __restrict__ dz, int C,
                                                           int cpg, int64_t hw, int pieces)
{
    const GnPiece w = gn_plane_piece(C, cpg, hw, pieces);
    const float mean = mean_rstd[2 * w.grp], rstd = mean_rstd[2 * w.grp + 1];
    const float2 sv = s12[w.grp];
    const float ga = gamma[w.ch], s1 = sv.x, s2 = sv.y;
    const float* dp = dy + w.off;
    const float* zp = z + w.off;
    const float* yp = RELU ? y + w.off : zp;          // (never read without the ReLU)
    float* op = dz + w.off;
    const uintptr_t a0 = (uintptr_t)dp;
    int head, nv;
    gn_split(a0, (a0 ^ (uintptr_t)zp) | (a0 ^ (uintptr_t)yp) | (a0 ^ (uintptr_t)op), w.len, head, nv);
    for (int i = threadIdx.x; i < head; i += 256)
        op[i] = gn_bwd_elem<RELU>(dp[i], RELU ? yp[i] : 0.f, zp[i], mean, rstd, ga, s1, s2);
    const float4* d4 = reinterpret_cast<const float4*>(dp + head);
    const float4* z4 = reinterpret_cast<const float4*>(zp + head);
    const float4* y4 = reinterpret_cast<const float4*>(yp + head);
    float4* o4 = reinterpret_cast<float4*>(op + head);
    for (int i = threadIdx.x; i < nv; i += 256) {
        const float4 d = d4[i], zz = z4[i];
        float4 yy = make_float4(0.f, 0.f, 0.f, 0.f), o;
        if (RELU) yy = y4[i];
        o.x = gn_bwd_elem<RELU>(d.x, yy.x, zz.x, mean, rstd, ga, s1, s2);
        o.y = gn_bwd_elem<RELU>(d.y, yy.y, zz.y, mean, rstd, ga, s1, s2);
        o.z = gn_bwd_elem<RELU>(d.z, yy.z, zz.z, mean, rstd, ga, s1, s2);
        o.w = gn_bwd_elem<RELU>(d.w, yy.w, zz.w, mean, rstd, ga, s1, s2);
        o4[i] = o;
    }
    for (int i = head + 4 * nv + threadIdx.x; i < w.len; i += 256)
        op[i] = gn_bwd_elem<RELU>(dp[i], RELU ? yp[i] : 0.f, zp[i], mean, rstd, ga, s1, s2);
}

inline int64_t al256(int64_t b) { return (b + 255) / 256 * 256; }

// workspace: forward [float2 x runs x run pieces]; backward [float2 x planes x plane pieces | double2 x planes | float2 x runs]
struct GnShape {
    int64_t L, runs, planes, run_pieces, plane_pieces;
    int64_t bwd_ab, bwd_s12, bytes;
};

inline GnShape gn_shape(int n, int c, int64_t hw, int groups)
{
    GnShape s;
    s.L = (int64_t)(c / groups) * hw;
    s.runs = (int64_t)n * groups;
    s.planes = (int64_t)n * c;
    s.run_pieces = cdiv64(s.L, GN_CHUNK);
    s.plane_pieces = cdiv64(hw, GN_CHUNK);
    const int64_t fwd = al256(8 * s.runs * s.run_pieces);
    s.bwd_ab = al256(8 * s.planes * s.plane_pieces);
    s.bwd_s12 = s.bwd_ab + al256(16 * s.planes);
    const int64_t bwd = s.bwd_s12 + al256(8 * s.runs);
    s.bytes = fwd > bwd ? fwd : bwd;
    return s;
}

inline bool gn_dims_ok(int n, int c, int64_t hw, int groups)
{
    return n >= 0 && c > 0 && hw >= 0 && groups > 0 && c % groups == 0;
}

constexpr int64_t GN_MAX_GRID = 0x7FFFFFFFll;

}  // namespace

extern "C" {

int ptmi_gn_chunk(void) { return GN_CHUNK; }

int64_t ptmi_gn_ws_bytes(int n, int c, int64_t hw, int groups)
{
    if (!gn_dims_ok(n, c, hw, groups)) {
        ptmi_set_error("gn_ws_bytes: bad shape n %d c %d hw %lld groups %d (c must be a multiple of groups)", n, c, (long long)hw,
                       groups);
        return -1;
    }
    if (n == 0 || hw == 0) return 256;
    return gn_shape(n, c, hw, groups).bytes;
}

int ptmi_gn_relu_fwd(const float* z, const float* gamma, const float* beta, float* y, float* mean_rstd, int n, int c,
                     int64_t hw, int groups, float eps, int relu, void* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(gn_dims_ok(n, c, hw, groups), "gn_relu_fwd: bad shape n %d c %d hw %lld groups %d (c must be a multiple of "
                   "groups)", n, c, (long long)hw, groups);
    if (n == 0 || hw == 0) return 0;
    PTMI_CHECK_ARG(z && gamma && beta && y && mean_rstd && ws, "gn_relu_fwd: null pointer");
    PTMI_CHECK_ARG(((uintptr_t)ws & 255) == 0 && (((uintptr_t)z | (uintptr_t)y | (uintptr_t)mean_rstd) & 3) == 0,
                   "gn_relu_fwd: misaligned workspace (256 bytes) or tensor (4 bytes)");
    PTMI_CHECK_ARG(eps > 0.f && (relu == 0 || relu == 1), "gn_relu_fwd: eps must be positive, relu 0 or 1");
    const GnShape g = gn_shape(n, c, hw, groups);
    PTMI_CHECK_ARG(g.runs * g.run_pieces <= GN_MAX_GRID && g.planes * g.plane_pieces <= GN_MAX_GRID && g.planes <= GN_MAX_GRID / 2,
                   "gn_relu_fwd: map too large for one launch");
    float2* part = reinterpret_cast<float2*>(ws);
    hipLaunchKernelGGL(gn_stats_chunk_kernel, dim3((unsigned)(g.runs * g.run_pieces)), dim3(256), 0, (hipStream_t)s, z, g.L,
                       (int)g.run_pieces, part);
    PTMI_LAUNCH_CHECK("gn_stats_chunk");
    hipLaunchKernelGGL(gn_stats_final_kernel, dim3((unsigned)cdiv64(g.runs, 64)), dim3(64), 0, (hipStream_t)s, part, g.L,
                       (int)g.run_pieces, (int)g.runs, eps, mean_rstd);
    PTMI_LAUNCH_CHECK("gn_stats_final");
    const dim3 grid((unsigned)(g.planes * g.plane_pieces));
    if (relu)
        hipLaunchKernelGGL(gn_apply_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)s, z, gamma, beta, mean_rstd, y, c,
                           c / groups, hw, (int)g.plane_pieces);
    else
        hipLaunchKernelGGL(gn_apply_fwd_kernel<0>, grid, dim3(256), 0, (hipStream_t)s, z, gamma, beta, mean_rstd, y, c,
                           c / groups, hw, (int)g.plane_pieces);
    PTMI_LAUNCH_CHECK("gn_apply_fwd");
    return 0;
}

int ptmi_gn_relu_bwd(const float* dy, const float* y, const float* z, const float* gamma, const float* mean_rstd,
                     float* dz, float* dgamma, float* dbeta, int n, int c, int64_t hw, int groups, int relu, void* ws,
                     ptmi_stream_t s)
{
    PTMI_CHECK_ARG(gn_dims_ok(n, c, hw, groups), "gn_relu_bwd: bad shape n %d c %d hw %lld groups %d (c must be a multiple of "
                   "groups)", n, c, (long long)hw, groups);
    if (n == 0 || hw == 0) return 0;
    PTMI_CHECK_ARG(relu == 0 || relu == 1, "gn_relu_bwd: relu must be 0 or 1");
    PTMI_CHECK_ARG(dy && z && gamma && mean_rstd && dz && dgamma && dbeta && ws && (y || !relu), "gn_relu_bwd: null pointer");
    PTMI_CHECK_ARG(((uintptr_t)ws & 255) == 0 && (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)z | (uintptr_t)dz) & 3) == 0,
                   "gn_relu_bwd: misaligned workspace (256 bytes) or tensor (4 bytes)");
    const GnShape g = gn_shape(n, c, hw, groups);
    PTMI_CHECK_ARG(g.planes * g.plane_pieces <= GN_MAX_GRID && g.planes <= GN_MAX_GRID / 2, "gn_relu_bwd: map too large for one launch");
    char* base = reinterpret_cast<char*>(ws);
    float2* part = reinterpret_cast<float2*>(base);
    double2* ab = reinterpret_cast<double2*>(base + g.bwd_ab);
    float2* s12 = reinterpret_cast<float2*>(base + g.bwd_s12);
    const dim3 grid((unsigned)(g.planes * g.plane_pieces));
    const int cpg = c / groups, pieces = (int)g.plane_pieces;
    if (relu)
        hipLaunchKernelGGL(gn_bwd_partial_kernel<1>, grid, dim3(256), 0, (hipStream_t)s, dy, y, z, mean_rstd, c, cpg, hw, pieces,
                           part);
    else
        hipLaunchKernelGGL(gn_bwd_partial_kernel<0>, grid, dim3(256), 0, (hipStream_t)s, dy, y, z, mean_rstd, c, cpg, hw, pieces,
                           part);
    PTMI_LAUNCH_CHECK("gn_bwd_partial");
    hipLaunchKernelGGL(gn_bwd_plane_kernel, dim3((unsigned)cdiv64(g.planes, 64)), dim3(64), 0, (hipStream_t)s, part, pieces,
                       (int)g.planes, ab);
    PTMI_LAUNCH_CHECK("gn_bwd_plane");
    hipLaunchKernelGGL(gn_bwd_final_kernel, dim3((unsigned)cdiv64(c + g.runs, 64)), dim3(64), 0, (hipStream_t)s, ab, gamma, n, c,
                       cpg, hw, dgamma, dbeta, s12);
    PTMI_LAUNCH_CHECK("gn_bwd_final");
    if (relu)
        hipLaunchKernelGGL(gn_bwd_apply_kernel<1>, grid, dim3(256), 0, (hipStream_t)s, dy, y, z, gamma, mean_rstd, s12, dz, c,
                           cpg, hw, pieces);
    else
        hipLaunchKernelGGL(gn_bwd_apply_kernel<0>, grid, dim3(256), 0, (hipStream_t)s, dy, y, z, gamma, mean_rstd, s12, dz, c,
                           cpg, hw, pieces);
    PTMI_LAUNCH_CHECK("gn_bwd_apply");
    return 0;
}

}  // extern "C"
