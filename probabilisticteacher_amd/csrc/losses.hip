// losses.hip -- fused loss + gradient kernels of the Probabilistic-Teacher step (gfx950).
//
// Each kernel evaluates one loss term of the reference AND its gradient w.r.t. the network outputs in a
// single pass (the autograd wrapper only scales by the upstream scalar).  Per-workgroup partial sums
// use wave64 shuffles + LDS, and a single-workgroup finaliser adds the partials in a fixed order, so
// the scalar losses are bitwise reproducible run to run.
//
//   bce_logits_sum      pt/modeling/proposal_generator/rpn.py:242-246
//   gaussian_nll_sum    pt/modeling/box_regression.py:33-35,165-176; pt/modeling/roi_heads/fast_rcnn.py:286-296
//   softmax_ce_mean     D2 FastRCNNOutputLayers.losses, fast_rcnn.py:408 (softmax)
//   soft_ce_efl         fast_rcnn.py:179-213
//   rpn_soft_obj_loss   rpn.py:285-304  (keeps the sigmoid(1-x) quirk of :299)
//   kl_efl_loss         rpn.py:321-355, fast_rcnn.py:215-263
//   laplace_nll_sum     box_regression.py:38-40,177-183; fast_rcnn.py:298-307       (UNSUPNET.MODEL_TYPE = LAPLACE)
//   laplace_kl_efl_loss rpn.py:319-344, fast_rcnn.py:238-257                         (UNSUPNET.MODEL_TYPE = LAPLACE)
//
// and the integer counters behind the logged training statistics (no loss, no gradient):
//   cls_stats           D2 0.5 _log_classification_stats, reached from FastRCNNOutputLayers.losses
//   label_counts        rpn.py:222-228
#include "common.h"

namespace {

constexpr int MAXB = 1024;        // partial slots
constexpr int WS_SUM = 0, WS_CNT = 1024, WS_SCALE = 2048;
constexpr float PI_F = 3.14159265358979323846f;
constexpr float E_F = 2.71828182845904523536f;

inline int blocks_for(int64_t n)
{
    int64_t b = (n + 255) / 256;
    if (b > MAXB) b = MAXB;
    if (b < 1) b = 1;
    return (int)b;
}

__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ ws, int nb, float scale, int mean_mode,
                                                       float* __restrict__ loss_out, float* __restrict__ ws_scale)
{
    __shared__ float sm[4];
    float a = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) {
        a += ws[WS_SUM + i];
        if (mean_mode) c += ws[WS_CNT + i];
    }
    const float ta = block_sum_256(a, sm);
    const float tc = block_sum_256(c, sm);
    if (threadIdx.x == 0) {
        if (mean_mode) {
            // mean over (selected rows x 4); 0/0 -> NaN exactly like torch's mean of an empty tensor
            const float denom = tc * 4.0f;
            loss_out[0] = ta / denom;
            ws_scale[0] = 1.0f / denom;
        } else {
            loss_out[0] = ta * scale;
        }
    }
}

__global__ void scale_rows_kernel(float* __restrict__ g, int64_t n, const float* __restrict__ sc)
{
    const float s = sc[0];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        g[i] *= s;
}

// ------------------------------------------------------------------------------------------ BCE
__global__ __launch_bounds__(256) void bce_kernel(const float* __restrict__ x, const int8_t* __restrict__ lab,
                                                  int64_t n, float inv_norm, float* __restrict__ dx,
                                                  float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int l = lab[i];
        float g = 0.f;
        if (l >= 0) {
            const float v = x[i], t = (float)l;
            // ATen binary_cross_entropy_with_logits: (1-t)*x + max(-x,0) + log(exp(-max) + exp(-x-max))
            const float mx = fmaxf(-v, 0.f);
            acc += (1.f - t) * v + mx + logf(expf(-mx) + expf(-v - mx));
            g = (sigmoidf_(v) - t) * inv_norm;
        }
        dx[i] = g;
    }
    const float t = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[WS_SUM + blockIdx.x] = t;
}

// ------------------------------------------------------------------------------------------ Gaussian NLL
__global__ __launch_bounds__(256) void gnll_kernel(const float* __restrict__ d, const float* __restrict__ tg,
                                                   int64_t rows, float inv_norm, float* __restrict__ dd,
                                                   float* __restrict__ dt, float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f;
    const int64_t total = rows * 4;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i >> 2;
        const int c = (int)(i & 3);
        const float mu = d[r * 8 + c], sl = d[r * 8 + 4 + c], t = tg[i];
        const float var = sigmoidf_(sl);
        const float diff = mu - t;
        const float e = diff * diff;
        const float A = expf(-e / (var + 1e-9f) / 2.0f);
        const float B = sqrtf(2.0f * PI_F * (var + 0.3f));
        const float pdf = A / B;
        acc += -logf(pdf + 1e-9f);
        const float dL_dpdf = -1.f / (pdf + 1e-9f);
        const float dpdf_dmu = pdf * (-diff / (var + 1e-9f));
        const float dpdf_dvar = pdf * (e / (2.f * (var + 1e-9f) * (var + 1e-9f)) - 1.f / (2.f * (var + 0.3f)));
        const float gmu = dL_dpdf * dpdf_dmu * inv_norm;
        dd[r * 8 + c] = gmu;
        dd[r * 8 + 4 + c] = dL_dpdf * dpdf_dvar * var * (1.f - var) * inv_norm;
        if (dt) dt[i] = -gmu;
    }
    const float t = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[WS_SUM + blockIdx.x] = t;
}

// ------------------------------------------------------------------------------------------ softmax CE (mean)
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                         int64_t R, int C, float inv_r, float* __restrict__ dx,
                                                         float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f;
    for (int64_t r = blockIdx.x * 256ll + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
        const float* p = x + r * C;
        float m = p[0];
        for (int j = 1; j < C; ++j) m = fmaxf(m, p[j]);
        float s = 0.f;
        for (int j = 0; j < C; ++j) s += expf(p[j] - m);
        const float ls = logf(s);
        const int t = (int)tgt[r];
        acc += -(p[t] - m - ls);
        for (int j = 0; j < C; ++j) {
            const float sj = expf(p[j] - m - ls);
            dx[r * C + j] = (sj - (j == t ? 1.f : 0.f)) * inv_r;
        }
    }
    const float t = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[WS_SUM + blockIdx.x] = t;
}

__global__ void softmax_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t R, int C)
{
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        const float* p = x + r * C;
        float m = p[0];
        for (int j = 1; j < C; ++j) m = fmaxf(m, p[j]);
        float s = 0.f;
        for (int j = 0; j < C; ++j) s += expf(p[j] - m);
        for (int j = 0; j < C; ++j) y[r * C + j] = expf(p[j] - m) / s;
    }
}

// entropy-focal weight of one teacher row: (1 - H(softmax T)/log C)^lambda   (0*log0 -> NaN kept).
// ONE deliberate deviation from the literal expression (round 6): for a near-uniform row the exact base 1 - H/log C is >= 0 but of the
// size of the rounding of the device's expf / logf (|logit gap| < ~1e-3: a few 1e-8), so it can come out as -6e-8, and a negative base to
// the power lambda = 0.5 is NaN -- it killed one of 24 loss-curve trajectories at iteration 452 (teacher logits (x, x + d), both cls
// terms NaN, every other term finite; profiles/r06_loss_curves_v5.txt).  The reference's `(1 - entropy / max_entropy) ** weight_lambda`
// (fast_rcnn.py:199-200, rpn.py:288-290) has the same hazard with ITS libm's rounding; a base below zero is clamped to the exact
// expression's limit, 0.  A NaN base (0 * log 0 at extreme confidence) still propagates.
__device__ __forceinline__ float efl_weight(const float* __restrict__ T, int C, float lambda)
{
    float m = T[0];
    for (int j = 1; j < C; ++j) m = fmaxf(m, T[j]);
    float s = 0.f;
    for (int j = 0; j < C; ++j) s += expf(T[j] - m);
    float H = 0.f;
    for (int j = 0; j < C; ++j) {
        const float p = expf(T[j] - m) / s;
        H += p * logf(p);
    }
    H = -H;
    const float base = 1.f - H / logf((float)C);
    return powf(base < 0.f ? 0.f : base, lambda);
}

// ------------------------------------------------------------------------------------------ soft CE + EFL (ROI)
__global__ __launch_bounds__(256) void soft_ce_efl_kernel(const float* __restrict__ T, const float* __restrict__ S,
                                                          int64_t R, int C, float tau, float lambda, int efl,
                                                          float inv_norm, float* __restrict__ dS,
                                                          float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f;
    for (int64_t r = blockIdx.x * 256ll + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
        const float* t = T + r * C;
        const float* s = S + r * C;
        const float w = efl ? efl_weight(t, C, lambda) : 1.f;
        // q = softmax(t / tau)
        float mq = t[0] / tau;
        for (int j = 1; j < C; ++j) mq = fmaxf(mq, t[j] / tau);
        float sq = 0.f;
        for (int j = 0; j < C; ++j) sq += expf(t[j] / tau - mq);
        // log_softmax(s)
        float ms = s[0];
        for (int j = 1; j < C; ++j) ms = fmaxf(ms, s[j]);
        float ss = 0.f;
        for (int j = 0; j < C; ++j) ss += expf(s[j] - ms);
        const float ls = logf(ss);
        float l = 0.f;
        for (int j = 0; j < C; ++j) {
            const float q = expf(t[j] / tau - mq) / sq * w;     // soft_label * weight (fast_rcnn.py:204-206)
            const float lsm = s[j] - ms - ls;
            l += q * (-lsm);
        }
        acc += l;
        // d/ds_j of sum_i qw_i * (-log_softmax(s)_i) = softmax(s)_j * sum_i qw_i - qw_j ; sum_i q_i = 1
        for (int j = 0; j < C; ++j) {
            const float q = expf(t[j] / tau - mq) / sq;
            const float pj = expf(s[j] - ms - ls);
            dS[r * C + j] = w * (pj - q) * inv_norm;
        }
    }
    const float t = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[WS_SUM + blockIdx.x] = t;
}

// ------------------------------------------------------------------------------------------ RPN soft objectness
__global__ __launch_bounds__(256) void rpn_soft_obj_kernel(const float* __restrict__ T, const float* __restrict__ x,
                                                           int64_t K, int C, float tau, float lambda, int efl,
                                                           float inv_norm, float* __restrict__ dx,
                                                           uint8_t* __restrict__ fg, float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f;
    for (int64_t r = blockIdx.x * 256ll + threadIdx.x; r < K; r += (int64_t)gridDim.x * 256) {
        const float* t = T + r * C;
        const float w = efl ? efl_weight(t, C, lambda) : 1.f;
        int am = 0;
        float mv = t[0];
        for (int j = 1; j < C; ++j)
            if (t[j] > mv) { mv = t[j]; am = j; }
        fg[r] = (uint8_t)(am != C - 1);
        float mq = t[0] / tau;
        for (int j = 1; j < C; ++j) mq = fmaxf(mq, t[j] / tau);
        float sq = 0.f;
        for (int j = 0; j < C; ++j) sq += expf(t[j] / tau - mq);
        float qfg = 0.f;
        for (int j = 0; j < C - 1; ++j) qfg += expf(t[j] / tau - mq) / sq;
        const float qbg = expf(t[C - 1] / tau - mq) / sq;
        const float v = x[r];
        const float sb = sigmoidf_(1.f - v), sf = sigmoidf_(v);      // rpn.py:299 (sic)
        const float nlb = -logf(sb + 1e-9f), nlf = -logf(sf + 1e-9f);
        acc += (qbg * w) * nlb + (qfg * w) * nlf;
        const float dnlb = sb * (1.f - sb) / (sb + 1e-9f);            // d(-log(sig(1-x)+eps))/dx
        const float dnlf = -sf * (1.f - sf) / (sf + 1e-9f);
        dx[r] = w * (qbg * dnlb + qfg * dnlf) * inv_norm;
    }
    const float t = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[WS_SUM + blockIdx.x] = t;
}

// ------------------------------------------------------------------------------------------ KL + EFL
__global__ __launch_bounds__(256) void kl_efl_kernel(const float* __restrict__ q, const float* __restrict__ mup,
                                                     const float* __restrict__ slp, const uint8_t* __restrict__ fg,
                                                     int64_t rows, float tau, float lambda, int efl, float gscale,
                                                     float* __restrict__ dq, float* __restrict__ dmup,
                                                     float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f, cnt = 0.f;
    const int64_t total = rows * 4;
    const float max_ent = 0.5f * logf(2.f * PI_F * E_F);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i >> 2;
        const int c = (int)(i & 3);
        float gmu = 0.f, gsl = 0.f;
        if (!fg || fg[r]) {
            const float var_p0 = sigmoidf_(slp[i]);
            float w = 1.f;
            if (efl) {
                const float ent = 0.5f * logf(2.f * PI_F * E_F * var_p0);
                w = powf(1.f - ent / max_ent, lambda);
            }
            const float var_p = var_p0 * tau;
            const float var_q = sigmoidf_(q[r * 8 + 4 + c]);
            const float diff = q[r * 8 + c] - mup[i];
            const float kl = 0.5f * logf(var_q / var_p) - 0.5f + (var_p + diff * diff) / (2.f * var_q);
            acc += kl * w;
            if (c == 0) cnt += 1.f;
            gmu = w * diff / var_q * gscale;
            const float dvq = w * (0.5f / var_q - (var_p + diff * diff) / (2.f * var_q * var_q));
            gsl = dvq * var_q * (1.f - var_q) * gscale;
        }
        dq[r * 8 + c] = gmu;
        dq[r * 8 + 4 + c] = gsl;
        if (dmup) dmup[i] = -gmu;
    }
    const float t = block_sum_256(acc, sm);
    const float tc = block_sum_256(cnt, sm);
    if (threadIdx.x == 0) {
        ws[WS_SUM + blockIdx.x] = t;
        ws[WS_CNT + blockIdx.x] = tc;
    }
}

// ------------------------------------------------------------------------------------------ Laplace (UNSUPNET.MODEL_TYPE = LAPLACE)
// The gradients are those of the reference expressions as written (+1e-9 terms included); sign(0) = 0, what torch's abs
// backward gives.
__device__ __forceinline__ float signf_(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// -log(laplace_dist_pdf(mu; t, var) + 1e-9), var = sigmoid(slog)   (box_regression.py:38-40; row layout of gnll_kernel)
__global__ __launch_bounds__(256) void lnll_kernel(const float* __restrict__ d, const float* __restrict__ tg,
                                                   int64_t rows, float inv_norm, float* __restrict__ dd,
                                                   float* __restrict__ dt, float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f;
    const int64_t total = rows * 4;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i >> 2;
        const int c = (int)(i & 3);
        const float mu = d[r * 8 + c], sl = d[r * 8 + 4 + c], t = tg[i];
        const float var = sigmoidf_(sl);
        const float diff = mu - t;
        const float ad = fabsf(diff);
        const float a = sqrtf(var + 1e-9f);
        const float pdf = expf(-ad / a) / sqrtf(4.0f * (var + 0.3f));
        acc += -logf(pdf + 1e-9f);
        const float gp = -1.f / (pdf + 1e-9f) * pdf;                     // dL/dpdf * pdf
        const float gmu = gp * (-signf_(diff) / a) * inv_norm;
        dd[r * 8 + c] = gmu;
        dd[r * 8 + 4 + c] = gp * (ad / (2.f * a * a * a) - 1.f / (2.f * (var + 0.3f))) * var * (1.f - var) * inv_norm;
        if (dt) dt[i] = -gmu;
    }
    const float t = block_sum_256(acc, sm);
    if (threadIdx.x == 0) ws[WS_SUM + blockIdx.x] = t;
}

// Laplace KL(p || q) with the Laplace entropy-focal weight (rpn.py:319-344, fast_rcnn.py:238-257); selection, reduction and
// gscale exactly as kl_efl_kernel.  The entropy base is not clamped (neither the reference nor kl_efl_kernel clamps it).
__global__ __launch_bounds__(256) void lkl_efl_kernel(const float* __restrict__ q, const float* __restrict__ mup,
                                                      const float* __restrict__ slp, const uint8_t* __restrict__ fg,
                                                      int64_t rows, float tau, float lambda, int efl, float gscale,
                                                      float* __restrict__ dq, float* __restrict__ dmup,
                                                      float* __restrict__ ws)
{
    __shared__ float sm[4];
    float acc = 0.f, cnt = 0.f;
    const int64_t total = rows * 4;
    const float max_ent = 1.f + logf(2.f);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i >> 2;
        const int c = (int)(i & 3);
        float gmu = 0.f, gsl = 0.f;
        if (!fg || fg[r]) {
            const float var_p0 = sigmoidf_(slp[i]);
            float w = 1.f;
            if (efl) {
                const float ent = 1.f + 0.5f * logf(4.f * var_p0);
                w = powf(1.f - ent / max_ent, lambda);
            }
            const float var_p = var_p0 * tau;
            const float var_q = sigmoidf_(q[r * 8 + 4 + c]);
            const float rp = sqrtf(var_p), rq = sqrtf(var_q);
            const float diff = q[r * 8 + c] - mup[i];
            const float ad = fabsf(diff);
            const float E = expf(-ad / rp);
            const float kl = rp * E / rq + ad / rq + 0.5f * logf(var_q / var_p) - 1.f;
            acc += kl * w;
            if (c == 0) cnt += 1.f;
            gmu = w * signf_(diff) * (1.f - E) / rq * gscale;
            const float rq3 = rq * rq * rq;
            const float dvq = w * (-0.5f * rp * E / rq3 - 0.5f * ad / rq3 + 0.5f / var_q);
            gsl = dvq * var_q * (1.f - var_q) * gscale;
        }
        dq[r * 8 + c] = gmu;
        dq[r * 8 + 4 + c] = gsl;
        if (dmup) dmup[i] = -gmu;
    }
    const float t = block_sum_256(acc, sm);
    const float tc = block_sum_256(cnt, sm);
    if (threadIdx.x == 0) {
        ws[WS_SUM + blockIdx.x] = t;
        ws[WS_CNT + blockIdx.x] = tc;
    }
}

// ------------------------------------------------------------------------------------------ statistics (integer counts)
// Sums of N int counters over a 256-thread block, stored by threads 0 .. N-1 to out[0 .. N-1].  smem: 4 N ints.
// Integer addition: the result does not depend on the order, so neither does anything derived from it.
template <int N>
__device__ __forceinline__ void block_counts_store(const int (&c)[N], int* smem, int32_t* __restrict__ out)
{
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int v = c[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) smem[(threadIdx.x >> 6) * N + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N)
        out[threadIdx.x] = (smem[threadIdx.x] + smem[N + threadIdx.x]) + (smem[2 * N + threadIdx.x] + smem[3 * N + threadIdx.x]);
}

// ws[block][4] = (argmax == gt, gt foreground, foreground and argmax == gt, foreground and argmax == background) over the
// block's rows.  One thread per row, as softmax_ce_kernel; the strict > keeps the lowest index among equal maxima.  gt is only
// compared, never used as an index.
__global__ __launch_bounds__(256) void cls_stats_kernel(const float* __restrict__ x, const int64_t* __restrict__ gt,
                                                        int64_t R, int C, int32_t* __restrict__ ws)
{
    __shared__ int sm[16];
    int c[4] = {0, 0, 0, 0};
    const int K = C - 1;
    for (int64_t r = blockIdx.x * 256ll + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
        const float* p = x + r * C;
        float m = p[0];
        int am = 0;
        for (int j = 1; j < C; ++j) {
            const float v = p[j];
            if (v > m) { m = v; am = j; }
        }
        const int64_t g = gt[r];
        const bool fg = g >= 0 && g < K, hit = (int64_t)am == g;
        c[0] += hit;
        c[1] += fg;
        c[2] += fg && hit;
        c[3] += fg && am == K;
    }
    block_counts_store<4>(c, sm, ws + 4 * (int64_t)blockIdx.x);
}

// ws[block][2] = (labels == 1, labels == 0) over the block's share
__global__ __launch_bounds__(256) void label_counts_kernel(const int8_t* __restrict__ lab, int64_t n,
                                                           int32_t* __restrict__ ws)
{
    __shared__ int sm[8];
    int c[2] = {0, 0};
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int l = lab[i];
        c[0] += l == 1;
        c[1] += l == 0;
    }
    block_counts_store<2>(c, sm, ws + 2 * (int64_t)blockIdx.x);
}

// out[0 .. N-1] = the sum of the nb block rows of ws; nb == 0 writes zeros
template <int N>
__global__ __launch_bounds__(256) void counts_final_kernel(const int32_t* __restrict__ ws, int nb, int32_t* __restrict__ out)
{
    __shared__ int sm[4 * N];
    int c[N];
#pragma unroll
    for (int k = 0; k < N; ++k) c[k] = 0;
    for (int i = threadIdx.x; i < nb; i += 256) {
#pragma unroll
        for (int k = 0; k < N; ++k) c[k] += ws[N * i + k];
    }
    block_counts_store<N>(c, sm, out);
}

int finalize(float* ws, int nb, float scale, int mean_mode, float* loss_out, hipStream_t st, const char* name)
{
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, st, ws, nb, scale, mean_mode, loss_out, ws + WS_SCALE);
    PTMI_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace

extern "C" {

int ptmi_bce_logits_sum(const float* logits, const int8_t* labels, int64_t n, float inv_norm, float* loss_out,
                        float* dlogits, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && n >= 0, "bce_logits_sum: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(n);
    if (n > 0) {
        PTMI_CHECK_ARG(logits && labels && dlogits, "bce_logits_sum: null buffer");
        hipLaunchKernelGGL(bce_kernel, dim3(nb), dim3(256), 0, st, logits, labels, n, inv_norm, dlogits, ws);
        PTMI_LAUNCH_CHECK("bce_logits_sum");
    }
    return finalize(ws, n > 0 ? nb : 0, inv_norm, 0, loss_out, st, "bce_finalize");
}

int ptmi_gaussian_nll_sum(const float* d, const float* t, int64_t rows, float inv_norm, float* loss_out, float* dd,
                          float* dt, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && rows >= 0, "gaussian_nll_sum: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(rows * 4);
    if (rows > 0) {
        PTMI_CHECK_ARG(d && t && dd, "gaussian_nll_sum: null buffer");
        hipLaunchKernelGGL(gnll_kernel, dim3(nb), dim3(256), 0, st, d, t, rows, inv_norm, dd, dt, ws);
        PTMI_LAUNCH_CHECK("gaussian_nll_sum");
    }
    return finalize(ws, rows > 0 ? nb : 0, inv_norm, 0, loss_out, st, "gnll_finalize");
}

int ptmi_softmax_ce_mean(const float* logits, const int64_t* target, int64_t r, int c, float* loss_out,
                         float* dlogits, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && r >= 0 && c > 0, "softmax_ce_mean: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(r);
    const float inv_r = r > 0 ? 1.0f / (float)r : 0.f;
    if (r > 0) {
        PTMI_CHECK_ARG(logits && target && dlogits, "softmax_ce_mean: null buffer");
        hipLaunchKernelGGL(softmax_ce_kernel, dim3(nb), dim3(256), 0, st, logits, target, r, c, inv_r, dlogits, ws);
        PTMI_LAUNCH_CHECK("softmax_ce_mean");
    }
    return finalize(ws, r > 0 ? nb : 0, inv_r, 0, loss_out, st, "ce_finalize");   // r == 0 -> 0 (D2 cross_entropy)
}

int ptmi_softmax_rows(const float* logits, float* probs, int64_t r, int c, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(r >= 0 && c > 0, "softmax_rows: bad args");
    if (r == 0) return 0;
    PTMI_CHECK_ARG(logits && probs, "softmax_rows: null buffer");
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(blocks_for(r)), dim3(256), 0, (hipStream_t)s, logits, probs, r, c);
    PTMI_LAUNCH_CHECK("softmax_rows");
    return 0;
}

int ptmi_soft_ce_efl(const float* t, const float* s_logits, int64_t r, int c, float tau, float lambda, int efl,
                     float inv_norm, float* loss_out, float* ds, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && r >= 0 && c > 0, "soft_ce_efl: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(r);
    if (r > 0) {
        PTMI_CHECK_ARG(t && s_logits && ds, "soft_ce_efl: null buffer");
        hipLaunchKernelGGL(soft_ce_efl_kernel, dim3(nb), dim3(256), 0, st, t, s_logits, r, c, tau, lambda, efl, inv_norm,
                           ds, ws);
        PTMI_LAUNCH_CHECK("soft_ce_efl");
    }
    return finalize(ws, r > 0 ? nb : 0, inv_norm, 0, loss_out, st, "soft_ce_finalize");
}

int ptmi_rpn_soft_obj_loss(const float* t, const float* x, int64_t k, int c, float tau, float lambda, int efl,
                           float inv_norm, float* loss_out, float* dx, uint8_t* fg, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && k >= 0 && c > 1, "rpn_soft_obj_loss: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(k);
    if (k > 0) {
        PTMI_CHECK_ARG(t && x && dx && fg, "rpn_soft_obj_loss: null buffer");
        hipLaunchKernelGGL(rpn_soft_obj_kernel, dim3(nb), dim3(256), 0, st, t, x, k, c, tau, lambda, efl, inv_norm, dx,
                           fg, ws);
        PTMI_LAUNCH_CHECK("rpn_soft_obj_loss");
    }
    return finalize(ws, k > 0 ? nb : 0, inv_norm, 0, loss_out, st, "rpn_soft_obj_finalize");
}

int ptmi_kl_efl_loss(const float* q, const float* mu_p, const float* slog_p, const uint8_t* fg, int64_t rows,
                     float tau, float lambda, int efl, int reduction, float inv_norm, float* loss_out, float* dq,
                     float* dmu_p, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && rows >= 0 && (reduction == 0 || reduction == 1), "kl_efl_loss: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(rows * 4);
    if (rows > 0) {
        PTMI_CHECK_ARG(q && mu_p && slog_p && dq, "kl_efl_loss: null buffer");
        hipLaunchKernelGGL(kl_efl_kernel, dim3(nb), dim3(256), 0, st, q, mu_p, slog_p, fg, rows, tau, lambda, efl,
                           reduction == 0 ? inv_norm : 1.0f, dq, dmu_p, ws);
        PTMI_LAUNCH_CHECK("kl_efl_loss");
    } else {
        hipError_t e = hipMemsetAsync(ws, 0, sizeof(float) * 2049, st);
        if (e != hipSuccess) { ptmi_set_error("kl_efl_loss: memset failed"); return -2; }
    }
    const int rc = finalize(ws, rows > 0 ? nb : 0, inv_norm, reduction, loss_out, st, "kl_finalize");
    if (rc) return rc;
    if (reduction == 1 && rows > 0) {
        hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for(rows * 8)), dim3(256), 0, st, dq, rows * 8, ws + WS_SCALE);
        PTMI_LAUNCH_CHECK("kl_scale");
        if (dmu_p) {
            hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for(rows * 4)), dim3(256), 0, st, dmu_p, rows * 4,
                               ws + WS_SCALE);
            PTMI_LAUNCH_CHECK("kl_scale_mu");
        }
    }
    return 0;
}

int ptmi_laplace_nll_sum(const float* d, const float* t, int64_t rows, float inv_norm, float* loss_out, float* dd,
                         float* dt, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && rows >= 0, "laplace_nll_sum: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(rows * 4);
    if (rows > 0) {
        PTMI_CHECK_ARG(d && t && dd, "laplace_nll_sum: null buffer");
        hipLaunchKernelGGL(lnll_kernel, dim3(nb), dim3(256), 0, st, d, t, rows, inv_norm, dd, dt, ws);
        PTMI_LAUNCH_CHECK("laplace_nll_sum");
    }
    return finalize(ws, rows > 0 ? nb : 0, inv_norm, 0, loss_out, st, "lnll_finalize");
}

int ptmi_laplace_kl_efl_loss(const float* q, const float* mu_p, const float* slog_p, const uint8_t* fg, int64_t rows,
                             float tau, float lambda, int efl, int reduction, float inv_norm, float* loss_out, float* dq,
                             float* dmu_p, float* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(loss_out && ws && rows >= 0 && (reduction == 0 || reduction == 1), "laplace_kl_efl_loss: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = blocks_for(rows * 4);
    if (rows > 0) {
        PTMI_CHECK_ARG(q && mu_p && slog_p && dq, "laplace_kl_efl_loss: null buffer");
        hipLaunchKernelGGL(lkl_efl_kernel, dim3(nb), dim3(256), 0, st, q, mu_p, slog_p, fg, rows, tau, lambda, efl,
                           reduction == 0 ? inv_norm : 1.0f, dq, dmu_p, ws);
        PTMI_LAUNCH_CHECK("laplace_kl_efl_loss");
    } else {
        hipError_t e = hipMemsetAsync(ws, 0, sizeof(float) * 2049, st);
        if (e != hipSuccess) { ptmi_set_error("laplace_kl_efl_loss: memset failed"); return -2; }
    }
    const int rc = finalize(ws, rows > 0 ? nb : 0, inv_norm, reduction, loss_out, st, "lkl_finalize");
    if (rc) return rc;
    if (reduction == 1 && rows > 0) {
        hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for(rows * 8)), dim3(256), 0, st, dq, rows * 8, ws + WS_SCALE);
        PTMI_LAUNCH_CHECK("lkl_scale");
        if (dmu_p) {
            hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks_for(rows * 4)), dim3(256), 0, st, dmu_p, rows * 4,
                               ws + WS_SCALE);
            PTMI_LAUNCH_CHECK("lkl_scale_mu");
        }
    }
    return 0;
}

int ptmi_cls_stats(const float* logits, const int64_t* gt_classes, int64_t r, int c, int32_t* counts_out, int32_t* ws,
                   ptmi_stream_t s)
{
    PTMI_CHECK_ARG(counts_out && ws && r >= 0 && r <= 0x7fffffffll && c > 0, "cls_stats: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = r > 0 ? blocks_for(r) : 0;
    if (r > 0) {
        PTMI_CHECK_ARG(logits && gt_classes, "cls_stats: null buffer");
        hipLaunchKernelGGL(cls_stats_kernel, dim3(nb), dim3(256), 0, st, logits, gt_classes, r, c, ws);
        PTMI_LAUNCH_CHECK("cls_stats");
    }
    hipLaunchKernelGGL(counts_final_kernel<4>, dim3(1), dim3(256), 0, st, ws, nb, counts_out);
    PTMI_LAUNCH_CHECK("cls_stats_final");
    return 0;
}

int ptmi_label_counts(const int8_t* labels, int64_t n, int32_t* counts_out, int32_t* ws, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(counts_out && ws && n >= 0 && n <= 0x7fffffffll, "label_counts: bad args");
    hipStream_t st = (hipStream_t)s;
    const int nb = n > 0 ? blocks_for(n) : 0;
    if (n > 0) {
        PTMI_CHECK_ARG(labels, "label_counts: null buffer");
        hipLaunchKernelGGL(label_counts_kernel, dim3(nb), dim3(256), 0, st, labels, n, ws);
        PTMI_LAUNCH_CHECK("label_counts");
    }
    hipLaunchKernelGGL(counts_final_kernel<2>, dim3(1), dim3(256), 0, st, ws, nb, counts_out);
    PTMI_LAUNCH_CHECK("label_counts_final");
    return 0;
}

}  // extern "C"
