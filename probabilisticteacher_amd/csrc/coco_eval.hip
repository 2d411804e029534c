// coco_eval.hip -- the matching step of the COCO detection protocol for gfx950: every (image, category) segment of an
// evaluation, all IoU thresholds and area ranges, in ONE launch.
//
// Restates pycocotools COCOeval.computeIoU / evaluateImg and maskApi.c bbIou (no counterpart under pt/: the reference reaches
// them through detectron2's COCOEvaluator, pt/engine/trainer.py:132-133).  Everything that decides a match is double
// arithmetic in bbIou's operation order, without FMA contraction (-ffp-contract=off), so a tie at a threshold falls the way a
// CPU evaluation of the same expressions lets it fall.
//
// Mapping: one wave per segment, lane = a * T + t owns the (area range, threshold) pair -- the pairs are independent and walk
// the same loops.  Per segment the wave stages the GT boxes in LDS once; per detection it fills one IoU row together (lane
// over GT), then every lane scans that row on its own with its own matched-GT bits.  pycocotools visits GT "non-ignored
// first, then ignored" (a stable argsort on the ignore flag) and stops once it holds a non-ignored match and reaches the
// ignored ones: that is a pass over the non-ignored GT in dataset order followed, only when it found nothing, by a pass over
// the ignored ones -- no per-range permutation is built.  Results wait in LDS as 16-bit words and leave in rows along the
// detections, one (a, t) plane at a time.
#include "common.h"

namespace {

constexpr int MAX_DT = 100;      // maxDets[-1]
constexpr int MAX_GT = 1024;
constexpr int MAX_T = 16;
constexpr int MAX_A = 4;
constexpr int CROWD = 1 << MAX_A;      // bit of the per-GT flag byte beside the MAX_A ignore bits

// LDS of one workgroup: gt boxes gcap x 4 doubles | iou row gcap doubles | matched bits (gcap / 32) x 64 words |
// results max_dt x 64 u16 | flags gcap bytes; gcap = GT capacity, a multiple of 32
__host__ __device__ inline size_t lds_bytes(int gcap, int max_dt)
{
    return (size_t)gcap * 32 + (size_t)gcap * 8 + (size_t)(gcap / 32) * 64 * 4 + (size_t)max_dt * 64 * 2 + (size_t)gcap;
}

__global__ __launch_bounds__(64) void coco_match_kernel(
    const double* __restrict__ dt_xywh, const double* __restrict__ dt_area, const int64_t* __restrict__ dt_off,
    const double* __restrict__ gt_xywh, const double* __restrict__ gt_area, const int32_t* __restrict__ gt_crowd,
    const int64_t* __restrict__ gt_off, int64_t nd, int64_t ng, int max_dt, int gcap, const double* __restrict__ iou_thr,
    int T, const double* __restrict__ area_rng, int A, int32_t* __restrict__ gt_ignore, int32_t* __restrict__ dt_match,
    int32_t* __restrict__ dt_ignore)
{
    extern __shared__ double smem[];
    double* gbox = smem;                                               // [gcap][4]
    double* iou = gbox + (size_t)gcap * 4;                             // [gcap]
    uint32_t* matched = reinterpret_cast<uint32_t*>(iou + gcap);       // [gcap / 32][64]
    uint16_t* res = reinterpret_cast<uint16_t*>(matched + (gcap / 32) * 64);   // [max_dt][64]
    uint8_t* flags = reinterpret_cast<uint8_t*>(res + (size_t)max_dt * 64);    // [gcap]

    const int64_t seg = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t dbeg = dt_off[seg], gbeg = gt_off[seg];
    const int64_t dlen = dt_off[seg + 1] - dbeg, glen = gt_off[seg + 1] - gbeg;
    // tables that do not describe the arrays, or a segment beyond what the caller sized the launch for: nothing is touched
    if (dbeg < 0 || gbeg < 0 || dlen < 0 || glen < 0 || dbeg + dlen > nd || gbeg + glen > ng || dlen > max_dt || glen > gcap)
        return;
    const int D = (int)dlen, G = (int)glen;
    if (D == 0 && G == 0) return;
    const int pairs = A * T;
    const int a = lane / T, t = lane - a * T;
    const bool live = lane < pairs;

    // ---- ground truth: boxes into LDS, ignore flags per area range
    for (int g = lane; g < G; g += 64) {
        const double* b = gt_xywh + (gbeg + g) * 4;
        gbox[g * 4 + 0] = b[0];
        gbox[g * 4 + 1] = b[1];
        gbox[g * 4 + 2] = b[2];
        gbox[g * 4 + 3] = b[3];
        const double ar = gt_area[gbeg + g];
        const bool crowd = gt_crowd[gbeg + g] != 0;
        int f = crowd ? CROWD : 0;
        for (int k = 0; k < A; ++k) {
            const bool ig = crowd || ar < area_rng[2 * k] || ar > area_rng[2 * k + 1];
            f |= ig ? 1 << k : 0;
            gt_ignore[(int64_t)k * ng + gbeg + g] = ig;
        }
        flags[g] = (uint8_t)f;
    }
    if (D == 0) return;
    const int words = (G + 31) / 32;
    for (int w = 0; w < words; ++w) matched[w * 64 + lane] = 0u;
    const double lo = live ? area_rng[2 * a] : 0.0, hi = live ? area_rng[2 * a + 1] : 0.0;
    const double thr = live ? fmin(iou_thr[t], 1.0 - 1e-10) : 0.0;
    __syncthreads();

    for (int d = 0; d < D; ++d) {
        const double* db = dt_xywh + (dbeg + d) * 4;
        const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
        // ---- bbIou of detection d against every GT of the segment
        for (int g = lane; g < G; g += 64) {
            const double gx = gbox[g * 4 + 0], gy = gbox[g * 4 + 1], gw = gbox[g * 4 + 2], gh = gbox[g * 4 + 3];
            const double da = dw * dh, ga = gw * gh;
            double o = 0.0;
            const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
            if (w > 0.0) {
                const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
                if (h > 0.0) {
                    const double i = w * h;
                    const double u = (flags[g] & CROWD) ? da : da + ga - i;
                    o = i / u;
                }
            }
            iou[g] = o;
        }
        __syncthreads();
        if (live) {
            double best = thr;
            int m = -1;
            for (int pass = 0; pass < 2; ++pass) {          // non-ignored GT, then (with nothing found) the ignored ones
                if (pass == 1 && m >= 0) break;
                for (int g = 0; g < G; ++g) {
                    const int f = flags[g];
                    if (((f >> a) & 1) != pass) continue;
                    if (((matched[(g >> 5) * 64 + lane] >> (g & 31)) & 1u) && !(f & CROWD)) continue;
                    const double o = iou[g];
                    if (o < best) continue;
                    best = o;
                    m = g;
                }
            }
            int ig;
            if (m >= 0) {
                ig = (flags[m] >> a) & 1;
                matched[(m >> 5) * 64 + lane] |= 1u << (m & 31);
            } else {
                const double ar = dt_area[dbeg + d];
                ig = ar < lo || ar > hi;
            }
            res[d * 64 + lane] = (uint16_t)((m + 1) | (ig << 15));
        }
        __syncthreads();
    }

    // ---- results: plane (a, t) by plane, lanes along the detections
    for (int p = 0; p < pairs; ++p) {
        for (int d = lane; d < D; d += 64) {
            const int r = res[d * 64 + p];
            const int64_t at = (int64_t)p * nd + dbeg + d;
            dt_match[at] = (r & 0x7fff) - 1;
            dt_ignore[at] = r >> 15;
        }
    }
}

}  // namespace

extern "C" {

int ptmi_coco_match_max_gt(void) { return MAX_GT; }

int ptmi_coco_match(const double* dt_xywh, const double* dt_area, const int64_t* dt_off, const double* gt_xywh,
                    const double* gt_area, const int32_t* gt_crowd, const int64_t* gt_off, int64_t nseg, int64_t nd,
                    int64_t ng, int max_dt, int max_gt, const double* iou_thr, int nthr, const double* area_rng, int narea,
                    int32_t* gt_ignore, int32_t* dt_match, int32_t* dt_ignore, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(nseg >= 0 && nd >= 0 && ng >= 0 && max_dt >= 0 && max_gt >= 0, "coco_match: negative size");
    PTMI_CHECK_ARG(nthr >= 1 && nthr <= MAX_T, "coco_match: %d IoU thresholds (1 .. %d are served)", nthr, MAX_T);
    PTMI_CHECK_ARG(narea >= 1 && narea <= MAX_A, "coco_match: %d area ranges (1 .. %d are served)", narea, MAX_A);
    PTMI_CHECK_ARG(max_dt <= MAX_DT, "coco_match: a segment of %d detections (at most %d are served)", max_dt, MAX_DT);
    PTMI_CHECK_ARG(max_gt <= MAX_GT, "coco_match: a segment of %d ground-truth boxes (at most %d are served)", max_gt,
                   MAX_GT);
    PTMI_CHECK_ARG(max_dt <= nd && max_gt <= ng, "coco_match: longest segment exceeds the arrays");
    PTMI_CHECK_ARG(nseg <= 0x7fffffffLL, "coco_match: %lld segments exceed the grid", (long long)nseg);
    PTMI_CHECK_ARG(iou_thr && area_rng, "coco_match: thresholds / area ranges missing");
    PTMI_CHECK_ARG(nseg == 0 || (dt_off && gt_off), "coco_match: offset tables missing");
    PTMI_CHECK_ARG(nd == 0 || (dt_xywh && dt_area && dt_match && dt_ignore), "coco_match: detection arrays missing");
    PTMI_CHECK_ARG(ng == 0 || (gt_xywh && gt_area && gt_crowd && gt_ignore), "coco_match: ground-truth arrays missing");
    if (nseg == 0 || (nd == 0 && ng == 0)) return 0;
    const int gcap = max_gt > 0 ? (max_gt + 31) / 32 * 32 : 32;
    const size_t lds = lds_bytes(gcap, max_dt);              // 61.8 KB at MAX_GT and MAX_DT
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)nseg), dim3(64), lds, (hipStream_t)s, dt_xywh, dt_area, dt_off,
                       gt_xywh, gt_area, gt_crowd, gt_off, nd, ng, max_dt, gcap, iou_thr, nthr, area_rng, narea, gt_ignore,
                       dt_match, dt_ignore);
    PTMI_LAUNCH_CHECK("coco_match");
    return 0;
}

}  // extern "C"
