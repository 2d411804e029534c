// tta.hip -- test-time augmentation (TEST.AUG): the detections of every augmentation of a batch mapped back to their original
// image and prepared for ONE merged NMS per image (gfx950).
//
// Restates detectron2 0.5 GeneralizedRCNNWithTTA._inverse_boxes / _merge_detections (D2 is not a dependency: parity by
// restatement).  D2 takes every augmentation's boxes to the host, runs TransformList.inverse().apply_box in numpy on float32
// arrays -- HFlipTransform (w - x), ResizeTransform back to the loader image, ResizeTransform back to the original size, each
// followed by a min / max over the box's four corners -- and then fast_rcnn_inference_single_image on the concatenation
// (finite filter, clip, score > 1e-8, batched_nms with torchvision's class offset).  Here a lane per detection does the same
// fp32 operations in the same order.  No multiply below feeds an add or a subtract except the class offset of
// tta_nms_boxes_kernel, and contraction is off for the whole file (build flag) and again inside every kernel (pragma): the
// results are the bits numpy / torch give on the CPU.
#include "common.h"

namespace {

// per-augmentation table, one row per augmentation: aug_meta (naug, 3) int32 = image, flipped, has pre-transform;
// aug_factors (naug, 5) float = w_s, fx_s, fy_s, gx, gy (the factors are formed in double on the host and rounded once)
constexpr int META = 3, FACT = 5;

__device__ __forceinline__ void minmax(float& lo, float& hi)
{
    const float a = lo, b = hi;
    lo = fminf(a, b);
    hi = fmaxf(a, b);
}

// aug_offsets (naug + 1): detections [aug_offsets[a], aug_offsets[a + 1]) belong to augmentation a; augmentations are grouped
// by image, so an image's detections are one contiguous segment.  Outputs are dense over the D detections: the mapped box,
// clipped to its image ((0, 0, 0, 0) for a row the finite filter drops, so that no NaN reaches the sort or the NMS), the sort
// key = score of a candidate / -inf otherwise (a stable descending sort per image then lists the candidates first, in the
// order batched_nms visits them); per image the candidate count and the largest candidate coordinate.  Coordinates are >= +0
// after the clip, so the float max is an integer max on the bits: the same bits whatever order the lanes arrive in.
__global__ __launch_bounds__(256) void tta_map_boxes_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                            const int32_t* __restrict__ aug_off,
                                                            const int32_t* __restrict__ aug_meta,
                                                            const float* __restrict__ aug_fact, const float* __restrict__ sizes,
                                                            float* __restrict__ boxes_out, float* __restrict__ keys_out,
                                                            unsigned* __restrict__ img_max, int32_t* __restrict__ img_cnt, int d,
                                                            int naug, float thresh)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d) return;
    int lo = 0, hi = naug - 1;                      // the last augmentation that starts at or before i (empty ones start later
    while (lo < hi) {                               // or end at their start: never chosen)
        const int mid = (lo + hi + 1) >> 1;
        if (aug_off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const int32_t* m = aug_meta + lo * META;
    const float* f = aug_fact + lo * FACT;
    const int img = m[0];
    const float4 b = reinterpret_cast<const float4*>(boxes)[i];
    const float sc = scores[i];
    float x1 = b.x, y1 = b.y, x2 = b.z, y2 = b.w;
    // numpy's min / max hand a NaN on, fminf / fmaxf drop it: the verdict on the inputs is taken here
    bool fin = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && isfinite(sc);
    if (m[1]) {                                     // HFlipTransform.apply_coords: x = w_s - x, then apply_box's min / max
        const float ws = f[0];
        x1 = ws - x1;
        x2 = ws - x2;
        minmax(x1, x2);
        minmax(y1, y2);
    }
    x1 = x1 * f[1];                                 // inverse of the augmentation's resize: x * fp32(w / w_s), y * fp32(h / h_s)
    x2 = x2 * f[1];
    y1 = y1 * f[2];
    y2 = y2 * f[2];
    minmax(x1, x2);
    minmax(y1, y2);
    if (m[2]) {                                     // inverse of the loader's resize (absent, not a multiply by 1, when equal)
        x1 = x1 * f[3];
        x2 = x2 * f[3];
        y1 = y1 * f[4];
        y2 = y2 * f[4];
        minmax(x1, x2);
        minmax(y1, y2);
    }
    fin = fin && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);          // (a product may overflow)
    const float H = sizes[2 * img], W = sizes[2 * img + 1];
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (fin) {
        c.x = fminf(fmaxf(x1, 0.f), W);
        c.y = fminf(fmaxf(y1, 0.f), H);
        c.z = fminf(fmaxf(x2, 0.f), W);
        c.w = fminf(fmaxf(y2, 0.f), H);
    }
    const bool cand = fin && sc > thresh;
    reinterpret_cast<float4*>(boxes_out)[i] = c;
    keys_out[i] = cand ? sc : -INFINITY;
    if (cand) {
        const float mx = fmaxf(fmaxf(c.x, c.y), fmaxf(c.z, c.w)) + 0.f;                 // (+ 0: a -0 would be the largest integer)
        atomicAdd(img_cnt + img, 1);
        atomicMax(img_max + img, __float_as_uint(mx));
    }
}

// boxes handed to NMS, in sorted order: box + class * (max coordinate of the image's candidates + 1), fp32 -- the expression
// of roi_infer_nms_boxes_kernel (boxes.hip) with the class read from the detection instead of its dense position.
// grid.y = image; `order` = position within the image's segment.
__global__ __launch_bounds__(256) void tta_nms_boxes_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ classes,
                                                            const int32_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                            const unsigned* __restrict__ img_max, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const int img = blockIdx.y;
    const int beg = seg[img], n = seg[img + 1] - beg;
    const float off1 = __uint_as_float(img_max[img]) + 1.0f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int dpos = order[beg + i];
        const float off = (float)classes[beg + dpos] * off1;
        const float4 b = reinterpret_cast<const float4*>(boxes)[beg + dpos];
        reinterpret_cast<float4*>(out)[beg + i] = make_float4(b.x + off, b.y + off, b.z + off, b.w + off);
    }
}

}  // namespace

extern "C" {

int ptmi_tta_map_boxes(const float* boxes, const float* scores, const int32_t* aug_offsets, const int32_t* aug_meta,
                       const float* aug_factors, const float* image_sizes_hw, float* boxes_out, float* keys_out,
                       float* img_max_out, int32_t* img_count_out, int64_t d, int naug, int nimg, float score_thresh,
                       ptmi_stream_t s)
{
    PTMI_CHECK_ARG(d >= 0 && d < (1ll << 31) - 256 && naug > 0 && nimg > 0 && img_max_out && img_count_out,
                   "tta_map_boxes: bad args");
    hipStream_t st = (hipStream_t)s;
    hipError_t e = hipMemsetAsync(img_max_out, 0, sizeof(float) * (size_t)nimg, st);
    if (e == hipSuccess) e = hipMemsetAsync(img_count_out, 0, sizeof(int32_t) * (size_t)nimg, st);
    if (e != hipSuccess) { ptmi_set_error("tta_map_boxes: memset failed"); return -2; }
    if (d == 0) return 0;
    PTMI_CHECK_ARG(boxes && scores && aug_offsets && aug_meta && aug_factors && image_sizes_hw && boxes_out && keys_out,
                   "tta_map_boxes: null buffer");
    hipLaunchKernelGGL(tta_map_boxes_kernel, dim3((unsigned)cdiv64(d, 256)), dim3(256), 0, st, boxes, scores, aug_offsets,
                       aug_meta, aug_factors, image_sizes_hw, boxes_out, keys_out, reinterpret_cast<unsigned*>(img_max_out),
                       img_count_out, (int)d, naug, score_thresh);
    PTMI_LAUNCH_CHECK("tta_map_boxes");
    return 0;
}

int ptmi_tta_nms_boxes(const float* boxes, const int64_t* classes, const int32_t* order, const int32_t* seg_offsets,
                       const float* img_max, int nimg, int max_count, float* out, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(seg_offsets && img_max && nimg > 0 && nimg < 65536 && max_count >= 0, "tta_nms_boxes: bad args");
    if (max_count == 0) return 0;
    PTMI_CHECK_ARG(boxes && classes && order && out, "tta_nms_boxes: null buffer");
    hipLaunchKernelGGL(tta_nms_boxes_kernel, dim3(cdiv(max_count, 256), nimg), dim3(256), 0, (hipStream_t)s, boxes, classes,
                       order, seg_offsets, reinterpret_cast<const unsigned*>(img_max), out);
    PTMI_LAUNCH_CHECK("tta_nms_boxes");
    return 0;
}

}  // extern "C"
