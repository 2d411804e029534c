// anomaly.hip -- anomaly mode (PTrainer(detect_anomaly=True); reference pt/engine/trainer.py:167 runs every step under
// torch.autograd.set_detect_anomaly): does a tensor hold a NaN or an infinity, and where is the first one.  gfx950 only.
//
// Both kernels are single-pass, bandwidth-bound reads.  A value is classified on its BIT PATTERN (exponent all ones; mantissa
// zero = infinity, else NaN), never by a float comparison a fast-math flag could fold away.  Every thread keeps two flag bits
// (1 = NaN, 2 = infinity) and the lowest non-finite element index it has seen; ballots combine the flags inside a wave, four LDS
// words inside the block, and ONE lane of a block that found something issues the global atomicOr / atomicMin -- a clean tensor
// costs its read and not one global write.  The reported index is a minimum over all elements, so it does not depend on the
// grid, the lane <-> element assignment or the order in which blocks finish.
//
//   nonfinite_scan_kernel<BF16>   one tensor -> flags[slot] |= bits, first[slot] = min(first[slot], lowest index); grid-stride,
//                                 capped grid.  16-byte loads from the first 16-byte boundary on, scalar head and tail.
//   seg_nonfinite_kernel          the flat gradient buffer -> the two bits per SEGMENT (parameter), one workgroup per chunk
//                                 descriptor of ops.SegmentTable (the tables of the per-parameter clipping kernels, misc.hip).
#include "common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_MAX_BLOCKS = 2048;          // 8 workgroups per CU of a 256-CU part: enough loads in flight for HBM

__device__ __forceinline__ unsigned classify_f32(unsigned u)
{
    return (u & 0x7F800000u) == 0x7F800000u ? ((u & 0x007FFFFFu) ? 1u : 2u) : 0u;
}
__device__ __forceinline__ unsigned classify_bf16(unsigned h)          // h: the 16 bits of one bf16 value
{
    return (h & 0x7F80u) == 0x7F80u ? ((h & 0x007Fu) ? 1u : 2u) : 0u;
}

template <int BF16>
__device__ __forceinline__ unsigned load_classify(const void* base, int64_t i)
{
    if (BF16) return classify_bf16(reinterpret_cast<const unsigned short*>(base)[i]);
    return classify_f32(reinterpret_cast<const unsigned*>(base)[i]);
}

__device__ __forceinline__ void note(unsigned c, int64_t i, unsigned& f, int64_t& first)
{
    if (c) {
        f |= c;
        if (i < first) first = i;
    }
}

// elements [0, len) at `base`, walked by `nthreads` threads of which this is `tid`: a scalar head up to the first 16-byte
// boundary, 16-byte vectors, a scalar tail.  Indices noted are relative to `base`.
template <int BF16>
__device__ __forceinline__ void scan_range(const void* base, int64_t len, int64_t tid, int64_t nthreads, unsigned& f,
                                           int64_t& first)
{
    constexpr int ES = BF16 ? 2 : 4, PER = 16 / ES;
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) / ES);
    if (head > len) head = len;
    const int64_t nv = (len - head) / PER;
    for (int64_t i = tid; i < head; i += nthreads) note(load_classify<BF16>(base, i), i, f, first);
    const u32x4* v4 = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base) + head * ES);
    for (int64_t i = tid; i < nv; i += nthreads) {
        const u32x4 v = v4[i];
        const int64_t e0 = head + i * PER;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (BF16) {
                note(classify_bf16(v[j] & 0xFFFFu), e0 + 2 * j, f, first);
                note(classify_bf16(v[j] >> 16), e0 + 2 * j + 1, f, first);
            } else {
                note(classify_f32(v[j]), e0 + j, f, first);
            }
        }
    }
    for (int64_t i = head + nv * PER + tid; i < len; i += nthreads) note(load_classify<BF16>(base, i), i, f, first);
}

// the two flag bits of the whole 256-thread block, in every thread (0 for a clean block)
__device__ __forceinline__ unsigned block_flags_256(unsigned f, unsigned* smem)
{
    const unsigned wf = (__ballot(f & 1u) ? 1u : 0u) | (__ballot(f & 2u) ? 2u : 0u);
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = wf;
    __syncthreads();
    return smem[0] | smem[1] | smem[2] | smem[3];
}

template <int BF16>
__global__ __launch_bounds__(SCAN_THREADS) void nonfinite_scan_kernel(const void* __restrict__ x, int64_t n,
                                                                      int32_t* __restrict__ flag,
                                                                      unsigned long long* __restrict__ first_out)
{
    __shared__ unsigned smf[4];
    __shared__ long long smi[4];
    unsigned f = 0u;
    int64_t first = INT64_MAX;
    scan_range<BF16>(x, n, (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x, (int64_t)gridDim.x * SCAN_THREADS, f, first);
    const unsigned bf = block_flags_256(f, smf);
    if (!bf) return;                                  // block-uniform: a clean block writes nothing
    long long m = first;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_down(m, o, 64);
        m = other < m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) smi[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long b = smi[0];
        for (int w = 1; w < 4; ++w) b = smi[w] < b ? smi[w] : b;
        atomicOr(flag, (int)bf);
        atomicMin(first_out, (unsigned long long)b);          // indices are >= 0 and the slot starts at INT64_MAX
    }
}

// Chunk descriptor -> [a, e) and its segment, by the rule of the per-parameter clipping kernels (misc.hip: seg_chunk_range):
// a descriptor that names no segment or does not start inside its segment is skipped, and the range ends with the chunk, the
// segment and the buffer, whichever comes first.
__device__ __forceinline__ bool seg_chunk_range(const int64_t* __restrict__ seg_off, int S,
                                                const int64_t* __restrict__ chunks, int64_t n, int64_t& a, int64_t& e,
                                                int& seg)
{
    a = chunks[2 * (int64_t)blockIdx.x];
    const int64_t sg = chunks[2 * (int64_t)blockIdx.x + 1];
    if (sg < 0 || sg >= S) return false;
    seg = (int)sg;
    if (a < 0 || a < seg_off[seg]) return false;
    e = a + PTMI_SEG_CHUNK;
    if (e > seg_off[seg + 1]) e = seg_off[seg + 1];
    if (e > n) e = n;
    return a < e;
}

__global__ __launch_bounds__(SCAN_THREADS) void seg_nonfinite_kernel(const float* __restrict__ g, int64_t n,
                                                                     const int64_t* __restrict__ seg_off, int S,
                                                                     const int64_t* __restrict__ chunks,
                                                                     int32_t* __restrict__ seg_flags)
{
    __shared__ unsigned smf[4];
    int64_t a, e;
    int seg;
    if (!seg_chunk_range(seg_off, S, chunks, n, a, e, seg)) return;
    unsigned f = 0u;
    int64_t first = INT64_MAX;                        // (not reported per segment: dead code to the compiler)
    scan_range<0>(g + a, e - a, threadIdx.x, SCAN_THREADS, f, first);
    const unsigned bf = block_flags_256(f, smf);
    if (bf && threadIdx.x == 0) atomicOr(&seg_flags[seg], (int)bf);
}

}  // namespace

extern "C" {

int ptmi_nonfinite_scan(const void* x, int64_t n, int dtype, int32_t* flags, int64_t* first, int slot, int nslots,
                        ptmi_stream_t s)
{
    PTMI_CHECK_ARG(n >= 0, "nonfinite_scan: negative length %lld", (long long)n);
    if (n == 0) return 0;
    PTMI_CHECK_ARG(dtype == 0 || dtype == 1, "nonfinite_scan: unknown dtype %d (0 = fp32, 1 = bf16)", dtype);
    PTMI_CHECK_ARG(nslots > 0 && slot >= 0 && slot < nslots, "nonfinite_scan: slot %d outside [0, %d)", slot, nslots);
    PTMI_CHECK_ARG(x && flags && first, "nonfinite_scan: null pointer");
    const int es = dtype ? 2 : 4;
    PTMI_CHECK_ARG(((uintptr_t)x & (uintptr_t)(es - 1)) == 0, "nonfinite_scan: tensor not aligned to its %d-byte elements", es);
    int64_t blocks = (n / (16 / es) + SCAN_THREADS - 1) / SCAN_THREADS;      // one 16-byte vector per thread and round
    if (blocks > SCAN_MAX_BLOCKS) blocks = SCAN_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    unsigned long long* fo = reinterpret_cast<unsigned long long*>(first + slot);
    if (dtype)
        hipLaunchKernelGGL(nonfinite_scan_kernel<1>, dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, (hipStream_t)s, x, n,
                           flags + slot, fo);
    else
        hipLaunchKernelGGL(nonfinite_scan_kernel<0>, dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, (hipStream_t)s, x, n,
                           flags + slot, fo);
    PTMI_LAUNCH_CHECK("nonfinite_scan");
    return 0;
}

int ptmi_seg_nonfinite(const float* g, int64_t n, const int64_t* seg_off, int S, const int64_t* chunks, int C,
                       int32_t* seg_flags, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(n >= 0 && S >= 0 && C >= 0, "seg_nonfinite: negative length");
    if (n == 0 || S == 0) return 0;
    PTMI_CHECK_ARG(g && seg_off && chunks && seg_flags && C > 0 && ((uintptr_t)g & 3u) == 0, "seg_nonfinite: bad args");
    hipError_t e = hipMemsetAsync(seg_flags, 0, sizeof(int32_t) * (size_t)S, (hipStream_t)s);
    if (e != hipSuccess) { ptmi_set_error("seg_nonfinite: memset failed"); return -2; }
    hipLaunchKernelGGL(seg_nonfinite_kernel, dim3((unsigned)C), dim3(SCAN_THREADS), 0, (hipStream_t)s, g, n, seg_off, S,
                       chunks, seg_flags);
    PTMI_LAUNCH_CHECK("seg_nonfinite");
    return 0;
}

}  // extern "C"
