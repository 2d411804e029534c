// conv.hip -- 3x3 s1 p1 convolution stack for gfx950 (CDNA4), fp32 on v_mfma_f32_32x32x2_f32.
//
// Replaces the cuDNN conv2d (+bias, +ReLU) the reference reaches at
// pt/modeling/backbone/vgg.py:45-53,66-69 (13 VGG16 layers) and the 3x3 conv of D2's
// StandardRPNHead (pt/modeling/proposal_generator/rpn.py:96), forward, dgrad and wgrad.
//
// Design (MI355X-first, not a cuDNN translation):
//   * implicit GEMM  M = Cout, N = output pixels, K = 9*Cin, NCHW fp32 end to end;
//   * forward / dgrad: `conv3x3_buf_kernel` -- 4 or 8 wave64s per workgroup, each wave owns 64 channels x two
//     4-row x 8-column pixel blocks (four 32x32 accumulator tiles = 64 VGPRs); K is walked in 4-channel chunks,
//     operands go global -> LDS with `buffer_load_dwordx4 ... lds`, double buffered, one barrier per chunk;
//   * dgrad reuses the same kernel with flipped/transposed packed weights; the producer's ReLU mask can be applied
//     in the epilogue (epilogue 3); frozen blocks fuse bias + ReLU + 2x2 max pool (epilogue 4);
//   * the 3-channel stem is a VALU kernel over the flattened plane (HBM-write bound; packed fp32 FMAs);
//   * wgrad: `conv3x3_wgrad_buf_kernel` -- M = Cout, N = Cin (x 9 taps as 9 accumulator tiles), K = pixels; split-K
//     over pixel tiles with a fixed-order second-stage reduction (deterministic).
// Shapes whose per-image byte offsets do not fit 32 bits are rejected with an error (no fallback kernels).

#include "common.h"
#include <type_traits>

namespace {

constexpr int TW = 32;   // output pixels per MFMA column block

// ------------------------------------------------------------------------------------ forward, buffer-DMA pipeline
// Default forward / dgrad kernel: K walked in 4-channel chunks, double-buffered LDS, ONE workgroup barrier per chunk,
// 72 MFMAs per wave per chunk:   issue DMA(chunk c+1 -> buf^1) ; MFMAs on buf ; s_waitcnt vmcnt(0) ; s_barrier.
// Its predecessor used global_load_lds with per-lane 4-B gathers; clock64() probes of that kernel
// (tools/exp_conv_timing.py) showed the main loop keeping the MFMA pipe ~93-100 % busy, with the losses in the MFMAs
// spent on pixels outside the image and in the VALU work of the DMA issue.  Hence:
//   * operands arrive through `buffer_load_dwordx4 ... lds`: per-lane byte offsets are loop invariants, the chunk
//     advance lives in the scalar buffer descriptor, halo / padded-channel pieces carry offset 0xFFFFFFFF and are
//     zero-filled by the buffer range check.  One 16-B patch DMA per lane per chunk (was four 4-B gathers with
//     64-bit address selects), no zero page.
//   * the MFMA N dimension (32 lanes) is a 4-row x 8-column pixel block instead of 32 consecutive pixels of one
//     row, and a wave skips the MFMAs of pixel blocks that lie wholly outside the image.  The tile granularity
//     drops from 32 to 8 columns: 100x166 maps waste 1 % instead of 16 %, 50x83 maps 10 % instead of 20 %.
// LDS patch row pitch is 40 floats (10 pieces; column m <-> image column x0 - 4 + m, so the left halo is one whole
// piece), which also puts the four rows of a pixel block on disjoint 8-bank groups for ds_read_b32.
typedef __attribute__((address_space(3))) void lds_void_b_t;
constexpr int PWB = 40;

__device__ __forceinline__ void* uniform_ptr(const void* p)
{
    const unsigned long long a = (unsigned long long)p;
    return (void*)(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32) |
                   (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a));
}

// (SOLVER.AMP.ENABLED runs the bf16-storage kernels of p8.hip; the bf16-INPUT variants that rounds 2-3 kept in this file --
// fp32 tensors in HBM and LDS, operands rounded between LDS and the MFMA -- are gone.)
template <int BM, int NWAVE>
__global__ __launch_bounds__(64 * NWAVE, (NWAVE == 8 ? 4 : 3)) void conv3x3_buf_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
    const float* __restrict__ mref, float* __restrict__ y, int N, int Cin, int Cout, int H, int W,
    int tilesX, int tilesY, int coTiles, int nChunks, int epi)
{
    constexpr int CK = 4;
    constexpr int NT = 64 * NWAVE;
    constexpr int WN = NWAVE / (BM / 64);            // waves along the pixel dimension: 2 -> 4 rows, 4 -> 8 rows
    constexpr int TH = 2 * WN, PR = TH + 2, PLANE = PR * PWB;
    // weight slab per chunk, in floats: 9 taps x CK channels x BM fp32
    constexpr int WS = 9 * CK * BM;
    constexpr int WPC = WS / 4;                      // ... in 16-B pieces
    constexpr int NWI = (WPC + NT - 1) / NT;
    constexpr int PPC = CK * PR * 10;                // patch pieces per chunk (240 / 400)
    constexpr int NPI = (PPC + NT - 1) / NT;         // ... per lane: 1 (2 for the 64-channel, 4-wave variant)
    constexpr int PS = ((PPC + 63) / 64) * 64 * 4;   // patch floats, padded to whole waves of pieces
    constexpr int STAGE = WS + PS;
    __shared__ __attribute__((aligned(16))) float lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // grid = (coTiles, N * tilesY, tilesX), linear workgroup order = channel tile, image, tile row, tile column:
    //   * the four channel tiles of one pixel tile are neighbours in time (they share the input patch through L2);
    //   * the XCD of a workgroup (linear id mod 8) alternates with the image index, so the light right-edge tiles
    //     (an even tilesX with row-major numbering put all of them on four XCDs: 13 % of slot-time empty at 100x166)
    //     spread evenly;
    //   * the light right-edge tile column is dispatched last, which shortens the tail of the launch.
    const int cot = blockIdx.x;
    const int ty = blockIdx.y / N, n = blockIdx.y - ty * N;
    const int tx = blockIdx.z;
    const int x0 = tx * TW, y0 = ty * TH;
    const int HW = H * W;
    const int wv = W - x0;                           // valid columns right of x0

    // this lane's patch piece(s): (channel, patch row, piece) -> byte offset from the chunk's first channel plane
    unsigned pvoff[NPI];
    int fix = 0;                                     // words 1..3 of piece i (bits 4i+1..4i+3) beyond the image edge
#pragma unroll
    for (int i = 0; i < NPI; ++i) {
        const int pidx = tid + i * NT;
        const int ci = pidx / (PR * 10), rem = pidx - ci * (PR * 10);
        const int r = rem / 10, q = rem - r * 10;
        const int gy = y0 - 1 + r, gx = x0 - 4 + 4 * q;
        pvoff[i] = 0xFFFFFFFFu;
        if (pidx < PPC && gy >= 0 && gy < H && gx >= 0 && gx < W) {
            pvoff[i] = (unsigned)(ci * HW + gy * W + gx) * 4u;
#pragma unroll
            for (int e = 1; e < 4; ++e) fix |= (gx + e >= W) ? (1 << (4 * i + e)) : 0;
        }
    }
    const unsigned wvoff = (unsigned)tid * 16u;
    const bool edge = wv < 33;                       // some loaded piece straddles the right image edge

    const char* xc = (const char*)(x + (size_t)n * Cin * HW);
    const char* wc = (const char*)(wp + (size_t)cot * nChunks * WS);
    unsigned xleft = (unsigned)Cin * (unsigned)HW * 4u;   // bytes from xc to the end of image n (< 2^32: launcher)

    auto issue = [&](int buf) {
        float* Wd = lds + buf * STAGE + wave * 256;
        float* Pd = lds + buf * STAGE + WS + wave * 256;
        // (both chunk pointers are wave-uniform; readfirstlane keeps the compiler from parking them in VGPRs when
        // SGPRs run short, which would turn every DMA into a waterfall loop)
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(wc), 0, WS * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
            uniform_ptr(xc), 0, __builtin_amdgcn_readfirstlane((int)xleft), 0x00020000);
#pragma unroll
        for (int i = 0; i < NWI; ++i) {
            if ((i + 1) * NT <= WPC || wave * 64 + i * NT < WPC)     // wave-uniform (WPC is a multiple of 64)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_b_t*)(Wd + i * NT * 4), 16, (int)wvoff,
                                                         i * NT * 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NPI; ++i) {
            if (wave * 64 + i * NT < PPC)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_b_t*)(Pd + i * NT * 4), 16, (int)pvoff[i], 0, 0, 0);
        }
        wc += WS * 4;
        xc += (size_t)CK * HW * 4;
        xleft -= (unsigned)CK * (unsigned)HW * 4u;
    };

    constexpr int WNX = 2;                            // two waves side by side cover the 32 columns
    const int wm = wave / WN, wn = wave % WN;
    const int cb = (wn % WNX) * 16, rb = (wn / WNX) * 4;
    const int nl = lane & 31;
    const int pr = nl >> 3, pc = nl & 7;              // pixel inside the 4 x 8 block
    const bool row_in = y0 + rb < H;
    const int mode = !row_in ? 0 : (cb + 8 < wv ? 2 : (cb < wv ? 1 : 0));      // pixel blocks with work: 0 / 1 / 2
    const int a_off = wm * 64 + nl + (lane >> 5) * BM;
    const int b_off = WS + (lane >> 5) * PLANE + (rb + pr) * PWB + cb + pc + 3;

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};     // acc[co half][pixel block]

    // One copy of the chunk loop per amount of MFMA work (2, 1 or 0 pixel blocks inside the image), selected once
    // by a wave-uniform branch: every copy runs the same DMA issue / wait / barrier sequence, and each gets a
    // register allocation of its own.
    auto run = [&](auto mode_c) {
        constexpr int MODE = decltype(mode_c)::value;
        issue(0);
        for (int chunk = 0; chunk < nChunks; ++chunk) {
            const int buf = chunk & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA pieces of `buf` have landed
            if (edge && fix) {
                float* pw = lds + buf * STAGE + WS + tid * 4;
#pragma unroll
                for (int i = 0; i < NPI; ++i) {
#pragma unroll
                    for (int e = 1; e < 4; ++e)
                        if (fix & (1 << (4 * i + e))) pw[i * NT * 4 + e] = 0.f;
                }
            }
            __syncthreads();                                      // everyone's pieces landed; buf^1 is free
            if (chunk + 1 < nChunks) issue(buf ^ 1);
            if (MODE == 0) continue;
            const float* wsl = lds + buf * STAGE + a_off;
            const float* psl = lds + buf * STAGE + b_off;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap % 3;
#pragma unroll
                for (int j = 0; j < CK / 2; ++j) {
                    const float a0 = wsl[(tap * CK + 2 * j) * BM];
                    const float a1 = wsl[(tap * CK + 2 * j) * BM + 32];
                    const float b0 = psl[2 * j * PLANE + ky * PWB + kx];
                    acc00 = mfma32(a0, b0, acc00);
                    acc10 = mfma32(a1, b0, acc10);
                    if (MODE == 2) {
                        const float b1 = psl[2 * j * PLANE + ky * PWB + kx + 8];
                        acc01 = mfma32(a0, b1, acc01);
                        acc11 = mfma32(a1, b1, acc11);
                    }
                }
            }
        }
    };
    if (mode == 2) run(std::integral_constant<int, 2>{});
    else if (mode == 1) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});
    if (mode == 0) return;

    // Epilogue.  clock64() probes showed the straightforward version (64-bit address arithmetic and bounds tests
    // per element, issued while the CU's other waves stream MFMAs) holding the workgroup's slot for 30-40 us after
    // its last MFMA -- 5-17 % of its life.  Here every store is `buffer_store_dword`: the per-lane byte offset
    // (pixel, + 4 channels for the upper lane half) is computed once, the channel advance is a scalar offset, and
    // out-of-image pixels (offset 0xFFFFFFFF) / channels >= Cout (past num_records) are dropped by the range check,
    // which counts the scalar offset too (held under guard bands by tests/test_conv_bounds_gpu.py).
    const int py = y0 + rb + pr;
    const int half4 = 4 * (lane >> 5);
    const int co_w = cot * BM + wm * 64;                                   // wave-uniform first channel
    const __amdgpu_buffer_rsrc_t rbias = ptmi_rsrc(bias ? bias : y, bias ? (unsigned)Cout * 4u : 0u);
    f32x4 bv[2][4];                                                        // bias of channels co_w + 32s + 8g + half4 + 0..3
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bv[s][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (epi <= 1 || epi == 4)
                bv[s][g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rbias, half4 * 4, (co_w + s * 32 + g * 8) * 4, 0));
        }
    }
    if (epi == 4) {
        // bias + ReLU + 2x2/2 max pool (floor mode) fused: the vertical partner of a pixel is lane^8, the
        // horizontal partner lane^1 (both inside the 4 x 8 block); lanes with even row and column store to the
        // pooled (H/2, W/2) tensor.  The full-resolution activation never reaches HBM (frozen blocks only).
        const int OH = H >> 1, OW = W >> 1, OHW = OH * OW;
        const __amdgpu_buffer_rsrc_t ry = ptmi_rsrc(y + (size_t)n * Cout * OHW, (unsigned)Cout * (unsigned)OHW * 4u);
        unsigned pv[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int oy = py >> 1, ox = (x0 + cb + 8 * q + pc) >> 1;
            const bool ok = !(pr & 1) && !(pc & 1) && oy < OH && ox < OW && (q == 0 || mode == 2);
            pv[q] = ok ? (unsigned)(half4 * OHW + oy * OW + ox) * 4u : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int soff = (co_w + s * 32 + (r & 3) + 8 * (r >> 2)) * OHW * 4;
                const float b = bv[s][r >> 2][r & 3];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (q == 1 && mode < 2) continue;
                    const float v = fmaxf(((s == 0) ? (q == 0 ? acc00[r] : acc01[r]) : (q == 0 ? acc10[r] : acc11[r])) + b, 0.f);
                    float m = fmaxf(v, __shfl_xor(v, 8, 64));
                    m = fmaxf(m, __shfl_xor(m, 1, 64));
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, m), ry, (int)pv[q], soff, 0);
                }
            }
        }
        return;
    }
    const unsigned img_bytes = (unsigned)Cout * (unsigned)HW * 4u;
    const __amdgpu_buffer_rsrc_t ry = ptmi_rsrc(y + (size_t)n * Cout * HW, img_bytes);
    const __amdgpu_buffer_rsrc_t rm = ptmi_rsrc(epi == 3 ? mref + (size_t)n * Cout * HW : y, epi == 3 ? img_bytes : 0u);
    unsigned pv[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int px = x0 + cb + 8 * q + pc;
        pv[q] = (py < H && px < W && (q == 0 || mode == 2)) ? (unsigned)(half4 * HW + py * W + px) * 4u : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = (co_w + s * 32 + (r & 3) + 8 * (r >> 2)) * HW * 4;
            const float b = bv[s][r >> 2][r & 3];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (q == 1 && mode < 2) continue;
                float v = (s == 0) ? (q == 0 ? acc00[r] : acc01[r]) : (q == 0 ? acc10[r] : acc11[r]);
                if (epi <= 1) {
                    v += b;
                    if (epi == 1) v = fmaxf(v, 0.f);
                } else if (epi == 3) {
                    const float mk = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, (int)pv[q], soff, 0));
                    v = (mk > 0.f) ? v : 0.f;
                }
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, (int)pv[q], soff, 0);
            }
        }
    }
}

// ------------------------------------------------------------------------------------ stem (Cin <= 4), VALU
// The 3-channel stem has K = 27: 3.7 GF per image against 273 MB of output -- an HBM-WRITE-bound layer whose MFMA
// formulation spends its time in per-workgroup latency chains.  What the write side can reach depends on the store
// pattern (tools/exp/store_pattern.hip, 48 x 64 x 800 x 1333 fp32): a flat fill 6.9 TB/s; 64 planes written as 1 KB runs
// that start on a 16-B boundary 5.9 TB/s; the same runs starting at each ROW's first pixel -- rows of 1333 floats are only
// 4-B aligned -- 2.9 TB/s; 256-B runs per row (one pixel per lane) 1.8 TB/s.  So the kernel tiles the FLATTENED plane:
//   * a lane owns the four consecutive flat pixel indices 4t .. 4t + 3 of a plane (one aligned 16-B store per channel,
//     1 KB per wave and channel) and a wave the 16 channels 16w .. 16w + 15 of the 64-channel tile;
//   * the four pixels usually sit in one row and share a 3 x 6 input window per input channel.  Where they wrap over a
//     row end the wave runs the body once per row touched ("frame": row y0 + f, first column x0 - f W) and each frame
//     stores the pixels whose column falls inside it -- one extra pass for the one wave in ~5 that holds a row end;
//   * weights arrive through the scalar cache (one s_load_dwordx16 = the wave's 16 channels of one (tap, ci)) and feed
//     v_pk_fma_f32 on channel pairs; the input pixel is picked out of a column-pair register with op_sel, so one scalar
//     load feeds 32 packed FMAs.  (The first version, one pixel x 64 channels per lane, needed 64 B of scalar loads per
//     8 FMAs and was bound by the scalar cache as well as by its 256-B stores.)
constexpr int STEM_PX = 4, STEM_CH = 16;
typedef float stem_f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float stem_f2 __attribute__((ext_vector_type(2)));
typedef float stem_f16 __attribute__((ext_vector_type(16)));

template <int CIN>
__global__ __launch_bounds__(256, 3) void conv3x3_stem_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                              const float* __restrict__ bias, float* __restrict__ y,
                                                              int Cin, int Cout, int H, int W, int coTiles, int relu)
{
    constexpr int BM = 64;
    const int lane = threadIdx.x & 63;
    const int cg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // this wave's 16-channel group
    const int HW = H * W, n = blockIdx.y;
    const int i0 = (blockIdx.x * 64 + lane) * STEM_PX;                     // first flat pixel index of this lane
    const int y0 = i0 / W, x0 = i0 - y0 * W;
    const int cnt = min(STEM_PX, HW - i0);                                 // pixels inside the plane (<= 0: idle lane)
    const int frames = cnt > 0 ? (i0 + cnt - 1) / W - y0 + 1 : 0;          // rows this lane's pixels touch
    const float* xn = x + (size_t)n * Cin * HW;
    float* yn = y + (size_t)n * Cout * HW + i0;
    // Input window of the block, staged once for its four waves: for (ci, ky) the flat input range
    // [b0 + (ky - 1) W - 1, + 64 STEM_PX + 2) is contiguous; what a lane needs sits at 4 lane .. 4 lane + 5 of it.  Row and
    // column padding is applied when the window is read (a flat neighbour beyond a row end is the next row's pixel).
    constexpr int TW = 64 * STEM_PX + 8;
    __shared__ __attribute__((aligned(16))) float tile[CIN * 3][TW];
    {
        const long long b0 = (long long)blockIdx.x * 64 * STEM_PX - 1;
        float stage[CIN * 3], extra = 0.f;
#pragma unroll
        for (int r = 0; r < CIN * 3; ++r) {                // all loads in flight before the first LDS write
            const long long g = b0 + (long long)(r % 3 - 1) * W + threadIdx.x;
            stage[r] = (r / 3 < Cin && g >= 0 && g < HW) ? xn[(size_t)(r / 3) * HW + g] : 0.f;
        }
        if (threadIdx.x < CIN * 3 * 2) {                   // the two trailing columns of each row
            const int r = threadIdx.x >> 1;
            const long long g = b0 + (long long)(r % 3 - 1) * W + 64 * STEM_PX + (threadIdx.x & 1);
            extra = (r / 3 < Cin && g >= 0 && g < HW) ? xn[(size_t)(r / 3) * HW + g] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < CIN * 3; ++r) tile[r][threadIdx.x] = stage[r];
        if (threadIdx.x < CIN * 3 * 2) tile[threadIdx.x >> 1][64 * STEM_PX + (threadIdx.x & 1)] = extra;
    }
    __syncthreads();
    for (int f = 0; __builtin_amdgcn_ballot_w64(f < frames) != 0; ++f) {   // wave-uniform trip count
        if (f >= frames) continue;
        const int py = y0 + f, px0 = x0 - f * W;                           // pixel p of the lane has column px0 + p in this frame
        bool cok[STEM_PX + 2];
#pragma unroll
        for (int j = 0; j < STEM_PX + 2; ++j) cok[j] = px0 - 1 + j >= 0 && px0 - 1 + j < W;
        const bool full = px0 >= 0 && px0 + STEM_PX <= W;                  // all four pixels in this row
#pragma unroll 1
        for (int cot = 0; cot < coTiles; ++cot) {
            const int co0 = cot * BM + cg * STEM_CH;
            const float* wt = wp + (size_t)cot * 9 * 4 * BM + cg * STEM_CH;     // packed [tap][ci (4)][64 channels]
            stem_f2 acc[STEM_PX][STEM_CH / 2];             // channel pairs: v_pk_fma_f32 with an SGPR weight pair
#pragma unroll
            for (int c = 0; c < STEM_CH / 2; ++c) {
                stem_f2 b;
                b.x = (co0 + 2 * c < Cout) ? bias[co0 + 2 * c] : 0.f;
                b.y = (co0 + 2 * c + 1 < Cout) ? bias[co0 + 2 * c + 1] : 0.f;
#pragma unroll
                for (int p = 0; p < STEM_PX; ++p) acc[p][c] = b;
            }
            // one s_load_dwordx16 per (tap, ci), requested one step ahead of its use
            stem_f16 wnext = *reinterpret_cast<const stem_f16*>(wt);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                // this kernel row's inputs: [ci][column pair] = columns px0 - 1 + 2j, px0 + 2j of row py + ky - 1
                stem_f2 v[CIN][STEM_PX / 2 + 1];
                const bool rok = py + ky - 1 >= 0 && py + ky - 1 < H;
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) {
                    const float4 q0 = *reinterpret_cast<const float4*>(&tile[ci * 3 + ky][lane * STEM_PX]);
                    const float2 q1 = *reinterpret_cast<const float2*>(&tile[ci * 3 + ky][lane * STEM_PX + 4]);
                    const float t[6] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y};
#pragma unroll
                    for (int j = 0; j < STEM_PX + 2; ++j) {
                        const float u = (rok && cok[j]) ? t[j] : 0.f;
                        if (j & 1) v[ci][j >> 1].y = u; else v[ci][j >> 1].x = u;
                    }
                }
#pragma unroll
                for (int s9 = 0; s9 < 3 * CIN; ++s9) {     // (channels >= Cin: zero inputs against zero weights)
                    const int kx = s9 / CIN, ci = s9 % CIN, step = ky * 3 * CIN + s9;
                    const stem_f16 wcur = wnext;
                    if (step + 1 < 9 * CIN)
                        wnext = *reinterpret_cast<const stem_f16*>(wt + (((step + 1) / CIN) * 4 + (step + 1) % CIN) * BM);
#pragma unroll
                    for (int c = 0; c < STEM_CH / 2; ++c) {
                        const stem_f2 wv = {wcur[2 * c], wcur[2 * c + 1]};
#pragma unroll
                        for (int p = 0; p < STEM_PX; ++p) {
                            // acc.{x,y} = fma(w.{x,y}, x, acc.{x,y}) with x one half of an input column pair,
                            // selected for both result halves by op_sel (no duplicated input registers)
                            if ((p + kx) & 1)
                                asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]"
                                             : "+v"(acc[p][c]) : "s"(wv), "v"(v[ci][(p + kx) >> 1]));
                            else
                                asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]"
                                             : "+v"(acc[p][c]) : "s"(wv), "v"(v[ci][(p + kx) >> 1]));
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < STEM_CH; ++c) {
                if (co0 + c >= Cout) continue;
                float* dst = yn + (size_t)(co0 + c) * HW;
                float o[STEM_PX];
#pragma unroll
                for (int p = 0; p < STEM_PX; ++p) {
                    const float a = (c & 1) ? acc[p][c >> 1].y : acc[p][c >> 1].x;
                    o[p] = relu ? fmaxf(a, 0.f) : a;
                }
                if (full) {
                    stem_f4u q = {o[0], o[1], o[2], o[3]};
                    *reinterpret_cast<stem_f4u*>(dst) = q;  // 16-B aligned whenever H W % 4 == 0 and y is
                } else {
#pragma unroll
                    for (int p = 0; p < STEM_PX; ++p)
                        if (px0 + p >= 0 && px0 + p < W) dst[p] = o[p];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------ weight pack
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int wCout,
                                    int wCin, int mode, int BM, int CK, int coTiles, int nChunks)
{
    const int64_t total = (int64_t)coTiles * nChunks * 9 * CK * BM;
    const int convCout = mode ? wCin : wCout, convCin = mode ? wCout : wCin;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = i;
        const int col = t % BM; t /= BM;
        const int cil = t % CK; t /= CK;
        const int tap = t % 9; t /= 9;
        const int chunk = t % nChunks;
        const int cot = t / nChunks;
        const int co = cot * BM + col, ci = chunk * CK + cil;
        float v = 0.f;
        if (co < convCout && ci < convCin) {
            const int ky = tap / 3, kx = tap % 3;
            if (mode == 0) v = w[((size_t)co * wCin + ci) * 9 + tap];
            else v = w[((size_t)ci * wCin + co) * 9 + (2 - ky) * 3 + (2 - kx)];
        }
        wp[i] = v;
    }
}
// ------------------------------------------------------------------------------------ wgrad, buffer-DMA pipeline
// Third-generation wgrad main loop (default).  Measured with clock64() probes (tools/exp_wgrad_timing.py): in the
// kernel above a wave spends as long issuing its 16 dword DMAs per stage (address VALU work that has to win issue
// slots against three MFMA-streaming waves) as it spends in its MFMA block.  This kernel removes that work:
//   * DMAs are `buffer_load_dwordx4 ... lds` (raw buffer -> LDS, 16 B per lane): the per-lane byte offset is a
//     loop-invariant VGPR, the tile origin lives in the (scalar) buffer descriptor, and lanes whose piece is
//     padding / outside the image carry offset 0xFFFFFFFF, which the buffer range check turns into zeros without
//     touching memory.  4-5 DMA instructions per wave per stage instead of 16, no per-DMA VALU in the common case.
//   * the MFMA k index is permuted (lane half h, step j <-> pixel 16h + j) so that every lane's A and B operands
//     are *contiguous* in LDS: 4 + 2 x 6 wide LDS reads per stage instead of 88 ds_read_b32, and the B row is
//     reused across the three kx taps from registers.
//   * pitches are odd multiples of 16 B (36 / 124 floats), conflict-free for ds_read_b128.
// LDS column m of an X row holds image column x0 - 4 + m, so the left halo is a whole (invalid) 16-B piece; pieces
// that straddle the right image edge are loaded as they lie and the stale lanes are zeroed in registers (only in
// the right-edge tile of each row).
constexpr int WB_DYP = 36;                  // dY row pitch: 8 data pieces + 1 pad piece
constexpr int WB_DY = 128 * WB_DYP;         // 4608 floats = 1152 pieces (18 waves' worth)
constexpr int WB_XROW = 40;                 // X row pitch: 10 pieces = image columns x0-4 .. x0+35
constexpr int WB_XPL = 124;                 // X plane pitch: 3 rows + 1 pad piece = 31 pieces
constexpr int WB_X = 1024 * 4;              // 32 planes x 31 pieces = 992 pieces, rounded to 16 waves' worth
constexpr int WB_STAGE = WB_DY + WB_X;      // 8704 floats = 34 KB; double buffered, two workgroups per CU

typedef __attribute__((address_space(3))) f32x4 lds_f32x4_t;
typedef __attribute__((address_space(3))) float lds_f32_t;
__device__ __forceinline__ void bdma16(__amdgpu_buffer_rsrc_t r, unsigned voff, float* lds_wave_base)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_b_t*)lds_wave_base, 16, (int)voff, 0, 0, 0);
}

template <int G>
__device__ __forceinline__ void wgrad_stage_buf(const float* __restrict__ al, const float* __restrict__ bl,
                                                f32x16 (&acc)[G == 0 ? 5 : 4])
{
    constexpr int TAP0 = G == 0 ? 0 : 5, TAP1 = G == 0 ? 5 : 9;
    float a[16];                                       // dY of this lane's 16 pixels 16h + 0..15
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(al + 4 * t);
        a[4 * t] = v.x; a[4 * t + 1] = v.y; a[4 * t + 2] = v.z; a[4 * t + 3] = v.w;
    }
#pragma unroll
    for (int ky = (G == 0 ? 0 : 1); ky < (G == 0 ? 2 : 3); ++ky) {
        // image columns x0 + 16h - 1 .. + 16 -> v[0..17]: four aligned 16-B reads and the two end words, ONCE for both
        // 8-pixel halves (the single-word reads are the ones that collide in the banks: plane pitch 124 = 4 * 31 words).
        // volatile + LDS address space keep the reads as written (the optimiser otherwise narrows the 16-B reads to
        // the lanes used and re-pairs the remains into 8-B reads).
        float v[18];
        const float* br = bl + ky * WB_XROW + 4;
        v[0] = *(const volatile lds_f32_t*)(br - 1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 q = *(const volatile lds_f32x4_t*)(br + 4 * t);
            v[1 + 4 * t] = q[0]; v[2 + 4 * t] = q[1]; v[3 + 4 * t] = q[2]; v[4 + 4 * t] = q[3];
        }
        v[17] = *(const volatile lds_f32_t*)(br + 16);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {               // pixels 16h + 8*hf + j, j = 0..7
#pragma unroll
            for (int j = 0; j < 8; ++j) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int tap = ky * 3 + kx;
                    if (tap >= TAP0 && tap < TAP1)
                        acc[tap - TAP0] = mfma32(a[8 * hf + j], v[8 * hf + j + kx], acc[tap - TAP0]);
                }
            }
        }
    }
}

// Right-edge stage with few valid columns (wv <= 24): the k index is interleaved instead (lane half h, step j <->
// pixel 2j + h), so only ceil(wv / 2) MFMA steps are issued instead of 16.  Operands are single-word LDS reads here.
template <int G>
__device__ __forceinline__ void wgrad_stage_edge(const float* __restrict__ al0, const float* __restrict__ bl0,
                                                 f32x16 (&acc)[G == 0 ? 5 : 4], int nj)
{
    constexpr int TAP0 = G == 0 ? 0 : 5, TAP1 = G == 0 ? 5 : 9;
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
        const float a = al0[2 * j];
#pragma unroll
        for (int ky = (G == 0 ? 0 : 1); ky < (G == 0 ? 2 : 3); ++ky) {
            const float* br = bl0 + ky * WB_XROW + 2 * j + 3;          // image column x0 + (2j + h) - 1
            const float v0 = br[0], v1 = br[1], v2 = br[2];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tap = ky * 3 + kx;
                if (tap >= TAP0 && tap < TAP1) acc[tap - TAP0] = mfma32(a, kx == 0 ? v0 : (kx == 1 ? v1 : v2), acc[tap - TAP0]);
            }
        }
    }
}

// one tap group's whole life: descriptors, stage loop, partial store.  Instantiated twice and selected by a
// wave-uniform branch so that each group gets its own register allocation (5 or 4 accumulator tiles).
template <int G, bool EDGE>
__device__ __forceinline__ void wgrad_buf_body(float* lds, const float* __restrict__ x, const float* __restrict__ dy,
                                               float* __restrict__ partial, int N, int Cin, int Cout, int H, int W,
                                               int tilesX, int tilesY, int ciTiles, int S, int txb, int bid, int wave,
                                               int lane)
{
    constexpr int NT = G == 0 ? 5 : 4;
    const int cw = wave & 3;
    const int s = bid % S; bid /= S;
    const int cit = bid % ciTiles;
    const int cot = bid / ciTiles;
    const int HW = H * W;
    const int co0 = cot * 128, ci0 = cit * 32;
    const int nTiles = N * tilesY * tilesX;
    const char* x_end = (const char*)(x + (size_t)N * Cin * HW);
    const char* dy_end = (const char*)(dy + (size_t)N * Cout * HW);

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x16){0};

    // Loop-invariant piece descriptors.  dY: instruction i covers pieces (i*8 + wave)*64 + lane; piece = row*9 + q.
    // X: pieces (i*8 + wave)*64 + lane; piece = plane*31 + r*10 + q.  Byte offsets from the tile's base pointer,
    // 0xFFFFFFFF = never loaded.  dqp / xrqp keep the pieces' column (and row) for the per-tile validity test.
    unsigned dvoff[3], xvoff[2];
    unsigned dqp = 0, xrqp = 0;          // packed per piece: dY column (6 bits); X row (2 bits) | column + 4 (6 bits)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int pc = (i * 8 + wave) * 64 + lane;
        const int row = pc / 9, q = pc - row * 9;
        const bool ok = pc < 1152 && q < 8 && (co0 + row) < Cout;
        dvoff[i] = ok ? (unsigned)(row * HW + 4 * q) * 4u : 0xFFFFFFFFu;
        dqp |= (unsigned)(4 * q) << (8 * i);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pc = (i * 8 + wave) * 64 + lane;
        const int pl = pc / 31, rem = pc - pl * 31;
        const int r = rem / 10, q = rem - r * 10;
        const bool ok = pc < 992 && rem < 30 && (ci0 + pl) < Cin;
        xvoff[i] = ok ? (unsigned)(pl * HW + r * W + 4 * q) * 4u : 0xFFFFFFFFu;
        xrqp |= ((unsigned)(4 * q) | ((unsigned)r << 6)) << (8 * i);
    }

    // tile walk: tile = s, s + S, ... decomposed once into (n, ty, tx) and advanced with carries (no divisions)
    int tx = s % tilesX, ty = (s / tilesX) % tilesY, n = s / (tilesX * tilesY);
    const int sx = S % tilesX, sy = (S / tilesX) % tilesY, sn = S / (tilesX * tilesY);

    auto issue = [&](int n_, int ty_, int tx_, int buf) {
        const int x0 = (txb + tx_) * TW, y0 = ty_;
        const float* dyn = dy + ((size_t)n_ * Cout + co0) * HW + (size_t)y0 * W + x0;
        const float* xb = x + ((size_t)n_ * Cin + ci0) * HW + ((ptrdiff_t)y0 - 1) * W + (x0 - 4);
        const long long drem = dy_end - (const char*)dyn, xrem = x_end - (const char*)xb;
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
            (void*)dyn, 0, (int)(drem > 0xFFFFFFFEll ? 0xFFFFFFFEll : drem), 0x00020000);
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
            (void*)xb, 0, (int)(xrem > 0xFFFFFFFEll ? 0xFFFFFFFEll : xrem), 0x00020000);
        float* Dd = lds + buf * WB_STAGE + wave * 256;
        float* Xd = lds + buf * WB_STAGE + WB_DY + wave * 256;
        const int wv = W - x0;                                   // valid columns right of x0
        const bool plain = y0 > 0 && y0 < H - 1 && x0 > 0 && wv >= 36;
        if (plain) {
            bdma16(rd, dvoff[0], Dd);
            bdma16(rd, dvoff[1], Dd + 8 * 256);
            if (wave < 2) bdma16(rd, dvoff[2], Dd + 16 * 256);
            bdma16(rx, xvoff[0], Xd);
            bdma16(rx, xvoff[1], Xd + 8 * 256);
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int q4 = (dqp >> (8 * i)) & 63;
                if (i < 2 || wave < 2) bdma16(rd, q4 < wv ? dvoff[i] : 0xFFFFFFFFu, Dd + i * 8 * 256);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int gy = y0 - 1 + (int)((xrqp >> (8 * i + 6)) & 3);
                const int q4 = (int)((xrqp >> (8 * i)) & 63) - 4;
                const bool ok = gy >= 0 && gy < H && (x0 + q4) >= 0 && q4 < wv;
                bdma16(rx, ok ? xvoff[i] : 0xFFFFFFFFu, Xd + i * 8 * 256);
            }
        }
    };

    const int h16 = (lane >> 5) * 16;
    const int a_off = (cw * 32 + (lane & 31)) * WB_DYP + h16;
    const int b_off = WB_DY + (lane & 31) * WB_XPL + h16;       // LDS column 16h <-> image column x0 + 16h - 4

    int tile = s, it = 0;
    if (tile < nTiles) issue(n, ty, tx, 0);
    for (; tile < nTiles; tile += S, ++it) {
        const int buf = it & 1;
        const int wv = W - (txb + tx) * TW;                      // valid columns of this stage's tile
        int ntx = tx + sx, nty = ty + sy, nn = n + sn;
        if (ntx >= tilesX) { ntx -= tilesX; ++nty; }
        if (nty >= tilesY) { nty -= tilesY; ++nn; }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wv < 33) {
            // right-edge tile: the pieces this lane loaded that straddle the image edge carry the next row's
            // first pixels in their tail; zero those LDS words (own pieces only, so no barrier is needed first)
            float* Db = lds + buf * WB_STAGE + (wave * 64 + lane) * 4;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int q4 = (dqp >> (8 * i)) & 63;
                if ((i < 2 || wave < 2) && q4 < wv && q4 + 4 > wv && dvoff[i] != 0xFFFFFFFFu) {
#pragma unroll
                    for (int e = 1; e < 4; ++e)
                        if (q4 + e >= wv) Db[i * 8 * 256 + e] = 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int q4 = (int)((xrqp >> (8 * i)) & 63) - 4;
                if (q4 < wv && q4 + 4 > wv && xvoff[i] != 0xFFFFFFFFu) {
#pragma unroll
                    for (int e = 1; e < 4; ++e)
                        if (q4 + e >= wv) Db[WB_DY + i * 8 * 256 + e] = 0.f;
                }
            }
        }
        __syncthreads();
        if (tile + S < nTiles) issue(nn, nty, ntx, buf ^ 1);
        if (!EDGE)
            wgrad_stage_buf<G>(lds + buf * WB_STAGE + a_off, lds + buf * WB_STAGE + b_off, acc);
        else
            wgrad_stage_edge<G>(lds + buf * WB_STAGE + a_off - h16 + (lane >> 5), lds + buf * WB_STAGE + b_off - h16 + (lane >> 5),
                                acc, (wv + 1) >> 1);
        tx = ntx; ty = nty; n = nn;
    }
    const int ci = ci0 + (lane & 31);
    constexpr int tap0 = G == 0 ? 0 : 5;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        float* dst = partial + ((size_t)s * 9 + tap0 + t) * Cout * Cin;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (co < Cout && ci < Cin) dst[(size_t)co * Cin + ci] = acc[t][r];
        }
    }
}

// One launch, two kinds of workgroups.  Workgroups 0 .. nMain-1 walk tile columns 0 .. tilesXm-1 with the full 16-step
// stage (split-K factor S).  When the last tile of a row has <= 24 valid columns (nEdge > 0), tilesXm excludes it and
// workgroups nMain .. nMain+nEdge-1 walk that column alone with the interleaved short stage (split-K factor Se, partials
// after the main ones in the workspace).  The short-stage workgroups are latency-bound (few MFMAs per DMA round trip);
// dispatched after the main ones they fill the tail of the launch instead of costing a launch of their own.
__global__ __launch_bounds__(512, 4) void conv3x3_wgrad_buf_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ partial, int N, int Cin,
    int Cout, int H, int W, int tilesXm, int tilesY, int coTiles, int ciTiles, int S, int nMain, int Se)
{
    __shared__ __attribute__((aligned(16))) float lds[2 * WB_STAGE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bid = blockIdx.x;
    if (bid < nMain) {
        if (wave < 4) wgrad_buf_body<0, false>(lds, x, dy, partial, N, Cin, Cout, H, W, tilesXm, tilesY, ciTiles, S, 0, bid, wave, lane);
        else wgrad_buf_body<1, false>(lds, x, dy, partial, N, Cin, Cout, H, W, tilesXm, tilesY, ciTiles, S, 0, bid, wave, lane);
    } else {
        float* pe = partial + (size_t)S * 9 * Cout * Cin;
        if (wave < 4) wgrad_buf_body<0, true>(lds, x, dy, pe, N, Cin, Cout, H, W, 1, tilesY, ciTiles, Se, tilesXm, bid - nMain, wave, lane);
        else wgrad_buf_body<1, true>(lds, x, dy, pe, N, Cin, Cout, H, W, 1, tilesY, ciTiles, Se, tilesXm, bid - nMain, wave, lane);
    }
}

__global__ void wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw, int Cout,
                                    int Cin, int S, int accumulate)
{
    const int64_t total = (int64_t)Cout * Cin * 9;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        // i indexes partial layout [tap][co][ci] for coalesced reads
        const int64_t cc = (int64_t)Cout * Cin;
        const int tap = i / cc;
        const int64_t rem = i - tap * cc;
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += partial[((size_t)s * 9 + tap) * cc + rem];
        const size_t o = (size_t)rem * 9 + tap;
        dw[o] = accumulate ? dw[o] + sum : sum;
    }
}

// db[co] = sum_{n,p} dy[n][co][p]: stage 1 = one workgroup per (channel, image slot) -> partial[c][slot];
// stage 2 = fixed-order sum over the slots (deterministic).
constexpr int BG_SLOTS = 16;

__global__ __launch_bounds__(256) void bias_grad_partial_kernel(const float* __restrict__ dy, float* __restrict__ part,
                                                                int N, int C, int HW)
{
    __shared__ float sm[4];
    auto rd = [](float v) { return v; };
    const int c = blockIdx.x, slot = blockIdx.y;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int n = slot; n < N; n += BG_SLOTS) {
        const float* p = dy + ((size_t)n * C + c) * HW;
        int i = threadIdx.x;
        for (; i + 768 < HW; i += 1024) {
            a0 += rd(p[i]);
            a1 += rd(p[i + 256]);
            a2 += rd(p[i + 512]);
            a3 += rd(p[i + 768]);
        }
        for (; i < HW; i += 256) a0 += rd(p[i]);
    }
    const float t = block_sum_256((a0 + a1) + (a2 + a3), sm);
    if (threadIdx.x == 0) part[c * BG_SLOTS + slot] = t;
}

__global__ void bias_grad_final_kernel(const float* __restrict__ part, float* __restrict__ db, int C, int accumulate)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float t = 0.f;
#pragma unroll
    for (int s = 0; s < BG_SLOTS; ++s) t += part[c * BG_SLOTS + s];
    db[c] = accumulate ? db[c] + t : t;
}

__global__ void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                float* __restrict__ dz, int64_t n)
{
    const int64_t n4 = n >> 2;
    const float4* dy4 = reinterpret_cast<const float4*>(dy);
    const float4* y4 = reinterpret_cast<const float4*>(y);
    float4* dz4 = reinterpret_cast<float4*>(dz);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * blockDim.x) {
        float4 g = dy4[i];
        const float4 v = y4[i];
        g.x = v.x > 0.f ? g.x : 0.f;
        g.y = v.y > 0.f ? g.y : 0.f;
        g.z = v.z > 0.f ? g.z : 0.f;
        g.w = v.w > 0.f ? g.w : 0.f;
        dz4[i] = g;
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        dz[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// split-K factor of the right-edge workgroups of the wgrad launch (0 = the edge tile column is handled by the main ones)
int wgrad_edge_splits(int n, int cin, int cout, int h, int w)
{
    const int tilesX = cdiv(w, TW), wv = w - (tilesX - 1) * TW;
    if (tilesX < 2 || wv > 24) return 0;
    const int base = cdiv(cout, 128) * cdiv(cin, 32);
    const int64_t nTiles = (int64_t)n * h;
    int S = cdiv(512, base);
    if (S > nTiles) S = (int)nTiles;
    return S < 1 ? 1 : S;
}

int wgrad_splits(int n, int cin, int cout, int h, int w)
{
    const int tilesX = cdiv(w, TW), tilesY = h;
    const int64_t nTiles = (int64_t)n * tilesX * tilesY;
    const int base = cdiv(cout, 128) * cdiv(cin, 32);
    int S = cdiv(1024, base);
    if (S > nTiles) S = (int)nTiles;
    if (S < 1) S = 1;
    if (S > 256) S = 256;
    return S;
}

int conv3x3_fwd_impl(const float* x, const float* wp, const float* bias, const float* mask_ref, float* y, int n,
                     int cin, int cout, int h, int w, int epilogue, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(x && wp && y && n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "conv3x3_fwd: bad args");
    PTMI_CHECK_ARG(epilogue >= 0 && epilogue <= 4, "conv3x3_fwd: bad epilogue %d", epilogue);
    // the buffer-DMA kernels address one image through 32-bit byte offsets and a 16-bit grid dimension: reject (loudly)
    // anything larger -- 1333x800 VGG maps use at most 273 MB per image
    PTMI_CHECK_ARG((int64_t)cin * h * w * 4 < (1ll << 32) && ((int64_t)cout + 128) * h * w * 4 < (1ll << 32) &&
                   (int64_t)n * cdiv(h, 4) < 65536, "conv3x3_fwd: image too large for 32-bit buffer offsets "
                   "(n=%d cin=%d cout=%d h=%d w=%d)", n, cin, cout, h, w);
    PTMI_CHECK_ARG(epilogue > 1 || bias, "conv3x3_fwd: bias required for epilogue %d", epilogue);
    PTMI_CHECK_ARG(epilogue != 3 || mask_ref, "conv3x3_fwd: mask_ref required for epilogue 3");
    const int BM = ptmi_conv3x3_bm(cout), CK = ptmi_conv3x3_ck(cin);
    // 8-wave workgroups (8 rows x 32 cols per 128 channels) share one weight slab among twice the pixels:
    // A/B +3.5 % at 400x666, -3 .. -14 % on the small maps
    const bool use8 = BM == 128 && cin > 4 && h >= 200;
    const int TH = (BM == 128 && !use8) ? 4 : 8;
    const int tilesX = cdiv(w, TW), tilesY = cdiv(h, TH), coTiles = cdiv(cout, BM), nChunks = cdiv(cin, CK);
    hipStream_t st = (hipStream_t)s;
    // 3-channel stem: K = 27 is too short to amortise the LDS pipeline's prologue and the layer is HBM-write bound
    if (BM == 64 && cin <= 4 && epilogue <= 1) {
        // (-ffp-contract=off: fmaf() is explicit in the kernel; K = 27 keeps the rounding difference at the 1e-7 level)
        PTMI_CHECK_ARG(n < 65536 && (int64_t)h * w < (int64_t)1 << 30, "conv3x3_fwd(stem): grid too large");
        const dim3 gs((unsigned)cdiv(h * w, 64 * STEM_PX), (unsigned)n);
        if (cin <= 3)
            hipLaunchKernelGGL(conv3x3_stem_kernel<3>, gs, dim3(256), 0, st, x, wp, bias, y, cin, cout, h, w, coTiles, epilogue == 1);
        else
            hipLaunchKernelGGL(conv3x3_stem_kernel<4>, gs, dim3(256), 0, st, x, wp, bias, y, cin, cout, h, w, coTiles, epilogue == 1);
        PTMI_LAUNCH_CHECK("conv3x3_fwd(stem)");
        return 0;
    }
    const dim3 grid3((unsigned)coTiles, (unsigned)(n * tilesY), (unsigned)tilesX);
#define LBUF(BM_, NW_)                                                                                                 \
    hipLaunchKernelGGL((conv3x3_buf_kernel<BM_, NW_>), grid3, dim3(64 * NW_), 0, st, x, wp, bias, mask_ref, y, n, cin, cout, h, \
                       w, tilesX, tilesY, coTiles, nChunks, epilogue)
    if (BM == 128 && use8) LBUF(128, 8);
    else if (BM == 128) LBUF(128, 4);
    else LBUF(64, 4);
#undef LBUF
    PTMI_LAUNCH_CHECK("conv3x3_fwd(buf)");
    return 0;
}

int conv3x3_wgrad_impl(const float* x, const float* dy, float* dw, float* db, float* ws, int n, int cin,
                       int cout, int h, int w, int accumulate, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(x && dy && dw && ws && n > 0 && cin > 0 && cout > 0, "conv3x3_wgrad: bad args");
    PTMI_CHECK_ARG((int64_t)128 * h * w < (1 << 28), "conv3x3_wgrad: map %dx%d too large for 32-bit buffer offsets", h, w);
    const int tilesX = cdiv(w, TW), tilesY = h;
    const int coTiles = cdiv(cout, 128), ciTiles = cdiv(cin, 32);
    int S = wgrad_splits(n, cin, cout, h, w);
    const int Se = wgrad_edge_splits(n, cin, cout, h, w);
    const int64_t bg_off = (int64_t)(S + wgrad_edge_splits(n, cin, cout, h, w)) * 9 * cout * cin;   // as ptmi_conv3x3_wgrad_ws_floats lays it out
    hipStream_t st = (hipStream_t)s;
    // Se > 0: the right-edge tile column has few valid pixels and gets the short interleaved stage
    const int nMain = coTiles * ciTiles * S, nEdge = coTiles * ciTiles * Se;
    hipLaunchKernelGGL(conv3x3_wgrad_buf_kernel, dim3(nMain + nEdge), dim3(512), 0, st, x, dy, ws, n, cin, cout, h, w,
                       Se > 0 ? tilesX - 1 : tilesX, tilesY, coTiles, ciTiles, S, nMain, Se);
    S += Se;
    PTMI_LAUNCH_CHECK("conv3x3_wgrad");
    const int64_t total = (int64_t)cout * cin * 9;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, dw,
                       cout, cin, S, accumulate);
    PTMI_LAUNCH_CHECK("conv3x3_wgrad_reduce");
    if (db) {
        float* part = ws + bg_off + 64;
        hipLaunchKernelGGL(bias_grad_partial_kernel, dim3(cout, BG_SLOTS), dim3(256), 0, st, dy, part, n, cout, h * w);
        PTMI_LAUNCH_CHECK("conv3x3_bias_grad_partial");
        hipLaunchKernelGGL(bias_grad_final_kernel, dim3(cdiv(cout, 256)), dim3(256), 0, st, part, db, cout, accumulate);
        PTMI_LAUNCH_CHECK("conv3x3_bias_grad_final");
    }
    return 0;
}

}  // namespace

extern "C" {

int ptmi_conv3x3_bm(int cout) { return cout <= 64 ? 64 : 128; }
int ptmi_conv3x3_ck(int cin) { (void)cin; return 4; }

int64_t ptmi_conv3x3_packed_floats(int cin, int cout)
{
    const int BM = ptmi_conv3x3_bm(cout), CK = ptmi_conv3x3_ck(cin);
    return (int64_t)cdiv(cout, BM) * cdiv(cin, CK) * 9 * CK * BM;
}

int ptmi_conv3x3_pack_weights(const float* w, float* wp, int w_cout, int w_cin, int mode,
                              ptmi_stream_t s)
{
    PTMI_CHECK_ARG(w && wp && w_cout > 0 && w_cin > 0, "conv3x3_pack_weights: bad args");
    const int convCout = mode ? w_cin : w_cout, convCin = mode ? w_cout : w_cin;
    const int BM = ptmi_conv3x3_bm(convCout), CK = ptmi_conv3x3_ck(convCin);
    const int coTiles = cdiv(convCout, BM), nChunks = cdiv(convCin, CK);
    const int64_t total = (int64_t)coTiles * nChunks * 9 * CK * BM;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, w, wp, w_cout,
                       w_cin, mode, BM, CK, coTiles, nChunks);
    PTMI_LAUNCH_CHECK("conv3x3_pack_weights");
    return 0;
}

int ptmi_conv3x3_fwd(const float* x, const float* wp, const float* bias, const float* mask_ref,
                     float* y, int n, int cin, int cout, int h, int w, int epilogue, ptmi_stream_t s)
{
    return conv3x3_fwd_impl(x, wp, bias, mask_ref, y, n, cin, cout, h, w, epilogue, s);
}

int64_t ptmi_conv3x3_wgrad_ws_floats(int n, int cin, int cout, int h, int w)
{
    // split-K partials (main + right-edge workgroups) + bias-gradient partials
    return (int64_t)(wgrad_splits(n, cin, cout, h, w) + wgrad_edge_splits(n, cin, cout, h, w)) * 9 * cout * cin + 64 +
           (int64_t)cout * BG_SLOTS;
}

int ptmi_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws, int n, int cin,
                       int cout, int h, int w, int accumulate, ptmi_stream_t s)
{
    return conv3x3_wgrad_impl(x, dy, dw, db, ws, n, cin, cout, h, w, accumulate, s);
}

int ptmi_relu_bwd(const float* dy, const float* y, float* dz, int64_t numel, ptmi_stream_t s)
{
    PTMI_CHECK_ARG(dy && y && dz && numel >= 0, "relu_bwd: bad args");
    if (numel == 0) return 0;
    int64_t blocks = (numel / 4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, dy, y, dz, numel);
    PTMI_LAUNCH_CHECK("relu_bwd");
    return 0;
}

}  // extern "C"
