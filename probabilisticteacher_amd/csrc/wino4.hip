// wino4.hip -- fused Winograd F(4x4, 3x3) convolution for gfx950 (CDNA4): 3x3 s1 p1, fp32 in / fp32 accumulate on
// v_mfma_f32_16x16x4_f32: forward and dgrad of the fp32 layers with many input channels (round 5).
//
// Replaces the cuDNN conv2d (+bias, +ReLU) the reference reaches at pt/modeling/backbone/vgg.py:45-53,66-69 and the 3x3 conv of
// D2's StandardRPNHead (pt/modeling/proposal_generator/rpn.py:96), like wino.hip -- with 36 instead of 64 transform-domain
// products per 4x4 outputs (F(2x2,3x3): 16 per 2x2), i.e. 1.78x fewer MFMAs; the direct algorithm needs 144.
//
// Interpolation points 0, +-3/4, +-3/2, inf (NOT the textbook 0, +-1, +-2: on fp32 the textbook set's inverse transform
// multiplies by up to 8 x 8 and its error against an fp64 convolution is 4e-5 at 512 channels; this set measures 1.2e-5
// max / 1.2e-6 rms, F(2x2,3x3) 2.3e-6 / 4e-7, direct fp32 1.2e-6 / 1.8e-7 -- tools/exp/wino4_numerics.py).  Every constant
// of B^T and A^T is exact in fp32:
//   B^T (6x6), row order (0, +a, -a, +b, -b, inf), a = 3/4, b = 3/2:
//       [a2b2, 0, -(a2+b2), 0, 1, 0]  [0, -ab2, -b2, a, 1, 0]  [0, ab2, -b2, -a, 1, 0]
//       [0, -a2b, -a2, b, 1, 0]  [0, a2b, -a2, -b, 1, 0]  [0, a2b2, 0, -(a2+b2), 0, 1]
//   A^T (4x6) = rows [p^k] over the same points (last column (0,0,0,1)); G (6x3) is whatever makes the identity hold:
//       [64/81,0,0] [-128/243,-32/81,-8/27] [-128/243,32/81,-8/27] [32/243,16/81,8/27] [32/243,-16/81,8/27] [0,0,1]
//   (G g G^T is evaluated in double by the pack kernel and rounded once).
//
// One kernel, nothing in HBM but x, the packed weights and y:
//   * M_p[co][tile] = sum_ci U_p[co][ci] V_p[ci][tile] for the 36 positions p = 6 i + j; a workgroup = 4 wave64s owns 64
//     output channels x (8 rows x 64 columns) = 2 x 16 tiles of the FLAT tile line of wino.hip (every (image, 8-row band) is a
//     strip of `period` columns; strips concatenated; a workgroup may straddle strips); a wave owns 32 channels x 16 tiles
//     (one tile row) x ALL 36 positions = 72 accumulator tiles of 16x16 = 288 registers: 256 AGPRs + 32 VGPRs, which is why
//     the MFMAs are inline asm ("+a" / "+v" on f32x4): the compiler picks one register class per function for the builtin;
//   * v_mfma_f32_16x16x4_f32 takes A[co = lane & 15][k = lane >> 4], B[k = lane >> 4][tile = lane & 15]: a lane IS one
//     (tile, input channel) pair, reads its own 6x6 window from the LDS patch (per row: b32 + b128 + b32), transforms it in
//     registers (12 FMAs per 1-D transform, 144 per window) and holds the B operands of all 36 positions; each feeds TWO
//     MFMAs (the wave's two 16-channel tiles).  The A operands are 16-byte reads of four positions of one channel;
//   * K is walked in chunks of 4 channels = ONE MFMA K = 72 MFMAs per wave (2304 matrix-pipe cycles); per chunk the weights
//     slab is 36 KB (4x the F(2x2) slab per channel) and the patch 11 KB, through `buffer_load_dwordx4 ... lds` into THREE
//     slab stages + FOUR patch stages (156 KB of the 160 KB): the patch of chunk c + 1 is transformed during chunk c, so it
//     has to land one chunk earlier than the slab of chunk c + 1;
//   * a chunk is 72 slots "MFMA + its share of the other work", pinned with sched_barrier: slot 60 is the hand-over for the
//     NEXT chunk (counted vmcnt, fix-ups, one s_barrier), after the last A read of this chunk and before the first of the next;
//   * epilogue: Y = A^T M A per (channel, tile) in registers (all 36 positions of a pair live in one lane), then the
//     epilogues of wino.hip: bias / bias+ReLU / none / ReLU mask of the producer (dgrad) / bias+ReLU+2x2 max pool.
// dgrad = the same kernel on dY with the flipped / transposed filter (pack mode 1).

#include "wino4_common.h"   // geometry, transforms, MFMA wrappers, DMA slots, pack arithmetic, host side

namespace {

// ---- the chunk schedule (compile-time tables; slot S = 8 g + 4 ct + q runs the MFMA of position 4 g + q, channel tile ct)
constexpr int XHAND = 64;                                   // hand-over slot: after the chunk's last A read (slot 61; three slots: it has
                                                             // landed when the hand-over drains lgkmcnt), before the next chunk's first (65)
__host__ __device__ constexpr bool x_is_aread(int s) { return (s & 3) == 1; }
// the k-th slot (k = 0 ..) that carries neither an A read nor a DMA instruction nor the hand-over, from slot 2 on
__host__ __device__ constexpr int x_free_slot(int k)
{
    int s = 2;
    for (;; ++s) {
        if (x_is_aread(s) || x_is_dma(s) || s == XHAND) continue;
        if (k-- == 0) return s;
    }
}
// window read r (0 .. 17: row r / 3, part r % 3) sits in the r-th free slot
__host__ __device__ constexpr int x_wread_at(int s)
{
    for (int r = 0; r < 18; ++r)
        if (x_free_slot(r) == s) return r;
    return -1;
}
// the 144 transform FMAs (0 .. 71 horizontal: window row k / 12; 72 .. 143 vertical: column (k - 72) / 12), three per slot in the
// slots from 9 on that carry neither a DMA instruction nor the hand-over
__host__ __device__ constexpr int x_valu_before(int s)
{
    int n = 0;
    for (int t = 9; t < s && t < 72; ++t)
        if (!x_is_dma(t) && t != XHAND) n += 3;
    return n > 144 ? 144 : n;
}

// DYN: the dynamic tile schedule (sched != nullptr).  Two instantiations: the schedule's scalar state (queue, pending draw, ids)
// costs the chunk loop 2.6 % through SGPR pressure (48 more scalar instructions per chunk pair between the MFMAs: measured on the
// same box against the round-5 kernel, profiles/r06_wino4_static_vs_dynamic.txt), which a single-GPU run need not pay
template <bool DYN>
__global__ __launch_bounds__(XNT, 1) void conv3x3_wino4_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
    const float* __restrict__ mref, float* __restrict__ y, int N, int Cin, int Cout, int H, int W, int nChunks, int epi,
    int coTiles, int bands, int period, int nPix, int colocate, int nTiles, int* __restrict__ sched)
{
    // ONE LDS object (a second __shared__ variable makes the LDS lowering attach alias scopes to every access, and the waitcnt pass
    // then protects each window / A read against the LDS-DMA instructions with s_waitcnt vmcnt(0): measured as 40 extra waits per
    // chunk pair in the ISA); the dynamic schedule's three words sit behind the stages
    __shared__ __attribute__((aligned(16))) float lds[XLDS + 8];
    typedef __attribute__((address_space(3))) int xlds_int_t;
    volatile xlds_int_t* const sched_ids = (volatile xlds_int_t*)(lds + XLDS);   // [0], [1] the workgroup's first two tile ids, [2] the id after the next,
                                                             // [3] the id of the tile the slab cursor is in, [4] / [5] wave 0's queue state

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HW = H * W;
    const int nStrips = N * bands;
    const int grid = gridDim.x;
    // PERSISTENT workgroups (one per CU: the LDS admits no second): workgroup b walks the tile ids b, b + grid, ...; the chunk
    // stream does not stop at a tile boundary -- "the next chunk" of a tile's last chunk is the first chunk of the workgroup's
    // next tile (its DMA, hand-over, window reads, transform, first A reads), so only the epilogue separates the MFMA streams of
    // two tiles, and its stores drain while the next tile computes.  (One tile per workgroup: 32 k cycles per tile outside the
    // chunk loop -- launch, 27 DMA issues + their latency, the first transform, the store burst of all CUs in lock step; 13 % of
    // conv3_2, 35 % of conv1_2 -- tools/exp/wino4_bench.py --custom, intercept of time over chunk count.)
    // tile id -> (channel tile, pixel tile): as wino.hip (colocate: the channel tiles of a pixel tile back to back on one XCD --
    // grid is a multiple of 8, so id mod 8 = the workgroup's XCD for all of its tiles); ids beyond the last pixel tile: the end
    auto decode = [&](int vid, int& cot, int& pix) __attribute__((always_inline)) {
        cot = 0; pix = 0;
        if (vid >= nTiles) return false;
        if (DYN && colocate) {
            // dynamic schedule, <= 4 channel tiles: queue q = vid & 7 owns the pixel tiles = q mod 8 (Gq of them); its index k = vid >> 3
            // walks them in RUNS of XRUN pixel tiles per channel tile -- the ~32 workgroups of an XCD then work on ONE weight slab
            // at a time (0.6 - 2.4 MB: L2-resident) instead of all of them (the static walk keeps 4 slabs = up to 9.4 MB live per 4-MB
            // L2).  The last, shorter cycle uses runs of the remaining length, so the valid indices of a queue are a PREFIX of it
            const int q = vid & 7, k = vid >> 3;
            const int Gq = (nPix - q + 7) >> 3;                      // pixel tiles of this queue
            if (k >= Gq * coTiles) return false;
            const int full = Gq / XRUN;                              // whole cycles of XRUN pixel tiles x coTiles
            const int c = k / (XRUN * coTiles);
            int g;
            if (c < full) {
                const int rem = k - c * (XRUN * coTiles);
                cot = rem / XRUN;
                g = c * XRUN + (rem - cot * XRUN);
            } else {
                const int rt = Gq - full * XRUN, kk = k - full * (XRUN * coTiles);
                cot = kk / rt;
                g = full * XRUN + (kk - cot * rt);
            }
            pix = g * 8 + q;
            return true;
        }
        if (colocate) {
            const int slot = vid >> 3;
            cot = slot % coTiles;
            pix = (slot / coTiles) * 8 + (vid & 7);
            return pix < nPix;
        }
        cot = vid % coTiles;
        pix = vid / coTiles;
        return true;
    };

    // ---- tile schedule.  sched == nullptr: STATIC -- workgroup b walks b, b + grid, ... (a workgroup that starts late -- its CU
    // was held by another kernel, e.g. a collective's -- still runs its whole share after the others have finished: up to 2x on the
    // launch).  sched != nullptr: DYNAMIC -- eight queues over the SAME enumeration (queue q = the ids = q mod 8, so a queue keeps
    // the XCD affinity of the static walk: one weight slab per XCD with 8 channel tiles, the channel tiles of a pixel tile back to
    // back with <= 4); a workgroup draws from the queue of the XCD it runs on (HW_REG_XCC_ID) and, once that is exhausted, from the
    // following ones.  sched[q] = next index of queue q, sched[8] = workgroups finished; the last one out zeroes all nine, so the
    // buffer is zero again when the launch ends (one buffer per stream: launches on one stream do not overlap).
    // Only wave 0 draws (lane 0 issues the atomic); ids reach the other waves through sched_ids[] behind a barrier.  ids are
    // drawn one tile ahead of make_next(), i.e. two tiles ahead of the MFMAs: no wave ever waits for an atomic in the steady state.
    constexpr bool dyn = DYN;
    // The schedule's state lives in LDS, not in SGPRs (a first version kept queue, flags and ids in scalar registers: 48 more scalar
    // instructions per chunk pair between the MFMAs -- spill reloads -- and a 4 % slower chunk loop): sched_ids[4] = the queue
    // wave 0 draws from, [5] = queues not yet seen exhausted; every tile draws exactly once (where its slab cursor wraps) and resolves
    // the draw at its end, so no flags are needed
    int pend_k = 0;                                          // (wave 0, lane 0) the unresolved draw's queue index
    auto id_ok = [&](int v) __attribute__((always_inline)) { int c_, p_; return decode(v, c_, p_); };
    auto draw_add = [&](int q, int cnt) __attribute__((always_inline)) {   // -> queue q's index before the add (wave-uniform)
        int k = 0;
        if (lane == 0) k = __hip_atomic_fetch_add(sched + q, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return __builtin_amdgcn_readfirstlane(k);
    };
    // a valid id for index k of queue sq -- or, the queue being exhausted there, the first valid id of the following queues;
    // nTiles = everything has been handed out (a queue's valid ids are a prefix of it: once exhausted, always exhausted)
    auto resolve = [&](int k, int& sq, int& sleft) __attribute__((always_inline)) {
        for (;;) {
            if (sleft == 0) return nTiles;
            const long long v = 8ll * k + sq;
            if (v < nTiles && id_ok((int)v)) return (int)v;
            sq = (sq + 1) & 7;
            --sleft;
            if (sleft) k = draw_add(sq, 1);
        }
    };

    // ---- DMA-side state of a tile: the lane's patch pieces (channel, patch row, 16-B piece) -> byte offset from the chunk's first
    // plane of the tile's first image; periods are multiples of 4, so a piece lies in ONE strip
    unsigned n_pvoff[XPI];                                   // the NEXT tile's (the DMA cursors switch to it when they wrap)
    int n_fix;
    bool n_edge;
    const char* n_xc;
    unsigned n_xleft;
    const float* n_slab;
    int n_urange;
    int n_vid;
    auto make_next = [&](int vid) __attribute__((always_inline)) {
        int cot, pix;
        const bool valid = decode(vid, cot, pix);
        n_vid = vid;
        const int u0 = pix * XTW;                            // flat column of the tile's first output column
        const int n = (u0 / period) / bands;                 // image of the first tile column: the address base
        const int s0 = (u0 > 4 ? u0 - 4 : 0) / period;       // strip / image / band of the patch's first column
        const int n0 = s0 / bands, b0 = s0 - n0 * bands;
        n_fix = 0;                                           // words 1..3 of piece i (bits 4i+1 .. 4i+3) beyond the image edge
#pragma unroll
        for (int i = 0; i < XPI; ++i) {
            const int pidx = tid + i * XNT;
            const int ci = pidx / (XPR * 18), rem = pidx - ci * (XPR * 18);
            const int r = rem / 18, q = rem - r * 18;
            int gx = u0 - 4 + 4 * q - s0 * period, band = b0, sn = n0;   // gx < 0 only in the very first patch (u0 = 0, q = 0)
            while (gx >= period) { gx -= period; ++band; }
            while (band >= bands) { band -= bands; ++sn; }
            const int gy = band * XTH - 1 + r;
            n_pvoff[i] = 0xFFFFFFFFu;
            if (valid && pidx < XPS / 4 && gx >= 0 && sn < N && gy >= 0 && gy < H && gx < W) {
                n_pvoff[i] = (unsigned)(((sn - n) * Cin + ci) * HW + gy * W + gx) * 4u;
#pragma unroll
                for (int e = 1; e < 4; ++e) n_fix |= (gx + e >= W) ? (1 << (4 * i + e)) : 0;
            }
        }
        n_edge = false;                                      // some loaded piece may straddle the right edge of an image row
        if (valid && (W & 3)) {
            const int e0 = W & ~3;
            for (int st = s0; st < nStrips && st * period + e0 < u0 + XPP - 4; ++st)
                n_edge |= st * period + e0 >= u0 - 4;
        }
        n_xc = (const char*)(x + (size_t)(valid ? n : 0) * Cin * HW);
        // bytes from xc to the end of the tensor, clamped (offsets reach into the next image: (span Cin + 4) HW 4 < 2^32, launcher)
        const long long xtail = valid ? (long long)(N - n) * Cin * HW * 4 : 0ll;
        n_xleft = (unsigned)(xtail > 0xFFFFFFFEll ? 0xFFFFFFFEll : xtail);
        n_slab = wp + (size_t)cot * nChunks * XUS;
        n_urange = valid ? nChunks * XUS * 4 : 0;            // no tile: every piece is zero fill
    };
    // the cursors: patch pieces of chunk pcur / slab pieces of chunk ucur of the tile they are in
    unsigned pvoff[XPI];
    int fix;
    bool edge;
    const char* xc;
    unsigned xleft;
    const float* slab;
    int urange;
    unsigned wv;                                             // byte offset of the lane's piece of slab chunk ucur, chunk advance included
    int pcur, ucur;                                          // (the range check is on vector + scalar offset: beyond the slab = zero fill)
    auto patch_wrap = [&]() __attribute__((always_inline)) {
        if (pcur == nChunks) {
#pragma unroll
            for (int i = 0; i < XPI; ++i) pvoff[i] = n_pvoff[i];
            fix = n_fix; edge = n_edge; xc = n_xc; xleft = n_xleft;
            pcur = 0;
        }
    };
    auto slab_wrap = [&]() __attribute__((always_inline)) {   // (always one chunk after the patch cursor wrapped: then the NEXT state is free)
        if (ucur == nChunks) {
            slab = n_slab; urange = n_urange; wv = (unsigned)tid * 16u;
            ucur = 0;
            int nid = n_vid + grid;
            if constexpr (DYN) {                             // (the slot: written by wave 0 at least one barrier ago)
                nid = __builtin_amdgcn_readfirstlane(sched_ids[2]);
                if (wave == 0) {
                    // the tile the cursor enters (= the next tile when this one ends), and the draw for the tile after `nid`: resolved
                    // and published at this tile's end.  The atomic is older than this chunk's DMA instructions, so the counted
                    // wait of this chunk's hand-over covers it (vector-memory results return in order) -- a chunk later
                    const int q = __builtin_amdgcn_readfirstlane(sched_ids[4]);
                    const int left = __builtin_amdgcn_readfirstlane(sched_ids[5]);
                    if (lane == 0) {
                        sched_ids[3] = n_vid;
                        if (left) pend_k = __hip_atomic_fetch_add(sched + q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            make_next(nid);
        }
    };

    float* const ldsU = lds;
    float* const ldsP = lds + XNU * XUS;
    auto dma_patch = [&](int i, int stage /* float offset of the stage */) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
            ptmi_uniform_ptr(xc), 0, __builtin_amdgcn_readfirstlane((int)xleft), 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (xlds_void_t*)(ldsP + stage + wave * 256 + i * XNT * 4), 16,
                                                 (int)pvoff[i], 0, 0, 0);
    };
    auto dma_u = [&](int i, int stage) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
            ptmi_uniform_ptr(slab), 0, __builtin_amdgcn_readfirstlane(urange), 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (xlds_void_t*)(ldsU + stage + wave * 256 + i * XNT * 4), 16,
                                                 (int)wv, i * XNT * 16, 0, 0);
    };
    auto advance_patch = [&]() __attribute__((always_inline)) {
        xc += (size_t)XKC * HW * 4;
        xleft = xleft == 0xFFFFFFFEu ? xleft : (xleft > (unsigned)XKC * (unsigned)HW * 4u ? xleft - (unsigned)XKC * (unsigned)HW * 4u : 0u);
        ++pcur;
    };
    auto advance_u = [&]() __attribute__((always_inline)) { wv += XUS * 4; ++ucur; };
    int fix_ho;                                              // fix-up mask / edge flag of the patch the NEXT hand-over completes (the
    bool edge_ho;                                            // one issued during the previous chunk)
    auto fixup = [&](int stage, int fx, bool ed) __attribute__((always_inline)) {
        if (ed && fx) {
            float* pw = ldsP + stage + tid * 4;
#pragma unroll
            for (int i = 0; i < XPI; ++i) {
#pragma unroll
                for (int e = 1; e < 4; ++e)
                    if (fx & (1 << (4 * i + e))) pw[i * XNT * 4 + e] = 0.f;
            }
        }
    };

    // ---- the lane's role in the MFMAs (the same for every tile)
    const int wm = wave >> 1, wn = wave & 1;                 // channel half (32) / tile row (4 image rows) of the workgroup's tile
    const int ttx = lane & 15, kq = lane >> 4;               // tile column / input channel of the chunk
    auto tile_geometry = [&](int u0v, int& tsn_o, int& py_o, int& px_o) __attribute__((always_inline)) {
        const int sf = u0v / period;
        int px_t = u0v + 4 * ttx - sf * period, sn = sf / bands, band = sf - sn * bands;
        while (px_t >= period) { px_t -= period; ++band; }
        while (band >= bands) { band -= bands; ++sn; }
        tsn_o = sn;
        py_o = band * XTH + wn * 4;
        px_o = px_t;
        return sn < N && px_o < W && py_o < H;
    };
    // LDS float offsets of the lane: A = U[kq][group][co = wm 32 + ct 16 + ttx][4], window = patch[kq][4 wn + row][4 ttx + 3 ..]
    const int a_off = (kq * 9 * XBM + wm * 32 + ttx) * 4;                                  // + g * 256 + ct * 64
    const int b_off = kq * XPL + (wn * 4) * XPP + 4 * ttx + 3;                             // + row * 72 + {0, 1 (b128), 5}

    int vid = blockIdx.x;
    int vid1 = vid + grid;                                   // the workgroup's second tile
    // the last workgroup out re-arms the schedule for the next launch on this stream
    auto sched_exit = [&]() __attribute__((always_inline)) {
        if (dyn && tid == 0) {
            const int done = __hip_atomic_fetch_add(sched + 8, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (done == grid - 1) {
#pragma unroll
                for (int i = 0; i < 9; ++i) __hip_atomic_store(sched + i, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };
    if (dyn) {
        if (wave == 0) {
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            int sq = (int)(xcc & 7u), sleft = 8;
            const int k = draw_add(sq, 3);                   // three ids in one round trip: this tile, the next, the one after
            // (sleft == 8 <=> still on the own queue, whose indices k .. k + 2 this workgroup owns; a later queue: a fresh draw each)
            const int a = resolve(k, sq, sleft);
            const int b = resolve(sleft == 8 ? k + 1 : (sleft ? draw_add(sq, 1) : 0), sq, sleft);
            const int c = resolve(sleft == 8 ? k + 2 : (sleft ? draw_add(sq, 1) : 0), sq, sleft);
            if (lane == 0) { sched_ids[4] = sq; sched_ids[5] = sleft; }
            if (lane == 0) { sched_ids[0] = a; sched_ids[1] = b; sched_ids[2] = c; }
        }
        __syncthreads();
        vid = __builtin_amdgcn_readfirstlane(sched_ids[0]);
        vid1 = __builtin_amdgcn_readfirstlane(sched_ids[1]);
    }
    {
        int c0, p0;
        if (!decode(vid, c0, p0)) {                          // (workgroup-uniform)
            sched_exit();
            return;
        }
    }
    // the lane's 8 biases of a tile (channels co_w + 16 ct + 4 kq + r), fetched at the head of the tile
    f32x4 bv[2];
    const __amdgpu_buffer_rsrc_t rbias = ptmi_rsrc(bias ? bias : y, bias ? (unsigned)Cout * 4u : 0u);
    auto load_bias = [&](int v) __attribute__((always_inline)) {
        int cot, pix;
        decode(v, cot, pix);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            bv[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (epi <= 1 || epi == 4)
                bv[ct] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rbias, (cot * XBM + wm * 32 + ct * 16 + 4 * kq) * 4, 0, 0));
        }
    };
    load_bias(vid);

    // prologue DMA of the workgroup's first tile, in the order the counted waits assume: patch 0, U 0, patch 1 | U 1, patch 2
    make_next(vid);
    pcur = ucur = nChunks;                                   // "wrapped": the first issue of either kind switches to the state just made
    patch_wrap();
    {                                                        // slab_wrap() by hand: the second tile's id is vid1, the slot stays untouched
        slab = n_slab; urange = n_urange; wv = (unsigned)tid * 16u;
        ucur = 0;
        make_next(vid1);
    }
    auto issue_patch = [&](int stage) __attribute__((always_inline)) {
        patch_wrap();
#pragma unroll
        for (int i = 0; i < XPI; ++i) dma_patch(i, stage);
        advance_patch();
    };
    auto issue_u = [&](int stage) __attribute__((always_inline)) {
        slab_wrap();
#pragma unroll
        for (int i = 0; i < XUI; ++i) dma_u(i, stage);
        advance_u();
    };
    issue_patch(0);
    const int fix_p0 = fix; const bool edge_p0 = edge;
    issue_u(0);
    issue_patch(XPSP);
    const int fix_p1 = fix; const bool edge_p1 = edge;
    issue_u(XUS);
    issue_patch(2 * XPSP);
    fix_ho = fix; edge_ho = edge;

    f32x4 accA[64];                        // positions 0 .. 31 (x 2 channel tiles): AGPRs
    f32x4 accV[8];                         // positions 32 .. 35: VGPRs
    float V0[36], V1[36];                  // B operands of the current / next chunk
    float Hh[6][6];                        // horizontally transformed window of the next chunk: Hh[row][j]
    float D[6][6];                         // raw window rows
    float E[4];
    f32x4 A[3];                            // A operands: eighteen half-groups (four positions of one channel tile) per chunk rotate
                                           // through THREE register quads -- 18 = 0 mod 3, so the rotation carries across chunks
                                           // and tiles; half-group h + 2 is read during half-group h

    auto wread = [&](auto r_c, const float* pb) __attribute__((always_inline)) {         // window read r: row r / 3, part r % 3
        constexpr int a = decltype(r_c)::value / 3, part = decltype(r_c)::value % 3;
        const float* p = pb + a * XPP;
        if constexpr (part == 0) D[a][0] = *(const volatile xlds_f32_t*)p;
        if constexpr (part == 1) {
            const f32x4 v = *(const volatile xlds_f32x4_t*)(p + 1);
            D[a][1] = v[0]; D[a][2] = v[1]; D[a][3] = v[2]; D[a][4] = v[3];
        }
        if constexpr (part == 2) D[a][5] = *(const volatile xlds_f32_t*)(p + 5);
    };
    auto hop = [&](auto h_c) __attribute__((always_inline)) {                           // horizontal operation h: row h / 12 -> Hh[row][0..5]
        constexpr int h = decltype(h_c)::value;
        xin_op<h % 12>(D[h / 12], Hh[h / 12], E);
    };
    auto vop = [&](auto v_c, float (&Vn)[36]) __attribute__((always_inline)) {          // vertical operation v: column j = v / 12 -> Vn[6 i + j]
        constexpr int v = decltype(v_c)::value;
        constexpr int j = v / 12;
        const float d[6] = {Hh[0][j], Hh[1][j], Hh[2][j], Hh[3][j], Hh[4][j], Hh[5][j]};
        float t[6] = {Vn[j], Vn[6 + j], Vn[12 + j], Vn[18 + j], Vn[24 + j], Vn[30 + j]};
        xin_op<v % 12>(d, t, E);
        Vn[j] = t[0]; Vn[6 + j] = t[1]; Vn[12 + j] = t[2]; Vn[18 + j] = t[3]; Vn[24 + j] = t[4]; Vn[30 + j] = t[5];
    };

    // float offsets of the slab stage of chunk c / c + 1 / c + 2 and of the patch stage of chunk c + 1 / c + 2 / c + 3 of the chunk
    // STREAM (it runs on across tiles), rotated by compare-and-select (a modulo costs a dozen scalar instructions each)
    int uo0 = 0, uo1 = XUS, uo2 = 2 * XUS, po1 = XPSP, po2 = 2 * XPSP, po3 = 3 * XPSP;
    bool first = true;                                       // the workgroup's first tile: its operands do not come out of a previous tile's last chunk
    bool skipwait = false;                                   // a tile's first hand-over: nothing older than the previous tile's vmcnt(0) is needed,
                                                             // and the epilogue's stores must not be waited for
    // One chunk = 72 slots; EVERY chunk runs the same body (no joins of differently specialised copies: at every join the register
    // allocator moved accumulator tiles around).  PAR: parity of the chunk (which of V0 / V1 is current).
    auto chunk = [&](auto par_c) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_c)::value;
        float(&Vc)[36] = PAR ? V1 : V0;
        float(&Vn)[36] = PAR ? V0 : V1;
        const float* ap = ldsU + uo0 + a_off;
        const float* apn = ldsU + uo1 + a_off;
        const float* pb = ldsP + po1 + b_off;
        const int ud = uo2, pf = po2, pd = po3;
        {
            const int t = uo0; uo0 = uo1; uo1 = uo2; uo2 = t;
            const int q = po3 + XPSP == XNP * XPSP ? 0 : po3 + XPSP;
            po1 = po2; po2 = po3; po3 = q;
        }
        slab_wrap();                                         // this chunk's DMA: slab chunk ucur, patch chunk pcur -- of this tile or the next
        patch_wrap();
        {   // one address register each for the chunk's A reads and window reads (immediate offsets)
            unsigned va = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)ap;
            unsigned vn = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)apn;
            unsigned vb = (unsigned)(size_t)(const __attribute__((address_space(3))) float*)pb;
            asm volatile("" : "+v"(va), "+v"(vn), "+v"(vb));
            ap = (const float*)(const __attribute__((address_space(3))) float*)(size_t)va;
            apn = (const float*)(const __attribute__((address_space(3))) float*)(size_t)vn;
            pb = (const float*)(const __attribute__((address_space(3))) float*)(size_t)vb;
        }
        xfor(std::make_integer_sequence<int, 72>{}, [&](auto s_c) __attribute__((always_inline)) {
            constexpr int S = decltype(s_c)::value;
            constexpr int hg = S >> 2, g = S >> 3, ct = hg & 1, q = S & 3, p = 4 * g + q;
            const float av = A[hg % 3][q], bvv = Vc[p];
            if constexpr (p < 32) xmfma_a(accA[2 * p + ct], av, bvv);   // [x4:mf]
            else xmfma_v(accV[2 * (p - 32) + ct], av, bvv);   // [x4:mf]
            if constexpr (q == 1) {                          // half-group hg + 2 (of this chunk, or 0 / 1 of the next one)
                constexpr int h2 = hg + 2;
                if constexpr (h2 < 18) A[h2 % 3] = *(const volatile xlds_f32x4_t*)(ap + (h2 >> 1) * 256 + (h2 & 1) * 64);   // [x4:ar]
                else A[h2 % 3] = *(const volatile xlds_f32x4_t*)(apn + (h2 & 1) * 64);   // [x4:ar]
            }
            if constexpr (S == XHAND) {
                // everything but this chunk's DMA instructions so far (10 of its 12) has landed: slab c + 1, patch c + 2
                if (!skipwait) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(x_dma_before(XHAND)) : "memory");   // [x4:ho]
                skipwait = false;
                fixup(pf, fix_ho, edge_ho);   // [x4:ho]
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // [x4:ho]
            }
            constexpr int wr = x_wread_at(S);
            if constexpr (wr >= 0) wread(std::integral_constant<int, (wr >= 0 ? wr : 0)>{}, pb);   // [x4:wr]
            constexpr int di = x_dma_at(S);
            if constexpr (di >= 0) {
                if constexpr (di < XUI) dma_u(di, ud);   // [x4:dma]
                else dma_patch(di - XUI, pd);   // [x4:dma]
                if constexpr (di == XUI - 1) advance_u();
                if constexpr (di == XDI - 1) advance_patch();
            }
            constexpr int k0 = x_valu_before(S), k1 = x_valu_before(S + 1);
            xfor(std::make_integer_sequence<int, k1 - k0>{}, [&](auto k_c) __attribute__((always_inline)) {
                constexpr int k = k0 + decltype(k_c)::value;
                if constexpr (k < 72) hop(std::integral_constant<int, (k < 72 ? k : 0)>{});   // [x4:xf]
                else vop(std::integral_constant<int, (k >= 72 ? k - 72 : 0)>{}, Vn);   // [x4:xf]
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        fix_ho = fix; edge_ho = edge;                        // (of the patch this chunk issued: the next hand-over completes it)
    };

    auto epilogue = [&](int tvid) __attribute__((always_inline)) {
        int cot, pix;
        decode(tvid, cot, pix);
        const int u0 = pix * XTW;
        const int n = (u0 / period) / bands;
        const int co_w = cot * XBM + wm * 32;
        // ---- epilogue: Y = A^T M A per (channel, tile) in registers, then bias / ReLU / mask / pool and buffer stores.
        // Accumulator element r of tile (p, ct): channel co_w + 16 ct + 4 kq + r, tile ttx, position p.
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");       // the last MFMAs' results (inline asm: the compiler pads nothing)
        int tsn, py, px;
        const bool tile_ok = tile_geometry(u0, tsn, py, px);
        const int cmax = Cout - co_w - 4 * kq;                   // channel 16 ct + r of this lane exists iff 16 ct + r < cmax
        auto rd = [](float a) __attribute__((always_inline)) { float v; asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a)); return v; };
        // the 4x4 outputs of channel (ct, r): o[k][l], k = output row, l = output column
        auto inverse = [&](auto ct_c, auto r_c, float (&o)[4][4]) __attribute__((always_inline)) {
            constexpr int ct = decltype(ct_c)::value, r = decltype(r_c)::value;
            float z[6][4];
            xfor(std::make_integer_sequence<int, 6>{}, [&](auto i_c) __attribute__((always_inline)) {
                constexpr int i = decltype(i_c)::value;
                float m[6];
                xfor(std::make_integer_sequence<int, 6>{}, [&](auto j_c) __attribute__((always_inline)) {
                    constexpr int p = 6 * i + decltype(j_c)::value;
                    if constexpr (p < 32) m[decltype(j_c)::value] = rd(accA[2 * p + ct][r]);
                    else m[decltype(j_c)::value] = accV[2 * (p - 32) + ct][r];
                });
                xout(m, z[i]);
            });
    #pragma unroll
            for (int l = 0; l < 4; ++l) {
                const float m[6] = {z[0][l], z[1][l], z[2][l], z[3][l], z[4][l], z[5][l]};
                float yk[4];
                xout(m, yk);
    #pragma unroll
                for (int k = 0; k < 4; ++k) o[k][l] = yk[k];
            }
        };
        auto for_channels = [&](auto&& f) __attribute__((always_inline)) {
            xfor(std::make_integer_sequence<int, 8>{}, [&](auto c_c) __attribute__((always_inline)) {
                f(std::integral_constant<int, (decltype(c_c)::value >> 2)>{}, std::integral_constant<int, (decltype(c_c)::value & 3)>{});
                __builtin_amdgcn_sched_barrier(0);
            });
        };
        if (epi == 4) {
            // bias + ReLU + 2x2/2 max pool (floor mode): the tile is four pool windows
            const int OH = H >> 1, OW = W >> 1, OHW = OH * OW;
            const long long ytail = (long long)(N - n) * Cout * OHW * 4;
            const __amdgpu_buffer_rsrc_t ry = ptmi_rsrc(y + (size_t)n * Cout * OHW, (unsigned)(ytail > 0xFFFFFFFEll ? 0xFFFFFFFEll : ytail));
            const int oy = py >> 1, ox = px >> 1;
            unsigned pv2[2], pv1[2];
    #pragma unroll
            for (int a = 0; a < 2; ++a) {
                const bool rok = tile_ok && oy + a < OH;
                const unsigned o = (unsigned)(((tsn - n) * Cout + 4 * kq) * OHW + (oy + a) * OW + ox) * 4u;
                pv2[a] = (rok && ox + 1 < OW) ? o : 0xFFFFFFFFu;
                pv1[a] = (rok && ox + 1 == OW) ? o : 0xFFFFFFFFu;
            }
            for_channels([&](auto ct_c, auto r_c) __attribute__((always_inline)) {
                constexpr int ct = decltype(ct_c)::value, r = decltype(r_c)::value;
                float o[4][4];
                inverse(ct_c, r_c, o);
                const float b = bv[ct][r];
                const bool cok = 16 * ct + r < cmax;
                const int soff = (co_w + 16 * ct + r) * OHW * 4;
    #pragma unroll
                for (int a = 0; a < 2; ++a) {
                    f32x2 m;
    #pragma unroll
                    for (int l = 0; l < 2; ++l)
                        m[l] = fmaxf(fmaxf(fmaxf(o[2 * a][2 * l] + b, o[2 * a][2 * l + 1] + b),
                                           fmaxf(o[2 * a + 1][2 * l] + b, o[2 * a + 1][2 * l + 1] + b)), 0.f);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, m), ry, cok ? (int)pv2[a] : -1, soff, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, m[0]), ry, cok ? (int)pv1[a] : -1, soff, 0);
                }
            });
            return;
        }
        const long long ytail = (long long)(N - n) * Cout * HW * 4;
        const unsigned img_bytes = (unsigned)(ytail > 0xFFFFFFFEll ? 0xFFFFFFFEll : ytail);     // to the end of the tensor, clamped
        const __amdgpu_buffer_rsrc_t ry = ptmi_rsrc(y + (size_t)n * Cout * HW, img_bytes);
        const __amdgpu_buffer_rsrc_t rm = ptmi_rsrc(epi == 3 ? mref + (size_t)n * Cout * HW : y, epi == 3 ? img_bytes : 0u);
        // per-lane byte offsets of the tile's four rows: pv4 = all four columns inside the image (16-byte access), pve[e] = column
        // e alone (tiles cut by the right edge)
        unsigned pv4[4];
        unsigned pve[4][3];
        bool partial = false;
    #pragma unroll
        for (int a = 0; a < 4; ++a) {
            const bool rok = tile_ok && py + a < H;
            const unsigned o = (unsigned)(((tsn - n) * Cout + 4 * kq) * HW + (py + a) * W + px) * 4u;
            pv4[a] = (rok && px + 3 < W) ? o : 0xFFFFFFFFu;
    #pragma unroll
            for (int e = 0; e < 3; ++e) {
                pve[a][e] = (rok && px + 3 >= W && px + e < W) ? o + 4u * e : 0xFFFFFFFFu;
                partial |= pve[a][e] != 0xFFFFFFFFu;
            }
        }
        const bool cut = __any(partial);                         // (wave-uniform) some lane's tile is cut by the right edge
        auto store_rows = [&](auto epi_c) __attribute__((always_inline)) {
            constexpr int EPI = decltype(epi_c)::value;
            for_channels([&](auto ct_c, auto r_c) __attribute__((always_inline)) {
                constexpr int ct = decltype(ct_c)::value, r = decltype(r_c)::value;
                const bool cok = 16 * ct + r < cmax;
                const int soff = (co_w + 16 * ct + r) * HW * 4;
                f32x4 mk[4];
                float ms[4][3];
                if constexpr (EPI == 3) {                                  // the producer's activations first: their latency hides
    #pragma unroll                                                         // behind the inverse transform
                    for (int a = 0; a < 4; ++a) {
                        mk[a] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, cok ? (int)pv4[a] : -1, soff, 0));
                        if (cut) {
    #pragma unroll
                            for (int e = 0; e < 3; ++e)
                                ms[a][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, cok ? (int)pve[a][e] : -1, soff, 0));
                        }
                    }
                }
                float o[4][4];
                inverse(ct_c, r_c, o);
                const float b = bv[ct][r];
    #pragma unroll
                for (int a = 0; a < 4; ++a) {
                    f32x4 st;
    #pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        float v = o[a][l];
                        if constexpr (EPI <= 1) v += b;
                        if constexpr (EPI == 1) v = fmaxf(v, 0.f);
                        if constexpr (EPI == 3) {
                            float m = mk[a][l];
                            if (cut && l < 3) m = (pve[a][l] != 0xFFFFFFFFu) ? ms[a][l] : m;
                            v = (m > 0.f) ? v : 0.f;
                        }
                        st[l] = v;
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, st), ry, cok ? (int)pv4[a] : -1, soff, 0);
                    // a 16-byte store reads its data registers for two more states: hipcc pads that against ITS next VALU, not against
                    // an inline-asm one (found the hard way: output (1, 1) of tile columns 12 .. 15 wrong, only with a bias)
                    asm volatile("s_nop 1" ::: "memory");
                    if (cut) {
    #pragma unroll
                        for (int e = 0; e < 3; ++e) {
                            const float sv = e == 0 ? st[0] : e == 1 ? st[1] : st[2];   // (bit_cast of a vector ELEMENT lvalue reads element 0)
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sv), ry, cok ? (int)pve[a][e] : -1, soff, 0);
                        }
                    }
                }
            });
        };
        if (epi == 0) store_rows(std::integral_constant<int, 0>{});
        else if (epi == 1) store_rows(std::integral_constant<int, 1>{});
        else if (epi == 2) store_rows(std::integral_constant<int, 2>{});
        else store_rows(std::integral_constant<int, 3>{});
    };

    for (;;) {
        // [x4@t0]
        // the accumulators: zeroed while the first tile's first pieces are in flight / the previous tile's stores leave
        xfor(std::make_integer_sequence<int, 64>{}, [&](auto i_c) __attribute__((always_inline)) {
            accA[decltype(i_c)::value] = (f32x4){0.f, 0.f, 0.f, 0.f};
            asm volatile("" : "+a"(accA[decltype(i_c)::value]));
        });
        xfor(std::make_integer_sequence<int, 8>{}, [&](auto i_c) __attribute__((always_inline)) {
            accV[decltype(i_c)::value] = (f32x4){0.f, 0.f, 0.f, 0.f};
            asm volatile("" : "+v"(accV[decltype(i_c)::value]));
        });
        if (first) {
            first = false;
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(XDI) : "memory");
            fixup(0, fix_p0, edge_p0);
            fixup(XPSP, fix_p1, edge_p1);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // B operands of chunk 0: window from patch stage 0; A half-groups 0, 1 from slab stage 0
            const float* pb = ldsP + b_off;
            xfor(std::make_integer_sequence<int, 18>{}, [&](auto r_c) __attribute__((always_inline)) { wread(r_c, pb); });
            xfor(std::make_integer_sequence<int, 72>{}, [&](auto h_c) __attribute__((always_inline)) { hop(h_c); });
            xfor(std::make_integer_sequence<int, 72>{}, [&](auto v_c) __attribute__((always_inline)) { vop(v_c, V0); });
            A[0] = *(const volatile xlds_f32x4_t*)(ldsU + a_off);
            A[1] = *(const volatile xlds_f32x4_t*)(ldsU + a_off + 64);
        }
        // [x4@t1]
        for (int c = 0; c < nChunks; c += 2) {              // nChunks is even (launcher: Cin % 8 == 0)
            chunk(std::integral_constant<int, 0>{});
            chunk(std::integral_constant<int, 1>{});
        }
        // [x4@t2]
        // the last chunk's own DMA instructions (the next tile's chunk 1 slab / chunk 2 patch): with them done, nothing the next
        // tile's counted waits rely on is older than the epilogue's stores
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (DYN) {
            if (wave == 0) {                                 // this tile's draw: valid, or the next queue's, or "none left"
                int sq = __builtin_amdgcn_readfirstlane(sched_ids[4]), sleft = __builtin_amdgcn_readfirstlane(sched_ids[5]);
                const int v = resolve(__builtin_amdgcn_readfirstlane(pend_k), sq, sleft);
                if (lane == 0) { sched_ids[2] = v; sched_ids[4] = sq; sched_ids[5] = sleft; }
            }
        }
        // [x4@t3]
        epilogue(vid);
        // [x4@t4]
        if constexpr (DYN) vid = __builtin_amdgcn_readfirstlane(sched_ids[3]);   // (written where this tile's slab cursor wrapped: barriers ago)
        else vid += grid;
        {
            int c0, p0;
            if (!decode(vid, c0, p0)) break;
        }
        load_bias(vid);
        skipwait = true;
    }
    sched_exit();
}

// U = G g G^T (6x6 per filter) laid out as the kernel's LDS image: [channel tile (64)][chunk (4 ci)][ci][position group 9][co 64]
// [position in group 4].  mode as ptmi_conv3x3_pack_weights (1: dgrad -- transposed channels, flipped taps).
__global__ void wino4_pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int wCout, int wCin, int mode,
                                          int coTiles, int nChunks)
{
    x_pack_weights(w, wp, wCout, wCin, mode, coTiles, nChunks, blockIdx.x * (int64_t)blockDim.x + threadIdx.x,
                   (int64_t)gridDim.x * blockDim.x, [](int col, int i, int j) __attribute__((always_inline)) {
        const int p = 6 * i + j;
        return col * 4 + (p >> 2) * (XBM * 4) + (p & 3);
    });
}

}  // namespace

extern "C" {

int64_t ptmi_conv3x3_wino4_packed_floats(int cin, int cout) { return x_packed_floats(cin, cout); }

int ptmi_conv3x3_wino4_pack_weights(const float* w, float* wp, int w_cout, int w_cin, int mode, ptmi_stream_t s)
{
    return x_pack_weights_launch("conv3x3_wino4_pack_weights", wino4_pack_weights_kernel, w, wp, w_cout, w_cin, mode, s);
}

int ptmi_conv3x3_wino4_fwd_fits(int cin, int cout, int h, int w) { return x_fwd_fits(cin, cout, h, w); }

int ptmi_conv3x3_wino4_fwd_sched(const float* x, const float* wp, const float* bias, const float* mask_ref, float* y, int n,
                                 int cin, int cout, int h, int w, int epilogue, int32_t* sched, ptmi_stream_t s)
{
    return x_fwd_sched("conv3x3_wino4_fwd", conv3x3_wino4_kernel<true>, conv3x3_wino4_kernel<false>, x, wp, bias, mask_ref, y, n, cin, cout,
                       h, w, epilogue, sched, s);
}

int ptmi_conv3x3_wino4_fwd(const float* x, const float* wp, const float* bias, const float* mask_ref, float* y, int n,
                           int cin, int cout, int h, int w, int epilogue, ptmi_stream_t s)
{
    return ptmi_conv3x3_wino4_fwd_sched(x, wp, bias, mask_ref, y, n, cin, cout, h, w, epilogue, nullptr, s);
}

}  // extern "C"
