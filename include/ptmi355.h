/*
 * ptmi355.h -- C ABI of libptmi355.so: the MI355X (gfx950 / CDNA4) operators behind the
 * ProbabilisticTeacher teacher+student train step (PTrainer.run_step, reference
 * /root/reference/pt/engine/trainer.py:263-392).
 *
 * The reference has NO native boundary of its own: it is pure Python and reaches native code
 * only through torch/ATen, cuDNN, torchvision C++/CUDA ops and NCCL.  Each entry point below
 * replaces one of those implicitly-invoked native operators; the comment on each names the
 * reference call site (file:line relative to /root/reference) whose operator it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no torch types.  All pointers are DEVICE pointers
 *     unless the name ends in _host.  fp32 tensors are dense row-major NCHW / (R,C) unless noted.
 *   - The caller allocates every output and workspace; the library never allocates, frees or
 *     synchronises; every kernel is enqueued on the passed hipStream_t (void* here).
 *   - Return 0 on success, negative on error; ptmi_last_error() gives a thread-local message.
 *   - int64 indices, uint8 masks, fp32 floats, matching the reference's observable dtypes.
 */
#ifndef PTMI355_H
#define PTMI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ptmi_stream_t; /* hipStream_t */

const char* ptmi_last_error(void);
int ptmi_abi_version(void);

/* ------------------------------------------------------------------ conv stack (N1, N3)
 * replaces cuDNN conv2d 3x3 s1 p1 (+bias) + F.relu_ at pt/modeling/backbone/vgg.py:45-53,66-69
 * and the D2 StandardRPNHead 3x3 conv at pt/modeling/proposal_generator/rpn.py:96.
 * fp32 implicit GEMM on v_mfma_f32_32x32x2_f32.
 *
 * Packed weight layout (built by ptmi_conv3x3_pack_weights): for BM = ptmi_conv3x3_bm(Cout),
 * CK = ptmi_conv3x3_ck(Cin):  [ceil(Cout/BM)][ceil(Cin/CK)][9 taps][CK][BM] fp32, zero padded.
 * mode 0 = forward weights  Wp[co][ci][ky][kx]            = W[co][ci][ky][kx]
 * mode 1 = dgrad weights    (roles of co/ci swapped)      = W[ci][co][2-ky][2-kx]
 *          i.e. dX = conv3x3(dY, pack(W, mode 1)) with "Cin" := Cout(W), "Cout" := Cin(W).
 */
int ptmi_conv3x3_bm(int cout);
int ptmi_conv3x3_ck(int cin);
int64_t ptmi_conv3x3_packed_floats(int cin, int cout);
int ptmi_conv3x3_pack_weights(const float* w, float* wp, int w_cout, int w_cin, int mode,
                              ptmi_stream_t s);
/* epilogue: 0 = y = acc + bias;  1 = y = relu(acc + bias);  2 = y = acc (bias may be NULL);
 *           3 = y = (mask_ref[idx] > 0) ? acc : 0   (dgrad through the producer's ReLU;
 *               mask_ref has the shape of y);
 *           4 = y = maxpool2x2(relu(acc + bias)), y is (n, cout, h/2, w/2): conv + F.relu_ + MaxPool2d of a
 *               VGG block (vgg.py:66-71) in one pass, for blocks whose activations are not kept. */
int ptmi_conv3x3_fwd(const float* x, const float* wp, const float* bias, const float* mask_ref,
                     float* y, int n, int cin, int cout, int h, int w, int epilogue,
                     ptmi_stream_t s);
/* wgrad: dw[co][ci][3][3] (+)= sum_{n,y,x} dy[n][co][y][x] * x[n][ci][y+ky-1][x+kx-1].
 * workspace: ptmi_conv3x3_wgrad_ws_floats(...) fp32; split-K partials reduced in a fixed order
 * (deterministic).  db (may be NULL) = sum dy over n,y,x.  accumulate != 0 adds into dw AND db. */
int64_t ptmi_conv3x3_wgrad_ws_floats(int n, int cin, int cout, int h, int w);
int ptmi_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws,
                       int n, int cin, int cout, int h, int w, int accumulate, ptmi_stream_t s);
/* Fused Winograd F(2x2,3x3) variant of ptmi_conv3x3_fwd for the layers with >= 32 input channels (conv1_2 .. conv5_3 at
 * pt/modeling/backbone/vgg.py:45-53,66-69 and the RPN 3x3 conv at pt/modeling/proposal_generator/rpn.py:96; cuDNN, which
 * the reference runs there, uses Winograd for these fp32 3x3 s1 layers too).  Same arguments, epilogues and dgrad
 * convention (mode 1 pack) as ptmi_conv3x3_fwd; fp32 in, fp32 accumulate on v_mfma_f32_32x32x2_f32, 16 instead of 36
 * multiplies per 2x2 output tile and channel pair.  Input transform (B^T d B), the 16 transform-domain GEMMs and the
 * output transform (A^T M A) run in ONE kernel; only x, the packed weights and y touch HBM.
 * Packed weights (ptmi_conv3x3_wino_pack_weights): U = G g G^T as
 * [ceil(Cout/64)][ceil(Cin/8)][8 ci][4 (position row)][64 co][4 (position column)] fp32, zero padded. */
int64_t ptmi_conv3x3_wino_packed_floats(int cin, int cout);
int ptmi_conv3x3_wino_pack_weights(const float* w, float* wp, int w_cout, int w_cin, int mode,
                                   ptmi_stream_t s);
int ptmi_conv3x3_wino_fwd(const float* x, const float* wp, const float* bias, const float* mask_ref,
                          float* y, int n, int cin, int cout, int h, int w, int epilogue,
                          ptmi_stream_t s);
/* 1 if the shape fits the 32-bit buffer offsets of ptmi_conv3x3_wino_fwd / ptmi_conv3x3_wino_wgrad (per-lane byte offsets
 * relative to a workgroup's first image; roughly h*w < 8 M pixels at 64 channels), else 0: the caller then routes the layer
 * to ptmi_conv3x3_fwd / ptmi_conv3x3_wgrad (the Winograd entry points themselves reject such shapes with an error). */
int ptmi_conv3x3_wino_fwd_fits(int cin, int cout, int h, int w);
int ptmi_conv3x3_wino_wgrad_fits(int h, int w);
/* Fused Winograd F(4x4,3x3) variant (round 5, csrc/wino4.hip) of ptmi_conv3x3_wino_fwd for the same layers
 * (pt/modeling/backbone/vgg.py:45-53,66-69, pt/modeling/proposal_generator/rpn.py:96) when the input channel count is a multiple
 * of 8: 36 transform-domain products per 4x4 outputs instead of 64, on v_mfma_f32_16x16x4_f32; interpolation points
 * 0, +-3/4, +-3/2, inf (every constant of B^T and A^T exact in fp32; measured error against an fp64 convolution 1.2e-5 of a
 * unit-scale output at 512 channels -- inside the 1e-4 bar of the parity tests, which are unchanged).  Same arguments,
 * epilogues and dgrad convention (mode 1 pack) as ptmi_conv3x3_fwd.  Packed weights: U = G g G^T as
 * [ceil(Cout/64)][Cin/4][4 ci][9 (groups of four positions p = 6 i + j)][64 co][4] fp32, zero padded.
 * ptmi_conv3x3_wino4_fwd_fits: 1 if the shape is served (cin % 8 == 0 and the 32-bit buffer offsets suffice). */
int64_t ptmi_conv3x3_wino4_packed_floats(int cin, int cout);
int ptmi_conv3x3_wino4_pack_weights(const float* w, float* wp, int w_cout, int w_cin, int mode,
                                    ptmi_stream_t s);
int ptmi_conv3x3_wino4_fwd(const float* x, const float* wp, const float* bias, const float* mask_ref,
                           float* y, int n, int cin, int cout, int h, int w, int epilogue,
                           ptmi_stream_t s);
int ptmi_conv3x3_wino4_fwd_fits(int cin, int cout, int h, int w);
/* ptmi_conv3x3_wino4_fwd with a DYNAMIC tile schedule (round 6).  The kernel runs one persistent workgroup per CU; with the
 * static schedule of ptmi_conv3x3_wino4_fwd workgroup b walks tiles b, b + grid, ..., so a workgroup whose CU is held by another
 * kernel when the launch starts (an RCCL collective overlapping backward: pt/engine/trainer.py:92-95,384 under DDP) still runs
 * its whole share after everyone else has finished -- up to 2x on the launch.  Here the workgroups draw tile ids from eight
 * queues (queue q = the ids = q mod 8 of the same enumeration: the XCD affinity of the static walk is kept; a workgroup starts
 * on the queue of the XCD it runs on and moves on when that is exhausted).  sched: 16 int32 in device memory, ZERO before the
 * first launch; the last workgroup of a launch zeroes it again, so one buffer serves every launch of ONE stream (launches that
 * may overlap -- different streams -- need different buffers).  sched == NULL: the static schedule.  Results are bit-identical
 * either way (a tile's arithmetic does not depend on who computes it). */
int ptmi_conv3x3_wino4_fwd_sched(const float* x, const float* wp, const float* bias, const float* mask_ref,
                                 float* y, int n, int cin, int cout, int h, int w, int epilogue,
                                 int32_t* sched, ptmi_stream_t s);
/* Winograd-domain weight gradient (same contract as ptmi_conv3x3_wgrad; replaces cuDNN's Winograd-nonfused BWD_FILTER
 * for the trainable 3x3 layers with >= 64 input and output channels): dU_p[co][ci] = sum over tiles of (A dY A^T)_p V_p on v_mfma_f32_32x32x2_f32 (16 instead
 * of 36 multiplies per tile and channel pair), split over contiguous tile ranges whose partials (workspace
 * [split][16][Cout][Cin] fp32, ptmi_conv3x3_wino_wgrad_ws_floats) are summed in a fixed order and mapped back by
 * dW = G^T dU G; db = sum of dy per channel (position (1,1) of A dY A^T is the tile's sum), accumulated by the same
 * workgroups and appended to the workspace as [split][Cout].  Deterministic. */
int64_t ptmi_conv3x3_wino_wgrad_ws_floats(int n, int cin, int cout, int h, int w);
int ptmi_conv3x3_wino_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws, int n,
                            int cin, int cout, int h, int w, int accumulate, ptmi_stream_t s);
/* F(4x4,3x3)-domain weight gradient (round 5, csrc/wino4w.hip; same contract as ptmi_conv3x3_wgrad / ptmi_conv3x3_wino_wgrad;
 * replaces cuDNN's BWD_FILTER at pt/modeling/backbone/vgg.py:45-53,66-69, pt/modeling/proposal_generator/rpn.py:96):
 * dU_p[co][ci] = sum over tiles of (A dY A^T)_p V_p for the 36 positions of the 6x6 transform domain on v_mfma_f32_32x32x2_f32
 * (36 multiplies per 4x4 tile and channel pair instead of 64 / 144), split over contiguous tile ranges whose partials (workspace
 * [split][36][Cout][Cin] fp32 + bias partials [split][ceil(Cin/32)][Cout], ptmi_conv3x3_wino4_wgrad_ws_floats) are summed in a fixed
 * order and mapped back by dW = G^T dU G.  Deterministic.  ptmi_conv3x3_wino4_wgrad_fits: the 32-bit buffer offsets suffice. */
int ptmi_conv3x3_wino4_wgrad_fits(int h, int w);
int64_t ptmi_conv3x3_wino4_wgrad_ws_floats(int n, int cin, int cout, int h, int w);
int ptmi_conv3x3_wino4_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws, int n,
                             int cin, int cout, int h, int w, int accumulate, ptmi_stream_t s);
/* ptmi_conv3x3_wino4_* with the 36 transform-domain positions SPLIT over the two waves of a tile row (round 6, csrc/wino4p.hip):
 * same layers (pt/modeling/backbone/vgg.py:45-53,66-69, pt/modeling/proposal_generator/rpn.py:96), same contract, epilogues, dgrad
 * convention (mode 1 pack), shape limits (ptmi_conv3x3_wino4p_fwd_fits == ptmi_conv3x3_wino4_fwd_fits) and tile schedules
 * (sched as ptmi_conv3x3_wino4_fwd_sched; NULL = static).  A wave owns all 64 output channels x 18 positions instead of 32 channels
 * x 36 positions: it transforms only its three rows of every window (72 instead of 144 FMAs per lane and 4-channel chunk -- beside
 * fp32 MFMAs every FMA is issue time), and the two waves exchange partial 4x4 outputs through LDS in the epilogue.  The packed
 * weights have their own layout (ptmi_conv3x3_wino4p_pack_weights); results agree with ptmi_conv3x3_wino4_fwd to fp32 rounding
 * (the inverse transform's row sum is associated differently), not bit for bit. */
int64_t ptmi_conv3x3_wino4p_packed_floats(int cin, int cout);
int ptmi_conv3x3_wino4p_pack_weights(const float* w, float* wp, int w_cout, int w_cin, int mode,
                                     ptmi_stream_t s);
int ptmi_conv3x3_wino4p_fwd(const float* x, const float* wp, const float* bias, const float* mask_ref,
                            float* y, int n, int cin, int cout, int h, int w, int epilogue,
                            ptmi_stream_t s);
int ptmi_conv3x3_wino4p_fwd_sched(const float* x, const float* wp, const float* bias,
                                  const float* mask_ref, float* y, int n, int cin, int cout, int h,
                                  int w, int epilogue, int32_t* sched, ptmi_stream_t s);
int ptmi_conv3x3_wino4p_fwd_fits(int cin, int cout, int h, int w);
/* ------------------------------------------------------------------ the constant frame of a shrink-pasted image (csrc/frame_skip.h)
 * PTrainer.resize (reference pt/engine/trainer.py:557-590) pastes every strong view, shrunk by r ~ U(0.5, 1), into the middle of a
 * canvas of one colour.  Inside that frame every 3x3 layer's output is a fixed pattern y[c][y & 3][x & 3] (period 4: the 4x4 output
 * tile of F(4x4, 3x3)); the entry points below let a forward launch leave those tiles out and write the pattern instead.
 * A RING is eight int32 per image -- outer (x0, y0, x1, y1), inner (x0, y0, x1, y1), half-open, in the resolution of a layer's
 * INPUT: every input pixel inside outer and outside inner holds the pattern; outer x1 <= x0 = the image has none.
 * ptmi_frame_ring_next: the rings of a layer's output from those of its h x w input.  op 0: conv3x3 pad 1 by a direct kernel -- an
 * output pixel is the pattern iff its 3x3 window is; op 1: max pool 2x2 / 2 (floor); op 2: conv3x3 by the F(4x4, 3x3) kernels -- the
 * roundoff of a tile's sixteen outputs depends on its whole 6x6 window, so only whole tiles that ptmi_frame_tile_skippable accepts
 * are the pattern BIT FOR BIT: outer shrinks and inner grows to tile boundaries.
 * ptmi_frame_tile_skippable: 1 iff the 4x4 output tile at (py, px) of an h x w image reads only the pattern (its whole 6x6 window
 * inside outer and outside inner) and lies inside the image.  ptmi_frame_pixel_tile_skippable: 1 iff all 32 tiles of pixel tile
 * `pix` of the F(4x4, 3x3) walk (64 flat columns x 8 rows of the concatenated strips; ptmi_frame_pixel_tiles of them) are.
 * ptmi_frame_skip_lists: the ascending lists of the pixel tiles to compute (keep) and to fill (skip), room for
 * ptmi_frame_pixel_tiles ints each, counts[0] / counts[1] their lengths.  All of these run on the host and touch no device. */
int ptmi_frame_ring_next(const int32_t* rings_in, int32_t* rings_out, int n, int op, int h, int w);
int64_t ptmi_frame_pixel_tiles(int n, int h, int w);
int ptmi_frame_tile_skippable(const int32_t* ring, int h, int w, int py, int px);
int ptmi_frame_pixel_tile_skippable(const int32_t* rings, int n, int h, int w, int pix);
int ptmi_frame_skip_lists(const int32_t* rings, int n, int h, int w, int32_t* keep, int32_t* skip,
                          int32_t* counts);
/* ptmi_conv3x3_wino4p_fwd over a LIST of pixel tiles (static schedule; a separate instantiation of the same kernel: a tile's
 * arithmetic is the plain launch's, bit for bit): pix_list = n_list ascending pixel-tile numbers in device memory, e.g. `keep` of
 * ptmi_frame_skip_lists.  Outputs of tiles outside the list are not written. */
int ptmi_conv3x3_wino4p_fwd_list(const float* x, const float* wp, const float* bias,
                                 const float* mask_ref, float* y, int n, int cin, int cout, int h, int w,
                                 int epilogue, const int32_t* pix_list, int n_list, ptmi_stream_t s);
/* Writes the outputs of the pixel tiles in skip_list (device memory, as `skip` of ptmi_frame_skip_lists for the rings `rings`, also
 * in device memory, of the layer's INPUT): y[n][c][y][x] = pattern[c][y & 3][x & 3] (pattern: cout x 4 x 4 floats), with 16-byte
 * stores.  pooled = 1: y is the (n, cout, h / 2, w / 2) output of epilogue 4 and the pattern is indexed by pooled coordinates.
 * Every tile is tested against its ring before it is written.  Writes only tiles the list launch leaves out: the two may run in
 * either order. */
int ptmi_frame_fill(const int32_t* skip_list, int n_skip, const int32_t* rings, const float* pattern,
                    float* y, int n, int cout, int h, int w, int pooled, ptmi_stream_t s);
/* The two Winograd-domain weight-gradient kernels with `waves` fills of the chip's one-workgroup-per-CU slots instead of one
 * (round 6): their workgroups each own a contiguous share of the (image, tile) list, so with one fill a workgroup whose CU is held by
 * another kernel when the launch starts -- an RCCL collective overlapping backward, pt/engine/trainer.py:92-95,384 under DDP --
 * runs its whole share after everyone else has finished: 2x on the launch (tools/exp/contention.py: 33 -> 65 ms per 8 + 8 step
 * with 8 of 256 CUs held).  With `waves` > 1 (clamped to 16) the later workgroups go to whichever CU frees up first: 45 ms at
 * waves = 4, for 8 % more time when nothing else runs (one more prologue and partial-sum store per workgroup).  Same contract and
 * the same bit-exact repeatability as the one-wave entry points (= waves 1); the workspace grows with the split count
 * (ptmi_conv3x3_wino*_wgrad_ws_floats_waves with the same `waves`). */
int64_t ptmi_conv3x3_wino_wgrad_ws_floats_waves(int n, int cin, int cout, int h, int w, int waves);
int ptmi_conv3x3_wino_wgrad_waves(const float* x, const float* dy, float* dw, float* db, float* ws,
                                  int n, int cin, int cout, int h, int w, int accumulate, int waves,
                                  ptmi_stream_t s);
int64_t ptmi_conv3x3_wino4_wgrad_ws_floats_waves(int n, int cin, int cout, int h, int w, int waves);
int ptmi_conv3x3_wino4_wgrad_waves(const float* x, const float* dy, float* dw, float* db, float* ws,
                                   int n, int cin, int cout, int h, int w, int accumulate, int waves,
                                   ptmi_stream_t s);
/* ------------------------------------------------------------------ bf16 STORAGE path of the conv stack ("P8", round 4)
 * SOLVER.AMP.ENABLED (reference pt/engine/trainer.py:98; BASELINE configs[4]): under autocast the reference's cuDNN convolutions
 * (pt/modeling/backbone/vgg.py:45-53,66-69, pt/modeling/proposal_generator/rpn.py:96) read and write bf16 activations.  The
 * entry points below keep activations and activation gradients in bf16 in HBM and LDS, in the P8 layout
 *     t[2 ceil(C/16)][ROWS = N (H + 1) + 1][WS = W + 1][8]  bf16
 * pixel (n, r, c) at row n (H + 1) + 1 + r, column 1 + c; rows n (H + 1) and column 0 hold zeros (the convolution's zero padding
 * is part of the tensor: a tap is a flat pixel offset, no kernel tests an image edge); every entry point writes them as zeros.
 * Accumulation, bias, losses and weight gradients are fp32; a value is rounded to bf16 (nearest even) when it is stored.
 * ptmi_p8_plane_pixels = ROWS * WS (a tensor holds ptmi_p8_planes(C) * that many 16-byte pixel vectors). */
int64_t ptmi_p8_plane_pixels(int n, int h, int w);
/* A tensor of c channels holds ptmi_p8_planes(c) = 2 ceil(c/16) planes (whole 16-channel chunks; channels >= c are zeros: the
 * 3-channel image is the 16-channel input of the first layer). */
int ptmi_p8_planes(int c);
/* fp32 NCHW <-> P8 */
int ptmi_p8_from_nchw(const float* x, void* y, int n, int c, int h, int w, ptmi_stream_t s);
int ptmi_p8_to_nchw(const void* x, float* y, int n, int c, int h, int w, ptmi_stream_t s);
/* MaxPool2d(2,2) forward / backward (vgg.py:59,71) on P8 tensors; backward as ptmi_maxpool2x2_bwd (first maximum, optional
 * ReLU mask of the pooled activation). */
int ptmi_p8_maxpool2x2_fwd(const void* x, void* y, int n, int c, int h, int w, ptmi_stream_t s);
int ptmi_p8_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int n, int c, int h, int w, int relu_mask,
                           ptmi_stream_t s);
/* dz = dy * (y > 0) over `pixels16` 16-byte pixel vectors of P8 tensors */
int ptmi_p8_relu_bwd(const void* dy, const void* y, void* dz, int64_t pixels16, ptmi_stream_t s);
/* conv3x3 s1 p1 on P8 tensors: v_mfma_f32_32x32x16_bf16, fp32 accumulate, bf16 out; any channel counts (planes as above).
 * Weights packed by ptmi_p8_pack_weights (bf16, MFMA A-operand order [coTile][cin/16][tap][mt][64 lanes][8]; mode 0 forward,
 * mode 1 dgrad = flipped taps, transposed channels; ptmi_p8_packed_elems bf16 elements).
 * epilogue 0: + bias; 1: + bias, ReLU; 2: none (dgrad); 3: dgrad times (mask_ref > 0), mask_ref = the producing layer's stored
 * activation (P8, cout channels); 4: + bias, ReLU, 2x2 max-pool (floor) -- y is the P8 tensor of the POOLED map (n, cout, h/2,
 * w/2), pads included, and the full-resolution activation never reaches HBM (layers without a backward pass). */
int64_t ptmi_p8_packed_elems(int cin, int cout);
int ptmi_p8_pack_weights(const float* w, void* wp, int w_cout, int w_cin, int mode, ptmi_stream_t s);
int ptmi_p8_conv3x3(const void* x, const void* wp, const float* bias, const void* mask_ref, void* y, int n,
                    int cin, int cout, int h, int w, int epilogue, ptmi_stream_t s);
/* Weight + bias gradient of the conv above from its P8 input x (cin channels) and P8 output gradient dy (cout channels; pads
 * zero): dW (Cout, Cin, 3, 3) and db (Cout) in fp32 (same contract as ptmi_conv3x3_wgrad: split partials in a caller-allocated
 * workspace of ptmi_p8_wgrad_ws_floats floats, summed in a fixed order; accumulate != 0 adds to dW / db).  The contraction runs
 * over pixels: operands reach the MFMA through ds_read_b64_tr_b16; db is the product of dy with an all-ones operand. */
/* 1 if ptmi_p8_wgrad / ptmi_p8_gemm_nt serve the shape (their per-launch 32-bit buffer offsets: a P8 tensor of at most 4 GiB,
 * e.g. conv1_2 (64 channels, 1333x800) up to 31 images; fc1 up to ~85 k ROIs); the host side routes larger shapes elsewhere
 * (p8.wgrad: the fp32 direct kernel on the widened operands -- the same products, fp32 accumulation). */
int ptmi_p8_wgrad_fits(int n, int cin, int cout, int h, int w);
int ptmi_p8_gemm_nt_fits(int m, int n, int k);
int64_t ptmi_p8_wgrad_ws_floats(int n, int cin, int cout, int h, int w);
int ptmi_p8_wgrad(const void* x, const void* dy, float* dw, float* db, float* ws, int n, int cin, int cout,
                  int h, int w, int accumulate, ptmi_stream_t s);
/* The bf16-storage convolution / weight gradient with `waves` fills of the one-workgroup-per-CU slots (round 6; same contract as the
 * one-fill entry points = waves 1).  ptmi_p8_conv3x3's persistent workgroups walk items b, b + grid, ...; ptmi_p8_wgrad's own one
 * contiguous share each: a CU held by another kernel when the launch starts -- an RCCL collective overlapping backward under DDP,
 * pt/engine/trainer.py:92-95,384, the configuration BASELINE configs[4] names -- makes its workgroup run after all others (2x on the
 * launch, tools/exp/contention.py).  With more, shorter workgroups the dispatcher rebalances: what PTrainer selects when its gradient
 * exchange is active (convolution 16 waves: one more prologue per workgroup; weight gradient 4 waves: one more partial-sum store). */
int ptmi_p8_conv3x3_waves(const void* x, const void* wp, const float* bias, const void* mask_ref, void* y,
                          int n, int cin, int cout, int h, int w, int epilogue, int waves,
                          ptmi_stream_t s);
int64_t ptmi_p8_wgrad_ws_floats_waves(int n, int cin, int cout, int h, int w, int waves);
int ptmi_p8_wgrad_waves(const void* x, const void* dy, float* dw, float* db, float* ws, int n, int cin,
                        int cout, int h, int w, int accumulate, int waves, ptmi_stream_t s);
/* bf16-STORAGE GEMM for the box head's large Linear layer under SOLVER.AMP.ENABLED (FastRCNNConvFCHead fc1 25088 -> 1024 behind
 * pt/modeling/roi_heads/roi_heads.py:126-128; cuBLAS bf16 under autocast): C[m][n] (fp32, row pitch ldc) = A . B^T (+ bias[n]) (+ ReLU)
 * with BOTH operands bf16 in the "P8 matrix" layout t[ceil(k/8)][rows][8] (k in octets, one 16-byte vector per (row, octet)).
 * ptmi_p8m_pack builds an operand from an fp32 matrix: element (row, k) = src[row * ld + k] (k_major = 1) or src[k * ld + row]
 * (k_major = 0), rounded to bf16 (nearest even), zero beyond k; ptmi_p8m_elems bf16 elements.  Forward, dX and dW of a Linear layer
 * are all of this form (operands packed with their contraction index as k).  Shapes with few tiles and long k run split-K through a
 * caller-allocated workspace (ptmi_p8_gemm_nt_ws_floats floats; 0 = none), reduced in a fixed order.
 * relu: bit 0 = ReLU; bit 1 = store the result TRANSPOSED, C[n][m] with row pitch ldc >= m (no bias / ReLU / split-K): with the
 * operands swapped by the caller this writes the same matrix with 16-byte stores (fc1's dX, 1.6 GB of fp32, is store-bound). */
int64_t ptmi_p8m_elems(int rows, int k);
int ptmi_p8m_pack(const float* src, void* dst, int rows, int k, int64_t ld, int k_major, ptmi_stream_t s);
int64_t ptmi_p8_gemm_nt_ws_floats(int m, int n, int k);
int ptmi_p8_gemm_nt(const void* a, const void* b, float* c, const float* bias, float* ws, int m, int n, int k,
                    int ldc, int relu, ptmi_stream_t s);
/* dz = dy * (y > 0), elementwise (ReLU backward; F.relu_ at vgg.py:67). In-place allowed. */
int ptmi_relu_bwd(const float* dy, const float* y, float* dz, int64_t numel, ptmi_stream_t s);

/* ------------------------------------------------------------------ max pool (N2)
 * replaces ATen MaxPool2d(2,2) fwd/bwd at vgg.py:59,71 (floor mode).  bwd routes the gradient to
 * the first maximum of each window in (0,0),(0,1),(1,0),(1,1) order (ATen CPU semantics). */
int ptmi_maxpool2x2_fwd(const float* x, float* y, int nc, int h, int w, ptmi_stream_t s);
/* relu_mask != 0: x is a post-ReLU activation and the result is additionally multiplied by (x > 0), i.e. the
 * gradient w.r.t. the conv pre-activation (MaxPool2d backward + F.relu_ backward of vgg.py:66-71 in one pass). */
int ptmi_maxpool2x2_bwd(const float* x, const float* dy, float* dx, int nc, int h, int w,
                        int relu_mask, ptmi_stream_t s);

/* ------------------------------------------------------------------ GEMM (N3 1x1 convs, N13 FC)
 * replaces cuBLAS Linear (D2 FastRCNNConvFCHead; fast_rcnn.py:164) and the 1x1 RPN convs.
 * C[b] (M,N) = op(A[b]) (M,K) * op(B[b]) (K,N)  [+ bias] [relu] [+ C if accumulate]
 * ta: 0 -> A stored (M,K) row-major with leading dim lda; 1 -> stored (K,M).
 * tb: 0 -> B stored (K,N) row-major with leading dim ldb; 1 -> stored (N,K).
 * bias_mode: 0 none, 1 per-row (M), 2 per-column (N).  batch strides in elements.
 * fp32 on v_mfma_f32_32x32x2_f32; k-ordered accumulation (deterministic).
 * ws / ws_floats: optional workspace of ptmi_gemm_ws_floats(m, n, k, batch) floats.  With it, shapes with few 128x128
 * tiles and a long K (the box head's weight gradients) or a tile count just above a multiple of the chip's workgroup
 * slots run split-K: K slices into ws, summed in a fixed order (still deterministic).  NULL / 0 = never split. */
int64_t ptmi_gemm_ws_floats(int m, int n, int k, int batch);
int ptmi_gemm_f32(const float* a, const float* b, float* c, const float* bias, int m, int n,
                  int k, int lda, int ldb, int ldc, int ta, int tb, int bias_mode, int relu,
                  int accumulate, int batch, int64_t stride_a, int64_t stride_b,
                  int64_t stride_c, float* ws, int64_t ws_floats, ptmi_stream_t s);
/* Same contract, bf16-input / fp32-accumulate (SOLVER.AMP.ENABLED, pt/engine/trainer.py:98; BASELINE configs[4]): A and B
 * are fp32 in memory, every operand element is rounded to bf16 (round-to-nearest-even) on its way into
 * v_mfma_f32_32x32x16_bf16; products are exact in fp32 and accumulated in fp32; bias / ReLU / C stay fp32. */
int ptmi_gemm_bf16(const float* a, const float* b, float* c, const float* bias, int m, int n,
                   int k, int lda, int ldb, int ldc, int ta, int tb, int bias_mode, int relu,
                   int accumulate, int batch, int64_t stride_a, int64_t stride_b,
                   int64_t stride_c, float* ws, int64_t ws_floats, ptmi_stream_t s);
/* column sums: out[j] (+)= sum_i a[i][j]  (bias gradients), a is (rows, cols) row-major. */
int ptmi_colsum(const float* a, float* out, int rows, int cols, int accumulate, ptmi_stream_t s);
/* the same for tall matrices (rows >> cols: the 1x1 RPN heads' bias gradients, rpn.py:96 backward): row ranges are summed by
 * separate workgroups into ws (ptmi_colsum_ws_floats(rows, cols) floats; 0 = not worth splitting), then reduced in a fixed
 * order.  ws == NULL falls back to ptmi_colsum. */
int64_t ptmi_colsum_ws_floats(int rows, int cols);
int ptmi_colsum_ws(const float* a, float* out, float* ws, int rows, int cols, int accumulate, ptmi_stream_t s);
/* row sums over the inner dim: out[i] (+)= sum_j a[i][j] for each of `batch` slabs summed. */
int ptmi_rowsum_batched(const float* a, float* out, int batch, int rows, int cols, int accumulate,
                        ptmi_stream_t s);

/* ------------------------------------------------------------------ ROIAlign (N12)
 * replaces torchvision roi_align(aligned=True, sampling_ratio=0) built at
 * pt/modeling/roi_heads/roi_heads.py:68-73 and called at :126.  rois (R,5)=[img,x1,y1,x2,y2]. */
int ptmi_roi_align_fwd(const float* feat, const float* rois, float* out, int n, int c, int h,
                       int w, int r, int pooled, float scale, ptmi_stream_t s);
/* Same result to fp32 rounding (a bin's cells are summed with separable row / column weights, not sample by sample) for rois
 * GROUPED BY IMAGE (img_offsets int32 (n+1) device array): every bin row's / column's first cell and weights are tabulated
 * once into `ws` (ptmi_roi_align_ws_bytes(r, h, w) bytes of device scratch), channel planes are staged in LDS once per image.
 * ws == NULL falls back to ptmi_roi_align_fwd. */
int64_t ptmi_roi_align_ws_bytes(int r, int h, int w);
int ptmi_roi_align_fwd_grouped(const float* feat, const float* rois, const int32_t* img_offsets,
                               float* out, void* ws, int n, int c, int h, int w, int r, int pooled,
                               float scale, ptmi_stream_t s);
/* The grouped forward writing the box head's first Linear layer's bf16 operands directly (SOLVER.AMP.ENABLED; replaces the
 * ROIPooler -> flatten -> autocast Linear hand-over of roi_heads.py:126-128): xk = "P8 matrix" [c*49/8][r][8] of the flattened
 * ROI features (what ptmi_p8m_pack(k_major) of the fp32 result would hold, round to nearest even), xt (may be NULL) =
 * [ceil(r/8)][c*49][8], the weight gradient's operand (contraction over ROIs; rows beyond r are zeros).  pooled = 7 and maps
 * whose planes fit the LDS budget only: ptmi_roi_align_fwd_p8m_fits. */
int ptmi_roi_align_fwd_p8m_fits(int c, int h, int w, int pooled);
int ptmi_roi_align_fwd_p8m(const float* feat, const float* rois, const int32_t* img_offsets, void* xk, void* xt, void* ws,
                           int n, int c, int h, int w, int r, int pooled, float scale, ptmi_stream_t s);
/* dfeat must be zeroed by the caller (atomic scatter-add). */
int ptmi_roi_align_bwd(const float* dout, const float* rois, float* dfeat, int n, int c, int h,
                       int w, int r, int pooled, float scale, ptmi_stream_t s);
/* Same result (to summation order) for rois GROUPED BY IMAGE (rows img_offsets[i]..img_offsets[i+1] belong to image i; int32
 * device array of n+1): each workgroup accumulates up to four channel planes of one image in LDS, every plane row owned
 * by one wave, and writes them once -- no global atomics, a fixed summation order (bitwise reproducible), dfeat need not be
 * zeroed (every element is written).  `ws`: ptmi_roi_align_bwd_ws_bytes(r, h, w) bytes of device scratch for the per-ROI
 * weight tables (NULL, or planes that do not fit the LDS: the atomic kernel on a zeroed dfeat). */
int64_t ptmi_roi_align_bwd_ws_bytes(int r, int h, int w);
int ptmi_roi_align_bwd_grouped(const float* dout, const float* rois, const int32_t* img_offsets,
                               float* dfeat, void* ws, int n, int c, int h, int w, int r, int pooled,
                               float scale, ptmi_stream_t s);

/* The ROIAlign variants of detectron2's ROIPooler (MODEL.ROI_BOX_HEAD.POOLER_TYPE "ROIAlign", POOLER_SAMPLING_RATIO > 0): the
 * four entry points above followed by torchvision roi_align's `aligned` (1: half-pixel shift, "ROIAlignV2"; 0: no shift and a
 * ROI at least one cell wide and high, "ROIAlign") and `sampling_ratio` (0: ceil(roi extent / pooled) samples a bin side;
 * > 0: that many).  (1, 0) computes what the entry points above compute (those launch kernels compiled without the two
 * parameters).  The ptmi_roi_align_*ws_bytes queries hold for every variant.  aligned outside {0, 1} or sampling_ratio < 0: error. */
int ptmi_roi_align_fwd_ex(const float* feat, const float* rois, float* out, int n, int c, int h,
                          int w, int r, int pooled, float scale, ptmi_stream_t s, int aligned, int sampling_ratio);
int ptmi_roi_align_bwd_ex(const float* dout, const float* rois, float* dfeat, int n, int c, int h,
                          int w, int r, int pooled, float scale, ptmi_stream_t s, int aligned, int sampling_ratio);
int ptmi_roi_align_fwd_grouped_ex(const float* feat, const float* rois, const int32_t* img_offsets,
                                  float* out, void* ws, int n, int c, int h, int w, int r, int pooled,
                                  float scale, ptmi_stream_t s, int aligned, int sampling_ratio);
int ptmi_roi_align_bwd_grouped_ex(const float* dout, const float* rois, const int32_t* img_offsets,
                                  float* dfeat, void* ws, int n, int c, int h, int w, int r, int pooled,
                                  float scale, ptmi_stream_t s, int aligned, int sampling_ratio);
/* torchvision roi_pool (POOLER_TYPE "ROIPool"): out (R, c, pooled, pooled) = the maximum over the integer cells of each bin
 * (roundf of the scaled corners, floor / ceil bin edges clamped to the map), argmax (same shape, int32) = flat index h * W + w
 * of the first maximum in raster order, -1 (and value 0) for an empty bin.  Bit-exact against the reference loop. */
int ptmi_roi_pool_fwd(const float* feat, const float* rois, float* out, int32_t* argmax, int n, int c, int h, int w, int r,
                      int pooled, float scale, ptmi_stream_t s);
/* dfeat (n, c, h, w) = scatter-add of dout through argmax.  dfeat is zeroed here (r = 0 gives zeros); hardware fp32 atomics:
 * where several bins meet in one cell the summation order varies from run to run.  No gradient to the boxes. */
int ptmi_roi_pool_bwd(const float* dout, const int32_t* argmax, const float* rois, float* dfeat, int n, int c, int h, int w,
                      int r, int pooled, ptmi_stream_t s);

/* Order-independent pooler backwards (ops.deterministic): no floating-point atomics, every element of dfeat is a sum whose order
 * depends on the inputs alone (image, ROI index, bin, sample), never on workgroup scheduling; dfeat is written in full.  Rows of
 * rois / dout / argmax are grouped by image, img_offsets (n + 1, int32) as for ptmi_roi_align_bwd_grouped.
 * ptmi_roi_align_bwd_det: every (aligned, sampling_ratio); ws of ptmi_roi_align_bwd_ws_bytes is required.  It runs the band
 * kernel of ptmi_roi_align_bwd_grouped(_ex) -- fixed row ownership, ROIs in index order -- and FAILS where that entry would fall
 * back to the atomic scatter (pooled != 7, h > 256, a padded plane beyond 160 KB of LDS).
 * ptmi_roi_pool_bwd_det: a wave owns an (image, channel) plane and walks the image's ROIs in index order, bins in bin order. */
int ptmi_roi_align_bwd_det(const float* dout, const float* rois, const int32_t* img_offsets, float* dfeat, void* ws, int n, int c,
                           int h, int w, int r, int pooled, float scale, ptmi_stream_t s, int aligned, int sampling_ratio);
int ptmi_roi_pool_bwd_det(const float* dout, const int32_t* argmax, const int32_t* img_offsets, float* dfeat, int n, int c, int h,
                          int w, int r, int pooled, ptmi_stream_t s);

/* ------------------------------------------------------------------ boxes (N4, N5, N9)
 * anchors: D2 DefaultAnchorGenerator / pt/modeling/anchor_generator.py:108-122: out (h*w*A,4),
 * anchor n=(y*w+x)*A+a = [x*stride,y*stride,x*stride,y*stride] + cell[a] (offset 0 folded in). */
int ptmi_grid_anchors(const float* cell, float* out, int h, int w, int a, float stride,
                      float offset, ptmi_stream_t s);
/* Box2BoxTransform.apply_deltas, pt/modeling/box_regression.py:101-139.
 * deltas (rows, 4*k) with row stride `dstride` floats, boxes (nb,4) with row i using box
 * i % nb (nb = rows, or the anchor count when the same anchors repeat per image). */
int ptmi_apply_deltas(const float* deltas, const float* boxes, float* out, int64_t rows, int k,
                      int dstride, int64_t nb, float wx, float wy, float ww, float wh,
                      float scale_clamp, ptmi_stream_t s);
/* Box2BoxTransform.get_deltas, box_regression.py:66-99 (with the +1e-9 inside the logs). */
int ptmi_get_deltas(const float* src, const float* tgt, float* out, int64_t rows, float wx,
                    float wy, float ww, float wh, ptmi_stream_t s);
/* pairwise_iou + Matcher fused (rpn.py:414-415; roi_heads.py:207-214).
 * gt (m,4), boxes (nb,4); thresholds_host / labels_host are HOST arrays.  Outputs per box: matched gt index (int64, argmax over gt, lowest
 * index on ties), label (int8).  thresholds: n_thr in {1,2}; labels[n_thr+1].
 * allow_low_quality: every box whose IoU with gt i equals gt i's best IoU gets label 1.
 * ws: m floats of workspace (per-gt best IoU).  m == 0 -> idx 0, label labels[0]. */
int ptmi_iou_match(const float* gt, const float* boxes, int m, int64_t nb, const float* thresholds_host,
                   const int* labels_host, int n_thr, int allow_low_quality, int64_t* matched_idx,
                   int8_t* matched_label, float* matched_iou, float* ws, ptmi_stream_t s);

/* The same for a whole batch in one launch per pass.  gt_all: the images' gt boxes concatenated, gt_off (nimg+1) int32
 * DEVICE row offsets; boxes: either concatenated per image with box_off (nimg+1) int32 DEVICE offsets (outputs in the
 * same row order), or box_off == NULL: the same max_boxes boxes for every image (RPN anchors; outputs (nimg, max_boxes)).
 * max_boxes = largest per-image box count; matched_idx is the gt index WITHIN the image; ws: total_gt floats. */
int ptmi_iou_match_batched(const float* gt_all, const int32_t* gt_off, const float* boxes, const int32_t* box_off,
                           int nimg, int64_t max_boxes, int64_t total_gt, const float* thresholds_host,
                           const int* labels_host, int n_thr, int allow_low_quality, int64_t* matched_idx,
                           int8_t* matched_label, float* matched_iou, float* ws, ptmi_stream_t s);
/* ptmi_iou_match_batched with MODEL.RPN.BOUNDARY_THRESH folded in (rpn.py:421-425 -> D2 0.5 Boxes.inside_box): the same
 * arguments plus sizes_hw (nimg, 2) float32 DEVICE = (h, w) per image (the layout ptmi_rpn_prepare takes) and
 * boundary_thresh = t >= 0.  box_off must be NULL (one box set shared by all images; anything else is an argument error).
 * Box (x1, y1, x2, y2) is inside image i iff x1 >= -t && y1 >= -t && x2 < w_i + t && y2 < h_i + t, compared in fp32 (upper
 * bounds strict, a NaN coordinate is outside); every box that is not inside gets label -1.  The test sits where the label is
 * stored, after the thresholds and the low-quality rule, so there is no extra pass over nimg * max_boxes and no extra launch.
 * matched_idx and matched_iou are bit for bit those of ptmi_iou_match_batched. */
int ptmi_iou_match_batched_bounds(const float* gt_all, const int32_t* gt_off, const float* boxes, const int32_t* box_off,
                                  int nimg, int64_t max_boxes, int64_t total_gt, const float* thresholds_host,
                                  const int* labels_host, int n_thr, int allow_low_quality, int64_t* matched_idx,
                                  int8_t* matched_label, float* matched_iou, float* ws, const float* sizes_hw,
                                  float boundary_thresh, ptmi_stream_t s);
/* D2 subsample_labels (rpn.py:433 via RPN._subsample_labels; D2 StandardROIHeads._sample_proposals) for
 * a batch of label vectors without host syncs: cls_all int64 (concatenated; -1 ignore, bg_label background, anything
 * else foreground), keys_all i.i.d. uniform keys, offsets (nimg+1) int32 DEVICE.  Per image: n_fg = min(#fg,
 * num_pos_max), n_bg = min(#bg, num_samples - n_fg); out_fg (nimg, num_pos_max) / out_bg (nimg, num_samples) get the
 * local indices of the n_fg / n_bg candidates with the smallest keys in ascending key order (== the prefix of the
 * permutation argsort(keys[candidates])); counts (nimg, 2) int32 = (n_fg, n_bg).  max_count <= 12288. */
int ptmi_sample_by_keys(const int64_t* cls_all, const float* keys_all, const int32_t* offsets, int nimg,
                        int64_t max_count, int num_samples, int num_pos_max, int bg_label, int64_t* out_fg,
                        int64_t* out_bg, int32_t* counts, ptmi_stream_t s);

/* RPN._subsample_labels for a whole batch (pt/modeling/proposal_generator/rpn.py:433 -> D2 subsample_labels; SURVEY A.4,
 * N6): labels (nimg, r) int8 in {-1 ignore, bg_label, anything else = positive}, keys (nimg, r) float32 >= 0 (i.i.d.
 * uniform in production).  Per image n_f = min(#positives, num_pos_max), n_b = min(#negatives, num_samples - n_f); out
 * (nimg, r) int8 = 1 for the n_f positives and 0 for the n_b negatives with the smallest keys (ties: lowest index), -1
 * everywhere else.  Radix select on the key bits, one workgroup per image, no host sync. */
int ptmi_rpn_subsample_relabel(const int8_t* labels, const float* keys, int8_t* out, int nimg, int64_t r, int num_samples,
                               int num_pos_max, int bg_label, ptmi_stream_t s);

/* ------------------------------------------------------------------ sort + proposals (N10)
 * replaces torch.sort(descending) at pt/modeling/proposal_generator/proposal_utils.py:87 and the
 * sort inside torchvision nms.  Stable: ties keep ascending original index.
 * seg_offsets (nseg+1) int32 device array.  ws sized by ptmi_segsort_ws_bytes. */
int64_t ptmi_segsort_ws_bytes(int64_t total, int nseg);
int ptmi_segsort_desc(const float* keys_in, float* keys_out, int32_t* idx_out, int64_t total,
                      int nseg, const int32_t* seg_offsets, void* ws, int64_t ws_bytes,
                      ptmi_stream_t s);
/* The same order from ONE workgroup per segment sorting in LDS (bitonic network on (key, index) pairs): whole segments of up to
 * 16 384 keys; of longer segments (< 65 536 keys) only the first `topk` <= 16 384 entries of the sorted order (radix select +
 * ordered compaction first) -- entries past topk come back as (-inf, 0).  max_len = the longest segment (the caller knows it;
 * no device read).  ptmi_segsort_topk_fits tells whether a (max_len, topk) pair is served; otherwise use ptmi_segsort_desc. */
int ptmi_segsort_topk_fits(int64_t max_len, int64_t topk);
int ptmi_segsort_topk_desc(const float* keys_in, float* keys_out, int32_t* idx_out, int nseg, const int32_t* seg_offsets,
                           int64_t max_len, int64_t topk, ptmi_stream_t s);
/* proposal_utils.py:92-138 for one batch: for image i and rank j < k:
 *   box = clip(decoded[i][sorted_idx[i][j]], image_size[i]); kept = finite & w>min & h>min;
 *   score = sorted_logit[i][j] * (1 - mean4(sigmoid(sigma_logits[i][j])))   <- row j, NOT idx (:94)
 * Outputs dense (n,k,*): boxes, keys = score for kept entries / -inf for dropped ones (a stable descending sort of the
 * keys lists the kept entries in the order batched_nms visits them), the number of kept entries and a nonfinite flag
 * per image -- no host synchronisation is needed before NMS. */
int ptmi_rpn_prepare(const float* decoded, const float* sorted_logits, const int32_t* sorted_idx,
                     const float* sigma_logits, const float* image_sizes_hw, float* boxes_out,
                     float* keys_out, int32_t* counts_out, int32_t* nonfinite_out, int n,
                     int64_t r, int k, float min_size, ptmi_stream_t s);

/* ------------------------------------------------------------------ NMS (N11)
 * replaces torchvision nms (detectron2 batched_nms) at proposal_utils.py:140, fast_rcnn.py:104.
 * Batched over `nimg` images: boxes (sum counts,4) ALREADY sorted by descending score per image,
 * seg_offsets (nimg+1) int32; seg_counts (nimg) int32 or NULL: only the first seg_counts[i] boxes of segment i exist
 * (fixed-capacity segments whose fill level is known on the device only).  keep_out (nimg, max_keep) int32 =
 * positions within the image's sorted list, keep_count (nimg) int32.  Suppress iff IoU > thr (strict), IoU evaluated
 * as inter/(area_i+area_j-inter) in fp32 without FMA contraction => bit-exact vs the CPU oracle.
 * ws: ptmi_nms_ws_bytes(max_count, nimg), max_count = largest segment capacity. */
int64_t ptmi_nms_ws_bytes(int64_t max_count, int nimg);
int ptmi_nms_batched(const float* boxes, const int32_t* seg_offsets, const int32_t* seg_counts, int nimg,
                     int64_t max_count, float thr, int max_keep, int32_t* keep_out, int32_t* keep_count,
                     void* ws, ptmi_stream_t s);

/* ------------------------------------------------------------------ teacher ROI inference (N12)
 * fast_rcnn.py:34-101 (fast_rcnn_inference_single_image up to the NMS call) for all R ROIs of a batch: decode the K
 * mean quadruples of deltas (R, 8K) on proposal_boxes (R,4) with weights (wx,wy,ww,wh) (:63 drops the sigma
 * quadruples), finite filter over a ROI's K boxes and K+1 probabilities (:67), clip to the image roi_img[r] (:78),
 * probs[r][j] > score_thresh (:85), score *= 1 - mean4(sigmoid(sigma logits)) (:101).
 * Outputs dense over (roi, class): boxes_out (R,K,4) clipped; keys_out (R,K) = rescored score of a candidate, -1
 * otherwise (scores are > 0: a stable descending sort of an image's keys lists its candidates in batched_nms order);
 * img_max_out (nimg) = largest candidate coordinate, img_count_out (nimg) = number of candidates;
 * roi_valid_out (R) u8 = the finite filter's verdict, img_invalid_out (nimg) = ROIs it dropped (the reference indexes
 * `scores_logists` and the returned ROI indices by position in the FILTERED list, :96,:126). */
int ptmi_roi_infer_prepare(const float* deltas, const float* proposal_boxes, const float* probs,
                           const int32_t* roi_img, const float* image_sizes_hw, float* boxes_out,
                           float* keys_out, uint8_t* roi_valid_out, float* img_max_out,
                           int32_t* img_count_out, int32_t* img_invalid_out, int64_t r, int k, int nimg,
                           float wx, float wy, float ww, float wh, float scale_clamp, float score_thresh,
                           ptmi_stream_t s);
/* torchvision batched_nms class offset (fast_rcnn.py:104): out[beg_i + p] = boxes[beg_i + order[beg_i + p]] +
 * (order[..] % k) * (img_max[i] + 1) in fp32, for the dense per-image segments seg_offsets (nimg+1) of (roi, class)
 * entries; max_count = largest segment. */
int ptmi_roi_infer_nms_boxes(const float* boxes, const int32_t* order, const int32_t* seg_offsets,
                             const float* img_max, int nimg, int max_count, int k, float* out,
                             ptmi_stream_t s);
/* NMS per (image, class) segment -- the path for many classes: the bitmask workspace of ptmi_nms_batched grows with
 * nimg * k * max_r * ceil(max_r / 64) * 8 bytes here instead of nimg * (k max_r) * ceil(k max_r / 64) * 8.  The three entry
 * points below feed ptmi_segsort_* / ptmi_nms_batched and collect from them; all share ONE description of the class-major
 * layout: cls_seg_offsets (nimg * k + 1) int32, segment s = img * k + c holds the R_img entries of class c of image img in
 * ROI order and starts at cls_seg_offsets[s] = k * roff[img] + c * R_img (roff = first ROI row of the image).  max_r = the
 * largest R_img.  No host synchronisation; integer atomics only.
 *
 * class_keys: keys (R, k) of ptmi_roi_infer_prepare -> keys_out (k * R) class-major; seg_count_out (nimg * k) = number of
 * candidates of the segment (key >= 0; every other entry holds -1). */
int ptmi_roi_infer_class_keys(const float* keys, const int32_t* cls_seg_offsets, int nimg, int k, int max_r,
                              float* keys_out, int32_t* seg_count_out, ptmi_stream_t s);
/* class_nms_boxes: order = the index-within-segment output of a descending segmented sort of keys_out.  For segment
 * (img, c), position p: out[beg + p] = boxes[roff[img] + order[beg + p]][c] + off in fp32, off = c * (img_max[img] + 1)
 * while img_count[img] < 40000 (the bits ptmi_roi_infer_nms_boxes gives the same entry) and 0 otherwise: D2 0.5 batched_nms
 * (fast_rcnn.py:104) leaves the coordinate-offset trick at 40 000 boxes for one NMS per class on the unshifted boxes. */
int ptmi_roi_infer_class_nms_boxes(const float* boxes, const int32_t* order, const int32_t* cls_seg_offsets,
                                   const float* img_max, const int32_t* img_count, int nimg, int k, int max_r,
                                   float* out, ptmi_stream_t s);
/* class_collect: keep (nimg * k, max_keep) / keep_count (nimg * k) of ptmi_nms_batched over the segments; sorted_keys /
 * order of the segmented sort.  dense_keys_out (R, k), total = R * k entries: the key of every kept entry at its dense
 * (roi, class) place, -1 everywhere else; img_kept_out (nimg) = kept entries of the image over all classes.  A stable
 * descending sort of dense_keys_out per image lists the detections in batched_nms order (score descending, then ascending
 * dense index roi * k + class). */
int ptmi_roi_infer_class_collect(const float* sorted_keys, const int32_t* order, const int32_t* keep,
                                 const int32_t* keep_count, const int32_t* cls_seg_offsets, int nimg, int k, int max_r,
                                 int max_keep, int64_t total, float* dense_keys_out, int32_t* img_kept_out,
                                 ptmi_stream_t s);

/* ------------------------------------------------------------------ test-time augmentation (TEST.AUG)
 * detectron2 0.5 GeneralizedRCNNWithTTA._inverse_boxes + _merge_detections up to the NMS call, for the D detections of ALL
 * augmentations of a batch of nimg images: boxes (D,4) / scores (D) in augmented-image coordinates, concatenated in
 * augmentation order, augmentations grouped by image (an image's detections are one contiguous segment).  aug_offsets
 * (naug+1) int32: detections [aug_offsets[a], aug_offsets[a+1]) belong to augmentation a.  aug_meta (naug,3) int32 = image,
 * flipped, has pre-transform; aug_factors (naug,5) float = w_s, fx_s = fp32(w / w_s), fy_s = fp32(h / h_s), gx = fp32(W / w),
 * gy = fp32(H / h) (formed in double on the host, rounded once).  Per detection, every step its own fp32 operation, never
 * contracted: flipped: x = w_s - x; x *= fx_s, y *= fy_s; has pre-transform: x *= gx, y *= gy; min / max per axis after each
 * step (apply_box).  Then fast_rcnn_inference_single_image: a row with a non-finite coordinate or score is dropped, boxes are
 * clipped to image_sizes_hw[image] = (H, W), rows with score > score_thresh (strict) are the candidates.
 * Outputs: boxes_out (D,4) mapped and clipped ((0,0,0,0) for a row the finite filter dropped); keys_out (D) = score of a
 * candidate, -inf otherwise (a stable descending sort per image lists the candidates first, in batched_nms order);
 * img_count_out (nimg) = candidates, img_max_out (nimg) = their largest coordinate -- an integer max on the bits of the
 * non-negative floats: the same bits on every run.  All table entries device arrays; d == 0 only clears the two per-image
 * outputs. */
int ptmi_tta_map_boxes(const float* boxes, const float* scores, const int32_t* aug_offsets, const int32_t* aug_meta,
                       const float* aug_factors, const float* image_sizes_hw, float* boxes_out, float* keys_out,
                       float* img_max_out, int32_t* img_count_out, int64_t d, int naug, int nimg, float score_thresh,
                       ptmi_stream_t s);
/* torchvision batched_nms class offset for the merged detections: out[beg_i + p] = boxes[beg_i + order[beg_i + p]] +
 * classes[beg_i + order[beg_i + p]] * (img_max[i] + 1) in fp32 (the rounding of ptmi_roi_infer_nms_boxes), for the per-image
 * segments seg_offsets (nimg+1); classes (D) int64; order = index within the segment from the segmented sort of keys_out;
 * max_count = largest segment. */
int ptmi_tta_nms_boxes(const float* boxes, const int64_t* classes, const int32_t* order, const int32_t* seg_offsets,
                       const float* img_max, int nimg, int max_count, float* out, ptmi_stream_t s);

/* ------------------------------------------------------------------ COCO evaluation: detection <-> ground-truth matching
 * pycocotools COCOeval.computeIoU / evaluateImg with maskApi.c bbIou (detectron2 COCOEvaluator, pt/engine/trainer.py:132-133)
 * for ALL nseg (image, category) segments of an evaluation in one launch.  Segment i holds detections
 * [dt_off[i], dt_off[i+1]) of dt_xywh (nd,4) / dt_area (nd), already in descending-score order, and ground truth
 * [gt_off[i], gt_off[i+1]) of gt_xywh (ng,4) / gt_area (ng) / gt_crowd (ng) int32 in dataset order; both tables int64[nseg+1],
 * ascending, tiling [0, nd) and [0, ng).  iou_thr (nthr <= 16), area_rng (narea <= 4, 2) [lo, hi].  All float64.
 * Outputs (written in full when the tables tile the arrays): gt_ignore (narea, ng) = crowd || area < lo || area > hi;
 * dt_match (narea, nthr, nd) = position of the matched GT inside its segment or -1; dt_ignore (narea, nthr, nd) = the matched
 * GT's ignore flag, or for an unmatched detection "its own area lies outside [lo, hi]".
 * IoU = i / (crowd ? da : da + ga - i), i = w h of the overlap (0 when w <= 0 or h <= 0), no + 1, in double and in that
 * operation order.  Per (range, threshold), detections in order: best = min(thr, 1 - 1e-10); GT visited non-ignored first, then
 * ignored, each in dataset order; a GT already matched is skipped unless crowd; the scan ends when it holds a non-ignored match
 * and reaches the ignored GT; a GT with iou < best is skipped, every other one becomes the match and raises best to its iou.
 * max_dt / max_gt = the longest segment of either table, known to the caller: max_dt > 100 (maxDets[-1]),
 * max_gt > ptmi_coco_match_max_gt() (1024), nthr > 16 or narea > 4 is an error BEFORE anything is launched; a segment longer than
 * announced is left untouched by the kernel.  One wave per segment, a lane per (range, threshold); no atomics. */
int ptmi_coco_match_max_gt(void);
int ptmi_coco_match(const double* dt_xywh, const double* dt_area, const int64_t* dt_off, const double* gt_xywh,
                    const double* gt_area, const int32_t* gt_crowd, const int64_t* gt_off, int64_t nseg, int64_t nd,
                    int64_t ng, int max_dt, int max_gt, const double* iou_thr, int nthr, const double* area_rng, int narea,
                    int32_t* gt_ignore, int32_t* dt_match, int32_t* dt_ignore, ptmi_stream_t s);

/* ------------------------------------------------------------------ losses (N7, N8, N14)
 * Every loss kernel writes the scalar loss (already normalised) to loss_out[0] and the gradient
 * w.r.t. its differentiable inputs (already multiplied by 1/normaliser) in the same launch;
 * reductions are block-tree + fixed-order final sum (deterministic).  ws: 4096 floats. */
/* rpn.py:242-246: sum BCE-with-logits over label>=0, / norm.  labels int8 (-1,0,1). */
int ptmi_bce_logits_sum(const float* logits, const int8_t* labels, int64_t n, float inv_norm,
                        float* loss_out, float* dlogits, float* ws, ptmi_stream_t s);
/* box_regression.py:165-176 / fast_rcnn.py:286-296: sum over rows of -log(pdf(mu;t,var)+1e-9),
 * var = sigmoid(slog); d (rows,8) = [mu(4), slog(4)] gathered rows; t (rows,4) targets.
 * Gradients: dd (rows,8); dt (rows,4) optional (NULL to skip; needed for d(loss)/d(anchors)). */
int ptmi_gaussian_nll_sum(const float* d, const float* t, int64_t rows, float inv_norm,
                          float* loss_out, float* dd, float* dt, float* ws, ptmi_stream_t s);
/* fast_rcnn.py:408 + D2 FastRCNNOutputLayers.losses: mean cross entropy; dlogits (r,c). */
int ptmi_softmax_ce_mean(const float* logits, const int64_t* target, int64_t r, int c,
                         float* loss_out, float* dlogits, float* ws, ptmi_stream_t s);
/* softmax over the last dim (fast_rcnn.py:408 predict_probs). */
int ptmi_softmax_rows(const float* logits, float* probs, int64_t r, int c, ptmi_stream_t s);
/* fast_rcnn.py:179-213 cls_loss_unsupervised: teacher logits T (r,c), student logits S (r,c):
 * sum_r w_r * softmax(T/tau)·(-log_softmax(S)) * inv_norm, w_r=(1-H(softmax T)/log c)^lambda
 * (w_r = 1 if !efl).  dS (r,c). */
int ptmi_soft_ce_efl(const float* t, const float* s_logits, int64_t r, int c, float tau,
                     float lambda, int efl, float inv_norm, float* loss_out, float* ds, float* ws,
                     ptmi_stream_t s);
/* rpn.py:285-304 RPN soft objectness loss (incl. the sigmoid(1-x) quirk at :299).
 * T (k,c) teacher logits of the matched pseudo box per positive anchor, x (k) student objectness.
 * Also emits fg[k] (uint8) = argmax T != c-1 (rpn.py:292-293). */
int ptmi_rpn_soft_obj_loss(const float* t, const float* x, int64_t k, int c, float tau, float lambda,
                           int efl, float inv_norm, float* loss_out, float* dx, uint8_t* fg,
                           float* ws, ptmi_stream_t s);
/* rpn.py:321-355 / fast_rcnn.py:215-263: KL(N(mu_p,var_p*tau) || N(mu_q,var_q)) with the
 * per-coordinate entropy-focal weight; rows selected by fg (NULL = all rows).
 * q (rows,8)=[mu_q, slog_q]; mu_p (rows,4); slog_p (rows,4) teacher sigma logits.
 * reduction: 0 = sum*inv_norm (RPN), 1 = mean over selected rows*4 (ROI, inv_norm ignored).
 * Gradients dq (rows,8), dmu_p (rows,4; NULL when mu_p is detached as in fast_rcnn.py:235). */
int ptmi_kl_efl_loss(const float* q, const float* mu_p, const float* slog_p, const uint8_t* fg,
                     int64_t rows, float tau, float lambda, int efl, int reduction, float inv_norm,
                     float* loss_out, float* dq, float* dmu_p, float* ws, ptmi_stream_t s);
/* UNSUPNET.MODEL_TYPE = LAPLACE counterpart of ptmi_gaussian_nll_sum (same arguments and layouts):
 * box_regression.py:38-40,177-183 / fast_rcnn.py:298-307: sum over rows of
 * -log(exp(-|mu-t|/sqrt(var+1e-9)) / sqrt(4(var+0.3)) + 1e-9) * inv_norm, var = sigmoid(slog). */
int ptmi_laplace_nll_sum(const float* d, const float* t, int64_t rows, float inv_norm,
                         float* loss_out, float* dd, float* dt, float* ws, ptmi_stream_t s);
/* UNSUPNET.MODEL_TYPE = LAPLACE counterpart of ptmi_kl_efl_loss (same arguments, selection and
 * reductions): rpn.py:319-344 / fast_rcnn.py:238-257, per coordinate with vp = var_p*tau,
 * KL = sqrt(vp) exp(-|mu_q-mu_p|/sqrt(vp))/sqrt(var_q) + |mu_q-mu_p|/sqrt(var_q)
 *      + 0.5 log(var_q/vp) - 1,
 * entropy-focal weight (1 - (1 + 0.5 log(4 var_p)) / (1 + log 2))^lambda (unclamped). */
int ptmi_laplace_kl_efl_loss(const float* q, const float* mu_p, const float* slog_p,
                             const uint8_t* fg, int64_t rows, float tau, float lambda, int efl,
                             int reduction, float inv_norm, float* loss_out, float* dq,
                             float* dmu_p, float* ws, ptmi_stream_t s);
/* backward of get_deltas w.r.t. the SOURCE boxes (anchors), accumulated into danchors (na,4):
 * rows index anchors via anchor_index[i] (int64).  Used only for the differentiable anchors
 * (rpn.py:311 with danchor=True, anchor_generator.py:147). */
int ptmi_get_deltas_bwd_src(const float* src, const float* tgt, const float* ddeltas,
                            const int64_t* src_index, int64_t rows, float wx, float wy, float ww,
                            float wh, float* dsrc, ptmi_stream_t s);
/* the same gradient by a fixed-order two-stage segmented reduction (no atomics; rows ascending within chunks of 4096, chunks
 * ascending): dsrc (n_dst, 4) is WRITTEN, no zero fill needed; src_index values outside [0, n_dst) are ignored.  src_index =
 * NULL means the identity (n_dst == rows, plain stores, no workspace).  ws: ptmi_get_deltas_bwd_src_det_ws_floats floats.  Made
 * for many rows on few destinations: the work grows with ceil(n_dst / 64) x rows. */
int64_t ptmi_get_deltas_bwd_src_det_ws_floats(int64_t rows, int64_t n_dst);
int ptmi_get_deltas_bwd_src_det(const float* src, const float* tgt, const float* ddeltas,
                                const int64_t* src_index, int64_t rows, float wx, float wy, float ww,
                                float wh, float* dsrc, int64_t n_dst, float* ws, ptmi_stream_t s);

/* ------------------------------------------------------------------ training statistics (integer counters)
 * What the reference logs beside its losses.  Counts only: the ratios are formed on the host after the step's one
 * metrics readback.  Two launches each (per-workgroup partial counts in ws, then their sum); no atomics, and integer
 * sums do not depend on the order.  ws: 4096 int32.  counts_out is written in full; r == 0 / n == 0 writes zeros.
 * D2 0.5 _log_classification_stats (FastRCNNOutputLayers.losses): logits (r, c) with c = K + 1, gt_classes (r) int64.
 * counts_out[4] = rows with argmax == gt; rows with 0 <= gt < K (foreground); foreground rows with argmax == gt;
 * foreground rows with argmax == K.  argmax = the lowest index among equal maxima; NaN logits: unspecified. */
int ptmi_cls_stats(const float* logits, const int64_t* gt_classes, int64_t r, int c, int32_t* counts_out,
                   int32_t* ws, ptmi_stream_t s);
/* pt/modeling/proposal_generator/rpn.py:222-228: counts_out[2] = entries == 1, entries == 0 of the n int8 anchor labels. */
int ptmi_label_counts(const int8_t* labels, int64_t n, int32_t* counts_out, int32_t* ws, ptmi_stream_t s);

/* ------------------------------------------------------------------ optimiser / EMA (N15-N17)
 * flat fp32 buffers.  EMA: trainer.py:431-449  t = s*(1-k) + t*k  (that evaluation order). */
int ptmi_ema_update(const float* student, float* teacher, int64_t n, float keep_rate,
                    float one_minus_keep_rate, ptmi_stream_t s);
/* trainer.py:592-603 clip_gradient: sumsq_out[0] = sum g^2 (two-stage, deterministic). */
int ptmi_sumsq(const float* g, int64_t n, float* sumsq_out, float* ws, ptmi_stream_t s);
/* fused clip + SGD(momentum, weight decay) step (trainer.py:385-386; torch.optim.SGD semantics):
 * s = clip/max(sqrt(sumsq[0]),clip); g' = g*s + wd*p; buf = first ? g' : mu*buf+g'; p -= lr*buf. */
int ptmi_clip_sgd_step(float* p, const float* g, float* buf, int64_t n, const float* sumsq,
                       float clip_norm, float lr, float momentum, float weight_decay, int first,
                       ptmi_stream_t s);
int ptmi_scale_by_clip(float* g, int64_t n, const float* sumsq, float clip_norm, ptmi_stream_t s);
/* SOLVER.CLIP_GRADIENTS (D2 0.5 solver/build.py maybe_add_gradient_clipping, reached at trainer.py:80): torch's
 * clip_grad_value_ / clip_grad_norm_ applied to every parameter on its own, i.e. to every SEGMENT of the flat buffers, after
 * the global scale s above and before the update.  Device tables, built once by the caller:
 *   seg_off   int64[S + 1]  ascending element offsets of the segments; segment i = [seg_off[i], seg_off[i + 1])
 *   chunks    int64[C][2]   (start, segment): the segments cut into pieces of at most PTMI_SEG_CHUNK elements, segment by
 *                           segment and ascending within one; a piece ends at start + PTMI_SEG_CHUNK or at its segment's end
 *   seg_chunk int64[S + 1]  segment i owns chunks [seg_chunk[i], seg_chunk[i + 1])
 * One workgroup per chunk.  A chunk whose descriptor does not lie inside its segment and inside [0, n) is skipped.
 * n == 0 or S == 0: nothing is launched, 0 is returned. */
#define PTMI_SEG_CHUNK 8192
/* seg_norm[i] = || g s ||_2 (inf_norm 0) or max |g s| (inf_norm 1) over segment i.  No atomics, one fixed summation tree per
 * chunk and per segment: the bits depend on the values and the tables only, not on the grid, the timing or the address of g.
 * ws: C floats. */
int ptmi_seg_gradnorm(const float* g, int64_t n, const int64_t* seg_off, const int64_t* seg_chunk, int S,
                      const int64_t* chunks, int C, const float* sumsq, float clip_norm, int inf_norm, float* ws,
                      float* seg_norm, ptmi_stream_t s);
/* ptmi_clip_sgd_step with the per-segment clip: g' = clip(g*s) + wd*p, then as above; g is not written.
 * clip_type 0 ("value"): clamp(g*s, -clip_value, clip_value), seg_norm unused (may be NULL).
 * clip_type 1 ("norm"):  g*s*c, c = min(clip_value / (seg_norm[segment] + 1e-6), 1), seg_norm from ptmi_seg_gradnorm. */
int ptmi_clip_sgd_step_seg(float* p, const float* g, float* buf, int64_t n, const int64_t* seg_off, int S,
                           const int64_t* chunks, int C, const float* sumsq, float clip_norm, int clip_type,
                           float clip_value, const float* seg_norm, float lr, float momentum, float weight_decay,
                           int first, ptmi_stream_t s);
/* ptmi_clip_sgd_step_seg with the weight decay of every segment read from the device table seg_wd[S] (D2's
 * SOLVER.WEIGHT_DECAY_NORM: norm parameters decay at their own rate), and one more clip_type, 2 ("none"): g' = g*s + wd*p,
 * clip_value and seg_norm unused -- a run without SOLVER.CLIP_GRADIENTS.  Same kernel body as the two entries above: with a
 * constant table the result is bit-identical to ptmi_clip_sgd_step_seg, with clip_type 2 and a constant table to
 * ptmi_clip_sgd_step. */
int ptmi_clip_sgd_step_seg_wd(float* p, const float* g, float* buf, int64_t n, const int64_t* seg_off, int S,
                              const int64_t* chunks, int C, const float* sumsq, float clip_norm, int clip_type,
                              float clip_value, const float* seg_norm, float lr, float momentum, const float* seg_wd,
                              int first, ptmi_stream_t s);

/* ------------------------------------------------------------------ GroupNorm (+ ReLU) (csrc/groupnorm.hip)
 * MODEL.VGG.NORM "GN": D2 get_norm("GN", C) = torch.nn.GroupNorm(32, C) behind the convolution's bias, F.relu_ behind it.
 * z, y, dy, dz are (n, c, hw) fp32 NCHW maps; group (i, g) is the contiguous run of L = (c / groups) * hw floats at
 * (i * groups + g) * L.  mean and BIASED variance over the run; y = (z - mean) * rsqrt(var + eps) * gamma[ch] + beta[ch], then
 * max(y, 0) if relu.  mean_rstd: n * groups * 2 floats (mean, rstd per group), written by fwd and read by bwd.
 * Sums: every run (fwd) and every channel plane (bwd) is cut into pieces of PTMI_GN_CHUNK floats, one workgroup each; element j
 * of a piece always goes to thread (j / 4) % 256, whatever the address (16-byte loads where the piece starts on a 16-byte
 * boundary, dwords otherwise), and threads, waves and pieces are combined in one fixed order -- pieces in double precision, as
 * (count, mean, M2) by the parallel-variance formula in fwd.  No atomics: the bits depend on the values and the shape alone.
 * No lane reads or writes outside its run / plane.  ws: ptmi_gn_ws_bytes bytes, 256-byte aligned.
 * n == 0 or hw == 0: nothing is launched, 0 is returned.  c % groups != 0, a null pointer, or more than 2^31 - 1 pieces: < 0. */
#define PTMI_GN_CHUNK 4096
int ptmi_gn_chunk(void);
int64_t ptmi_gn_ws_bytes(int n, int c, int64_t hw, int groups);
int ptmi_gn_relu_fwd(const float* z, const float* gamma, const float* beta, float* y, float* mean_rstd, int n, int c,
                     int64_t hw, int groups, float eps, int relu, void* ws, ptmi_stream_t s);
/* g = dy * (y > 0) (relu) or dy; per plane A = sum g, B = sum g * xhat (xhat recomputed from z, mean, rstd);
 * dbeta[ch] = sum_i A, dgamma[ch] = sum_i B (WRITTEN, not accumulated); s1 = sum_{ch in g} gamma A, s2 = sum gamma B;
 * dz = rstd * (g * gamma - (s1 + xhat * s2) / L).  y may be NULL when relu == 0. */
int ptmi_gn_relu_bwd(const float* dy, const float* y, const float* z, const float* gamma, const float* mean_rstd,
                     float* dz, float* dgamma, float* dbeta, int n, int c, int64_t hw, int groups, int relu, void* ws,
                     ptmi_stream_t s);

/* ------------------------------------------------------------------ ROI mosaic (csrc/roi_mosaic.hip)
 * MODEL.ROI_BOX_HEAD.NUM_CONV > 0 (D2 FastRCNNConvFCHead's conv layers): pooled ROIs (r, c, pooled, pooled) are packed into
 * canvases so that the 3x3 kernels see ordinary maps.  p = pooled + 1, gx = max(1, 64 / p), S = gx * p: canvases are
 * (ceil(r / gx^2), c, S, S); ROI i sits in canvas i / gx^2, cell row (i % gx^2) / gx, cell column i % gx, its data in the cell's
 * first `pooled` rows and columns.  Row and column `pooled` of every cell (the gutter) and the cells past r hold exactly 0.0 in
 * every tensor a convolution reads.  All entries: no sync, the passed stream only, r == 0 launches nothing and returns 0; the
 * bits of every result depend on the values and the shape alone, not on the addresses (16-byte accesses where the canvas sits
 * on a 16-byte boundary, dwords otherwise; no atomics).
 * pack: x -> canvas, zeros written to gutters and empty cells (every canvas element is written).  unpack: canvas -> x, its
 * backward (and pack is unpack's).  mask: out = in on the data pixels, 0.0 on gutters and empty cells; out != in (the saved
 * output of the producing convolution stays as it is); its own backward. */
int ptmi_roi_mosaic_pack(const float* x, float* canvas, int r, int c, int pooled, ptmi_stream_t s);
int ptmi_roi_mosaic_unpack(const float* canvas, float* x, int r, int c, int pooled, ptmi_stream_t s);
int ptmi_roi_mosaic_mask(const float* in, float* out, int r, int c, int pooled, ptmi_stream_t s);
/* relu(GroupNorm(groups, c)(z)) per (ROI, group) over the data pixels of canvases: L = (c / groups) * pooled^2 values, mean and
 * BIASED variance, one wave per (ROI, group) with the cell in registers (at most PTMI_ROI_MOSAIC_GN_MAX_CELL =
 * (c / groups) * (pooled + 1)^2 floats): sum -> mean, corrected by the residual sum, then M2 about the mean.  y and dz get 0.0 on
 * gutters and empty cells.  mean_rstd: r * groups * 2 floats.  bwd: g = dy * (y > 0); dz = rstd * (g * gamma - (s1 + xhat * s2) / L);
 * dgamma / dbeta (WRITTEN) in two stages: per (canvas, channel) plane into ws (ptmi_roi_mosaic_gn_ws_bytes, 256-byte aligned),
 * then canvases in canvas order in double. */
#define PTMI_ROI_MOSAIC_GN_MAX_CELL 2048
int ptmi_roi_mosaic_gn_max_cell(void);
int64_t ptmi_roi_mosaic_gn_ws_bytes(int r, int c, int pooled, int groups);
int ptmi_roi_mosaic_gn_relu_fwd(const float* z, const float* gamma, const float* beta, float* y, float* mean_rstd, int r, int c,
                                int pooled, int groups, float eps, ptmi_stream_t s);
int ptmi_roi_mosaic_gn_relu_bwd(const float* dy, const float* y, const float* z, const float* gamma, const float* mean_rstd,
                                float* dz, float* dgamma, float* dbeta, int r, int c, int pooled, int groups, void* ws,
                                ptmi_stream_t s);

/* ------------------------------------------------------------------ anomaly mode (csrc/anomaly.hip)
 * PTrainer(detect_anomaly=True); the reference runs every step under torch.autograd.set_detect_anomaly (trainer.py:167).
 * Does a tensor hold a NaN or an infinity, and where is the first: x = n elements of dtype 0 (fp32) or 1 (bf16, 2-byte elements
 * as P8 tensors hold them), classified on the bit pattern (exponent all ones; mantissa zero or not).
 *   flags[slot] |= 1 if any element is NaN, |= 2 if any is +-inf;  first[slot] = min(first[slot], lowest non-finite index).
 * The caller resets the slots (flags 0, first INT64_MAX); scans into one slot accumulate.  One read pass; a clean tensor causes
 * NO global write (flags are combined inside the wave and the block, one lane of a block that found something issues the
 * atomicOr / atomicMin), and the index is the lowest one whatever the grid or the timing.  n == 0: nothing is launched, 0.
 * slot outside [0, nslots), a null pointer with n > 0 or an unknown dtype: < 0, ptmi_last_error() = "nonfinite_scan: ...". */
int ptmi_nonfinite_scan(const void* x, int64_t n, int dtype, int32_t* flags, int64_t* first, int slot, int nslots,
                        ptmi_stream_t s);
/* The same two flag bits for every SEGMENT of the flat gradient buffer g, over the tables of the per-parameter clipping kernels
 * above (seg_off int64[S + 1], chunks int64[C][2]; one workgroup per chunk, a descriptor outside its segment is skipped).
 * seg_flags int32[S] is cleared on the stream first; g is not written.  n == 0 or S == 0: nothing is launched, 0 is returned
 * (also with null tables). */
int ptmi_seg_nonfinite(const float* g, int64_t n, const int64_t* seg_off, int S, const int64_t* chunks, int C,
                       int32_t* seg_flags, ptmi_stream_t s);

/* ------------------------------------------------------------------ image prep (N18)
 * rcnn.py:40 -> D2 preprocess_image: out[i] (3,hmax,wmax) = (u8 - mean)/std, zero padded.
 * One launch per image (images have individual sizes). */
int ptmi_preprocess_image(const uint8_t* img, float* out, int h, int w, int hmax, int wmax,
                          float m0, float m1, float m2, float s0, float s1, float s2,
                          ptmi_stream_t s);
/* trainer.py:557-590 resize: bilinear (align_corners=False) shrink to (dh,dw), truncated to u8,
 * pasted at (y1,x1) on a canvas filled with int(pixel_mean).  Byte-exact with ATen's CPU kernel as the reference
 * runs it (generic NCHW path, FMA-contracted; see csrc/misc.hip). */
int ptmi_shrink_paste(const uint8_t* img, uint8_t* out, int h, int w, int dh, int dw, int y1,
                      int x1, int m0, int m1, int m2, ptmi_stream_t s);

/* Whole-batch variants (one launch instead of one per image; the step prepares 64 + 32 images).  `desc` is a DEVICE
 * array of 8 int64 words per image: [src u8 pointer, dst u8 pointer, h, w, dh, dw, y1, x1] (dst and dh..x1 are ignored
 * by preprocess; every pointed-to buffer is owned by the caller and must stay alive until the launch has run).
 * preprocess: out is (n, 3, hmax, wmax) fp32.  shrink_paste: max_elems = max_i 3*h_i*w_i (sizes the grid). */
int ptmi_preprocess_batched(const int64_t* desc, float* out, int n, int hmax, int wmax, float m0, float m1,
                            float m2, float s0, float s1, float s2, ptmi_stream_t s);
int ptmi_shrink_paste_batched(const int64_t* desc, int n, int64_t max_elems, int m0, int m1, int m2,
                              ptmi_stream_t s);

/* ------------------------------------------------------------------ strong augmentation on the device
 * replaces the per-image PIL / torchvision work of the two-crop mapper: pt/data/detection_utils.py:38-60
 * (ColorJitter(0.4,0.4,0.4,0.1), RandomGrayscale, GaussianBlur, Solarize), pt/data/transforms/augmentation_impl.py:21-53,
 * applied at pt/data/dataset_mapper.py:151-159.  Byte-exact with Pillow (oracle/csrc/ref_aug.c).  Planar uint8 (3,H,W)
 * images, batched through a DEVICE table of 8 int64 words per image: [src, dst, h, w, p4, p5, p6, p7].
 *   gray_sum : sums_out[i] = sum of convert("L") grey levels of image i (ImageStat, for ImageEnhance.Contrast)
 *   color    : p4 = op (0 copy, 1 brightness, 2 contrast, 3 saturation, 4 hue, 5 grayscale, 6 solarize); p5 = the float
 *              enhancement factor (its bit pattern); p6 = hue shift in 1/256 turns / solarize threshold; contrast reads
 *              gray_sums[i].  src == dst is allowed.
 *   box_blur : one pass of Pillow's extended box blur (GaussianBlur = 3 horizontal + 3 vertical passes):
 *              p4 = 0 along x / 1 along y, p5 = integer radius, p6 = ww, p7 = fw (24-bit fixed-point weights).  src != dst.
 *   hflip    : p4 = 1 flips the image left-right (D2 RandomFlip), 0 copies.  src != dst. */
int ptmi_aug_gray_sum_batched(const int64_t* desc, int n, int64_t max_hw, uint64_t* sums_out, ptmi_stream_t s);
int ptmi_aug_color_batched(const int64_t* desc, int n, int64_t max_hw, const uint64_t* gray_sums, ptmi_stream_t s);
int ptmi_aug_box_blur_batched(const int64_t* desc, int n, int64_t max_elems, ptmi_stream_t s);
int ptmi_aug_hflip_batched(const int64_t* desc, int n, int64_t max_elems, ptmi_stream_t s);
/*   resize   : one pass of Pillow's Image.resize(..., BILINEAR) (D2 ResizeShortestEdge / ResizeTransform of the weak
 *              augmentation, dataset_mapper.py:107-109; antialiasing triangle filter, 22-bit fixed-point coefficients):
 *              p4 = output size along the pass, p5 = 0: (3,h,w) -> (3,h,p4), 1: (3,h,w) -> (3,p4,w).  A resize is the x pass
 *              followed by the y pass (a pass whose size does not change is skipped).  Down-scaling factors up to 15. */
int ptmi_aug_resize_pass_batched(const int64_t* desc, int n, int64_t max_out_elems, ptmi_stream_t s);
/* Windowed sources: D2 RandomCrop (INPUT.CROP) in front of the resize / flip of the weak augmentation
 * (dataset_mapper.py:53-60) without a cropped copy.  `wdesc` is a DEVICE table of 16 int64 words per image:
 * [src, dst, row pitch, plane pitch, x0, y0, ch, cw, p8, p9, 0 x 6] -- src = element (0,0,0) of the underlying planar uint8
 * image (pitches in bytes), the window is rows y0 .. y0+ch-1, columns x0 .. x0+cw-1 of each of its 3 planes and must lie
 * inside the image (the caller checks; the kernels do not know the image's size); dst is dense.  src != dst.
 *   resize_window : the arithmetic of `resize` on the window: p8 = output size along the pass, p9 = 0: -> (3,ch,p8),
 *              1: -> (3,p8,cw).  The filter support is clamped to the WINDOW, so the result is Pillow's resize of the
 *              cropped array: no neighbour outside the crop contributes.  max_out_elems = max_i 3 * output pixels.
 *   flip_window : p8 = 0 copies the window, 1 flips it left-right, 2 top-bottom (D2 RandomFlip horizontal / vertical)
 *              -> (3,ch,cw).  max_elems = max_i 3*ch*cw.
 * Four output bytes per thread, moved as one dword where the addresses are 4-byte aligned and as bytes where not. */
int ptmi_aug_resize_window_pass_batched(const int64_t* wdesc, int n, int64_t max_out_elems, ptmi_stream_t s);
int ptmi_aug_flip_window_batched(const int64_t* wdesc, int n, int64_t max_elems, ptmi_stream_t s);
/* Decoded image -> record format: the HWC -> CHW transpose and the BGR swap of read_image (D2 detection_utils.read_image +
 * dataset_mapper.py:162-169) for the loader's decode workers, which stage Pillow's packed RGB bytes as they are.
 * `desc` is a DEVICE table of 8 int64 words per image: [src packed u8 (h,w,3), dst planar u8 (3,h,w), h, w, p4, 0, 0, 0];
 * p4 = 0 keeps the channel order, 1 reverses it (RGB -> BGR).  src may start at any byte address; src != dst.
 * max_pixels = max_i h_i*w_i (sizes the grid).  Four pixels per thread: three dword loads and one dword store per plane
 * where the addresses are 4-byte aligned, bytes where not. */
int ptmi_aug_unpack_hwc_batched(const int64_t* desc, int n, int64_t max_pixels, ptmi_stream_t s);

/* ------------------------------------------------------------------ diagnostics
 * CU-contention probe (round 6; no counterpart in the reference): n_cus workgroups that each hold one CU (64 KB of LDS: no
 * MFMA workgroup of this library fits beside one) for `microseconds` on stream s -- stands in for a collective's kernels
 * (RCCL all-reduce overlapping backward under DDP, pt/engine/trainer.py:92-95,384) when only one GPU is at hand.
 * tools/exp/contention.py, tests/test_wino4_gpu.py.  scratch: one int32 in device memory (never written). */
int ptmi_hold_cus(int32_t* scratch, int n_cus, int microseconds, ptmi_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* PTMI355_H */
