"""torch-facing wrappers of the HIP operators in libptmi355.so.

PyTorch is used here for device memory (caching allocator), the current HIP stream and the autograd tape
only; every operator body is a hand-written gfx950 kernel reached through the C ABI (include/ptmi355.h).
There is no CPU path: tensors must live on a ROCm device and the shared library must be present.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

F32 = torch.float32


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, dtype=F32, name="tensor"):
    if not t.is_cuda:
        raise _lib.PtmiError(f"{name}: expected a ROCm device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.PtmiError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.PtmiError(f"{name}: expected a contiguous tensor")
    return t


_WS = {}


def _ws(name: str, nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffers, one set per (device, stream): kernels of one stream are ordered, so reuse within it is
    safe; work on another stream (a teacher forward on its own stream, say) gets its own buffers instead of racing."""
    key = (name, device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _loss_ws(device) -> torch.Tensor:
    return _ws("loss", 4096 * 4, device)


# ---------------------------------------------------------------------------- HIP-event profiling (bench.py)
_PROF = None


def profile_start() -> None:
    """Start recording a HIP event pair around every launch group below, on the stream the kernels use."""
    global _PROF
    _PROF = []


def profile_stop() -> dict:
    """Synchronise and return {kernel: {"ms", "flops", "issued", "bytes", "calls"}} accumulated since profile_start()."""
    global _PROF
    rec, _PROF = _PROF or [], None
    torch.cuda.synchronize()
    out = {}
    for name, flops, nbytes, issued, e0, e1 in rec:
        d = out.setdefault(name, {"ms": 0.0, "flops": 0.0, "issued": 0.0, "bytes": 0.0, "calls": 0})
        d["ms"] += e0.elapsed_time(e1)
        d["flops"] += flops
        d["issued"] += issued
        d["bytes"] += nbytes
        d["calls"] += 1
    return out


class _prof:
    """flops / nbytes = ALGORITHMIC work of the launch group (every operand read once, every result written once; for a
    convolution the DIRECT-convolution FLOPs, whatever algorithm runs); issued = FLOPs of the MFMA instructions the launch
    actually issues (Winograd: 16 instead of 36 multiplies per 2x2 tile and channel pair, plus its tile padding)."""

    def __init__(self, name, flops=0.0, nbytes=0.0, issued=None):
        self.name, self.flops, self.nbytes = name, float(flops), float(nbytes)
        self.issued = float(flops if issued is None else issued)

    def __enter__(self):
        if _PROF is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _PROF is not None:
            self.e1.record()
            _PROF.append((self.name, self.flops, self.nbytes, self.issued, self.e0, self.e1))
        return False


# ============================================================================ bf16 operands (SOLVER.AMP.ENABLED)
# BASELINE.json configs[4] ("mixed bf16 convs + fp32 loss"; the reference's AMP flag, pt/engine/trainer.py:98): the
# conv / FC GEMM operands -- activations, weights and, in backward, the incoming gradients -- are rounded to bf16
# (round-to-nearest-even), products are accumulated in fp32; losses, box codec, NMS, optimiser are untouched.  Two ways to run it:
#   "bf16"          what SOLVER.AMP.ENABLED selects.  3x3 convolutions: the bf16-STORAGE kernels (p8.py / csrc/p8.hip, round 4):
#                   activations and activation gradients live in bf16 in HBM and LDS (what autocast stores in the reference), in
#                   the padded 8-channel-block layout; the backbone keeps them that way from the image to the block-5 feature
#                   map.  FC layers / 1x1 convolutions: ptmi_gemm_bf16 (fp32 tensors, operands rounded between LDS and the MFMA).
#   "bf16_emulate"  the same numerics on the fp32 kernels: operands are rounded by a separate pass (x.to(bf16).to(f32))
#                   and multiplied by v_mfma_f32_32x32x2_f32 -- a bf16 x bf16 product is exact in fp32 -- and what the storage
#                   kernels store in bf16 (3x3-conv outputs and input gradients) is rounded by a pass as well (`_rnd`;
#                   it matters beyond the next layer's operand rounding: max-pool backward breaks TIES between rounded values
#                   as autocast's bf16 pooling does), so the two modes differ in summation order only.  The native kernels
#                   are tested against this mode.
# Never enabled by bench.py's headline run (the headline metric is fp32).
_OPERAND_ROUNDING = None


def set_operand_rounding(mode: Optional[str]) -> None:
    global _OPERAND_ROUNDING
    if mode not in (None, "bf16", "bf16_emulate"):
        raise ValueError(f"unknown operand rounding {mode!r}")
    _OPERAND_ROUNDING = mode


@contextlib.contextmanager
def operand_rounding(mode: Optional[str]):
    """Scope the operand-rounding mode: a trainer (or an evaluation) carries its own mode and applies it around its forward /
    backward, so that two models with different SOLVER.AMP settings in one process do not change each other's numerics."""
    prev = _OPERAND_ROUNDING
    set_operand_rounding(mode)
    try:
        yield
    finally:
        set_operand_rounding(prev)


# ============================================================================ order-independent backward (SEED >= 0)
# The two backward kernels that add floats with hardware atomics -- the ROI pooler's scatter and get_deltas' gradient into the
# source boxes -- have atomic-free counterparts with a fixed summation order (ptmi_roi_align_bwd_det / ptmi_roi_pool_bwd_det /
# ptmi_get_deltas_bwd_src_det).  The flag routes the autograd backwards below to them; like the operand rounding it belongs to
# a trainer, which applies it around each of its steps.
_DETERMINISTIC = False


def is_deterministic() -> bool:
    return _DETERMINISTIC


@contextlib.contextmanager
def deterministic(flag: bool = True):
    """Scope the order-independent backward kernels (see above); restores the previous setting on exit."""
    global _DETERMINISTIC
    prev = _DETERMINISTIC
    _DETERMINISTIC = bool(flag)
    try:
        yield
    finally:
        _DETERMINISTIC = prev


# ============================================================================ anomaly mode (PTrainer(detect_anomaly=True))
# With a sink (probabilisticteacher_amd/anomaly.py: AnomalySink) every autograd Function below and in p8.py scans each tensor it
# returns from forward and each gradient it returns from backward -- one ptmi_nonfinite_scan launch per tensor into the sink's next
# slot.  Like the two flags above the sink belongs to a trainer, which applies it around each of its steps.  Without one a
# Function pays one `is None` test and executes the statements it executed before: no launch, no allocation.
# Labels: modules push scope names (anomaly_scope) and the model pushes the branch (anomaly_branch); a Function remembers the
# labels of its forward on its ctx, so that its backward -- which runs outside every `with` -- reports under the same path.
_ANOMALY = None
_ANOMALY_SCOPES: List[str] = []
_ANOMALY_BRANCHES: List[str] = []


@contextlib.contextmanager
def anomaly(sink):
    """Scope an anomaly sink (None = off); restores the previous one on exit."""
    global _ANOMALY
    prev = _ANOMALY
    _ANOMALY = sink
    try:
        yield sink
    finally:
        _ANOMALY = prev


@contextlib.contextmanager
def anomaly_scope(name: str):
    """Push a scope label ("backbone", "vgg_block5.0", ...: joined with dots they read like a state-dict path) for the scans made
    inside; a no-op without a sink."""
    if _ANOMALY is None:
        yield
        return
    _ANOMALY_SCOPES.append(name)
    try:
        yield
    finally:
        _ANOMALY_SCOPES.pop()


@contextlib.contextmanager
def anomaly_branch(name: str):
    """the model's branch ("supervised", "unsupervised", "unsup_data_weak", "joint") for the scans made inside; the innermost
    one counts.  A no-op without a sink."""
    if _ANOMALY is None:
        yield
        return
    _ANOMALY_BRANCHES.append(name)
    try:
        yield
    finally:
        _ANOMALY_BRANCHES.pop()


def anomaly_labels() -> Tuple[str, str]:
    """(branch, scope path) in force"""
    return (_ANOMALY_BRANCHES[-1] if _ANOMALY_BRANCHES else "", ".".join(_ANOMALY_SCOPES))


def _anomaly_scan(where: Tuple[str, str], phase: str, op: str, items) -> None:
    """items: (output name, tensor or None[, scope suffix[, P8 (n, c, h, w)]]) in the order the launches produced them"""
    branch, scope = where
    for item in items:
        name, t = item[0], item[1]
        if t is None:
            continue
        sub = item[2] if len(item) > 2 else None
        _ANOMALY.scan(t, phase, op, name, branch, (scope + "." + sub if scope else sub) if sub else scope,
                      item[3] if len(item) > 3 else None)


def _anomaly_fwd(ctx, op: str, items) -> None:
    """a Function's forward, sink active: remember the labels for backward, scan the results"""
    ctx.anomaly_where = where = anomaly_labels()
    _anomaly_scan(where, "forward", op, items)


def _anomaly_bwd(ctx, op: str, items) -> None:
    """a Function's backward, sink active: scan the gradients it returns under the labels of its forward"""
    _anomaly_scan(getattr(ctx, "anomaly_where", None) or anomaly_labels(), "backward", op, items)


def seg_nonfinite(g: torch.Tensor, table: "SegmentTable", seg_flags: torch.Tensor) -> torch.Tensor:
    """seg_flags[:S] (int32) = 1 if segment i of the flat gradient holds a NaN, | 2 if it holds an infinity (ptmi_seg_nonfinite);
    cleared by the entry point first; g is not written."""
    table.check(g)
    _chk(seg_flags, torch.int32, "seg_flags")
    if seg_flags.numel() < table.S:
        raise ValueError(f"seg_flags holds {seg_flags.numel()} words for {table.S} segments")
    _lib.call("ptmi_seg_nonfinite", _ptr(g), g.numel(), _ptr(table.seg_off), table.S, _ptr(table.chunks), table.C, _ptr(seg_flags),
              _stream())
    return seg_flags[: table.S]


def _rnd(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if _OPERAND_ROUNDING != "bf16_emulate" or t is None:
        return t
    return t.to(torch.bfloat16).to(F32)


def _rnd_grad(t: torch.Tensor) -> torch.Tensor:
    """Incoming gradient of a Linear / 1x1 conv: rounded by a tensor pass in BOTH bf16 modes -- besides the GEMMs (which
    would round it themselves in native mode) it feeds the bias-gradient reductions, which must see the same values."""
    return t if _OPERAND_ROUNDING is None else t.to(torch.bfloat16).to(F32)


def _native_bf16() -> bool:
    return _OPERAND_ROUNDING == "bf16"


def _no_native_bf16(what: str) -> None:
    if _native_bf16():
        raise _lib.PtmiError(f"{what} is an fp32-tensor entry point: in \"bf16\" mode the 3x3 convolutions run on the bf16-storage "
                             "kernels (probabilisticteacher_amd.p8; ops.conv3x3 / ops.vgg_block route there)")


def conv3x3_wgrad(x: torch.Tensor, dz: torch.Tensor, cout: int):
    """(dW, db) of a 3x3 s1 p1 convolution from its input and output gradient (N1 wgrad): the Winograd-domain kernel on
    the fp32 layers with >= 64 input and output channels whose map fits its 32-bit offsets, the direct split-K kernel otherwise
    (and under bf16 operand rounding)."""
    _no_native_bf16("ops.conv3x3_wgrad")
    n, cin, h, w = x.shape
    dw = torch.empty(cout, cin, 3, 3, dtype=F32, device=x.device)
    db = torch.empty(cout, dtype=F32, device=x.device)
    ws_query, entry, key, issued, takes_waves = _WGRAD_ROUTES[_wgrad_kind(cin, cout, h, w)]
    waves = (_WGRAD_WAVES,) if takes_waves else ()
    ws = _ws("wgrad", getattr(_lib.load(), ws_query)(n, cin, cout, h, w, *waves) * 4, x.device)
    with _prof(key, 2.0 * 9 * cin * cout * h * w * n, issued=issued(n, cin, cout, h, w) if issued else None):
        _lib.call(entry, _ptr(x), _ptr(dz), _ptr(dw), _ptr(db), _ptr(ws), n, cin, cout, h, w, 0, *waves, _stream())
    return dw, db


# ============================================================================ conv 3x3
# Forward / dgrad algorithm of the fp32 3x3 layers: "auto" = fused Winograd F(4x4,3x3) (csrc/wino4p.hip, round 6) where the
# input channel count is a multiple of 8 and >= 64, else fused Winograd F(2x2,3x3) (csrc/wino.hip) wherever the
# input has enough channels to amortise its per-workgroup prologue, the direct implicit GEMM (csrc/conv.hip) for the
# 3-channel stem; "wino2" = as "auto" without the F(4x4,3x3) kernel; "direct" = the direct kernel everywhere (comparison
# runs, tests).  "bf16_emulate" keeps the direct
# kernels (its parity statement -- products of rounded operands are exact in fp32 -- does not survive a transform); "bf16"
# does not come here at all (p8.py).
_CONV_ALGO = "auto"
_WINO_MIN_CIN = 32
_WINO4_MIN_CIN = 64
_WINO_WGRAD_MIN_C = 64         # the wgrad workgroup owns 64 co x 64 ci
_WINO4_WGRAD_MIN_CIN = 32      # the F(4x4,3x3) wgrad workgroup owns 64 co x 32 ci
_WINO4_WGRAD_MIN_FILL = 0.9    # ... and walks the map in chunks of 4 rows x 16 columns: below this share of real pixels per chunk the
                               # F(2x2,3x3)-domain kernel (7- or 8-k-step chunks, whichever fits the row) was faster (50 x 83, fill 0.83:
                               # 0.91x).  Re-measured with the border masks built once (tools/exp/wino4w_bench.py --layers conv5_1
                               # --n 48, twice; profiles/wino4w_border_masks_per_layer.txt): 50 x 83 1.034x / 1.031x (3.82 against
                               # 3.95 ms; 100 x 166 was 1.08x and 200 x 333 1.17x before it); with both kernels' chunk hand-over and set-up
                               # cut since (profiles/edge_fixup_per_layer.txt): 1.08x (3.38 against 3.65 ms).  So 50 x 83 would now gain 8 % here (1 ms of the step);
                               # the bar stays because tests/test_wino_gpu.py pins those maps to the older kernel -- lowering it is a
                               # change of its own together with that test


def _wino4_wgrad_fill(h: int, w: int) -> float:
    return (h * w) / float(-(-h // 4) * 4 * -(-w // 16) * 16)


def _wgrad_kind(cin: int, cout: int, h: int, w: int) -> str:
    """'wino4w' | 'wino' | 'direct': the kernel family ops.conv3x3_wgrad routes a weight-gradient launch of this shape to
    (F(4x4,3x3)-domain csrc/wino4w.hip, F(2x2,3x3)-domain csrc/wino.hip, direct split-K csrc/conv.hip)"""
    lib = _lib.load()
    if (_CONV_ALGO == "auto" and _OPERAND_ROUNDING is None and cin >= _WINO4_WGRAD_MIN_CIN and cout >= _WINO_WGRAD_MIN_C
            and lib.ptmi_conv3x3_wino4_wgrad_fits(h, w) and _wino4_wgrad_fill(h, w) >= _WINO4_WGRAD_MIN_FILL):
        return "wino4w"
    if (_use_wino(cin) and cin >= _WINO_WGRAD_MIN_C and cout >= _WINO_WGRAD_MIN_C
            and lib.ptmi_conv3x3_wino_wgrad_fits(h, w)):
        return "wino"
    return "direct"


def set_conv_algo(mode: str) -> None:
    global _CONV_ALGO
    if mode not in ("auto", "wino2", "direct"):
        raise ValueError(f"unknown conv algorithm {mode!r}")
    _CONV_ALGO = mode


@functools.lru_cache(maxsize=256)
def wino_issued_flops(n: int, cin: int, cout: int, h: int, w: int) -> float:
    """FLOPs of the v_mfma_f32_32x32x2_f32 instructions one ptmi_conv3x3_wino_fwd launch issues: a wave runs 16 MFMAs
    (4096 FLOP each) per 2-channel k-step for its 32 channels x 32 tiles (2 tile rows x 16 tile columns of the FLAT tile line:
    every (image, 8-row band) is a strip of `period` columns, csrc/wino.hip); waves none of whose tiles lies inside an image
    issue none.  (Checked against SQ_INSTS_VALU_MFMA_MOPS_F32, profiles/r03_*.)"""
    import numpy as np
    co_tiles, chunks, bands = -(-cout // 64), -(-cin // 8), -(-h // 8)
    period = (w + 4) & ~3
    n_strips = n * bands
    n_pix = -(-(n_strips * period) // 32)
    tu = (np.arange(n_pix, dtype=np.int64)[:, None] * 32 + 2 * np.arange(16, dtype=np.int64)[None, :])
    st, px = tu // period, tu % period
    col_ok = (st < n_strips) & (px < w)
    band = st % bands
    waves = 0
    for wn in (0, 1):
        waves += int((col_ok & (band * 8 + 4 * wn < h)).any(axis=1).sum())
    return float(waves) * 2 * co_tiles * chunks * 4 * 16 * 4096


@functools.lru_cache(maxsize=256)
def wino4_issued_flops(n: int, cin: int, cout: int, h: int, w: int) -> float:
    """FLOPs of the v_mfma_f32_16x16x4_f32 instructions one ptmi_conv3x3_wino4{,p}_fwd launch issues: a wave runs 72 MFMAs
    (2048 FLOP each) per 4-channel chunk for one tile row (16 tiles) of the FLAT tile line -- 36 positions x two 16-channel
    tiles in csrc/wino4.hip, 18 positions x four in csrc/wino4p.hip (the default family); the persistent kernel runs every wave
    of every tile (a wave whose tile row lies below the image would idle its SIMD either way).  (Checked against
    SQ_INSTS_VALU_MFMA_MOPS_F32 x 512, profiles/r05_*.)"""
    co_tiles, chunks, bands = -(-cout // 64), cin // 4, -(-h // 8)
    period = (w + 4) & ~3
    n_pix = -(-(n * bands * period) // 64)
    return float(n_pix) * co_tiles * 4 * chunks * 72 * 2048


def wino4_wgrad_issued_flops(n: int, cin: int, cout: int, h: int, w: int) -> float:
    """FLOPs of the MFMAs one ptmi_conv3x3_wino4_wgrad launch issues: per 64 co x 32 ci pair and chunk (one tile row x 16
    columns = 4 tiles = two k-steps) 2 x 18 v_mfma_f32_32x32x2_f32 x 4 waves x 4096 FLOP (csrc/wino4w.hip)"""
    pairs = -(-cout // 64) * -(-cin // 32)
    chunks = n * -(-h // 4) * -(-w // 16)
    return float(pairs) * chunks * 2 * 18 * 4 * 4096


def wino_wgrad_issued_flops(n: int, cin: int, cout: int, h: int, w: int) -> float:
    """FLOPs of the MFMAs one ptmi_conv3x3_wino_wgrad launch issues: per 64 co x 64 ci pair and chunk (one tile row x KSN
    tile pairs; KSN = 7 or 8, whichever pads a tile row less -- csrc/wino.hip: wino_wgrad_ksn) KSN k-steps x 16 positions x
    4 waves x 4096 FLOP"""
    pairs = -(-cout // 64) * -(-cin // 64)
    tile_pairs = -(-(-(-w // 2)) // 2)
    ksn = 7 if -(-tile_pairs // 7) * 7 < -(-tile_pairs // 8) * 8 else 8
    chunks = n * -(-h // 2) * -(-w // (4 * ksn))
    return float(pairs) * chunks * ksn * 16 * 4 * 4096


# _wgrad_kind -> (workspace query, entry point, profile key, issued-FLOP function, takes the `waves` argument): what
# conv3x3_wgrad launches.  wino4w: csrc/wino4w.hip (workgroup = 64 co x 32 ci); wino: csrc/wino.hip; direct: csrc/conv.hip
_WGRAD_ROUTES = {
    "wino4w": ("ptmi_conv3x3_wino4_wgrad_ws_floats_waves", "ptmi_conv3x3_wino4_wgrad_waves", "conv3x3_wino4_wgrad",
               wino4_wgrad_issued_flops, True),
    "wino": ("ptmi_conv3x3_wino_wgrad_ws_floats_waves", "ptmi_conv3x3_wino_wgrad_waves", "conv3x3_wino_wgrad",
             wino_wgrad_issued_flops, True),
    "direct": ("ptmi_conv3x3_wgrad_ws_floats", "ptmi_conv3x3_wgrad", "conv3x3_wgrad", None, False),
}


def _use_wino(conv_cin: int, conv_cout: Optional[int] = None, hw: Optional[Tuple[int, int]] = None) -> bool:
    """Winograd routing of a 3x3 layer: fp32, enough input channels, and -- when the caller knows the map size -- a shape
    that fits the kernel's 32-bit buffer offsets (ptmi_conv3x3_wino_fwd_fits; larger maps run the direct kernel)."""
    if not (_CONV_ALGO in ("auto", "wino2") and _OPERAND_ROUNDING is None and conv_cin >= _WINO_MIN_CIN):
        return False
    if hw is None or conv_cout is None:
        return True
    return bool(_lib.load().ptmi_conv3x3_wino_fwd_fits(conv_cin, conv_cout, int(hw[0]), int(hw[1])))


def _use_wino4(conv_cin: int, conv_cout: Optional[int] = None, hw: Optional[Tuple[int, int]] = None) -> bool:
    """F(4x4,3x3) routing of a 3x3 layer (checked BEFORE _use_wino): fp32, input channels a multiple of 8 and >= 64, and -- when
    the caller knows the map size -- a shape that fits the kernel's 32-bit buffer offsets (ptmi_conv3x3_wino4_fwd_fits)."""
    if not (_CONV_ALGO == "auto" and _OPERAND_ROUNDING is None and conv_cin >= _WINO4_MIN_CIN and conv_cin % 8 == 0):
        return False
    if hw is None or conv_cout is None:
        return True
    return bool(getattr(_lib.load(), _conv_abi("wino4") + "_fwd_fits")(conv_cin, conv_cout, int(hw[0]), int(hw[1])))


def _conv_kind(conv_cin: int, conv_cout: Optional[int] = None, hw: Optional[Tuple[int, int]] = None) -> str:
    """'wino4' | 'wino' | 'mfma' (the direct kernel): the kernel family a forward / dgrad launch of this shape is routed to"""
    if _use_wino4(conv_cin, conv_cout, hw):
        return "wino4"
    return "wino" if _use_wino(conv_cin, conv_cout, hw) else "mfma"


# kind -> C-ABI family.  "wino4" is served by csrc/wino4p.hip since round 6 (positions split over the wave pair: 2 - 4 % faster on every
# layer shape but one, tools/exp/wino4_bench.py --p); set_wino4_family("wino4") selects round 5's csrc/wino4.hip (comparison runs)
_WINO4_FAMILY = "wino4p"


def _conv_abi(kind: str) -> str:
    """C-ABI prefix of a _conv_kind: the entry points are <prefix>_packed_floats / _pack_weights / _fwd (wino4: + _fwd_fits, _fwd_sched)"""
    return {"wino4": "ptmi_conv3x3_" + _WINO4_FAMILY, "wino": "ptmi_conv3x3_wino", "mfma": "ptmi_conv3x3"}[kind]


def set_wino4_family(name: str) -> None:
    """the kernel family behind the "wino4" route: "wino4p" (default, csrc/wino4p.hip) | "wino4" (csrc/wino4.hip).  Packed weights
    are family-specific: packs made before the switch must not be used after it."""
    global _WINO4_FAMILY
    if name not in ("wino4", "wino4p"):
        raise ValueError(f"unknown F(4x4,3x3) kernel family {name!r}")
    _WINO4_FAMILY = name


def _conv_issued(kind: str, n: int, cin: int, cout: int, h: int, w: int):
    return (wino4_issued_flops(n, cin, cout, h, w) if kind == "wino4" else
            wino_issued_flops(n, cin, cout, h, w) if kind == "wino" else None)


def conv3x3_pack(w: torch.Tensor, mode: int, epilogue: int, hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """Packed weights for conv3x3_raw(..., epilogue) (mode 0) or for the dgrad launch (mode 1: epilogue 2 / 3).  hw = (H, W)
    of the map the weights will be applied to: decides between the Winograd and the direct pack for maps beyond the Winograd
    kernel's 32-bit offsets (None = the map fits; conv3x3_raw checks the pack it is handed against its own routing)."""
    _no_native_bf16("ops.conv3x3_pack")
    _chk(w, name="conv weight")
    co, ci = w.shape[0], w.shape[1]
    conv_cin, conv_cout = (ci, co) if mode == 0 else (co, ci)
    abi = _conv_abi(_conv_kind(conv_cin, conv_cout, hw))
    n = getattr(_lib.load(), abi + "_packed_floats")(conv_cin, conv_cout)
    wp = torch.empty(n, dtype=F32, device=w.device)
    _lib.call(abi + "_pack_weights", _ptr(w), _ptr(wp), co, ci, mode, _stream())
    return wp


# Tile schedule of the persistent F(4x4,3x3) kernel (csrc/wino4p.hip; csrc/wino4.hip alike): "dynamic" (work queues) or "static"
# (b, b + grid, ...).  PTrainer selects "dynamic" when the gradient exchange is active.
_TILE_SCHEDULE = "static"
_SCHED_BUFS: dict = {}


def set_tile_schedule(mode: str) -> None:
    """Tile schedule of the persistent forward / dgrad kernel: "static" (the walk b, b + grid, ...: fastest when nothing else runs
    on the GPU) or "dynamic" (workgroups draw tiles from eight XCD queues, so CUs held by another kernel -- an RCCL collective
    overlapping backward -- cost their share, not a second pass: tools/exp/contention.py; +0.5 % without contention, and the
    dynamic instantiation's chunk loop is 2.6 % slower).  PTrainer selects "dynamic" whenever its gradient exchange is active."""
    global _TILE_SCHEDULE
    if mode not in ("dynamic", "static"):
        raise ValueError(f"unknown tile schedule {mode!r}")
    _TILE_SCHEDULE = mode


_WGRAD_WAVES = 1                # fills of the one-workgroup-per-CU slots by the Winograd-domain weight-gradient kernels


_P8_CONV_WAVES = 1               # ... and by the persistent bf16-storage convolution (ptmi_p8_conv3x3_waves)


def set_p8_conv_waves(waves: int) -> None:
    """1 (default): one persistent workgroup per CU; > 1: that many fills, each workgroup walking a 1 / waves share of the tiles --
    PTrainer selects 16 when its gradient exchange is active."""
    global _P8_CONV_WAVES
    if not 1 <= int(waves) <= 64:
        raise ValueError(f"p8 conv waves {waves!r} outside 1 .. 64")
    _P8_CONV_WAVES = int(waves)


def set_wgrad_waves(waves: int) -> None:
    """1 (default): one long workgroup per CU; > 1: that many waves of shorter workgroups (ptmi_conv3x3_wino*_wgrad_waves) -- what
    PTrainer selects when its gradient exchange is active, so that CUs held by the collectives cost their share."""
    global _WGRAD_WAVES
    if not 1 <= int(waves) <= 16:
        raise ValueError(f"wgrad waves {waves!r} outside 1 .. 16")
    _WGRAD_WAVES = int(waves)


def _sched_buf(device):
    """the 16-int32 schedule words of ptmi_conv3x3_wino4_fwd_sched for the CURRENT stream of `device` (zero at creation; the
    kernel leaves them zero) -- one buffer per (device, stream): launches that may overlap must not share one"""
    if _TILE_SCHEDULE != "dynamic":
        return None
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    b = _SCHED_BUFS.get(key)
    if b is None:
        b = _SCHED_BUFS[key] = torch.zeros(16, dtype=torch.int32, device=device)
    return b


def _conv_fwd_call(kind: str, x, wp, bias, mask_ref, y, n, cin, cout, h, w, epilogue):
    if kind == "wino4":
        _lib.call(_conv_abi(kind) + "_fwd_sched", _ptr(x), _ptr(wp), _ptr(bias), _ptr(mask_ref), _ptr(y), n, cin, cout, h, w,
                  epilogue, _ptr(_sched_buf(x.device)), _stream())
    else:
        _lib.call(_conv_abi(kind) + "_fwd", _ptr(x), _ptr(wp), _ptr(bias), _ptr(mask_ref), _ptr(y), n, cin, cout, h, w, epilogue,
                  _stream())


# ---------------------------------------------------------------------------- the constant frame of shrink-pasted images
# PTrainer.resize pastes every strong view, shrunk, into a canvas of one colour: inside that frame every layer's output is a fixed
# 4x4-periodic pattern.  A FrameState travels with such a batch through the backbone's forward pass: per image the ring where the
# NEXT layer's input holds the pattern (csrc/frame_skip.h), and the pattern itself.  A routed layer then runs the tile-list launch
# (ptmi_conv3x3_wino4p_fwd_list) over the pixel tiles that hold anything else and ptmi_frame_fill over the rest; the pattern of its
# output comes out of the layer's own kernel, run on a small probe canvas tiled with the input pattern.
_FRAME_SKIP = True
# A layer takes the list launch only if the list drops at least this share of its pixel tiles.  Measured per layer at n = 48
# (profiles/frame_skip_per_layer.txt): the list kernel costs 0.4 - 1.4 % per tile more than the plain one, and a list that drops
# 2 - 3 % of conv3_2 / conv3_3 ran 4 - 6 % SLOWER than the plain launch; 7.2 % (conv3_1) was the smallest share that won.
_FRAME_MIN_SHARE = 0.07
_FRAME_PROBE_HW = (24, 128)
_FRAME_CACHE: dict = {}


def set_frame_skip(on: bool) -> None:
    """False: every forward launch walks all of its tiles, whatever rings a batch carries (tests, A/B runs)."""
    global _FRAME_SKIP
    _FRAME_SKIP = bool(on)


def frame_skip_active() -> bool:
    """the tile-list launch exists for the static schedule of the fp32 wino4p family only"""
    return (_FRAME_SKIP and _TILE_SCHEDULE == "static" and _WINO4_FAMILY == "wino4p" and _CONV_ALGO == "auto" and
            _OPERAND_ROUNDING is None)


class FrameState:
    """rings: CPU int32 (n, 8) -- per image outer / inner rectangle in the resolution of the next layer's input (outer x1 <= x0:
    no ring); pattern: device (C, 4, 4) -- what that input holds inside the rings, indexed [c][y & 3][x & 3]; key: a hashable
    identity of the pattern (None: not cacheable, it depends on trainable parameters)."""

    def __init__(self, rings: torch.Tensor, pattern: torch.Tensor, key=None):
        self.rings = rings.to(torch.int32).contiguous()
        self.pattern = pattern
        self.key = key
        self.alive = True
        self._lists = None

    def lists(self, n: int, h: int, w: int, device):
        """(device int32 buffer [rings | keep | skip], n_keep, n_skip) for an (n, *, h, w) input: built on the host from the
        rings, uploaded from pinned memory on the current stream -- no round trip, no synchronisation"""
        if self._lists is not None and self._lists[0] == (n, h, w):
            return self._lists[1:]
        lib = _lib.load()
        n_pix = int(lib.ptmi_frame_pixel_tiles(n, h, w))
        host = torch.empty(n * 8 + n_pix, dtype=torch.int32).pin_memory()
        host[:n * 8] = self.rings.reshape(-1)
        skip = torch.empty(n_pix, dtype=torch.int32)
        counts = torch.zeros(2, dtype=torch.int32)
        _lib.call("ptmi_frame_skip_lists", ctypes.c_void_p(self.rings.data_ptr()), n, h, w,
                  ctypes.c_void_p(host.data_ptr() + 4 * n * 8), ctypes.c_void_p(skip.data_ptr()), ctypes.c_void_p(counts.data_ptr()))
        nk, ns = int(counts[0]), int(counts[1])
        if ns:
            host[n * 8 + nk:] = skip[:ns]
        buf = host.to(device, non_blocking=True) if ns else None
        self._lists = ((n, h, w), buf, nk, ns)
        return self._lists[1:]

    def share(self, n: int, h: int, w: int, device) -> float:
        _, nk, ns = self.lists(n, h, w, device)
        return ns / float(max(nk + ns, 1))

    def advance(self, op: int, h: int, w: int, pattern: torch.Tensor, key=None) -> None:
        """the state behind a layer with an h x w input: op 0 = conv3x3 by a direct kernel, 1 = max pool 2x2, 2 = conv3x3 by the
        F(4x4, 3x3) kernels (whole tiles only: ptmi_frame_ring_next)"""
        nxt = torch.empty_like(self.rings)
        _lib.call("ptmi_frame_ring_next", ctypes.c_void_p(self.rings.data_ptr()), ctypes.c_void_p(nxt.data_ptr()),
                  int(self.rings.shape[0]), op, int(h), int(w))
        self.rings, self.pattern, self.key, self._lists = nxt, pattern, key, None


def frame_rings(frames: Sequence[Optional[Tuple[int, int, int, int]]], sizes: Sequence[Tuple[int, int]]) -> Optional[torch.Tensor]:
    """per image (x1, y1, dw, dh) of PTrainer.resize (None: not a shrink-pasted image) and its (h, w) -> rings at image resolution,
    or None if no image has one"""
    if not any(f is not None for f in frames):
        return None
    rows = []
    for f, (h, w) in zip(frames, sizes):
        rows.append([0] * 8 if f is None else [0, 0, int(w), int(h), int(f[0]), int(f[1]), int(f[0]) + int(f[2]), int(f[1]) + int(f[3])])
    return torch.tensor(rows, dtype=torch.int32)


def _frame_tile_pattern(pattern: torch.Tensor, h: int, w: int) -> torch.Tensor:
    return pattern.repeat(1, h // 4, w // 4).unsqueeze(0).contiguous()


def _frame_probe(run, frame: FrameState, cache_key, pooled: bool) -> Tuple[torch.Tensor, object]:
    """The pattern of a layer's output from the layer's own kernel: run(probe canvas) -> its output on a canvas tiled with the input
    pattern; one interior, tile-aligned 4x4 block per channel.  cache_key (frozen layers: parameter versions, kernel family) makes the
    result a constant of the model as long as the input pattern is one too."""
    key = None if (cache_key is None or frame.key is None) else (frame.key, cache_key, pooled)
    if key is not None and key in _FRAME_CACHE:
        return _FRAME_CACHE[key], key
    ph, pw = _FRAME_PROBE_HW
    with _prof("frame_probe"):
        y = run(_frame_tile_pattern(frame.pattern, ph, pw))
        pat = (y[0, :, 4:8, 4:8] if pooled else y[0, :, 8:12, 8:12]).contiguous()
    if key is not None:
        if len(_FRAME_CACHE) >= 64:          # (parameters reloaded many times over: start again)
            _FRAME_CACHE.clear()
        _FRAME_CACHE[key] = pat
    return pat, key


class _param_key:
    """identity of frozen parameters as a cache key: storage, version counter and shape when the key was made.  The key holds the
    tensors, so a cached entry's storage cannot be freed and handed to other parameters."""

    def __init__(self, *params):
        self.params = params
        self.id = tuple((p.data_ptr(), p._version, tuple(p.shape)) for p in params)

    def __hash__(self):
        return hash(self.id)

    def __eq__(self, other):
        return isinstance(other, _param_key) and self.id == other.id


def frame_pool(frame: Optional[FrameState], h: int, w: int) -> None:
    """a separate 2x2 max pool of an h x w map behind the layer: the pooled pattern is the pool kernel's output on the tiled pattern"""
    if frame is None or not frame.alive:
        return
    c = frame.pattern.shape[0]
    src = _frame_tile_pattern(frame.pattern, 8, 8)
    out = torch.empty((1, c, 4, 4), dtype=F32, device=src.device)
    _lib.call("ptmi_maxpool2x2_fwd", _ptr(src), _ptr(out), c, 8, 8, _stream())
    frame.advance(1, h, w, out[0], None if frame.key is None else (frame.key, "pool"))


def _frame_end(frame: Optional[FrameState]) -> None:
    """a path that does not serve a FrameState ends its chain: no layer behind it probes or takes the list launch"""
    if frame is not None:
        frame.alive = False


def _frame_key(frame: Optional[FrameState], weight, bias):
    """cache identity of a layer's parameters for _frame_probe: None without a frame, or when either is trainable (probe every step)"""
    return None if (frame is None or weight.requires_grad or bias.requires_grad) else _param_key(weight, bias)


def _conv3x3_launch(x, wp, bias, mask_ref, cout: int, epilogue: int, frame: Optional[FrameState] = None, frame_key=None) -> torch.Tensor:
    """The one launch of an fp32 3x3 layer, forward (epilogue 0 / 1 / 4) or dgrad (2 / 3): output, route, pack check, work figures,
    profile bracket.  A live FrameState is served on the forward epilogues 1 and 4: the output pattern from a probe launch of the
    layer's own entry point (same packed weights, bias and epilogue), then the list launch + fill or the plain launch, then the
    state moves to the layer's output.  Every other path ends it."""
    n, cin, h, w = x.shape
    pooled = epilogue == 4
    y = torch.empty((n, cout, h // 2, w // 2) if pooled else (n, cout, h, w), dtype=F32, device=x.device)
    kind = _conv_kind(cin, cout, (h, w))
    want = getattr(_lib.load(), _conv_abi(kind) + "_packed_floats")(cin, cout)
    if wp.numel() != want:
        raise _lib.PtmiError(f"conv3x3_raw: packed weights have {wp.numel()} floats, the {kind} kernel this {h}x{w} map is "
                             f"routed to takes {want} (pass hw=(H, W) to conv3x3_pack)")
    flops = 2.0 * 9 * cin * cout * h * w * n
    nbytes = 4.0 * (n * h * w * (cin + cout * {3: 2, 4: 0.25}.get(epilogue, 1)) + 9 * cin * cout)
    ph, pw = _FRAME_PROBE_HW
    # a frame is served by a kernel whose outputs are known to repeat bit for bit: the F(4x4, 3x3) family (tile by tile) or the
    # 3-channel stem kernel (pixel by pixel); and the probe must run the same one
    served = (frame is not None and frame.alive and frame_skip_active() and epilogue in (1, 4) and
              (kind == "wino4" or (kind == "mfma" and cin < 8)) and _conv_kind(cin, cout, (ph, pw)) == kind)
    base = None
    if served:
        def run(canvas):
            out = torch.empty((1, cout, ph // 2, pw // 2) if pooled else (1, cout, ph, pw), dtype=F32, device=x.device)
            _conv_fwd_call(kind, canvas, wp, bias, None, out, 1, cin, cout, ph, pw, epilogue)
            return out

        pat, key = _frame_probe(run, frame, None if frame_key is None else (frame_key, kind, _WINO4_FAMILY), pooled)
        if kind == "wino4":       # the list launch + fill, if the list drops a worthwhile share of the pixel tiles
            buf, nk, ns = frame.lists(n, h, w, x.device)
            if ns > 0 and ns >= _FRAME_MIN_SHARE * (nk + ns):
                base = buf.data_ptr()
    else:
        _frame_end(frame)
    with _prof("conv3x3_" + kind, flops, nbytes, _conv_issued(kind, n, cin, cout, h, w)):
        if base is not None:
            _lib.call("ptmi_conv3x3_wino4p_fwd_list", _ptr(x), _ptr(wp), _ptr(bias), None, _ptr(y), n, cin, cout, h, w, epilogue,
                      ctypes.c_void_p(base + 4 * n * 8), nk, _stream())
            _lib.call("ptmi_frame_fill", ctypes.c_void_p(base + 4 * (n * 8 + nk)), ns, ctypes.c_void_p(base), _ptr(pat), _ptr(y), n,
                      cout, h, w, int(pooled), _stream())
        else:
            _conv_fwd_call(kind, x, wp, bias, mask_ref, y, n, cin, cout, h, w, epilogue)
    if served:
        op = 2 if kind == "wino4" else 0
        if pooled:        # the pattern is the pooled one already; the rings pass the convolution, then the pool
            frame.advance(op, h, w, pat, None)
            frame.advance(1, h, w, pat, key)
            h, w = h // 2, w // 2
        else:
            frame.advance(op, h, w, pat, key)
        # the chain ends at the first layer whose input would not be worth a list launch (rings only shrink, tiles only grow)
        if h < 8 or w < 8 or frame.share(n, h, w, x.device) < _FRAME_MIN_SHARE:
            _frame_end(frame)
    return y


def conv3x3_raw(x, wp, bias, mask_ref, cout: int, epilogue: int, frame: Optional[FrameState] = None, frame_key=None) -> torch.Tensor:
    """wp = conv3x3_pack(w, mode, epilogue) with the SAME epilogue.  frame: the batch's FrameState at this layer's input; a forward
    layer with a ReLU (epilogue 1; the pooled epilogue 4 comes through conv3x3_relu_pool_nograd) advances it to the layer's output,
    every other epilogue ends it.  frame_key: identity of (weights, bias) if they are frozen."""
    _no_native_bf16("ops.conv3x3_raw")
    return _conv3x3_launch(_chk(x, name="conv input"), wp, bias, mask_ref, cout, epilogue, frame, frame_key)


def conv3x3_relu_pool_nograd(x, weight, bias, frame: Optional[FrameState] = None) -> torch.Tensor:
    """conv3x3 + bias + ReLU + MaxPool(2,2) in ONE kernel (epilogue 4); inference-only (no autograd state).  frame: as conv3x3_raw
    (the layer's parameters have no backward pass here: they count as frozen)."""
    if _native_bf16():
        from . import p8
        _frame_end(frame)
        return p8.conv3x3_relu_pool_nograd_nchw(_chk(x.contiguous(), name="conv input"), weight, bias)
    x = _chk(_rnd(x).contiguous(), name="conv input")
    wp = conv3x3_pack(_chk(_rnd(weight).contiguous()), 0, 4, x.shape[-2:])
    frame_key = _frame_key(frame, weight.detach(), bias.detach())       # (detached: frozen as far as this call goes)
    return _rnd(_conv3x3_launch(x, wp, _chk(bias.contiguous()), None, weight.shape[0], 4, frame, frame_key))


def relu_bwd(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    dz = torch.empty_like(dy)
    if dy.numel() == 0:
        return dz
    with _prof("relu_bwd"):
        _lib.call("ptmi_relu_bwd", _ptr(_chk(dy.contiguous())), _ptr(_chk(y)), _ptr(dz), dy.numel(), _stream())
    return dz


# ============================================================================ max pool
def _maxpool2x2_fwd(x, frame: Optional[FrameState] = None) -> torch.Tensor:
    """2x2 max pool of a checked map; a live FrameState passes the pool with it"""
    n, c, h, w = x.shape
    y = torch.empty((n, c, h // 2, w // 2), dtype=F32, device=x.device)
    with _prof("maxpool_fwd"):
        _lib.call("ptmi_maxpool2x2_fwd", _ptr(x), _ptr(y), n * c, h, w, _stream())
    frame_pool(frame, h, w)
    return y


def _maxpool2x2_bwd(x, dy, relu_mask: bool) -> torch.Tensor:
    """gradient of the pool's input x from that of its output; relu_mask: times (x > 0), the mask of the ReLU that produced x"""
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    _lib.call("ptmi_maxpool2x2_bwd", _ptr(x), _ptr(_chk(dy)), _ptr(dx), n * c, h, w, int(relu_mask), _stream())
    return dx


class _MaxPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, frame=None):
        x = _chk(x.contiguous(), name="pool input")
        y = _maxpool2x2_fwd(x, frame)
        ctx.save_for_backward(x)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "maxpool2x2", (("y", y),))
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = _maxpool2x2_bwd(ctx.saved_tensors[0], dy.contiguous(), False)
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "maxpool2x2", (("dx", dx),))
        return dx, None


def maxpool2x2(x, frame: Optional[FrameState] = None):
    """frame: as conv3x3 (the state passes the pool with the map)"""
    return _MaxPool2x2.apply(x, frame)


# ============================================================================ GroupNorm + ReLU (MODEL.VGG.NORM "GN")
def gn_chunk() -> int:
    """PTMI_GN_CHUNK: the piece size of the GroupNorm reductions (floats)"""
    return int(_lib.load().ptmi_gn_chunk())


def _gn_ws(n: int, c: int, hw: int, groups: int, device) -> torch.Tensor:
    nbytes = int(_lib.load().ptmi_gn_ws_bytes(n, c, hw, groups))
    if nbytes < 0:
        raise _lib.PtmiError(f"ptmi_gn_ws_bytes failed: {_lib.load().ptmi_last_error().decode()}")
    return _ws("groupnorm", nbytes, device)


def _gn_bytes(n: int, c: int, hw: int, maps: int) -> float:
    return 4.0 * (maps * n * c * hw + 2 * c)


class _GroupNormReLU(torch.autograd.Function):
    """relu(GroupNorm(groups, C)(z)): D2's Conv2d norm child + VGGBlock's F.relu_ (vgg.py:52,65-72).  Saves z, y and the group
    statistics; backward recomputes xhat from z."""

    @staticmethod
    def forward(ctx, z, gamma, beta, groups: int, eps: float, relu: bool):
        z = _chk(z.contiguous(), name="group norm input")
        gamma, beta = _chk(gamma.contiguous(), name="group norm weight"), _chk(beta.contiguous(), name="group norm bias")
        if z.dim() < 2:
            raise ValueError(f"group_norm_relu: expected (N, C, ...) input, got {tuple(z.shape)}")
        n, c = int(z.shape[0]), int(z.shape[1])
        if groups <= 0 or c % groups:
            raise ValueError(f"group_norm_relu: {c} channels do not divide into {groups} groups")
        if gamma.numel() != c or beta.numel() != c:
            raise ValueError(f"group_norm_relu: weight / bias of {gamma.numel()} / {beta.numel()} elements for {c} channels")
        hw = z.numel() // (n * c) if n * c else 0
        y = torch.empty_like(z)
        stats = torch.empty((n * groups, 2), dtype=F32, device=z.device)
        with _prof("gn_relu_fwd", 0.0, _gn_bytes(n, c, hw, 3)):         # z twice (statistics, apply), y once
            _lib.call("ptmi_gn_relu_fwd", _ptr(z), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(stats), n, c, hw, groups, float(eps),
                      int(bool(relu)), _ptr(_gn_ws(n, c, hw, groups, z.device)), _stream())
        ctx.groups, ctx.relu = groups, bool(relu)
        ctx.save_for_backward(z, y if relu else None, gamma, stats)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "group_norm_relu", (("y", y),))
        return y

    @staticmethod
    def backward(ctx, dy):
        z, y, gamma, stats = ctx.saved_tensors
        dy = _chk(dy.contiguous(), name="group norm grad")
        n, c = int(z.shape[0]), int(z.shape[1])
        hw = z.numel() // (n * c) if n * c else 0
        dz = torch.empty_like(z)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        if z.numel() == 0:
            dgamma.zero_(), dbeta.zero_()
        with _prof("gn_relu_bwd", 0.0, _gn_bytes(n, c, hw, 7 if ctx.relu else 5)):      # dy, z (and y) twice, dz once
            _lib.call("ptmi_gn_relu_bwd", _ptr(dy), _ptr(y), _ptr(z), _ptr(gamma), _ptr(stats), _ptr(dz), _ptr(dgamma), _ptr(dbeta),
                      n, c, hw, ctx.groups, int(ctx.relu), _ptr(_gn_ws(n, c, hw, ctx.groups, z.device)), _stream())
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "group_norm_relu", (("dgamma", dgamma), ("dbeta", dbeta), ("dz", dz)))
        return dz, dgamma, dbeta, None, None, None


def group_norm_relu(z, gamma, beta, groups: int = 32, eps: float = 1e-5, relu: bool = True):
    """relu(group_norm(z, groups, gamma, beta, eps)) on (N, C, ...) fp32 maps (csrc/groupnorm.hip); fp32 only: the bf16-storage
    stack has no norm layer"""
    _no_native_bf16("ops.group_norm_relu")
    return _GroupNormReLU.apply(z, gamma, beta, int(groups), float(eps), bool(relu))


# ============================================================================ ROI mosaic (MODEL.ROI_BOX_HEAD.NUM_CONV > 0)
# Pooled ROIs (R, C, P, P) packed into canvases (ceil(R / gx^2), C, S, S) -- cell pitch p = P + 1, gx = max(1, 64 // p) cells a side,
# S = gx * p -- so that conv3x3 sees ordinary maps (csrc/roi_mosaic.hip).  Invariant: gutters (row / column P of a cell) and the
# cells past R are exactly 0.0 in every tensor a convolution reads (x in forward, dz in backward).
ROI_MOSAIC_CHUNK = 8192     # ROIs per pack: 128 canvases of 64 x 64, far inside every conv entry's 32-bit offsets and grid bounds


def roi_mosaic_geometry(r: int, pooled: int) -> Tuple[int, int, int, int]:
    """(p, gx, S, canvases) of r ROIs pooled to `pooled` x `pooled`"""
    p = int(pooled) + 1
    gx = max(1, 64 // p)
    return p, gx, gx * p, -(-int(r) // (gx * gx))


ROI_MOSAIC_GN_MAX_CELL = 2048   # PTMI_ROI_MOSAIC_GN_MAX_CELL, for code that must not load the library (model construction)


def roi_mosaic_gn_max_cell() -> int:
    """PTMI_ROI_MOSAIC_GN_MAX_CELL: floats of a (ROI, group) cell, (C / G) * (P + 1)^2, the mosaic GroupNorm holds in a wave"""
    return int(_lib.load().ptmi_roi_mosaic_gn_max_cell())


def _mosaic_bytes(r: int, c: int, pooled: int, maps: int) -> float:
    _, _, s, ncv = roi_mosaic_geometry(r, pooled)
    return 4.0 * maps * ncv * c * s * s


def _mosaic_canvas(canvas, r: int, pooled: int, name: str):
    _, _, s, ncv = roi_mosaic_geometry(r, pooled)
    canvas = _chk(canvas.contiguous(), name=name)
    if canvas.dim() != 4 or canvas.shape[0] != ncv or tuple(canvas.shape[2:]) != (s, s):
        raise ValueError(f"{name}: expected ({ncv}, C, {s}, {s}) canvases for {r} ROIs of {pooled} x {pooled}, got {tuple(canvas.shape)}")
    return canvas


def _mosaic_pack(x):
    x = _chk(x.contiguous(), name="roi mosaic input")
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f"roi_mosaic_pack: expected (R, C, P, P) pooled ROIs, got {tuple(x.shape)}")
    r, c, pooled = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    _, _, s, ncv = roi_mosaic_geometry(r, pooled)
    canvas = torch.empty((ncv, c, s, s), dtype=F32, device=x.device)
    with _prof("roi_mosaic_pack", 0.0, 4.0 * x.numel() + _mosaic_bytes(r, c, pooled, 1)):
        _lib.call("ptmi_roi_mosaic_pack", _ptr(x), _ptr(canvas), r, c, pooled, _stream())
    return canvas


def _mosaic_unpack(canvas, r: int, pooled: int):
    canvas = _mosaic_canvas(canvas, r, pooled, "roi mosaic canvas")
    c = int(canvas.shape[1])
    x = torch.empty((r, c, pooled, pooled), dtype=F32, device=canvas.device)
    with _prof("roi_mosaic_unpack", 0.0, 4.0 * x.numel() + _mosaic_bytes(r, c, pooled, 1)):
        _lib.call("ptmi_roi_mosaic_unpack", _ptr(canvas), _ptr(x), r, c, pooled, _stream())
    return x


def _mosaic_mask(canvas, r: int, pooled: int):
    canvas = _mosaic_canvas(canvas, r, pooled, "roi mosaic canvas")
    out = torch.empty_like(canvas)
    with _prof("roi_mosaic_mask", 0.0, _mosaic_bytes(r, int(canvas.shape[1]), pooled, 2)):
        _lib.call("ptmi_roi_mosaic_mask", _ptr(canvas), _ptr(out), r, int(canvas.shape[1]), pooled, _stream())
    return out


class _RoiMosaicPack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.meta = (int(x.shape[0]), int(x.shape[2]))
        return _mosaic_pack(x)

    @staticmethod
    def backward(ctx, dcanvas):
        return _mosaic_unpack(dcanvas, *ctx.meta)


class _RoiMosaicUnpack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, canvas, r, pooled):
        return _mosaic_unpack(canvas, r, pooled)

    @staticmethod
    def backward(ctx, dx):
        return _mosaic_pack(dx), None, None         # (writes the zeros of gutters and empty cells)


class _RoiMosaicMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, canvas, r, pooled):
        ctx.meta = (r, pooled)
        return _mosaic_mask(canvas, r, pooled)

    @staticmethod
    def backward(ctx, dout):
        return _mosaic_mask(dout, *ctx.meta), None, None


def roi_mosaic_pack(x):
    """(R, C, P, P) pooled ROIs -> (ceil(R / gx^2), C, S, S) canvases, gutters and empty cells 0.0; backward: roi_mosaic_unpack"""
    _no_native_bf16("ops.roi_mosaic_pack")
    return _RoiMosaicPack.apply(x)


def roi_mosaic_unpack(canvas, r: int, pooled: int):
    """the data pixels of the canvases -> (r, C, pooled, pooled); backward: roi_mosaic_pack"""
    _no_native_bf16("ops.roi_mosaic_unpack")
    return _RoiMosaicUnpack.apply(canvas, int(r), int(pooled))


def roi_mosaic_mask(canvas, r: int, pooled: int):
    """a copy of the canvases with gutters and empty cells zeroed (the input -- a convolution's saved output -- is not written);
    its own backward"""
    _no_native_bf16("ops.roi_mosaic_mask")
    return _RoiMosaicMask.apply(canvas, int(r), int(pooled))


def _mosaic_gn_ws(r: int, c: int, pooled: int, groups: int, device) -> torch.Tensor:
    nbytes = int(_lib.load().ptmi_roi_mosaic_gn_ws_bytes(r, c, pooled, groups))
    if nbytes < 0:
        raise _lib.PtmiError(f"ptmi_roi_mosaic_gn_ws_bytes failed: {_lib.load().ptmi_last_error().decode()}")
    return _ws("roi_mosaic_gn", nbytes, device)


class _RoiMosaicGNReLU(torch.autograd.Function):
    """relu(GroupNorm(groups, C)(z)) per ROI over the data pixels of canvases; y and dz get 0.0 on gutters and empty cells.  Saves
    z, y and the (ROI, group) statistics; backward recomputes xhat from z."""

    @staticmethod
    def forward(ctx, z, gamma, beta, r, pooled, groups, eps):
        z = _mosaic_canvas(z, r, pooled, "roi mosaic group norm input")
        gamma, beta = _chk(gamma.contiguous(), name="group norm weight"), _chk(beta.contiguous(), name="group norm bias")
        c = int(z.shape[1])
        if groups <= 0 or c % groups:
            raise ValueError(f"roi_mosaic_gn_relu: {c} channels do not divide into {groups} groups")
        if gamma.numel() != c or beta.numel() != c:
            raise ValueError(f"roi_mosaic_gn_relu: weight / bias of {gamma.numel()} / {beta.numel()} elements for {c} channels")
        y = torch.empty_like(z)
        stats = torch.empty((r * groups, 2), dtype=F32, device=z.device)
        with _prof("roi_mosaic_gn_fwd", 0.0, _mosaic_bytes(r, c, pooled, 2)):
            _lib.call("ptmi_roi_mosaic_gn_relu_fwd", _ptr(z), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(stats), r, c, pooled, groups,
                      float(eps), _stream())
        ctx.meta = (r, pooled, groups)
        ctx.save_for_backward(z, y, gamma, stats)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "roi_mosaic_gn_relu", (("y", y),))
        return y

    @staticmethod
    def backward(ctx, dy):
        z, y, gamma, stats = ctx.saved_tensors
        r, pooled, groups = ctx.meta
        dy = _chk(dy.contiguous(), name="roi mosaic group norm grad")
        c = int(z.shape[1])
        dz = torch.empty_like(z)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        if r == 0:
            dgamma.zero_(), dbeta.zero_()
        with _prof("roi_mosaic_gn_bwd", 0.0, _mosaic_bytes(r, c, pooled, 7)):       # dy, y, z twice (dgamma / dbeta, dz), dz once
            _lib.call("ptmi_roi_mosaic_gn_relu_bwd", _ptr(dy), _ptr(y), _ptr(z), _ptr(gamma), _ptr(stats), _ptr(dz), _ptr(dgamma),
                      _ptr(dbeta), r, c, pooled, groups, _ptr(_mosaic_gn_ws(r, c, pooled, groups, z.device)), _stream())
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "roi_mosaic_gn_relu", (("dgamma", dgamma), ("dbeta", dbeta), ("dz", dz)))
        return dz, dgamma, dbeta, None, None, None, None


def roi_mosaic_gn_relu(z, gamma, beta, r: int, pooled: int, groups: int = 32, eps: float = 1e-5):
    """relu(group_norm(.)) of each of the r ROIs on (ceil(r / gx^2), C, S, S) canvases, statistics over the ROI's data pixels; the
    gutters and empty cells of the result (and of the input gradient) are 0.0 whatever z holds there"""
    _no_native_bf16("ops.roi_mosaic_gn_relu")
    return _RoiMosaicGNReLU.apply(z, gamma, beta, int(r), int(pooled), int(groups), float(eps))


_ZERO_BIAS = {}


def zero_bias(n: int, device) -> torch.Tensor:
    """a cached all-zero fp32 vector: the bias operand of a convolution that has none (D2 Conv2d(bias=not norm)); not a parameter"""
    device = torch.device(device)
    key = (int(n), device.type, device.index)
    t = _ZERO_BIAS.get(key)
    if t is None:
        t = _ZERO_BIAS[key] = torch.zeros(int(n), dtype=F32, device=device)
    return t


# ============================================================================ the 3x3 stack: one block node, one conv node
class NCHW:
    """The fp32 (N, C, H, W) storage layout of the 3x3 stack, as _ConvBlock / _Conv / frozen_block see one (p8.P8 is the bf16 one):
    how a layer is checked, packed, launched and reported.  Every method is handed the logical (n, c, h, w) of its operand -- an
    fp32 tensor knows it, a P8 tensor does not."""
    block_op, conv_op = "vgg_block", "conv3x3"          # anomaly op names.  ("bf16_emulate" rounding is the nodes' own: _rnd)
    pack = staticmethod(conv3x3_pack)
    relu_bwd = staticmethod(relu_bwd)

    @staticmethod
    def chk(t, n, c, h, w, name):
        return _chk(t.contiguous(), name=name)

    @staticmethod
    def scan_shape(n, c, h, w):
        return None

    @staticmethod
    def conv(x, wp, bias, mask_ref, n, cin, cout, h, w, epilogue, frame=None, frame_key=None):
        return conv3x3_raw(x, wp, bias, mask_ref, cout, epilogue, frame, frame_key)

    @staticmethod
    def wgrad(x, dz, n, cin, cout, h, w):
        return conv3x3_wgrad(x, dz, cout)

    @staticmethod
    def pool_fwd(x, n, c, h, w, frame=None):
        return _maxpool2x2_fwd(x, frame)

    @staticmethod
    def pool_bwd(y, dout, n, c, h, w):
        return _maxpool2x2_bwd(y, dout, True)

    @staticmethod
    def frozen_conv(x, n, cin, h, w, weight, bias, pooled: bool, frame, scope: str):
        """the public entry points: the _Conv node (x may ask for a gradient; scans under `scope`) or the one launch of epilogue 4"""
        if pooled:
            return conv3x3_relu_pool_nograd(x, weight, bias, frame)
        with anomaly_scope(scope):
            return conv3x3(x, weight, bias, True, frame)

    @staticmethod
    def frozen_pool(x, n, c, h, w, frame=None):
        return maxpool2x2(x, frame)        # (the autograd node: frozen_block may run with grad mode on)


_WB = 8     # _ConvBlock / _Conv arguments: (x, layout, n, cin, h, w, pool or relu, frame), then the weights and biases


class _Conv(torch.autograd.Function):
    """conv3x3 s1 p1 + bias (+ ReLU) in the storage layout L.  Replaces Conv2d + F.relu_ (vgg.py:45-53,66-69)."""

    @staticmethod
    def forward(ctx, x, L, n, cin, h, w, relu, frame, weight, bias):
        frame_key = _frame_key(frame, weight, bias)
        x = L.chk(_rnd(x), n, cin, h, w, "conv input")
        weight = _chk(_rnd(weight).contiguous(), name="conv weight")
        bias = _chk(bias.contiguous(), name="conv bias")
        cout, epilogue = weight.shape[0], 1 if relu else 0
        y = _rnd(L.conv(x, L.pack(weight, 0, epilogue, (h, w)), bias, None, n, cin, cout, h, w, epilogue, frame, frame_key))
        ctx.meta = (L, n, cin, h, w, relu)
        ctx.save_for_backward(x, weight, y if relu else None)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, L.conv_op, (("y", y, None, L.scan_shape(n, cout, h, w)),))
        return y

    @staticmethod
    def backward(ctx, dy):
        L, n, cin, h, w, relu = ctx.meta
        x, weight, y = ctx.saved_tensors
        cout = weight.shape[0]
        dy = L.chk(dy.contiguous(), n, cout, h, w, "conv grad")
        dz = _rnd(L.relu_bwd(dy, y) if relu else dy)
        dx = dw = db = None
        if ctx.needs_input_grad[_WB] or ctx.needs_input_grad[_WB + 1]:
            dw, db = L.wgrad(x, dz, n, cin, cout, h, w)
        if ctx.needs_input_grad[0]:
            dx = _rnd(L.conv(dz, L.pack(weight, 1, 2, (h, w)), None, None, n, cout, cin, h, w, 2))
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, L.conv_op, (("dw", dw), ("db", db), ("dx", dx, None, L.scan_shape(n, cin, h, w))))
        return (dx,) + (None,) * (_WB - 1) + (dw, db)


def conv3x3(x, weight, bias, relu: bool = True, frame: Optional[FrameState] = None):
    """frame: the batch's FrameState at this layer's input (advanced to its output; dropped on paths that do not serve it)"""
    if _native_bf16():
        from . import p8
        _frame_end(frame)
        return p8.conv3x3_nchw(_chk(x.contiguous(), name="conv input"), weight, bias, relu)
    return _Conv.apply(x, NCHW, *x.shape, relu, frame, weight, bias)


class _ConvBlock(torch.autograd.Function):
    """One VGG block = k x [conv3x3 + bias + ReLU] (+ MaxPool 2x2) in the storage layout L as a single autograd node
    (vgg.py:65-72).

    The backward chain is fused: max-pool backward also applies the last ReLU's mask, and every dgrad launch
    applies the mask of the producing layer's ReLU in its epilogue (epilogue 3), so no separate ReLU-backward
    passes (read dy + read y + write dz per layer) remain inside a block; one kernel per layer yields dW and db.  (The layout's
    functions are bound once per call.)"""

    @staticmethod
    def forward(ctx, x, L, n, cin, h, w, pool, frame, *wb):
        k, conv, pack, shape = len(wb) // 2, L.conv, L.pack, L.scan_shape
        acts, ws, c = [L.chk(x, n, cin, h, w, "block input")], [], cin
        for j in range(k):
            wt, b = _chk(wb[2 * j].contiguous()), _chk(wb[2 * j + 1].contiguous())
            ws.append(wt)
            acts.append(conv(acts[-1], pack(wt, 0, 1, (h, w)), b, None, n, c, wt.shape[0], h, w, 1, frame,
                             _frame_key(frame, wb[2 * j], wb[2 * j + 1])))
            c = wt.shape[0]
        out = L.pool_fwd(acts[-1], n, c, h, w, frame) if pool else acts[-1]
        ctx.meta = (L, k, pool, n, h, w)
        ctx.save_for_backward(*acts, *ws)
        if _ANOMALY is not None:        # layer granularity: the node covers a whole block
            items = [("y", acts[j], f"conv{j}", shape(n, ws[j - 1].shape[0], h, w)) for j in range(1, k + 1)]
            _anomaly_fwd(ctx, L.block_op, items + ([("pooled", out, None, shape(n, c, h // 2, w // 2))] if pool else []))
        return out

    @staticmethod
    def backward(ctx, dout):
        L, k, pool, n, h, w = ctx.meta
        conv, pack, wgrad, shape = L.conv, L.pack, L.wgrad, L.scan_shape
        saved = ctx.saved_tensors
        acts, ws = saved[: k + 1], saved[k + 1:]
        cout = ws[-1].shape[0]
        dout = dout.contiguous()
        dz = L.pool_bwd(acts[k], dout, n, cout, h, w) if pool else L.relu_bwd(dout, acts[k])
        grads, dx = [None] * (2 * k), None
        seen = None if _ANOMALY is None else [("dz", dz, f"conv{k}", shape(n, cout, h, w))]
        for j in range(k, 0, -1):
            xin, wt = acts[j - 1], ws[j - 1]
            co, ci = wt.shape[0], wt.shape[1]
            if ctx.needs_input_grad[_WB + 2 * (j - 1)] or ctx.needs_input_grad[_WB + 2 * (j - 1) + 1]:
                dw, db = wgrad(xin, dz, n, ci, co, h, w)
                grads[2 * (j - 1)], grads[2 * (j - 1) + 1] = dw, db
                if seen is not None:
                    seen += [("dw", dw, f"conv{j}"), ("db", db, f"conv{j}")]
            if j > 1:
                dz = conv(dz, pack(wt, 1, 3, (h, w)), None, xin, n, co, ci, h, w, 3)       # dgrad + ReLU mask of layer j - 1
                if seen is not None:
                    seen.append(("dz", dz, f"conv{j - 1}", shape(n, ci, h, w)))
            elif ctx.needs_input_grad[0]:
                dx = conv(dz, pack(wt, 1, 2, (h, w)), None, None, n, co, ci, h, w, 2)
                if seen is not None:
                    seen.append(("dx", dx, "conv1", shape(n, ci, h, w)))
        if seen is not None:
            _anomaly_bwd(ctx, L.block_op, seen)
        return (dx,) + (None,) * (_WB - 1) + tuple(grads)


def vgg_block(x, pool: bool, params, frame: Optional[FrameState] = None):
    """params = [w1, b1, w2, b2, ...].  frame: as conv3x3."""
    if _native_bf16():
        from . import p8
        _frame_end(frame)
        return p8.vgg_block_nchw(_chk(x.contiguous(), name="block input"), pool, params)
    if _OPERAND_ROUNDING == "bf16_emulate":    # layer by layer: every conv rounds its own operands
        _frame_end(frame)
        for j in range(len(params) // 2):
            x = conv3x3(x, params[2 * j], params[2 * j + 1], True)
        return maxpool2x2(x) if pool else x
    return _ConvBlock.apply(x, NCHW, *x.shape, pool, frame, *params)


def frozen_block(L, x, n, cin, h, w, pool: bool, params, frame: Optional[FrameState] = None):
    """The block layer by layer, for a block whose parameters have no backward pass: conv + bias + ReLU per layer, then the pool.
    With grad mode off the last convolution pools in its epilogue (4): the full-resolution activation is not needed.  What a
    layer is differs by layout: NCHW the public entry points, which scan under the scope "conv{j}"; P8 raw launches."""
    k, fuse_pool, layer = len(params) // 2, pool and not torch.is_grad_enabled(), L.frozen_conv
    for j in range(k):
        x = layer(x, n, cin, h, w, params[2 * j], params[2 * j + 1], fuse_pool and j == k - 1, frame, f"conv{j + 1}")
        cin = params[2 * j].shape[0]
    return L.frozen_pool(x, n, cin, h, w, frame) if pool and not fuse_pool else x


# ============================================================================ GEMM family
def gemm(a, b, m, n, k, lda, ldb, ta, tb, bias=None, bias_mode=0, relu=False, out=None, accumulate=False,
         batch=1, stride_a=0, stride_b=0, stride_c=0, ldc=None):
    """C = op(A) op(B) (+bias)(relu); see ptmi_gemm_f32."""
    if out is None:
        shape = (m, n) if batch == 1 else (batch, m, n)
        out = torch.empty(shape, dtype=F32, device=a.device)
    ldc = n if ldc is None else ldc
    if m == 0 or n == 0:
        return out
    nws = _lib.load().ptmi_gemm_ws_floats(m, n, k, batch)                   # > 0: this shape runs split-K
    ws = _ws("gemm", nws * 4, a.device) if nws else None
    with _prof("gemm_f32", 2.0 * m * n * k * batch):
        _lib.call("ptmi_gemm_bf16" if _native_bf16() else "ptmi_gemm_f32", _ptr(a), _ptr(b), _ptr(out), _ptr(bias), m, n, k, lda, ldb, ldc, ta, tb, bias_mode,
                  int(relu), int(accumulate), batch, stride_a, stride_b, stride_c, _ptr(ws), int(nws), _stream())
    return out


def colsum(a: torch.Tensor) -> torch.Tensor:
    rows, cols = a.shape
    out = torch.empty(cols, dtype=F32, device=a.device)
    if rows == 0:
        return out.zero_()
    nws = _lib.load().ptmi_colsum_ws_floats(rows, cols)                     # > 0: tall matrix, summed by row ranges
    ws = _ws("colsum", nws * 4, a.device) if nws else None
    _lib.call("ptmi_colsum_ws", _ptr(a), _ptr(out), _ptr(ws), rows, cols, 0, _stream())
    return out


class _Linear(torch.autograd.Function):
    """y = x W^T + b (+ReLU).  Replaces nn.Linear/F.relu of FastRCNNConvFCHead + predictors."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu: bool):
        x = _chk(_rnd(x).contiguous(), name="linear input")
        weight = _chk(_rnd(weight).contiguous())
        bias = _chk(bias.contiguous())
        r, k = x.shape
        nout = weight.shape[0]
        y = gemm(x, weight, r, nout, k, k, k, 0, 1, bias=bias, bias_mode=2, relu=relu)
        ctx.relu = relu
        ctx.save_for_backward(x, weight, y if relu else None)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "linear", (("y", y),))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = _chk(dy.contiguous())
        dz = _rnd_grad(relu_bwd(dy, y) if ctx.relu else dy)
        r, k = x.shape
        nout = weight.shape[0]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = gemm(dz, weight, r, k, nout, nout, k, 0, 0)                  # (r,nout) x (nout,k)
        if ctx.needs_input_grad[1]:
            if r == 0:
                dw = torch.zeros_like(weight)
            else:
                dw = gemm(dz, x, nout, k, r, nout, k, 1, 0)                   # dz^T (nout,r) x x (r,k)
        if ctx.needs_input_grad[2]:
            db = colsum(dz)
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "linear", (("dx", dx), ("dw", dw), ("db", db)))
        return dx, dw, db, None


def linear(x, weight, bias, relu: bool = False):
    if _native_bf16() and x.shape[0] > 0:
        from . import p8
        if weight.shape[1] >= p8.LINEAR_MIN_K:          # fc1 (25088 -> 1024): bf16-storage GEMMs
            return p8.linear(x, weight, bias, relu)
    return _Linear.apply(x, weight, bias, relu)


class _Conv1x1(torch.autograd.Function):
    """1x1 conv as a batched GEMM over images (D2 StandardRPNHead objectness / anchor-delta convs)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _chk(_rnd(x).contiguous())
        n, ci, h, w = x.shape
        co = weight.shape[0]
        w2 = _chk(_rnd(weight).reshape(co, ci).contiguous())
        hw = h * w
        y = torch.empty((n, co, h, w), dtype=F32, device=x.device)
        gemm(w2, x, co, hw, ci, ci, hw, 0, 0, bias=_chk(bias.contiguous()), bias_mode=1, out=y, batch=n, stride_a=0,
             stride_b=ci * hw, stride_c=co * hw, ldc=hw)
        ctx.save_for_backward(x, w2)
        ctx.wshape = weight.shape
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "conv1x1", (("y", y),))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        dy = _chk(_rnd_grad(dy).contiguous())
        n, ci, h, w = x.shape
        co, hw = w2.shape[0], h * w
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(w2, dy, ci, hw, co, ci, hw, 1, 0, out=dx, batch=n, stride_a=0, stride_b=co * hw, stride_c=ci * hw,
                 ldc=hw)
        if ctx.needs_input_grad[1]:
            # per-image partials in ONE batched launch, then a fixed-order sum over images
            part = gemm(dy, x, co, ci, hw, hw, hw, 0, 1, batch=n, stride_a=co * hw, stride_b=ci * hw,
                        stride_c=co * ci)
            dw = colsum(part.view(n, co * ci)).view(ctx.wshape)
        if ctx.needs_input_grad[2]:
            db = torch.empty(co, dtype=F32, device=x.device)
            _lib.call("ptmi_rowsum_batched", _ptr(dy), _ptr(db), n, co, hw, 0, _stream())
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "conv1x1", (("dx", dx), ("dw", dw), ("db", db)))
        return dx, dw, db


class _RPNHead1x1(torch.autograd.Function):
    """The two 1x1 convolutions of the RPN head (D2 StandardRPNHead: objectness 512 -> A, anchor deltas 512 -> 8A) WRITING
    THE LAYOUTS THE RPN CONSUMES: the reference permutes (N, A, H, W) -> (N, HWA) and (N, 8A, H, W) -> (N, HWA, 8)
    (rpn.py:97-113) with anchor index (y w + x) A + a -- i.e. the transposed GEMM.  Here each image's output is computed as
    X^T (HW x 512) . W^T (512 x A | 8A) with the bias per column, so the GEMM's row-major C IS that layout: no permute
    copies in forward, none of their transposes in backward."""

    @staticmethod
    def forward(ctx, x, w_obj, b_obj, w_del, b_del):
        x = _chk(_rnd(x).contiguous())
        n, ci, h, w = x.shape
        hw = h * w
        outs, w2s = [], []
        for wt, b in ((w_obj, b_obj), (w_del, b_del)):
            co = wt.shape[0]
            w2 = _chk(_rnd(wt).reshape(co, ci).contiguous())
            y = torch.empty((n, hw, co), dtype=F32, device=x.device)
            # A = x[n] stored (K = ci, M = hw): ta = 1;  B = W stored (N = co, K = ci): tb = 1;  C (hw, co)
            gemm(x, w2, hw, co, ci, hw, ci, 1, 1, bias=_chk(b.contiguous()), bias_mode=2, out=y, batch=n, stride_a=ci * hw,
                 stride_b=0, stride_c=hw * co, ldc=co)
            outs.append(y)
            w2s.append(w2)
        ctx.save_for_backward(x, *w2s)
        ctx.shapes = (w_obj.shape, w_del.shape)
        a = w_obj.shape[0]
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "rpn_head_1x1", (("logits", outs[0], "objectness_logits"), ("deltas", outs[1], "anchor_deltas")))
        return outs[0].view(n, hw * a), outs[1].view(n, hw * a, 8)

    @staticmethod
    def backward(ctx, g_obj, g_del):
        x, w_o, w_d = ctx.saved_tensors
        n, ci, h, w = x.shape
        hw = h * w
        dx = None
        grads = []
        first = True
        for g, w2, shape in ((g_obj, w_o, ctx.shapes[0]), (g_del, w_d, ctx.shapes[1])):
            co = w2.shape[0]
            dy = _chk(_rnd_grad(g.reshape(n, hw, co)).contiguous())
            if ctx.needs_input_grad[0]:
                if dx is None:
                    dx = torch.empty_like(x)
                # dX (ci, hw) = W^T (ci, co) . dY^T (co, hw):  A = W stored (K = co, M = ci): ta = 1;  B = dY stored (N = hw, K = co): tb = 1
                gemm(w2, dy, ci, hw, co, ci, co, 1, 1, out=dx, accumulate=not first, batch=n, stride_a=0, stride_b=hw * co,
                     stride_c=ci * hw, ldc=hw)
                first = False
            # dW (co, ci) = dY^T (co, hw) . X^T (hw, ci) per image, then a fixed-order sum over the images
            part = gemm(dy, x, co, ci, hw, co, hw, 1, 1, batch=n, stride_a=hw * co, stride_b=ci * hw, stride_c=co * ci)
            grads.append(colsum(part.view(n, co * ci)).view(shape))
            grads.append(colsum(dy.view(n * hw, co)))
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "rpn_head_1x1", (("dw", grads[0], "objectness_logits"), ("db", grads[1], "objectness_logits"),
                                               ("dw", grads[2], "anchor_deltas"), ("db", grads[3], "anchor_deltas"), ("dx", dx)))
        return dx, grads[0], grads[1], grads[2], grads[3]


def rpn_head_1x1(x, w_obj, b_obj, w_del, b_del):
    """-> (objectness logits (N, H W A), anchor deltas (N, H W A, 8)) in the RPN's anchor order"""
    return _RPNHead1x1.apply(x, w_obj, b_obj, w_del, b_del)


def conv1x1(x, weight, bias):
    return _Conv1x1.apply(x, weight, bias)


# ============================================================================ ROIAlign
def _roi_variant(aligned, sampling_ratio) -> Tuple[int, int]:
    aligned, sampling_ratio = int(bool(aligned)), int(sampling_ratio)
    if sampling_ratio < 0:
        raise ValueError(f"roi_align: sampling_ratio must be >= 0, got {sampling_ratio}")
    return aligned, sampling_ratio


class _ROIAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rois, pooled: int, scale: float, img_offsets, aligned: int = 1, sampling_ratio: int = 0):
        feat = _chk(feat.contiguous())
        rois = _chk(rois.contiguous())
        n, c, h, w = feat.shape
        r = rois.shape[0]
        out = torch.empty((r, c, pooled, pooled), dtype=F32, device=feat.device)
        # (aligned, sampling_ratio) = (1, 0), ROIAlignV2 with the adaptive grid, keeps its own entry points and kernels
        sfx, var = ("", ()) if (aligned, sampling_ratio) == (1, 0) else ("_ex", (aligned, sampling_ratio))
        with _prof("roi_align_fwd"):
            if img_offsets is not None:
                ws = torch.empty(_lib.load().ptmi_roi_align_ws_bytes(r, h, w), dtype=torch.uint8, device=feat.device)
                _lib.call("ptmi_roi_align_fwd_grouped" + sfx, _ptr(feat), _ptr(rois), _ptr(_chk(img_offsets, torch.int32)),
                          _ptr(out), _ptr(ws), n, c, h, w, r, pooled, float(scale), _stream(), *var)
            else:
                _lib.call("ptmi_roi_align_fwd" + sfx, _ptr(feat), _ptr(rois), _ptr(out), n, c, h, w, r, pooled, float(scale),
                          _stream(), *var)
        ctx.save_for_backward(rois, img_offsets)
        ctx.meta = (n, c, h, w, pooled, float(scale), aligned, sampling_ratio)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "roi_align", (("out", out),))
        return out

    @staticmethod
    def backward(ctx, dout):
        rois, img_offsets = ctx.saved_tensors
        n, c, h, w, pooled, scale, aligned, sampling_ratio = ctx.meta
        dout = _chk(dout.contiguous())
        if _DETERMINISTIC:
            dfeat = roi_align_bwd_det(dout, rois, img_offsets, n, c, h, w, pooled, scale, aligned, sampling_ratio)
        elif img_offsets is not None:
            # rois grouped by image: LDS-accumulating kernel, no global atomics, writes every element of dfeat
            dfeat = roi_align_bwd_grouped(dout, rois, img_offsets, n, c, h, w, pooled, scale, aligned, sampling_ratio)
        else:
            dfeat = torch.zeros((n, c, h, w), dtype=F32, device=dout.device)
            sfx, var = ("", ()) if (aligned, sampling_ratio) == (1, 0) else ("_ex", (aligned, sampling_ratio))
            with _prof("roi_align_bwd"):
                _lib.call("ptmi_roi_align_bwd" + sfx, _ptr(dout), _ptr(rois), _ptr(dfeat), n, c, h, w, rois.shape[0], pooled,
                          scale, _stream(), *var)
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "roi_align", (("dfeat", dfeat),))
        return dfeat, None, None, None, None, None, None


def _group_by_image(rois: torch.Tensor, n: int):
    """(row order, img_offsets) that group the rows of rois by image index, rows of one image in their given order (a stable sort:
    a function of rois alone); rows naming no image fall outside every group.  No host sync."""
    img = rois[:, 0].to(torch.int32)
    img_sorted, order = torch.sort(img, stable=True)
    offsets = torch.searchsorted(img_sorted, torch.arange(n + 1, dtype=torch.int32, device=rois.device)).to(torch.int32)
    return order, offsets


def roi_align_bwd_det(dout: torch.Tensor, rois: torch.Tensor, img_offsets: Optional[torch.Tensor], n: int, c: int, h: int, w: int,
                      pooled: int, scale: float, aligned=True, sampling_ratio: int = 0) -> torch.Tensor:
    """roi_align_bwd_grouped through ptmi_roi_align_bwd_det: the atomic-free kernel or an error, never the atomic scatter.  Rows
    not grouped by image (img_offsets None) are grouped here first."""
    aligned, sampling_ratio = _roi_variant(aligned, sampling_ratio)
    dout = _chk(dout.contiguous())
    rois = _chk(rois.contiguous())
    if img_offsets is None:
        order, img_offsets = _group_by_image(rois, n)
        rois, dout = rois[order].contiguous(), dout[order].contiguous()
    dfeat = torch.empty((n, c, h, w), dtype=F32, device=dout.device)
    with _prof("roi_align_bwd"):
        ws = torch.empty(_lib.load().ptmi_roi_align_bwd_ws_bytes(rois.shape[0], h, w), dtype=torch.uint8, device=dout.device)
        _lib.call("ptmi_roi_align_bwd_det", _ptr(dout), _ptr(rois), _ptr(_chk(img_offsets, torch.int32)), _ptr(dfeat), _ptr(ws),
                  n, c, h, w, rois.shape[0], pooled, float(scale), _stream(), aligned, sampling_ratio)
    return dfeat


def roi_pool_bwd_det(dout: torch.Tensor, argmax: torch.Tensor, rois: torch.Tensor, img_offsets: Optional[torch.Tensor], n: int,
                     c: int, h: int, w: int, pooled: int) -> torch.Tensor:
    """ROIPool's feature-map gradient with a fixed summation order (ptmi_roi_pool_bwd_det)"""
    dout = _chk(dout.contiguous())
    argmax = _chk(argmax.contiguous(), torch.int32)
    if img_offsets is None:
        order, img_offsets = _group_by_image(_chk(rois.contiguous()), n)
        dout, argmax = dout[order].contiguous(), argmax[order].contiguous()
    dfeat = torch.empty((n, c, h, w), dtype=F32, device=dout.device)
    with _prof("roi_pool_bwd"):
        _lib.call("ptmi_roi_pool_bwd_det", _ptr(dout), _ptr(argmax), _ptr(_chk(img_offsets, torch.int32)), _ptr(dfeat), n, c, h, w,
                  dout.shape[0], pooled, _stream())
    return dfeat


def roi_align_bwd_grouped(dout: torch.Tensor, rois: torch.Tensor, img_offsets: torch.Tensor, n: int, c: int, h: int, w: int,
                          pooled: int, scale: float, aligned=True, sampling_ratio: int = 0) -> torch.Tensor:
    """d(feature map) (n, c, h, w) from the gradient of ROIAlign's output (R, c * pooled * pooled) for rois grouped by image"""
    if _DETERMINISTIC:
        return roi_align_bwd_det(dout, rois, img_offsets, n, c, h, w, pooled, scale, aligned, sampling_ratio)
    aligned, sampling_ratio = _roi_variant(aligned, sampling_ratio)
    dout = _chk(dout.contiguous())
    dfeat = torch.empty((n, c, h, w), dtype=F32, device=dout.device)
    sfx, var = ("", ()) if (aligned, sampling_ratio) == (1, 0) else ("_ex", (aligned, sampling_ratio))
    with _prof("roi_align_bwd"):
        ws = torch.empty(_lib.load().ptmi_roi_align_bwd_ws_bytes(rois.shape[0], h, w), dtype=torch.uint8, device=dout.device)
        _lib.call("ptmi_roi_align_bwd_grouped" + sfx, _ptr(dout), _ptr(rois), _ptr(_chk(img_offsets, torch.int32)), _ptr(dfeat),
                  _ptr(ws), n, c, h, w, rois.shape[0], pooled, scale, _stream(), *var)
    return dfeat


def roi_align_p8m_fits(c: int, h: int, w: int, pooled: int) -> bool:
    return bool(_lib.load().ptmi_roi_align_fwd_p8m_fits(int(c), int(h), int(w), int(pooled)))


def roi_align_p8m(feat: torch.Tensor, rois: torch.Tensor, img_offsets: torch.Tensor, pooled: int, scale: float, need_xt: bool):
    """ROIAlign (rois grouped by image) straight into the bf16 "P8 matrix" operands of the box head's first Linear layer:
    xk (c * pooled^2 / 8, R, 8) and, if need_xt, xt (ceil(R / 8), c * pooled^2, 8)  (ptmi_roi_align_fwd_p8m)"""
    feat = _chk(feat.contiguous())
    rois = _chk(rois.contiguous())
    n, c, h, w = feat.shape
    r, kd = rois.shape[0], c * pooled * pooled
    xk = torch.empty((kd // 8, r, 8), dtype=torch.bfloat16, device=feat.device)
    xt = torch.empty((-(-r // 8), kd, 8), dtype=torch.bfloat16, device=feat.device) if need_xt else None
    if r:
        with _prof("roi_align_fwd"):
            ws = torch.empty(_lib.load().ptmi_roi_align_ws_bytes(r, h, w), dtype=torch.uint8, device=feat.device)
            _lib.call("ptmi_roi_align_fwd_p8m", _ptr(feat), _ptr(rois), _ptr(_chk(img_offsets, torch.int32)), _ptr(xk), _ptr(xt), _ptr(ws),
                      n, c, h, w, r, pooled, float(scale), _stream())
    return xk, xt


def roi_align(feat, rois, pooled: int, scale: float, img_offsets=None, aligned=True, sampling_ratio: int = 0):
    """rois (R,5) = [image index, x1, y1, x2, y2].  If the rows are grouped by image, pass `img_offsets`
    (int32 (N+1,) device tensor of row offsets) to enable the atomic-free backward.
    `aligned` / `sampling_ratio`: torchvision roi_align's (detectron2 "ROIAlignV2" = aligned, "ROIAlign" = not aligned;
    sampling_ratio 0 = ceil(roi extent / pooled) samples a bin side)."""
    aligned, sampling_ratio = _roi_variant(aligned, sampling_ratio)
    return _ROIAlign.apply(feat, rois, pooled, scale, img_offsets, aligned, sampling_ratio)


# ============================================================================ ROIPool
class _ROIPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, rois, pooled: int, scale: float, img_offsets=None):
        feat = _chk(feat.contiguous())
        rois = _chk(rois.contiguous())
        n, c, h, w = feat.shape
        r = rois.shape[0]
        ctx.img_offsets = img_offsets
        out = torch.empty((r, c, pooled, pooled), dtype=F32, device=feat.device)
        argmax = torch.empty((r, c, pooled, pooled), dtype=torch.int32, device=feat.device)
        with _prof("roi_pool_fwd"):
            _lib.call("ptmi_roi_pool_fwd", _ptr(feat), _ptr(rois), _ptr(out), _ptr(argmax), n, c, h, w, r, pooled, float(scale),
                      _stream())
        ctx.save_for_backward(rois, argmax)
        ctx.meta = (n, c, h, w, pooled)
        ctx.mark_non_differentiable(argmax)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "roi_pool", (("out", out),))
        return out, argmax

    @staticmethod
    def backward(ctx, dout, _dargmax):
        rois, argmax = ctx.saved_tensors
        n, c, h, w, pooled = ctx.meta
        dout = _chk(dout.contiguous())
        if _DETERMINISTIC:
            dfeat = roi_pool_bwd_det(dout, argmax, rois, ctx.img_offsets, n, c, h, w, pooled)
            if _ANOMALY is not None:
                _anomaly_bwd(ctx, "roi_pool", (("dfeat", dfeat),))
            return dfeat, None, None, None, None
        dfeat = torch.empty((n, c, h, w), dtype=F32, device=dout.device)        # (zeroed by the entry point)
        with _prof("roi_pool_bwd"):
            _lib.call("ptmi_roi_pool_bwd", _ptr(dout), _ptr(argmax), _ptr(rois), _ptr(dfeat), n, c, h, w, rois.shape[0], pooled,
                      _stream())
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "roi_pool", (("dfeat", dfeat),))
        return dfeat, None, None, None, None


def roi_pool(feat, rois, pooled: int, scale: float, return_argmax: bool = False, img_offsets=None):
    """torchvision roi_pool: the maximum over each bin's integer cells; rois (R,5) = [image index, x1, y1, x2, y2].  The int32
    argmax (flat h * W + w of the first maximum in raster order, -1 for an empty bin) is saved for the backward (an atomic
    scatter: the feature-map gradient's summation order varies run to run; under ops.deterministic the owner-computes kernel,
    which takes `img_offsets` if the rows are grouped by image and groups them itself otherwise) and returned on request."""
    out, argmax = _ROIPool.apply(feat, rois, pooled, scale, img_offsets)
    return (out, argmax) if return_argmax else out


# ============================================================================ boxes
def grid_anchors(cell: torch.Tensor, h: int, w: int, stride: float, offset: float) -> torch.Tensor:
    cell = _chk(cell.contiguous())
    a = cell.shape[0]
    out = torch.empty((h * w * a, 4), dtype=F32, device=cell.device)
    _lib.call("ptmi_grid_anchors", _ptr(cell), _ptr(out), h, w, a, float(stride), float(offset), _stream())
    return out


def apply_deltas(deltas: torch.Tensor, boxes: torch.Tensor, weights: Sequence[float], scale_clamp: float,
                 k: Optional[int] = None, dstride: Optional[int] = None) -> torch.Tensor:
    """deltas (rows, >=4k) [row stride dstride], boxes (nb,4) cycled over rows -> (rows, 4k)."""
    _chk(deltas)
    boxes = _chk(boxes.contiguous())
    rows = deltas.shape[0]
    dstride = deltas.shape[1] if dstride is None else dstride
    k = deltas.shape[1] // 4 if k is None else k
    out = torch.empty((rows, 4 * k), dtype=F32, device=deltas.device)
    wx, wy, ww, wh = [float(v) for v in weights]
    if rows:
        _lib.call("ptmi_apply_deltas", _ptr(deltas), _ptr(boxes), _ptr(out), rows, k, dstride, boxes.shape[0], wx, wy,
                  ww, wh, float(scale_clamp), _stream())
    return out


class _GetDeltas(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, tgt, wx, wy, ww, wh):
        src = _chk(src.contiguous())
        tgt = _chk(tgt.contiguous())
        out = torch.empty_like(src)
        if src.shape[0]:
            _lib.call("ptmi_get_deltas", _ptr(src), _ptr(tgt), _ptr(out), src.shape[0], wx, wy, ww, wh, _stream())
        ctx.save_for_backward(src, tgt)
        ctx.w = (wx, wy, ww, wh)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "get_deltas", (("deltas", out),))
        return out

    @staticmethod
    def backward(ctx, dd):
        src, tgt = ctx.saved_tensors
        dsrc = None
        if ctx.needs_input_grad[0]:
            rows = src.shape[0]
            if _DETERMINISTIC:          # row i is its own destination: the identity form of the fixed-order entry
                dsrc = get_deltas_bwd_src_det(src, tgt, dd, None, rows, ctx.w)
                if _ANOMALY is not None:
                    _anomaly_bwd(ctx, "get_deltas", (("dsrc", dsrc),))
                return dsrc, None, None, None, None, None
            dsrc = torch.zeros_like(src)
            if rows:
                idx = torch.arange(rows, dtype=torch.int64, device=src.device)
                _lib.call("ptmi_get_deltas_bwd_src", _ptr(src), _ptr(tgt), _ptr(_chk(dd.contiguous())), _ptr(idx), rows,
                          *ctx.w, _ptr(dsrc), _stream())
            if _ANOMALY is not None:
                _anomaly_bwd(ctx, "get_deltas", (("dsrc", dsrc),))
        return dsrc, None, None, None, None, None


def get_deltas_bwd_src(src, tgt, ddeltas, src_index: torch.Tensor, n_dst: int, weights: Sequence[float]) -> torch.Tensor:
    """d(loss)/d(source boxes) of get_deltas summed into (n_dst, 4) by src_index (int64, one destination per row).  Default: the
    atomic scatter (ptmi_get_deltas_bwd_src); under ops.deterministic the fixed-order segmented reduction."""
    if _DETERMINISTIC:
        return get_deltas_bwd_src_det(src, tgt, ddeltas, src_index, n_dst, weights)
    src, tgt, ddeltas = _chk(src.contiguous()), _chk(tgt.contiguous()), _chk(ddeltas.contiguous())
    dsrc = torch.zeros((n_dst, 4), dtype=F32, device=src.device)
    if src.shape[0]:
        _lib.call("ptmi_get_deltas_bwd_src", _ptr(src), _ptr(tgt), _ptr(ddeltas), _ptr(_chk(src_index.contiguous(), torch.int64)),
                  src.shape[0], *[float(v) for v in weights], _ptr(dsrc), _stream())
    return dsrc


def get_deltas_bwd_src_det(src, tgt, ddeltas, src_index: Optional[torch.Tensor], n_dst: int, weights: Sequence[float]) -> torch.Tensor:
    """ptmi_get_deltas_bwd_src_det: src_index None = the identity (n_dst == rows)"""
    src, tgt, ddeltas = _chk(src.contiguous()), _chk(tgt.contiguous()), _chk(ddeltas.contiguous())
    rows = src.shape[0]
    dsrc = torch.empty((n_dst, 4), dtype=F32, device=src.device)
    ws = None
    if src_index is not None:
        src_index = _chk(src_index.contiguous(), torch.int64)
        ws = _ws("get_deltas_det", 4 * _lib.load().ptmi_get_deltas_bwd_src_det_ws_floats(rows, n_dst), src.device)
    _lib.call("ptmi_get_deltas_bwd_src_det", _ptr(src), _ptr(tgt), _ptr(ddeltas), _ptr(src_index), rows,
              *[float(v) for v in weights], _ptr(dsrc), n_dst, _ptr(ws), _stream())
    return dsrc


def get_deltas(src, tgt, weights: Sequence[float]):
    wx, wy, ww, wh = [float(v) for v in weights]
    return _GetDeltas.apply(src, tgt, wx, wy, ww, wh)


def iou_match(gt: torch.Tensor, boxes: torch.Tensor, thresholds: Sequence[float], labels: Sequence[int],
              allow_low_quality: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pairwise_iou + Matcher fused -> (matched_idx int64, matched_label int8, matched_iou f32)."""
    boxes = _chk(boxes.contiguous())
    gt = _chk(gt.contiguous())
    nb, m = boxes.shape[0], gt.shape[0]
    dev = boxes.device
    midx = torch.empty(nb, dtype=torch.int64, device=dev)
    mlab = torch.empty(nb, dtype=torch.int8, device=dev)
    miou = torch.empty(nb, dtype=F32, device=dev)
    ws = _ws("ioum", max(m, 1) * 4, dev)
    thr = (ctypes.c_float * len(thresholds))(*[float(t) for t in thresholds])
    lab = (ctypes.c_int * len(labels))(*[int(l) for l in labels])
    _lib.call("ptmi_iou_match", _ptr(gt), _ptr(boxes), m, nb, thr, lab, len(thresholds), int(allow_low_quality),
              _ptr(midx), _ptr(mlab), _ptr(miou), _ptr(ws), _stream())
    return midx, mlab, miou


def dev_i32(values, device) -> torch.Tensor:
    """Small host list -> int32 device tensor without a stream synchronisation (pinned staging, async copy)."""
    return torch.tensor(values, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def dev_sizes_hw(image_sizes, device) -> torch.Tensor:
    """Per-image (h, w) -> (N, 2) float32 device tensor (the layout ptmi_rpn_prepare and ptmi_iou_match_batched_bounds take)
    without a stream synchronisation (pinned staging, async copy)."""
    return torch.tensor([[float(h), float(w)] for h, w in image_sizes], dtype=F32).reshape(-1, 2).pin_memory().to(
        device, non_blocking=True)


def check_boundary_thresh(value) -> int:
    """MODEL.RPN.BOUNDARY_THRESH is an integer, as in D2 (Boxes.inside_box(box_size, boundary_threshold: int)); any negative
    value means off."""
    if isinstance(value, bool) or not isinstance(value, int):
        raise TypeError(f"MODEL.RPN.BOUNDARY_THRESH must be an integer (negative = off), got {value!r}")
    return value


def iou_match_batched(gt_all: torch.Tensor, gt_counts: Sequence[int], boxes: torch.Tensor, box_counts, thresholds,
                      labels, allow_low_quality: bool, image_sizes_hw=None, boundary_thresh: int = -1):
    """ptmi_iou_match for a whole batch in one launch per pass.  gt_all: the images' gt boxes concatenated
    (gt_counts[i] rows each).  boxes: concatenated per image (box_counts[i] rows each) or, with box_counts=None, ONE
    box set shared by all images (outputs (N, nb)).  Returns (matched_idx within the image, label int8, iou).
    boundary_thresh >= 0 (MODEL.RPN.BOUNDARY_THRESH, shared box set only): boxes that are not inside their image by that many
    pixels get label -1 (ptmi_iou_match_batched_bounds); image_sizes_hw = the images' (h, w), a host sequence or an (N, 2)
    float32 device tensor.  boundary_thresh < 0: the existing entry, image_sizes_hw is not looked at."""
    boundary_thresh = check_boundary_thresh(boundary_thresh)
    boxes = _chk(boxes.contiguous())
    gt_all = _chk(gt_all.contiguous())
    dev = boxes.device
    n = len(gt_counts)
    goff = [0]
    for c in gt_counts:
        goff.append(goff[-1] + int(c))
    gt_off = dev_i32(goff, dev)
    if box_counts is None:
        nb, box_off, shape = boxes.shape[0], None, (n, boxes.shape[0])
    else:
        boff = [0]
        for c in box_counts:
            boff.append(boff[-1] + int(c))
        nb, box_off, shape = max(box_counts) if len(box_counts) else 0, dev_i32(boff, dev), (boff[-1],)
    midx = torch.empty(shape, dtype=torch.int64, device=dev)
    mlab = torch.empty(shape, dtype=torch.int8, device=dev)
    miou = torch.empty(shape, dtype=F32, device=dev)
    ws = _ws("ioumb", max(goff[-1], 1) * 4, dev)
    thr = (ctypes.c_float * len(thresholds))(*[float(t) for t in thresholds])
    lab = (ctypes.c_int * len(labels))(*[int(l) for l in labels])
    if boundary_thresh >= 0:
        if box_counts is not None or image_sizes_hw is None:
            raise _lib.PtmiError("iou_match_batched: boundary_thresh >= 0 needs one shared box set (box_counts=None) and image_sizes_hw")
        sizes = image_sizes_hw if isinstance(image_sizes_hw, torch.Tensor) else dev_sizes_hw(image_sizes_hw, dev)
        sizes = _chk(sizes.contiguous())
        if tuple(sizes.shape) != (n, 2):
            raise _lib.PtmiError(f"iou_match_batched: image_sizes_hw {tuple(sizes.shape)} for {n} images")
        if midx.numel():
            _lib.call("ptmi_iou_match_batched_bounds", _ptr(gt_all), _ptr(gt_off), _ptr(boxes), None, n, nb, goff[-1], thr,
                      lab, len(thresholds), int(allow_low_quality), _ptr(midx), _ptr(mlab), _ptr(miou), _ptr(ws), _ptr(sizes),
                      float(boundary_thresh), _stream())
    elif midx.numel():
        _lib.call("ptmi_iou_match_batched", _ptr(gt_all), _ptr(gt_off), _ptr(boxes), _ptr(box_off), n, nb, goff[-1], thr,
                  lab, len(thresholds), int(allow_low_quality), _ptr(midx), _ptr(mlab), _ptr(miou), _ptr(ws), _stream())
    return midx, mlab, miou, gt_off, box_off


def sample_by_keys(cls_all: torch.Tensor, keys_all: torch.Tensor, offsets: torch.Tensor, max_count: int,
                   num_samples: int, num_pos_max: int, bg_label: int):
    """D2 subsample_labels for a batch without host syncs (ptmi_sample_by_keys): (fg (N,num_pos_max) int64, bg
    (N,num_samples) int64, counts (N,2) int32); entries beyond the counts are unspecified."""
    cls_all = _chk(cls_all.contiguous(), torch.int64)
    keys_all = _chk(keys_all.contiguous())
    n = offsets.numel() - 1
    dev = cls_all.device
    fg = torch.empty((n, max(num_pos_max, 1)), dtype=torch.int64, device=dev)
    bg = torch.empty((n, num_samples), dtype=torch.int64, device=dev)
    cnt = torch.empty((n, 2), dtype=torch.int32, device=dev)
    _lib.call("ptmi_sample_by_keys", _ptr(cls_all), _ptr(keys_all), _ptr(_chk(offsets, torch.int32)), n, int(max_count),
              num_samples, num_pos_max, bg_label, _ptr(fg), _ptr(bg), _ptr(cnt), _stream())
    return fg, bg, cnt


def rpn_subsample_relabel(labels: torch.Tensor, keys: torch.Tensor, num_samples: int, num_pos_max: int,
                          bg_label: int) -> torch.Tensor:
    """RPN._subsample_labels for a batch (ptmi_rpn_subsample_relabel): labels (N, R) int8, keys (N, R) float32 >= 0 ->
    (N, R) int8 with the sampled positives = 1, sampled negatives = 0, everything else -1."""
    labels = _chk(labels.contiguous(), torch.int8)
    keys = _chk(keys.contiguous())
    assert labels.dim() == 2 and keys.shape == labels.shape
    out = torch.empty_like(labels)
    if labels.numel():
        _lib.call("ptmi_rpn_subsample_relabel", _ptr(labels), _ptr(keys), _ptr(out), labels.shape[0], labels.shape[1],
                  int(num_samples), int(num_pos_max), int(bg_label), _stream())
    return out


# ============================================================================ sort / proposals / NMS
def segsort_desc(keys: torch.Tensor, seg_offsets: torch.Tensor, max_len: Optional[int] = None,
                 topk: Optional[int] = None, lengths: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable descending sort inside each segment.  Returns (sorted keys, index within segment int32).
    max_len: the longest segment, if the caller knows it (no device read here) -- segments of up to 16 384 keys are then sorted
    by the LDS kernel; topk: the caller only reads the first topk entries of every segment (longer segments come back with
    their first topk entries in order and (-inf, 0) behind them).  lengths: the HOST copy of the segment lengths the caller
    built seg_offsets from -- checked here against max_len and the key count (a max_len that does not describe the
    segments makes the LDS kernel emit NaN keys, which only one of the three callers would have noticed; all three now pass
    their host lengths, so the mismatch is a PtmiError before any launch)."""
    keys = _chk(keys.contiguous())
    seg_offsets = _chk(seg_offsets.contiguous(), torch.int32)
    total, nseg = keys.numel(), seg_offsets.numel() - 1
    if lengths is not None:
        longest = max(lengths) if len(lengths) else 0
        if len(lengths) != nseg or sum(lengths) != total or (max_len is not None and longest > max_len):
            raise _lib.PtmiError(f"segsort_desc: segment lengths {list(lengths)[:8]}... (n = {len(lengths)}, sum {sum(lengths)}, longest "
                                 f"{longest}) do not match {nseg} segments / {total} keys / max_len {max_len}")
        max_len = longest if max_len is None else max_len
    out = torch.empty_like(keys)
    idx = torch.empty(total, dtype=torch.int32, device=keys.device)
    if total == 0:
        return out, idx
    lib = _lib.load()
    if max_len is not None and lib.ptmi_segsort_topk_fits(int(max_len), int(topk or 0)):
        with _prof("segsort_desc"):
            _lib.call("ptmi_segsort_topk_desc", _ptr(keys), _ptr(out), _ptr(idx), nseg, _ptr(seg_offsets), int(max_len),
                      int(topk or 0), _stream())
        return out, idx
    nbytes = lib.ptmi_segsort_ws_bytes(total, nseg)
    ws = _ws("sort", nbytes, keys.device)
    with _prof("segsort_desc"):
        _lib.call("ptmi_segsort_desc", _ptr(keys), _ptr(out), _ptr(idx), total, nseg, _ptr(seg_offsets), _ptr(ws),
                  nbytes, _stream())
    return out, idx


def rpn_prepare(decoded, sorted_logits, sorted_idx, sigma_logits, image_sizes_hw, k: int, min_size: float):
    """-> boxes (n,k,4) clipped, keys (n,k) (rescored logit, -inf for dropped entries), counts (n,) int32, nonfinite (n,)"""
    n, r = sorted_logits.shape
    dev = decoded.device
    boxes = torch.empty((n, k, 4), dtype=F32, device=dev)
    keys = torch.empty((n, k), dtype=F32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    nonfinite = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.call("ptmi_rpn_prepare", _ptr(_chk(decoded)), _ptr(_chk(sorted_logits)), _ptr(_chk(sorted_idx, torch.int32)),
              _ptr(_chk(sigma_logits)), _ptr(_chk(image_sizes_hw)), _ptr(boxes), _ptr(keys), _ptr(counts),
              _ptr(nonfinite), n, r, k, float(min_size), _stream())
    return boxes, keys, counts, nonfinite


def nms_batched(boxes_sorted: torch.Tensor, seg_offsets: torch.Tensor, max_count: int, thr: float, max_keep: int,
                seg_counts: Optional[torch.Tensor] = None):
    """boxes (sum,4) sorted by descending score per image; returns keep (nimg,max_keep) int32 positions, counts.
    seg_counts (nimg,) int32: fill level of fixed-capacity segments (device-side, no host read needed)."""
    boxes_sorted = _chk(boxes_sorted.contiguous())
    seg_offsets = _chk(seg_offsets.contiguous(), torch.int32)
    nimg = seg_offsets.numel() - 1
    dev = boxes_sorted.device
    keep = torch.empty((nimg, max_keep), dtype=torch.int32, device=dev)
    cnt = torch.empty(nimg, dtype=torch.int32, device=dev)
    nbytes = _lib.load().ptmi_nms_ws_bytes(max_count, nimg)
    ws = _ws("nms", nbytes, dev)
    with _prof("nms_batched"):
        _lib.call("ptmi_nms_batched", _ptr(boxes_sorted), _ptr(seg_offsets),
                  _ptr(_chk(seg_counts, torch.int32)) if seg_counts is not None else None, nimg, int(max_count),
                  float(thr), max_keep, _ptr(keep), _ptr(cnt), _ptr(ws), _stream())
    return keep, cnt


def roi_infer_prepare(deltas, proposal_boxes, probs, roi_img, image_sizes_hw, k: int, weights, scale_clamp: float,
                      score_thresh: float):
    """fast_rcnn.py:34-101 for all ROIs of a batch (ptmi_roi_infer_prepare): -> boxes (R,K,4) clipped, keys (R,K),
    roi_valid (R,) u8, img_max (nimg,), img_count (nimg,) int32, img_invalid (nimg,) int32."""
    r, nimg = deltas.shape[0], image_sizes_hw.shape[0]
    dev = deltas.device
    boxes = torch.empty((r, k, 4), dtype=F32, device=dev)
    keys = torch.empty((r, k), dtype=F32, device=dev)
    valid = torch.empty(r, dtype=torch.uint8, device=dev)
    img_max = torch.empty(nimg, dtype=F32, device=dev)
    img_cnt = torch.empty(nimg, dtype=torch.int32, device=dev)
    img_inv = torch.empty(nimg, dtype=torch.int32, device=dev)
    wx, wy, ww, wh = [float(v) for v in weights]
    _lib.call("ptmi_roi_infer_prepare", _ptr(_chk(deltas)), _ptr(_chk(proposal_boxes)), _ptr(_chk(probs)),
              _ptr(_chk(roi_img, torch.int32)), _ptr(_chk(image_sizes_hw)), _ptr(boxes), _ptr(keys), _ptr(valid),
              _ptr(img_max), _ptr(img_cnt), _ptr(img_inv), r, k, nimg, wx, wy, ww, wh, float(scale_clamp),
              float(score_thresh), _stream())
    return boxes, keys, valid, img_max, img_cnt, img_inv


def roi_infer_nms_boxes(boxes, order, seg_offsets, img_max, max_count: int, k: int) -> torch.Tensor:
    out = torch.empty((boxes.shape[0] * boxes.shape[1], 4), dtype=F32, device=boxes.device)
    _lib.call("ptmi_roi_infer_nms_boxes", _ptr(_chk(boxes)), _ptr(_chk(order, torch.int32)),
              _ptr(_chk(seg_offsets, torch.int32)), _ptr(_chk(img_max)), seg_offsets.numel() - 1, int(max_count), k,
              _ptr(out), _stream())
    return out


# ---- test-time augmentation (TEST.AUG): map every augmentation's detections back, one merged NMS per image
TTA_SCORE_THRESH = 1e-8          # D2 0.5 GeneralizedRCNNWithTTA._merge_detections


def _tta_tables(aug_rows, aug_counts, image_sizes, d: int):
    """Host side of the per-augmentation table: aug_rows[a] = (image, flipped, w_s, fx_s, fy_s, gx, gy, has pre-transform),
    aug_counts[a] = its detections.  Checks everything a kernel indexes with and returns (offsets, meta, factors, per-image
    segment lengths) as host lists."""
    nimg = len(image_sizes)
    if len(aug_rows) != len(aug_counts) or not aug_rows or nimg == 0:
        raise ValueError(f"tta: {len(aug_rows)} augmentation rows, {len(aug_counts)} counts, {nimg} images")
    offs, meta, fact, lengths, prev = [0], [], [], [0] * nimg, 0
    for row, c in zip(aug_rows, aug_counts):
        img, flip, w_s, fx, fy, gx, gy, pre = row
        img, c = int(img), int(c)
        if not (prev <= img < nimg) or c < 0:
            raise ValueError(f"tta: augmentation rows must be grouped by image in ascending order (image {img} after {prev}, "
                             f"{nimg} images) with non-negative counts (got {c})")
        prev = img
        offs.append(offs[-1] + c)
        lengths[img] += c
        meta.append([img, int(bool(flip)), int(bool(pre))])
        fact.append([float(w_s), float(fx), float(fy), float(gx), float(gy)])
    if offs[-1] != d:
        raise ValueError(f"tta: the augmentations hold {offs[-1]} detections, the arrays {d}")
    return offs, meta, fact, lengths


def tta_map_boxes(boxes: torch.Tensor, scores: torch.Tensor, aug_rows, aug_counts: Sequence[int], image_sizes,
                  score_thresh: float = TTA_SCORE_THRESH):
    """ptmi_tta_map_boxes: boxes (D,4) / scores (D) of all augmentations of a batch, concatenated in augmentation order ->
    mapped + clipped boxes (D,4), keys (D) (score of a candidate, -inf otherwise), img_max (nimg,), img_count (nimg,) int32.
    aug_rows / aug_counts: see _tta_tables; image_sizes: the original (H, W) of every image.  No host read."""
    return _tta_map(boxes, scores, _tta_tables(aug_rows, aug_counts, image_sizes, scores.numel()), image_sizes, score_thresh)


def _tta_map(boxes, scores, tables, image_sizes, score_thresh):
    boxes, scores = _chk(boxes.contiguous()), _chk(scores.contiguous())
    d, nimg, dev = scores.numel(), len(image_sizes), boxes.device
    assert boxes.shape == (d, 4)
    offs, meta, fact, _ = tables
    out = torch.empty((d, 4), dtype=F32, device=dev)
    keys = torch.empty(d, dtype=F32, device=dev)
    img_max = torch.empty(nimg, dtype=F32, device=dev)
    img_cnt = torch.empty(nimg, dtype=torch.int32, device=dev)
    offs_d, meta_d = dev_i32(offs, dev), dev_i32(meta, dev)
    fact_d = torch.tensor(fact, dtype=F32).pin_memory().to(dev, non_blocking=True)
    _lib.call("ptmi_tta_map_boxes", _ptr(boxes), _ptr(scores), _ptr(offs_d), _ptr(meta_d), _ptr(fact_d),
              _ptr(dev_sizes_hw(image_sizes, dev)), _ptr(out), _ptr(keys), _ptr(img_max), _ptr(img_cnt), d, len(meta), nimg,
              float(score_thresh), _stream())
    return out, keys, img_max, img_cnt


def tta_nms_boxes(boxes, classes, order, seg_offsets, img_max, max_count: int) -> torch.Tensor:
    """ptmi_tta_nms_boxes: the mapped boxes in sorted order per image segment + class * (img_max + 1), fp32."""
    out = torch.empty((boxes.shape[0], 4), dtype=F32, device=boxes.device)
    _lib.call("ptmi_tta_nms_boxes", _ptr(_chk(boxes)), _ptr(_chk(classes, torch.int64)), _ptr(_chk(order, torch.int32)),
              _ptr(_chk(seg_offsets, torch.int32)), _ptr(_chk(img_max)), seg_offsets.numel() - 1, int(max_count), _ptr(out),
              _stream())
    return out


def tta_merge(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, aug_rows, aug_counts: Sequence[int],
              image_sizes, nms_thresh: float, max_det: int, score_thresh: float = TTA_SCORE_THRESH):
    """D2 0.5 GeneralizedRCNNWithTTA._inverse_boxes + _merge_detections (plain fast_rcnn_inference_single_image) for all
    images of a batch at once: the detections of every augmentation -- boxes (D,4), scores (D), classes (D) int64 in
    augmented-image coordinates, concatenated in augmentation order, augmentations grouped by image -- are mapped back, filtered,
    sorted per image (ties: position in the concatenation), passed through batched_nms at `nms_thresh`, and the first `max_det`
    kept (negative: all).  Returns one (boxes (k,4), scores (k,), classes (k,)) per image.
    Four entry points whatever the number of augmentations or detections (map, sort, class offsets, NMS) and ONE device->host
    read, the kept counts.  An image with more detections than the single-pass bitmask NMS holds is a ValueError before any
    launch.  (D2's batched_nms leaves the class-offset trick at 40 000 boxes for one NMS per class; this merge keeps the
    offsets at every size -- the same pairs are compared either way.)"""
    from .modeling.roi_heads import NMS_SEGMENT_MAX
    nimg, dev = len(image_sizes), boxes.device
    d = scores.numel()
    tables = _tta_tables(aug_rows, aug_counts, image_sizes, d)
    lengths = tables[3]
    cap = max(lengths)
    if cap > NMS_SEGMENT_MAX:
        raise ValueError(f"TEST.AUG: {cap} detections of one image over all augmentations exceed the {NMS_SEGMENT_MAX} the "
                         "single-pass bitmask NMS holds; lower TEST.DETECTIONS_PER_IMAGE or use fewer TEST.AUG.MIN_SIZES")
    classes = _chk(classes.contiguous(), torch.int64)
    if tuple(boxes.shape) != (d, 4) or classes.numel() != d:
        raise ValueError(f"tta_merge: {d} scores, boxes {tuple(boxes.shape)}, {classes.numel()} classes")
    if d == 0:
        return [(torch.empty((0, 4), dtype=F32, device=dev), torch.empty(0, dtype=F32, device=dev),
                 torch.empty(0, dtype=torch.int64, device=dev)) for _ in range(nimg)]
    mapped, keys, img_max, img_cnt = _tta_map(boxes, scores, tables, image_sizes, score_thresh)
    seg_h = [0]
    for n in lengths:
        seg_h.append(seg_h[-1] + n)
    seg = dev_i32(seg_h, dev)
    srt, order = segsort_desc(keys, seg, max_len=cap, lengths=lengths)
    nms_boxes = tta_nms_boxes(mapped, classes, order, seg, img_max, cap)
    max_keep = min(max_det, cap) if max_det >= 0 else cap
    keep, kcnt = nms_batched(nms_boxes, seg, cap, float(nms_thresh), max(int(max_keep), 1), seg_counts=img_cnt)
    kc = [min(k, max_keep) for k in kcnt.cpu().tolist()]                  # the one sync
    first = seg[:-1].long()
    keep_g = keep.long() + first.unsqueeze(1)                              # position in the sorted concatenation
    out = []
    for i in range(nimg):
        pos = keep_g[i, :kc[i]]
        src = first[i] + order[pos].long()
        out.append((mapped[src], srt[pos], classes[src]))
    return out


def roi_class_seg_offsets(counts: Sequence[int], k: int) -> list:
    """Host list of the nimg * k + 1 offsets of the class-major layout of ROI inference by class (include/ptmi355.h): segment
    img * k + c = the counts[img] entries of class c of image img, starting at k * roff[img] + c * counts[img]."""
    offs, base = [], 0
    for c in counts:
        offs.extend(base + j * int(c) for j in range(k))
        base += k * int(c)
    offs.append(base)
    return offs


def roi_infer_class_keys(keys, cls_seg, nimg: int, k: int, max_r: int):
    """dense keys (R, K) -> class-major keys (K * R,) and the candidate count of every (image, class) segment, int32."""
    out = torch.empty(keys.numel(), dtype=F32, device=keys.device)
    cnt = torch.empty(nimg * k, dtype=torch.int32, device=keys.device)
    _lib.call("ptmi_roi_infer_class_keys", _ptr(_chk(keys)), _ptr(_chk(cls_seg, torch.int32)), nimg, k, int(max_r), _ptr(out),
              _ptr(cnt), _stream())
    return out, cnt


def roi_infer_class_nms_boxes(boxes, order, cls_seg, img_max, img_count, nimg: int, k: int, max_r: int) -> torch.Tensor:
    """the boxes NMS sees, per (image, class) segment in sorted order (class offset below 40 000 candidates per image)"""
    out = torch.empty((boxes.shape[0] * boxes.shape[1], 4), dtype=F32, device=boxes.device)
    _lib.call("ptmi_roi_infer_class_nms_boxes", _ptr(_chk(boxes)), _ptr(_chk(order, torch.int32)),
              _ptr(_chk(cls_seg, torch.int32)), _ptr(_chk(img_max)), _ptr(_chk(img_count, torch.int32)), nimg, k, int(max_r),
              _ptr(out), _stream())
    return out


def roi_infer_class_collect(sorted_keys, order, keep, keep_count, cls_seg, nimg: int, k: int, max_r: int, rows: int):
    """kept entries of every (image, class) segment -> dense keys (rows, K) (-1 where nothing was kept) and the kept count per
    image, int32"""
    dense = torch.empty((rows, k), dtype=F32, device=sorted_keys.device)
    kept = torch.empty(nimg, dtype=torch.int32, device=sorted_keys.device)
    assert keep.dim() == 2 and keep.shape[0] == nimg * k and keep_count.numel() == nimg * k
    _lib.call("ptmi_roi_infer_class_collect", _ptr(_chk(sorted_keys)), _ptr(_chk(order, torch.int32)),
              _ptr(_chk(keep, torch.int32)), _ptr(_chk(keep_count, torch.int32)), _ptr(_chk(cls_seg, torch.int32)), nimg, k,
              int(max_r), keep.shape[1], rows * k, _ptr(dense), _ptr(kept), _stream())
    return dense, kept


# ============================================================================ COCO evaluation (csrc/coco_eval.hip)
COCO_MAX_DETS, COCO_MAX_THRESHOLDS, COCO_MAX_AREA_RANGES = 100, 16, 4


def coco_match_max_gt() -> int:
    """the largest ground-truth segment ptmi_coco_match serves"""
    return int(_lib.load().ptmi_coco_match_max_gt())


def coco_match(dt_xywh, dt_area, dt_off, gt_xywh, gt_area, gt_crowd, gt_off, iou_thr, area_rng, out=None):
    """pycocotools computeIoU + evaluateImg over every (image, category) segment, threshold and area range in one launch
    (ptmi_coco_match, which states the protocol).  dt_xywh (ND,4) / dt_area (ND) float64 in descending-score order per segment,
    gt_xywh (NG,4) / gt_area (NG) float64, gt_crowd (NG) int32, dt_off / gt_off (S+1) int64, iou_thr (T) and area_rng (A,2)
    float64.  Returns gt_ignore (A,NG), dt_match (A,T,ND), dt_ignore (A,T,ND), int32 (`out`: that triple, preallocated).
    The offset tables are read back once to check that they tile the arrays and to size the launch: a segment of more than 100
    detections or coco_match_max_gt() boxes, T > 16 or A > 4 is a ValueError before anything is launched."""
    dev = dt_xywh.device
    dt_xywh, dt_area = _chk(dt_xywh, torch.float64, "dt_xywh"), _chk(dt_area, torch.float64, "dt_area")
    gt_xywh, gt_area = _chk(gt_xywh, torch.float64, "gt_xywh"), _chk(gt_area, torch.float64, "gt_area")
    gt_crowd = _chk(gt_crowd, torch.int32, "gt_crowd")
    iou_thr, area_rng = _chk(iou_thr, torch.float64, "iou_thr"), _chk(area_rng, torch.float64, "area_rng")
    nd, ng, nthr, narea = dt_area.numel(), gt_area.numel(), iou_thr.numel(), area_rng.numel() // 2
    if tuple(dt_xywh.shape) != (nd, 4) or tuple(gt_xywh.shape) != (ng, 4) or gt_crowd.numel() != ng \
            or tuple(area_rng.shape) != (narea, 2) or iou_thr.dim() != 1:
        raise ValueError("coco_match: expected dt_xywh (ND,4), dt_area (ND), gt_xywh (NG,4), gt_area (NG), gt_crowd (NG), "
                         "iou_thr (T), area_rng (A,2)")
    if not 1 <= nthr <= COCO_MAX_THRESHOLDS or not 1 <= narea <= COCO_MAX_AREA_RANGES:
        raise ValueError(f"coco_match: {nthr} IoU thresholds / {narea} area ranges (at most {COCO_MAX_THRESHOLDS} / "
                         f"{COCO_MAX_AREA_RANGES} are served)")
    longest = []
    for name, off, n in (("dt_off", dt_off, nd), ("gt_off", gt_off, ng)):
        if off.dtype != torch.int64 or off.dim() != 1 or off.numel() != dt_off.numel() or off.numel() < 1:
            raise ValueError(f"coco_match: {name} must be int64 (S+1), the same S for both tables")
        host = off.detach().cpu()
        lens = host[1:] - host[:-1]
        if int(host[0]) != 0 or int(host[-1]) != n or (lens.numel() and int(lens.min()) < 0):
            raise ValueError(f"coco_match: {name} does not tile its {n} rows")
        longest.append(int(lens.max()) if lens.numel() else 0)
    max_dt, max_gt = longest
    if max_dt > COCO_MAX_DETS:
        raise ValueError(f"coco_match: a segment holds {max_dt} detections (maxDets[-1] = {COCO_MAX_DETS}: keep the first "
                         f"{COCO_MAX_DETS} by score)")
    if max_gt > coco_match_max_gt():
        raise ValueError(f"coco_match: a segment holds {max_gt} ground-truth boxes (at most {coco_match_max_gt()} are served)")
    dt_off, gt_off = _chk(dt_off.to(dev), torch.int64, "dt_off"), _chk(gt_off.to(dev), torch.int64, "gt_off")
    if out is None:
        out = (torch.empty((narea, ng), dtype=torch.int32, device=dev),
               torch.empty((narea, nthr, nd), dtype=torch.int32, device=dev),
               torch.empty((narea, nthr, nd), dtype=torch.int32, device=dev))
    gt_ignore, dt_match, dt_ignore = out
    if tuple(gt_ignore.shape) != (narea, ng) or tuple(dt_match.shape) != (narea, nthr, nd) \
            or tuple(dt_ignore.shape) != (narea, nthr, nd):
        raise ValueError("coco_match: out = (gt_ignore (A,NG), dt_match (A,T,ND), dt_ignore (A,T,ND))")
    for name, t in (("gt_ignore", gt_ignore), ("dt_match", dt_match), ("dt_ignore", dt_ignore)):
        _chk(t, torch.int32, name)
    with _prof("coco_match"):
        _lib.call("ptmi_coco_match", _ptr(dt_xywh), _ptr(dt_area), _ptr(dt_off), _ptr(gt_xywh), _ptr(gt_area), _ptr(gt_crowd),
                  _ptr(gt_off), dt_off.numel() - 1, nd, ng, max_dt, max_gt, _ptr(iou_thr), nthr, _ptr(area_rng), narea,
                  _ptr(gt_ignore), _ptr(dt_match), _ptr(dt_ignore), _stream())
    return gt_ignore, dt_match, dt_ignore


# ============================================================================ losses (loss + gradient in one launch)
class _BCELogitsSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, inv_norm: float):
        logits = _chk(logits.contiguous())
        labels = _chk(labels.contiguous(), torch.int8)
        loss = torch.empty(1, dtype=F32, device=logits.device)
        dl = torch.empty_like(logits)
        _lib.call("ptmi_bce_logits_sum", _ptr(logits), _ptr(labels), logits.numel(), float(inv_norm), _ptr(loss),
                  _ptr(dl), _ptr(_loss_ws(logits.device)), _stream())
        ctx.save_for_backward(dl)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "bce_logits_sum", (("loss", loss),))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        if _ANOMALY is not None:
            out = dl * g
            _anomaly_bwd(ctx, "bce_logits_sum", (("dlogits", out),))
            return out, None, None
        return dl * g, None, None


def bce_logits_sum(logits, labels_i8, inv_norm):
    return _BCELogitsSum.apply(logits, labels_i8, inv_norm)


def _nll_sum_forward(ctx, entry: str, d, t, inv_norm: float):
    """forward of the box-regression NLL Functions: `entry` = ptmi_gaussian_nll_sum | ptmi_laplace_nll_sum (same arguments)"""
    d = _chk(d.contiguous())
    t = _chk(t.contiguous())
    rows = d.shape[0]
    loss = torch.empty(1, dtype=F32, device=d.device)
    dd = torch.empty_like(d)
    dt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
    _lib.call(entry, _ptr(d), _ptr(t), rows, float(inv_norm), _ptr(loss), _ptr(dd), _ptr(dt),
              _ptr(_loss_ws(d.device)), _stream())
    ctx.has_dt = dt is not None
    ctx.save_for_backward(dd, dt) if dt is not None else ctx.save_for_backward(dd)
    if _ANOMALY is not None:
        _anomaly_fwd(ctx, entry[5:], (("loss", loss),))
    return loss.reshape(())


class _GaussianNLLSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, t, inv_norm: float):
        return _nll_sum_forward(ctx, "ptmi_gaussian_nll_sum", d, t, inv_norm)

    @staticmethod
    def backward(ctx, g):
        if ctx.has_dt:
            dd, dt = ctx.saved_tensors
            out = (dd * g, dt * g, None)
        else:
            (dd,) = ctx.saved_tensors
            out = (dd * g, None, None)
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "nll_sum", (("ddeltas", out[0]), ("dtarget", out[1])))
        return out


def gaussian_nll_sum(d, t, inv_norm):
    return _GaussianNLLSum.apply(d, t, inv_norm)


class _LaplaceNLLSum(_GaussianNLLSum):
    """UNSUPNET.MODEL_TYPE = LAPLACE: -log(laplace_dist_pdf + 1e-9) summed (ptmi_laplace_nll_sum); backward as the Gaussian's"""

    @staticmethod
    def forward(ctx, d, t, inv_norm: float):
        return _nll_sum_forward(ctx, "ptmi_laplace_nll_sum", d, t, inv_norm)


def laplace_nll_sum(d, t, inv_norm):
    return _LaplaceNLLSum.apply(d, t, inv_norm)


class _SoftmaxCEMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        logits = _chk(logits.contiguous())
        target = _chk(target.contiguous(), torch.int64)
        r, c = logits.shape
        loss = torch.empty(1, dtype=F32, device=logits.device)
        dl = torch.empty_like(logits)
        _lib.call("ptmi_softmax_ce_mean", _ptr(logits), _ptr(target), r, c, _ptr(loss), _ptr(dl),
                  _ptr(_loss_ws(logits.device)), _stream())
        ctx.save_for_backward(dl)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "softmax_ce_mean", (("loss", loss),))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        if _ANOMALY is not None:
            out = dl * g
            _anomaly_bwd(ctx, "softmax_ce_mean", (("dlogits", out),))
            return out, None
        return dl * g, None


def softmax_ce_mean(logits, target):
    return _SoftmaxCEMean.apply(logits, target)


def softmax_rows(logits: torch.Tensor) -> torch.Tensor:
    logits = _chk(logits.contiguous())
    out = torch.empty_like(logits)
    _lib.call("ptmi_softmax_rows", _ptr(logits), _ptr(out), logits.shape[0], logits.shape[1], _stream())
    return out


# ---------------------------------------------------------------------------- training statistics (integer counters)
def cls_stats(logits: torch.Tensor, gt_classes: torch.Tensor) -> torch.Tensor:
    """The counts behind fast_rcnn/cls_accuracy, fg_cls_accuracy and false_negative (D2 0.5 _log_classification_stats;
    ptmi_cls_stats): logits (R, K + 1) fp32, gt_classes (R,) int64 -> int32 (4,) on the device = (argmax == gt, 0 <= gt < K,
    foreground and argmax == gt, foreground and argmax == K).  Lowest index among equal maxima; R = 0 gives zeros.  No host read."""
    logits = _chk(logits.detach().contiguous(), name="cls_stats logits")
    gt_classes = _chk(gt_classes.contiguous(), torch.int64, "cls_stats gt_classes")
    assert logits.dim() == 2 and gt_classes.shape == (logits.shape[0],)
    out = torch.empty(4, dtype=torch.int32, device=logits.device)
    _lib.call("ptmi_cls_stats", _ptr(logits), _ptr(gt_classes), logits.shape[0], logits.shape[1], _ptr(out),
              _ptr(_ws("stats", 4096 * 4, logits.device)), _stream())
    return out


def label_counts(labels_i8: torch.Tensor) -> torch.Tensor:
    """The counts behind rpn/num_pos_anchors and rpn/num_neg_anchors (rpn.py:222-228; ptmi_label_counts): int8 labels of any
    shape -> int32 (2,) on the device = (entries == 1, entries == 0).  No host read."""
    labels_i8 = _chk(labels_i8.contiguous(), torch.int8, "label_counts labels")
    out = torch.empty(2, dtype=torch.int32, device=labels_i8.device)
    _lib.call("ptmi_label_counts", _ptr(labels_i8), labels_i8.numel(), _ptr(out), _ptr(_ws("stats", 4096 * 4, labels_i8.device)),
              _stream())
    return out


class _SoftCEEFL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, teacher, student, tau, lam, efl, inv_norm):
        teacher = _chk(teacher.contiguous())
        student = _chk(student.contiguous())
        r, c = student.shape
        loss = torch.empty(1, dtype=F32, device=student.device)
        ds = torch.empty_like(student)
        _lib.call("ptmi_soft_ce_efl", _ptr(teacher), _ptr(student), r, c, float(tau), float(lam), int(efl),
                  float(inv_norm), _ptr(loss), _ptr(ds), _ptr(_loss_ws(student.device)), _stream())
        ctx.save_for_backward(ds)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "soft_ce_efl", (("loss", loss),))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (ds,) = ctx.saved_tensors
        if _ANOMALY is not None:
            out = ds * g
            _anomaly_bwd(ctx, "soft_ce_efl", (("dstudent", out),))
            return None, out, None, None, None, None
        return None, ds * g, None, None, None, None


def soft_ce_efl(teacher, student, tau, lam, efl, inv_norm):
    return _SoftCEEFL.apply(teacher, student, tau, lam, efl, inv_norm)


class _RPNSoftObj(torch.autograd.Function):
    @staticmethod
    def forward(ctx, teacher, x, tau, lam, efl, inv_norm):
        teacher = _chk(teacher.contiguous())
        x = _chk(x.contiguous())
        k, c = teacher.shape
        loss = torch.empty(1, dtype=F32, device=x.device)
        dx = torch.empty_like(x)
        fg = torch.empty(k, dtype=torch.uint8, device=x.device)
        _lib.call("ptmi_rpn_soft_obj_loss", _ptr(teacher), _ptr(x), k, c, float(tau), float(lam), int(efl),
                  float(inv_norm), _ptr(loss), _ptr(dx), _ptr(fg), _ptr(_loss_ws(x.device)), _stream())
        ctx.save_for_backward(dx)
        ctx.mark_non_differentiable(fg)
        if _ANOMALY is not None:
            _anomaly_fwd(ctx, "rpn_soft_obj_loss", (("loss", loss),))
        return loss.reshape(()), fg

    @staticmethod
    def backward(ctx, g, _gfg):
        (dx,) = ctx.saved_tensors
        if _ANOMALY is not None:
            out = dx * g
            _anomaly_bwd(ctx, "rpn_soft_obj_loss", (("dx", out),))
            return None, out, None, None, None, None
        return None, dx * g, None, None, None, None


def rpn_soft_obj_loss(teacher, x, tau, lam, efl, inv_norm):
    return _RPNSoftObj.apply(teacher, x, tau, lam, efl, inv_norm)


def _kl_efl_forward(ctx, entry: str, q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
    """forward of the KL + entropy-weight Functions: `entry` = ptmi_kl_efl_loss | ptmi_laplace_kl_efl_loss (same arguments)"""
    q = _chk(q.contiguous())
    mu_p = _chk(mu_p.contiguous())
    slog_p = _chk(slog_p.contiguous())
    if fg is not None:
        fg = _chk(fg.contiguous(), torch.uint8)
    rows = q.shape[0]
    loss = torch.empty(1, dtype=F32, device=q.device)
    dq = torch.empty_like(q)
    dmu = torch.empty_like(mu_p) if ctx.needs_input_grad[1] else None
    _lib.call(entry, _ptr(q), _ptr(mu_p), _ptr(slog_p), _ptr(fg), rows, float(tau), float(lam),
              int(efl), int(reduction), float(inv_norm), _ptr(loss), _ptr(dq), _ptr(dmu),
              _ptr(_loss_ws(q.device)), _stream())
    ctx.has_dmu = dmu is not None
    ctx.save_for_backward(dq, dmu) if dmu is not None else ctx.save_for_backward(dq)
    if _ANOMALY is not None:
        _anomaly_fwd(ctx, entry[5:], (("loss", loss),))
    return loss.reshape(())


class _KLEFL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
        return _kl_efl_forward(ctx, "ptmi_kl_efl_loss", q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm)

    @staticmethod
    def backward(ctx, g):
        if ctx.has_dmu:
            dq, dmu = ctx.saved_tensors
            out = (dq * g, dmu * g)
        else:
            (dq,) = ctx.saved_tensors
            out = (dq * g, None)
        if _ANOMALY is not None:
            _anomaly_bwd(ctx, "kl_efl_loss", (("dq", out[0]), ("dmu", out[1])))
        return out[0], out[1], None, None, None, None, None, None, None


def kl_efl_loss(q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
    return _KLEFL.apply(q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm)


class _LaplaceKLEFL(_KLEFL):
    """UNSUPNET.MODEL_TYPE = LAPLACE: the Laplace KL with the Laplace entropy weight (ptmi_laplace_kl_efl_loss); backward as
    the Gaussian's"""

    @staticmethod
    def forward(ctx, q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
        return _kl_efl_forward(ctx, "ptmi_laplace_kl_efl_loss", q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm)


def laplace_kl_efl_loss(q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm):
    return _LaplaceKLEFL.apply(q, mu_p, slog_p, fg, tau, lam, efl, reduction, inv_norm)


# ============================================================================ optimiser / EMA / image prep
def ema_update(student_flat: torch.Tensor, teacher_flat: torch.Tensor, keep_rate: float) -> None:
    _lib.call("ptmi_ema_update", _ptr(_chk(student_flat)), _ptr(_chk(teacher_flat)), student_flat.numel(),
              float(keep_rate), float(1 - keep_rate), _stream())


def sumsq(g_flat: torch.Tensor) -> torch.Tensor:
    out = torch.empty(1, dtype=F32, device=g_flat.device)
    ws = _ws("sumsq", 1024 * 4, g_flat.device)
    _lib.call("ptmi_sumsq", _ptr(_chk(g_flat)), g_flat.numel(), _ptr(out), _ptr(ws), _stream())
    return out


def clip_sgd_step(p, g, buf, sumsq_t, clip_norm, lr, momentum, weight_decay, first: bool) -> None:
    _lib.call("ptmi_clip_sgd_step", _ptr(_chk(p)), _ptr(_chk(g)), _ptr(_chk(buf)), p.numel(), _ptr(sumsq_t),
              float(clip_norm), float(lr), float(momentum), float(weight_decay), int(first), _stream())


def scale_by_clip(g, sumsq_t, clip_norm) -> None:
    _lib.call("ptmi_scale_by_clip", _ptr(_chk(g)), g.numel(), _ptr(sumsq_t), float(clip_norm), _stream())


SEG_CHUNK = 8192       # PTMI_SEG_CHUNK of include/ptmi355.h


class SegmentTable:
    """Device tables of the per-parameter clipping kernels (include/ptmi355.h), built ONCE from the S + 1 host offsets of the
    segments: one int64 tensor [seg_off (S + 1) | seg_chunk (S + 1) | chunks (C x 2)] and the two fp32 workspaces."""

    def __init__(self, offsets: Sequence[int], device):
        from .engine.flat import segment_chunks
        offsets = [int(o) for o in offsets]
        if len(offsets) < 1:
            raise ValueError("a segment table needs at least the offset 0")
        chunks, first = segment_chunks(offsets, SEG_CHUNK)
        self.S, self.C, self.n = len(offsets) - 1, len(chunks), offsets[-1]
        if offsets[0] != 0:
            raise ValueError("the first segment must start at element 0 of the flat buffers")
        words = offsets + first + [w for c in chunks for w in c]
        self.table = torch.tensor(words, dtype=torch.int64).to(device)
        self.seg_off, self.seg_chunk = self.table[: self.S + 1], self.table[self.S + 1: 2 * self.S + 2]
        self.chunks = self.table[2 * self.S + 2:]
        self.ws = torch.empty(max(self.C, 1), dtype=F32, device=device)
        self.seg_norm = torch.empty(max(self.S, 1), dtype=F32, device=device)

    def check(self, *flats):
        for t in flats:
            _chk(t)
            if t.numel() != self.n or t.device != self.table.device:
                raise ValueError(f"flat buffer of {t.numel()} elements on {t.device}: the segment table covers {self.n} on "
                                 f"{self.table.device}")


def seg_gradnorm(g, table: SegmentTable, sumsq_t, clip_norm, inf_norm: bool) -> torch.Tensor:
    """Per-segment norm (L2, or max-abs) of g * clip_norm / max(sqrt(sumsq), clip_norm) into table.seg_norm[:S]."""
    table.check(g)
    _lib.call("ptmi_seg_gradnorm", _ptr(g), g.numel(), _ptr(table.seg_off), _ptr(table.seg_chunk), table.S,
              _ptr(table.chunks), table.C, _ptr(sumsq_t), float(clip_norm), int(bool(inf_norm)), _ptr(table.ws),
              _ptr(table.seg_norm), _stream())
    return table.seg_norm[: table.S]


def clip_sgd_step_seg(p, g, buf, table: SegmentTable, sumsq_t, clip_norm, clip_type: str, clip_value, seg_norm, lr, momentum,
                      weight_decay, first: bool) -> None:
    """clip_sgd_step with SOLVER.CLIP_GRADIENTS: clip_type "value" clamps g * s per element, "norm" scales every segment by
    min(clip_value / (seg_norm + 1e-6), 1) with seg_norm from seg_gradnorm.  g is not written."""
    if clip_type not in ("value", "norm"):
        raise ValueError(f"unknown clip type {clip_type!r}")
    if clip_type == "norm" and seg_norm is None:
        raise ValueError("clip type 'norm' needs the segment norms of seg_gradnorm")
    table.check(p, g, buf)
    _lib.call("ptmi_clip_sgd_step_seg", _ptr(p), _ptr(g), _ptr(buf), p.numel(), _ptr(table.seg_off), table.S,
              _ptr(table.chunks), table.C, _ptr(sumsq_t), float(clip_norm), int(clip_type == "norm"), float(clip_value),
              _ptr(seg_norm) if clip_type == "norm" else None, float(lr), float(momentum), float(weight_decay), int(first),
              _stream())


_CLIP_TYPES = {"value": 0, "norm": 1, "none": 2}


def clip_sgd_step_seg_wd(p, g, buf, table: SegmentTable, sumsq_t, clip_norm, clip_type: str, clip_value, seg_norm, lr, momentum,
                         seg_wd: torch.Tensor, first: bool) -> None:
    """clip_sgd_step_seg with one weight decay per segment, read from the device table seg_wd (fp32, table.S entries: D2's
    SOLVER.WEIGHT_DECAY_NORM), and the clip type "none" (no SOLVER.CLIP_GRADIENTS; clip_value and seg_norm unused)."""
    if clip_type not in _CLIP_TYPES:
        raise ValueError(f"unknown clip type {clip_type!r}")
    if clip_type == "norm" and seg_norm is None:
        raise ValueError("clip type 'norm' needs the segment norms of seg_gradnorm")
    table.check(p, g, buf)
    _chk(seg_wd, name="seg_wd")
    if seg_wd.numel() != table.S or seg_wd.device != table.table.device:
        raise ValueError(f"seg_wd holds {seg_wd.numel()} values on {seg_wd.device} for {table.S} segments on {table.table.device}")
    _lib.call("ptmi_clip_sgd_step_seg_wd", _ptr(p), _ptr(g), _ptr(buf), p.numel(), _ptr(table.seg_off), table.S,
              _ptr(table.chunks), table.C, _ptr(sumsq_t), float(clip_norm), _CLIP_TYPES[clip_type],
              float(clip_value) if clip_type != "none" else 0.0, _ptr(seg_norm) if clip_type == "norm" else None, float(lr),
              float(momentum), _ptr(seg_wd), int(first), _stream())


def _image_desc(rows, device) -> torch.Tensor:
    """rows of 8 ints -> device int64 descriptor table (pinned staging, async copy: no stream synchronisation)."""
    return torch.tensor(rows, dtype=torch.int64).pin_memory().to(device, non_blocking=True)


def preprocess_images(images_u8: List[torch.Tensor], mean: Sequence[float], std: Sequence[float]):
    """D2 preprocess_image + ImageList.from_tensors: (x-mean)/std, zero pad to the batch max; ONE launch per batch."""
    hmax = max(im.shape[-2] for im in images_u8)
    wmax = max(im.shape[-1] for im in images_u8)
    dev = images_u8[0].device
    images_u8 = [_chk(im.contiguous(), torch.uint8, "image") for im in images_u8]
    out = torch.empty((len(images_u8), 3, hmax, wmax), dtype=F32, device=dev)
    desc = _image_desc([[im.data_ptr(), 0, im.shape[-2], im.shape[-1], 0, 0, 0, 0] for im in images_u8], dev)
    _lib.call("ptmi_preprocess_batched", _ptr(desc), _ptr(out), len(images_u8), hmax, wmax, float(mean[0]), float(mean[1]),
              float(mean[2]), float(std[0]), float(std[1]), float(std[2]), _stream())
    return out


def shrink_paste_geometry(h: int, w: int, ratio: float) -> Tuple[int, int, int, int]:
    """(dh, dw, x1, y1) of trainer.py:563-566."""
    dh, dw = int(h * ratio), int(w * ratio)
    return dh, dw, int((w - dw) / 2), int((h - dh) / 2)


def shrink_paste(img_u8: torch.Tensor, ratio: float, mean_int: Sequence[int]) -> Tuple[torch.Tensor, int, int]:
    """trainer.py:557-590 image part for one image; returns (canvas, x1, y1)."""
    img_u8 = _chk(img_u8.contiguous(), torch.uint8, "image")
    h, w = img_u8.shape[-2:]
    dh, dw, x1, y1 = shrink_paste_geometry(h, w, ratio)
    out = torch.empty_like(img_u8)
    _lib.call("ptmi_shrink_paste", _ptr(img_u8), _ptr(out), h, w, dh, dw, y1, x1, int(mean_int[0]), int(mean_int[1]),
              int(mean_int[2]), _stream())
    return out, x1, y1


def shrink_paste_batch(images_u8: List[torch.Tensor], ratios: Sequence[float], mean_int: Sequence[int]):
    """trainer.py:557-590 image part for a whole batch in ONE launch; returns (canvases, [(x1, y1), ...])."""
    images_u8 = [_chk(im.contiguous(), torch.uint8, "image") for im in images_u8]
    if not images_u8:
        return [], []
    dev = images_u8[0].device
    sizes = [3 * im.shape[-2] * im.shape[-1] for im in images_u8]
    buf = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
    outs, rows, offs, o = [], [], [], 0
    for im, ratio, sz in zip(images_u8, ratios, sizes):
        h, w = im.shape[-2:]
        dh, dw, x1, y1 = shrink_paste_geometry(h, w, ratio)
        canvas = buf[o:o + sz].view(3, h, w)
        o += sz
        outs.append(canvas)
        offs.append((x1, y1))
        rows.append([im.data_ptr(), canvas.data_ptr(), h, w, dh, dw, y1, x1])
    desc = _image_desc(rows, dev)
    _lib.call("ptmi_shrink_paste_batched", _ptr(desc), len(images_u8), max(sizes), int(mean_int[0]), int(mean_int[1]),
              int(mean_int[2]), _stream())
    return outs, offs
