"""GPU (pytest -m gpu): every ROIAlign entry of csrc/roi_align.hip through the C ABI -- ptmi_roi_align_fwd[_ex], _fwd_grouped[_ex],
_bwd[_ex], _bwd_grouped[_ex], _bwd_det -- against the float64 reference of tests/roi_pooler_ref.py with its fp32 yardsticks (see the
header of that file's second half: scale-aware error, derived hard bounds, tight bound 4 x err(yardstick)), over every choice the host
code makes: channel planes per workgroup and LDS class forward and backward, the band limit, ROIs per image, box geometry, pooled
size, scale and the (aligned, sampling_ratio) variants.  tests/test_roi_dispatch_cpu.py proves that the map table reaches the classes
listed below and that every case's boxes contain every path a ROI can take.

    C, H, W         forward                                     backward
    9, 48, 100      8 planes, exactly 150 KB, ragged 8 + 1      3 planes (3 + 3 + 3)
    5, 25, 31       4 planes, ragged 4 + 1                      4 + 1
    3, 25, 31       3 planes under NCH = 4 (one aliased)        3
    1, 5, 9         1 plane                                     bands of 1 row, three waves own none, map narrower than a window
    9, 50, 100      3 planes                                    3
    5, 100, 120     1 plane                                     1 plane, 80 KB
    5, 128, 144     1 plane, exactly 72 KB                      2 planes, 160 KB class (162,432 B)
    5, 140, 140     gather fallback                             1 plane, 160 KB
    5, 193, 193     gather fallback                             no fit: atomic fallback
    9, 256 | 257, 9 8 planes                                    bands of 32 rows served | 33: atomic fallback

Cases (tests/roi_pooler_ref.all_cases): (1) every map with the ROI counts (0, 3, 21), the first, second and fourth also with
(0, 1, 2, 3, 0, 21, 0), (41,) and (20, 19); (2) the variants (0, 0), (0, 2), (1, 2), (1, 1) on the first and seventh map; (3) scale
1/8 and 1 on 5 x 25 x 31 with the boxes rescaled; (4) pooled size 1, 2, 5, 14 on 5 x 25 x 31 (the grouped entries route to the plain
kernels).  Boxes: the 24 edge boxes of roi_pooler_ref.edge_boxes first, seeded random ones after them.  Features and gradients: randn
with every (image, channel) plane at its own power of two from 2^-10 .. 2^10.

Every operand is the payload of a tests/guarded.py buffer and every workspace has exactly the queried size.  After every launch: the
guards of output and workspace intact, no output element left unwritten, read-only operands bit-unchanged, the output finite, both
bounds against float64; a second launch of the grouped forward and of the band backward gives the same bits; a ROI without a valid
sample is exactly 0 in every channel; a cell no tap lands on -- all of an image without ROIs included -- is exactly 0; bwd_det and
bwd_grouped give the same bits where the band kernel serves; where it does not, bwd_det is an error that launches nothing (also
through ops.deterministic) and bwd_grouped reaches parity through the atomic kernel; where the forward is not served the grouped
entry equals the plain one bit for bit.

Measured on an MI355X (first device run of this file): per group and entry the largest err(got) / err(yardstick) and the largest
share of the hard bound (the atomic scatter's figures move in the last digit from run to run).

    group                          entry         cases | ratio | of hard bound
    (1) map classes x ROI counts   fwd              17 |  1.00 |  0.201
    (1) map classes x ROI counts   fwd_grouped      17 |  1.85 |  0.201
    (1) map classes x ROI counts   bwd              17 |  1.41 |  0.469
    (1) map classes x ROI counts   bwd_grouped      17 |  1.19 |  0.431
    (1) map classes x ROI counts   bwd_det          15 |  0.89 |  0.091
    (2) variants                   fwd               8 |  1.00 |  0.183
    (2) variants                   fwd_grouped       8 |  1.69 |  0.183
    (2) variants                   bwd               8 |  1.16 |  0.458
    (2) variants                   bwd_grouped       8 |  1.00 |  0.115
    (2) variants                   bwd_det           8 |  1.00 |  0.115
    (3) scale                      fwd               2 |  1.00 |  0.134
    (3) scale                      fwd_grouped       2 |  1.62 |  0.133
    (3) scale                      bwd               2 |  1.15 |  0.327
    (3) scale                      bwd_grouped       2 |  0.61 |  0.070
    (3) scale                      bwd_det           2 |  0.61 |  0.070
    (4) pooled size                fwd               4 |  1.00 |  0.188
    (4) pooled size                fwd_grouped       4 |  1.00 |  0.188
    (4) pooled size                bwd               4 |  1.07 |  0.419
    (4) pooled size                bwd_grouped       4 |  1.25 |  0.419

Every ratio is below 2, so MARGINS is empty.  The gather kernel sums in the yardstick's order (ratio 1.00: the same error); the table
kernels round the 1 / count and the table sums in addition and sit at 1.6 - 1.85.  The band kernel's share of ITS hard bound is small
because that bound counts 7 roundings for every later ROI on a cell, while most of those FMAs add an exact zero; the shares near 0.45
are the atomic kernel on cells where a handful of taps meet (K + 3 roundings allowed, 4 - 5 units of 2^-24 spent), and
bwd_grouped of group (1) and (4) includes the shapes that fall back to it.  (1) bwd_det: 15 cases, 5 x 193 x 193 and 9 x 257 x 9 are
refused.  Nothing here found a defect: csrc/roi_align.hip is unchanged.
"""
import os

import numpy as np
import pytest
import torch

from tests import roi_pooler_ref as ref
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
F32, U8 = torch.float32, torch.uint8
# a (group, entry) whose device ratio exceeds roi_pooler_ref.MARGIN gets its own margin here, with the measured ratio and the reason
MARGINS = {}
STATS = {}
CASES = ref.all_cases()


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from probabilisticteacher_amd import _lib, ops
    lib = _lib.load()
    yield _lib, lib, ops
    if os.environ.get("PTMI_TEST_VERBOSE"):
        for (group, entry), (cases, ratio, frac) in sorted(STATS.items()):
            print(f"[group] {group:30s} {entry:12s} cases {cases:3d} | ratio {ratio:5.2f} | of hard bound {frac:6.3f}")


def _p(gd):
    from probabilisticteacher_amd import ops
    return ops._ptr(None if gd is None else gd.payload)


def _stream():
    from probabilisticteacher_amd import ops
    return ops._stream()


def _ro(arr):
    return Guarded.of(torch.tensor(arr), GUARD, GUARD, DEV).snapshot()          # (a copy: the case's arrays are read-only)


def _out(shape, dtype=F32):
    return Guarded(shape, dtype, GUARD, GUARD, DEV)


def _ws(nbytes):
    assert nbytes > 0
    return Guarded((int(nbytes),), U8, GUARD, GUARD, DEV)


def _record(case, entry, ratio, frac):
    cases, r, f = STATS.get((case.group, entry), (0, 0.0, 0.0))
    STATS[(case.group, entry)] = (cases + 1, max(r, ratio), max(f, frac))


class Launcher:
    """the guarded operands of one case and one method per entry; every method returns after `_after`"""

    def __init__(self, api, case):
        self._lib, self.lib, self.ops = api
        self.case, self.o = case, ref.build(case)
        o = self.o
        self.n, self.R = o.shape[0], len(o.rois)
        self.feat, self.rois, self.offs, self.dout = _ro(o.feat), _ro(o.rois), _ro(o.offs), _ro(o.dout)
        self.sfx, self.var = ("", ()) if (case.aligned, case.ratio) == (1, 0) else ("_ex", (case.aligned, case.ratio))
        self.dims = (self.n, case.C, case.H, case.W, self.R, case.P, case.scale)

    def _after(self, what, out, ws, reads, expect_written=True):
        torch.cuda.synchronize()
        out.assert_guards_intact(f"{what}: output")
        if ws is not None:
            ws.assert_guards_intact(f"{what}: workspace")
        for name in reads:
            getattr(self, name).assert_unchanged(f"{what}: {name}")
        if expect_written:
            assert out.unwritten() == 0, f"{what}: {out.unwritten()} output elements still hold the fill pattern"
            got = out.payload.cpu().numpy()
            bad = ~np.isfinite(got)
            assert not bad.any(), f"{what}: {int(bad.sum())} non-finite outputs, first at {np.argwhere(bad)[0]}"
            return got
        return None

    # ------------------------------------------------------------------ forward
    def fwd(self):
        what = f"{self.case.name}: ptmi_roi_align_fwd{self.sfx}"
        out = _out((self.R, self.case.C, self.case.P, self.case.P))
        self._lib.call("ptmi_roi_align_fwd" + self.sfx, _p(self.feat), _p(self.rois), _p(out), *self.dims, _stream(), *self.var)
        return out, self._after(what, out, None, ("feat", "rois")), what

    def fwd_grouped(self):
        what = f"{self.case.name}: ptmi_roi_align_fwd_grouped{self.sfx}"
        out = _out((self.R, self.case.C, self.case.P, self.case.P))
        ws = _ws(self.lib.ptmi_roi_align_ws_bytes(self.R, self.case.H, self.case.W))
        self._lib.call("ptmi_roi_align_fwd_grouped" + self.sfx, _p(self.feat), _p(self.rois), _p(self.offs), _p(out), _p(ws), *self.dims,
                       _stream(), *self.var)
        return out, self._after(what, out, ws, ("feat", "rois", "offs")), what

    # ------------------------------------------------------------------ backward
    def bwd(self):
        """the atomic scatter adds into a dfeat the caller zeroed"""
        what = f"{self.case.name}: ptmi_roi_align_bwd{self.sfx}"
        dfeat = _out(self.o.shape)
        dfeat.payload.zero_()
        self._lib.call("ptmi_roi_align_bwd" + self.sfx, _p(self.dout), _p(self.rois), _p(dfeat), *self.dims, _stream(), *self.var)
        return dfeat, self._after(what, dfeat, None, ("dout", "rois")), what

    def bwd_grouped(self, det=False):
        """dfeat arrives holding the fill pattern: the entry writes every cell itself"""
        entry, var = ("ptmi_roi_align_bwd_det", (self.case.aligned, self.case.ratio)) if det else ("ptmi_roi_align_bwd_grouped" + self.sfx, self.var)
        what = f"{self.case.name}: {entry}"
        dfeat = _out(self.o.shape)
        ws = _ws(self.lib.ptmi_roi_align_bwd_ws_bytes(self.R, self.case.H, self.case.W))
        args = (_p(self.dout), _p(self.rois), _p(self.offs), _p(dfeat), _p(ws), *self.dims, _stream(), *var)
        if det and not self.case.bwd_served:
            with pytest.raises(self._lib.PtmiError, match="not served"):
                self._lib.call(entry, *args)
            self._after(what, dfeat, ws, ("dout", "rois", "offs"), expect_written=False)
            assert dfeat.unwritten() == dfeat.numel, f"{what}: the refused call wrote {dfeat.numel - dfeat.unwritten()} cells of dfeat"
            return dfeat, None, what
        self._lib.call(entry, *args)
        return dfeat, self._after(what, dfeat, ws, ("dout", "rois", "offs")), what


def _check_fwd(case, o, got, what, entry):
    ratio, frac = ref.check(got, o.f64, o.fS, ref.fwd_terms(o.fT), o.fe32, MARGINS.get((case.group, entry), ref.MARGIN), what)
    _record(case, entry, ratio, frac)
    dead = np.flatnonzero(o.fS.reshape(len(o.rois), -1).max(1) == 0)
    assert len(dead) >= 2, "the case holds ROIs without a valid sample"
    assert not got[dead].any(), f"{what}: a ROI with no valid sample must give exactly 0.0 in every channel"


def _check_bwd(case, o, got, what, entry, band):
    terms = ref.bwd_terms_band(o.b64) if band else ref.bwd_terms_atomic(o.b64)
    ratio, frac = ref.check(got, o.b64.value, o.b64.S, terms, o.be32, MARGINS.get((case.group, entry), ref.MARGIN), what)
    _record(case, entry, ratio, frac)
    untouched = np.broadcast_to(o.b64.K == 0, got.shape)
    assert not got[untouched].any(), f"{what}: a cell outside every ROI's support must be exactly 0.0"
    for img, cnt in enumerate(case.counts):
        if cnt == 0:
            assert not got[img].any(), f"{what}: image {img} has no ROI: every cell exactly 0.0"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_roi_align_entries_at_float64_parity(api, case):
    run = Launcher(api, case)
    o = run.o
    # forward: the gather kernel, then the grouped entry (LDS planes + per-bin tables where the shape is served)
    plain, got, what = run.fwd()
    _check_fwd(case, o, got, what, "fwd")
    grouped, got, what = run.fwd_grouped()
    _check_fwd(case, o, got, what, "fwd_grouped")
    again, _, _ = run.fwd_grouped()
    assert torch.equal(grouped.raw, again.raw), f"{what}: a second launch gives other bits"
    if not case.fwd_served:
        assert torch.equal(grouped.payload, plain.payload), f"{what}: not served by the LDS kernel: the plain kernel, bit for bit"
    del plain, grouped, again
    # backward: the atomic scatter, the grouped entry (band kernel where served, else zero fill + atomic scatter), the deterministic entry
    _, got, what = run.bwd()
    _check_bwd(case, o, got, what, "bwd", band=False)
    grouped, got, what = run.bwd_grouped()
    _check_bwd(case, o, got, what, "bwd_grouped", band=case.bwd_served)
    det, got, what = run.bwd_grouped(det=True)
    if case.bwd_served:
        _check_bwd(case, o, got, what, "bwd_det", band=True)
        assert torch.equal(det.raw, grouped.raw), f"{what}: the launch path of bwd_grouped: the same bits"
        again, _, _ = run.bwd_grouped()
        assert torch.equal(again.raw, grouped.raw), f"{what}: a second launch of the band kernel gives other bits"


@pytest.mark.parametrize("case", [c for c in CASES if not c.bwd_served], ids=lambda c: c.name)
def test_deterministic_mode_refuses_the_shapes_the_band_kernel_does_not_serve(api, case):
    """through ops: no quiet fall-back to the atomic scatter"""
    _lib, _, ops = api
    o = ref.build(case)
    fd = torch.tensor(o.feat, device=DEV).requires_grad_()
    out = ops.roi_align(fd, torch.tensor(o.rois, device=DEV), case.P, case.scale, torch.tensor(o.offs, device=DEV), bool(case.aligned),
                        case.ratio)
    with ops.deterministic(True), pytest.raises(_lib.PtmiError, match="not served"):
        out.backward(torch.tensor(o.dout, device=DEV))
    assert fd.grad is None and not ops.is_deterministic()
