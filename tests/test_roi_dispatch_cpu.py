"""CPU: the conditions on the INPUTS of tests/test_roi_dispatch_gpu.py -- the float64 ROIAlign reference, its fp32 yardsticks, the box
sets and the map table of tests/roi_pooler_ref.py -- so that the device file can leave out no dispatch class without this file noticing.

(1) roi_align64 agrees with the oracle the project already trusts (oracle.d2.roi_align, fp32) on the edge boxes to within the forward
    hard bound, and roi_align_backward64 with roi_align_backward to one rounding per term;
(2) the yardsticks pass `check` on every case the device sees: they err (the tight bound is not a demand for exactness), they stay
    within 0.6 of their own hard bound, and forward MARGIN times their error is inside the smallest hard bound: the tight bound decides;
(3) every case's ROIs contain every `classify` class its map and sampling grid admit, and every count list has what it is there for;
(4) a restatement of the host's plane / LDS-class / band rules gives, for the map table, exactly the classes listed in it;
(5) `classify` by hand on boxes whose path can be read off."""
import numpy as np
import pytest
import torch

from oracle import d2
from tests import roi_pooler_ref as ref

CASES = ref.all_cases()


# ================================================================================================ (1) the reference
@pytest.mark.parametrize("c,fh,fw", [(3, 25, 31), (2, 48, 100), (2, 5, 9)])
def test_float64_reference_agrees_with_the_oracle_on_the_edge_boxes(c, fh, fw):
    boxes = ref.edge_boxes(fh, fw, 1 / 16)
    assert boxes.shape == (24, 4) and boxes.dtype == np.float32
    rois, offs = ref.counts_to_rois(boxes, (11, 0, 13))
    assert offs.tolist() == [0, 11, 11, 24] and rois[:, 0].tolist() == [0.0] * 11 + [2.0] * 13
    gen = np.random.default_rng([3, fh, fw])
    feat = ref.scaled_randn(gen, (3, c, fh, fw))
    want = d2.roi_align(torch.from_numpy(feat), torch.from_numpy(rois), 7, 1 / 16).numpy()
    val, S, T = ref.roi_align64(feat, rois, 7, 1 / 16)
    e = ref.scaled_err(want, val, S)
    assert (e <= ref.fwd_terms(T) * ref.U24 * 1.01).all(), f"oracle vs float64 reference: {e.max() / ref.U24:.2f} x 2^-24"
    assert 0 < e.max() <= 8 * ref.U24, f"{e.max() / ref.U24:.2f} x 2^-24: an honest sequential fp32 sum errs by 2 - 4"
    assert np.array_equal(want, ref.roi_align(feat, rois, 7, 1 / 16)), "the fp32 yardstick is the oracle's sum, bit for bit"
    # backward: the older float64 restatement rounds each tap weight to fp32 first: at most one rounding per term apart
    dout = ref.scaled_randn(gen, (24, c, 7, 7), rois[:, 0], 3)
    b64 = ref.roi_align_backward64(dout, rois, feat.shape, 7, 1 / 16)
    old = ref.roi_align_backward(dout, rois, feat.shape, 7, 1 / 16)
    assert ref.err(old, b64.value, b64.S) <= ref.U24 * 1.01
    assert not b64.value[1].any() and not b64.S[1].any() and not b64.K[1].any(), "image 1 has no ROI"


def test_magnitude_and_term_counts_by_hand():
    """one 14 x 14 cell aligned box on a 1-channel map of ones: 2 x 2 samples a bin, every sample inside"""
    feat = np.ones((1, 1, 20, 20), np.float32)
    roi = np.array([[0, 16.0, 16.0, 240.0, 240.0]], np.float32)             # cells 1 .. 15: sw = 0.5, bins of 2 cells
    val, S, T = ref.roi_align64(feat, roi, 7, 1 / 16)
    assert np.allclose(val, 1.0, rtol=0, atol=1e-15) and np.allclose(S, 1.0, rtol=0, atol=1e-15) and (T == 16).all()
    assert (ref.fwd_terms(T) == 40).all()
    b = ref.roi_align_backward64(np.ones((1, 1, 7, 7), np.float32), roi, feat.shape, 7, 1 / 16)
    assert abs(b.value.sum() - 49.0) < 1e-12 and abs(b.S.sum() - 49.0) < 1e-12
    assert b.K.sum() == 49 * 16 and b.nroi.max() == 1 and (b.gmax[b.nroi > 0] == 8).all()
    assert ref.bwd_terms_band(b).max() == 24 and ref.bwd_terms_atomic(b).max() == b.K.max() + 3
    assert not b.value[0, 0, 16:].any() and not b.value[0, 0, :, 16:].any(), "samples reach 1.0 .. 14.5: cells 1 .. 15"
    y32 = ref.roi_align_backward32(np.ones((1, 1, 7, 7), np.float32), roi, feat.shape, 7, 1 / 16)
    assert y32.dtype == np.float32 and ref.err(y32, b.value, b.S) <= 4 * ref.U24


def test_check_sees_what_it_is_for():
    o = ref.build(CASES[3])                                                  # 5 x 25 x 31, the long count list
    good = o.f32y.copy()
    ref.check(good, o.f64, o.fS, ref.fwd_terms(o.fT), o.fe32)
    leak = good.copy()
    leak[3, 0] = o.f32y[3, 1]                                                # another channel's plane
    with pytest.raises(AssertionError, match="hard bound"):
        ref.check(leak, o.f64, o.fS, ref.fwd_terms(o.fT), o.fe32)
    off = good * np.float32(1 + 2.0 ** -19)                                  # 32 units of 2^-24: inside the hard bound of a large grid only
    with pytest.raises(AssertionError):
        ref.check(off, o.f64, o.fS, ref.fwd_terms(o.fT), o.fe32)
    nan = good.copy()
    nan[0, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        ref.check(nan, o.f64, o.fS, ref.fwd_terms(o.fT), o.fe32)
    dead = (o.fS == 0)
    assert dead.any(), "the case holds outputs with no valid sample"
    stray = good.copy()
    stray[dead] = 1e-30                                                       # where S == 0 only the exact value passes
    with pytest.raises(AssertionError):
        ref.check(stray, o.f64, o.fS, ref.fwd_terms(o.fT), o.fe32)


# ================================================================================================ (2) the yardsticks
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_yardsticks_pass_check_on_every_case(case):
    o = ref.build(case)
    for what, y, r64, S, terms, e32 in (("forward", o.f32y, o.f64, o.fS, ref.fwd_terms(o.fT), o.fe32),
                                        ("backward", o.b32y, o.b64.value, o.b64.S, ref.bwd_terms_atomic(o.b64), o.be32)):
        ratio, frac = ref.check(y, r64, S, terms, e32, what=f"{case.name} {what} yardstick")
        assert e32 > 0 and ratio == 1.0, f"{what}: the yardstick is exact here: the tight bound would ask for exactness"
        assert frac <= 0.6, f"{what}: the yardstick uses {frac:.3f} of its own hard bound"
        assert np.isfinite(y).all() and y.dtype == np.float32
    # forward: the tight bound is the one that decides: MARGIN x err(yardstick) is inside the smallest hard bound there is.  (Backward
    # the yardstick's worst cell is one where many taps meet; on a cell with few the hard bound is the narrower one and decides.)
    assert ref.MARGIN * o.fe32 <= ref.fwd_terms(4) * ref.U24, "forward: a one-sample bin's hard bound (16 roundings)"


# ================================================================================================ (3) what the cases contain
@pytest.mark.parametrize("case", [c for c in CASES if c.P == 7], ids=lambda c: c.name)
def test_every_case_contains_every_class_its_map_admits(case):
    o = ref.build(case)
    need = ref.admitted_classes(case.H, case.W, case.ratio)
    have = ref.classes_present(o.rois, case.H, case.W, 7, case.scale, bool(case.aligned), case.ratio)
    assert need <= have, f"{case.name}: no ROI of class {sorted(need - have)}"
    # per image too: the image with 21 (or 41, or 20) ROIs sees every class by itself
    big = int(np.argmax(case.counts))
    rows = o.rois[o.offs[big]: o.offs[big + 1]]
    if case.counts[big] >= 24:
        assert need <= ref.classes_present(rows, case.H, case.W, 7, case.scale, bool(case.aligned), case.ratio)


def test_the_case_list_is_the_planned_one():
    by_group = {}
    for c in CASES:
        by_group.setdefault(c.group, []).append(c)
    maps = by_group["(1) map classes x ROI counts"]
    assert [(c.C, c.H, c.W) for c in maps if c.counts == (0, 3, 21)] == [m[:3] for i, m in enumerate(ref.MAPS) if i not in (0, 1, 3)]
    for i in (0, 1, 3):
        assert [c.counts for c in maps if (c.C, c.H, c.W) == ref.MAPS[i][:3]] == [(0, 1, 2, 3, 0, 21, 0), (41,), (20, 19)]
    assert {(c.C, c.H, c.W, c.aligned, c.ratio) for c in by_group["(2) variants"]} == \
        {m + v for m in ((9, 48, 100), (5, 128, 144)) for v in ((0, 0), (0, 2), (1, 2), (1, 1))}
    assert [(c.C, c.H, c.W, c.scale) for c in by_group["(3) scale"]] == [(5, 25, 31, 1 / 8), (5, 25, 31, 1.0)]
    assert [(c.C, c.H, c.W, c.P) for c in by_group["(4) pooled size"]] == [(5, 25, 31, p) for p in (1, 2, 5, 14)]
    assert all(c.P == 7 and c.scale == 1 / 16 and (c.aligned, c.ratio) == (1, 0) for c in maps) and len(CASES) == 31
    # the long count list: empty images first, in the middle and last; 1, 2 and 3 ROIs (the band pipeline's prologue: headers two
    # ahead, data one ahead); 21 = one more than the forward's 20 slots; 41 = two strides and one
    o = ref.build(maps[0])
    assert np.diff(o.offs).tolist() == [0, 1, 2, 3, 0, 21, 0] and o.offs.dtype == np.int32
    assert (np.diff(o.rois[:, 0]) >= 0).all() and o.rois[:, 0].tolist() == sorted(o.rois[:, 0].tolist())


def test_scaled_boxes_are_the_same_boxes_in_cells():
    a, b, c = (ref.edge_boxes(25, 31, s).astype(np.float64) * s for s in (1 / 16, 1 / 8, 1.0))
    assert np.allclose(a, b, rtol=1e-6, atol=0) and np.allclose(a, c, rtol=1e-6, atol=0)
    e = ref.edge_boxes(25, 31, 1 / 16)
    assert e[:5].tolist() == [[-30.0, -20.0, 40.0, 35.0], [31 * 16 - 96.0, 25 * 16 - 100.0, 31 * 16 + 24.0, 25 * 16 + 20.0],
                              [10.0, 10.0, 10.5, np.float32(10.2)], [0.0, 0.0, 31 * 16.0, 25 * 16.0],
                              [-9000.0, -7000.0, 9500.0, 8000.0]], "the specials of special_boxes"
    # operands: each (image, channel) plane at its own power of two
    x = ref.scaled_randn(np.random.default_rng(1), (4, 6, 9, 9))
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(axis=(2, 3)))
    assert rms.max() / rms.min() >= 2.0 ** 10


# ================================================================================================ (4) the map table
def test_map_table_reaches_every_listed_dispatch_class():
    got = [(c, h, w, ref.fwd_planes(c, h, w, 7), *ref.bwd_plan(c, h, w, 7)[:2]) for c, h, w, *_ in ref.MAPS]
    assert got == ref.MAPS
    # every forward choice (8, 4, 3, 1 planes, the fallback) and backward choice (4, 3, 2, 1 planes, both LDS classes, both fallbacks)
    assert {m[3] for m in ref.MAPS} == {8, 4, 3, 1, 0}
    assert {(m[4], m[5]) for m in ref.MAPS} == {(4, 80), (3, 80), (1, 80), (2, 160), (1, 160), (0, 0)}
    # the exact limits
    assert 8 * 48 * 100 * 4 == 150 * 1024 and ref.fwd_planes(9, 48, 100, 7) == 8 and ref.fwd_planes(9, 50, 100, 7) == 3
    assert 128 * 144 * 4 == 72 * 1024 and ref.fwd_planes(5, 128, 144, 7) == 1 and ref.fwd_planes(5, 128, 145, 7) == 0
    assert ref.bwd_plan(5, 128, 144, 7) == (2, 160, 162432)
    assert ref.bwd_plan(5, 193, 193, 7)[0] == 0 and ref.bwd_plan(5, 192, 193, 7)[0] == 1, "the first map with no plane in 160 KB"
    assert ref.bwd_plan(9, 256, 9, 7)[0] == 4 and ref.bwd_plan(9, 257, 9, 7)[0] == 0, "bands of 32 rows served, 33 not"
    # ragged channel groups: 8 + 1, 4 + 1, 3 under a 4-plane kernel, 3 + 3 + 3
    assert (9 % 8, 5 % 4, 3 < 4, 9 % 3) == (1, 1, True, 0)
    # 1 x 5 x 9: bands of one row, waves 5 .. 7 own none; pooled != 7 is never served
    assert -(-5 // ref.BANDS) == 1 and ref.fwd_planes(5, 25, 31, 5) == 0 and ref.bwd_plan(5, 25, 31, 14)[0] == 0


def test_the_fallback_and_refusal_cases_are_the_ones_meant():
    assert {(c.C, c.H, c.W, c.P) for c in CASES if not c.bwd_served} == \
        {(5, 193, 193, 7), (9, 257, 9, 7)} | {(5, 25, 31, p) for p in (1, 2, 5, 14)}
    assert {(c.C, c.H, c.W, c.P) for c in CASES if not c.fwd_served} == \
        {(5, 140, 140, 7), (5, 193, 193, 7)} | {(5, 25, 31, p) for p in (1, 2, 5, 14)}


# ================================================================================================ (5) classify by hand
def test_classify_by_hand():
    H, W = 48, 100
    e = ref.edge_boxes(H, W, 1 / 16)
    roi = lambda i: np.concatenate([[0.0], e[i]]).astype(np.float32)
    cl = lambda i, **kw: ref.classify(roi(i), H, W, 7, 1 / 16, **kw)
    assert ref.tab_stride(H, W) == 20 and ref.tab_stride(5, 9) == 4
    assert cl(2) == ("unrolled", 1, frozenset({0}))                            # tiny: one cell pair, the first band (6 rows)
    assert cl(3)[0] == "generic" and cl(3)[1] == 7 and cl(3)[2] == frozenset(range(8))      # the whole image: 100 columns
    assert cl(4)[0] == "notable"                                             # many times the map
    for i in (5, 6, 7, 8, 9, 10, 11):                                        # adaptive grid: no extent, no sample
        assert cl(i) == ("novalid", 0, frozenset()), i
    assert cl(7, aligned=True, sampling_ratio=2)[0] == "notable", "a fixed grid on an inverted box descends"
    assert cl(7, aligned=False, sampling_ratio=2)[0] == "unrolled", "not aligned: an inverted box is one cell wide"
    assert cl(12) == ("unrolled", 1, frozenset({0, 1})) and cl(13)[2] == frozenset({7})
    assert cl(15)[1] == 2 and cl(17)[1] == 2 and cl(18)[1] == 3
    assert cl(19)[0] == "generic" and cl(20) == ("unrolled", 1, frozenset({0}))
    assert cl(23, aligned=False, sampling_ratio=2)[0] == "notable" and cl(23, aligned=True, sampling_ratio=1)[0] == "unrolled"
    # samples exactly on -1.0 and on W / H are valid (inclusive test) -- and one ulp further out they are not
    _, sw, sh, bw, bh, gw, gh, _ = ref._align_geom(roi(12), 7, 1 / 16, True, 0)
    assert (sw, bw, gw) == (-1.5, 1.0, 1) and len(ref._axis_taps(sw, bw, 0, gw, W)[0]) == 1
    assert len(ref._axis_taps(np.nextafter(np.float32(sw), np.float32(-2)), bw, 0, gw, W)[0]) == 0
    _, sw, sh, bw, bh, gw, gh, _ = ref._align_geom(roi(13), 7, 1 / 16, True, 0)
    lo, hi, l, h = ref._axis_taps(sw, bw, 6, gw, W)
    assert sw + 6 * bw + np.float32(.5) * bw == W and (lo.tolist(), hi.tolist(), l.tolist()) == ([W - 1], [W - 1], [0.0])
    _, sw, _, bw, _, gw, _, _ = ref._align_geom(roi(21), 7, 1 / 16, False, 0)
    assert (sw, bw, gw) == (-1.5, 1.0, 1)
