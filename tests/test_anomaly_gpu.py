"""GPU (pytest -m gpu): anomaly mode -- the two kernels of csrc/anomaly.hip and PTrainer(detect_anomaly=True).

Every comparison is exact: flag bits, indices, names, bitwise tensor equality (there is no tolerance to choose).  Expected flags
and first indices are computed on the host from the very array the kernel reads.  Values are planted in tensor CONTENTS only."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MAX = 2 ** 63 - 1
NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)

LENGTHS = [1, 3, 255, 256, 257, 1025, 4099, 70001]
SEG_LENGTHS = [1, 3, 18, 255, 256, 257, 1024, 1025, 4099, 70001]
VARIANTS = ("clean", "nan_first", "nan_last", "inf_middle", "inf_then_nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from probabilisticteacher_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib():
    from probabilisticteacher_amd import _lib
    return _lib.load()


def bits_equal(a, b):
    """bitwise tensor equality (NaN == NaN when the bits agree)"""
    view = torch.int32 if a.dtype == torch.float32 else torch.int16 if a.dtype == torch.bfloat16 else a.dtype
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ============================================================================ ptmi_nonfinite_scan
_CLEAN = {}


def _clean(n, bf16):
    """normal values plus the largest finite magnitudes, denormals and -0.0 (every one of them finite), drawn once"""
    key = (n, bf16)
    if key not in _CLEAN:
        gen = torch.Generator().manual_seed(1000 + n)
        x = torch.randn(n, generator=gen)
        if bf16:
            x = x.to(torch.bfloat16)
            special = torch.tensor([0x7F7F, 0xFF7F, 0x0001, 0x807F, 0x8000], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
        else:
            special = torch.tensor([FLT_MAX, -FLT_MAX, 1e-45, -1e-40, -0.0])
        for j in range(len(special)):
            x[(7 * j + 1) % n] = special[j]
        _CLEAN[key] = x
    return _CLEAN[key]


def _variant(n, bf16, name):
    x = _clean(n, bf16).clone()
    if name == "nan_first":
        x[0] = NAN
    elif name == "nan_last":
        x[n - 1] = NAN
    elif name == "inf_middle":
        x[n // 2] = INF
        if n // 2 + 1 < n:
            x[n // 2 + 1] = -INF
    elif name == "inf_then_nan":            # the lower index holds the inf (a 1-element tensor has room for the inf only)
        x[n // 3] = -INF
        if n > 1:
            x[n - 1] = NAN
    return x


def _expect(x):
    """(flags, first) from the bit patterns of the host array: exponent all ones; mantissa zero = inf, else NaN"""
    if x.dtype == torch.bfloat16:
        b = x.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
        expo, mant = (b & 0x7F80) == 0x7F80, (b & 0x7F) != 0
    else:
        b = x.numpy().view(np.uint32).astype(np.int64)
        expo, mant = (b & 0x7F800000) == 0x7F800000, (b & 0x007FFFFF) != 0
    nan, inf = expo & mant, expo & ~mant
    bad = np.nonzero(expo)[0]
    return int(nan.any()) | (int(inf.any()) << 1), int(bad[0]) if bad.size else INT64_MAX


def _on_device(x, shift):
    """x at `shift` elements past a 16-byte boundary: a slice of a larger allocation"""
    big = torch.zeros(x.numel() + 16, dtype=x.dtype, device=DEV)
    v = big[shift:shift + x.numel()]
    v.copy_(x)
    assert v.data_ptr() % 16 == shift * x.element_size()
    return v


def _scan(ops, lib, v, flags, first, slot, dtype=None):
    code = (1 if v.dtype == torch.bfloat16 else 0) if dtype is None else dtype
    return lib.ptmi_nonfinite_scan(ops._ptr(v), v.numel(), code, ops._ptr(flags), ops._ptr(first), slot, flags.numel(), ops._stream())


def _slots(k=4):
    return torch.zeros(k, dtype=torch.int32, device=DEV), torch.full((k,), INT64_MAX, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", LENGTHS)
def test_nonfinite_scan(ops, lib, n, bf16):
    """every variant at every base offset; two slots scanned back to back do not touch each other or their neighbours; a second
    scan into a slot accumulates"""
    shifts = (0, 1, 2, 4, 6) if bf16 else (0, 1, 2, 3)          # bf16: 0 / 2 / 4 / 8 / 12 bytes, fp32: 0 / 4 / 8 / 12
    want_all, got_all = [], []
    for shift in shifts:
        prev = None
        for name in VARIANTS:
            x = _variant(n, bf16, name)
            want = _expect(x)
            assert (want == (0, INT64_MAX)) == (name == "clean")
            v = _on_device(x, shift)
            keep = v.clone()
            flags, first = _slots(4)
            assert _scan(ops, lib, v, flags, first, 1) == 0
            if prev is not None:                                 # the neighbour slot, back to back
                assert _scan(ops, lib, prev[0], flags, first, 2) == 0
            f, i = flags.cpu().tolist(), first.cpu().tolist()
            assert bits_equal(v, keep), "the scan wrote its input"
            want_all.append(want)
            got_all.append((f[1], i[1]))
            assert (f[0], i[0], f[3], i[3]) == (0, INT64_MAX, 0, INT64_MAX), (name, shift, f, i)
            if prev is not None:
                assert (f[2], i[2]) == prev[1], (name, shift, f, i)
                # accumulate: the previous variant into THIS variant's slot
                assert _scan(ops, lib, prev[0], flags, first, 1) == 0
                assert (int(flags[1]), int(first[1])) == (want[0] | prev[1][0], min(want[1], prev[1][1])), (name, shift)
            prev = (v, want)
    assert got_all == want_all, list(zip(got_all, want_all))
    if n > 1:
        assert {w[0] for w in want_all} == {0, 1, 2, 3}


def test_nonfinite_scan_index_is_the_lowest_one_whatever_the_block(ops, lib):
    """many blocks hit at once (every 1000th element of a tensor that fills the capped grid several times): the minimum wins"""
    n = 3 * 2048 * 256 * 4 + 5
    x = torch.zeros(n)
    x[12345::1000] = NAN
    x[777] = INF
    v = x.to(DEV)
    flags, first = _slots(2)
    for _ in range(2):
        assert _scan(ops, lib, v, flags, first, 0) == 0
    assert (flags.cpu().tolist(), first.cpu().tolist()) == ([3, 0], [777, INT64_MAX])
    assert _expect(x) == (3, 777)


def test_nonfinite_scan_argument_checks(ops, lib):
    v = _on_device(_variant(257, False, "nan_first"), 0)
    keep = v.clone()
    flags, first = _slots(4)
    ptr = ops._ptr

    def call(x=v, n=257, dtype=0, fl=flags, fi=first, slot=0, nslots=4):
        return lib.ptmi_nonfinite_scan(ptr(x), n, dtype, ptr(fl), ptr(fi), slot, nslots, ops._stream())

    # one call at a time: the error string is that of the last failed call
    for bad in (dict(slot=-1), dict(slot=4), dict(slot=0, nslots=0), dict(x=None), dict(fl=None), dict(fi=None), dict(dtype=2),
                dict(dtype=-1), dict(n=-1)):
        rc = call(**bad)
        msg = lib.ptmi_last_error().decode()
        assert rc < 0 and msg.startswith("nonfinite_scan:"), (bad, rc, msg)
    # n == 0 launches nothing, also with null pointers
    assert call(n=0) == 0 and call(n=0, x=None, fl=None, fi=None) == 0
    torch.cuda.synchronize()
    assert bits_equal(v, keep) and int(flags.abs().sum()) == 0 and bool((first == INT64_MAX).all())
    from probabilisticteacher_amd import _lib
    with pytest.raises(_lib.PtmiError, match="nonfinite_scan: slot 9"):
        _lib.call("ptmi_nonfinite_scan", ptr(v), 257, 0, ptr(flags), ptr(first), 9, 4, ops._stream())


# ============================================================================ ptmi_seg_nonfinite
def _offsets(lengths):
    offs = [0]
    for k in lengths:
        offs.append(offs[-1] + k)
    return offs


@pytest.mark.parametrize("reverse", [False, True])
def test_seg_nonfinite(ops, reverse):
    lengths = SEG_LENGTHS[::-1] if reverse else SEG_LENGTHS
    offs = _offsets(lengths)
    table = ops.SegmentTable(offs, DEV)
    assert table.S == len(lengths) and table.C == sum(-(-k // ops.SEG_CHUNK) for k in lengths)
    g = torch.randn(offs[-1], generator=torch.Generator().manual_seed(3))
    one, big = offs[lengths.index(1)], offs[lengths.index(70001)]
    plants = {"one": (one, NAN), "last": (big + 70000, -INF), "chunk2": (big + 8192, NAN)}
    for which in (("one", "last", "chunk2"), ("last",), ("chunk2",), ()):
        x = g.clone()
        for k in which:
            x[plants[k][0]] = plants[k][1]
        want = [_expect(x[a:b])[0] for a, b in zip(offs[:-1], offs[1:])]
        assert sum(1 for w in want if w) == len({k == "one" for k in which})
        gd = x.to(DEV)
        keep = gd.clone()
        flags = torch.full((table.S + 2,), 7, dtype=torch.int32, device=DEV)        # stale on entry; two words beyond S
        got = ops.seg_nonfinite(gd, table, flags)
        assert got.cpu().tolist() == want, (which, got.cpu().tolist(), want)
        assert flags[table.S:].cpu().tolist() == [7, 7], "wrote beyond the S flags"
        assert bits_equal(gd, keep), "seg_nonfinite wrote g"
    if which == ():
        assert want == [0] * table.S


def test_seg_nonfinite_segments_off_the_16_byte_grid(ops):
    """the flat buffer 4 bytes past a 16-byte boundary: every chunk takes its scalar head / tail path"""
    offs = _offsets(SEG_LENGTHS)
    table = ops.SegmentTable(offs, DEV)
    x = torch.randn(offs[-1], generator=torch.Generator().manual_seed(4))
    x[offs[4] + 255], x[offs[9]] = INF, NAN
    want = [_expect(x[a:b])[0] for a, b in zip(offs[:-1], offs[1:])]
    assert want == [0, 0, 0, 0, 2, 0, 0, 0, 0, 1]
    flags = torch.zeros(table.S, dtype=torch.int32, device=DEV)
    assert ops.seg_nonfinite(_on_device(x, 1), table, flags).cpu().tolist() == want


def test_seg_nonfinite_argument_checks(ops, lib):
    n, offs = 100, [0, 40, 100]
    table = ops.SegmentTable(offs, DEV)
    g = torch.full((n,), NAN, device=DEV)
    keep = g.clone()
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    ptr = ops._ptr

    def call(g_=g, n_=n, seg=table.seg_off, S=table.S, chunks=table.chunks, C=table.C, fl=flags):
        return lib.ptmi_seg_nonfinite(ptr(g_), n_, ptr(seg), S, ptr(chunks), C, ptr(fl), ops._stream())

    for bad in (dict(g_=None), dict(seg=None), dict(chunks=None), dict(fl=None), dict(n_=-1), dict(S=-1), dict(C=-2), dict(C=0)):
        rc = call(**bad)
        msg = lib.ptmi_last_error().decode()
        assert rc < 0 and msg.startswith("seg_nonfinite:"), (bad, rc, msg)
    # S == 0 and n == 0 are no-ops, also with null tables
    assert call(S=0) == 0 and call(n_=0) == 0 and call(S=0, seg=None, chunks=None, C=0, fl=None) == 0
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0, 0] and bits_equal(g, keep)
    assert call() == 0 and flags.cpu().tolist() == [1, 1]
    # a descriptor outside its segment is skipped, not followed
    bad = table.table.clone()
    bad_chunks = bad[2 * table.S + 2:]
    bad_chunks[0], bad_chunks[3] = 50, 7             # chunk 0 starts outside segment 0; chunk 1 names segment 7 of 2
    assert call(chunks=bad_chunks) == 0
    assert flags.cpu().tolist() == [0, 0] and bits_equal(g, keep)
    with pytest.raises(ValueError):
        ops.seg_nonfinite(g[:50], table, flags)


# ============================================================================ the trainer
CLS_BIAS = "roi_heads.box_predictor.cls_score.bias"


def _cfg(burn_up, *opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_s2c.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "UNSUPNET.BURN_UP_STEP", burn_up, "SOLVER.IMG_PER_BATCH_LABEL", 1,
        "SOLVER.IMG_PER_BATCH_UNLABEL", 1, "SOLVER.WARMUP_ITERS", 0, "SEED", 0] + list(opts))


def _trainer(cfg, **kw):
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    seed_all_rng(cfg.SEED)
    return PTrainer(cfg, **kw)


def _step(tr, batch):
    """one run_step under a `_lib.call` spy -> (metrics or None, the error or None, launch list)"""
    from probabilisticteacher_amd import _lib
    from probabilisticteacher_amd.anomaly import AnomalyError
    calls, call = [], _lib.call

    def spy(name, *a):
        calls.append(name)
        return call(name, *a)
    _lib.call = spy
    metrics = err = None
    try:
        metrics = dict(tr.run_step(batch))
    except AnomalyError as e:
        err = e
    finally:
        _lib.call = call
    torch.cuda.synchronize()
    return metrics, err, calls


def _param(tr, name):
    return dict(tr.model.named_parameters())[name]


def _state(tr):
    return dict(flat=tr.student.flat.clone(), mom=tr.momentum_buf.clone(), teacher=tr.teacher.flat.clone(), iter=tr.iter,
                first=tr._first_step)


def _planted_step(tr, batch, name, index, value):
    """plant `value` at element `index` of parameter `name`, run a step, put the element back -> what the step left behind"""
    p = _param(tr, name)
    before = _state(tr)
    flat_index = tr.student.index[name][0] + int(np.ravel_multi_index(index, tuple(p.shape)))
    saved = p.data[index].clone()
    with torch.no_grad():
        p.data[index] = value
    assert not bool(torch.isfinite(tr.student.flat[flat_index]))
    metrics, err, calls = _step(tr, batch)
    after = _state(tr)
    with torch.no_grad():
        p.data[index] = saved
    keep = torch.ones(before["flat"].numel(), dtype=torch.bool, device=DEV)
    keep[flat_index] = False
    untouched = (bits_equal(after["flat"][keep], before["flat"][keep]) and bits_equal(after["mom"], before["mom"])
                 and after["iter"] == before["iter"] and after["first"] == before["first"]
                 and bits_equal(tr.student.flat, before["flat"]))
    return dict(metrics=metrics, err=err, calls=calls, untouched=untouched, before=before, after=after)


SCANS = ("ptmi_nonfinite_scan", "ptmi_seg_nonfinite")


@pytest.fixture(scope="module")
def runs():
    from bench import synth_records
    cfg0, cfg10 = _cfg(0), _cfg(10)
    K = cfg0.MODEL.ROI_HEADS.NUM_CLASSES
    batch = tuple(synth_records(torch.Generator().manual_seed(77), 1, 192, 256, K, DEV) for _ in range(4))
    out = dict(batch=batch)
    # mutual-learning step: the trainer as it was, the new keyword off, the mode on
    for key, kw in (("plain", {}), ("off", dict(detect_anomaly=False)), ("on", dict(detect_anomaly=True))):
        tr = _trainer(cfg0, **kw)
        m, err, calls = _step(tr, batch)
        out[key] = dict(tr=tr, metrics=m, err=err, calls=calls)
    # burn-in step, planted.  A: forward NaN (then used up by the test that steps it on).  B: the same on a second fresh trainer,
    # then -- the trainer being what it was before each stopped step -- the backward-only and the forward-check plants
    a = _trainer(cfg10, detect_anomaly=True)
    out["a"] = a
    out["a3"] = _planted_step(a, batch, CLS_BIAS, (0,), NAN)
    b = _trainer(cfg10, detect_anomaly=True)
    out["b3"] = _planted_step(b, batch, CLS_BIAS, (0,), NAN)
    out["b4"] = _planted_step(b, batch, "backbone.vgg_block5.0.conv1.weight", (0, 0, 0, 0), NAN)
    out["b5"] = _planted_step(b, batch, "proposal_generator.rpn_head.objectness_logits.bias", (0,), INF)
    return out


def _same_step(a, b):
    ma = {k: v for k, v in a["metrics"].items() if k != "data_time"}
    mb = {k: v for k, v in b["metrics"].items() if k != "data_time"}
    assert ma == mb, (ma, mb)
    for name in ("student", "teacher"):
        assert bits_equal(getattr(a["tr"], name).flat, getattr(b["tr"], name).flat), name
    assert bits_equal(a["tr"].momentum_buf, b["tr"].momentum_buf)
    assert a["tr"].iter == b["tr"].iter == 1


def test_mode_off_is_the_trainer_as_it_was(runs):
    plain, off = runs["plain"], runs["off"]
    assert off["tr"]._anomaly is None and off["tr"]._anomaly_segments is None and off["tr"]._segments is None
    assert off["calls"] == plain["calls"] and not [n for n in plain["calls"] if n in SCANS]
    assert plain["metrics"].keys() == off["metrics"].keys()
    _same_step(plain, off)


def test_mode_on_clean_step_changes_nothing_but_the_scans(runs):
    off, on = runs["off"], runs["on"]
    assert on["err"] is None
    _same_step(off, on)
    assert [n for n in on["calls"] if n not in SCANS] == off["calls"]
    assert on["calls"].count("ptmi_seg_nonfinite") == 1 and on["calls"].count("ptmi_nonfinite_scan") > 50
    # the flags launch sits between backward and the update
    i = on["calls"].index("ptmi_seg_nonfinite")
    assert on["calls"][i + 1:] == ["ptmi_sumsq", "ptmi_clip_sgd_step"]
    sink = on["tr"]._anomaly
    assert sink.collect() == [] and sink.segment_flags == [0] * sink.segments
    print(f"[anomaly] mutual-learning step: {sink.last_used} slots of {sink.capacity}, "
          f"{on['calls'].count('ptmi_nonfinite_scan')} scans, {len(off['calls'])} launches without the mode")
    assert sink.last_used == on["calls"].count("ptmi_nonfinite_scan") and 0 < sink.last_used < sink.capacity


def _check_stopped_before_update(run):
    from probabilisticteacher_amd.anomaly import AnomalyError
    assert isinstance(run["err"], AnomalyError) and run["metrics"] is None
    assert run["untouched"], "student.flat (but the planted element), momentum_buf, _first_step and iter must be what they were"
    assert not [n for n in run["calls"] if n in ("ptmi_sumsq", "ptmi_clip_sgd_step", "ptmi_clip_sgd_step_seg")]
    assert run["err"].iteration == run["before"]["iter"]


def test_forward_nan_is_named_and_the_step_is_not_applied(runs, tmp_path):
    from probabilisticteacher_amd import checkpoint
    run = runs["a3"]
    _check_stopped_before_update(run)
    err = run["err"]
    r = err.records[0]
    print("[anomaly] forward NaN:", str(err).splitlines()[0])
    assert (r.phase, r.branch, r.scope, r.kind, r.first_index) == ("forward", "supervised", "roi_heads.box_predictor.cls_score",
                                                                   "nan", 0)
    assert r.coordinate == (0, 0) and r.op == "linear" and str(err).startswith("non-finite values at iteration 0")
    names = err.parameter_names
    assert CLS_BIAS in names and "roi_heads.box_head.fc1.weight" in names
    # the RPN head is a sibling of the ROI head, and the box-regression loss does not depend on the class logits
    assert not [n for n in names if n.startswith("proposal_generator.rpn_head.") or n.startswith("roi_heads.box_predictor.bbox_pred.")]
    order = [n for n, _ in run_named(runs["a"])]
    assert names == [n for n in order if n in set(names)], "named_parameters() order"
    assert any(x.phase == "backward" for x in err.records)
    # the plant is gone again: the same trainer steps on
    a = runs["a"]
    metrics, err2, calls = _step(a, runs["batch"])
    assert err2 is None and a.iter == 1 and all(np.isfinite(v) for v in metrics.values()), metrics
    assert calls[-2:] == ["ptmi_sumsq", "ptmi_clip_sgd_step"]
    path = checkpoint.save_checkpoint(a, str(tmp_path / "after.pth"))
    assert os.path.exists(path) and torch.load(path, map_location="cpu", weights_only=False)["iteration"] == 0


def run_named(tr):
    return list(tr.model.named_parameters())


def test_backward_only_nan_is_caught_before_the_update(runs):
    run = runs["b4"]
    _check_stopped_before_update(run)
    err = run["err"]
    print("[anomaly] backward-only NaN, first record:", err.records[0].describe())
    print("[anomaly] backward-only NaN, forward records:", [(r.scope, r.output) for r in err.records if r.phase == "forward"])
    assert any(r.phase == "backward" for r in err.records)
    names = err.parameter_names
    assert "backbone.vgg_block4.0.conv3.weight" in names
    assert not [n for n in names if n.startswith("proposal_generator.rpn_head.") or n.startswith("roi_heads.")]
    assert not [r for r in err.records if r.phase == "forward" and
                (r.scope.startswith("roi_heads") or r.scope.startswith("proposal_generator"))]


def test_inf_through_the_existing_forward_check(runs):
    run = runs["b5"]
    _check_stopped_before_update(run)
    err = run["err"]
    assert type(err.__cause__) is FloatingPointError and "Inf/NaN" in str(err.__cause__)
    r = err.records[0]
    assert (r.phase, r.scope, r.op, r.output, r.kind) == ("forward", "proposal_generator.rpn_head.objectness_logits", "rpn_head_1x1",
                                                         "logits", "inf")
    assert err.parameters == [] and "raised in forward" in str(err)
    assert "ptmi_seg_nonfinite" not in run["calls"]


def test_teacher_branch_is_reported_first(runs):
    """mutual learning from iteration 0: the keep-rate-0 EMA copies the plant into the teacher, which runs first"""
    from probabilisticteacher_amd.anomaly import AnomalyError
    run = _planted_step(_trainer(_cfg(0), detect_anomaly=True), runs["batch"], CLS_BIAS, (0,), NAN)
    assert isinstance(run["err"], AnomalyError)
    r = run["err"].records[0]
    assert (r.phase, r.branch, r.scope, r.kind) == ("forward", "unsup_data_weak", "roi_heads.box_predictor.cls_score", "nan")
    # the EMA at the head of the step has happened (keep rate 0: the teacher is the student, plant included); no update followed
    assert run["after"]["iter"] == 0 and bits_equal(run["after"]["mom"], run["before"]["mom"])
    assert bits_equal(run["after"]["teacher"], run["after"]["flat"]) and not bits_equal(run["after"]["teacher"], run["before"]["teacher"])
    assert not [n for n in run["calls"] if n in ("ptmi_sumsq", "ptmi_clip_sgd_step")]


def test_the_report_is_repeatable(runs):
    a, b = runs["a3"]["err"], runs["b3"]["err"]
    assert a.to_json() == b.to_json() and len(a.records) >= 2


def test_amp_clean_step_and_forward_nan(runs):
    batch, amp, res = runs["batch"], _cfg(0, "SOLVER.AMP.ENABLED", True), {}
    for key, kw in (("amp_off", {}), ("amp_on", dict(detect_anomaly=True))):
        tr = _trainer(amp, **kw)
        m, err, calls = _step(tr, batch)
        res[key] = dict(tr=tr, metrics=m, err=err, calls=calls)
    off, on = res["amp_off"], res["amp_on"]
    assert on["err"] is None and "ptmi_p8_conv3x3_waves" in off["calls"]
    _same_step(off, on)
    assert [n for n in on["calls"] if n not in SCANS] == off["calls"]
    sink = on["tr"]._anomaly
    print(f"[anomaly] AMP mutual-learning step: {sink.last_used} slots of {sink.capacity}")
    assert 0 < sink.last_used < sink.capacity
    run = _planted_step(_trainer(_cfg(10, "SOLVER.AMP.ENABLED", True), detect_anomaly=True), batch, CLS_BIAS, (0,), NAN)
    _check_stopped_before_update(run)
    r = run["err"].records[0]
    assert (r.phase, r.branch, r.scope, r.kind, r.first_index) == ("forward", "supervised", "roi_heads.box_predictor.cls_score",
                                                                   "nan", 0)
    assert CLS_BIAS in run["err"].parameter_names


# ---------------------------------------------------------------------------- two ranks sharing the GPU over gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bench import synth_records
    from probabilisticteacher_amd.anomaly import AnomalyError
    cfg = _cfg(10)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    batch = tuple(synth_records(torch.Generator().manual_seed(77 + rank), 1, 192, 256, K, DEV) for _ in range(4))
    tr = _trainer(cfg, detect_anomaly=True)
    assert tr.world_size == 2 and tr.reducer.active
    before = tr.student.flat.clone()
    if rank == 1:                                   # after construction (and its start-up broadcast): this rank only
        with torch.no_grad():
            _param(tr, CLS_BIAS).data[0] = NAN
    err = None
    try:
        tr.run_step(batch)
    except AnomalyError as e:
        err = e
    if rank == 1:
        with torch.no_grad():
            _param(tr, CLS_BIAS).data[0] = before[tr.student.index[CLS_BIAS][0]]
    q.put(dict(rank=rank, err=err, iter=tr.iter, untouched=bits_equal(tr.student.flat, before), first=tr._first_step))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_raise_in_the_same_step():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=900) for _ in procs], key=lambda d: d["rank"])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    a, b = out
    from probabilisticteacher_amd.anomaly import AnomalyError
    for d in out:
        assert isinstance(d["err"], AnomalyError) and d["err"].iteration == 0 and d["iter"] == 0 and d["untouched"] and d["first"]
        assert d["err"].reporting_ranks == [1]
    # rank 0 produced nothing non-finite itself; the averaged gradient it holds is, and it says who reported
    assert a["err"].records == [] and "ranks that reported records: 1" in str(a["err"])
    assert CLS_BIAS in a["err"].parameter_names and "roi_heads.box_head.fc1.weight" in a["err"].parameter_names
    assert a["err"].parameters == b["err"].parameters
    assert b["err"].records[0].scope == "roi_heads.box_predictor.cls_score" and b["err"].records[0].branch == "supervised"


# ---------------------------------------------------------------------------- train_net.py --synthetic --detect-anomaly
def test_train_net_stops_and_leaves_the_last_good_state(tmp_path):
    weights = tmp_path / "planted.pth"
    torch.save({"model": {"modelStudent." + CLS_BIAS: torch.tensor([NAN, 0.0])}}, str(weights))
    out_dir = tmp_path / "out"
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train_net.py"), "--config-file",
           os.path.join(ROOT, "configs/pt/final_s2c.yaml"), "--synthetic", "--detect-anomaly", "--max-iter", "2",
           "MODEL.VGG.PRETRAIN", "", "MODEL.WEIGHTS", str(weights), "OUTPUT_DIR", str(out_dir), "SEED", "0",
           "SOLVER.IMG_PER_BATCH_LABEL", "1", "SOLVER.IMG_PER_BATCH_UNLABEL", "1", "UNSUPNET.BURN_UP_STEP", "10"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert res.returncode not in (0, 124, 137), (res.returncode, res.stderr[-2000:])
    assert "AnomalyError: non-finite values at iteration 0" in res.stderr, res.stderr[-2000:]
    d = json.loads((out_dir / "anomaly.json").read_text())
    assert d["iteration"] == 0 and d["records"][0]["scope"] == "roi_heads.box_predictor.cls_score"
    assert CLS_BIAS in [p["name"] for p in d["parameters"]]
    ckpt = torch.load(str(out_dir / "model_before_anomaly.pth"), map_location="cpu", weights_only=False)
    assert ckpt["iteration"] == -1 and "modelStudent." + CLS_BIAS in ckpt["model"]
    assert not (out_dir / "last_checkpoint").exists() and not (out_dir / "metrics.json").exists()
