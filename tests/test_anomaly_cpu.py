"""CPU: the host side of anomaly mode (probabilisticteacher_amd/anomaly.py, ops.anomaly / ops.anomaly_scope) with a fake sink --
its device arrays are host tensors and its "kernel" classifies with torch -- so no HIP kernel runs here.  Every comparison is
exact."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from probabilisticteacher_amd import anomaly, ops
from probabilisticteacher_amd.anomaly import INT64_MAX, AnomalyError, AnomalyRecord, AnomalySink

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeSink(AnomalySink):
    """AnomalySink whose slots live on the host: `_launch` restates ptmi_nonfinite_scan's contract with torch"""

    def __init__(self, capacity=8, segments=0):
        self.copies = []
        super().__init__(torch.device("cpu"), capacity, segments)

    def _launch(self, tensor, dtype, slot):
        flat = tensor.reshape(-1).float()
        nan, inf = torch.isnan(flat), torch.isinf(flat)
        bad = torch.nonzero(nan | inf).reshape(-1)
        self.flags[self.segments + slot] |= int(nan.any()) | (int(inf.any()) << 1)
        if bad.numel():
            self.first[slot] = min(int(self.first[slot]), int(bad[0]))

    def _fetch_flags(self, used):
        self.copies.append(("flags", used))
        return super()._fetch_flags(used)

    def _fetch_first(self, used):
        self.copies.append(("first", used))
        return super()._fetch_first(used)


def _rec(**kw):
    base = dict(phase="forward", branch="supervised", scope="roi_heads.box_predictor.cls_score", op="linear", output="y",
                kind="nan", shape=(4, 2), dtype="float32", first_index=0, coordinate=(0, 0))
    base.update(kw)
    return AnomalyRecord(**base)


def test_records_come_back_in_execution_order_with_kind_index_and_coordinate():
    sink = FakeSink(capacity=8)
    sink.begin_step()
    clean = torch.arange(6.0).reshape(2, 3)
    a = clean.clone()
    a[1, 2] = float("inf")
    b = clean.clone()
    b[0, 1], b[1, 0] = float("-inf"), float("nan")
    c = clean.clone().to(torch.bfloat16)
    c[1, 1] = float("nan")
    sink.scan(clean, "forward", "linear", "y", "supervised", "roi_heads.box_head.fc1")
    sink.scan(b, "forward", "linear", "y", "supervised", "roi_heads.box_head.fc2")
    sink.scan(torch.zeros(3, dtype=torch.int32), "forward", "roi_pool", "argmax")          # no slot: cannot be non-finite
    sink.scan(torch.zeros(0), "forward", "linear", "y")                                     # no slot: empty
    sink.scan(a, "backward", "linear", "dx", "supervised", "roi_heads.box_head.fc2")
    sink.scan(c, "backward", "p8_block", "dz", "joint", "backbone.vgg_block5.0.conv1")
    assert sink.used == 4
    recs = sink.collect()
    assert sink.last_used == 4
    assert [(r.phase, r.scope, r.output, r.kind, r.first_index, r.coordinate, r.dtype) for r in recs] == [
        ("forward", "roi_heads.box_head.fc2", "y", "nan+inf", 1, (0, 1), "float32"),
        ("backward", "roi_heads.box_head.fc2", "dx", "inf", 5, (1, 2), "float32"),
        ("backward", "backbone.vgg_block5.0.conv1", "dz", "nan", 4, (1, 1), "bfloat16")]
    assert recs[2].branch == "joint" and recs[0].shape == (2, 3)
    # one copy of the flags, the indices only because a flag was set; a clean step makes the one copy
    assert sink.copies == [("flags", 4), ("first", 4)]
    sink.begin_step()
    assert sink.used == 0 and int(sink.flags.abs().sum()) == 0 and bool((sink.first == INT64_MAX).all())
    sink.scan(clean, "forward", "linear", "y")
    sink.copies.clear()
    assert sink.collect() == [] and sink.copies == [("flags", 1)]


def test_a_second_scan_into_a_slot_accumulates_and_segment_flags_ride_in_the_same_copy():
    sink = FakeSink(capacity=4, segments=3)
    sink.begin_step()
    sink.seg_flags[1] = 2                       # what ops.seg_nonfinite would have written
    x = torch.zeros(5)
    x[3] = float("nan")
    sink.scan(x, "backward", "linear", "dw")
    y = torch.zeros(5)
    y[1] = float("inf")
    sink._launch(y, 0, 0)                       # same slot again: flags OR, lower index wins
    (r,) = sink.collect()
    assert (r.kind, r.first_index) == ("nan+inf", 1)
    assert sink.segment_flags == [0, 2, 0] and sink.copies[0] == ("flags", 1)
    names = ["anchor", "b.weight", "a.bias"]
    assert anomaly.flagged_parameters(sink.segment_flags, names, ["a.bias", "b.weight", "anchor"]) == [("b.weight", "inf")]
    assert anomaly.flagged_parameters([1, 3, 2], names, ["a.bias", "b.weight", "anchor"]) == [
        ("a.bias", "inf"), ("b.weight", "nan+inf"), ("anchor", "nan")]


def test_capacity_overflow_is_an_error_not_a_dropped_record():
    sink = FakeSink(capacity=2)
    sink.begin_step()
    sink.scan(torch.zeros(2), "forward", "linear", "y")
    sink.scan(torch.zeros(2), "forward", "linear", "y")
    with pytest.raises(RuntimeError, match="more than 2 tensors.*larger capacity"):
        sink.scan(torch.zeros(2), "backward", "conv3x3", "dx", "supervised", "backbone.vgg_block3.0.conv1")
    assert sink.used == 2
    sink.begin_step()                           # the next step starts over
    sink.scan(torch.zeros(2), "forward", "linear", "y")
    with pytest.raises(ValueError):
        FakeSink(capacity=0)


def test_scope_and_branch_stacks():
    assert ops._ANOMALY is None
    with ops.anomaly_scope("backbone"), ops.anomaly_branch("supervised"):          # no sink: nothing is pushed
        assert ops.anomaly_labels() == ("", "") and ops._ANOMALY_SCOPES == [] and ops._ANOMALY_BRANCHES == []
    sink = FakeSink()
    with ops.anomaly(sink) as s:
        assert s is sink and ops._ANOMALY is sink
        with ops.anomaly_branch("joint"), ops.anomaly_scope("backbone"):
            with ops.anomaly_scope("vgg_block5.0"):
                assert ops.anomaly_labels() == ("joint", "backbone.vgg_block5.0")
                with ops.anomaly_branch("unsupervised"):
                    assert ops.anomaly_labels()[0] == "unsupervised"
                with pytest.raises(KeyError):
                    with ops.anomaly_scope("conv1"):
                        raise KeyError("popped on the way out")
                assert ops.anomaly_labels() == ("joint", "backbone.vgg_block5.0")
            assert ops.anomaly_labels() == ("joint", "backbone")
        assert ops.anomaly_labels() == ("", "")
        with ops.anomaly(None):
            assert ops._ANOMALY is None
        assert ops._ANOMALY is sink
    assert ops._ANOMALY is None


def test_function_helpers_label_forward_and_backward_alike():
    """what every autograd Function does with a sink: forward remembers the labels on its ctx, backward -- called outside every
    `with` -- reports under them; a scope suffix names the layer inside a fused node"""
    class Ctx:
        pass
    sink, ctx = FakeSink(), Ctx()
    bad = torch.tensor([1.0, float("nan")])
    with ops.anomaly(sink):
        sink.begin_step()
        with ops.anomaly_branch("supervised"), ops.anomaly_scope("backbone"), ops.anomaly_scope("vgg_block4.0"):
            ops._anomaly_fwd(ctx, "vgg_block", [("y", torch.zeros(2), "conv1"), ("y", bad, "conv2"), ("pooled", None)])
        ops._anomaly_bwd(ctx, "vgg_block", [("dw", bad, "conv3"), ("dx", None), ("dx", bad)])
        recs = sink.collect()
    assert sink.last_used == 4
    assert [(r.phase, r.branch, r.scope, r.output) for r in recs] == [
        ("forward", "supervised", "backbone.vgg_block4.0.conv2", "y"),
        ("backward", "supervised", "backbone.vgg_block4.0.conv3", "dw"),
        ("backward", "supervised", "backbone.vgg_block4.0", "dx")]


def test_error_message_json_and_pickle_round_trip():
    recs = [_rec(), _rec(phase="backward", scope="roi_heads.box_head.fc2", output="dx", kind="nan+inf", first_index=7,
                         coordinate=(3, 1)),
            _rec(phase="backward", branch="joint", scope="backbone.vgg_block5.0.conv1", op="p8_block", output="dz", kind="inf",
                 shape=(64, 3, 5, 8), dtype="bfloat16", first_index=9, coordinate="halo")]
    params = [("roi_heads.box_head.fc1.weight", "nan"), ("roi_heads.box_predictor.cls_score.bias", "nan+inf")]
    err = AnomalyError(12, recs, params, [1], "raised in forward: boxes")
    assert isinstance(err, FloatingPointError)
    msg = str(err)
    first_line = msg.splitlines()[0]
    assert first_line.startswith("non-finite values at iteration 12, the update was not applied; first: forward of supervised / "
                                 "roi_heads.box_predictor.cls_score: linear -> y")
    assert "holds nan, first at flat index 0 = (0, 0)" in first_line
    assert msg.index("roi_heads.box_predictor.cls_score: linear") < msg.index("roi_heads.box_head.fc2") < msg.index("vgg_block5")
    assert "ranks that reported records: 1" in msg and "roi_heads.box_head.fc1.weight (nan)" in msg and msg.endswith("boxes")
    assert (err.iteration, err.parameter_names) == (12, [n for n, _ in params])
    # JSON
    d = json.loads(err.to_json())
    assert d["iteration"] == 12 and d["message"] == msg and len(d["records"]) == 3
    assert d["records"][2]["coordinate"] == "halo" and d["records"][1]["coordinate"] == [3, 1]
    assert d["parameters"][1] == {"name": "roi_heads.box_predictor.cls_score.bias", "kind": "nan+inf"}
    back = AnomalyError.from_json(err.to_json())
    assert back.records == recs and back.parameters == params and str(back) == msg and back.to_json() == err.to_json()
    # pickle (the error crosses multiprocessing queues)
    again = pickle.loads(pickle.dumps(err))
    assert type(again) is AnomalyError and again.records == recs and again.parameters == params
    assert (again.iteration, again.reporting_ranks, again.note, str(again)) == (12, [1], err.note, msg)
    # a rank that saw nothing itself
    quiet = AnomalyError(3, [], params, [1])
    assert "no tensor scanned on this rank was non-finite" in str(quiet) and "ranks that reported records: 1" in str(quiet)
    assert pickle.loads(pickle.dumps(quiet)).records == []


@pytest.mark.parametrize("n,c,h,w", [(2, 24, 3, 5), (1, 16, 1, 1)])
def test_p8_offset_decoding_against_a_brute_force_index_map(n, c, h, w):
    """every element of t[2 ceil(C/16)][N (H + 1) + 1][W + 1][8]: the map is built the way the layout is stated in
    include/ptmi355.h -- pixel (n, y, x) at row n (H + 1) + 1 + y, column 1 + x, channel ch at plane ch // 8, lane ch % 8"""
    planes, rows, ws = 2 * (-(-c // 16)), n * (h + 1) + 1, w + 1
    tag = np.full((planes, rows, ws, 8), -1, dtype=np.int64)            # -1 = halo, -2 = channel padding
    tag[:, 1:, 1:, :] = -2
    for i in range(n + 1):
        tag[:, i * (h + 1), :, :] = -1
    coords = {}
    for i in range(n):
        for ch in range(c):
            for y in range(h):
                for x in range(w):
                    k = len(coords)
                    coords[k] = (i, ch, y, x)
                    tag[ch // 8, i * (h + 1) + 1 + y, 1 + x, ch % 8] = k
    flat = tag.reshape(-1)
    assert int((flat >= 0).sum()) == n * c * h * w
    for off, t in enumerate(flat.tolist()):
        want = "halo" if t == -1 else "channel padding" if t == -2 else coords[t]
        assert anomaly.p8_decode(off, n, c, h, w) == want, off
    if c % 16:
        assert int((flat == -2).sum()) > 0
    for off in (-1, flat.size):
        with pytest.raises(ValueError):
            anomaly.p8_decode(off, n, c, h, w)
    assert anomaly.unravel(0, ()) == () and anomaly.unravel(23, (2, 3, 4)) == (1, 2, 3)


def test_train_net_parses_detect_anomaly():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_net.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--detect-anomaly" in out.stdout
    src = open(os.path.join(ROOT, "train_net.py")).read()
    assert "detect_anomaly=args.detect_anomaly" in src and "model_before_anomaly.pth" in src and "anomaly.json" in src


def test_header_and_binding_table_name_the_two_entry_points():
    from probabilisticteacher_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptmi355.h")).read()
    for name in ("ptmi_nonfinite_scan", "ptmi_seg_nonfinite"):
        assert name in _lib.SIGNATURES and f"int {name}(" in hdr
    assert len(_lib.SIGNATURES["ptmi_nonfinite_scan"][1]) == 8 and len(_lib.SIGNATURES["ptmi_seg_nonfinite"][1]) == 8
