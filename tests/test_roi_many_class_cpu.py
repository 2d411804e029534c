"""Host side of teacher ROI inference with NMS per (image, class) segment (no GPU): the rule that picks the path, the two
bitmask-workspace laws, the class-major segment offsets, and header / binding-table agreement on the new entry points."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ptmi_roi_infer_class_keys", "ptmi_roi_infer_class_nms_boxes", "ptmi_roi_infer_class_collect")


def test_selection_rule():
    from probabilisticteacher_amd.modeling.roi_heads import GuassianFastRCNNOutputLayers, select_nms_by_class as sel
    assert GuassianFastRCNNOutputLayers.nms_by_class is None
    assert sel(8, [2000, 1873]) is False                    # the shipped configs: 16 000 entries, dense
    assert sel(1, [2000]) is False
    assert sel(9, [2000]) is True                           # 18 000 > 16 384
    assert sel(20, [130]) is False and sel(20, [130], True) is True and sel(20, [130], False) is False
    assert sel(8, [2048]) is False and sel(8, [2049]) is True, "16 384 itself is still dense"
    assert sel(9, [2000], False) is False, "False forces the dense path above the automatic range"
    assert sel(8, []) is False and sel(8, [0, 0]) is False
    # the 524 288-box segment limit: K * max R_i on the dense path, max R_i alone by class
    with pytest.raises(ValueError, match="524288"):
        sel(80, [7000], False)
    assert sel(80, [7000]) is True and sel(80, [7000], True) is True
    assert sel(1, [524288], True) is True
    with pytest.raises(ValueError, match="524288"):
        sel(1, [524289], True)
    with pytest.raises(ValueError, match="524288"):
        sel(80, [524289])


def test_workspace_laws():
    from probabilisticteacher_amd.modeling.roi_heads import nms_ws_bytes_by_class as by_class, nms_ws_bytes_dense as dense
    assert dense(1, 8, 2000) == 32_000_000
    assert dense(1, 20, 2000) == 200_000_000 and dense(16, 20, 2000) == 3_200_000_000
    assert dense(1, 80, 2000) == 3_200_000_000 and dense(16, 80, 2000) == 51_200_000_000
    assert dense(2, 80, 2000) == 6_400_000_000
    assert by_class(16, 8, 2000) == 65_536_000
    assert by_class(16, 20, 2000) == 163_840_000
    assert by_class(16, 80, 2000) == 655_360_000
    assert by_class(2, 80, 2000) == 81_920_000
    for n, k, r in ((1, 1, 1), (3, 21, 130), (2, 8, 64), (2, 8, 65)):
        words_c, words_d = -(-r // 64), -(-(k * r) // 64)
        assert by_class(n, k, r) == n * k * r * words_c * 8 and dense(n, k, r) == n * k * r * words_d * 8
        assert by_class(n, 1, r) == dense(n, 1, r), "one class: the two layouts are the same"


def test_workspace_laws_are_what_the_library_allocates():
    """ptmi_nms_ws_bytes (a host function of the library) for the segments each path hands to ptmi_nms_batched"""
    from probabilisticteacher_amd import _lib
    from probabilisticteacher_amd.modeling.roi_heads import nms_ws_bytes_by_class as by_class, nms_ws_bytes_dense as dense
    lib = _lib.load()
    for n, k, r in ((16, 8, 2000), (16, 20, 2000), (2, 80, 2000), (4, 21, 130)):
        assert lib.ptmi_nms_ws_bytes(k * r, n) == dense(n, k, r)
        assert lib.ptmi_nms_ws_bytes(r, n * k) == by_class(n, k, r)


def test_class_segment_offsets():
    from probabilisticteacher_amd import ops
    assert ops.roi_class_seg_offsets([3, 0, 2], 2) == [0, 3, 6, 6, 6, 8, 10]
    counts, k = [130, 0, 65, 1], 21
    offs = ops.roi_class_seg_offsets(counts, k)
    assert len(offs) == len(counts) * k + 1 and offs[-1] == k * sum(counts)
    roff = 0
    for i, c in enumerate(counts):
        for j in range(k):
            assert offs[i * k + j] == k * roff + j * c and offs[i * k + j + 1] - offs[i * k + j] == c
        roff += c
    assert ops.roi_class_seg_offsets([], 5) == [0]


def test_header_and_binding_table_agree_on_the_new_symbols():
    from probabilisticteacher_amd import _lib
    src = open(os.path.join(ROOT, "include", "ptmi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in ptmi355.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        res, args = _lib.SIGNATURES[name]
        want = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            if "*" in p or p.startswith("ptmi_stream_t"):
                want.append(_lib._vp)
            elif p.startswith("int64_t"):
                want.append(_lib._i64)
            elif p.startswith("float"):
                want.append(_lib._f)
            else:
                assert p.startswith("int "), p
                want.append(_lib._i)
        assert res is _lib._i and list(args) == want, f"{name}: binding {args} vs header {m.group(1)}"
        assert hasattr(lib, name)
