"""CPU: the ROI pooler variants (MODEL.ROI_BOX_HEAD.POOLER_TYPE / POOLER_SAMPLING_RATIO).

(1) the numpy restatement the GPU tests compare against (tests/roi_pooler_ref.py) is pinned to the oracle the project already
    trusts: with aligned=True, sampling_ratio=0 it equals oracle.d2.roi_align at 1e-6 on the box set of test_ops_gpu.py::test_roi_align;
(2) hand-checkable ROIPool cases; (3) ROIPooler's validation of the two config keys."""
import numpy as np
import pytest
import torch

from oracle import d2
from tests import roi_pooler_ref as ref
from tests.helpers import close


# ============================================================================ (1) the restatement vs the trusted oracle
@pytest.mark.parametrize("fh,fw", [(25, 31), (70, 27), (83, 83)])
def test_restatement_equals_the_oracle_for_roialignv2(fh, fw):
    gen = torch.Generator().manual_seed(23)
    feat = torch.randn(2, 18, fh, fw, generator=gen)
    rois = ref.special_boxes(gen, 40, fh, fw)
    assert float((rois[:, 3] - rois[:, 1]).min()) < 16.0            # the tiny box
    want = d2.roi_align(feat, rois, 7, 1 / 16).numpy()
    got = ref.roi_align(feat.numpy(), rois.numpy(), 7, 1 / 16, aligned=True, sampling_ratio=0)
    close(got, want, 1e-6, 1e-6, "restatement (aligned, ratio 0) vs oracle.d2.roi_align")
    # and its float64 backward against the oracle's fp32 one (the existing test's backward tolerance)
    gy = torch.randn(want.shape, generator=gen)
    fr = feat.clone().requires_grad_()
    d2.roi_align(fr, rois, 7, 1 / 16).backward(gy)
    gb = ref.roi_align_backward(gy.numpy(), rois.numpy(), feat.shape, 7, 1 / 16)
    close(fr.grad.numpy(), gb, 1e-4, 1e-4, "restatement backward vs oracle")


def test_restatement_variants_by_hand():
    """one 1-channel ramp f(y, x) = 10 y + x: bilinear interpolation of a ramp is the ramp, so a bin's value is the mean of its
    sample positions"""
    H = W = 8
    feat = (10.0 * np.arange(H)[:, None] + np.arange(W)[None, :]).astype(np.float32)[None, None]
    roi = np.array([[0, 1.0, 2.0, 5.0, 6.0]], np.float32)          # scale 1: a 4 x 4 box, P = 2: 2 x 2 bins
    # not aligned, one sample per bin: bin centres at x = 1 + {1, 3}, y = 2 + {1, 3}
    got = ref.roi_align(feat, roi, 2, 1.0, aligned=False, sampling_ratio=1)[0, 0]
    np.testing.assert_allclose(got, [[32.0, 34.0], [52.0, 54.0]], rtol=0, atol=1e-5)
    # aligned: everything moves by -0.5 in x and y
    got = ref.roi_align(feat, roi, 2, 1.0, aligned=True, sampling_ratio=1)[0, 0]
    np.testing.assert_allclose(got, [[26.5, 28.5], [46.5, 48.5]], rtol=0, atol=1e-5)
    # a 2 x 2 grid's mean is the bin centre again
    got = ref.roi_align(feat, roi, 2, 1.0, aligned=False, sampling_ratio=2)[0, 0]
    np.testing.assert_allclose(got, [[32.0, 34.0], [52.0, 54.0]], rtol=0, atol=1e-5)
    # not aligned: a box narrower than one cell is one cell wide (x in [3, 4], one bin, one sample at 3.5), the aligned one is not
    thin = np.array([[0, 3.0, 2.0, 3.25, 3.0]], np.float32)
    assert abs(ref.roi_align(feat, thin, 1, 1.0, aligned=False, sampling_ratio=1)[0, 0, 0, 0] - 28.5) < 1e-5
    assert abs(ref.roi_align(feat, thin, 1, 1.0, aligned=True, sampling_ratio=1)[0, 0, 0, 0] - (20.0 + 2.625)) < 1e-5
    # backward: the taps of one sample carry g / count in total
    g = ref.roi_align_backward(np.ones((1, 1, 2, 2)), roi, feat.shape, 2, 1.0, aligned=False, sampling_ratio=2)
    assert abs(g.sum() - 4.0) < 1e-6


# ============================================================================ (2) ROIPool by hand
def _ramp(H, W):
    return np.arange(H * W, dtype=np.float32).reshape(1, 1, H, W)


def test_roi_pool_one_cell_roi():
    feat = _ramp(6, 8)
    out, arg = ref.roi_pool(feat, np.array([[0, 3.0, 2.0, 3.0, 2.0]], np.float32), 2, 1.0)
    # rw = rh = 1, bin size 0.5: every bin is [floor(p / 2), ceil((p + 1) / 2)) = the one cell (2, 3)
    assert (out == feat[0, 0, 2, 3]).all() and (arg == 2 * 8 + 3).all()


def test_roi_pool_roi_outside_the_map_is_empty():
    feat = _ramp(6, 8)
    rois = np.array([[0, 20.0, 30.0, 25.0, 36.0], [0, -40.0, -30.0, -20.0, -10.0]], np.float32)
    out, arg = ref.roi_pool(feat, rois, 3, 1.0)
    assert (out == 0).all() and (arg == -1).all()
    g = ref.roi_pool_backward(np.ones_like(out), arg, rois, feat.shape)
    assert not g.any()


def test_roi_pool_rounds_half_away_from_zero():
    assert [ref._roundf(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 2.4999, 0.49999997)] == [1, 2, 3, -1, -2, 2, 0]
    feat = _ramp(6, 8)
    # x1 * s = 2.5 -> 3 (round-half-even would give 2), x2 * s = 4.5 -> 5; y1 * s = 0.5 -> 1, y2 * s = 1.5 -> 2
    roi = np.array([[0, 5.0, 1.0, 9.0, 3.0]], np.float32)
    hb, wb = ref.roi_pool_bins(roi[0], 1, 0.5, 6, 8)
    assert hb == [(1, 3)] and wb == [(3, 6)]
    out, arg = ref.roi_pool(feat, roi, 1, 0.5)
    assert out[0, 0, 0, 0] == feat[0, 0, 2, 5] and arg[0, 0, 0, 0] == 2 * 8 + 5
    # a negative corner: -2.5 -> -3, so rw = 3 - (-3) + 1 = 7 and the single bin is [-3, 4) clamped to [0, 4)
    hb, wb = ref.roi_pool_bins(np.array([0, -5.0, 0.0, 6.0, 0.0], np.float32), 1, 0.5, 6, 8)
    assert wb == [(0, 4)] and hb == [(0, 1)]


def test_roi_pool_bins_overlap_by_one_row():
    feat = _ramp(6, 8)
    # rows 1..3 (rh = 3) in two bins: bh = 1.5: [floor(0), ceil(1.5)) = rows 1..2 and [floor(1.5), ceil(3)) = rows 2..3
    roi = np.array([[0, 0.0, 1.0, 7.0, 3.0]], np.float32)
    hb, wb = ref.roi_pool_bins(roi[0], 2, 1.0, 6, 8)
    assert hb == [(1, 3), (2, 4)] and wb == [(0, 4), (4, 8)]
    feat[0, 0, 2, 1] = 1000.0                     # a cell of the shared row wins both bins of the left column
    out, arg = ref.roi_pool(feat, roi, 2, 1.0)
    assert arg[0, 0, 0, 0] == arg[0, 0, 1, 0] == 2 * 8 + 1 and out[0, 0, 0, 0] == out[0, 0, 1, 0] == 1000.0
    assert arg[0, 0, 0, 1] == 2 * 8 + 7 and arg[0, 0, 1, 1] == 3 * 8 + 7
    g = ref.roi_pool_backward(np.full((1, 1, 2, 2), 0.5), arg, roi, feat.shape)
    assert g[0, 0, 2, 1] == 1.0 and g[0, 0, 2, 7] == 0.5 and g[0, 0, 3, 7] == 0.5 and g.sum() == 2.0


def test_roi_pool_first_maximum_wins():
    feat = np.zeros((1, 1, 4, 4), np.float32)
    feat[0, 0, 1:3, 1:3] = 7.0                    # a plateau: the first cell in raster order is (1, 1)
    out, arg = ref.roi_pool(feat, np.array([[0, 0.0, 0.0, 3.0, 3.0]], np.float32), 1, 1.0)
    assert out[0, 0, 0, 0] == 7.0 and arg[0, 0, 0, 0] == 1 * 4 + 1


# ============================================================================ (3) ROIPooler validation
def test_pooler_validation_names_the_key():
    from probabilisticteacher_amd.modeling.roi_heads import ROIPooler
    for bad in ("ROIAlignRotated", "roialign", ""):
        with pytest.raises(ValueError, match="POOLER_TYPE"):
            ROIPooler(7, (1 / 16,), 0, bad)
    for t in ("ROIAlignV2", "ROIAlign", "ROIPool"):
        with pytest.raises(ValueError, match="POOLER_SAMPLING_RATIO"):
            ROIPooler(7, (1 / 16,), -1, t)
    with pytest.raises(ValueError, match="multi-level"):
        ROIPooler(7, (1 / 4, 1 / 8, 1 / 16), 0, "ROIAlignV2")
    with pytest.raises(ValueError, match="multi-level"):
        ROIPooler(7, (), 0, "ROIAlign")


@pytest.mark.parametrize("ptype,ratio", [("ROIAlignV2", 0), ("ROIAlignV2", 2), ("ROIAlign", 0), ("ROIAlign", 2), ("ROIPool", 0),
                                         ("ROIPool", 2)])
def test_accepted_poolers_construct_on_cpu_without_the_library(monkeypatch, tmp_path, ptype, ratio):
    from probabilisticteacher_amd import _lib, modeling
    from probabilisticteacher_amd.config import setup_cfg
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "absent.so"))        # any load() would raise
    monkeypatch.setattr(_lib, "_lib", None)
    cfg = setup_cfg("configs/pt/final_c2f.yaml", ["MODEL.DEVICE", "cpu", "MODEL.VGG.PRETRAIN", "",
                                                  "MODEL.ROI_BOX_HEAD.POOLER_TYPE", ptype,
                                                  "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", ratio])
    model = modeling.build_model(cfg)
    pooler = model.roi_heads.box_pooler
    assert (pooler.pooler_type, pooler.sampling_ratio, pooler.output_size) == (ptype, ratio, 7)
    assert pooler.defers == (ptype == "ROIAlignV2" and ratio == 0)             # the fused bf16 hand-over is ROIAlignV2 / ratio 0 only


def test_bad_pooler_config_fails_at_model_construction():
    from probabilisticteacher_amd import modeling
    from probabilisticteacher_amd.config import setup_cfg
    base = ["MODEL.DEVICE", "cpu", "MODEL.VGG.PRETRAIN", ""]
    with pytest.raises(ValueError, match="POOLER_TYPE"):
        modeling.build_model(setup_cfg("configs/pt/final_c2f.yaml", base + ["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIAlignRotated"]))
    with pytest.raises(ValueError, match="POOLER_SAMPLING_RATIO"):
        modeling.build_model(setup_cfg("configs/pt/final_c2f.yaml", base + ["MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", -2]))
