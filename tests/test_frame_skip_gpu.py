"""GPU: the tile-list launch of the fused F(4x4, 3x3) forward kernel plus the frame fill against the plain launch -- bit for bit.

The premise under test: a 4x4 output tile whose 6x6 window holds the same bits gets the same output bits wherever it lies, so the
tiles inside the constant frame of a shrink-pasted image can be written from one pattern, which a probe launch of the same kernel
yields.  Nothing here has a tolerance: every comparison is torch.equal on NaN-free tensors, into NaN-poisoned guarded buffers."""
import ctypes
import os

import pytest
import torch

from probabilisticteacher_amd import _lib, ops
from tests.guarded import Guarded, conv_guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n = 3: no ring / a ring / another ring; pasted rectangles at odd offsets (tests/test_frame_skip_cpu.py checks the geometry)
INNER = {(40, 152): ((85, 21, 120, 37), (31, 9, 52, 20)), (48, 333): ((201, 3, 290, 22), (101, 15, 200, 40))}


def _rings(h, w):
    a, b = INNER[(h, w)]
    return torch.tensor([[0] * 8, [0, 0, w, h, *a], [0, 0, w, h, *b]], dtype=torch.int32)


def _framed(x, rings, pattern):
    """x with the pattern written wherever the rings say the input holds it"""
    n, c, h, w = x.shape
    tiled = pattern.repeat(1, -(-h // 4), -(-w // 4))[:, :h, :w]
    for i, r in enumerate(rings.tolist()):
        if r[2] > r[0]:
            m = torch.zeros(h, w, dtype=torch.bool)
            m[r[1]:r[3], r[0]:r[2]] = True
            m[r[5]:r[7], r[4]:r[6]] = False
            x[i][:, m] = tiled[:, m]
    return x


def _layer(cin, cout, gen):
    wt = (torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5).to(DEV)
    b = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    return wt, b


def _plain(x, wp, b, cout, epi):
    n, cin, h, w = x.shape
    y = torch.empty((n, cout, h // 2, w // 2) if epi == 4 else (n, cout, h, w), device=DEV)
    _lib.call("ptmi_conv3x3_wino4p_fwd", ops._ptr(x), ops._ptr(wp), ops._ptr(b), None, ops._ptr(y), n, cin, cout, h, w, epi, ops._stream())
    return y


def _probe(pattern, wp, b, cout, epi):
    frame = ops.FrameState(torch.zeros(1, 8, dtype=torch.int32), pattern)
    ph, pw = ops._FRAME_PROBE_HW

    def run(canvas):
        return _plain(canvas, wp, b, cout, epi)

    return ops._frame_probe(run, frame, None, epi == 4)[0]


def _list_and_fill(x, wp, b, cout, epi, rings, pat_out):
    n, cin, h, w = x.shape
    oh, ow = (h // 2, w // 2) if epi == 4 else (h, w)
    g = Guarded((n, cout, oh, ow), torch.float32, front=conv_guard(oh * ow), back=conv_guard(oh * ow), device=DEV)
    frame = ops.FrameState(rings, None)
    buf, nk, ns = frame.lists(n, h, w, torch.device(DEV))
    assert ns > 0 and nk > 0
    base = buf.data_ptr()
    _lib.call("ptmi_frame_fill", ctypes.c_void_p(base + 4 * (n * 8 + nk)), ns, ctypes.c_void_p(base), ops._ptr(pat_out),
              ops._ptr(g.payload), n, cout, h, w, int(epi == 4), ops._stream())
    _lib.call("ptmi_conv3x3_wino4p_fwd_list", ops._ptr(x), ops._ptr(wp), ops._ptr(b), None, ops._ptr(g.payload), n, cin, cout, h, w,
              epi, ctypes.c_void_p(base + 4 * n * 8), nk, ops._stream())
    torch.cuda.synchronize()
    return g, buf[n * 8 + nk:].cpu().tolist()


@pytest.mark.parametrize("hw", [(40, 152), (48, 333)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("epi", [1, 4])
@pytest.mark.parametrize("chan", [(64, 64), (64, 128), (128, 512)], ids=lambda c: f"{c[0]}to{c[1]}")
def test_list_launch_plus_fill_equals_plain_launch(chan, epi, hw):
    (cin, cout), (h, w), n = chan, hw, 3
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + epi + h)
    rings = _rings(h, w)
    pat_in = torch.randn(cin, 4, 4, generator=gen).abs()
    x = _framed(torch.randn(n, cin, h, w, generator=gen), rings, pat_in).to(DEV)
    wt, b = _layer(cin, cout, gen)
    wp = ops.conv3x3_pack(wt, 0, epi, (h, w))
    want = _plain(x, wp, b, cout, epi)
    assert not torch.isnan(want).any()
    pat_out = _probe(pat_in.to(DEV), wp, b, cout, epi)
    assert pat_out.shape == (cout, 4, 4)
    g, skipped = _list_and_fill(x, wp, b, cout, epi, rings, pat_out)
    g.assert_guards_intact("y")
    assert g.unwritten() == 0, "list launch + fill left output elements unwritten"
    assert torch.equal(g.payload, want), f"{int((g.payload != want).sum())} elements differ from the plain launch"
    g2, _ = _list_and_fill(x, wp, b, cout, epi, rings, pat_out)
    assert torch.equal(g2.payload, g.payload)
    g2.assert_guards_intact("y (second run)")
    # the probe's pattern IS what the plain launch computes in the frame: first tile of the first skipped pixel tile
    lib = _lib.load()
    bands, period = -(-h // 8), (w + 4) & ~3
    u = skipped[0] * 64
    sf = u // period
    sn, py, px = sf // bands, (sf % bands) * 8, u - sf * period
    assert lib.ptmi_frame_tile_skippable(ctypes.c_void_p(rings[sn].contiguous().data_ptr()), h, w, py, px)
    if epi == 4:
        tile = want[sn, :, py // 2:py // 2 + 2, px // 2:px // 2 + 2]
        ref = pat_out.repeat(1, 2, 2)[:, (py // 2) & 3:, (px // 2) & 3:][:, :2, :2]
    else:
        tile, ref = want[sn, :, py:py + 4, px:px + 4], pat_out
    assert torch.equal(tile, ref)


def _count_calls(monkeypatch):
    seen = []
    real = _lib.call

    def spy(name, *a):
        seen.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    return seen


@pytest.mark.parametrize("fused_pool", [False, True], ids=["conv_pool_conv", "convpool_conv"])
def test_two_layer_chain_with_a_pool_between(monkeypatch, fused_pool):
    """ring propagation end to end through the ops layer: conv (64 -> 64), 2x2 pool (its own kernel or epilogue 4), conv (64 -> 128),
    with the frame state against without it"""
    monkeypatch.setattr(ops, "_FRAME_MIN_SHARE", 0.0)
    h, w, n = 48, 333, 3
    gen = torch.Generator().manual_seed(5)
    rings = _rings(h, w)
    pat_in = torch.randn(64, 4, 4, generator=gen).abs()
    x = _framed(torch.randn(n, 64, h, w, generator=gen), rings, pat_in).to(DEV)
    (w1, b1), (w2, b2) = _layer(64, 64, gen), _layer(64, 128, gen)

    def chain(frame, alive=True):
        with torch.no_grad():
            if fused_pool:
                y = ops.conv3x3_relu_pool_nograd(x, w1, b1, frame)
            else:
                y = ops.conv3x3(x, w1, b1, True, frame)
                y = ops.maxpool2x2(y)
                ops.frame_pool(frame, h, w)
            assert frame is None or frame.alive == alive
            return ops.conv3x3(y, w2, b2, True, frame)

    want = chain(None)
    seen = _count_calls(monkeypatch)
    got = chain(ops.FrameState(rings, pat_in.to(DEV), ("test", 0)))
    assert seen.count("ptmi_conv3x3_wino4p_fwd_list") == 2 and seen.count("ptmi_frame_fill") == 2, seen
    assert not torch.isnan(want).any() and torch.equal(got, want)
    ops.set_frame_skip(False)
    try:
        del seen[:]
        off = chain(ops.FrameState(rings, pat_in.to(DEV), ("test", 0)), alive=False)
        assert "ptmi_conv3x3_wino4p_fwd_list" not in seen and torch.equal(off, want)
    finally:
        ops.set_frame_skip(True)


def _run_steps(skip: bool, seen=None):
    from bench import synth_records
    from probabilisticteacher_amd.config import setup_cfg
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    cfg = setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "MODEL.ANCHOR_GENERATOR.NAME", "DifferentiableAnchorGenerator",
        "UNSUPNET.BURN_UP_STEP", 1, "SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEED", 3])
    gen = torch.Generator().manual_seed(77)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    batches = [tuple(synth_records(gen, 2, 192, 256, K, DEV) for _ in range(4)) for _ in range(2)]
    ops.set_frame_skip(skip)
    try:
        seed_all_rng(3)
        tr = PTrainer(cfg)
        metrics = []
        for b in batches:                      # one burn-in step, one mutual-learning step (the joint student pass)
            m = dict(tr.run_step(b))
            m.pop("data_time", None)
            metrics.append(m)
        torch.cuda.synchronize()
    finally:
        ops.set_frame_skip(True)
    return metrics, tr.student.grad.clone(), tr.student.flat.clone()


def test_run_step_is_bit_identical_with_and_without_skipping(monkeypatch):
    monkeypatch.setattr(ops, "_FRAME_MIN_SHARE", 0.0)          # (every layer with a skippable tile takes the list launch)
    seen = _count_calls(monkeypatch)
    on = _run_steps(True)
    lists = seen.count("ptmi_conv3x3_wino4p_fwd_list")
    assert lists > 0 and seen.count("ptmi_frame_fill") == lists, "no layer took the list launch: the comparison would be empty"
    del seen[:]
    off = _run_steps(False)
    assert "ptmi_conv3x3_wino4p_fwd_list" not in seen
    for i, (a, b) in enumerate(zip(on[0], off[0])):
        assert a.keys() == b.keys() and len(a) >= 4
        diff = {k: (a[k], b[k]) for k in a if not (a[k] == b[k])}
        assert not diff, f"step {i}: metrics differ with / without skipping: {diff}"
    assert torch.equal(on[1], off[1]), "student.grad differs"
    assert torch.equal(on[2], off[2]), "student.flat differs"


# ---------------------------------------------------------------------------- the branches of the forward launcher, one by one
SCHED, LIST, FILL = "ptmi_conv3x3_wino4p_fwd_sched", "ptmi_conv3x3_wino4p_fwd_list", "ptmi_frame_fill"


def _ring_next(rings, op, h, w):
    nxt = torch.empty_like(rings)
    _lib.call("ptmi_frame_ring_next", ctypes.c_void_p(rings.data_ptr()), ctypes.c_void_p(nxt.data_ptr()), int(rings.shape[0]), op, h, w)
    return nxt


def _case(cin, h, w, seed, n=3):
    """(rings, input pattern on the device, framed input)"""
    gen = torch.Generator().manual_seed(seed)
    rings = _rings(h, w)
    pat = torch.randn(cin, 4, 4, generator=gen).abs()
    return gen, rings, pat.to(DEV), _framed(torch.randn(n, cin, h, w, generator=gen), rings, pat).to(DEV)


def test_unsupported_kind_ends_the_frame(monkeypatch):
    monkeypatch.setattr(ops, "_FRAME_CACHE", {})
    h, w = 40, 152
    assert ops._conv_kind(32, 32, (h, w)) == "wino"
    gen, rings, pat, x = _case(32, h, w, 11)
    wt, b = _layer(32, 32, gen)
    with torch.no_grad():
        want = ops.conv3x3(x, wt, b, True, None)
        seen = _count_calls(monkeypatch)
        frame = ops.FrameState(rings, pat, ("test", 0))
        got = ops.conv3x3(x, wt, b, True, frame)
    assert not torch.isnan(want).any() and torch.equal(got, want)
    assert frame.alive is False
    assert seen.count("ptmi_conv3x3_wino_fwd") == 1, seen               # the layer; no probe
    assert LIST not in seen and FILL not in seen and SCHED not in seen and "ptmi_conv3x3_fwd" not in seen, seen


def test_stem_then_a_wino4_layer(monkeypatch):
    monkeypatch.setattr(ops, "_FRAME_CACHE", {})
    monkeypatch.setattr(ops, "_FRAME_MIN_SHARE", 0.0)
    h, w = 48, 333
    assert ops._conv_kind(3, 64, (h, w)) == "mfma"
    gen, rings, pat, x = _case(3, h, w, 12)
    (w1, b1), (w2, b2) = _layer(3, 64, gen), _layer(64, 64, gen)
    with torch.no_grad():
        want = ops.conv3x3(ops.conv3x3(x, w1, b1, True, None), w2, b2, True, None)
        seen = _count_calls(monkeypatch)
        frame = ops.FrameState(rings, pat, ("test", 0))
        y = ops.conv3x3(x, w1, b1, True, frame)
        assert seen.count("ptmi_conv3x3_fwd") == 2, seen                 # the probe canvas, then the layer
        assert LIST not in seen and FILL not in seen, seen
        assert frame.alive is True
        assert torch.equal(frame.rings, _ring_next(rings, 0, h, w))
        assert frame.pattern.shape == (64, 4, 4)
        del seen[:]
        got = ops.conv3x3(y, w2, b2, True, frame)
    assert seen.count(LIST) == 1 and seen.count(FILL) == 1, seen
    assert not torch.isnan(want).any() and torch.equal(got, want)


def test_share_below_the_bar_takes_the_plain_launch(monkeypatch):
    monkeypatch.setattr(ops, "_FRAME_CACHE", {})
    monkeypatch.setattr(ops, "_FRAME_MIN_SHARE", 0.99)
    h, w = 48, 333
    gen, rings, pat, x = _case(64, h, w, 13)
    wt, b = _layer(64, 64, gen)
    with torch.no_grad():
        want = ops.conv3x3(x, wt, b, True, None)
        seen = _count_calls(monkeypatch)
        frame = ops.FrameState(rings, pat, ("test", 0))
        got = ops.conv3x3(x, wt, b, True, frame)
    assert not torch.isnan(want).any() and torch.equal(got, want)
    assert seen.count(SCHED) == 2, seen                                  # one probe, one plain launch of the layer
    assert LIST not in seen and FILL not in seen, seen
    assert frame.alive is False


@pytest.mark.parametrize("with_frame", [True, False], ids=["frame", "no_frame"])
def test_pack_mismatch_raises_before_any_launch(monkeypatch, with_frame):
    monkeypatch.setattr(ops, "_FRAME_CACHE", {})
    h, w = 48, 333
    gen, rings, pat, x = _case(64, h, w, 14)
    wt, b = _layer(64, 64, gen)
    wp = ops.conv3x3_pack(wt, 0, 1, (h, w))
    wrong = torch.zeros(wp.numel() + 1, device=DEV)
    frame = ops.FrameState(rings, pat, ("test", 0)) if with_frame else None
    seen = _count_calls(monkeypatch)
    with pytest.raises(_lib.PtmiError, match="packed weights"):
        ops.conv3x3_raw(x, wrong, b, None, 64, 1, frame, None)
    assert seen == []


def test_probe_cache(monkeypatch):
    """a frozen layer behind a keyed pattern probes once; a new parameter version, or a pattern without a key, probes again.  The
    first call is the probe (one plain launch, of the canvas) and the list + fill of the layer -- no second plain launch."""
    monkeypatch.setattr(ops, "_FRAME_CACHE", {})
    monkeypatch.setattr(ops, "_FRAME_MIN_SHARE", 0.0)
    h, w = 40, 152
    gen, rings, pat, x = _case(64, h, w, 15)
    wt, b = _layer(64, 64, gen)
    assert not wt.requires_grad and not b.requires_grad
    want = ops.conv3x3(x, wt, b, True, None)
    assert not torch.isnan(want).any()
    seen = _count_calls(monkeypatch)

    def call(key, probes):
        del seen[:]
        frame = ops.FrameState(rings, pat, key)
        got = ops.conv3x3(x, wt, b, True, frame)
        assert (seen.count(SCHED), seen.count(LIST), seen.count(FILL)) == (probes, 1, 1), seen
        assert torch.equal(got, want)
        return frame

    assert call(("test", 0), 1).key is not None
    assert len(ops._FRAME_CACHE) == 1
    call(("test", 0), 0)
    wt.mul_(1.0)                                   # same values, next version
    call(("test", 0), 1)
    call(("test", 0), 0)
    assert call(None, 1).key is None
    call(None, 1)
    assert len(ops._FRAME_CACHE) == 2


def test_fused_pool_advances_through_conv_and_pool(monkeypatch):
    monkeypatch.setattr(ops, "_FRAME_CACHE", {})
    h, w = 48, 333
    gen, rings, pat, x = _case(64, h, w, 16)
    wt, b = _layer(64, 64, gen)
    want = ops.conv3x3_relu_pool_nograd(x, wt, b, None)
    frame = ops.FrameState(rings, pat, ("test", 0))
    got = ops.conv3x3_relu_pool_nograd(x, wt, b, frame)
    assert not torch.isnan(want).any() and torch.equal(got, want)
    assert torch.equal(frame.rings, _ring_next(_ring_next(rings, 2, h, w), 1, h, w))
    assert frame.pattern.shape == (64, 4, 4)
    assert frame.key is not None
