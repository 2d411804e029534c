"""GPU guard-band tests (pytest -m gpu) of the convolution family through the C ABI: every operand of every launch is the payload of
a tests/guarded.py buffer, so besides the usual parity (float64 conv2d / autograd) each launch is checked for what the parity
tests cannot see:

  * nothing before or after an output (y, dW, db, a packed-weight buffer, a split workspace of EXACTLY the queried size) was
    written -- the store paths drop channels >= Cout, rows >= H, columns >= W and pooled rows / columns at the floor edge either
    through the buffer descriptor's range check or through one predicate;
  * every element of an output was written (`unwritten() == 0`);
  * the read-only operands (x, packed weights, bias, mask, dy; the schedule words apart from their re-arming to zero) come back
    bit-identical, guards included.

The shapes are the smallest at which each predicate is live (see the comments on the lists).  What a guard can see is bounded by
its size (tests/guarded.py): one 128-channel tile of output planes on each side of a convolution output."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.guarded import Guarded, conv_guard
from tests.test_p8_gpu import bf16_close, pads_are_zero, rb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


def g(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, rtol, atol, what=""):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    err = np.abs(a - b)                                  # (a payload element still holding the NaN fill fails here too)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max abs err {np.nanmax(err):.3e}, max |ref| {np.abs(b).max():.3e}, " \
                               f"{int((~(err <= tol)).sum())} of {err.size} off, first at {np.argwhere(~(err <= tol))[0]}"


def _api():
    from probabilisticteacher_amd import _lib, ops
    return _lib, _lib.load(), ops._ptr, ops._stream


def _ro(t, guard=4096):
    """a read-only operand: guarded copy on the device + snapshot"""
    return Guarded.of(t, guard, guard, DEV).snapshot()


def _ptr_of(gd):
    from probabilisticteacher_amd import ops
    return ops._ptr(None if gd is None else gd.payload)


def _after_launch(outs, ros, what):
    """the per-launch assertions that are not parity: outs = {name: (Guarded, must_be_fully_written)}, ros = {name: Guarded}"""
    torch.cuda.synchronize()
    for name, (o, full) in outs.items():
        o.assert_guards_intact(f"{what}: {name}")
        if full:
            assert o.unwritten() == 0, f"{what}: {o.unwritten()} of {o.numel} elements of {name} were never written"
    for name, r in ros.items():
        if r is not None:
            r.assert_unchanged(f"{what}: {name}")


def test_the_helper_sees_a_planted_stray_on_the_device():
    """tests/test_guarded_cpu.py on the device in one case: a channel plane written one plane past the end of y, a never-written
    element and a modified input are all reported (the assertions below are what every test of this file leans on)"""
    y = Guarded((1, 3, 4, 5), F32, conv_guard(20), conv_guard(20), DEV)
    y.payload.zero_()
    y.payload.view(-1)[7] = float("nan")
    y.assert_guards_intact("clean")
    assert y.unwritten() == 0
    y.raw.view(F32)[y.front + y.numel + 20: y.front + y.numel + 40] = 0.0           # "channel 4" of a 3-channel output
    with pytest.raises(AssertionError, match=r"20 guard element\(s\) overwritten \(0 before, 20 after.*nearest at \+21, farthest at \+40"):
        y.assert_guards_intact("planted")
    y.payload.view(torch.int32)[0, 2, 3, 4] = y.raw.view(torch.int32)[0]
    assert y.unwritten() == 1
    x = _ro(torch.ones(2, 8))
    x.payload[1, 7] = 2.0
    with pytest.raises(AssertionError, match="first at payload index 15"):
        x.assert_unchanged("x")


# =================================================================================================== fp32 forward and dgrad
FAMS = {"direct": "ptmi_conv3x3", "wino": "ptmi_conv3x3_wino", "wino4": "ptmi_conv3x3_wino4", "wino4p": "ptmi_conv3x3_wino4p"}

FWD_SHAPES = [  # n, cin, cout, h, w
    (1, 24, 70, 11, 17),      # Cout not a multiple of any channel tile, ONE image: nothing later repairs a channel overrun
    (1, 40, 130, 1, 70),      # the same, a single row
    (2, 24, 70, 5, 9),        # the same with a second image: an overrun of image 0 races with image 1's rightful writer
    (3, 32, 64, 4, 3),        # narrower than one 16-byte piece
    (1, 8, 7, 2, 1),          # one column
    (2, 64, 128, 19, 35),     # odd H and W: pooled rows / columns at the floor edge, workgroups straddling images
    (3, 16, 48, 7, 21),
    (2, 32, 128, 3, 333),     # right-edge pieces straddling the image edge
]
DIRECT_ONLY = [
    (2, 3, 64, 37, 45),       # the stem path
    (1, 20, 70, 11, 17),      # Cin not a multiple of 8 (the Winograd F(4x4) kernels do not serve it), ragged Cout
    (1, 16, 64, 9, 701),      # the wide-map variant (W >= 600)
]
FWD_CASES = [(f, s) for f in FAMS for s in FWD_SHAPES] + [("direct", s) for s in DIRECT_ONLY]
_ids = [f"{f}-{'x'.join(map(str, s))}" for f, s in FWD_CASES]


@functools.lru_cache(maxsize=None)
def _case(n, cin, cout, h, w):
    """inputs and float64 references of one shape, computed once and shared by the families (unit-scale outputs)"""
    gen = g(n * 1000 + cin * 7 + cout * 3 + h * 11 + w)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cin))
    b = torch.randn(cout, generator=gen) * 0.1
    gy = torch.randn(n, cout, h, w, generator=gen) * math.sqrt(cin / (2.0 * cout))      # dX of unit scale
    mask = torch.randn(n, cin, h, w, generator=gen)                                     # "activation of the producing layer"
    ref = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    xr = x.double().requires_grad_()
    F.conv2d(xr, wt.double(), None, padding=1).backward(gy.double())
    return dict(x=x, wt=wt, b=b, gy=gy, mask=mask, ref=ref, dx=xr.grad)


def _fits(fam, cin, cout, h, w):
    _, lib, _, _ = _api()
    return True if fam == "direct" else bool(getattr(lib, f"{FAMS[fam]}_fwd_fits")(cin, cout, h, w))


def _pack(fam, wt_g, mode):
    """<family>_pack_weights under guards: the packed buffer holds exactly <family>_packed_floats floats"""
    _lib, lib, ptr, stream = _api()
    co, ci = wt_g.shape[0], wt_g.shape[1]
    conv_cin, conv_cout = (ci, co) if mode == 0 else (co, ci)
    wp = Guarded((getattr(lib, f"{FAMS[fam]}_packed_floats")(conv_cin, conv_cout),), F32, 4096, 4096, DEV)
    _lib.call(f"{FAMS[fam]}_pack_weights", _ptr_of(wt_g), _ptr_of(wp), co, ci, mode, stream())
    _after_launch({"packed weights": (wp, True)}, {"w": wt_g}, f"{fam} pack mode {mode}")
    return wp.snapshot()


def _fwd(fam, xg, wp, bias, mask, n, cin, cout, h, w, epi, ref, what, sched=None):
    """one guarded launch of <family>_fwd (or _fwd_sched) + every assertion"""
    _lib, _, ptr, stream = _api()
    oh, ow = (h // 2, w // 2) if epi == 4 else (h, w)
    guard = conv_guard(oh * ow)
    y = Guarded((n, cout, oh, ow), F32, guard, guard, DEV)
    args = [_ptr_of(xg), _ptr_of(wp), _ptr_of(bias), _ptr_of(mask), _ptr_of(y), n, cin, cout, h, w, epi]
    if sched is None:
        _lib.call(f"{FAMS[fam]}_fwd", *args, stream())
    else:
        _lib.call(f"{FAMS[fam]}_fwd_sched", *args, _ptr_of(sched), stream())
    _after_launch({"y": (y, True)}, {"x": xg, "packed weights": wp, "bias": bias, "mask": mask}, what)
    close(y.payload, ref, 1e-4, 1e-4, what)


@pytest.mark.parametrize("fam,shape", FWD_CASES, ids=_ids)
def test_forward_writes_its_output_and_nothing_else(fam, shape):
    """epilogues 0 (bias), 1 (+ ReLU), 2 (none), 4 (+ ReLU + 2x2 max-pool into the (h // 2, w // 2) tensor)"""
    n, cin, cout, h, w = shape
    if not _fits(fam, cin, cout, h, w):
        pytest.skip(f"{FAMS[fam]}_fwd_fits({cin}, {cout}, {h}, {w}) == 0")
    c = _case(*shape)
    xg, bg = _ro(c["x"]), _ro(c["b"])
    wp = _pack(fam, _ro(c["wt"]), 0)
    ref = c["ref"]
    _fwd(fam, xg, wp, bg, None, n, cin, cout, h, w, 0, ref, f"{fam} {shape} epilogue 0")
    _fwd(fam, xg, wp, bg, None, n, cin, cout, h, w, 1, F.relu(ref), f"{fam} {shape} epilogue 1")
    _fwd(fam, xg, wp, None, None, n, cin, cout, h, w, 2, ref - c["b"].double().view(1, -1, 1, 1), f"{fam} {shape} epilogue 2")
    if h >= 2 and w >= 2:
        _fwd(fam, xg, wp, bg, None, n, cin, cout, h, w, 4, F.max_pool2d(F.relu(ref), 2, 2), f"{fam} {shape} epilogue 4")


@pytest.mark.parametrize("fam,shape", FWD_CASES, ids=_ids)
def test_dgrad_writes_its_output_and_nothing_else(fam, shape):
    """pack mode 1 (dX = conv(dY, W^T flipped): the conv's input channels are W's Cout) with epilogues 2 (plain) and 3 (times the
    producer's ReLU mask, a read-only operand of y's shape)"""
    n, cin, cout, h, w = shape
    if not _fits(fam, cout, cin, h, w):
        pytest.skip(f"{FAMS[fam]}_fwd_fits({cout}, {cin}, {h}, {w}) == 0")
    c = _case(*shape)
    gyg, mg = _ro(c["gy"]), _ro(c["mask"])
    wp = _pack(fam, _ro(c["wt"]), 1)
    _fwd(fam, gyg, wp, None, None, n, cout, cin, h, w, 2, c["dx"], f"{fam} {shape} dgrad epilogue 2")
    _fwd(fam, gyg, wp, None, mg, n, cout, cin, h, w, 3, c["dx"] * (c["mask"] > 0), f"{fam} {shape} dgrad epilogue 3")


@pytest.mark.parametrize("fam", ["wino4", "wino4p"])
def test_dynamic_schedule_under_guards(fam):
    """<family>_fwd_sched with a live schedule buffer that is itself guarded: the 16 words are zero again after every launch (their
    documented re-arming) and nothing around them is touched"""
    shape = (2, 64, 128, 19, 35)
    n, cin, cout, h, w = shape
    c = _case(*shape)
    xg, bg = _ro(c["x"]), _ro(c["b"])
    wp = _pack(fam, _ro(c["wt"]), 0)
    sched = Guarded((16,), torch.int32, 4096, 4096, DEV)
    sched.payload.zero_()
    sched.snapshot()
    ref = c["ref"]
    for epi, bias, want in ((1, bg, F.relu(ref)), (2, None, ref - c["b"].double().view(1, -1, 1, 1)),
                            (4, bg, F.max_pool2d(F.relu(ref), 2, 2))):
        what = f"{fam}_fwd_sched {shape} epilogue {epi}"
        _fwd(fam, xg, wp, bias, None, n, cin, cout, h, w, epi, want, what, sched=sched)
        sched.assert_guards_intact(what + ": sched")
        sched.assert_unchanged(what + ": sched (re-armed to zero)")


# =================================================================================================== bf16-storage (P8) convolution
P8_SHAPES = [(3, 16, 8, 4, 3), (1, 48, 72, 9, 83), (1, 16, 24, 1, 1), (2, 64, 64, 24, 40)]


def _p8_shape(c, n, h, w):
    return (2 * (-(-c // 16)), n * (h + 1) + 1, w + 1, 8)


def _p8_from_nchw(t, ro=True):
    """ptmi_p8_from_nchw into a guarded P8 buffer"""
    _lib, _, ptr, stream = _api()
    n, c, h, w = t.shape
    src = _ro(t)
    guard = conv_guard((n * (h + 1) + 1) * (w + 1))
    dst = Guarded(_p8_shape(c, n, h, w), BF16, guard, guard, DEV)
    _lib.call("ptmi_p8_from_nchw", _ptr_of(src), _ptr_of(dst), n, c, h, w, stream())
    _after_launch({"P8 tensor": (dst, True)}, {"nchw source": src}, f"p8_from_nchw {tuple(t.shape)}")
    pads_are_zero(dst.payload, n, h, w)
    return dst.snapshot() if ro else dst


@functools.lru_cache(maxsize=None)
def _p8_case(n, cin, cout, h, w):
    gen = g(5 + n * 1000 + cin * 7 + cout * 3 + h * 11 + w)
    x = rb(torch.randn(n, cin, h, w, generator=gen))
    wt = rb(torch.randn(cout, cin, 3, 3, generator=gen) * math.sqrt(2.0 / (9 * cin)))
    b = torch.randn(cout, generator=gen) * 0.1
    act = rb(torch.relu(torch.randn(n, cout, h, w, generator=gen)))          # epilogue 3's mask: a post-ReLU activation, exact zeros
    lin = F.conv2d(x.double(), wt.double(), None, padding=1)
    return dict(x=x, wt=wt, b=b, act=act, lin=lin)


@pytest.mark.parametrize("entry,waves", [("ptmi_p8_conv3x3", None), ("ptmi_p8_conv3x3_waves", 16)])
@pytest.mark.parametrize("shape", P8_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_p8_conv_writes_its_output_and_nothing_else(shape, entry, waves):
    """epilogues 0 .. 3 and the pooling epilogue 4 on guarded P8 buffers; the stored value against a float64 convolution of the
    bf16-rounded operands at the bf16-storage bar of tests/test_p8_gpu.py; pad rows and columns of y are zeros"""
    _lib, lib, ptr, stream = _api()
    from probabilisticteacher_amd import p8
    n, cin, cout, h, w = shape
    c = _p8_case(*shape)
    xp, mp, bg = _p8_from_nchw(c["x"]), _p8_from_nchw(c["act"]), _ro(c["b"])
    wt_g = _ro(c["wt"])
    wp = Guarded((lib.ptmi_p8_packed_elems(cin, cout),), BF16, 4096, 4096, DEV)
    _lib.call("ptmi_p8_pack_weights", _ptr_of(wt_g), _ptr_of(wp), cout, cin, 0, stream())
    _after_launch({"packed weights": (wp, True)}, {"w": wt_g}, "p8 pack")
    wp.snapshot()
    lin, bias = c["lin"], c["b"].double().view(1, -1, 1, 1)
    cases = [(0, bg, None, lin + bias), (1, bg, None, F.relu(lin + bias)), (2, None, None, lin), (3, None, mp, lin * (c["act"] > 0))]
    if h >= 2 and w >= 2:
        cases.append((4, bg, None, F.max_pool2d(F.relu(lin + bias), 2, 2)))
    for epi, b_, m_, want in cases:
        what = f"{entry} {shape} epilogue {epi}"
        oh, ow = (h // 2, w // 2) if epi == 4 else (h, w)
        guard = conv_guard((n * (oh + 1) + 1) * (ow + 1))
        y = Guarded(_p8_shape(cout, n, oh, ow), BF16, guard, guard, DEV)
        args = [_ptr_of(xp), _ptr_of(wp), _ptr_of(b_), _ptr_of(m_), _ptr_of(y), n, cin, cout, h, w, epi]
        _lib.call(entry, *(args + ([waves] if waves else [])), stream())
        _after_launch({"y": (y, True)}, {"x": xp, "packed weights": wp, "bias": b_, "mask": m_}, what)
        pads_are_zero(y.payload, n, oh, ow)
        bf16_close(p8.to_nchw(y.payload, n, cout, oh, ow), want.float(), what)


# =================================================================================================== weight gradients
WG_SHAPES = [
    (1, 32, 64, 4, 16),       # one chunk, one workgroup
    (2, 64, 128, 19, 35),     # odd H and W: border chunks
    (1, 40, 70, 11, 17),      # channel counts that are not multiples of the tiles
    (2, 32, 128, 3, 333),     # H = 3: every chunk is a border chunk
    (3, 32, 64, 4, 3),        # narrower than one 16-byte piece
]
WAVES = [1, 3, 4, 16]
WG_FAMS = {  # family -> (entry, fits(lib, shape), variants [(suffix, waves)])
    "direct": ("ptmi_conv3x3_wgrad", lambda lib, s: True, [("", None)]),
    "wino": ("ptmi_conv3x3_wino_wgrad", lambda lib, s: lib.ptmi_conv3x3_wino_wgrad_fits(s[3], s[4]),
             [("", None)] + [("_waves", k) for k in WAVES]),
    "wino4": ("ptmi_conv3x3_wino4_wgrad", lambda lib, s: lib.ptmi_conv3x3_wino4_wgrad_fits(s[3], s[4]),
              [("", None)] + [("_waves", k) for k in WAVES]),
    "p8": ("ptmi_p8_wgrad", lambda lib, s: lib.ptmi_p8_wgrad_fits(*s), [("", None)] + [("_waves", k) for k in WAVES]),
}


@functools.lru_cache(maxsize=None)
def _wg_case(n, cin, cout, h, w, bf16):
    gen = g(31 + n * 1000 + cin * 7 + cout * 3 + h * 11 + w)
    x = torch.relu(torch.randn(n, cin, h, w, generator=gen))
    gy = torch.randn(n, cout, h, w, generator=gen)
    if bf16:
        x, gy = rb(x), rb(gy)
    wr = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, br, padding=1).backward(gy.double())
    dw0 = torch.randn(cout, cin, 3, 3, generator=gen)                      # what accumulate = 1 adds into
    db0 = torch.randn(cout, generator=gen)
    return dict(x=x, gy=gy, dw=wr.grad, db=br.grad, dw0=dw0, db0=db0)


def _ws_guard(ws_floats):
    return min(max(4096, int(ws_floats)), 1 << 20)      # a formula one partial short overruns by at most the workspace's own size


@pytest.mark.parametrize("shape", WG_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fam", list(WG_FAMS))
def test_wgrad_writes_dw_db_and_its_exactly_sized_workspace_only(fam, shape):
    """dW and db against float64 autograd at 1e-4 of the gradient's max, accumulate 0 and 1, every `waves` form, db == NULL where the
    header allows it; the split workspace is a guarded payload of exactly *_ws_floats[_waves] floats"""
    _lib, lib, ptr, stream = _api()
    entry, fits, variants = WG_FAMS[fam]
    if not fits(lib, shape):
        pytest.skip(f"{entry}_fits{shape} == 0")
    n, cin, cout, h, w = shape
    c = _wg_case(*shape, fam == "p8")
    if fam == "p8":
        xg, gyg = _p8_from_nchw(c["x"]), _p8_from_nchw(c["gy"])
    else:
        xg, gyg = _ro(c["x"]), _ro(c["gy"])
    sw, sb = float(c["dw"].abs().max()), float(c["db"].abs().max())
    runs = [(sfx, k, acc, True) for sfx, k in variants for acc in (0, 1)]
    if fam == "direct":
        runs += [("", None, 0, False), ("", None, 1, False)]                 # db == NULL
    for sfx, k, acc, with_db in runs:
        what = f"{entry}{sfx} {shape} waves {k} accumulate {acc}" + ("" if with_db else " db NULL")
        q = getattr(lib, f"{entry}_ws_floats{sfx}")
        nws = q(n, cin, cout, h, w, k) if k is not None else q(n, cin, cout, h, w)
        assert nws > 0, what
        ws = Guarded((nws,), F32, _ws_guard(nws), _ws_guard(nws), DEV)
        dw = Guarded((cout, cin, 3, 3), F32, conv_guard(9 * cin), conv_guard(9 * cin), DEV)
        db = Guarded((cout,), F32, 4096, 4096, DEV)
        if acc:
            dw.payload.copy_(c["dw0"])
            db.payload.copy_(c["db0"])
        args = [_ptr_of(xg), _ptr_of(gyg), _ptr_of(dw), _ptr_of(db) if with_db else None, _ptr_of(ws), n, cin, cout, h, w, acc]
        _lib.call(entry + sfx, *(args + ([k] if k is not None else [])), stream())
        _after_launch({"dw": (dw, not acc), "db": (db, not acc and with_db), "ws": (ws, False)}, {"x": xg, "dy": gyg}, what)
        want_w = c["dw"] + (c["dw0"].double() if acc else 0)
        err = float((dw.payload.cpu().double() - want_w).abs().max())
        print(f"[bounds] {what}: dW err {err:.3e} (bar {1e-4 * sw:.3e})")
        assert err <= 1e-4 * sw, f"{what}: dW max abs err {err:.3e} > 1e-4 x {sw:.3e}"       # (a NaN left in dw fails here too)
        if with_db:
            want_b = c["db"] + (c["db0"].double() if acc else 0)
            errb = float((db.payload.cpu().double() - want_b).abs().max())
            assert errb <= 1e-4 * sb, f"{what}: db max abs err {errb:.3e} > 1e-4 x {sb:.3e}"
        elif acc:
            assert torch.equal(db.payload.cpu(), c["db0"]), f"{what}: db written although NULL was passed"
        else:
            assert db.unwritten() == db.numel, f"{what}: db written although NULL was passed"
