"""GPU (pytest -m gpu): MODEL.VGG.NORM "GN" -- the GroupNorm + ReLU kernels (csrc/groupnorm.hip), the fused step with one weight
decay per segment (ptmi_clip_sgd_step_seg_wd), the GN backbone and the trainer on it.

Reference: plain torch on the CPU (tests/groupnorm_ref.py): torch.nn.functional.group_norm + relu, the primitive D2's
get_norm("GN", C) wraps, in float64, with the float32 CPU result as the yardstick of tests/losses_ref.py::check --
err(got) <= max(base_rtol, 4 * err(ref32)), base_rtol 1e-5 for y and 1e-4 for gradients, floor 1e-3 * max |ref64| per tensor.
Inputs are randn + offset with offset 0 and 3 (at offset 10 the fp32 CPU backward itself is off by about the floor-scaled bound:
a yardstick that bad proves nothing).  The fused step is held to the tolerances of tests/test_clip_gradients_gpu.py; the backbone
to the project's 1e-4 bar, scale-aware as tests/test_wino4_gpu.py compares."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import groupnorm_ref as gr
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from probabilisticteacher_amd import ops as _ops
    return _ops


# ============================================================================ the two entries
def _raw(ops, z, gamma, beta, dy, relu, bufs=None, ws=None):
    """ptmi_gn_relu_fwd + ptmi_gn_relu_bwd on device tensors -> {"y", "stats", "dz", "dgamma", "dbeta"}; bufs: outputs to write
    into (default: fresh ones), ws: the workspace (default: the cache's)"""
    from probabilisticteacher_amd import _lib
    n, c = int(z.shape[0]), int(z.shape[1])
    hw = z.numel() // (n * c)
    o = bufs or {"y": torch.empty_like(z), "stats": torch.empty(n * gr.GROUPS * 2, device=z.device), "dz": torch.empty_like(z),
                 "dgamma": torch.empty(c, device=z.device), "dbeta": torch.empty(c, device=z.device)}
    ws = ops._gn_ws(n, c, hw, gr.GROUPS, z.device) if ws is None else ws
    p = ops._ptr
    _lib.call("ptmi_gn_relu_fwd", p(z), p(gamma), p(beta), p(o["y"]), p(o["stats"]), n, c, hw, gr.GROUPS, gr.EPS, int(relu), p(ws),
              ops._stream())
    _lib.call("ptmi_gn_relu_bwd", p(dy), p(o["y"]) if relu else None, p(z), p(gamma), p(o["stats"]), p(o["dz"]), p(o["dgamma"]),
              p(o["dbeta"]), n, c, hw, gr.GROUPS, int(relu), p(ws), ops._stream())
    return o


def _all_shapes(ops):
    return gr.SHAPES + [gr.chunk_plus_one_shape(ops.gn_chunk())]


def _shape_ids():
    return [f"{n}x{c}x{h}x{w}" for n, c, h, w in gr.SHAPES] + ["chunk_plus_one"]


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("offset", gr.OFFSETS)
@pytest.mark.parametrize("idx", range(len(gr.SHAPES) + 1), ids=_shape_ids())
def test_operator_parity(ops, idx, offset, relu):
    """ops.group_norm_relu through autograd: y, dz, dgamma, dbeta"""
    shape = _all_shapes(ops)[idx]
    if idx == len(gr.SHAPES):
        n, c, h, w = shape
        assert (c // gr.GROUPS) * h * w == ops.gn_chunk() + 1 == 4097, "tests/test_groupnorm_cpu.py checks the yardstick at 4097"
    ref64, ref32, (z, gamma, beta, dy) = gr.references(shape, offset, relu)
    zd, gd, bd = (t.to(DEV).requires_grad_() for t in (z, gamma, beta))
    y = ops.group_norm_relu(zd, gd, bd, gr.GROUPS, gr.EPS, relu)
    y.backward(dy.to(DEV))
    got = {"y": y, "dz": zd.grad, "dgamma": gd.grad, "dbeta": bd.grad}
    errs = gr.check_all(got, ref64, ref32, f"{shape} offset {offset} relu {relu}")
    print(f"[groupnorm] {shape} offset {offset} relu {relu}: " +
          ", ".join(f"{k} {e:.2e} (fp32 cpu {e32:.2e})" for k, (e, e32) in errs.items()))
    if relu:
        assert bool((y >= 0).all()) and 0.2 < float((y == 0).float().mean()) < 0.8


def test_statistics_of_a_large_mean(ops):
    """mean 1000, deviation 1: sum / sumsq in fp32 would lose the variance (1e6 + 1 has 3 digits left for it); the chunked
    (count, mean, M2) form keeps it.  mean and rstd against float64."""
    shape = (2, 64, 37, 53)
    gen = torch.Generator().manual_seed(9)
    z = torch.randn(shape, generator=gen) + 1000.0
    o = _raw(ops, z.to(DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(shape, device=DEV), False)
    runs = z.double().view(2 * gr.GROUPS, -1)
    mean, var = runs.mean(1), runs.var(1, unbiased=False)
    stats = o["stats"].view(-1, 2).cpu().double()
    assert float(((stats[:, 0] - mean).abs() / mean).max()) <= 2e-7
    rstd = 1.0 / torch.sqrt(var + gr.EPS)
    # the fp32 inputs near 1000 carry 6e-5 of rounding each; their variance over 3922 values is exact to ~1e-6 in double
    assert float(((stats[:, 1] - rstd).abs() / rstd).max()) <= 1e-6


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
def test_same_bits_whatever_the_address(ops, relu):
    """twice on the same buffers; after an unrelated allocation; and with every map 4, 8, 12 bytes further inside a larger
    allocation (the 16-byte paths change, the lane <-> element assignment does not)"""
    for shape in ((1, 64, 37, 53), (2, 64, 5, 7), gr.chunk_plus_one_shape(ops.gn_chunk()), (3, 128, 64, 96)):
        z, gamma, beta, dy = (t.to(DEV) for t in gr.inputs(shape, 3.0, seed=2))
        first = {k: v.clone() for k, v in _raw(ops, z, gamma, beta, dy, relu).items()}
        again = _raw(ops, z, gamma, beta, dy, relu)
        assert all(torch.equal(first[k], again[k]) for k in first), "two launches"
        junk = torch.randn(123457, device=DEV)                            # moves what the allocator hands out next
        later = _raw(ops, z.clone(), gamma.clone(), beta.clone(), dy.clone(), relu)
        assert all(torch.equal(first[k], later[k]) for k in first), "after an unrelated allocation"
        del junk
        numel = z.numel()
        for shift in (1, 2, 3):
            def moved(t, by=shift):
                big = torch.zeros(numel + 8, device=DEV)
                v = big[by:by + numel].view(shape)
                if t is not None:
                    v.copy_(t)
                assert v.data_ptr() % 16 == 4 * by
                return v
            # y with its input, dz one dword further (shift 3: back on the grid): the elementwise kernels then take their
            # 16-byte path in forward and their dword path in backward
            bufs = {"y": moved(None), "dz": moved(None, (shift + 1) % 4), "stats": torch.empty(shape[0] * gr.GROUPS * 2, device=DEV),
                    "dgamma": torch.empty(shape[1], device=DEV), "dbeta": torch.empty(shape[1], device=DEV)}
            o = _raw(ops, moved(z), gamma, beta, moved(dy), relu, bufs)
            for k in first:
                assert torch.equal(first[k], o[k].reshape(first[k].shape)), f"{shape}: {k} with the maps moved by {4 * shift} bytes"


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
def test_guard_bands(ops, relu):
    """y, dz, mean_rstd, dgamma, dbeta and the workspace between guard bands: every guard word intact, every payload element of the
    outputs written, the inputs unchanged -- also with the maps 4 bytes off the 16-byte grid inside their payload"""
    from probabilisticteacher_amd import _lib
    for shape in ((1, 64, 37, 53), (2, 64, 5, 7), (2, 256, 1, 1), gr.chunk_plus_one_shape(ops.gn_chunk()), (1, 512, 50, 83)):
        n, c, h, w = shape
        z, gamma, beta, dy = gr.inputs(shape, 0.0, seed=3)
        zg, gg, bg, dg = (Guarded.of(t, device=DEV).snapshot() for t in (z, gamma, beta, dy))
        bufs = {"y": Guarded(shape, device=DEV), "dz": Guarded(shape, device=DEV), "stats": Guarded((n * gr.GROUPS * 2,), device=DEV),
                "dgamma": Guarded((c,), device=DEV), "dbeta": Guarded((c,), device=DEV)}
        nbytes = int(_lib.load().ptmi_gn_ws_bytes(n, c, h * w, gr.GROUPS))
        assert nbytes > 0 and nbytes % 256 == 0
        ws = Guarded((nbytes,), torch.uint8, front=65536, back=65536, device=DEV)
        o = _raw(ops, zg.payload, gg.payload, bg.payload, dg.payload, relu, {k: v.payload for k, v in bufs.items()}, ws.payload)
        torch.cuda.synchronize()
        for k, v in bufs.items():
            v.assert_guards_intact(f"{shape} {k}")
            assert v.unwritten() == 0, f"{shape} {k}: {v.unwritten()} elements not written"
        ws.assert_guards_intact(f"{shape} workspace")
        for t, name in ((zg, "z"), (gg, "gamma"), (bg, "beta"), (dg, "dy")):
            t.assert_unchanged(f"{shape} {name}")
        plain = _raw(ops, z.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV), relu)
        assert all(torch.equal(plain[k].reshape(-1), o[k].reshape(-1)) for k in plain)
        # one float further in: a (numel + 1) payload, the map behind its first element
        zs, ds = (Guarded.of(torch.cat([torch.zeros(1), t.reshape(-1)]), device=DEV).snapshot() for t in (z, dy))
        ys, dzs = Guarded((z.numel() + 1,), device=DEV), Guarded((z.numel() + 1,), device=DEV)
        b2 = {"y": ys.payload[1:].view(shape), "dz": dzs.payload[1:].view(shape), "stats": torch.empty(n * gr.GROUPS * 2, device=DEV),
              "dgamma": torch.empty(c, device=DEV), "dbeta": torch.empty(c, device=DEV)}
        o2 = _raw(ops, zs.payload[1:].view(shape), gg.payload, bg.payload, ds.payload[1:].view(shape), relu, b2, ws.payload)
        torch.cuda.synchronize()
        for v, name in ((ys, "y"), (dzs, "dz")):
            v.assert_guards_intact(f"{shape} shifted {name}")
            assert v.unwritten() == 1, f"{shape} shifted {name}: the element in front of the map was written"
        ws.assert_guards_intact(f"{shape} workspace, shifted maps")
        zs.assert_unchanged("shifted z"), ds.assert_unchanged("shifted dy")
        assert all(torch.equal(plain[k].reshape(-1), o2[k].reshape(-1)) for k in plain)


def test_abi_argument_checks(ops):
    from probabilisticteacher_amd import _lib
    lib = _lib.load()
    shape = (1, 64, 4, 4)
    z, gamma, beta, dy = (t.to(DEV) for t in gr.inputs(shape, 0.0))
    y, dz, st = torch.full(shape, 7.0, device=DEV), torch.full(shape, 7.0, device=DEV), torch.full((64,), 7.0, device=DEV)
    dg, db = torch.full((64,), 7.0, device=DEV), torch.full((64,), 7.0, device=DEV)
    ws = ops._gn_ws(1, 64, 16, 32, z.device)
    p, s = ops._ptr, ops._stream()

    def fwd(z_=z, g_=gamma, y_=y, n=1, c=64, hw=16, groups=32, ws_=ws):
        return lib.ptmi_gn_relu_fwd(p(z_), p(g_), p(beta), p(y_), p(st), n, c, hw, groups, gr.EPS, 1, p(ws_), s)

    def bwd(dy_=dy, y_=y, dz_=dz, n=1, c=64, hw=16, groups=32, relu=1, ws_=ws):
        return lib.ptmi_gn_relu_bwd(p(dy_), p(y_), p(z), p(gamma), p(st), p(dz_), p(dg), p(db), n, c, hw, groups, relu, p(ws_), s)

    for fn, what, bad in ([(fwd, "gn_relu_fwd", kw) for kw in (dict(c=48), dict(groups=0), dict(z_=None), dict(g_=None), dict(y_=None),
                                                               dict(ws_=None), dict(n=-1))] +
                          [(bwd, "gn_relu_bwd", kw) for kw in (dict(c=48), dict(dy_=None), dict(y_=None), dict(dz_=None),
                                                               dict(ws_=None), dict(hw=-3), dict(relu=2))]):
        rc = fn(**bad)
        msg = lib.ptmi_last_error().decode()
        assert rc < 0 and msg.startswith(what + ":"), (what, bad, rc, msg)
    assert lib.ptmi_gn_ws_bytes(1, 48, 16, 32) < 0
    # nothing to do: 0, nothing launched, also with null pointers
    assert fwd(n=0) == 0 and fwd(hw=0) == 0 and fwd(n=0, z_=None, y_=None, ws_=None) == 0
    assert bwd(n=0) == 0 and bwd(hw=0) == 0 and bwd(n=0, dy_=None, y_=None, dz_=None, ws_=None) == 0
    torch.cuda.synchronize()
    for t in (y, dz, st, dg, db):
        assert bool((t == 7.0).all()), "nothing above may have written an output"
    with pytest.raises(ValueError):
        ops.group_norm_relu(torch.zeros(1, 48, 4, 4, device=DEV), torch.ones(48, device=DEV), torch.zeros(48, device=DEV))
    e = ops.group_norm_relu(torch.zeros(0, 64, 4, 4, device=DEV), gamma, beta)
    assert e.shape == (0, 64, 4, 4)


# ============================================================================ the fused step with one weight decay per segment
LENGTHS = [1, 63, 64, 65, 8191, 8192, 8193, 20000]
RTOL, ATOL = 1e-5, 1e-6                                  # tests/test_clip_gradients_gpu.py
LR, MU, WD, CLIP = 0.016, 0.9, 1e-4, 10.0
CLIP_VALUE = {"value": 0.05, "norm": 1.0, "none": 0.0}


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, tol = (a - b).abs(), ATOL + RTOL * b.abs()
    assert bool((err <= tol).all()), f"{what}: max abs err {float(err.max()):.3e}, max |ref| {float(b.abs().max()):.3e}"


_STEP = {}


def _step_case():
    if not _STEP:
        offs = [0]
        for k in LENGTHS:
            offs.append(offs[-1] + k)
        gen = torch.Generator().manual_seed(21)
        n = offs[-1]
        _STEP.update(offs=offs, g=torch.randn(n, generator=gen) * 3, p=torch.randn(n, generator=gen), junk=torch.randn(n, generator=gen))
    return _STEP


@pytest.mark.parametrize("start", [0, 1], ids=["wd_first_0", "wd_first_1e-4"])
@pytest.mark.parametrize("clip_type", ["value", "norm", "none"])
def test_seg_wd_step_against_float64(ops, clip_type, start):
    c = _step_case()
    offs, g, p0 = c["offs"], c["g"], c["p"]
    assert ops.SEG_CHUNK == 8192
    wds = [WD if (i + start) % 2 else 0.0 for i in range(len(LENGTHS))]
    table = ops.SegmentTable(offs, DEV)
    gd, pd, bd = g.to(DEV), p0.to(DEV), c["junk"].to(DEV)                  # first = True must not read the momentum buffer
    wd_t = torch.tensor(wds, dtype=torch.float32, device=DEV)
    ss = ops.sumsq(gd)
    assert float(ss) > CLIP ** 2, "the global clip is active"
    v = CLIP_VALUE[clip_type]
    gs = g.double() * (CLIP / math.sqrt(float(ss)))
    if clip_type == "value":
        assert 100 < int((gs.abs() > v).sum()) < g.numel() - 100
    if clip_type == "norm":
        norms64 = [float(gs[a:b].norm()) for a, b in zip(offs[:-1], offs[1:])]
        assert min(norms64) < 0.5 * v and max(norms64) > 2 * v
    p_ref, b_ref = p0.double(), torch.zeros_like(p0).double()
    g_bits = gd.clone()
    for step in range(3):
        norms = ops.seg_gradnorm(gd, table, ss, CLIP, False) if clip_type == "norm" else None
        ops.clip_sgd_step_seg_wd(pd, gd, bd, table, ss, CLIP, clip_type, v, norms, LR, MU, wd_t, step == 0)
        p_ref, b_ref = gr.sgd_step64(p_ref, g, b_ref, offs, wds, float(ss), CLIP, clip_type, v, False, LR, MU, step == 0)
        assert torch.equal(gd, g_bits), "the step wrote g"
        _close(bd, b_ref, f"{clip_type} momentum, step {step}")
        _close(pd, p_ref, f"{clip_type} parameters, step {step}")
    # the table is read.  Three steps of decay move a parameter by lr * wd * p * (1 + 1.9 + 2.71) = 9e-6 p, just inside the
    # tolerance above, so the two alternations are told apart by distance: the result is fp32 rounding (~1e-7 p) away from the
    # restatement with its own table and 9e-6 p away from the one with the segments' decays swapped
    other = [WD - w for w in wds]
    q, bq = p0.double(), torch.zeros_like(p0).double()
    for step in range(3):
        q, bq = gr.sgd_step64(q, g, bq, offs, other, float(ss), CLIP, clip_type, v, False, LR, MU, step == 0)
    got = pd.cpu().double()
    own, swapped = float((got - p_ref).abs().max()), float((got - q).abs().max())
    print(f"[groupnorm] seg_wd {clip_type}: max |p - restated| {own:.3e}, with the decays swapped {swapped:.3e}")
    assert swapped > 10 * own


@pytest.mark.parametrize("shift", [0, 1])
def test_seg_wd_step_with_a_constant_table_is_the_existing_step(ops, shift):
    """bit for bit: "value" and "norm" against ptmi_clip_sgd_step_seg, "none" against ptmi_clip_sgd_step.  shift 1: g sits 4 bytes
    off the 16-byte grid p and buf are on (the one-dword-per-lane path)."""
    c = _step_case()
    offs, n = c["offs"], c["g"].numel()
    table = ops.SegmentTable(offs, DEV)
    gd = torch.zeros(n + 4, device=DEV)[shift:shift + n].copy_(c["g"].to(DEV))
    wd_t = torch.full((len(LENGTHS),), WD, dtype=torch.float32, device=DEV)
    ss = ops.sumsq(gd)
    for clip_type in ("value", "norm", "none"):
        v = CLIP_VALUE[clip_type]
        p1, b1, p2, b2 = c["p"].to(DEV), c["junk"].to(DEV), c["p"].to(DEV), c["junk"].to(DEV)
        for step in range(3):
            norms = ops.seg_gradnorm(gd, table, ss, CLIP, False).clone() if clip_type == "norm" else None
            ops.clip_sgd_step_seg_wd(p1, gd, b1, table, ss, CLIP, clip_type, v, norms, LR, MU, wd_t, step == 0)
            if clip_type == "none":
                ops.clip_sgd_step(p2, gd.contiguous(), b2, ss, CLIP, LR, MU, WD, step == 0)
            else:
                ops.clip_sgd_step_seg(p2, gd, b2, table, ss, CLIP, clip_type, v, norms, LR, MU, WD, step == 0)
            assert torch.equal(p1, p2) and torch.equal(b1, b2), f"{clip_type}, step {step}"
        assert not torch.equal(p1, c["p"].to(DEV))


def test_seg_wd_argument_checks(ops):
    from probabilisticteacher_amd import _lib
    table = ops.SegmentTable([0, 40, 100], DEV)
    p, g, buf = (torch.randn(100, device=DEV) for _ in range(3))
    ss = ops.sumsq(g)
    wd_t = torch.zeros(2, device=DEV)
    bits = p.clone()
    with pytest.raises(ValueError):
        ops.clip_sgd_step_seg_wd(p, g, buf, table, ss, CLIP, "none", 0.0, None, LR, MU, torch.zeros(3, device=DEV), True)
    with pytest.raises(ValueError):
        ops.clip_sgd_step_seg_wd(p, g, buf, table, ss, CLIP, "both", 0.0, None, LR, MU, wd_t, True)
    with pytest.raises(ValueError):
        ops.clip_sgd_step_seg_wd(p, g, buf, table, ss, CLIP, "norm", 1.0, None, LR, MU, wd_t, True)
    with pytest.raises(_lib.PtmiError, match="clip_sgd_step_seg_wd"):
        ops.clip_sgd_step_seg_wd(p, g, buf, table, ss, CLIP, "value", 0.0, None, LR, MU, wd_t, True)
    lib, ptr = _lib.load(), ops._ptr
    assert lib.ptmi_clip_sgd_step_seg_wd(ptr(p), ptr(g), ptr(buf), 100, ptr(table.seg_off), 2, ptr(table.chunks), table.C, ptr(ss),
                                         CLIP, 2, 0.0, None, LR, MU, None, 1, ops._stream()) < 0
    assert lib.ptmi_last_error().decode().startswith("clip_sgd_step_seg_wd:")
    assert lib.ptmi_clip_sgd_step_seg_wd(ptr(p), ptr(g), ptr(buf), 0, None, 0, None, 0, ptr(ss), CLIP, 2, 0.0, None, LR, MU, None, 1,
                                         ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, bits)


# ============================================================================ the backbone
def _cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_s2c.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1,
        "SEED", 0] + list(opts))


def _backbone64(sd, x, freeze_at):
    """conv2d -> group_norm -> relu (-> max_pool2d) in float64 on the CPU from the model's own state dict -> (features, leaves)"""
    leaves = {k: v.detach().cpu().double().requires_grad_(int(k.split(".")[0][-1]) > freeze_at) for k, v in sd.items()}
    t = x.double()
    for b, convs in enumerate((2, 2, 3, 3, 3), start=1):
        for k in range(1, convs + 1):
            q = f"vgg_block{b}.0.conv{k}."
            t = F.conv2d(t, leaves[q + "weight"], leaves[q + "bias"], padding=1)
            t = F.relu(F.group_norm(t, 32, leaves[q + "norm.weight"], leaves[q + "norm.bias"], 1e-5))
        if b < 5:
            t = F.max_pool2d(t, 2, 2)
    return t, leaves


@pytest.mark.parametrize("freeze_at", [0, 2])
def test_backbone_parity(ops, freeze_at):
    from probabilisticteacher_amd.modeling.backbone import build_backbone
    torch.manual_seed(7)
    bb = build_backbone(_cfg("MODEL.VGG.NORM", "GN", "MODEL.BACKBONE.FREEZE_AT", freeze_at)).to(DEV)
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for n, p in bb.named_parameters():      # norm parameters away from their 1 / 0 init, conv biases away from 0
            if n.endswith("norm.weight"):
                p.copy_(1.0 + (torch.rand(p.shape, generator=gen) - 0.5))
            elif n.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)
    x = torch.randn(2, 3, 64, 96, generator=gen)
    want, leaves = _backbone64(bb.state_dict(), x, freeze_at)
    up = torch.randn(want.shape, generator=gen)
    (want * up.double()).sum().backward()
    got = bb(x.to(DEV))["vgg_block5"]
    assert got.shape == want.shape == (2, 512, 4, 6)
    (got * up.to(DEV)).sum().backward()

    def close(a, b, what):
        a, b = a.detach().cpu().double(), b.detach().double()
        err, tol = (a - b).abs(), 1e-4 * float(b.abs().max()) + 1e-4 * b.abs()
        print(f"[groupnorm] backbone freeze {freeze_at} {what}: max err {float(err.max()):.3e} of scale {float(b.abs().max()):.3e}")
        assert bool((err <= tol).all()), f"{what}: max abs err {float(err.max()):.3e}, scale {float(b.abs().max()):.3e}"

    close(got, want, "features")
    for n, p in bb.named_parameters():
        frozen = int(n.split(".")[0][-1]) <= freeze_at
        assert p.requires_grad != frozen
        if frozen:
            assert p.grad is None and leaves[n].grad is None, n
        else:
            close(p.grad, leaves[n].grad, n)


def test_anomaly_mode_names_the_norm_layer(ops):
    """a NaN in one norm weight: the first record is the forward output of that layer's GroupNorm, under the state-dict path of
    its module (conv{k}.norm); a clean backbone leaves no record and its convolutions report under conv{k}"""
    from probabilisticteacher_amd.anomaly import AnomalySink
    from probabilisticteacher_amd.modeling.backbone import build_backbone
    torch.manual_seed(7)
    bb = build_backbone(_cfg("MODEL.VGG.NORM", "GN", "MODEL.BACKBONE.FREEZE_AT", 0)).to(DEV)
    x = torch.randn(1, 3, 32, 48, generator=torch.Generator().manual_seed(1)).to(DEV)
    sink = AnomalySink(torch.device(DEV))

    def run():
        sink.begin_step()
        with ops.anomaly(sink), ops.anomaly_branch("supervised"), ops.anomaly_scope("backbone"):
            bb(x)["vgg_block5"].sum().backward()
        return sink.collect()
    assert run() == []
    scopes = {s[2] for s in sink._slots}
    assert {"backbone.vgg_block3.0.conv2", "backbone.vgg_block3.0.conv2.norm"} <= scopes
    assert {s[3] for s in sink._slots if s[2].endswith(".norm")} == {"group_norm_relu"}
    with torch.no_grad():
        bb.vgg_block3[0].conv2.norm.weight[5] = float("nan")
    recs = run()
    r = recs[0]
    assert (r.phase, r.branch, r.scope, r.op, r.output, r.kind) == ("forward", "supervised", "backbone.vgg_block3.0.conv2.norm",
                                                                    "group_norm_relu", "y", "nan"), r.describe()
    assert r.coordinate[:2] == (0, 5)
    assert any(q.phase == "backward" and q.scope == "backbone.vgg_block3.0.conv2.norm" and q.output == "dgamma" for q in recs)


# ============================================================================ the trainer
def _spy_step(tr, batch):
    """one run_step with the library calls logged on tr.calls and what the optimiser tail saw on tr.seen"""
    from probabilisticteacher_amd import _lib
    real = tr._clip_and_step

    def recording(clip_norm):
        tr.seen = tuple(t.clone() for t in (tr.student.trainable(), tr.student.grad, tr.momentum_buf))
        return real(clip_norm)
    tr._clip_and_step = recording
    tr.calls, call = [], _lib.call

    def spy(name, *a):
        tr.calls.append(name)
        return call(name, *a)
    _lib.call = spy
    try:
        return dict(tr.run_step(batch))
    finally:
        _lib.call = call
        tr._clip_and_step = real


def _trainer(cfg):
    """A fresh trainer from SEED, in a regime where the unsupervised losses are defined.  The reference's unsupervised box loss is
    a MEAN over the proposals whose teacher class is not background (fast_rcnn.py:215-263): with none it is NaN, there as here.
    At a random initialisation the sign of (foreground - background logit) is nearly the same for every proposal -- the box
    head's features are non-negative and alike -- so whether any row is foreground is a coin toss of the seed, and two steps at
    the full learning rate push every proposal to background.  So: the config's own warm-up stays on (final_s2c: 400 iterations
    from 1e-3 of BASE_LR; the burn-in steps move the logits by ~1e-2), and the one foreground class starts with a logit bias
    of +1: the teacher then calls proposals foreground by construction, not by luck."""
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    seed_all_rng(cfg.SEED)
    tr = PTrainer(cfg)
    assert cfg.MODEL.ROI_HEADS.NUM_CLASSES == 1 and cfg.SOLVER.WARMUP_ITERS == 400
    with torch.no_grad():
        for model in (tr.model, tr.model_teacher):
            model.roi_heads.box_predictor.cls_score.bias[0] = 1.0
    return tr


def _strip(metrics):
    return {k: v for k, v in metrics.items() if k not in ("data_time", "time")}


GN = ["MODEL.VGG.NORM", "GN", "UNSUPNET.BURN_UP_STEP", 2]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from bench import synth_records
    from probabilisticteacher_amd import checkpoint
    gen = torch.Generator().manual_seed(77)
    batches = [tuple(synth_records(gen, 1, 192, 256, 1, DEV) for _ in range(4)) for _ in range(4)]
    out = {"batches": batches}
    a = _trainer(_cfg(*GN))
    out["a"], out["a_metrics"], out["a_seen"], out["a_calls"], out["ema"] = a, [], [], [], None
    path = str(tmp_path_factory.mktemp("gn") / "after3.pth")
    for i, batch in enumerate(batches):
        if i == 3:
            checkpoint.save_checkpoint(a, path)
            out["streams"] = (a._rng.getstate(), a._key_gen.get_state())
            out["ema"] = (a.student.flat.clone(), a.teacher.flat.clone())      # what the EMA of step 3 starts from
        out["a_metrics"].append(_spy_step(a, batch))
        out["a_seen"].append(a.seen)
        out["a_calls"].append(a.calls)
        if i == 3:
            out["teacher_after"] = a.teacher.flat.clone()
    torch.cuda.synchronize()
    b = _trainer(_cfg(*GN))
    out["b"], out["b_metrics"] = b, [_spy_step(b, batch) for batch in batches]
    # a fresh trainer that resumes from the file written after three steps; the checkpoint does not hold the random streams
    # (shrink-paste ratio, sampling keys), so the test carries them over
    c = _trainer(_cfg(*GN))
    checkpoint.load_checkpoint(c, path, resume=True)
    c._rng.setstate(out["streams"][0])
    c._key_gen.set_state(out["streams"][1])
    out["c"], out["c_metrics"] = c, _spy_step(c, batches[3])
    same = _trainer(_cfg(*GN, "SOLVER.WEIGHT_DECAY_NORM", 0.0001))
    out["same"], out["same_metrics"] = same, _spy_step(same, batches[0])
    plain = _trainer(_cfg("UNSUPNET.BURN_UP_STEP", 2))
    out["plain"], out["plain_metrics"] = plain, _spy_step(plain, batches[0])
    torch.cuda.synchronize()
    return out


def test_trainer_losses_are_finite(runs):
    a = runs["a"]
    assert a.iter == 4 and a.deterministic
    for i, m in enumerate(runs["a_metrics"]):
        losses = {k: v for k, v in m.items() if k.startswith("loss")}
        assert len(losses) >= 4 and all(k.endswith("sup") for k in losses if i >= 2), (i, sorted(m))
        assert all(math.isfinite(v) for v in m.values()), (i, m)
    assert a.cfg.MODEL.BACKBONE.FREEZE_AT == 2
    for i, calls in enumerate(runs["a_calls"]):
        # 13 normalised layers per backbone pass, 9 of them (blocks 3-5) with a backward pass; mutual learning adds the teacher's
        # pass and runs the student's two branches in one pass or in two
        assert calls.count("ptmi_gn_relu_fwd") in ((13,) if i < 2 else (26, 39)), (i, calls.count("ptmi_gn_relu_fwd"))
        assert calls.count("ptmi_gn_relu_bwd") in ((9,) if i < 2 else (9, 18)), (i, calls.count("ptmi_gn_relu_bwd"))
        assert calls[-2:] == ["ptmi_sumsq", "ptmi_clip_sgd_step_seg_wd"]
        assert "ptmi_conv3x3_wino4p_fwd_list" not in calls and "ptmi_frame_fill" not in calls, "no frame skip under GN"


def test_trainer_teacher_norm_parameters_follow_the_ema(runs):
    a = runs["a"]
    k = a.cfg.UNSUPNET.EMA_KEEP_RATE
    s, t = runs["ema"]
    want = s * float(1 - k) + t * float(k)
    names = [n for n in a.student.index if ".norm." in n]
    assert len(names) == 26
    moved = 0
    for n in names:
        off, cnt = a.student.index[n]
        got, w = runs["teacher_after"][off:off + cnt], want[off:off + cnt]
        assert bool(((got - w).abs() <= 1e-6 * w.abs()).all()), n
        moved += int((got != t[off:off + cnt]).sum())
    assert moved > 0, "the student's norm parameters have moved away from the teacher's by step 3"
    # at the first mutual-learning step the teacher became the student
    s2 = runs["a_seen"][2][0]
    assert a.cfg.UNSUPNET.BURN_UP_STEP == 2 and s2.numel() == a.student.n_trainable


def test_trainer_first_step_is_the_restated_update(runs):
    """p_new == p - lr (s g + wd_seg p) at 1e-6 relative, g read back from the flat gradient buffer; the momentum buffer of the
    first step IS s g + wd_seg p, which tells the two decays apart whatever the learning rate (under warm-up lr wd p is below one
    fp32 ulp of p)"""
    from probabilisticteacher_amd.solver import lr_at
    a = runs["a"]
    p0, g, buf0 = (t.cpu().double() for t in runs["a_seen"][0])
    assert not bool(buf0.any())
    lr = lr_at(a.cfg, 0)
    s = 10.0 / max(float(g.norm()), 10.0)
    p1, buf1 = runs["a_seen"][1][0].cpu().double(), runs["a_seen"][1][2].cpu().double()
    names = [m for m, q in a.student.params.items() if q.requires_grad]
    checked = {}
    for n, wd in (("backbone.vgg_block3.0.conv2.norm.weight", 0.0), ("backbone.vgg_block3.0.conv2.weight", a.cfg.SOLVER.WEIGHT_DECAY)):
        off, cnt = a.student.index[n]
        assert a.segment_wd[names.index(n)] == wd and a.cfg.SOLVER.WEIGHT_DECAY == 1e-4
        p, gg = p0[off:off + cnt], g[off:off + cnt]
        assert bool(gg.abs().max() > 0), f"{n} got a gradient"
        upd = s * gg + wd * p
        err_p = (p1[off:off + cnt] - (p - lr * upd)).abs()
        assert bool((err_p <= 1e-6 * (p.abs() + lr * upd.abs())).all()), f"{n}: max err {float(err_p.max()):.3e}"
        tol_b = 1e-6 * ((s * gg).abs() + (wd * p).abs())
        err_b = (buf1[off:off + cnt] - upd).abs()
        assert bool((err_b <= tol_b).all()), f"{n} momentum: max err {float(err_b.max()):.3e}"
        other = s * gg + (1e-4 - wd) * p                                   # the other segment kind's decay
        assert not bool(((buf1[off:off + cnt] - other).abs() <= 1e-6 * ((s * gg).abs() + 1e-4 * p.abs())).all()), n
        checked[n] = (float(err_p.max()), float(err_b.max()))
    print("[groupnorm] first step, max |p_new - restated|, max |buf - restated|:", checked)


def test_trainer_is_reproducible(runs):
    a, b = runs["a"], runs["b"]
    for ma, mb in zip(runs["a_metrics"], runs["b_metrics"]):
        assert _strip(ma) == _strip(mb)
    assert torch.equal(a.student.flat, b.student.flat) and torch.equal(a.teacher.flat, b.teacher.flat)
    assert torch.equal(a.momentum_buf, b.momentum_buf)


def test_trainer_resume_continues_bit_for_bit(runs):
    a, c = runs["a"], runs["c"]
    assert c.iter == 4 and c.start_iter == 3
    assert _strip(runs["c_metrics"]) == _strip(runs["a_metrics"][3])
    assert torch.equal(a.student.flat, c.student.flat) and torch.equal(a.teacher.flat, c.teacher.flat)
    assert torch.equal(a.momentum_buf, c.momentum_buf)


def test_equal_weight_decays_call_the_existing_entry(runs):
    same = runs["same"]
    assert same._seg_wd is None and same.calls[-2:] == ["ptmi_sumsq", "ptmi_clip_sgd_step"]
    assert "ptmi_clip_sgd_step_seg_wd" not in same.calls and same.calls.count("ptmi_gn_relu_fwd") > 0
    assert all(math.isfinite(v) for v in runs["same_metrics"].values())
    # the decay of the norm parameters is the one difference from run a's first step: its momentum buffer holds it
    assert torch.equal(runs["a_seen"][0][1], same.seen[1]), "the same gradient"
    assert not torch.equal(runs["a_seen"][1][2], same.momentum_buf)


def test_default_is_untouched(runs):
    plain = runs["plain"]
    keys = list(plain.model.state_dict().keys())
    assert not [k for k in keys if "norm" in k]
    convs = [(1, 2), (2, 2), (3, 3), (4, 3), (5, 3)]
    assert [k for k in keys if k.startswith("backbone.")] == [f"backbone.vgg_block{b}.0.conv{k}.{s}" for b, nk in convs
                                                              for k in range(1, nk + 1) for s in ("weight", "bias")]
    assert not [n for n in plain.calls if n.startswith("ptmi_gn_") or n == "ptmi_clip_sgd_step_seg_wd"]
    assert plain.calls[-2:] == ["ptmi_sumsq", "ptmi_clip_sgd_step"]
    assert plain._seg_wd is None and plain._wd_segments is None and plain._segments is None
    assert all(math.isfinite(v) for v in runs["plain_metrics"].values())
