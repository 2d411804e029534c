"""GPU (pytest -m gpu): SOLVER.CLIP_GRADIENTS -- the segment-aware clip + SGD step and the per-segment gradient norm.

Reference: torch itself on the CPU in fp32 -- torch.optim.SGD(momentum, weight_decay) on separate parameter tensors, preceded
per step by the global scale g *= 10 / max(||g||, 10) and by torch.nn.utils.clip_grad_value_ / clip_grad_norm_ called per
parameter (what detectron2 0.5's maybe_add_gradient_clipping does inside optimizer.step()).

Tolerance: rtol 1e-5 / atol 1e-6, the one tests/test_ops_gpu.py::test_ema_clip_sgd applies to the existing fused step against
its torch restatement; the added arithmetic is one multiply or one clamp per element.  The per-segment norms themselves are
compared with float64 norms of the same fp32 values at rtol 1e-5: an fp32 sum of n <= 70001 squares through 8 serial adds per
accumulator and a fixed tree of depth ~13 is off by at most ~21 roundings of 6e-8, and the square root halves that."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-5, 1e-6
LR, MU, WD, CLIP = 0.016, 0.9, 1e-4, 10.0

LENGTHS = [1, 3, 18, 255, 256, 257, 1024, 1025, 4099, 70001]
# norm of each segment's gradient before the global scale, in units of the one segment that sits at the clip value (1025):
# far above, far below, all zeros (256)
WEIGHT = {1: 3.0, 3: 0.01, 18: 50.0, 255: 0.02, 256: 0.0, 257: 0.3, 1024: 40.0, 1025: 1.0, 4099: 0.05, 70001: 2.0}
NEAR, VALUE_V = 1025, float(torch.tensor(0.004, dtype=torch.float32))


def close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} vs {tuple(b.shape)}"
    err, tol = (a - b).abs(), ATOL + RTOL * b.abs()
    assert bool((err <= tol).all()), f"{what}: max abs err {float(err.max()):.3e}, max |ref| {float(b.abs().max()):.3e}"


def _offsets(lengths):
    offs = [0]
    for k in lengths:
        offs.append(offs[-1] + k)
    return offs


def _norm(x, inf_norm):
    return x.abs().max() if inf_norm else x.norm()


def _gradient(lengths, big: bool, inf_norm: bool, seed=5):
    """random segments of norm WEIGHT (L2 or max-abs), scaled down when the global L2 norm is to stay below 10 (L2: sqrt(sum
    w^2) = 64.1, x 0.1; max-abs 2 over 70001 normal values is an L2 norm of ~120, x 0.01); some elements exactly at +-VALUE_V"""
    gen = torch.Generator().manual_seed(seed)
    small = 0.01 if inf_norm else 0.1
    parts = []
    for k in lengths:
        x = torch.randn(k, generator=gen)
        parts.append(x / _norm(x, inf_norm) * (WEIGHT[k] * (1.0 if big else small)))
    g = torch.cat(parts)
    offs = _offsets(lengths)
    a = offs[lengths.index(70001)]
    g[a + 7], g[a + 8], g[a + 4096], g[a + 70000] = VALUE_V, -VALUE_V, VALUE_V, -VALUE_V
    b = offs[lengths.index(257)]
    g[b], g[b + 256] = -VALUE_V, VALUE_V
    return g, offs


def _global_scale(g):
    """the reference's global clip coefficient, from the float64 norm: torch's fp32 CPU norm of these deliberately uneven
    gradients is itself off by 2e-5 (64.1399 for 64.14119), twice the tolerance the update is held to"""
    return CLIP / max(float(g.double().norm()), CLIP)


def torch_steps(p0, g, offs, steps, clip_type, v, inf_norm, lr=LR, mu=MU, wd=WD):
    """[(parameters, momentum)] after each of `steps` reference steps on the same gradient"""
    segs = list(zip(offs[:-1], offs[1:]))
    params = [p0[a:b].clone().requires_grad_() for a, b in segs]
    sgd = torch.optim.SGD(params, lr=lr, momentum=mu, weight_decay=wd)
    out = []
    for _ in range(steps):
        s = _global_scale(g)
        for q, (a, b) in zip(params, segs):
            q.grad = g[a:b].clone().mul_(s)
            if clip_type == "value":
                torch.nn.utils.clip_grad_value_(q, v)
            elif clip_type == "norm":
                torch.nn.utils.clip_grad_norm_(q, v, math.inf if inf_norm else 2.0)
        sgd.step()
        out.append((torch.cat([q.detach() for q in params]), torch.cat([sgd.state[q]["momentum_buffer"] for q in params])))
    return out


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from probabilisticteacher_amd import ops as _ops
    return _ops


_CASES = {}


def _case(lengths, big, inf_norm):
    """gradient, parameters and garbage momentum of one layout, drawn once and never written"""
    key = (tuple(lengths), big, inf_norm)
    if key not in _CASES:
        g, offs = _gradient(lengths, big, inf_norm)
        gen = torch.Generator().manual_seed(11)
        _CASES[key] = (g, offs, torch.randn(g.numel(), generator=gen), torch.randn(g.numel(), generator=gen))
    return _CASES[key]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("clip_type,inf_norm", [("value", False), ("norm", False), ("norm", True)])
def test_three_steps_against_torch(ops, clip_type, inf_norm, big, reverse):
    lengths = LENGTHS[::-1] if reverse else LENGTHS
    g, offs, p0, junk = _case(lengths, big, inf_norm)
    s = _global_scale(g)
    assert (s < 0.5) if big else (s == 1.0)
    gs = g * s
    ref_norms = torch.stack([_norm(gs[a:b].double(), inf_norm) for a, b in zip(offs[:-1], offs[1:])])
    if clip_type == "value":
        v = VALUE_V
        assert int((gs.abs() > v).sum()) > 100 and int((gs.abs() < v).sum()) > 100
        assert big or int((gs.abs() == v).sum()) == 6, "elements exactly at +-v"
    else:
        near = lengths.index(NEAR)
        v = float(ref_norms[near]) * (1 + 5e-4)                       # one segment within 1e-3 of v ...
        rel = ref_norms / v
        assert abs(float(rel[near]) - 1) < 1e-3 and int((rel > 10).sum()) >= 2 and int(((rel < 0.1) & (rel > 0)).sum()) >= 2
        assert float(ref_norms[lengths.index(256)]) == 0.0           # ... far above, far below, and one all zeros
    want = torch_steps(p0, g, offs, 3, clip_type, v, inf_norm)
    table = ops.SegmentTable(offs, DEV)
    assert table.S == len(lengths) and table.C == sum(-(-k // ops.SEG_CHUNK) for k in lengths)
    gd, pd, bd = g.to(DEV), p0.to(DEV), junk.to(DEV)                   # first = True must not read the momentum buffer
    g_bits = gd.clone()
    ss = ops.sumsq(gd)
    for step, (pw, bw) in enumerate(want):
        norms = None
        if clip_type == "norm":
            norms = ops.seg_gradnorm(gd, table, ss, CLIP, inf_norm)
            assert torch.equal(gd, g_bits), "seg_gradnorm wrote g"
            got = norms.cpu().double()
            print(f"[clip] norms max rel err {float(((got - ref_norms).abs() / ref_norms.clamp_min(1e-30)).max()):.3e}")
            assert bool(((got - ref_norms).abs() <= 1e-5 * ref_norms).all()), (got, ref_norms)
        ops.clip_sgd_step_seg(pd, gd, bd, table, ss, CLIP, clip_type, v, norms, LR, MU, WD, step == 0)
        assert torch.equal(gd, g_bits), "clip_sgd_step_seg wrote g"
        print(f"[clip] {clip_type} inf={inf_norm} big={big} rev={reverse} step {step}: max |dp| "
              f"{float((pd.cpu() - pw).abs().max()):.3e} max |dbuf| {float((bd.cpu() - bw).abs().max()):.3e}")
        close(bd, bw, f"momentum, step {step}")
        close(pd, pw, f"param, step {step}")
    # the clip is not a no-op at this tolerance: the unclipped reference is somewhere else
    plain = torch_steps(p0, g, offs, 3, None, v, inf_norm)[-1][1]
    assert not bool(((bd.cpu().double() - plain.double()).abs() <= ATOL + RTOL * plain.double().abs()).all())


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shift", [0, 1])
def test_value_mode_is_the_existing_step_on_a_clamped_gradient(ops, reverse, shift):
    """s = 1: bit-equal to ops.clip_sgd_step on clamp(g, -v, v).  shift 1: g sits 4 bytes off the 16-byte grid p and buf are on,
    so the kernel takes its one-dword-per-lane path; shift 0 the 16-byte one with scalar heads and tails."""
    lengths = LENGTHS[::-1] if reverse else LENGTHS
    g, offs, p0, junk = _case(lengths, False, False)
    assert _global_scale(g) == 1.0
    n = g.numel()
    table = ops.SegmentTable(offs, DEV)
    gd = torch.zeros(n + 4, device=DEV)[shift:shift + n].copy_(g.to(DEV))
    pre = g.clamp(-VALUE_V, VALUE_V).to(DEV)
    g_bits = gd.clone()
    ss = ops.sumsq(gd)
    p1, b1, p2, b2 = p0.to(DEV), junk.to(DEV), p0.to(DEV), junk.to(DEV)
    for step in range(3):
        ops.clip_sgd_step_seg(p1, gd, b1, table, ss, CLIP, "value", VALUE_V, None, LR, MU, WD, step == 0)
        ops.clip_sgd_step(p2, pre, b2, ss, CLIP, LR, MU, WD, step == 0)
        assert torch.equal(gd, g_bits), "clip_sgd_step_seg wrote g"
        assert torch.equal(b1, b2) and torch.equal(p1, p2), f"step {step}"
    assert not torch.equal(p1, p0.to(DEV))


@pytest.mark.parametrize("inf_norm", [False, True])
def test_segment_norms_are_a_function_of_the_data_alone(ops, inf_norm):
    """twice on the same buffer, and on the same values 4, 8 and 12 bytes further inside a larger allocation: the same bits
    (element j of a chunk always goes to thread j % 256, whatever the address)"""
    g, offs, _, _ = _case(LENGTHS, True, inf_norm)
    n = g.numel()
    table = ops.SegmentTable(offs, DEV)
    gd = g.to(DEV)
    ss = ops.sumsq(gd)
    first = ops.seg_gradnorm(gd, table, ss, CLIP, inf_norm).clone()
    again = ops.seg_gradnorm(gd, table, ss, CLIP, inf_norm).clone()
    assert torch.equal(first, again)
    assert bool((first[torch.tensor([k > 0 for k in LENGTHS])] >= 0).all()) and float(first[LENGTHS.index(256)]) == 0.0
    big = torch.zeros(n + 8, device=DEV)
    for shift in (1, 2, 3):
        moved = big[shift:shift + n].copy_(gd)
        assert moved.data_ptr() % 16 == (gd.data_ptr() + 4 * shift) % 16
        assert torch.equal(ops.seg_gradnorm(moved, table, ss, CLIP, inf_norm), first), f"base moved by {4 * shift} bytes"


def test_abi_argument_checks(ops):
    from probabilisticteacher_amd import _lib
    lib = _lib.load()
    n, offs = 100, [0, 40, 100]
    table = ops.SegmentTable(offs, DEV)
    p, g, buf = (torch.randn(n, device=DEV) for _ in range(3))
    ss = ops.sumsq(g)
    ptr = ops._ptr
    p_bits, b_bits = p.clone(), buf.clone()

    def step(p_=p, g_=g, buf_=buf, n_=n, seg=table.seg_off, S=table.S, chunks=table.chunks, C=table.C):
        return lib.ptmi_clip_sgd_step_seg(ptr(p_), ptr(g_), ptr(buf_), n_, ptr(seg), S, ptr(chunks), C, ptr(ss), CLIP, 0, 0.5,
                                          None, LR, MU, WD, 1, ops._stream())

    def norm(g_=g, n_=n, seg=table.seg_off, first=table.seg_chunk, S=table.S, chunks=table.chunks, C=table.C):
        return lib.ptmi_seg_gradnorm(ptr(g_), n_, ptr(seg), ptr(first), S, ptr(chunks), C, ptr(ss), CLIP, 0, ptr(table.ws),
                                     ptr(table.seg_norm), ops._stream())

    # one call at a time: the error string is that of the last failed call
    for fn, what, bad in ([(step, "clip_sgd_step_seg", kw) for kw in (dict(seg=None), dict(chunks=None), dict(n_=-1), dict(S=-1),
                                                                      dict(C=-2), dict(p_=None))] +
                          [(norm, "seg_gradnorm", kw) for kw in (dict(seg=None), dict(first=None), dict(chunks=None), dict(n_=-5),
                                                                 dict(S=-1), dict(g_=None))]):
        rc = fn(**bad)
        msg = lib.ptmi_last_error().decode()
        assert rc < 0 and msg.startswith(what + ":"), (what, bad, rc, msg)
    # "norm" without the segment norms is refused; the wrapper refuses buffers the table does not cover
    assert lib.ptmi_clip_sgd_step_seg(ptr(p), ptr(g), ptr(buf), n, ptr(table.seg_off), table.S, ptr(table.chunks), table.C,
                                      ptr(ss), CLIP, 1, 0.5, None, LR, MU, WD, 1, ops._stream()) < 0
    with pytest.raises(ValueError):
        ops.clip_sgd_step_seg(p[:50], g[:50], buf[:50], table, ss, CLIP, "value", 0.5, None, LR, MU, WD, True)
    with pytest.raises(_lib.PtmiError):
        ops.clip_sgd_step_seg(p, g, buf, table, ss, CLIP, "value", 0.0, None, LR, MU, WD, True)
    # S = 0 and n = 0 are no-ops, also with null tables
    assert step(S=0) == 0 and step(n_=0) == 0 and step(S=0, seg=None, chunks=None, C=0) == 0
    assert norm(S=0) == 0 and norm(n_=0) == 0 and norm(S=0, seg=None, first=None, chunks=None, C=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, p_bits) and torch.equal(buf, b_bits), "nothing above may have touched the buffers"
    # a descriptor outside its segment is skipped, not followed
    bad = table.table.clone()
    bad_chunks = bad[2 * table.S + 2:]
    bad_chunks[0], bad_chunks[3] = 50, 7             # chunk 0 starts outside segment 0; chunk 1 names segment 7 of 2
    assert step(chunks=bad_chunks) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, p_bits) and torch.equal(buf, b_bits)


# ============================================================================ the trainer
KEY = "SOLVER.CLIP_GRADIENTS."


def _cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_s2c.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "UNSUPNET.BURN_UP_STEP", 0, "SOLVER.IMG_PER_BATCH_LABEL", 1,
        "SOLVER.IMG_PER_BATCH_UNLABEL", 1, "SOLVER.WARMUP_ITERS", 0, "SEED", 0] + list(opts))


def _one_step(cfg, batch):
    """a fresh trainer from SEED, one mutual-learning step; what the optimiser tail saw is kept on the trainer"""
    from probabilisticteacher_amd import _lib
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    seed_all_rng(cfg.SEED)
    tr = PTrainer(cfg)
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
        tr.metrics = dict(tr.run_step(batch))
    finally:
        _lib.call = call
    torch.cuda.synchronize()
    return tr


@pytest.fixture(scope="module")
def trainers():
    from bench import synth_records
    from probabilisticteacher_amd.engine.flat import segment_offsets
    plain_cfg = _cfg()
    gen = torch.Generator().manual_seed(77)
    K = plain_cfg.MODEL.ROI_HEADS.NUM_CLASSES
    assert K == 1
    batch = tuple(synth_records(gen, 1, 192, 256, K, DEV) for _ in range(4))
    plain = _one_step(plain_cfg, batch)
    # the clip value comes from the gradient this very step produces: the median of the per-parameter norms of the globally
    # scaled gradient, so that about half of the parameters are clipped
    offs = segment_offsets(plain.student)
    g = plain.seen[1].cpu()
    gs = g * _global_scale(g)
    norms = torch.stack([gs[a:b].norm() for a, b in zip(offs[:-1], offs[1:])])
    v = float(norms[norms > 0].median()) * 1.01
    on = [KEY + "ENABLED", True, KEY + "CLIP_TYPE", "norm", KEY + "CLIP_VALUE", v]
    clipped = _one_step(_cfg(*on), batch)
    again = _one_step(_cfg(*on), batch)
    off = _one_step(_cfg(KEY + "ENABLED", False, KEY + "CLIP_TYPE", "norm", KEY + "CLIP_VALUE", v), batch)
    return dict(plain=plain, clipped=clipped, again=again, off=off, v=v, offs=offs, norms=norms)


def test_trainer_clipped_step_is_the_torch_restatement(trainers):
    from probabilisticteacher_amd.solver import lr_at
    tr, v, offs, norms = trainers["clipped"], trainers["v"], trainers["offs"], trainers["norms"]
    assert len(offs) - 1 >= 30 and offs[-1] == tr.student.n_trainable
    assert int((norms > v * 1.001).sum()) >= 1 and int((norms < v * 0.999).sum()) >= 1, "some parameters clipped, some not"
    p0, g, buf0 = (t.cpu() for t in tr.seen)
    assert torch.equal(g, trainers["plain"].seen[1].cpu()), "SEED 0: the clipped trainer saw the gradient the value came from"
    assert not bool(buf0.any())
    S = tr.cfg.SOLVER
    lr = lr_at(tr.cfg, 0)
    pw, bw = torch_steps(p0, g, offs, 1, "norm", v, False, lr=lr, mu=S.MOMENTUM, wd=S.WEIGHT_DECAY)[0]
    print(f"[clip] trainer: v {v:.4e}, {int((norms > v).sum())} of {len(norms)} clipped, max |dp| "
          f"{float((tr.student.trainable().cpu() - pw).abs().max()):.3e}")
    close(tr.momentum_buf, bw, "trainer momentum")
    close(tr.student.trainable(), pw, "trainer parameters")
    # grad_norm stays the global pre-clip norm
    assert abs(tr.metrics["grad_norm"] - float(g.double().norm())) <= 1e-5 * float(g.double().norm())
    assert tr.metrics["grad_norm"] == trainers["plain"].metrics["grad_norm"]


def test_trainer_clipping_changes_the_step(trainers):
    a, b = trainers["clipped"], trainers["plain"]
    assert not torch.equal(a.student.trainable(), b.student.trainable())
    bw = b.momentum_buf.cpu().double()
    assert not bool(((a.momentum_buf.cpu().double() - bw).abs() <= ATOL + RTOL * bw.abs()).all()), "not within the tolerance either"
    assert torch.equal(a.student.flat[a.student.n_trainable:], b.student.flat[b.student.n_trainable:])     # frozen part


def test_trainer_clipped_step_is_reproducible(trainers):
    a, b = trainers["clipped"], trainers["again"]
    assert a.deterministic and a.metrics.keys() == b.metrics.keys()
    assert {k: v for k, v in a.metrics.items() if k != "data_time"} == {k: v for k, v in b.metrics.items() if k != "data_time"}
    assert torch.equal(a.student.flat, b.student.flat) and torch.equal(a.momentum_buf, b.momentum_buf)


def test_trainer_disabled_is_the_step_without_the_keys(trainers):
    a, b = trainers["off"], trainers["plain"]
    assert a._segments is None and b._segments is None
    assert torch.equal(a.student.flat, b.student.flat) and torch.equal(a.momentum_buf, b.momentum_buf)
    assert torch.equal(a.teacher.flat, b.teacher.flat)


def test_trainer_launches(trainers):
    """ENABLED False launches what it launched before; "norm" adds the norm pass and swaps the update"""
    plain, off, clipped = (trainers[k].calls for k in ("plain", "off", "clipped"))
    assert plain == off and plain[-2:] == ["ptmi_sumsq", "ptmi_clip_sgd_step"]
    assert not [n for n in plain if n.endswith("_seg") or n == "ptmi_seg_gradnorm"]
    assert clipped[:-3] == plain[:-2] and clipped[-3:] == ["ptmi_sumsq", "ptmi_seg_gradnorm", "ptmi_clip_sgd_step_seg"]
