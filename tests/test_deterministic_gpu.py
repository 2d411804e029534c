"""The order-independent backward kernels (ops.deterministic) and the run-to-run reproducible train step (SEED >= 0).

Kernels: heavily overlapping ROIs at the training shape (C = 512, 50 x 84 map, several hundred ROIs per image, many identical or
nested).  The deterministic kernel run twice must give `torch.equal` results; it AND the atomic kernel are compared with the
float64 restatements of tests/roi_pooler_ref.py at the tolerance tests/test_roi_pooler_gpu.py applies to the atomic kernel
(rtol 1e-4 / atol 1e-4) -- both against the reference, not against each other.  get_deltas: torch autograd in float64 at the
tolerance of tests/test_ops_gpu.py (rtol 1e-4 / atol 1e-6).  Every comparison is between exactly two runs."""
import os

import numpy as np
import pytest
import torch

from oracle import pt as opt
from tests import roi_pooler_ref as ref
from tests.helpers import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, FH, FW = 512, 50, 84
PER_IMG = 300


def _overlapping_rois(gen, n_img=2, per_img=PER_IMG):
    """per image: 60 random boxes, each of them repeated, 3 shrinking copies nested in each of 40, boxes over the border"""
    h, w = FH * 16.0, FW * 16.0
    rows = []
    for b in range(n_img):
        cx, cy = torch.rand(60, generator=gen) * w, torch.rand(60, generator=gen) * h
        bw, bh = 24 + torch.rand(60, generator=gen) * 420, 24 + torch.rand(60, generator=gen) * 330
        base = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
        base[58] = torch.tensor([-40.0, -30.0, 200.0, 160.0])              # partly outside
        base[59] = torch.tensor([0.0, 0.0, w, h])                          # the whole image
        boxes = [base, base.clone()]                                       # identical pairs
        for k in (1, 2, 3):                                                # nested
            m = base[:40].clone()
            dw, dh = (m[:, 2] - m[:, 0]) * 0.1 * k, (m[:, 3] - m[:, 1]) * 0.1 * k
            m[:, 0] += dw; m[:, 2] -= dw; m[:, 1] += dh; m[:, 3] -= dh
            boxes.append(m)
        boxes.append(base[:per_img - 240])
        bx = torch.cat(boxes)[torch.randperm(per_img, generator=gen)]
        rows.append(torch.cat([torch.full((per_img, 1), float(b)), bx], 1))
    return torch.cat(rows).float()


@pytest.fixture(scope="module")
def inputs():
    gen = torch.Generator().manual_seed(41)
    rois = _overlapping_rois(gen)
    gy = torch.randn(rois.shape[0], C, 7, 7, generator=gen)
    feat = torch.randn(2, C, FH, FW, generator=gen)
    offs = torch.tensor([0, PER_IMG, 2 * PER_IMG], dtype=torch.int32, device=DEV)
    return feat, rois, gy, offs


@pytest.mark.parametrize("aligned,ratio", [(1, 0), (1, 2), (0, 0), (0, 2)])
def test_roi_align_backward_det(inputs, aligned, ratio):
    from probabilisticteacher_amd import _lib, ops
    feat, rois, gy, offs = inputs
    want = ref.roi_align_backward(gy.numpy(), rois.numpy(), feat.shape, 7, 1 / 16, bool(aligned), ratio)
    gd, rd = gy.to(DEV), rois.to(DEV)
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call, grads = spy, []
    try:
        for _ in range(2):
            fd = feat.to(DEV).requires_grad_()
            with ops.deterministic(True):
                assert ops.is_deterministic()
                ops.roi_align(fd, rd, 7, 1 / 16, offs, bool(aligned), ratio).backward(gd)
            grads.append(fd.grad)
        assert not ops.is_deterministic()
    finally:
        _lib.call = real
    assert names.count("ptmi_roi_align_bwd_det") == 2 and not [n for n in names if "bwd" in n and not n.endswith("_det")]
    assert torch.equal(grads[0], grads[1]), "deterministic ROIAlign backward: two runs, the same bits"
    print(f"[det] aligned={aligned} ratio={ratio} max |err| det {np.abs(grads[0].cpu().numpy() - want).max():.3e}")
    close(grads[0].cpu().numpy(), want, 1e-4, 1e-4, f"roi_align bwd det aligned={aligned} ratio={ratio}")
    # rows not grouped by image: the wrapper groups them (stable), the sums are those of the grouped call
    perm = torch.randperm(rois.shape[0], generator=torch.Generator().manual_seed(5))
    fd = feat.to(DEV).requires_grad_()
    with ops.deterministic(True):
        ops.roi_align(fd, rd[perm.to(DEV)], 7, 1 / 16, None, bool(aligned), ratio).backward(gd[perm.to(DEV)])
    close(fd.grad.cpu().numpy(), want, 1e-4, 1e-4, "roi_align bwd det, ungrouped rows")
    # the atomic kernel at the same tolerance on the same inputs
    fa = feat.to(DEV).requires_grad_()
    ops.roi_align(fa, rd, 7, 1 / 16, None, bool(aligned), ratio).backward(gd)
    print(f"[det] aligned={aligned} ratio={ratio} max |err| atomic {np.abs(fa.grad.cpu().numpy() - want).max():.3e}")
    close(fa.grad.cpu().numpy(), want, 1e-4, 1e-4, f"roi_align bwd atomic aligned={aligned} ratio={ratio}")


def test_roi_align_backward_det_refuses_what_it_cannot_serve(inputs):
    """no quiet fall-back to the atomic scatter: a pooled size the band kernel does not serve is an error"""
    from probabilisticteacher_amd import _lib, ops
    feat, rois, gy, offs = inputs
    fd = feat[:, :8].to(DEV).requires_grad_()
    out = ops.roi_align(fd, rois.to(DEV), 5, 1 / 16, offs)
    with ops.deterministic(True), pytest.raises(_lib.PtmiError, match="not served"):
        out.backward(torch.ones_like(out))


def test_roi_pool_backward_det(inputs):
    from probabilisticteacher_amd import ops
    feat, rois, gy, offs = inputs
    _, arg = ref.roi_pool(feat.numpy(), rois.numpy(), 7, 1 / 16)
    want = ref.roi_pool_backward(gy.numpy(), arg, rois.numpy(), feat.shape)
    gd, rd = gy.to(DEV), rois.to(DEV)
    grads = []
    for _ in range(2):
        fd = feat.to(DEV).requires_grad_()
        with ops.deterministic(True):
            ops.roi_pool(fd, rd, 7, 1 / 16, img_offsets=offs).backward(gd)
        grads.append(fd.grad)
    assert torch.equal(grads[0], grads[1]), "deterministic ROIPool backward: two runs, the same bits"
    print(f"[det] roi_pool max |err| det {np.abs(grads[0].cpu().numpy() - want).max():.3e}")
    close(grads[0].cpu().numpy(), want, 1e-4, 1e-4, "roi_pool bwd det")
    perm = torch.randperm(rois.shape[0], generator=torch.Generator().manual_seed(6)).to(DEV)
    fd = feat.to(DEV).requires_grad_()
    with ops.deterministic(True):
        ops.roi_pool(fd, rd[perm], 7, 1 / 16).backward(gd[perm])
    close(fd.grad.cpu().numpy(), want, 1e-4, 1e-4, "roi_pool bwd det, ungrouped rows")
    fa = feat.to(DEV).requires_grad_()
    ops.roi_pool(fa, rd, 7, 1 / 16).backward(gd)
    print(f"[det] roi_pool max |err| atomic {np.abs(fa.grad.cpu().numpy() - want).max():.3e}")
    close(fa.grad.cpu().numpy(), want, 1e-4, 1e-4, "roi_pool bwd atomic")


@pytest.mark.parametrize("fh,fw", [(64, 128), (100, 120)])
def test_roi_pool_backward_det_at_the_lds_tile_limit(fh, fw):
    """the kernel holds a plane in LDS tiles of 8192 cells: a plane of exactly one tile (64 x 128) and one of two tiles, the second
    partial (100 x 120 = 12000 cells); images with 0, 3 and 21 ROIs, the edge boxes of tests/roi_pooler_ref.py"""
    from probabilisticteacher_amd import ops
    counts, c = (0, 3, 21), 3
    rois_np, offs_np = ref.counts_to_rois(ref.box_set(sum(counts), fh, fw, 1 / 16, 9), counts)
    gen = torch.Generator().manual_seed(fh + fw)
    feat = torch.randn(len(counts), c, fh, fw, generator=gen)
    gy = torch.randn(len(rois_np), c, 7, 7, generator=gen)
    _, arg = ref.roi_pool(feat.numpy(), rois_np, 7, 1 / 16)
    assert (arg >= 8192).any() == (fh * fw > 8192) and (arg == fh * fw - 1).any() and (arg == -1).any()
    want = ref.roi_pool_backward(gy.numpy(), arg, rois_np, feat.shape)
    gd, rd, offs = gy.to(DEV), torch.from_numpy(rois_np).to(DEV), torch.from_numpy(offs_np).to(DEV)
    grads = []
    for _ in range(2):
        fd = feat.to(DEV).requires_grad_()
        with ops.deterministic(True):
            ops.roi_pool(fd, rd, 7, 1 / 16, img_offsets=offs).backward(gd)
        grads.append(fd.grad)
    assert torch.equal(grads[0], grads[1]), "deterministic ROIPool backward: two runs, the same bits"
    close(grads[0].cpu().numpy(), want, 1e-4, 1e-4, f"roi_pool bwd det {fh}x{fw}")
    assert not grads[0][0].any(), "an image without ROIs gets an exactly zero gradient"
    perm = torch.randperm(len(rois_np), generator=torch.Generator().manual_seed(6)).to(DEV)
    fd = feat.to(DEV).requires_grad_()
    with ops.deterministic(True):
        ops.roi_pool(fd, rd[perm], 7, 1 / 16).backward(gd[perm])
    close(fd.grad.cpu().numpy(), want, 1e-4, 1e-4, "roi_pool bwd det, ungrouped rows")
    fa = feat.to(DEV).requires_grad_()
    ops.roi_pool(fa, rd, 7, 1 / 16).backward(gd)
    close(fa.grad.cpu().numpy(), want, 1e-4, 1e-4, "roi_pool bwd atomic")


@pytest.mark.parametrize("rows,n_dst", [(6000, 9), (4096, 9), (700, 150)])
def test_get_deltas_source_gradient_det(rows, n_dst):
    """thousands of rows onto 9 anchors (one destination tile, two row chunks), and more destinations than one tile holds"""
    from probabilisticteacher_amd import ops
    gen = torch.Generator().manual_seed(rows + n_dst)
    cell = torch.rand(n_dst, 2, generator=gen) * 200 + 30
    anchors = torch.cat([-cell / 2, cell / 2], 1)
    idx = torch.randint(0, n_dst, (rows,), generator=gen)
    shift = torch.rand(rows, 2, generator=gen) * 600
    tgt = torch.cat([shift, shift + 20 + torch.rand(rows, 2, generator=gen) * 300], 1)
    dd = torch.randn(rows, 4, generator=gen)
    wts = (1.0, 1.0, 1.0, 1.0)
    src32 = anchors[idx] + torch.cat([shift, shift], 1)          # the fp32 boxes both sides see
    s64 = src32.double().requires_grad_()
    opt.get_deltas(s64, tgt.double(), wts).mul(dd.double()).sum().backward()
    want = torch.zeros(n_dst, 4, dtype=torch.float64).index_add_(0, idx, s64.grad)
    src = src32.to(DEV)
    got = []
    for _ in range(2):
        with ops.deterministic(True):
            got.append(ops.get_deltas_bwd_src(src, tgt.to(DEV), dd.to(DEV), idx.to(DEV), n_dst, wts))
    assert torch.equal(got[0], got[1]), "deterministic get_deltas source gradient: two runs, the same bits"
    close(got[0].cpu(), want, 1e-4, 1e-6, "get_deltas d/dsrc det")
    close(ops.get_deltas_bwd_src(src, tgt.to(DEV), dd.to(DEV), idx.to(DEV), n_dst, wts).cpu(), want, 1e-4, 1e-6, "get_deltas d/dsrc atomic")
    # the autograd path (row i is its own destination): det and atomic entry, same reference
    s_r = src.cpu().double().requires_grad_()
    opt.get_deltas(s_r, tgt.double(), wts).mul(dd.double()).sum().backward()
    for flag in (True, False):
        s_d = src.clone().requires_grad_()
        with ops.deterministic(flag):
            ops.get_deltas(s_d, tgt.to(DEV), wts).mul(dd.to(DEV)).sum().backward()
        close(s_d.grad.cpu(), s_r.grad, 1e-4, 1e-6, f"get_deltas autograd d/dsrc deterministic={flag}")


# ============================================================================ the full step
def _cfg(*opts):
    from probabilisticteacher_amd.config import setup_cfg
    return setup_cfg(os.path.join(ROOT, "configs/pt/final_c2f.yaml"), [
        "MODEL.DEVICE", DEV, "MODEL.VGG.PRETRAIN", "", "MODEL.ANCHOR_GENERATOR.NAME", "DifferentiableAnchorGenerator",
        "UNSUPNET.BURN_UP_STEP", 2, "SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2] + list(opts))


def _batches(cfg, seed=77, steps=5, n=2, dev=DEV):
    from bench import synth_records
    gen = torch.Generator().manual_seed(seed)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    return [tuple(synth_records(gen, n, 256, 384, K, dev) for _ in range(4)) for _ in range(steps)]


def _run(cfg, batches, **kw):
    """a fresh trainer (weights from SEED, as train_net.py seeds them), two burn-in + three mutual-learning steps"""
    from probabilisticteacher_amd.engine import PTrainer
    from probabilisticteacher_amd.seeding import seed_all_rng
    seed_all_rng(cfg.SEED if cfg.SEED >= 0 else 0)
    tr = PTrainer(cfg, **kw)
    metrics = []
    for b in batches:
        m = dict(tr.run_step(b))
        m.pop("data_time", None)
        metrics.append(m)
    torch.cuda.synchronize()
    return tr, metrics


def _assert_same_run(a, b, what):
    (ta, ma), (tb, mb) = a, b
    for i, (x, y) in enumerate(zip(ma, mb)):
        assert x.keys() == y.keys() and len(x) >= 4
        diff = {k: (x[k], y[k]) for k in x if not (x[k] == y[k])}
        assert not diff, f"{what}: step {i} metrics differ: {diff}"
    assert torch.equal(ta.student.flat, tb.student.flat), f"{what}: student parameters differ"
    assert torch.equal(ta.teacher.flat, tb.teacher.flat), f"{what}: teacher parameters differ"


def test_two_trainers_with_one_seed_train_bit_for_bit():
    cfg = _cfg("SEED", 3)
    batches = _batches(cfg)
    a = _run(cfg, batches)
    assert a[0].deterministic and a[0].iter == 5 and any(k.endswith("_unsup") for k in a[1][-1])
    b = _run(cfg, batches)
    _assert_same_run(a, b, "SEED 3")


@pytest.fixture
def rccl_world1():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    yield
    dist.destroy_process_group()


def test_two_trainers_with_one_seed_through_the_gradient_reducer(rccl_world1):
    from probabilisticteacher_amd import ops
    cfg = _cfg("SEED", 3)
    batches = _batches(cfg)
    a = _run(cfg, batches, force_grad_reducer=True)
    assert a[0].reducer.active and ops._TILE_SCHEDULE == "static" and ops._WGRAD_WAVES == 1, "deterministic keeps the 1-GPU policy"
    b = _run(cfg, batches, force_grad_reducer=True)
    _assert_same_run(a, b, "SEED 3, gradient reducer")


def _two_rank_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = f"cuda:{rank}"
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
    try:
        cfg = _cfg("SEED", 3, "MODEL.DEVICE", dev, "SOLVER.IMG_PER_BATCH_LABEL", 2 * world, "SOLVER.IMG_PER_BATCH_UNLABEL", 2 * world)
        batches = _batches(cfg, seed=77 + rank, dev=dev)
        a = _run(cfg, batches)
        b = _run(cfg, batches)
        _assert_same_run(a, b, f"SEED 3, rank {rank} of {world}")
        q.put((rank, "ok"))
    except BaseException as e:                        # noqa: BLE001 -- reported to the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_trainers_with_one_seed_on_two_ranks():
    if torch.cuda.device_count() < 2:
        pytest.skip(f"{torch.cuda.device_count()} GPU visible: the 2-rank RCCL run needs 2")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, 29543, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(60)
    assert got == {0: "ok", 1: "ok"}, got


def test_default_routing_and_amp():
    """SEED -1: ops.deterministic is off inside the step and the backward goes through the existing entries.  SOLVER.AMP.ENABLED
    flows through the same two kernels (p8.roi_align_linear's backward calls ops.roi_align_bwd_grouped), so it is in scope: a
    SEED 3 AMP trainer pair is bit-identical too."""
    from probabilisticteacher_amd import _lib, ops
    from probabilisticteacher_amd.engine import PTrainer
    cfg = _cfg("SEED", -1)
    batches = _batches(cfg, steps=3)
    names, flags = [], []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        if name.startswith(("ptmi_roi_align_bwd", "ptmi_get_deltas_bwd")):
            flags.append(ops.is_deterministic())
        return real(name, *a)
    _lib.call = spy
    try:
        tr, _ = _run(cfg, batches)
    finally:
        _lib.call = real
    assert not tr.deterministic and tr._rng is None and tr._key_gen is None
    assert flags and not any(flags) and not ops.is_deterministic()
    assert "ptmi_roi_align_bwd_grouped" in names and "ptmi_get_deltas_bwd_src" in names
    assert not [n for n in names if n.endswith("_det")], "SEED -1 launches what it launched before"
    names.clear()
    _lib.call = spy
    try:
        PTrainer(_cfg("SEED", 3)).run_step(batches[0])
    finally:
        _lib.call = real
    assert "ptmi_roi_align_bwd_det" in names and "ptmi_roi_align_bwd_grouped" not in names
    amp = _cfg("SEED", 3, "SOLVER.AMP.ENABLED", True)
    a = _run(amp, batches)
    b = _run(amp, batches)
    _assert_same_run(a, b, "SEED 3, AMP")
