"""GPU guard-band tests (pytest -m gpu) of the caller-sized workspaces outside the convolution family: every kernel that trusts a
`*_ws_floats` / `*_ws_bytes` query gets a tests/guarded.py payload of EXACTLY the queried size (production hands out grow-only
buffers of at least 256 bytes, the other tests fresh blocks that the allocator rounds up: a size formula one partial short has never
been binding), with 4096 guard elements on each side; the outputs are guarded too.  Results against the references of the existing
tests (tests/test_ops_gpu.py, tests/test_p8_gpu.py, tests/test_deterministic_gpu.py), smallest shapes that take the workspace
path.  Nothing here asserts how much of a workspace is used."""
import math

import numpy as np
import pytest
import torch

from oracle import d2, pt as opt
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
GUARD = 4096


def g(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, rtol, atol, what=""):
    a = a.detach().cpu().double().numpy()
    b = b.detach().cpu().double().numpy()
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max abs err {np.nanmax(err):.3e}, max |ref| {np.abs(b).max():.3e}"


def _api():
    from probabilisticteacher_amd import _lib, ops
    return _lib, _lib.load(), ops._stream


def _p(gd):
    from probabilisticteacher_amd import ops
    return ops._ptr(None if gd is None else gd.payload)


def _ro(t):
    return Guarded.of(t, GUARD, GUARD, DEV).snapshot()


def _out(shape, dtype=F32):
    return Guarded(shape, dtype, GUARD, GUARD, DEV)


def _ws(count, dtype=F32):
    assert count > 0, "this shape is meant to take the workspace path"
    return Guarded((count,), dtype, GUARD, GUARD, DEV)


def _after(outs, ros, what):
    torch.cuda.synchronize()
    for name, o in outs.items():
        o.assert_guards_intact(f"{what}: {name}")
    for name, r in ros.items():
        r.assert_unchanged(f"{what}: {name}")


@pytest.mark.parametrize("m,n,k", [(9, 130, 4099), (200, 300, 5000)])
def test_gemm_split_k_in_an_exactly_sized_workspace(m, n, k):
    _lib, lib, stream = _api()
    nws = lib.ptmi_gemm_ws_floats(m, n, k, 1)
    gen = g(m + n + k)
    a, b, bias = torch.randn(m, k, generator=gen), torch.randn(k, n, generator=gen), torch.randn(n, generator=gen)
    ref = torch.relu(a.double() @ b.double() + bias.double())
    ag, bg, biasg, c, ws = _ro(a), _ro(b), _ro(bias), _out((m, n)), _ws(nws)
    _lib.call("ptmi_gemm_f32", _p(ag), _p(bg), _p(c), _p(biasg), m, n, k, k, n, n, 0, 0, 2, 1, 0, 1, 0, 0, 0, _p(ws), int(nws), stream())
    _after({"c": c, "ws": ws}, {"a": ag, "b": bg, "bias": biasg}, f"gemm_f32 split-K {m}x{n}x{k}")
    assert c.unwritten() == 0
    close(c.payload, ref, 1e-4, 2e-4 * math.sqrt(k / 1000.0), "split-K gemm")


def test_p8_gemm_nt_split_k_in_an_exactly_sized_workspace():
    """(64, 1024, 25088): few tiles, long k -- the split shape of tests/test_p8_gpu.py; operands packed by ptmi_p8m_pack into guarded
    buffers of ptmi_p8m_elems elements"""
    _lib, lib, stream = _api()
    from tests.test_p8_gpu import rb
    m, n, k = 64, 1024, 25088
    a, b, bias = rb(torch.randn(m, k, generator=g(51))), rb(torch.randn(n, k, generator=g(52))), torch.randn(n, generator=g(53))
    want = a.double() @ b.double().t() + bias.double()
    packed = []
    for src, rows in ((a, m), (b, n)):
        sg = _ro(src)
        assert lib.ptmi_p8m_elems(rows, k) == -(-k // 8) * rows * 8
        dst = _out((-(-k // 8), rows, 8), torch.bfloat16)
        _lib.call("ptmi_p8m_pack", _p(sg), _p(dst), rows, k, k, 1, stream())
        _after({"packed operand": dst}, {"source": sg}, f"p8m_pack {rows}x{k}")
        assert dst.unwritten() == 0
        packed.append(dst.snapshot())
    biasg, c, ws = _ro(bias), _out((m, n)), _ws(lib.ptmi_p8_gemm_nt_ws_floats(m, n, k))
    _lib.call("ptmi_p8_gemm_nt", _p(packed[0]), _p(packed[1]), _p(c), _p(biasg), _p(ws), m, n, k, n, 0, stream())
    _after({"c": c, "ws": ws}, {"a": packed[0], "b": packed[1], "bias": biasg}, "p8_gemm_nt split-K")
    assert c.unwritten() == 0
    err = float((c.payload.cpu().double() - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()) + 4e-6 * math.sqrt(k) + 1e-5, f"p8_gemm_nt: max abs err {err:.3e}"


@pytest.mark.parametrize("rows,cols", [(5000, 7), (4096, 60)])
def test_colsum_in_an_exactly_sized_workspace(rows, cols):
    _lib, lib, stream = _api()
    a = torch.randn(rows, cols, generator=g(rows + cols))
    ref = a.double().sum(0)
    ag, out, ws = _ro(a), _out((cols,)), _ws(lib.ptmi_colsum_ws_floats(rows, cols))
    _lib.call("ptmi_colsum_ws", _p(ag), _p(out), _p(ws), rows, cols, 0, stream())
    _after({"out": out, "ws": ws}, {"a": ag}, f"colsum_ws {rows}x{cols}")
    assert out.unwritten() == 0
    close(out.payload, ref, 1e-5, 1e-5 * math.sqrt(rows), "colsum")


def _roi_case(fh, fw):
    """the map, boxes (partly outside, beyond the far border, tiny, whole image, many times the map) and float32 oracle results of
    test_roi_align, rows grouped by image"""
    gen = g(23)
    feat = torch.randn(2, 18, fh, fw, generator=gen)
    n = 40
    cx, cy = torch.rand(n, generator=gen) * fw * 16, torch.rand(n, generator=gen) * fh * 16
    bw, bh = 4.0 + torch.rand(n, generator=gen) * fw * 16 * 0.7, 4.0 + torch.rand(n, generator=gen) * fh * 16 * 0.7
    boxes = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    boxes[0] = torch.tensor([-30.0, -20.0, 40.0, 35.0])
    boxes[1] = torch.tensor([fw * 16 - 96.0, fh * 16 - 100.0, fw * 16 + 24.0, fh * 16 + 20.0])
    boxes[2] = torch.tensor([10.0, 10.0, 10.5, 10.2])
    boxes[3] = torch.tensor([0.0, 0.0, fw * 16.0, fh * 16.0])
    boxes[4] = torch.tensor([-9000.0, -7000.0, 9500.0, 8000.0])
    rois = torch.cat([torch.randint(0, 2, (n, 1), generator=gen).float(), boxes], 1)
    rois = rois[torch.argsort(rois[:, 0], stable=True)]
    offs = torch.tensor([0, int((rois[:, 0] == 0).sum()), n], dtype=I32)
    fr = feat.clone().requires_grad_()
    ref = d2.roi_align(fr, rois, 7, 1 / 16)
    gy = torch.randn(ref.shape, generator=gen)
    ref.backward(gy)
    return feat, rois, offs, ref.detach(), gy, fr.grad


@pytest.mark.parametrize("fh,fw", [(25, 31), (70, 27)])
def test_roi_align_grouped_kernels_in_exactly_sized_workspaces(fh, fw):
    _lib, lib, stream = _api()
    feat, rois, offs, ref, gy, dref = _roi_case(fh, fw)
    n, c, r = feat.shape[0], feat.shape[1], rois.shape[0]
    fg, rg, og, gyg = _ro(feat), _ro(rois), _ro(offs), _ro(gy)
    out, ws = _out((r, c, 7, 7)), _ws(lib.ptmi_roi_align_ws_bytes(r, fh, fw), U8)
    _lib.call("ptmi_roi_align_fwd_grouped", _p(fg), _p(rg), _p(og), _p(out), _p(ws), n, c, fh, fw, r, 7, 1 / 16, stream())
    _after({"out": out, "ws": ws}, {"feat": fg, "rois": rg, "img_offsets": og}, f"roi_align_fwd_grouped {fh}x{fw}")
    assert out.unwritten() == 0
    close(out.payload, ref, 1e-5, 1e-5, "grouped forward vs the oracle")
    for entry, extra in (("ptmi_roi_align_bwd_grouped", ()), ("ptmi_roi_align_bwd_det", (1, 0))):
        dfeat, wsb = _out((n, c, fh, fw)), _ws(lib.ptmi_roi_align_bwd_ws_bytes(r, fh, fw), U8)
        _lib.call(entry, _p(gyg), _p(rg), _p(og), _p(dfeat), _p(wsb), n, c, fh, fw, r, 7, 1 / 16, stream(), *extra)
        _after({"dfeat": dfeat, "ws": wsb}, {"dout": gyg, "rois": rg, "img_offsets": og}, f"{entry} {fh}x{fw}")
        assert dfeat.unwritten() == 0, f"{entry}: every element of dfeat is written (no zero fill needed)"
        close(dfeat.payload, dref, 1e-4, 1e-4, entry)


def test_segsort_in_an_exactly_sized_workspace():
    _lib, lib, stream = _api()
    sizes = [300, 0, 5, 17000]
    total = sum(sizes)
    keys = torch.randn(total, generator=g(41))
    keys[10:20] = keys[10]                     # ties -> stable order
    offs = torch.tensor([0] + list(np.cumsum(sizes)), dtype=I32)
    nbytes = lib.ptmi_segsort_ws_bytes(total, len(sizes))
    kg, og, sk, si, ws = _ro(keys), _ro(offs), _out((total,)), _out((total,), I32), _ws(nbytes, U8)
    _lib.call("ptmi_segsort_desc", _p(kg), _p(sk), _p(si), total, len(sizes), _p(og), _p(ws), int(nbytes), stream())
    _after({"keys_out": sk, "idx_out": si, "ws": ws}, {"keys_in": kg, "seg_offsets": og}, "segsort_desc")
    assert sk.unwritten() == 0 and si.unwritten() == 0
    for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
        rk, ri = torch.sort(keys[a:b], descending=True, stable=True)
        assert torch.equal(sk.payload[a:b].cpu(), rk)
        assert torch.equal(si.payload[a:b].cpu().long(), ri)


def test_nms_in_an_exactly_sized_workspace():
    _lib, lib, stream = _api()
    counts, thr, max_keep = [300, 0, 1, 65, 1000], 0.7, 2000
    gen = g(sum(counts))
    boxes_all, keep_ref = [], []
    for c in counts:
        ctr = torch.rand(c, 2, generator=gen) * torch.tensor([1333.0, 800.0])
        wh = torch.exp(torch.rand(c, 2, generator=gen) * 3.0 + 2.5)
        b = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
        b = b[d2.descending_order(torch.rand(c, generator=gen))]
        boxes_all.append(b)
        keep_ref.append(d2.nms(b, torch.arange(c, 0, -1).float(), thr)[:max_keep])
    offs = torch.tensor([0] + list(np.cumsum(counts)), dtype=I32)
    nimg = len(counts)
    bg, og = _ro(torch.cat(boxes_all, 0)), _ro(offs)
    keep, cnt = _out((nimg, max_keep), I32), _out((nimg,), I32)
    ws = _ws(lib.ptmi_nms_ws_bytes(max(counts), nimg), U8)
    _lib.call("ptmi_nms_batched", _p(bg), _p(og), None, nimg, max(counts), thr, max_keep, _p(keep), _p(cnt), _p(ws), stream())
    _after({"keep": keep, "keep_count": cnt, "ws": ws}, {"boxes": bg, "seg_offsets": og}, "nms_batched")
    assert cnt.unwritten() == 0
    for i, ref in enumerate(keep_ref):
        k = int(cnt.payload[i])
        assert k == len(ref), f"image {i}: kept {k} vs {len(ref)}"
        assert torch.equal(keep.payload[i, :k].cpu().long(), ref), f"image {i}: keep lists differ"


@pytest.mark.parametrize("rows,n_dst", [(4096, 9), (700, 150)])
def test_get_deltas_source_gradient_det_in_an_exactly_sized_workspace(rows, n_dst):
    _lib, lib, stream = _api()
    gen = g(rows + n_dst)
    cell = torch.rand(n_dst, 2, generator=gen) * 200 + 30
    anchors = torch.cat([-cell / 2, cell / 2], 1)
    idx = torch.randint(0, n_dst, (rows,), generator=gen)
    shift = torch.rand(rows, 2, generator=gen) * 600
    tgt = torch.cat([shift, shift + 20 + torch.rand(rows, 2, generator=gen) * 300], 1)
    dd = torch.randn(rows, 4, generator=gen)
    wts = (1.0, 1.0, 1.0, 1.0)
    src = anchors[idx] + torch.cat([shift, shift], 1)
    s64 = src.double().requires_grad_()
    opt.get_deltas(s64, tgt.double(), wts).mul(dd.double()).sum().backward()
    want = torch.zeros(n_dst, 4, dtype=torch.float64).index_add_(0, idx, s64.grad)
    sg, tg, dg, ig = _ro(src), _ro(tgt), _ro(dd), _ro(idx)
    dsrc, ws = _out((n_dst, 4)), _ws(lib.ptmi_get_deltas_bwd_src_det_ws_floats(rows, n_dst))
    _lib.call("ptmi_get_deltas_bwd_src_det", _p(sg), _p(tg), _p(dg), _p(ig), rows, *wts, _p(dsrc), n_dst, _p(ws), stream())
    _after({"dsrc": dsrc, "ws": ws}, {"src": sg, "tgt": tg, "ddeltas": dg, "src_index": ig}, f"get_deltas_bwd_src_det {rows}->{n_dst}")
    assert dsrc.unwritten() == 0, "stage 2 writes every element of dsrc (no zero fill needed)"
    close(dsrc.payload, want, 1e-4, 1e-6, "get_deltas d/dsrc det")
