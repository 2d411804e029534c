"""GPU (pytest -m gpu): the GEMM family through the C ABI -- ptmi_gemm_f32 / ptmi_gemm_bf16 / ptmi_rowsum_batched (csrc/gemm.hip),
ptmi_p8m_pack / ptmi_p8_gemm_nt (csrc/p8gemm.hip) -- against the float64 reference of tests/gemm_ref.py with its fp32 yardstick
(see that docstring: scale-aware error, hard bound (K + 3) 2^-24, tight bound 4 x err(seq32)), over every option and K tail.

Every operand is the payload of a tests/guarded.py buffer, so every word a kernel may fetch but must not use -- lda / ldb above
natural, stride gaps, the guards -- is a NaN; after every launch: output guards intact, unwritten() == exactly the padding elements
of the output, read-only operands bit-unchanged, a second launch gives the same bits, the result finite and at parity.

 (1) plain path: 4 layouts x bias_mode {0, 1, 2} x ReLU x accumulate at 130 x 66 x 70, lda + 3, ldb + 5, ldc + 7;
 (2) batched: stride-0 A / stride-0 B / gaps / stride_c > m ldc, with accumulate and both bias modes, 65 x 40 x 33, batch 3;
 (3) split-K: the same 12 epilogues x 4 layouts with ldc = n + 7 at (5, 3, 1027) (S = 4, the K % 4 fix-up in the last slice),
     (9, 130, 4099), (130, 200, 1500); when the workspace query is 0; a workspace one float short takes the plain path;
 (4) K sweep 1 .. 97 over every residue of 4, 8, 32 on both sides of a stage, both kernels, 4 layouts;
 (5) M / N edges incl. 641 x 129 (12 tiles on a grid of 16 workgroups);  (6) ptmi_gemm_bf16 rounds to nearest even, bit for bit;
 (7) ptmi_rowsum_batched;  (8) ptmi_p8m_pack with ld above natural, ptmi_p8_gemm_nt with ldc > n and its transposed-store form at
 ldc % 4 != 0 and M % 4 != 0;  (9) refusals that launch nothing.

Measured on an MI355X (first device run of this file): per group the largest err(got) / err(seq32) among its tight-bound cases and the
largest err(got) / hard bound among all its cases.

    group                                        cases | ratio | of hard bound
    (1) plain option matrix                         48 |  0.77 |  0.043
    (2) batched option matrix                       20 |  1.55 |  0.102
    (3) split-K 5 x 3 x 1027                        48 |  1.32 |  0.001
    (3) split-K 9 x 130 x 4099                      48 |  0.19 |  0.000
    (3) split-K 130 x 200 x 1500                    48 |  0.28 |  0.001
    (4) K sweep, fp32                               88 |  1.29 |  0.340
    (4) K sweep, bf16                               88 |  1.33 |  0.214
    (5) M / N edges                                 12 |  1.54 |  0.120
    (7) rowsum_batched                              40 |  0.90 |  0.295
    (8) p8_gemm_nt                                  20 |  1.13 |  0.078
    (8) p8_gemm_nt, transposed store                 5 |  1.00 |  0.028

Every ratio is below 2, so MARGINS is empty.  The long-K groups sit far below 1: four slices (and 16 k per lane half inside a stage)
are partial sums of partial sums, whose error grows more slowly than the yardstick's one long chain.  The largest share of the hard
bound is fp32 at K = 2 (1.72 of 5 units of 2^-24), where that bound decides (gemm_ref.governs).  With one exact product per output
(bf16, K = 1; rowsum of one term) kernel and yardstick are both exact.  Nothing here found a defect: csrc/gemm.hip and
csrc/p8gemm.hip are unchanged.
"""
import numpy as np
import pytest
import torch

from tests import gemm_ref as gr
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096
# a named case whose device ratio exceeds gemm_ref.MARGIN gets its own margin here, with the measured ratio and the reason next to it
MARGINS = {}
STATS = {}


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from probabilisticteacher_amd import _lib, ops
    lib = _lib.load()
    yield _lib, lib, ops
    import os
    if os.environ.get("PTMI_TEST_VERBOSE"):
        for group, (cases, ratio, frac) in STATS.items():
            print(f"[group] {group:44s} cases {cases:4d} | ratio {ratio:5.2f} | of hard bound {frac:6.3f}")


def _p(gd):
    from probabilisticteacher_amd import ops
    return ops._ptr(None if gd is None else gd.payload)


def _stream():
    from probabilisticteacher_amd import ops
    return ops._stream()


def _ro(arr):
    return None if arr is None else Guarded.of(torch.from_numpy(np.ascontiguousarray(arr)), GUARD, GUARD, DEV).snapshot()


def _out(arr):
    """an output buffer holding `arr` (the pattern wherever the launch is to write without reading)"""
    return Guarded.of(torch.from_numpy(np.ascontiguousarray(arr)), GUARD, GUARD, DEV)


def _ws(count):
    return Guarded((int(count),), torch.float32, GUARD, GUARD, DEV) if count else None


def _record(group, spec, ratio, frac):
    cases, r, f = STATS.get(group, (0, 0.0, 0.0))
    STATS[group] = (cases + 1, max(r, ratio if gr.governs(spec) == "tight" else 0.0), max(f, frac))


def _gemm(_lib, spec, a, b, bias, c, ws=None, nws=0):
    _lib.call("ptmi_gemm_bf16" if spec.bf16 else "ptmi_gemm_f32", _p(a), _p(b), _p(c), _p(bias), spec.m, spec.n, spec.k, spec.lda,
              spec.ldb, spec.ldc, spec.ta, spec.tb, spec.bias_mode, spec.relu, spec.accumulate, spec.batch, spec.stride_a,
              spec.stride_b, spec.stride_c, _p(ws), int(nws), _stream())


def _after(spec, c, ros, what, launch):
    """the assertions after every launch that are not parity; `launch(c)` repeats it into a fresh output -> the (batch, m, n) result"""
    torch.cuda.synchronize()
    c.assert_guards_intact(f"{what}: c")
    assert c.unwritten() == spec.padding, f"{what}: {c.unwritten()} output elements hold the fill pattern, {spec.padding} are padding"
    for name, r in ros.items():
        if r is not None:
            r.assert_unchanged(f"{what}: {name}")
    c2 = _out(spec.c0)
    launch(c2)
    torch.cuda.synchronize()
    assert torch.equal(c.raw, c2.raw), f"{what}: a second launch gives other bits"
    got = gr.c_view(c.payload.cpu().numpy(), spec)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite outputs, first at {np.argwhere(~np.isfinite(got))[0]}"
    return got


def run_gemm(api, spec, group, bufs, split=False):
    """one case: launch, all per-launch assertions, parity.  `bufs` caches the guarded operands of specs that share them"""
    _lib, lib, _ = api
    for arr in (spec.a, spec.b):
        if id(arr) not in bufs:
            bufs[id(arr)] = (_ro(arr), arr)                                  # (the array is kept alive with its id)
    a, b, bias = bufs[id(spec.a)][0], bufs[id(spec.b)][0], _ro(spec.bias)
    nws = lib.ptmi_gemm_ws_floats(spec.m, spec.n, spec.k, spec.batch)
    assert (nws > 0) == split, f"{spec.name}: workspace query {nws}"
    wss = []

    def launch(c):
        wss.append(_ws(nws))                                                 # exactly the queried size, fresh (all NaN) per launch
        _gemm(_lib, spec, a, b, bias, c, wss[-1], nws)
    c = _out(spec.c0)
    assert c.unwritten() == spec.padding + (0 if spec.accumulate else spec.batch * spec.m * spec.n)
    launch(c)
    got = _after(spec, c, {"a": a, "b": b, "bias": bias}, spec.name, launch)
    for w in wss:
        if w is not None:
            w.assert_guards_intact(f"{spec.name}: workspace")
    ratio, frac = gr.check(got, spec, MARGINS.get(spec.name, gr.MARGIN))
    _record(group, spec, ratio, frac)
    return c


# ================================================================================================ (1) (2) option matrix
@pytest.mark.parametrize("ta,tb", gr.LAYOUTS)
def test_gemm_option_matrix_plain(api, ta, tb):
    bufs = {}
    cases = gr.plain_cases(ta, tb)
    assert len(cases) == 12 and cases[0].k % 4 == 2 and cases[0].ldc == cases[0].n + 7
    for spec in cases:
        run_gemm(api, spec, "(1) plain option matrix", bufs)


@pytest.mark.parametrize("ta,tb", gr.LAYOUTS)
def test_gemm_option_matrix_batched(api, ta, tb):
    bufs = {}
    cases = gr.batched_cases(ta, tb)
    assert {(s.stride_a == 0, s.stride_b == 0, s.accumulate) for s in cases} >= {(True, False, 0), (False, True, 1), (True, False, 1)}
    assert sum(s.stride_c > s.m * s.ldc for s in cases) >= 2 and {s.bias_mode for s in cases} == {0, 1, 2}
    for spec in cases:
        run_gemm(api, spec, "(2) batched option matrix", bufs)


# ================================================================================================ (3) split-K
@pytest.mark.parametrize("shape", gr.SPLITK_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ta,tb", gr.LAYOUTS)
def test_gemm_option_matrix_split_k(api, ta, tb, shape):
    bufs = {}
    for spec in gr.splitk_cases(ta, tb, shape):
        run_gemm(api, spec, f"(3) split-K {'x'.join(map(str, shape))}", bufs, split=True)


def test_gemm_split_k_workspace_query_and_short_workspace(api):
    _lib, lib, _ = api
    m, n, k = gr.SPLITK_SHAPES[0]
    assert lib.ptmi_gemm_ws_floats(m, n, k, 1) == 4 * m * n, "(5, 3, 1027): four slices of 288, the last one 163 = 5 * 32 + 3 long"
    for mm, nn, kk in gr.SPLITK_SHAPES + [(64, 64, 1024), (200, 300, 5000)]:
        nws = lib.ptmi_gemm_ws_floats(mm, nn, kk, 1)
        assert nws > 0 and nws % (mm * nn) == 0 and nws // (mm * nn) >= 2
        assert lib.ptmi_gemm_ws_floats(mm, nn, kk, 2) == 0 and lib.ptmi_gemm_ws_floats(mm, nn, kk, 3) == 0, "batched: never split"
        assert lib.ptmi_gemm_ws_floats(mm, nn, 1023, 1) == 0 and lib.ptmi_gemm_ws_floats(mm, nn, 512, 1) == 0, "k < 1024: never split"
    # a workspace one float short of the query: the plain path, bit for bit what a call without a workspace gives
    for ta, tb in gr.LAYOUTS:
        spec = gr.splitk_cases(ta, tb, (9, 130, 4099))[7]
        assert spec.bias_mode and spec.relu and spec.accumulate
        nws = lib.ptmi_gemm_ws_floats(spec.m, spec.n, spec.k, 1)
        a, b, bias = _ro(spec.a), _ro(spec.b), _ro(spec.bias)
        outs = []
        for ws, count in ((None, 0), (_ws(nws - 1), nws - 1), (_ws(nws), nws)):
            c = _out(spec.c0)
            _gemm(_lib, spec, a, b, bias, c, ws, count)
            torch.cuda.synchronize()
            c.assert_guards_intact(f"{spec.name}: c")
            if ws is not None:
                ws.assert_guards_intact(f"{spec.name}: workspace of {count}")
                assert (ws.unwritten() == count) == (count < nws), "the short workspace is not touched, the full one is used"
            gr.check(gr.c_view(c.payload.cpu().numpy(), spec), spec)
            outs.append(c)
        assert torch.equal(outs[0].raw, outs[1].raw), f"{spec.name}: short workspace vs none"


# ================================================================================================ (4) (5) K sweep, M / N edges
@pytest.mark.parametrize("ta,tb", gr.LAYOUTS)
def test_gemm_k_sweep_both_kernels(api, ta, tb):
    bufs = {}
    cases = gr.ksweep_cases(ta, tb)
    assert len(cases) == 2 * 22 and all(s.lda > gr.natural_lda(s.m, s.k, ta) and s.ldb > gr.natural_ldb(s.n, s.k, tb) for s in cases)
    for spec in cases:
        run_gemm(api, spec, "(4) K sweep, bf16" if spec.bf16 else "(4) K sweep, fp32", bufs)


@pytest.mark.parametrize("ta,tb", gr.EDGE_LAYOUTS)
def test_gemm_m_n_edges(api, ta, tb):
    for spec in gr.edge_cases(ta, tb):
        assert spec.padding == 0
        c = run_gemm(api, spec, "(5) M / N edges", {})
        assert c.unwritten() == 0, "every tile was drawn exactly where it belongs"


# ================================================================================================ (6) rounding mode
@pytest.mark.parametrize("ta,tb", gr.LAYOUTS)
def test_gemm_bf16_rounds_operands_to_nearest_even(api, ta, tb):
    """K = 1: every output is ONE product of two rounded operands, exact in fp32, added to an accumulator of +0 -- compared bit for
    bit.  Operands on bf16 ties (to even: down and up), just above and just below a tie, +-0, negative, and plain randn"""
    _lib, lib, _ = api
    e8, e20 = 2.0 ** -8, 2.0 ** -20
    special = np.array([1 + e8, 1 + 3 * e8, 1 + e8 + e20, 1 + e8 - e20, 1 + 3 * e8 + e20, 1 + 3 * e8 - e20, 0.0, -0.0, -(1 + e8), -(1 + 3 * e8),
                        (1 + e8) * 2.0 ** 40, (1 + 3 * e8) * 2.0 ** -40, 1.0, -1.5], dtype=np.float32)
    want_r = np.array([1.0, 1 + 2 ** -6, 1 + 2 ** -7, 1.0, 1 + 2 ** -6, 1 + 2 ** -7, 0.0, -0.0, -1.0, -(1 + 2 ** -6), 2.0 ** 40,
                       (1 + 2 ** -6) * 2.0 ** -40, 1.0, -1.5], dtype=np.float32)
    assert (gr.round_bf16(special).view(np.uint32) == want_r.view(np.uint32)).all()
    gen = np.random.default_rng(19)
    va = np.concatenate([special, gen.standard_normal(27, dtype=np.float32)])                  # m = 41
    vb = np.concatenate([gen.standard_normal(21, dtype=np.float32), special[::-1]])            # n = 35
    m, n = len(va), len(vb)
    spec = gr.make(m, n, 1, ta, tb, gr.natural_lda(m, 1, ta) + 3, gr.natural_ldb(n, 1, tb) + 5, n + 7, bf16=True, seed=19)
    a, b = spec.a.copy(), spec.b.copy()
    a[np.arange(m) * (1 if ta else spec.lda)] = va
    b[np.arange(n) * (spec.ldb if tb else 1)] = vb
    spec.a, spec.b = a, b
    want = np.float32(0.0) + gr.round_bf16(va)[:, None] * gr.round_bf16(vb)[None, :]
    assert (want.astype(np.float64) == gr.round_bf16(va).astype(np.float64)[:, None] * gr.round_bf16(vb)[None, :]).all(), "exact in fp32"
    assert (want.astype(np.float64) == gr.reference(spec)[0]).all()
    ag, bg, c = _ro(a), _ro(b), _out(spec.c0)
    _gemm(_lib, spec, ag, bg, None, c)
    got = _after(spec, c, {"a": ag, "b": bg}, f"rounding ta{ta} tb{tb}", lambda c2: _gemm(_lib, spec, ag, bg, None, c2))
    bad = np.argwhere(got[0].view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} products differ, first a = {va[bad[0][0]]!r} b = {vb[bad[0][1]]!r}: {got[0][tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


# ================================================================================================ (7) row sums
@pytest.mark.parametrize("batch", gr.ROWSUM_BATCH)
def test_rowsum_batched(api, batch):
    _lib, lib, _ = api
    for rows in gr.ROWSUM_ROWS:
        for cols in gr.ROWSUM_COLS:
            a, out0 = gr.rowsum_inputs(batch, rows, cols)
            ag = _ro(a)
            for acc in (0, 1):
                what = f"rowsum {batch}x{rows}x{cols} acc{acc}"
                outs = []
                for _ in range(2):
                    out = _out(out0 if acc else gr.pattern(rows))
                    _lib.call("ptmi_rowsum_batched", _p(ag), _p(out), batch, rows, cols, acc, _stream())
                    torch.cuda.synchronize()
                    out.assert_guards_intact(what)
                    assert out.unwritten() == 0, what
                    outs.append(out)
                ag.assert_unchanged(f"{what}: a")
                assert torch.equal(outs[0].raw, outs[1].raw), f"{what}: a second launch gives other bits"
                got = outs[0].payload.cpu().numpy()
                assert np.isfinite(got).all(), what
                ratio, frac = gr.rowsum_check(got, a, out0, acc, MARGINS.get(what, gr.MARGIN), what)
                cases, r, f = STATS.get("(7) rowsum_batched", (0, 0.0, 0.0))
                STATS["(7) rowsum_batched"] = (cases + 1, max(r, ratio if batch * cols >= 8 else 0.0), max(f, frac))


# ================================================================================================ (8) bf16-storage GEMM
def _pack(api, src, rows, k, ld, k_major, what):
    """ptmi_p8m_pack of a guarded source into a guarded operand of exactly ptmi_p8m_elems elements"""
    _lib, lib, _ = api
    ko = -(-k // 8)
    assert lib.ptmi_p8m_elems(rows, k) == ko * rows * 8
    dst = Guarded((ko, rows, 8), torch.bfloat16, GUARD, GUARD, DEV)
    _lib.call("ptmi_p8m_pack", _p(src), _p(dst), rows, k, ld, int(k_major), _stream())
    torch.cuda.synchronize()
    dst.assert_guards_intact(f"{what}: packed operand")
    assert dst.unwritten() == 0, what
    src.assert_unchanged(f"{what}: source")
    return dst


def _packed_operands(api, spec):
    """both operands of a (0, 1)-layout bf16 spec, packed from their k-major sources (ld = k + 3, NaN padding) and checked exactly;
    -> (A packed, B packed), snapshots taken"""
    A, B = gr.operands(spec, np.float32)                                       # bf16-rounded already
    out = []
    for name, flat, rows, logical in (("A", spec.a, spec.m, A[0]), ("B", spec.b, spec.n, B[0].T)):
        ld = spec.k + 3
        dst = _pack(api, _ro(flat), rows, spec.k, ld, True, f"{spec.name}: pack {name} k-major")
        back = dst.payload.cpu().float().permute(1, 0, 2).reshape(rows, -1).numpy()
        assert (back[:, : spec.k].view(np.uint32) == np.ascontiguousarray(logical).view(np.uint32)).all(), f"{name}: bf16 rounding of the payload"
        assert (back[:, spec.k:].view(np.uint32) == 0).all(), f"{name}: zero octets beyond K"
        # the other source orientation: src[k * ld + row], ld = rows + 3
        t = gr.pattern(spec.k * (rows + 3))
        t.reshape(spec.k, rows + 3)[:, :rows] = flat.reshape(rows, ld)[:, : spec.k].T
        dst2 = _pack(api, _ro(t), rows, spec.k, rows + 3, False, f"{spec.name}: pack {name} row-major")
        assert torch.equal(dst.raw, dst2.raw), f"{name}: the two source orientations give the same operand"
        out.append(dst.snapshot())
    return out


@pytest.mark.parametrize("shape", gr.P8_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_p8_pack_and_gemm_nt(api, shape):
    _lib, lib, _ = api
    cases = gr.p8_cases(shape)
    assert len(cases) == 4 and cases[0].ldc == cases[0].n + 5
    m, n, k = shape
    nws = lib.ptmi_p8_gemm_nt_ws_floats(m, n, k)
    assert (nws > 0) == (shape == (70, 40, 1030)) and nws in (0, 2 * m * n), "S = 2 at k = 1030"
    ap, bp = _packed_operands(api, cases[0])
    for spec in cases:
        bias = _ro(spec.bias)
        wss = []

        def launch(c):
            wss.append(_ws(nws))
            _lib.call("ptmi_p8_gemm_nt", _p(ap), _p(bp), _p(c), _p(bias), _p(wss[-1]), m, n, k, spec.ldc, spec.relu, _stream())
        c = _out(spec.c0)
        launch(c)
        got = _after(spec, c, {"a": ap, "b": bp, "bias": bias}, f"p8_gemm_nt {spec.name}", launch)
        for w in wss:
            if w is not None:
                w.assert_guards_intact(f"{spec.name}: workspace")
        ratio, frac = gr.check(got, spec, MARGINS.get(spec.name, gr.MARGIN))
        _record("(8) p8_gemm_nt", spec, ratio, frac)


@pytest.mark.parametrize("km,kn,k,ldc", gr.P8_TOUT)
def test_p8_gemm_nt_transposed_store(api, km, kn, k, ldc):
    """flag bit 1: C[n][m] with row pitch ldc >= m.  ldc % 4 == 0 and m % 4 == 0: 16-byte stores throughout; otherwise the scalar path,
    for every row group (ldc % 4 != 0) or for the ragged last one (m % 4 != 0)"""
    _lib, lib, _ = api
    spec = gr.p8_tout_case(km, kn, k, ldc)
    assert (spec.m, spec.n, spec.ldc) == (kn, km, ldc) and spec.padding == kn * (ldc - km)
    bp, ap = _packed_operands(api, spec)                                       # the spec's A is the kernel's b

    def launch(c):
        _lib.call("ptmi_p8_gemm_nt", _p(ap), _p(bp), _p(c), None, None, km, kn, k, ldc, 2, _stream())
    c = _out(spec.c0)
    launch(c)
    got = _after(spec, c, {"a": ap, "b": bp}, f"p8_gemm_nt transposed store {km}x{kn}x{k} ldc {ldc}", launch)
    ratio, frac = gr.check(got, spec, MARGINS.get(spec.name, gr.MARGIN))
    _record("(8) p8_gemm_nt transposed store", spec, ratio, frac)


# ================================================================================================ (9) refusals
def test_refusals_launch_nothing(api):
    """argument checks of gemm_impl and ptmi_p8_gemm_nt that return before the first launch: PtmiError with its message, the output
    bit-unchanged.  Tiny stand-in buffers: nothing is read"""
    _lib, lib, _ = api
    a, b, bias = (_ro(np.ones(64, dtype=np.float32)) for _ in range(3))
    pk = Guarded((1, 8, 8), torch.bfloat16, GUARD, GUARD, DEV).snapshot()
    c = Guarded((64,), torch.float32, GUARD, GUARD, DEV).snapshot()

    def gemm(fn, m, n, k, lda, ldb, ldc, bias_mode, bias_buf):
        _lib.call(fn, _p(a), _p(b), _p(c), _p(bias_buf), m, n, k, lda, ldb, ldc, 0, 0, bias_mode, 0, 0, 1, 0, 0, 0, None, 0, _stream())

    for fn in ("ptmi_gemm_f32", "ptmi_gemm_bf16"):
        with pytest.raises(_lib.PtmiError, match="bad args"):
            gemm(fn, 4, 4, 0, 4, 4, 4, 0, None)
        for mode in (1, 2):
            with pytest.raises(_lib.PtmiError, match="bias missing"):
                gemm(fn, 4, 4, 4, 4, 4, 4, mode, None)
        for lds in ((1 << 22, 4, 4), (4, 1 << 22, 4), (4, 4, 1 << 22)):
            assert 128 * max(lds) * 4 >= 2 ** 31
            with pytest.raises(_lib.PtmiError, match="leading dimension too large"):
                gemm(fn, 4, 4, 4, *lds, 0, None)
    with pytest.raises(_lib.PtmiError, match="transposed-store form takes no bias"):
        _lib.call("ptmi_p8_gemm_nt", _p(pk), _p(pk), _p(c), _p(bias), None, 8, 8, 8, 8, 2, _stream())
    with pytest.raises(_lib.PtmiError, match="needs ldc >= m"):
        _lib.call("ptmi_p8_gemm_nt", _p(pk), _p(pk), _p(c), None, None, 8, 4, 8, 7, 2, _stream())
    with pytest.raises(_lib.PtmiError, match="transposed-store form"):
        _lib.call("ptmi_p8_gemm_nt", _p(pk), _p(pk), _p(c), None, None, 8, 8, 8, 8, 3, _stream())      # with ReLU
    with pytest.raises(_lib.PtmiError, match="bad args"):
        _lib.call("ptmi_p8_gemm_nt", _p(pk), _p(pk), _p(c), None, None, 8, 8, 8, 7, 0, _stream())      # plain form, ldc < n
    torch.cuda.synchronize()
    for name, buf in (("c", c), ("a", a), ("b", b), ("bias", bias), ("packed", pk)):
        buf.assert_unchanged(f"refusals: {name}")
