"""CPU: tests/gemm_ref.py states the GEMM ABI correctly, its yardstick conditions hold for every case tests/test_gemm_family_gpu.py
launches, and `check` catches a planted defect of each kind the kernels could have."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as gr
from tests.guarded import PATTERN


def _materialise(spec):
    """A (batch, m, k), B (batch, k, n), C0 (batch, m, n) as float64 torch tensors, gathered element by element with plain index
    arithmetic (not with gemm_ref's strided views)"""
    z, i, j, kk = (torch.arange(v) for v in (spec.batch, spec.m, spec.n, spec.k))
    ia = z[:, None, None] * spec.stride_a + (kk[None, None, :] * spec.lda + i[None, :, None] if spec.ta else
                                             i[None, :, None] * spec.lda + kk[None, None, :])
    ib = z[:, None, None] * spec.stride_b + (j[None, None, :] * spec.ldb + kk[None, :, None] if spec.tb else
                                             kk[None, :, None] * spec.ldb + j[None, None, :])
    ic = z[:, None, None] * spec.stride_c + i[None, :, None] * spec.ldc + j[None, None, :]
    a, b, c0 = (torch.from_numpy(np.array(v)) for v in (spec.a, spec.b, spec.c0))
    return a[ia].double(), b[ib].double(), c0[ic].double()


def _torch_reference(spec):
    A, B, C0 = _materialise(spec)
    if spec.bf16:
        A, B = A.float().to(torch.bfloat16).double(), B.float().to(torch.bfloat16).double()
    out = torch.bmm(A, B)
    if spec.bias_mode == 1:
        out += torch.from_numpy(spec.bias).double()[None, :, None]
    elif spec.bias_mode == 2:
        out += torch.from_numpy(spec.bias).double()[None, None, :]
    if spec.accumulate:
        out += C0
    return torch.relu(out) if spec.relu else out


def _abi_cases():
    m, n, k = 19, 13, 10
    for ta, tb in gr.LAYOUTS:
        la, lb = gr.natural_lda(m, k, ta), gr.natural_ldb(n, k, tb)
        yield from gr.epilogues(gr.make(m, n, k, ta, tb, la + 3, lb + 5, n + 7, seed=1))                  # every epilogue flag, ld above natural
        yield gr.make(m, n, k, ta, tb, seed=2, bias_mode=2, relu=1)                                       # natural
        ea, eb = (k if ta else m) * (la + 3), (n if tb else k) * (lb + 5)
        kw = dict(ta=ta, tb=tb, lda=la + 3, ldb=lb + 5, ldc=n + 7, batch=3, seed=3)
        yield gr.make(m, n, k, stride_a=0, stride_b=eb + 4, stride_c=m * (n + 7) + 6, bias_mode=1, accumulate=1, **kw)
        yield gr.make(m, n, k, stride_a=ea + 2, stride_b=0, bias_mode=2, relu=1, **kw)
        yield gr.make(m, n, k, stride_a=ea, stride_b=eb, bf16=True, accumulate=1, **kw)


def test_reference_equals_torch_bmm_in_float64():
    """every layout, lda / ldb / ldc above natural, stride 0 and strides with gaps, each epilogue flag, bf16 rounding -- and the
    padding words, all NaN, never reach the result"""
    count = 0
    for spec in _abi_cases():
        assert np.isnan(spec.c0).sum() == spec.padding + (0 if spec.accumulate else spec.batch * spec.m * spec.n)
        got, want = gr.reference(spec, np.float64), _torch_reference(spec).numpy()
        assert got.dtype == np.float64 and np.isfinite(got).all(), spec.name
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=spec.name)
        s = gr.scale(spec)
        assert (s >= np.abs(got) * (1 - 1e-12)).all() and (s > 0).all(), f"{spec.name}: s bounds |ref| from above"
        assert gr.err(got, spec) <= 1e-13
        count += 1
    assert count == 4 * 16


def test_padding_is_the_guard_pattern_and_operands_are_spread_in_scale():
    spec = gr.make(7, 5, 6, 0, 1, 9, 11, 8, batch=2, stride_a=7 * 9 + 4, stride_b=5 * 11 + 2, stride_c=7 * 8 + 3, accumulate=1, seed=4)
    for buf, real in ((spec.a, 2 * 7 * 6), (spec.b, 2 * 5 * 6), (spec.c0, 2 * 7 * 5)):
        bits = buf.view(np.uint32)
        assert int((bits == PATTERN).sum()) == buf.size - real and int(np.isnan(buf).sum()) == buf.size - real
    assert spec.padding == spec.c0.size - 70
    big = gr.make(*gr.PLAIN_SHAPE, seed=11)
    A, B = gr.operands(big, np.float64)
    rows, cols = np.abs(A[0]).max(axis=1), np.abs(B[0]).max(axis=0)
    assert rows.max() / rows.min() > 2.0 ** 15 and cols.max() / cols.min() > 2.0 ** 15


def test_round_bf16_is_nearest_even_and_equals_torch():
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20, 0.0, -0.0, -1 - 2.0 ** -8, 3.0e38],
                 dtype=np.float32)
    want = np.array([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1.0, 0.0, -0.0, -1.0, 3.0e38], dtype=np.float32)
    got = gr.round_bf16(x)
    assert (got.view(np.uint32)[:7] == want.view(np.uint32)[:7]).all()
    r = np.random.default_rng(5).standard_normal(100000).astype(np.float32) * np.exp2(np.random.default_rng(6).integers(-30, 30, 100000))
    r = r.astype(np.float32)
    assert (gr.round_bf16(r).view(np.uint32) == torch.from_numpy(r).to(torch.bfloat16).float().numpy().view(np.uint32)).all()


def test_yardstick_conditions_hold_for_every_case_the_gpu_file_launches():
    """err(seq32) > 0, err(seq32) within the hard bound, and MARGIN * err(seq32) within it too (the tight bound governs) -- conditions
    on the inputs.  Two kinds of case cannot meet them by any choice of seed, `gr.governs` names them from the inputs alone and this
    test pins them: one exact bf16 product (K = 1), where the yardstick is exact, and fp32 at K < 8, where the hard bound is the
    narrower of the two and decides."""
    seen = {"exact": 0, "hard": 0, "tight": 0}
    worst = 0.0
    for spec in gr.all_gemm_cases():
        ref64, s = gr.reference(spec, np.float64), gr.scale(spec)
        assert np.isfinite(ref64).all() and (s > 0).all(), spec.name
        e32, hard, kind = gr.scaled_err(gr.seq32(spec), ref64, s), gr.hard_bound(spec.k + 3), gr.governs(spec)
        seen[kind] += 1
        if kind == "exact":
            assert e32 == 0.0, f"{spec.name}: one bf16 x bf16 product is exact"
            continue
        assert 0 < e32 <= hard, f"{spec.name}: err(seq32) {e32 / gr.U24:.2f} x 2^-24, hard bound {hard / gr.U24:.2f}"
        if kind == "hard":
            assert spec.k < 8 and e32 <= 3.0 * gr.U24, spec.name
            continue
        gr.yardstick_conditions(e32, hard, spec.name)
        worst = max(worst, e32)
    assert seen["exact"] == 4 and seen["hard"] == 4 * 6 and seen["tight"] > 380, seen
    assert worst <= 6 * gr.U24, f"err(seq32) is a few units of 2^-24 at every K: {worst / gr.U24:.2f}"


def test_rowsum_yardstick_conditions():
    for batch in gr.ROWSUM_BATCH:
        for rows in gr.ROWSUM_ROWS:
            for cols in gr.ROWSUM_COLS:
                a, out0 = gr.rowsum_inputs(batch, rows, cols)
                for acc in (0, 1):
                    ref64, s = gr.rowsum_reference(a, out0, acc, np.float64), gr.rowsum_scale(a, out0, acc)
                    e32 = gr.scaled_err(gr.rowsum_reference(a, out0, acc, np.float32), ref64, s)
                    what = f"rowsum {batch}x{rows}x{cols} acc{acc}"
                    if batch * cols + acc == 1:
                        assert e32 == 0.0, f"{what}: a single term is copied"
                    else:
                        assert (s > 0).all()
                        hard = gr.hard_bound(batch * cols + 1)
                        assert 0 < e32 <= hard, what
                        if batch * cols >= 8:
                            gr.yardstick_conditions(e32, hard, what)
    a, out0 = gr.rowsum_inputs(3, 9, 257)
    np.testing.assert_allclose(gr.rowsum_reference(a, out0, 1, np.float64), out0.astype(np.float64) + a.astype(np.float64).sum((0, 2)),
                               rtol=1e-14)


# ------------------------------------------------------------------------------------------------ planted defects
def _fails(got, spec):
    with pytest.raises(AssertionError):
        gr.check(got, spec)


def _worst_of(spec, values):
    """index of the element where |values| / s is largest"""
    return np.unravel_index(np.argmax(np.abs(values) / gr.scale(spec)), values.shape)


def test_check_passes_the_yardstick_and_another_honest_order():
    for spec in (gr.plain_cases(0, 0)[3], gr.splitk_cases(1, 1, gr.SPLITK_SHAPES[0])[11], gr.ksweep_cases(0, 1)[25]):
        ratio, frac = gr.check(gr.seq32(spec), spec)
        assert ratio == 1.0 and frac < 0.25
        gr.check(gr.reference(spec, np.float32), spec)                          # matmul's own fp32 order
        gr.check(gr.reference(spec, np.float64).astype(np.float32), spec)       # the correctly rounded result


def test_check_catches_one_dropped_k_term():
    """in ONE element, at the plain shape and at K = 4099 (where one term is 1 / 4099 of the sum)"""
    for spec in (gr.plain_cases(0, 1)[0], gr.splitk_cases(0, 0, (9, 130, 4099))[0]):
        A, B = gr.operands(spec, np.float32)
        got = gr.seq32(spec)
        z, i, j = 0, spec.m // 2, spec.n // 3
        terms = np.abs(A[z, i].astype(np.float64) * B[z, :, j])
        kk = int(np.argsort(terms)[len(terms) // 2])                                             # a term of median size, not the largest
        got[z, i, j] -= A[z, i, kk] * B[z, kk, j]
        _fails(got, spec)


def test_check_catches_bias_taken_from_the_next_row():
    spec = next(s for s in gr.plain_cases(1, 0) if s.bias_mode == 1 and not s.relu and not s.accumulate)
    got = gr.seq32(spec) + (np.roll(spec.bias, -1) - spec.bias)[None, :, None]
    _fails(got, spec)
    # on one row only, the one where the wrong value is nearest to the right one
    i = int(np.argmin(np.abs(np.roll(spec.bias, -1) - spec.bias) / (np.abs(spec.bias) + 1e-30)))
    got = gr.seq32(spec)
    got[0, i] += np.roll(spec.bias, -1)[i] - spec.bias[i]
    _fails(got, spec)
    spec2 = next(s for s in gr.plain_cases(0, 0) if s.bias_mode == 2 and s.relu and s.accumulate)
    wrong = spec2.with_epilogue(2, 1, 1, np.roll(spec2.bias, -1))
    _fails(gr.seq32(wrong), spec2)


def test_check_catches_one_unzeroed_tail_word():
    """K % 4 == 2 with lda = K + 3: the word after a row's last element is padding (NaN) -- against a B whose rows k >= K are zero the
    product is NaN, not 0, which is how the device test sees a lost fix-up; against finite garbage on both sides it is a finite
    error of one extra term"""
    spec = gr.plain_cases(0, 1)[0]
    assert spec.k % 4 == 2 and spec.lda > spec.k and np.isnan(spec.a[spec.k])
    got = gr.seq32(spec)
    got[0, 0, :] += spec.a[spec.k] * np.float32(0.0)
    assert np.isnan(got[0, 0]).all()
    _fails(got, spec)
    A, B = gr.operands(spec, np.float32)
    # finite garbage: with natural lda the straddled word is the next row's first word, on both sides; one element, the worst
    leak = A[0, 1:, :1] * B[0, :1, 1:]
    i, j = np.unravel_index(np.argmax(np.abs(leak) / gr.scale(spec)[0, :-1, :-1]), leak.shape)
    got = gr.seq32(spec)
    got[0, i, j] += leak[i, j]
    _fails(got, spec)


def test_check_catches_relu_skipped_on_one_element():
    spec = next(s for s in gr.plain_cases(1, 1) if s.relu and s.bias_mode == 2 and not s.accumulate)
    pre = gr.seq32(spec.with_epilogue(2, 0, 0, spec.bias))
    neg = np.argwhere(pre < 0)
    assert len(neg) > 1000
    # the negative pre-activation that is smallest against its scale among those that are not rounding noise
    rel = np.where(pre < 0, -pre / gr.scale(spec), np.inf)
    rel[rel < 1e-3] = np.inf
    z, i, j = np.unravel_index(np.argmin(rel), rel.shape)
    got = gr.seq32(spec)
    assert got[z, i, j] == 0
    got[z, i, j] = pre[z, i, j]
    _fails(got, spec)


def test_check_catches_nan_inf_and_a_written_zero_scale_element():
    spec = gr.plain_cases(0, 0)[0]
    for bad in (np.nan, np.inf):
        got = gr.seq32(spec)
        got[0, 3, 4] = bad
        _fails(got, spec)
    ref64 = np.zeros((1, 2, 2))
    assert gr.scaled_err(np.array([[[0.0, 0.0], [0.0, 1e-30]]]), ref64, np.zeros((1, 2, 2))) == np.inf
    assert gr.scaled_err(ref64, ref64, np.zeros((1, 2, 2))) == 0.0
