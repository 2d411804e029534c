"""Self-test of tests/guarded.py on CPU tensors: the evidence that the guard-band helper CAN fail -- every kind of stray write the
GPU bounds tests rely on it to see is planted here by hand and must be reported, with the right count, distances and value."""
import re

import pytest
import torch

from tests.guarded import ALIGN, PATTERN, Guarded, conv_guard


def _flat(g):
    """the whole allocation as elements of the payload dtype (front guard | payload | back guard)"""
    return g.raw.view(g.dtype)


def _fail(fn, *a):
    with pytest.raises(AssertionError) as e:
        fn(*a)
    return str(e.value)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32, torch.uint8, torch.int64, torch.float64])
def test_fresh_buffer_is_aligned_patterned_and_clean(dtype):
    g = Guarded((3, 5, 7), dtype, front=10, back=3)
    assert g.payload.shape == (3, 5, 7) and g.payload.dtype == dtype and g.payload.is_contiguous()
    assert g.payload.data_ptr() % ALIGN == 0
    assert g.front >= 10 and g.back >= 3
    words = g.raw.view(torch.int32)
    assert bool((words == PATTERN - (1 << 32)).all()), "every byte comes from the one 32-bit pattern"
    g.assert_guards_intact("fresh")
    assert g.unwritten() == 105
    g.snapshot().assert_unchanged("fresh")


def test_pattern_is_a_negative_quiet_nan_with_a_payload():
    v = torch.tensor([PATTERN - (1 << 32)], dtype=torch.int32).view(torch.float32)
    assert bool(torch.isnan(v).all())
    assert PATTERN >> 31 == 1 and (PATTERN >> 22) & 1 == 1 and PATTERN & 0x3FFFFF != 0
    assert PATTERN != torch.tensor([float("nan")]).view(torch.int32).item() & 0xFFFFFFFF


def test_writes_to_the_payload_alone_pass():
    g = Guarded((4, 6), torch.float32, front=64, back=64)
    g.payload.copy_(torch.randn(4, 6))
    g.assert_guards_intact("payload only")
    assert g.unwritten() == 0


@pytest.mark.parametrize("where,dist", [("just before", -1), ("just after", +1), ("far front", None), ("far back", None)])
def test_one_stray_element_is_reported_with_its_distance(where, dist):
    g = Guarded((2, 50), torch.float32, front=300, back=300)
    flat, f0 = _flat(g), g.front
    if dist is None:
        dist = -g.front if where == "far front" else g.back
    idx = f0 + dist if dist < 0 else f0 + g.numel + dist - 1
    assert idx in (0, f0 - 1, f0 + g.numel, flat.numel() - 1)
    flat[idx] = 1.5
    msg = _fail(g.assert_guards_intact, where)
    assert msg.startswith(where) and "1 guard element(s) overwritten" in msg
    assert f"nearest at {dist:+d}, farthest at {dist:+d}" in msg and "1.5" in msg


def test_nearest_and_farthest_of_several_strays():
    g = Guarded((7,), torch.float32, front=1000, back=1000)
    flat, f0 = _flat(g), g.front
    flat[f0 - 5] = 2.0                    # -5
    flat[f0 - 900] = 3.0                  # -900
    flat[f0 + 7 + 2] = 4.0                # +3
    msg = _fail(g.assert_guards_intact, "y")
    assert "3 guard element(s) overwritten (2 before, 1 after" in msg
    assert "nearest at +3, farthest at -900" in msg and "4.0" in msg


@pytest.mark.parametrize("value", [0.0, float("nan"), float("-inf"), -0.0])
def test_a_stray_zero_or_ordinary_nan_is_a_write(value):
    """float `==` would call a NaN-for-NaN overwrite 'untouched' and could not tell -0.0 from 0.0; the bit patterns differ"""
    g = Guarded((3, 3), torch.float32, front=16, back=16)
    _flat(g)[g.front + 9] = value
    msg = _fail(g.assert_guards_intact, "y")
    assert "nearest at +1" in msg and re.search(r"0x[0-9a-f]{8}", msg)
    h = Guarded((3, 3), torch.float32, front=16, back=16)
    h.payload.fill_(value)
    assert h.unwritten() == 0, "an ordinary NaN / zero in the payload counts as written"


def test_a_single_stray_byte_in_a_two_byte_type_is_seen():
    g = Guarded((5, 8), torch.bfloat16, front=128, back=128)
    g.raw[g.front * 2 - 3] ^= 0x01        # low byte of the element two before the payload
    msg = _fail(g.assert_guards_intact, "p8")
    assert "1 guard element(s) overwritten" in msg and "nearest at -2, farthest at -2" in msg


def test_unwritten_counts_the_payload_elements_left_alone():
    g = Guarded((4, 5), torch.float32, front=8, back=8)
    g.payload.zero_()
    assert g.unwritten() == 0
    g.payload.view(torch.int32)[2, 3] = PATTERN - (1 << 32)
    assert g.unwritten() == 1
    p = Guarded((6, 8), torch.bfloat16, front=8, back=8)
    p.payload[:5].zero_()
    assert p.unwritten() == 8


def test_a_modified_read_only_operand_is_reported():
    x = Guarded.of(torch.arange(24, dtype=torch.float32).view(2, 3, 4), front=32, back=32)
    x.snapshot()
    x.assert_unchanged("x")
    x.payload[1, 0, 2] = -7.0                                  # payload index 14, was 14.0
    msg = _fail(x.assert_unchanged, "x")
    assert "1 element(s) changed (1 in the payload" in msg and "first at payload index 14" in msg and "14.0 -> -7.0" in msg
    x.snapshot()                                               # documented re-arming: a new snapshot accepts the new state
    x.assert_unchanged("x")
    _flat(x)[x.front - 1] = 0.0                                # a write into a read-only operand's guard
    msg = _fail(x.assert_unchanged, "x")
    assert "0 in the payload" in msg and "1 in its guards" in msg and "first at payload index -1" in msg
    m = Guarded.of(torch.tensor([1, 0, 1], dtype=torch.uint8), front=4, back=4).snapshot()
    m.payload[1] = 1
    assert "first at payload index 1" in _fail(m.assert_unchanged, "mask")


def test_same_value_rewrite_of_a_read_only_operand_passes():
    x = Guarded.of(torch.ones(8), front=8, back=8).snapshot()
    x.payload.fill_(1.0)
    x.assert_unchanged("x")


def test_conv_guard_is_a_full_channel_tile_of_planes():
    assert conv_guard(1) == 4096 and conv_guard(11 * 17) == 128 * 187 and conv_guard(32) == 4096 and conv_guard(33) == 4224
