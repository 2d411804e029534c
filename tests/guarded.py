"""Guard-band buffers for the out-of-bounds-write tests (tests/test_conv_bounds_gpu.py, tests/test_workspace_bounds_gpu.py;
self-test: tests/test_guarded_cpu.py).

The parity tests check every element INSIDE an output.  A `Guarded` operand also shows what a launch did OUTSIDE it: the payload
sits in the middle of one flat allocation whose every byte, payload included, is filled from one fixed 32-bit pattern --
0xFFC5A5A5, as fp32 a negative quiet NaN with a payload, which no kernel here produces -- and every comparison is made on bit
patterns (uint8 / int32 views), never with float `==`: a stray 0.0, -inf or ordinary NaN counts as a write.

    g = Guarded((n, cout, h, w), torch.float32, front=conv_guard(h * w), back=conv_guard(h * w), device=DEV)
    _lib.call(..., ops._ptr(g.payload), ...)
    g.assert_guards_intact("y")          # nothing before / after the payload was written
    assert g.unwritten() == 0            # every payload element was written

    x = Guarded.of(x_cpu, device=DEV); x.snapshot(); ...launch...; x.assert_unchanged("x")     # read-only operands

Reach: a stray write is seen only if it lands inside this allocation, i.e. at most `front` elements before or `back` elements
after the payload (conv outputs: one full 128-channel tile of planes on each side, `conv_guard`).  A write beyond that goes to
someone else's memory and is out of these tests' sight.  A stray write of the pattern's own bytes is invisible too.
"""
import math

import torch

PATTERN = 0xFFC5A5A5                       # fp32: sign 1, exponent 0xFF, quiet bit, payload 0x45A5A5
_PATTERN_I32 = PATTERN - (1 << 32)
ALIGN = 256                                # bytes: payload.data_ptr() % ALIGN == 0


def conv_guard(out_plane):
    """guard elements on each side of a convolution output whose channel planes hold `out_plane` elements"""
    return max(4096, 128 * int(out_plane))


def _round_up(v, m):
    return -(-v // m) * m


class Guarded:
    def __init__(self, shape, dtype=torch.float32, front=4096, back=4096, device="cpu"):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.shape, self.dtype, self.item = shape, dtype, torch.empty(0, dtype=dtype).element_size()
        self.numel = math.prod(shape)
        self._fb = _round_up(int(front) * self.item, ALIGN)                      # front guard, bytes
        self._pb = self.numel * self.item                                       # payload, bytes
        total = _round_up(self._fb + self._pb + _round_up(int(back) * self.item, ALIGN), ALIGN)
        self._bb = total - self._fb - self._pb                                  # back guard, bytes (takes the payload's ragged tail)
        store = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
        skip = -store.data_ptr() % ALIGN
        assert skip % 4 == 0
        self.raw = store[skip: skip + total]                                    # uint8 view of the whole allocation
        self.raw.view(torch.int32).fill_(_PATTERN_I32)
        self._pristine = self.raw.clone()
        self.front, self.back = self._fb // self.item, self._bb // self.item    # guard elements actually watched
        self.payload = self.raw[self._fb: self._fb + self._pb].view(dtype).view(shape)
        assert self.payload.data_ptr() % ALIGN == 0 and self.payload.is_contiguous()
        self._snap = None

    @classmethod
    def of(cls, t, front=4096, back=4096, device=None):
        """a guarded copy of tensor `t`"""
        g = cls(t.shape, t.dtype, front, back, t.device if device is None else device)
        g.payload.copy_(t)
        return g

    # ------------------------------------------------------------------ helpers on bytes
    def _element(self, byte0):
        """(value, hex of the bytes) of the payload-dtype element that starts at byte `byte0` of the allocation"""
        b = self.raw[byte0: byte0 + self.item].cpu().contiguous()
        hexs = "0x" + "".join(f"{int(v):02x}" for v in reversed(b.tolist()))
        return (b.view(self.dtype)[0].item() if b.numel() == self.item else None), hexs

    def _strays(self, lo, hi, origin, sign):
        """element distances (from `origin`, counted in direction `sign`) of the modified elements within bytes [lo, hi)"""
        bad = (self.raw[lo:hi] != self._pristine[lo:hi]).nonzero().flatten()
        if bad.numel() == 0:
            return bad
        if sign < 0:                                           # front guard: element k before the payload = distance -k
            return -torch.unique((origin - 1 - (bad + lo)) // self.item + 1)
        return torch.unique((bad + lo - origin) // self.item + 1)

    # ------------------------------------------------------------------ the checks
    def assert_guards_intact(self, what=""):
        end = self._fb + self._pb
        d = torch.cat([self._strays(0, self._fb, self._fb, -1), self._strays(end, end + self._bb, end, +1)]).cpu()
        if d.numel() == 0:
            return
        near = int(d[d.abs().argmin()])
        far = int(d[d.abs().argmax()])
        byte0 = self._fb + near * self.item if near < 0 else end + (near - 1) * self.item
        val, hexs = self._element(byte0)
        raise AssertionError(
            f"{what}: {d.numel()} guard element(s) overwritten ({int((d < 0).sum())} before, {int((d > 0).sum())} after the payload of "
            f"{self.numel} x {self.dtype}); nearest at {near:+d}, farthest at {far:+d} elements from the payload "
            f"(-1 = the element just before it, +1 = just after it; guards watch -{self.front} .. +{self.back}); "
            f"value found at {near:+d}: {val!r} ({hexs}, fill {PATTERN:#010x})")

    def unwritten(self):
        """number of payload elements that still hold the fill pattern"""
        lo, hi = self._fb, self._fb + self._pb
        same = (self.raw[lo:hi] == self._pristine[lo:hi]).view(self.numel, self.item).all(dim=1)
        return int(same.sum())

    def snapshot(self):
        """remember the whole allocation (payload and guards) as a read-only operand's state before a launch"""
        self._snap = self.raw.clone()
        return self

    def assert_unchanged(self, what=""):
        """the whole allocation is bit-identical to the last snapshot()"""
        assert self._snap is not None, "assert_unchanged without snapshot()"
        bad = (self.raw != self._snap).nonzero().flatten()
        if bad.numel() == 0:
            return
        el = torch.unique(torch.div(bad - self._fb, self.item, rounding_mode="floor")).cpu()
        first = int(el[0])
        val, hexs = self._element(self._fb + first * self.item)
        was = self._snap[self._fb + first * self.item: self._fb + (first + 1) * self.item].cpu().contiguous().view(self.dtype)[0].item()
        inside = int(((el >= 0) & (el < self.numel)).sum())
        raise AssertionError(
            f"{what}: read-only operand modified: {el.numel()} element(s) changed ({inside} in the payload of {self.numel} x {self.dtype}, "
            f"{el.numel() - inside} in its guards); first at payload index {first} (last at {int(el[-1])}): {was!r} -> {val!r} ({hexs})")
