"""Guard-band arenas for the kernel tests: an operand or an output placed in the middle of a larger allocation that is filled
with a sentinel bit pattern, so that a store outside the logical output - past the last row, past the last valid column of a padded
row, in front of the first row - changes a sentinel and fails an assertion instead of landing in the allocator's slack or in a
neighbouring tensor.  Used for INPUTS the sentinel (a NaN in the float types) poisons every result computed from a gap or guard
element, so a read outside the logical operand shows up in the value comparison.

    a = Arena(rows, cols, dtype, device, ld=cols + 8)        # .view: (rows, cols), strides (ld, 1), 16-byte aligned
    kernel(..., out=a.view)
    a.assert_untouched("C")

Arena.flat(shape, ...) is the form for contiguous N-D buffers (attention operands, states, statistics): guards in front and behind.
Padded64 is the fp64 form (the sentinel is a value of the caller's choice: NaN around an input, a marker around an output)."""
import numpy as np
import torch

SENTINEL = {torch.bfloat16: 0x7FA5, torch.float16: 0x7EA5, torch.float32: 0x7FA5A5A5, torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8}
ALIGN = 16                      # bytes: the alignment every kernel entry point may assume of an operand
GUARD_ROWS = 256                # one edge of the largest tile (the 256x256 GEMM tile, the 256-row query block)
FLAT_GUARD = 256 * 256          # elements in front of and behind a flat arena
PAD = 1024                      # doubles in front of and behind a padded fp64 buffer


class Arena:
    def __init__(self, rows, cols, dtype, device, ld=None, guard_rows=GUARD_ROWS, elem_offset=0, _guard_elems=None, _shape=None):
        ld = cols if ld is None else ld
        assert rows >= 1 and cols >= 1 and ld >= cols and elem_offset >= 0 and dtype in SENTINEL
        self.rows, self.cols, self.ld, self.dtype, self.elem_offset = rows, cols, ld, dtype, elem_offset
        isz = torch.empty((), dtype=dtype).element_size()
        guard = guard_rows * ld if _guard_elems is None else _guard_elems
        slack = ALIGN // isz + elem_offset
        self.n = 2 * guard + rows * ld + slack
        self.bits = torch.full((self.n,), SENTINEL[dtype], dtype=_BITS[dtype], device=device)
        self.raw = self.bits.view(dtype)
        # first element at or behind the front guard whose address is 16-byte aligned, then `elem_offset` elements on
        addr = self.bits.data_ptr() + guard * isz
        self.origin = guard + (-addr % ALIGN) // isz + elem_offset
        assert (-addr % ALIGN) % isz == 0 and self.origin + rows * ld + guard <= self.n
        self.view = torch.as_strided(self.raw, (rows, cols), (ld, 1), self.origin)
        assert (self.view.data_ptr() - elem_offset * isz) % ALIGN == 0
        if _shape is not None:
            self.view = self.view.view(_shape)

    @classmethod
    def flat(cls, shape, dtype, device, guard_elems=FLAT_GUARD, elem_offset=0):
        """A contiguous tensor of `shape` with `guard_elems` sentinels in front and behind; offsets are reported as (row, col) of
        the tensor flattened to (-1, shape[-1])."""
        shape = tuple(int(s) for s in shape)
        last = shape[-1]
        numel = 1
        for s in shape:
            numel *= s
        return cls(numel // last, last, dtype, device, ld=last, elem_offset=elem_offset, _guard_elems=guard_elems, _shape=shape)

    @classmethod
    def of(cls, t, ld=None, elem_offset=0, guard_rows=GUARD_ROWS):
        """An arena holding a copy of the 2-D tensor `t` (an input operand: gaps and guards stay poisoned)."""
        a = cls(t.shape[0], t.shape[1], t.dtype, t.device, ld=ld, guard_rows=guard_rows, elem_offset=elem_offset)
        a.view.copy_(t)
        return a

    @classmethod
    def flat_of(cls, t, guard_elems=FLAT_GUARD):
        a = cls.flat(t.shape, t.dtype, t.device, guard_elems=guard_elems)
        a.view.copy_(t)
        return a

    def _outside(self):
        """bool (n,): True on every element that is not part of .view."""
        m = torch.ones((self.n,), dtype=torch.bool, device=self.bits.device)
        torch.as_strided(m, (self.rows, self.cols), (self.ld, 1), self.origin).fill_(False)
        return m

    def violations(self):
        """(count, [(row, col), ...] of the first few) of the elements outside .view that no longer hold the sentinel.  Integer
        comparison: NaN != NaN cannot hide a change, and a changed NaN payload counts.  Offsets are relative to the view: row -1 is
        the last guard row in front, row `rows` the first one behind, col >= cols the gap of a padded row."""
        bad = (self.bits != SENTINEL[self.dtype]) & self._outside()
        count = int(bad.sum())
        if count == 0:
            return 0, []
        rel = bad.nonzero().flatten()[:8].cpu() - self.origin
        row = torch.div(rel, self.ld, rounding_mode="floor")
        col = rel - row * self.ld
        return count, list(zip(row.tolist(), col.tolist()))

    def assert_untouched(self, what):
        count, first = self.violations()
        assert count == 0, (f"{what}: {count} element(s) outside the ({self.rows}, {self.cols}) view (ld {self.ld}) were written; "
                            f"first (row, col) offsets relative to the view: {first}")


class Padded64:
    """A contiguous fp64 tensor of `shape` with PAD doubles of `fill` on each side."""

    def __init__(self, shape, dev, fill, data=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=torch.float64, device=dev)
        self.view = self.buf[PAD:PAD + n].view(shape)
        if data is not None:
            self.view.copy_(data)
        self.before = self.buf.clone()
        self.n = n

    def assert_untouched(self, what, written=False):
        now, was = self.buf.view(torch.int64), self.before.view(torch.int64)
        assert torch.equal(now[:PAD], was[:PAD]) and torch.equal(now[PAD + self.n:], was[PAD + self.n:]), f"{what}: a guard changed"
        if not written:
            assert torch.equal(now, was), f"{what}: an input changed"
