"""The guard-band arena helper (tests/_guard.py) on CPU tensors: its geometry, and its teeth - one changed element anywhere outside the
view is found and reported at the right offset, for every dtype, with and without an element offset, natural and padded rows."""
import pytest
import torch

from _guard import SENTINEL, Arena

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.uint8]
ROWS, COLS, GUARD = 5, 24, 3


def _written(dtype, shape):
    """Values of the kind the tests write through a view: finite numbers (and zeros) - never the sentinel's bits."""
    g = torch.Generator().manual_seed(1)
    if dtype in (torch.int32, torch.uint8):
        return torch.randint(0, 100, shape, generator=g).to(dtype)
    return torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("elem_offset", [0, 4])
@pytest.mark.parametrize("pad", [0, 8])
def test_geometry_and_a_clean_write(dtype, elem_offset, pad):
    ld = COLS + pad
    a = Arena(ROWS, COLS, dtype, "cpu", ld=ld if pad else None, guard_rows=GUARD, elem_offset=elem_offset)
    isz = a.view.element_size()
    assert tuple(a.view.shape) == (ROWS, COLS) and a.view.stride() == (ld, 1) and a.view.dtype == dtype
    assert (a.view.data_ptr() - elem_offset * isz) % 16 == 0
    assert a.n == (GUARD + ROWS + GUARD) * ld + 16 // isz + elem_offset
    assert a.origin >= GUARD * ld and a.n - (a.origin + ROWS * ld) >= GUARD * ld          # whole guard rows on both sides
    if dtype.is_floating_point:
        assert bool(torch.isnan(a.raw).all()), "the float sentinels are NaNs: a value computed from a gap is poisoned"
    a.assert_untouched("fresh arena")
    vals = _written(dtype, (ROWS, COLS))
    a.view.copy_(vals)
    a.assert_untouched("after a write through the view")
    assert torch.equal(a.view, vals)
    assert not bool((a.view.contiguous().view(a.bits.dtype) == SENTINEL[dtype]).any()), "a written value equals the sentinel"
    assert int((a.bits != SENTINEL[dtype]).sum()) <= ROWS * COLS


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("elem_offset", [0, 4])
@pytest.mark.parametrize("pad,where", [(pad, where) for pad in (0, 8) for where in ("gap", "row_after", "row_before", "arena_end", "arena_start")
                                       if pad or where != "gap"])        # the natural layout has no gap columns
def test_one_planted_element_is_found(dtype, elem_offset, pad, where):
    ld = COLS + pad
    a = Arena(ROWS, COLS, dtype, "cpu", ld=ld if pad else None, guard_rows=GUARD, elem_offset=elem_offset)
    a.view.copy_(_written(dtype, (ROWS, COLS)))
    if where == "gap":
        row, col = ROWS - 1, COLS                       # right behind the last valid column of the last row
    elif where == "row_after":
        row, col = ROWS, 0
    elif where == "row_before":
        row, col = -1, ld - 1                           # the element in front of view[0, 0]
    elif where == "arena_end":
        rel = a.n - 1 - a.origin
        row, col = rel // ld, rel % ld
    else:
        rel = -a.origin
        row, col = rel // ld, rel % ld                  # floor division: negative rows count back from the view
    idx = a.origin + row * ld + col
    assert 0 <= idx < a.n
    one = torch.ones((), dtype=dtype)
    a.raw[idx] = one
    count, first = a.violations()
    assert (count, first) == (1, [(row, col)])
    with pytest.raises(AssertionError, match=r"1 element\(s\) outside .*\[\(%d, %d\)\]" % (row, col)):
        a.assert_untouched("planted")
    a.bits[idx] = SENTINEL[dtype]
    a.assert_untouched("restored")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_a_nan_for_a_nan_is_still_a_change(dtype):
    """A float comparison would call the arena untouched (NaN != NaN both before and after, or `equal_nan`); the integer one
    sees another payload, and sees a canonical NaN - what a kernel computing on poisoned data would store."""
    a = Arena(ROWS, COLS, dtype, "cpu", ld=COLS + 8, guard_rows=GUARD)
    a.raw[a.origin + COLS] = float("nan")                          # canonical quiet NaN in the first gap column of row 0
    assert a.bits[a.origin + COLS] != SENTINEL[dtype]
    assert a.violations() == (1, [(0, COLS)])
    a.bits[a.origin + COLS] = SENTINEL[dtype]
    a.bits[a.origin - 1] = SENTINEL[dtype] ^ 1                     # same class of NaN, payload off by one bit
    assert bool(torch.isnan(a.raw[a.origin - 1]))
    assert a.violations() == (1, [(-1, COLS + 7)])


def test_flat_arena():
    a = Arena.flat((2, 3, 4, 8), torch.float32, "cpu", guard_elems=40)
    assert tuple(a.view.shape) == (2, 3, 4, 8) and a.view.is_contiguous() and a.view.data_ptr() % 16 == 0
    a.view.zero_()
    a.assert_untouched("flat")
    a.raw[a.origin + 2 * 3 * 4 * 8] = 0.0                           # first element behind
    assert a.violations() == (1, [(24, 0)])
    a.bits[a.origin + 192] = SENTINEL[torch.float32]
    a.raw[a.origin - 1] = 0.0
    a.raw[0] = 0.0
    count, first = a.violations()
    assert count == 2 and first[1] == (-1, 7) and first[0] == ((-a.origin) // 8, (-a.origin) % 8)


def test_of_copies_and_keeps_the_gaps_poisoned():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    a = Arena.of(t, ld=8, guard_rows=2)
    assert torch.equal(a.view, t) and a.view.stride() == (8, 1)
    whole = torch.as_strided(a.raw, (3, 8), (8, 1), a.origin)
    assert bool(torch.isnan(whole[:, 4:]).all()) and bool(torch.isnan(whole.sum(1)).all())
    a.assert_untouched("input arena")
