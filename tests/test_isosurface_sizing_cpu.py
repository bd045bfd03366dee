"""The sizing step both extraction methods share (actionmesh_amd/isosurface.py `_sized`: the two prefix sums, the one read of their
totals, the limit, the empty result, the exclusive offsets), without a device: the shipped Python on CPU tensors with the numpy
restatements in place of the kernels.

The figures are the contract's.  One cell whose corner 000 alone is inside: marching tetrahedra cuts the seven edges from that corner
(three axes, three face diagonals, the body diagonal) and every one of the six Kuhn tetrahedra, which all start there, gives one
triangle; dual marching cubes gives the cell one patch - one vertex - and no quad, a quad needing four cells around an edge.
"""
import numpy as np
import pytest
import torch

import _dualcubes_ref as D
import _isosurface_ref as R
from actionmesh_amd import isosurface as ISO

BACKENDS = dict(backend=R.NumpyBackend(), dual_backend=D.NumpyBackend())
ONE_CELL = np.full((2, 2, 2), -1.0, np.float32)
ONE_CELL[0, 0, 0] = 1.0


def extract(values, method):
    v, f = ISO.extract_isosurface(torch.from_numpy(values), method=method, **BACKENDS)
    assert v.dtype == torch.float32 and f.dtype == torch.int64
    return tuple(v.shape), tuple(f.shape)


@pytest.mark.parametrize("method", ISO.METHODS)
def test_an_empty_field_is_the_empty_result(method):
    assert extract(np.full((3, 2, 4), -1.0, np.float32), method) == ((0, 3), (0, 3))


def test_one_crossing_cell():
    assert extract(ONE_CELL, "tetrahedra") == ((7, 3), (6, 3))
    assert extract(ONE_CELL, "dual") == ((0, 3), (0, 3))                # a vertex and no triangle: empty as well


@pytest.mark.parametrize("method, limit, counts", [("tetrahedra", 6, "7 vertices and 6 triangles"), ("dual", 0, "1 vertices and 0 triangles")])
def test_more_than_the_limit_of_either_raises_before_anything_is_extracted(monkeypatch, method, limit, counts):
    monkeypatch.setattr(ISO, "MAX_ITEMS", limit)
    with pytest.raises(ValueError, match=rf"^extract_isosurface: {counts}; more than 2\^31 - 1 of either is not supported$"):
        extract(ONE_CELL, method)
    monkeypatch.setattr(ISO, "MAX_ITEMS", 7)
    assert extract(ONE_CELL, method)[0] == ((7, 3) if method == "tetrahedra" else (0, 3))
