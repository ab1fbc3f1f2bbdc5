"""ops.topk_indices and gpu.topk_route where no GPU is involved: CPU tensors
keep the full sort, and the route refuses what the kernel does not take."""

import numpy as np
import pytest
import torch

from bodo_amd import ops
from bodo_amd.core.column import Column
from bodo_amd.ops import gpu


def _cols(names, n=500):
    rng = np.random.default_rng(11)
    ranged = Column.from_numpy(rng.integers(0, 50, n).astype(np.int64))
    ranged.val_range = (0, 49)
    f = rng.integers(-20, 20, n) / 4.0
    f[::7] = np.nan
    pool = {"ranged": ranged, "float": Column.from_numpy(f),
            "flag": Column.from_numpy(rng.random(n) < 0.5),
            "masked": Column.from_numpy(rng.integers(-9, 9, n).astype(np.int32),
                                        mask=rng.random(n) < 0.8)}
    return [pool[c] for c in names]


@pytest.mark.parametrize("names,asc", [
    (("float",), (False,)),                      # single
    (("ranged", "flag"), (False, True)),         # packed
    (("masked", "float", "ranged"), (True, False, True)),
])
@pytest.mark.parametrize("k", [0, 1, 37, 500, 600])
def test_cpu_topk_is_the_sorted_prefix(monkeypatch, names, asc, k):
    monkeypatch.setattr(gpu, "TOPK_SELECT_MIN_ROWS", 0)
    cols = _cols(names)
    assert (ops.pack_ordered_keys(cols, asc) is not None) == \
        (names[0] == "ranged")
    for na_position in ("first", "last"):
        assert torch.equal(ops.topk_indices(cols, asc, na_position, k),
                           ops.sort_indices(cols, asc, na_position)[:k])


class _Shape:
    """What topk_route looks at, for row counts no test can allocate."""
    is_cuda, dtype = True, torch.int64

    def __init__(self, n):
        self._n = n

    def numel(self):
        return self._n


def test_topk_route(monkeypatch):
    n = max(gpu.TOPK_SELECT_MIN_ROWS, 1024)
    k = max(1, int(n * gpu.TOPK_SELECT_MAX_FRACTION))
    assert gpu.topk_route(_Shape(n), k)
    assert not gpu.topk_route(torch.zeros(n, dtype=torch.int64), k)  # CPU
    assert not gpu.topk_route(_Shape(n), n)
    assert not gpu.topk_route(_Shape(n), n + 1)
    assert not gpu.topk_route(_Shape(n), 0)
    assert gpu.topk_route(_Shape(2**31 - 1), 10)
    assert not gpu.topk_route(_Shape(2**31), 10)
    monkeypatch.setattr(gpu, "TOPK_SELECT", False)
    assert not gpu.topk_route(_Shape(n), k)
