"""The packed sort key reports its width: what the radix sort route is told
about how many key bits matter."""

import numpy as np
import pyarrow as pa
import pytest
import torch

from bodo_amd import ops
from bodo_amd.core.column import Column


def _ranged(lo, hi, n, rng):
    c = Column.from_numpy(rng.integers(lo, hi, n, endpoint=True))
    c.val_range = (lo, hi)
    return c


def _columns(n=500):
    rng = np.random.default_rng(8)
    return {
        "dict5": Column.from_arrow(pa.array(
            rng.choice(["a", "bb", "c", "dd", "e"], n)).dictionary_encode()),
        "bool": Column.from_numpy(rng.random(n) < 0.5),   # 2 values: 2 bits
        "r940": _ranged(-40, 899, n, rng),        # 940 values: 10 bits
        "r256": _ranged(0, 255, n, rng),          # 256 values: 9 bits
        "r1": _ranged(5, 5, n, rng),              # one value: 1 bit
        "wide": _ranged(0, 2**40, n, rng),        # 41 bits
        "float": Column.from_numpy(rng.random(n)),
    }


@pytest.mark.parametrize("names,asc,nbits", [
    (("dict5", "bool", "r940"), (False, True, False), 3 + 2 + 10),
    (("r256", "r1"), (True, True), 9 + 1),
    (("bool",), (False,), 2),
    (("wide", "r940", "r256", "dict5"), (True, False, True, True), 63),
])
def test_packed_width(names, asc, nbits):
    cols = [_columns()[k] for k in names]
    packed, got_bits = ops._pack_ordered_keys_bits(cols, asc)
    assert torch.equal(packed, ops.pack_ordered_keys(cols, asc))
    assert got_bits == nbits
    assert 0 <= int(packed.min()) and int(packed.max()) < 2 ** nbits


@pytest.mark.parametrize("names", [("float",), ("wide", "wide"), ()])
def test_unpackable_has_no_width(names):
    cols = [_columns()[k] for k in names]
    asc = [True] * len(cols)
    assert ops._pack_ordered_keys_bits(cols, asc) == (None, 0)
    assert ops.pack_ordered_keys(cols, asc) is None
