"""CPU tests of the host side of the dense (direct-address) groupby and
join routes in ``bodo_amd.ops.gpu``: the slot encoding against a numpy
model, the eligibility rules at each of their boundaries, and the join's
lookup-table build (plain torch ops, so it runs on CPU tensors)."""

import numpy as np
import pyarrow as pa
import pytest
import torch

from bodo_amd.core import types as bt
from bodo_amd.core.column import Column
from bodo_amd.ops import gpu
from tests.relational_ref import np_encode


# ----------------------------------------------------------------------
# slot encoding
# ----------------------------------------------------------------------

@pytest.mark.parametrize("plan", [
    [(1, 265), (1, 265), (1, 12), (0, 2), (0, 2), (0, 5)],  # the flagship
    [(-2**63, 7)],
    [(2**63 - 9, 9), (-5, 1), (0, 2)],                      # a radix-1 key
    [(0, 1), (0, 1)],
    [(-300, 1000), (7, 1), (-128, 256)],
])
def test_slot_encoding_round_trips(plan):
    rng = np.random.default_rng(len(plan))
    n = 4099
    keys = [(rng.integers(0, radix, n) + lo).astype(np.int64)
            for lo, radix in plan]
    for key, (lo, radix) in zip(keys, plan):  # both ends of every range
        key[:2] = [lo, lo + radix - 1]
    slots, nslots = np_encode(keys, plan)
    assert nslots == int(np.prod([r for _, r in plan], dtype=object))
    assert slots.min() >= 0 and slots.max() < nslots
    digits = gpu.slot_digits(torch.from_numpy(slots), plan)
    assert len(digits) == len(plan)
    for key, (lo, _), digit in zip(keys, plan, digits):
        np.testing.assert_array_equal((digit + lo).numpy(), key)
    # distinct key rows get distinct slots
    rows = np.stack(keys, axis=1)
    assert len(np.unique(rows, axis=0)) == len(np.unique(slots))


# ----------------------------------------------------------------------
# groupby eligibility
# ----------------------------------------------------------------------

def _int_key(lo, hi, mask=False):
    c = Column(bt.int64, torch.zeros(4, dtype=torch.int64),
               torch.ones(4, dtype=torch.bool) if mask else None)
    c.val_range = (lo, hi)
    return c


def _f64():
    return Column(bt.float64, torch.zeros(4, dtype=torch.float64))


def _string():
    return Column.from_arrow(pa.array(["a", "b", "c", "d"]))


_MEAN = [("m", _f64(), "mean")]
_BIG_N = 1 << 30


def test_plan_flagship_shape():
    keys = [_int_key(1, 265), _int_key(1, 265), _int_key(1, 12),
            Column(bt.boolean, torch.zeros(4, dtype=torch.bool)),
            Column(bt.dictionary, torch.zeros(4, dtype=torch.int32),
                   dictionary=pa.array(list("abcde"), type=pa.large_string()))]
    plan = gpu.dense_groupby_plan(keys, [("n", None, "size")] + _MEAN, _BIG_N)
    assert plan == [(1, 265), (1, 265), (1, 12), (0, 2), (0, 5)]


def test_plan_slot_limit():
    at = [_int_key(0, 2**13 - 1), _int_key(-5, 2**12 - 6)]       # 2^25
    assert gpu.dense_groupby_plan(at, _MEAN, _BIG_N) == \
        [(0, 2**13), (-5, 2**12)]
    over = [_int_key(0, 2**25)]                                  # 2^25 + 1
    assert gpu.dense_groupby_plan(over, _MEAN, _BIG_N) is None
    assert gpu.dense_groupby_plan([_int_key(0, 2**25 - 1)], _MEAN,
                                  _BIG_N) is not None


def test_plan_table_no_larger_than_4n():
    keys = [_int_key(0, 3999)]                                   # 4000 slots
    assert gpu.dense_groupby_plan(keys, _MEAN, 1000) is not None
    assert gpu.dense_groupby_plan(keys, _MEAN, 999) is None


def test_plan_lds_line():
    """n_aggs * nslots * 16 B <= 48 KiB stays with the LDS kernel."""
    two = [("n", None, "size")] + _MEAN
    assert gpu.dense_groupby_plan([_int_key(0, 3071)], _MEAN, _BIG_N) is None
    assert gpu.dense_groupby_plan([_int_key(0, 3072)], _MEAN,
                                  _BIG_N) == [(0, 3073)]
    assert gpu.dense_groupby_plan([_int_key(0, 1535)], two, _BIG_N) is None
    assert gpu.dense_groupby_plan([_int_key(0, 1536)], two,
                                  _BIG_N) is not None


def test_plan_aggregates():
    keys = [_int_key(0, 9999)]
    four = [(f"a{i}", _f64(), f) for i, f in
            enumerate(("sum", "mean", "min", "max"))]
    assert gpu.dense_groupby_plan(keys, four, _BIG_N) is not None
    five = four + [("n", None, "size")]
    assert gpu.dense_groupby_plan(keys, five, _BIG_N) is None
    assert gpu.dense_groupby_plan(keys, [], _BIG_N) is None
    assert gpu.dense_groupby_plan(keys, [("s", _string(), "count")],
                                  _BIG_N) is None
    assert gpu.dense_groupby_plan(keys, [("v", _f64(), "var")],
                                  _BIG_N) is None


def test_plan_keys():
    assert gpu.dense_groupby_plan([_int_key(0, 9999, mask=True)], _MEAN,
                                  _BIG_N) is None
    no_range = Column(bt.int64, torch.zeros(4, dtype=torch.int64))
    assert gpu.dense_groupby_plan([no_range], _MEAN, _BIG_N) is None
    assert gpu.dense_groupby_plan([_f64()], _MEAN, _BIG_N) is None
    assert gpu.dense_groupby_plan([_int_key(0, 9999)] * 9, _MEAN,
                                  _BIG_N) is None
    # the packed route and the dense route read the same bounds
    assert gpu._key_bounds(_int_key(-3, 4)) == (-3, 4)
    assert gpu._key_bounds(_int_key(-3, 4, mask=True)) is None


# ----------------------------------------------------------------------
# join eligibility and lookup table
# ----------------------------------------------------------------------

def _key(values, dtype=bt.int64, mask=None):
    store = bt.torch_storage_dtype(dtype)
    return Column(dtype, torch.tensor(values, dtype=store),
                  None if mask is None else torch.tensor(mask))


def test_join_eligibility():
    b, p = _key([1, 2, 3]), _key([3, 3, 9, 1])
    assert gpu.dense_join_eligible([b], [p], "inner")
    for how in ("left", "outer", "semi", "anti", "right"):
        assert not gpu.dense_join_eligible([b], [p], how)
    assert not gpu.dense_join_eligible([b, b], [p, p], "inner")
    assert not gpu.dense_join_eligible([_key([1], bt.int32)], [p], "inner")
    assert gpu.dense_join_eligible([_key([1], bt.date32)],
                                   [_key([1, 2], bt.date32)], "inner")
    assert not gpu.dense_join_eligible([_f64()], [_f64()], "inner")
    # one masked side is fine; with both the hash route pairs null with null
    bm = _key([1, 2, 3], mask=[True, False, True])
    pm = _key([3, 3, 9, 1], mask=[True, True, False, True])
    assert gpu.dense_join_eligible([bm], [p], "inner")
    assert gpu.dense_join_eligible([b], [pm], "inner")
    assert not gpu.dense_join_eligible([bm], [pm], "inner")


def test_join_lut():
    lut, lo, dup = gpu._dense_join_lut(_key([7, 3, 5]))
    assert lo == 3 and not bool(dup)
    assert lut.dtype == torch.int32
    assert lut.tolist() == [1, -1, 2, -1, 0]


def test_join_lut_null_build_rows_left_out():
    lut, lo, dup = gpu._dense_join_lut(
        _key([7, 100, 5, 5], mask=[True, False, True, False]))
    assert (lut.tolist(), lo, bool(dup)) == ([2, -1, 0], 5, False)


def test_join_lut_duplicate_flag():
    _, _, dup = gpu._dense_join_lut(_key([7, 3, 7]))
    assert bool(dup)


def test_join_lut_empty_and_span():
    lut, lo, dup = gpu._dense_join_lut(_key([]))
    assert (lut.tolist(), lo, bool(dup)) == ([-1], 0, False)
    lut, lo, dup = gpu._dense_join_lut(_key([5], mask=[False]))
    assert lut.tolist() == [-1]
    assert gpu._dense_join_lut(_key([0, 2**22 - 1])) is not None
    assert gpu._dense_join_lut(_key([0, 2**22])) is None
    assert gpu._dense_join_lut(_key([-2**63, 2**63 - 1])) is None


@pytest.mark.parametrize("base", [-2**63, 2**63 - 4])
def test_join_lut_at_the_ends_of_int64(base):
    lut, lo, dup = gpu._dense_join_lut(_key([base + 3, base, base + 1]))
    assert (lut.tolist(), lo, bool(dup)) == ([1, 2, -1, 0], base, False)
