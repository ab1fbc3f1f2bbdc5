"""The radix select kernels (csrc/select.hip) called directly, ops.topk_indices
against the full sort it replaces, and Limit(Sort) through the public
interface with the route on and off.

Nothing is rounded, so every comparison is ``torch.equal`` against a numpy
stable argsort of the same keys.  Sizes are the smallest that cross each
boundary: wave (64), tile (``RADIX_TILE``), a ragged last tile, several tiles
per block (``max_blocks`` 1 to 3), the survivor buffer's capacity, and once
more tiles than the 2048-block grid.
"""

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

from bodo_amd import ops
from bodo_amd.core.column import Column
from bodo_amd.ops import gpu

pytestmark = pytest.mark.gpu
_DEV = "cuda"
T = getattr(gpu._K, "RADIX_TILE", 2048)
NS = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
TIES = ["first", "all"]


def _ks(n):
    return sorted({1, 2, n // 2, n - 1, n, n + 3})


def _expect(K, k, ties):
    """sort(o[:k]), or with ties="all" every row at or below K[o[k-1]]."""
    o = np.argsort(K, kind="stable")
    if ties == "all" and 0 < k < len(K):
        s = K[o]
        same = np.isnan(s) if s.dtype.kind == "f" and np.isnan(s[k - 1]) \
            else s == s[k - 1]
        k = np.nonzero(same)[0][-1] + 1
    return torch.from_numpy(np.sort(o[:max(k, 0)]).astype(np.int64))


def _check(keys, ks, max_blocks=2048, begin=0, end=None, ref=None):
    dev = torch.from_numpy(keys).to(_DEV)
    for ties in TIES:
        for k in ks:
            got = gpu.radix_select(dev, k, begin, end, ties=ties,
                                   max_blocks=max_blocks)
            assert got.dtype == torch.int64 and got.is_cuda
            exp = _expect(keys if ref is None else ref, k, ties)
            assert torch.equal(got.cpu(), exp), (ties, k)


def _pattern(name, n, rng):
    if name == "equal":
        return np.full(n, -7, np.int64)
    if name == "two":
        return rng.integers(0, 2, n).astype(np.int64) * 2**40 - 5
    if name == "low8":  # one bin until the last digit: every pass runs
        return 0x0123456789ABCD00 + rng.integers(0, 256, n)
    if name == "top":  # one key per top digit while n <= 256: early stop
        return (rng.permutation(n) % 256 - 128).astype(np.int64) << 56
    return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)


@pytest.mark.parametrize("pattern", ["equal", "two", "random", "low8", "top"])
@pytest.mark.parametrize("max_blocks", [1, 2, 3])
@pytest.mark.parametrize("n", NS)
def test_sizes_and_patterns(n, max_blocks, pattern):
    keys = _pattern(pattern, n, np.random.default_rng([1, n]))
    _check(keys, _ks(n), max_blocks)


@pytest.mark.parametrize("extra", [0, 1], ids=["fits", "overflows"])
@pytest.mark.parametrize("max_blocks", [2, 2048])
def test_survivor_buffer_capacity(max_blocks, extra):
    """The lowest top digit holds exactly the buffer's capacity of keys, or
    one more (the column is then read again through the prefix filter)."""
    n = 3 * T + 5
    m = gpu.kernels().select_capacity(n) + extra
    assert m < n
    rng = np.random.default_rng([2, extra])
    keys = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    low = rng.permutation(n)[:m]
    keys[keys >> 56 == -128] += 2**60
    keys[low] = (keys[low] & (2**56 - 1)) + np.iinfo(np.int64).min
    assert (keys >> 56 == -128).sum() == m
    _check(keys, [1, m // 2, m - 1, m, m + 1], max_blocks)


def _float_keys(dtype, n, rng):
    keys = rng.integers(-3, 4, n).astype(dtype) / 2
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], dtype)
    keys[rng.permutation(n)[:12]] = np.tile(special, 2)
    return keys


@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.int64, np.uint8,
                                   np.bool_, np.float32, np.float64])
@pytest.mark.parametrize("n,max_blocks", [(65, 2048), (T + 1, 2048),
                                          (3 * T + 5, 2)])
def test_dtypes(n, max_blocks, dtype):
    rng = np.random.default_rng([3, n])
    if dtype is np.bool_:
        keys = rng.random(n) < 0.5
    elif np.issubdtype(dtype, np.floating):
        keys = _float_keys(dtype, n, rng)
    else:
        ii = np.iinfo(dtype)
        keys = rng.integers(ii.min, ii.max, n, dtype=dtype, endpoint=True)
        keys[rng.permutation(n)[:4]] = [ii.min, ii.max, ii.min, ii.max]
    _check(keys, _ks(n), max_blocks)


@pytest.mark.parametrize("begin,end", [(0, 1), (0, 17), (5, 14), (3, 64)])
def test_bit_range_ignores_outside_bits(begin, end):
    n = 3 * T + 5
    keys = _pattern("random", n, np.random.default_rng([4, end]))
    ref = ((keys.view(np.uint64) ^ np.uint64(1 << 63)) >> np.uint64(begin)) \
        & np.uint64((1 << (end - begin)) - 1)
    _check(keys, _ks(n), 3, begin, end, ref)


def test_ties_all_max_out():
    keys = np.random.default_rng(5).integers(0, 3, T + 1).astype(np.int32)
    exp = _expect(keys, 10, "all")
    dev = torch.from_numpy(keys).to(_DEV)
    assert gpu.radix_select(dev, 10, ties="all", max_out=len(exp) - 1) is None
    got = gpu.radix_select(dev, 10, ties="all", max_out=len(exp))
    assert torch.equal(got.cpu(), exp)


@pytest.mark.parametrize("n,k", [(2**16 + 1, 1000),
                                 (2050 * T + 7, 10), (2050 * T + 7, 2**18)])
def test_many_blocks(n, k):
    """2050 tiles: the grid stops at 2048 blocks and two of them own two."""
    keys = np.random.default_rng([6, n]).integers(
        -2**31, 2**31 - 1, n, dtype=np.int32)
    _check(keys, [k])


def test_bad_arguments():
    dev = torch.zeros(8, dtype=torch.int32, device=_DEV)
    with pytest.raises(ValueError):
        gpu.radix_select(dev, 2, ties="last")
    assert gpu.radix_select(dev, 0).numel() == 0
    assert gpu.radix_select(dev[:0], 3).numel() == 0


# ---------------------------------------------------------------- routes

@pytest.fixture
def counted(monkeypatch):
    """The route open to small inputs, and how often the kernel ran."""
    calls = []
    real = gpu.radix_select
    monkeypatch.setattr(gpu, "TOPK_SELECT_MIN_ROWS", 0)
    monkeypatch.setattr(gpu, "TOPK_SELECT_MAX_FRACTION", 0.5)
    monkeypatch.setattr(gpu, "radix_select",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    return calls


def _key_columns(n):
    rng = np.random.default_rng([7, n])
    ranged = Column.from_numpy(rng.integers(-40, 900, n).astype(np.int64))
    ranged.val_range = (-40, 899)
    f = rng.integers(-50, 50, n) / 4.0
    f[rng.random(n) < 0.1] = np.nan
    words = ["other", "morning", "midday", "afternoon", "evening"]
    return {
        "dict": Column.from_arrow(
            pa.array(rng.choice(words, n)).dictionary_encode()),
        "str": Column.from_arrow(pa.array(rng.choice(words, n))),
        "ranged": ranged,
        "float": Column.from_numpy(f),
        "four": Column.from_numpy(rng.integers(0, 4, n) / 2.0),
        "masked": Column.from_numpy(rng.integers(-99, 99, n).astype(np.int32),
                                    mask=rng.random(n) < 0.8),
    }


@pytest.mark.parametrize("names,asc,na_position,ran", [
    (("dict", "ranged"), (False, True), "last", True),        # packed
    (("float",), (True,), "last", True),
    (("float", "ranged"), (False, True), "first", True),
    (("masked", "dict"), (True, False), "last", True),
    (("masked", "dict"), (False, True), "first", True),
    (("four", "float", "masked"), (True, True, True), "last", True),  # None
    (("str", "ranged"), (True, True), "last", False),         # sort route
])
def test_topk_indices_equals_sorted_prefix(counted, names, asc, na_position,
                                           ran):
    cols = [_key_columns(3 * T + 5)[c].to_device(_DEV) for c in names]
    full = ops.sort_indices(cols, asc, na_position)
    for k in (1, 10, T):
        assert torch.equal(ops.topk_indices(cols, asc, na_position, k),
                           full[:k])
    assert bool(counted) == ran


@pytest.mark.parametrize("on", [True, False], ids=["select", "sort"])
def test_limit_sort_through_public_interface(counted, monkeypatch, on):
    import bodo_amd.config as cfg
    import bodo_amd.pandas as bpd
    from bodo_amd.sql import BodoSQLContext

    monkeypatch.setattr(cfg, "DEVICE", "cuda")
    monkeypatch.setattr(gpu, "TOPK_SELECT", on)
    n = 2 * T + 5
    rng = np.random.default_rng(8)
    df = pd.DataFrame({"a": rng.integers(-40, 40, n) / 4.0,
                       "b": rng.integers(0, 1000, n), "i": np.arange(n)})
    bdf = bpd.from_pandas(df)

    def same(got, exp):
        pd.testing.assert_frame_equal(got.reset_index(drop=True),
                                      exp.reset_index(drop=True),
                                      check_dtype=False)

    same(bdf.nlargest(7, "b").to_pandas(),
         df.sort_values("b", ascending=False, kind="stable").head(7))
    got = bdf["b"].nsmallest(9)
    assert list(got) == list(df["b"].sort_values(kind="stable").head(9))
    by = dict(by=["a", "b"], ascending=[False, True])
    same(bdf.sort_values(**by).head(11).to_pandas(),
         df.sort_values(kind="stable", **by).head(11))
    same(BodoSQLContext({"t": df}).sql(
        "select a, b, i from t order by a desc, b limit 11 offset 3"
    ).to_pandas(), df.sort_values(kind="stable", **by).iloc[3:14])
    assert bool(counted) == on
