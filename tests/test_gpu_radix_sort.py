"""The radix argsort kernels (csrc/sort.hip) called directly, the sort and
partition routes built on them with the route on and off, and one frame end
to end.

A stable sort's permutation is unique, so every comparison is
``torch.equal`` against ``np.argsort(kind="stable")`` of the same key on
the CPU.  Sizes are the smallest that cross each boundary of the design:
wave (64), block (256), tile (``RADIX_TILE``), a partial last tile, and
several tiles per block with an uneven split (``max_blocks`` 2 and 3).
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
# (n, max_blocks)
SIZES = [(n, 2048) for n in (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1)]
SIZES += [(3 * T + 17, 2), (5 * T + 1, 3)]
# 17 blocks: a count table of more than one round of the scan kernel
SIZES += [(17 * T + 3, 2048)]
_WORDS = ["other", "morning", "midday", "afternoon", "evening"]


def _check(keys, begin=0, end=-1, perm=None, max_blocks=2048, ref=None):
    """radix_argsort(keys...) == p[argsort(ref[p])], ref defaulting to keys."""
    ref = keys if ref is None else ref
    got = gpu.kernels().radix_argsort(
        torch.from_numpy(keys).to(_DEV), begin, end,
        None if perm is None else torch.from_numpy(perm).to(_DEV), max_blocks)
    exp = np.argsort(ref, kind="stable") if perm is None \
        else perm[np.argsort(ref[perm], kind="stable")]
    assert got.dtype == torch.int64 and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(exp.astype(np.int64)))


def _pattern(name, n, rng):
    if name == "equal":
        return np.full(n, 7, np.int64)
    if name == "few":
        return rng.integers(0, 3, n).astype(np.int64)
    if name == "descending":
        return np.arange(n, 0, -1, dtype=np.int64) * 1000003
    return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)


@pytest.mark.parametrize("pattern", ["equal", "few", "random", "descending"])
@pytest.mark.parametrize("n,max_blocks", SIZES)
def test_sizes_and_patterns(n, max_blocks, pattern):
    keys = _pattern(pattern, n, np.random.default_rng([1, n]))
    _check(keys, max_blocks=max_blocks)


@pytest.mark.parametrize("begin,end", [(0, 1), (0, 8), (0, 9), (0, 17),
                                       (0, 63), (5, 14)])
@pytest.mark.parametrize("n,max_blocks", [(T + 1, 2048), (3 * T + 17, 2)])
def test_bit_ranges_ignore_outside_bits(n, max_blocks, begin, end):
    keys = _pattern("random", n, np.random.default_rng([2, n, end]))
    ref = (keys.view(np.uint64) >> np.uint64(begin)) \
        & np.uint64((1 << (end - begin)) - 1)
    _check(keys, begin, end, max_blocks=max_blocks, ref=ref)


def _float_keys(dtype, n, rng):
    fi = np.finfo(dtype)
    # bits ...fffe: sign and exponent all ones, a payload -> a negative NaN
    neg_nan = np.array([-2], {np.float32: np.int32,
                              np.float64: np.int64}[dtype]).view(dtype)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.tiny / 4,
                        -fi.tiny / 4, fi.max, fi.min, 1.5, 1.5], dtype)
    special = np.concatenate([special, neg_nan])
    keys = rng.standard_normal(n).astype(dtype)
    keys[rng.permutation(n)[:4 * len(special)]] = np.tile(special, 4)
    nan = np.isnan(keys)
    assert np.signbit(keys[nan]).any() and not np.signbit(keys[nan]).all()
    return keys


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64,
                                   np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("n", [257, T + 1])
def test_dtypes(n, dtype):
    rng = np.random.default_rng([3, n])
    if np.issubdtype(dtype, np.floating):
        keys = _float_keys(dtype, n, rng)
    else:
        ii = np.iinfo(dtype)
        keys = rng.integers(ii.min, ii.max, n, dtype=dtype, endpoint=True)
        keys[rng.integers(0, n, 6)] = [ii.min, ii.max, 0, ii.min, ii.max, 0]
    _check(keys)


@pytest.mark.parametrize("pattern", ["few", "random"])
@pytest.mark.parametrize("n,max_blocks", [(T + 1, 2048), (3 * T + 17, 2)])
def test_through_permutation(n, max_blocks, pattern):
    rng = np.random.default_rng([4, n])
    _check(_pattern(pattern, n, rng), perm=rng.permutation(n).astype(np.int64),
           max_blocks=max_blocks)


# ---------------------------------------------------------------- routes

@pytest.fixture(params=[True, False], ids=["radix", "torch"])
def route(request, monkeypatch):
    monkeypatch.setattr(gpu, "RADIX_SORT", request.param)
    monkeypatch.setattr(gpu, "RADIX_SORT_FORCE", request.param)


def _key_columns(n):
    """name -> CPU column: a dictionary, a bool, a ranged integer, a float
    with NaN, a masked int32."""
    rng = np.random.default_rng([5, n])
    ranged = Column.from_numpy(rng.integers(-40, 900, n).astype(np.int64))
    ranged.val_range = (-40, 899)
    f = rng.integers(-5, 5, n) / 4.0
    f[rng.random(n) < 0.2] = np.nan
    return {
        "dict": Column.from_arrow(
            pa.array(rng.choice(_WORDS, n)).dictionary_encode()),
        "bool": Column.from_numpy(rng.random(n) < 0.5),
        "ranged": ranged,
        "float": Column.from_numpy(f),
        "masked": Column.from_numpy(rng.integers(-3, 3, n).astype(np.int32),
                                    mask=rng.random(n) < 0.8),
    }


def _ref_sort(cols, asc, na_position):
    idx = np.arange(len(cols[0]))
    for c, a in reversed(list(zip(cols, asc))):
        k = ops._sort_key_tensor(c, a, na_position).numpy()
        idx = idx[np.argsort(k[idx], kind="stable")]
    return torch.from_numpy(idx)


@pytest.mark.parametrize("names,asc,na_position", [
    (("dict", "bool", "ranged"), (False, True, False), "last"),
    (("float", "masked", "dict"), (True, False, True), "last"),
    (("float", "masked", "dict"), (False, True, False), "first"),
])
def test_sort_indices_routes(route, names, asc, na_position):
    cols = [_key_columns(T + 1)[k] for k in names]
    packable = ops.pack_ordered_keys(cols, asc) is not None
    assert packable == (names[0] == "dict")
    got = ops.sort_indices([c.to_device(_DEV) for c in cols], asc, na_position)
    assert torch.equal(got.cpu(), _ref_sort(cols, asc, na_position))


@pytest.mark.parametrize("nparts", [1, 2, 8, 257])
def test_partition_indices_routes(route, nparts):
    h = np.random.default_rng([6, nparts]).integers(
        -2**63, 2**63 - 1, 3 * T + 17, dtype=np.int64)
    perm, counts = ops.partition_indices(torch.from_numpy(h).to(_DEV), nparts)
    p = np.mod(h, nparts)
    assert torch.equal(perm.cpu(), torch.from_numpy(np.argsort(p, kind="stable")))
    assert torch.equal(counts.cpu(),
                       torch.from_numpy(np.bincount(p, minlength=nparts)))


def test_sort_values_and_order_by_end_to_end(route):
    import bodo_amd.config as cfg
    import bodo_amd.pandas as bpd
    from bodo_amd.sql import BodoSQLContext

    cfg.DEVICE = "cuda"
    n = 2 * T + 5
    rng = np.random.default_rng(7)
    df = pd.DataFrame({"a": rng.integers(-4, 4, n), "w": rng.choice(_WORDS, n),
                       "x": rng.integers(-8, 8, n) / 8.0, "i": np.arange(n)})
    exp = df.sort_values(["a", "w", "x"], ascending=[True, False, True],
                         kind="stable").reset_index(drop=True)
    got = bpd.from_pandas(df).sort_values(
        ["a", "w", "x"], ascending=[True, False, True]).to_pandas()
    got = got.reset_index(drop=True).astype({"w": object})
    pd.testing.assert_frame_equal(got, exp, check_dtype=False)
    got = BodoSQLContext({"t": df}).sql(
        "select a, w, x, i from t order by x desc, a").to_pandas()
    exp = df.sort_values(["x", "a"], ascending=[False, True],
                         kind="stable").reset_index(drop=True)
    got = got.reset_index(drop=True).astype({"w": object})
    pd.testing.assert_frame_equal(got, exp, check_dtype=False)
