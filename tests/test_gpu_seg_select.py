"""The segmented radix select (csrc/segselect.hip) called directly, the grouped
median with the route on against the route off, and median / quantile /
PERCENTILE_* / Series.quantile through the public interface against pandas.

The kernel rounds nothing: lo and hi are compared exactly with the entries
``[r]`` and ``[min(r + 1, L - 1)]`` of ``np.sort(segment)`` (NaN last, equal
to NaN; -0.0 equal to 0.0).  Lengths sit on every boundary between the wave,
block and large classes and the tile.
"""

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

from bodo_amd.core.column import Column
from bodo_amd.ops import gpu, relational

pytestmark = pytest.mark.gpu
_DEV = "cuda"
W = gpu.kernels().SEG_WAVE_KEYS
B = gpu.kernels().SEG_BLOCK_KEYS
T = gpu.kernels().RADIX_TILE
LENGTHS = [1, 2, 63, 64, 65, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + T + 5]
DTYPES = ["int8", "int32", "int64", "float32", "float64"]
PATTERNS = ["equal", "two", "random", "low8", "top"]
INTERPOLATIONS = ["linear", "lower", "higher", "midpoint", "nearest"]


def _keys(dtype, pattern, n, rng):
    """n keys of `dtype`; the float ones are integer patterns seen as floats
    (NaNs, infinities and subnormals among them) plus the special values."""
    dt = np.dtype(dtype)
    it = np.dtype(f"int{8 * dt.itemsize}")
    bits = 8 * dt.itemsize
    if pattern == "equal":
        k = np.full(n, -7, it)
    elif pattern == "two":
        k = (rng.integers(0, 2, n) * (1 << (bits - 3)) - 5).astype(it)
    elif pattern == "low8":  # one bin until the last digit: every pass runs
        k = ((0x0123456789ABCD00 >> (64 - bits)) & ~0xFF) + rng.integers(0, 256, n)
        k = k.astype(np.uint64).astype(f"uint{bits}").view(it)
    elif pattern == "top":  # one key per top digit while n <= 256: early stop
        k = ((rng.permutation(n) % 256 - 128).astype(np.int64)
             << (bits - 8)).astype(it)
    else:
        info = np.iinfo(it)
        k = rng.integers(info.min, info.max, n, dtype=it, endpoint=True)
    k = k.view(dt).copy()
    if dt.kind == "f" and pattern == "random" and n >= 8:
        k[rng.choice(n, 6, replace=False)] = [-0.0, 0.0, np.inf, -np.inf,
                                              np.nan, np.nan]
    return k


def _ranks(L):
    return [0, (L - 1) // 2, L // 2, L - 1, L + 3]


def _check(keys, lengths, ranks, max_blocks):
    """One call over segments of `lengths` (0: empty) laid end to end."""
    start = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    lo, hi = gpu.seg_select(torch.from_numpy(keys).to(_DEV),
                            torch.from_numpy(start).to(_DEV),
                            torch.tensor(ranks, dtype=torch.int64, device=_DEV),
                            max_blocks)
    exp_lo, exp_hi = np.zeros(len(lengths), keys.dtype), \
        np.zeros(len(lengths), keys.dtype)
    for s, L in enumerate(lengths):
        if L:
            seg = np.sort(keys[start[s]:start[s + 1]])
            r = min(max(ranks[s], 0), L - 1)
            exp_lo[s], exp_hi[s] = seg[r], seg[min(r + 1, L - 1)]
    assert lo.dtype == hi.dtype == torch.from_numpy(keys).dtype
    np.testing.assert_array_equal(lo.cpu().numpy(), exp_lo)
    np.testing.assert_array_equal(hi.cpu().numpy(), exp_hi)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_length_alone(dtype, pattern):
    rng = np.random.default_rng([1, DTYPES.index(dtype), PATTERNS.index(pattern)])
    for L in LENGTHS:
        keys = _keys(dtype, pattern, L, rng)
        for max_blocks in ([1, 2, 3] if L > B else [2]):
            for r in _ranks(L):
                _check(keys, [L], [r], max_blocks)


@pytest.mark.parametrize("max_blocks", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_lengths_in_one_call(dtype, max_blocks):
    """Empty segments between the others; the large segments start mid-tile."""
    rng = np.random.default_rng([2, DTYPES.index(dtype)])
    lengths = [x for L in reversed(LENGTHS) for x in (3, 0, L, 0)]
    for pattern in ("random", "two", "low8"):
        keys = _keys(dtype, pattern, sum(lengths), rng)
        for pick in range(5):
            _check(keys, lengths, [_ranks(L)[pick] for L in lengths], max_blocks)


def test_negative_rank_and_no_segments():
    keys = np.arange(10, dtype=np.int32)
    _check(keys, [10], [-4], 2)
    _check(keys, [], [], 2)
    _check(keys[:0], [0, 0], [0, 1], 2)


def _group_case(n, ngroups, seed):
    """Group ids with one group above the block class and many small ones."""
    rng = np.random.default_rng(seed)
    gid = rng.integers(0, ngroups, n)
    gid[: 2 * B + 7] = 1
    return rng, rng.permutation(gid).astype(np.int32)


@pytest.mark.parametrize("name", ["masked", "nan", "big_int64", "bool"])
def test_median_route_on_equals_route_off(monkeypatch, name):
    n, ngroups = 3 * B, 40
    rng, gid = _group_case(n, ngroups, 3)
    mask = None
    if name == "masked":
        data = rng.integers(-99, 99, n).astype(np.int32)
        mask = (rng.random(n) < 0.8) & (gid != 5)  # group 5 is all null
    elif name == "nan":
        data = rng.integers(-50, 50, n) / 4.0
        data[(rng.random(n) < 0.1) | (gid == 5)] = np.nan
    elif name == "big_int64":
        data = 2**62 + rng.integers(-2**40, 2**40, n) * 3
    else:
        data = rng.random(n) < 0.5
    col = Column.from_numpy(data, mask=mask).to_device(_DEV)
    row_gid = torch.from_numpy(gid).to(_DEV)
    out = {}
    monkeypatch.setattr(gpu, "SEG_SELECT_MEDIAN_MIN_GROUP_ROWS", 0)
    for on in (True, False):
        monkeypatch.setattr(gpu, "SEG_SELECT", on)
        med = gpu._median_by_group(col, row_gid, ngroups)
        assert med.data.dtype == torch.float64
        out[on] = med.data.cpu().numpy()
    np.testing.assert_array_equal(out[True], out[False])
    assert np.isnan(out[True][5]) == (name in ("masked", "nan"))


@pytest.mark.parametrize("storage", ["signed", "unsigned"])
@pytest.mark.parametrize("dtype", ["uint16", "uint32", "uint64"])
def test_wide_unsigned_columns(dtype, storage):
    """Values in the upper half of the range, in both storages a column of
    these kinds can have, grouped and as a masked single segment."""
    from bodo_amd.pandas.series import BodoSeries
    from bodo_amd.plan.nodes import QuantileAgg

    n, ngroups = 3 * B, 7
    rng, gid = _group_case(n, ngroups, 5)
    top = np.iinfo(dtype).max
    data = rng.integers(top // 2, top, n, dtype=dtype, endpoint=True)
    col = Column.from_numpy(data).to_device(_DEV) if storage == "signed" \
        else Column.from_arrow(pa.array(data)).to_device(_DEV)
    got = gpu._quantile_by_group(col, torch.from_numpy(gid).to(_DEV), ngroups,
                                 QuantileAgg(0.3, "higher")).data.cpu().numpy()
    exp = pd.Series(data).groupby(gid).agg(
        lambda s: s.quantile(0.3, interpolation="higher"))
    np.testing.assert_array_equal(got, exp.to_numpy().astype(np.float64))
    mask = rng.random(n) < 0.7
    col = Column.from_numpy(data, mask=mask).to_device(_DEV)
    got = BodoSeries._quantile_gpu(col, [0.5], "lower")
    assert got == [float(np.quantile(data[mask], 0.5, method="lower"))]


@pytest.fixture
def frames(monkeypatch):
    """A GPU table and its pandas twin; the host groupby is an error."""
    import bodo_amd.config as cfg
    import bodo_amd.pandas as bpd

    def no_host(*a, **kw):
        raise AssertionError("the groupby went to the host")

    monkeypatch.setattr(cfg, "DEVICE", "cuda")
    monkeypatch.setattr(relational, "_groupby_pandas", no_host)
    n = 3 * B
    rng, gid = _group_case(n, 40, 4)
    x = rng.integers(-1000, 1000, n) / 8.0
    x[rng.random(n) < 0.05] = np.nan
    df = pd.DataFrame({"g": gid, "x": x,
                       "i": rng.integers(-10**6, 10**6, n).astype(np.int32),
                       "u": rng.integers(2**31, 2**32, n, dtype=np.uint32)})
    return bpd.from_pandas(df), df


def _close(got, exp, col):
    """Order statistics are exact and an interpolation rounds at most three
    times on each side: 4 ulp of the column's largest magnitude."""
    atol = 4 * 2.0**-52 * float(np.nanmax(np.abs(col)))
    np.testing.assert_allclose(np.asarray(got, float), np.asarray(exp, float),
                               rtol=0, atol=atol)


def test_groupby_median(frames):
    bdf, df = frames
    got = bdf.groupby("g", as_index=False)[["x", "i"]].median() \
        .to_pandas().sort_values("g")
    exp = df.groupby("g", as_index=False)[["x", "i"]].median()
    for c in ("x", "i"):
        np.testing.assert_array_equal(got[c].to_numpy(), exp[c].to_numpy())


@pytest.mark.filterwarnings("error:.*falling back to pandas")
@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
@pytest.mark.parametrize("q", [0, 0.3, 0.5, 1])
def test_groupby_quantile(frames, q, interpolation):
    bdf, df = frames
    got = bdf.groupby("g", as_index=False).quantile(
        q, interpolation=interpolation).to_pandas().sort_values("g")
    ser = bdf.groupby("g")["x"].quantile(q, interpolation).sort_index()
    exp = df.groupby("g").agg(
        lambda s: s.quantile(q, interpolation=interpolation))
    for c in ("x", "i", "u"):
        if interpolation in ("lower", "higher", "nearest"):
            np.testing.assert_array_equal(got[c].to_numpy(), exp[c].to_numpy())
        else:
            _close(got[c], exp[c], df[c])
    np.testing.assert_array_equal(ser.to_numpy(), got["x"].to_numpy())


def test_sql_percentiles(frames):
    from bodo_amd.sql import BodoSQLContext

    bdf, df = frames
    got = BodoSQLContext({"t": bdf}).sql(
        "select g, percentile_cont(0.3) within group (order by x) as pc, "
        "percentile_disc(0.7) within group (order by i) as pd, "
        "sum(i) as s from t group by g").to_pandas().sort_values("g")
    gb = df.groupby("g")
    _close(got["pc"], gb["x"].agg(lambda s: s.quantile(0.3)), df["x"])
    np.testing.assert_array_equal(
        got["pd"].to_numpy(),
        gb["i"].agg(lambda s: s.quantile(0.7, interpolation="nearest")))
    np.testing.assert_array_equal(got["s"].to_numpy(), gb["i"].sum())


def test_series_quantile(frames, monkeypatch):
    from bodo_amd.pandas.series import BodoSeries

    def no_gather(self):
        raise AssertionError("the series went to the host")

    bdf, df = frames
    monkeypatch.setattr(BodoSeries, "to_pandas", no_gather)
    qs = [0.25, 0.5, 0.75]
    got = bdf["x"].quantile(qs)
    assert list(got.index) == qs
    _close(got, df["x"].quantile(qs), df["x"])
    assert bdf["i"].median() == df["i"].median()
    assert bdf["u"].quantile(0.3, "lower") == df["u"].quantile(
        0.3, interpolation="lower")
    assert bdf["i"].quantile(0.3, "higher") == df["i"].quantile(
        0.3, interpolation="higher")
