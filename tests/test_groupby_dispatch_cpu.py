"""CPU tests of the host side of groupby in ``bodo_amd.ops.gpu``:
``groupby_local``, ``_agg_one``, the fused and dense batches and
``distinct_local`` run on CPU tensors with ``gpu._K`` replaced by
``relational_sim.SimKernels``.

Values are compared with pandas; the launches (ops, identities, dtype kinds,
``want_count`` flags, masks) are compared with literal logs.  Float inputs
are small integers over 8, so every power sum up to the fourth is exact in
double and no result depends on the order of a summation.
"""

import datetime
import math
from functools import lru_cache

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

from bodo_amd.core.table import Table
from bodo_amd.core.types import TypeKind
from bodo_amd.ops import gpu
from tests.relational_ref import I64_MAX, I64_MIN
from tests.relational_sim import SimKernels

INF = math.inf


@pytest.fixture
def sim(monkeypatch):
    k = SimKernels()
    monkeypatch.setattr(gpu, "_K", k)
    return k


# ----------------------------------------------------------------------
# the frame
# ----------------------------------------------------------------------

N = 300
_WORDS = ["ash", "birch", "cedar", "elm", "fir", "oak", "pine"]


@lru_cache(maxsize=None)
def _frame():
    """300 rows in 12 groups.  Group 0 has no valid value in any nullable
    column and groups 1..4 have exactly 1, 2, 3 and 4 (the NaN thresholds
    of var/std/sem, skew and kurt); groups 5..11 have about 38 rows each
    with a fifth of them null."""
    rng = np.random.default_rng(81)
    k = np.concatenate([np.zeros(8), np.repeat([1, 2, 3, 4], 6),
                        rng.integers(5, 12, N - 32)]).astype(np.int64)
    null = np.zeros(N, dtype=bool)
    null[:8] = True
    for g in (1, 2, 3, 4):
        null[np.nonzero(k == g)[0][g:]] = True
    big = k >= 5
    null_f = null | (big & (rng.random(N) < 0.2))
    null_i = null | (big & (rng.random(N) < 0.2))
    null_d = null | (big & (rng.random(N) < 0.2))
    order = rng.permutation(N)
    k, null_f, null_i, null_d = k[order], null_f[order], null_i[order], \
        null_d[order]

    f64 = rng.integers(-64, 64, N) / 8.0
    f64[null_f] = np.nan
    i32 = pd.array(rng.integers(-50, 50, N).astype(np.int32), dtype="Int32")
    i32[null_i] = pd.NA
    b = rng.random(N) < 0.5
    b[k == 5] = True
    b[k == 6] = False
    words = np.array(_WORDS, dtype=object)[rng.integers(0, len(_WORDS), N)]
    words[null_d] = None
    day0 = datetime.date(2020, 1, 1)
    return pd.DataFrame({
        "k": k, "f64": f64, "i32": i32,
        "i64": rng.integers(-1000, 1000, N).astype(np.int64),
        "i8": rng.choice([-2, -1, 1, 2], N).astype(np.int8),
        "ts": pd.to_datetime(rng.integers(0, 2**60, N)),
        "d32": [day0 + datetime.timedelta(days=int(d))
                for d in rng.integers(-4000, 4000, N)],
        "b": b,
        "u16": rng.integers(0, 2**16, N).astype(np.uint16),
        "d": words, "s": words,
    })


def _table(df, dict_cols=("d",)):
    """No dictionary encoding but of ``dict_cols`` (``s`` stays a STRING),
    and float columns keep their NaNs and get no mask."""
    at = pa.Table.from_pandas(df, preserve_index=False)
    for i, name in enumerate(at.column_names):
        if df[name].dtype == np.float64:
            at = at.set_column(i, name, pa.array(df[name].to_numpy(),
                                                 from_pandas=False))
    for name in dict_cols:
        if name in at.column_names:
            i = at.column_names.index(name)
            at = at.set_column(
                i, name, at.column(i).combine_chunks().dictionary_encode())
    return Table.from_arrow(at)


def test_frame_layout():
    df, t = _frame(), _table(_frame())
    valid = df.groupby("k")[["f64", "i32", "d"]].count()
    for c in ("f64", "i32", "d"):
        assert valid[c].tolist()[:5] == [0, 1, 2, 3, 4], c
        assert (valid[c][5:] > 4).all()
    kinds = {n: t.column(n).dtype.kind for n in t.names}
    assert kinds == {
        "k": TypeKind.INT64, "f64": TypeKind.FLOAT64, "i32": TypeKind.INT32,
        "i64": TypeKind.INT64, "i8": TypeKind.INT8,
        "ts": TypeKind.TIMESTAMP_NS, "d32": TypeKind.DATE32,
        "b": TypeKind.BOOL, "u16": TypeKind.UINT16, "d": TypeKind.DICT,
        "s": TypeKind.STRING}
    masked = {n for n in t.names if t.column(n).mask is not None}
    assert masked == {"i32", "d", "s"}


# ----------------------------------------------------------------------
# values against pandas
# ----------------------------------------------------------------------

_MOMENTS = ("var", "std", "sem", "skew", "kurt")
_NUMERIC = ("sum", "mean", "min", "max", "count", "size", "first", "last",
            "any", "all", "median", "nunique") + _MOMENTS
_ORDERED = ("min", "max", "count", "size", "first", "last", "nunique")
FUNCS = {
    # not ``any`` over a float column with NaNs: a NaN counts as true
    # there, where pandas skips it
    "f64": tuple(f for f in _NUMERIC if f != "any") + ("prod",),
    "i32": _NUMERIC,
    "i64": _NUMERIC,
    "i8": ("sum", "prod", "min", "max", "mean"),
    "ts": _ORDERED,
    "d32": _ORDERED,
    "b": ("sum", "mean", "min", "max", "count", "first", "last", "any",
          "all", "nunique"),
    "u16": ("sum", "min", "max", "count", "first", "last", "nunique"),
    "d": ("count", "first", "last", "nunique"),
    "s": ("count", "first", "last", "nunique"),
}
# compared exactly; the rest to rtol 1e-9, the bound of the project's
# other kurtosis and skew tests
_EXACT = {"count", "size", "min", "max", "first", "last", "sum", "any",
          "all", "nunique"}
# A relative bound says nothing where the true value is 0: group 4 of f64
# holds four values symmetric about their mean, its skewness is exactly 0
# and pandas returns -1.35e-16, its own rounding of O(1) terms.  The
# absolute floor is 45 ulp of 1.0, a hundred-thousandth of rtol at the O(1)
# size of every other skewness and kurtosis here.
_ZERO_ATOL = 1e-14


def _pandas_func(f):
    return (lambda x: x.kurt()) if f == "kurt" else f


def _expected(df, keys, aggs, dropna=True):
    named = {o: (c or keys[0], _pandas_func(f)) for o, c, f in aggs}
    return df.groupby(keys, dropna=dropna).agg(**named).reset_index()


def _values(series):
    """Python values with None for every kind of null."""
    return [None if v is None or v is pd.NA or v is pd.NaT
            or (isinstance(v, float) and v != v) else v
            for v in series.tolist()]


def _assert_column(got, exp, func, what):
    if func in _EXACT:
        assert _values(got) == _values(exp), what
    else:
        g = pd.to_numeric(got).to_numpy(dtype=np.float64, na_value=np.nan)
        e = pd.to_numeric(exp).to_numpy(dtype=np.float64, na_value=np.nan)
        np.testing.assert_allclose(g, e, rtol=1e-9, atol=_ZERO_ATOL,
                                   equal_nan=True, err_msg=str(what))


def _check_groupby(df, tbl, keys, aggs, dropna=True):
    res = gpu.groupby_local(tbl, keys, aggs, dropna=dropna)
    assert res.names == list(keys) + [o for o, _, _ in aggs]
    got = res.to_pandas().sort_values(keys).reset_index(drop=True)
    exp = _expected(df, keys, aggs, dropna)
    assert len(got) == len(exp)
    for k in keys:
        assert _values(got[k]) == _values(exp[k]), k
    for o, _, f in aggs:
        _assert_column(got[o], exp[o], f, o)
    return res


@pytest.mark.parametrize("col", sorted(FUNCS))
def test_values_match_pandas(sim, col):
    """Every function of the fused path and of ``_agg_one`` over every
    column kind it is used with, but ``kurt`` (below)."""
    aggs = [(f"{col}_{f}", col, f) for f in FUNCS[col] if f != "kurt"]
    _check_groupby(_frame(), _table(_frame()), ["k"], aggs)


@pytest.mark.parametrize("col", ["f64", "i32", "i64"])
def test_kurt_matches_pandas(sim, col):
    _check_groupby(_frame(), _table(_frame()), ["k"],
                   [("kurt", col, "kurt")])


def test_moment_nan_thresholds(sim):
    """var/std/sem need 2 valid values, skew 3 and kurt 4."""
    df = _frame()
    aggs = [(f, "f64", f) for f in _MOMENTS]
    got = gpu.groupby_local(_table(df), ["k"], aggs).to_pandas() \
        .sort_values("k").reset_index(drop=True)
    for f, need in (("var", 2), ("std", 2), ("sem", 2), ("skew", 3),
                    ("kurt", 4)):
        nan = got[f].isna().tolist()
        assert nan == [g < need for g in range(12)], f


# ----------------------------------------------------------------------
# batching
# ----------------------------------------------------------------------

_HASH_BUILD = [("hash_columns", ("INT64",)), ("groupby_build", ("INT64",))]


def _launches(log):
    """(entry point, number of aggregates) per logged call."""
    return [(e[0], len(e[1])) if e[0] == "agg_update_fused" else (e[0], 1)
            for e in log]


_FUSABLE9 = [("a0", "f64", "sum"), ("a1", "i32", "mean"), ("a2", "i64", "min"),
             ("a3", "ts", "max"), ("a4", "", "size"), ("a5", "i32", "count"),
             ("a6", "b", "sum"), ("a7", "d32", "min"), ("a8", "f64", "max")]


@pytest.mark.parametrize("n_fusable", [1, 4, 5, 9])
def test_fused_batches(sim, n_fusable):
    """Fusable aggregates gather in batches of at most four, launched when
    the fourth arrives and at the end; an aggregate of ``_agg_one`` between
    them launches at once and does not break a batch up."""
    aggs = []
    for i, a in enumerate(_FUSABLE9[:n_fusable]):
        aggs.append(a)
        if i % 2 == 0:
            aggs.append((f"n{i}", "f64", "first" if i % 4 else "var"))
    _check_groupby(_frame(), _table(_frame()), ["k"], aggs)
    assert sim.log[:2] == _HASH_BUILD
    exp, pending = [], 0
    for _, _, f in aggs:
        if f in gpu.FUSABLE:
            pending += 1
            if pending == 4:
                exp.append(("agg_update_fused", 4))
                pending = 0
        else:
            exp += [("agg_update", 1)] * (2 if f == "var" else 1)
    if pending:
        exp.append(("agg_update_fused", pending))
    assert _launches(sim.log[2:]) == exp
    assert exp.count(("agg_update_fused", 4)) == n_fusable // 4


# ----------------------------------------------------------------------
# the shared-size mean
# ----------------------------------------------------------------------

def _clean_frame(nan_at=None):
    rng = np.random.default_rng(82)
    df = pd.DataFrame({"k": rng.integers(0, 7, 200).astype(np.int64),
                       "x": rng.integers(-64, 64, 200) / 8.0,
                       "i": rng.integers(-9, 9, 200).astype(np.int64)})
    if nan_at is not None:
        df.loc[nan_at, "x"] = np.nan
    return df


def _fused_wants(log):
    (fused,) = [e for e in log if e[0] == "agg_update_fused"]
    return [(op, want) for op, _, _, _, want, _ in fused[1]]


@pytest.mark.parametrize("partner", [("n", "", "size"), ("n", "i", "count")],
                         ids=["size", "count_non_nullable"])
def test_mean_shares_the_size_count(sim, partner):
    df = _clean_frame()
    _check_groupby(df, _table(df), ["k"], [("m", "x", "mean"), partner])
    assert _fused_wants(sim.log) == [("sum_f64", False), ("size", True)]


def test_shared_mean_divides_by_the_size_not_a_count(sim):
    """A count of a nullable column ahead of the size in the batch: its
    valid count is not the group size."""
    df = _clean_frame()
    df["y"] = df["x"].where(np.arange(len(df)) % 3 != 0)
    _check_groupby(df, _table(df), ["k"], [
        ("c", "y", "count"), ("m", "x", "mean"), ("n", "", "size")])
    assert _fused_wants(sim.log) == [("count", True), ("sum_f64", False),
                                     ("size", True)]


def test_mean_with_nan_keeps_its_count(sim):
    df = _clean_frame(nan_at=17)
    _check_groupby(df, _table(df), ["k"],
                   [("m", "x", "mean"), ("n", "", "size")])
    assert _fused_wants(sim.log) == [("sum_f64", True), ("size", True)]


def test_mean_without_size_keeps_its_count(sim):
    df = _clean_frame()
    _check_groupby(df, _table(df), ["k"],
                   [("m", "x", "mean"), ("s", "i", "sum")])
    assert _fused_wants(sim.log) == [("sum_f64", True), ("sum_i64", False)]


# ----------------------------------------------------------------------
# routes: 2 keys of radix 64 are 4096 slots, over the LDS limit of two
# aggregates (1536) and under 4 n for 2048 rows
# ----------------------------------------------------------------------

_ROUTE_AGGS = [("n", "", "size"), ("m", "x", "mean"), ("lo", "i", "min")]


def _route_frame(stray=False):
    rng = np.random.default_rng(83)
    n = 2048
    df = pd.DataFrame({"a": rng.integers(0, 64, n).astype(np.int64),
                       "b": (rng.integers(0, 64, n) - 32).astype(np.int16),
                       "x": rng.integers(-64, 64, n) / 8.0,
                       "i": rng.integers(-9, 9, n).astype(np.int64)})
    df.loc[rng.random(n) < 0.1, "x"] = np.nan
    if stray:
        df.loc[5, "b"] = 32
    t = _table(df)
    t.column("a").val_range = (0, 63)
    t.column("b").val_range = (-32, 31)
    return df, t


def _calls(log):
    return [e[0] for e in log]


def test_route_dense(sim):
    df, t = _route_frame()
    assert gpu.DENSE_GROUPBY
    _check_groupby(df, t, ["a", "b"], _ROUTE_AGGS)
    assert _calls(sim.log) == ["groupby_dense_fused"]
    assert sim.log[0][1:4] == (("INT64", "INT16"), (0, -32), (64, 64))


def test_route_key_outside_val_range(sim):
    """The dense kernel reports the stray key; the fallback compares the
    key columns and does not pack them with the bounds that were wrong."""
    df, t = _route_frame(stray=True)
    _check_groupby(df, t, ["a", "b"], _ROUTE_AGGS)
    assert _calls(sim.log) == ["groupby_dense_fused", "hash_columns",
                               "groupby_build", "agg_update_fused"]


def test_route_dense_off(sim, monkeypatch):
    monkeypatch.setattr(gpu, "DENSE_GROUPBY", False)
    df, t = _route_frame()
    _check_groupby(df, t, ["a", "b"], _ROUTE_AGGS)
    assert _calls(sim.log) == ["groupby_build_packed", "agg_update_fused"]


# ----------------------------------------------------------------------
# edges
# ----------------------------------------------------------------------

def _null_key_frame():
    rng = np.random.default_rng(84)
    n = 120
    ki = pd.array(rng.integers(0, 3, n), dtype="Int64")
    ki[rng.random(n) < 0.2] = pd.NA
    kf = rng.integers(0, 3, n) / 2.0
    kf[rng.random(n) < 0.2] = np.nan
    return pd.DataFrame({"ki": ki, "kf": kf,
                         "x": rng.integers(-64, 64, n) / 8.0})


@pytest.mark.parametrize("dropna", [True, False])
def test_null_keys(sim, dropna):
    df = _null_key_frame()
    aggs = [("n", "", "size"), ("s", "x", "sum"), ("v", "x", "var")]
    res = gpu.groupby_local(_table(df), ["ki", "kf"], aggs, dropna=dropna)
    got = res.to_pandas()
    exp = _expected(df, ["ki", "kf"], aggs, dropna)
    assert len(got) == len(exp) == (9 if dropna else 16)
    assert got["ki"].isna().any() == (not dropna)

    def rows(frame):
        cols = [_values(frame[c]) for c in ("ki", "kf", "n", "s")]
        return sorted(zip(zip(*cols), frame["v"].tolist()),
                      key=lambda row: repr(row[0]))
    for (gk, gv), (ek, ev) in zip(rows(got), rows(exp)):
        assert gk == ek
        np.testing.assert_allclose(gv, ev, rtol=1e-9, equal_nan=True)


def test_zero_rows(sim):
    df = _frame().iloc[:0]
    aggs = [("n", "", "size"), ("c", "f64", "count"), ("u", "d", "nunique"),
            ("m", "f64", "mean"), ("lo", "i64", "min"), ("v", "f64", "var")]
    res = gpu.groupby_local(_table(df), ["k", "d"], aggs)
    assert len(res) == 0 and sim.log == []
    assert res.names == ["k", "d", "n", "c", "u", "m", "lo", "v"]
    assert [c.dtype.kind for c in res.columns] == [
        TypeKind.INT64, TypeKind.DICT, TypeKind.INT64, TypeKind.INT64,
        TypeKind.INT64, TypeKind.FLOAT64, TypeKind.FLOAT64, TypeKind.FLOAT64]
    assert all(len(c) == 0 for c in res.columns)


def _distinct_frame():
    rng = np.random.default_rng(85)
    n = 150
    return pd.DataFrame({"a": rng.integers(0, 12, n).astype(np.int64),
                         "b": rng.integers(0, 6, n).astype(np.int32),
                         "r": np.arange(n, dtype=np.int64)})


@pytest.mark.parametrize("keep", ["first", "last", False])
def test_distinct_local(sim, keep):
    df = _distinct_frame()
    got = gpu.distinct_local(_table(df), ["a", "b"], keep=keep).to_pandas()
    exp = df.drop_duplicates(["a", "b"], keep=keep).reset_index(drop=True)
    assert 0 < len(exp) < len(df)
    pd.testing.assert_frame_equal(got, exp, check_exact=True)


def test_distinct_local_any_member(sim):
    """Any other ``keep`` returns one row of each group, whichever the build
    claimed, in original row order."""
    df = _distinct_frame()
    got = gpu.distinct_local(_table(df), ["a", "b"], keep="any").to_pandas()
    assert got["r"].is_monotonic_increasing
    pd.testing.assert_frame_equal(
        got, df.loc[got["r"]].reset_index(drop=True), check_exact=True)
    exp = df.drop_duplicates(["a", "b"])
    assert sorted(zip(got["a"], got["b"])) == sorted(zip(exp["a"], exp["b"]))


def test_distinct_local_all_columns_and_empty(sim):
    df = _distinct_frame()[["a", "b"]]
    got = gpu.distinct_local(_table(df)).to_pandas()
    pd.testing.assert_frame_equal(
        got, df.drop_duplicates().reset_index(drop=True), check_exact=True)
    assert len(gpu.distinct_local(_table(df.iloc[:0]))) == 0


# ----------------------------------------------------------------------
# the pinned launch log
# ----------------------------------------------------------------------

# one request per branch of the fused specs, then one per family of
# _agg_one; all group _frame() by k
_PIN_GROUPBY = {
    "size": [("o", "", "size")],
    "count_non_nullable": [("o", "i64", "count")],
    "count_nullable": [("o", "f64", "count"), ("p", "d", "count")],
    "sum_float": [("o", "f64", "sum")],
    "mean_own_count": [("o", "i32", "mean"), ("p", "f64", "mean")],
    "mean_shared_count": [("o", "i8", "sum"), ("p", "x", "mean"),
                          ("q", "", "size")],
    "sum_int": [("o", "i64", "sum"), ("p", "b", "sum"), ("q", "u16", "sum")],
    "minmax_float": [("o", "f64", "min"), ("p", "f64", "max")],
    "minmax_int": [("o", "i32", "min"), ("p", "ts", "max"),
                   ("q", "d32", "min"), ("r", "b", "max")],
    "var": [("o", "f64", "var")],
    "sem": [("o", "i32", "sem")],
    "skew": [("o", "i32", "skew")],
    "kurt": [("o", "i64", "kurt")],
    "any": [("o", "b", "any")],
    "first": [("o", "f64", "first")],
    "prod": [("o", "i8", "prod")],
    "nunique": [("o", "d", "nunique")],
    "string_count": [("o", "s", "count")],
}


def _pinned_log(sim, name):
    if name in _PIN_GROUPBY:
        df = _frame().assign(x=np.arange(N) / 8.0)  # a NaN-free float column
        gpu.groupby_local(_table(df), ["k"], _PIN_GROUPBY[name])
    elif name == "dense":
        _, t = _route_frame()
        gpu.groupby_local(t, ["a", "b"], _ROUTE_AGGS)
    else:
        keep = {"distinct_first": "first", "distinct_last": "last",
                "distinct_none": False}[name]
        gpu.distinct_local(_table(_distinct_frame()), ["a", "b"], keep=keep)
    return sim.log


def _one(*entry):
    return ("agg_update",) + entry


_POWER = _one("sum_f64", "FLOAT64", 0.0, 0, False, False)
_POWER_MASKED = _one("sum_f64", "FLOAT64", 0.0, 0, False, True)
_DISTINCT_BUILD = [("hash_columns", ("INT64", "INT32")),
                   ("groupby_build", ("INT64", "INT32"))]

# What each request launches: entry point, op, dtype kind the kernel reads
# the column as, (init_f, init_i), want_count, mask passed.  Captured from
# the code as it was before the aggregates became table-driven.  Since then
# one thing moved, on purpose: the first launch of skew and kurt reads the
# column in its own type (INT32, INT64 below) where it read a float64 copy.
PINNED = {
    "size": _HASH_BUILD + [
        ("agg_update_fused", (("size", "INT8", 0.0, 0, True, False),))],
    "count_non_nullable": _HASH_BUILD + [
        ("agg_update_fused", (("size", "INT8", 0.0, 0, True, False),))],
    "count_nullable": _HASH_BUILD + [
        ("agg_update_fused", (("count", "FLOAT64", 0.0, 0, True, False),
                              ("count", "DICT", 0.0, 0, True, True)))],
    "sum_float": _HASH_BUILD + [
        ("agg_update_fused", (("sum_f64", "FLOAT64", 0.0, 0, True, False),))],
    "mean_own_count": _HASH_BUILD + [
        ("agg_update_fused", (("sum_f64", "INT32", 0.0, 0, True, True),
                              ("sum_f64", "FLOAT64", 0.0, 0, True, False)))],
    "mean_shared_count": _HASH_BUILD + [
        ("agg_update_fused", (("sum_i64", "INT8", 0.0, 0, False, False),
                              ("sum_f64", "FLOAT64", 0.0, 0, False, False),
                              ("size", "INT8", 0.0, 0, True, False)))],
    "sum_int": _HASH_BUILD + [
        ("agg_update_fused", (("sum_i64", "INT64", 0.0, 0, False, False),
                              ("sum_i64", "BOOL", 0.0, 0, False, False),
                              ("sum_i64", "UINT16", 0.0, 0, False, False)))],
    "minmax_float": _HASH_BUILD + [
        ("agg_update_fused", (("min_f64", "FLOAT64", INF, 0, True, False),
                              ("max_f64", "FLOAT64", -INF, 0, True, False)))],
    "minmax_int": _HASH_BUILD + [
        ("agg_update_fused", (
            ("min_i64", "INT32", 0.0, I64_MAX, True, True),
            ("max_i64", "TIMESTAMP_NS", 0.0, I64_MIN, True, False),
            ("min_i64", "DATE32", 0.0, I64_MAX, True, False),
            ("max_i64", "BOOL", 0.0, I64_MIN, True, False)))],
    "var": _HASH_BUILD + [
        _one("sum_f64", "FLOAT64", 0.0, 0, True, False), _POWER],
    "sem": _HASH_BUILD + [
        _one("sum_f64", "INT32", 0.0, 0, True, True), _POWER_MASKED],
    "skew": _HASH_BUILD + [
        _one("sum_f64", "INT32", 0.0, 0, True, True),
        _POWER_MASKED, _POWER_MASKED],
    "kurt": _HASH_BUILD + [
        _one("sum_f64", "INT64", 0.0, 0, True, False),
        _POWER, _POWER, _POWER],
    "any": _HASH_BUILD + [
        _one("max_i64", "INT64", 0.0, I64_MIN, True, False)],
    "first": _HASH_BUILD + [
        _one("first_row", "FLOAT64", 0.0, I64_MAX, True, False)],
    "prod": _HASH_BUILD + [_one("prod_f64", "INT8", 1.0, 0, True, False)],
    "nunique": _HASH_BUILD + [("hash_columns", ("INT32", "DICT")),
                              ("groupby_build", ("INT32", "DICT"))],
    "string_count": _HASH_BUILD + [
        _one("count", "STRING", 0.0, 0, False, True)],
    "distinct_first": _DISTINCT_BUILD + [
        _one("first_row", "INT8", 0.0, I64_MAX, False, False)],
    "distinct_last": _DISTINCT_BUILD + [
        _one("last_row", "INT8", 0.0, I64_MIN, False, False)],
    "distinct_none": _DISTINCT_BUILD + [
        _one("size", "INT8", 0.0, 0, True, False)],
    "dense": [("groupby_dense_fused", ("INT64", "INT16"), (0, -32), (64, 64),
               (("size", "INT8", 0.0, 0, False),
                ("sum_f64", "FLOAT64", 0.0, 0, False),
                ("min_i64", "INT64", 0.0, I64_MAX, False)))],
}


@pytest.mark.parametrize("name", list(PINNED))
def test_pinned_launch_log(sim, name):
    assert _pinned_log(sim, name) == PINNED[name]


# ----------------------------------------------------------------------
# the stand-in refuses what the kernels refuse or cannot survive
# ----------------------------------------------------------------------

def test_stand_in_contracts():
    import torch

    k = SimKernels()
    gid = torch.arange(16, dtype=torch.int32) % 2
    one = torch.zeros(1, dtype=torch.int8)
    col = torch.ones(16, dtype=torch.float64)
    assert len(k.agg_update(one, None, None, 0, gid, 2, 7, 0.0, 0,
                            False)) == 2                       # size
    assert len(k.agg_update(col, None, None, 5, gid, 2, 0, 0.0, 0,
                            False)) == 1                       # sum_f64
    flat = k.agg_update_fused([col], [None], [5], [0], [0.0], [0], [0],
                              gid, 2)
    assert flat[0].dtype == torch.float64 and flat[1].numel() == 0
    for bad in (
            # first_row reads row i of its column: no placeholder
            lambda: k.agg_update(one, None, None, 0, gid, 2, 8, 0.0, I64_MAX,
                                 False),
            # not the identity of min_f64
            lambda: k.agg_update(col, None, None, 5, gid, 2, 3, 0.0, 0, True),
            # int64 row_gid, bool data, bool mask
            lambda: k.agg_update(col, None, None, 5, gid.long(), 2, 0, 0.0,
                                 0, True),
            lambda: k.agg_update(col > 0, None, None, 6, gid, 2, 1, 0.0, 0,
                                 False),
            lambda: k.agg_update(col, col > 0, None, 5, gid, 2, 0, 0.0, 0,
                                 True),
            # no fused form of first_row; five aggregates
            lambda: k.agg_update_fused([col], [None], [5], [8], [0.0],
                                       [I64_MAX], [1], gid, 2),
            lambda: k.agg_update_fused([col] * 5, [None] * 5, [5] * 5,
                                       [0] * 5, [0.0] * 5, [0] * 5, [1] * 5,
                                       gid, 2),
            lambda: k.groupby_dense_fused([gid], [2], [0], [2], [col], [None],
                                          [5], [10], [1.0], [0], 16)):
        with pytest.raises(RuntimeError):
            bad()
    # a key outside [lo, lo + radix): nothing computed
    assert k.groupby_dense_fused([gid], [2], [1], [2], [col], [None], [5],
                                 [0], [0.0], [0], 16) == []
    slots, acc, cnt = k.groupby_dense_fused(
        [gid], [2], [0], [2], [col], [None], [5], [0], [0.0], [0], 16)
    assert slots.tolist() == [0, 1] and acc.tolist() == [8.0, 8.0]
    assert cnt.tolist() == [8, 8]
