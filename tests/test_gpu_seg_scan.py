"""The segmented scan kernels (csrc/window.hip) called directly, and the
window functions built on them called through ``_ordered_local_device``
(``_ordered_local`` would hide a broken kernel behind its pandas fallback).

The reference is a per-segment numpy loop on the CPU.  Every value in the
exact tests is an integer below 2^20 in magnitude, so float64 sums are exact
in any order and all comparisons are ``torch.equal``.  NaN is never fed
through ``values`` without its ``invalid`` bit: the window layer flags every
NaN before it calls the scan.
"""

import numpy as np
import pandas as pd
import pytest
import torch

from bodo_amd.core.table import Table
from bodo_amd.engine import window
from bodo_amd.ops import gpu

pytestmark = pytest.mark.gpu
_DEV = "cuda"
T = getattr(gpu._K, "SEG_SCAN_TILE", 2048)
OPS = gpu.SEG_SCAN_OPS
# (n, max_blocks); the last has more blocks than the spine has threads
MULTI = [(3 * T + 17, 2), (5 * T + 1, 3), (257 * T + 5, 2048)]
SIZES = [(n, 2048) for n in (1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1)]
PATTERNS = ["one", "all", "tiles", "around_tile", "long_then_short"]
CASES = [(n, mb, "random") for n, mb in SIZES + MULTI] + \
    [(n, mb, p) for n, mb in MULTI for p in PATTERNS]
_ACC = {"sum": np.cumsum, "min": np.minimum.accumulate,
        "max": np.maximum.accumulate}


def _ref(vals, heads, op, invalid=None, reverse=False, dtype=None):
    """(acc, cnt) of the scan, one numpy accumulate per segment."""
    n = len(vals)
    dtype = dtype or (np.int64 if op == "sum_i64" else np.float64)
    heads = heads.astype(bool).copy()
    invalid = np.zeros(n, bool) if invalid is None else invalid.astype(bool)
    if reverse:  # a row starts a reversed segment where its successor is a head
        vals, invalid, heads = vals[::-1], invalid[::-1], heads[::-1]
        heads = np.roll(heads, 1)
    heads[0] = True
    ident = {"sum": 0, "min": np.inf, "max": -np.inf}[op[:3]]
    x = np.where(invalid, ident, vals).astype(dtype)
    acc = np.empty(n, dtype)
    starts = np.flatnonzero(heads)
    for s, e in zip(starts, np.r_[starts[1:], n]):
        acc[s:e] = _ACC[op[:3]](x[s:e])
    upto = np.cumsum(~invalid)
    cnt = upto - (upto - ~invalid)[starts[np.cumsum(heads) - 1]]
    return (acc[::-1], cnt[::-1]) if reverse else (acc, cnt)


def _heads(pattern, n, rng):
    h = np.zeros(n, np.uint8)
    if pattern == "all":
        h[:] = 1
    elif pattern == "random":
        h = (rng.random(n) < 1 / 3).astype(np.uint8)
    elif pattern == "tiles":
        h[::T] = 1
    elif pattern == "around_tile":
        h[[T - 1, T + 1]] = 1
    elif pattern == "long_then_short":
        # blocks without a head take their carry through the spine
        h[n - n // 7::5] = 1
    return h


def _values(op, n, rng, dtype=None):
    v = rng.integers(-1000, 1000, n)
    return v.astype(dtype or (np.int64 if op == "sum_i64" else np.float64))


def _run(vals, heads, op, invalid=None, reverse=False, want_count=False,
         max_blocks=2048):
    dev = lambda a: None if a is None else torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a)).to(_DEV)
    out = gpu.kernels().seg_scan(dev(vals), dev(invalid), dev(heads), OPS[op],
                                 reverse, want_count, max_blocks)
    assert len(out) == 1 + want_count
    return [o.cpu() for o in out]


def _same(got, exp):
    assert got.dtype == torch.from_numpy(exp[:0].copy()).dtype
    assert torch.equal(got, torch.from_numpy(np.ascontiguousarray(exp)))


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("n,max_blocks,pattern", CASES)
def test_kernel_against_reference(n, max_blocks, pattern, op):
    rng = np.random.default_rng([1, n])
    vals, heads = _values(op, n, rng), _heads(pattern, n, rng)
    got, = _run(vals, heads, op, max_blocks=max_blocks)
    _same(got, _ref(vals, heads, op)[0])


N2, MB2 = 3 * T + 17, 2


@pytest.mark.parametrize("op", ["sum_i64", "max_f64"])
def test_reverse(op):
    rng = np.random.default_rng(2)
    vals, heads = _values(op, N2, rng), _heads("random", N2, rng)
    inv = rng.random(N2) < 0.3
    got = _run(vals, heads, op, inv.view(np.uint8), True, True, MB2)
    for g, e in zip(got, _ref(vals, heads, op, inv, reverse=True)):
        _same(g, e)


@pytest.mark.parametrize("op", list(OPS))
def test_count_and_invalid_rows(op):
    rng = np.random.default_rng(3)
    vals, heads = _values(op, N2, rng), _heads("random", N2, rng)
    inv = rng.random(N2) < 0.3
    starts = np.flatnonzero(heads)
    inv[starts[5]:starts[6]] = True      # a whole segment of invalid rows
    inv[starts[9]] = True                # an invalid row at a head
    got = _run(vals, heads, op, inv.view(np.uint8), want_count=True,
               max_blocks=MB2)
    for g, e in zip(got, _ref(vals, heads, op, inv)):
        _same(g, e)


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64,
                                   np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("op", ["sum", "min"])
def test_dtypes(op, dtype):
    rng = np.random.default_rng(4)
    is_int = np.issubdtype(dtype, np.integer)
    op = "min_f64" if op == "min" else "sum_i64" if is_int else "sum_f64"
    vals = rng.integers(0 if dtype == np.uint8 else -100, 100, N2).astype(dtype)
    heads = _heads("random", N2, rng)
    got, = _run(vals, heads, op, max_blocks=MB2)
    _same(got, _ref(vals, heads, op)[0])


def test_sum_i64_is_exact_past_2_53():
    rng = np.random.default_rng(5)
    vals = (2**60 - rng.integers(0, 1000, N2)) * rng.choice([-1, 1], N2)
    heads = _heads("random", N2, rng) | (np.arange(N2) % 4 == 0)
    got, = _run(vals, heads.astype(np.uint8), "sum_i64", max_blocks=MB2)
    _same(got, _ref(vals, heads, "sum_i64")[0])


def test_sum_f64_random_doubles_within_the_summation_bound():
    """|got - ref| <= (L-1) 2^-53 sum|x| over the row's prefix of length L:
    the bound of any summation order; the reference sums in longdouble."""
    rng = np.random.default_rng(6)
    vals, heads = rng.uniform(-1, 1, N2), _heads("random", N2, rng)
    got, = _run(vals, heads, "sum_f64", max_blocks=MB2)
    ref = _ref(vals, heads, "sum_f64", dtype=np.longdouble)[0]
    mag, length = _ref(np.abs(vals), heads, "sum_f64", dtype=np.longdouble)
    err = np.abs(got.numpy().astype(np.longdouble) - ref)
    assert (err <= (length - 1) * np.longdouble(2.0) ** -53 * mag).all()


# ---------------------------------------------------------------- window

def _window(df, specs, order_by=("o",)):
    out = window._ordered_local_device(
        Table.from_pandas(df, device=_DEV), ["k"], list(order_by),
        [True] * len(order_by), specs)
    return None if out is None else out.to_pandas()


@pytest.mark.parametrize("vals", [
    np.array([2**53 + 1, 1, 1, 3, 5, 7], np.int64),
    np.array([1e300, -1e300 / 3, 1e299, 0.1, 0.2, 0.3])])
def test_cumsum_of_a_partition_ignores_the_partitions_before_it(vals):
    df = pd.DataFrame({"k": [0, 0, 0, 1, 1, 1], "v": vals})
    got = _window(df, [("r", "v", "cumsum", None)], order_by=())
    assert got is not None
    exp = df.groupby("k")["v"].cumsum()
    assert got["r"].dtype == exp.dtype
    # twice the bound of any summation order; zero for the integers
    mag = df["v"].abs().groupby(df["k"]).cumsum() if vals.dtype.kind == "f" \
        else 0 * exp
    bound = 2 * df.groupby("k").cumcount() * 2.0 ** -53 * mag
    assert ((got["r"] - exp).abs() <= bound).all()


@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(7)
    n = 5000
    k = rng.integers(0, 36, n)
    k[0] = 36                                   # a single-row partition
    k[1:] = np.where(k[1:] == 36, 0, k[1:])
    f = rng.integers(-1000, 1000, n).astype(np.float64)
    f[rng.random(n) < 0.1] = np.nan
    i = pd.array(rng.integers(-1000, 1000, n), dtype="Int64")
    i[rng.random(n) < 0.1] = pd.NA
    return pd.DataFrame({"k": k, "o": rng.permutation(n), "f": f, "i": i})


def _expected(df, col, func, w):
    s = df.sort_values("o", kind="stable").astype({"i": "float64"})
    g = s.groupby("k", sort=False)[col]
    if func == "cumsum":
        res = g.cumsum()
    elif func == "cumcount_v":
        res = g.transform(lambda x: x.notna().cumsum())
    elif func.startswith("cum"):
        res = g.transform(lambda x: getattr(
            x.expanding(min_periods=1), func[3:])())
    else:
        res = getattr(g.rolling(w, min_periods=1), func[8:])().droplevel(0)
    return res.reindex(df.index)


_FUNCS = [(f, None) for f in ("cumsum", "cummean", "cumcount_v", "cummin",
                              "cummax")] + \
    [("rolling_" + b, w) for b in ("sum", "mean", "count", "min", "max")
     for w in (1, 3, 128, 129, 1000)]


@pytest.mark.parametrize("func,w", _FUNCS)
def test_window_functions_against_pandas(frame, func, w, monkeypatch):
    # narrow rolling min/max goes to torch by default; here the kernels
    monkeypatch.setattr(gpu, "SEG_SCAN_ROLLING_MINMAX_MIN_WIDTH", 1)
    got = _window(frame, [("rf", "f", func, w), ("ri", "i", func, w)])
    assert got is not None
    for col in "fi":
        exp, res = _expected(frame, col, func, w), got["r" + col]
        assert res.dtype == exp.dtype
        assert (res.isna() == exp.isna()).all()
        assert (res.dropna() == exp.dropna()).all()


def test_route_off_is_the_parent(frame, monkeypatch):
    monkeypatch.setattr(gpu, "SEG_SCAN", False)
    assert _window(frame, [("r", "f", "rolling_max", 200)]) is None
    got = _window(frame, [("r", "f", "cummax", None)])
    exp = _expected(frame, "f", "cummax", None)
    assert (got["r"].isna() == exp.isna()).all()
    assert (got["r"].dropna() == exp.dropna()).all()
