"""Differential tests of the dense (direct-address) groupby and join
routes: ``gpu.groupby_local`` and ``gpu.join_local`` with the route on and
off, and ``groupby_dense_fused`` called without the eligibility rules,
against pandas on the same inputs.

Float inputs of sums are k / 1024 (``relational_cases``), so every partial
sum is exact, the order of the atomics cannot matter and results are
compared exactly after sorting the groups by key.  Nothing here asserts
which route ran: below ``n_aggs * nslots * 16 B == 48 KiB`` or above
``nslots == 4 n`` ``groupby_local`` keeps the hash route, which is why the
small sizes also call the dense route directly.
"""

from functools import lru_cache

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest
import torch

from tests import relational_cases as C
from tests import relational_ref as R

pytestmark = pytest.mark.gpu
_DEV = "cuda"


@pytest.fixture(autouse=True)
def _cuda_required():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------
# dense groupby
# ----------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 257, 70001)
KEYS = ["k_i64", "k_i16", "k_u8", "k_b", "k_d", "k_one"]
_WORDS = ["other", "morning", "midday", "afternoon", "evening"]
# radix of k_i64 per size: with the other keys' 120 combinations the table
# has 120 * r0 slots, which for 257 and 70,001 rows lies between the 48 KiB
# line of four aggregates (768 slots) and 4 n
_R0 = {70001: 100, 257: 7}
AGG_SETS = {
    "size_count_sum_mean": [("n", None, "size"), ("c_im", "im", "count"),
                            ("s_i", "i", "sum"), ("m_f", "f", "mean")],
    "sumf_minmaxf_minim": [("s_f", "f", "sum"), ("lo_g", "g", "min"),
                           ("hi_g", "g", "max"), ("lo_im", "im", "min")],
    "maxim_minmaxi_countf": [("hi_im", "im", "max"), ("lo_i", "i", "min"),
                             ("hi_i", "i", "max"), ("c_f", "f", "count")],
}


@lru_cache(maxsize=None)
def _gb_frame(n):
    """Keys of every packable kind and four value columns.  k_i64 uses
    the lower 60 % of its val_range (empty slots) and every row with
    k_i64 == -3 is null in f, g and im (groups without a valid value)."""
    rng = np.random.default_rng([71, n])
    r0 = _R0.get(n, 4)
    used = max(1, (r0 * 3) // 5)
    k0 = (rng.integers(0, used, n) - 3).astype(np.int64)
    dead = k0 == -3
    f = C._agg_values("float64", n, rng)
    f[rng.random(n) < 0.2] = np.nan
    f[dead] = np.nan
    g = C._agg_values("float64", n, rng)
    g[rng.random(n) < 0.1] = np.inf
    g[rng.random(n) < 0.1] = -np.inf
    g[rng.random(n) < 0.2] = np.nan
    g[dead] = np.nan
    im_valid = (rng.random(n) > 0.2) & ~dead
    df = pd.DataFrame({
        "k_i64": k0,
        "k_i16": rng.integers(-2, 1, n).astype(np.int16),
        "k_u8": rng.integers(250, 254, n).astype(np.uint8),
        "k_b": rng.integers(0, 2, n).astype(bool),
        "k_d": rng.integers(0, 5, n).astype(np.int32),
        "k_one": np.full(n, 7, dtype=np.int32),
        "i": C._agg_values("int64", n, rng),
        "f": f, "g": g,
        "im": rng.integers(-1000, 1000, n).astype(np.int64),
    })
    return df, im_valid, r0


def _gb_table(n, k0_range=None):
    from bodo_amd.core import types as bt
    from bodo_amd.core.column import Column
    from bodo_amd.core.table import Table

    df, im_valid, r0 = _gb_frame(n)
    cols = {}
    for name in df.columns:
        if name == "k_d":
            cols[name] = Column(
                bt.dictionary, torch.from_numpy(df[name].to_numpy().copy()),
                dictionary=pa.array(_WORDS, type=pa.large_string()))
        elif name == "im":
            cols[name] = Column.from_numpy(df[name].to_numpy().copy(),
                                           mask=im_valid.copy())
        else:
            cols[name] = Column.from_numpy(df[name].to_numpy().copy())
    cols["k_i64"].val_range = k0_range or (-3, r0 - 4)
    cols["k_i16"].val_range = (-2, 0)
    cols["k_u8"].val_range = (250, 253)
    cols["k_one"].val_range = (7, 7)
    return Table(list(cols), [c.to_device(_DEV) for c in cols.values()], n)


@lru_cache(maxsize=None)
def _gb_expected(n, set_name):
    df, im_valid, _ = _gb_frame(n)
    pdf = df.copy()
    pdf["im"] = pd.array(df["im"].to_numpy(), dtype="Int64")
    pdf.loc[~im_valid, "im"] = pd.NA
    pdf["k_d"] = np.array(_WORDS, dtype=object)[df["k_d"].to_numpy()]
    named = {o: (i or "k_i64", f) for o, i, f in AGG_SETS[set_name]}
    exp = pdf.groupby(KEYS, sort=True).agg(**named).reset_index()
    for o, (_, f) in named.items():
        if str(exp[o].dtype) == "Int64":
            # a masked column's min/max comes back as float64
            exp[o] = exp[o].astype("float64" if f in ("min", "max")
                                   else "int64")
    return exp


def _check_groups(got_tbl, n, set_name, what):
    exp = _gb_expected(n, set_name)
    got = got_tbl.to_pandas()
    got["k_d"] = got["k_d"].astype(object)
    got = got.sort_values(KEYS).reset_index(drop=True)
    assert len(got) == len(exp), (what, len(got), len(exp))
    for c in exp.columns:
        g, e = got[c].to_numpy(), exp[c].to_numpy()
        if c not in KEYS:
            assert g.dtype == e.dtype, (what, c, g.dtype, e.dtype)
        np.testing.assert_array_equal(g, e, err_msg=str((what, c)))
    return got


@pytest.mark.parametrize("set_name", sorted(AGG_SETS))
@pytest.mark.parametrize("n", SIZES)
def test_groupby_local_dense_on_off_pandas(n, set_name, monkeypatch):
    from bodo_amd.ops import gpu

    t = _gb_table(n)
    aggs = AGG_SETS[set_name]
    monkeypatch.setattr(gpu, "DENSE_GROUPBY", True)
    on = _check_groups(gpu.groupby_local(t, KEYS, aggs), n, set_name, "on")
    monkeypatch.setattr(gpu, "DENSE_GROUPBY", False)
    off = _check_groups(gpu.groupby_local(t, KEYS, aggs), n, set_name, "off")
    pd.testing.assert_frame_equal(on, off, check_exact=True)


@pytest.mark.parametrize("set_name", sorted(AGG_SETS))
@pytest.mark.parametrize("n", SIZES)
def test_groupby_dense_direct(n, set_name):
    """The dense route itself at every size, and its key columns: dtype,
    dictionary object and val_range of a gather of the input keys."""
    from bodo_amd.ops import gpu

    t = _gb_table(n)
    key_cols = [t.column(k) for k in KEYS]
    batch = [(o, t.column(i) if i else None, f)
             for o, i, f in AGG_SETS[set_name]]
    plan = [gpu._key_bounds(c) for c in key_cols]
    plan = [(lo, hi - lo + 1) for lo, hi in plan]
    res = gpu._groupby_dense(KEYS, key_cols, batch, plan, n)
    assert res is not None
    _check_groups(res, n, set_name, "direct")
    for k, c in zip(KEYS, key_cols):
        r = res.column(k)
        assert r.dtype == c.dtype and r.data.dtype == c.data.dtype, k
        assert r.mask is None and r.dictionary is c.dictionary, k
        assert r.val_range == c.val_range, k


@pytest.mark.parametrize("k0_range", [(-3, 40), (-2, 96), (-1, 30)],
                         ids=["above_hi", "below_lo", "both"])
def test_groupby_val_range_narrower_than_data(k0_range):
    """Keys outside val_range (k_i64 runs from -3 to 56): the dense kernel
    reports it and computes nothing, and groupby_local still returns the
    right groups.  All three ranges keep the table above the 48 KiB line,
    so groupby_local does try the dense route: the packed hash build
    trusts val_range and is not what this test is about."""
    from bodo_amd.ops import gpu

    n = 70001
    t = _gb_table(n, k0_range=k0_range)
    set_name = "size_count_sum_mean"
    aggs = AGG_SETS[set_name]
    key_cols = [t.column(k) for k in KEYS]
    batch = [(o, t.column(i) if i else None, f) for o, i, f in aggs]
    plan = [gpu._key_bounds(c) for c in key_cols]
    plan = [(lo, hi - lo + 1) for lo, hi in plan]
    assert gpu._groupby_dense(KEYS, key_cols, batch, plan, n) is None
    _check_groups(gpu.groupby_local(t, KEYS, aggs), n, set_name, k0_range)


# ----------------------------------------------------------------------
# dense join
# ----------------------------------------------------------------------

PROBE_SIZES = (0, 1, 65, 70001)
_I64_LO = -2**63


def _join_inputs(case, n_probe):
    """(build keys, probe keys, probe validity or None, kind name)."""
    rng = np.random.default_rng([72, n_probe, sorted(JOIN_CASES).index(case)])
    kind = "int64"
    valid = None
    if case == "all_matched":
        bk = rng.permutation(np.arange(-5, 360)).astype(np.int64)
        pk = rng.integers(-5, 360, n_probe).astype(np.int64)
    elif case == "some_unmatched":
        # holes inside the range, probe keys below lo and above hi
        bk = rng.permutation(np.arange(100, 465)[np.arange(365) % 7 != 3])
        bk = bk.astype(np.int64)
        pk = rng.integers(80, 490, n_probe).astype(np.int64)
        if n_probe > 2:
            pk[:2] = [99, 465]
    elif case == "date32":
        kind = "date32"
        bk = rng.permutation(np.arange(19358, 19358 + 365)).astype(np.int32)
        pk = rng.integers(19350, 19358 + 370, n_probe).astype(np.int32)
    elif case in ("int64_low_end", "int64_high_end"):
        base = _I64_LO if case == "int64_low_end" else 2**63 - 300
        bk = np.array([base + int(d) for d in rng.permutation(300)[:200]],
                      dtype=np.int64)
        far = np.array([0, -1, 1, 2**63 - 1, _I64_LO, 2**62, -2**62],
                       dtype=np.int64)
        near = np.array([base + int(d) for d in rng.integers(0, 300, n_probe)],
                        dtype=np.int64)
        pk = np.where(rng.random(n_probe) < 0.3,
                      far[rng.integers(0, len(far), n_probe)], near)
    elif case == "masked_probe":
        bk = rng.permutation(np.arange(0, 365)).astype(np.int64)
        pk = rng.integers(0, 365, n_probe).astype(np.int64)
        valid = rng.random(n_probe) > 0.3
    elif case == "empty_build":
        bk = np.zeros(0, dtype=np.int64)
        pk = rng.integers(0, 365, n_probe).astype(np.int64)
    elif case == "duplicate_build_key":
        bk = np.concatenate([rng.permutation(np.arange(0, 365)), [17]])
        bk = bk.astype(np.int64)
        pk = rng.integers(0, 365, n_probe).astype(np.int64)
        if n_probe:
            pk[0] = 17
    elif case == "int32_probe_int64_build":
        kind = "int32"
        bk = rng.permutation(np.arange(-5, 360)).astype(np.int64)
        pk = rng.integers(-20, 380, n_probe).astype(np.int32)
    else:
        raise ValueError(case)
    return bk, pk, valid, kind


JOIN_CASES = {
    "all_matched", "some_unmatched", "date32", "int64_low_end",
    "int64_high_end", "masked_probe", "empty_build", "duplicate_build_key",
    "int32_probe_int64_build",
}


def _join_tables(case, n_probe):
    from bodo_amd.core import types as bt
    from bodo_amd.core.column import Column
    from bodo_amd.core.table import Table

    bk, pk, valid, kind = _join_inputs(case, n_probe)
    rng = np.random.default_rng(73)
    left = pd.DataFrame({"k": pk, "lv": np.arange(len(pk), dtype=np.int64)})
    right = pd.DataFrame({"k": bk, "rv": np.arange(len(bk), dtype=np.int64),
                          "w": rng.integers(0, 2**20, len(bk)) / 1024.0})

    def key_col(vals, mask=None):
        if kind == "date32":
            return Column(bt.date32, torch.from_numpy(vals.copy()))
        return Column.from_numpy(vals.copy(), mask=mask)

    lt = Table(["k", "lv"], [key_col(pk, valid).to_device(_DEV),
                             Column.from_numpy(left["lv"].to_numpy())
                             .to_device(_DEV)], len(pk))
    rt = Table(["k", "rv", "w"],
               [key_col(bk).to_device(_DEV)] +
               [Column.from_numpy(right[c].to_numpy()).to_device(_DEV)
                for c in ("rv", "w")], len(bk))
    if valid is not None:
        left["k"] = pd.array(pk, dtype="Int64")
        left.loc[~valid, "k"] = pd.NA
    exp = left.merge(right, on="k", how="inner")
    return lt, rt, exp, kind


def _joined(gpu, lt, rt, ordered):
    got = gpu.join_local(lt, rt, ["k"], ["k"], "inner").to_pandas()
    assert list(got.columns) == ["k", "lv", "rv", "w"]
    if not ordered:
        got = got.sort_values(["lv", "rv"]).reset_index(drop=True)
    return got


@pytest.mark.parametrize("n_probe", PROBE_SIZES)
@pytest.mark.parametrize("case", sorted(JOIN_CASES))
def test_join_local_dense_on_off_pandas(case, n_probe, monkeypatch):
    """Probe order, one match each: the rows of pandas' inner merge in its
    order (left order), whichever route ran.  With a duplicate build key
    the order of a probe row's matches is the hash chain's, so that case
    is compared after sorting."""
    from bodo_amd.ops import gpu

    lt, rt, exp, kind = _join_tables(case, n_probe)
    ordered = case != "duplicate_build_key"
    if not ordered:
        exp = exp.sort_values(["lv", "rv"]).reset_index(drop=True)
    monkeypatch.setattr(gpu, "DENSE_JOIN", True)
    on = _joined(gpu, lt, rt, ordered)
    monkeypatch.setattr(gpu, "DENSE_JOIN", False)
    off = _joined(gpu, lt, rt, ordered)
    for what, got in (("on", on), ("off", off)):
        assert len(got) == len(exp), (what, len(got), len(exp))
        for c in ("lv", "rv", "w"):
            np.testing.assert_array_equal(
                got[c].to_numpy(), exp[c].to_numpy().astype(got[c].dtype),
                err_msg=str((what, c)))
        if kind != "date32" and len(exp):
            np.testing.assert_array_equal(
                got["k"].to_numpy().astype(np.int64),
                exp["k"].to_numpy().astype(np.int64), err_msg=what)
    if case in ("all_matched", "int32_probe_int64_build") and n_probe > 1:
        assert (len(exp) == n_probe) == (case == "all_matched")
    if case in ("some_unmatched", "int64_low_end") and n_probe > 1:
        assert 0 < len(exp) < n_probe


@pytest.mark.parametrize("case", ["some_unmatched", "int64_low_end",
                                  "int64_high_end", "masked_probe"])
def test_join_probe_dense_kernel(case):
    """The probe kernel alone against a dictionary lookup in python:
    out_build row by row, and the miss count."""
    from bodo_amd.ops import gpu

    n_probe = 70001
    bk, pk, valid, _ = _join_inputs(case, n_probe)
    lo, span = int(bk.min()), int(bk.max()) - int(bk.min()) + 1
    lut = np.full(span, -1, dtype=np.int32)
    lut[(bk.astype(object) - lo).astype(np.int64)] = np.arange(len(bk))
    row_of = {int(k): r for r, k in enumerate(bk.tolist())}
    ok = np.ones(n_probe, dtype=bool) if valid is None else valid
    exp = np.array([row_of.get(int(k), -1) if v else -1
                    for k, v in zip(pk.tolist(), ok.tolist())], dtype=np.int64)
    out_build, misses = gpu.kernels().join_probe_dense(
        torch.from_numpy(pk).cuda(),
        None if valid is None else torch.from_numpy(valid).cuda()
        .view(torch.uint8),
        R.INT64, n_probe, torch.from_numpy(lut).cuda(), lo)
    np.testing.assert_array_equal(out_build.cpu().numpy(), exp)
    assert int(misses.item()) == int((exp < 0).sum())
