"""The oracle of ``test_gpu_hash_kernels.py`` checked against pandas, on the
very inputs the GPU tests use.  Needs no GPU."""

import numpy as np
import pandas as pd
import pytest

from tests import relational_cases as C
from tests import relational_ref as R


def _value_series(case):
    """The case's values as pandas sees them: NA where the kernel contract
    says invalid."""
    iv, dv, _ = R.load_values(case["data"], case["kind"])
    ok = R.valid_rows(case["data"], case["mask"], case["kind"])
    if case["kind"] in (R.FLOAT32, R.FLOAT64):
        return pd.Series(np.where(ok, dv, np.nan)), ok
    return pd.Series(pd.arrays.IntegerArray(iv, ~ok)), ok


def _check_agg_vs_pandas(case, ops):
    ngroups = case["ngroups"]
    vals, ok = _value_series(case)
    is_float = case["kind"] in (R.FLOAT32, R.FLOAT64)
    df = pd.DataFrame({"g": case["row_gid"].astype(np.int64), "v": vals,
                       "r": np.arange(len(vals))})
    gb = df.groupby("g")["v"]
    valid_r = df[ok].groupby("g")["r"]
    groups = np.arange(ngroups)
    exp_count = gb.count().reindex(groups, fill_value=0).to_numpy(np.int64)
    exp_size = gb.size().reindex(groups, fill_value=0).to_numpy(np.int64)
    has = exp_count > 0
    for op in ops:
        acc, cnt = R.ref_agg(case["data"], case["mask"], case["kind"],
                             case["row_gid"], ngroups, op)
        if op == "size":
            np.testing.assert_array_equal(cnt, exp_size)
            continue
        np.testing.assert_array_equal(cnt, exp_count, err_msg=op)
        init_f, init_i = R.AGG_INIT[op]
        init = init_f if op in R.F64_OPS else init_i
        assert (acc[~has] == init).all(), op
        if op == "count":
            continue
        if op in ("first_row", "last_row"):
            exp = (valid_r.min() if op == "first_row" else valid_r.max())
        else:
            fn = op.split("_")[0]
            exp = gb.sum(min_count=1) if fn == "sum" else getattr(gb, fn)()
        exp = exp.reindex(groups)[has]
        if op in R.F64_OPS:
            if not is_float:
                # pandas reduces integers exactly; the f64 ops see doubles
                _, dv, _ = R.load_values(case["data"], case["kind"])
                fl = pd.Series(np.where(ok, dv, np.nan)).groupby(df["g"])
                fn = op.split("_")[0]
                exp = (fl.sum(min_count=1) if fn == "sum"
                       else getattr(fl, fn)()).reindex(groups)[has]
            np.testing.assert_array_equal(
                acc[has], exp.to_numpy(np.float64), err_msg=op)
        else:
            np.testing.assert_array_equal(
                acc[has], exp.to_numpy(np.int64), err_msg=op)


@pytest.mark.parametrize("ngroups", C.AGG_NGROUPS)
@pytest.mark.parametrize("type_name", C.AGG_TYPES)
def test_ref_agg_vs_pandas(type_name, ngroups):
    for variant in C.agg_variants_for(type_name):
        case = C.agg_case(type_name, ngroups, variant)
        _check_agg_vs_pandas(case, C.agg_ops_for(type_name))


def test_ref_agg_layout_has_empty_and_all_null_groups():
    case = C.agg_case("float64", 2049, "nan")
    _, cnt = R.ref_agg(case["data"], None, case["kind"], case["row_gid"],
                       2049, "count")
    _, size = R.ref_agg(case["data"], None, case["kind"], case["row_gid"],
                        2049, "size")
    assert (size == 0).any()                 # groups without any row
    assert ((size > 0) & (cnt == 0)).any()   # groups whose rows are all null
    assert (cnt > 1).any()


def test_ref_agg_skew_vs_pandas():
    case = C.agg_case("float64", 7, "masked", skew=True)
    assert (case["row_gid"] == 0).mean() > 0.85
    _check_agg_vs_pandas(case, C.agg_ops_for("float64"))
    case = C.agg_case("int32", 7, "masked", skew=True)
    _check_agg_vs_pandas(case, C.agg_ops_for("int32"))


def test_ref_agg_int_edges_vs_pandas():
    for name, (case, op) in C.agg_int_edge_cases().items():
        _check_agg_vs_pandas(case, (op,))
    case, op = C.agg_int_edge_cases()["sum_wraps"]
    acc, _ = R.ref_agg(case["data"], None, case["kind"], case["row_gid"],
                       case["ngroups"], op)
    exact = [int(case["data"][case["row_gid"] == g].astype(object).sum())
             for g in range(case["ngroups"])]
    assert any(abs(e) >= 2**63 for e in exact), "the case must overflow"
    with np.errstate(over="ignore"):
        wrapped = np.array([case["data"][case["row_gid"] == g].sum()
                            for g in range(case["ngroups"])])
    np.testing.assert_array_equal(acc, wrapped)


def test_ref_agg_freeform_sum_within_its_own_bound():
    """pandas' compensated sum must sit inside the bound the GPU test
    allows the atomics, and the bound must be tight enough to notice one
    dropped row."""
    case = C.agg_freeform_case()
    acc, cnt = R.ref_agg(case["data"], None, case["kind"], case["row_gid"],
                         case["ngroups"], "sum_f64")
    bound = R.ref_sum_bound(case["data"], None, case["kind"],
                            case["row_gid"], case["ngroups"])
    exp = pd.Series(case["data"]).groupby(case["row_gid"]).sum() \
        .reindex(np.arange(case["ngroups"]), fill_value=0.0).to_numpy()
    assert (np.abs(acc - exp) <= bound).all()
    smallest = np.abs(case["data"]).min()
    assert bound.max() < smallest, (bound.max(), smallest)


def test_ref_agg_prod_vs_pandas():
    case = C.agg_prod_case()
    acc, cnt = R.ref_agg(case["data"], case["mask"], case["kind"],
                         case["row_gid"], case["ngroups"], "prod_f64")
    vals, ok = _value_series(case)
    gb = vals.groupby(case["row_gid"].astype(np.int64))
    exp = gb.prod().reindex(np.arange(case["ngroups"]), fill_value=1.0)
    np.testing.assert_array_equal(acc, exp.to_numpy())
    np.testing.assert_array_equal(
        cnt, gb.count().reindex(np.arange(case["ngroups"]), fill_value=0))


def test_ref_fused_inputs_share_the_layout():
    for launch in C.FUSED_LAUNCHES:
        gid, aggs = C.fused_case(launch)
        assert 1 <= len(aggs) <= 4
        for case, op, want in aggs:
            assert case["row_gid"] is gid
            if op != "size":
                _check_agg_vs_pandas(case, (op,))


_FUSED_OPS = {"sum_f64", "sum_i64", "count", "min_f64", "max_f64", "min_i64",
              "max_i64", "size"}
# loader branches of the fused kernels, by storage type
_FUSED_TYPES = {"int8", "int16", "int32", "uint8", "bool", "float32",
                "float64", "timestamp"}


@pytest.mark.parametrize("is_global", [False, True], ids=["lds", "global"])
def test_fused_launches_cover_each_kernel_on_their_own(is_global):
    """Each of the two fused kernels must meet every op, every loader
    branch, NaN-as-null, masks, the dummy ``size`` tensor and both values
    of want_count in the launches that reach it."""
    launches = [la for la in C.FUSED_LAUNCHES
                if C.fused_is_global(la) == is_global]
    specs = [sp for la in launches for sp in C.fused_specs(la)]
    assert {op for _, _, op, _ in specs} == _FUSED_OPS
    assert {t for t, _, _, _ in specs if t} >= _FUSED_TYPES
    assert {len(la[1]) for la in launches} >= ({1, 4} if is_global
                                               else {1, 2, 3, 4})
    variants = {(t, v) for t, v, _, _ in specs}
    for need in (("float32", "nan"), ("float64", "nan"),
                 ("float32", "masked"), ("float64", "masked"),
                 ("float64", "plain"), (None, None)):
        assert need in variants, need
    assert {w for _, _, o, w in specs if o not in ("size", "count")} \
        == {0, 1}
    # float min and max each with and without their own count
    for op in ("min_f64", "max_f64"):
        assert {w for _, _, o, w in specs if o == op} == {0, 1}, op


def test_fused_launches_straddle_the_lds_limit():
    shapes = {(len(idx), ng): C.fused_is_global((ng, idx))
              for ng, idx in C.FUSED_LAUNCHES}
    assert shapes[(4, 768)] is False and shapes[(4, 769)] is True
    assert shapes[(1, 3072)] is False and shapes[(1, 3073)] is True
    by_shape = {(len(idx), ng): idx for ng, idx in C.FUSED_LAUNCHES
                if (len(idx), ng) != (1, 3073) or idx == (3,)}
    # the same aggregates on both sides of each limit
    assert by_shape[(4, 768)] == by_shape[(4, 769)]
    assert by_shape[(1, 3072)] == by_shape[(1, 3073)]
    assert {len(idx) for _, idx in C.FUSED_LAUNCHES} == {1, 2, 3, 4}


# ----------------------------------------------------------------------
# partition
# ----------------------------------------------------------------------

def _check_partition(cols):
    labels = R.ref_partition(cols)
    df = C.key_frame(cols)
    exp = df.groupby(list(df.columns), dropna=False, sort=False).ngroup()
    np.testing.assert_array_equal(labels, exp.to_numpy())
    first = df.drop_duplicates(keep="first").index.to_numpy()
    got_first = np.array([np.nonzero(labels == g)[0][0]
                          for g in range(labels.max() + 1)])
    np.testing.assert_array_equal(got_first, first)


@pytest.mark.parametrize("collide", [False, True])
@pytest.mark.parametrize("name", sorted(C.KEY_LAYOUTS))
def test_ref_partition_vs_pandas(name, collide):
    cols = C.build_key_case(name, collide)
    _check_partition(cols)
    ngroups = int(R.ref_partition(cols).max()) + 1
    assert ngroups > 8
    if collide:
        assert ngroups <= 50 and len(R.row_keys(cols)) <= 4000


def test_ref_partition_float_and_null_rules():
    nan2 = np.array([0x7FF8000000000000, 0xFFF8000000000123],
                    dtype=np.uint64).view(np.float64)
    f = C.KeyCol(np.array([0.0, -0.0, nan2[0], nan2[1], 1.0]), None, None,
                 R.FLOAT64)
    assert R.ref_partition([f]).tolist() == [0, 0, 1, 1, 2]
    m = C.KeyCol(np.array([5, 6, 7, 5], dtype=np.int32),
                 np.array([0, 0, 1, 1], dtype=np.uint8), None, R.INT32)
    assert R.ref_partition([m]).tolist() == [0, 0, 1, 2]
    s = C.string_col([b"", b"a", b"ab", b"a", b""])
    assert R.ref_partition([s]).tolist() == [0, 1, 2, 1, 0]


def test_ref_partition_packed_and_chunk_inputs_vs_pandas():
    for keys in C.packed_key_cases().values():
        assert keys.min() >= 0  # below 2^63: never the all-ones sentinel
        _check_partition([C.KeyCol(keys, None, None, R.INT64)])
    assert C.packed_key_cases()["int64_max"].max() == R.I64_MAX
    assert int(C.packed_key_cases()["three_columns_63_bits"].max()) \
        .bit_length() == 63
    cc = C.chunk_cases()
    for name, (keys, chunk_rows, cap) in cc.items():
        labels = R.ref_partition([C.KeyCol(keys, None, None, R.INT64)])
        assert labels.max() + 1 == pd.Series(keys).nunique()
    keys, chunk_rows, cap = cc["A_grow"]
    assert len(np.unique(keys)) == len(keys) and chunk_rows * 4 == cap
    keys, chunk_rows, cap = cc["B_later_chunks"]
    assert len(np.unique(keys)) == 10
    # a group whose first row lies in a later chunk
    first = pd.Series(keys).drop_duplicates().index.to_numpy()
    assert first.max() >= chunk_rows
    assert cc["C_chunk_above_cap"][1] > cc["C_chunk_above_cap"][2]


# ----------------------------------------------------------------------
# join
# ----------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.join_cases()))
def test_ref_join_vs_pandas(name):
    build, probe = C.join_cases()[name]
    bdf = C.key_frame(build)
    pdf = C.key_frame(probe)
    on = list(bdf.columns)
    bdf["b"] = np.arange(len(bdf))
    pdf["p"] = np.arange(len(pdf))
    inner = pdf.merge(bdf, on=on, how="inner")
    left = pdf.merge(bdf, on=on, how="left")
    exp_inner = sorted(zip(inner["p"], inner["b"]))
    exp_left = sorted(zip(left["p"], left["b"].fillna(-1).astype(np.int64)))
    exp_matched = set(inner["b"])
    hit = set(inner["p"])

    pairs, matched = R.ref_join_pairs(build, probe, 0)
    assert sorted(pairs.elements()) == exp_inner
    assert matched == exp_matched
    pairs, matched = R.ref_join_pairs(build, probe, 1)
    assert sorted(pairs.elements()) == exp_left
    assert matched == exp_matched
    pairs, _ = R.ref_join_pairs(build, probe, 2)
    assert sorted(p for p, _ in pairs.elements()) == sorted(hit)
    pairs, _ = R.ref_join_pairs(build, probe, 3)
    assert sorted(p for p, _ in pairs.elements()) == \
        sorted(set(range(len(pdf))) - hit)


def test_join_inputs_cover_what_they_claim():
    cases = C.join_cases()
    build, probe = cases["many_to_many"]
    dup = pd.Series(build[0].data).value_counts()
    assert dup.max() == 3000 and dup.min() == 1 and (dup == 50).any()
    assert (probe[0].data == 9999).sum() == 10
    pairs, matched = R.ref_join_pairs(*cases["no_match"], 0)
    assert not pairs and not matched
    for name in ("masked_both", "constant_hash"):
        build, probe = cases[name]
        bk, pk = set(R.row_keys(build)), set(R.row_keys(probe))
        both_null = [k for k in bk & pk if any(v is None for v in k)]
        assert both_null, name  # null keys that do meet across the sides
    build, probe = cases["float64_nan"]
    assert ("nan",) in set(R.row_keys(build)) & set(R.row_keys(probe))
    assert len(cases["constant_hash"][0][0].data) <= 2000
    assert len(R.row_keys(cases["empty_build"][0])) == 0
    assert len(R.row_keys(cases["empty_probe"][1])) == 0
