"""Differential tests of the groupby and join hash kernels in
``csrc/kernels.hip``: each pybind entry point is called directly and compared
with the plain references in ``relational_ref`` (themselves checked against
pandas in ``test_relational_ref.py``, on the same inputs).

The sizes pick the kernel, nothing here asserts which one ran:
``agg_update`` switches from the LDS to the global kernel above 2048 groups,
``agg_update_fused`` above ``n_aggs * ngroups * 16 B == 48 KiB``.
"""

import datetime
from collections import Counter
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import torch

from tests import relational_cases as C
from tests import relational_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _cuda_required():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _K():
    from bodo_amd.ops import gpu

    return gpu.kernels()


def _dev(a):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_bits_equal(got, exp, what):
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype, (what, got.dtype, exp.dtype)
    bad = np.nonzero(_bits(got) != _bits(exp))[0]
    assert len(bad) == 0, (what, "groups", bad[:8].tolist(),
                           "got", got[bad[:8]].tolist(),
                           "expected", exp[bad[:8]].tolist())


# ----------------------------------------------------------------------
# agg_update
# ----------------------------------------------------------------------

def _run_agg(case, op, want_count=True, row_gid=None):
    init_f, init_i = R.AGG_INIT[op]
    gid = _dev(case["row_gid"]) if row_gid is None else row_gid
    return _K().agg_update(_dev(case["data"]), _dev(case["mask"]), None,
                           case["kind"], gid, case["ngroups"], R.AGG_OPS[op],
                           init_f, init_i, want_count)


def _check_agg(case, op, want_count=True, what=""):
    res = _run_agg(case, op, want_count)
    acc, cnt = R.ref_agg(case["data"], case["mask"], case["kind"],
                         case["row_gid"], case["ngroups"], op)
    if op not in ("size", "count"):
        _assert_bits_equal(res[0], acc, (what, op, "acc"))
    if want_count or op in ("size", "count"):
        assert len(res) == 2, (what, op)
        _assert_bits_equal(res[1], cnt, (what, op, "cnt"))
    else:
        assert len(res) == 1, (what, op)


@pytest.mark.parametrize("ngroups", C.AGG_NGROUPS)
@pytest.mark.parametrize("type_name", C.AGG_TYPES)
def test_agg_update_matches_reference(type_name, ngroups):
    """Every op and storage type, bit for bit: the float inputs are
    k / 1024, so every partial sum is exact and the order of the atomics
    cannot matter."""
    for variant in C.agg_variants_for(type_name):
        case = C.agg_case(type_name, ngroups, variant)
        for op in C.agg_ops_for(type_name):
            _check_agg(case, op, want_count=(variant != "plain"),
                       what=(type_name, ngroups, variant))


@pytest.mark.parametrize("type_name", ["float64", "int32"])
def test_agg_update_skewed_group(type_name):
    """90 % of the rows in one group: a single LDS slot takes the load."""
    case = C.agg_case(type_name, 7, "masked", skew=True)
    for op in C.agg_ops_for(type_name):
        _check_agg(case, op, what=("skew", type_name))


@pytest.mark.parametrize("ngroups", [2048, 2049])
def test_agg_update_last_group_at_the_switch(ngroups):
    """Rows in the very last group on both sides of the LDS limit."""
    case = C.agg_case("int64", ngroups, "masked")
    case["row_gid"][::3] = ngroups - 1
    for op in ("sum_i64", "min_i64", "max_i64", "count", "size", "sum_f64",
               "first_row", "last_row"):
        _check_agg(case, op, what=("last group", ngroups))


def test_agg_update_freeform_float_sum():
    """Uniform values in [-1e6, 1e6]: |got - fsum| <= 2 (n_g - 1) 2^-53
    sum|x_i| per group, the bound taken from the reference alone."""
    case = C.agg_freeform_case()
    res = _run_agg(case, "sum_f64")
    acc, cnt = R.ref_agg(case["data"], None, case["kind"], case["row_gid"],
                         case["ngroups"], "sum_f64")
    bound = R.ref_sum_bound(case["data"], None, case["kind"],
                            case["row_gid"], case["ngroups"])
    got = res[0].cpu().numpy()
    err = np.abs(got - acc)
    print("freeform sum: max err", err.max(), "max bound", bound.max())
    assert (err <= bound).all(), (err.max(), bound.max())
    _assert_bits_equal(res[1], cnt, "freeform cnt")


def test_agg_update_prod():
    case = C.agg_prod_case()
    _check_agg(case, "prod_f64", what="prod")


@pytest.mark.parametrize("name", sorted(C.agg_int_edge_cases()))
def test_agg_update_integer_edges(name):
    case, op = C.agg_int_edge_cases()[name]
    _check_agg(case, op, what=name)


# ----------------------------------------------------------------------
# agg_update_fused
# ----------------------------------------------------------------------

@pytest.mark.parametrize("launch", C.FUSED_LAUNCHES, ids=C.fused_launch_id)
def test_agg_update_fused_matches_reference_and_agg_update(launch):
    """The launches below and above the 48 KiB limit each cover every op,
    loader branch and want_count value on their own, so the LDS and the
    global fused kernel are both pinned op by op."""
    gid_np, aggs = C.fused_case(launch)
    n_aggs, ngroups = len(aggs), launch[0]
    gid = _dev(gid_np)
    datas = [_dev(c["data"]) for c, _, _ in aggs]
    masks = [_dev(c["mask"]) for c, _, _ in aggs]
    dtypes = [c["kind"] for c, _, _ in aggs]
    ops = [R.AGG_OPS[op] for _, op, _ in aggs]
    init_fs = [R.AGG_INIT[op][0] for _, op, _ in aggs]
    init_is = [R.AGG_INIT[op][1] for _, op, _ in aggs]
    wants = [w for _, _, w in aggs]
    flat = _K().agg_update_fused(datas, masks, dtypes, ops, init_fs, init_is,
                                 wants, gid, ngroups)
    assert len(flat) == 2 * n_aggs
    for k, (case, op, want) in enumerate(aggs):
        what = ("fused", n_aggs, ngroups, k, op)
        acc, cnt = flat[2 * k], flat[2 * k + 1]
        if op == "size":
            # the reference of ``size`` only reads row_gid
            racc, rcnt = R.ref_agg(None, None, R.INT8, gid_np, ngroups, op)
            single = _K().agg_update(
                torch.zeros(len(gid_np), dtype=torch.int8, device="cuda"),
                None, None, R.INT8, gid, ngroups, R.AGG_OPS[op], 0.0, 0,
                True)
        else:
            racc, rcnt = R.ref_agg(case["data"], case["mask"], case["kind"],
                                   gid_np, ngroups, op)
            single = _run_agg(case, op, True, row_gid=gid)
        if op not in ("size", "count"):
            _assert_bits_equal(acc, racc, what + ("acc",))
            assert torch.equal(acc.view(torch.int64),
                               single[0].view(torch.int64)), what
        if want or op in ("size", "count"):
            _assert_bits_equal(cnt, rcnt, what + ("cnt",))
            assert torch.equal(cnt, single[1]), what
        else:
            assert cnt.numel() == 0, what


# ----------------------------------------------------------------------
# +-inf, -0.0 and unsigned columns through groupby_local
# ----------------------------------------------------------------------

def _inf_frame():
    inf = np.inf
    groups = {
        0: [inf, inf, inf],                # all +inf
        1: [-inf, -inf],                   # all -inf
        2: [inf, -inf, 1.5, -2.0],         # both, with finite values
        3: [np.nan, np.nan],               # all NaN
        4: [-0.0, 0.0, -0.0],
        5: [inf, 3.0, np.nan],
        6: [-inf, -3.0],
        7: [1.0, 2.0, 4.0],
    }
    k = np.concatenate([[g] * len(v) for g, v in groups.items()])
    v = np.concatenate(list(groups.values()))
    # many copies (shuffled) so more than one block takes part
    rng = np.random.default_rng(61)
    order = rng.permutation(len(k) * 300)
    return pd.DataFrame({"k": np.tile(k, 300)[order].astype(np.int64),
                         "v": np.tile(v, 300)[order]})


_INF_FUNCS = ("min", "max", "sum", "mean")


def _sorted(df, by):
    return df.sort_values(by).reset_index(drop=True)


def test_groupby_local_inf_fused_path():
    from bodo_amd.core.table import Table
    from bodo_amd.ops import gpu

    df = _inf_frame()
    t = Table.from_pandas(df, device="cuda")
    got = gpu.groupby_local(t, ["k"], [(f, "v", f) for f in _INF_FUNCS]) \
        .to_pandas()
    exp = df.groupby("k").agg(**{f: ("v", f) for f in _INF_FUNCS}) \
        .reset_index()
    pd.testing.assert_frame_equal(_sorted(got, "k"), exp, check_dtype=False,
                                  check_exact=True)


def test_groupby_local_inf_agg_one_path():
    """``first`` in the list sends only itself through ``_agg_one``; call
    it directly for min/max/sum/mean as well."""
    from bodo_amd.core.table import Table
    from bodo_amd.ops import gpu

    df = _inf_frame()
    t = Table.from_pandas(df, device="cuda")
    row_gid, uniq_rows = gpu.groupby_build([t.column("k")])
    ngroups = int(uniq_rows.numel())
    keys = t.column("k").data[uniq_rows].cpu().numpy()
    exp = df.groupby("k").agg(**{f: ("v", f) for f in _INF_FUNCS})
    for f in _INF_FUNCS:
        col = gpu._agg_one(t.column("v"), row_gid, ngroups, f, uniq_rows, t)
        got = pd.Series(col.data.cpu().numpy(), index=keys).sort_index()
        np.testing.assert_array_equal(got.to_numpy(), exp[f].to_numpy(),
                                      err_msg=f)
    mixed = [("fi", "v", "first")] + [(f, "v", f) for f in ("min", "max")]
    got = gpu.groupby_local(t, ["k"], mixed).to_pandas()
    got = _sorted(got, "k")
    np.testing.assert_array_equal(got["min"].to_numpy(),
                                  exp["min"].to_numpy())
    np.testing.assert_array_equal(got["max"].to_numpy(),
                                  exp["max"].to_numpy())


def _unsigned_frame():
    rng = np.random.default_rng(62)
    n = 6007
    u16 = rng.integers(0, 2**16, n).astype(np.uint16)
    u32 = rng.integers(0, 2**32, n).astype(np.uint32)
    k = rng.integers(0, 40, n).astype(np.int64)
    # groups wholly below, wholly above and across 2^15 / 2^31
    u16[k == 0] = u16[k == 0] % 2**15
    u16[k == 1] = u16[k == 1] | 2**15
    u32[k == 0] = u32[k == 0] % 2**31
    u32[k == 1] = u32[k == 1] | 2**31
    return pd.DataFrame({"k": k, "u16": u16, "u32": u32})


def test_groupby_local_unsigned_vs_pandas():
    from bodo_amd.core.table import Table
    from bodo_amd.ops import gpu

    df = _unsigned_frame()
    t = Table.from_pandas(df, device="cuda")
    exp_all = df.groupby("k").agg(
        **{f"{c}_{f}": (c, f) for c in ("u16", "u32")
           for f in ("sum", "min", "max")}).reset_index()
    for c in ("u16", "u32"):
        names = [f"{c}_{f}" for f in ("sum", "min", "max")]
        aggs = [(f"{c}_{f}", c, f) for f in ("sum", "min", "max")]
        got = _sorted(gpu.groupby_local(t, ["k"], aggs).to_pandas(), "k")
        for name in names:
            np.testing.assert_array_equal(
                got[name].to_numpy().astype(np.int64),
                exp_all[name].to_numpy().astype(np.int64), err_msg=name)
        # the same three through _agg_one
        row_gid, uniq_rows = gpu.groupby_build([t.column("k")])
        ngroups = int(uniq_rows.numel())
        keys = t.column("k").data[uniq_rows].cpu().numpy()
        for f in ("sum", "min", "max"):
            col = gpu._agg_one(t.column(c), row_gid, ngroups, f, uniq_rows, t)
            vals = col.to_pandas().to_numpy().astype(np.int64)
            got1 = pd.Series(vals, index=keys).sort_index()
            np.testing.assert_array_equal(
                got1.to_numpy(),
                exp_all[f"{c}_{f}"].to_numpy().astype(np.int64),
                err_msg=f"_agg_one {c} {f}")


_FINISH_COLS = ("i32", "i64", "ts", "d32", "b", "f64")


def _finisher_frame():
    """257 rows in 5 groups, one column per branch of the min/max
    finishers: masked int32 and float64 with NaN (group 3 all null in
    both), unmasked int64, timestamp, date32 and bool."""
    rng = np.random.default_rng(63)
    n = 257
    k = rng.integers(0, 5, n).astype(np.int64)
    k[:5] = np.arange(5)
    null = k == 3
    i32 = pd.array(rng.integers(-1000, 1000, n).astype(np.int32),
                   dtype="Int32")
    i32[null | (rng.random(n) < 0.2)] = pd.NA
    f64 = rng.integers(-4096, 4096, n) / 1024.0
    f64[null | (rng.random(n) < 0.2)] = np.nan
    day0 = datetime.date(2020, 1, 1)
    b = rng.random(n) < 0.5
    b[k == 1] = True
    b[k == 2] = False
    return pd.DataFrame({
        "k": k, "i32": i32,
        "i64": rng.integers(-2**40, 2**40, n).astype(np.int64),
        "ts": pd.to_datetime(rng.integers(0, 2**60, n)),
        "d32": [day0 + datetime.timedelta(days=int(d))
                for d in rng.integers(-4000, 4000, n)],
        "b": b, "f64": f64,
    })


def test_groupby_minmax_finishers_fused_and_agg_one():
    """min and max of every finisher branch through the fused path and
    through ``_agg_one``: the two agree exactly in value and type, and both
    match pandas (min/max do not depend on the order of the atomics)."""
    from bodo_amd.core.table import Table
    from bodo_amd.core.types import TypeKind
    from bodo_amd.ops import gpu

    df = _finisher_frame()
    t = Table.from_pandas(df, device="cuda")
    assert t.column("i32").mask is not None and t.column("i64").mask is None
    assert t.column("d32").dtype.kind == TypeKind.DATE32
    aggs = [(f"{c}_{f}", c, f) for c in _FINISH_COLS for f in ("min", "max")]
    exp = df.groupby("k").agg(**{o: (c, f) for o, c, f in aggs}).reset_index()
    assert exp.loc[3, ["i32_min", "f64_max"]].isna().all()
    for o in ("i32_min", "i32_max"):  # a masked column comes back as float64
        exp[o] = exp[o].astype("float64")

    fused = gpu.groupby_local(t, ["k"], aggs)
    row_gid, uniq_rows = gpu.groupby_build([t.column("k")])
    ngroups = int(uniq_rows.numel())
    one = Table(["k"] + [o for o, _, _ in aggs],
                [gpu._gather_any(t.column("k"), uniq_rows)] +
                [gpu._agg_one(t.column(c), row_gid, ngroups, f, uniq_rows, t)
                 for _, c, f in aggs], ngroups)
    for o, _, _ in aggs:
        a, b = fused.column(o), one.column(o)
        assert a.dtype == b.dtype and a.data.dtype == b.data.dtype, o
        assert (a.mask is None) and (b.mask is None), o
        _assert_bits_equal(a.data, b.data.cpu().numpy(), o)
    for got in (fused, one):
        pd.testing.assert_frame_equal(_sorted(got.to_pandas(), "k"), exp,
                                      check_dtype=False, check_exact=True)


_MOMENTS = ("var", "std", "sem", "skew", "kurt")


def _moments_table():
    """257 rows in 6 groups: group 0 has no valid value in either column,
    groups 1 and 2 have exactly 3 and 4, groups 3..5 about 80 rows with a
    fifth of them null.  f is float64 with NaNs, i a masked int32; the
    floats are integers over 8, so every power sum up to the fourth is
    exact and the order of the atomics cannot matter."""
    from bodo_amd.core.column import Column
    from bodo_amd.core.table import Table

    rng = np.random.default_rng(64)
    n = 257
    k = np.concatenate([np.zeros(5), np.full(6, 1), np.full(6, 2),
                        rng.integers(3, 6, n - 17)]).astype(np.int64)
    null = rng.random(n) < 0.2
    null[k == 0] = True
    for g, valid in ((1, 3), (2, 4)):
        rows = np.nonzero(k == g)[0]
        null[rows[:valid]] = False
        null[rows[valid:]] = True
    order = rng.permutation(n)
    k, null = k[order], null[order]
    f = rng.integers(-64, 64, n) / 8.0
    f[null] = np.nan
    i = rng.integers(-50, 50, n).astype(np.int32)
    df = pd.DataFrame({"k": k, "f": f, "i": pd.array(i, dtype="Int32")})
    df.loc[null, "i"] = pd.NA
    cols = [Column.from_numpy(k), Column.from_numpy(f),
            Column.from_numpy(i, mask=~null)]
    return df, Table(["k", "f", "i"], cols, n)


def test_groupby_local_moments_vs_pandas():
    """var, std, sem, skew and kurt through the kernels (no aggregate in
    the request sends the groupby elsewhere), against pandas at 1e-9."""
    from bodo_amd.ops import gpu

    df, t = _moments_table()
    aggs = [(f"{c}_{f}", c, f) for c in ("f", "i") for f in _MOMENTS]
    got = _sorted(gpu.groupby_local(t.to_device("cuda"), ["k"], aggs)
                  .to_pandas(), "k")
    exp = df.groupby("k").agg(**{
        o: (c, (lambda x: x.kurt()) if f == "kurt" else f)
        for o, c, f in aggs}).reset_index()
    assert df.groupby("k")["f"].count().tolist()[:3] == [0, 3, 4]
    assert exp.loc[1, "f_kurt"] != exp.loc[1, "f_kurt"]      # 3 values: NaN
    assert exp.loc[2, "i_kurt"] == exp.loc[2, "i_kurt"]      # 4: a number
    for o, _, _ in aggs:
        g = got[o].to_numpy(dtype=np.float64, na_value=np.nan)
        e = exp[o].to_numpy(dtype=np.float64, na_value=np.nan)
        print(o, "max abs diff", np.nanmax(np.abs(g - e)))
        np.testing.assert_allclose(g, e, rtol=1e-9, atol=0, equal_nan=True,
                                   err_msg=o)


@pytest.mark.parametrize("op", [8, 9, 10])
def test_agg_update_fused_rejects_unsupported_ops(op):
    """first_row, last_row and prod_f64 have no fused form: rejected on the
    host, before any launch."""
    gid = torch.arange(16, dtype=torch.int32, device="cuda") % 2
    data = torch.ones(16, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError):
        _K().agg_update_fused([data], [None], [R.FLOAT64], [op], [0.0], [0],
                              [1], gid, 2)


def test_hash_unsigned_matches_cpu():
    """CPU and GPU ranks share shuffles: unsigned columns must hash alike
    on both, whichever way the column was ingested."""
    from bodo_amd import ops
    from bodo_amd.core.column import Column
    from bodo_amd.core.table import Table

    df = _unsigned_frame()
    df["u8"] = (df["u16"] % 256).astype(np.uint8)
    df["u64"] = df["u32"].astype(np.uint64) << np.uint64(32)
    t = Table.from_pandas(df)
    for name in ("u8", "u16", "u32", "u64"):
        for c in (t.column(name), Column.from_numpy(df[name].to_numpy())):
            h_cpu = ops.hash_columns([c])
            h_gpu = ops.hash_columns([c.to_device("cuda")]).cpu()
            assert torch.equal(h_cpu, h_gpu), name
    a = ops.hash_columns([t.column("u16")])
    b = ops.hash_columns([Column.from_numpy(df["u16"].to_numpy())])
    assert torch.equal(a, b)


# ----------------------------------------------------------------------
# group build
# ----------------------------------------------------------------------

def _fnv(b):
    h = 0xcbf29ce484222325
    for ch in b:
        h = ((h ^ ch) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _key_args(cols):
    datas, masks, offsets, auxs, dtypes = [], [], [], [], []
    for c in cols:
        datas.append(_dev(c.data))
        masks.append(_dev(c.mask))
        offsets.append(_dev(c.offsets))
        aux = None
        if c.kind == R.DICT:
            lut = np.array([_fnv(v) for v in c.dictionary], dtype=np.uint64)
            aux = _dev(lut.view(np.int64))
        auxs.append(aux)
        dtypes.append(c.kind)
    return datas, masks, offsets, auxs, dtypes


def _n_rows(cols):
    c = cols[0]
    return len(c.offsets) - 1 if c.kind == R.STRING else len(c.data)


def _hashes(args, n):
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device="cuda")
    return _K().hash_columns(*args, n, 0)


def _check_build(row_gid, uniq_rows, exp_labels):
    got = row_gid.cpu().numpy().astype(np.int64)
    uniq = uniq_rows.cpu().numpy()
    ngroups = int(exp_labels.max()) + 1
    assert len(uniq) == ngroups, (len(uniq), ngroups)
    assert got.min() >= 0 and got.max() == ngroups - 1
    np.testing.assert_array_equal(R.canonical_labels(got), exp_labels)
    # one representative row per group, and it lies in its group
    assert ((uniq >= 0) & (uniq < len(got))).all()
    np.testing.assert_array_equal(got[uniq], np.arange(ngroups))


@pytest.mark.parametrize("name", sorted(C.KEY_LAYOUTS))
def test_groupby_build_matches_partition(name):
    cols = C.build_key_case(name)
    n = _n_rows(cols)
    args = _key_args(cols)
    row_gid, uniq_rows = _K().groupby_build(*args, n, _hashes(args, n))
    _check_build(row_gid, uniq_rows, R.ref_partition(cols))


@pytest.mark.parametrize("name", sorted(C.KEY_LAYOUTS))
def test_groupby_build_forced_collisions(name):
    """One constant hash for 4000 rows in about 50 groups: every row walks
    the same probe chain and only ``rows_eq`` tells the groups apart."""
    cols = C.build_key_case(name, collide=True)
    n = _n_rows(cols)
    args = _key_args(cols)
    const = torch.full((n,), 0x1234567, dtype=torch.int64, device="cuda")
    row_gid, uniq_rows = _K().groupby_build(*args, n, const)
    _check_build(row_gid, uniq_rows, R.ref_partition(cols))


@pytest.mark.parametrize("name", sorted(C.packed_key_cases()))
def test_groupby_build_packed_matches_partition(name):
    # keys stay below 2^63: the all-ones word marks an empty slot and the
    # packer, which stops at 63 bits, cannot produce it
    keys = C.packed_key_cases()[name]
    row_gid, uniq_rows = _K().groupby_build_packed(_dev(keys))
    _check_build(row_gid, uniq_rows,
                 R.ref_partition([C.KeyCol(keys, None, None, R.INT64)]))


@pytest.mark.parametrize("packed", [False, True], ids=["generic", "packed"])
@pytest.mark.parametrize("name", sorted(C.chunk_cases()))
def test_groupby_build_chunked_insert(name, packed):
    """Multi-chunk insert with a small table: growth and rebuild (A), groups
    first seen in a later chunk (B), chunk_rows above the capacity (C).
    Occupancy stays below the capacity in all three by construction."""
    keys, chunk_rows, max_cap = C.chunk_cases()[name]
    col = C.KeyCol(keys, None, None, R.INT64)
    if packed:
        row_gid, uniq_rows = _K().groupby_build_packed(
            _dev(keys), chunk_rows, max_cap)
    else:
        args = _key_args([col])
        row_gid, uniq_rows = _K().groupby_build(
            *args, len(keys), _hashes(args, len(keys)), chunk_rows, max_cap)
    _check_build(row_gid, uniq_rows, R.ref_partition([col]))
    # the defaults give the same partition
    if packed:
        d_gid, d_uniq = _K().groupby_build_packed(_dev(keys))
    else:
        d_gid, d_uniq = _K().groupby_build(
            *args, len(keys), _hashes(args, len(keys)))
    _check_build(d_gid, d_uniq, R.ref_partition([col]))


# ----------------------------------------------------------------------
# join_build + join_probe
# ----------------------------------------------------------------------

@lru_cache(maxsize=None)
def _join_cases():
    return C.join_cases()


@lru_cache(maxsize=None)
def _join_ref(name, how):
    build, probe = _join_cases()[name]
    return R.ref_join_pairs(build, probe, how)


@pytest.mark.parametrize("track", [False, True], ids=["notrack", "track"])
@pytest.mark.parametrize("how", [0, 1, 2, 3],
                         ids=["inner", "left", "semi", "anti"])
@pytest.mark.parametrize("name", sorted(C.join_cases()))
def test_join_probe_matches_reference(name, how, track):
    K = _K()
    build, probe = _join_cases()[name]
    n_build, n_probe = _n_rows(build), _n_rows(probe)
    bargs, pargs = _key_args(build), _key_args(probe)
    if name == "constant_hash":
        bh = torch.full((n_build,), 99, dtype=torch.int64, device="cuda")
        ph = torch.full((n_probe,), 99, dtype=torch.int64, device="cuda")
    else:
        bh, ph = _hashes(bargs, n_build), _hashes(pargs, n_probe)
    heads, nxt = K.join_build(bh, n_build)
    res = K.join_probe(*bargs, n_build, bh, *pargs, n_probe, ph, heads, nxt,
                       how, track)
    assert len(res) == (3 if track else 2)
    out_probe = res[0].cpu().numpy()
    out_build = res[1].cpu().numpy()
    exp_pairs, exp_matched = _join_ref(name, how)
    if how in (0, 1):
        assert len(out_build) == len(out_probe)
        got = Counter(zip(out_probe.tolist(), out_build.tolist()))
    else:
        assert len(out_build) == 0
        got = Counter((p, None) for p in out_probe.tolist())
    assert got == exp_pairs
    # per-probe-row counts.  That the output is ordered by probe row follows
    # from the count/prefix-sum/fill scheme; it is a fact of this
    # implementation that callers may not rely on, checked here only because
    # a violation today would mean wrong offsets.
    exp_counts = np.zeros(n_probe, dtype=np.int64)
    for (p, _), c in exp_pairs.items():
        exp_counts[p] += c
    np.testing.assert_array_equal(
        np.bincount(out_probe, minlength=n_probe)[:n_probe]
        if len(out_probe) else np.zeros(n_probe, dtype=np.int64), exp_counts)
    assert (np.diff(out_probe) >= 0).all()
    if how == 1:
        # -1 fill exactly for the probe rows without a match
        unmatched = {p for (p, b) in exp_pairs if b == -1}
        assert set(out_probe[out_build == -1].tolist()) == unmatched
    if track:
        flags = res[2].cpu().numpy()[:n_build]
        assert set(np.unique(flags).tolist()) <= {0, 1}
        # only the pair-producing joins mark build rows today; that semi
        # and anti leave the flags clear is how the kernel is written, not
        # a requirement (no caller tracks matches for them)
        exp = exp_matched if how in (0, 1) else set()
        assert set(np.nonzero(flags)[0].tolist()) == exp


def _join_frames(name):
    build, probe = _join_cases()[name]
    left = C.key_frame(probe)
    right = C.key_frame(build)
    on = list(left.columns)
    left["lv"] = np.arange(len(left), dtype=np.int64)
    right["rv"] = np.arange(len(right), dtype=np.int64)
    return left, right, on


def _check_join_local(join_local, name, how, device):
    from bodo_amd.core.table import Table

    left, right, on = _join_frames(name)
    lt = Table.from_pandas(left, device=device)
    rt = Table.from_pandas(right, device=device)
    got = join_local(lt, rt, on, on, how).to_pandas()
    exp = left.merge(right, on=on, how=how)
    assert sorted(got.columns) == sorted(exp.columns)
    got = got[list(exp.columns)]
    for c in on:
        if exp[c].dtype == object:
            got[c] = got[c].astype(object)
    by = ["lv", "rv"]
    got = got.sort_values(by, na_position="last").reset_index(drop=True)
    exp = exp.sort_values(by, na_position="last").reset_index(drop=True)
    pd.testing.assert_frame_equal(got, exp, check_dtype=False)


@pytest.mark.parametrize("how", ["inner", "left", "outer", "right"])
@pytest.mark.parametrize("name", ["many_to_many", "int64_string"])
def test_join_local_vs_pandas_merge(name, how):
    from bodo_amd.ops import gpu

    _check_join_local(gpu.join_local, name, how, "cuda")
