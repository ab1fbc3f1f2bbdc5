"""Host helpers of the in-place parquet decode: the incremental dictionary
unification must agree with ops.concat_columns, and val_range must come
out of the footer statistics exactly when every chunk has them."""

import datetime

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from bodo_amd import ops
from bodo_amd.core import types as bt
from bodo_amd.core.column import Column
from bodo_amd.io import parquet_gpu as g

DICT_LISTS = {
    "equal": [["a", "b", "c"], ["a", "b", "c"], ["a", "b", "c"]],
    "permuted": [["a", "b", "c"], ["c", "a", "b"], ["b", "c", "a"]],
    "growing": [["a"], ["a", "b"], ["a", "b", "c", "d"]],
    "shrinking": [["a", "b", "c"], ["a", "b"], ["a"]],
    "disjoint": [["a", "b"], ["c", "d"], ["e"]],
    "missing_one": [["x", "y", "z"], ["z", "x"], ["y", "w", "x", "z"]],
    "single": [["only", "one"]],
}


@pytest.mark.parametrize("case", sorted(DICT_LISTS))
def test_unifier_matches_concat_columns(case):
    dicts = DICT_LISTS[case]
    rng = np.random.default_rng(len(case))
    cols, codes = [], []
    for d in dicts:
        c = rng.integers(0, len(d), 37).astype(np.int32)
        codes.append(c)
        cols.append(Column(bt.dictionary, torch.from_numpy(c.copy()),
                           dictionary=pa.array(d, type=pa.large_string()),
                           length=len(c)))
    ref = ops.concat_columns(cols)

    u = g._DictUnifier()
    got = []
    for d, c in zip(dicts, codes):
        lut = u.add(np.array(d, dtype=object))
        if lut is None:
            # codes already unified: the dictionary so far starts with d,
            # or d starts with it
            k = min(len(d), len(u.values))
            assert u.values[:k] == d[:k]
            got.append(c)
        else:
            assert lut.dtype == np.int32 and len(lut) == len(d)
            got.append(lut[c])
    assert u.dictionary().to_pylist() == ref.dictionary.to_pylist()
    assert u.dictionary().type == pa.large_string()
    assert (np.concatenate(got) == ref.data.numpy()).all()


def test_unifier_identity_gets_no_table():
    u = g._DictUnifier()
    assert u.add(np.array(["a", "b"], dtype=object)) is None
    assert u.add(np.array(["a", "b", "c"], dtype=object)) is None
    assert u.add(np.array(["a"], dtype=object)) is None
    lut = u.add(np.array(["b", "a"], dtype=object))
    assert lut.tolist() == [1, 0]


def _chunk_metas(path, name):
    md = pq.ParquetFile(path).metadata
    out = []
    for r in range(md.num_row_groups):
        rg = md.row_group(r)
        for c in range(rg.num_columns):
            if rg.column(c).path_in_schema == name:
                out.append(rg.column(c))
    return out


def test_val_range_from_footer(tmp_path):
    rng = np.random.default_rng(5)
    n = 3000
    i64 = rng.integers(-500, 900, n).astype(np.int64)
    i32 = rng.integers(7, 266, n).astype(np.int32)
    nul = pa.array(rng.integers(10, 20, n), type=pa.int64(),
                   mask=rng.random(n) < 0.2)
    d32 = pa.array(rng.integers(19000, 19400, n).astype(np.int32),
                   type=pa.date32())
    tbl = pa.table({
        "i64": i64, "i32": i32, "nul": nul, "d32": d32,
        "f": rng.random(n),
        "ts": pa.array(rng.integers(0, 10**15, n), type=pa.timestamp("us")),
        "allnull": pa.array([None] * n, type=pa.int64()),
    })
    with_stats = str(tmp_path / "s.parquet")
    no_stats = str(tmp_path / "n.parquet")
    pq.write_table(tbl, with_stats, row_group_size=1000)
    pq.write_table(tbl, no_stats, row_group_size=1000,
                   write_statistics=False)
    sch = tbl.schema

    def vr(path, name):
        cms = _chunk_metas(path, name)
        assert len(cms) == 3
        return g._val_range_from_meta(cms, sch.field(name).type)

    assert vr(with_stats, "i64") == (int(i64.min()), int(i64.max()))
    assert vr(with_stats, "i32") == (int(i32.min()), int(i32.max()))
    valid = np.array(nul.is_valid())
    nv = np.array(nul.fill_null(15))[valid]
    assert vr(with_stats, "nul") == (int(nv.min()), int(nv.max()))
    days = np.array(d32.cast(pa.int32()))
    assert vr(with_stats, "d32") == (int(days.min()), int(days.max()))
    assert all(isinstance(v, int) for v in vr(with_stats, "d32"))
    # not integer columns, or a chunk without min/max
    assert vr(with_stats, "f") is None
    assert vr(with_stats, "ts") is None
    assert vr(with_stats, "allnull") is None
    for name in tbl.column_names:
        assert vr(no_stats, name) is None
    # one chunk without statistics spoils the column
    mixed = _chunk_metas(with_stats, "i64")[:2] + \
        _chunk_metas(no_stats, "i64")[2:]
    assert g._val_range_from_meta(mixed, pa.int64()) is None
    assert g._val_range_from_meta([], pa.int64()) is None


def test_stat_int():
    assert g._stat_int(5) == 5
    assert g._stat_int(np.int64(-3)) == -3
    assert g._stat_int(datetime.date(1970, 1, 11)) == 10
    assert g._stat_int(1.5) is None
    assert g._stat_int("a") is None


def test_direct_chunk_kind(tmp_path):
    rng = np.random.default_rng(6)
    n = 2000
    tbl = pa.table({
        "i64": rng.integers(0, 9, n),
        "nul": pa.array(rng.integers(0, 9, n), type=pa.int64(),
                        mask=rng.random(n) < 0.2),
        "s": pa.array(rng.choice(["a", "b"], n)),
        "num_dict": rng.integers(0, 9, n),
        "s_plain": pa.array([str(v) for v in range(n)]),
        "b": pa.array(rng.random(n) < 0.5),
        "cat": pa.DictionaryArray.from_arrays(
            pa.array(rng.integers(0, 3, n).astype(np.int32)),
            pa.array(["x", "y", "z"], type=pa.large_string())),
    })
    path = str(tmp_path / "k.parquet")
    pq.write_table(tbl, path, use_dictionary=["s", "num_dict", "cat"],
                   compression="SNAPPY")
    sch = pq.ParquetFile(path).schema_arrow
    kinds = {name: g._direct_chunk_kind(_chunk_metas(path, name)[0],
                                        sch.field(name))
             for name in tbl.column_names}
    assert kinds == {"i64": "plain", "nul": None, "s": "dict",
                     "num_dict": None, "s_plain": None, "b": None,
                     "cat": "dict"}
    nostat = str(tmp_path / "k2.parquet")
    pq.write_table(tbl, nostat, use_dictionary=["s"],
                   write_statistics=False)
    assert g._direct_chunk_kind(_chunk_metas(nostat, "i64")[0],
                                sch.field("i64")) is None
    required = pa.field("i64", pa.int64(), nullable=False)
    assert g._direct_chunk_kind(_chunk_metas(nostat, "i64")[0],
                                required) == "plain"
    gz = str(tmp_path / "k3.parquet")
    pq.write_table(tbl, gz, use_dictionary=["s"], compression="GZIP")
    assert g._direct_chunk_kind(_chunk_metas(gz, "i64")[0],
                                sch.field("i64")) is None
