"""Inputs shared by the GPU hash-kernel tests (``test_gpu_hash_kernels.py``)
and the CPU tests that verify their oracle (``test_relational_ref.py``).

Everything is numpy with fixed seeds.  Columns are handed out in the raw
storage form the kernels take (see ``relational_ref``).
"""

from collections import namedtuple

import numpy as np

from tests import relational_ref as R

# a key column as the kernels see it; ``dictionary`` (list of bytes) only for
# DICT columns, whose hash LUT is built from it
KeyCol = namedtuple("KeyCol", "data mask offsets kind dictionary",
                    defaults=(None,))

# ----------------------------------------------------------------------
# aggregate inputs
# ----------------------------------------------------------------------

AGG_NGROUPS = (1, 7, 2048, 2049, 5000)
AGG_ROWS = 20011  # odd, 79 blocks of 256
AGG_TYPES = ("int8", "int16", "int32", "int64", "uint8", "bool", "float32",
             "float64", "date32", "timestamp")
_KIND = {"int8": R.INT8, "int16": R.INT16, "int32": R.INT32,
         "int64": R.INT64, "uint8": R.UINT8, "bool": R.BOOL,
         "float32": R.FLOAT32, "float64": R.FLOAT64, "date32": R.DATE32,
         "timestamp": R.TIMESTAMP_NS}
_ALL_OPS = ("sum_f64", "sum_i64", "count", "min_f64", "max_f64", "min_i64",
            "max_i64", "size", "first_row", "last_row")
_FLOAT_OPS = ("sum_f64", "count", "min_f64", "max_f64", "size", "first_row",
              "last_row")


def agg_ops_for(type_name):
    if type_name in ("float32", "float64"):
        # the integer ops convert with (int64_t)f, which no host path uses
        return _FLOAT_OPS
    if type_name == "timestamp":
        # ns-since-epoch values are not exact in a double sum
        return tuple(o for o in _ALL_OPS if o != "sum_f64")
    return _ALL_OPS


def agg_variants_for(type_name):
    if type_name in ("float32", "float64"):
        return ("plain", "masked", "nan")
    return ("plain", "masked")


def _agg_values(type_name, n, rng):
    if type_name == "int8":
        return rng.integers(-128, 128, n).astype(np.int8)
    if type_name == "int16":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    if type_name == "int32":
        return rng.integers(-2**31, 2**31, n).astype(np.int32)
    if type_name == "int64":
        # |v| < 2^30 keeps every double partial sum of < 2^20 rows exact
        return rng.integers(-2**30, 2**30, n).astype(np.int64)
    if type_name == "uint8":
        return rng.integers(0, 256, n).astype(np.uint8)
    if type_name == "bool":
        return rng.integers(0, 2, n).astype(np.uint8)
    if type_name == "date32":
        return rng.integers(-20000, 20000, n).astype(np.int32)
    if type_name == "timestamp":
        return rng.integers(-2**60, 2**60, n).astype(np.int64)
    # floats: k / 1024 with |k| < 2^20, so any partial sum of < 2^20 rows is
    # exactly representable and the order of the atomics cannot matter
    k = rng.integers(-2**20 + 1, 2**20, n)
    dt = np.float32 if type_name == "float32" else np.float64
    return (k / 1024.0).astype(dt)


def agg_row_gid(ngroups, n, rng, skew=False):
    """Group ids that leave every group with g % 5 == 3 without any row."""
    live = np.array([g for g in range(ngroups) if g % 5 != 3 or ngroups < 5])
    gid = live[rng.integers(0, len(live), n)]
    if skew:
        gid[rng.random(n) < 0.9] = live[0]
    return gid.astype(np.int32)


def agg_case(type_name, ngroups, variant, n=AGG_ROWS, skew=False, seed=0):
    """One aggregate input: dict(data, mask, kind, row_gid, ngroups).

    ``masked`` and ``nan`` make every row of the groups with g % 5 == 1
    null (by mask / by NaN) and about a fifth of the other rows; the masked
    float variant also keeps some NaN under a set mask byte.
    """
    rng = np.random.default_rng(
        [seed, AGG_TYPES.index(type_name), ngroups, int(skew)])
    gid = agg_row_gid(ngroups, n, rng, skew)
    data = _agg_values(type_name, n, rng)
    mask = None
    null = (gid % 5 == 1) | (rng.random(n) < 0.2)
    is_float = type_name in ("float32", "float64")
    if variant == "masked":
        mask = (~null).astype(np.uint8)
        if is_float:
            data[rng.random(n) < 0.05] = np.nan
    elif variant == "nan":
        data[null] = np.nan
    else:
        assert variant == "plain"
    return dict(data=data, mask=mask, kind=_KIND[type_name], row_gid=gid,
                ngroups=ngroups)


def agg_freeform_case():
    rng = np.random.default_rng(11)
    n, ngroups = 60013, 37
    gid = agg_row_gid(ngroups, n, rng)
    return dict(data=rng.uniform(-1e6, 1e6, n), mask=None, kind=R.FLOAT64,
                row_gid=gid, ngroups=ngroups)


def agg_prod_case():
    """Factors +-1, 2 and 1/2: every product is a signed power of two, so
    it is exact whatever order the CAS loop multiplies in."""
    rng = np.random.default_rng(12)
    n, ngroups = 5003, 50
    gid = agg_row_gid(ngroups, n, rng)
    data = rng.choice(np.array([1.0, -1.0, 2.0, 0.5]), n)
    data[rng.random(n) < 0.05] = np.nan
    mask = (rng.random(n) > 0.1).astype(np.uint8)
    return dict(data=data, mask=mask, kind=R.FLOAT64, row_gid=gid,
                ngroups=ngroups)


def agg_int_edge_cases():
    """name -> (case, op) for the integer edges."""
    rng = np.random.default_rng(13)
    n, ngroups = 3001, 9
    gid = agg_row_gid(ngroups, n, rng)
    out = {}
    v = rng.integers(-2**62, 2**62, n).astype(np.int64)
    lo = v.copy()
    lo[gid == 0] = R.I64_MIN       # a group of nothing but INT64_MIN
    lo[np.nonzero(gid == 2)[0][:1]] = R.I64_MIN  # and one among others
    out["max_with_int64_min"] = (dict(data=lo, mask=None, kind=R.INT64,
                                      row_gid=gid, ngroups=ngroups),
                                 "max_i64")
    hi = v.copy()
    hi[gid == 0] = R.I64_MAX
    hi[np.nonzero(gid == 2)[0][:1]] = R.I64_MAX
    out["min_with_int64_max"] = (dict(data=hi, mask=None, kind=R.INT64,
                                      row_gid=gid, ngroups=ngroups),
                                 "min_i64")
    big = rng.integers(2**61, 2**62, n).astype(np.int64)
    big[gid == 4] *= -1
    out["sum_wraps"] = (dict(data=big, mask=None, kind=R.INT64, row_gid=gid,
                             ngroups=ngroups), "sum_i64")
    for name, dt, kind in (("int8_negative", np.int8, R.INT8),
                           ("int16_negative", np.int16, R.INT16)):
        info = np.iinfo(dt)
        neg = rng.integers(info.min, 0, n).astype(dt)
        for op in ("sum_i64", "min_i64", "max_i64", "sum_f64"):
            out[f"{name}_{op}"] = (dict(data=neg, mask=None, kind=kind,
                                        row_gid=gid, ngroups=ngroups), op)
    return out


# (type, variant, op, want_count); type None is ``size`` with the dummy
# one-element data tensor
_FUSED_SPECS = (
    ("float64", "masked", "sum_f64", 1),     # 0
    ("int32", "plain", "min_i64", 0),        # 1
    (None, None, "size", 1),                 # 2
    ("float32", "nan", "max_f64", 1),        # 3
    ("int16", "masked", "sum_i64", 0),       # 4
    ("float64", "nan", "min_f64", 0),        # 5
    ("uint8", "masked", "count", 1),         # 6
    ("timestamp", "masked", "max_i64", 1),   # 7
    ("int8", "plain", "sum_f64", 0),         # 8
    ("float32", "masked", "min_f64", 1),     # 9
    ("float64", "plain", "max_f64", 0),      # 10
    ("uint8", "plain", "sum_i64", 1),        # 11
    ("int16", "plain", "max_i64", 1),        # 12
    ("bool", "masked", "count", 0),          # 13
)

# fused launches: (ngroups, indices into _FUSED_SPECS).
# n_aggs * ngroups * 16 B <= 48 KiB runs the LDS kernel: 4 * 768 and
# 1 * 3072 are the last LDS sizes, everything above runs the global one.
# The specs of each launch are chosen by hand so that the launches above the
# limit cover every op of the fused kernels and every loader branch on
# their own, as the launches below it do (checked in test_relational_ref).
FUSED_LAUNCHES = (
    (100, (2,)),
    (100, (0, 13)),
    (100, (3, 4, 1)),
    (100, (6, 7, 8, 12)),
    (700, (2, 9, 10, 11)),
    (768, (5, 3, 4, 6)),
    (769, (5, 3, 4, 6)),
    (800, (2, 9, 10, 11)),
    (801, (7, 8, 0, 1)),
    (802, (12, 13, 2, 5)),
    (3072, (3,)),
    (3073, (3,)),
    (3073, (2,)),
)
FUSED_LDS_BYTES = 48 * 1024


def fused_launch_id(launch):
    ngroups, idx = launch
    return "%d-%d-%s" % (len(idx), ngroups,
                         "+".join(_FUSED_SPECS[i][2] for i in idx))


def fused_specs(launch):
    return [_FUSED_SPECS[i] for i in launch[1]]


def fused_is_global(launch):
    return len(launch[1]) * launch[0] * 16 > FUSED_LDS_BYTES


def fused_case(launch, n=AGG_ROWS):
    """row_gid plus the launch's (case, op, want_count) sharing it."""
    ngroups = launch[0]
    gid = agg_row_gid(ngroups, n, np.random.default_rng([21, ngroups]))
    aggs = []
    for k, (tname, variant, op, want) in enumerate(fused_specs(launch)):
        if tname is None:
            case = dict(data=np.zeros(1, np.int8), mask=None, kind=R.INT8,
                        row_gid=gid, ngroups=ngroups)
        else:
            case = agg_case(tname, ngroups, variant, n=n, seed=30 + k)
            null = (gid % 5 == 1)
            if case["mask"] is not None:
                case["mask"][null] = 0
            elif variant == "nan":
                case["data"][null] = np.nan
            case["row_gid"] = gid
        aggs.append((case, op, want))
    return gid, aggs


# ----------------------------------------------------------------------
# key inputs (group build and join)
# ----------------------------------------------------------------------

_WORDS = [b"", b"a", b"ab", b"abc", b"abd", b"b", b"ab\x00", b"abcdefgh",
          b"abcdefghi", b"abcdefgh\xc3\xa9", b"x" * 40, b"x" * 41,
          b"x" * 39 + b"y"]


def string_col(values, mask=None):
    lens = np.array([len(v) for v in values], dtype=np.int64)
    offsets = np.zeros(len(values) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer(b"".join(values), dtype=np.uint8).copy()
    return KeyCol(data, mask, offsets, R.STRING)


def _proto_column(name, g, rng):
    """``g`` prototype values of one key column type (duplicates allowed;
    prototypes are made distinct row-wise by the caller)."""
    if name == "int64":
        v = rng.integers(-2**62, 2**62, g).astype(np.int64)
        v[:4] = [R.I64_MIN, R.I64_MAX, 0, -1]
        return ("fixed", v, R.INT64)
    if name == "int32":
        return ("fixed", rng.integers(-50, 50, g).astype(np.int32), R.INT32)
    if name == "int16":
        return ("fixed", rng.integers(-2**15, 2**15, g).astype(np.int16),
                R.INT16)
    if name == "int8":
        return ("fixed", rng.integers(-128, 128, g).astype(np.int8), R.INT8)
    if name == "bool":
        return ("fixed", rng.integers(0, 2, g).astype(np.uint8), R.BOOL)
    if name == "date32":
        return ("fixed", rng.integers(-9000, 9000, g).astype(np.int32),
                R.DATE32)
    if name == "float64":
        v = rng.integers(-40, 40, g) / 8.0
        v[:2] = [0.0, -0.0]
        v[2] = np.nan
        # a NaN with another payload and sign is still the same key
        v[3] = np.array([0xFFF8000000000123], dtype=np.uint64).view(
            np.float64)[0]
        v[4:6] = [np.inf, -np.inf]
        return ("fixed", v.astype(np.float64), R.FLOAT64)
    if name == "float32":
        v = (rng.integers(-40, 40, g) / 8.0).astype(np.float32)
        v[:3] = [0.0, -0.0, np.nan]
        return ("fixed", v, R.FLOAT32)
    if name == "string":
        words = _WORDS + [b"k%d" % i for i in range(400)]
        return ("string", [words[i] for i in rng.integers(0, len(words), g)],
                R.STRING)
    if name == "dict":
        return ("dict", rng.integers(0, 40, g).astype(np.int32), R.DICT)
    raise ValueError(name)


DICT_VALUES = [b"d%03d" % i if i else b"" for i in range(40)]


def _take_column(proto, idx, mask):
    form, vals, kind = proto
    if form == "string":
        return string_col([vals[i] for i in idx], mask)
    data = vals[idx].copy()
    return KeyCol(data, mask, None, kind,
                  DICT_VALUES if form == "dict" else None)


def key_case(col_names, masked, n_groups, n, seed):
    """Key columns of ``n`` rows drawn from about ``n_groups`` distinct
    prototype rows.  Columns listed in ``masked`` get a validity mask; the
    data under a null differs from row to row and must not split the group.
    """
    rng = np.random.default_rng([seed, n_groups, n])
    g = n_groups
    protos = [_proto_column(c, g, rng) for c in col_names]
    pmask = [(rng.random(g) > 0.15) if c_i in masked else None
             for c_i in range(len(col_names))]
    idx = rng.integers(0, g, n)
    idx[:g] = np.arange(g)  # every prototype occurs
    cols = []
    for ci, proto in enumerate(protos):
        mask = None
        if pmask[ci] is not None:
            mask = pmask[ci][idx].astype(np.uint8)
        col = _take_column(proto, idx, mask)
        if mask is not None and col.kind not in (R.STRING, R.DICT):
            # scramble what lies under the nulls (masked float columns keep
            # NaN out of their valid rows: pandas cannot tell the two apart)
            junk = rng.integers(0, 100, n).astype(col.data.dtype)
            data = np.where(mask.astype(bool), col.data, junk)
            if col.kind in (R.FLOAT32, R.FLOAT64):
                bad = np.isnan(data) & mask.astype(bool)
                data[bad] = 7.0
            col = col._replace(data=data.astype(col.data.dtype))
        cols.append(col)
    return cols


# name -> (column types, indices of masked columns)
KEY_LAYOUTS = {
    "int64": (("int64",), ()),
    "string": (("string",), ()),
    "dict": (("dict",), ()),
    "float64": (("float64",), ()),
    "float32": (("float32",), ()),
    "masked_int32": (("int32",), (0,)),
    "masked_string": (("string",), (0,)),
    "masked_float64": (("float64",), (0,)),
    "int64_string": (("int64", "string"), ()),
    "int8m_float32_string": (("int8", "float32", "string"), (0,)),
    "int16_bool_date32": (("int16", "bool", "date32"), (1,)),
    "dict_int32m": (("dict", "int32"), (1,)),
}


def build_key_case(name, collide=False):
    """Group-build input.  ``collide``: 4000 rows in about 50 groups, for
    the constant-hash run where only the row equality separates groups."""
    names, masked = KEY_LAYOUTS[name]
    seed = sorted(KEY_LAYOUTS).index(name)
    if collide:
        return key_case(names, masked, 50, 4000, 100 + seed)
    return key_case(names, masked, 300, 5003, 200 + seed)


def packed_key_cases():
    """name -> int64 packed keys (< 2^63; all-ones is the empty-slot
    sentinel and cannot come out of the packer, which stops at 63 bits)."""
    rng = np.random.default_rng(41)
    n = 5003
    out = {"single": rng.integers(0, 1000, n).astype(np.int64)}
    a = rng.integers(0, 30, n).astype(np.int64)
    b = rng.integers(0, 2**20, n).astype(np.int64) % 17
    c = rng.integers(0, 2**23, n).astype(np.int64) % 5
    out["three_columns_63_bits"] = a | (b << 20) | ((c + 2**23 - 5) << 40)
    wide = rng.integers(0, 40, n).astype(np.int64) << 57
    wide[::7] = R.I64_MAX  # 2^63 - 1, the largest packable key
    wide[1::7] = 0
    out["int64_max"] = wide
    return out


def chunk_cases():
    """Test A/B/C of the chunked insert: name -> (keys, chunk_rows,
    max_initial_cap).  In A chunks are a quarter of the table, so it is at
    most 3/4 full before a load check grows it; B and C hold 10 keys."""
    rng = np.random.default_rng(42)
    n = 20000
    distinct = rng.permutation(n).astype(np.int64) * 3 + 1
    few = (rng.integers(0, 10, n).astype(np.int64) * 1001 + 5)
    # the last of the 10 keys first shows up deep inside a later chunk
    few[few == few.max()] = few.min()
    few[n - 300] = 9 * 1001 + 5
    return {
        "A_grow": (distinct, 256, 1024),
        "B_later_chunks": (few, 256, 1024),
        "C_chunk_above_cap": (few, 4096, 1024),
    }


# ----------------------------------------------------------------------
# join inputs: name -> (build key columns, probe key columns)
# ----------------------------------------------------------------------

def _split_case(names, masked, n_groups, n_build, n_probe, seed,
                probe_only=0.25):
    """Build and probe rows drawn from one prototype set; about
    ``probe_only`` of the groups occur on the probe side alone."""
    cols = key_case(names, masked, n_groups, n_build + n_probe, seed)
    labels = R.ref_partition(cols)
    rng = np.random.default_rng(seed)
    only = set(np.nonzero(rng.random(labels.max() + 1) < probe_only)[0])
    rows = np.arange(n_build + n_probe)
    is_build = (rows < n_build) & ~np.isin(labels, list(only))
    return take_rows(cols, rows[is_build]), take_rows(cols, rows[n_build:])


def take_rows(cols, rows):
    out = []
    for c in cols:
        mask = None if c.mask is None else c.mask[rows]
        if c.kind == R.STRING:
            raw = c.data.tobytes()
            vals = [raw[c.offsets[i]:c.offsets[i + 1]] for i in rows]
            out.append(string_col(vals, mask))
        else:
            out.append(c._replace(data=c.data[rows].copy(), mask=mask))
    return out


def _many_to_many():
    rng = np.random.default_rng(51)
    dup = rng.integers(1, 51, 200)
    build = np.concatenate([np.repeat(np.arange(200), dup),
                            np.full(3000, 9999)]).astype(np.int64)
    build = build[rng.permutation(len(build))]
    probe = np.concatenate([rng.integers(0, 260, 2000),
                            np.full(10, 9999)]).astype(np.int64)
    probe = probe[rng.permutation(len(probe))]
    return ([KeyCol(build, None, None, R.INT64)],
            [KeyCol(probe, None, None, R.INT64)])


def _no_match():
    rng = np.random.default_rng(52)
    return ([KeyCol(rng.integers(0, 100, 700).astype(np.int64), None, None,
                    R.INT64)],
            [KeyCol(rng.integers(100, 200, 900).astype(np.int64), None, None,
                    R.INT64)])


def join_cases():
    two = _split_case(("int64", "string"), (), 120, 3000, 2000, 53)
    const = _split_case(("int64", "string"), (1,), 60, 1500, 500, 56)
    empty_b, empty_p = _split_case(("int64", "string"), (), 20, 300, 200, 57)
    none = [c for c in take_rows(empty_b, np.zeros(0, dtype=np.int64))]
    return {
        "many_to_many": _many_to_many(),
        "int64_string": two,
        "masked_both": _split_case(("int32", "int16"), (0, 1), 150, 3000,
                                   2000, 54),
        "float64_nan": _split_case(("float64",), (), 60, 1500, 1500, 55),
        "constant_hash": const,
        "empty_build": (none, empty_p),
        "empty_probe": (empty_b, take_rows(empty_p,
                                           np.zeros(0, dtype=np.int64))),
        "no_match": _no_match(),
    }


def key_frame(cols, prefix="k"):
    """pandas frame of key columns: nulls as NA/None, strings as bytes
    decoded latin-1 (a bijection on bytes), dictionary codes as integers."""
    import pandas as pd

    out = {}
    for i, c in enumerate(cols):
        name = f"{prefix}{i}"
        mask = None if c.mask is None else c.mask.astype(bool)
        if c.kind == R.STRING:
            raw = c.data.tobytes()
            vals = [raw[c.offsets[j]:c.offsets[j + 1]].decode("latin-1")
                    for j in range(len(c.offsets) - 1)]
            if mask is not None:
                vals = [v if ok else None for v, ok in zip(vals, mask)]
            out[name] = pd.Series(vals, dtype=object)
        elif c.kind in (R.FLOAT32, R.FLOAT64):
            v = c.data.astype(np.float64)
            if mask is not None:
                v = np.where(mask, v, np.nan)
            out[name] = pd.Series(v)
        else:
            v = c.data.astype(np.int64)
            if mask is None:
                out[name] = pd.Series(v)
            else:
                out[name] = pd.Series(pd.arrays.IntegerArray(v, ~mask))
    return pd.DataFrame(out)
