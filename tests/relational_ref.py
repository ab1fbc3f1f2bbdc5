"""Plain numpy/python references for the relational HIP kernels
(``agg_update``, ``agg_update_fused``, ``groupby_build``,
``groupby_build_packed``, ``join_build`` + ``join_probe``).

Every function takes the raw arrays the kernel takes: storage-typed numpy
data (unsigned 16/32/64-bit columns arrive as bit-identical signed arrays,
bool as uint8), an optional uint8/bool validity mask, int64 string offsets
and the ``TypeKind`` id.  Nothing here needs a GPU or torch; the CPU tests in
``test_relational_ref.py`` check these references against pandas.
"""

import math
from collections import Counter

import numpy as np

# csrc/common.h BodoType / bodo_amd.core.types.TypeKind
INT8, INT16, INT32, INT64, FLOAT32, FLOAT64, BOOL, DATE32, TIMESTAMP_NS, \
    STRING, DICT, DECIMAL128, UINT8, UINT16, UINT32, UINT64 = range(16)

I64_MAX = int(np.iinfo(np.int64).max)
I64_MIN = int(np.iinfo(np.int64).min)

# csrc/kernels.hip AggOp
AGG_OPS = {
    "sum_f64": 0, "sum_i64": 1, "count": 2, "min_f64": 3, "max_f64": 4,
    "min_i64": 5, "max_i64": 6, "size": 7, "first_row": 8, "last_row": 9,
    "prod_f64": 10,
}
F64_OPS = ("sum_f64", "min_f64", "max_f64", "prod_f64")

# (init_f, init_i) the host passes for each op: the identity of the op
AGG_INIT = {
    "sum_f64": (0.0, 0), "sum_i64": (0.0, 0), "count": (0.0, 0),
    "min_f64": (math.inf, 0), "max_f64": (-math.inf, 0),
    "min_i64": (0.0, I64_MAX), "max_i64": (0.0, I64_MIN), "size": (0.0, 0),
    "first_row": (0.0, I64_MAX), "last_row": (0.0, I64_MIN),
    "prod_f64": (1.0, 0),
}

_LOAD_VIEW = {
    INT8: np.int8, UINT8: np.uint8, BOOL: np.uint8, INT16: np.int16,
    UINT16: np.uint16, INT32: np.int32, DATE32: np.int32, DICT: np.int32,
    UINT32: np.uint32, INT64: np.int64, UINT64: np.int64,
    TIMESTAMP_NS: np.int64, DECIMAL128: np.int64,
    FLOAT32: np.float32, FLOAT64: np.float64,
}


def load_values(data, dtype_kind):
    """The kernels' value loader: (iv int64, dv float64, is_nan bool)."""
    raw = np.ascontiguousarray(data)
    if raw.dtype == np.bool_:
        raw = raw.view(np.uint8)
    v = raw.view(_LOAD_VIEW[dtype_kind])
    if dtype_kind in (FLOAT32, FLOAT64):
        dv = v.astype(np.float64)
        nan = np.isnan(dv)
        # (int64_t)f of a NaN/inf is undefined in C++: only finite values
        # take part in integer ops
        with np.errstate(invalid="ignore"):
            iv = np.where(np.isfinite(dv), dv, 0.0).astype(np.int64)
        return iv, dv, nan
    iv = v.astype(np.int64)
    return iv, iv.astype(np.float64), np.zeros(len(v), dtype=bool)


def valid_rows(data, mask, dtype_kind):
    """Kernel validity contract: mask byte non-zero and float not NaN."""
    _, _, nan = load_values(data, dtype_kind)
    ok = ~nan
    if mask is not None:
        ok &= np.asarray(mask).astype(bool)
    return ok


def _rows_by_group(row_gid, ngroups, keep):
    gid = np.asarray(row_gid).astype(np.int64)
    rows = np.nonzero(keep)[0]
    order = rows[np.argsort(gid[rows], kind="stable")]
    bounds = np.searchsorted(gid[order], np.arange(ngroups + 1))
    return order, bounds


def ref_agg(data, mask, dtype_kind, row_gid, ngroups, op):
    """Reference of one ``agg_update`` launch: ``(acc, cnt)``.

    ``acc`` is float64 for the f64 ops and int64 otherwise, and starts at
    ``AGG_INIT[op]``; a group with no valid row keeps it and has cnt == 0.
    ``size`` counts every row, all other ops only valid ones.  Integer sums
    wrap modulo 2^64; float sums are ``math.fsum`` per group.
    """
    n = len(row_gid)
    init_f, init_i = AGG_INIT[op]
    if op in F64_OPS:
        acc = np.full(ngroups, init_f, dtype=np.float64)
    else:
        acc = np.full(ngroups, init_i, dtype=np.int64)
    if op == "size":
        cnt = np.bincount(np.asarray(row_gid).astype(np.int64),
                          minlength=ngroups).astype(np.int64)
        return acc, cnt
    iv, dv, _ = load_values(data, dtype_kind)
    ok = valid_rows(data, mask, dtype_kind)
    assert len(iv) >= n
    order, bounds = _rows_by_group(row_gid, ngroups, ok[:n])
    cnt = np.diff(bounds).astype(np.int64)
    for g in range(ngroups):
        rows = order[bounds[g]:bounds[g + 1]]
        if len(rows) == 0 or op == "count":
            continue
        if op == "sum_f64":
            acc[g] = math.fsum(dv[rows].tolist())
        elif op == "sum_i64":
            acc[g] = _wrap_sum(iv[rows])
        elif op == "min_f64":
            acc[g] = dv[rows].min()
        elif op == "max_f64":
            acc[g] = dv[rows].max()
        elif op == "min_i64":
            acc[g] = iv[rows].min()
        elif op == "max_i64":
            acc[g] = iv[rows].max()
        elif op == "first_row":
            acc[g] = rows.min()
        elif op == "last_row":
            acc[g] = rows.max()
        elif op == "prod_f64":
            p = 1.0
            for x in dv[rows].tolist():
                p *= x
            acc[g] = p
        else:
            raise ValueError(op)
    return acc, cnt


def _wrap_sum(iv):
    """Sum of int64 values modulo 2^64, as a signed int64."""
    total = sum(int(x) for x in iv.tolist()) & 0xFFFFFFFFFFFFFFFF
    return np.array(total, dtype=np.uint64).view(np.int64)[()]


def ref_sum_bound(data, mask, dtype_kind, row_gid, ngroups):
    """Per-group bound on |atomic float sum - fsum|.

    Summing n_g doubles in any order with round-to-nearest is off by at most
    (n_g - 1) * u * sum|x_i| (u = 2^-53) to first order; the LDS path adds
    block partials in a second level of the same kind, covered by a factor 2.
    """
    _, dv, _ = load_values(data, dtype_kind)
    ok = valid_rows(data, mask, dtype_kind)
    order, bounds = _rows_by_group(row_gid, ngroups, ok[:len(row_gid)])
    out = np.zeros(ngroups, dtype=np.float64)
    for g in range(ngroups):
        rows = order[bounds[g]:bounds[g + 1]]
        if len(rows) > 1:
            out[g] = 2.0 * (len(rows) - 1) * 2.0 ** -53 * \
                math.fsum(np.abs(dv[rows]).tolist())
    return out


# ----------------------------------------------------------------------
# keys: a key column is (data, mask, offsets, dtype_kind)
# ----------------------------------------------------------------------

def _key_values(col):
    """Canonical python value per row: None for null, bytes for strings,
    0.0 for both zeros, the string "nan" for every NaN, else the number
    (dictionary columns compare by code, as the kernel does)."""
    data, mask, offsets, kind = col[:4]
    if kind == STRING:
        raw = np.ascontiguousarray(data).view(np.uint8).tobytes()
        off = np.asarray(offsets).astype(np.int64)
        vals = [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    elif kind in (FLOAT32, FLOAT64):
        f = np.ascontiguousarray(data).view(_LOAD_VIEW[kind]).astype(np.float64)
        vals = ["nan" if x != x else (0.0 if x == 0.0 else x)
                for x in f.tolist()]
    else:
        # equality is on the stored bits; widths never mix within a column
        raw = np.ascontiguousarray(data)
        if raw.dtype == np.bool_:
            raw = raw.view(np.uint8)
        vals = raw.tolist()
    if mask is not None:
        m = np.asarray(mask).astype(bool)
        vals = [v if ok else None for v, ok in zip(vals, m.tolist())]
    return vals


def row_keys(key_columns):
    cols = [_key_values(c) for c in key_columns]
    return list(zip(*cols))


def ref_partition(key_columns):
    """Group label per row, numbered by first appearance.  Null-aware (null
    equals null), -0.0 == 0.0, NaN == NaN, strings compare by bytes."""
    seen = {}
    keys = row_keys(key_columns)
    labels = np.empty(len(keys), dtype=np.int64)
    for i, k in enumerate(keys):
        labels[i] = seen.setdefault(k, len(seen))
    return labels


def canonical_labels(labels):
    """Relabel any group labelling by first appearance."""
    seen = {}
    out = np.empty(len(labels), dtype=np.int64)
    for i, g in enumerate(np.asarray(labels).tolist()):
        out[i] = seen.setdefault(g, len(seen))
    return out


def np_encode(keys, plan):
    """slot = sum_k (key_k - lo_k) * stride_k, the last key fastest, in
    64-bit unsigned arithmetic as groupby_dense_fused_kernel forms it."""
    slot = np.zeros(len(keys[0]), dtype=np.uint64)
    stride = 1
    for key, (lo, radix) in reversed(list(zip(keys, plan))):
        digit = key.astype(np.int64).view(np.uint64) - np.uint64(lo % 2**64)
        assert (digit < radix).all()
        slot += digit * np.uint64(stride)
        stride *= radix
    return slot.astype(np.int64), stride


def ref_join_pairs(build_keys, probe_keys, how):
    """Reference of ``join_build`` + ``join_probe``.

    how: 0 inner, 1 left, 2 semi, 3 anti.  Returns ``(pairs, matched)``:
    ``pairs`` is a Counter of (probe_row, build_row); build_row is -1 for a
    left-join row with no match and None for semi/anti, which emit probe
    rows only.  ``matched`` is the set of build rows equal to some probe
    row.  A key that is null on both sides is equal (``rows_eq2``).
    """
    table = {}
    for b, k in enumerate(row_keys(build_keys)):
        table.setdefault(k, []).append(b)
    pairs = Counter()
    matched = set()
    for p, k in enumerate(row_keys(probe_keys)):
        hits = table.get(k, [])
        matched.update(hits)
        if how == 0:
            pairs.update((p, b) for b in hits)
        elif how == 1:
            pairs.update(((p, b) for b in hits) if hits else [(p, -1)])
        elif how == 2:
            if hits:
                pairs[(p, None)] += 1
        elif how == 3:
            if not hits:
                pairs[(p, None)] += 1
        else:
            raise ValueError(how)
    return pairs, matched
