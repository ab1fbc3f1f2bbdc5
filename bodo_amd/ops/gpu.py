"""GPU op implementations: thin wrappers over the hand-written gfx950 HIP
kernels in csrc/ (built in-tree as ``bodo_amd_kernels``).

Fails loudly if the native extension is missing on a CUDA device (no silent
eager fallback; round-end native check).
"""

from __future__ import annotations

import os
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ..core import types as bt
from ..core.column import Column
from ..core.table import Table
from ..core.types import TypeKind

try:
    import bodo_amd_kernels as _K
except ImportError as e:  # pragma: no cover
    _K = None
    _IMPORT_ERR = e


def kernels():
    if _K is None:
        raise ImportError(
            "bodo_amd_kernels HIP extension not built; run "
            "`python setup.py build_ext --inplace` "
            f"(import error: {_IMPORT_ERR})")
    return _K


def _fnv_bytes(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for ch in b:
        h = ((h ^ ch) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


_DICT_HASH_CACHE: dict = {}


def _dict_hash_lut(col: Column) -> torch.Tensor:
    key = (id(col.dictionary), str(col.device))
    # the entry keeps its dictionary alive, so the id cannot be reused by
    # another dictionary while the entry exists
    lut = _DICT_HASH_CACHE.get(key, (None, None))[0]
    if lut is None:
        vals = col.dictionary.to_pylist()
        arr = np.array(
            [_fnv_bytes(v.encode() if v is not None else b"") for v in vals],
            dtype=np.uint64)
        lut = torch.from_numpy(arr.view(np.int64)).to(col.device)
        _DICT_HASH_CACHE[key] = (lut, col.dictionary)
        if len(_DICT_HASH_CACHE) > 256:
            _DICT_HASH_CACHE.clear()
            _DICT_HASH_CACHE[key] = (lut, col.dictionary)
    return lut


def _data_mask8(col: Column):
    """(data, mask) as the kernels read them: bool values and the validity
    mask as uint8."""
    data = col.data
    if data is not None and data.dtype == torch.bool:
        data = data.view(torch.uint8)
    return data, None if col.mask is None else col.mask.view(torch.uint8)


def _col_args(cols: Sequence[Column]):
    datas, masks, offsets, auxs, dtypes = [], [], [], [], []
    for c in cols:
        data, mask8 = _data_mask8(c)
        if c.dtype.kind == TypeKind.STRING:
            datas.append(data if data is not None else
                         torch.zeros(0, dtype=torch.uint8, device=c.device))
            offsets.append(c.offsets)
            auxs.append(None)
        elif c.dtype.kind == TypeKind.DICT:
            datas.append(data)
            offsets.append(None)
            auxs.append(_dict_hash_lut(c))
        else:
            datas.append(data)
            offsets.append(None)
            auxs.append(None)
        masks.append(mask8)
        dtypes.append(int(c.dtype.kind))
    return datas, masks, offsets, auxs, dtypes


def hash_columns(cols: Sequence[Column], seed: int = 0) -> torch.Tensor:
    K = kernels()
    n = len(cols[0])
    datas, masks, offsets, auxs, dtypes = _col_args(cols)
    return K.hash_columns(datas, masks, offsets, auxs, dtypes, n, seed)


_DT_FIELD_ID = {
    "year": 0, "month": 1, "day": 2, "hour": 3, "minute": 4, "second": 5,
    "dayofweek": 6, "weekday": 6, "dayofyear": 7, "quarter": 8, "date": 9,
    "normalize": 10, "floor_day": 10,
}

_DT_RANGE = {
    "month": (1, 12), "day": (1, 31), "hour": (0, 23), "minute": (0, 59),
    "second": (0, 59), "dayofweek": (0, 6), "weekday": (0, 6),
    "dayofyear": (1, 366), "quarter": (1, 4),
}

_DT_OUT_KIND = {
    "year": (0, bt.int16), "month": (0, bt.int8), "day": (0, bt.int8),
    "hour": (0, bt.int8), "minute": (0, bt.int8), "second": (0, bt.int8),
    "dayofweek": (0, bt.int8), "weekday": (0, bt.int8),
    "dayofyear": (0, bt.int16), "quarter": (0, bt.int8),
    "date": (1, bt.date32), "normalize": (2, bt.timestamp_ns),
    "floor_day": (2, bt.timestamp_ns),
}


def dt_field(col: Column, fld: str) -> Column:
    K = kernels()
    is_date32 = 1 if col.dtype.kind == TypeKind.DATE32 else 0
    out_kind, out_dtype = _DT_OUT_KIND[fld]
    res = K.dt_field(col.data, is_date32, _DT_FIELD_ID[fld], out_kind)
    # int16 kernel output narrowed per field on the python side
    store = bt.torch_storage_dtype(out_dtype)
    if res.dtype != store:
        res = res.to(store)
    out = Column(out_dtype, res, col.mask)
    out.val_range = _DT_RANGE.get(fld)
    return out


def gather_string(col: Column, idx: torch.Tensor) -> Column:
    K = kernels()
    data = col.data if col.data is not None else torch.zeros(
        0, dtype=torch.uint8, device=col.device)
    out, new_off = K.gather_string(data, col.offsets, idx.to(torch.int64))
    mask = col.mask[idx] if col.mask is not None else None
    return Column(bt.string, out, mask, offsets=new_off, length=int(idx.numel()))


# ----------------------------------------------------------------------
# groupby
# ----------------------------------------------------------------------

# op name -> (id in csrc/kernels.hip AggOp, init_f, init_i).  Accumulators
# start at the identity of the op, so a group whose valid values are all
# +inf (min) or all -inf (max) keeps them.
_I64_MAX = int(np.iinfo(np.int64).max)
_I64_MIN = int(np.iinfo(np.int64).min)
_AGG_OPS = {
    "sum_f64": (0, 0.0, 0), "sum_i64": (1, 0.0, 0), "count": (2, 0.0, 0),
    "min_f64": (3, float("inf"), 0), "max_f64": (4, -float("inf"), 0),
    "min_i64": (5, 0.0, _I64_MAX), "max_i64": (6, 0.0, _I64_MIN),
    "size": (7, 0.0, 0), "first_row": (8, 0.0, _I64_MAX),
    "last_row": (9, 0.0, _I64_MIN), "prod_f64": (10, 1.0, 0),
}


def _keys_valid_mask(cols: Sequence[Column]) -> Optional[torch.Tensor]:
    m = None
    for c in cols:
        v = None
        if c.mask is not None:
            v = c.mask
        if c.dtype.is_float:
            nn = ~torch.isnan(c.data)
            v = nn if v is None else (v & nn)
        if v is not None:
            m = v if m is None else (m & v)
    return m


def _key_bounds(c: Column) -> Optional[Tuple[int, int]]:
    """Known inclusive (lo, hi) of an unmasked small-range key column:
    dictionary codes, bools, and integer/date32 columns with val_range.
    None for anything else."""
    if c.mask is not None:
        return None
    k = c.dtype.kind
    if k == TypeKind.DICT:
        return 0, max(0, len(c.dictionary) - 1)
    if k == TypeKind.BOOL:
        return 0, 1
    if (c.dtype.is_integer or k == TypeKind.DATE32) and c.val_range:
        lo, hi = c.val_range
        return int(lo), int(hi)
    return None


def _try_pack_keys(key_cols: Sequence[Column]) -> Optional[Column]:
    """Pack small-range integer/dict/bool keys into ONE int64 column so the
    hash-table equality check reads 8 bytes instead of one random read per
    key column (reference analog: key normalization in _hash_join.cpp)."""
    shift = 0
    packed = None
    for c in key_cols:
        bounds = _key_bounds(c)
        if bounds is None:
            return None
        lo, hi = bounds
        width = max(1, int(hi - lo + 1).bit_length())
        if shift + width > 63:
            return None
        part = (c.data.long() - lo) << shift
        packed = part if packed is None else (packed | part)
        shift += width
    if packed is None:
        return None
    return Column(bt.int64, packed)


FUSABLE = {"count", "size", "sum", "mean", "min", "max"}
MAX_FUSED_AGGS = 4
# below this many accumulator bytes agg_update_fused aggregates in LDS
FUSED_LDS_BYTES = 48 * 1024

# Dense (direct-address) groupby: when the keys' known ranges bound the key
# space, the mixed-radix key is the group's slot and one kernel reads keys
# and values and updates the accumulators (groupby_dense_fused).
# BODO_AMD_DENSE_GROUPBY=0 turns the route off.
DENSE_GROUPBY = os.environ.get("BODO_AMD_DENSE_GROUPBY", "1") != "0"
DENSE_MAX_KEYS = 8
DENSE_MAX_SLOTS = 1 << 25


def dense_groupby_plan(key_cols: Sequence[Column], batch, n: int):
    """Per-key (lo, radix) when the dense route applies to ``n`` rows
    grouped by ``key_cols`` with the aggregates ``batch`` of (out_name,
    column or None, func); None when the hash route has to run."""
    if not 1 <= len(key_cols) <= DENSE_MAX_KEYS:
        return None
    if not 1 <= len(batch) <= MAX_FUSED_AGGS:
        return None
    for _, col, func in batch:
        if func not in FUSABLE:
            return None
        if col is not None and col.dtype.kind == TypeKind.STRING:
            return None
    plan = []
    nslots = 1
    for c in key_cols:
        bounds = _key_bounds(c)
        if bounds is None:
            return None
        lo, hi = bounds
        radix = hi - lo + 1
        if radix < 1 or not -2**63 <= lo < 2**63:
            return None
        nslots *= radix
        if nslots > DENSE_MAX_SLOTS:
            return None
        plan.append((lo, radix))
    if nslots > 4 * n:
        return None  # the table would outgrow the hash table of 2n slots
    if len(batch) * nslots * 16 <= FUSED_LDS_BYTES:
        return None  # few groups: the LDS kernel behind the hash route wins
    return plan


def slot_digits(slots: torch.Tensor, plan):
    """Digit of every key in mixed-radix slot ids (the last key varies
    fastest): the inverse of groupby_dense_fused's slot encoding."""
    digits = []
    for _, radix in reversed(plan):
        digits.append(slots % radix)
        slots = slots // radix
    return digits[::-1]


def _groupby_dense(keys, key_cols, batch, plan, n) -> Optional[Table]:
    """Dense route of groupby_local; None when a key lay outside its
    val_range, in which case nothing was computed."""
    recs = [_fused_agg(col, func) for _, col, func in batch]
    flat = kernels().groupby_dense_fused(
        [_data_mask8(c)[0] for c in key_cols],
        [int(c.dtype.kind) for c in key_cols],
        [lo for lo, _ in plan], [radix for _, radix in plan],
        *_fused_args(recs, key_cols[0].device), n)
    if not flat:
        return None
    slots = flat[0]
    ngroups = int(slots.numel())
    out_cols = []
    for c, (lo, _), digit in zip(key_cols, plan, slot_digits(slots, plan)):
        data = (digit + lo).to(c.data.dtype)
        col = Column(c.dtype, data, None, dictionary=c.dictionary,
                     length=ngroups)
        col.val_range = c.val_range
        out_cols.append(col)
    out_cols += _finish_fused(recs, flat[1:])
    return Table(list(keys) + [o for o, _, _ in batch], out_cols, ngroups)


def groupby_build(key_cols: Sequence[Column],
                  pack: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row_gid, uniq_rows) of the hash build.  ``pack=False`` keeps keys
    with known bounds out of the packed build, which relies on them."""
    K = kernels()
    n = len(key_cols[0])
    pk = _try_pack_keys(key_cols) if pack else None
    if pk is not None:
        return K.groupby_build_packed(pk.data)
    h = hash_columns(key_cols)
    datas, masks, offsets, auxs, dtypes = _col_args(key_cols)
    row_gid, uniq_rows = K.groupby_build(datas, masks, offsets, auxs, dtypes, n, h)
    return row_gid, uniq_rows


def groupby_local(tbl: Table, keys: Sequence[str],
                  aggs: Sequence[Tuple[str, str, str]], dropna: bool = True) -> Table:
    from . import take_table

    key_cols = [tbl.column(k) for k in keys]
    n = len(tbl)
    if dropna and n:
        valid = _keys_valid_mask(key_cols)
        if valid is not None:
            idx = torch.nonzero(valid, as_tuple=False).reshape(-1)
            if int(idx.numel()) != n:
                tbl = take_table(tbl, idx)
                key_cols = [tbl.column(k) for k in keys]
                n = len(tbl)
    if n == 0:
        return _empty_gb_result(tbl, keys, aggs)
    # (out_name, column or None, func) per aggregate, for both routes
    batch = [(o, tbl.column(i) if i and tbl.has_column(i) else None, f)
             for o, i, f in aggs]
    bounds_hold = True
    if DENSE_GROUPBY:
        plan = dense_groupby_plan(key_cols, batch, n)
        if plan is not None:
            dense = _groupby_dense(keys, key_cols, batch, plan, n)
            if dense is not None:
                return dense
            # a key lies outside its val_range: packing it with those
            # bounds would merge groups or produce the packed table's
            # empty-slot word, so the build below compares the key columns
            bounds_hold = False
    row_gid, uniq_rows = groupby_build(key_cols, pack=bounds_hold)
    ngroups = int(uniq_rows.numel())
    # fused path: batch simple aggs (count/size/sum/mean/min/max) into one
    # kernel pass sharing the row_gid read; complex aggs go one-by-one
    results = {}
    fused = []
    for out_name, col, func in batch:
        if func in FUSABLE and (col is None or col.dtype.kind != TypeKind.STRING):
            fused.append((out_name, col, func))
            if len(fused) == MAX_FUSED_AGGS:
                results.update(_run_fused(fused, row_gid, ngroups))
                fused = []
        else:
            results[out_name] = _agg_one(col, row_gid, ngroups, func,
                                         uniq_rows, tbl)
    if fused:
        results.update(_run_fused(fused, row_gid, ngroups))
    out_cols = [_gather_any(c, uniq_rows) for c in key_cols]
    out_cols += [results[o] for o, _, _ in batch]
    return Table(list(keys) + [o for o, _, _ in batch], out_cols, ngroups)


class _FusedAgg(NamedTuple):
    """One aggregate of an agg_update_fused / groupby_dense_fused launch."""
    op: str                 # key of _AGG_OPS
    col: Optional[Column]   # column the kernel reads; None for `size`
    want_count: bool        # the aggregate carries a valid count of its own
    # (acc, cnt, size count shared by the batch or None) -> result
    finish: Callable[[torch.Tensor, torch.Tensor, Optional[torch.Tensor]],
                     Column]


def _fused_agg(col: Optional[Column], func: str,
               shared: bool = False) -> _FusedAgg:
    """The launch and the finisher of one FUSABLE aggregate.  A mean with
    ``shared`` set carries no valid count of its own and divides by the
    size count of its batch."""
    is_float = col is not None and col.dtype.is_float
    if func == "size" or col is None or (
            func == "count" and col.mask is None and not is_float):
        # count over a non-nullable column == size: no column read
        return _FusedAgg("size", None, True,
                         lambda acc, cnt, size: Column(bt.int64, cnt))
    if func == "count":
        return _FusedAgg("count", col, True,
                         lambda acc, cnt, size: Column(bt.int64, cnt))
    if func == "mean":
        if shared:
            return _FusedAgg("sum_f64", col, False, lambda acc, cnt, size:
                             Column(bt.float64, acc / size.to(torch.float64)))
        return _FusedAgg("sum_f64", col, True, lambda acc, cnt, size:
                         Column(bt.float64, acc / cnt.to(torch.float64)))
    if func == "sum":
        if is_float:
            return _FusedAgg("sum_f64", col, True,
                             lambda acc, cnt, size: Column(bt.float64, acc))
        # pandas: bool sum -> int64
        return _FusedAgg("sum_i64", col, False,
                         lambda acc, cnt, size: Column(bt.int64, acc))
    if is_float:  # min / max
        return _FusedAgg(f"{func}_f64", col, True, lambda acc, cnt, size:
                         _finish_minmax_f64(acc, cnt))
    return _FusedAgg(f"{func}_i64", col, True, lambda acc, cnt, size:
                     _finish_minmax_i64(col, acc, cnt))


def _fused_args(recs: Sequence[_FusedAgg], device):
    """(datas, masks, dtypes, ops, init_fs, init_is) of a fused launch."""
    datas, masks, dtypes = [], [], []
    for r in recs:
        if r.col is None:
            datas.append(torch.zeros(1, dtype=torch.int8, device=device))
            masks.append(None)
            dtypes.append(int(TypeKind.INT8))
        else:
            data, mask8 = _data_mask8(r.col)
            datas.append(data)
            masks.append(mask8)
            dtypes.append(int(r.col.dtype.kind))
    ops_, init_fs, init_is = zip(*(_AGG_OPS[r.op] for r in recs))
    return datas, masks, dtypes, list(ops_), list(init_fs), list(init_is)


def _finish_fused(recs: Sequence[_FusedAgg], flat) -> List[Column]:
    """Results of a fused batch from its flat [acc, cnt] pairs."""
    size = next((flat[2 * k + 1] for k, r in enumerate(recs)
                 if r.op == "size"), None)
    return [r.finish(flat[2 * k], flat[2 * k + 1], size)
            for k, r in enumerate(recs)]


def _run_fused(batch, row_gid, ngroups) -> dict:
    """One agg_update_fused launch for up to MAX_FUSED_AGGS (out_name, col,
    func); the results by out_name."""
    # means over provably-NaN-free unmasked float columns can reuse a shared
    # group-size count instead of carrying their own valid-count atomics
    clean_float = {}
    for _, col, func in batch:
        if func == "mean" and col is not None and col.mask is None \
                and col.dtype.is_float and id(col) not in clean_float:
            clean_float[id(col)] = not bool(torch.isnan(col.data).any().item())
    recs = [_fused_agg(col, func) for _, col, func in batch]
    if any(clean_float.values()) and any(r.op == "size" for r in recs):
        recs = [_fused_agg(col, func, shared=func == "mean"
                           and clean_float.get(id(col), False))
                for _, col, func in batch]
    flat = kernels().agg_update_fused(
        *_fused_args(recs, row_gid.device),
        [int(r.want_count) for r in recs], row_gid, ngroups)
    return {o: c for (o, _, _), c in zip(batch, _finish_fused(recs, flat))}


def _finish_minmax_f64(acc: torch.Tensor, cnt: torch.Tensor) -> Column:
    """Float min/max: NaN for groups without a valid value."""
    return Column(bt.float64, torch.where(
        cnt == 0, torch.full_like(acc, float("nan")), acc))


def _finish_minmax_i64(col: Column, acc: torch.Tensor,
                       cnt: torch.Tensor) -> Column:
    """Integer min/max of ``col`` from its int64 accumulator: a masked
    column becomes float64 with NaN for groups without a valid value,
    anything else returns to the column's own type."""
    if col.mask is not None:
        return Column(bt.float64, torch.where(
            cnt == 0, torch.full_like(acc, float("nan"), dtype=torch.float64),
            acc.to(torch.float64)))
    if col.dtype.kind == TypeKind.TIMESTAMP_NS:
        return Column(bt.timestamp_ns, acc)
    if col.dtype.kind == TypeKind.DATE32:
        return Column(bt.date32, acc.to(torch.int32))
    if col.dtype.kind == TypeKind.BOOL:
        return Column(bt.boolean, acc.to(torch.bool))
    return Column(col.dtype, acc.to(col.data.dtype))


def _gather_any(col: Column, idx: torch.Tensor) -> Column:
    from . import gather

    return gather(col, idx)


# ---- one aggregate per launch: agg_update ----

def _agg_launch(op: str, data, mask8, kind, row_gid, ngroups,
                want_count=False, offsets=None):
    """[acc] or [acc, cnt] of one agg_update launch with the op's identity."""
    op_id, init_f, init_i = _AGG_OPS[op]
    return kernels().agg_update(data, mask8, offsets, int(kind), row_gid,
                                ngroups, op_id, init_f, init_i, want_count)


def _agg_column(op: str, col: Column, row_gid, ngroups, want_count=False):
    data, mask8 = _data_mask8(col)
    offsets = col.offsets if col.dtype.kind == TypeKind.STRING else None
    return _agg_launch(op, data, mask8, col.dtype.kind, row_gid, ngroups,
                       want_count, offsets)


def _agg_rows(op: str, row_gid, ngroups, want_count=False):
    """An aggregate over row ids only (size, first_row, last_row).  The
    kernel's loader still reads row i of the column for every op but size,
    so the stand-in column has a zero for every row."""
    zeros = torch.zeros(int(row_gid.numel()), dtype=torch.int8,
                        device=row_gid.device)
    return _agg_launch(op, zeros, None, TypeKind.INT8, row_gid, ngroups,
                       want_count)


def _power_sums(col: Column, row_gid, ngroups, k: int):
    """(n, s1, .., sk) as float64: the valid count and the sums of the
    first k powers of the column per group.  The first launch reads the
    column in its own type and carries the count; the later ones run over
    float64 powers with the column's mask."""
    s1, cnt = _agg_column("sum_f64", col, row_gid, ngroups, want_count=True)
    x = col.data.to(torch.float64)
    mask8 = _data_mask8(col)[1]
    sums, power = [s1], x
    for _ in range(k - 1):
        power = power * x
        sums.append(_agg_launch("sum_f64", power, mask8, TypeKind.FLOAT64,
                                row_gid, ngroups)[0])
    return (cnt.to(torch.float64), *sums)


def _nan_below(n: torch.Tensor, least: int, x: torch.Tensor) -> torch.Tensor:
    return torch.where(n < least, torch.full_like(x, float("nan")), x)


def _one_count(col, row_gid, ngroups, func, uniq_rows):
    res = _agg_rows(func, row_gid, ngroups) if col is None else \
        _agg_column(func, col, row_gid, ngroups)
    return Column(bt.int64, res[1])


def _one_fusable(col, row_gid, ngroups, func, uniq_rows):
    """sum, mean, min and max launch and finish as they do in a batch."""
    rec = _fused_agg(col, func)
    res = _agg_column(rec.op, col, row_gid, ngroups, rec.want_count)
    return rec.finish(res[0], res[-1], None)


def _one_first_last(col, row_gid, ngroups, func, uniq_rows):
    acc, cnt = _agg_column(f"{func}_row", col, row_gid, ngroups,
                           want_count=True)
    has = cnt > 0
    rows = torch.where(has, acc, uniq_rows[:ngroups] if uniq_rows.numel() >= ngroups else acc)
    got = _gather_any(col, rows.clamp(min=0))
    if col.mask is None and not col.dtype.is_float and (~has).any():
        got = Column(got.dtype, got.data, has.clone(), got.offsets,
                     got.dictionary, len(got))
    return got


def _one_prod(col, row_gid, ngroups, func, uniq_rows):
    acc = _agg_column("prod_f64", col, row_gid, ngroups, want_count=True)[0]
    if col.dtype.is_float:
        return Column(bt.float64, acc)
    return Column(bt.int64, acc.to(torch.int64))


def _one_var(col, row_gid, ngroups, func, uniq_rows):
    n, s1, s2 = _power_sums(col, row_gid, ngroups, 2)
    var = _nan_below(n, 2, (s2 - s1 * s1 / n) / (n - 1))
    if func == "var":
        return Column(bt.float64, var)
    return Column(bt.float64, (var / n if func == "sem" else var).sqrt())


def _one_any_all(col, row_gid, ngroups, func, uniq_rows):
    nz = (col.data != 0).to(torch.int64)
    acc, cnt = _agg_launch("max_i64" if func == "any" else "min_i64", nz,
                           _data_mask8(col)[1], TypeKind.INT64, row_gid,
                           ngroups, want_count=True)
    default = func == "all"  # empty/all-null group: any=False, all=True
    return Column(bt.boolean, torch.where(
        cnt == 0, torch.tensor(default, device=acc.device), acc != 0))


def _one_skew(col, row_gid, ngroups, func, uniq_rows):
    n, s1, s2, s3 = _power_sums(col, row_gid, ngroups, 3)
    mean = s1 / n
    m2 = s2 / n - mean * mean
    m3 = s3 / n - 3 * mean * s2 / n + 2 * mean ** 3
    # pandas adjusted Fisher-Pearson
    g = torch.sqrt(n * (n - 1)) / (n - 2) * m3 / m2.clamp(min=0) ** 1.5
    return Column(bt.float64, _nan_below(n, 3, g))


def _one_kurt(col, row_gid, ngroups, func, uniq_rows):
    n, s1, s2, s3, s4 = _power_sums(col, row_gid, ngroups, 4)
    mean = s1 / n
    m2 = s2 / n - mean ** 2
    m4 = (s4 - 4 * mean * s3 + 6 * mean ** 2 * s2) / n - 3 * mean ** 4
    # pandas adjusted kurtosis (Fisher, bias-corrected); m2 and m4 are
    # central moments, already divided by n
    g2 = m4 / m2.clamp(min=0) ** 2 - 3
    g = (n - 1) / ((n - 2) * (n - 3)) * ((n + 1) * g2 + 6)
    return Column(bt.float64, _nan_below(n, 4, g))


_AGG_ONE = {
    "size": _one_count, "count": _one_count,
    "sum": _one_fusable, "mean": _one_fusable,
    "min": _one_fusable, "max": _one_fusable,
    "first": _one_first_last, "last": _one_first_last,
    "prod": _one_prod,
    "var": _one_var, "std": _one_var, "sem": _one_var,
    "any": _one_any_all, "all": _one_any_all,
    "skew": _one_skew, "kurt": _one_kurt,
    "median": lambda col, row_gid, ngroups, func, uniq_rows:
        _median_by_group(col, row_gid, ngroups),
    "nunique": lambda col, row_gid, ngroups, func, uniq_rows:
        _nunique_by_group(col, row_gid, ngroups),
}


def _agg_one(col: Optional[Column], row_gid: torch.Tensor, ngroups: int,
             func: str, uniq_rows: torch.Tensor, tbl: Table) -> Column:
    """One aggregate outside a fused batch, from its own launches."""
    if func not in _AGG_ONE:
        raise NotImplementedError(f"gpu agg {func}")
    return _AGG_ONE[func](col, row_gid, ngroups, func, uniq_rows)


def _median_by_group(col: Column, row_gid: torch.Tensor, ngroups: int) -> Column:
    # sort (gid, value) pairs; segmented median (device, torch-composable)
    vals = col.data.to(torch.float64)
    valid = ~torch.isnan(vals) if col.dtype.is_float else torch.ones_like(vals, dtype=torch.bool)
    if col.mask is not None:
        valid &= col.mask
    idx = torch.nonzero(valid, as_tuple=False).reshape(-1)
    v = vals[idx]
    g = row_gid[idx].to(torch.int64)
    order = torch.argsort(v, stable=True)
    g2, v2 = g[order], v[order]
    order2 = torch.argsort(g2, stable=True)
    gs, vs = g2[order2], v2[order2]
    cnt = torch.bincount(gs, minlength=ngroups)
    start = torch.zeros(ngroups, dtype=torch.int64, device=vals.device)
    torch.cumsum(cnt, 0, out=start)
    start = start - cnt
    mid = start + (cnt - 1) // 2
    mid2 = start + cnt // 2
    n_tot = int(vs.numel())
    safe_mid = mid.clamp(0, max(n_tot - 1, 0))
    safe_mid2 = mid2.clamp(0, max(n_tot - 1, 0))
    if n_tot == 0:
        return Column(bt.float64, torch.full((ngroups,), float("nan"),
                                             dtype=torch.float64, device=vals.device))
    med = (vs[safe_mid] + vs[safe_mid2]) / 2
    med = torch.where(cnt == 0, torch.full_like(med, float("nan")), med)
    return Column(bt.float64, med)


def _nunique_by_group(col: Column, row_gid: torch.Tensor,
                      ngroups: int) -> Column:
    # distinct (gid, value) pairs via a second hash groupby
    _, rows = groupby_build([Column(bt.int32, row_gid), col])
    # count valid values per group among distinct pairs
    g = row_gid[rows].to(torch.int64)
    valid = torch.ones(int(rows.numel()), dtype=torch.bool, device=rows.device)
    if col.mask is not None:
        valid &= col.mask[rows]
    if col.dtype.is_float:
        valid &= ~torch.isnan(col.data[rows])
    cnt = torch.bincount(g[valid], minlength=ngroups)
    return Column(bt.int64, cnt)


# ----------------------------------------------------------------------
# join
# ----------------------------------------------------------------------

def _unify_dict_keys(bkeys: Sequence[Column],
                     pkeys: Sequence[Column]) -> List[Column]:
    """The probe kernels compare dictionary-encoded keys by code, so a
    DICT/DICT key pair must index one dictionary: extend the probe side's
    dictionary with the build side's unseen values and remap the build
    codes into it (hashes are by value and stay as they were).  The probe
    side keeps its codes, so only one column is rewritten; concat_columns
    and the shuffle's _remap_dict_codes merge dictionaries too, but remap
    every input.

    A DICT key against a STRING key is not handled here or in the kernels
    (rows_eq2 switches on the probe column's type only); callers must bring
    both sides to one encoding first."""
    import pyarrow as pa

    out = list(bkeys)
    for i, (b, p) in enumerate(zip(bkeys, pkeys)):
        if b.dtype.kind != TypeKind.DICT or p.dtype.kind != TypeKind.DICT:
            continue
        if b.dictionary is p.dictionary or b.dictionary.equals(p.dictionary):
            continue
        merged = p.dictionary.to_pylist()
        code_of = {}
        for j, v in enumerate(merged):
            code_of.setdefault(v, j)
        remap = np.empty(len(b.dictionary), dtype=np.int32)
        for j, v in enumerate(b.dictionary.to_pylist()):
            c = code_of.get(v)
            if c is None:
                c = code_of[v] = len(merged)
                merged.append(v)
            remap[j] = c
        codes = b.data
        if len(remap):
            # the code under a null row is unspecified: clamp before indexing
            idx = b.data.long().clamp(0, len(remap) - 1)
            codes = torch.from_numpy(remap).to(b.device)[idx]
        out[i] = Column(bt.dictionary, codes, b.mask,
                        dictionary=pa.array(merged, type=pa.large_string()),
                        length=len(b))
    return out


_SIGNED_INT_KINDS = (TypeKind.INT8, TypeKind.INT16, TypeKind.INT32,
                     TypeKind.INT64)


def _widen_int_keys(bkeys: Sequence[Column], pkeys: Sequence[Column]):
    """The probe kernels read both sides of a key pair with the probe
    column's type, so a pair of signed integer keys of different widths is
    compared as int64 (the hashes are by value and do not change)."""
    bkeys, pkeys = list(bkeys), list(pkeys)
    for i, (b, p) in enumerate(zip(bkeys, pkeys)):
        if b.dtype.kind != p.dtype.kind and b.dtype.kind in _SIGNED_INT_KINDS \
                and p.dtype.kind in _SIGNED_INT_KINDS:
            bkeys[i] = Column(bt.int64, b.data.long(), b.mask, length=len(b))
            pkeys[i] = Column(bt.int64, p.data.long(), p.mask, length=len(p))
    return bkeys, pkeys


# Dense (direct-address) join: an inner join on one integer key whose build
# side is unique and spans a small range probes a lookup table indexed by
# key - min instead of hashing both sides.  BODO_AMD_DENSE_JOIN=0 turns the
# route off.
DENSE_JOIN = os.environ.get("BODO_AMD_DENSE_JOIN", "1") != "0"
DENSE_JOIN_MAX_SPAN = 1 << 22
_DENSE_JOIN_KINDS = (TypeKind.INT8, TypeKind.INT16, TypeKind.INT32,
                     TypeKind.INT64, TypeKind.DATE32)


def dense_join_eligible(bkeys: Sequence[Column], pkeys: Sequence[Column],
                        how: str) -> bool:
    """What can be told without looking at the build keys' values."""
    if how != "inner" or len(bkeys) != 1 or len(pkeys) != 1:
        return False
    b, p = bkeys[0], pkeys[0]
    if b.dtype.kind != p.dtype.kind or b.dtype.kind not in _DENSE_JOIN_KINDS:
        return False
    if b.mask is not None and p.mask is not None:
        return False  # the hash route matches a null key with a null key
    return len(b) <= DENSE_JOIN_MAX_SPAN


def _dense_join_lut(bkey: Column):
    """(lut, lo, dup) of a build key column: int32 lut[key - lo] = build
    row, -1 where no row has that key; rows with a null key are left out.
    ``dup`` is a device flag, set when two build rows share a key (the lut
    is then unusable).  None when the keys span more than
    DENSE_JOIN_MAX_SPAN.  One host sync, for the min and max."""
    dev = bkey.device
    data = bkey.data.long()
    rows = torch.arange(len(bkey), dtype=torch.int32, device=dev)
    if bkey.mask is not None:
        data, rows = data[bkey.mask], rows[bkey.mask]
    if int(data.numel()) == 0:
        return (torch.full((1,), -1, dtype=torch.int32, device=dev), 0,
                torch.zeros((), dtype=torch.bool, device=dev))
    lo, hi = torch.stack(torch.aminmax(data)).tolist()
    span = hi - lo + 1
    if span > DENSE_JOIN_MAX_SPAN:
        return None
    idx = data - lo  # wraps to [0, span) in two's complement
    per_key = torch.zeros(span, dtype=torch.int32, device=dev)
    per_key.scatter_add_(0, idx, torch.ones_like(rows))
    lut = torch.full((span,), -1, dtype=torch.int32, device=dev)
    lut[idx] = rows
    return lut, lo, (per_key > 1).any()


def _join_dense(build: Table, probe: Table, bkey: Column, pkey: Column):
    """(probe table, build table) of the matching rows in probe order, or
    None when the hash route has to run."""
    from . import take_table

    built = _dense_join_lut(bkey)
    if built is None:
        return None
    lut, lo, dup = built
    pdata, pmask8 = _data_mask8(pkey)
    out_build, misses = kernels().join_probe_dense(
        pdata, pmask8, int(pkey.dtype.kind), len(probe), lut, lo)
    n_miss, is_dup = torch.stack(
        [misses[0], dup.to(torch.int64)]).tolist()
    if is_dup:
        return None
    if n_miss:
        out_probe = torch.nonzero(out_build >= 0, as_tuple=False).reshape(-1)
        out_build = out_build[out_probe]
        probe = take_table(probe, out_probe)
    return probe, take_table(build, out_build)


def join_local(left: Table, right: Table, left_on: Sequence[str],
               right_on: Sequence[str], how: str, suffixes=("_x", "_y")) -> Table:
    from . import take_table
    from .relational import _merge_joined, _null_out

    K = kernels()
    if how == "cross":
        nl, nr = len(left), len(right)
        li = torch.arange(nl, dtype=torch.int64, device=left.device).repeat_interleave(nr)
        ri = torch.arange(nr, dtype=torch.int64, device=left.device).repeat(nl)
        lt, rt = take_table(left, li), take_table(right, ri)
        return _merge_joined(lt, rt, [], [], suffixes, how)
    # build on the right side for inner/left/semi/anti; for right join swap
    swap = how == "right"
    if swap:
        left, right = right, left
        left_on, right_on = right_on, left_on
    build, probe = right, left
    bkeys = [build.column(k) for k in right_on]
    pkeys = [probe.column(k) for k in left_on]
    bkeys = _unify_dict_keys(bkeys, pkeys)
    n_build, n_probe = len(build), len(probe)
    if DENSE_JOIN and dense_join_eligible(bkeys, pkeys, how):
        dense = _join_dense(build, probe, bkeys[0], pkeys[0])
        if dense is not None:  # inner: never swapped
            return _merge_joined(dense[0], dense[1], list(left_on),
                                 list(right_on), suffixes, how)
    bkeys, pkeys = _widen_int_keys(bkeys, pkeys)
    bh = hash_columns(bkeys) if n_build else torch.zeros(0, dtype=torch.int64, device=build.device)
    ph = hash_columns(pkeys) if n_probe else torch.zeros(0, dtype=torch.int64, device=build.device)
    heads, nxt = K.join_build(bh, n_build)
    how_id = {"inner": 0, "left": 1, "semi": 2, "anti": 3, "outer": 1,
              "right": 1}[how if not swap else "left"]
    bdatas, bmasks, boffs, bauxs, bdtypes = _col_args(bkeys)
    pdatas, pmasks, poffs, pauxs, pdtypes = _col_args(pkeys)
    track = how == "outer"
    res = K.join_probe(bdatas, bmasks, boffs, bauxs, bdtypes, n_build, bh,
                       pdatas, pmasks, poffs, pauxs, pdtypes, n_probe, ph,
                       heads, nxt, how_id, track)
    out_probe, out_build = res[0], res[1]
    if how == "semi":
        return take_table(probe, out_probe)
    if how == "anti":
        return take_table(probe, out_probe)
    if how == "outer":
        matched = res[2]
        unmatched = torch.nonzero(matched == 0, as_tuple=False).reshape(-1)
        out_probe = torch.cat([out_probe,
                               torch.full((int(unmatched.numel()),), -1,
                                          dtype=torch.int64, device=out_probe.device)])
        out_build = torch.cat([out_build, unmatched])
    # materialize (inner joins produce only valid pairs by construction;
    # skip the 1B-row .all() reductions/syncs there)
    if how == "inner":
        elide = False
        if int(out_probe.numel()) == n_probe and n_probe > 0:
            # identity iff strictly increasing (out_probe is sorted runs of
            # repeated probe ids; strict monotonic + length n => arange(n))
            elide = bool((out_probe[1:] > out_probe[:-1]).all().item())
        if elide:
            pt = probe  # every probe row matched exactly once: skip gather
        else:
            pt = take_table(probe, out_probe)
        btb = take_table(build, out_build)
    else:
        p_valid = out_probe >= 0
        b_valid = out_build >= 0
        pt = take_table(probe, out_probe.clamp(min=0))
        btb = take_table(build, out_build.clamp(min=0))
        if not bool(p_valid.all().item()):
            pt = _null_out(pt, p_valid)
        if not bool(b_valid.all().item()):
            btb = _null_out(btb, b_valid)
    if swap:
        # right join: probe side was the right table
        return _merge_joined(btb, pt, list(right_on), list(left_on), suffixes, how)
    return _merge_joined(pt, btb, list(left_on), list(right_on), suffixes, how)


def distinct_local(tbl: Table, subset=None, keep: str = "first") -> Table:
    from . import take_table

    keys = list(subset) if subset else list(tbl.names)
    key_cols = [tbl.column(k) for k in keys]
    if len(tbl) == 0:
        return tbl
    row_gid, uniq_rows = groupby_build(key_cols)
    ngroups = int(uniq_rows.numel())
    if keep == "first":
        # uniq_rows is the first CLAIMER (race order); recompute true min row
        rows = _agg_rows("first_row", row_gid, ngroups)[0]
    elif keep == "last":
        rows = _agg_rows("last_row", row_gid, ngroups)[0]
    elif keep is False:
        # drop every member of any duplicated group
        cnt = _agg_rows("size", row_gid, ngroups, want_count=True)[1]
        singles = cnt[row_gid.long()] == 1
        rows = torch.nonzero(singles, as_tuple=False).reshape(-1)
    else:
        rows = uniq_rows
    rows = torch.sort(rows).values  # preserve original row order
    return take_table(tbl, rows)


def _empty_gb_result(tbl: Table, keys, aggs) -> Table:
    from ..core.table import Table as T

    base = T.empty_like(tbl.select([k for k in keys]))
    names = list(keys)
    cols = list(base.columns)
    for out_name, in_name, func in aggs:
        dt = bt.int64 if func in ("count", "size", "nunique") else bt.float64
        cols.append(Column(dt, torch.zeros(0, dtype=bt.torch_storage_dtype(dt),
                                           device=tbl.device), length=0))
        names.append(out_name)
    return T(names, cols, 0)


def take_table_fused(tbl: Table, idx: torch.Tensor) -> Optional[Table]:
    """All fixed-width columns (+masks) of a take materialize in ONE kernel
    launch (join-heavy queries were launch-bound on per-column
    index_select; reference role: cudf::gather single pass)."""
    from . import gather as _gather

    K = kernels()
    srcs = []
    plan = []  # (col_index, has_mask)
    for i, c in enumerate(tbl.columns):
        if c.dtype.kind == TypeKind.STRING:
            plan.append((i, None))
            continue
        srcs.append(c.data)
        if c.mask is not None:
            srcs.append(c.mask)
            plan.append((i, True))
        else:
            plan.append((i, False))
    if len(srcs) < 2:
        return None
    outs = K.gather_multi(srcs, idx)
    n = int(idx.numel())
    cols = []
    k = 0
    for i, has_mask in plan:
        c = tbl.columns[i]
        if has_mask is None:
            cols.append(_gather(c, idx))
            continue
        data = outs[k]
        k += 1
        mask = None
        if has_mask:
            mask = outs[k]
            k += 1
        out = Column(c.dtype, data, mask, dictionary=c.dictionary, length=n)
        out.val_range = c.val_range
        cols.append(out)
    return Table(tbl.names, cols, n)
