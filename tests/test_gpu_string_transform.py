"""csrc/strxform.hip, direct and through str_op, the evaluator and SQL,
against plain Python on the decoded rows."""

import numpy as np
import pandas as pd
import pytest
import torch

from bodo_amd import config
from bodo_amd.core import types as bt
from bodo_amd.core.column import Column
from bodo_amd.core.table import Table
from bodo_amd.ops import gpu
from bodo_amd.ops.evaluate import eval_expr, str_op
from bodo_amd.plan.expr import BinOp, ColRef, Const

pytestmark = pytest.mark.gpu
L = getattr(gpu._K, "STRXFORM_LDS_BYTES", 32768)
STRIPS = [("strip", ()), ("lstrip", ()), ("rstrip", ())]
OPS = [("len", ()), ("lower", ()), ("upper", ())] + STRIPS + \
    [("slice", (1, 4, 1)), ("slice", (-3, None, 1)), ("slice", (2, -2))]
PAIRS = [(0, 3), (-3, None), (1, -1), (2, 100), (-100, 2), (3, 1), (0, None)]
WS = [9, 10, 11, 12, 13, 28, 29, 30, 31, 32]


def _col(rows, mask=None, device="cuda"):
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    data = np.frombuffer(b"".join(rows), np.uint8).copy()
    return Column(bt.string, torch.from_numpy(data).to(device),
                  None if mask is None else torch.from_numpy(mask).to(device),
                  offsets=torch.from_numpy(offs).to(device), length=len(rows))


def _random_rows(n, lo, hi, seed=0):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(list(b"aBc \t"), rng.integers(lo, hi + 1)).tolist())
            for _ in range(n)]


def _ref(row, op, args):
    s = row.decode()
    if op == "len":
        return len(s)
    if op == "slice":
        return s[args[0]:args[1] if len(args) > 1 else None].encode()
    return getattr(s, op)().encode()


def _same_strings(got, want, mask, null_bytes=False):
    """`got` holds exactly the rows `want` (bytes), empty where null unless
    `null_bytes`: lower and upper share the source's offsets, so what a null
    row held is mapped like the rest."""
    if mask is not None and not null_bytes:
        want = [w if ok else b"" for w, ok in zip(want, mask)]
    offs = np.zeros(len(want) + 1, np.int64)
    np.cumsum([len(w) for w in want], out=offs[1:])
    assert got.dtype == bt.string and len(got) == len(want)
    assert got.offsets.cpu().numpy().tolist() == offs.tolist()
    assert bytes(got.data.cpu().numpy()) == b"".join(want)
    assert (got.mask is None) if mask is None else \
        got.mask.cpu().numpy().tolist() == mask.tolist()


def _check(rows, op, args=(), mask=None, **kw):
    got = gpu.string_transform(_col(rows, mask), op, args, **kw)
    want = [_ref(r, op, args) for r in rows]
    if op != "len":
        return _same_strings(got, want, mask, op in ("lower", "upper"))
    if mask is not None:
        want = np.where(mask, want, 0)
        assert got.mask.cpu().numpy().tolist() == mask.tolist()
    assert got.dtype == bt.int64 and got.data.cpu().tolist() == list(want)


def _check_concat(a, b, mask_a=None, mask_b=None, **kw):
    """a, b: lists of rows, or bytes for a literal."""
    n = len(b if isinstance(a, bytes) else a)
    side = [x if isinstance(x, bytes) else _col(x, m)
            for x, m in ((a, mask_a), (b, mask_b))]
    rows = [[x] * n if isinstance(x, bytes) else x for x in (a, b)]
    masks = [m for m in (mask_a, mask_b) if m is not None]
    _same_strings(gpu.string_concat(*side, **kw),
                  [x + y for x, y in zip(*rows)],
                  np.logical_and.reduce(masks) if masks else None)


@pytest.mark.parametrize("max_blocks", [2048, 2])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 + 17])
def test_row_counts(n, max_blocks):
    rows = _random_rows(n, 0, 40, seed=n)
    for op, args in OPS:
        _check(rows, op, args, max_blocks=max_blocks)
        _check([b""] * n, op, args, max_blocks=max_blocks)
    other = _random_rows(n, 0, 40, seed=n + 1)
    for a, b in ((rows, other), (rows, b"-x"), (b"-x", rows), (rows, b""),
                 ([b""] * n, [b""] * n)):
        _check_concat(a, b, max_blocks=max_blocks)


def _stage_rows(total, seed):
    """Two tiles: 257 bytes, so the second starts misaligned to 16 in the
    source and, its first row trimmed or not, in the output, then `total`."""
    per = (total - 2) // 256
    return [b" c"] + [b"c"] * 255 + _random_rows(255, per, per, seed) + \
        [b" " + b"X" * (total - 255 * per - 2) + b" "]


@pytest.mark.parametrize("total", [L - 1, L, L + 1])
def test_stage_boundary(total):
    rows = _stage_rows(total, total)
    for op, args in OPS:
        _check(rows, op, args)
    for a, b in ((rows, b"-"), (b"", rows)):
        _check_concat(a, b)


@pytest.mark.parametrize("ta,tb", [(L // 2, L // 2), (L // 2, L // 2 + 1),
                                   (L - 300, 300), (L - 300, 301)])
def test_concat_stage_boundary(ta, tb):
    # each source tile fits the stage; together they fit or just do not
    _check_concat(_stage_rows(ta, 1), _stage_rows(tb, 2))


def test_long_row():
    # a row of 3 L bytes: its tile takes the wave-per-row paths
    body = ("a" + "é" * 40 + "Z" * (3 * L - 85)).encode()
    long_row = b" \t" + body + b"\n "
    ncp = len(long_row.decode())
    rows = _random_rows(40, 0, 40) + [long_row] + \
        [b" ab ", b"", b"\t"] + _random_rows(300, 0, 40, seed=1)
    for op, args in [("len", ())] + STRIPS + [
            ("slice", b) for b in [(0, 63), (63, 65), (64, None), (65, -1),
                                   (-1, None), (ncp - 1, ncp), (-ncp, 1)]]:
        _check(rows, op, args)
    ascii_rows = [r.replace("é".encode(), b"eE") for r in rows]
    _check(ascii_rows, "lower")
    _check(ascii_rows, "upper")
    _check_concat(rows, ascii_rows)
    _check_concat(b"<", rows)


def test_hand_built_strip():
    rows = [bytes([w]) + b"ab" + bytes([w]) for w in WS] + \
        [b"\x1ba\x1b", b"!a!", bytes(WS), b"", b"  ", b" a b ", b"\t\n a"]
    for op, args in STRIPS:
        _check(rows, op, args)


@pytest.mark.parametrize("start,stop", PAIRS)
def test_hand_built_slice(start, stop):
    rows = [s.encode() for s in
            ["héllo wörld", "日本語", "\U0001F600a\U0001F600é", "ab", ""]]
    _check(rows, "slice", (start, stop, 1))
    _check(rows, "len")


def _as_list(col):
    return col.to_device("cpu").to_arrow().to_pylist()


@pytest.mark.parametrize("op,rows", [
    ("upper", ["straße", "abc"]), ("lower", ["STRAßE", "ABC"]),
    ("strip", ["\u00a0ab\u00a0", " x "]), ("rstrip", ["ab\u00a0", "x"])])
def test_fallback(op, rows):
    rows = [r.encode() for r in rows]
    assert gpu.string_transform(_col(rows), op) is None
    assert _as_list(str_op(_col(rows), op, ())) == \
        _as_list(str_op(_col(rows, device="cpu"), op, ()))


def test_interior_multibyte_stays_on_device():
    rows = [s.encode() for s in [" héllo ", "\ta日本語b\n", "x日 本y", ""]]
    for op, args in STRIPS:
        _check(rows, op, args)


def _plain(device, seed=3):
    rows = _random_rows(700, 0, 40, seed=seed) + [b" a\nB ", b"", b"  "]
    mask = np.random.default_rng(seed + 1).random(len(rows)) > 0.2
    return _col(rows, mask, device), rows, mask


def test_nulls():
    _, rows, mask = _plain("cuda")
    _, other, mask2 = _plain("cuda", seed=7)
    for op, args in OPS:
        _check(rows, op, args, mask)
    _check_concat(rows, other, mask, None)
    _check_concat(rows, other, None, mask2)
    _check_concat(rows, other, mask, mask2)
    _check_concat(b"x", rows, None, mask)


@pytest.mark.parametrize("route", [True, False])
@pytest.mark.parametrize("op,args", OPS)
def test_str_op_equals_cpu(op, args, route, monkeypatch):
    monkeypatch.setattr(config, "STRING_TRANSFORM", route)
    got = str_op(_plain("cuda")[0], op, args)
    assert got.is_cuda
    assert _as_list(got) == _as_list(str_op(_plain("cpu")[0], op, args))


@pytest.mark.parametrize("route", [True, False])
@pytest.mark.parametrize("expr", [
    BinOp("concat", ColRef("a"), ColRef("b")),
    BinOp("concat", ColRef("a"), Const("-x")),
    BinOp("concat", Const("-x"), ColRef("b"))])
def test_evaluator_concat_equals_cpu(expr, route, monkeypatch):
    monkeypatch.setattr(config, "STRING_TRANSFORM", route)
    got, want = [eval_expr(expr, Table(["a", "b"], [_plain(dev)[0],
                                                    _plain(dev, 7)[0]]))
                 for dev in ("cuda", "cpu")]
    assert got.is_cuda and _as_list(got) == _as_list(want)


def test_sql_end_to_end(monkeypatch):
    from bodo_amd.sql import BodoSQLContext

    monkeypatch.setattr(config, "DEVICE", "cuda")
    n = 70_001  # past the size below which every string column is encoded
    rows = [" " * (i % 3) + r.decode() + str(i) + " " * (i % 2)
            for i, r in enumerate(_random_rows(n, 0, 12, seed=5))]
    df = pd.DataFrame({"c": rows})
    got = BodoSQLContext({"t": df}).sql(
        "SELECT UPPER(TRIM(c)) || '-' || SUBSTR(c, 2, 3), LENGTH(c) FROM t"
    ).to_pandas()
    want = df.c.str.strip().str.upper() + "-" + df.c.str.slice(1, 4)
    assert got.iloc[:, 0].tolist() == want.tolist()
    assert got.iloc[:, 1].tolist() == df.c.str.len().tolist()
