"""csrc/strmatch.hip, direct and through str_op and SQL, against ``re``."""

import re

import numpy as np
import pandas as pd
import pytest
import torch

from bodo_amd import config
from bodo_amd.core import types as bt
from bodo_amd.core.column import Column
from bodo_amd.ops import gpu
from bodo_amd.ops.evaluate import str_op

pytestmark = pytest.mark.gpu
L = getattr(gpu._K, "STRMATCH_LDS_BYTES", 32768)
LONG = 3 * L
NINE = "%".join("abcabcabc")  # nine segments, more than the kernel takes
ANCHORS = [(s, e) for s in (False, True) for e in (False, True)]


def _ref(rows, segs, anchor_start, anchor_end, mask=None):
    rx = re.compile(b"(?s)" + (b"" if anchor_start else b".*")
                    + b".*".join(map(re.escape, segs))
                    + (b"" if anchor_end else b".*"))
    out = np.array([rx.fullmatch(r) is not None for r in rows])
    return torch.from_numpy(out if mask is None else out & mask)


def _col(rows, mask=None, device="cuda"):
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    data = np.frombuffer(b"".join(rows), np.uint8).copy()
    return Column(bt.string, torch.from_numpy(data).to(device),
                  None if mask is None else torch.from_numpy(mask).to(device),
                  offsets=torch.from_numpy(offs).to(device), length=len(rows))


def _random_rows(n, lo, hi, seed=0):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(list(b"abc"), rng.integers(lo, hi + 1)).tolist())
            for _ in range(n)]


def _check(rows, segs, anchor_start, anchor_end, mask=None, **kw):
    got = gpu.string_match(_col(rows, mask), segs, anchor_start, anchor_end,
                           **kw)
    want = _ref(rows, segs, anchor_start, anchor_end, mask)
    assert got.dtype == torch.bool and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("segs", [[b"ab"], [b"ab", b"ca"], [b"a", b"a", b"a"]])
@pytest.mark.parametrize("max_blocks", [2048, 2])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 + 17])
def test_row_counts(n, max_blocks, segs):
    rows = _random_rows(n, 0, 40, seed=n)
    for anchor_start, anchor_end in ANCHORS:
        _check(rows, segs, anchor_start, anchor_end, max_blocks=max_blocks)


X = [b"x"] * 255
ENDS = [b"abxx", b"xxab", b"xabx"]
JP = ["日本語".encode(), "語日本".encode(), "日x本".encode()]
LF = [b"xa\nb", b"a\n\nb", b"\na\nb\n", b"b\na"]
HAND = [
    ([b"", b"a", b"ab"], [b"ab"], False, False),   # empty, shorter, equal
    (ENDS, [b"ab"], False, False), (ENDS, [b"ab"], True, False),
    (ENDS, [b"ab"], False, True), (LF, [b"a", b"b"], False, False),
    ([b"ab", b"abx", b"xab"], [b"ab"], True, True),  # equality
    ([b"ab", b"cd", b"abcd"], [b"bc"], False, False),  # row boundary
    (X + [b"ab", b"cd"], [b"bc"], False, False),       # tile boundary
    (X + [b"ab", b"cd"], [b"ab"], False, True),
    (X + [b"ab", b"cd"], [b"cd"], True, False),
    ([b"ababa", b"abaaba", b"abaxaba"], [b"aba", b"aba"], True, True),
    ([b"abab", b"ab", b"aba"], [b"ab"], False, True),   # not the leftmost hit
    ([b"a", b"aa", b"aba"], [b"a", b"a"], True, True),  # no overlap at the end
    ([b"aaab", b"aab", b"aaaa"], [b"aab"], False, False),
    (["cafés".encode(), b"\xc3"] + JP, ["é".encode()], False, False),
    (JP, ["日本".encode()], False, False),
    (JP, ["日".encode(), "本".encode()], True, True),
    (LF, [b"a", b"b"], True, True)]


@pytest.mark.parametrize("rows,segs,anchor_start,anchor_end", HAND)
def test_hand_built(rows, segs, anchor_start, anchor_end):
    _check(rows, segs, anchor_start, anchor_end)


@pytest.mark.parametrize("anchor_end", [False, True])
@pytest.mark.parametrize("total", [L - 1, L, L + 1])
def test_stage_boundary(total, anchor_end):
    # the second tile starts at byte 257, misaligned to 16, and ends in 'ab'
    first = [b"cc"] + [b"c"] * 255
    per = (total - 2) // 256
    rows = first + _random_rows(255, per, per, seed=total) + \
        [b"c" * (total - 255 * per - 2) + b"ab"]
    _check(rows, [b"ab"], False, anchor_end)
    _check(rows, [b"b", b"ab"], False, anchor_end)


@pytest.mark.parametrize("where,segs", [
    ([(0, b"ab")], [b"ab"]), ([(63, b"ab")], [b"ab"]), ([(64, b"ab")], [b"ab"]),
    ([(65, b"ab")], [b"ab"]), ([(LONG - 2, b"ab")], [b"ab"]), ([], [b"ab"]),
    ([(10, b"ab"), (200, b"cd")], [b"ab", b"cd"]),
    ([(10, b"ab"), (LONG - 2, b"cd")], [b"ab", b"cd"]),
    ([(200, b"ab"), (10, b"cd")], [b"ab", b"cd"]),
])
def test_long_rows(where, segs):
    # a row of 3 L bytes: its tile takes the wave-per-row path
    long_row = bytearray(b"x" * LONG)
    for pos, lit in where:
        long_row[pos:pos + len(lit)] = lit
    rows = _random_rows(40, 0, 40) + [bytes(long_row)] + \
        [b"abcd", b"cdab", b"", b"ab"] + _random_rows(300, 0, 40, seed=1)
    for anchor_start, anchor_end in ANCHORS:
        _check(rows, segs, anchor_start, anchor_end)


def _plain(device):
    rows = _random_rows(700, 0, 40, seed=3) + [b"xa\nb", b"", b"ab%c"]
    mask = np.random.default_rng(4).random(len(rows)) > 0.2
    return _col(rows, mask, device), rows, mask


def test_nulls():
    col, rows, mask = _plain("cuda")
    _check(rows, [b"a", b"b"], False, False, mask)
    out = str_op(col, "like", ("%a%b%",))
    assert out.mask is col.mask and not out.data[~col.mask].any()


@pytest.mark.parametrize("route", [True, False])
@pytest.mark.parametrize("op,pat", [
    ("contains", "ab"), ("contains", "%"), ("startswith", "ab"),
    ("endswith", "ab"), ("startswith", ""), ("like", "%a%b%"),
    ("like", "ab%c"), ("like", "%"), ("like", ""), ("like", NINE)])
def test_str_op_equals_cpu(op, pat, route, monkeypatch):
    monkeypatch.setattr(config, "STRING_MATCH", route)
    col, rows, mask = _plain("cuda")
    got = str_op(col, op, (pat,))
    want = str_op(_plain("cpu")[0], op, (pat,))
    assert got.data.is_cuda and torch.equal(got.mask.cpu(), want.mask)
    assert torch.equal((got.data & got.mask).cpu(), want.data & want.mask)


@pytest.mark.parametrize("neg", ["", "NOT "])
def test_sql_like(neg, monkeypatch):
    from bodo_amd.sql import BodoSQLContext

    monkeypatch.setattr(config, "DEVICE", "cuda")
    n = 70_000  # past the size below which every string column is encoded
    rows = [r.decode() + str(i) for i, r in
            enumerate(_random_rows(n, 0, 12, seed=5))]
    rows[7] = "a\nc"
    df = pd.DataFrame({"i": np.arange(n), "c": rows})
    got = BodoSQLContext({"t": df}).sql(
        f"SELECT i FROM t WHERE c {neg}LIKE '%a%c%'").to_pandas()
    hit = df.c.str.contains("a.*c", regex=True, flags=re.S) ^ bool(neg)
    assert sorted(got["i"].tolist()) == df.i[hit].tolist()
