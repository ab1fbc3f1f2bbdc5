"""LIKE without a GPU: segment split, str_op "like" against ``re``, lowering."""

import re

import pyarrow as pa
import pytest

from bodo_amd.core.column import Column
from bodo_amd.ops.evaluate import str_op
from bodo_amd.ops.gpu import like_segments
from bodo_amd.plan import expr as ex
from bodo_amd.sql.planner import _like_expr

ROWS = ["xa\nb", None, "ab", "ba", "", "a.b", "special packages requests",
        "requests special", "PROMO BRASS", "a%b"]


@pytest.mark.parametrize("pattern,want", [
    ("%special%requests%", ([b"special", b"requests"], False, False)),
    ("PROMO%", ([b"PROMO"], True, False)),
    ("%BRASS", ([b"BRASS"], False, True)),
    ("a%%b", ([b"a", b"b"], True, True)),
    ("%", ([], False, False)), ("", ([], True, True))])
def test_like_segments(pattern, want):
    assert like_segments(pattern) == want


@pytest.mark.parametrize("dictionary", [False, True])
@pytest.mark.parametrize("pattern", [
    "%a%b%", "a%b", "%special%requests%", "PROMO%BRASS", "a.%", "%", "", "%%b"])
def test_str_op_like(pattern, dictionary):
    arr = pa.array(ROWS, type=pa.large_string())
    col = Column.from_arrow(arr.dictionary_encode() if dictionary else arr)
    segs, anchor_start, anchor_end = like_segments(pattern)
    rx = re.compile(b"(?s)" + (b"" if anchor_start else b".*")
                    + b".*".join(map(re.escape, segs))
                    + (b"" if anchor_end else b".*"))
    want = [None if r is None else rx.fullmatch(r.encode()) is not None
            for r in ROWS]
    got = str_op(col, "like", (pattern,)).to_pandas()
    assert got.astype(object).where(got.notna(), None).tolist() == want


def test_like_expr_forms():
    ops = {p: _like_expr(ex.ColRef("c"), p) for p in
           ("%x%", "x%", "%x", "x", "%x%y%", "x%y", "%x_y%")}
    assert [(ops[p].op, ops[p].args) for p in ("%x%", "x%", "%x")] == [
        ("contains", ("x",)), ("startswith", ("x",)), ("endswith", ("x",))]
    assert isinstance(ops["x"], ex.Cmp) and ops["x"].op == "eq"
    assert (ops["%x%y%"].op, ops["%x%y%"].args) == ("like", ("%x%y%",))
    assert (ops["x%y"].op, ops["x%y"].args) == ("like", ("x%y",))
    assert ops["%x_y%"].op == "contains_re"
