"""The decode-stream route on the GPU: a group's decode kernels run on the
extension's own stream while the reader goes on uploading.  Row groups of
2^12 rows, shards of 1, 3 and 9 of them, groups of 1 and 2 row groups; the
tables must equal pyarrow's and, bit for bit, those of the route off."""

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from tests.test_parquet_direct_decode_gpu import _bits, _page

pytestmark = pytest.mark.gpu

RG = 1 << 12
WORDS = ["alpha", "beta", "gamma", "delta", "epsilon"]


def _table(n_rgs, nullable):
    rng = np.random.default_rng(1000 + n_rgs)
    n = n_rgs * RG
    cols = {
        "i": pa.array(rng.integers(-10**12, 10**12, n), type=pa.int64()),
        "f": pa.array(rng.random(n), type=pa.float64()),
        "s": pa.array(rng.choice(WORDS, n).tolist(), type=pa.string()),
    }
    if nullable:
        cols["nul"] = pa.array(rng.integers(0, 10**6, n), type=pa.int64(),
                               mask=rng.random(n) < 0.2)
    return pa.table(cols)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    """(n_rgs, nullable) -> (directory, the table as pyarrow reads it)."""
    out = {}
    for n_rgs in (1, 3, 9):
        for nullable in (False, True):
            d = tmp_path_factory.mktemp(f"ds{n_rgs}{int(nullable)}")
            path = str(d / "part-00000.parquet")
            pq.write_table(_table(n_rgs, nullable), path, row_group_size=RG,
                           compression="SNAPPY", use_dictionary=["s"],
                           data_page_size=4096)
            assert pq.ParquetFile(path).metadata.num_row_groups == n_rgs
            out[n_rgs, nullable] = (str(d), pq.read_table(path))
    return out


def _read(g, path):
    from bodo_amd.engine.executor import ExecutionContext

    ctx = ExecutionContext("cuda")
    ctx.world, ctx.rank = 1, 0
    t = g.read_shard_gpu(path, None, ctx)
    assert t is not None, "GPU decode fell back"
    return t


def _assert_same(on, off):
    assert on.names == off.names
    for name in on.names:
        a, b = on.column(name), off.column(name)
        assert a.val_range == b.val_range, name
        if a.dictionary is not None:
            assert a.dictionary.to_pylist() == b.dictionary.to_pylist()
        assert a.data.dtype == b.data.dtype, name
        assert torch.equal(a.data.view(dtype=_bits(a.data)),
                           b.data.view(dtype=_bits(b.data))), name
        assert (a.mask is None) == (b.mask is None), name
        if a.mask is not None:
            assert torch.equal(a.mask, b.mask), name


def _assert_equals_pyarrow(t, ref_tbl):
    ref = ref_tbl.to_pandas()
    out = t.to_pandas()
    for c in out.columns:
        if out[c].dtype.name == "category":
            out[c] = out[c].astype(object)
    assert list(out.columns) == list(ref.columns) and len(out) == len(ref)
    for c in ref.columns:
        a, b = out[c], ref[c]
        assert (a.isna().to_numpy() == b.isna().to_numpy()).all(), c
        ok = ~b.isna().to_numpy()
        assert (a.to_numpy()[ok] == b.to_numpy()[ok]).all(), c


@pytest.mark.parametrize("nullable", [False, True],
                         ids=["all_direct", "with_nullable"])
@pytest.mark.parametrize("group", [1, 2], ids=["g1", "g2"])
@pytest.mark.parametrize("n_rgs", [1, 3, 9])
def test_route_on_matches_pyarrow_and_route_off(shards, n_rgs, group,
                                                nullable, monkeypatch):
    import bodo_amd_kernels as K

    from bodo_amd.io import parquet_gpu as g

    path, ref = shards[n_rgs, nullable]
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", group)
    monkeypatch.setattr(g, "DECODE_STREAM", True)
    calls = []
    group_call = K.pq_decode_group
    monkeypatch.setattr(K, "pq_decode_group",
                        lambda *a: calls.append(1) or group_call(*a))
    before = dict(g.STATS)
    on = _read(g, path)
    assert len(calls) == -(-n_rgs // group)
    assert g.STATS["slow"] == before["slow"]
    assert g.STATS["direct"] == before["direct"] + 3 * n_rgs
    _assert_equals_pyarrow(on, ref)
    if nullable:
        assert on.column("nul").mask is not None
    monkeypatch.setattr(g, "DECODE_STREAM", False)
    off = _read(g, path)
    assert len(calls) == -(-n_rgs // group)
    _assert_same(on, off)


def test_buffers_of_an_undecoded_group_are_not_reused(shards, monkeypatch):
    """20 reads of the 9-row-group shard in groups of 1, with tensors of
    the chunk buffers' sizes allocated, filled and freed in between: the
    allocator has blocks of exactly those sizes to hand to a later group's
    uploads, and may do so only after the decode that reads them."""
    from bodo_amd.io import parquet_gpu as g

    path, ref = shards[9, False]
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", 1)
    monkeypatch.setattr(g, "DECODE_STREAM", True)
    md = pq.ParquetFile(path + "/part-00000.parquet").metadata
    sizes = sorted({g._chunk_range(md.row_group(r).column(c))[1]
                    for r in range(md.num_row_groups)
                    for c in range(md.num_columns)})
    first = _read(g, path)
    _assert_equals_pyarrow(first, ref)
    for i in range(19):
        junk = [torch.full((s,), 0xA5, dtype=torch.uint8, device="cuda")
                for s in sizes for _ in range(2)]
        del junk
        _assert_same(_read(g, path), first)


def test_error_word_still_takes_the_retry(shards, monkeypatch):
    """A page whose definition levels hold a 0 (page A of the direct-decode
    tests) goes through pq_values_multi against the reader's error word
    just before the first group's decode: the read must see the word after
    its groups ran on the decode stream, read again without the direct
    path, and give the right table."""
    import bodo_amd_kernels as K

    from bodo_amd.io import parquet_gpu as g

    path, ref = shards[3, False]
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", 1)
    monkeypatch.setattr(g, "DECODE_STREAM", True)
    vals = np.arange(1, 9, dtype=np.int64)
    page = _page(bytes([3, 0b11110111]), 2, vals.tobytes())
    scratch_np = np.zeros(((len(page) + 7) & ~7) + 16, dtype=np.uint8)
    scratch_np[:len(page)] = np.frombuffer(page, dtype=np.uint8)
    scratch = torch.from_numpy(scratch_np).to("cuda")
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    tbl = np.zeros(1, dtype=g._VALPAGE_DT)
    tbl["page"], tbl["out"] = scratch.data_ptr(), out.data_ptr()
    tbl["dst_len"], tbl["nv"], tbl["kind"] = len(page), 8, 8
    tbl["flags"] = g._PQF_HAS_DEF
    bad = torch.from_numpy(tbl.view(np.uint8)).to("cuda")
    group_call = K.pq_decode_group
    calls = []

    def pq_decode_group(blob, dec_bytes, n_dec, val_bytes, n_val, err,
                        tensors):
        if not calls:
            K.pq_values_multi(bad, 1, err)
        calls.append(n_val)
        return group_call(blob, dec_bytes, n_dec, val_bytes, n_val, err,
                          tensors)

    monkeypatch.setattr(K, "pq_decode_group", pq_decode_group)
    before = dict(g.STATS)
    t = _read(g, path)
    # three direct groups, then three of the retry with no values pages
    assert [bool(n) for n in calls] == [True] * 3 + [False] * 3
    assert g.STATS["direct"] == before["direct"]
    assert not bool(out.any())  # the bad page was not written
    _assert_equals_pyarrow(t, ref)
