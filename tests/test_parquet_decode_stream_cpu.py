"""The decode-stream route of the pipelined shard reader on the CPU.

K.pq_decode_group and K.pq_decode_join get a stand-in that behaves like a
stream: a group's simulated kernels are only queued by pq_decode_group and
run, in order, when something waits for the group (pq_decode_join, or the
host in throttle).  A reader that touches a group's results without joining
therefore sees memory the decode has not written, and the error word is
set only once the group has run.  The simulators resolve every address
through the `tensors` list of the call alone, so a tensor missing from it
is an assertion here, where it would be a reused buffer on the GPU.  Every
call goes into one log whose order the tests check."""

import numpy as np
import pytest
import torch

from tests import kernel_sim as ks
from tests.parquet_shards import (DIRECT_COLS, N_FILES, RG_ROWS, SCHEMA,
                                  write_shard)
from tests.test_parquet_batched_sim import _ctx
from tests.test_parquet_pipelined_sim import (_assert_same_table, _Harness,
                                              _pieces, _within_limit)

N_RGS = N_FILES * len(RG_ROWS)


class _Done:
    """Stand-in for the event pq_decode_group returns."""

    def __init__(self, stream, k):
        self.stream, self.k = stream, k

    def synchronize(self):
        self.stream.log.append(("host_wait", self.k))
        self.stream.run_through(self.k)


class _DecodeStream:
    def __init__(self, g, log):
        self.g, self.log = g, log
        self.pending = []  # (group number, closure), in queue order
        self.n_groups = 0
        self.poison_first = False

    def decode_group(self, blob, dec_bytes, n_dec, val_bytes, n_val, err,
                     tensors):
        g, k = self.g, self.n_groups
        self.n_groups += 1
        self.log.append(("decode_group", k))
        assert dec_bytes == n_dec * g._PAGEPTR_DT.itemsize
        assert val_bytes == n_val * g._VALPAGE_DT.itemsize
        assert dec_bytes + val_bytes <= blob.numel()
        assert n_val == 0 or err is not None
        amap = ks.AddressMap()  # holds the tensors until the group has run
        for t in tensors:
            amap.add(t)

        def run():
            self.log.append(("run", k))
            b = blob.numpy()
            ks.sim_decompress_multi(b[:dec_bytes].view(g._PAGEPTR_DT), amap)
            if n_val:
                ks.sim_values_multi(
                    b[dec_bytes:dec_bytes + val_bytes].view(g._VALPAGE_DT),
                    amap, err.numpy())
            if self.poison_first and k == 0:
                err.numpy()[0] |= ks.PQE_LEVELS

        self.pending.append((k, run))
        return _Done(self, k)

    def run_through(self, k):
        while self.pending and self.pending[0][0] <= k:
            self.pending.pop(0)[1]()

    def join(self, done):
        self.log.append(("join", done.k))
        self.run_through(done.k)


class _Rig:
    """The sim harness plus the decode-stream stand-in and the call log."""

    def __init__(self, g, mp, n_slots=3):
        self.g, self.log = g, []
        mp.setattr(g, "_NSLOTS", n_slots)
        self.harness = _Harness(g)
        self.stream = _DecodeStream(g, self.log)
        m = self.harness.module()
        dm, vm = m.pq_decompress_multi, m.pq_values_multi
        log = self.log

        def pq_decompress_multi(*a):
            log.append(("decompress_multi",))
            dm(*a)

        def pq_values_multi(*a):
            log.append(("values_multi",))
            vm(*a)

        m.pq_decompress_multi = pq_decompress_multi
        m.pq_values_multi = pq_values_multi
        m.pq_decode_group = self.stream.decode_group
        m.pq_decode_join = self.stream.join
        self.harness.module = lambda: m
        self.harness.install(mp)
        # the route follows the flag alone: there is no CUDA device here
        mp.setattr(g, "_decode_stream_on", lambda device: g.DECODE_STREAM)

        upload, finish, impl = (g._upload_staged, g._GroupDecoder._finish,
                                g._read_pieces_impl)

        def _upload_staged(staging, np_u8, dev_out):
            if staging is g._TABLE_STAGING:
                log.append(("table",))
            upload(staging, np_u8, dev_out)

        def _finish(dec, e):
            if e.prep is not None and e.direct is None:
                log.append(("finish", e.name))
            finish(dec, e)

        def _read_pieces_impl(my, columns, ctx, direct):
            log.append(("read", direct))
            try:
                return impl(my, columns, ctx, direct)
            finally:
                # where the error word is read, and on every other way out
                log.append(("read_end", direct))

        mp.setattr(g, "_upload_staged", _upload_staged)
        mp.setattr(g._GroupDecoder, "_finish", _finish)
        mp.setattr(g, "_read_pieces_impl", _read_pieces_impl)

    def calls(self):
        """The log without the stand-in's own notes of when a group ran."""
        return [e for e in self.log if e[0] != "run"]

    def kinds(self):
        return [e[0] for e in self.log]


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    d, ref = write_shard(tmp_path_factory.mktemp("dstream"))
    return d, ref


@pytest.fixture
def rig(monkeypatch):
    from bodo_amd.io import parquet_gpu as g

    monkeypatch.setattr(g, "DECODE_STREAM", True)
    return _Rig(g, monkeypatch)


def _ref_rows(ref, rgs):
    """The rows of row groups rgs (indices into the shard's six) as pandas."""
    import pyarrow as pa

    sizes = list(RG_ROWS) * N_FILES
    starts = np.cumsum([0] + sizes)
    return pa.concat_tables(
        [ref.slice(int(starts[r]), sizes[r]) for r in rgs]).to_pandas()


def _assert_equals_pyarrow(t, ref):
    out = t.to_pandas()
    for c in out.columns:
        if out[c].dtype.name == "category":
            out[c] = out[c].astype(object)
    assert list(out.columns) == list(ref.columns)
    assert len(out) == len(ref)
    for c in ref.columns:
        a, b = out[c], ref[c]
        if b.dtype.name == "category":
            b = b.astype(object)
        assert (a.isna().to_numpy() == b.isna().to_numpy()).all(), c
        ok = ~b.isna().to_numpy()
        assert (a.to_numpy()[ok] == b.to_numpy()[ok]).all(), c


def _check_order(log, all_direct):
    """The order every read on the route must keep."""
    n_table = 0
    decoded = -1  # last group handed to the decode stream
    joined = -1  # groups up to here are waited for by the current stream
    for e in log:
        if e[0] == "table":
            n_table += 1
        elif e[0] == "decode_group":
            decoded = e[1]
            # issued after its own table upload, and one upload per group
            assert n_table == decoded + 1, log
        elif e[0] == "join":
            joined = max(joined, e[1])
        elif e[0] == "finish":
            assert not all_direct
            assert joined == decoded, f"_finish before the join: {log}"
        elif e[0] == "read_end":
            assert joined == decoded, f"read left without a join: {log}"
        elif e[0] in ("decompress_multi", "values_multi"):
            raise AssertionError(f"a launch on the current stream: {log}")
    assert decoded >= 0


# 1, 2, 3 and 5 groups at both group sizes; a row group index past the
# shard's six reads that row group again, and an odd count leaves the last
# group of two half full
CASES = [(1, [0]), (1, [0, 1]), (1, [1, 2, 3]), (1, [0, 1, 2, 3, 4]),
         (2, [0]), (2, [0, 1, 2, 3]), (2, [0, 1, 2, 3, 4]),
         (2, [0, 1, 2, 3, 4, 5, 0, 1, 2])]
N_GROUPS = [1, 2, 3, 5, 1, 2, 3, 5]


@pytest.mark.parametrize("columns", [None, DIRECT_COLS],
                         ids=["mixed", "all_direct"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_route_on_matches_pyarrow_and_keeps_order(shard, rig, monkeypatch,
                                                  case, columns):
    g = rig.g
    group, rgs = CASES[case]
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", group)
    path, ref = shard
    pieces = _pieces(path)
    my = [pieces[r] for r in rgs]
    before = dict(g.STATS)
    t = _within_limit(lambda: g._read_pieces_pipelined(my, columns, _ctx()))
    assert t is not None
    n_cols = len(columns or SCHEMA.names)
    assert g.STATS["slow"] == before["slow"]
    assert g.STATS["direct"] == before["direct"] + len(rgs) * len(DIRECT_COLS)
    assert g.STATS["batched"] == before["batched"] + len(rgs) * n_cols
    want = _ref_rows(ref, rgs)
    _assert_equals_pyarrow(t, want[columns] if columns else want)

    assert rig.stream.n_groups == N_GROUPS[case]
    assert not rig.stream.pending
    assert rig.harness.calls["pq_decompress_multi"] == 0
    assert rig.harness.calls["pq_values_multi"] == 0
    _check_order(rig.log, columns is not None)
    kinds = rig.kinds()
    assert kinds.count("read") == 1
    if columns is not None:
        # nothing but back-pressure and the end of the read waits
        assert kinds.count("join") == 1
        assert rig.calls()[-2] == ("join", N_GROUPS[case] - 1)
        # the newest flushed group is never what the host waits for: its
        # decode is to run under the next group's uploads
        flushed = -1
        for e in rig.log:
            if e[0] == "decode_group":
                flushed = e[1]
            elif e[0] == "host_wait":
                assert e[1] < flushed, rig.log
    else:
        # every group holds chunks the current stream finishes
        assert kinds.count("join") >= N_GROUPS[case]


@pytest.mark.parametrize("group", [1, 2])
def test_route_off_is_todays_sequence(shard, rig, monkeypatch, group):
    g = rig.g
    monkeypatch.setattr(g, "DECODE_STREAM", False)
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", group)
    path, ref = shard
    t = g._read_pieces_pipelined(_pieces(path), None, _ctx())
    assert t is not None
    _assert_equals_pyarrow(t, ref.to_pandas())
    n_groups = N_RGS // group
    others = [n for n in SCHEMA.names if n not in DIRECT_COLS]
    # per group: the table upload, the two calls on the current stream, then
    # the other chunks' second halves in chunk order
    per_group = [("table",), ("decompress_multi",), ("values_multi",)] + \
        [("finish", n) for n in others] * group
    assert rig.log == \
        [("read", True)] + per_group * n_groups + [("read_end", True)]
    assert rig.stream.n_groups == 0
    assert rig.harness.calls == {"pq_decompress": 0,
                                 "pq_decompress_multi": n_groups,
                                 "pq_values_multi": n_groups}


def test_route_on_and_off_give_the_same_table(shard, rig, monkeypatch):
    g = rig.g
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", 2)
    my = _pieces(shard[0])
    on = g._read_pieces_pipelined(my, None, _ctx())
    assert rig.stream.n_groups == 3
    monkeypatch.setattr(g, "DECODE_STREAM", False)
    off = g._read_pieces_pipelined(my, None, _ctx())
    assert rig.stream.n_groups == 3
    _assert_same_table(on, off)


def test_error_word_is_read_after_the_join(shard, rig, monkeypatch):
    """The first group's decode sets the error word, and only once it has
    run: a read that looked at the word before joining would not retry.
    The retry starts with nothing left on the decode stream."""
    g = rig.g
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", 2)
    rig.stream.poison_first = True
    before = dict(g.STATS)
    my = _pieces(shard[0])
    t = g._read_pieces_pipelined(my, DIRECT_COLS, _ctx())
    assert t is not None
    assert g.STATS["direct"] == before["direct"]
    log = rig.calls()
    second = log.index(("read", False))
    assert log[second - 1] == ("read_end", True)
    assert log[second - 2] == ("join", 2), log
    full = rig.log
    assert [e for e in full[:full.index(("read", False))]
            if e[0] == "run"] == [("run", 0), ("run", 1), ("run", 2)]
    assert not rig.stream.pending
    _check_order(log, False)
    monkeypatch.setattr(g, "DIRECT", False)
    monkeypatch.setattr(g, "DECODE_STREAM", False)
    _assert_same_table(t, g._read_pieces_pipelined(my, DIRECT_COLS, _ctx()))


def test_retry_from_inside_the_loop_joins_first(shard, rig, monkeypatch):
    """Page headers that contradict the footer end the direct read half way
    through the shard, with a group still on the decode stream."""
    g = rig.g
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", 1)
    info = g._direct_info
    n_direct = len(DIRECT_COLS)
    seen = []

    def _direct_info(dc, prep, chunk):
        seen.append(chunk.name)
        # the second chunk of the third row group: two groups are flushed
        return None if len(seen) == 2 * n_direct + 2 else info(dc, prep, chunk)

    monkeypatch.setattr(g, "_direct_info", _direct_info)
    my = _pieces(shard[0])
    t = _within_limit(
        lambda: g._read_pieces_pipelined(my, DIRECT_COLS, _ctx()))
    assert t is not None
    first = rig.log[:rig.log.index(("read", False))]
    assert ("run", 1) in first  # nothing is left queued behind the retry
    first = [e for e in first if e[0] != "run"]
    assert ("decode_group", 1) in first and ("decode_group", 2) not in first
    assert first[-1] == ("read_end", True) and first[-2] == ("join", 1), first
    _assert_equals_pyarrow(t, shard[1].to_pandas()[DIRECT_COLS])


def test_early_none_joins_first(tmp_path, rig, monkeypatch):
    """A chunk no route decodes (GZIP) ends the read with None; the groups
    already on the decode stream are joined before the read lets go."""
    g = rig.g
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", 1)
    path, _ = write_shard(tmp_path, ("SNAPPY", "GZIP"))
    out = _within_limit(
        lambda: g._read_pieces_pipelined(_pieces(path), None, _ctx()))
    assert out is None
    log = rig.log
    decoded = max(e[1] for e in log if e[0] == "decode_group")
    assert decoded >= 2
    assert ("join", decoded) in log
    assert log.index(("join", decoded)) < log.index(("read_end", True))
    assert not rig.stream.pending


def test_flag_is_off_without_a_gpu_device():
    from bodo_amd.io import parquet_gpu as g

    assert g._decode_stream_on("cpu") is False
    assert g._decode_stream_on(torch.device("cpu")) is False
