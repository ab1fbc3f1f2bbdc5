"""The pipelined shard reader end to end on the CPU: the real prefetcher,
gate, group tables and C++ header parser, with bit-faithful simulators in
place of the HIP kernels.  The simulators of the two absolute-address
kernels resolve every address through the tensors the reader allocated and
assert on anything outside them, so index and address bugs that would be
hardware faults show here first; the gate and the early-exit shutdown are
driven under a time limit that turns a hang into a failure."""

import random
import sys
import threading
import time

import numpy as np
import pytest
import torch

from tests import kernel_sim as ks
from tests.parquet_shards import (DIRECT_COLS, N_FILES, RG_ROWS, SCHEMA,
                                  write_shard)
from tests.test_parquet_batched_sim import _ctx, _sim_module

N_RGS = N_FILES * len(RG_ROWS)
N_CHUNKS = N_RGS * len(SCHEMA.names)


class _Harness:
    """Simulated kernels plus a record of what the reader allocated."""

    def __init__(self, g):
        self.g = g
        self.amap = ks.AddressMap()
        self.calls = {"pq_decompress": 0, "pq_decompress_multi": 0,
                      "pq_values_multi": 0}
        self.tables = []  # one dict per _GroupTables.fill
        self.poison_first_values_call = False

    def module(self):
        m = _sim_module()
        single = m.pq_decompress

        def pq_decompress(*a):
            self.calls["pq_decompress"] += 1
            single(*a)

        def pq_decompress_multi(blob, n):
            self.calls["pq_decompress_multi"] += 1
            # the slice starts the blob: record the whole allocation
            self.amap.add(torch.empty(0, dtype=torch.uint8).set_(
                blob.untyped_storage()))
            dt = self.g._PAGEPTR_DT
            ks.sim_decompress_multi(
                blob.numpy()[:n * dt.itemsize].view(dt), self.amap)

        def pq_values_multi(blob, n, err):
            self.calls["pq_values_multi"] += 1
            dt = self.g._VALPAGE_DT
            ks.sim_values_multi(blob.numpy()[:n * dt.itemsize].view(dt),
                                self.amap, err.numpy())
            if self.poison_first_values_call and \
                    self.calls["pq_values_multi"] == 1:
                err.numpy()[0] |= ks.PQE_LEVELS

        m.pq_decompress = pq_decompress
        m.pq_decompress_multi = pq_decompress_multi
        m.pq_values_multi = pq_values_multi
        return m

    def install(self, mp):
        g = self.g
        mp.setitem(sys.modules, "bodo_amd_kernels", self.module())
        mp.setattr(g, "FORCE_BATCHED", True)
        prepare, plan, fill = (g._ChunkReader._prepare_batched,
                               g._plan_direct, g._GroupTables.fill)
        h = self

        def _prepare_batched(reader, *a, **kw):
            prep = prepare(reader, *a, **kw)
            if prep is not None:
                h.amap.add(prep.src_dev)
                h.amap.add(prep.scratch)
            return prep

        def _plan_direct(*a, **kw):
            out = plan(*a, **kw)
            for dc in out.values():
                h.amap.add(dc.data)
            return out

        def _fill(tables, blob_addr):
            host = fill(tables, blob_addr)
            h.tables.append({
                "t": tables, "base": blob_addr, "host": host.copy(),
                # the entries let go of their prep once the group is done
                "directs": [(e.prep, e.direct) for e in tables.directs]})
            return host

        mp.setattr(g._ChunkReader, "_prepare_batched", _prepare_batched)
        mp.setattr(g, "_plan_direct", _plan_direct)
        mp.setattr(g._GroupTables, "fill", _fill)
        return self


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    d, ref = write_shard(tmp_path_factory.mktemp("pipe"))
    return d, ref, ref.to_pandas()


def _pieces(path):
    import glob
    import os

    return [(fp, rg) for fp in sorted(glob.glob(os.path.join(path,
                                                             "*.parquet")))
            for rg in range(len(RG_ROWS))]


@pytest.fixture
def harness(monkeypatch):
    from bodo_amd.io import parquet_gpu as g

    monkeypatch.setattr(g, "_NSLOTS", 3)
    return _Harness(g).install(monkeypatch)


@pytest.fixture(scope="module")
def direct_off_table(shard):
    """The shard read with DIRECT off: what a retry must give."""
    from bodo_amd.io import parquet_gpu as g

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(g, "_NSLOTS", 3)
        mp.setattr(g, "DIRECT", False)
        _Harness(g).install(mp)
        t = g._read_pieces_pipelined(_pieces(shard[0]), None, _ctx())
    assert t is not None
    return t


def _within_limit(fn, seconds=60):
    """Run fn in a thread; a hang fails the test instead of stopping it."""
    out = {}

    def body():
        try:
            out["value"] = fn()
        except BaseException as e:  # noqa: BLE001 - re-raised below
            out["error"] = e

    th = threading.Thread(target=body, daemon=True)
    th.start()
    th.join(seconds)
    assert not th.is_alive(), f"still running after {seconds} s: hung"
    if "error" in out:
        raise out["error"]
    return out["value"]


def _bits(t):
    return {1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()]


def _assert_same_table(on, off):
    assert on.names == off.names
    for name in on.names:
        a, b = on.column(name), off.column(name)
        assert a.val_range == b.val_range, name
        assert a.dtype.kind == b.dtype.kind, name
        if a.dictionary is not None:
            assert a.dictionary.to_pylist() == b.dictionary.to_pylist()
        if a.offsets is not None:
            assert bool((a.offsets == b.offsets).all()), name
        assert a.data.dtype == b.data.dtype, name
        assert bool((a.data.view(dtype=_bits(a.data)) ==
                     b.data.view(dtype=_bits(b.data))).all()), name
        assert (a.mask is None) == (b.mask is None), name
        if a.mask is not None:
            assert bool((a.mask == b.mask).all()), name


@pytest.mark.parametrize("group", [None, 1, 2, 4],
                         ids=["default", "g1", "g2", "g4"])
def test_pipelined_read_matches_pyarrow(shard, group, harness, monkeypatch):
    g = harness.g
    path, _, ref = shard
    if group is not None:
        monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", group)
    assert g.DIRECT
    before = dict(g.STATS)
    t = g._read_pieces_pipelined(_pieces(path), None, _ctx())
    assert t is not None, "decode fell back"
    assert g.STATS["slow"] == before["slow"]
    assert g.STATS["direct"] == before["direct"] + N_RGS * len(DIRECT_COLS)
    assert g.STATS["batched"] == before["batched"] + N_CHUNKS

    # one launch pair per group of row groups, no per-chunk decompress
    n_groups = -(-N_RGS // g._GROUP_ROW_GROUPS)
    assert n_groups == {None: 1, 1: 6, 2: 3, 4: 2}[group]
    assert harness.calls == {"pq_decompress": 0,
                             "pq_decompress_multi": n_groups,
                             "pq_values_multi": n_groups}

    # the dictionary column: unified in first-seen order, one code space
    sd = t.column("s_dict")
    assert sd.dictionary.to_pylist() == ["alpha", "beta", "gamma", "delta"]
    assert len(sd) == len(ref) and sd.mask is None

    # val_range from the footer: integer columns with statistics only
    for c in ("loc", "i32", "req"):
        v = ref[c].to_numpy()
        assert t.column(c).val_range == (int(v.min()), int(v.max())), c
    nul = ref["nul"].dropna().to_numpy()
    assert t.column("nul").val_range == (int(nul.min()), int(nul.max()))
    for c in ("nostat", "f", "f32", "ts", "s_dict", "s_plain", "cat"):
        assert t.column(c).val_range is None, c
    assert t.column("nul").mask is not None
    for c in DIRECT_COLS + ["nostat"]:
        assert t.column(c).mask is None, c

    out = t.to_pandas()
    for c in out.columns:
        if out[c].dtype.name == "category":
            out[c] = out[c].astype(object)
    assert list(out.columns) == list(ref.columns)
    assert len(out) == len(ref) == N_FILES * sum(RG_ROWS)
    for c in ref.columns:
        a, b = out[c], ref[c]
        assert (a.isna().to_numpy() == b.isna().to_numpy()).all(), c
        ok = ~b.isna().to_numpy()
        assert (a.to_numpy()[ok] == b.to_numpy()[ok]).all(), c
    assert int(ref["nul"].isna().sum()) > 0


def _inside(addr, n, t):
    return t.data_ptr() <= addr and \
        addr + n <= t.data_ptr() + t.numel() * t.element_size()


def test_group_table_invariants(shard, harness, monkeypatch):
    """The address tables of a read whose second group crosses the file
    boundary (groups of 2 row groups out of 3 per file)."""
    g = harness.g
    monkeypatch.setattr(g, "_GROUP_ROW_GROUPS", 2)
    t = g._read_pieces_pipelined(_pieces(shard[0]), None, _ctx())
    assert t is not None and len(harness.tables) == 3
    total_rows = N_FILES * sum(RG_ROWS)

    dsts = []
    outs = {}  # id of a direct column -> (column, [(offset, bytes)])
    n_luts = 0
    for rec in harness.tables:
        tb, base, host = rec["t"], rec["base"], rec["host"]
        assert len(host) == tb.nbytes
        dec = host[:tb.dec_bytes].view(g._PAGEPTR_DT)
        assert len(dec) == sum(p.n_pages for p in tb.preps)
        at = 0
        for p in tb.preps:
            for e in dec[at:at + p.n_pages]:
                assert _inside(int(e["src"]), int(e["src_len"]), p.src_dev)
                assert _inside(int(e["dst"]), int(e["dst_len"]), p.scratch)
                dsts.append((int(e["dst"]), int(e["dst_len"])))
            at += p.n_pages
        val = host[tb.dec_bytes:tb.dec_bytes + tb.val_bytes] \
            .view(g._VALPAGE_DT)
        assert len(val) == sum(p.n_pages for p, _ in rec["directs"])
        at = 0
        for p, d in rec["directs"]:
            dc = d.col
            for e in val[at:at + p.n_pages]:
                assert _inside(int(e["page"]), int(e["dst_len"]), p.scratch)
                off = int(e["out"]) - dc.data.data_ptr()
                outs.setdefault(id(dc), (dc, []))[1].append(
                    (off, int(e["nv"]) * dc.esize))
                lut = int(e["lut"])
                if dc.kind == "plain":
                    assert int(e["kind"]) == dc.esize and lut == 0
                    continue
                assert int(e["kind"]) == g._PQK_CODES
                assert int(e["code_lim"]) == len(p.dict_vals)
                assert (lut != 0) == (d.lut is not None)
                if lut:
                    n_luts += 1
                    assert lut % 8 == 0
                    assert base + tb.dec_bytes + tb.val_bytes <= lut
                    assert lut + d.lut.nbytes <= base + tb.nbytes
                    got = host[lut - base:lut - base + d.lut.nbytes]
                    assert (got.view(np.int32) == d.lut).all()
                    assert len(d.lut) == len(p.dict_vals)
            at += p.n_pages
    assert n_luts > 0  # the row groups meet the words in different orders

    dsts.sort()
    for (a, n), (b, _) in zip(dsts, dsts[1:]):
        assert a + n <= b, "decompress destinations overlap"
    assert len(outs) == len(DIRECT_COLS)
    for dc, spans in outs.values():
        spans.sort()
        at = 0
        for off, n in spans:
            assert off == at, "pages do not tile the shard column"
            at += n
        assert at == total_rows * dc.esize == \
            dc.data.numel() * dc.data.element_size()


def test_error_word_retries_without_direct(shard, harness, direct_off_table):
    g = harness.g
    harness.poison_first_values_call = True
    before = dict(g.STATS)
    t = g._read_pieces_pipelined(_pieces(shard[0]), None, _ctx())
    assert t is not None
    assert harness.calls["pq_values_multi"] == 1
    assert harness.calls["pq_decompress_multi"] == 2
    assert g.STATS["direct"] == before["direct"]
    assert g.STATS["batched"] == before["batched"] + N_CHUNKS
    _assert_same_table(t, direct_off_table)


def test_early_exit_stops_the_readers(tmp_path, harness, monkeypatch):
    """A chunk no route decodes (GZIP) ends the read with None half way
    through the shard; the reader threads must be gone when it returns."""
    g = harness.g
    monkeypatch.setattr(g, "_NSLOTS", 2)
    path, _ = write_shard(tmp_path, ("SNAPPY", "GZIP"))
    threads_before = set(threading.enumerate())

    def body():
        out = g._read_pieces_pipelined(_pieces(path), None, _ctx())
        return out, set(threading.enumerate()) - threads_before

    out, left = _within_limit(body)
    assert out is None
    assert not [th for th in left if th.is_alive()
                and th is not threading.current_thread()], left


GATE_TASKS, GATE_BYTES, GATE_SLOTS = 40, 1024, 3


@pytest.fixture(scope="module")
def gate_file(tmp_path_factory):
    data = np.random.default_rng(7).integers(
        0, 256, GATE_TASKS * GATE_BYTES, dtype=np.uint8).tobytes()
    path = str(tmp_path_factory.mktemp("gate") / "bytes.bin")
    with open(path, "wb") as f:
        f.write(data)
    return path, data


def _consume(g, gate_file, upto, pause):
    """Take tasks 0 .. upto-1 in order; every range must hold its own
    bytes for as long as the consumer holds it."""
    path, data = gate_file
    ranges = [(path, k * GATE_BYTES, GATE_BYTES) for k in range(GATE_TASKS)]
    threads_before = set(threading.enumerate())
    with g._Prefetcher(ranges, GATE_SLOTS, torch.device("cpu")) as pf:
        for k in range(upto):
            want = data[k * GATE_BYTES:(k + 1) * GATE_BYTES]
            buf = pf.get(k)
            assert bytes(buf.numpy()) == want, f"task {k} on arrival"
            time.sleep(pause)
            assert bytes(buf.numpy()) == want, f"task {k} overwritten"
            pf.release(k, g._record_event("cpu"))
    return [th for th in set(threading.enumerate()) - threads_before
            if th.is_alive() and th is not threading.current_thread()]


def test_gate_slow_consumer(gate_file):
    from bodo_amd.io import parquet_gpu as g

    assert _within_limit(
        lambda: _consume(g, gate_file, GATE_TASKS, 0.003)) == []


def test_gate_workers_delayed_at_random(gate_file, monkeypatch):
    """A worker that is slow between passing the gate and reading must not
    lose its slot to task k + N, nor overwrite what the consumer holds."""
    from bodo_amd.io import parquet_gpu as g

    read = g._Prefetcher._read
    rng = random.Random(11)
    delays = [rng.random() * 0.004 for _ in range(GATE_TASKS)]

    def _read(pf, k):
        time.sleep(delays[k])
        read(pf, k)

    monkeypatch.setattr(g._Prefetcher, "_read", _read)
    assert _within_limit(
        lambda: _consume(g, gate_file, GATE_TASKS, 0.0005)) == []


def test_gate_consumer_leaves_early(gate_file):
    from bodo_amd.io import parquet_gpu as g

    assert _within_limit(lambda: _consume(g, gate_file, 6, 0.001)) == []
