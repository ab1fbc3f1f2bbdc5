"""On-GPU Parquet decode (BASELINE config 2; reference role:
cudf::io::read_parquet in bodo/pandas/physical/gpu_read_parquet.h).

Host side: footer metadata (pyarrow), raw column-chunk byte ranges read from
disk into pinned staging, page headers parsed in C++ (Thrift compact
protocol), the small dictionary page decoded on the host.  Device side, per
column chunk: snappy (or uncompressed) v1 data pages decompress one wave per
page, definition levels expand to a validity mask (nullable columns),
then PLAIN fixed-width values, PLAIN BYTE_ARRAY strings or RLE_DICTIONARY
codes are assembled into a Column.  The pipelined shard reader decompresses
the pages of every column chunk of a few row groups in one launch, and
decodes chunks that hold no nulls by their footer statistics (PLAIN
fixed-width values, string-dictionary codes) straight into whole-shard
columns allocated once: one pq_values_multi call per group checks each
page's definition levels and writes its values in place, so such columns
need no mask, no per-chunk launches and no concatenation.  Integer and
date32 columns take val_range from the footer's min/max.  Chunks outside
these paths (other codecs, v2 pages, BOOLEAN/INT96/FIXED_LEN, mixed
plain/dict) take the older per-page route and then the host Arrow decoder.

The pipelined reader is built from parts that run without a GPU, so CPU
tests drive it end to end against kernel simulators: _scan_chunks (footers
to _Chunk records), _Prefetcher (reader threads, staging slots and their
ordered gate), _GroupTables (the absolute-address page tables of a group,
computed on the host) and _GroupDecoder (the launches of a group).  The
one device switch is in _Staging and _record_event: off CUDA the staging
buffers are ordinary memory and an event is None, which waits for nothing.
"""

from __future__ import annotations

import glob
import os
import struct
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

from ..core import types as bt
from ..core.column import Column
from ..core.table import Table


class ThriftCompact:
    """Minimal Thrift compact protocol reader (field skeleton only)."""

    def __init__(self, buf: bytes, pos: int = 0):
        self.buf = buf
        self.pos = pos

    def varint(self) -> int:
        out = 0
        shift = 0
        while True:
            b = self.buf[self.pos]
            self.pos += 1
            out |= (b & 0x7F) << shift
            if not b & 0x80:
                return out
            shift += 7

    def zigzag(self) -> int:
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def read_struct(self) -> dict:
        out = {}
        field_id = 0
        while True:
            b = self.buf[self.pos]
            self.pos += 1
            if b == 0:
                return out
            delta = (b >> 4) & 0x0F
            ftype = b & 0x0F
            if delta:
                field_id += delta
            else:
                field_id = self.zigzag()
            out[field_id] = self.read_value(ftype)

    def read_value(self, ftype: int):
        if ftype in (1, 2):  # bool true/false encoded in type nibble
            return ftype == 1
        if ftype == 3:  # byte
            v = self.buf[self.pos]
            self.pos += 1
            return v
        if ftype in (4, 5, 6):  # i16/i32/i64 zigzag
            return self.zigzag()
        if ftype == 7:  # double
            v = struct.unpack_from("<d", self.buf, self.pos)[0]
            self.pos += 8
            return v
        if ftype == 8:  # binary/string
            n = self.varint()
            v = self.buf[self.pos:self.pos + n]
            self.pos += n
            return v
        if ftype == 9:  # list
            b = self.buf[self.pos]
            self.pos += 1
            size = (b >> 4) & 0x0F
            etype = b & 0x0F
            if size == 15:
                size = self.varint()
            return [self.read_value(etype) for _ in range(size)]
        if ftype == 12:  # struct
            return self.read_struct()
        raise ValueError(f"thrift type {ftype}")


PAGE_DATA = 0
PAGE_DICT = 2
ENC_PLAIN = 0
ENC_PLAIN_DICT = 2
ENC_RLE = 3
ENC_RLE_DICT = 8

_PHYS_NP = {
    "INT32": np.int32, "INT64": np.int64, "FLOAT": np.float32,
    "DOUBLE": np.float64, "BOOLEAN": np.bool_,
}


def _parse_rle_runs(buf: bytes, pos: int, end: int, bitwidth: int,
                    n_values: int):
    """Scan RLE/bit-packed hybrid run headers -> run table (host)."""
    runs: List[Tuple[int, int, int, int]] = []  # out_start, count, kind, val/bitoff
    out = 0
    t = ThriftCompact(buf, pos)
    width_bytes = (bitwidth + 7) // 8
    while out < n_values and t.pos < end:
        h = t.varint()
        if h & 1:  # bit-packed group of (h>>1)*8 values
            groups = h >> 1
            count = min(groups * 8, n_values - out)
            bitoff = t.pos * 8
            runs.append((out, count, 1, bitoff))
            t.pos += groups * bitwidth  # groups*8 values * bw /8 bits
            out += count
        else:
            count = min(h >> 1, n_values - out)
            v = int.from_bytes(t.buf[t.pos:t.pos + width_bytes], "little") \
                if width_bytes else 0
            t.pos += width_bytes
            runs.append((out, count, 0, v))
            out += count
    return runs, out


def _runs_blob(runs) -> np.ndarray:
    arr = np.zeros(len(runs), dtype=[("out_start", np.int64),
                                     ("count", np.int32), ("kind", np.int32),
                                     ("val", np.int64)])
    for i, (o, c, k, v) in enumerate(runs):
        arr[i] = (o, c, k, v)
    return arr


def _record_event(device):
    """An event recorded on the device's current stream.  None when the
    device is not CUDA: work there is done when the call returns, and
    _wait_event(None) waits for nothing."""
    if torch.device(device).type != "cuda":
        return None
    ev = torch.cuda.Event()
    ev.record()
    return ev


def _wait_event(ev) -> None:
    if ev is not None:
        ev.synchronize()


class _Staging:
    """A ring of pinned host buffers for async copies to the device.
    take(k, n, device) gives buffer k % len of at least n bytes once the
    previous copy out of it has finished; after queueing the next copy out
    the user hands its event to sent(k, ev).  For a device that is not CUDA
    the buffers are ordinary memory and the events None."""

    def __init__(self, n_bufs: int, min_bytes: int):
        self.min_bytes = min_bytes
        self.bufs: list = [None] * n_bufs
        self.pinned = [False] * n_bufs
        self.events: list = [None] * n_bufs
        self.turn = 0

    def next_turn(self) -> int:
        """Round-robin k for users that have no task numbers of their own."""
        k = self.turn
        self.turn = (k + 1) % len(self.bufs)
        return k

    def take(self, k: int, n: int, device) -> torch.Tensor:
        i = k % len(self.bufs)
        _wait_event(self.events[i])  # the copy out of this buffer is done
        self.events[i] = None
        pin = torch.device(device).type == "cuda"
        buf = self.bufs[i]
        if buf is None or buf.numel() < n or self.pinned[i] != pin:
            buf = torch.empty(max(n, self.min_bytes), dtype=torch.uint8,
                              pin_memory=pin)
            self.bufs[i], self.pinned[i] = buf, pin
        return buf

    def sent(self, k: int, ev) -> None:
        self.events[k % len(self.bufs)] = ev


# chunk uploads outside the pipelined reader: double-buffered so the host
# memcpy into one buffer overlaps the async H2D copy from the other
_CHUNK_STAGING = _Staging(2, 1 << 22)
# page tables of a group: written into a pinned buffer and copied with
# non_blocking=True, so the consumer thread never waits for the chunk
# copies queued before them
_TABLE_STAGING = _Staging(4, 1 << 21)


def _upload_staged(staging: _Staging, np_u8: np.ndarray,
                   dev_out: torch.Tensor) -> None:
    """Copy host bytes to dev_out through the ring's next buffer."""
    n = len(np_u8)
    k = staging.next_turn()
    buf = staging.take(k, n, dev_out.device)
    buf.numpy()[:n] = np_u8
    dev_out.copy_(buf[:n], non_blocking=True)
    staging.sent(k, _record_event(dev_out.device))

# decode-path counters (tests assert the batched path actually ran)
STATS = {"batched": 0, "slow": 0, "direct": 0}
# CPU tests flip this with simulated kernels monkeypatched in
FORCE_BATCHED = False

_PAGEMETA_DT = np.dtype([
    ("src_off", np.int64), ("dst_off", np.int64), ("val_off", np.int64),
    ("src_len", np.int32), ("dst_len", np.int32), ("nv", np.int32),
    ("flags", np.int32),
])
_PQF_HAS_DEF = 1
_PQF_SNAPPY = 2

# page table entry of K.pq_decompress_multi: absolute device addresses
_PAGEPTR_DT = np.dtype([
    ("src", np.uint64), ("dst", np.uint64), ("src_len", np.int32),
    ("dst_len", np.int32), ("flags", np.int32), ("pad", np.int32),
])
# page table entry of K.pq_values_multi (struct ValPage, csrc/parquet.hip)
_VALPAGE_DT = np.dtype([
    ("page", np.uint64), ("out", np.uint64), ("lut", np.uint64),
    ("dst_len", np.int32), ("nv", np.int32), ("kind", np.int32),
    ("flags", np.int32), ("code_lim", np.int32), ("pad", np.int32),
])
_PQK_CODES = 0  # ValPage.kind of dictionary codes; PLAIN: element size
# row groups whose column chunks share one decompress launch in the
# pipelined reader (1..32 measured: profiles/decode_parallel_snappy.md)
_GROUP_ROW_GROUPS = 16


class _Prepared:
    """A column chunk between the two halves of the batched decode: page
    table built and scratch allocated, pages not yet decompressed."""

    __slots__ = ("mode", "dict_vals", "metas", "metas_dev", "n_pages",
                 "src_dev", "scratch", "val_off", "total_nv")


def _chunk_range(chunk_meta):
    start = chunk_meta.dictionary_page_offset
    if start is None or start <= 0:
        start = chunk_meta.data_page_offset
    return int(start), int(chunk_meta.total_compressed_size)


class _ChunkReader:
    def __init__(self, f, chunk_meta, phys_type: str, max_def: int = 1,
                 prefetched=None):
        self.meta = chunk_meta
        self.phys = phys_type
        self.max_def = max_def
        self._hdrs = None
        self._dev = None
        self._dict_raw = None
        self._lazy_src = None
        self._buf = None
        if prefetched is not None:
            # (hdrs np, device tensor of the raw chunk, dict page raw bytes
            #  or None, (path, start, size) for the rare host fallback)
            self._hdrs, self._dev, self._dict_raw, self._lazy_src = prefetched
        else:
            start, size = _chunk_range(chunk_meta)
            f.seek(start)
            self._buf = f.read(size)

    @property
    def buf(self) -> bytes:
        if self._buf is None:
            path, start, size = self._lazy_src
            with open(path, "rb") as f:
                f.seek(start)
                self._buf = f.read(size)
        return self._buf

    # ------------------------------------------------------------------
    # batched page-parallel device decode (the fast path)
    # ------------------------------------------------------------------
    def decode_column(self, device, field: pa.Field) -> Optional[Column]:
        """Full device decode of this chunk into a Column, or None for the
        next fallback tier (old per-page path, then host Arrow)."""
        try:
            col = self._decode_batched(device, field)
        except Exception:
            col = None
        if col is not None:
            STATS["batched"] += 1
            return col
        STATS["slow"] += 1
        try:
            res = self.decode(device)
        except Exception:
            res = None
        if res is None:
            return None
        vals, dict_vals, mask = res
        col = _to_column(vals, dict_vals, field, device)
        if mask is not None:
            col.mask = mask
        return col

    def _decode_batched(self, device, field: pa.Field) -> Optional[Column]:
        prep = self._prepare_batched(device)
        if prep is None:
            return None
        import bodo_amd_kernels as K

        K.pq_decompress(prep.src_dev, prep.metas_dev, prep.n_pages,
                        prep.scratch)
        return self._finish_batched(prep, device, field)

    def _prepare_batched(self, device,
                         upload_metas: bool = True) -> Optional[_Prepared]:
        """First half: headers, dictionary page, page table, scratch.
        None when the chunk is outside the batched path.  A chunk decoded
        in place needs no device copy of its page table (upload_metas)."""
        if torch.device(device).type != "cuda" and not FORCE_BATCHED:
            return None  # batched kernels are device-only (tests simulate)
        comp = self.meta.compression
        if comp not in ("SNAPPY", "UNCOMPRESSED"):
            return None
        if self.phys in ("BOOLEAN", "INT96", "FIXED_LEN_BYTE_ARRAY"):
            return None
        import bodo_amd_kernels as K

        if self._hdrs is not None:
            hdrs = self._hdrs
        else:
            buf_np = np.frombuffer(self.buf, dtype=np.uint8)
            hdrs = K.pq_parse_headers(torch.from_numpy(buf_np)).numpy()
        if hdrs.size == 0:
            return None
        ptype, usize, csize, body, nv, enc, defenc = (hdrs[:, i]
                                                      for i in range(7))
        if not np.isin(ptype, (PAGE_DATA, PAGE_DICT)).all():
            return None  # v2 data pages etc.
        if (defenc[ptype == PAGE_DATA] > ENC_RLE).any():
            return None
        data_sel = ptype == PAGE_DATA
        n_pages = int(data_sel.sum())
        if n_pages == 0:
            return None
        d_usize = usize[data_sel]
        d_csize = csize[data_sel]
        d_body = body[data_sel]
        d_nv = nv[data_sel]
        d_enc = enc[data_sel]
        encs = set(d_enc.tolist())
        if encs <= {ENC_PLAIN}:
            mode = "plain"
        elif encs <= {ENC_RLE_DICT, ENC_PLAIN_DICT}:
            mode = "dict"
        else:
            return None  # mixed plain/dict chunk: old per-page path
        # host-decode the (small) dictionary page if present
        dict_vals = None
        if mode == "dict":
            di = np.nonzero(ptype == PAGE_DICT)[0]
            if len(di) != 1:
                return None
            i = int(di[0])
            raw = (self._dict_raw if self._dict_raw is not None
                   else self.buf[int(body[i]):int(body[i]) + int(csize[i])])
            if comp == "SNAPPY":
                raw = pa.Codec("snappy").decompress(
                    raw, decompressed_size=int(usize[i]))
                if isinstance(raw, pa.Buffer):
                    raw = raw.to_pybytes()
            # dict page num_values
            dnv = int(nv[i])
            dict_vals = self._decode_plain(raw, 0, dnv)

        # page table: 8-byte-aligned decompression offsets, value offsets
        metas = np.zeros(n_pages, dtype=_PAGEMETA_DT)
        metas["src_off"] = d_body
        metas["src_len"] = d_csize
        metas["dst_len"] = d_usize
        metas["nv"] = d_nv
        dst = np.cumsum(np.concatenate([[0], (d_usize + 7) & ~7]))[:-1]
        metas["dst_off"] = dst
        val_off = np.cumsum(np.concatenate([[0], d_nv]))[:-1]
        metas["val_off"] = val_off
        total_nv = int(d_nv.sum())
        flags = 0
        if self.max_def > 0:
            flags |= _PQF_HAS_DEF
        if comp == "SNAPPY":
            flags |= _PQF_SNAPPY
        metas["flags"] = flags

        if self._dev is not None:
            src_dev = self._dev
        else:
            src_dev = torch.empty(len(self.buf), dtype=torch.uint8,
                                  device=device)
            _upload_staged(_CHUNK_STAGING,
                           np.frombuffer(self.buf, dtype=np.uint8), src_dev)
        metas_dev = torch.from_numpy(metas.view(np.uint8)).to(device) \
            if upload_metas else None
        scratch_size = int(((d_usize + 7) & ~7).sum()) + 16
        scratch = torch.empty(scratch_size, dtype=torch.uint8, device=device)
        prep = _Prepared()
        prep.mode, prep.dict_vals = mode, dict_vals
        prep.metas, prep.metas_dev, prep.n_pages = metas, metas_dev, n_pages
        prep.src_dev, prep.scratch = src_dev, scratch
        prep.val_off, prep.total_nv = val_off, total_nv
        return prep

    def _finish_batched(self, prep: _Prepared, device,
                        field: pa.Field) -> Optional[Column]:
        """Second half, once prep.scratch holds the decompressed pages:
        def levels, then codes / strings / fixed-width values."""
        import bodo_amd_kernels as K

        mode, dict_vals = prep.mode, prep.dict_vals
        metas_dev, n_pages, scratch = prep.metas_dev, prep.n_pages, prep.scratch
        val_off, total_nv = prep.val_off, prep.total_nv
        mask_t = None
        n_valid = None
        vdo = None
        if self.max_def > 0:
            mask_u8, n_valid, vdo = K.pq_def_levels(
                scratch, metas_dev, n_pages, 1, 1, total_nv)
            # chunk statistics carry the null count: avoids a device sync
            # per chunk (the round-1 pipeline serializer)
            st = self.meta.statistics
            if st is not None and st.has_null_count:
                nvalid_total = total_nv - int(st.null_count)
            else:
                nvalid_total = int(n_valid.sum().item())
            dense_off = torch.cumsum(n_valid.long(), 0) - n_valid.long()
            if nvalid_total < total_nv:
                mask_t = mask_u8.to(torch.bool)
        else:
            nvalid_total = total_nv
            dense_off = torch.from_numpy(val_off).to(device)

        if mode == "dict":
            codes = K.pq_expand_codes(scratch, metas_dev, n_pages, vdo,
                                      dense_off, n_valid, nvalid_total)
            if mask_t is not None:
                full = torch.zeros(total_nv, dtype=torch.int32, device=device)
                full.masked_scatter_(mask_t, codes)
                codes = full
            col = _to_column(codes, dict_vals, field, device)
            if mask_t is not None:
                col.mask = mask_t
            return col

        # PLAIN
        if self.phys == "BYTE_ARRAY":
            lens, src_abs = K.pq_byte_array_lengths(
                scratch, metas_dev, n_pages, vdo, dense_off, n_valid,
                nvalid_total)
            if mask_t is not None:
                lens_full = torch.zeros(total_nv, dtype=torch.int32,
                                        device=device)
                lens_full.masked_scatter_(mask_t, lens)
            else:
                lens_full = lens
            offs = torch.zeros(total_nv + 1, dtype=torch.int64, device=device)
            torch.cumsum(lens_full.long(), 0, out=offs[1:])
            total_bytes = int(offs[-1].item())
            if mask_t is not None:
                dst0 = offs[:-1].masked_select(mask_t)
            else:
                dst0 = offs[:-1]
            data = K.pq_copy_strings(scratch, src_abs, dst0, lens,
                                     nvalid_total, total_bytes)
            col = Column(bt.string, data, mask_t, offsets=offs,
                         length=total_nv)
            return col
        npdt = _PHYS_NP[self.phys]
        esize = np.dtype(npdt).itemsize
        dense = K.pq_copy_fixed(scratch, metas_dev, n_pages, vdo, dense_off,
                                n_valid, esize, nvalid_total)
        tdt = torch.from_numpy(np.zeros(0, dtype=npdt)).dtype
        vals = dense.view(tdt)
        if mask_t is not None:
            full = torch.zeros(total_nv, dtype=tdt, device=device)
            full.masked_scatter_(mask_t, vals)
            vals = full
        col = _fixed_column(vals, field.type)
        if mask_t is not None:
            col.mask = mask_t
        return col

    def decode(self, device):
        """Returns (device values or codes, dictionary or None, validity
        mask or None); None if the chunk needs the host fallback.
        SNAPPY pages decompress on host (pyarrow codec) before device
        expansion; nulls build a device mask from the definition-level RLE
        and scatter the dense values into place."""
        comp = self.meta.compression
        codec = None
        if comp == "SNAPPY":
            codec = pa.Codec("snappy")
        elif comp != "UNCOMPRESSED":
            return None
        if self.phys in ("BOOLEAN", "INT96", "FIXED_LEN_BYTE_ARRAY"):
            return None  # bit-packed plain / legacy types: host fallback
        pos = 0
        n = len(self.buf)
        dict_vals: Optional[np.ndarray] = None
        parts: List[Tuple[object, Optional[torch.Tensor], str]] = []
        has_nulls = False
        while pos < n:
            t = ThriftCompact(self.buf, pos)
            hdr = t.read_struct()
            body = t.pos
            ptype = hdr.get(1)
            comp_size = hdr.get(3)
            raw = self.buf[body:body + comp_size]
            if codec is not None and ptype in (PAGE_DICT, PAGE_DATA):
                pb = codec.decompress(raw, decompressed_size=hdr.get(2))
            else:
                pb = raw
            if isinstance(pb, pa.Buffer):
                pb = pb.to_pybytes()
            if ptype == PAGE_DICT:
                dph = hdr.get(7, {})
                nv = dph.get(1, 0)
                dict_vals = self._decode_plain(pb, 0, nv)
            elif ptype == PAGE_DATA:
                dph = hdr.get(5, {})
                nv = dph.get(1, 0)
                enc = dph.get(2, ENC_PLAIN)
                p = 0
                mask_t: Optional[torch.Tensor] = None
                n_valid = nv
                if self.max_def > 0:
                    (lvl_len,) = struct.unpack_from("<i", pb, p)
                    lv_runs, got = _parse_rle_runs(pb, p + 4, p + 4 + lvl_len,
                                                   1, nv)
                    p += 4 + lvl_len
                    if got != nv:
                        return None
                    if any(k == 1 or v != 1 for _, _, k, v in lv_runs):
                        # page has nulls (or bit-packed def levels): expand
                        # the level stream on device into a validity mask
                        import bodo_amd_kernels as K

                        pb_dev = _dev_bytes(pb, device)
                        blob = torch.from_numpy(
                            _runs_blob(lv_runs).view(np.uint8)).to(device)
                        lv = K.rle_expand(blob, len(lv_runs), pb_dev, 1, nv)
                        mask_t = lv.to(torch.bool)
                        n_valid = int(mask_t.sum().item())
                        has_nulls = True
                if enc == ENC_PLAIN:
                    if self.phys == "BYTE_ARRAY" and mask_t is not None:
                        return None  # dense plain strings + nulls: host
                    dense = self._decode_plain(pb, p, n_valid)
                    parts.append((dense, mask_t, "plain"))
                elif enc in (ENC_RLE_DICT, ENC_PLAIN_DICT):
                    bitwidth = pb[p]
                    if bitwidth > 24:
                        return None
                    if bitwidth == 0:
                        codes = torch.zeros(n_valid, dtype=torch.int32,
                                            device=device)
                    else:
                        runs, got = _parse_rle_runs(pb, p + 1, len(pb),
                                                    bitwidth, n_valid)
                        if got != n_valid:
                            return None
                        import bodo_amd_kernels as K

                        pb_dev = _dev_bytes(pb, device)
                        blob = torch.from_numpy(
                            _runs_blob(runs).view(np.uint8)).to(device)
                        codes = K.rle_expand(blob, len(runs), pb_dev,
                                             int(bitwidth), n_valid)
                    parts.append((codes, mask_t, "codes"))
                else:
                    return None
            pos = body + comp_size
        kinds = {k for _, _, k in parts}
        if not kinds:
            return None
        if "codes" in kinds and dict_vals is None:
            return None
        # all-dict chunks stay dictionary-encoded; chunks that switched to
        # PLAIN mid-way (dictionary overflow on high-cardinality data)
        # decode their dict pages to values so both page kinds concatenate
        use_dict_col = kinds == {"codes"}
        dict_dev = None
        if not use_dict_col and "codes" in kinds:
            if dict_vals is None or dict_vals.dtype == object:
                return None  # mixed string pages: host fallback
            dict_dev = torch.from_numpy(
                np.ascontiguousarray(dict_vals)).to(device)
        # assemble per page: scatter dense values into null positions
        out_parts: List[torch.Tensor] = []
        mask_parts: List[torch.Tensor] = []
        for dense, mask_t, k in parts:
            if k == "plain":
                vals_t = torch.from_numpy(
                    np.ascontiguousarray(dense)).to(device)
            elif use_dict_col:
                vals_t = dense
            else:
                vals_t = dict_dev[dense.long()]
            if mask_t is None:
                out_parts.append(vals_t)
                mask_parts.append(torch.ones(len(vals_t), dtype=torch.bool,
                                             device=device)
                                  if has_nulls else None)
            else:
                full = torch.zeros(len(mask_t), dtype=vals_t.dtype,
                                   device=device)
                full[mask_t] = vals_t
                out_parts.append(full)
                mask_parts.append(mask_t)
        vals = torch.cat(out_parts) if len(out_parts) > 1 else out_parts[0]
        mask = None
        if has_nulls:
            mask = torch.cat(mask_parts) if len(mask_parts) > 1 \
                else mask_parts[0]
        return vals, (dict_vals if use_dict_col else None), mask

    def _decode_plain(self, buf: bytes, pos: int, nv: int):
        if self.phys == "BYTE_ARRAY":
            out = []
            p = pos
            for _ in range(nv):
                (ln,) = struct.unpack_from("<i", buf, p)
                out.append(buf[p + 4:p + 4 + ln].decode())
                p += 4 + ln
            return np.array(out, dtype=object)
        npdt = _PHYS_NP[self.phys]
        return np.frombuffer(buf, dtype=npdt, count=nv, offset=pos)


def _dev_bytes(pb: bytes, device) -> torch.Tensor:
    arr = np.frombuffer(pb, dtype=np.uint8)
    padded = np.concatenate([arr, np.zeros(8, dtype=np.uint8)])
    return torch.from_numpy(padded).to(device)


def read_shard_gpu(path: str, columns, ctx) -> Optional[Table]:
    """Read a parquet file (or list) with device-side decode; returns None
    when the file layout is outside the fast path."""
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "*.parquet")))
    else:
        files = [path]
    # split row groups across ranks
    pieces = []
    for fp in files:
        md = pq.ParquetFile(fp).metadata
        for rg in range(md.num_row_groups):
            pieces.append((fp, rg))
    w, r = ctx.world, ctx.rank
    base, rem = divmod(len(pieces), w)
    start = r * base + min(r, rem)
    my = pieces[start:start + base + (1 if r < rem else 0)]
    if not my:
        return None
    if torch.device(ctx.device).type == "cuda":
        return _read_pieces_pipelined(my, columns, ctx)
    out_tables = []
    for fp, rg in my:
        t = _read_row_group_gpu(fp, rg, columns, ctx)
        if t is None:
            return None
        out_tables.append(t)
    if len(out_tables) == 1:
        return out_tables[0]
    from .. import ops

    return ops.concat_tables(out_tables)


# reader threads = pinned staging slots.  The stream waits for these threads
# (page cache -> pinned memory), not the other way round: 8 / 12 / 14 threads
# gave 1003-1165 / 839-867 / 841-897 ms per flagship step
# (profiles/decode_in_place.md)
_NSLOTS = int(os.environ.get("BODO_AMD_READ_THREADS", "12"))

# decode eligible chunks straight into whole-shard columns (off: every
# chunk takes the per-chunk finish and the pieces are concatenated)
DIRECT = os.environ.get("BODO_AMD_PQ_DIRECT", "1") != "0"

_DICT_ENCODINGS = {"RLE_DICTIONARY", "PLAIN_DICTIONARY"}
_DIRECT_PLAIN = {"INT32": torch.int32, "INT64": torch.int64,
                 "FLOAT": torch.float32, "DOUBLE": torch.float64}


class _DictUnifier:
    """Dictionary of a whole shard column, grown chunk by chunk on the
    host: values in first-seen order across the chunks in shard order,
    which is what ops.concat_columns makes of the chunks' dictionaries."""

    def __init__(self):
        self.values: list = []
        self.index: dict = {}

    def add(self, dict_vals) -> Optional[np.ndarray]:
        """Take in one chunk's dictionary.  Returns the int32 table from
        the chunk's codes to unified codes, or None when every code already
        is its unified code (the chunk's dictionary is a prefix of the
        unified one, or extends it)."""
        lut = np.empty(len(dict_vals), dtype=np.int32)
        same = True
        for i, v in enumerate(dict_vals):
            j = self.index.get(v)
            if j is None:
                j = len(self.values)
                self.index[v] = j
                self.values.append(v)
            lut[i] = j
            same = same and j == i
        return None if same else lut

    def dictionary(self) -> pa.Array:
        return pa.array(self.values, type=pa.large_string())


def _stat_int(v) -> Optional[int]:
    import datetime

    if isinstance(v, bool):
        return None
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, datetime.date) and not isinstance(v, datetime.datetime):
        return (v - datetime.date(1970, 1, 1)).days
    return None


def _val_range_from_meta(chunk_metas, t: pa.DataType
                         ) -> Optional[Tuple[int, int]]:
    """(min, max) of an integer or date32 column from the footer statistics
    of its chunks; None unless every chunk carries min and max."""
    if not (pa.types.is_integer(t) or pa.types.is_date32(t)):
        return None
    lo = hi = None
    for cm in chunk_metas:
        st = cm.statistics if cm.is_stats_set else None
        if st is None or not st.has_min_max:
            return None
        a, b = _stat_int(st.min), _stat_int(st.max)
        if a is None or b is None:
            return None
        lo = a if lo is None else min(lo, a)
        hi = b if hi is None else max(hi, b)
    if lo is None:
        return None
    return lo, hi


def _direct_chunk_kind(cm, field: pa.Field) -> Optional[str]:
    """'plain' or 'dict' when the footer says this chunk can be decoded in
    place: no nulls by its statistics (or a required field), PLAIN
    fixed-width values or a string dictionary.  Page headers can still
    disagree later (v2 pages, a dictionary that overflowed to PLAIN)."""
    if cm.compression not in ("SNAPPY", "UNCOMPRESSED"):
        return None
    if field.nullable:
        st = cm.statistics if cm.is_stats_set else None
        if st is None or not st.has_null_count or st.null_count != 0:
            return None
    has_dict = bool(_DICT_ENCODINGS & set(cm.encodings))
    t = field.type
    if cm.physical_type in _DIRECT_PLAIN:
        if has_dict:
            return None
        if cm.physical_type == "INT32":
            ok = pa.types.is_int32(t) or pa.types.is_date32(t)
        elif cm.physical_type == "INT64":
            ok = pa.types.is_int64(t) or pa.types.is_timestamp(t)
        elif cm.physical_type == "FLOAT":
            ok = pa.types.is_float32(t)
        else:
            ok = pa.types.is_float64(t)
        return "plain" if ok else None
    if pa.types.is_dictionary(t):  # written from a dictionary array
        t = t.value_type
    if cm.physical_type == "BYTE_ARRAY" and has_dict and (
            pa.types.is_string(t) or pa.types.is_large_string(t)):
        return "dict"
    return None


@dataclass(slots=True)
class _Chunk:
    """One column chunk of a shard, as the footer describes it."""

    path: str
    rg: int
    cm: object  # pyarrow ColumnChunkMetaData
    field: pa.Field
    start: int  # byte range of the chunk in the file
    size: int
    first_of_rg: bool  # first selected chunk of its row group
    row0: int  # first row of the row group in the shard
    rows: int  # rows of the row group

    @property
    def name(self) -> str:
        return self.cm.path_in_schema


def _scan_chunks(my, columns) -> Tuple[List[_Chunk], List[str], int]:
    """The selected column chunks of the (file, row group) pieces in shard
    order, the output column names (as the last piece has them) and the
    shard's row count."""
    chunks: List[_Chunk] = []
    pf_cache: dict = {}
    names: List[str] = []
    total_rows = 0
    for fp, rg in my:
        pf = pf_cache.get(fp)
        if pf is None:
            pf = pq.ParquetFile(fp)
            pf_cache[fp] = pf
        schema = pf.schema_arrow
        rgm = pf.metadata.row_group(rg)
        names = columns or [schema.field(i).name
                            for i in range(len(schema.names))]
        first = True
        for ci in range(rgm.num_columns):
            cm = rgm.column(ci)
            if cm.path_in_schema not in names:
                continue
            start, size = _chunk_range(cm)
            chunks.append(_Chunk(fp, rg, cm, schema.field(cm.path_in_schema),
                                 start, size, first, total_rows,
                                 int(rgm.num_rows)))
            first = False
        total_rows += int(rgm.num_rows)
    return chunks, names, total_rows


class _DirectCol:
    """A shard column that its chunks are decoded into in place."""

    __slots__ = ("kind", "esize", "data", "field", "unifier")


def _plan_direct(chunks: List[_Chunk], n_rgs: int, total_rows: int,
                 device) -> dict:
    """name -> _DirectCol for the columns whose every chunk is eligible by
    the footer; their whole-shard tensors are allocated here, once."""
    by_name: dict = {}
    for c in chunks:
        by_name.setdefault(c.name, []).append(c)
    plan = {}
    for name, its in by_name.items():
        field = its[0].field
        if len(its) != n_rgs or any(c.field.type != field.type or
                                    c.field.nullable != field.nullable
                                    for c in its):
            continue
        kinds = {_direct_chunk_kind(c.cm, c.field) for c in its}
        phys = {c.cm.physical_type for c in its}
        if len(kinds) != 1 or None in kinds or len(phys) != 1:
            continue
        dc = _DirectCol()
        dc.kind = kinds.pop()
        dc.field = field
        if dc.kind == "plain":
            tdt = _DIRECT_PLAIN[phys.pop()]
            dc.unifier = None
        else:
            tdt = torch.int32
            dc.unifier = _DictUnifier()
        dc.data = torch.empty(total_rows, dtype=tdt, device=device)
        dc.esize = dc.data.element_size()
        plan[name] = dc
    return plan


@dataclass(slots=True)
class _DirectInfo:
    """Where a chunk that is decoded in place goes."""

    col: _DirectCol  # the shard column
    row0: int  # first row of the chunk in it
    lut: Optional[np.ndarray]  # chunk codes -> unified codes, or None


@dataclass(slots=True)
class _GroupEntry:
    """A chunk of the group being collected."""

    name: str
    reader: _ChunkReader
    field: pa.Field
    prep: Optional[_Prepared]  # None: outside the batched path, or finished
    column: Optional[Column]  # the decoded chunk, unless it is direct
    direct: Optional[_DirectInfo]


class _GroupTables:
    """Layout and host image of the one blob a group uploads: a _PAGEPTR_DT
    entry per page of every prepared chunk (pq_decompress_multi), then a
    _VALPAGE_DT entry per page of the direct chunks (pq_values_multi), then
    their code tables, each at an 8-byte-aligned offset.  Needs no GPU: the
    addresses come from the tensors the chunks were prepared with."""

    def __init__(self, preps: List[_Prepared], directs: List[_GroupEntry]):
        self.preps, self.directs = preps, directs
        self.n_dec = sum(p.n_pages for p in preps)
        self.n_val = sum(e.prep.n_pages for e in directs)
        self.dec_bytes = self.n_dec * _PAGEPTR_DT.itemsize
        self.val_bytes = self.n_val * _VALPAGE_DT.itemsize
        self.lut_at = []  # blob offset of each direct chunk's code table
        self.nbytes = self.dec_bytes + self.val_bytes
        for e in directs:
            self.lut_at.append(self.nbytes)
            if e.direct.lut is not None:
                self.nbytes += (e.direct.lut.nbytes + 7) & ~7

    def fill(self, blob_addr: int) -> np.ndarray:
        """The blob's bytes, given the device address it will live at."""
        host = np.zeros(self.nbytes, dtype=np.uint8)
        tbl = host[:self.dec_bytes].view(_PAGEPTR_DT)
        at = 0
        for p in self.preps:
            v = tbl[at:at + p.n_pages]
            v["src"] = p.src_dev.data_ptr() + p.metas["src_off"]
            v["dst"] = p.scratch.data_ptr() + p.metas["dst_off"]
            v["src_len"] = p.metas["src_len"]
            v["dst_len"] = p.metas["dst_len"]
            v["flags"] = p.metas["flags"] & _PQF_SNAPPY
            at += p.n_pages
        vt = host[self.dec_bytes:self.dec_bytes + self.val_bytes] \
            .view(_VALPAGE_DT)
        at = 0
        for e, la in zip(self.directs, self.lut_at):
            p, dc, lut = e.prep, e.direct.col, e.direct.lut
            v = vt[at:at + p.n_pages]
            v["page"] = p.scratch.data_ptr() + p.metas["dst_off"]
            v["out"] = dc.data.data_ptr() + \
                (e.direct.row0 + p.metas["val_off"]) * dc.esize
            v["dst_len"] = p.metas["dst_len"]
            v["nv"] = p.metas["nv"]
            v["kind"] = dc.esize if dc.kind == "plain" else _PQK_CODES
            v["flags"] = p.metas["flags"] & _PQF_HAS_DEF
            if dc.kind == "dict":
                v["code_lim"] = len(p.dict_vals)
                if lut is not None:
                    v["lut"] = blob_addr + la
                    host[la:la + lut.nbytes] = lut.view(np.uint8)
            at += p.n_pages
        return host


class _Prefetcher:
    """Reader threads that pull byte ranges of files into a ring of pinned
    staging buffers ahead of one consumer that takes them in order:

        with _Prefetcher(ranges, n_slots, device) as pf:
            for k in range(len(ranges)):
                buf = pf.get(k)          # task k's bytes, pinned
                ... queue the async copy of buf to the device ...
                pf.release(k, _record_event(device))

    DETERMINISTIC slot assignment: task k uses slot k % N once the
    consumer is done with the slot's previous occupant, task k-N.  The
    consumer takes tasks in order, so the gate is one counter of tasks it
    has let go of.  A shared free-slot queue deadlocked: workers for tasks
    AHEAD of the consumer could hoard every released slot while the
    consumer waited on the one starved task (observed as all threads
    parked in slot_q.get on 600-chunk shards); a semaphore per slot let
    task k+N take the slot from a task k that was slow to wake up.

    Leaving the with block on any path sets the stop flag, wakes the
    waiting workers and shuts the pool down before it returns."""

    def __init__(self, ranges, n_slots: int, device):
        self.ranges = ranges  # (path, start, size) of task k
        self.device = device
        self.n_slots = n_slots
        self.slots = _Staging(n_slots, 1 << 24)
        self.gate = threading.Condition()
        self.released = 0  # tasks 0 .. released-1 no longer need their slots
        self.stop = False  # the consumer left early: fetches return at once
        self.pool = ThreadPoolExecutor(max_workers=n_slots)
        self.futs: list = []

    def __enter__(self):
        self.futs = [self.pool.submit(self._fetch, k)
                     for k in range(len(self.ranges))]
        return self

    def __exit__(self, *exc) -> None:
        with self.gate:
            self.stop = True
            self.gate.notify_all()
        self.pool.shutdown(wait=True, cancel_futures=True)

    def _fetch(self, k: int) -> None:
        with self.gate:
            while self.released <= k - self.n_slots and not self.stop:
                self.gate.wait()
        if not self.stop:
            self._read(k)

    def _read(self, k: int) -> None:
        path, start, size = self.ranges[k]
        t0 = time.perf_counter()  # read time proper: not the slot wait
        # take() waits for the previous H2D copy out of this slot
        buf = self.slots.take(k, size, self.device)
        with open(path, "rb") as f:
            f.seek(start)
            f.readinto(memoryview(buf.numpy()[:size]))
        STATS["t_read"] = STATS.get("t_read", 0.0) + time.perf_counter() - t0

    def get(self, k: int) -> torch.Tensor:
        """Task k's bytes in its slot, once they are read."""
        self.futs[k].result()
        _, _, size = self.ranges[k]
        return self.slots.bufs[k % self.n_slots][:size]

    def release(self, k: int, copied) -> None:
        """The consumer is done with task k's slot, bar the async copy out
        of it that `copied` marks.  The event is stored before the counter
        advances: the worker that gets the slot next waits for it."""
        self.slots.sent(k, copied)
        with self.gate:
            self.released = k + 1
            self.gate.notify_all()


_RETRY = object()  # the direct read gave up: read again without it


def _read_pieces_pipelined(my, columns, ctx) -> Optional[Table]:
    """Threaded disk->pinned prefetch overlapped with device decode.

    _scan_chunks lists the shard's column chunks (_Chunk) from the footers.
    The _NSLOTS reader threads of a _Prefetcher pull their byte ranges
    straight into a ring of pinned staging buffers (`f.readinto`, no
    intermediate copy); the consumer parses page headers (C++), snips the
    small dictionary page, issues the async H2D copy and releases the slot
    for reuse once the copy's event fires.  Chunks are decoded in groups of
    _GROUP_ROW_GROUPS row groups by a _GroupDecoder: each is prepared as it
    arrives (_GroupEntry) and one decompress launch covers the pages of the
    whole group.

    Columns whose every chunk is free of nulls by the footer statistics and
    holds PLAIN fixed-width values or string-dictionary codes are *direct*:
    their whole-shard tensors are allocated up front from the footer's row
    counts, and one pq_values_multi call per group checks each page's
    definition levels and writes its values at the page's place in the
    shard column (dictionary codes through a per-chunk table into the
    shard's unified dictionary).  Both page tables and the code tables of a
    group are laid out on the host by _GroupTables and go up in one pinned,
    non-blocking copy.  The kernels report bad pages through one error word
    read once at the end; if it is set, or page headers contradict the
    footer, the shard is read again with the direct path off.  All other
    chunks are finished one by one as before and joined per column with
    ops.concat_columns.  Integer and date32 columns get val_range from the
    footer's min/max on both routes.

    Disk read overlaps PCIe upload and decode kernels of other chunks
    (reference role: bodo/io/parquet_reader.cpp prefetch +
    _io_cpu_thread_pool.cpp)."""
    if DIRECT:
        saved = {k: STATS.get(k, 0) for k in ("batched", "slow", "direct")}
        out = _read_pieces_impl(my, columns, ctx, True)
        if out is not _RETRY:
            return out
        STATS.update(saved)
    return _read_pieces_impl(my, columns, ctx, False)


class _GroupDecoder:
    """The consumer's decode state: the chunks of the group being collected
    and the work already queued on the GPU."""

    def __init__(self, device, err: Optional[torch.Tensor]):
        self.device = device
        self.err = err  # error word of pq_values_multi, or None: no direct
        self.entries: List[_GroupEntry] = []
        self.row_groups = 0  # row groups begun in the current group
        # (event, chunk count) per flushed group or per-chunk fallback decode
        self.inflight: list = []
        self.pieces: dict = {}  # name -> Columns of the non-direct chunks

    def queued(self, n_chunks: int) -> None:
        """n_chunks more chunks were just queued on the current stream."""
        self.inflight.append((_record_event(self.device), n_chunks))

    def throttle(self, limit: int) -> None:
        """Backpressure: keep at most ~2x the slot depth of decoded chunks
        in flight on the GPU (unbounded enqueue ran the allocator far ahead
        of execution on 600+-chunk shards); the group being prepared
        counts, flushed work is waited for."""
        while self.inflight and (sum(c for _, c in self.inflight)
                                 + len(self.entries) >= limit):
            done, _ = self.inflight.pop(0)
            _wait_event(done)

    def flush(self) -> bool:
        """One decompress launch for every prepared chunk of the group and
        one values call for its direct chunks, then the second half of
        each other chunk's decode.  False when a chunk could not be
        decoded on any route."""
        if not self.entries:
            return True
        import bodo_amd_kernels as K

        t0 = time.perf_counter()
        preps = [e.prep for e in self.entries if e.prep is not None]
        directs = [e for e in self.entries if e.direct is not None]
        if preps:
            tables = _GroupTables(preps, directs)
            blob = torch.empty(tables.nbytes, dtype=torch.uint8,
                               device=self.device)
            _upload_staged(_TABLE_STAGING, tables.fill(blob.data_ptr()), blob)
            K.pq_decompress_multi(blob[:tables.dec_bytes], tables.n_dec)
            if tables.n_val:
                K.pq_values_multi(
                    blob[tables.dec_bytes:tables.dec_bytes + tables.val_bytes],
                    tables.n_val, self.err)
        for e in self.entries:
            self._finish(e)
        if preps:
            self.queued(len(preps))
        STATS["t_decode"] = STATS.get("t_decode", 0.0) + \
            time.perf_counter() - t0
        ok = True
        for e in self.entries:
            if e.direct is not None:
                continue
            if e.column is None:
                ok = False
                break
            self.pieces.setdefault(e.name, []).append(e.column)
        self.entries, self.row_groups = [], 0
        return ok

    def _finish(self, e: _GroupEntry) -> None:
        """After the group's launches: count a direct chunk, decode the
        second half of any other prepared chunk into e.column."""
        if e.prep is None:
            return
        prep, e.prep = e.prep, None  # drop the chunk's source and scratch
        if e.direct is not None:  # written in place by pq_values_multi
            STATS["batched"] += 1
            STATS["direct"] += 1
            return
        try:
            col = e.reader._finish_batched(prep, self.device, e.field)
        except Exception:
            col = None
        if col is not None:
            STATS["batched"] += 1
        else:  # today's per-chunk route, from the top
            col = e.reader.decode_column(self.device, e.field)
        e.column = col


def _direct_info(dc: _DirectCol, prep: Optional[_Prepared],
                 chunk: _Chunk) -> Optional[_DirectInfo]:
    """Place of a chunk in its direct column, or None when its pages are
    not what the footer promised."""
    if (prep is None or prep.mode != dc.kind or prep.total_nv != chunk.rows
            or (dc.kind == "dict" and (prep.dict_vals is None
                                       or prep.dict_vals.dtype != object))):
        return None
    lut = dc.unifier.add(prep.dict_vals) if dc.kind == "dict" else None
    return _DirectInfo(dc, chunk.row0, lut)


def _read_pieces_impl(my, columns, ctx, direct: bool):
    import bodo_amd_kernels as K

    from .. import ops

    device = ctx.device
    chunks, names, total_rows = _scan_chunks(my, columns)
    if not chunks:
        return None
    plan = _plan_direct(chunks, len(my), total_rows, device) if direct else {}
    err = torch.zeros(1, dtype=torch.int32, device=device) if plan else None
    dec = _GroupDecoder(device, err)
    metas_of: dict = {}  # name -> chunk metadata, for val_range
    field_of: dict = {}
    group_rgs, n_slots = _GROUP_ROW_GROUPS, _NSLOTS
    ranges = [(c.path, c.start, c.size) for c in chunks]
    with _Prefetcher(ranges, n_slots, device) as pf:
        for k, c in enumerate(chunks):
            if c.first_of_rg:
                if dec.row_groups >= group_rgs and not dec.flush():
                    return None
                dec.row_groups += 1
            dec.throttle(2 * n_slots)
            staged = pf.get(k)
            t0 = time.perf_counter()
            hdrs = K.pq_parse_headers(staged).numpy()
            dict_raw = None
            if hdrs.size and hdrs[0, 0] == PAGE_DICT:
                b0, c0 = int(hdrs[0, 3]), int(hdrs[0, 2])
                dict_raw = bytes(staged.numpy()[b0:b0 + c0])
            dev = torch.empty(c.size, dtype=torch.uint8, device=device)
            dev.copy_(staged, non_blocking=True)
            pf.release(k, _record_event(device))
            dc = plan.get(c.name)
            reader = _ChunkReader(
                None, c.cm, c.cm.physical_type,
                max_def=1 if c.field.nullable else 0,
                prefetched=(hdrs, dev, dict_raw, ranges[k]))
            try:
                prep = reader._prepare_batched(device,
                                               upload_metas=dc is None)
            except Exception:
                prep = None
            col = None
            dinfo = None
            if dc is not None:
                dinfo = _direct_info(dc, prep, c)
                if dinfo is None:
                    return _RETRY
            elif prep is None:
                # not eligible for the batched path: the per-chunk route
                # now, so the chunk does not hold up its group
                col = reader.decode_column(device, c.field)
                dec.queued(1)
            STATS["t_decode"] = STATS.get("t_decode", 0.0) + \
                time.perf_counter() - t0
            if prep is None and col is None:
                return None
            field_of.setdefault(c.name, c.field)
            metas_of.setdefault(c.name, []).append(c.cm)
            dec.entries.append(
                _GroupEntry(c.name, reader, c.field, prep, col, dinfo))
        if not dec.flush():
            return None
    if err is not None and int(err.item()) != 0:  # the read's one sync
        return _RETRY
    out_names = [n for n in names if n in metas_of]
    out_cols = []
    for n in out_names:
        dc = plan.get(n)
        if dc is None:
            col = ops.concat_columns(dec.pieces[n])
        elif dc.kind == "dict":
            col = Column(bt.dictionary, dc.data,
                         dictionary=dc.unifier.dictionary(),
                         length=total_rows)
        else:
            col = _fixed_column(dc.data, dc.field.type)
        vr = _val_range_from_meta(metas_of[n], field_of[n].type)
        if vr is not None:
            col.val_range = vr
        out_cols.append(col)
    return Table(out_names, out_cols, total_rows)


def _read_row_group_gpu(fp: str, rg: int, columns, ctx) -> Optional[Table]:
    chunks, names, _ = _scan_chunks([(fp, rg)], columns)
    cols, out_names = [], []
    with open(fp, "rb") as f:
        for c in chunks:
            reader = _ChunkReader(f, c.cm, c.cm.physical_type,
                                  max_def=1 if c.field.nullable else 0)
            col = reader.decode_column(ctx.device, c.field)
            if col is None:
                return None
            cols.append(col)
            out_names.append(c.name)
    ordered = [n for n in names if n in out_names]
    tbl = Table(out_names, cols)
    return tbl.select(ordered)


def _to_column(vals: torch.Tensor, dict_vals, field: pa.Field, device) -> Column:
    t = field.type
    if dict_vals is not None:
        # dictionary-encoded column: codes on device + host dictionary
        if dict_vals.dtype == object:
            return Column(bt.dictionary, vals.to(torch.int32),
                          dictionary=pa.array(list(dict_vals),
                                              type=pa.large_string()),
                          length=int(vals.numel()))
        # numeric dictionary: gather values on device
        dv = torch.from_numpy(np.ascontiguousarray(dict_vals)).to(device)
        data = dv[vals.long()]
        return _fixed_column(data, t)
    return _fixed_column(vals, t)


_TS_SCALE = {"ns": 1, "us": 1000, "ms": 1_000_000, "s": 1_000_000_000}


def _fixed_column(data: torch.Tensor, t: pa.DataType) -> Column:
    if pa.types.is_timestamp(t):
        v = data.view(torch.int64)
        scale = _TS_SCALE.get(t.unit, 1)
        if scale != 1:
            v = v * scale
        return Column(bt.timestamp_ns, v)
    if pa.types.is_date32(t):
        return Column(bt.date32, data.to(torch.int32))
    if pa.types.is_float64(t):
        return Column(bt.float64, data)
    if pa.types.is_float32(t):
        return Column(bt.float32, data)
    if pa.types.is_int64(t):
        return Column(bt.int64, data)
    if pa.types.is_int32(t):
        return Column(bt.int32, data)
    if pa.types.is_boolean(t):
        return Column(bt.boolean, data.to(torch.bool))
    kind = bt.from_numpy_dtype(np.dtype(t.to_pandas_dtype()))
    return Column(kind, data)
