"""Hand-built parquet data pages for the level, code and value decoders.

A page is put together from explicit stream elements (RLE runs, bit-packed
runs, PLAIN values) and carries the values those elements stand for: the
expectation is the list handed to the builder, no decoder stands between
the input and it.  spec_decode_hybrid, written from the format description,
only proves the builder's streams valid."""

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

FILL = 0xEE    # alignment gaps and the scratch padding: never zero
CANARY = 0xA5  # destinations the caller allocates


# ---------------------------------------------------------------------
# run encoders
# ---------------------------------------------------------------------

def varint(v: int) -> bytes:
    assert v >= 0
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def rle_run(value: int, count: int, bitwidth: int) -> bytes:
    """Header count << 1, then ceil(bitwidth / 8) value bytes."""
    assert 0 <= value < 1 << bitwidth and count >= 0
    return varint(count << 1) + value.to_bytes((bitwidth + 7) // 8, "little")


def bitpacked_run(values, bitwidth: int, pad_bits: int = 0,
                  groups=None) -> bytes:
    """Header (groups << 1) | 1, then groups * bitwidth bytes, LSB first.
    The run carries groups * 8 values; those past len(values) are padding:
    all bits 0 (as writers emit) or, with pad_bits=1, all bits 1."""
    assert pad_bits in (0, 1)
    if groups is None:
        groups = (len(values) + 7) // 8
    assert groups >= 1 and groups * 8 >= len(values)
    big = 0
    for i, v in enumerate(values):
        assert 0 <= v < 1 << bitwidth
        big |= int(v) << (i * bitwidth)
    if pad_bits:
        n_pad = (groups * 8 - len(values)) * bitwidth
        big |= ((1 << n_pad) - 1) << (len(values) * bitwidth)
    return varint((groups << 1) | 1) + big.to_bytes(groups * bitwidth, "little")


@dataclass
class Rle:
    value: int
    count: int
    declared: Optional[int] = None  # header count; > count: a clipped run


@dataclass
class Packed:
    values: list
    pad_bits: int = 0
    groups: Optional[int] = None  # more than the values need: padding groups


@dataclass
class Section:
    """An encoded piece of a page and what it stands for."""
    data: bytes
    values: list
    # (out_start, count, kind, value | byte offset of the packed bytes in
    # data): what a parser of data must find
    runs: list = field(default_factory=list)
    bitwidth: int = 0
    kind: str = "raw"  # levels | codes | fixed | strings | raw
    esize: int = 0
    str_off: list = field(default_factory=list)  # strings: offset of each


def _encode_runs(runs, bitwidth, base):
    """(stream, values, run table) of runs; base is where the stream will
    sit in its section.  Only the last run may hold fewer values than its
    header announces: anything else cannot be expressed."""
    body = bytearray()
    values, table = [], []
    for k, r in enumerate(runs):
        last = k == len(runs) - 1
        if isinstance(r, Rle):
            declared = r.count if r.declared is None else r.declared
            assert declared >= r.count
            if declared != r.count and not last:
                raise ValueError("only the last run can be clipped")
            table.append((len(values), r.count, 0, r.value))
            body += rle_run(r.value, declared, bitwidth)
            values += [r.value] * r.count
        else:
            vals = [int(v) for v in r.values]
            groups = (len(vals) + 7) // 8 if r.groups is None else r.groups
            assert groups * 8 >= len(vals)
            if groups * 8 != len(vals) and not last:
                raise ValueError("a bit-packed run that is not the last of "
                                 "its section holds groups * 8 values")
            enc = bitpacked_run(vals, bitwidth, r.pad_bits, groups)
            hdr = len(varint((groups << 1) | 1))
            table.append((len(values), len(vals), 1, base + len(body) + hdr))
            body += enc
            values += vals
    return bytes(body), values, table


def level_section(runs) -> Section:
    """4-byte little-endian length + the hybrid stream at bit width 1."""
    body, values, table = _encode_runs(runs, 1, 4)
    return Section(len(body).to_bytes(4, "little") + body, values, table, 1,
                   "levels")


def codes_section(bitwidth: int, runs) -> Section:
    """Bit-width byte + the hybrid stream."""
    body, values, table = _encode_runs(runs, bitwidth, 1)
    return Section(bytes([bitwidth]) + body, values, table, bitwidth, "codes")


def raw_codes(data: bytes, values=()) -> Section:
    """A codes section given byte for byte (malformed streams)."""
    return Section(bytes(data), list(values), [], data[0] if data else 0,
                   "codes")


def plain_fixed(values: np.ndarray) -> Section:
    values = np.ascontiguousarray(values)
    assert values.dtype.itemsize in (4, 8)
    return Section(values.tobytes(), values, kind="fixed",
                   esize=values.dtype.itemsize)


def plain_byte_array(strings: List[bytes]) -> Section:
    body = bytearray()
    offs = []
    for s in strings:
        body += len(s).to_bytes(4, "little")
        offs.append(len(body))
        body += s
    return Section(bytes(body), list(strings), kind="strings", str_off=offs)


@dataclass
class Page:
    data: bytes
    nv: int              # values including nulls
    has_def: bool
    mask: np.ndarray     # uint8[nv], 1 = valid
    n_valid: int
    val_data_off: int    # 4 + lvl_len, 0 without a level section
    body: Section
    levels: Optional[Section]

    @property
    def values(self):
        return self.body.values


def page(levels: Optional[Section], body: Section, nv=None) -> Page:
    """nv: only for a malformed body that holds fewer values than the page
    announces."""
    if levels is None:
        n = len(body.values) if nv is None else nv
        return Page(body.data, n, False, np.ones(n, np.uint8), n, 0, body,
                    None)
    mask = np.array(levels.values, dtype=np.uint8)
    n_valid = int(mask.sum())
    if nv is None:
        assert len(body.values) == n_valid, (len(body.values), n_valid)
    return Page(levels.data + body.data, len(mask), True, mask, n_valid,
                len(levels.data), body, levels)


def expected_runs(section: Section, n: int, shift: int = 0):
    """The run table a parser finds for the first n values of section, byte
    offsets moved by shift and turned into bit offsets."""
    out = []
    for start, count, kind, v in section.runs:
        if start >= n:
            break
        out.append((start, min(count, n - start), kind,
                    (v + shift) * 8 if kind else v))
    return out


# ---------------------------------------------------------------------
# decoder from the format description: validates the builder only
# ---------------------------------------------------------------------

def spec_decode_hybrid(data: bytes, bitwidth: int, n: int) -> list:
    """The first n values of an RLE / bit-packed hybrid stream.  A
    bit-packed run is read as one big integer."""
    out, pos = [], 0
    width_bytes = (bitwidth + 7) // 8
    while len(out) < n:
        h = shift = 0
        while True:
            if pos >= len(data):
                raise ValueError(f"stream ends after {len(out)} of {n}")
            b = data[pos]
            pos += 1
            h |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        if h & 1:
            nbytes = (h >> 1) * bitwidth
            if pos + nbytes > len(data):
                raise ValueError("bit-packed run past the end")
            big = int.from_bytes(data[pos:pos + nbytes], "little")
            pos += nbytes
            take = min((h >> 1) * 8, n - len(out))
            out += [(big >> (i * bitwidth)) & ((1 << bitwidth) - 1)
                    for i in range(take)]
        else:
            if pos + width_bytes > len(data):
                raise ValueError("RLE value past the end")
            v = int.from_bytes(data[pos:pos + width_bytes], "little")
            pos += width_bytes
            out += [v] * min(h >> 1, n - len(out))
    return out


# ---------------------------------------------------------------------
# placement
# ---------------------------------------------------------------------

def all_valid_levels(n: int, resid: int, pad_bits: int = 0) -> Section:
    """n levels, all 1, in a section of 4 + lvl_len = resid (mod 8) bytes:
    an RLE run and a bit-packed run whose last groups are padding."""
    lvl_len = 8 + (resid - 4) % 8
    if n <= 1:
        runs = [Packed([1] * n, pad_bits, groups=lvl_len - 1)]
    else:
        in_packed = min(n - 1, 8)
        rle = Rle(1, n - in_packed)
        used = len(rle_run(1, rle.count, 1))
        runs = [rle, Packed([1] * in_packed, pad_bits,
                            groups=lvl_len - used - 1)]
    sec = level_section(runs)
    assert len(sec.data) % 8 == resid and len(sec.values) == n
    return sec


@dataclass
class Layout:
    scratch: np.ndarray  # uint8
    offs: list           # page i starts at scratch[offs[i]]
    metas: np.ndarray    # PageMeta table of the per-chunk entry points
    mask: np.ndarray     # expected whole mask
    n_valid: np.ndarray  # int32 per page
    vdo: np.ndarray      # int32 per page
    dense_off: np.ndarray  # int64 per page: exclusive cumsum of n_valid


def place(pages: List[Page], meta_dt, shifts=None) -> Layout:
    """Pages back to back in scratch at 8-aligned offsets (+ shifts[i] for
    entry points that take any byte address), gaps and the reader's 16
    bytes of padding at the end filled with FILL: what follows a page's
    values is never zero."""
    offs, at = [], 0
    for i, p in enumerate(pages):
        at = (at + 7) & ~7
        at += shifts[i] if shifts is not None else 0
        offs.append(at)
        at += len(p.data)
    size = ((at + 7) & ~7) + 16
    scratch = np.full(size, FILL, dtype=np.uint8)
    for o, p in zip(offs, pages):
        scratch[o:o + len(p.data)] = np.frombuffer(p.data, np.uint8)
    n = len(pages)
    metas = np.zeros(n, dtype=meta_dt)
    nv = np.array([p.nv for p in pages], dtype=np.int64)
    metas["dst_off"] = offs
    metas["val_off"] = np.cumsum(nv) - nv
    metas["dst_len"] = [len(p.data) for p in pages]
    metas["nv"] = nv
    metas["flags"] = [1 if p.has_def else 0 for p in pages]
    n_valid = np.array([p.n_valid for p in pages], dtype=np.int32)
    return Layout(
        scratch, offs, metas,
        np.concatenate([p.mask for p in pages] + [np.zeros(0, np.uint8)]),
        n_valid,
        np.array([p.val_data_off for p in pages], dtype=np.int32),
        np.cumsum(n_valid, dtype=np.int64) - n_valid)


@dataclass
class OutPlan:
    """Destinations of a pq_values_multi launch inside one canary buffer."""
    size: int
    offs: list  # byte offset of each page's output
    lens: list  # bytes each page writes when it is good


def plan_outputs(nbytes: List[int], align4_only=None) -> OutPlan:
    """8-aligned destinations with guard gaps; align4_only[i] puts page i at
    an address that is 4- but not 8-byte aligned."""
    offs, at = [], 16
    for i, nb in enumerate(nbytes):
        at = (at + 7) & ~7
        if align4_only is not None and align4_only[i]:
            at += 4
        offs.append(at)
        at += nb + 12
    return OutPlan(((at + 7) & ~7) + 16, offs, list(nbytes))


def check_outputs(out: np.ndarray, plan: OutPlan, expected: list,
                  skip=()):
    """out: the canary buffer after the launch; expected[i]: the bytes of
    page i, or None for a page that must be left unwritten.  Pages in skip
    may hold anything inside their own range.  Everything else keeps the
    canary."""
    untouched = np.ones(len(out), dtype=bool)
    for i, (o, nb) in enumerate(zip(plan.offs, plan.lens)):
        if i in skip:
            untouched[o:o + nb] = False
            continue
        exp = expected[i]
        if exp is None:
            continue
        exp = np.frombuffer(bytes(exp), np.uint8)
        assert len(exp) == nb, (i, len(exp), nb)
        got = out[o:o + nb]
        if not np.array_equal(got, exp):
            first = int(np.nonzero(got != exp)[0][0])
            raise AssertionError(
                f"page {i} of {nb} bytes differs first at byte {first}")
        untouched[o:o + nb] = False
    bad = np.nonzero(out[untouched] != CANARY)[0]
    assert len(bad) == 0, \
        f"canary overwritten at byte {int(np.nonzero(untouched)[0][bad[0]])}"
