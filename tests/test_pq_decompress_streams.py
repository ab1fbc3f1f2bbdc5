"""Snappy page decompression (K.pq_decompress / K.pq_decompress_multi)
on hand-built and codec-produced streams.

The CPU part proves every stream valid: pyarrow's snappy codec must decode
it to the bytes the builder predicts.  The GPU part feeds the same streams
to both native entry points and compares byte for byte with pyarrow's
output; canary bytes around every destination must survive."""

import functools

import numpy as np
import pyarrow as pa
import pytest
import torch

CANARY = 0xA5


# ---------------------------------------------------------------------
# stream builder
# ---------------------------------------------------------------------

class Snappy:
    """Emits explicit snappy elements and tracks the bytes they decode to."""

    def __init__(self):
        self.body = bytearray()
        self.out = bytearray()

    def literal(self, data: bytes, nb=None):
        """nb: length bytes after the tag (0 = length in the tag)."""
        n = len(data)
        assert n >= 1
        if nb is None:
            nb = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
        if nb == 0:
            assert n <= 60
            self.body.append((n - 1) << 2)
        else:
            assert n - 1 < 1 << (8 * nb)
            self.body.append((59 + nb) << 2)
            self.body += (n - 1).to_bytes(nb, "little")
        self.body += data
        self.out += data
        return self

    def _emit_copy(self, ln, off):
        assert 1 <= off <= len(self.out)
        for _ in range(ln):
            self.out.append(self.out[-off])

    def copy1(self, ln, off):
        assert 4 <= ln <= 11 and off < 2048
        self.body.append(1 | (ln - 4) << 2 | (off >> 8) << 5)
        self.body.append(off & 0xFF)
        self._emit_copy(ln, off)
        return self

    def copy2(self, ln, off):
        assert 1 <= ln <= 64 and off < 1 << 16
        self.body.append(2 | (ln - 1) << 2)
        self.body += off.to_bytes(2, "little")
        self._emit_copy(ln, off)
        return self

    def copy4(self, ln, off):
        assert 1 <= ln <= 64
        self.body.append(3 | (ln - 1) << 2)
        self.body += off.to_bytes(4, "little")
        self._emit_copy(ln, off)
        return self

    def stream(self) -> bytes:
        n = len(self.out)
        pre = bytearray()
        while True:
            b = n & 0x7F
            n >>= 7
            if n:
                pre.append(b | 0x80)
            else:
                pre.append(b)
                break
        return bytes(pre + self.body)


def _rb(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _page(s: Snappy):
    return (s.stream(), True, bytes(s.out))


def _case_forms(rng):
    """Each element form alone (after the literal a copy needs) and mixed."""
    pages = []
    for n in (1, 60, 61, 256, 257, 65536):
        pages.append(_page(Snappy().literal(_rb(rng, n))))
    # non-minimal 3- and 4-byte literal length forms
    pages.append(_page(Snappy().literal(_rb(rng, 300), nb=3)))
    pages.append(_page(Snappy().literal(_rb(rng, 70), nb=4)))
    for ln in range(4, 12):
        pages.append(_page(Snappy().literal(_rb(rng, 2047))
                           .copy1(ln, 2047).copy1(ln, ln)))
    for ln in (1, 2, 31, 32, 33, 63, 64):
        pages.append(_page(Snappy().literal(_rb(rng, 3000))
                           .copy2(ln, 3000).copy2(ln, max(ln, 1))))
    for ln in (1, 17, 64):
        pages.append(_page(Snappy().literal(_rb(rng, 70000))
                           .copy4(ln, 70000).copy4(ln, 66000)))
    s = Snappy()  # mixed, ~200 KB
    s.literal(_rb(rng, 5000))
    while len(s.out) < 200_000:
        k = int(rng.integers(0, 5))
        cur = len(s.out)
        if k == 0:
            s.literal(_rb(rng, int(rng.integers(1, 90))))
        elif k == 1:
            ln = int(rng.integers(4, 12))
            s.copy1(ln, int(rng.integers(ln, 2048)))
        elif k == 2:
            ln = int(rng.integers(1, 65))
            s.copy2(ln, int(rng.integers(1, min(cur, 65535) + 1)))
        elif k == 3:
            ln = int(rng.integers(1, 65))
            s.copy4(ln, int(rng.integers(1, cur + 1)))
        else:
            s.literal(_rb(rng, int(rng.integers(61, 3000))))
    pages.append(_page(s))
    return pages


def _case_overlap(rng):
    pages = []
    for off in (1, 2, 3, 7, 8):
        pages.append(_page(Snappy().literal(_rb(rng, 8)).copy2(64, off)
                           .literal(_rb(rng, 5)).copy2(64, off)))
    return pages


def _case_chain(rng):
    s = Snappy().literal(_rb(rng, 8))
    for _ in range(200):
        s.copy1(8, 8)
    return [_page(s)]


def _case_straddle(rng):
    # a long literal ends a batch; the copy's source is half that literal,
    # half the short literal that opens the next batch
    a = Snappy().literal(_rb(rng, 40)).literal(_rb(rng, 4)).copy2(8, 8)
    # the same across a batch filled by 64 short elements
    b = Snappy()
    for _ in range(64):
        b.literal(_rb(rng, 2))
    b.literal(_rb(rng, 4)).copy2(8, 8).copy1(8, 12)
    # every split of an 8-byte source across the boundary
    pages = [_page(a), _page(b)]
    for k in range(1, 8):
        c = Snappy().literal(_rb(rng, 50)).literal(_rb(rng, k)).copy1(8, 8)
        pages.append(_page(c))
    return pages


def _case_window_sweep(rng):
    pages = []
    for n in range(1, 1025):
        s = Snappy().literal(_rb(rng, n)).literal(_rb(rng, 8))
        s.copy1(8, 8).copy2(6, 10).literal(_rb(rng, 3)).copy2(12, 20)
        s.copy4(9, 9).copy1(4, 5)
        pages.append(_page(s))
    return pages


def _case_odd(rng):
    pages = [_page(Snappy().literal(b"\x7f"))]  # 1-byte page
    for n in (3, 7, 9, 13, 1001, 4099):
        s = Snappy().literal(_rb(rng, min(5, n)))
        while len(s.out) + 11 < n:
            s.copy1(int(rng.integers(4, 8)), int(rng.integers(4, 6)))
        if n > len(s.out):
            s.literal(_rb(rng, n - len(s.out)))
        assert len(s.out) == n
        pages.append(_page(s))
    return pages


def _case_mixed_flags(rng):
    pages = _case_odd(rng)[:4]
    for n in (1, 15, 16, 17, 1000, 70001):
        raw = _rb(rng, n)
        pages.append((raw, False, raw))
    pages += _case_overlap(rng)[:2]
    return pages


def _case_codec(rng):
    codec = pa.Codec("snappy")
    text = (b"the quick brown fox jumps over the lazy dog; " * 3000)[:120_000]
    raws = [
        rng.integers(1, 266, 131072).astype(np.int64).tobytes(),
        _rb(rng, 1 << 20),
        bytes(1 << 20),
        text,
    ]
    return [(codec.compress(r, asbytes=True), True, r) for r in raws]


CASES = {
    "forms": _case_forms, "overlap": _case_overlap, "chain": _case_chain,
    "straddle": _case_straddle, "window_sweep": _case_window_sweep,
    "odd": _case_odd, "mixed_flags": _case_mixed_flags, "codec": _case_codec,
}


@functools.lru_cache(maxsize=None)
def _pages(kind):
    """(stream, is_snappy, builder's bytes, pyarrow's bytes) per page."""
    codec = pa.Codec("snappy")
    out = []
    for stream, snappy, exp in CASES[kind](np.random.default_rng(1234)):
        ref = exp
        if snappy:
            ref = codec.decompress(stream, decompressed_size=len(exp),
                                   asbytes=True)
        out.append((stream, snappy, exp, ref))
    return out


@pytest.mark.parametrize("kind", sorted(CASES))
def test_streams_are_valid_snappy(kind):
    pages = _pages(kind)
    assert pages
    for i, (stream, snappy, exp, ref) in enumerate(pages):
        assert ref == exp, (kind, i)


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------

def _layout(pages, n_tensors):
    """Place pages round-robin over n_tensors source/scratch pairs: sources
    at unaligned offsets, destinations 8-aligned with a canary gap."""
    srcs = [bytearray() for _ in range(n_tensors)]
    dst_sizes = [0] * n_tensors
    place = []
    for i, (stream, snappy, exp, ref) in enumerate(pages):
        t = i % n_tensors
        srcs[t] += bytes((i * 7) % 13 + 1)  # unaligned src_off
        src_off = len(srcs[t])
        srcs[t] += stream
        dst_off = dst_sizes[t]
        dst_sizes[t] = ((dst_off + len(ref) + 7) & ~7) + 24
        place.append((t, src_off, dst_off))
    dst_sizes = [d + 64 for d in dst_sizes]
    return srcs, dst_sizes, place


def _check(pages, place, scratches):
    host = [s.cpu().numpy() for s in scratches]
    untouched = [np.ones(len(h), dtype=bool) for h in host]
    for (stream, snappy, exp, ref), (t, src_off, dst_off) in zip(pages, place):
        got = host[t][dst_off:dst_off + len(ref)].tobytes()
        if got != ref:
            a = np.frombuffer(got, np.uint8)
            b = np.frombuffer(ref, np.uint8)
            first = int(np.nonzero(a != b)[0][0])
            raise AssertionError(
                f"page of {len(ref)} bytes differs first at byte {first}")
        untouched[t][dst_off:dst_off + len(ref)] = False
    for h, u in zip(host, untouched):
        assert (h[u] == CANARY).all(), "canary bytes overwritten"


def _run(kind, multi):
    import bodo_amd_kernels as K
    from bodo_amd.io import parquet_gpu as g

    pages = _pages(kind)
    n_t = 3 if multi else 1
    srcs, dst_sizes, place = _layout(pages, n_t)
    dev = "cuda"
    src_t = [torch.from_numpy(np.frombuffer(bytes(s), np.uint8).copy()).to(dev)
             for s in srcs]
    scr_t = [torch.full((d,), CANARY, dtype=torch.uint8, device=dev)
             for d in dst_sizes]
    n = len(pages)
    if multi:
        tbl = np.zeros(n, dtype=g._PAGEPTR_DT)
        for i, ((stream, snappy, exp, ref), (t, so, do)) in enumerate(
                zip(pages, place)):
            tbl[i] = (src_t[t].data_ptr() + so, scr_t[t].data_ptr() + do,
                      len(stream), len(ref), g._PQF_SNAPPY if snappy else 0, 0)
        K.pq_decompress_multi(torch.from_numpy(tbl.view(np.uint8)).to(dev), n)
    else:
        tbl = np.zeros(n, dtype=g._PAGEMETA_DT)
        for i, ((stream, snappy, exp, ref), (t, so, do)) in enumerate(
                zip(pages, place)):
            tbl[i] = (so, do, 0, len(stream), len(ref), 0,
                      g._PQF_SNAPPY if snappy else 0)
        K.pq_decompress(src_t[0], torch.from_numpy(tbl.view(np.uint8)).to(dev),
                        n, scr_t[0])
    torch.cuda.synchronize()
    _check(pages, place, scr_t)


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("kind", sorted(CASES))
def test_gpu_decompress_streams(kind, multi):
    _run(kind, multi)
