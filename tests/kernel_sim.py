"""Bit-faithful host simulators of the csrc/parquet.hip kernels with hard
bounds assertions.  Used by CPU tests to validate the device decode logic
(index arithmetic, parse state machines) without a GPU; any out-of-bounds
access that would be a hardware fault on the MI355X raises here."""

import numpy as np
import torch

PQF_HAS_DEF = 1
PQF_SNAPPY = 2


class Buf:
    """Bounds-checked byte view."""

    def __init__(self, arr: np.ndarray, lo=0, hi=None, slack=0):
        self.a = arr
        self.lo = lo
        self.hi = len(arr) if hi is None else hi
        self.slack = slack  # allowed overread (scratch pad)

    def __getitem__(self, i):
        assert self.lo + i < self.hi + self.slack, \
            f"OOB read at +{i} (len {self.hi - self.lo}, slack {self.slack})"
        assert i >= 0, f"negative index {i}"
        j = self.lo + i
        return int(self.a[j]) if j < len(self.a) else 0

    def set(self, i, v):
        assert 0 <= i and self.lo + i < self.hi, f"OOB write at +{i}"
        self.a[self.lo + i] = v


def sim_decompress(src: np.ndarray, metas, scratch: np.ndarray):
    for pm in metas:
        inb = Buf(src, int(pm["src_off"]), int(pm["src_off"]) + int(pm["src_len"]))
        out = Buf(scratch, int(pm["dst_off"]), int(pm["dst_off"]) + int(pm["dst_len"]))
        if not (int(pm["flags"]) & PQF_SNAPPY):
            for i in range(int(pm["dst_len"])):
                out.set(i, inb[i])
            continue
        ip, opos = 0, 0
        src_len, dst_len = int(pm["src_len"]), int(pm["dst_len"])
        while inb[ip] & 0x80:
            ip += 1
        ip += 1
        while ip < src_len and opos < dst_len:
            tag = inb[ip]
            k = tag & 3
            if k == 0:
                ln = (tag >> 2) + 1
                hl = 1
                if ln > 60:
                    nb = ln - 60
                    ln = 0
                    for i in range(nb):
                        ln |= inb[ip + 1 + i] << (8 * i)
                    ln += 1
                    hl = 1 + nb
                srcoff = ip + hl
                ip += hl + ln
                assert ln > 0 and opos + ln <= dst_len, "literal overrun"
                for i in range(ln):
                    out.set(opos + i, inb[srcoff + i])
            else:
                if k == 1:
                    ln = ((tag >> 2) & 7) + 4
                    off = ((tag >> 5) << 8) | inb[ip + 1]
                    hl = 2
                elif k == 2:
                    ln = (tag >> 2) + 1
                    off = inb[ip + 1] | (inb[ip + 2] << 8)
                    hl = 3
                else:
                    ln = (tag >> 2) + 1
                    off = (inb[ip + 1] | (inb[ip + 2] << 8)
                           | (inb[ip + 3] << 16) | (inb[ip + 4] << 24))
                    hl = 5
                ip += hl
                assert 0 < off <= opos, f"bad copy offset {off} at opos {opos}"
                assert opos + ln <= dst_len, "copy overrun"
                for i in range(ln):
                    out.set(opos + i, out[opos - off + (i % off if off < ln else i)])
            opos += ln
        assert opos == dst_len, f"decompress short: {opos} != {dst_len}"


def _varint(buf: Buf, pos):
    out, shift = 0, 0
    while True:
        v = buf[pos]
        pos += 1
        out |= (v & 0x7F) << shift
        if not (v & 0x80):
            return out, pos
        shift += 7
        assert shift < 64, "runaway varint"


def sim_def_levels(scratch, metas, bitwidth, max_def, total_nv, slack=16):
    mask = np.zeros(total_nv, dtype=np.uint8)
    n_valid = np.zeros(len(metas), dtype=np.int32)
    vdo = np.zeros(len(metas), dtype=np.int32)
    for p, pm in enumerate(metas):
        base = Buf(scratch, int(pm["dst_off"]),
                   int(pm["dst_off"]) + int(pm["dst_len"]), slack)
        nv = int(pm["nv"])
        mv = Buf(mask, int(pm["val_off"]), int(pm["val_off"]) + nv)
        if not (int(pm["flags"]) & PQF_HAS_DEF):
            for i in range(nv):
                mv.set(i, 1)
            n_valid[p] = nv
            continue
        lvl_len = base[0] | (base[1] << 8) | (base[2] << 16) | (base[3] << 24)
        vdo[p] = 4 + lvl_len
        lv = Buf(scratch, int(pm["dst_off"]) + 4,
                 int(pm["dst_off"]) + int(pm["dst_len"]), slack)
        pos, out, valid = 0, 0, 0
        wb = (bitwidth + 7) // 8
        while out < nv and pos < lvl_len:
            h, pos = _varint(lv, pos)
            if h & 1:
                groups = h >> 1
                count = min(groups * 8, nv - out)
                bitoff = pos * 8
                for i in range(count):
                    bp = bitoff + i * bitwidth
                    w = lv[bp >> 3] | (lv[(bp >> 3) + 1] << 8)
                    v = (w >> (bp & 7)) & ((1 << bitwidth) - 1)
                    ok = 1 if v == max_def else 0
                    mv.set(out + i, ok)
                    valid += ok
                pos += groups * bitwidth
            else:
                count = min(h >> 1, nv - out)
                val = 0
                for i in range(wb):
                    val |= lv[pos + i] << (8 * i)
                pos += wb
                ok = 1 if val == max_def else 0
                for i in range(count):
                    mv.set(out + i, ok)
                valid += ok * count
            out += count
        assert out == nv, f"def levels short: {out} != {nv}"
        n_valid[p] = valid
    return mask, n_valid, vdo


def sim_expand_codes(scratch, metas, vdo, dense_off, n_valid, dense_total,
                     slack=16):
    out = np.zeros(dense_total, dtype=np.int32)
    for p, pm in enumerate(metas):
        start = int(pm["dst_off"]) + (int(vdo[p]) if vdo is not None else 0)
        base = Buf(scratch, start,
                   int(pm["dst_off"]) + int(pm["dst_len"]), slack)
        nval = int(n_valid[p]) if n_valid is not None else int(pm["nv"])
        o = Buf(out, int(dense_off[p]), int(dense_off[p]) + nval)
        if start >= int(pm["dst_off"]) + int(pm["dst_len"]):
            # no codes section: the kernel reads nothing, not even the
            # bit-width byte
            assert nval == 0, f"codes short: 0 != {nval}"
            continue
        bitwidth = base[0]
        d = Buf(scratch, start + 1, int(pm["dst_off"]) + int(pm["dst_len"]),
                slack)
        if bitwidth == 0:
            for i in range(nval):
                o.set(i, 0)
            continue
        assert 0 < bitwidth <= 24, f"bitwidth {bitwidth}"
        wb = (bitwidth + 7) // 8
        pos, outp = 0, 0
        dlen = int(pm["dst_len"]) - (start + 1 - int(pm["dst_off"]))
        while outp < nval and pos < dlen:
            h, pos = _varint(d, pos)
            if h & 1:
                groups = h >> 1
                count = min(groups * 8, nval - outp)
                bitoff = pos * 8
                for i in range(count):
                    bp = bitoff + i * bitwidth
                    byte = bp >> 3
                    w = (d[byte] | (d[byte + 1] << 8) | (d[byte + 2] << 16)
                         | (d[byte + 3] << 24))
                    o.set(outp + i, (w >> (bp & 7)) & ((1 << bitwidth) - 1))
                pos += groups * bitwidth
            else:
                count = min(h >> 1, nval - outp)
                val = 0
                for i in range(wb):
                    val |= d[pos + i] << (8 * i)
                pos += wb
                for i in range(count):
                    o.set(outp + i, val)
            outp += count
        assert outp == nval, f"codes short: {outp} != {nval}"
    return out


def sim_copy_fixed(scratch, metas, vdo, dense_off, n_valid, esize,
                   dense_total):
    out = np.zeros(dense_total * esize, dtype=np.uint8)
    for p, pm in enumerate(metas):
        start = int(pm["dst_off"]) + (int(vdo[p]) if vdo is not None else 0)
        nval = int(n_valid[p]) if n_valid is not None else int(pm["nv"])
        nbytes = nval * esize
        assert start + nbytes <= int(pm["dst_off"]) + int(pm["dst_len"]), \
            f"fixed copy source overrun page {p}"
        do = int(dense_off[p]) * esize
        out[do:do + nbytes] = scratch[start:start + nbytes]
    return out


def sim_byte_array(scratch, metas, vdo, dense_off, n_valid, dense_total):
    lengths = np.zeros(dense_total, dtype=np.int32)
    src_abs = np.zeros(dense_total, dtype=np.int64)
    for p, pm in enumerate(metas):
        voff = int(pm["dst_off"]) + (int(vdo[p]) if vdo is not None else 0)
        s = Buf(scratch, voff, int(pm["dst_off"]) + int(pm["dst_len"]))
        nval = int(n_valid[p]) if n_valid is not None else int(pm["nv"])
        pos = 0
        for i in range(nval):
            ln = s[pos] | (s[pos + 1] << 8) | (s[pos + 2] << 16) | (s[pos + 3] << 24)
            lengths[int(dense_off[p]) + i] = ln
            src_abs[int(dense_off[p]) + i] = voff + pos + 4
            pos += 4 + ln
        assert pos <= int(pm["dst_len"]) - (voff - int(pm["dst_off"])), \
            f"byte array walk overran page {p}"
    return lengths, src_abs


# ---------------------------------------------------------------------
# kernels that take tables of absolute addresses (pq_decompress_multi,
# pq_values_multi).  The simulators never touch a raw address: an
# AddressMap of the tensors the reader allocated turns [addr, addr + n)
# into (bytes of one tensor, offset), and asserts when the range is not
# wholly inside one of them.
# ---------------------------------------------------------------------

PQK_CODES = 0
PQE_PREFIX = 1
PQE_LEVELS = 2
PQE_ENTRY = 4
PQE_CODES = 8
PQE_RANGE = 16


class AddressMap:
    """Tensors by address.  Holds them, so no address is handed out twice
    while the map lives."""

    def __init__(self):
        self.tensors = {}  # data_ptr -> flat uint8 tensor over its bytes

    def add(self, t: torch.Tensor):
        assert t.is_contiguous()
        self.tensors[t.data_ptr()] = t.reshape(-1).view(torch.uint8)

    def find(self, addr: int, n: int):
        """(base address, bytes) of the tensor holding [addr, addr + n)."""
        assert n >= 0, f"negative length {n}"
        for base, t in self.tensors.items():
            if base <= addr < base + t.numel() or (n == 0 and addr == base):
                assert addr + n <= base + t.numel(), \
                    f"[{addr:#x}, +{n}) runs {addr + n - base - t.numel()} " \
                    f"bytes past its tensor of {t.numel()}"
                return base, t.numpy()
        raise AssertionError(f"[{addr:#x}, +{n}) is in no recorded tensor")

    def resolve(self, addr: int, n: int):
        base, arr = self.find(addr, n)
        return arr, addr - base


def sim_decompress_multi(pages, amap: AddressMap):
    """pages: PagePtr entries (src, dst, src_len, dst_len, flags)."""
    for pm in pages:
        src, so = amap.resolve(int(pm["src"]), int(pm["src_len"]))
        dst, do = amap.resolve(int(pm["dst"]), int(pm["dst_len"]))
        sim_decompress(src, [{"src_off": so, "src_len": pm["src_len"],
                              "dst_off": do, "dst_len": pm["dst_len"],
                              "flags": pm["flags"]}], dst)


def _varint32(b: Buf, pos, end):
    """pq_varint32: at most 5 bytes inside [pos, end); None when it runs
    out."""
    v = 0
    for shift in range(0, 35, 7):
        if pos >= end:
            return None, pos
        c = b[pos]
        pos += 1
        v |= (c & 0x7F) << shift
        if not (c & 0x80):
            return v, pos
    return None, pos


def _check_levels(page: Buf, dst_len, nv):
    """pq_check_levels: (PQE_* bits, offset of the values section)."""
    if dst_len < 4:
        return PQE_PREFIX, 4
    lvl_len = page[0] | (page[1] << 8) | (page[2] << 16) | (page[3] << 24)
    if lvl_len >= 1 << 31:
        lvl_len -= 1 << 32
    if lvl_len < 0 or 4 + lvl_len > dst_len:
        return PQE_PREFIX, 4 + lvl_len
    lv = Buf(page.a, page.lo + 4, page.hi)
    bad, pos, out = 0, 0, 0
    while out < nv and pos < lvl_len:
        h, pos = _varint32(lv, pos, lvl_len)
        if h is None:
            break
        if h & 1:  # bit-packed, 1 bit per level
            groups = h >> 1
            if pos + groups > lvl_len:
                break
            count = min(groups * 8, nv - out)
            full, rest = count >> 3, count & 7
            for i in range(full):
                if lv[pos + i] != 0xFF:
                    bad = PQE_LEVELS
            if rest and lv[pos + full] & ((1 << rest) - 1) != (1 << rest) - 1:
                bad = PQE_LEVELS
            pos += groups
        else:
            count = min(h >> 1, nv - out)
            if pos >= lvl_len:
                break
            if count and lv[pos] != 1:
                bad = PQE_LEVELS
            pos += 1
        out += count
    if out != nv:
        bad |= PQE_LEVELS
    return bad, 4 + lvl_len


def _expand_codes_checked(d: Buf, dlen, nval, o, lut, code_lim):
    """pq_expand_codes_page: d starts at the bit-width byte and may be read
    up to d.slack bytes past dlen; o is the int32 destination of nval
    codes.  Returns PQE_CODES / PQE_RANGE bits."""
    if dlen < 1:
        return PQE_CODES if nval else 0
    bitwidth = d[0]
    d = Buf(d.a, d.lo + 1, d.hi, d.slack)
    dlen -= 1

    def store(i, c):
        assert 0 <= i < nval, f"code store at {i} of {nval}"
        if c < code_lim:
            o[i] = lut[c] if lut is not None else c
            return 0
        return PQE_RANGE

    if bitwidth == 0:
        if not nval:
            return 0
        if not code_lim:
            return PQE_RANGE
        o[:nval] = lut[0] if lut is not None else 0
        return 0
    if bitwidth > 24:
        return PQE_CODES
    wb = (bitwidth + 7) // 8
    st, pos, outp = 0, 0, 0
    while outp < nval and pos < dlen:
        h, pos = _varint32(d, pos, dlen)
        if h is None:
            break
        if h & 1:
            groups = h >> 1
            if pos + groups * bitwidth > dlen:
                break
            count = min(groups * 8, nval - outp)
            bitoff = pos * 8
            for i in range(count):
                bp = bitoff + i * bitwidth
                byte = bp >> 3
                w = (d[byte] | (d[byte + 1] << 8) | (d[byte + 2] << 16)
                     | (d[byte + 3] << 24))
                st |= store(outp + i, (w >> (bp & 7)) & ((1 << bitwidth) - 1))
            pos += groups * bitwidth
        else:
            count = min(h >> 1, nval - outp)
            if pos + wb > dlen:
                break
            val = 0
            for i in range(wb):
                val |= d[pos + i] << (8 * i)
            pos += wb
            val &= 0xFFFFFFFF
            if val < code_lim:
                assert outp + count <= nval
                o[outp:outp + count] = lut[val] if lut is not None else val
            elif count:
                st |= PQE_RANGE
        outp += count
    if outp < nval:
        st |= PQE_CODES
    return st


def _fixed_read_span(s, nbytes, out_addr):
    """[lo, hi) of the addresses pq_copy_fixed_page loads to copy nbytes
    from address s: aligned u64 words merged by a shift, so it starts at s
    rounded down to 8 and may take in the word after the last one needed."""
    m = s & 7
    lo, hi = s, s + nbytes
    if out_addr & 7 == 0:
        nw = nbytes // 8
        if nw and m:
            lo, hi = s - m, max(hi, s - m + 8 * (nw + 1))
        return lo, hi
    for i in range(max(nbytes // 4 - 2, 0), nbytes // 4):
        bit = i * 32 + m * 8
        words = (bit >> 6) + (2 if bit & 63 > 32 else 1)
        lo, hi = s - m, max(hi, s - m + 8 * words)
    return lo, hi


def sim_values_multi(pages, amap: AddressMap, err: np.ndarray):
    """pages: ValPage entries; err: int32[1], ORed into.  A page that fails
    a check is left unwritten (a codes page: from the bad code on, as the
    kernel), and its PQE_* bits go into err."""
    for e in pages:
        kind, out_addr = int(e["kind"]), int(e["out"])
        dst_len, nv = int(e["dst_len"]), int(e["nv"])
        codes = kind == PQK_CODES
        bad, voff = 0, 0
        if dst_len < 0 or nv < 0:
            bad = PQE_ENTRY
        if not codes:
            if kind not in (4, 8) or out_addr & 3 or \
                    (kind == 8 and out_addr & 7):
                bad = PQE_ENTRY
        elif out_addr & 3:
            bad = PQE_ENTRY
        if not bad:
            base, arr = amap.find(int(e["page"]), dst_len)
            po = int(e["page"]) - base
            if int(e["flags"]) & PQF_HAS_DEF:
                bad, voff = _check_levels(Buf(arr, po, po + dst_len),
                                          dst_len, nv)
        if not bad and not codes:
            nbytes = nv * kind
            if voff + nbytes > dst_len:
                bad = PQE_PREFIX
            else:
                lo, hi = _fixed_read_span(int(e["page"]) + voff, nbytes,
                                          out_addr)
                assert amap.find(lo, hi - lo)[0] == base, \
                    "word loads leave the page's tensor"
                vals = sim_copy_fixed(
                    arr, [{"dst_off": po, "dst_len": dst_len, "nv": nv}],
                    [voff], [0], None, kind, nv)
                out, oo = amap.resolve(out_addr, nbytes)
                out[oo:oo + nbytes] = vals
        elif not bad:
            out, oo = amap.resolve(out_addr, nv * 4)
            code_lim = max(int(e["code_lim"]), 0)
            lut = None
            if int(e["lut"]):
                assert int(e["lut"]) % 4 == 0, "unaligned code table"
                la, lo = amap.resolve(int(e["lut"]), code_lim * 4)
                lut = la[lo:lo + code_lim * 4].view(np.int32)
            # a bit-packed value is read as a 4-byte word that may end up
            # to 3 bytes past the page: it must still be inside the tensor
            slack = min(3, len(arr) - (po + dst_len))
            st = _expand_codes_checked(
                Buf(arr, po + voff, po + dst_len, slack), dst_len - voff, nv,
                out[oo:oo + nv * 4].view(np.int32), lut, code_lim)
            bad |= st
        if bad:
            err[0] |= bad
