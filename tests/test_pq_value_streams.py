"""The parquet stages behind decompression on hand-built pages: definition
levels, dictionary codes, PLAIN fixed-width values, PLAIN byte arrays and
rle_expand with its host run parser (tests/parquet_streams.py builds the
pages; the expectation is what the builder was given).

The CPU part proves every stream valid with a decoder written from the
format description, and holds the simulators of tests/kernel_sim.py and
the host parser _parse_rle_runs to the builder's values.  The GPU part
feeds the same pages to the native entry points and compares exactly.
Malformed code streams go to pq_values_multi only, the one entry point
with an error contract, and only after the bounds-checked simulator has
accepted them."""

import functools
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

from bodo_amd.io import parquet_gpu as g
from tests import kernel_sim as ks
from tests import parquet_streams as S
from tests.parquet_streams import Packed, Rle

BITWIDTHS = list(range(0, 25))
RLE_EXPAND_WIDTHS = [1, 2, 7, 8, 9, 16, 17, 24]
COUNTS = (0, 1, 2, 3, 255, 256, 257, 513)  # words below, at, above 256


# ---------------------------------------------------------------------
# cases: lists of pages, built once
# ---------------------------------------------------------------------

def _bits(rng, n):
    """n random levels with both values present."""
    b = [int(v) for v in rng.integers(0, 2, n)]
    if n >= 2:
        b[0], b[-1] = 1, 0
    return b


@functools.lru_cache(maxsize=None)
def _code_pages(bw):
    """[(page, code_lim)] for bit width bw: every header size, run shape
    and tail the decoders distinguish.  code_lim is the smallest
    dictionary the page's codes fit."""
    rng = np.random.default_rng(100 + bw)
    top = (1 << bw) - 1

    def rnd(hi=top + 1):
        return int(rng.integers(0, hi))

    def packed(groups):  # the maximum code first and last
        v = [rnd() for _ in range(groups * 8)]
        v[0] = v[-1] = top
        return Packed(v)

    def fitting(n, pad, hi=top + 1):
        """Runs that hold exactly n codes below hi."""
        if n == 0:
            return []
        runs = [Rle(rnd(hi), n // 3)] if n >= 3 else []
        return runs + [Packed([rnd(hi) for _ in range(n - n // 3)], pad)]

    out = []

    def add(levels, runs, lim=top + 1):
        out.append((S.page(levels, S.codes_section(bw, runs)), lim))

    if bw == 0:
        add(None, [Rle(0, 37)])
        add(None, [Rle(0, 64), Packed([0] * 16), Rle(0, 8192)])
        add(None, [Packed([0] * 5)])
        out.append((S.page(None, S.raw_codes(b"\x00", [0] * 41)), 1))
    else:
        add(None, [Rle(rnd(), 1), packed(1), Rle(rnd(), 63), packed(8),
                   Rle(top, 64)])
        add(None, [Rle(rnd(), 8191), packed(9)])
        add(None, [packed(63), Rle(rnd(), 8192)])
        # a run of maximum codes: every neighbour's bits are ones
        add(None, [packed(64), Packed([top] * 16), Rle(top, 3), packed(1)])
        # 1..7 real values in the last group.  The codes stay below top
        # and the dictionary has top entries, so all-ones padding is
        # neither a valid code nor inside the dictionary
        lim = max(top, 1)
        for pad in (0, 1):
            for k in range(1, 8):
                add(None, [Rle(rnd(lim), 3),
                           Packed([rnd(lim) for _ in range(8 + k)], pad)],
                    lim)
            add(None, [Packed([rnd(lim) for _ in range(3)], pad, groups=3)],
                lim)
        # a last RLE run that announces more than the page holds
        add(None, [packed(1), Rle(rnd(), 10, declared=1000)])
        add(None, [Rle(rnd(), 70, declared=9000)])
    # no values: a bare bit-width byte, and nothing at all
    add(None, [])
    out.append((S.page(None, S.raw_codes(b"")), top + 1))
    # behind an all-valid level section: the bit-width byte on every
    # residue mod 8
    for resid in range(8):
        n = 20 + resid
        add(S.all_valid_levels(n, resid, resid & 1), fitting(n, resid & 1))
    # nulls
    lv = S.level_section([Rle(1, 5), Packed(_bits(rng, 16)), Rle(0, 7),
                          Packed(_bits(rng, 11), 1)])
    add(lv, fitting(sum(lv.values), 1))
    lv = S.level_section([Rle(0, 9)])
    add(lv, [])
    lv = S.level_section([Packed(_bits(rng, 64)), Rle(1, 3, declared=50)])
    add(lv, fitting(sum(lv.values), 0))
    assert len(out) >= 9
    return out


@functools.lru_cache(maxsize=None)
def _level_pages():
    """Pages for pq_def_levels; every body is PLAIN int32."""
    rng = np.random.default_rng(7)
    out = []

    def add(levels, n=None):
        n = sum(levels.values) if levels is not None else n
        body = S.plain_fixed(rng.integers(0, 1 << 32, n, dtype=np.uint32))
        out.append(S.page(levels, body))

    def lv(runs):
        add(S.level_section(runs))

    lv([Rle(1, 1), Packed(_bits(rng, 8)), Rle(0, 63), Packed(_bits(rng, 64)),
        Rle(1, 64), Packed(_bits(rng, 72))])
    lv([Rle(0, 8191), Packed(_bits(rng, 63 * 8))])
    lv([Packed(_bits(rng, 64 * 8)), Rle(1, 8192)])
    lv([Rle(1, 8191), Rle(0, 1)])
    add(None, 5)
    lv([Packed(_bits(rng, 8)), Rle(1, 9, declared=8192)])
    lv([Rle(0, 9, declared=100)])
    for k in range(1, 8):  # partial last group, padding all ones
        lv([Rle(1, 2), Packed(_bits(rng, 8 + k), 1)])
    add(None, 0)
    for k in (1, 4, 7):  # ... and zeros, as writers pad
        lv([Packed(_bits(rng, 16 + k), 0)])
    lv([Packed(_bits(rng, 3), 1, groups=4)])  # whole groups of padding
    add(None, 300)
    add(S.all_valid_levels(0, 0))
    for resid in range(8):
        add(S.all_valid_levels(10 + 3 * resid, resid, resid & 1))
    return out


def _pattern(rng, n, esize):
    if esize == 4:
        return rng.integers(0, 1 << 32, n, dtype=np.uint32)
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _fixed_pages(esize, with_levels):
    """PLAIN pages for pq_copy_fixed: every count at every source
    misalignment (from the length of the level section), and, as the odd
    counts shift dense_off, at both parities of the destination."""
    rng = np.random.default_rng(40 + esize)
    out = []
    for flip in (0, 1):
        if flip:  # one more value: every page of the second pass moves
            out.append(S.page(S.all_valid_levels(1, 0) if with_levels
                              else None,
                              S.plain_fixed(_pattern(rng, 1, esize))))
        for resid in range(8 if with_levels else 1):
            for n in COUNTS:
                lv = S.all_valid_levels(n, resid, (resid + n) & 1) \
                    if with_levels else None
                out.append(S.page(lv, S.plain_fixed(_pattern(rng, n, esize))))
    return out


@functools.lru_cache(maxsize=None)
def _string_pages():
    rng = np.random.default_rng(11)

    def rb(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    lens = [0, 1, 3, 4, 5, 255, 256, 65_541]
    out = [S.page(None, S.plain_byte_array([rb(n) for n in lens])),
           S.page(None, S.plain_byte_array([b"\x00", b"\x80\xff\x00", b""]
                                           + [rb(n) for n in lens[::-1]]))]
    lv = S.level_section([Rle(1, 3), Packed(_bits(rng, 16)), Rle(0, 4),
                          Packed(_bits(rng, 13), 1)])
    out.append(S.page(lv, S.plain_byte_array(
        [rb(int(rng.integers(0, 11))) for _ in range(sum(lv.values))])))
    out.append(S.page(None, S.plain_byte_array([])))
    lv = S.level_section([Rle(0, 6)])
    out.append(S.page(lv, S.plain_byte_array([])))
    for resid in range(8):
        n = 3 + resid
        out.append(S.page(S.all_valid_levels(n, resid, resid & 1),
                          S.plain_byte_array([rb(resid + i)
                                              for i in range(n)])))
    return out


# ---------------------------------------------------------------------
# pq_values_multi launches
# ---------------------------------------------------------------------

@dataclass
class Launch:
    pages: list
    kinds: list            # 0 = codes, 4 / 8 = PLAIN element size
    expected: list         # bytes per page; None: must stay unwritten
    err: int = 0
    luts: list = None      # per page: int32 array or None
    lims: list = None
    shifts: list = None    # page address mod 8
    align4: list = None    # destination 4- but not 8-byte aligned
    skip: tuple = ()       # pages whose own output range is not checked
    plan: S.OutPlan = field(init=False, default=None)

    def __post_init__(self):
        n = len(self.pages)
        self.luts = self.luts or [None] * n
        self.lims = self.lims or [0] * n
        self.plan = S.plan_outputs(
            [p.nv * (k or 4) for p, k in zip(self.pages, self.kinds)],
            self.align4)


def _lut(bw):
    """code -> value for a dictionary of 2^bw entries: a permutation plus
    an offset.  None above 16 bits: the codes are stored as they are."""
    if bw > 16:
        return None
    rng = np.random.default_rng(500 + bw)
    return (rng.permutation(1 << bw) + 1000).astype(np.int32)


def _coded(values, lut):
    v = np.array(values, dtype=np.int64)
    return (lut[v] if lut is not None else v).astype(np.int32).tobytes()


@functools.lru_cache(maxsize=None)
def _launch_codes(bw):
    """The null-free pages of _code_pages(bw), each with code_lim exactly
    its dictionary size."""
    lut = _lut(bw)
    pl = [(p, lim) for p, lim in _code_pages(bw) if p.n_valid == p.nv]
    assert len(pl) >= 9
    return Launch([p for p, _ in pl], [0] * len(pl),
                  [_coded(p.values, lut) for p, _ in pl],
                  luts=[lut] * len(pl), lims=[lim for _, lim in pl])


@functools.lru_cache(maxsize=None)
def _launch_plain():
    """PLAIN pages at any byte address: page address mod 8 and level
    section length together give every source misalignment, with the
    destination 8-aligned or, for 4-byte elements, only 4-aligned."""
    rng = np.random.default_rng(21)
    pages, kinds, shifts, align4 = [], [], [], []
    for a in range(8):
        for with_levels in (False, True):
            for n in COUNTS:
                for esize, a4 in ((8, False), (4, False), (4, True)):
                    lv = S.all_valid_levels(n, (3 * a + 1) % 8, n & 1) \
                        if with_levels else None
                    pages.append(S.page(
                        lv, S.plain_fixed(_pattern(rng, n, esize))))
                    kinds.append(esize)
                    shifts.append(a)
                    align4.append(a4)
    return Launch(pages, kinds, [p.body.data for p in pages], shifts=shifts,
                  align4=align4)


def _good_level_sections():
    secs = [S.level_section([Rle(1, n)]) for n in (1, 63, 64, 8191, 8192)]
    secs += [S.level_section([Packed([1] * 8 * gr)])
             for gr in (1, 8, 9, 63, 64, 300)]
    for pad in (0, 1):
        secs += [S.level_section([Packed([1] * (8 + k), pad)])
                 for k in range(1, 8)]
        secs.append(S.level_section([Packed([1] * 8 * 257 + [1] * 3, pad)]))
        secs.append(S.level_section([Packed([1] * 5, pad, groups=3)]))
        secs += [S.all_valid_levels(n, n % 8, pad) for n in (0, 1, 2, 9, 300)]
    secs.append(S.level_section([Rle(1, 7, declared=8192)]))
    secs.append(S.level_section([Packed([1] * 16), Rle(1, 2), Rle(1, 64),
                                 Packed([1] * 72), Rle(1, 1, declared=3)]))
    return secs


CHECK_BW = 3  # codes pages of the level checks


def _check_page(rng, levels, kind, nv):
    """A page of nv values behind levels, PLAIN or codes (64 threads)."""
    if kind:
        return S.page(levels, S.plain_fixed(_pattern(rng, nv, kind)), nv=nv)
    runs = [Packed([int(v) for v in rng.integers(0, 8, nv)], 1)] if nv else []
    return S.page(levels, S.codes_section(CHECK_BW, runs), nv=nv)


def _expected(p, kind, lut):
    return p.body.data if kind else _coded(p.values, lut)


@functools.lru_cache(maxsize=None)
def _launch_good_levels():
    """All-ones levels in every representation in front of a PLAIN page
    (256 threads check them) and of a codes page (64 threads)."""
    rng = np.random.default_rng(31)
    lut = _lut(CHECK_BW)
    pages, kinds = [], []
    for i, sec in enumerate(_good_level_sections()):
        for kind in ((8, 0) if i & 1 else (4, 0)):
            pages.append(_check_page(rng, sec, kind, len(sec.values)))
            kinds.append(kind)
    return Launch(pages, kinds,
                  [_expected(p, k, lut) for p, k in zip(pages, kinds)],
                  luts=[lut] * len(pages), lims=[8] * len(pages))


def _one_zero(n, at):
    b = [1] * n
    b[at] = 0
    return b


BAD_LEVELS = {
    # a single 0 among the levels of a page that must hold none
    "full_first": [Packed(_one_zero(32, 0))],
    "full_middle": [Packed(_one_zero(32, 13))],
    "full_last": [Packed(_one_zero(32, 31))],
    "tail_first": [Packed(_one_zero(29, 24), 0)],
    "tail_middle": [Packed(_one_zero(29, 26), 0)],
    "tail_last": [Packed(_one_zero(29, 28), 0)],
    "tail_last_ones_padding": [Packed(_one_zero(29, 28), 1)],
    "byte_280": [Packed(_one_zero(2400, 8 * 280 + 3))],
    "byte_299_last": [Packed(_one_zero(2400, 2399))],
    "rle_first": [Rle(0, 1), Rle(1, 20)],
    "rle_middle": [Rle(1, 10), Rle(0, 1), Rle(1, 10)],
    "rle_last": [Rle(1, 20), Rle(0, 1)],
    "rle_last_clipped": [Rle(1, 20), Rle(0, 1, declared=9)],
}


@functools.lru_cache(maxsize=None)
def _launch_bad_levels(name, kind):
    """One page with a 0 level and one good page of the other kind."""
    rng = np.random.default_rng(33)
    lut = _lut(CHECK_BW)
    sec = S.level_section(BAD_LEVELS[name])
    bad = _check_page(rng, sec, kind, len(sec.values))
    good_kind = 0 if kind else 8
    good = _check_page(rng, S.all_valid_levels(21, 5), good_kind, 21)
    return Launch([bad, good], [kind, good_kind],
                  [None, _expected(good, good_kind, lut)],
                  err=ks.PQE_LEVELS, luts=[lut, lut], lims=[8, 8])


MAL_BW = 5
MAL_LIM = 20  # dictionary entries of the malformed pages

MALFORMED = {
    # name: (codes section bytes, nv, PQE_* word, levels in front)
    "header_varint_cut": (
        bytes([MAL_BW]) + S.rle_run(3, 5, MAL_BW) + b"\xc8", 10,
        ks.PQE_CODES, False),
    "packed_run_past_end": (
        bytes([MAL_BW]) + S.varint((4 << 1) | 1) + bytes([0x21] * 10), 32,
        ks.PQE_CODES, False),
    "rle_value_cut": (
        bytes([16]) + S.varint(10 << 1) + b"\x07", 10, ks.PQE_CODES, True),
    "stream_short_of_nv": (
        bytes([MAL_BW]) + S.rle_run(3, 10, MAL_BW), 20, ks.PQE_CODES, False),
    "stream_short_behind_levels": (
        bytes([MAL_BW]) + S.bitpacked_run([1, 2, 3, 4, 5, 6, 7, 8], MAL_BW),
        9, ks.PQE_CODES, True),
    "bitwidth_25": (
        bytes([25]) + S.rle_run(3, 4, 25), 4, ks.PQE_CODES, False),
    "empty_section": (b"", 3, ks.PQE_CODES, False),
    "empty_section_behind_levels": (b"", 3, ks.PQE_CODES, True),
    "code_at_lim_packed": (
        bytes([MAL_BW]) + S.rle_run(19, 4, MAL_BW)
        + S.bitpacked_run([0, 19, 5, MAL_LIM, 7, 1, 2, 3], MAL_BW), 12,
        ks.PQE_RANGE, False),
    "code_at_lim_rle": (
        bytes([MAL_BW]) + S.bitpacked_run([0, 19, 5, 4, 7, 1, 2, 3], MAL_BW)
        + S.rle_run(MAL_LIM, 4, MAL_BW), 12, ks.PQE_RANGE, True),
}


@functools.lru_cache(maxsize=None)
def _launch_malformed(name):
    """The bad page, then a good one whose bytes follow it in scratch."""
    data, nv, err, with_levels = MALFORMED[name]
    rng = np.random.default_rng(35)
    lut = (rng.permutation(MAL_LIM) + 1000).astype(np.int32)
    lv = S.all_valid_levels(nv, 3, 1) if with_levels else None
    bad = S.page(lv, S.raw_codes(data), nv=nv)
    vals = [int(v) for v in rng.integers(0, MAL_LIM, 40)]
    vals[0] = vals[-1] = MAL_LIM - 1
    good = S.page(None, S.codes_section(
        MAL_BW, [Rle(MAL_LIM - 1, 9), Packed(vals)]))
    return Launch([bad, good], [0, 0], [None, _coded(good.values, lut)],
                  err=err, luts=[lut, lut], lims=[MAL_LIM, MAL_LIM],
                  skip=(0,))


def _run_launch(launch: Launch, device):
    """The launch on the simulator (device "cpu") or on the GPU: (err
    word, bytes of the canary buffer afterwards)."""
    lay = S.place(launch.pages, g._PAGEMETA_DT, launch.shifts)
    scratch = torch.from_numpy(lay.scratch).to(device)
    out = torch.full((launch.plan.size,), S.CANARY, dtype=torch.uint8,
                     device=device)
    lut_t = {}
    for lut in launch.luts:
        if lut is not None and id(lut) not in lut_t:
            lut_t[id(lut)] = torch.from_numpy(lut).to(device)
    n = len(launch.pages)
    tbl = np.zeros(n, dtype=g._VALPAGE_DT)
    tbl["page"] = [scratch.data_ptr() + o for o in lay.offs]
    tbl["out"] = [out.data_ptr() + o for o in launch.plan.offs]
    tbl["lut"] = [0 if lut is None else lut_t[id(lut)].data_ptr()
                  for lut in launch.luts]
    tbl["dst_len"] = [len(p.data) for p in launch.pages]
    tbl["nv"] = [p.nv for p in launch.pages]
    tbl["kind"] = launch.kinds
    tbl["flags"] = [g._PQF_HAS_DEF if p.has_def else 0 for p in launch.pages]
    tbl["code_lim"] = launch.lims
    assert out.data_ptr() % 8 == 0 and scratch.data_ptr() % 8 == 0
    if torch.device(device).type == "cpu":
        amap = ks.AddressMap()
        for t in [scratch, out] + list(lut_t.values()):
            amap.add(t)
        err = np.zeros(1, dtype=np.int32)
        ks.sim_values_multi(tbl, amap, err)
        return int(err[0]), out.numpy()
    import bodo_amd_kernels as K

    err = torch.zeros(1, dtype=torch.int32, device=device)
    K.pq_values_multi(torch.from_numpy(tbl.view(np.uint8)).to(device), n, err)
    torch.cuda.synchronize()
    return int(err.item()), out.cpu().numpy()


def _check_launch(launch: Launch, device):
    err, out = _run_launch(launch, device)
    assert err == launch.err, f"err word {err}, expected {launch.err}"
    S.check_outputs(out, launch.plan, launch.expected, launch.skip)


# ---------------------------------------------------------------------
# per-chunk entry points: expectations
# ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _chunk(kind, arg=None, arg2=None):
    """(pages, layout) of a per-chunk case."""
    if kind == "codes":
        pages = [p for p, _ in _code_pages(arg)]
    elif kind == "levels":
        pages = _level_pages()
    elif kind == "fixed":
        pages = _fixed_pages(arg, arg2)
    else:
        pages = _string_pages()
    assert len(pages) >= 9  # more than one block of four waves
    return pages, S.place(pages, g._PAGEMETA_DT)


def _expected_codes(pages):
    return np.array([v for p in pages for v in p.values], dtype=np.int32)


def _check_levels_out(lay, mask, n_valid, vdo):
    assert np.array_equal(np.asarray(n_valid), lay.n_valid)
    assert np.array_equal(np.asarray(vdo), lay.vdo)  # 4 + lvl_len, or 0
    assert np.array_equal(np.asarray(mask), lay.mask)


def _check_strings(pages, lay, lengths, src_abs):
    exp_len = np.array([len(s) for p in pages for s in p.values],
                       dtype=np.int32)
    exp_src = np.array([o + p.val_data_off + so for p, o in
                        zip(pages, lay.offs) for so in p.body.str_off],
                       dtype=np.int64)
    assert np.array_equal(np.asarray(lengths), exp_len)
    assert np.array_equal(np.asarray(src_abs), exp_src)
    return exp_len, b"".join(s for p in pages for s in p.values)


# ---------------------------------------------------------------------
# CPU part
# ---------------------------------------------------------------------

def _assert_streams_valid(pages):
    for i, p in enumerate(pages):
        if p.levels is not None:
            got = S.spec_decode_hybrid(p.levels.data[4:], 1, p.nv)
            assert got == p.levels.values == list(p.mask), i
            assert int.from_bytes(p.data[:4], "little") + 4 == p.val_data_off
        if p.body.kind == "codes" and len(p.body.data) > 1:
            sec = p.body
            assert sec.data[0] == sec.bitwidth
            got = S.spec_decode_hybrid(sec.data[1:], sec.bitwidth, p.n_valid)
            assert got == sec.values, i


@pytest.mark.parametrize("bw", BITWIDTHS)
def test_code_streams_are_valid(bw):
    pages = [p for p, _ in _code_pages(bw)]
    _assert_streams_valid(pages)
    for p, lim in _code_pages(bw):
        assert all(v < lim for v in p.values)
    residues = {p.val_data_off % 8 for p in pages if p.has_def}
    assert residues == set(range(8))


def test_other_streams_are_valid():
    _assert_streams_valid(_level_pages())
    _assert_streams_valid(_string_pages())
    _assert_streams_valid(_launch_good_levels().pages)
    _assert_streams_valid(_launch_plain().pages)
    for sec in _good_level_sections():
        assert all(sec.values)


def test_builder_rejects_short_run_mid_stream():
    with pytest.raises(ValueError):
        S.codes_section(3, [Packed([1, 2, 3]), Rle(1, 4)])
    with pytest.raises(ValueError):
        S.codes_section(3, [Rle(1, 4, declared=9), Rle(1, 4)])


@pytest.mark.parametrize("bw", BITWIDTHS)
def test_sim_codes_per_chunk(bw):
    pages, lay = _chunk("codes", bw)
    _check_levels_out(lay, *ks.sim_def_levels(lay.scratch, lay.metas, 1, 1,
                                              len(lay.mask)))
    got = ks.sim_expand_codes(lay.scratch, lay.metas, lay.vdo, lay.dense_off,
                              lay.n_valid, int(lay.n_valid.sum()))
    assert np.array_equal(got, _expected_codes(pages))


@pytest.mark.parametrize("bw", BITWIDTHS)
def test_sim_codes_values_multi(bw):
    _check_launch(_launch_codes(bw), "cpu")


def test_sim_def_levels():
    pages, lay = _chunk("levels")
    _check_levels_out(lay, *ks.sim_def_levels(lay.scratch, lay.metas, 1, 1,
                                              len(lay.mask)))
    assert any(p.n_valid < p.nv for p in pages)
    got = ks.sim_copy_fixed(lay.scratch, lay.metas, lay.vdo, lay.dense_off,
                            lay.n_valid, 4, int(lay.n_valid.sum()))
    assert got.tobytes() == b"".join(p.body.data for p in pages)


def test_sim_check_levels_accepts_all_ones():
    _check_launch(_launch_good_levels(), "cpu")


@pytest.mark.parametrize("kind", [8, 0], ids=["plain", "codes"])
@pytest.mark.parametrize("name", sorted(BAD_LEVELS))
def test_sim_check_levels_reports_a_zero(name, kind):
    _check_launch(_launch_bad_levels(name, kind), "cpu")


@pytest.mark.parametrize("with_levels", [True, False],
                         ids=["levels", "nolevels"])
@pytest.mark.parametrize("esize", [4, 8])
def test_sim_copy_fixed(esize, with_levels):
    pages, lay = _chunk("fixed", esize, with_levels)
    if esize == 4:  # destinations at both parities
        assert {int(d) & 1 for d, p in zip(lay.dense_off, pages)
                if p.nv >= 255} == {0, 1}
    if with_levels:
        assert {(o + v) % 8 for o, v in zip(lay.offs, lay.vdo)} == \
            set(range(8))
    got = ks.sim_copy_fixed(lay.scratch, lay.metas,
                            lay.vdo if with_levels else None, lay.dense_off,
                            lay.n_valid if with_levels else None, esize,
                            int(lay.n_valid.sum()))
    assert got.tobytes() == b"".join(p.body.data for p in pages)


def test_sim_values_multi_plain():
    _check_launch(_launch_plain(), "cpu")


def test_sim_byte_array():
    pages, lay = _chunk("strings")
    _check_levels_out(lay, *ks.sim_def_levels(lay.scratch, lay.metas, 1, 1,
                                              len(lay.mask)))
    lengths, src_abs = ks.sim_byte_array(
        lay.scratch, lay.metas, lay.vdo, lay.dense_off, lay.n_valid,
        int(lay.n_valid.sum()))
    exp_len, exp_bytes = _check_strings(pages, lay, lengths, src_abs)
    got = b"".join(lay.scratch[a:a + n].tobytes()
                   for a, n in zip(src_abs, exp_len))
    assert got == exp_bytes


def _rle_pages(bw):
    """(page bytes, offset of the stream, its end, values, run table)."""
    out = []
    for p, _ in _code_pages(bw):
        if len(p.body.data) > 1:
            v = p.val_data_off
            out.append((p.data, v + 1, len(p.data), bw, p.values,
                        S.expected_runs(p.body, p.n_valid, v)))
    if bw == 1:  # and the level streams
        for p in _level_pages() + [q for q, _ in _code_pages(1)]:
            if p.levels is not None:
                out.append((p.data, 4, p.val_data_off, 1, p.levels.values,
                            S.expected_runs(p.levels, p.nv, 0)))
    return out


@pytest.mark.parametrize("bw", RLE_EXPAND_WIDTHS)
def test_parse_rle_runs_matches_builder(bw):
    cases = _rle_pages(bw)
    assert cases
    for i, (pb, pos, end, w, values, runs) in enumerate(cases):
        got, n = g._parse_rle_runs(pb, pos, end, w, len(values))
        assert n == len(values), i
        assert got == runs, i
        blob = g._runs_blob(got)
        assert blob.dtype.itemsize == 24  # struct RleRun
        assert [tuple(int(x) for x in r) for r in blob] == runs, i


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_sim_malformed_codes(name):
    _check_launch(_launch_malformed(name), "cpu")


def test_sim_per_chunk_route_rejects_short_stream():
    """The per-chunk kernel drops the status of a stream that stops short
    of nv and leaves the rest of its output unwritten; its simulator
    raises instead.  Recorded here, never sent to a GPU."""
    data, nv, _, _ = MALFORMED["stream_short_of_nv"]
    lay = S.place([S.page(None, S.raw_codes(data), nv=nv)], g._PAGEMETA_DT)
    with pytest.raises(AssertionError, match="codes short"):
        ks.sim_expand_codes(lay.scratch, lay.metas, None, lay.dense_off,
                            None, nv)


# ---------------------------------------------------------------------
# GPU part
# ---------------------------------------------------------------------

def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _gpu_levels(pages, lay):
    import bodo_amd_kernels as K

    scratch = _dev(lay.scratch)
    metas = _dev(lay.metas.view(np.uint8))
    mask, n_valid, vdo = K.pq_def_levels(scratch, metas, len(pages), 1, 1,
                                         len(lay.mask))
    torch.cuda.synchronize()
    _check_levels_out(lay, mask.cpu().numpy(), n_valid.cpu().numpy(),
                      vdo.cpu().numpy())
    return K, scratch, metas


@pytest.mark.gpu
@pytest.mark.parametrize("bw", BITWIDTHS)
def test_gpu_codes_per_chunk(bw):
    pages, lay = _chunk("codes", bw)
    K, scratch, metas = _gpu_levels(pages, lay)
    got = K.pq_expand_codes(scratch, metas, len(pages), _dev(lay.vdo),
                            _dev(lay.dense_off), _dev(lay.n_valid),
                            int(lay.n_valid.sum()))
    assert np.array_equal(got.cpu().numpy(), _expected_codes(pages))


@pytest.mark.gpu
@pytest.mark.parametrize("bw", BITWIDTHS)
def test_gpu_codes_values_multi(bw):
    _check_launch(_launch_codes(bw), "cuda")


@pytest.mark.gpu
def test_gpu_def_levels():
    pages, lay = _chunk("levels")
    K, scratch, metas = _gpu_levels(pages, lay)
    got = K.pq_copy_fixed(scratch, metas, len(pages), _dev(lay.vdo),
                          _dev(lay.dense_off), _dev(lay.n_valid), 4,
                          int(lay.n_valid.sum()))
    assert got.cpu().numpy().tobytes() == b"".join(p.body.data for p in pages)


@pytest.mark.gpu
def test_gpu_check_levels_accepts_all_ones():
    _check_launch(_launch_good_levels(), "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [8, 0], ids=["plain", "codes"])
@pytest.mark.parametrize("name", sorted(BAD_LEVELS))
def test_gpu_check_levels_reports_a_zero(name, kind):
    _check_launch(_launch_bad_levels(name, kind), "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("with_levels", [True, False],
                         ids=["levels", "nolevels"])
@pytest.mark.parametrize("esize", [4, 8])
def test_gpu_copy_fixed(esize, with_levels):
    import bodo_amd_kernels as K

    pages, lay = _chunk("fixed", esize, with_levels)
    got = K.pq_copy_fixed(
        _dev(lay.scratch), _dev(lay.metas.view(np.uint8)), len(pages),
        _dev(lay.vdo) if with_levels else None, _dev(lay.dense_off),
        _dev(lay.n_valid) if with_levels else None, esize,
        int(lay.n_valid.sum()))
    assert got.cpu().numpy().tobytes() == b"".join(p.body.data for p in pages)


@pytest.mark.gpu
def test_gpu_values_multi_plain():
    _check_launch(_launch_plain(), "cuda")


@pytest.mark.gpu
def test_gpu_byte_array():
    pages, lay = _chunk("strings")
    K, scratch, metas = _gpu_levels(pages, lay)
    total = int(lay.n_valid.sum())
    lengths, src_abs = K.pq_byte_array_lengths(
        scratch, metas, len(pages), _dev(lay.vdo), _dev(lay.dense_off),
        _dev(lay.n_valid), total)
    exp_len, exp_bytes = _check_strings(pages, lay, lengths.cpu().numpy(),
                                        src_abs.cpu().numpy())
    dst_off = np.cumsum(exp_len, dtype=np.int64) - exp_len
    got = K.pq_copy_strings(scratch, src_abs, _dev(dst_off), lengths, total,
                            len(exp_bytes))
    assert got.cpu().numpy()[:len(exp_bytes)].tobytes() == exp_bytes


@pytest.mark.gpu
@pytest.mark.parametrize("bw", RLE_EXPAND_WIDTHS)
def test_gpu_rle_expand(bw):
    import bodo_amd_kernels as K

    for i, (pb, pos, end, w, values, _) in enumerate(_rle_pages(bw)):
        runs, n = g._parse_rle_runs(pb, pos, end, w, len(values))
        assert n == len(values), i
        blob = _dev(g._runs_blob(runs).view(np.uint8))
        got = K.rle_expand(blob, len(runs), g._dev_bytes(pb, "cuda"), w, n)
        assert got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(),
                              np.array(values, dtype=np.int32)), i


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_gpu_malformed_codes(name):
    launch = _launch_malformed(name)
    # the simulator asserts on every out-of-bounds access: it goes first
    _check_launch(launch, "cpu")
    _check_launch(launch, "cuda")
