// Transforms of plain (offsets + bytes) string columns for gfx950: len,
// strip / lstrip / rstrip, slice(start, stop), lower / upper and concat.
//
// The geometry is strmatch.hip's: 256-thread blocks, a tile is 256
// consecutive rows, tiles grid-strided over at most max_blocks blocks, int64
// offsets throughout.  A tile's bytes are contiguous in the column; when they
// fit the stage they are copied HBM -> LDS with 16-byte loads from the
// address rounded down to 16 (vectors not wholly inside the buffer are loaded
// byte by byte), otherwise the tile takes a wave-per-row path over global
// memory.  The staging lines are strmatch.hip's, repeated here so that file
// stays as it is.
//
// Every offset read from a column is clamped to its tile's byte range, which
// is clamped to the buffer, by the same two functions in every kernel, so
// the lengths one kernel measures are the lengths the next one copies and
// nothing outside a buffer is read or written whatever the offsets say.
//
//  * string_measure_kernel: one row -> its output byte length and, but for
//    len, the position of its first output byte in the source (the end is
//    that plus the length, so it is not stored).  Thread t scans row t of the
//    staged tile; past the stage a wave takes a row 64 bytes a step with a
//    ballot of lead / non-blank bytes.  A trim that stops at a byte >= 0x80
//    raises the fallback flag (it may be Unicode white space; the kernel does
//    not decode it).  Lengths land in out_offsets[1:], which the host turns
//    into offsets with one in-place cumsum.
//  * string_concat_measure_kernel: the same for a[i] ++ b[i], from the
//    offsets alone.
//  * string_build_kernel: output row i is a part of source A followed by a
//    part of source B (B is the empty literal for the one-source ops; either
//    side of a concat may be a literal of at most 256 bytes, which travels in
//    the kernel arguments).  A tile's output bytes are contiguous.  The block
//    stages both source tiles, the tile's 257 output offsets and the rows'
//    begins and lengths, then writes the output as 16-byte vectors aligned in
//    HBM, thread t taking vectors t, t + 256, ...: a binary search in the LDS
//    offsets finds the row of the vector's first byte, the 16 bytes are
//    gathered from the stage across row boundaries, and one vector store
//    leaves (byte stores at the two ragged edges of the tile's range).  A
//    tile past the stage is copied row by row, one wave per row, global to
//    global.
//  * string_case_kernel: a flat pass over the whole byte buffer, 16-byte
//    loads, a branch-free SWAR ASCII map, 16-byte stores; the offsets are
//    reused by the caller.  Any byte >= 0x80 raises the flag, a plain store
//    of 1.
//
// Stage: SX_STAGE = 32 KiB shared by the two sources of a build (a tile is
// staged when its A bytes plus its B bytes fit), which with the literal, the
// alignment slack and 5 KiB of row tables is 38.4 KiB of LDS a block: four
// blocks a CU of gfx950's 160 KiB, and under the 64 KiB a static allocation
// may take.  Two stages of 32 KiB would have left two blocks and needed a
// dynamic allocation.

#include <torch/extension.h>
#include <ATen/ATen.h>

#include <algorithm>
#include <cstring>

#include "common.h"
#include "hip_host.h"

#define SX_THREADS 256
#define SX_WAVES (SX_THREADS / WAVE)
#define SX_TILE SX_THREADS
#define SX_STAGE 32768
#define SX_MAX_LIT 256
// per source a misaligned head of up to 15 bytes and a tail rounded up to 16
#define SX_LIT_POS (SX_STAGE + 64)
#define SX_STAGE_ALLOC (SX_LIT_POS + SX_MAX_LIT)
#define SX_MAX_BLOCKS 2048

enum SxOp : int { SX_LEN = 0, SX_STRIP = 1, SX_LSTRIP = 2, SX_RSTRIP = 3,
                  SX_SLICE = 4 };

// ------------------------------------------------------------ shared parts

DEV_INLINE int64_t clamp64(int64_t x, int64_t lo, int64_t hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}

// byte range of rows [r0, r0 + rows), inside the buffer
DEV_INLINE void tile_range(const int64_t* offsets, int64_t nbytes, int64_t r0,
                           int rows, int64_t& b0, int64_t& b1) {
  b0 = clamp64(offsets[r0], 0, nbytes);
  b1 = clamp64(offsets[r0 + rows], b0, nbytes);
}

// byte range of row r, inside its tile's range
DEV_INLINE void row_range(const int64_t* offsets, int64_t r, int64_t b0,
                          int64_t b1, int64_t& s, int64_t& e) {
  s = clamp64(offsets[r], b0, b1);
  e = clamp64(offsets[r + 1], s, b1);
}

// Copies buf[b0, b0 + tile_bytes) to the 16-byte aligned LDS `dst`; byte b0
// lands at dst[lead], lead < 16 returned.  The block calls it together.
DEV_INLINE int stage_tile(uint8_t* dst, const uint8_t* buf, int64_t nbytes,
                          int64_t b0, int tile_bytes, int t) {
  const uintptr_t buf_lo = (uintptr_t)buf;
  const uintptr_t buf_hi = buf_lo + (uint64_t)nbytes;
  const uintptr_t src0 = (buf_lo + (uint64_t)b0) & ~(uintptr_t)15;
  const int lead = (int)(buf_lo + (uint64_t)b0 - src0);
  const int nvec = tile_bytes ? (lead + tile_bytes + 15) >> 4 : 0;
  for (int v = t; v < nvec; v += SX_THREADS) {
    const uintptr_t src = src0 + (uintptr_t)v * 16;
    uint4 q;
    if (src >= buf_lo && src + 16 <= buf_hi) {
      q = *(const uint4*)src;
    } else {
      uint8_t* qb = (uint8_t*)&q;
      for (int k = 0; k < 16; ++k)
        qb[k] = (src + k >= buf_lo && src + k < buf_hi)
                    ? *(const uint8_t*)(src + k) : (uint8_t)0;
    }
    ((uint4*)dst)[v] = q;
  }
  return lead;
}

// the white space str.strip() and arrow trim among the bytes below 0x80
DEV_INLINE bool is_blank(uint8_t b) {
  return (unsigned)(b - 9) <= 4u || (unsigned)(b - 28) <= 4u;
}

DEV_INLINE bool is_lead(uint8_t b) { return (b & 0xC0) != 0x80; }

// ----------------------------------------------------------- measure, LDS

// code points in stage[s, e): the bytes that are no continuation byte
DEV_INLINE int lds_count(const uint8_t* stage, int s, int e) {
  const uint32_t* words = (const uint32_t*)stage;
  int cnt = 0;
  for (int p = s; p < e;) {
    const uint32_t x = words[p >> 2];
    const uint32_t lead = ~((x >> 7) & ~(x >> 6)) & 0x01010101u;
    const int nxt = (p | 3) + 1;
    uint32_t m = 0xFFFFFFFFu << ((p & 3) * 8);
    if (nxt > e) m &= 0xFFFFFFFFu >> ((nxt - e) * 8);
    cnt += __popc(lead & m);
    p = nxt;
  }
  return cnt;
}

// Python's s[start:stop] over stage[s, e) -> byte range [pa, pb)
DEV_INLINE void lds_slice(const uint8_t* stage, int s, int e, int64_t start,
                          int64_t stop, bool has_stop, int& pa, int& pb) {
  int64_t a = start, b = has_stop ? stop : INT64_MAX;
  if (start < 0 || (has_stop && stop < 0)) {
    const int64_t L = lds_count(stage, s, e);
    if (start < 0) a = L + start < 0 ? 0 : L + start;
    if (has_stop && stop < 0) b = L + stop < 0 ? 0 : L + stop;
  }
  pa = pb = e;
  if (a >= b) return;
  int64_t cp = 0;
  int p = s;
  if (a == 0) {
    pa = s;
  } else {
    for (; p < e; ++p)
      if (is_lead(stage[p])) {
        if (cp == a) { pa = p; break; }
        ++cp;
      }
  }
  if (pa == e || b == INT64_MAX) return;
  // cp lead bytes lie before p; the one of index b ends the slice
  for (; p < e; ++p)
    if (is_lead(stage[p])) {
      if (cp == b) { pb = p; break; }
      ++cp;
    }
}

// --------------------------------------------------- measure, wave per row

DEV_INLINE int64_t wave_count(const uint8_t* bytes, int64_t s, int64_t e,
                              int lane) {
  int64_t cnt = 0;
  for (int64_t base = s; base < e; base += WAVE) {
    const int64_t p = base + lane;
    const bool lead = p < e && is_lead(bytes[p]);
    cnt += __popcll(__ballot(lead));
  }
  return cnt;
}

// position of the lead byte of index k (from 0) in bytes[s, e), or e
DEV_INLINE int64_t wave_nth_lead(const uint8_t* bytes, int64_t s, int64_t e,
                                 int64_t k, int lane) {
  int64_t cum = 0;
  for (int64_t base = s; base < e; base += WAVE) {
    const int64_t p = base + lane;
    const bool lead = p < e && is_lead(bytes[p]);
    const uint64_t b = __ballot(lead);
    const int c = __popcll(b);
    if (cum + c > k) {
      const int want = (int)(k - cum);
      const bool me =
          lead && __popcll(b & ((1ull << lane) - 1ull)) == want;
      const uint64_t mb = __ballot(me);
      return base + (__ffsll((unsigned long long)mb) - 1);
    }
    cum += c;
  }
  return e;
}

struct SxMeasureArgs {
  const uint8_t* bytes;
  const int64_t* offsets;
  const uint8_t* mask;
  int64_t* out_len;  // n entries
  int64_t* zero;     // set to 0 (the first output offset), or nullptr
  int64_t* begin;    // n entries, or nullptr for len
  int64_t* flag;
  int64_t n;
  int64_t nbytes;
  int64_t start;
  int64_t stop;
  int32_t has_stop;
  int32_t op;
};

__global__ void __launch_bounds__(SX_THREADS)
string_measure_kernel(const SxMeasureArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[SX_STAGE + 32];
  __shared__ int32_t s_off[SX_TILE + 1];

  const int t = threadIdx.x;
  const int lane = t & (WAVE - 1);
  const int wave = t / WAVE;
  const int op = a.op;
  const bool has_stop = a.has_stop != 0;
  const int64_t tiles = (a.n + SX_TILE - 1) / SX_TILE;
  if (blockIdx.x == 0 && t == 0 && a.zero != nullptr) *a.zero = 0;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * SX_TILE;
    const int rows = (int)(a.n - r0 < SX_TILE ? a.n - r0 : SX_TILE);
    int64_t b0, b1;
    tile_range(a.offsets, a.nbytes, r0, rows, b0, b1);
    __syncthreads();  // previous tile's scans done

    if (b1 - b0 <= SX_STAGE) {
      const int lead =
          stage_tile(s_stage, a.bytes, a.nbytes, b0, (int)(b1 - b0), t);
      for (int i = t; i <= rows; i += SX_THREADS)
        s_off[i] = (int)(clamp64(a.offsets[r0 + i], b0, b1) - b0) + lead;
      __syncthreads();
      if (t < rows) {
        const int64_t r = r0 + t;
        const bool valid = a.mask == nullptr || a.mask[r] != 0;
        const int s = s_off[t];
        const int e = s_off[t + 1] < s ? s : s_off[t + 1];
        int ps = s, pe = valid ? e : s;
        bool high = false;
        if (!valid) {
        } else if (op == SX_LEN) {
          pe = s + lds_count(s_stage, s, e);
        } else if (op == SX_SLICE) {
          lds_slice(s_stage, s, e, a.start, a.stop, has_stop, ps, pe);
        } else {
          if (op != SX_RSTRIP) {
            while (ps < pe && is_blank(s_stage[ps])) ++ps;
            high |= ps < pe && s_stage[ps] >= 0x80;
          }
          if (op != SX_LSTRIP) {
            while (pe > ps && is_blank(s_stage[pe - 1])) --pe;
            high |= pe > ps && s_stage[pe - 1] >= 0x80;
          }
        }
        a.out_len[r] = pe - ps;
        if (a.begin != nullptr) a.begin[r] = b0 + (ps - lead);
        if (high) *a.flag = 1;
      }
    } else {
      for (int i = wave; i < rows; i += SX_WAVES) {
        const int64_t r = r0 + i;
        const bool valid = a.mask == nullptr || a.mask[r] != 0;
        int64_t s, e;
        row_range(a.offsets, r, b0, b1, s, e);
        int64_t ps = s, pe = valid ? e : s;
        bool high = false;
        if (!valid) {
        } else if (op == SX_LEN) {
          pe = s + wave_count(a.bytes, s, e, lane);
        } else if (op == SX_SLICE) {
          int64_t x = a.start, y = has_stop ? a.stop : INT64_MAX;
          if (x < 0 || (has_stop && y < 0)) {
            const int64_t L = wave_count(a.bytes, s, e, lane);
            if (x < 0) x = L + x < 0 ? 0 : L + x;
            if (has_stop && y < 0) y = L + y < 0 ? 0 : L + y;
          }
          if (x >= y) {
            ps = pe = e;
          } else {
            ps = x == 0 ? s : wave_nth_lead(a.bytes, s, e, x, lane);
            pe = (ps == e || y == INT64_MAX)
                     ? e : wave_nth_lead(a.bytes, ps, e, y - x, lane);
          }
        } else {
          if (op != SX_RSTRIP) {
            ps = e;
            for (int64_t base = s; base < e; base += WAVE) {
              const int64_t p = base + lane;
              const uint64_t b = __ballot(p < e && !is_blank(a.bytes[p]));
              if (b) {
                ps = base + (__ffsll((unsigned long long)b) - 1);
                break;
              }
            }
            high |= ps < e && a.bytes[ps] >= 0x80;
          }
          if (op != SX_LSTRIP) {
            pe = ps;
            for (int64_t hi = e; hi > ps; hi -= WAVE) {
              const int64_t p = hi - WAVE + lane;
              const uint64_t b = __ballot(p >= ps && !is_blank(a.bytes[p]));
              if (b) {
                pe = hi - WAVE + (64 - __clzll((long long)b));
                break;
              }
            }
            high |= pe > ps && a.bytes[pe - 1] >= 0x80;
          }
        }
        if (lane == 0) {
          a.out_len[r] = pe - ps;
          if (a.begin != nullptr) a.begin[r] = ps;
          if (high) *a.flag = 1;
        }
      }
    }
  }
}

// One side of a build: a column's bytes and offsets, or (bytes == nullptr)
// the literal.  `begin`, where set, holds the first byte of each row's part
// in place of offsets[r], and the part runs as far as the output row does.
struct SxSrc {
  const uint8_t* bytes;
  const int64_t* offsets;
  const int64_t* begin;
  int64_t nbytes;
};

struct SxConcatMeasureArgs {
  SxSrc a, b;
  const uint8_t* mask;
  int64_t* out_off;  // n + 1 entries: 0, then the lengths
  int64_t n;
  int64_t lit_len;
};

__global__ void __launch_bounds__(SX_THREADS)
string_concat_measure_kernel(const SxConcatMeasureArgs c) {
  const int t = threadIdx.x;
  const int64_t tiles = (c.n + SX_TILE - 1) / SX_TILE;
  if (blockIdx.x == 0 && t == 0) c.out_off[0] = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * SX_TILE;
    const int rows = (int)(c.n - r0 < SX_TILE ? c.n - r0 : SX_TILE);
    if (t >= rows) continue;
    const int64_t r = r0 + t;
    int64_t len = 0;
    if (c.mask == nullptr || c.mask[r] != 0) {
      const SxSrc* side[2] = {&c.a, &c.b};
      for (int k = 0; k < 2; ++k) {
        if (side[k]->offsets == nullptr) {
          len += c.lit_len;
          continue;
        }
        int64_t b0, b1, s, e;
        tile_range(side[k]->offsets, side[k]->nbytes, r0, rows, b0, b1);
        row_range(side[k]->offsets, r, b0, b1, s, e);
        len += e - s;
      }
    }
    c.out_off[1 + r] = len;
  }
}

// ------------------------------------------------------------------ build

struct SxBuildArgs {
  SxSrc a, b;
  const int64_t* out_off;  // n + 1
  uint8_t* out;
  int64_t n;
  int64_t total;
  int32_t lit_len;
  uint32_t lit[SX_MAX_LIT / 4];
};

__global__ void __launch_bounds__(SX_THREADS)
string_build_kernel(const SxBuildArgs g) {
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[SX_STAGE_ALLOC];
  __shared__ int32_t s_oo[SX_TILE + 1];  // output offsets within the tile
  __shared__ int32_t s_ab[SX_TILE], s_al[SX_TILE];  // A part: stage pos, len
  __shared__ int32_t s_bb[SX_TILE], s_bl[SX_TILE];  // B part

  const int t = threadIdx.x;
  const int lane = t & (WAVE - 1);
  const int wave = t / WAVE;
  const bool a_lit = g.a.bytes == nullptr, b_lit = g.b.bytes == nullptr;
  const int lit_len = g.lit_len;
  if (t < SX_MAX_LIT / 4) ((uint32_t*)(s_stage + SX_LIT_POS))[t] = g.lit[t];
  const int64_t tiles = (g.n + SX_TILE - 1) / SX_TILE;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * SX_TILE;
    const int rows = (int)(g.n - r0 < SX_TILE ? g.n - r0 : SX_TILE);
    const int64_t O0 = clamp64(g.out_off[r0], 0, g.total);
    const int64_t O1 = clamp64(g.out_off[r0 + rows], O0, g.total);
    int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (!a_lit) tile_range(g.a.offsets, g.a.nbytes, r0, rows, a0, a1);
    if (!b_lit) tile_range(g.b.offsets, g.b.nbytes, r0, rows, b0, b1);
    __syncthreads();  // literal staged; previous tile's gathers done
    if (O1 == O0) continue;

    if ((a1 - a0) + (b1 - b0) <= SX_STAGE) {
      int lead_a = 0, lead_b = 0, pos_b = 0;
      if (!a_lit) {
        lead_a = stage_tile(s_stage, g.a.bytes, g.a.nbytes, a0,
                            (int)(a1 - a0), t);
        pos_b = a1 > a0 ? ((lead_a + (int)(a1 - a0) + 15) >> 4) << 4 : 0;
      }
      if (!b_lit)
        lead_b = stage_tile(s_stage + pos_b, g.b.bytes, g.b.nbytes, b0,
                            (int)(b1 - b0), t);
      for (int i = t; i <= rows; i += SX_THREADS)
        s_oo[i] = (int)(clamp64(g.out_off[r0 + i], O0, O1) - O0);
      if (t < rows) {
        const int64_t r = r0 + t;
        int64_t s, e;
        if (a_lit) {
          s_ab[t] = SX_LIT_POS;
          s_al[t] = lit_len;
        } else {
          row_range(g.a.offsets, r, a0, a1, s, e);
          if (g.a.begin != nullptr) {
            s = clamp64(g.a.begin[r], a0, a1);
            e = a1;
          }
          s_ab[t] = lead_a + (int)(s - a0);
          s_al[t] = (int)(e - s);
        }
        if (b_lit) {
          s_bb[t] = SX_LIT_POS;
          s_bl[t] = lit_len;
        } else {
          row_range(g.b.offsets, r, b0, b1, s, e);
          s_bb[t] = pos_b + lead_b + (int)(s - b0);
          s_bl[t] = (int)(e - s);
        }
      }
      __syncthreads();

      const int out_bytes = (int)(O1 - O0);
      const uintptr_t dst0 = (uintptr_t)g.out + (uint64_t)O0;
      const uintptr_t vb = dst0 & ~(uintptr_t)15;
      const int lead_o = (int)(dst0 - vb);
      const int nvec = (lead_o + out_bytes + 15) >> 4;
      for (int v = t; v < nvec; v += SX_THREADS) {
        const int ob = v * 16 - lead_o;  // output byte of the vector's byte 0
        const int first = ob < 0 ? 0 : ob;
        // the last row that starts at or before `first`: the rows between it
        // and `first` are empty, and it is not, as first < s_oo[rows]
        int lo = 0, hi = rows;
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (s_oo[mid] <= first) lo = mid; else hi = mid;
        }
        int row = lo, rs = s_oo[row], re = s_oo[row + 1];
        int al = min(s_al[row], re - rs), ab = s_ab[row];
        int bb = s_bb[row], bl = s_bl[row];
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int o = ob + k;
          if (o < 0 || o >= out_bytes) continue;
          while (o >= re) {  // o < s_oo[rows], so row stays below rows
            ++row;
            rs = re;
            re = s_oo[row + 1];
            al = min(s_al[row], re - rs);
            ab = s_ab[row];
            bb = s_bb[row];
            bl = s_bl[row];
          }
          const int d = o - rs;
          uint32_t byte = 0;
          if (d < al) byte = s_stage[min(ab + d, SX_STAGE_ALLOC - 1)];
          else if (d - al < bl)
            byte = s_stage[min(bb + d - al, SX_STAGE_ALLOC - 1)];
          w[k >> 2] |= byte << ((k & 3) * 8);
        }
        uint8_t* dst = (uint8_t*)(vb + (uintptr_t)v * 16);
        if (ob >= 0 && ob + 16 <= out_bytes) {
          *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (ob + k >= 0 && ob + k < out_bytes)
              dst[k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
        }
      }
    } else {
      const uint8_t* lit = s_stage + SX_LIT_POS;
      for (int i = wave; i < rows; i += SX_WAVES) {
        const int64_t r = r0 + i;
        const int64_t o0 = clamp64(g.out_off[r], O0, O1);
        const int64_t len = clamp64(g.out_off[r + 1], o0, O1) - o0;
        int64_t as = 0, ae = lit_len, bs = 0, be = lit_len;
        if (!a_lit) {
          row_range(g.a.offsets, r, a0, a1, as, ae);
          if (g.a.begin != nullptr) {
            as = clamp64(g.a.begin[r], a0, a1);
            ae = a1;
          }
        }
        if (!b_lit) row_range(g.b.offsets, r, b0, b1, bs, be);
        const int64_t al = ae - as < len ? ae - as : len;
        const int64_t bl = be - bs;
        for (int64_t j = lane; j < len; j += WAVE) {
          uint8_t byte = 0;
          if (j < al) byte = a_lit ? lit[j] : g.a.bytes[as + j];
          else if (j - al < bl)
            byte = b_lit ? lit[j - al] : g.b.bytes[bs + j - al];
          g.out[o0 + j] = byte;
        }
      }
    }
  }
}

// --------------------------------------------------------------- case map

// bit 5 flipped in the bytes of x within [first, first + 26); bytes >= 0x80
// pass through
DEV_INLINE uint32_t case_word(uint32_t x, uint32_t first) {
  const uint32_t y = x & 0x7F7F7F7Fu;
  const uint32_t ge = y + (0x80u - first) * 0x01010101u;
  const uint32_t gt = y + (0x80u - first - 26u) * 0x01010101u;
  return x ^ ((ge & ~gt & ~x & 0x80808080u) >> 2);
}

__global__ void __launch_bounds__(SX_THREADS)
string_case_kernel(const uint8_t* in, uint8_t* out, int64_t nbytes,
                   uint32_t first, int64_t* flag) {
  const int64_t tid = blockIdx.x * (int64_t)SX_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * SX_THREADS;
  uint32_t high = 0;
  int64_t done = 0;
  if ((((uintptr_t)in | (uintptr_t)out) & 15) == 0) {
    const int64_t nvec = nbytes >> 4;
    for (int64_t v = tid; v < nvec; v += stride) {
      uint4 q = ((const uint4*)in)[v];
      high |= q.x | q.y | q.z | q.w;
      q.x = case_word(q.x, first);
      q.y = case_word(q.y, first);
      q.z = case_word(q.z, first);
      q.w = case_word(q.w, first);
      ((uint4*)out)[v] = q;
    }
    done = nvec << 4;
  }
  for (int64_t p = done + tid; p < nbytes; p += stride) {
    const uint32_t x = in[p];
    high |= x;
    out[p] = (uint8_t)case_word(x, first);
  }
  if (high & 0x80808080u) *flag = 1;
}

// ------------------------------------------------------------------- host

int64_t strxform_lds_bytes() { return SX_STAGE; }

namespace {

bool dev1d(const torch::Tensor& x, const torch::Tensor& like,
           torch::ScalarType st) {
  return x.is_cuda() && x.device() == like.device() && x.dim() == 1 &&
         x.is_contiguous() && x.scalar_type() == st;
}

int blocks_for(int64_t n, int64_t max_blocks, const char* who) {
  TORCH_CHECK(1 <= max_blocks && max_blocks <= SX_MAX_BLOCKS, who,
              ": max_blocks must be in [1, ", SX_MAX_BLOCKS, "]");
  return (int)std::min<int64_t>(max_blocks, (n + SX_TILE - 1) / SX_TILE);
}

// a column side: bytes and offsets of n + 1 entries on one device
SxSrc column_src(const torch::Tensor& bytes, const torch::Tensor& offsets,
                 int64_t n, const char* who) {
  TORCH_CHECK(dev1d(offsets, offsets, torch::kInt64) &&
                  offsets.numel() == n + 1,
              who, ": offsets must be a contiguous int64 device tensor of "
              "n + 1 entries");
  TORCH_CHECK(dev1d(bytes, offsets, torch::kUInt8), who,
              ": bytes must be a contiguous uint8 tensor on the offsets' "
              "device");
  SxSrc s;
  s.bytes = bytes.data_ptr<uint8_t>();
  s.offsets = offsets.data_ptr<int64_t>();
  s.begin = nullptr;
  s.nbytes = bytes.numel();
  return s;
}

const SxSrc kLiteral = {nullptr, nullptr, nullptr, 0};

}  // namespace

std::vector<torch::Tensor> string_measure(torch::Tensor bytes,
                                          torch::Tensor offsets,
                                          c10::optional<torch::Tensor> mask,
                                          int64_t op, int64_t start,
                                          int64_t stop, bool has_stop,
                                          int64_t max_blocks) {
  TORCH_CHECK(offsets.dim() == 1 && offsets.numel() >= 1,
              "string_measure: offsets must have n + 1 entries");
  const int64_t n = offsets.numel() - 1;
  const SxSrc src = column_src(bytes, offsets, n, "string_measure");
  TORCH_CHECK(!mask.has_value() ||
                  (dev1d(*mask, offsets, torch::kUInt8) && mask->numel() == n),
              "string_measure: mask must be a contiguous uint8 tensor of n "
              "entries on the offsets' device");
  TORCH_CHECK(SX_LEN <= op && op <= SX_SLICE, "string_measure: op ", op);
  const int nblocks = blocks_for(n, max_blocks, "string_measure");
  auto i64 = torch::dtype(torch::kInt64).device(offsets.device());

  SxMeasureArgs a;
  std::memset(&a, 0, sizeof(a));
  std::vector<torch::Tensor> out;
  if (op == SX_LEN) {
    out = {torch::empty({n}, i64)};
    a.out_len = out[0].data_ptr<int64_t>();
  } else {
    out = {torch::zeros({n + 1}, i64), torch::empty({n}, i64),
           torch::zeros({1}, i64)};
    a.out_len = out[0].data_ptr<int64_t>() + 1;
    a.zero = out[0].data_ptr<int64_t>();
    a.begin = out[1].data_ptr<int64_t>();
    a.flag = out[2].data_ptr<int64_t>();
  }
  if (n == 0) return out;
  a.bytes = src.bytes;
  a.offsets = src.offsets;
  a.mask = mask.has_value() ? mask->data_ptr<uint8_t>() : nullptr;
  a.n = n;
  a.nbytes = src.nbytes;
  a.start = start;
  a.stop = stop;
  a.has_stop = has_stop ? 1 : 0;
  a.op = (int32_t)op;
  hipLaunchKernelGGL(string_measure_kernel, dim3(nblocks), dim3(SX_THREADS),
                     0, current_stream(), a);
  check_launch("string_measure");
  return out;
}

torch::Tensor string_concat_measure(c10::optional<torch::Tensor> a_offsets,
                                    int64_t a_nbytes,
                                    c10::optional<torch::Tensor> b_offsets,
                                    int64_t b_nbytes, int64_t lit_len,
                                    c10::optional<torch::Tensor> mask,
                                    int64_t max_blocks) {
  TORCH_CHECK(a_offsets.has_value() || b_offsets.has_value(),
              "string_concat_measure: one side at least is a column");
  const torch::Tensor& ref = a_offsets.has_value() ? *a_offsets : *b_offsets;
  TORCH_CHECK(ref.dim() == 1 && ref.numel() >= 1,
              "string_concat_measure: offsets must have n + 1 entries");
  const int64_t n = ref.numel() - 1;
  TORCH_CHECK(0 <= lit_len && lit_len <= SX_MAX_LIT,
              "string_concat_measure: a literal has at most ", SX_MAX_LIT,
              " bytes");
  SxConcatMeasureArgs c;
  std::memset(&c, 0, sizeof(c));
  auto side = [&](const c10::optional<torch::Tensor>& offs, int64_t nbytes) {
    SxSrc s = kLiteral;
    if (offs.has_value()) {
      TORCH_CHECK(dev1d(*offs, ref, torch::kInt64) && offs->numel() == n + 1 &&
                      nbytes >= 0,
                  "string_concat_measure: offsets must be contiguous int64 "
                  "device tensors of n + 1 entries");
      s.offsets = offs->data_ptr<int64_t>();
      s.nbytes = nbytes;
    }
    return s;
  };
  c.a = side(a_offsets, a_nbytes);
  c.b = side(b_offsets, b_nbytes);
  TORCH_CHECK(!mask.has_value() ||
                  (dev1d(*mask, ref, torch::kUInt8) && mask->numel() == n),
              "string_concat_measure: mask must be a contiguous uint8 tensor "
              "of n entries on the offsets' device");
  const int nblocks = blocks_for(n, max_blocks, "string_concat_measure");
  auto out = torch::zeros(
      {n + 1}, torch::dtype(torch::kInt64).device(ref.device()));
  if (n == 0) return out;
  c.mask = mask.has_value() ? mask->data_ptr<uint8_t>() : nullptr;
  c.out_off = out.data_ptr<int64_t>();
  c.n = n;
  c.lit_len = lit_len;
  hipLaunchKernelGGL(string_concat_measure_kernel, dim3(nblocks),
                     dim3(SX_THREADS), 0, current_stream(), c);
  check_launch("string_concat_measure");
  return out;
}

torch::Tensor string_build(torch::Tensor out_offsets, int64_t total,
                           c10::optional<torch::Tensor> a_bytes,
                           c10::optional<torch::Tensor> a_offsets,
                           c10::optional<torch::Tensor> a_begin,
                           c10::optional<torch::Tensor> b_bytes,
                           c10::optional<torch::Tensor> b_offsets,
                           torch::Tensor literal, int64_t max_blocks) {
  TORCH_CHECK(dev1d(out_offsets, out_offsets, torch::kInt64) &&
                  out_offsets.numel() >= 1 && total >= 0,
              "string_build: out_offsets must be a contiguous int64 device "
              "tensor of n + 1 entries");
  const int64_t n = out_offsets.numel() - 1;
  TORCH_CHECK(a_bytes.has_value() == a_offsets.has_value() &&
                  b_bytes.has_value() == b_offsets.has_value() &&
                  (a_bytes.has_value() || b_bytes.has_value()),
              "string_build: a side is bytes with offsets, or the literal, "
              "and one side at least is a column");
  TORCH_CHECK(literal.is_cpu() && literal.dim() == 1 &&
                  literal.is_contiguous() &&
                  literal.scalar_type() == torch::kUInt8 &&
                  literal.numel() <= SX_MAX_LIT,
              "string_build: the literal is a host uint8 tensor of at most ",
              SX_MAX_LIT, " bytes; it travels in the kernel arguments");
  SxBuildArgs g;
  std::memset(&g, 0, sizeof(g));
  g.a = a_bytes.has_value()
            ? column_src(*a_bytes, *a_offsets, n, "string_build") : kLiteral;
  g.b = b_bytes.has_value()
            ? column_src(*b_bytes, *b_offsets, n, "string_build") : kLiteral;
  TORCH_CHECK((!a_offsets.has_value() ||
               a_offsets->device() == out_offsets.device()) &&
                  (!b_offsets.has_value() ||
                   b_offsets->device() == out_offsets.device()),
              "string_build: every tensor is on one device");
  if (a_begin.has_value()) {
    TORCH_CHECK(a_bytes.has_value() &&
                    dev1d(*a_begin, out_offsets, torch::kInt64) &&
                    a_begin->numel() == n,
                "string_build: a_begin must be a contiguous int64 tensor of n "
                "entries beside a column");
    g.a.begin = a_begin->data_ptr<int64_t>();
  }
  const int nblocks = blocks_for(n, max_blocks, "string_build");
  auto out = torch::empty(
      {total}, torch::dtype(torch::kUInt8).device(out_offsets.device()));
  if (n == 0 || total == 0) return out;
  g.out_off = out_offsets.data_ptr<int64_t>();
  g.out = out.data_ptr<uint8_t>();
  g.n = n;
  g.total = total;
  g.lit_len = (int32_t)literal.numel();
  std::memcpy(g.lit, literal.data_ptr<uint8_t>(), (size_t)literal.numel());
  hipLaunchKernelGGL(string_build_kernel, dim3(nblocks), dim3(SX_THREADS), 0,
                     current_stream(), g);
  check_launch("string_build");
  return out;
}

std::vector<torch::Tensor> string_case(torch::Tensor bytes, bool upper,
                                       int64_t max_blocks) {
  TORCH_CHECK(dev1d(bytes, bytes, torch::kUInt8),
              "string_case: bytes must be a contiguous uint8 device tensor");
  const int64_t nbytes = bytes.numel();
  // a thread takes a 16-byte vector a step
  const int nblocks =
      blocks_for((nbytes + 15) / 16, max_blocks, "string_case");
  auto out = torch::empty_like(bytes);
  auto flag = torch::zeros(
      {1}, torch::dtype(torch::kInt64).device(bytes.device()));
  if (nbytes == 0) return {out, flag};
  hipLaunchKernelGGL(string_case_kernel, dim3(nblocks), dim3(SX_THREADS), 0,
                     current_stream(), bytes.data_ptr<uint8_t>(),
                     out.data_ptr<uint8_t>(), nbytes,
                     (uint32_t)(upper ? 'a' : 'A'), flag.data_ptr<int64_t>());
  check_launch("string_case");
  return {out, flag};
}
