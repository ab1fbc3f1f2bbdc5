// On-GPU Parquet decode kernels for gfx950 (MI355X): page-parallel snappy
// decompression, definition-level -> validity-mask expansion, RLE/bit-packed
// dictionary-code expansion, fixed-width value copy and BYTE_ARRAY (string)
// assembly.  One 64-lane wavefront per page.  Snappy streams are parsed 64
// candidate headers at a time out of an LDS window and executed one element
// per lane (see pq_decompress_page); in the level / code / string kernels lane 0
// parses run headers and varints and broadcasts work items with __shfl, and
// all 64 lanes execute the expansions.  Pages are the parallel axis.  The
// per-chunk entry points run one column chunk's pages per launch (420
// pages of about 160 KB for a 2^23-row int64 chunk of the flagship shard);
// pq_decompress_multi takes a table of absolute page addresses, so the
// pipelined shard reader decompresses every column chunk of a group of row
// groups in one launch (about 2100 pages per row group of that shard), and
// pq_values_multi then writes the values of the group's null-free chunks
// straight into the shard's columns.
//
// Also hosts the C++ (host-side) page-header parser: a minimal Thrift
// compact-protocol walk over the chunk buffer, returning a page table as
// numpy-compatible tensors (the Python version cost ~10-30us/page).
//
// Reference behavioral spec (no code reuse): parquet-format spec;
// reference role: cudf::io::read_parquet used by
// bodo/pandas/physical/gpu_read_parquet.h and bodo/io/parquet_reader.cpp.

#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <cstring>
#include <vector>

#include "common.h"

#define CHECK_HIP_PQ(x)                                                 \
  do {                                                                  \
    hipError_t e = (x);                                                 \
    TORCH_CHECK(e == hipSuccess, "HIP error: ", hipGetErrorString(e));  \
  } while (0)

static hipStream_t pq_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// Per data-page metadata, filled on host from page headers.
struct PageMeta {
  int64_t src_off;   // compressed page body offset in the chunk buffer
  int64_t dst_off;   // decompressed offset in scratch (8-byte aligned)
  int64_t val_off;   // first value index of this page within the chunk
  int32_t src_len;   // compressed body length
  int32_t dst_len;   // decompressed length
  int32_t nv;        // value count incl. nulls
  int32_t flags;     // bit0: page has def-level section; bit1: snappy
};

#define PQF_HAS_DEF 1
#define PQF_SNAPPY 2

// ---------------------------------------------------------------------
// snappy decompression, one wave per page.
//
// The stream is walked 64 bytes at a time:
//   window  - 1 KiB of the compressed stream sits in LDS (one wave per
//             block), loaded with one coalesced 16-B load per lane;
//   parse   - lane l decodes the element header that would start at byte
//             l of the 64, then six rounds of pointer jumping over the
//             lanes' "next header" links mark the lanes on the chain
//             from byte 0: those hold the true elements.  A prefix sum
//             of their lengths gives every element its output position;
//   execute - every marked lane copies its own element.  A copy whose
//             source lies in this batch's own output waits for a later
//             round: a round runs each pending element whose source
//             ends at or below the output position of the first pending
//             element.
// Elements longer than PQ_SHORT and overlapping copies (off < len) end a
// batch and run wave-cooperatively, 16 B per lane where source and
// destination do not overlap.  Between rounds the wave drains its own
// vector-memory operations and fences at workgroup scope: the ordering
// needed is between lanes of this one wave.
// ---------------------------------------------------------------------

#define PQ_WIN 1024   // window bytes: 16 per lane
#define PQ_WIN_WORDS (PQ_WIN / 4 + 4)  // + zero words a peek may touch
#define PQ_SHORT 32   // longest element a single lane copies

struct PagePtr {  // page table entry of pq_decompress_multi
  const uint8_t* src;  // compressed page body
  uint8_t* dst;        // decompressed page
  int32_t src_len;
  int32_t dst_len;
  int32_t flags;       // PQF_SNAPPY
  int32_t pad;
};

DEV_INLINE int pq_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <class T>
DEV_INLINE T* pq_uni_ptr(T* p) {
  uint64_t v = (uint64_t)p;
  uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (T*)(((uint64_t)hi << 32) | lo);
}

// stores of this wave become visible to later loads of this wave
DEV_INLINE void pq_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Load stream bytes [pos, pos + PQ_WIN) into win, pos = ip rounded down
// to a 16-B address; returns pos (may be < 0).  Bytes outside
// [0, src_len) are never read: they are 0.  The block is one wave.
DEV_INLINE int pq_window_load(uint32_t* win, const uint8_t* __restrict__ in,
                              int ip, int src_len, int lane) {
  int pos = ip - (int)((uintptr_t)(in + ip) & 15);
  int c = pos + lane * 16;
  const uint8_t* g = in + c;
  uint4 v;
  if (c >= 0 && c + 16 <= src_len) {
    v = *(const uint4*)g;
  } else {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      int q = c + b;
      if (q >= 0 && q < src_len) w[b >> 2] |= (uint32_t)g[b] << (8 * (b & 3));
    }
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  __syncthreads();  // reads of the previous window are done
  *(uint4*)(win + lane * 4) = v;
  if (lane < 4) win[PQ_WIN / 4 + lane] = 0;
  __syncthreads();
  return pos;
}

// 8 bytes at window offset rel, 0 <= rel < PQ_WIN
DEV_INLINE uint64_t pq_window_peek(const uint32_t* win, int rel) {
  const uint32_t* q = win + (rel >> 2);
  uint64_t v = (uint64_t)q[0] | ((uint64_t)q[1] << 32);
  return v >> ((rel & 3) * 8);  // 5 bytes or more are valid
}

DEV_INLINE int pq_lane_get(int v, int src_lane) {  // per-lane source
  return __builtin_amdgcn_ds_bpermute(src_lane << 2, v);
}

// one lane copies len <= PQ_SHORT bytes; [s, s+len) and [d, d+len) are
// disjoint, nothing outside them is touched
DEV_INLINE void pq_lane_copy(uint8_t* d, const uint8_t* s, int len) {
  uint64_t v[PQ_SHORT / 8];
  uint32_t t4 = 0;
  uint16_t t2 = 0;
  uint8_t t1 = 0;
  int nq = len >> 3;
#pragma unroll
  for (int q = 0; q < PQ_SHORT / 8; ++q)
    if (q < nq) __builtin_memcpy(&v[q], s + 8 * q, 8);
  int r = nq * 8;
  if (len & 4) { __builtin_memcpy(&t4, s + r, 4); r += 4; }
  if (len & 2) { __builtin_memcpy(&t2, s + r, 2); r += 2; }
  if (len & 1) t1 = s[r];
#pragma unroll
  for (int q = 0; q < PQ_SHORT / 8; ++q)
    if (q < nq) __builtin_memcpy(d + 8 * q, &v[q], 8);
  r = nq * 8;
  if (len & 4) { __builtin_memcpy(d + r, &t4, 4); r += 4; }
  if (len & 2) { __builtin_memcpy(d + r, &t2, 2); r += 2; }
  if (len & 1) d[r] = t1;
}

// the wave copies len bytes, disjoint ranges: byte head up to a 16-B
// destination boundary, 16 B per lane, byte tail
DEV_INLINE void pq_wave_copy(uint8_t* d, const uint8_t* s, int len, int lane) {
  int head = (int)((0 - (uintptr_t)d) & 15);
  if (head > len) head = len;
  if (lane < head) d[lane] = s[lane];
  int body = (len - head) & ~15;
  uint8_t* db = d + head;
  const uint8_t* sb = s + head;
  int i = lane * 16;
  for (; i + 3 * WAVE * 16 < body; i += 4 * WAVE * 16) {  // 4 loads in flight
    uint4 v0, v1, v2, v3;
    __builtin_memcpy(&v0, sb + i, 16);
    __builtin_memcpy(&v1, sb + i + WAVE * 16, 16);
    __builtin_memcpy(&v2, sb + i + 2 * WAVE * 16, 16);
    __builtin_memcpy(&v3, sb + i + 3 * WAVE * 16, 16);
    *(uint4*)(db + i) = v0;
    *(uint4*)(db + i + WAVE * 16) = v1;
    *(uint4*)(db + i + 2 * WAVE * 16) = v2;
    *(uint4*)(db + i + 3 * WAVE * 16) = v3;
  }
  for (; i < body; i += WAVE * 16) {
    uint4 v;
    __builtin_memcpy(&v, sb + i, 16);
    *(uint4*)(db + i) = v;
  }
  int t = head + body + lane;
  if (t < len) d[t] = s[t];
}

// All arguments but lane are wave-uniform; win is this wave's window.
DEV_INLINE void pq_decompress_page(const uint8_t* __restrict__ in,
                                   uint8_t* out, int src_len, int dst_len,
                                   int flags, int lane, uint32_t* win) {
  if (!(flags & PQF_SNAPPY)) {  // uncompressed page: copy into scratch
    pq_wave_copy(out, in, dst_len, lane);
    return;
  }
  if (src_len <= 0) return;
  int wpos = pq_window_load(win, in, 0, src_len, lane);
  int ip = 0, opos = 0;
  {  // skip the uncompressed-length varint preamble (at most 5 bytes)
    bool more = true;
    for (int i = 0; i < 5 && more; ++i) {
      if (ip >= src_len) return;
      more = pq_window_peek(win, ip - wpos) & 0x80;
      ip++;
    }
    if (more) return;  // corrupt
  }
  while (ip < src_len && opos < dst_len) {
    // 64 candidate headers + 5 header bytes stay inside the window
    if (ip - wpos > PQ_WIN - WAVE - 5)
      wpos = pq_window_load(win, in, ip, src_len, lane);
    // ---- parse: this lane's candidate header at stream position p
    int p = ip + lane;
    uint64_t h = pq_window_peek(win, p - wpos);
    int tag = (int)(h & 0xFF);
    int k = tag & 3;
    int len = (tag >> 2) + 1, hl, off = 0;
    bool bad = false;
    if (k == 0) {  // literal
      hl = 1;
      if (len > 60) {
        int nb = len - 60;
        uint32_t raw = (uint32_t)(h >> 8);
        if (nb < 4) raw &= (1u << (8 * nb)) - 1;
        bad = raw >= 0x7FFFFFFFu;
        len = bad ? 1 : (int)raw + 1;
        hl = 1 + nb;
      }
    } else if (k == 1) {
      len = ((tag >> 2) & 7) + 4;
      off = ((tag >> 5) << 8) | (int)((h >> 8) & 0xFF);
      hl = 2;
    } else if (k == 2) {
      off = (int)((h >> 8) & 0xFFFF);
      hl = 3;
    } else {
      uint32_t o = (uint32_t)(h >> 8);
      bad = o > 0x7FFFFFFFu;
      off = (int)(o & 0x7FFFFFFFu);
      hl = 5;
    }
    // corrupt input stops the page: header or literal past src_len, ...
    bool live = p < src_len;
    bad = bad || hl > src_len - p;
    if (k == 0) bad = bad || len > src_len - p - hl;
    else bad = bad || off <= 0;
    bool coop = len > PQ_SHORT || (k != 0 && off < len);
    bool stop = bad || coop;
    // stream bytes to the next header; meaningful when !stop: <= 37
    int adv = hl + (k == 0 && !stop ? len : 0);
    // ---- the lanes on the chain from byte 0 hold the real elements
    uint32_t mlo = live && lane < 32 ? 1u << lane : 0;
    uint32_t mhi = live && lane >= 32 ? 1u << (lane - 32) : 0;
    int jump = (!live || stop || lane + adv > WAVE - 1) ? WAVE : lane + adv;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      int sl = jump & (WAVE - 1);
      uint32_t tlo = (uint32_t)pq_lane_get((int)mlo, sl);
      uint32_t thi = (uint32_t)pq_lane_get((int)mhi, sl);
      int tj = pq_lane_get(jump, sl);
      if (jump < WAVE) {
        mlo |= tlo;
        mhi |= thi;
        jump = tj;
      }
    }
    uint64_t chain = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)mhi) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)mlo);
    bool on = (chain >> lane) & 1;
    // ---- output positions: exclusive prefix sum of the element lengths
    // (a long element is last on the chain, so the sum cannot overflow)
    int mylen = on ? len : 0;
    int incl = mylen;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    int m_o = opos + (incl - mylen);
    // ... output past dst_len, copy from before the start of the output
    bad = bad || len > dst_len - m_o || (k != 0 && off > m_o);
    stop = bad || coop;
    uint64_t stops = __ballot(on && stop);
    int s = stops ? __builtin_ctzll(stops) : WAVE;  // first stopping element
    uint64_t batch = s < WAVE ? chain & ((1ull << s) - 1) : chain;
    // ---- execute the short elements before s
    bool pend = (batch >> lane) & 1;
    int m_src = p + hl;
    while (true) {
      uint64_t pm = __ballot(pend);
      if (!pm) break;
      // everything below the first pending element's output is complete
      int done_to = __builtin_amdgcn_readlane(m_o, __builtin_ctzll(pm));
      if (pend && (k == 0 || m_o - off + len <= done_to)) {
        const uint8_t* sp = k ? out + (m_o - off) : in + m_src;
        pq_lane_copy(out + m_o, sp, len);
        pend = false;
      }
      pq_wave_sync();
    }
    if (s == WAVE) {  // the whole chain ran: go on behind its last element
      int last = 63 - __builtin_clzll(chain);
      opos += __builtin_amdgcn_readlane(incl, last);
      ip += __builtin_amdgcn_readlane(lane + adv, last);
      continue;
    }
    if (__builtin_amdgcn_readlane((int)bad, s)) return;  // corrupt
    // ---- element s runs wave-cooperatively
    opos = __builtin_amdgcn_readlane(m_o, s);
    int big_len = __builtin_amdgcn_readlane(len, s);
    int big_off = __builtin_amdgcn_readlane(off, s);
    int big_k = __builtin_amdgcn_readlane(k, s);
    int big_src = ip + s + __builtin_amdgcn_readlane(hl, s);
    uint8_t* d = out + opos;
    if (big_k == 0) {
      pq_wave_copy(d, in + big_src, big_len, lane);
    } else if (big_off >= big_len) {
      pq_wave_copy(d, d - big_off, big_len, lane);
    } else {  // overlapping copy = pattern replication
      const uint8_t* sp = d - big_off;
      for (int i = lane; i < big_len; i += WAVE) d[i] = sp[i % big_off];
    }
    pq_wave_sync();
    opos += big_len;
    ip = big_src + (big_k == 0 ? big_len : 0);
  }
}

__global__ void pq_decompress_kernel(const uint8_t* __restrict__ src,
                                     const PageMeta* __restrict__ pages,
                                     int n_pages, uint8_t* dst) {
  int wave = pq_uni((int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE));
  int lane = threadIdx.x % WAVE;
  int n_waves = (int)((gridDim.x * blockDim.x) / WAVE);
  __shared__ uint32_t win[PQ_WIN_WORDS];  // blocks are one wave
  for (int p = wave; p < n_pages; p += n_waves) {
    const PageMeta* pm = pages + p;
    pq_decompress_page(pq_uni_ptr(src + pm->src_off),
                       pq_uni_ptr(dst + pm->dst_off), pq_uni(pm->src_len),
                       pq_uni(pm->dst_len), pq_uni(pm->flags), lane, win);
  }
}

// same body over a table of absolute addresses: one launch covers pages
// of many column chunks, each with its own source and scratch tensor
__global__ void pq_decompress_multi_kernel(const PagePtr* __restrict__ pages,
                                           int n_pages) {
  int wave = pq_uni((int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE));
  int lane = threadIdx.x % WAVE;
  int n_waves = (int)((gridDim.x * blockDim.x) / WAVE);
  __shared__ uint32_t win[PQ_WIN_WORDS];  // blocks are one wave
  for (int p = wave; p < n_pages; p += n_waves) {
    const PagePtr* pm = pages + p;
    pq_decompress_page(pq_uni_ptr(pm->src), pq_uni_ptr(pm->dst),
                       pq_uni(pm->src_len), pq_uni(pm->dst_len),
                       pq_uni(pm->flags), lane, win);
  }
}

// ---------------------------------------------------------------------
// definition levels -> validity mask (+ per-page valid counts and the
// byte offset of the values section, which is only knowable after
// decompression because lvl_len lives inside the page)
// ---------------------------------------------------------------------

DEV_INLINE int wave_sum_i32(int v) {
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  return __shfl(v, 0);
}

DEV_INLINE int64_t dev_varint(const uint8_t* b, int64_t* pos) {
  int64_t out = 0;
  int shift = 0;
  while (true) {
    uint8_t v = b[*pos];
    (*pos)++;
    out |= (int64_t)(v & 0x7F) << shift;
    if (!(v & 0x80)) return out;
    shift += 7;
  }
}

__global__ void pq_def_levels_kernel(const uint8_t* __restrict__ scratch,
                                     const PageMeta* __restrict__ pages,
                                     int n_pages, int bitwidth, int max_def,
                                     uint8_t* __restrict__ mask,
                                     int32_t* __restrict__ n_valid,
                                     int32_t* __restrict__ val_data_off) {
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int lane = threadIdx.x % WAVE;
  int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / WAVE;
  for (int64_t p = wave; p < n_pages; p += n_waves) {
    PageMeta pm = pages[p];
    const uint8_t* base = scratch + pm.dst_off;
    uint8_t* m = mask + pm.val_off;
    int64_t nv = pm.nv;
    if (!(pm.flags & PQF_HAS_DEF)) {
      for (int64_t i = lane; i < nv; i += WAVE) m[i] = 1;
      if (lane == 0) {
        n_valid[p] = (int32_t)nv;
        val_data_off[p] = 0;
      }
      continue;
    }
    int32_t lvl_len = (int32_t)base[0] | ((int32_t)base[1] << 8) |
                      ((int32_t)base[2] << 16) | ((int32_t)base[3] << 24);
    if (lane == 0) val_data_off[p] = 4 + lvl_len;
    const uint8_t* lv = base + 4;
    int64_t pos = 0, out = 0;
    int width_bytes = (bitwidth + 7) / 8;
    int valid = 0;
    while (out < nv && pos < lvl_len) {
      int64_t h = 0, val = 0, bitoff = 0, count;
      if (lane == 0) h = dev_varint(lv, &pos);
      h = __shfl(h, 0);
      if (h & 1) {  // bit-packed groups
        int64_t groups = h >> 1;
        count = groups * 8;
        if (count > nv - out) count = nv - out;
        bitoff = __shfl(pos, 0) * 8;
        int my = 0;
        for (int64_t i = lane; i < count; i += WAVE) {
          int64_t bp = bitoff + i * bitwidth;
          uint32_t w = (uint32_t)lv[bp >> 3] | ((uint32_t)lv[(bp >> 3) + 1] << 8);
          int v = (int)((w >> (bp & 7)) & ((1u << bitwidth) - 1));
          uint8_t ok = (v == max_def);
          m[out + i] = ok;
          my += ok;
        }
        valid += wave_sum_i32(my);
        if (lane == 0) pos += groups * bitwidth;
        pos = __shfl(pos, 0);
      } else {  // RLE run
        count = h >> 1;
        if (count > nv - out) count = nv - out;
        if (lane == 0) {
          val = 0;
          for (int i = 0; i < width_bytes; ++i)
            val |= (int64_t)lv[pos + i] << (8 * i);
          pos += width_bytes;
        }
        val = __shfl(val, 0);
        pos = __shfl(pos, 0);
        uint8_t ok = (val == max_def);
        for (int64_t i = lane; i < count; i += WAVE) m[out + i] = ok;
        if (ok) valid += (int)count;
      }
      out += count;
    }
    if (lane == 0) n_valid[p] = valid;
  }
}

// ---------------------------------------------------------------------
// RLE/bit-packed dictionary codes -> dense int32 codes
// ---------------------------------------------------------------------

// varint of at most 5 bytes inside b[*pos, end); false when it runs out
DEV_INLINE bool pq_varint32(const uint8_t* b, int64_t* pos, int64_t end,
                            int64_t* out) {
  int64_t v = 0;
  for (int shift = 0; shift < 35; shift += 7) {
    if (*pos >= end) return false;
    uint8_t c = b[*pos];
    (*pos)++;
    v |= (int64_t)(c & 0x7F) << shift;
    if (!(c & 0x80)) {
      *out = v;
      return true;
    }
  }
  return false;
}

#define PQ_CODES_OK 0
#define PQ_CODES_STREAM 1  // bit width or run structure, or fewer than nval
#define PQ_CODES_RANGE 2   // a code at or above code_lim (not stored)

// One wave expands the codes section of one page: base points at the
// bit-width byte, dlen bytes are the page's from there on, nval codes go
// to o[0, nval).  A code c is stored as lut[c] when lut is set and is
// dropped, with PQ_CODES_RANGE returned, unless (uint32_t)c < code_lim.
// A bit-packed value may be read as a 4-byte word that ends up to 3 bytes
// past its run: the page tables keep pages inside padded scratch.
DEV_INLINE int pq_expand_codes_page(const uint8_t* base, int64_t dlen,
                                    int64_t nval, int32_t* __restrict__ o,
                                    const int32_t* __restrict__ lut,
                                    uint32_t code_lim, int lane) {
  if (dlen < 1) return nval ? PQ_CODES_STREAM : PQ_CODES_OK;
  int bitwidth = base[0];
  const uint8_t* d = base + 1;
  dlen -= 1;
  int st = PQ_CODES_OK;
  if (bitwidth == 0) {
    if (!nval) return PQ_CODES_OK;
    if (!code_lim) return PQ_CODES_RANGE;
    int32_t v = lut ? lut[0] : 0;
    for (int64_t i = lane; i < nval; i += WAVE) o[i] = v;
    return PQ_CODES_OK;
  }
  if (bitwidth > 24) return PQ_CODES_STREAM;
  int width_bytes = (bitwidth + 7) / 8;
  int64_t pos = 0, outp = 0;
  int oob = 0;
  while (outp < nval && pos < dlen) {
    int64_t h = 0, val = 0, count;
    int okh = 1;
    if (lane == 0) okh = pq_varint32(d, &pos, dlen, &h);
    if (!__shfl(okh, 0)) break;
    h = __shfl(h, 0);
    pos = __shfl(pos, 0);
    if (h & 1) {
      int64_t groups = h >> 1;
      if (pos + groups * bitwidth > dlen) break;
      count = groups * 8;
      if (count > nval - outp) count = nval - outp;
      int64_t bitoff = pos * 8;
      for (int64_t i = lane; i < count; i += WAVE) {
        int64_t bp = bitoff + i * bitwidth;
        int64_t byte = bp >> 3;
        uint32_t w = (uint32_t)d[byte] | ((uint32_t)d[byte + 1] << 8) |
                     ((uint32_t)d[byte + 2] << 16) |
                     ((uint32_t)d[byte + 3] << 24);
        uint32_t c = (w >> (bp & 7)) & ((1u << bitwidth) - 1);
        if (c < code_lim) o[outp + i] = lut ? lut[c] : (int32_t)c;
        else oob = 1;
      }
      pos += groups * bitwidth;
    } else {
      count = h >> 1;
      if (count > nval - outp) count = nval - outp;
      if (pos + width_bytes > dlen) break;
      if (lane == 0) {
        val = 0;
        for (int i = 0; i < width_bytes; ++i)
          val |= (int64_t)d[pos + i] << (8 * i);
      }
      pos += width_bytes;
      val = __shfl(val, 0);
      uint32_t c = (uint32_t)val;
      if (c < code_lim) {
        int32_t v = lut ? lut[c] : (int32_t)c;
        for (int64_t i = lane; i < count; i += WAVE) o[outp + i] = v;
      } else if (count) {
        oob = 1;
      }
    }
    outp += count;
  }
  if (outp < nval) st |= PQ_CODES_STREAM;
  if (__ballot(oob)) st |= PQ_CODES_RANGE;
  return st;
}

__global__ void pq_expand_codes_kernel(const uint8_t* __restrict__ scratch,
                                       const PageMeta* __restrict__ pages,
                                       int n_pages,
                                       const int32_t* __restrict__ val_data_off,
                                       const int64_t* __restrict__ dense_off,
                                       const int32_t* __restrict__ n_valid,
                                       int32_t* __restrict__ out) {
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int lane = threadIdx.x % WAVE;
  int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / WAVE;
  for (int64_t p = wave; p < n_pages; p += n_waves) {
    PageMeta pm = pages[p];
    int64_t voff = val_data_off ? val_data_off[p] : 0;
    int64_t nval = n_valid ? (int64_t)n_valid[p] : (int64_t)pm.nv;
    // codes are not range-checked here: the dictionary lives on the host
    pq_expand_codes_page(scratch + pm.dst_off + voff, pm.dst_len - voff, nval,
                         out + dense_off[p], nullptr, 0xFFFFFFFFu, lane);
  }
}

// ---------------------------------------------------------------------
// PLAIN fixed-width values -> dense value buffer (byte copy; source is
// unaligned inside the decompressed page, destination is esize-aligned)
// ---------------------------------------------------------------------

// nthreads threads (tid of them this one) copy nbytes from s, at any byte
// address inside a decompressed page, to o, which is 8-byte aligned or, for
// 4-byte elements, 4-byte aligned.  Loads are aligned u64 words merged by
// a shift; the word after the last one needed may be read too, at most 15
// bytes past s + nbytes, which the 16 bytes of scratch padding cover.
// Stores: with o 8-byte aligned, nbytes / 8 words and then the bytes
// [8 * (nbytes / 8), nbytes); otherwise nbytes / 4 words and then the bytes
// [4 * (nbytes / 4), nbytes).  Either way the last byte stored is
// o[nbytes - 1], so the destination needs no padding.
DEV_INLINE void pq_copy_fixed_page(const uint8_t* __restrict__ s,
                                   uint8_t* __restrict__ o, int64_t nbytes,
                                   int tid, int nthreads) {
  int m = (int)((uintptr_t)s & 7);
  const uint64_t* sa = (const uint64_t*)(s - m);
  int sh = m * 8;
  if ((((uintptr_t)o) & 7) == 0) {
    int64_t nw = nbytes / 8;
    if (sh == 0) {
      for (int64_t i = tid; i < nw; i += nthreads) ((uint64_t*)o)[i] = sa[i];
    } else {
      for (int64_t i = tid; i < nw; i += nthreads)
        ((uint64_t*)o)[i] = (sa[i] >> sh) | (sa[i + 1] << (64 - sh));
    }
    for (int64_t i = nw * 8 + tid; i < nbytes; i += nthreads) o[i] = s[i];
  } else {  // esize 4 destination at 4-byte alignment
    int64_t nw = nbytes / 4;
    for (int64_t i = tid; i < nw; i += nthreads) {
      int64_t bit = (int64_t)i * 32 + sh;
      uint64_t w = sa[bit >> 6];
      int off = (int)(bit & 63);
      uint32_t v = (off <= 32)
                       ? (uint32_t)(w >> off)
                       : (uint32_t)((w >> off) |
                                    (sa[(bit >> 6) + 1] << (64 - off)));
      ((uint32_t*)o)[i] = v;
    }
    for (int64_t i = nw * 4 + tid; i < nbytes; i += nthreads) o[i] = s[i];
  }
}

__global__ void pq_copy_fixed_kernel(const uint8_t* __restrict__ scratch,
                                     const PageMeta* __restrict__ pages,
                                     int n_pages,
                                     const int32_t* __restrict__ val_data_off,
                                     const int64_t* __restrict__ dense_off,
                                     const int32_t* __restrict__ n_valid,
                                     int esize, uint8_t* __restrict__ out) {
  // one BLOCK per page slot (pages are up to ~1 MiB: need more than a wave)
  for (int64_t p = blockIdx.x; p < n_pages; p += gridDim.x) {
    PageMeta pm = pages[p];
    const uint8_t* s = scratch + pm.dst_off +
                       (val_data_off ? val_data_off[p] : 0);
    uint8_t* o = out + dense_off[p] * esize;
    int64_t nbytes = (n_valid ? (int64_t)n_valid[p] : (int64_t)pm.nv) * esize;
    pq_copy_fixed_page(s, o, nbytes, threadIdx.x, blockDim.x);
  }
}

// ---------------------------------------------------------------------
// Values of a whole group of row groups, decoded in place: a table of
// pages of many column chunks, each with the absolute address in the final
// shard column where its first value goes.  These chunks hold no nulls, by
// their statistics, so a page's definition levels are only checked: they
// must cover nv values, all of them 1.  A page that fails a check is left
// unwritten and its reason is ORed into *err; the reader then decodes the
// shard again on the per-chunk route.
// ---------------------------------------------------------------------

struct ValPage {  // page table entry of pq_values_multi
  const uint8_t* page;  // decompressed page (PagePtr::dst)
  uint8_t* out;         // where this page's first value goes
  const int32_t* lut;   // codes: code -> unified code, or null
  int32_t dst_len;      // decompressed page length
  int32_t nv;           // values in the page
  int32_t kind;         // PQK_CODES, or the element size of PLAIN: 4 or 8
  int32_t flags;        // PQF_HAS_DEF
  int32_t code_lim;     // codes: entries of lut, or of the dictionary
  int32_t pad;
};

#define PQK_CODES 0

#define PQE_PREFIX 1  // level section or PLAIN values do not fit the page
#define PQE_LEVELS 2  // levels malformed, short of nv, or not all 1
#define PQE_ENTRY 4   // table entry: kind, alignment, negative counts
#define PQE_CODES 8   // code stream malformed or short of nv
#define PQE_RANGE 16  // dictionary code outside the LUT / dictionary

// The block checks the level prefix of one page and returns 0 with *voff =
// offset of the values section, or PQE_* bits.  Run headers are parsed by
// every thread alike (a few bytes for RLE runs); the bytes of bit-packed
// runs are spread over the threads.  Every thread of the block calls this.
DEV_INLINE int pq_check_levels(const uint8_t* __restrict__ page, int dst_len,
                               int nv, int tid, int nthreads, int* voff) {
  int bad = 0, mine = 0;
  int64_t lvl_len = 0;
  if (dst_len < 4) {
    bad = PQE_PREFIX;
  } else {
    lvl_len = (int32_t)((uint32_t)page[0] | ((uint32_t)page[1] << 8) |
                        ((uint32_t)page[2] << 16) | ((uint32_t)page[3] << 24));
    if (lvl_len < 0 || 4 + lvl_len > dst_len) bad = PQE_PREFIX;
  }
  if (!bad) {
    const uint8_t* lv = page + 4;
    int64_t pos = 0, out = 0;
    while (out < nv && pos < lvl_len) {
      int64_t h;
      if (!pq_varint32(lv, &pos, lvl_len, &h)) break;
      int64_t count;
      if (h & 1) {  // bit-packed, 1 bit per level: groups bytes
        int64_t groups = h >> 1;
        if (pos + groups > lvl_len) break;
        count = groups * 8;
        if (count > nv - out) count = nv - out;
        int64_t full = count >> 3;
        for (int64_t i = tid; i < full; i += nthreads)
          if (lv[pos + i] != 0xFF) mine = PQE_LEVELS;
        int rest = (int)(count & 7);
        if (rest && (lv[pos + full] & ((1 << rest) - 1)) != (1 << rest) - 1)
          bad = PQE_LEVELS;
        pos += groups;
      } else {
        count = h >> 1;
        if (count > nv - out) count = nv - out;
        if (pos >= lvl_len) break;
        if (count && lv[pos] != 1) bad = PQE_LEVELS;
        pos += 1;
      }
      out += count;
    }
    if (out != nv) bad |= PQE_LEVELS;
  }
  if (__syncthreads_or(mine)) bad |= PQE_LEVELS;
  *voff = 4 + (int)lvl_len;
  return bad;
}

// KIND_CODES false: one block per PLAIN page; true: one wave (= block) per
// codes page.  Entries of the other kind are skipped.
template <bool KIND_CODES>
__global__ void pq_values_multi_kernel(const ValPage* __restrict__ pages,
                                       int n_pages, int32_t* err) {
  for (int p = blockIdx.x; p < n_pages; p += gridDim.x) {
    ValPage e = pages[p];
    if ((e.kind == PQK_CODES) != KIND_CODES) continue;
    int bad = 0, voff = 0;
    if (e.dst_len < 0 || e.nv < 0) bad = PQE_ENTRY;
    if (!KIND_CODES) {
      if (e.kind != 4 && e.kind != 8) bad = PQE_ENTRY;
      else if ((uintptr_t)e.out & 3) bad = PQE_ENTRY;
      else if (e.kind == 8 && ((uintptr_t)e.out & 7)) bad = PQE_ENTRY;
    } else if ((uintptr_t)e.out & 3) {
      bad = PQE_ENTRY;
    }
    if (!bad && (e.flags & PQF_HAS_DEF))
      bad = pq_check_levels(e.page, e.dst_len, e.nv, threadIdx.x, blockDim.x,
                            &voff);
    if (!bad) {
      if (!KIND_CODES) {
        int64_t nbytes = (int64_t)e.nv * e.kind;
        if (voff + nbytes > e.dst_len) bad = PQE_PREFIX;
        else pq_copy_fixed_page(e.page + voff, e.out, nbytes, threadIdx.x,
                                blockDim.x);
      } else {
        int st = pq_expand_codes_page(
            e.page + voff, (int64_t)e.dst_len - voff, e.nv, (int32_t*)e.out,
            e.lut, (uint32_t)(e.code_lim < 0 ? 0 : e.code_lim), threadIdx.x);
        if (st & PQ_CODES_STREAM) bad |= PQE_CODES;
        if (st & PQ_CODES_RANGE) bad |= PQE_RANGE;
      }
    }
    if (bad && threadIdx.x == 0) atomicOr(err, bad);
  }
}

// ---------------------------------------------------------------------
// PLAIN BYTE_ARRAY: pass 1 walks the 4-byte length prefixes (sequential
// per page, lane 0) emitting per-value lengths and absolute source byte
// offsets in scratch; pass 2 copies string bytes to packed destinations.
// ---------------------------------------------------------------------

__global__ void pq_byte_array_lengths_kernel(
    const uint8_t* __restrict__ scratch, const PageMeta* __restrict__ pages,
    int n_pages, const int32_t* __restrict__ val_data_off,
    const int64_t* __restrict__ dense_off, const int32_t* __restrict__ n_valid,
    int32_t* __restrict__ lengths, int64_t* __restrict__ src_abs) {
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int lane = threadIdx.x % WAVE;
  int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / WAVE;
  for (int64_t p = wave; p < n_pages; p += n_waves) {
    if (lane != 0) continue;  // sequential walk; parallelism is across pages
    PageMeta pm = pages[p];
    int64_t voff = pm.dst_off + (val_data_off ? val_data_off[p] : 0);
    const uint8_t* s = scratch + voff;
    int64_t nval = n_valid ? (int64_t)n_valid[p] : (int64_t)pm.nv;
    int32_t* L = lengths + dense_off[p];
    int64_t* A = src_abs + dense_off[p];
    int64_t pos = 0;
    for (int64_t i = 0; i < nval; ++i) {
      int32_t ln;
      __builtin_memcpy(&ln, s + pos, 4);
      L[i] = ln;
      A[i] = voff + pos + 4;
      pos += 4 + ln;
    }
  }
}

__global__ void pq_copy_strings_kernel(const uint8_t* __restrict__ scratch,
                                       const int64_t* __restrict__ src_abs,
                                       const int64_t* __restrict__ dst_off,
                                       const int32_t* __restrict__ lengths,
                                       int64_t n, uint8_t* __restrict__ out) {
  GRID_STRIDE_LOOP(i, n) {
    const uint8_t* s = scratch + src_abs[i];
    uint8_t* o = out + dst_off[i];
    int32_t ln = lengths[i];
    for (int32_t k = 0; k < ln; ++k) o[k] = s[k];
  }
}

// ---------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------

static int pq_grid_waves(int64_t n_pages, int block) {
  int waves_per_block = block / WAVE;
  int64_t b = (n_pages + waves_per_block - 1) / waves_per_block;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

// one wave per page, one wave per block: the pages of a launch differ a
// lot in cost, and single-wave blocks let the dispatcher spread them
static int pq_grid_pages(int64_t n_pages) {
  return (int)std::min<int64_t>(std::max<int64_t>(n_pages, 1), 1 << 20);
}

void pq_decompress(torch::Tensor src, torch::Tensor pages_blob,
                   int64_t n_pages, torch::Tensor scratch) {
  if (!n_pages) return;
  hipLaunchKernelGGL(pq_decompress_kernel, dim3(pq_grid_pages(n_pages)),
                     dim3(WAVE), 0, pq_stream(),
                     (const uint8_t*)src.data_ptr(),
                     (const PageMeta*)pages_blob.data_ptr(), (int)n_pages,
                     (uint8_t*)scratch.data_ptr());
  CHECK_HIP_PQ(hipGetLastError());
}

// pages_blob: device bytes of n_pages PagePtr entries (absolute device
// addresses).  The caller keeps the tensors they point into alive.
void pq_decompress_multi(torch::Tensor pages_blob, int64_t n_pages) {
  if (!n_pages) return;
  TORCH_CHECK(pages_blob.is_contiguous() &&
                  pages_blob.numel() * pages_blob.element_size() >=
                      n_pages * (int64_t)sizeof(PagePtr),
              "pq_decompress_multi: page table too small");
  hipLaunchKernelGGL(pq_decompress_multi_kernel,
                     dim3(pq_grid_pages(n_pages)), dim3(WAVE), 0, pq_stream(),
                     (const PagePtr*)pages_blob.data_ptr(), (int)n_pages);
  CHECK_HIP_PQ(hipGetLastError());
}

// pages_blob: device bytes of n_pages ValPage entries; err: one int32 on
// the device, ORed into.  Two launches whatever the table holds: PLAIN
// pages one block each, codes pages one wave each.
void pq_values_multi(torch::Tensor pages_blob, int64_t n_pages,
                     torch::Tensor err) {
  if (!n_pages) return;
  TORCH_CHECK(pages_blob.is_contiguous() &&
                  pages_blob.numel() * pages_blob.element_size() >=
                      n_pages * (int64_t)sizeof(ValPage),
              "pq_values_multi: page table too small");
  TORCH_CHECK(n_pages < (1ll << 31), "pq_values_multi: too many pages");
  TORCH_CHECK(err.scalar_type() == torch::kInt32 && err.numel() >= 1 &&
                  err.device() == pages_blob.device(),
              "pq_values_multi: err must be an int32 on the table's device");
  int grid = (int)std::min<int64_t>(n_pages, 1 << 16);
  hipLaunchKernelGGL(pq_values_multi_kernel<false>, dim3(grid), dim3(256), 0,
                     pq_stream(), (const ValPage*)pages_blob.data_ptr(),
                     (int)n_pages, (int32_t*)err.data_ptr());
  CHECK_HIP_PQ(hipGetLastError());
  hipLaunchKernelGGL(pq_values_multi_kernel<true>, dim3(grid), dim3(WAVE), 0,
                     pq_stream(), (const ValPage*)pages_blob.data_ptr(),
                     (int)n_pages, (int32_t*)err.data_ptr());
  CHECK_HIP_PQ(hipGetLastError());
}

std::vector<torch::Tensor> pq_def_levels(torch::Tensor scratch,
                                         torch::Tensor pages_blob,
                                         int64_t n_pages, int64_t bitwidth,
                                         int64_t max_def, int64_t total_nv) {
  auto dev = scratch.device();
  auto mask = torch::empty({total_nv}, torch::dtype(torch::kUInt8).device(dev));
  auto n_valid = torch::empty({n_pages},
                              torch::dtype(torch::kInt32).device(dev));
  auto vdo = torch::empty({n_pages}, torch::dtype(torch::kInt32).device(dev));
  if (n_pages) {
    int block = 256;
    hipLaunchKernelGGL(pq_def_levels_kernel,
                       dim3(pq_grid_waves(n_pages, block)), dim3(block), 0,
                       pq_stream(), (const uint8_t*)scratch.data_ptr(),
                       (const PageMeta*)pages_blob.data_ptr(), (int)n_pages,
                       (int)bitwidth, (int)max_def,
                       (uint8_t*)mask.data_ptr(),
                       (int32_t*)n_valid.data_ptr(),
                       (int32_t*)vdo.data_ptr());
    CHECK_HIP_PQ(hipGetLastError());
  }
  return {mask, n_valid, vdo};
}

torch::Tensor pq_expand_codes(torch::Tensor scratch, torch::Tensor pages_blob,
                              int64_t n_pages,
                              c10::optional<torch::Tensor> val_data_off,
                              torch::Tensor dense_off,
                              c10::optional<torch::Tensor> n_valid,
                              int64_t dense_total) {
  auto dev = scratch.device();
  auto out = torch::empty({dense_total},
                          torch::dtype(torch::kInt32).device(dev));
  if (n_pages) {
    int block = 256;
    hipLaunchKernelGGL(
        pq_expand_codes_kernel, dim3(pq_grid_waves(n_pages, block)),
        dim3(block), 0, pq_stream(), (const uint8_t*)scratch.data_ptr(),
        (const PageMeta*)pages_blob.data_ptr(), (int)n_pages,
        val_data_off.has_value() ? (const int32_t*)val_data_off->data_ptr()
                                 : nullptr,
        (const int64_t*)dense_off.data_ptr(),
        n_valid.has_value() ? (const int32_t*)n_valid->data_ptr() : nullptr,
        (int32_t*)out.data_ptr());
    CHECK_HIP_PQ(hipGetLastError());
  }
  return out;
}

torch::Tensor pq_copy_fixed(torch::Tensor scratch, torch::Tensor pages_blob,
                            int64_t n_pages,
                            c10::optional<torch::Tensor> val_data_off,
                            torch::Tensor dense_off,
                            c10::optional<torch::Tensor> n_valid,
                            int64_t esize, int64_t dense_total) {
  auto dev = scratch.device();
  auto out = torch::empty({dense_total * esize},
                          torch::dtype(torch::kUInt8).device(dev));
  if (n_pages) {
    int block = 256;
    int grid = (int)std::min<int64_t>(n_pages, 4096);
    hipLaunchKernelGGL(
        pq_copy_fixed_kernel, dim3(grid), dim3(block), 0, pq_stream(),
        (const uint8_t*)scratch.data_ptr(),
        (const PageMeta*)pages_blob.data_ptr(), (int)n_pages,
        val_data_off.has_value() ? (const int32_t*)val_data_off->data_ptr()
                                 : nullptr,
        (const int64_t*)dense_off.data_ptr(),
        n_valid.has_value() ? (const int32_t*)n_valid->data_ptr() : nullptr,
        (int)esize, (uint8_t*)out.data_ptr());
    CHECK_HIP_PQ(hipGetLastError());
  }
  return out;
}

std::vector<torch::Tensor> pq_byte_array_lengths(
    torch::Tensor scratch, torch::Tensor pages_blob, int64_t n_pages,
    c10::optional<torch::Tensor> val_data_off, torch::Tensor dense_off,
    c10::optional<torch::Tensor> n_valid, int64_t dense_total) {
  auto dev = scratch.device();
  auto lengths = torch::zeros({dense_total},
                              torch::dtype(torch::kInt32).device(dev));
  auto src_abs = torch::zeros({dense_total},
                              torch::dtype(torch::kInt64).device(dev));
  if (n_pages) {
    int block = 256;
    hipLaunchKernelGGL(
        pq_byte_array_lengths_kernel, dim3(pq_grid_waves(n_pages, block)),
        dim3(block), 0, pq_stream(), (const uint8_t*)scratch.data_ptr(),
        (const PageMeta*)pages_blob.data_ptr(), (int)n_pages,
        val_data_off.has_value() ? (const int32_t*)val_data_off->data_ptr()
                                 : nullptr,
        (const int64_t*)dense_off.data_ptr(),
        n_valid.has_value() ? (const int32_t*)n_valid->data_ptr() : nullptr,
        (int32_t*)lengths.data_ptr(), (int64_t*)src_abs.data_ptr());
    CHECK_HIP_PQ(hipGetLastError());
  }
  return {lengths, src_abs};
}

torch::Tensor pq_copy_strings(torch::Tensor scratch, torch::Tensor src_abs,
                              torch::Tensor dst_off, torch::Tensor lengths,
                              int64_t n, int64_t total_bytes) {
  auto dev = scratch.device();
  auto out = torch::empty({std::max<int64_t>(total_bytes, 1)},
                          torch::dtype(torch::kUInt8).device(dev));
  if (n) {
    int block = 256;
    hipLaunchKernelGGL(pq_copy_strings_kernel, dim3(grid_for(n, block)),
                       dim3(block), 0, pq_stream(),
                       (const uint8_t*)scratch.data_ptr(),
                       (const int64_t*)src_abs.data_ptr(),
                       (const int64_t*)dst_off.data_ptr(),
                       (const int32_t*)lengths.data_ptr(), n,
                       (uint8_t*)out.data_ptr());
    CHECK_HIP_PQ(hipGetLastError());
  }
  return out;
}

// ---------------------------------------------------------------------
// host-side page header parse (Thrift compact protocol): the Python
// version cost 10-30us per page; this walks a whole chunk in C++.
// Returns int64 tensor [n_pages, 7]:
//   0 ptype, 1 uncompressed_size, 2 compressed_size, 3 body_off,
//   4 nv, 5 encoding, 6 def_level_encoding
// ---------------------------------------------------------------------

namespace {

struct TR {
  const uint8_t* b;
  size_t pos, end;
  bool ok = true;

  uint64_t varint() {
    uint64_t out = 0;
    int shift = 0;
    while (pos < end) {
      uint8_t v = b[pos++];
      out |= (uint64_t)(v & 0x7F) << shift;
      if (!(v & 0x80)) return out;
      shift += 7;
    }
    ok = false;
    return 0;
  }
  int64_t zigzag() {
    uint64_t v = varint();
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  }
  void skip(int ftype);
  void skip_struct() {
    int16_t fid = 0;
    while (ok && pos < end) {
      uint8_t t = b[pos++];
      if (t == 0) return;
      int delta = (t >> 4) & 0x0F;
      int ft = t & 0x0F;
      fid = delta ? fid + delta : (int16_t)zigzag();
      skip(ft);
    }
  }
};

void TR::skip(int ftype) {
  switch (ftype) {
    case 1: case 2: return;               // bool encoded in type
    case 3: pos += 1; return;             // byte
    case 4: case 5: case 6: zigzag(); return;
    case 7: pos += 8; return;             // double
    case 8: { uint64_t n = varint(); pos += n; return; }  // binary
    case 9: {                              // list
      if (pos >= end) { ok = false; return; }
      uint8_t h = b[pos++];
      uint64_t sz = (h >> 4) & 0x0F;
      int et = h & 0x0F;
      if (sz == 15) sz = varint();
      for (uint64_t i = 0; i < sz && ok; ++i) skip(et);
      return;
    }
    case 12: skip_struct(); return;
    default: ok = false; return;
  }
}

}  // namespace

torch::Tensor pq_parse_headers(torch::Tensor chunk_buf) {
  const uint8_t* buf = (const uint8_t*)chunk_buf.data_ptr();
  size_t n = (size_t)chunk_buf.numel();
  std::vector<int64_t> rows;  // 7 per page
  size_t pos = 0;
  while (pos < n) {
    TR t{buf, pos, n};
    int64_t ptype = -1, usize = 0, csize = 0, nv = 0, enc = -1, defenc = -1;
    int16_t fid = 0;
    // walk PageHeader struct
    bool done = false;
    while (t.ok && !done && t.pos < n) {
      uint8_t tb = buf[t.pos++];
      if (tb == 0) { done = true; break; }
      int delta = (tb >> 4) & 0x0F;
      int ft = tb & 0x0F;
      fid = delta ? fid + delta : (int16_t)t.zigzag();
      switch (fid) {
        case 1: ptype = t.zigzag(); break;
        case 2: usize = t.zigzag(); break;
        case 3: csize = t.zigzag(); break;
        case 5: case 7: {  // data_page_header / dictionary_page_header
          if (ft != 12) { t.skip(ft); break; }
          int16_t f2 = 0;
          bool d2 = false;
          while (t.ok && !d2 && t.pos < n) {
            uint8_t b2 = buf[t.pos++];
            if (b2 == 0) { d2 = true; break; }
            int dl2 = (b2 >> 4) & 0x0F;
            int ft2 = b2 & 0x0F;
            f2 = dl2 ? f2 + dl2 : (int16_t)t.zigzag();
            if (f2 == 1 && (ft2 == 4 || ft2 == 5 || ft2 == 6)) {
              nv = t.zigzag();
            } else if (f2 == 2 && (ft2 == 4 || ft2 == 5 || ft2 == 6)) {
              enc = t.zigzag();
            } else if (fid == 5 && f2 == 3 &&
                       (ft2 == 4 || ft2 == 5 || ft2 == 6)) {
              defenc = t.zigzag();
            } else {
              t.skip(ft2);
            }
          }
          break;
        }
        default: t.skip(ft); break;
      }
    }
    if (!t.ok || !done || csize <= 0) break;
    int64_t body = (int64_t)t.pos;
    rows.insert(rows.end(), {ptype, usize, csize, body, nv, enc, defenc});
    pos = (size_t)(body + csize);
  }
  auto out = torch::empty({(int64_t)(rows.size() / 7), 7},
                          torch::dtype(torch::kInt64));
  std::memcpy(out.data_ptr(), rows.data(), rows.size() * sizeof(int64_t));
  return out;
}

// ---------------------------------------------------------------------
// fused multi-column gather: one launch materializes every fixed-width
// column (and mask) of a take_table/join output instead of one torch
// index_select per column (join-heavy queries were launch-bound;
// reference role: the single-pass materialization in cudf::gather).
// Layout: consecutive threads walk consecutive output rows of one column
// so loads from idx broadcast and stores coalesce.
// ---------------------------------------------------------------------

struct GatherCol {
  const uint8_t* src;
  uint8_t* dst;
  int64_t esize;
};

__global__ void gather_multi_kernel(const GatherCol* __restrict__ cols,
                                    int ncols, const int64_t* __restrict__ idx,
                                    int64_t n) {
  int64_t total = (int64_t)ncols * n;
  GRID_STRIDE_LOOP(t, total) {
    int c = (int)(t / n);
    int64_t i = t - (int64_t)c * n;
    int64_t j = idx[i];
    const GatherCol g = cols[c];
    switch (g.esize) {
      case 1: g.dst[i] = g.src[j]; break;
      case 2: ((uint16_t*)g.dst)[i] = ((const uint16_t*)g.src)[j]; break;
      case 4: ((uint32_t*)g.dst)[i] = ((const uint32_t*)g.src)[j]; break;
      default: ((uint64_t*)g.dst)[i] = ((const uint64_t*)g.src)[j]; break;
    }
  }
}

std::vector<torch::Tensor> gather_multi(std::vector<torch::Tensor> srcs,
                                        torch::Tensor idx) {
  int64_t n = idx.numel();
  auto dev = idx.device();
  std::vector<torch::Tensor> outs;
  std::vector<GatherCol> cols;
  for (auto& s : srcs) {
    auto o = torch::empty({n}, s.options());
    outs.push_back(o);
    GatherCol g;
    g.src = (const uint8_t*)s.data_ptr();
    g.dst = (uint8_t*)o.data_ptr();
    g.esize = s.element_size();
    cols.push_back(g);
  }
  if (n && !srcs.empty()) {
    auto cpu = torch::from_blob((void*)cols.data(),
                                {(int64_t)(cols.size() * sizeof(GatherCol))},
                                torch::kUInt8);
    auto cols_dev = cpu.to(dev, /*non_blocking=*/false);
    int block = 256;
    int64_t total = (int64_t)srcs.size() * n;
    hipLaunchKernelGGL(gather_multi_kernel, dim3(grid_for(total, block)),
                       dim3(block), 0, pq_stream(),
                       (const GatherCol*)cols_dev.data_ptr(),
                       (int)srcs.size(), (const int64_t*)idx.data_ptr(), n);
    CHECK_HIP_PQ(hipGetLastError());
  }
  return outs;
}
