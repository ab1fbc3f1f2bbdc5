// What the radix sort (sort.hip) and the radix selects (select.hip,
// segselect.hip) share: the order-preserving u64 form of every sortable
// dtype, ballot-based digit grouping, the fixed-grid split of n keys into
// per-block tile ranges, and the selects' tile load and block scan.
#pragma once

#include "common.h"

#define RS_THREADS 256
#define RS_WAVES (RS_THREADS / WAVE)
// keys per thread per tile: 8 keeps the scatter kernel at zero scratch and
// its LDS (tile of keys + ids + counters) at 30 KiB, five blocks per CU
#define RS_KPT 8
#define RS_TILE (RS_THREADS * RS_KPT)
#define RS_BINS 256
#define RS_MAX_BLOCKS 2048

// source dtypes of radix_keys_kernel and the select kernels
enum RadixKind : int {
  RK_I8 = 0, RK_I16, RK_I32, RK_I64, RK_U8, RK_F32, RK_F64,
};

// u64 whose unsigned order is torch.argsort's order of the source value
DEV_INLINE uint64_t radix_norm(const void* src, int kind, int64_t i) {
  switch (kind) {
    case RK_I8: return (uint8_t)(((const uint8_t*)src)[i] ^ 0x80u);
    case RK_I16: return (uint16_t)(((const uint16_t*)src)[i] ^ 0x8000u);
    case RK_I32: return ((const uint32_t*)src)[i] ^ 0x80000000u;
    case RK_I64: return ((const uint64_t*)src)[i] ^ 0x8000000000000000ULL;
    case RK_U8: return ((const uint8_t*)src)[i];
    case RK_F32: {
      uint32_t b = ((const uint32_t*)src)[i];
      if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;  // NaN last
      if (b == 0x80000000u) b = 0;                              // -0.0
      return (b & 0x80000000u) ? (uint32_t)~b : (b | 0x80000000u);
    }
    case RK_F64: {
      uint64_t b = ((const uint64_t*)src)[i];
      if ((b & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL) return ~0ULL;
      if (b == 0x8000000000000000ULL) b = 0;
      return (b & 0x8000000000000000ULL) ? ~b : (b | 0x8000000000000000ULL);
    }
  }
  return 0;
}

struct RadixRange {
  int64_t begin, end;  // key positions [begin, end) owned by this block
};

// block b of nblocks owns a contiguous run of whole tiles; the first
// (tiles % nblocks) blocks own one tile more
DEV_INLINE RadixRange radix_block_range(int64_t n, int64_t tiles, int nblocks,
                                        int b) {
  int64_t per = tiles / nblocks, rem = tiles % nblocks;
  int64_t t0 = b * per + (b < rem ? b : rem);
  int64_t t1 = t0 + per + (b < rem ? 1 : 0);
  RadixRange r;
  r.begin = t0 * RS_TILE;
  r.end = t1 * RS_TILE < n ? t1 * RS_TILE : n;
  return r;
}

DEV_INLINE uint32_t radix_digit(uint64_t key, int shift, uint32_t dmask) {
  return (uint32_t)(key >> shift) & dmask;
}

// lanes of this wave that are valid and hold the same digit as the caller;
// one ballot per digit bit.  Every lane of the wave must call it.
DEV_INLINE uint64_t radix_peers(uint32_t d, int nbits, bool valid) {
  uint64_t peers = __ballot(valid);
  for (int b = 0; b < nbits; ++b) {
    bool bit = (d >> b) & 1u;
    uint64_t m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}

DEV_INLINE uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    uint32_t t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// exclusive scan of one value per thread over the block's 256 threads;
// *all gets the block total
DEV_INLINE uint32_t select_block_excl_scan(uint32_t v, uint32_t* wsum, int t,
                                           uint32_t* all) {
  const int lane = t % WAVE, wave = t / WAVE;
  uint32_t inc = wave_incl_scan(v, lane);
  if (lane == WAVE - 1) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int w = 0; w < RS_WAVES; ++w) {
    uint32_t x = wsum[w];
    if (w < wave) before += x;
    total += x;
  }
  __syncthreads();
  *all = total;
  return before + inc - v;
}

// The tile's keys for this thread, in no particular order: k[j] is valid
// where bit j of the returned mask is set.  Whole tiles of an aligned column
// go through 16-byte loads (8-byte for one-byte dtypes: a thread owns 8
// keys per tile), the ragged last tile through guarded scalar loads.
template <int WB>
DEV_INLINE uint32_t select_load_tile(const void* __restrict__ src, int kind,
                                     int64_t base, int64_t end, bool aligned,
                                     int t, uint64_t k[RS_KPT]) {
  constexpr int V = WB == 8 ? 2 : WB == 4 ? 4 : 8;  // keys per vector load
  if (aligned && base + RS_TILE <= end) {
#pragma unroll
    for (int v = 0; v < RS_KPT / V; ++v) {
      const char* p = (const char*)src +
                      (base + ((int64_t)v * RS_THREADS + t) * V) * WB;
      if constexpr (V * WB == 16) {
        uint4 raw = *(const uint4*)p;
#pragma unroll
        for (int j = 0; j < V; ++j) k[v * V + j] = radix_norm(&raw, kind, j);
      } else {
        uint2 raw = *(const uint2*)p;
#pragma unroll
        for (int j = 0; j < V; ++j) k[v * V + j] = radix_norm(&raw, kind, j);
      }
    }
    return (1u << RS_KPT) - 1u;
  }
  uint32_t ok = 0;
#pragma unroll
  for (int j = 0; j < RS_KPT; ++j) {
    int64_t i = base + j * RS_THREADS + t;
    bool in = i < end;
    k[j] = in ? radix_norm(src, kind, i) : 0;
    ok |= (uint32_t)in << j;
  }
  return ok;
}

// the kinds a kernel built for WB-byte keys can meet, so that radix_norm's
// switch folds to them
template <int WB>
DEV_INLINE int select_kind(int kind) {
  if (WB == 1) return kind == RK_U8 ? RK_U8 : RK_I8;
  if (WB == 2) return RK_I16;
  if (WB == 4) return kind == RK_F32 ? RK_F32 : RK_I32;
  return kind == RK_F64 ? RK_F64 : RK_I64;
}
