// What the radix sort (sort.hip) and the radix selects (select.hip,
// segselect.hip) share: the order-preserving u64 form of every sortable
// dtype, ballot-based digit grouping and histograms, the fixed-grid split of
// n keys into per-block tile ranges, wave reductions, the selects' tile load,
// block scan and wave-level rank pick, and the hosts' argument checks.
#pragma once

#include <torch/extension.h>

#include "common.h"
#include "hip_host.h"

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

// One key into the wave-private histogram wh, by its nbits-bit digit at
// `shift` (dmask is (1 << nbits) - 1, which the caller keeps out of its
// loop): the lowest lane of each peer group (lt masks the lanes below the
// caller) adds the group's size.  Every lane of the wave must call it.
DEV_INLINE void radix_hist_add(bool valid, uint64_t key, int shift, int nbits,
                               uint32_t dmask, volatile uint32_t* wh,
                               uint64_t lt) {
  const uint32_t d = radix_digit(key, shift, dmask);
  const uint64_t peers = radix_peers(d, nbits, valid);
  if (valid && (peers & lt) == 0) wh[d] = wh[d] + (uint32_t)__popcll(peers);
}

DEV_INLINE uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    uint32_t t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// the wave's minimum, in every lane
DEV_INLINE uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    uint64_t o = __shfl_xor((unsigned long long)v, off);
    v = o < v ? o : v;
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

// the bin that holds a rank, the rank inside it, the keys in the bins before
// it and the keys in it
struct RadixPick {
  uint32_t digit, left, below, count;
};

// One wave, lane l holding bins 4l .. 4l+3; every lane gets the pick.
DEV_INLINE RadixPick radix_wave_pick(const uint32_t c[4], uint32_t rank,
                                     int lane) {
  uint32_t sum = c[0] + c[1] + c[2] + c[3];
  uint32_t excl = wave_incl_scan(sum, lane) - sum;
  RadixPick p = {0, 0, 0, 0};
  bool hit = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (!hit && excl <= rank && rank - excl < c[q]) {
      hit = true;
      p = {(uint32_t)lane * 4 + q, rank - excl, excl, c[q]};
    }
    excl += c[q];
  }
  const uint64_t m = __ballot(hit);
  const int src = m ? __ffsll((unsigned long long)m) - 1 : 0;
  p.digit = __shfl(p.digit, src);
  p.left = __shfl(p.left, src);
  p.below = __shfl(p.below, src);
  p.count = __shfl(p.count, src);
  return p;
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

// ---------------------------------------------------------------- host
// (`who` is the entry point's name and opens every message)
struct RadixKeys {
  const void* src;
  int kind;   // RadixKind
  int width;  // bits of the dtype
  int64_t n;
};

inline RadixKeys radix_keys_arg(const torch::Tensor& keys, const char* who) {
  TORCH_CHECK(keys.is_cuda() && keys.dim() == 1 && keys.is_contiguous(), who,
              ": keys must be a contiguous 1-d device tensor");
  RadixKeys k = {keys.data_ptr(), 0, 0, keys.numel()};
  switch (keys.scalar_type()) {
    case torch::kInt8: k.kind = RK_I8; k.width = 8; break;
    case torch::kInt16: k.kind = RK_I16; k.width = 16; break;
    case torch::kInt32: k.kind = RK_I32; k.width = 32; break;
    case torch::kInt64: k.kind = RK_I64; k.width = 64; break;
    case torch::kUInt8: k.kind = RK_U8; k.width = 8; break;
    case torch::kFloat32: k.kind = RK_F32; k.width = 32; break;
    case torch::kFloat64: k.kind = RK_F64; k.width = 64; break;
    default:
      TORCH_CHECK(false, who, ": unsupported key dtype ", keys.scalar_type());
  }
  TORCH_CHECK(k.n < (1LL << 31), who, ": 2^31 rows or more");
  return k;
}

// In-place exclusive scan of a digit-major count table on one block
// (sort.hip).  total is a multiple of 4 and the table is 16-byte aligned.
void radix_scan_counts(uint32_t* counts, int total, hipStream_t stream);

inline void radix_check_max_blocks(int64_t max_blocks, const char* who) {
  TORCH_CHECK(1 <= max_blocks && max_blocks <= RS_MAX_BLOCKS, who,
              ": max_blocks must be in [1, ", RS_MAX_BLOCKS, "]");
}

// the end of the bit range [begin_bit, end_bit); end_bit < 0 is the width
inline int64_t radix_end_bit(int64_t begin_bit, int64_t end_bit, int width,
                             const char* who) {
  if (end_bit < 0) end_bit = width;
  TORCH_CHECK(0 <= begin_bit && begin_bit < end_bit && end_bit <= 64, who,
              ": bad bit range [", begin_bit, ", ", end_bit, ")");
  return end_bit;
}

// whether x is a contiguous 1-d int64 tensor on the keys' device
inline bool radix_aux_ok(const torch::Tensor& x, const torch::Tensor& keys) {
  return x.is_cuda() && x.device() == keys.device() && x.dim() == 1 &&
         x.is_contiguous() && x.scalar_type() == torch::kInt64;
}

// FN<key bytes>(...) for keys of `width` bits
#define RADIX_DISPATCH_BYTES(width, FN, ...) \
  switch ((width) / 8) {                     \
    case 1: FN<1>(__VA_ARGS__); break;       \
    case 2: FN<2>(__VA_ARGS__); break;       \
    case 4: FN<4>(__VA_ARGS__); break;       \
    default: FN<8>(__VA_ARGS__); break;      \
  }
