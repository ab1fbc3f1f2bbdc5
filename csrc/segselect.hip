// Segmented radix select for gfx950: one order statistic, and the one after
// it, inside every segment of a key column at once.
//
// Segment s is keys[seg_start[s] : seg_start[s + 1]].  Per segment the
// result is lo = the key of rank r = clamp(rank[s], 0, L - 1) in radix_norm's
// order and hi = the key of rank min(r + 1, L - 1), which is what a median or
// an interpolated quantile reads.  Both come back in the source dtype, built
// from the normalised key: a NaN is the canonical quiet NaN, a zero is +0.0.
//
// MSD radix select, one 8-bit digit per pass from the top of the dtype's
// width: histogram the keys that match the digits chosen so far, pick the
// bin that holds the rank, append its digit, lower the rank.  Segments fall
// into three classes by what one wave or one block can hold:
//
//  * wave  (L <= SEG_WAVE_KEYS): one wave owns the segment.  Its keys are
//    loaded once and stay in registers (SEG_KPL per lane); every pass fills
//    the wave's private 256-counter LDS histogram and scans it 4 bins per
//    lane.  Waves grid-stride over the segments; nothing per segment costs a
//    launch or a global atomic.
//  * block (L <= SEG_BLOCK_KEYS): one block owns the segment and stages its
//    normalised keys in LDS once (64 KiB; with the histograms two blocks fit
//    a CU's 160 KiB).
//  * large: per-segment state lives in a slot array indexed by
//    seg_start / (SEG_BLOCK_KEYS + 1), which two large segments cannot
//    share, so it is sized from n alone and nothing is compacted.  Each pass
//    is a histogram launch over the fixed grid of radix_block_range and a
//    spine launch with one wave per slot.  A block finds the segment at the
//    start of its range by binary search and walks forward; a run of its
//    range inside one large segment accumulates in LDS and is flushed to
//    that segment's bins when the run ends, and runs inside small segments
//    are skipped without reading their keys.  A segment whose chosen bin
//    holds a single key is done early; when none is pending the remaining
//    launches return at once.  There is no survivor buffer: every pass
//    re-reads the large segments that are not done.
//
// hi: the passes leave the number of keys below lo and equal to it.  When
// rank + 1 is still inside the equal run, or nothing is above it, hi = lo;
// otherwise hi is the smallest key above lo: a min over the registers or the
// LDS copy, and for large segments one more pass over the keys with a
// wave-reduced 64-bit atomic min (which also finds lo for a segment that
// was done early).
//
// No host synchronisation, fixed grids, no block waits on another.  Segment
// bounds are clamped to [0, n] and ranks to [0, L - 1] on the device, so
// every index is in range whatever the arguments hold.

#include <torch/extension.h>
#include <ATen/ATen.h>

#include <algorithm>
#include <vector>

#include "radix.h"

// keys one lane keeps in registers: 16 u64 are 32 VGPRs
#define SEG_KPL 16
#define SEG_WAVE_KEYS (WAVE * SEG_KPL)
// u64 keys one block stages in LDS
#define SEG_BLOCK_KEYS 8192

struct SegHeader {
  int32_t pending;  // large segments not done
  int32_t nlarge;   // large segments
};

struct SegLarge {
  uint64_t prefix;  // digits chosen so far
  uint64_t lo, hi;  // atomic-min targets of the last pass
  uint32_t rank;    // rank still to find among the prefix's keys
  uint32_t rank0;   // the clamped rank asked for
  uint32_t below;   // keys below the prefix
  uint32_t equal;   // keys with the prefix
  uint32_t len;
  int32_t seg;      // segment + 1; 0: no large segment owns this slot
  int32_t done;
  int32_t shift;    // low key bits the prefix does not cover
  uint32_t bins[RS_BINS];
};

struct SegBounds {
  int64_t b, e;
};

DEV_INLINE SegBounds seg_bounds(const int64_t* __restrict__ seg_start,
                                int64_t s, int64_t n) {
  int64_t b = seg_start[s], e = seg_start[s + 1];
  SegBounds r;
  r.b = b < 0 ? 0 : (b > n ? n : b);
  r.e = e < r.b ? r.b : (e > n ? n : e);
  return r;
}

DEV_INLINE uint32_t seg_rank(const int64_t* __restrict__ rank, int64_t s,
                             int64_t len) {
  int64_t r = rank[s];
  r = r < 0 ? 0 : r;
  return (uint32_t)(r > len - 1 ? len - 1 : r);
}

// the source bits of a normalised key (radix_norm's inverse)
DEV_INLINE uint64_t seg_denorm(uint64_t k, int kind) {
  switch (kind) {
    case RK_I8: return k ^ 0x80u;
    case RK_I16: return k ^ 0x8000u;
    case RK_I32: return k ^ 0x80000000u;
    case RK_I64: return k ^ 0x8000000000000000ULL;
    case RK_U8: return k;
    case RK_F32: {
      uint32_t b = (uint32_t)k;
      if (b == 0xFFFFFFFFu) return 0x7FC00000u;
      return (b & 0x80000000u) ? (b & 0x7FFFFFFFu) : (uint32_t)~b;
    }
    case RK_F64:
      if (k == ~0ULL) return 0x7FF8000000000000ULL;
      return (k & 0x8000000000000000ULL) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
  }
  return 0;
}

template <int WB>
DEV_INLINE void seg_store(void* __restrict__ out, int64_t s, uint64_t key,
                          int kind) {
  const uint64_t raw = seg_denorm(key, kind);
  if (WB == 1) ((uint8_t*)out)[s] = (uint8_t)raw;
  else if (WB == 2) ((uint16_t*)out)[s] = (uint16_t)raw;
  else if (WB == 4) ((uint32_t*)out)[s] = (uint32_t)raw;
  else ((uint64_t*)out)[s] = raw;
}

// whether the key's bits above the current digit are the digits chosen so
// far; `hi` is the digit's upper bit position, 64 only on a first pass
DEV_INLINE bool seg_match(uint64_t key, bool first, int hi, uint64_t prefix) {
  return first || (key >> (hi & 63)) == prefix;
}

// ---------------------------------------------------------------- wave class

template <int WB>
__global__ __launch_bounds__(RS_THREADS) void seg_wave_kernel(
    const void* __restrict__ src, int kind, int64_t n,
    const int64_t* __restrict__ seg_start, const int64_t* __restrict__ rank,
    int64_t nseg, void* __restrict__ lo_out, void* __restrict__ hi_out) {
  __shared__ uint32_t hist[RS_WAVES][RS_BINS];
  kind = select_kind<WB>(kind);
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint64_t lt = (1ULL << lane) - 1ULL;
  volatile uint32_t* wh = hist[wave];
  const int64_t nwaves = (int64_t)gridDim.x * RS_WAVES;
  for (int64_t s = (int64_t)blockIdx.x * RS_WAVES + wave; s < nseg;
       s += nwaves) {
    const SegBounds sb = seg_bounds(seg_start, s, n);
    const int64_t len = sb.e - sb.b;
    if (len <= 0 || len > SEG_WAVE_KEYS) continue;
    uint64_t k[SEG_KPL];
#pragma unroll
    for (int j = 0; j < SEG_KPL; ++j) {
      const int64_t i = sb.b + j * WAVE + lane;
      k[j] = i < sb.e ? radix_norm(src, kind, i) : 0;
    }
    const uint32_t r0 = seg_rank(rank, s, len);
    uint32_t r = r0, below = 0, equal = 0;
    uint64_t prefix = 0;
#pragma unroll
    for (int p = 0; p < WB; ++p) {
      const int shift = 8 * (WB - 1 - p);
#pragma unroll
      for (int q = 0; q < 4; ++q) wh[lane * 4 + q] = 0;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < SEG_KPL; ++j) {
        if (j * WAVE < len) {  // the same for every lane
          const bool in = j * WAVE + lane < len;
          radix_hist_add(in && seg_match(k[j], p == 0, shift + 8, prefix),
                         k[j], shift, 8, RS_BINS - 1, wh, lt);
        }
      }
      __builtin_amdgcn_wave_barrier();
      uint32_t c[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) c[q] = wh[lane * 4 + q];
      const RadixPick pk = radix_wave_pick(c, r, lane);
      prefix = (prefix << 8) | pk.digit;
      r = pk.left;
      below += pk.below;
      equal = pk.count;
    }
    // prefix is lo; the smallest key above it is hi when rank + 1 leaves
    // the run of keys equal to lo
    uint64_t above = ~0ULL;
#pragma unroll
    for (int j = 0; j < SEG_KPL; ++j) {
      const bool in = j * WAVE + lane < len;
      if (in && k[j] > prefix && k[j] < above) above = k[j];
    }
    above = wave_min(above);
    const uint32_t upto = below + equal;
    const uint64_t hi = (r0 + 1 < upto || upto >= (uint32_t)len) ? prefix : above;
    if (lane == 0) {
      seg_store<WB>(lo_out, s, prefix, kind);
      seg_store<WB>(hi_out, s, hi, kind);
    }
  }
}

// --------------------------------------------------------------- block class

template <int WB>
__global__ __launch_bounds__(RS_THREADS) void seg_block_kernel(
    const void* __restrict__ src, int kind, int64_t n,
    const int64_t* __restrict__ seg_start, const int64_t* __restrict__ rank,
    int64_t nseg, void* __restrict__ lo_out, void* __restrict__ hi_out) {
  __shared__ uint64_t sk[SEG_BLOCK_KEYS];
  __shared__ uint32_t hist[RS_WAVES][RS_BINS];
  __shared__ uint32_t wsum[RS_WAVES];
  __shared__ uint64_t wmin[RS_WAVES];
  __shared__ uint32_t pick[3];
  kind = select_kind<WB>(kind);
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint64_t lt = (1ULL << lane) - 1ULL;
  volatile uint32_t* wh = hist[wave];
  for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
    const SegBounds sb = seg_bounds(seg_start, s, n);
    const int64_t len64 = sb.e - sb.b;
    if (len64 <= SEG_WAVE_KEYS || len64 > SEG_BLOCK_KEYS) continue;
    const int len = (int)len64;
    const int rounds = (len + RS_THREADS - 1) / RS_THREADS;
    for (int i = t; i < len; i += RS_THREADS)
      sk[i] = radix_norm(src, kind, sb.b + i);
    const uint32_t r0 = seg_rank(rank, s, len64);
    uint32_t r = r0, below = 0, equal = 0;
    uint64_t prefix = 0;
#pragma unroll 1
    for (int p = 0; p < WB; ++p) {
      const int shift = 8 * (WB - 1 - p);
      for (int w = 0; w < RS_WAVES; ++w) hist[w][t] = 0;
      if (t == 0) pick[0] = pick[1] = pick[2] = 0;
      __syncthreads();
      for (int m = 0; m < rounds; ++m) {
        const int i = m * RS_THREADS + t;
        const bool in = i < len;
        const uint64_t key = in ? sk[i] : 0;
        radix_hist_add(in && seg_match(key, p == 0, shift + 8, prefix), key,
                       shift, 8, RS_BINS - 1, wh, lt);
      }
      __syncthreads();
      uint32_t c = 0;
      for (int w = 0; w < RS_WAVES; ++w) c += hist[w][t];
      uint32_t total;
      const uint32_t excl = select_block_excl_scan(c, wsum, t, &total);
      if (excl <= r && r - excl < c) {  // one thread: bins are disjoint
        pick[0] = (uint32_t)t;
        pick[1] = r - excl;
        pick[2] = excl;
        wsum[0] = c;  // free after the scan's last barrier
      }
      __syncthreads();
      prefix = (prefix << 8) | pick[0];
      r = pick[1];
      below += pick[2];
      equal = wsum[0];
      __syncthreads();
    }
    uint64_t above = ~0ULL;
    for (int i = t; i < len; i += RS_THREADS) {
      const uint64_t key = sk[i];
      if (key > prefix && key < above) above = key;
    }
    above = wave_min(above);
    if (lane == 0) wmin[wave] = above;
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < RS_WAVES; ++w) above = wmin[w] < above ? wmin[w] : above;
      const uint32_t upto = below + equal;
      const uint64_t hi =
          (r0 + 1 < upto || upto >= (uint32_t)len) ? prefix : above;
      seg_store<WB>(lo_out, s, prefix, kind);
      seg_store<WB>(hi_out, s, hi, kind);
    }
    __syncthreads();  // sk and wmin are free for the next segment
  }
}

// --------------------------------------------------------------- large class

DEV_INLINE SegLarge* seg_slot(SegLarge* st, int64_t seg_begin) {
  return st + seg_begin / (SEG_BLOCK_KEYS + 1);
}

__global__ __launch_bounds__(RS_THREADS) void seg_large_init_kernel(
    int64_t n, const int64_t* __restrict__ seg_start,
    const int64_t* __restrict__ rank, int64_t nseg, SegHeader* hdr,
    SegLarge* st) {
  GRID_STRIDE_LOOP(s, nseg) {
    const SegBounds sb = seg_bounds(seg_start, s, n);
    const int64_t len = sb.e - sb.b;
    if (len <= SEG_BLOCK_KEYS) continue;
    SegLarge* g = seg_slot(st, sb.b);
    g->seg = (int32_t)(s + 1);
    g->len = (uint32_t)len;
    g->rank = g->rank0 = seg_rank(rank, s, len);
    g->lo = g->hi = ~0ULL;
    atomicAdd(&hdr->pending, 1);
    atomicAdd(&hdr->nlarge, 1);
  }
}

// the last segment that starts at or before pos (0 when none does)
DEV_INLINE int64_t seg_find(const int64_t* __restrict__ seg_start,
                            int64_t nseg, int64_t pos) {
  int64_t lo = 0, hi = nseg + 1;  // first index whose start is above pos
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (seg_start[mid] <= pos) lo = mid + 1; else hi = mid;
  }
  return lo > 0 ? lo - 1 : 0;
}

// Adds the digit counts of this block's keys to their large segments' bins.
template <int WB>
__global__ __launch_bounds__(RS_THREADS) void seg_large_hist_kernel(
    const void* __restrict__ src, int kind, int64_t n, int64_t tiles,
    const int64_t* __restrict__ seg_start, int64_t nseg, int shift, bool first,
    const SegHeader* hdr, SegLarge* st) {
  __shared__ uint32_t hist[RS_WAVES][RS_BINS];
  if (hdr->pending == 0) return;
  kind = select_kind<WB>(kind);
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint64_t lt = (1ULL << lane) - 1ULL;
  volatile uint32_t* wh = hist[wave];
  const RadixRange r = radix_block_range(n, tiles, gridDim.x, blockIdx.x);
  if (r.begin >= r.end) return;
  for (int w = 0; w < RS_WAVES; ++w) hist[w][t] = 0;
  __syncthreads();
  for (int64_t s = seg_find(seg_start, nseg, r.begin); s < nseg; ++s) {
    const SegBounds sb = seg_bounds(seg_start, s, n);
    if (sb.b >= r.end) break;
    if (sb.e - sb.b <= SEG_BLOCK_KEYS) continue;
    const int64_t a = sb.b > r.begin ? sb.b : r.begin;
    const int64_t z = sb.e < r.end ? sb.e : r.end;
    if (a >= z) continue;
    SegLarge* g = seg_slot(st, sb.b);
    if (g->done) continue;
    const uint64_t prefix = g->prefix;
    const bool aligned = (((uintptr_t)src + (uint64_t)a * WB) & 15) == 0;
    uint64_t k[RS_KPT];
    for (int64_t base = a; base < z; base += RS_TILE) {
      const uint32_t ok = select_load_tile<WB>(src, kind, base, z, aligned, t, k);
#pragma unroll
      for (int j = 0; j < RS_KPT; ++j)
        radix_hist_add(((ok >> j) & 1u) &&
                           seg_match(k[j], first, shift + 8, prefix),
                       k[j], shift, 8, RS_BINS - 1, wh, lt);
    }
    __syncthreads();
    uint32_t c = 0;
    for (int w = 0; w < RS_WAVES; ++w) {  // total and clear in one sweep
      c += hist[w][t];
      hist[w][t] = 0;
    }
    if (c) atomicAdd(&g->bins[t], c);
    __syncthreads();
  }
}

// One wave per slot: pick the digit, clear the bins.
__global__ __launch_bounds__(RS_THREADS) void seg_large_spine_kernel(
    SegHeader* hdr, SegLarge* st, int64_t nslots, int shift) {
  if (hdr->pending == 0) return;
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * RS_WAVES;
  for (int64_t i = (int64_t)blockIdx.x * RS_WAVES + wave; i < nslots;
       i += nwaves) {
    SegLarge* g = st + i;
    if (g->seg == 0 || g->done) continue;
    uint32_t c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c[q] = g->bins[lane * 4 + q];
      g->bins[lane * 4 + q] = 0;
    }
    const RadixPick pk = radix_wave_pick(c, g->rank, lane);
    if (lane == 0) {
      g->prefix = (g->prefix << 8) | pk.digit;
      g->rank = pk.left;
      g->below += pk.below;
      g->equal = pk.count;
      g->shift = shift;
      // a bin of one key: the last pass finds that key by its prefix
      if (shift == 0 || pk.count <= 1) {
        g->done = 1;
        atomicSub(&hdr->pending, 1);
      }
    }
  }
}

// whether hi is a key above lo, which only the last pass can find
DEV_INLINE bool seg_large_needs_hi(const SegLarge* g) {
  const uint32_t upto = g->below + g->equal;
  return g->rank0 + 1 >= upto && upto < g->len;
}

// The last pass: the smallest key with the prefix (lo of a segment that was
// done early) and the smallest key above it, by atomic min per wave.
template <int WB>
__global__ __launch_bounds__(RS_THREADS) void seg_large_last_kernel(
    const void* __restrict__ src, int kind, int64_t n, int64_t tiles,
    const int64_t* __restrict__ seg_start, int64_t nseg, const SegHeader* hdr,
    SegLarge* st) {
  if (hdr->nlarge == 0) return;
  kind = select_kind<WB>(kind);
  const int t = threadIdx.x, lane = t % WAVE;
  const RadixRange r = radix_block_range(n, tiles, gridDim.x, blockIdx.x);
  if (r.begin >= r.end) return;
  for (int64_t s = seg_find(seg_start, nseg, r.begin); s < nseg; ++s) {
    const SegBounds sb = seg_bounds(seg_start, s, n);
    if (sb.b >= r.end) break;
    if (sb.e - sb.b <= SEG_BLOCK_KEYS) continue;
    const int64_t a = sb.b > r.begin ? sb.b : r.begin;
    const int64_t z = sb.e < r.end ? sb.e : r.end;
    if (a >= z) continue;
    SegLarge* g = seg_slot(st, sb.b);
    const int sh = g->shift & 63;
    if (sh == 0 && !seg_large_needs_hi(g)) continue;
    const uint64_t prefix = g->prefix;
    const bool aligned = (((uintptr_t)src + (uint64_t)a * WB) & 15) == 0;
    uint64_t k[RS_KPT], lo = ~0ULL, hi = ~0ULL;
    for (int64_t base = a; base < z; base += RS_TILE) {
      const uint32_t ok = select_load_tile<WB>(src, kind, base, z, aligned, t, k);
#pragma unroll
      for (int j = 0; j < RS_KPT; ++j) {
        const bool in = (ok >> j) & 1u;
        const uint64_t top = k[j] >> sh;
        if (in && top == prefix && k[j] < lo) lo = k[j];
        if (in && top > prefix && k[j] < hi) hi = k[j];
      }
    }
    lo = wave_min(lo);
    hi = wave_min(hi);
    if (lane == 0) {
      if (lo != ~0ULL) atomicMin((unsigned long long*)&g->lo, (unsigned long long)lo);
      if (hi != ~0ULL) atomicMin((unsigned long long*)&g->hi, (unsigned long long)hi);
    }
  }
}

template <int WB>
__global__ __launch_bounds__(RS_THREADS) void seg_large_finish_kernel(
    const SegHeader* hdr, const SegLarge* st, int64_t nslots, int64_t nseg,
    int kind, void* __restrict__ lo_out, void* __restrict__ hi_out) {
  if (hdr->nlarge == 0) return;
  kind = select_kind<WB>(kind);
  GRID_STRIDE_LOOP(i, nslots) {
    const SegLarge* g = st + i;
    const int64_t s = (int64_t)g->seg - 1;
    if (s < 0 || s >= nseg) continue;
    const uint64_t lo = (g->shift & 63) ? g->lo : g->prefix;
    const uint64_t hi = seg_large_needs_hi(g) ? g->hi : lo;
    seg_store<WB>(lo_out, s, lo, kind);
    seg_store<WB>(hi_out, s, hi, kind);
  }
}

// ---------------------------------------------------------------- host

namespace {

struct SegArgs {
  const void* src;
  int kind;
  int64_t n, nseg;
  const int64_t* seg_start;
  const int64_t* rank;
  void* lo;
  void* hi;
  int max_blocks;
  hipStream_t stream;
};

template <int WB>
void seg_launch(const SegArgs& a, SegHeader* hdr, SegLarge* st,
                int64_t nslots) {
  const dim3 block(RS_THREADS);
  const int64_t tiles = (a.n + RS_TILE - 1) / RS_TILE;
  const dim3 tile_grid((int)std::min<int64_t>(a.max_blocks, tiles));
  const dim3 seg_grid(grid_for(a.nseg, RS_THREADS, a.max_blocks));
  const dim3 wave_grid(grid_for(a.nseg, RS_WAVES, a.max_blocks));
  const dim3 blk_grid((int)std::min<int64_t>(a.max_blocks, a.nseg));
  const dim3 slot_grid(grid_for(nslots, RS_WAVES, a.max_blocks));
  hipLaunchKernelGGL(seg_wave_kernel<WB>, wave_grid, block, 0, a.stream, a.src,
                     a.kind, a.n, a.seg_start, a.rank, a.nseg, a.lo, a.hi);
  hipLaunchKernelGGL(seg_block_kernel<WB>, blk_grid, block, 0, a.stream, a.src,
                     a.kind, a.n, a.seg_start, a.rank, a.nseg, a.lo, a.hi);
  hipLaunchKernelGGL(seg_large_init_kernel, seg_grid, block, 0, a.stream, a.n,
                     a.seg_start, a.rank, a.nseg, hdr, st);
  for (int p = 0; p < WB; ++p) {
    const int shift = 8 * (WB - 1 - p);
    hipLaunchKernelGGL(seg_large_hist_kernel<WB>, tile_grid, block, 0, a.stream,
                       a.src, a.kind, a.n, tiles, a.seg_start, a.nseg, shift,
                       p == 0, (const SegHeader*)hdr, st);
    hipLaunchKernelGGL(seg_large_spine_kernel, slot_grid, block, 0, a.stream,
                       hdr, st, nslots, shift);
  }
  hipLaunchKernelGGL(seg_large_last_kernel<WB>, tile_grid, block, 0, a.stream,
                     a.src, a.kind, a.n, tiles, a.seg_start, a.nseg,
                     (const SegHeader*)hdr, st);
  hipLaunchKernelGGL(seg_large_finish_kernel<WB>,
                     dim3(grid_for(nslots, RS_THREADS, a.max_blocks)), block, 0,
                     a.stream, (const SegHeader*)hdr, (const SegLarge*)st,
                     nslots, a.nseg, a.kind, a.lo, a.hi);
  CHECK_HIP(hipGetLastError());
}

}  // namespace

int64_t seg_wave_keys() { return SEG_WAVE_KEYS; }
int64_t seg_block_keys() { return SEG_BLOCK_KEYS; }

// (lo, hi) per segment: the keys of rank r = clamp(rank[s], 0, L - 1) and
// min(r + 1, L - 1) of keys[seg_start[s] : seg_start[s + 1]], in the keys'
// dtype; zero for an empty segment.
std::vector<torch::Tensor> seg_select(torch::Tensor keys,
                                      torch::Tensor seg_start,
                                      torch::Tensor rank, int64_t max_blocks) {
  const char* who = "seg_select";
  const RadixKeys ka = radix_keys_arg(keys, who);
  TORCH_CHECK(radix_aux_ok(seg_start, keys) && radix_aux_ok(rank, keys),
              "seg_select: seg_start and rank must be contiguous int64 "
              "tensors on the keys' device");
  const int64_t nseg = rank.numel();
  TORCH_CHECK(seg_start.numel() == nseg + 1,
              "seg_select: seg_start must have one entry more than rank");
  radix_check_max_blocks(max_blocks, who);
  const int64_t n = ka.n;
  TORCH_CHECK(nseg < (1LL << 31), "seg_select: 2^31 segments or more");

  auto lo = torch::zeros({nseg}, keys.options());
  auto hi = torch::zeros({nseg}, keys.options());
  if (nseg == 0 || n == 0) return {lo, hi};

  auto i64 = torch::dtype(torch::kInt64).device(keys.device());
  static_assert(sizeof(SegLarge) % 8 == 0 && sizeof(SegHeader) == 8,
                "the states are whole int64 tensors");
  const int64_t nslots = n / (SEG_BLOCK_KEYS + 1) + 1;
  auto header = torch::zeros({1}, i64);
  auto state = torch::zeros({nslots * (int64_t)(sizeof(SegLarge) / 8)}, i64);

  SegArgs a;
  a.src = ka.src;
  a.kind = ka.kind;
  a.n = n;
  a.nseg = nseg;
  a.seg_start = (const int64_t*)seg_start.data_ptr();
  a.rank = (const int64_t*)rank.data_ptr();
  a.lo = lo.data_ptr();
  a.hi = hi.data_ptr();
  a.max_blocks = (int)max_blocks;
  a.stream = current_stream();
  SegHeader* hdr = (SegHeader*)header.data_ptr();
  SegLarge* st = (SegLarge*)state.data_ptr();
  RADIX_DISPATCH_BYTES(ka.width, seg_launch, a, hdr, st, nslots);
  return {lo, hi};
}
