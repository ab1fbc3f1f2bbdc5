// Radix select for gfx950: the row ids of the k smallest keys, in row order,
// without ordering the other n - k rows.
//
// Keys are bits [begin_bit, end_bit) of the order-preserving u64 form of the
// source column (radix.h), computed on the fly from the column itself.
//
// 1. Threshold.  One pass per 8-bit digit, most significant first: a
//    histogram launch over the keys that still match the digits chosen so
//    far, then a one-block spine that scans the 256 bins, picks the bin
//    holding rank k, appends its digit to the prefix and lowers the rank.
//    The first pass whose chosen bin fits the survivor buffer arms it: the
//    next histogram launch appends every matching key to the buffer (one
//    atomic add per wave per tile), and the passes after that read the
//    buffer instead of the column.  With no such bin (an all-equal key),
//    every pass reads the column through the prefix filter.  The passes end
//    early when the chosen bin holds exactly the keys still needed.
// 2. Emission.  With the threshold T known: per-block counts of rows below
//    and equal to T, a one-block scan of them, and a scatter over the same
//    block ranges that writes int64 row ids ascending: every row below T,
//    and the first `m` rows equal to T.
//
// The grid is fixed, block b owns a contiguous run of whole tiles, no block
// waits on another, and everything the launches tell each other is in one
// SelectState in device memory; the host reads nothing back unless the
// caller wants every tie (ties="all"), whose count it cannot know.
//
// Histograms use the sort's wave-private LDS counters and ballot grouping,
// so all-equal and few-valued digits cost what random ones do.

#include <torch/extension.h>
#include <ATen/ATen.h>

#include <algorithm>

#include "radix.h"

enum SurvivorState : int { SV_NONE = 0, SV_FILL = 1, SV_VALID = 2 };

struct SelectState {
  uint64_t prefix;     // digits chosen so far (the key's top bits)
  uint64_t thresh;     // prefix, then ones: the k-th key once done
  uint32_t rank;       // 0-based rank still to find among the prefix's keys
  uint32_t count_lt;   // keys below the prefix
  uint32_t bin_count;  // keys with the prefix
  uint32_t surv_n;     // cursor of the survivor buffer
  int32_t surv;        // SurvivorState
  int32_t done;        // thresh is final; later passes return at once
  int32_t bits_done;
  uint32_t total_lt, total_eq;  // rows below / equal to thresh
  uint32_t take_eq;    // rows equal to thresh that are emitted (the first)
  uint32_t out_count;  // total_lt + take_eq
  uint32_t pad;
  uint32_t hist[RS_BINS];
};

// survivor buffer capacity.  A random digit leaves n/256 keys in the chosen
// bin; n/8 takes bins 32 times heavier than that, costs n bytes (no more
// than an int8 key column) and bounds a buffer pass at the bytes of one pass
// over an int64 column's eighth.  A bin above it means the digit barely
// narrowed the keys, and the next digit gets its chance.
int64_t select_capacity(int64_t n) {
  return std::max<int64_t>(n / 8, 1024);
}

// ---------------------------------------------------------------- loading

DEV_INLINE uint64_t select_key(uint64_t norm, int begin_bit, uint64_t wmask) {
  return (norm >> begin_bit) & wmask;
}

// ---------------------------------------------------------------- histogram

// One tile's keys into the wave-private histogram; with `fill`, the matching
// keys also go to the survivor buffer behind one atomic add per wave.
DEV_INLINE void select_hist_tile(const uint64_t k[RS_KPT], uint32_t ok,
                                 bool filter, int hi, uint64_t prefix,
                                 int shift, int nbits, uint32_t dmask,
                                 uint64_t lt, volatile uint32_t* wh, bool fill,
                                 uint64_t* __restrict__ buf, int64_t cap,
                                 SelectState* st, int lane) {
  uint64_t m[RS_KPT];
  uint32_t total = 0;
#pragma unroll
  for (int j = 0; j < RS_KPT; ++j) {
    bool valid = (ok >> j) & 1u;
    if (filter) valid = valid && (k[j] >> hi) == prefix;
    radix_hist_add(valid, k[j], shift, nbits, dmask, wh, lt);
    m[j] = __ballot(valid);
    total += (uint32_t)__popcll(m[j]);
  }
  if (fill && total) {
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(&st->surv_n, total);
    at = __shfl(at, 0);
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      int64_t dst = (int64_t)at + __popcll(m[j] & lt);
      // holds whenever the spine's bin count matches the keys
      if (((m[j] >> lane) & 1ULL) && dst < cap) buf[dst] = k[j];
      at += (uint32_t)__popcll(m[j]);
    }
  }
}

// Adds to st->hist the digit counts (bits [shift, shift + nbits) of the key)
// of the keys whose bits above the digit equal st->prefix; the first pass
// takes every key.  Reads the column, or the survivor buffer once valid.
template <int WB>
__global__ __launch_bounds__(RS_THREADS) void select_hist_kernel(
    const void* __restrict__ src, int kind, int64_t n, int64_t tiles,
    bool aligned, int begin_bit, uint64_t wmask, int shift, int nbits,
    bool first, uint64_t* __restrict__ buf, int64_t cap, SelectState* st) {
  __shared__ uint32_t hist[RS_WAVES][RS_BINS];
  if (!first && st->done) return;
  kind = select_kind<WB>(kind);
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint32_t dmask = (1u << nbits) - 1u;
  const uint64_t lt = (1ULL << lane) - 1ULL;
  const int mode = first ? SV_NONE : st->surv;
  const uint64_t prefix = first ? 0 : st->prefix;
  const int hi = (shift + nbits) & 63;  // below 64 on every pass but the first
  for (int w = 0; w < RS_WAVES; ++w) hist[w][t] = 0;
  __syncthreads();
  volatile uint32_t* wh = hist[wave];
  uint64_t k[RS_KPT];
  if (mode == SV_VALID) {
    int64_t nb = st->surv_n;
    nb = nb < cap ? nb : cap;
    RadixRange r = radix_block_range(nb, (nb + RS_TILE - 1) / RS_TILE,
                                     gridDim.x, blockIdx.x);
    for (int64_t base = r.begin; base < r.end; base += RS_TILE) {
      uint32_t ok = 0;
#pragma unroll
      for (int j = 0; j < RS_KPT; ++j) {
        int64_t i = base + j * RS_THREADS + t;
        bool in = i < r.end;
        k[j] = in ? buf[i] : 0;
        ok |= (uint32_t)in << j;
      }
      select_hist_tile(k, ok, true, hi, prefix, shift, nbits, dmask, lt, wh,
                       false, buf, cap, st, lane);
    }
  } else {
    RadixRange r = radix_block_range(n, tiles, gridDim.x, blockIdx.x);
    for (int64_t base = r.begin; base < r.end; base += RS_TILE) {
      uint32_t ok = select_load_tile<WB>(src, kind, base, r.end, aligned, t, k);
#pragma unroll
      for (int j = 0; j < RS_KPT; ++j) k[j] = select_key(k[j], begin_bit, wmask);
      select_hist_tile(k, ok, !first, hi, prefix, shift, nbits, dmask, lt, wh,
                       mode == SV_FILL, buf, cap, st, lane);
    }
  }
  __syncthreads();
  uint32_t s = 0;
  for (int w = 0; w < RS_WAVES; ++w) s += hist[w][t];
  if (s) atomicAdd(&st->hist[t], s);
}

// One block after every histogram: pick the bin that holds the rank, extend
// the prefix, decide what the next pass reads, clear the histogram.
__global__ __launch_bounds__(RS_THREADS) void select_spine_kernel(
    SelectState* st, int64_t k, int shift, int nbits, bool first, bool last,
    int64_t cap) {
  __shared__ uint32_t wsum[RS_WAVES];
  if (!first && st->done) return;
  const int t = threadIdx.x;
  const uint32_t c = st->hist[t];
  const uint32_t rank = first ? (uint32_t)(k - 1) : st->rank;
  const uint64_t prefix = first ? 0 : st->prefix;
  const uint32_t count_lt = first ? 0 : st->count_lt;
  const int surv = first ? SV_NONE : st->surv;
  uint32_t total;
  const uint32_t excl = select_block_excl_scan(c, wsum, t, &total);
  st->hist[t] = 0;
  if (excl <= rank && rank - excl < c) {  // one thread: bins are disjoint
    const uint64_t p = (prefix << nbits) | (uint64_t)t;
    const uint32_t left = rank - excl;
    st->prefix = p;
    st->rank = left;
    st->count_lt = count_lt + excl;
    st->bin_count = c;
    st->bits_done += nbits;
    st->thresh = (p << shift) | ((1ULL << shift) - 1ULL);
    // every key of the bin is needed: all of them are at or below thresh
    const bool done = last || c == left + 1;
    st->done = done;
    if (surv == SV_FILL) {
      st->surv = SV_VALID;
    } else if (surv == SV_NONE && !done && (int64_t)c <= cap) {
      st->surv = SV_FILL;
      st->surv_n = 0;
    }
  }
}

// ---------------------------------------------------------------- emission

// cnt_lt[b], cnt_eq[b] = rows of block b's range below / equal to thresh
template <int WB>
__global__ __launch_bounds__(RS_THREADS) void select_count_kernel(
    const void* __restrict__ src, int kind, int64_t n, int64_t tiles,
    bool aligned, int begin_bit, uint64_t wmask, const SelectState* st,
    uint32_t* __restrict__ cnt_lt, uint32_t* __restrict__ cnt_eq) {
  __shared__ uint32_t s_lt[RS_WAVES], s_eq[RS_WAVES];
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint64_t T = st->thresh;
  kind = select_kind<WB>(kind);
  RadixRange r = radix_block_range(n, tiles, gridDim.x, blockIdx.x);
  uint32_t lt = 0, eq = 0;
  uint64_t k[RS_KPT];
  for (int64_t base = r.begin; base < r.end; base += RS_TILE) {
    uint32_t ok = select_load_tile<WB>(src, kind, base, r.end, aligned, t, k);
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      uint64_t key = select_key(k[j], begin_bit, wmask);
      bool in = (ok >> j) & 1u;
      lt += in && key < T;
      eq += in && key == T;
    }
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    lt += __shfl_down(lt, off);
    eq += __shfl_down(eq, off);
  }
  if (lane == 0) {
    s_lt[wave] = lt;
    s_eq[wave] = eq;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t a = 0, b = 0;
    for (int w = 0; w < RS_WAVES; ++w) {
      a += s_lt[w];
      b += s_eq[w];
    }
    cnt_lt[blockIdx.x] = a;
    cnt_eq[blockIdx.x] = b;
  }
}

// One block: exclusive scans of the per-block counts (thread t owns blocks
// 8t .. 8t+7), the totals, and how many ties are emitted.
__global__ __launch_bounds__(RS_THREADS) void select_emit_spine_kernel(
    SelectState* st, int64_t k, bool ties_all, int nblocks,
    const uint32_t* __restrict__ cnt_lt, const uint32_t* __restrict__ cnt_eq,
    uint32_t* __restrict__ base_lt, uint32_t* __restrict__ base_eq) {
  __shared__ uint32_t wsum[RS_WAVES];
  constexpr int PER = RS_MAX_BLOCKS / RS_THREADS;
  const int t = threadIdx.x;
  uint32_t a[PER], b[PER], sa = 0, sb = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    int i = t * PER + j;
    a[j] = i < nblocks ? cnt_lt[i] : 0;
    b[j] = i < nblocks ? cnt_eq[i] : 0;
    sa += a[j];
    sb += b[j];
  }
  uint32_t total_lt, total_eq;
  uint32_t ea = select_block_excl_scan(sa, wsum, t, &total_lt);
  uint32_t eb = select_block_excl_scan(sb, wsum, t, &total_eq);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    int i = t * PER + j;
    if (i < nblocks) {
      base_lt[i] = ea;
      base_eq[i] = eb;
    }
    ea += a[j];
    eb += b[j];
  }
  if (t == 0) {
    uint32_t take = total_eq;
    if (!ties_all) {
      int64_t want = k - (int64_t)total_lt;
      want = want < 0 ? 0 : want;
      take = want < (int64_t)total_eq ? (uint32_t)want : total_eq;
    }
    st->total_lt = total_lt;
    st->total_eq = total_eq;
    st->take_eq = take;
    st->out_count = total_lt + take;
  }
}

// Block b walks its tiles in order and writes the ids of its emitted rows at
// (rows below thresh before the row) + min(ties before the row, take_eq).
// A wave owns 512 consecutive rows of the tile, lane l rows l, l + 64, ...,
// so one ballot per round ranks a row among the wave's.
__global__ __launch_bounds__(RS_THREADS) void select_scatter_kernel(
    const void* __restrict__ src, int kind, int64_t n, int64_t tiles,
    int begin_bit, uint64_t wmask, const SelectState* st,
    const uint32_t* __restrict__ cnt_lt, const uint32_t* __restrict__ cnt_eq,
    const uint32_t* __restrict__ base_lt, const uint32_t* __restrict__ base_eq,
    int64_t* __restrict__ out, int64_t out_n) {
  __shared__ uint32_t s_lt[RS_WAVES], s_eq[RS_WAVES];
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint64_t ltm = (1ULL << lane) - 1ULL;
  const uint64_t T = st->thresh;
  const uint32_t take = st->take_eq;
  uint32_t run_lt = base_lt[blockIdx.x], run_eq = base_eq[blockIdx.x];
  // nothing of this block's range is emitted
  if (cnt_lt[blockIdx.x] == 0 && (cnt_eq[blockIdx.x] == 0 || run_eq >= take))
    return;
  RadixRange r = radix_block_range(n, tiles, gridDim.x, blockIdx.x);
  for (int64_t base = r.begin; base < r.end; base += RS_TILE) {
    const int64_t slice = base + (int64_t)wave * (WAVE * RS_KPT);
    uint64_t mlt[RS_KPT], meq[RS_KPT];
    uint32_t wl = 0, we = 0;
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      int64_t i = slice + j * WAVE + lane;
      bool in = i < r.end;
      uint64_t key =
          in ? select_key(radix_norm(src, kind, i), begin_bit, wmask) : 0;
      mlt[j] = __ballot(in && key < T);
      meq[j] = __ballot(in && key == T);
      wl += (uint32_t)__popcll(mlt[j]);
      we += (uint32_t)__popcll(meq[j]);
    }
    if (lane == 0) {
      s_lt[wave] = wl;
      s_eq[wave] = we;
    }
    __syncthreads();
    uint32_t lt_before = run_lt, eq_before = run_eq;
    for (int w = 0; w < RS_WAVES; ++w) {
      uint32_t a = s_lt[w], b = s_eq[w];
      if (w < wave) {
        lt_before += a;
        eq_before += b;
      }
      run_lt += a;
      run_eq += b;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      bool is_lt = (mlt[j] >> lane) & 1ULL, is_eq = (meq[j] >> lane) & 1ULL;
      uint32_t l = lt_before + (uint32_t)__popcll(mlt[j] & ltm);
      uint32_t e = eq_before + (uint32_t)__popcll(meq[j] & ltm);
      int64_t pos = (int64_t)l + (e < take ? e : take);
      if ((is_lt || (is_eq && e < take)) && pos < out_n)
        out[pos] = slice + j * WAVE + lane;
      lt_before += (uint32_t)__popcll(mlt[j]);
      eq_before += (uint32_t)__popcll(meq[j]);
    }
  }
}

// ---------------------------------------------------------------- host

namespace {

struct SelectArgs {
  const void* src;
  int kind;
  int64_t n, tiles;
  bool aligned;
  int begin_bit;
  uint64_t wmask;
  int nblocks;
  hipStream_t stream;
};

template <int WB>
void select_launch(const SelectArgs& a, int64_t k, int width, bool ties_all,
                   uint64_t* buf, int64_t cap, SelectState* st,
                   uint32_t* blk) {
  const dim3 grid(a.nblocks), block(RS_THREADS);
  const int passes = (width + 7) / 8;
  for (int p = 0; p < passes; ++p) {
    // the top digit takes what is left over from whole 8-bit digits below
    const int shift = 8 * (passes - 1 - p);
    const int nbits = p == 0 ? width - shift : 8;
    hipLaunchKernelGGL(select_hist_kernel<WB>, grid, block, 0, a.stream, a.src,
                       a.kind, a.n, a.tiles, a.aligned, a.begin_bit, a.wmask,
                       shift, nbits, p == 0, buf, cap, st);
    hipLaunchKernelGGL(select_spine_kernel, dim3(1), block, 0, a.stream, st, k,
                       shift, nbits, p == 0, p == passes - 1, cap);
  }
  hipLaunchKernelGGL(select_count_kernel<WB>, grid, block, 0, a.stream, a.src,
                     a.kind, a.n, a.tiles, a.aligned, a.begin_bit, a.wmask,
                     (const SelectState*)st, blk, blk + a.nblocks);
  hipLaunchKernelGGL(select_emit_spine_kernel, dim3(1), block, 0, a.stream, st,
                     k, ties_all, a.nblocks, (const uint32_t*)blk,
                     (const uint32_t*)(blk + a.nblocks), blk + 2 * a.nblocks,
                     blk + 3 * a.nblocks);
  CHECK_HIP(hipGetLastError());
}

}  // namespace

// Row ids, ascending, of the k smallest keys (1 <= k < n) over bits
// [begin_bit, end_bit) of the normalised key.  ties_all false: exactly k
// ids, ties with the k-th key taken in row order.  ties_all true: every row
// at or below the k-th key, or nothing when they are more than max_out.
c10::optional<torch::Tensor> radix_select(torch::Tensor keys, int64_t k,
                                          int64_t begin_bit, int64_t end_bit,
                                          bool ties_all, int64_t max_out,
                                          int64_t max_blocks) {
  const char* who = "radix_select";
  const RadixKeys ka = radix_keys_arg(keys, who);
  end_bit = radix_end_bit(begin_bit, end_bit, ka.width, who);
  radix_check_max_blocks(max_blocks, who);
  const int64_t n = ka.n;
  TORCH_CHECK(1 <= k && k < n, "radix_select: k must be in [1, n)");
  if (max_out < 0) max_out = n;

  auto i64 = torch::dtype(torch::kInt64).device(keys.device());
  auto i32 = torch::dtype(torch::kInt32).device(keys.device());
  SelectArgs a;
  a.src = ka.src;
  a.kind = ka.kind;
  a.n = n;
  a.tiles = (n + RS_TILE - 1) / RS_TILE;
  a.aligned = ((uintptr_t)a.src & 15) == 0;
  a.begin_bit = (int)begin_bit;
  const int sel_width = (int)(end_bit - begin_bit);
  a.wmask = sel_width == 64 ? ~0ULL : (1ULL << sel_width) - 1ULL;
  a.nblocks = (int)std::min<int64_t>(max_blocks, a.tiles);
  a.stream = current_stream();

  const int64_t cap = select_capacity(n);
  static_assert(sizeof(SelectState) % 8 == 0, "state is a whole int64 tensor");
  auto state = torch::zeros({(int64_t)(sizeof(SelectState) / 8)}, i64);
  auto buf = torch::empty({cap}, i64);
  auto blk = torch::empty({4 * (int64_t)a.nblocks}, i32);
  SelectState* st = (SelectState*)state.data_ptr();
  uint64_t* bufp = (uint64_t*)buf.data_ptr();
  uint32_t* blkp = (uint32_t*)blk.data_ptr();
  RADIX_DISPATCH_BYTES(ka.width, select_launch, a, k, sel_width, ties_all, bufp,
                       cap, st, blkp);

  int64_t out_n = k;
  if (ties_all) {
    // the one read-back: how many rows tie with the k-th key is data
    auto counts = state.view(torch::kInt32)
                      .slice(0, offsetof(SelectState, out_count) / 4,
                             offsetof(SelectState, out_count) / 4 + 1)
                      .cpu();
    out_n = (int64_t)(uint32_t)counts.item<int32_t>();
    if (out_n > max_out) return c10::nullopt;
  }
  auto out = torch::empty({out_n}, i64);
  hipLaunchKernelGGL(select_scatter_kernel, dim3(a.nblocks), dim3(RS_THREADS),
                     0, a.stream, a.src, a.kind, a.n, a.tiles, a.begin_bit,
                     a.wmask, (const SelectState*)st, (const uint32_t*)blkp,
                     (const uint32_t*)(blkp + a.nblocks),
                     (const uint32_t*)(blkp + 2 * a.nblocks),
                     (const uint32_t*)(blkp + 3 * a.nblocks),
                     (int64_t*)out.data_ptr(), out_n);
  CHECK_HIP(hipGetLastError());
  return out;
}
