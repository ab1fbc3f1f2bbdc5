// Segmented inclusive scan for running and rolling window frames on gfx950.
//
// Each row carries a head flag; the scanned element is (flag, acc, cnt)
// under (f1,a1,c1) + (f2,a2,c2) = (f1|f2, f2 ? a2 : a1 op a2,
// f2 ? c2 : c1 + c2), which is associative, so a row's result depends on
// the rows of its own segment only.
//
// One call = three launches on a fixed grid (reduce, spine, apply).  Block
// b owns one contiguous range of whole tiles in both the reduce and the
// apply kernel; the only cross-block communication is the table of block
// aggregates between launches.  No look-back, no atomics, no block waits
// on another, and the order of combination is a function of n and
// max_blocks alone.
//
// reduce needs only "acc and cnt after the block's last head", so it walks
// its tiles from the last towards the first and stops at the first tile
// that holds a head: with short partitions it reads one tile per block.
//
// A tile is 256 threads x 8 rows.  Rows are loaded coalesced (thread t
// takes rows t, t+256, ...), pass through LDS into a blocked layout
// (thread t holds rows 8t..8t+7; one pad word per 8 keeps the 64-bit LDS
// accesses of a wave on distinct banks), are scanned serially in
// registers, then across the wave in 6 shuffle steps, then across the 4
// waves through LDS; the running carry goes from tile to tile in
// registers.  Results leave through the same LDS buffer, coalesced.
//
// reverse=true scans towards lower row numbers by mirroring the row index
// (logical row l is physical row n-1-l); no data is copied.

#include <torch/extension.h>
#include <ATen/ATen.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "hip_host.h"

#define SS_THREADS 256
#define SS_WAVES (SS_THREADS / WAVE)
#define SS_RPT 8
#define SS_TILE (SS_THREADS * SS_RPT)
#define SS_PAD(i) ((i) + ((i) >> 3))
#define SS_LDS_VALS (SS_TILE + SS_TILE / 8)
#define SS_MAX_BLOCKS 2048

enum SegScanOp : int {
  SS_SUM_F64 = 0, SS_SUM_I64 = 1, SS_MIN_F64 = 2, SS_MAX_F64 = 3,
};

// source dtypes of the values
enum SegKind : int {
  SK_I8 = 0, SK_I16, SK_I32, SK_I64, SK_U8, SK_F32, SK_F64,
};

// row flag bits in LDS
#define SS_HEAD 1u
#define SS_INVALID 2u

template <int OP>
struct SegOp {
  using A = typename std::conditional<OP == SS_SUM_I64, int64_t, double>::type;
  static DEV_INLINE A identity() {
    if constexpr (OP == SS_MIN_F64) return __builtin_huge_val();
    else if constexpr (OP == SS_MAX_F64) return -__builtin_huge_val();
    else return A(0);
  }
  static DEV_INLINE A comb(A a, A b) {
    if constexpr (OP == SS_SUM_I64) return (A)((uint64_t)a + (uint64_t)b);
    else if constexpr (OP == SS_SUM_F64) return a + b;
    else if constexpr (OP == SS_MIN_F64) return b < a ? b : a;
    else return b > a ? b : a;
  }
};

template <typename A>
DEV_INLINE A seg_load(const void* src, int kind, int64_t i) {
  switch (kind) {
    case SK_I8: return (A)((const int8_t*)src)[i];
    case SK_I16: return (A)((const int16_t*)src)[i];
    case SK_I32: return (A)((const int32_t*)src)[i];
    case SK_I64: return (A)((const int64_t*)src)[i];
    case SK_U8: return (A)((const uint8_t*)src)[i];
    case SK_F32: return (A)((const float*)src)[i];
    case SK_F64: return (A)((const double*)src)[i];
  }
  return A(0);
}

DEV_INLINE int seg_shfl_up(int v, int off) { return __shfl_up(v, off); }
DEV_INLINE int64_t seg_shfl_up(int64_t v, int off) {
  int lo = __shfl_up((int)(uint32_t)(uint64_t)v, off);
  int hi = __shfl_up((int)(uint32_t)((uint64_t)v >> 32), off);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
DEV_INLINE double seg_shfl_up(double v, int off) {
  return __longlong_as_double(seg_shfl_up((int64_t)__double_as_longlong(v), off));
}

struct SegArgs {
  const void* values;
  const uint8_t* invalid;  // or nullptr
  const uint8_t* heads;
  int kind;
  int reverse;
  int64_t n;
};

DEV_INLINE int64_t seg_phys(const SegArgs& g, int64_t l) {
  return g.reverse ? g.n - 1 - l : l;
}

// logical row l starts a segment; reversed, that is the physical row whose
// successor is a head, and always row n-1
DEV_INLINE bool seg_is_head(const SegArgs& g, int64_t l) {
  if (l == 0) return true;
  return g.heads[g.reverse ? g.n - l : l] != 0;
}

struct SegRange {
  int64_t begin, end;  // logical rows [begin, end) owned by this block
};

// block b of nblocks owns a contiguous run of whole tiles; the first
// (tiles % nblocks) blocks own one tile more
DEV_INLINE SegRange seg_block_range(int64_t n, int64_t tiles, int nblocks,
                                    int b) {
  int64_t per = tiles / nblocks, rem = tiles % nblocks;
  int64_t t0 = b * per + (b < rem ? b : rem);
  int64_t t1 = t0 + per + (b < rem ? 1 : 0);
  SegRange r;
  r.begin = t0 * SS_TILE;
  r.end = t1 * SS_TILE < n ? t1 * SS_TILE : n;
  return r;
}

struct SegWaveLds {
  uint64_t acc[SS_WAVES];
  int64_t cnt[SS_WAVES];
  int flag[SS_WAVES];
};

// (f, a, c) <- (ef, ea, ec) + (f, a, c): the operand comes earlier
template <int OP, typename C>
DEV_INLINE void seg_prepend(bool ef, typename SegOp<OP>::A ea, C ec, bool& f,
                            typename SegOp<OP>::A& a, C& c) {
  if (!f) {
    a = SegOp<OP>::comb(ea, a);
    c += ec;
  }
  f = f || ef;
}

// Every thread of the block brings one element (f, a, c), in thread order.
// Returns the thread's exclusive prefix (ef, ea, ec) and the block total
// (tf, ta, tc), the same in every thread.  `w` is written before and read
// after the one barrier in here; the caller puts another barrier between
// two calls.
template <int OP, typename C, bool COUNT>
DEV_INLINE void seg_block_exclusive(bool f, typename SegOp<OP>::A a, C c,
                                    SegWaveLds& w, bool& ef,
                                    typename SegOp<OP>::A& ea, C& ec, bool& tf,
                                    typename SegOp<OP>::A& ta, C& tc) {
  using Op = SegOp<OP>;
  using A = typename Op::A;
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    bool f2 = seg_shfl_up((int)f, off) != 0;
    A a2 = seg_shfl_up(a, off);
    C c2 = COUNT ? seg_shfl_up(c, off) : C(0);
    if (lane >= off) seg_prepend<OP, C>(f2, a2, c2, f, a, c);
  }
  if (lane == WAVE - 1) {
    w.acc[wave] = __builtin_bit_cast(uint64_t, a);
    w.cnt[wave] = (int64_t)c;
    w.flag[wave] = f;
  }
  // the lane below, exclusive within the wave
  bool lf = seg_shfl_up((int)f, 1) != 0;
  A la = seg_shfl_up(a, 1);
  C lc = COUNT ? seg_shfl_up(c, 1) : C(0);
  if (lane == 0) {
    lf = false;
    la = Op::identity();
    lc = 0;
  }
  __syncthreads();
  tf = false;
  ta = Op::identity();
  tc = 0;
  ef = false;
  ea = Op::identity();
  ec = 0;
#pragma unroll
  for (int k = 0; k < SS_WAVES; ++k) {
    if (k == wave) {
      ef = tf;
      ea = ta;
      ec = tc;
    }
    bool kf = w.flag[k] != 0;
    A ka = __builtin_bit_cast(A, w.acc[k]);
    C kc = (C)w.cnt[k];
    // total <- total + wave k
    if (kf) {
      ta = ka;
      tc = kc;
    } else {
      ta = Op::comb(ta, ka);
      tc += kc;
    }
    tf = tf || kf;
  }
  // exclusive <- waves before + lanes before
  if (lf) {
    ea = la;
    ec = lc;
  } else {
    ea = Op::comb(ea, la);
    ec += lc;
  }
  ef = ef || lf;
}

// Loads the tile at logical row `base` (rows at or past `end` count as
// invalid, headless rows), leaves each thread its 8 rows' segment-local
// running values in x[] and their flag bytes in fl, and returns the
// thread's exclusive prefix within the tile and the tile total.
template <int OP, bool COUNT>
DEV_INLINE void seg_tile_local(const SegArgs& g, int64_t base, int64_t end,
                               uint64_t* s_val, uint8_t* s_flag, SegWaveLds& w,
                               typename SegOp<OP>::A (&x)[SS_RPT], uint64_t& fl,
                               bool& ef, typename SegOp<OP>::A& ea, int& ec,
                               bool& tf, typename SegOp<OP>::A& ta, int& tc) {
  using Op = SegOp<OP>;
  using A = typename Op::A;
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < SS_RPT; ++j) {
    const int slot = j * SS_THREADS + t;
    const int64_t l = base + slot;
    A v = Op::identity();
    uint32_t bits = SS_INVALID;
    if (l < end) {
      const int64_t p = seg_phys(g, l);
      bool inv = g.invalid != nullptr && g.invalid[p] != 0;
      if (!inv) v = seg_load<A>(g.values, g.kind, p);
      bits = (inv ? SS_INVALID : 0u) | (seg_is_head(g, l) ? SS_HEAD : 0u);
    }
    s_val[SS_PAD(slot)] = __builtin_bit_cast(uint64_t, v);
    s_flag[slot] = (uint8_t)bits;
  }
  __syncthreads();
  fl = *(const uint64_t*)(s_flag + t * SS_RPT);
  bool f = false;
  A run = Op::identity();
  int c = 0;
#pragma unroll
  for (int j = 0; j < SS_RPT; ++j) {
    const uint32_t bits = (uint32_t)(fl >> (8 * j)) & 0xFFu;
    if (bits & SS_HEAD) {
      run = Op::identity();
      c = 0;
      f = true;
    }
    run = Op::comb(run, __builtin_bit_cast(A, s_val[SS_PAD(t * SS_RPT + j)]));
    c += (bits & SS_INVALID) ? 0 : 1;
    x[j] = run;
  }
  seg_block_exclusive<OP, int, COUNT>(f, run, c, w, ef, ea, ec, tf, ta, tc);
}

// ---------------------------------------------------------------- reduce

// agg_*[b] = (a head in the block's range, acc after its last head, cnt
// after its last head)
template <int OP, bool COUNT>
__global__ __launch_bounds__(SS_THREADS) void seg_reduce_kernel(
    SegArgs g, int64_t tiles, int32_t* __restrict__ agg_flag,
    uint64_t* __restrict__ agg_acc, int64_t* __restrict__ agg_cnt) {
  using Op = SegOp<OP>;
  using A = typename Op::A;
  __shared__ uint64_t s_val[SS_LDS_VALS];
  __shared__ __attribute__((aligned(8))) uint8_t s_flag[SS_TILE];
  __shared__ SegWaveLds s_w;
  const SegRange r = seg_block_range(g.n, tiles, gridDim.x, blockIdx.x);
  bool f = false;
  A a = Op::identity();
  int64_t c = 0;
  // the tile total is the same in every thread, so the exit is uniform
  for (int64_t base = r.end - 1 - (r.end - 1 - r.begin) % SS_TILE;
       base >= r.begin && !f; base -= SS_TILE) {
    A x[SS_RPT];
    uint64_t fl;
    bool ef, tf;
    A ea, ta;
    int ec, tc;
    seg_tile_local<OP, COUNT>(g, base, r.end, s_val, s_flag, s_w, x, fl, ef,
                              ea, ec, tf, ta, tc);
    seg_prepend<OP, int64_t>(tf, ta, (int64_t)tc, f, a, c);
  }
  if (threadIdx.x == 0) {
    agg_flag[blockIdx.x] = f;
    agg_acc[blockIdx.x] = __builtin_bit_cast(uint64_t, a);
    agg_cnt[blockIdx.x] = c;
  }
}

// ---------------------------------------------------------------- spine

// pre_*[b] = the carry into block b: the segmented sum of the aggregates of
// blocks 0..b-1.  One block, one aggregate per thread per round.
template <int OP>
__global__ __launch_bounds__(SS_THREADS) void seg_spine_kernel(
    int nblocks, const int32_t* __restrict__ agg_flag,
    const uint64_t* __restrict__ agg_acc, const int64_t* __restrict__ agg_cnt,
    uint64_t* __restrict__ pre_acc, int64_t* __restrict__ pre_cnt) {
  using Op = SegOp<OP>;
  using A = typename Op::A;
  __shared__ SegWaveLds s_w;
  A carry = Op::identity();
  int64_t carry_cnt = 0;
  for (int base = 0; base < nblocks; base += SS_THREADS) {
    const int i = base + threadIdx.x;
    bool f = false;
    A a = Op::identity();
    int64_t c = 0;
    if (i < nblocks) {
      f = agg_flag[i] != 0;
      a = __builtin_bit_cast(A, agg_acc[i]);
      c = agg_cnt[i];
    }
    bool ef, tf;
    A ea, ta;
    int64_t ec, tc;
    seg_block_exclusive<OP, int64_t, true>(f, a, c, s_w, ef, ea, ec, tf, ta,
                                           tc);
    if (i < nblocks) {
      pre_acc[i] = __builtin_bit_cast(uint64_t, ef ? ea : Op::comb(carry, ea));
      pre_cnt[i] = ef ? ec : carry_cnt + ec;
    }
    carry = tf ? ta : Op::comb(carry, ta);
    carry_cnt = tf ? tc : carry_cnt + tc;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- apply

// thread t stores slots t, t+256, ... of the tile from the LDS buffer
DEV_INLINE void seg_store_tile(const SegArgs& g, int64_t base, int64_t end,
                               const uint64_t* s_val,
                               uint64_t* __restrict__ out) {
#pragma unroll
  for (int j = 0; j < SS_RPT; ++j) {
    const int slot = j * SS_THREADS + threadIdx.x;
    const int64_t l = base + slot;
    if (l < end) out[seg_phys(g, l)] = s_val[SS_PAD(slot)];
  }
}

template <int OP, bool COUNT>
__global__ __launch_bounds__(SS_THREADS) void seg_apply_kernel(
    SegArgs g, int64_t tiles, const uint64_t* __restrict__ pre_acc,
    const int64_t* __restrict__ pre_cnt, uint64_t* __restrict__ out_acc,
    int64_t* __restrict__ out_cnt) {
  using Op = SegOp<OP>;
  using A = typename Op::A;
  __shared__ uint64_t s_val[SS_LDS_VALS];
  __shared__ __attribute__((aligned(8))) uint8_t s_flag[SS_TILE];
  __shared__ SegWaveLds s_w;
  const int t = threadIdx.x;
  const SegRange r = seg_block_range(g.n, tiles, gridDim.x, blockIdx.x);
  A carry = __builtin_bit_cast(A, pre_acc[blockIdx.x]);
  int64_t carry_cnt = COUNT ? pre_cnt[blockIdx.x] : 0;
  for (int64_t base = r.begin; base < r.end; base += SS_TILE) {
    A x[SS_RPT];
    uint64_t fl;
    bool ef, tf;
    A ea, ta;
    int ec, tc;
    seg_tile_local<OP, COUNT>(g, base, r.end, s_val, s_flag, s_w, x, fl, ef,
                              ea, ec, tf, ta, tc);
    const A before = ef ? ea : Op::comb(carry, ea);
    // this thread's rows sit in slots only it reads and writes
    bool seen = false;
#pragma unroll
    for (int j = 0; j < SS_RPT; ++j) {
      seen = seen || ((fl >> (8 * j)) & SS_HEAD);
      const A y = seen ? x[j] : Op::comb(before, x[j]);
      s_val[SS_PAD(t * SS_RPT + j)] = __builtin_bit_cast(uint64_t, y);
    }
    __syncthreads();
    seg_store_tile(g, base, r.end, s_val, out_acc);
    if constexpr (COUNT) {
      __syncthreads();
      int64_t c = ef ? (int64_t)ec : carry_cnt + ec;
#pragma unroll
      for (int j = 0; j < SS_RPT; ++j) {
        const uint32_t bits = (uint32_t)(fl >> (8 * j)) & 0xFFu;
        if (bits & SS_HEAD) c = 0;
        c += (bits & SS_INVALID) ? 0 : 1;
        s_val[SS_PAD(t * SS_RPT + j)] = (uint64_t)c;
      }
      __syncthreads();
      seg_store_tile(g, base, r.end, s_val, (uint64_t*)out_cnt);
    }
    carry = tf ? ta : Op::comb(carry, ta);
    carry_cnt = tf ? (int64_t)tc : carry_cnt + tc;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- combine

// Last step of a rolling min/max of width w by van Herk / Gil-Werman.
// Chunks of w rows start at each partition's first row; P is the forward
// and S the reverse scan over the chunks, pc and sc their counts of valid
// rows.  The frame of row i starts at lo = i - min(w-1, row_in_seg[i]);
// it lies in i's chunk, or ends the chunk before it.
__global__ __launch_bounds__(256) void seg_window_combine_kernel(
    const double* __restrict__ P, const double* __restrict__ S,
    const int64_t* __restrict__ pc, const int64_t* __restrict__ sc,
    const int64_t* __restrict__ row_in_seg, int64_t w, int is_max, int64_t n,
    double* __restrict__ out, uint8_t* __restrict__ out_invalid) {
  GRID_STRIDE_LOOP(i, n) {
    const int64_t ris = row_in_seg[i];
    const int64_t back = ris < w - 1 ? ris : w - 1;
    double v = P[i];
    int64_t c = pc[i];
    if (back >= 0 && back <= i && (ris - back) / w != ris / w) {
      const double s = S[i - back];
      v = is_max ? (s > v ? s : v) : (s < v ? s : v);
      c += sc[i - back];
    }
    out[i] = v;
    out_invalid[i] = c == 0;
  }
}

// ---------------------------------------------------------------- host

int64_t seg_scan_tile() { return SS_TILE; }

template <int OP, bool COUNT>
static void seg_scan_launch(const SegArgs& g, int64_t tiles, int nblocks,
                            torch::Tensor& table, uint64_t* out_acc,
                            int64_t* out_cnt, hipStream_t stream) {
  // table rows: agg_acc, agg_cnt, pre_acc, pre_cnt, agg_flag
  int64_t* tp = (int64_t*)table.data_ptr();
  uint64_t* agg_acc = (uint64_t*)tp;
  int64_t* agg_cnt = tp + nblocks;
  uint64_t* pre_acc = (uint64_t*)(tp + 2 * (int64_t)nblocks);
  int64_t* pre_cnt = tp + 3 * (int64_t)nblocks;
  int32_t* agg_flag = (int32_t*)(tp + 4 * (int64_t)nblocks);
  hipLaunchKernelGGL((seg_reduce_kernel<OP, COUNT>), dim3(nblocks),
                     dim3(SS_THREADS), 0, stream, g, tiles, agg_flag, agg_acc,
                     agg_cnt);
  hipLaunchKernelGGL((seg_spine_kernel<OP>), dim3(1), dim3(SS_THREADS), 0,
                     stream, nblocks, (const int32_t*)agg_flag,
                     (const uint64_t*)agg_acc, (const int64_t*)agg_cnt, pre_acc,
                     pre_cnt);
  hipLaunchKernelGGL((seg_apply_kernel<OP, COUNT>), dim3(nblocks),
                     dim3(SS_THREADS), 0, stream, g, tiles,
                     (const uint64_t*)pre_acc, (const int64_t*)pre_cnt, out_acc,
                     out_cnt);
}

std::vector<torch::Tensor> seg_scan(torch::Tensor values,
                                    c10::optional<torch::Tensor> invalid,
                                    torch::Tensor heads, int64_t op,
                                    bool reverse, bool want_count,
                                    int64_t max_blocks) {
  TORCH_CHECK(values.is_cuda() && values.dim() == 1 && values.is_contiguous(),
              "seg_scan: values must be a contiguous 1-d device tensor");
  const int64_t n = values.numel();
  auto flags_ok = [&](const torch::Tensor& x) {
    return x.is_cuda() && x.device() == values.device() && x.dim() == 1 &&
           x.is_contiguous() && x.scalar_type() == torch::kUInt8 &&
           x.numel() == n;
  };
  TORCH_CHECK(flags_ok(heads),
              "seg_scan: heads must be a contiguous uint8 tensor of the "
              "values' length on their device");
  TORCH_CHECK(!invalid.has_value() || flags_ok(*invalid),
              "seg_scan: invalid must be a contiguous uint8 tensor of the "
              "values' length on their device");
  int kind;
  switch (values.scalar_type()) {
    case torch::kInt8: kind = SK_I8; break;
    case torch::kInt16: kind = SK_I16; break;
    case torch::kInt32: kind = SK_I32; break;
    case torch::kInt64: kind = SK_I64; break;
    case torch::kUInt8: kind = SK_U8; break;
    case torch::kFloat32: kind = SK_F32; break;
    case torch::kFloat64: kind = SK_F64; break;
    default:
      TORCH_CHECK(false, "seg_scan: unsupported value dtype ",
                  values.scalar_type());
  }
  TORCH_CHECK(SS_SUM_F64 <= op && op <= SS_MAX_F64, "seg_scan: bad op ", op);
  TORCH_CHECK(op != SS_SUM_I64 || (kind != SK_F32 && kind != SK_F64),
              "seg_scan: SUM_I64 takes integer values");
  TORCH_CHECK(1 <= max_blocks && max_blocks <= SS_MAX_BLOCKS,
              "seg_scan: max_blocks must be in [1, ", SS_MAX_BLOCKS, "]");
  TORCH_CHECK(n < (1LL << 31), "seg_scan: 2^31 rows or more");
  auto i64 = torch::dtype(torch::kInt64).device(values.device());
  std::vector<torch::Tensor> outs;
  outs.push_back(torch::empty(
      {n}, op == SS_SUM_I64 ? i64 : i64.dtype(torch::kFloat64)));
  if (want_count) outs.push_back(torch::empty({n}, i64));
  if (n == 0) return outs;

  hipStream_t stream = current_stream();
  const int64_t tiles = (n + SS_TILE - 1) / SS_TILE;
  const int nblocks = (int)std::min<int64_t>(max_blocks, tiles);
  auto table = torch::empty({5 * (int64_t)nblocks}, i64);
  SegArgs g;
  g.values = values.data_ptr();
  g.invalid = invalid.has_value() ? (const uint8_t*)invalid->data_ptr()
                                  : (const uint8_t*)nullptr;
  g.heads = (const uint8_t*)heads.data_ptr();
  g.kind = kind;
  g.reverse = reverse ? 1 : 0;
  g.n = n;
  uint64_t* out_acc = (uint64_t*)outs[0].data_ptr();
  int64_t* out_cnt = want_count ? (int64_t*)outs[1].data_ptr() : nullptr;
#define SEG_SCAN_CASE(OP)                                                    \
  case OP:                                                                   \
    if (want_count)                                                          \
      seg_scan_launch<OP, true>(g, tiles, nblocks, table, out_acc, out_cnt,  \
                                stream);                                     \
    else                                                                     \
      seg_scan_launch<OP, false>(g, tiles, nblocks, table, out_acc, out_cnt, \
                                 stream);                                    \
    break;
  switch (op) {
    SEG_SCAN_CASE(SS_SUM_F64)
    SEG_SCAN_CASE(SS_SUM_I64)
    SEG_SCAN_CASE(SS_MIN_F64)
    SEG_SCAN_CASE(SS_MAX_F64)
  }
#undef SEG_SCAN_CASE
  check_launch("seg_scan");
  return outs;
}

std::vector<torch::Tensor> seg_window_combine(
    torch::Tensor P, torch::Tensor S, torch::Tensor pc, torch::Tensor sc,
    torch::Tensor row_in_seg, int64_t w, bool is_max) {
  const int64_t n = P.numel();
  auto ok = [&](const torch::Tensor& x, torch::ScalarType st) {
    return x.is_cuda() && x.device() == P.device() && x.dim() == 1 &&
           x.is_contiguous() && x.scalar_type() == st && x.numel() == n;
  };
  TORCH_CHECK(ok(P, torch::kFloat64) && ok(S, torch::kFloat64) &&
                  ok(pc, torch::kInt64) && ok(sc, torch::kInt64) &&
                  ok(row_in_seg, torch::kInt64),
              "seg_window_combine: P, S float64 and pc, sc, row_in_seg int64, "
              "contiguous, of one length, on one device");
  TORCH_CHECK(w >= 1, "seg_window_combine: w must be positive");
  auto out = torch::empty_like(P);
  auto inv = torch::empty({n}, torch::dtype(torch::kUInt8).device(P.device()));
  if (n == 0) return {out, inv};
  hipStream_t stream = current_stream();
  hipLaunchKernelGGL(seg_window_combine_kernel, dim3(grid_for(n, 256)),
                     dim3(256), 0, stream, (const double*)P.data_ptr(),
                     (const double*)S.data_ptr(), (const int64_t*)pc.data_ptr(),
                     (const int64_t*)sc.data_ptr(),
                     (const int64_t*)row_in_seg.data_ptr(), w,
                     is_max ? 1 : 0, n, (double*)out.data_ptr(),
                     (uint8_t*)inv.data_ptr());
  check_launch("seg_window_combine");
  return {out, inv};
}
