// Stable LSD radix argsort of (u64 key, u32 row id) pairs for gfx950.
//
// One call = one key-normalisation kernel + ceil(bits/8) passes of three
// kernels (count, scan, scatter) over a caller-given bit range of the
// normalised key.  The caller knows how many key bits matter (packed sort
// keys, partition ids), so a 20-bit key costs 3 passes where a generic
// 64-bit sort pays 8.
//
// No kernel waits on another block: the grid of a pass is fixed, block b
// owns one contiguous range of whole tiles in both the count and the
// scatter kernel, and the only cross-block communication is the count
// table between launches.  The price against a single-pass (look-back)
// scatter is a second read of the keys per pass.
//
// Ranking uses no atomics.  A wave handles one item per lane at a time;
// the lanes holding the same digit find each other with one ballot per
// digit bit, rank themselves by popcount of lower peer lanes, and the
// lowest peer advances the wave's private LDS counter with a plain
// read-modify-write.  All-equal and few-valued digits (partition ids,
// the high digits of packed keys) therefore cost the same as random ones.

#include <torch/extension.h>
#include <ATen/ATen.h>

#include <algorithm>

#include "radix.h"

#define RS_SCAN_THREADS 1024

// ---------------------------------------------------------------- keys

// keys[i] = norm(src[perm ? perm[i] : i]), ids[i] = perm ? perm[i] : i.
// A perm entry outside [0, n_src) reads nothing and sorts last.
__global__ __launch_bounds__(RS_THREADS) void radix_keys_kernel(
    const void* __restrict__ src, int kind, int64_t n_src,
    const int64_t* __restrict__ perm, int64_t n,
    uint64_t* __restrict__ keys, uint32_t* __restrict__ ids) {
  GRID_STRIDE_LOOP(i, n) {
    int64_t r = perm ? perm[i] : i;
    bool ok = r >= 0 && r < n_src;
    keys[i] = ok ? radix_norm(src, kind, r) : ~0ULL;
    ids[i] = (uint32_t)r;
  }
}

// ---------------------------------------------------------------- count

// counts[digit * nblocks + block] = number of keys of the block's range
// with that digit.  Wave-private histograms, advanced by the lowest lane
// of each peer group with the group's size.
__global__ __launch_bounds__(RS_THREADS) void radix_count_kernel(
    const uint64_t* __restrict__ keys, int64_t n, int64_t tiles, int shift,
    int nbits, uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[RS_WAVES][RS_BINS];
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint32_t dmask = (1u << nbits) - 1u;
  const uint64_t lt = (1ULL << lane) - 1ULL;
  for (int w = 0; w < RS_WAVES; ++w) hist[w][t] = 0;
  __syncthreads();
  RadixRange r = radix_block_range(n, tiles, gridDim.x, blockIdx.x);
  volatile uint32_t* wh = hist[wave];
  // whole-tile ranges: every thread runs the same number of rounds
  for (int64_t base = r.begin; base < r.end; base += RS_TILE) {
    uint64_t k[RS_KPT];
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      int64_t i = base + j * RS_THREADS + t;
      k[j] = i < r.end ? keys[i] : 0;
    }
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j)
      radix_hist_add(base + j * RS_THREADS + t < r.end, k[j], shift, nbits,
                     dmask, wh, lt);
  }
  __syncthreads();
  uint32_t s = 0;
  for (int w = 0; w < RS_WAVES; ++w) s += hist[w][t];
  counts[(int64_t)t * gridDim.x + blockIdx.x] = s;
}

// ---------------------------------------------------------------- scan

// in-place exclusive scan of the digit-major count table (total is a
// multiple of 4).  One block: 4 entries per thread per round, a wave scan,
// the 16 wave sums through LDS, and a running carry.
__global__ __launch_bounds__(RS_SCAN_THREADS) void radix_scan_kernel(
    uint32_t* __restrict__ counts, int total) {
  __shared__ uint32_t wsum[RS_SCAN_THREADS / WAVE];
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  uint32_t carry = 0;
  for (int base = 0; base < total; base += RS_SCAN_THREADS * 4) {
    int i = base + t * 4;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i < total) v = *(const uint4*)(counts + i);
    uint32_t s = v.x + v.y + v.z + v.w;
    uint32_t inc = wave_incl_scan(s, lane);
    if (lane == WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < RS_SCAN_THREADS / WAVE; ++w) {
      uint32_t x = wsum[w];
      if (w < wave) before += x;
      all += x;
    }
    if (i < total) {
      uint32_t e = carry + before + inc - s;
      uint4 o;
      o.x = e;
      o.y = e + v.x;
      o.z = o.y + v.y;
      o.w = o.z + v.z;
      *(uint4*)(counts + i) = o;
    }
    carry += all;
    __syncthreads();
  }
}

void radix_scan_counts(uint32_t* counts, int total, hipStream_t stream) {
  hipLaunchKernelGGL(radix_scan_kernel, dim3(1), dim3(RS_SCAN_THREADS), 0,
                     stream, counts, total);
}

// ---------------------------------------------------------------- scatter

// Block b walks its tiles in order.  base[d] is where the block's next key
// of digit d goes (from the scanned table, then advanced tile by tile).
// Per tile: rank in the wave (ballots), wave counts -> tile-local digit
// starts, keys and ids to their tile-local sorted slot in LDS, then thread
// t stores slots t, t+256, ... so equal digits leave as contiguous runs.
// out_final != nullptr on the last pass: row ids go out as int64 and the
// keys are not written.
__global__ __launch_bounds__(RS_THREADS) void radix_scatter_kernel(
    const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ ids_in,
    uint64_t* __restrict__ keys_out, uint32_t* __restrict__ ids_out,
    int64_t* __restrict__ out_final, int64_t n, int64_t tiles, int shift,
    int nbits, const uint32_t* __restrict__ offsets) {
  __shared__ uint64_t s_keys[RS_TILE];
  __shared__ uint32_t s_ids[RS_TILE];
  __shared__ uint32_t s_wcnt[RS_WAVES][RS_BINS];
  __shared__ uint32_t s_base[RS_BINS];
  __shared__ uint32_t s_start[RS_BINS];
  __shared__ uint32_t s_wsum[RS_WAVES];
  const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
  const uint32_t dmask = (1u << nbits) - 1u;
  const uint64_t lt = (1ULL << lane) - 1ULL;
  RadixRange r = radix_block_range(n, tiles, gridDim.x, blockIdx.x);
  s_base[t] = offsets[(int64_t)t * gridDim.x + blockIdx.x];
  volatile uint32_t* wc = s_wcnt[wave];
  uint32_t tile_total = 0;  // thread t: keys of digit t in the last tile

  for (int64_t base = r.begin; base < r.end; base += RS_TILE) {
    // (previous tile's stores are behind the barrier that ends the loop)
    s_base[t] += tile_total;
    for (int j = 0; j < RS_BINS / WAVE; ++j) wc[j * WAVE + lane] = 0;

    const int64_t slice = base + (int64_t)wave * (WAVE * RS_KPT);
    uint64_t k[RS_KPT];
    uint32_t id[RS_KPT];
    uint32_t off[RS_KPT];
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      int64_t i = slice + j * WAVE + lane;
      bool valid = i < r.end;
      k[j] = valid ? keys_in[i] : 0;
      id[j] = valid ? ids_in[i] : 0;
    }
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      bool valid = slice + j * WAVE + lane < r.end;
      uint32_t d = radix_digit(k[j], shift, dmask);
      uint64_t peers = radix_peers(d, nbits, valid);
      uint32_t rank = (uint32_t)__popcll(peers & lt);
      uint32_t old = valid ? wc[d] : 0;
      if (valid && rank == 0) wc[d] = old + (uint32_t)__popcll(peers);
      off[j] = old + rank;
    }
    __syncthreads();

    // thread t owns digit t: wave counts -> exclusive wave offsets, block
    // scan of the digit totals -> tile-local digit starts
    uint32_t c[RS_WAVES];
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) {
      c[w] = s_wcnt[w][t];
      total += c[w];
    }
    uint32_t inc = wave_incl_scan(total, lane);
    if (lane == WAVE - 1) s_wsum[wave] = inc;
    __syncthreads();
    uint32_t start = inc - total;
    for (int w = 0; w < wave; ++w) start += s_wsum[w];
    s_start[t] = start;
    uint32_t run = start;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) {
      s_wcnt[w][t] = run;
      run += c[w];
    }
    tile_total = total;
    __syncthreads();

#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      if (slice + j * WAVE + lane < r.end) {
        uint32_t d = radix_digit(k[j], shift, dmask);
        uint32_t pos = s_wcnt[wave][d] + off[j];
        s_keys[pos] = k[j];
        s_ids[pos] = id[j];
      }
    }
    __syncthreads();

    const int tile_n = (int)(r.end - base < RS_TILE ? r.end - base : RS_TILE);
#pragma unroll
    for (int j = 0; j < RS_KPT; ++j) {
      int pos = j * RS_THREADS + t;
      if (pos < tile_n) {
        uint64_t key = s_keys[pos];
        uint32_t d = radix_digit(key, shift, dmask);
        int64_t dst = (int64_t)s_base[d] + (pos - (int)s_start[d]);
        if (dst < n) {  // holds whenever the count table matches the keys
          if (out_final) {
            out_final[dst] = (int64_t)s_ids[pos];
          } else {
            keys_out[dst] = key;
            ids_out[dst] = s_ids[pos];
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- host

int64_t radix_tile() { return RS_TILE; }

torch::Tensor radix_argsort(torch::Tensor keys, int64_t begin_bit,
                            int64_t end_bit,
                            c10::optional<torch::Tensor> perm,
                            int64_t max_blocks) {
  const char* who = "radix_argsort";
  const RadixKeys ka = radix_keys_arg(keys, who);
  end_bit = radix_end_bit(begin_bit, end_bit, ka.width, who);
  radix_check_max_blocks(max_blocks, who);
  int64_t n = ka.n;
  const int64_t* perm_p = nullptr;
  if (perm.has_value()) {
    const torch::Tensor& p = *perm;
    TORCH_CHECK(radix_aux_ok(p, keys),
                "radix_argsort: perm must be a contiguous int64 tensor on "
                "the keys' device");
    n = p.numel();
    perm_p = (const int64_t*)p.data_ptr();
    TORCH_CHECK(n < (1LL << 31), "radix_argsort: 2^31 rows or more");
  }
  auto i64 = torch::dtype(torch::kInt64).device(keys.device());
  auto i32 = torch::dtype(torch::kInt32).device(keys.device());
  auto out = torch::empty({n}, i64);
  if (n == 0) return out;

  hipStream_t stream = current_stream();
  const int64_t tiles = (n + RS_TILE - 1) / RS_TILE;
  const int nblocks = (int)std::min<int64_t>(max_blocks, tiles);
  torch::Tensor kbuf[2] = {torch::empty({n}, i64), torch::empty({n}, i64)};
  torch::Tensor ibuf[2] = {torch::empty({n}, i32), torch::empty({n}, i32)};
  auto counts = torch::empty({(int64_t)RS_BINS * nblocks}, i32);

  hipLaunchKernelGGL(radix_keys_kernel, dim3(grid_for(n, RS_THREADS)),
                     dim3(RS_THREADS), 0, stream, ka.src, ka.kind, ka.n,
                     perm_p, n, (uint64_t*)kbuf[0].data_ptr(),
                     (uint32_t*)ibuf[0].data_ptr());
  CHECK_HIP(hipGetLastError());

  int cur = 0;
  for (int64_t bit = begin_bit; bit < end_bit; bit += 8) {
    const int nbits = (int)std::min<int64_t>(8, end_bit - bit);
    const bool last = bit + 8 >= end_bit;
    hipLaunchKernelGGL(radix_count_kernel, dim3(nblocks), dim3(RS_THREADS), 0,
                       stream, (const uint64_t*)kbuf[cur].data_ptr(), n, tiles,
                       (int)bit, nbits, (uint32_t*)counts.data_ptr());
    radix_scan_counts((uint32_t*)counts.data_ptr(), RS_BINS * nblocks, stream);
    hipLaunchKernelGGL(
        radix_scatter_kernel, dim3(nblocks), dim3(RS_THREADS), 0, stream,
        (const uint64_t*)kbuf[cur].data_ptr(),
        (const uint32_t*)ibuf[cur].data_ptr(),
        (uint64_t*)kbuf[cur ^ 1].data_ptr(),
        (uint32_t*)ibuf[cur ^ 1].data_ptr(),
        last ? (int64_t*)out.data_ptr() : (int64_t*)nullptr, n, tiles,
        (int)bit, nbits, (const uint32_t*)counts.data_ptr());
    CHECK_HIP(hipGetLastError());
    cur ^= 1;
  }
  return out;
}
