// LIKE-style pattern matching on plain (offsets + bytes) string columns for
// gfx950.
//
// A pattern is m literal byte segments in order, separated by '%' (any run
// of bytes, the empty one and line feeds included), 1 <= m <= 8 and at most
// 256 pattern bytes.  anchor_start pins the first segment to the row's first
// byte, anchor_end pins the last segment to the row's last byte.  Segments
// must not overlap, so each segment is searched from the end of the match
// before it, and taking the leftmost hit every time decides the pattern:
// any other choice only leaves less room for the segments that follow.  An
// anchored segment is the same search over a range of one position.
//
// A tile is 256 consecutive rows, one block of 256 threads, tiles
// grid-strided.  The bytes of a tile are contiguous in the column.
//
//  * Tile bytes <= SM_STAGE: the block copies them HBM -> LDS once, with
//    16-byte loads from the address rounded down to 16 (vectors that are not
//    wholly inside the buffer are loaded byte by byte, so nothing outside
//    the buffer is read), together with the tile's 257 offsets as 32-bit
//    positions in the stage.  Thread t then scans row t out of LDS: aligned
//    32-bit reads, a SWAR test for the segment's first byte, and a byte
//    compare of the rest at each candidate.
//  * Tile bytes > SM_STAGE (long rows): the block's four waves take the
//    tile's rows in turn; the 64 lanes test 64 consecutive candidate
//    positions straight from global memory and a ballot picks the leftmost
//    hit.  A row of any length is served, with no length check on the host.
//
// The pattern travels in the kernel arguments and is copied to LDS at block
// start, since the compare indexes it per lane.  One byte store per row.

#include <torch/extension.h>
#include <ATen/ATen.h>

#include <algorithm>
#include <cstring>

#include "common.h"
#include "hip_host.h"

#define SM_THREADS 256
#define SM_WAVES (SM_THREADS / WAVE)
#define SM_TILE SM_THREADS
#define SM_STAGE 32768
// a misaligned head of up to 15 bytes and a tail rounded up to 16
#define SM_STAGE_ALLOC (SM_STAGE + 32)
#define SM_MAX_SEGS 8
#define SM_MAX_PAT 256
#define SM_MAX_BLOCKS 2048

struct StrMatchArgs {
  const uint8_t* bytes;
  const int64_t* offsets;
  const uint8_t* mask;
  uint8_t* out;
  int64_t n;
  int64_t nbytes;
  int32_t m;
  int32_t anchor_start;
  int32_t anchor_end;
  int32_t seg[SM_MAX_SEGS + 1];    // segment j is pat[seg[j], seg[j + 1])
  uint32_t pat[SM_MAX_PAT / 4];
};

// Leftmost p in [lo, hi] with row[p, p + len) == pat[0, len), or -1.  `row`
// is the LDS stage, 4-byte aligned; words past hi are in the stage, and a
// candidate past hi is dropped.
DEV_INLINE int lds_find(const uint8_t* stage, int lo, int hi,
                        const uint8_t* pat, int len) {
  const uint32_t* words = (const uint32_t*)stage;
  const uint32_t first = pat[0] * 0x01010101u;
  int p = lo;
  while (p <= hi) {
    uint32_t x = words[p >> 2] ^ first;
    // 0x80 in every byte of x that is zero.  A zero byte below may flag a
    // byte of value 1 through the borrow, so a flag is a candidate only and
    // the compare starts at the first byte.
    uint32_t z = (x - 0x01010101u) & ~x & 0x80808080u;
    z &= 0xFFFFFFFFu << ((p & 3) * 8);
    if (z == 0) {
      p = (p | 3) + 1;
      continue;
    }
    p = (p & ~3) + ((__ffs(z) - 1) >> 3);
    if (p > hi) break;
    int k = 0;
    while (k < len && stage[p + k] == pat[k]) ++k;
    if (k == len) return p;
    ++p;
  }
  return -1;
}

// The same over global memory by one wave: lane l tests position base + l.
DEV_INLINE int64_t wave_find(const uint8_t* bytes, int64_t lo, int64_t hi,
                             const uint8_t* pat, int len, int lane) {
  for (int64_t base = lo; base <= hi; base += WAVE) {
    int64_t p = base + lane;
    bool hit = false;
    if (p <= hi && bytes[p] == pat[0]) {
      int k = 1;
      while (k < len && bytes[p + k] == pat[k]) ++k;
      hit = k == len;
    }
    uint64_t b = __ballot(hit);
    if (b) return base + (__ffsll((unsigned long long)b) - 1);
  }
  return -1;
}

// Candidate range of segment j in the row [s, e) after a match ending at
// cur: [cur, e - len], cut to one position by an anchor.
#define SM_RANGE(T)                                                  \
  T lo = cur, hi = e - len;                                          \
  if (j == 0 && anchor_start) hi = hi < s ? hi : s;                  \
  if (j == m - 1 && anchor_end) lo = lo > e - len ? lo : e - len;

__global__ void __launch_bounds__(SM_THREADS)
string_match_kernel(const StrMatchArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[SM_STAGE_ALLOC];
  __shared__ int32_t s_off[SM_TILE + 1];
  __shared__ __attribute__((aligned(4))) uint8_t s_pat[SM_MAX_PAT];
  __shared__ int32_t s_seg[SM_MAX_SEGS + 1];

  const int t = threadIdx.x;
  const int lane = t & (WAVE - 1);
  const int wave = t / WAVE;
  if (t < SM_MAX_PAT / 4) ((uint32_t*)s_pat)[t] = a.pat[t];
  if (t <= SM_MAX_SEGS) s_seg[t] = a.seg[t];
  const int m = a.m;
  const bool anchor_start = a.anchor_start != 0;
  const bool anchor_end = a.anchor_end != 0;
  const uintptr_t buf_lo = (uintptr_t)a.bytes;
  const uintptr_t buf_hi = buf_lo + (uint64_t)a.nbytes;
  const int64_t tiles = (a.n + SM_TILE - 1) / SM_TILE;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * SM_TILE;
    const int rows = (int)(a.n - r0 < SM_TILE ? a.n - r0 : SM_TILE);
    // the row's bytes lie inside the buffer whatever the offsets say
    int64_t b0 = a.offsets[r0], b1 = a.offsets[r0 + rows];
    b0 = b0 < 0 ? 0 : (b0 > a.nbytes ? a.nbytes : b0);
    b1 = b1 < b0 ? b0 : (b1 > a.nbytes ? a.nbytes : b1);
    __syncthreads();  // pattern staged; previous tile's scans done

    if (b1 - b0 <= SM_STAGE) {
      const int tile_bytes = (int)(b1 - b0);
      const uintptr_t src0 = (buf_lo + (uint64_t)b0) & ~(uintptr_t)15;
      const int lead = (int)(buf_lo + (uint64_t)b0 - src0);
      const int nvec = (lead + tile_bytes + 15) >> 4;
      for (int v = t; v < nvec; v += SM_THREADS) {
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
        ((uint4*)s_stage)[v] = q;
      }
      for (int i = t; i <= rows; i += SM_THREADS) {
        int64_t o = a.offsets[r0 + i];
        o = o < b0 ? b0 : (o > b1 ? b1 : o);
        s_off[i] = (int)(o - b0) + lead;
      }
      __syncthreads();
      if (t < rows) {
        bool ok = a.mask == nullptr || a.mask[r0 + t] != 0;
        const int s = s_off[t];
        const int e = s_off[t + 1] < s ? s : s_off[t + 1];
        int cur = s;
        for (int j = 0; ok && j < m; ++j) {
          const int len = s_seg[j + 1] - s_seg[j];
          SM_RANGE(int)
          const int p =
              lo <= hi ? lds_find(s_stage, lo, hi, s_pat + s_seg[j], len) : -1;
          ok = p >= 0;
          cur = p + len;
        }
        a.out[r0 + t] = ok ? 1 : 0;
      }
    } else {
      for (int i = wave; i < rows; i += SM_WAVES) {
        const int64_t r = r0 + i;
        bool ok = a.mask == nullptr || a.mask[r] != 0;
        int64_t s = a.offsets[r], e = a.offsets[r + 1];
        s = s < b0 ? b0 : (s > b1 ? b1 : s);
        e = e < s ? s : (e > b1 ? b1 : e);
        int64_t cur = s;
        for (int j = 0; ok && j < m; ++j) {
          const int len = s_seg[j + 1] - s_seg[j];
          SM_RANGE(int64_t)
          const int64_t p =
              lo <= hi ? wave_find(a.bytes, lo, hi, s_pat + s_seg[j], len, lane)
                       : -1;
          ok = p >= 0;
          cur = p + len;
        }
        if (lane == 0) a.out[r] = ok ? 1 : 0;
      }
    }
  }
}

#undef SM_RANGE

// ---------------------------------------------------------------- host

int64_t strmatch_lds_bytes() { return SM_STAGE; }

torch::Tensor string_match(torch::Tensor bytes, torch::Tensor offsets,
                           c10::optional<torch::Tensor> mask,
                           torch::Tensor segs, torch::Tensor seg_ends,
                           bool anchor_start, bool anchor_end,
                           int64_t max_blocks) {
  auto dev1d = [&](const torch::Tensor& x, torch::ScalarType st) {
    return x.is_cuda() && x.device() == offsets.device() && x.dim() == 1 &&
           x.is_contiguous() && x.scalar_type() == st;
  };
  TORCH_CHECK(offsets.is_cuda() && dev1d(offsets, torch::kInt64) &&
                  offsets.numel() >= 1,
              "string_match: offsets must be a contiguous int64 device tensor "
              "of n + 1 entries");
  TORCH_CHECK(dev1d(bytes, torch::kUInt8),
              "string_match: bytes must be a contiguous uint8 tensor on the "
              "offsets' device");
  const int64_t n = offsets.numel() - 1;
  TORCH_CHECK(!mask.has_value() ||
                  (dev1d(*mask, torch::kUInt8) && mask->numel() == n),
              "string_match: mask must be a contiguous uint8 tensor of n "
              "entries on the offsets' device");
  auto host1d = [](const torch::Tensor& x, torch::ScalarType st) {
    return x.is_cpu() && x.dim() == 1 && x.is_contiguous() &&
           x.scalar_type() == st;
  };
  TORCH_CHECK(host1d(segs, torch::kUInt8) && host1d(seg_ends, torch::kInt32),
              "string_match: segs (uint8) and seg_ends (int32) are host "
              "tensors; the pattern travels in the kernel arguments");
  const int64_t m = seg_ends.numel();
  TORCH_CHECK(1 <= m && m <= SM_MAX_SEGS, "string_match: 1 to ", SM_MAX_SEGS,
              " segments, got ", m);
  TORCH_CHECK(segs.numel() <= SM_MAX_PAT, "string_match: at most ", SM_MAX_PAT,
              " pattern bytes, got ", segs.numel());
  TORCH_CHECK(1 <= max_blocks && max_blocks <= SM_MAX_BLOCKS,
              "string_match: max_blocks must be in [1, ", SM_MAX_BLOCKS, "]");

  StrMatchArgs a;
  std::memset(&a, 0, sizeof(a));
  const int32_t* ends = seg_ends.data_ptr<int32_t>();
  for (int64_t j = 0; j < m; ++j) {
    TORCH_CHECK(ends[j] > a.seg[j], "string_match: empty segment ", j);
    a.seg[j + 1] = ends[j];
  }
  TORCH_CHECK(a.seg[m] == segs.numel(),
              "string_match: seg_ends must end at the length of segs");
  std::memcpy(a.pat, segs.data_ptr<uint8_t>(), (size_t)segs.numel());

  auto out = torch::empty(
      {n}, torch::dtype(torch::kUInt8).device(offsets.device()));
  if (n == 0) return out;
  a.bytes = bytes.data_ptr<uint8_t>();
  a.offsets = offsets.data_ptr<int64_t>();
  a.mask = mask.has_value() ? mask->data_ptr<uint8_t>() : nullptr;
  a.out = out.data_ptr<uint8_t>();
  a.n = n;
  a.nbytes = bytes.numel();
  a.m = (int32_t)m;
  a.anchor_start = anchor_start ? 1 : 0;
  a.anchor_end = anchor_end ? 1 : 0;

  const int64_t tiles = (n + SM_TILE - 1) / SM_TILE;
  const int nblocks = (int)std::min<int64_t>(max_blocks, tiles);
  hipStream_t stream = current_stream();
  hipLaunchKernelGGL(string_match_kernel, dim3(nblocks), dim3(SM_THREADS), 0,
                     stream, a);
  check_launch("string_match");
  return out;
}
