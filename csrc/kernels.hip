// bodo_amd gfx950 kernels: row hashing, datetime extraction, string gather,
// hash groupby (open addressing + atomics), hash join (bucket chains).
//
// Design notes (MI355X/CDNA4):
//  * memory-bound table kernels: 256-thread blocks (4 waves), grid capped at
//    2048 blocks with grid-stride loops (guide Guideline 11)
//  * hash tables live in HBM (groups/build sides up to hundreds of GB fit in
//    288 GB); LDS pre-aggregation fast path for low-cardinality groupbys is
//    in groupby_lds.hip
//  * all hashes bit-match the host path (ops/__init__.py) so CPU ranks and
//    GPU ranks can share shuffles
//
// Reference behavioral spec (no code reuse): bodo/libs/_array_hash.cpp,
// bodo/libs/streaming/_groupby.cpp, _join.cpp, _datetime_ext.cpp.

#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <cstring>
#include <vector>

#include "common.h"

#define CHECK_HIP(x)                                                    \
  do {                                                                  \
    hipError_t e = (x);                                                 \
    TORCH_CHECK(e == hipSuccess, "HIP error: ", hipGetErrorString(e));  \
  } while (0)

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// ---------------------------------------------------------------------
// ColumnDesc marshalling
// ---------------------------------------------------------------------

struct DescSet {
  torch::Tensor dev_buf;  // device copy of ColumnDesc[]
  std::vector<ColumnDesc> host;
  ColumnDesc* ptr() { return (ColumnDesc*)dev_buf.data_ptr(); }
};

static ColumnDesc make_desc(const torch::Tensor& data,
                            const c10::optional<torch::Tensor>& mask,
                            const c10::optional<torch::Tensor>& offsets,
                            const c10::optional<torch::Tensor>& aux,
                            int64_t dtype, int64_t n) {
  ColumnDesc d;
  d.data = data.numel() ? data.data_ptr() : nullptr;
  d.offsets = offsets.has_value() ? (const int64_t*)offsets->data_ptr() : nullptr;
  d.mask = mask.has_value() ? (const uint8_t*)mask->data_ptr() : nullptr;
  d.aux = aux.has_value() ? (const uint64_t*)aux->data_ptr() : nullptr;
  d.dtype = (int)dtype;
  d.n = n;
  return d;
}

static DescSet upload_descs(const std::vector<ColumnDesc>& descs,
                            const torch::Device& dev) {
  DescSet s;
  s.host = descs;
  auto cpu = torch::from_blob((void*)s.host.data(),
                              {(int64_t)(descs.size() * sizeof(ColumnDesc))},
                              torch::kUInt8);
  s.dev_buf = cpu.to(dev, /*non_blocking=*/false);
  return s;
}

static DescSet build_descset(
    const std::vector<torch::Tensor>& datas,
    const std::vector<c10::optional<torch::Tensor>>& masks,
    const std::vector<c10::optional<torch::Tensor>>& offsets,
    const std::vector<c10::optional<torch::Tensor>>& auxs,
    const std::vector<int64_t>& dtypes, int64_t n) {
  std::vector<ColumnDesc> descs;
  for (size_t i = 0; i < datas.size(); ++i) {
    descs.push_back(make_desc(datas[i], masks[i], offsets[i], auxs[i],
                              dtypes[i], n));
  }
  return upload_descs(descs, datas[0].device());
}

// ---------------------------------------------------------------------
// row hashing
// ---------------------------------------------------------------------

__global__ void hash_columns_kernel(const ColumnDesc* __restrict__ cols,
                                    int ncols, uint64_t seed,
                                    uint64_t* __restrict__ out, int64_t n) {
  GRID_STRIDE_LOOP(i, n) {
    uint64_t acc = 0;
    for (int c = 0; c < ncols; ++c) {
      uint64_t h = is_valid_at(cols[c], i) ? hash_value(cols[c], i) : NULL_HASH;
      if (seed) h = mix64(h ^ seed);
      acc = (c == 0) ? h : mix64(acc * GOLDEN + h);
    }
    out[i] = acc;
  }
}

torch::Tensor hash_columns(
    std::vector<torch::Tensor> datas,
    std::vector<c10::optional<torch::Tensor>> masks,
    std::vector<c10::optional<torch::Tensor>> offsets,
    std::vector<c10::optional<torch::Tensor>> auxs,
    std::vector<int64_t> dtypes, int64_t n, int64_t seed) {
  auto dev = datas[0].device();
  auto ds = build_descset(datas, masks, offsets, auxs, dtypes, n);
  auto out = torch::empty({n}, torch::dtype(torch::kInt64).device(dev));
  int block = 256;
  hipLaunchKernelGGL(hash_columns_kernel, dim3(grid_for(n, block)),
                     dim3(block), 0, cur_stream(), ds.ptr(),
                     (int)datas.size(), (uint64_t)seed,
                     (uint64_t*)out.data_ptr(), n);
  CHECK_HIP(hipGetLastError());
  return out;
}

// ---------------------------------------------------------------------
// datetime extraction (Howard Hinnant civil-from-days algorithm)
// ---------------------------------------------------------------------

DEV_INLINE int64_t floordiv(int64_t a, int64_t b) {
  int64_t q = a / b;
  return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

DEV_INLINE void civil_from_days(int64_t z, int& y, unsigned& m, unsigned& d) {
  z += 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const unsigned doe = (unsigned)(z - era * 146097);
  const unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const int64_t y_ = (int64_t)yoe + era * 400;
  const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const unsigned mp = (5 * doy + 2) / 153;
  d = doy - (153 * mp + 2) / 5 + 1;
  m = mp < 10 ? mp + 3 : mp - 9;
  y = (int)(y_ + (m <= 2));
}

enum DtField : int {
  DT_YEAR = 0, DT_MONTH = 1, DT_DAY = 2, DT_HOUR = 3, DT_MINUTE = 4,
  DT_SECOND = 5, DT_DAYOFWEEK = 6, DT_DAYOFYEAR = 7, DT_QUARTER = 8,
  DT_DATE = 9, DT_NORMALIZE = 10,
};

#define NS_PER_DAY 86400000000000LL

template <typename OUT>
__global__ void dt_field_kernel(const int64_t* __restrict__ ts, int is_date32,
                                const int32_t* __restrict__ ts32, int field,
                                OUT* __restrict__ out, int64_t n) {
  GRID_STRIDE_LOOP(i, n) {
    int64_t days, ns_in_day;
    if (is_date32) {
      days = ts32[i];
      ns_in_day = 0;
    } else {
      int64_t v = ts[i];
      days = floordiv(v, NS_PER_DAY);
      ns_in_day = v - days * NS_PER_DAY;
    }
    OUT r = 0;
    switch (field) {
      case DT_DATE: r = (OUT)days; break;
      case DT_NORMALIZE: r = (OUT)(days * NS_PER_DAY); break;
      case DT_HOUR: r = (OUT)(ns_in_day / 3600000000000LL); break;
      case DT_MINUTE: r = (OUT)((ns_in_day / 60000000000LL) % 60); break;
      case DT_SECOND: r = (OUT)((ns_in_day / 1000000000LL) % 60); break;
      case DT_DAYOFWEEK: {
        // 1970-01-01 is a Thursday = 3 (Mon=0)
        int64_t dow = (days + 3) % 7;
        if (dow < 0) dow += 7;
        r = (OUT)dow;
        break;
      }
      default: {
        int y; unsigned m, d;
        civil_from_days(days, y, m, d);
        if (field == DT_YEAR) r = (OUT)y;
        else if (field == DT_MONTH) r = (OUT)m;
        else if (field == DT_DAY) r = (OUT)d;
        else if (field == DT_QUARTER) r = (OUT)((m - 1) / 3 + 1);
        else if (field == DT_DAYOFYEAR) {
          // days since Jan 1 of year y
          int64_t jan1 = days;
          // compute days-from-civil(y,1,1)
          int64_t yy = y;
          yy -= 1 <= 2;
          const int64_t era = (yy >= 0 ? yy : yy - 399) / 400;
          const unsigned yoe = (unsigned)(yy - era * 400);
          const unsigned doy0 = (153 * (1 + 9) + 2) / 5 + 1 - 1;
          const unsigned doe = yoe * 365 + yoe / 4 - yoe / 100 + doy0;
          jan1 = era * 146097 + (int64_t)doe - 719468;
          r = (OUT)(days - jan1 + 1);
        }
      }
    }
    out[i] = r;
  }
}

torch::Tensor dt_field(torch::Tensor data, int64_t is_date32, int64_t field,
                       int64_t out_kind) {
  int64_t n = data.numel();
  auto dev = data.device();
  torch::Tensor out;
  int block = 256;
  auto grid = dim3(grid_for(n, block));
  const int64_t* ts = is_date32 ? nullptr : (const int64_t*)data.data_ptr();
  const int32_t* ts32 = is_date32 ? (const int32_t*)data.data_ptr() : nullptr;
  if (out_kind == 0) {  // int16
    out = torch::empty({n}, torch::dtype(torch::kInt16).device(dev));
    hipLaunchKernelGGL(dt_field_kernel<int16_t>, grid, dim3(block), 0,
                       cur_stream(), ts, (int)is_date32, ts32, (int)field,
                       (int16_t*)out.data_ptr(), n);
  } else if (out_kind == 1) {  // int32
    out = torch::empty({n}, torch::dtype(torch::kInt32).device(dev));
    hipLaunchKernelGGL(dt_field_kernel<int32_t>, grid, dim3(block), 0,
                       cur_stream(), ts, (int)is_date32, ts32, (int)field,
                       (int32_t*)out.data_ptr(), n);
  } else {  // int64
    out = torch::empty({n}, torch::dtype(torch::kInt64).device(dev));
    hipLaunchKernelGGL(dt_field_kernel<int64_t>, grid, dim3(block), 0,
                       cur_stream(), ts, (int)is_date32, ts32, (int)field,
                       (int64_t*)out.data_ptr(), n);
  }
  CHECK_HIP(hipGetLastError());
  return out;
}

// ---------------------------------------------------------------------
// string gather: one wave per row, 8-byte chunks
// ---------------------------------------------------------------------

__global__ void string_gather_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off,
    const int64_t* __restrict__ idx, const int64_t* __restrict__ dst_off,
    uint8_t* __restrict__ dst, int64_t n_rows) {
  // one wave (64 lanes) per row; lanes copy bytes cooperatively
  int64_t row = blockIdx.x * (int64_t)(blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  int64_t stride = (int64_t)gridDim.x * (blockDim.x / WAVE);
  for (; row < n_rows; row += stride) {
    int64_t s = src_off[idx[row]];
    int64_t len = src_off[idx[row] + 1] - s;
    int64_t d = dst_off[row];
    for (int64_t k = lane; k < len; k += WAVE) {
      dst[d + k] = src[s + k];
    }
  }
}

std::vector<torch::Tensor> gather_string(torch::Tensor bytes,
                                         torch::Tensor offsets,
                                         torch::Tensor idx) {
  int64_t n = idx.numel();
  auto dev = bytes.device();
  auto starts = offsets.index({idx});
  auto lens = offsets.index({idx + 1}) - starts;
  auto new_off = torch::zeros({n + 1}, torch::dtype(torch::kInt64).device(dev));
  auto off_tail = new_off.slice(0, 1, n + 1);
  at::cumsum_out(off_tail, lens, 0);
  int64_t total = n ? new_off[n].item<int64_t>() : 0;
  auto out = torch::empty({total}, torch::dtype(torch::kUInt8).device(dev));
  if (n && total) {
    int block = 256;
    int waves_per_block = block / WAVE;
    int grid = (int)std::min<int64_t>((n + waves_per_block - 1) / waves_per_block, 2048);
    hipLaunchKernelGGL(string_gather_kernel, dim3(grid), dim3(block), 0,
                       cur_stream(), (const uint8_t*)bytes.data_ptr(),
                       (const int64_t*)offsets.data_ptr(),
                       (const int64_t*)idx.data_ptr(),
                       (const int64_t*)new_off.data_ptr(),
                       (uint8_t*)out.data_ptr(), n);
    CHECK_HIP(hipGetLastError());
  }
  return {out, new_off};
}

// ---------------------------------------------------------------------
// hash groupby: open-addressing table in HBM (reference semantics:
// streaming/_groupby.cpp HashGroupbyTable)
// ---------------------------------------------------------------------

__global__ void gb_insert_kernel(const ColumnDesc* __restrict__ cols, int ncols,
                                 const uint64_t* __restrict__ hashes,
                                 uint32_t* __restrict__ slots, uint64_t cap_mask,
                                 uint32_t* __restrict__ row_slot, int64_t n,
                                 int64_t row0, const uint64_t* __restrict__ all_hashes) {
  // rows [row0, row0+n) of the table; hashes/row_slot pre-offset by caller,
  // all_hashes/cols indexed globally (slots store global row+1)
  GRID_STRIDE_LOOP(i, n) {
    uint64_t h = hashes[i];
    int64_t gi = row0 + i;
    uint64_t s = h & cap_mask;
    while (true) {
      uint32_t old = atomicCAS(&slots[s], 0u, (uint32_t)(gi + 1));
      if (old == 0u) {  // we claimed the slot: new group
        row_slot[i] = (uint32_t)s;
        break;
      }
      int64_t cand = (int64_t)old - 1;
      if (all_hashes[cand] == h && rows_eq(cols, ncols, cand, gi)) {
        row_slot[i] = (uint32_t)s;
        break;
      }
      s = (s + 1) & cap_mask;
    }
  }
}

// Host-side sizing shared by both group builds.  The open-addressing insert
// kernels probe until they find their key or an empty slot, so the host must
// never launch an insert that could fill the table.
#define GB_CHUNK_ROWS (int64_t(1) << 27)
#define GB_MAX_INITIAL_CAP (int64_t(1) << 26)
#define GB_PACKED_MAX_INITIAL_CAP (int64_t(1) << 25)

static void check_build_limits(int64_t chunk_rows, int64_t max_initial_cap) {
  TORCH_CHECK(chunk_rows >= 1, "chunk_rows must be positive");
  TORCH_CHECK(max_initial_cap >= 16 &&
                  (max_initial_cap & (max_initial_cap - 1)) == 0,
              "max_initial_cap must be a power of two >= 16");
}

// Rows per insert launch.  With cap >= 2n the whole input fits below half
// load and chunk_rows is used as is.  Otherwise each launch is clamped to
// cap/2 - 1 rows and the load factor is checked after it: a launch starts
// with occupied <= cap/2 (else the check before it would have grown the
// table) and adds at most cap/2 - 1 entries, so occupied <= cap - 1.
static int64_t insert_step(int64_t chunk_rows, int64_t cap, int64_t n) {
  if (cap >= 2 * n) return chunk_rows;
  return std::min(chunk_rows, cap / 2 - 1);
}

// Capacity after the load factor crossed 1/2 with `occupied` slots in use:
// grow 8x (more if the groups seen so far suggest it), never past the
// smallest power of two >= 2n, at which no further check is needed.
static int64_t grown_cap(int64_t cap, int64_t occupied, int64_t n) {
  int64_t want = cap * 8;
  while (want < 2 * std::min(n, occupied * 8)) want <<= 1;
  if (want > 2 * n) {
    int64_t c2 = 16;
    while (c2 < 2 * n) c2 <<= 1;
    want = c2;
  }
  return want;
}

// Packed-key fast path: keys pre-packed into one u64 (< 2^63), slots hold
// the KEY itself (CAS, sentinel ~0) so probing never dereferences candidate
// rows or a hash array; the slot hash is computed in-kernel.
#define PACKED_EMPTY 0xFFFFFFFFFFFFFFFFULL

__global__ void gb_insert_packed_kernel(const int64_t* __restrict__ keys,
                                        unsigned long long* __restrict__ slot_keys,
                                        uint32_t* __restrict__ slot_rows,
                                        uint64_t cap_mask,
                                        uint32_t* __restrict__ row_slot,
                                        int64_t n, int64_t row0) {
  // rows [row0, row0+n) of the table; keys/row_slot pre-offset by caller,
  // slot_rows stores the global row+1
  GRID_STRIDE_LOOP(i, n) {
    unsigned long long key = (unsigned long long)keys[i];
    uint64_t s = mix64(key) & cap_mask;
    while (true) {
      unsigned long long old = slot_keys[s];
      if (old == key) {
        row_slot[i] = (uint32_t)s;
        break;
      }
      if (old == PACKED_EMPTY) {
        old = atomicCAS(&slot_keys[s], PACKED_EMPTY, key);
        if (old == PACKED_EMPTY) {
          slot_rows[s] = (uint32_t)(row0 + i + 1);
          row_slot[i] = (uint32_t)s;
          break;
        }
        if (old == key) {
          row_slot[i] = (uint32_t)s;
          break;
        }
      }
      s = (s + 1) & cap_mask;
    }
  }
}

// What the passes after the insert need to know about a table: whether slot
// s holds a group, and the first row of that group.
struct GenericSlots {  // gb_insert_kernel: slot = row + 1, 0 = empty
  const uint32_t* slots;
  DEV_INLINE bool occupied(int64_t s) const { return slots[s] != 0u; }
  DEV_INLINE int64_t row(int64_t s) const { return (int64_t)slots[s] - 1; }
};

struct PackedSlots {  // gb_insert_packed_kernel: key slots + row + 1 beside
  const unsigned long long* slot_keys;
  const uint32_t* slot_rows;
  DEV_INLINE bool occupied(int64_t s) const {
    return slot_keys[s] != PACKED_EMPTY;
  }
  DEV_INLINE int64_t row(int64_t s) const { return (int64_t)slot_rows[s] - 1; }
};

// two-pass group-id assignment: pass 1 counts occupied slots per block
// (no atomics), host cumsums 2048 values, pass 2 assigns gids via an LDS
// counter (one global atomic total: zero).  Replaces a single-global-counter
// atomicAdd that measured 43% of NYC-taxi Q1 step time at 300M rows.
template <typename Slots>
__global__ void gb_count_kernel(const Slots table, int64_t chunk, int64_t cap,
                                int64_t* __restrict__ block_counts) {
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t stop = min(start + chunk, cap);
  int64_t local = 0;
  for (int64_t s = start + threadIdx.x; s < stop; s += blockDim.x) {
    local += table.occupied(s);
  }
  __shared__ int64_t red[256];
  red[threadIdx.x] = local;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) block_counts[blockIdx.x] = red[0];
}

template <typename Slots>
__global__ void gb_assign_gid_kernel(const Slots table, int64_t chunk,
                                     int64_t cap,
                                     const int64_t* __restrict__ block_base,
                                     int32_t* __restrict__ slot_gid,
                                     int64_t* __restrict__ uniq_rows) {
  int64_t start = (int64_t)blockIdx.x * chunk;
  int64_t stop = min(start + chunk, cap);
  __shared__ int lds_cnt;
  if (threadIdx.x == 0) lds_cnt = 0;
  __syncthreads();
  int64_t base = block_base[blockIdx.x];
  for (int64_t s = start + threadIdx.x; s < stop; s += blockDim.x) {
    if (table.occupied(s)) {
      int32_t gid = (int32_t)(base + atomicAdd(&lds_cnt, 1));
      if (slot_gid != nullptr) slot_gid[s] = gid;
      uniq_rows[gid] = table.row(s);
    }
  }
}

__global__ void gb_rowgid_kernel(const uint32_t* __restrict__ row_slot,
                                 const int32_t* __restrict__ slot_gid,
                                 int32_t* __restrict__ row_gid, int64_t n) {
  GRID_STRIDE_LOOP(i, n) { row_gid[i] = slot_gid[row_slot[i]]; }
}

// Number the occupied slots of a table of `cap` slots: uniq_rows[gid] =
// table.row(slot), and slot_gid[slot] = gid when asked for.  The count of
// groups is the one device-to-host transfer; `extra_word` (a one-element
// int64 device tensor, or null) travels with it and comes back in `extra`.
struct CompactedSlots {
  int64_t ngroups;
  int64_t extra;
  torch::Tensor slot_gid;   // int32 [cap], undefined unless asked for
  torch::Tensor uniq_rows;  // int64 [max(ngroups, 1)]
};

template <typename Slots>
static CompactedSlots compact_slots(Slots table, int64_t cap,
                                    const torch::Device& dev,
                                    bool want_slot_gid,
                                    const torch::Tensor* extra_word) {
  int block = 256;
  int nblocks = 2048;
  int64_t chunk = (cap + nblocks - 1) / nblocks;
  auto block_counts = torch::zeros({nblocks},
                                   torch::dtype(torch::kInt64).device(dev));
  hipLaunchKernelGGL(gb_count_kernel<Slots>, dim3(nblocks), dim3(block), 0,
                     cur_stream(), table, chunk, cap,
                     (int64_t*)block_counts.data_ptr());
  CHECK_HIP(hipGetLastError());
  auto block_base = torch::zeros({nblocks}, torch::dtype(torch::kInt64).device(dev));
  auto bb_tail = block_base.slice(0, 1, nblocks);
  at::cumsum_out(bb_tail, block_counts.slice(0, 0, nblocks - 1), 0);
  CompactedSlots out;
  out.extra = 0;
  if (extra_word == nullptr) {
    out.ngroups = block_counts.sum().item<int64_t>();
  } else {
    auto both = torch::cat({block_counts.sum().reshape({1}), *extra_word}).cpu();
    out.ngroups = both[0].item<int64_t>();
    out.extra = both[1].item<int64_t>();
  }
  if (want_slot_gid)
    out.slot_gid = torch::empty({cap}, torch::dtype(torch::kInt32).device(dev));
  out.uniq_rows = torch::empty({std::max<int64_t>(out.ngroups, 1)},
                               torch::dtype(torch::kInt64).device(dev));
  hipLaunchKernelGGL(gb_assign_gid_kernel<Slots>, dim3(nblocks), dim3(block),
                     0, cur_stream(), table, chunk, cap,
                     (const int64_t*)block_base.data_ptr(),
                     want_slot_gid ? (int32_t*)out.slot_gid.data_ptr() : nullptr,
                     (int64_t*)out.uniq_rows.data_ptr());
  CHECK_HIP(hipGetLastError());
  return out;
}

// Skeleton shared by both group builds.  The caller supplies its table:
//   alloc(cap)                    allocate an empty table of cap slots
//   insert(cap, start, cnt, rs)   launch the insert of rows [start, start+cnt),
//                                 rs = row_slot + start
//   occupied()                    slots in use (device sync)
//   view()                        GenericSlots / PackedSlots of the table
// Insert in chunks, checking the load factor between chunks; grow and
// re-insert when it crosses 1/2.  While the table is smaller than 2n slots a
// chunk is at most cap/2 - 1 rows (insert_step), each followed by a device
// sync and a count of the table.
template <typename Alloc, typename Insert, typename Occupied, typename View>
static std::vector<torch::Tensor> build_groups(
    int64_t n, const torch::Device& dev, int64_t chunk_rows,
    int64_t max_initial_cap, Alloc alloc, Insert insert, Occupied occupied,
    View view) {
  check_build_limits(chunk_rows, max_initial_cap);
  int block = 256;
  int64_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  if (cap > max_initial_cap) cap = max_initial_cap;
  auto row_slot = torch::empty({n}, torch::dtype(torch::kInt32).device(dev));
  while (true) {
    alloc(cap);
    bool grown = false;
    // Invariant (see insert_step): while cap < 2n a launch adds at most
    // cap/2 - 1 groups and starts with occupied <= cap/2, so occupied < cap
    // always holds and every probe finds a free slot or its group.
    const int64_t step = insert_step(chunk_rows, cap, n);
    for (int64_t start = 0; start < n; start += step) {
      int64_t cnt = std::min(step, n - start);
      insert(cap, start, cnt, (uint32_t*)row_slot.data_ptr() + start);
      CHECK_HIP(hipGetLastError());
      if (start + cnt < n && cap < 2 * n) {
        int64_t occ = occupied();
        if (occ * 2 > cap) {
          cap = grown_cap(cap, occ, n);
          grown = true;
          break;  // rebuild from scratch at the bigger capacity
        }
      }
    }
    if (!grown) break;
  }
  auto groups = compact_slots(view(), cap, dev, /*want_slot_gid=*/true,
                              nullptr);
  int64_t ngroups = groups.ngroups;
  auto& slot_gid = groups.slot_gid;
  auto& uniq_rows = groups.uniq_rows;
  auto row_gid = torch::empty({n}, torch::dtype(torch::kInt32).device(dev));
  hipLaunchKernelGGL(gb_rowgid_kernel, dim3(grid_for(n, block)), dim3(block),
                     0, cur_stream(), (const uint32_t*)row_slot.data_ptr(),
                     (const int32_t*)slot_gid.data_ptr(),
                     (int32_t*)row_gid.data_ptr(), n);
  CHECK_HIP(hipGetLastError());
  return {row_gid, uniq_rows.slice(0, 0, ngroups)};
}

std::vector<torch::Tensor> groupby_build_packed(torch::Tensor keys,
                                                int64_t chunk_rows,
                                                int64_t max_initial_cap) {
  auto dev = keys.device();
  torch::Tensor slot_keys, slot_rows;
  // 2^25 slots x 8 B = 256 MB: Infinity-Cache resident; grow on pressure
  return build_groups(
      keys.numel(), dev, chunk_rows, max_initial_cap,
      [&](int64_t cap) {
        slot_keys = torch::full({cap}, -1, torch::dtype(torch::kInt64).device(dev));
        slot_rows = torch::empty({cap}, torch::dtype(torch::kInt32).device(dev));
      },
      [&](int64_t cap, int64_t start, int64_t cnt, uint32_t* row_slot) {
        hipLaunchKernelGGL(gb_insert_packed_kernel, dim3(grid_for(cnt, 256)),
                           dim3(256), 0, cur_stream(),
                           (const int64_t*)keys.data_ptr() + start,
                           (unsigned long long*)slot_keys.data_ptr(),
                           (uint32_t*)slot_rows.data_ptr(), (uint64_t)(cap - 1),
                           row_slot, cnt, start);
      },
      [&] { return (slot_keys != -1).sum().item<int64_t>(); },
      [&] {
        return PackedSlots{(const unsigned long long*)slot_keys.data_ptr(),
                           (const uint32_t*)slot_rows.data_ptr()};
      });
}

std::vector<torch::Tensor> groupby_build(
    std::vector<torch::Tensor> datas,
    std::vector<c10::optional<torch::Tensor>> masks,
    std::vector<c10::optional<torch::Tensor>> offsets,
    std::vector<c10::optional<torch::Tensor>> auxs,
    std::vector<int64_t> dtypes, int64_t n, torch::Tensor hashes,
    int64_t chunk_rows, int64_t max_initial_cap) {
  auto dev = datas[0].device();
  auto ds = build_descset(datas, masks, offsets, auxs, dtypes, n);
  torch::Tensor slots;
  // Start with an Infinity-Cache-resident table (2^26 slots = 256 MB):
  // the random atomicCAS probes then hit L3 instead of HBM (guide §2).
  // Growth is 8x at a time (few groupbys exceed 32M groups/rank); n above
  // 2^25 rows takes several insert launches where chunk_rows alone would
  // give one.
  return build_groups(
      n, dev, chunk_rows, max_initial_cap,
      [&](int64_t cap) {
        slots = torch::zeros({cap}, torch::dtype(torch::kInt32).device(dev));
      },
      [&](int64_t cap, int64_t start, int64_t cnt, uint32_t* row_slot) {
        hipLaunchKernelGGL(gb_insert_kernel, dim3(grid_for(cnt, 256)),
                           dim3(256), 0, cur_stream(), ds.ptr(),
                           (int)datas.size(),
                           (const uint64_t*)hashes.data_ptr() + start,
                           (uint32_t*)slots.data_ptr(), (uint64_t)(cap - 1),
                           row_slot, cnt, start,
                           (const uint64_t*)hashes.data_ptr());
      },
      [&] { return torch::count_nonzero(slots).item<int64_t>(); },
      [&] { return GenericSlots{(const uint32_t*)slots.data_ptr()}; });
}

// ------------------------------------------------------------ agg update

enum AggOp : int {
  AGG_SUM_F64 = 0, AGG_SUM_I64 = 1, AGG_COUNT = 2, AGG_MIN_F64 = 3,
  AGG_MAX_F64 = 4, AGG_MIN_I64 = 5, AGG_MAX_I64 = 6, AGG_SIZE = 7,
  AGG_FIRST_ROW = 8, AGG_LAST_ROW = 9, AGG_PROD_F64 = 10,
};

// accumulators hold doubles for these ops and int64 for all others
__host__ __device__ inline bool is_f64_acc(int64_t op) {
  return op == AGG_SUM_F64 || op == AGG_MIN_F64 || op == AGG_MAX_F64 ||
         op == AGG_PROD_F64;
}

// One column value as both double and int64 (the op picks one).  Null rows
// and float NaNs are invalid; STRING and DECIMAL128 load nothing (only
// their validity is counted).
struct AggValue {
  bool valid;
  double dv;
  int64_t iv;
};

DEV_INLINE AggValue agg_load(const ColumnDesc& col, int64_t i) {
  AggValue v = {is_valid_at(col, i), 0.0, 0};
  if (!v.valid) return v;
  switch (col.dtype) {
    case BT_INT8: v.iv = ((const int8_t*)col.data)[i]; v.dv = (double)v.iv; break;
    case BT_UINT8: case BT_BOOL: v.iv = ((const uint8_t*)col.data)[i]; v.dv = (double)v.iv; break;
    case BT_INT16: v.iv = ((const int16_t*)col.data)[i]; v.dv = (double)v.iv; break;
    case BT_UINT16: v.iv = ((const uint16_t*)col.data)[i]; v.dv = (double)v.iv; break;
    case BT_INT32: case BT_DATE32: case BT_DICT:
      v.iv = ((const int32_t*)col.data)[i]; v.dv = (double)v.iv; break;
    case BT_UINT32: v.iv = ((const uint32_t*)col.data)[i]; v.dv = (double)v.iv; break;
    case BT_INT64: case BT_UINT64: case BT_TIMESTAMP_NS:
      v.iv = ((const int64_t*)col.data)[i]; v.dv = (double)v.iv; break;
    case BT_FLOAT32: {
      float f = ((const float*)col.data)[i];
      v.valid = !(f != f);
      v.dv = (double)f; v.iv = (int64_t)f;
      break;
    }
    case BT_FLOAT64: {
      double f = ((const double*)col.data)[i];
      v.valid = !(f != f);
      v.dv = f; v.iv = (int64_t)f;
      break;
    }
  }
  return v;
}

// Fold one contribution into accumulator slot `a`, which lives in global
// memory or in LDS (inlined, so the compiler picks the atomic's address
// space from the call site).  SIZE and COUNT only count; AGG_PROD_F64 has
// no LDS form and is handled by agg_update_kernel alone.
DEV_INLINE void agg_apply(int op, double* a, double dv, int64_t iv,
                          int64_t row) {
  switch (op) {
    case AGG_SUM_F64: atomicAdd(a, dv); break;
    case AGG_SUM_I64: atomicAdd((unsigned long long*)a, (unsigned long long)iv); break;
    case AGG_MIN_F64: atomic_min_f64(a, dv); break;
    case AGG_MAX_F64: atomic_max_f64(a, dv); break;
    case AGG_MIN_I64: atomic_min_i64((int64_t*)a, iv); break;
    case AGG_MAX_I64: atomic_max_i64((int64_t*)a, iv); break;
    case AGG_FIRST_ROW: atomic_min_i64((int64_t*)a, row); break;
    case AGG_LAST_ROW: atomic_max_i64((int64_t*)a, row); break;
  }
}

// Merge one block's LDS partial for group g (value bits `part`, `c` rows
// counted) into the global accumulators.  Groups the block never saw still
// hold the op's init value and are skipped.
DEV_INLINE void agg_merge(int op, void* acc, int64_t* cnt, int g, double part,
                          long long c) {
  if (c == 0) return;
  if (cnt != nullptr) atomicAdd((unsigned long long*)&cnt[g], (unsigned long long)c);
  int64_t bits = __double_as_longlong(part);
  agg_apply(op, (double*)acc + g, part, bits, bits);
}

__global__ void agg_update_kernel(const ColumnDesc col,
                                  const int32_t* __restrict__ row_gid,
                                  int op, void* __restrict__ acc,
                                  int64_t* __restrict__ cnt, int64_t n) {
  GRID_STRIDE_LOOP(i, n) {
    int32_t g = row_gid[i];
    if (op == AGG_SIZE) {
      atomicAdd((unsigned long long*)&cnt[g], 1ull);
      continue;
    }
    AggValue v = agg_load(col, i);
    if (!v.valid) continue;
    if (op == AGG_PROD_F64) {
      // CAS-loop multiply
      unsigned long long* a = (unsigned long long*)acc + g;
      unsigned long long old = *a, assumed;
      do {
        assumed = old;
        double nv = __longlong_as_double(assumed) * v.dv;
        old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(nv));
      } while (old != assumed);
    } else {
      agg_apply(op, (double*)acc + g, v.dv, v.iv, i);
    }
    if (cnt != nullptr) atomicAdd((unsigned long long*)&cnt[g], 1ull);
  }
}

// LDS pre-aggregation path for low-cardinality groupbys (TPC-H Q1 shape):
// per-block accumulators in LDS, one global atomic per (block, group).
// Replaces 60M global atomics on 6 slots (measured 243 ms/call) with
// 60M LDS atomics + ~2048*6 global ones.
#define LDS_AGG_MAX_GROUPS 2048

__global__ void agg_update_lds_kernel(const ColumnDesc col,
                                      const int32_t* __restrict__ row_gid,
                                      int op, int ngroups,
                                      void* __restrict__ acc,
                                      int64_t* __restrict__ cnt, int64_t n,
                                      double init_f, int64_t init_i) {
  __shared__ double lacc[LDS_AGG_MAX_GROUPS];
  __shared__ long long lcnt[LDS_AGG_MAX_GROUPS];
  for (int g = threadIdx.x; g < ngroups; g += blockDim.x) {
    lacc[g] = is_f64_acc(op) ? init_f : __longlong_as_double(init_i);
    lcnt[g] = 0;
  }
  __syncthreads();
  GRID_STRIDE_LOOP(i, n) {
    int32_t g = row_gid[i];
    if (op != AGG_SIZE) {
      AggValue v = agg_load(col, i);
      if (!v.valid) continue;
      agg_apply(op, &lacc[g], v.dv, v.iv, i);
    }
    // counted even when cnt == nullptr: the merge skips groups with c == 0
    atomicAdd((unsigned long long*)&lcnt[g], 1ull);
  }
  __syncthreads();
  for (int g = threadIdx.x; g < ngroups; g += blockDim.x)
    agg_merge(op, acc, cnt, g, lacc[g], lcnt[g]);
}

// fused multi-aggregate: one pass over row_gid updating up to 4 aggregates
// (taxi Q1: count + sum + count in ONE read of the gid array).  Ops are
// AGG_SUM_F64..AGG_SIZE only; agg_update_fused rejects the rest.
#define MAX_FUSED_AGGS 4

struct FusedAgg {
  ColumnDesc col;
  int op;
  void* acc;
  int64_t* cnt;
  double init_f;
  int64_t init_i;
};

__global__ void agg_update_fused_kernel(FusedAgg a0, FusedAgg a1, FusedAgg a2,
                                        FusedAgg a3, int n_aggs,
                                        const int32_t* __restrict__ row_gid,
                                        int64_t n) {
  FusedAgg aggs[MAX_FUSED_AGGS] = {a0, a1, a2, a3};
  GRID_STRIDE_LOOP(i, n) {
    int32_t g = row_gid[i];
    for (int k = 0; k < n_aggs; ++k) {
      int op = aggs[k].op;
      int64_t* cnt = aggs[k].cnt;
      if (op == AGG_SIZE) {
        atomicAdd((unsigned long long*)&cnt[g], 1ull);
        continue;
      }
      AggValue v = agg_load(aggs[k].col, i);
      if (!v.valid) continue;
      agg_apply(op, (double*)aggs[k].acc + g, v.dv, v.iv, i);
      if (cnt != nullptr) atomicAdd((unsigned long long*)&cnt[g], 1ull);
    }
  }
}

// LDS pre-aggregation variant of the fused kernel for low-cardinality keys
// (TPC-H Q1: 6 groups, 8 aggregates).  Without it 60M rows x 4 aggs of
// global atomics on 6 slots measured 274 ms/launch; with block-local LDS
// accumulators the global traffic is ~grid*ngroups atomics.
__global__ void agg_update_fused_lds_kernel(
    FusedAgg a0, FusedAgg a1, FusedAgg a2, FusedAgg a3, int n_aggs,
    int ngroups, const int32_t* __restrict__ row_gid, int64_t n) {
  FusedAgg aggs[MAX_FUSED_AGGS] = {a0, a1, a2, a3};
  extern __shared__ double smem[];
  double* lacc = smem;                              // n_aggs * ngroups
  long long* lcnt = (long long*)(smem + (size_t)n_aggs * ngroups);
  for (int j = threadIdx.x; j < n_aggs * ngroups; j += blockDim.x) {
    int k = j / ngroups;
    lacc[j] = is_f64_acc(aggs[k].op) ? aggs[k].init_f
                                     : __longlong_as_double(aggs[k].init_i);
    lcnt[j] = 0;
  }
  __syncthreads();
  GRID_STRIDE_LOOP(i, n) {
    int32_t g = row_gid[i];
    for (int k = 0; k < n_aggs; ++k) {
      int op = aggs[k].op;
      if (op != AGG_SIZE) {
        AggValue v = agg_load(aggs[k].col, i);
        if (!v.valid) continue;
        agg_apply(op, &lacc[(size_t)k * ngroups + g], v.dv, v.iv, i);
      }
      atomicAdd((unsigned long long*)&lcnt[(size_t)k * ngroups + g], 1ull);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_aggs * ngroups; j += blockDim.x) {
    int k = j / ngroups;
    agg_merge(aggs[k].op, aggs[k].acc, aggs[k].cnt, j - k * ngroups, lacc[j],
              lcnt[j]);
  }
}

// accumulator filled with the op's init value, plus the valid-row count
// when asked for or when the count is the op's result (else undefined)
static std::pair<torch::Tensor, torch::Tensor> alloc_agg(
    int64_t op, int64_t ngroups, double init_f, int64_t init_i,
    bool want_count, const torch::Device& dev) {
  torch::Tensor acc = is_f64_acc(op)
      ? torch::full({ngroups}, init_f, torch::dtype(torch::kFloat64).device(dev))
      : torch::full({ngroups}, init_i, torch::dtype(torch::kInt64).device(dev));
  torch::Tensor cnt;
  if (want_count || op == AGG_SIZE || op == AGG_COUNT)
    cnt = torch::zeros({ngroups}, torch::dtype(torch::kInt64).device(dev));
  return {acc, cnt};
}

// returns per agg: [acc, cnt?] pairs flattened
std::vector<torch::Tensor> agg_update_fused(
    std::vector<torch::Tensor> datas,
    std::vector<c10::optional<torch::Tensor>> masks,
    std::vector<int64_t> dtypes, std::vector<int64_t> ops,
    std::vector<double> init_fs, std::vector<int64_t> init_is,
    std::vector<int64_t> want_counts,
    torch::Tensor row_gid, int64_t ngroups) {
  auto dev = row_gid.device();
  int64_t n = row_gid.numel();
  int n_aggs = (int)datas.size();
  TORCH_CHECK(n_aggs >= 1 && n_aggs <= MAX_FUSED_AGGS);
  for (int k = 0; k < n_aggs; ++k)
    TORCH_CHECK(ops[k] >= AGG_SUM_F64 && ops[k] <= AGG_SIZE,
                "agg_update_fused: unsupported op ", ops[k]);
  std::vector<torch::Tensor> out;
  FusedAgg fas[MAX_FUSED_AGGS] = {};
  for (int k = 0; k < n_aggs; ++k) {
    auto [acc, cnt] = alloc_agg(ops[k], ngroups, init_fs[k], init_is[k],
                                want_counts[k] != 0, dev);
    fas[k].col = make_desc(datas[k], masks[k], c10::nullopt, c10::nullopt,
                           dtypes[k], n);
    fas[k].op = (int)ops[k];
    fas[k].acc = acc.data_ptr();
    fas[k].cnt = cnt.defined() ? (int64_t*)cnt.data_ptr() : nullptr;
    fas[k].init_f = init_fs[k];
    fas[k].init_i = init_is[k];
    out.push_back(acc);
    out.push_back(cnt.defined() ? cnt : torch::empty({0}));
  }
  int block = 256;
  size_t lds_bytes = (size_t)n_aggs * (size_t)ngroups * 16;
  if (lds_bytes <= 48 * 1024) {
    hipLaunchKernelGGL(agg_update_fused_lds_kernel, dim3(grid_for(n, block)),
                       dim3(block), lds_bytes, cur_stream(), fas[0], fas[1],
                       fas[2], fas[3], n_aggs, (int)ngroups,
                       (const int32_t*)row_gid.data_ptr(), n);
  } else {
    hipLaunchKernelGGL(agg_update_fused_kernel, dim3(grid_for(n, block)),
                       dim3(block), 0, cur_stream(), fas[0], fas[1], fas[2],
                       fas[3], n_aggs, (const int32_t*)row_gid.data_ptr(), n);
  }
  CHECK_HIP(hipGetLastError());
  return out;
}

std::vector<torch::Tensor> agg_update(
    torch::Tensor data, c10::optional<torch::Tensor> mask,
    c10::optional<torch::Tensor> offsets, int64_t dtype,
    torch::Tensor row_gid, int64_t ngroups, int64_t op, double init_f,
    int64_t init_i, bool want_count) {
  int64_t n = row_gid.numel();
  auto [acc, cnt] = alloc_agg(op, ngroups, init_f, init_i, want_count,
                              data.device());
  int64_t* cnt_ptr = cnt.defined() ? (int64_t*)cnt.data_ptr() : nullptr;
  ColumnDesc col = make_desc(data, mask, offsets, c10::nullopt, dtype, n);
  int block = 256;
  bool lds_ok = ngroups <= LDS_AGG_MAX_GROUPS && op != AGG_PROD_F64;
  if (lds_ok) {
    hipLaunchKernelGGL(agg_update_lds_kernel, dim3(grid_for(n, block)),
                       dim3(block), 0, cur_stream(), col,
                       (const int32_t*)row_gid.data_ptr(), (int)op,
                       (int)ngroups, acc.data_ptr(), cnt_ptr, n,
                       init_f, init_i);
  } else {
    hipLaunchKernelGGL(agg_update_kernel, dim3(grid_for(n, block)), dim3(block),
                       0, cur_stream(), col,
                       (const int32_t*)row_gid.data_ptr(), (int)op,
                       acc.data_ptr(), cnt_ptr, n);
  }
  CHECK_HIP(hipGetLastError());
  if (cnt.defined()) return {acc, cnt};
  return {acc};
}

// ---------------------------------------------------------------------
// dense groupby: keys of a small known range address the table directly.
// slot = sum_k (key_k - lo_k) * stride_k in mixed radix is a perfect group
// id, so one row pass reads every key and value column once and updates the
// accumulators; no key packing, hash insert, row_slot or row_gid.
//
// Table layout: nslots rows of (1 + n_aggs) 64-bit words, word 0 the row
// count of the slot (the `size` of its group), word 1 + k the accumulator
// of aggregate k: a row's atomics fall into one or two cache lines.  An
// aggregate over a column that can hold nulls or NaNs has an array of
// per-slot *invalid* counts beside the table, touched by such rows only;
// its valid count is size - invalid.
// ---------------------------------------------------------------------

#define MAX_DENSE_KEYS 8
#define DENSE_MAX_SLOTS (int64_t(1) << 25)

struct DenseKeys {
  const void* data[MAX_DENSE_KEYS];
  int dtype[MAX_DENSE_KEYS];
  int64_t lo[MAX_DENSE_KEYS];
  uint64_t radix[MAX_DENSE_KEYS];
  uint64_t stride[MAX_DENSE_KEYS];
  int nkeys;
};

struct DenseAgg {
  ColumnDesc col;
  int op;
  int64_t* invalid;  // per-slot count of null/NaN rows, or nullptr
};

struct DenseAggs {
  DenseAgg a[MAX_FUSED_AGGS];
  int n_aggs;
};

// integer-family value of row i (key columns and dense join keys)
DEV_INLINE int64_t load_int_key(const void* data, int dtype, int64_t i) {
  switch (dtype) {
    case BT_INT8: return ((const int8_t*)data)[i];
    case BT_UINT8: case BT_BOOL: return ((const uint8_t*)data)[i];
    case BT_INT16: return ((const int16_t*)data)[i];
    case BT_UINT16: return ((const uint16_t*)data)[i];
    case BT_INT32: case BT_DATE32: case BT_DICT:
      return ((const int32_t*)data)[i];
    case BT_UINT32: return ((const uint32_t*)data)[i];
    default: return ((const int64_t*)data)[i];  // INT64, UINT64
  }
}

static int64_t int_key_width(int64_t dtype) {
  switch (dtype) {
    case BT_INT8: case BT_UINT8: case BT_BOOL: return 1;
    case BT_INT16: case BT_UINT16: return 2;
    case BT_INT32: case BT_DATE32: case BT_DICT: case BT_UINT32: return 4;
    case BT_INT64: case BT_UINT64: return 8;
  }
  return 0;  // not an integer-family key
}

__global__ void dense_init_kernel(uint64_t* __restrict__ table, int words,
                                  uint64_t i0, uint64_t i1, uint64_t i2,
                                  uint64_t i3, int64_t nslots) {
  GRID_STRIDE_LOOP(j, nslots * words) {
    int w = (int)(j % words);
    table[j] = w == 0 ? 0ull : w == 1 ? i0 : w == 2 ? i1 : w == 3 ? i2 : i3;
  }
}

__global__ void groupby_dense_fused_kernel(const DenseKeys keys,
                                           const DenseAggs aggs,
                                           uint64_t* __restrict__ table,
                                           int64_t* __restrict__ err,
                                           int64_t n) {
  const int words = 1 + aggs.n_aggs;
  GRID_STRIDE_LOOP(i, n) {
    uint64_t slot = 0;
    bool in_range = true;
    for (int k = 0; k < keys.nkeys; ++k) {
      uint64_t digit = (uint64_t)load_int_key(keys.data[k], keys.dtype[k], i) -
                       (uint64_t)keys.lo[k];
      in_range &= digit < keys.radix[k];
      slot += digit * keys.stride[k];
    }
    if (!in_range) {  // val_range lied: the host reruns the hash route
      *err = 1;
      continue;
    }
    uint64_t* row = table + slot * words;
    atomicAdd((unsigned long long*)row, 1ull);
    for (int k = 0; k < aggs.n_aggs; ++k) {
      int op = aggs.a[k].op;
      if (op == AGG_SIZE) continue;
      AggValue v = agg_load(aggs.a[k].col, i);
      if (!v.valid) {
        atomicAdd((unsigned long long*)&aggs.a[k].invalid[slot], 1ull);
        continue;
      }
      agg_apply(op, (double*)(row + 1 + k), v.dv, v.iv, i);
    }
  }
}

struct DenseSlots {  // dense table: occupied = row count != 0, row = slot
  const uint64_t* table;
  int words;
  DEV_INLINE bool occupied(int64_t s) const { return table[s * words] != 0; }
  DEV_INLINE int64_t row(int64_t s) const { return s; }
};

// accumulators and valid counts of the occupied slots, in group order:
// acc[k][g] = word 1 + k of slot_ids[g]; cnt[g] = size (row 0 of cnt) and
// cnt[1 + k][g] = size - invalid_k where aggregate k has invalid counts
__global__ void dense_gather_kernel(const uint64_t* __restrict__ table,
                                    const DenseAggs aggs,
                                    const int64_t* __restrict__ slot_ids,
                                    uint64_t* __restrict__ acc,
                                    int64_t* __restrict__ cnt,
                                    int64_t ngroups) {
  const int words = 1 + aggs.n_aggs;
  GRID_STRIDE_LOOP(g, ngroups) {
    int64_t s = slot_ids[g];
    const uint64_t* row = table + s * words;
    int64_t size = (int64_t)row[0];
    cnt[g] = size;
    for (int k = 0; k < aggs.n_aggs; ++k) {
      acc[k * ngroups + g] = row[1 + k];
      if (aggs.a[k].invalid != nullptr)
        cnt[(1 + k) * ngroups + g] = size - aggs.a[k].invalid[s];
    }
  }
}

// Returns {} when a key fell outside its [lo, lo + radix): nothing of the
// result is valid then.  Otherwise [slot_ids, acc_0, cnt_0, acc_1, ...]:
// slot_ids int64 [ngroups], and per aggregate what agg_update_fused returns
// with want_count set (aggregates that cannot be invalid share one cnt).
std::vector<torch::Tensor> groupby_dense_fused(
    std::vector<torch::Tensor> key_datas, std::vector<int64_t> key_dtypes,
    std::vector<int64_t> key_los, std::vector<int64_t> key_radices,
    std::vector<torch::Tensor> datas,
    std::vector<c10::optional<torch::Tensor>> masks,
    std::vector<int64_t> dtypes, std::vector<int64_t> ops,
    std::vector<double> init_fs, std::vector<int64_t> init_is, int64_t n) {
  int nkeys = (int)key_datas.size();
  int n_aggs = (int)datas.size();
  TORCH_CHECK(nkeys >= 1 && nkeys <= MAX_DENSE_KEYS, "groupby_dense_fused: ",
              nkeys, " keys");
  TORCH_CHECK(n_aggs >= 1 && n_aggs <= MAX_FUSED_AGGS);
  TORCH_CHECK(n >= 1);
  TORCH_CHECK((int)key_dtypes.size() == nkeys && (int)key_los.size() == nkeys &&
              (int)key_radices.size() == nkeys);
  TORCH_CHECK((int)masks.size() == n_aggs && (int)dtypes.size() == n_aggs &&
              (int)ops.size() == n_aggs && (int)init_fs.size() == n_aggs &&
              (int)init_is.size() == n_aggs);
  auto dev = key_datas[0].device();
  DenseKeys keys = {};
  keys.nkeys = nkeys;
  int64_t nslots = 1;
  for (int k = nkeys - 1; k >= 0; --k) {  // last key varies fastest
    int64_t width = int_key_width(key_dtypes[k]);
    TORCH_CHECK(width != 0, "groupby_dense_fused: key dtype ", key_dtypes[k]);
    TORCH_CHECK(key_datas[k].is_contiguous() && key_datas[k].numel() >= n &&
                key_datas[k].element_size() == width,
                "groupby_dense_fused: key ", k, " storage");
    TORCH_CHECK(key_radices[k] >= 1 && key_radices[k] <= DENSE_MAX_SLOTS);
    keys.data[k] = key_datas[k].data_ptr();
    keys.dtype[k] = (int)key_dtypes[k];
    keys.lo[k] = key_los[k];
    keys.radix[k] = (uint64_t)key_radices[k];
    keys.stride[k] = (uint64_t)nslots;
    nslots *= key_radices[k];
    TORCH_CHECK(nslots <= DENSE_MAX_SLOTS, "groupby_dense_fused: key space");
  }
  DenseAggs aggs = {};
  aggs.n_aggs = n_aggs;
  uint64_t init_bits[MAX_FUSED_AGGS] = {};
  std::vector<torch::Tensor> invalids(n_aggs);
  for (int k = 0; k < n_aggs; ++k) {
    TORCH_CHECK(ops[k] >= AGG_SUM_F64 && ops[k] <= AGG_SIZE,
                "groupby_dense_fused: unsupported op ", ops[k]);
    aggs.a[k].op = (int)ops[k];
    aggs.a[k].col = make_desc(datas[k], masks[k], c10::nullopt, c10::nullopt,
                              dtypes[k], n);
    bool nullable = false;
    if (ops[k] != AGG_SIZE) {
      TORCH_CHECK(datas[k].is_contiguous() && datas[k].numel() >= n,
                  "groupby_dense_fused: value column ", k);
      TORCH_CHECK(!masks[k].has_value() ||
                  (masks[k]->is_contiguous() && masks[k]->numel() >= n &&
                   masks[k]->element_size() == 1));
      nullable = masks[k].has_value() || dtypes[k] == BT_FLOAT32 ||
                 dtypes[k] == BT_FLOAT64;
    }
    if (nullable) {
      invalids[k] = torch::zeros({nslots},
                                 torch::dtype(torch::kInt64).device(dev));
      aggs.a[k].invalid = (int64_t*)invalids[k].data_ptr();
    }
    if (is_f64_acc(ops[k])) {
      memcpy(&init_bits[k], &init_fs[k], 8);
    } else {
      init_bits[k] = (uint64_t)init_is[k];
    }
  }
  int words = 1 + n_aggs;
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto table = torch::empty({nslots * words}, i64);
  auto err = torch::zeros({1}, i64);
  int block = 256;
  hipLaunchKernelGGL(dense_init_kernel, dim3(grid_for(nslots * words, block)),
                     dim3(block), 0, cur_stream(),
                     (uint64_t*)table.data_ptr(), words, init_bits[0],
                     init_bits[1], init_bits[2], init_bits[3], nslots);
  CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(groupby_dense_fused_kernel, dim3(grid_for(n, block)),
                     dim3(block), 0, cur_stream(), keys, aggs,
                     (uint64_t*)table.data_ptr(), (int64_t*)err.data_ptr(), n);
  CHECK_HIP(hipGetLastError());
  DenseSlots view{(const uint64_t*)table.data_ptr(), words};
  auto groups = compact_slots(view, nslots, dev, /*want_slot_gid=*/false, &err);
  if (groups.extra != 0) return {};
  int64_t ngroups = groups.ngroups;
  auto acc = torch::empty({n_aggs, ngroups}, i64);
  auto cnt = torch::empty({1 + n_aggs, ngroups}, i64);
  if (ngroups) {
    hipLaunchKernelGGL(dense_gather_kernel, dim3(grid_for(ngroups, block)),
                       dim3(block), 0, cur_stream(),
                       (const uint64_t*)table.data_ptr(), aggs,
                       (const int64_t*)groups.uniq_rows.data_ptr(),
                       (uint64_t*)acc.data_ptr(), (int64_t*)cnt.data_ptr(),
                       ngroups);
    CHECK_HIP(hipGetLastError());
  }
  std::vector<torch::Tensor> out = {groups.uniq_rows.slice(0, 0, ngroups)};
  for (int k = 0; k < n_aggs; ++k) {
    auto a = acc.select(0, k);
    out.push_back(is_f64_acc(ops[k]) ? a.view(torch::kFloat64) : a);
    out.push_back(cnt.select(0, invalids[k].defined() ? 1 + k : 0));
  }
  return out;
}

// ---------------------------------------------------------------------
// hash join: bucket-chained build table + two-pass probe
// ---------------------------------------------------------------------

__global__ void join_build_kernel(const uint64_t* __restrict__ hashes,
                                  uint32_t* __restrict__ heads,
                                  uint32_t* __restrict__ next,
                                  uint64_t cap_mask, int64_t n) {
  GRID_STRIDE_LOOP(i, n) {
    uint64_t s = hashes[i] & cap_mask;
    uint32_t old = atomicExch(&heads[s], (uint32_t)i);
    next[i] = old;  // old == 0xFFFFFFFF means end of chain
  }
}

// count pass: matches per probe row
__global__ void join_probe_count_kernel(
    const ColumnDesc* __restrict__ bcols, const ColumnDesc* __restrict__ pcols,
    int ncols, const uint64_t* __restrict__ bh, const uint64_t* __restrict__ ph,
    const uint32_t* __restrict__ heads, const uint32_t* __restrict__ next,
    uint64_t cap_mask, int how,  // 0=inner,1=left,2=semi,3=anti
    int64_t* __restrict__ counts, int64_t n_probe) {
  GRID_STRIDE_LOOP(i, n_probe) {
    uint64_t h = ph[i];
    uint32_t cur = heads[h & cap_mask];
    int64_t c = 0;
    while (cur != 0xFFFFFFFFu) {
      if (bh[cur] == h && rows_eq2(pcols, bcols, ncols, i, (int64_t)cur)) {
        ++c;
        if (how == 2 || how == 3) break;  // semi/anti need existence only
      }
      cur = next[cur];
    }
    if (how == 0) counts[i] = c;
    else if (how == 1) counts[i] = c ? c : 1;  // left: null row when no match
    else if (how == 2) counts[i] = c ? 1 : 0;
    else counts[i] = c ? 0 : 1;  // anti
  }
}

__global__ void join_probe_fill_kernel(
    const ColumnDesc* __restrict__ bcols, const ColumnDesc* __restrict__ pcols,
    int ncols, const uint64_t* __restrict__ bh, const uint64_t* __restrict__ ph,
    const uint32_t* __restrict__ heads, const uint32_t* __restrict__ next,
    uint64_t cap_mask, int how, const int64_t* __restrict__ offsets,
    int64_t* __restrict__ out_probe, int64_t* __restrict__ out_build,
    uint8_t* __restrict__ build_matched, int64_t n_probe) {
  GRID_STRIDE_LOOP(i, n_probe) {
    uint64_t h = ph[i];
    uint32_t cur = heads[h & cap_mask];
    int64_t o = offsets[i];
    int64_t c = 0;
    while (cur != 0xFFFFFFFFu) {
      if (bh[cur] == h && rows_eq2(pcols, bcols, ncols, i, (int64_t)cur)) {
        if (how == 0 || how == 1) {
          out_probe[o + c] = i;
          out_build[o + c] = (int64_t)cur;
          if (build_matched) build_matched[cur] = 1;
        } else if (how == 2) {  // semi
          out_probe[o] = i;
        }
        ++c;
        if (how >= 2) break;
      }
      cur = next[cur];
    }
    if (how == 1 && c == 0) {
      out_probe[o] = i;
      out_build[o] = -1;
    }
    if (how == 3 && c == 0) out_probe[o] = i;
  }
}

std::vector<torch::Tensor> join_build(torch::Tensor hashes, int64_t n_build) {
  auto dev = hashes.device();
  int64_t cap = 16;
  while (cap < 2 * std::max<int64_t>(n_build, 1)) cap <<= 1;
  auto heads = torch::full({cap}, (int64_t)-1,
                           torch::dtype(torch::kInt32).device(dev));
  auto next = torch::empty({std::max<int64_t>(n_build, 1)},
                           torch::dtype(torch::kInt32).device(dev));
  if (n_build) {
    int block = 256;
    hipLaunchKernelGGL(join_build_kernel, dim3(grid_for(n_build, block)),
                       dim3(block), 0, cur_stream(),
                       (const uint64_t*)hashes.data_ptr(),
                       (uint32_t*)heads.data_ptr(),
                       (uint32_t*)next.data_ptr(), (uint64_t)(cap - 1),
                       n_build);
    CHECK_HIP(hipGetLastError());
  }
  return {heads, next};
}

std::vector<torch::Tensor> join_probe(
    // build key columns
    std::vector<torch::Tensor> bdatas,
    std::vector<c10::optional<torch::Tensor>> bmasks,
    std::vector<c10::optional<torch::Tensor>> boffsets,
    std::vector<c10::optional<torch::Tensor>> bauxs,
    std::vector<int64_t> bdtypes, int64_t n_build, torch::Tensor bh,
    // probe key columns
    std::vector<torch::Tensor> pdatas,
    std::vector<c10::optional<torch::Tensor>> pmasks,
    std::vector<c10::optional<torch::Tensor>> poffsets,
    std::vector<c10::optional<torch::Tensor>> pauxs,
    std::vector<int64_t> pdtypes, int64_t n_probe, torch::Tensor ph,
    torch::Tensor heads, torch::Tensor next, int64_t how,
    bool track_build_matched) {
  auto dev = bh.device();
  auto bds = build_descset(bdatas, bmasks, boffsets, bauxs, bdtypes, n_build);
  auto pds = build_descset(pdatas, pmasks, poffsets, pauxs, pdtypes, n_probe);
  int64_t cap = heads.numel();
  auto counts = torch::zeros({n_probe}, torch::dtype(torch::kInt64).device(dev));
  int block = 256;
  if (n_probe) {
    hipLaunchKernelGGL(join_probe_count_kernel,
                       dim3(grid_for(n_probe, block)), dim3(block), 0,
                       cur_stream(), bds.ptr(), pds.ptr(), (int)bdatas.size(),
                       (const uint64_t*)bh.data_ptr(),
                       (const uint64_t*)ph.data_ptr(),
                       (const uint32_t*)heads.data_ptr(),
                       (const uint32_t*)next.data_ptr(),
                       (uint64_t)(cap - 1), (int)how,
                       (int64_t*)counts.data_ptr(), n_probe);
    CHECK_HIP(hipGetLastError());
  }
  auto offs = torch::zeros({n_probe + 1}, torch::dtype(torch::kInt64).device(dev));
  auto offs_tail = offs.slice(0, 1, n_probe + 1);
  at::cumsum_out(offs_tail, counts, 0);
  int64_t total = n_probe ? offs[n_probe].item<int64_t>() : 0;
  auto out_probe = torch::empty({total}, torch::dtype(torch::kInt64).device(dev));
  auto out_build = torch::empty({(how == 0 || how == 1) ? total : 0},
                                torch::dtype(torch::kInt64).device(dev));
  torch::Tensor matched;
  uint8_t* matched_ptr = nullptr;
  if (track_build_matched) {
    matched = torch::zeros({std::max<int64_t>(n_build, 1)},
                           torch::dtype(torch::kUInt8).device(dev));
    matched_ptr = (uint8_t*)matched.data_ptr();
  }
  if (n_probe && total) {
    hipLaunchKernelGGL(join_probe_fill_kernel,
                       dim3(grid_for(n_probe, block)), dim3(block), 0,
                       cur_stream(), bds.ptr(), pds.ptr(), (int)bdatas.size(),
                       (const uint64_t*)bh.data_ptr(),
                       (const uint64_t*)ph.data_ptr(),
                       (const uint32_t*)heads.data_ptr(),
                       (const uint32_t*)next.data_ptr(),
                       (uint64_t)(cap - 1), (int)how,
                       (const int64_t*)offs.data_ptr(),
                       (int64_t*)out_probe.data_ptr(),
                       (int64_t*)out_build.data_ptr(), matched_ptr, n_probe);
    CHECK_HIP(hipGetLastError());
  }
  if (track_build_matched) return {out_probe, out_build, matched};
  return {out_probe, out_build};
}

// Dense probe for a unique integer build key of small range: lut[key - lo]
// is the build row of that key or -1.  One pass: out_build[i] is the build
// row matching probe row i, or -1 for a null key, a key outside the table
// or an empty entry; *misses counts the -1 rows.
__global__ void join_probe_dense_kernel(const void* __restrict__ pdata,
                                        const uint8_t* __restrict__ pmask,
                                        int pdtype,
                                        const int32_t* __restrict__ lut,
                                        uint64_t lut_len, int64_t lo,
                                        int64_t* __restrict__ out_build,
                                        int64_t* __restrict__ misses,
                                        int64_t n_probe) {
  int64_t local = 0;
  GRID_STRIDE_LOOP(i, n_probe) {
    int64_t b = -1;
    if (pmask == nullptr || pmask[i]) {
      uint64_t d = (uint64_t)load_int_key(pdata, pdtype, i) - (uint64_t)lo;
      if (d < lut_len) b = lut[d];
    }
    out_build[i] = b;
    local += b < 0;
  }
  __shared__ int64_t red[256];
  red[threadIdx.x] = local;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0])
    atomicAdd((unsigned long long*)misses, (unsigned long long)red[0]);
}

// returns [out_build int64 [n_probe], misses int64 [1]] (both on device)
std::vector<torch::Tensor> join_probe_dense(
    torch::Tensor pdata, c10::optional<torch::Tensor> pmask, int64_t pdtype,
    int64_t n_probe, torch::Tensor lut, int64_t lo) {
  auto dev = lut.device();
  int64_t width = int_key_width(pdtype);
  TORCH_CHECK(width != 0 && pdtype != BT_DICT && pdtype != BT_BOOL,
              "join_probe_dense: key dtype ", pdtype);
  TORCH_CHECK(n_probe >= 0 && pdata.is_contiguous() &&
              pdata.numel() >= n_probe && pdata.element_size() == width,
              "join_probe_dense: key storage");
  TORCH_CHECK(!pmask.has_value() ||
              (pmask->is_contiguous() && pmask->numel() >= n_probe &&
               pmask->element_size() == 1), "join_probe_dense: mask");
  TORCH_CHECK(lut.scalar_type() == torch::kInt32 && lut.is_contiguous() &&
              lut.numel() >= 1, "join_probe_dense: lut");
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto out_build = torch::empty({n_probe}, i64);
  auto misses = torch::zeros({1}, i64);
  if (n_probe) {
    int block = 256;
    hipLaunchKernelGGL(join_probe_dense_kernel, dim3(grid_for(n_probe, block)),
                       dim3(block), 0, cur_stream(), pdata.data_ptr(),
                       pmask.has_value() ? (const uint8_t*)pmask->data_ptr()
                                         : nullptr,
                       (int)pdtype, (const int32_t*)lut.data_ptr(),
                       (uint64_t)lut.numel(), lo,
                       (int64_t*)out_build.data_ptr(),
                       (int64_t*)misses.data_ptr(), n_probe);
    CHECK_HIP(hipGetLastError());
  }
  return {out_build, misses};
}

// ---------------------------------------------------------------------
// Parquet RLE/bit-packed hybrid expansion (on-GPU parquet decode path;
// reference role: cudf::io::read_parquet in gpu_read_parquet.h, here a
// hand-written gfx950 kernel).  Run table parsed on host from page bytes:
// kind 0 = RLE run (value repeated count times), kind 1 = bit-packed group
// (count values packed at `bitwidth` starting at bit_offset).

struct RleRun {
  int64_t out_start;
  int32_t count;
  int32_t kind;
  int64_t value_or_bitoff;
};

__global__ void rle_expand_kernel(const RleRun* __restrict__ runs, int n_runs,
                                  const uint8_t* __restrict__ packed,
                                  int bitwidth, int32_t* __restrict__ out) {
  // one wave per run slot, grid-stride over runs; lanes fill values
  int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  int lane = threadIdx.x % WAVE;
  int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / WAVE;
  for (int64_t r = wave_id; r < n_runs; r += n_waves) {
    RleRun run = runs[r];
    if (run.kind == 0) {
      int32_t v = (int32_t)run.value_or_bitoff;
      for (int64_t i = lane; i < run.count; i += WAVE) {
        out[run.out_start + i] = v;
      }
    } else {
      int64_t bit0 = run.value_or_bitoff;
      for (int64_t i = lane; i < run.count; i += WAVE) {
        int64_t bp = bit0 + i * bitwidth;
        int64_t byte = bp >> 3;
        int shift = (int)(bp & 7);
        // up to 32-bit reads cover bitwidth <= 24; parquet dict ids fit
        uint32_t w = (uint32_t)packed[byte]
                     | ((uint32_t)packed[byte + 1] << 8)
                     | ((uint32_t)packed[byte + 2] << 16)
                     | ((uint32_t)packed[byte + 3] << 24);
        out[run.out_start + i] = (int32_t)((w >> shift)
                                           & ((1u << bitwidth) - 1));
      }
    }
  }
}

torch::Tensor rle_expand(torch::Tensor runs_blob, int64_t n_runs,
                         torch::Tensor packed, int64_t bitwidth,
                         int64_t n_out) {
  auto dev = packed.device();
  auto out = torch::empty({n_out}, torch::dtype(torch::kInt32).device(dev));
  if (n_runs) {
    int block = 256;
    int waves_per_block = block / WAVE;
    int grid = (int)std::min<int64_t>(
        (n_runs + waves_per_block - 1) / waves_per_block, 2048);
    hipLaunchKernelGGL(rle_expand_kernel, dim3(grid), dim3(block), 0,
                       cur_stream(), (const RleRun*)runs_blob.data_ptr(),
                       (int)n_runs, (const uint8_t*)packed.data_ptr(),
                       (int)bitwidth, (int32_t*)out.data_ptr());
    CHECK_HIP(hipGetLastError());
  }
  return out;
}

torch::Tensor gemm_f32(torch::Tensor A, torch::Tensor B);  // gemm.hip

// parquet.hip: page-parallel on-GPU parquet decode
void pq_decompress(torch::Tensor src, torch::Tensor pages_blob,
                   int64_t n_pages, torch::Tensor scratch);
void pq_decompress_multi(torch::Tensor pages_blob, int64_t n_pages);
void pq_values_multi(torch::Tensor pages_blob, int64_t n_pages,
                     torch::Tensor err);
std::vector<torch::Tensor> pq_def_levels(torch::Tensor scratch,
                                         torch::Tensor pages_blob,
                                         int64_t n_pages, int64_t bitwidth,
                                         int64_t max_def, int64_t total_nv);
torch::Tensor pq_expand_codes(torch::Tensor scratch, torch::Tensor pages_blob,
                              int64_t n_pages,
                              c10::optional<torch::Tensor> val_data_off,
                              torch::Tensor dense_off,
                              c10::optional<torch::Tensor> n_valid,
                              int64_t dense_total);
torch::Tensor pq_copy_fixed(torch::Tensor scratch, torch::Tensor pages_blob,
                            int64_t n_pages,
                            c10::optional<torch::Tensor> val_data_off,
                            torch::Tensor dense_off,
                            c10::optional<torch::Tensor> n_valid,
                            int64_t esize, int64_t dense_total);
std::vector<torch::Tensor> pq_byte_array_lengths(
    torch::Tensor scratch, torch::Tensor pages_blob, int64_t n_pages,
    c10::optional<torch::Tensor> val_data_off, torch::Tensor dense_off,
    c10::optional<torch::Tensor> n_valid, int64_t dense_total);
torch::Tensor pq_copy_strings(torch::Tensor scratch, torch::Tensor src_abs,
                              torch::Tensor dst_off, torch::Tensor lengths,
                              int64_t n, int64_t total_bytes);
torch::Tensor pq_parse_headers(torch::Tensor chunk_buf);
std::vector<torch::Tensor> gather_multi(std::vector<torch::Tensor> srcs,
                                        torch::Tensor idx);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("gemm_f32", &gemm_f32, "f32 MFMA GEMM (v_mfma_f32_16x16x4_f32)");
  m.def("rle_expand", &rle_expand, "parquet RLE/bit-packed hybrid expand");
  m.def("agg_update_fused", &agg_update_fused, "fused multi-aggregate update");
  m.def("groupby_build_packed", &groupby_build_packed,
        "packed-u64-key hash groupby build", py::arg("keys"),
        py::arg("chunk_rows") = GB_CHUNK_ROWS,
        py::arg("max_initial_cap") = GB_PACKED_MAX_INITIAL_CAP);
  m.def("hash_columns", &hash_columns, "multi-column row hash");
  m.def("dt_field", &dt_field, "datetime field extraction");
  m.def("gather_string", &gather_string, "string column gather");
  m.def("groupby_build", &groupby_build, "hash groupby build",
        py::arg("datas"), py::arg("masks"), py::arg("offsets"),
        py::arg("auxs"), py::arg("dtypes"), py::arg("n"), py::arg("hashes"),
        py::arg("chunk_rows") = GB_CHUNK_ROWS,
        py::arg("max_initial_cap") = GB_MAX_INITIAL_CAP);
  m.def("agg_update", &agg_update, "aggregate update");
  m.def("join_build", &join_build, "hash join build");
  m.def("join_probe", &join_probe, "hash join probe");
  m.def("groupby_dense_fused", &groupby_dense_fused,
        "direct-address groupby: keys + fused aggregates in one row pass");
  m.def("join_probe_dense", &join_probe_dense,
        "direct-address probe of a unique small-range integer build key");
  m.def("pq_decompress", &pq_decompress,
        "page-parallel snappy decompress (one wave/page)");
  m.def("pq_decompress_multi", &pq_decompress_multi,
        "snappy decompress over a table of absolute page addresses");
  m.def("pq_values_multi", &pq_values_multi,
        "checked PLAIN / dictionary-code pages of a group -> shard columns");
  m.def("pq_def_levels", &pq_def_levels,
        "definition levels -> validity mask + per-page valid counts");
  m.def("pq_expand_codes", &pq_expand_codes,
        "RLE/bit-packed dictionary codes -> dense int32");
  m.def("pq_copy_fixed", &pq_copy_fixed,
        "PLAIN fixed-width page values -> dense buffer");
  m.def("pq_byte_array_lengths", &pq_byte_array_lengths,
        "PLAIN BYTE_ARRAY length/offset walk");
  m.def("pq_copy_strings", &pq_copy_strings,
        "gather string bytes to packed buffer");
  m.def("pq_parse_headers", &pq_parse_headers,
        "host-side thrift page-header parse of a chunk buffer");
  m.def("gather_multi", &gather_multi,
        "fused multi-column fixed-width gather (one launch per table)");
  m.attr("_native") = true;
}
