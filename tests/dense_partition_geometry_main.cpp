// Checks dense_part_geometry (csrc/dense_partition.h) over edge values.
// Built and run by tests/test_dense_partition_geometry_cpu.py with
// -fsanitize=address,undefined; exits non-zero at the first failure.
#include <cstdio>
#include <cstdlib>

#include "dense_partition.h"

#define REQUIRE(cond)                                                      \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "nslots=%lld words=%d n=%lld: %s\n",            \
                   (long long)nslots, words, (long long)n, #cond);         \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static void check(int64_t nslots, int words, int64_t n) {
  const DensePartGeom g = dense_part_geometry(nslots, words, n);
  const int64_t S = int64_t(1) << g.part_bits;
  // one partition's accumulators and invalid counters fit the LDS arrays
  REQUIRE(S * words <= DP_ACC_WORDS);
  REQUIRE(S * (words - 1) <= DP_INV_WORDS);
  // the partitions cover the slots, the last one possibly ragged
  REQUIRE(g.partitions >= 1);
  REQUIRE(g.partitions * S >= nslots);
  REQUIRE((g.partitions - 1) * S < nslots);
  REQUIRE((int64_t(1) << g.sort_bits) >= g.partitions);
  REQUIRE(g.sort_bits == 0 || (int64_t(1) << (g.sort_bits - 1)) < g.partitions);
  // the passes tile the partition id's bits inside the slot bits
  REQUIRE(g.passes >= 0 && g.passes <= DP_MAX_PASSES);
  REQUIRE((g.passes == 0) == (g.partitions == 1));
  int shift = g.part_bits;
  for (int p = 0; p < g.passes; ++p) {
    REQUIRE(g.pass_shift[p] == shift);
    REQUIRE(g.pass_bits[p] >= 1 && g.pass_bits[p] <= DP_PASS_BITS);
    shift += g.pass_bits[p];
  }
  REQUIRE(shift == g.part_bits + g.sort_bits);
  REQUIRE(shift <= DP_SLOT_BITS);
  // work items: one block per partition, and chunks that cover the rows
  REQUIRE(g.chunk_cap >= 1);
  REQUIRE(g.single_items == g.partitions);
  REQUIRE(g.single_items <= (int64_t(1) << 16));
  REQUIRE(g.split_items * g.chunk_cap >= n);
  REQUIRE((g.split_items - 1) * g.chunk_cap < n);
  REQUIRE(g.split_items <= (int64_t(1) << 16));
  REQUIRE(g.tiles * DP_TILE >= n && (g.tiles - 1) * DP_TILE < n);
  REQUIRE(g.radix_blocks >= 1 && g.radix_blocks <= DP_MAX_BLOCKS);
  REQUIRE(g.radix_blocks <= g.tiles);
}

int main() {
  const int64_t max_slots = int64_t(1) << DP_SLOT_BITS;
  int cases = 0;
  for (int words = 1; words <= 5; ++words) {
    const int64_t S = int64_t(1) << dense_part_geometry(1, words, 1).part_bits;
    const int64_t slots[] = {1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1,
                             128 * S, 128 * S + 1, 351125, 16854000,
                             max_slots - 1, max_slots};
    const int64_t rows[] = {1, DP_TILE - 1, DP_TILE, DP_TILE + 1,
                            DP_CHUNK_CAP, DP_CHUNK_CAP + 1, 1036465968,
                            (int64_t(1) << 31) - 1};
    for (int64_t nslots : slots)
      for (int64_t n : rows) {
        check(nslots, words, n);
        ++cases;
      }
  }
  // the flagship's shape: two 7-bit passes over 8230 partitions of 2048
  const DensePartGeom f = dense_part_geometry(16854000, 3, 1036465968);
  if (f.part_bits != 11 || f.partitions != 8230 || f.passes != 2 ||
      f.pass_bits[0] != 7 || f.pass_bits[1] != 7) {
    std::fprintf(stderr, "flagship geometry\n");
    return 1;
  }
  std::printf("dense_part_geometry: %d cases OK\n", cases);
  return 0;
}
