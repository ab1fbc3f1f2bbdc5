// Geometry of the partitioned dense groupby (kernels.hip): how the slot
// space is cut into partitions that one block aggregates in LDS, and how
// many radix passes bring the rows of a partition together.  Plain C++ with
// no HIP or torch dependency, so a host program can check it on its own
// (tests/dense_partition_geometry_main.cpp).
#pragma once

#include <stdint.h>

// rows per radix tile; kernels.hip asserts that it equals radix.h's RS_TILE
#define DP_TILE 2048
// fixed grid of a radix pass (radix.h's RS_MAX_BLOCKS)
#define DP_MAX_BLOCKS 2048
// slot bits of a record word (DENSE_MAX_SLOTS is 2^25)
#define DP_SLOT_BITS 25
// a radix pass sorts by at most this many bits
#define DP_PASS_BITS 7
#define DP_MAX_PASSES 3
// LDS words (8 B) for one partition's accumulators: 48 KiB
#define DP_ACC_WORDS 6144
// LDS invalid counters (4 B): 16 KiB, one array of S per aggregate
#define DP_INV_WORDS 4096
// A partition with more rows than this is split over several blocks, which
// merge with global atomics.  Twice the flagship's rows per partition.
#define DP_CHUNK_CAP (int64_t(1) << 18)

struct DensePartGeom {
  int part_bits;        // log2 of S, the slots per partition
  int64_t partitions;   // ceil(nslots / S)
  int sort_bits;        // bits of the partition id that the passes sort by
  int passes;           // radix passes, 0 when there is one partition
  int pass_shift[DP_MAX_PASSES];  // bit of the record word a pass starts at
  int pass_bits[DP_MAX_PASSES];   // 1 .. DP_PASS_BITS
  int64_t chunk_cap;    // rows one block aggregates at most
  int64_t single_items;  // blocks of the one-block-per-partition launch
  int64_t split_items;   // blocks of the split launch: ceil(n / chunk_cap)
  int64_t tiles;        // ceil(n / DP_TILE)
  int radix_blocks;     // grid of every radix pass
};

// words = 1 + n_aggs (1 .. 5), 1 <= nslots <= 2^25, 1 <= n < 2^31.
// S is 2048 slots up to three words and 1024 above: the accumulators
// (S * words * 8 B) and invalid counters (S * (words - 1) * 4 B) of one
// partition fit DP_ACC_WORDS and DP_INV_WORDS.
inline DensePartGeom dense_part_geometry(int64_t nslots, int words,
                                         int64_t n) {
  DensePartGeom g = {};
  g.part_bits = words <= 3 ? 11 : 10;
  const int64_t S = int64_t(1) << g.part_bits;
  g.partitions = (nslots + S - 1) / S;
  g.sort_bits = 0;
  while ((int64_t(1) << g.sort_bits) < g.partitions) ++g.sort_bits;
  g.passes = (g.sort_bits + DP_PASS_BITS - 1) / DP_PASS_BITS;
  int left = g.sort_bits, shift = g.part_bits;
  for (int p = 0; p < g.passes; ++p) {  // even split, low bits first
    int bits = (left + (g.passes - p) - 1) / (g.passes - p);
    g.pass_shift[p] = shift;
    g.pass_bits[p] = bits;
    shift += bits;
    left -= bits;
  }
  g.chunk_cap = DP_CHUNK_CAP;
  g.single_items = g.partitions;
  g.split_items = (n + g.chunk_cap - 1) / g.chunk_cap;
  g.tiles = (n + DP_TILE - 1) / DP_TILE;
  g.radix_blocks = (int)(g.tiles < DP_MAX_BLOCKS ? g.tiles : DP_MAX_BLOCKS);
  return g;
}
