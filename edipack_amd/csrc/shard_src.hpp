// shard_src.hpp -- where a row of the SOURCE vector sits once the ranks' shards have been all-gathered (the seeds on
// shards: edigpu_shard_seeds.hip; kernels_axisop.hip, kernels_pairs.hip, kernels_ops.hip).
//
// A rank holds `cnt_r` consecutive electronic units (down rows of normal mode, rows of superc / nonsu2) in every one of the
// nblk phonon blocks, block after block: [nblk][cnt_r][unit_len].  The all-gather concatenates the ranks' chunks, each
// padded to chunk = q unit_len nblk.  With phonon blocks that is NOT the reference's layout [nblk][units][unit_len]: a
// block of the gathered vector holds the rows of one rank only, and the last rank's blocks are shorter than the others'.
// With q = units (one rank, or a whole vector) the offset below is (p units + g) unit_len, the reference's layout, which is
// what lets one kernel body serve whole vectors and gathered shards.
//
// Plain C++, exact integer division (no multiply-high magic), shared by the kernels, the host-only _info entry points and
// the CPU suite (tests/host_shard_src.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SHARD_SRC_HD __host__ __device__ inline
#else
#define SHARD_SRC_HD inline
#endif

namespace edigpu {

// q: units per rank (the tail ranks hold fewer, or none), units: electronic units of the sector, chunk: elements a rank
// contributes to the all-gather (q unit_len nblk), unit_len: elements of a unit.  chunk and unit_len count doubles in the
// C-ABI layer; a kernel whose element is a double2 is handed both halved (shard_src_in_pairs).
struct ShardSrc {
  int64_t q = 1, units = 1, chunk = 1, unit_len = 1;
  int nblk = 1;
};

// offset of electronic unit g of phonon block p in the concatenation of the ranks' padded chunks
SHARD_SRC_HD int64_t shard_src_offset(const ShardSrc& s, int64_t p, int64_t g) {
  const int64_t r = g / s.q;
  const int64_t left = s.units - r * s.q, cnt = left < s.q ? left : s.q;
  return r * s.chunk + (p * cnt + (g - r * s.q)) * s.unit_len;
}

// The two forms of a gather kernel.  WholeVector: source and destination are whole vectors in the reference's layout (the
// single-GPU calls).  ShardWindow: the destination is the window [j_first, j_first + j_count) of the units the operators
// change, written block after block as [nblk][j_count][unit_len] -- a rank's shard --, the partner tables are indexed by
// the global unit, and the source is the gathered vector described by s.
struct WholeVector {
  static constexpr bool kWindow = false;
};
struct ShardWindow {
  static constexpr bool kWindow = true;
  int64_t j_first = 0, j_count = 0;
  ShardSrc s;
};

// the same geometry counted in pairs of doubles (chunk and unit_len must be even)
SHARD_SRC_HD ShardSrc shard_src_in_pairs(ShardSrc s) {
  s.chunk /= 2;
  s.unit_len /= 2;
  return s;
}

}  // namespace edigpu
