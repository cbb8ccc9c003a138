// rpc_amd/csrc/crc32_gather.h -- the gather fold (crc32_gather.hip, DESIGN.md
// 4.10): per-segment CRCs -> per-body CRCs of bodies given as segment lists.
//
// Body i is the concatenation of segments first[i] .. first[i + 1] - 1.  With
// (crc_s, len_s) of every segment (the ragged pass, kModeFinal), the body's CRC
// is the left fold of zlib's combine,
//     c = seed_i (or 0);  for s in order: c = A_{len_s}(c) ^ crc_s,
// and the pairs (crc, len) form a monoid under
//     (c1, l1) . (c2, l2) = (A_{l2}(c1) ^ c2, l1 + l2),   identity (0, 0),
// so a long body is folded as a tree: per-thread runs, lanes, waves, tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "workspace.h"

namespace rpccrc {

// Bodies of at most this many segments are folded by one lane (64 consecutive
// bodies per wave); longer ones go to a device worklist, one workgroup each.
constexpr uint32_t kGatherLaneMax = 32;
// Worklist 0 (narrow): bodies of kGatherLaneMax < segments < kGatherWideMin, one
// workgroup of kGatherNarrowNT threads folds the body's segments (several
// workgroups per CU: many medium bodies at once).
// Worklist 1 (wide): the rest.  A wide body is cut into tiles of kGatherTile
// segments, one workgroup of kGatherWideNT threads each, anywhere on the chip;
// then one workgroup folds the body's tile values as a narrow body's segments.
constexpr uint32_t kGatherNarrowNT = 256;
constexpr uint32_t kGatherWideNT = 1024;
constexpr uint32_t kGatherRunMax = 16;  // pairs per thread and tile, at most
constexpr uint64_t kGatherWideMin = (uint64_t)kGatherNarrowNT * kGatherRunMax; // one narrow tile
constexpr uint64_t kGatherTile = (uint64_t)kGatherWideNT * kGatherRunMax;

struct GatherArgs {
  const uint32_t *seg_crc;   // nseg CRCs (rpc_crc32 values; 0 for an empty segment)
  const uint32_t *seg_len;   // nseg lengths
  const uint64_t *seg_first; // n + 1 (CSR)
  uint64_t nseg;
  uint64_t n;
  const uint32_t *seed;      // n running CRCs, or nullptr (0)
  uint32_t *out;             // n (may be seed)
  const uint4 *shift_nib;    // NIB[k][i][j] = A_{2^k bytes}(j << 4i) (kShiftNibWords)
  uint64_t *work_n;          // [3] fill counts of the two worklists and the tile list, ZERO at the lane kernel's launch
  uint64_t *work[2];         // body indices
  uint64_t work_cap[2];
  uint64_t *wide_tile0;      // work_cap[1]: a wide body's first entry in the tile list
  uint64_t *tile_slot;       // tile_cap: the tile's body, as its slot in worklist 1
  uint32_t *tile_crc;        // tile_cap: the tile's pair (gather_tile_kernel)
  uint64_t *tile_len;
  uint64_t tile_cap;
};

// Workspace behind the segment CRCs: the counters, the worklists, the tile
// list.  Sets them and the capacities (the caller fills in the rest).
void gather_layout(WsLayout &w, uint64_t n, uint64_t nseg, GatherArgs *a);
// Zeroes the counters, then the lane kernel, the narrow fold, the tile pass and
// the wide fold.  Stream-ordered; the launch shapes depend on n, nseg and cus only.
hipError_t launch_gather_fold(const GatherArgs &a, int cus, hipStream_t s);

} // namespace rpccrc
