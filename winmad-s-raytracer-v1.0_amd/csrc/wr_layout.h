// Layout constants of the KD traversal's HBM arrays that both the kernels
// (wr_traverse.h) and the host flattening (wr_flatten.cpp) need.  No HIP here:
// g++ and hipcc include it alike, and both get the -D knobs from CXXFLAGS.
#pragma once

namespace wrd {

#ifndef WR_NODE_LEVELS
// tree levels resolved per dependent record load (2, 3 or 4); 3 over 2: C2
// 892 -> 911 Mrays/s; 4 (128-byte records, exact) loses 13-16 % on C2/C3
#define WR_NODE_LEVELS 3
#endif
static_assert(WR_NODE_LEVELS >= 2 && WR_NODE_LEVELS <= 4, "node record levels: 2, 3 or 4");
constexpr int kRecLevels = WR_NODE_LEVELS < 3 ? 3 : WR_NODE_LEVELS;  // nrec3 layout
constexpr int kRecU4 = kRecLevels == 4 ? 8 : 4;                      // uint4 per record
#ifndef WR_LEAVES_PER_ROUND
#define WR_LEAVES_PER_ROUND 4
#endif
constexpr int kLeavesPerRound = WR_LEAVES_PER_ROUND;  // leaves a lane may collect per round

}  // namespace wrd
