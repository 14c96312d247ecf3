// The ray slab of a BDPT pipeline: the arrays a traversal launch
// reads and writes -- origins, directions, t, prim of every group member's
// shadow / aux queue and extension queue -- are segments of one slab per
// parity, so that a launch addresses a ray as base[k * stride + e] with one
// base pointer per field and one plane stride (wr_traverse.h, SlabQueues).
// Plain C++17 with no HIP in it, so that the carving is tested without a GPU
// (tests/native/queue_slab_check.cpp).
#pragma once
#include <cstdint>

namespace wr {

constexpr int kSlabMaxMembers = 8;  // >= the pipelines' group size
constexpr int kSlabAlign = 64;      // segment bases: whole waves of entries

// Segments in launch order -- member 0's shadow queue, its extension queue,
// member 1's shadow queue, ... -- so a launch's indices map to slab entries in
// ascending order.
struct QueueSlabLayout {
  int members = 0;
  int cap_sq = 0;   // entries of a shadow / aux segment (its clamp)
  int cap_ext = 0;  // entries of an extension segment
  int stride = 0;   // entries of the slab = the plane stride of its 3-plane arrays; 0: no layout
  int sq_base[kSlabMaxMembers] = {};
  int ext_base[kSlabMaxMembers] = {};
};

inline int slab_round(int n) { return (n + kSlabAlign - 1) / kSlabAlign * kSlabAlign; }

// stride 0 when the arguments are out of range or a 3-plane index 3 * stride
// would pass INT_MAX (the kernels index with int)
inline QueueSlabLayout queue_slab_layout(int members, int cap_sq, int cap_ext) {
  QueueSlabLayout L;
  constexpr int kMaxCap = INT32_MAX - kSlabAlign;  // slab_round stays in range
  if (members < 1 || members > kSlabMaxMembers || cap_sq < 0 || cap_ext < 0 || cap_sq > kMaxCap || cap_ext > kMaxCap)
    return L;
  int64_t at = 0;
  for (int m = 0; m < members; ++m) {
    if (at > INT32_MAX) return L;
    L.sq_base[m] = static_cast<int>(at);
    at += slab_round(cap_sq);
    if (at > INT32_MAX) return L;
    L.ext_base[m] = static_cast<int>(at);
    at += slab_round(cap_ext);
  }
  if (at == 0 || 3 * at > INT32_MAX) return L;
  L.members = members;
  L.cap_sq = cap_sq;
  L.cap_ext = cap_ext;
  L.stride = static_cast<int>(at);
  return L;
}

}  // namespace wr
