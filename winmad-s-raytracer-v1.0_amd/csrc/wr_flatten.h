// wr::Scene flattened into the HBM layout the KD traversal and the vertex
// kernels read (DevScene, wr_traverse.h:5-19): node records, reference records
// with the triangle inlined, per-primitive arrays, lights and materials -- and
// the facts the context derives from the scene's counts.  Pure host arithmetic
// (g++, no HIP headers), so tests/native/flatten_check.cpp checks it without a
// GPU.  wr_render.hip uploads the arrays as they are and pins the layouts of
// the element types against HIP's with static_asserts.
#pragma once
#include <cstdint>
#include <vector>

#include "wr_layout.h"
#include "wr_scene.h"

namespace wr {

// same layout as HIP's uint2 / uint4 / float2 / float4
struct alignas(8) U2 {
  uint32_t x, y;
};
struct alignas(16) U4 {
  uint32_t x, y, z, w;
};
struct alignas(8) F2 {
  float x, y;
};
struct alignas(16) F4 {
  float x, y, z, w;
};

struct SceneFlat {
  // node i as (self, left child), (right child), and its subtree of
  // kRecLevels levels in heap order, two entries per U4 (kRecU4 per node)
  std::vector<U4> nrec;
  std::vector<U2> nrec_r;
  std::vector<U4> nrec3;
  // per leaf reference: (p0.xyz, A), (B, C, D, E), (F, prim bits)
  std::vector<F4> ref_a, ref_b;
  std::vector<F2> ref_c;
  // per primitive
  std::vector<int> prim_mat, prim_type;
  std::vector<F4> prim_tri;    // (A, B, C, D)
  std::vector<F2> prim_tri2;   // (E, F)
  std::vector<F4> prim_sph;    // (cx, cy, cz, r)
  std::vector<F4> prim_sbox0;  // (lx, ly, lz, rx)
  std::vector<F2> prim_sbox1;  // (ry, rz)
  std::vector<F4> prim_rec;    // [2i] = prim_tri, [2i+1] = (E, F, material bits, type bits)
  // Light and Material are DLight and DMat field for field
  std::vector<Light> lights;
  std::vector<Material> mats;  // at least one entry (zero when the scene has none)
  int max_stack = 1;           // traversal stack bound, at least 1
  bool spheres = false;        // the scene has a primitive that is no triangle
  // <= 65536 nodes, leaves small enough for 16-bit stack nodes and pair
  // offsets (64 lanes x kLeavesPerRound leaves x max leaf size < 65536)
  bool narrow = false;
  // kd_walk_wave can run: node index and depth share a word, the leaf key and
  // the position in the leaf 64 bits (the key's lowest bit is 64 - dep_max, so
  // every leaf must hold fewer than 2^(64 - dep_max) references)
  bool walk_wave = false;
};

void flatten_scene(const Scene& s, SceneFlat& out);

}  // namespace wr
