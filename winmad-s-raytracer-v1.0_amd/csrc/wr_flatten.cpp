// The tree + primitives of wr::Scene in the HBM layout of wr_traverse.h.
// Compiled with -ffp-contract=off: the A..F terms are the reference's float
// subtractions (triangle.cpp:24-30), rounded as it rounds them.
#include "wr_flatten.h"

#include <algorithm>
#include <cstring>

namespace wr {

namespace {
float bits_of(int v) {  // an int field's bits in a float slot
  float f;
  std::memcpy(&f, &v, 4);
  return f;
}
}  // namespace

void flatten_scene(const Scene& s, SceneFlat& o) {
  const size_t nn = s.nodes.size(), nr = s.refs.size(), np = s.prims.size();
  std::vector<U2> nodes(nn);
  for (size_t i = 0; i < nn; ++i) {
    const KdNode& k = s.nodes[i];
    if (k.axis >= 0) {
      uint32_t bits;
      std::memcpy(&bits, &k.split, 4);
      nodes[i] = U2{bits, (static_cast<uint32_t>(k.right) << 2) | static_cast<uint32_t>(k.axis)};
    } else {
      nodes[i] = U2{static_cast<uint32_t>(k.first), (static_cast<uint32_t>(k.count) << 2) | 3u};
    }
  }
  o.nrec.assign(nn, U4{0u, 0u, 0u, 0u});
  o.nrec_r.assign(nn, U2{0u, 0u});
  for (size_t i = 0; i < nn; ++i) {
    const U2 self = nodes[i];
    U2 l{0u, 0u};
    if (s.nodes[i].axis >= 0) {
      l = nodes[i + 1];
      o.nrec_r[i] = nodes[static_cast<size_t>(s.nodes[i].right)];
    }
    o.nrec[i] = U4{self.x, self.y, l.x, l.y};
  }
  // multi-level records (WR_NODE_LEVELS = 3 or 4): node i's subtree of
  // kRecLevels levels in heap order (entry 0 = i, entries 2h+1 / 2h+2 = the
  // children of entry h; 0 below a leaf), two entries per U4
  o.nrec3.assign(wrd::kRecU4 * nn, U4{0u, 0u, 0u, 0u});
  {
    constexpr int kEnt = (1 << wrd::kRecLevels) - 1;
    for (size_t i = 0; i < nn; ++i) {
      int64_t e[kEnt];
      e[0] = static_cast<int64_t>(i);
      for (int h = 0; 2 * h + 2 < kEnt; ++h) {
        e[2 * h + 1] = e[2 * h + 2] = -1;
        if (e[h] >= 0 && s.nodes[static_cast<size_t>(e[h])].axis >= 0) {
          e[2 * h + 1] = e[h] + 1;
          e[2 * h + 2] = s.nodes[static_cast<size_t>(e[h])].right;
        }
      }
      for (int h = 0; h < kEnt; ++h) {  // entry h: words 2h, 2h + 1 of the record
        const U2 v = e[h] >= 0 ? nodes[static_cast<size_t>(e[h])] : U2{0u, 0u};
        U4& r = o.nrec3[wrd::kRecU4 * i + static_cast<size_t>(h / 2)];
        if (h & 1) {
          r.z = v.x;
          r.w = v.y;
        } else {
          r.x = v.x;
          r.y = v.y;
        }
      }
    }
  }
  o.ref_a.resize(nr);
  o.ref_b.resize(nr);
  o.ref_c.resize(nr);
  for (size_t i = 0; i < nr; ++i) {
    const int pi = s.refs[i];
    const Prim& p = s.prims[pi];
    if (p.type == kTri) {
      // A..F exactly as Triangle::hit forms them (triangle.cpp:24-30)
      o.ref_a[i] = F4{p.p0.x, p.p0.y, p.p0.z, p.p0.x - p.p1.x};
      o.ref_b[i] = F4{p.p0.y - p.p1.y, p.p0.z - p.p1.z, p.p0.x - p.p2.x, p.p0.y - p.p2.y};
      o.ref_c[i] = F2{p.p0.z - p.p2.z, bits_of(pi)};
    } else {
      o.ref_a[i] = F4{0, 0, 0, 0};
      o.ref_b[i] = F4{0, 0, 0, 0};
      o.ref_c[i] = F2{0.f, bits_of(-(pi + 1))};
    }
  }
  o.prim_mat.resize(np);
  o.prim_type.resize(np);
  o.prim_tri.resize(np);
  o.prim_tri2.resize(np);
  o.prim_sph.resize(np);
  o.prim_sbox0.resize(np);
  o.prim_sbox1.resize(np);
  o.prim_rec.resize(2 * np);
  o.spheres = false;
  for (size_t i = 0; i < np; ++i) {
    const Prim& p = s.prims[i];
    o.prim_mat[i] = p.mat;
    o.prim_type[i] = p.type;
    o.prim_tri[i] = F4{p.p0.x - p.p1.x, p.p0.y - p.p1.y, p.p0.z - p.p1.z, p.p0.x - p.p2.x};
    o.prim_tri2[i] = F2{p.p0.y - p.p2.y, p.p0.z - p.p2.z};
    o.prim_sph[i] = F4{p.c.x, p.c.y, p.c.z, p.r};
    o.prim_sbox0[i] = F4{p.bl.x, p.bl.y, p.bl.z, p.br.x};
    o.prim_sbox1[i] = F2{p.br.y, p.br.z};
    o.prim_rec[2 * i] = o.prim_tri[i];
    o.prim_rec[2 * i + 1] = F4{o.prim_tri2[i].x, o.prim_tri2[i].y, bits_of(p.mat), bits_of(p.type)};
    o.spheres |= p.type != kTri;
  }
  o.lights = s.lights;
  o.mats = s.mats;
  if (o.mats.empty()) o.mats.push_back(Material{});

  o.max_stack = std::max(1, s.max_stack);
  int max_leaf = 0;
  for (const KdNode& k : s.nodes)
    if (k.axis < 0) max_leaf = std::max(max_leaf, k.count);
  o.narrow = nn <= 65536 && static_cast<int64_t>(max_leaf) * 64 * wrd::kLeavesPerRound < 65536;
  o.walk_wave = nn < (size_t(1) << 26) && s.dep_max <= 43 &&
                static_cast<size_t>(max_leaf) < (size_t(1) << (64 - std::max(s.dep_max, 0)));
}

}  // namespace wr
