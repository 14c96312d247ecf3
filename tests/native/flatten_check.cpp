// Check of the flattened scene (wr_flatten.cpp) against wr::Scene, CPU only:
// built and run by tests/test_flatten_host.py.  What is expected is derived
// from the scene by another route than the code under test: node words are
// packed here, the multi-level records are followed down the child links
// recursively.  Prints "OK <stats>" or the first violated property and exits
// non-zero.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wr_flatten.h"
#include "wr_scene.h"

static int fail(const std::string& m) {
  std::printf("FAIL %s\n", m.c_str());
  return 1;
}

struct Word {
  uint32_t x, y;
  bool operator==(const Word& o) const { return x == o.x && y == o.y; }
};

static uint32_t fbits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static int ibits(float f) {
  int i;
  std::memcpy(&i, &f, 4);
  return i;
}

// the packed word of node n (wr_traverse.h:6-8); n < 0: below a leaf
static Word packed(const wr::Scene& s, int64_t n) {
  if (n < 0) return Word{0u, 0u};
  const wr::KdNode& k = s.nodes[static_cast<size_t>(n)];
  if (k.axis >= 0) return Word{fbits(k.split), (static_cast<uint32_t>(k.right) << 2) | static_cast<uint32_t>(k.axis)};
  return Word{static_cast<uint32_t>(k.first), (static_cast<uint32_t>(k.count) << 2) | 3u};
}

// the node reached from n by heap entry h's path: the entry's parent first,
// then left (odd h) or right (even h); -1 below a leaf
static int64_t descend(const wr::Scene& s, int64_t n, int h) {
  if (h == 0) return n;
  const int64_t up = descend(s, n, (h - 1) / 2);
  if (up < 0 || s.nodes[static_cast<size_t>(up)].axis < 0) return -1;
  return (h & 1) ? up + 1 : s.nodes[static_cast<size_t>(up)].right;
}

static bool same_bits(float a, float b) { return fbits(a) == fbits(b); }

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: flatten_check scene");
  wr::Scene s;
  std::string err;
  if (!wr::load_scene(argv[1], s, err)) return fail("load: " + err);
  wr::SceneFlat f;
  wr::flatten_scene(s, f);
  const size_t nn = s.nodes.size(), nr = s.refs.size(), np = s.prims.size();
  const size_t u4 = static_cast<size_t>(wrd::kRecU4);
  if (f.nrec.size() != nn || f.nrec_r.size() != nn || f.nrec3.size() != u4 * nn) return fail("node array sizes");
  if (f.ref_a.size() != nr || f.ref_b.size() != nr || f.ref_c.size() != nr) return fail("reference array sizes");
  if (f.prim_mat.size() != np || f.prim_type.size() != np || f.prim_tri.size() != np || f.prim_tri2.size() != np ||
      f.prim_sph.size() != np || f.prim_sbox0.size() != np || f.prim_sbox1.size() != np || f.prim_rec.size() != 2 * np)
    return fail("primitive array sizes");

  // 1. node records: (self, left), (right); inner / leaf words; leaves have no children
  const int ent = (1 << wrd::kRecLevels) - 1;
  if (static_cast<size_t>(2 * ent) > 4 * u4) return fail("a record does not hold its entries");
  size_t inner = 0;
  for (size_t i = 0; i < nn; ++i) {
    const wr::KdNode& k = s.nodes[i];
    const bool in = k.axis >= 0;
    inner += in ? 1 : 0;
    const std::string at = " at node " + std::to_string(i);
    if (in && (k.axis > 2 || k.right <= static_cast<int>(i) + 1 || static_cast<size_t>(k.right) >= nn))
      return fail("scene: bad inner node" + at);
    const Word self = packed(s, static_cast<int64_t>(i));
    if ((self.y & 3u) != (in ? static_cast<uint32_t>(k.axis) : 3u)) return fail("axis / leaf tag" + at);
    const Word l = in ? packed(s, static_cast<int64_t>(i) + 1) : Word{0u, 0u};
    const Word r = in ? packed(s, k.right) : Word{0u, 0u};
    const wr::U4& a = f.nrec[i];
    if (!(Word{a.x, a.y} == self)) return fail("nrec self" + at);
    if (!(Word{a.z, a.w} == l)) return fail("nrec left child" + at);
    if (!(Word{f.nrec_r[i].x, f.nrec_r[i].y} == r)) return fail("nrec_r right child" + at);
    // 2. multi-level record: entry h = the packed node the path h leads to
    std::vector<uint32_t> w(4 * u4);
    std::memcpy(w.data(), &f.nrec3[u4 * i], 16 * u4);
    for (int h = 0; h < ent; ++h) {
      const Word want = packed(s, descend(s, static_cast<int64_t>(i), h));
      if (!(Word{w[2 * h], w[2 * h + 1]} == want)) return fail("nrec3 entry " + std::to_string(h) + at);
    }
    for (size_t x = static_cast<size_t>(2 * ent); x < 4 * u4; ++x)
      if (w[x] != 0u) return fail("nrec3 padding" + at);
  }

  // 3. reference records: primitive index and Triangle::hit's A..F (triangle.cpp:24-30)
  for (size_t i = 0; i < nr; ++i) {
    const int pi = s.refs[i];
    if (pi < 0 || static_cast<size_t>(pi) >= np) return fail("scene: bad reference");
    const wr::Prim& p = s.prims[static_cast<size_t>(pi)];
    const std::string at = " at reference " + std::to_string(i);
    const int got = ibits(f.ref_c[i].y);
    const wr::F4 &a = f.ref_a[i], &b = f.ref_b[i];
    if (p.type == wr::kTri) {
      if (got != pi) return fail("triangle index" + at);
      const float want[9] = {p.p0.x, p.p0.y, p.p0.z, p.p0.x - p.p1.x, p.p0.y - p.p1.y, p.p0.z - p.p1.z,
                             p.p0.x - p.p2.x, p.p0.y - p.p2.y, p.p0.z - p.p2.z};
      const float have[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, f.ref_c[i].x};
      if (std::memcmp(want, have, sizeof want) != 0) return fail("triangle terms" + at);
    } else {
      if (got != -(pi + 1)) return fail("sphere index" + at);
      const float have[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, f.ref_c[i].x};
      for (float v : have)
        if (fbits(v) != 0u) return fail("sphere record not zero" + at);
    }
  }

  // 4. per-primitive arrays and the 32-byte record
  bool spheres = false;
  for (size_t i = 0; i < np; ++i) {
    const wr::Prim& p = s.prims[i];
    const std::string at = " at primitive " + std::to_string(i);
    spheres = spheres || p.type != wr::kTri;
    const float tri[6] = {p.p0.x - p.p1.x, p.p0.y - p.p1.y, p.p0.z - p.p1.z,
                          p.p0.x - p.p2.x, p.p0.y - p.p2.y, p.p0.z - p.p2.z};
    const wr::F4& t = f.prim_tri[i];
    const wr::F2& t2 = f.prim_tri2[i];
    const float have[6] = {t.x, t.y, t.z, t.w, t2.x, t2.y};
    if (std::memcmp(tri, have, sizeof tri) != 0) return fail("prim_tri / prim_tri2" + at);
    if (f.prim_mat[i] != p.mat || f.prim_type[i] != p.type) return fail("material / type" + at);
    const wr::F4 &r0 = f.prim_rec[2 * i], &r1 = f.prim_rec[2 * i + 1];
    if (std::memcmp(&r0, &t, sizeof t) != 0) return fail("prim_rec[2i] is not prim_tri" + at);
    if (!same_bits(r1.x, t2.x) || !same_bits(r1.y, t2.y)) return fail("prim_rec[2i+1] is not prim_tri2" + at);
    if (ibits(r1.z) != p.mat || ibits(r1.w) != p.type) return fail("prim_rec material / type bits" + at);
    const float sph[4] = {p.c.x, p.c.y, p.c.z, p.r}, box[6] = {p.bl.x, p.bl.y, p.bl.z, p.br.x, p.br.y, p.br.z};
    const wr::F4& b0 = f.prim_sbox0[i];
    const float hbox[6] = {b0.x, b0.y, b0.z, b0.w, f.prim_sbox1[i].x, f.prim_sbox1[i].y};
    if (std::memcmp(sph, &f.prim_sph[i], sizeof sph) != 0) return fail("prim_sph" + at);
    if (std::memcmp(box, hbox, sizeof box) != 0) return fail("prim_sbox0 / prim_sbox1" + at);
  }

  // 5. lights, materials, and the facts derived from the counts
  if (f.lights.size() != s.lights.size() ||
      (!s.lights.empty() && std::memcmp(f.lights.data(), s.lights.data(), s.lights.size() * sizeof(wr::Light)) != 0))
    return fail("lights");
  if (f.mats.size() != std::max<size_t>(1, s.mats.size()) ||
      (!s.mats.empty() && std::memcmp(f.mats.data(), s.mats.data(), s.mats.size() * sizeof(wr::Material)) != 0))
    return fail("materials");
  if (f.spheres != spheres) return fail("spheres");
  if (f.max_stack != std::max(1, s.max_stack)) return fail("max_stack");
  int64_t max_leaf = 0;
  for (const wr::KdNode& k : s.nodes)
    if (k.axis < 0) max_leaf = std::max<int64_t>(max_leaf, k.count);
  const bool narrow = nn <= 65536 && max_leaf * 64 * wrd::kLeavesPerRound < 65536;
  if (f.narrow != narrow) return fail("narrow");
  // every leaf holds fewer than 2^(64 - dep_max) references
  const bool walk = nn < (size_t(1) << 26) && s.dep_max <= 43 &&
                    static_cast<uint64_t>(max_leaf) < (uint64_t(1) << (64 - std::max(s.dep_max, 0)));
  if (f.walk_wave != walk) return fail("walk_wave");
  std::printf("OK nodes %zu (inner %zu) refs %zu prims %zu lights %zu levels %d narrow %d walk_wave %d spheres %d\n", nn,
              inner, nr, np, s.lights.size(), wrd::kRecLevels, narrow ? 1 : 0, walk ? 1 : 0, spheres ? 1 : 0);
  return 0;
}
