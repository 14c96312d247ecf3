// CPU model of the BVH search's outer rounds (wr_fast.h trace_fast, WR_BVH_SPEC):
// what the rule that ends a round's node loop costs and saves, before GPU time
// is spent on it (DESIGN.md 4b "When a round ends").  Rays are packed into
// 64-lane waves that run the kernel's round: refill the idle lanes, step inner
// nodes -- a lane that reaches a leaf parks it and descends on under its stale
// bound -- until at most K lanes still lack a leaf, test the parked leaves,
// retire the finished rays.  K = (active lanes * num) >> shift, 0 for a wave
// with fewer than 16 active lanes, as kStragglerNum / kStragglerShift.
// The walk is scripts/bvh_cost.cpp's (binary tree, nearer child first, window
// t1 + 2 EPS, no per-ray margins), one step at a time; the rays are its
// secondary rays (random surface points, cosine directions about either side).
// Weights: wave-level VALU instructions per node-loop iteration, leaf phase,
// refill and finish block, read from the gfx950 listing of
// k_trace_fast<false, 2, false, true, true> (48 / 330 / 140 / 35); a block is
// charged when any lane runs it.  No memory latency, no camera rays, no settle
// batches: a direction and a rough size, not a measurement.
// Build: g++ -O2 -std=c++17 -I winmad-s-raytracer-v1.0_amd/csrc -I include
//   -I scripts scripts/search_round_model.cpp winmad-s-raytracer-v1.0_amd/csrc/{wr_scene,wr_bvh}.cpp -lpthread
// Usage: search_round_model scene [rays [rays_per_lane]]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "bvh_tool_common.h"
#include "wr_bvh.h"
#include "wr_scene.h"

namespace {
using namespace bvhtool;  // kEps, V and its helpers, tri(), the secondary rays
constexpr int kDone = 0x7fffffff;
constexpr double kNodeValu = 48, kLeafValu = 330, kRefillValu = 140, kFinishValu = 35;

struct Ray {
  V o, d;
};

// one lane of the search: trace_fast's cur / pl / stack, stepped by the wave
struct Lane {
  bool act = false;
  V o{}, d{}, inv{};
  float t1 = INFINITY;
  struct E {
    int link;
    float t;
  } st[128];
  int sp = 0, cur = 0, pl = 0;
  float hi() const { return t1 + 2.f * kEps; }
  void start(const Ray& r) {
    act = true;
    o = r.o;
    d = r.d;
    inv = {1.f / d.x, 1.f / d.y, 1.f / d.z};
    t1 = INFINITY;
    sp = 0;
    cur = 0;
    pl = 0;
  }
  void pop() {
    cur = kDone;
    while (sp > 0) {
      --sp;
      if (st[sp].t <= hi()) {
        cur = st[sp].link;
        break;
      }
    }
  }
  bool slab(const float* b, float& tn) const {
    const float x0 = (b[0] - o.x) * inv.x, x1 = (b[3] - o.x) * inv.x;
    const float y0 = (b[1] - o.y) * inv.y, y1 = (b[4] - o.y) * inv.y;
    const float z0 = (b[2] - o.z) * inv.z, z1 = (b[5] - o.z) * inv.z;
    tn = std::fmax(std::fmax(std::fmin(x0, x1), std::fmin(y0, y1)), std::fmax(std::fmin(z0, z1), 0.f));
    const float tf = std::fmin(std::fmin(std::fmax(x0, x1), std::fmax(y0, y1)), std::fmin(std::fmax(z0, z1), hi()));
    return tn <= tf;
  }
  void node(const wrf::FastHost& F) {
    const wrf::BNode& n = F.nodes[static_cast<size_t>(cur)];
    float ta, tb;
    const bool ha = slab(n.b, ta), hb = slab(n.b + 6, tb);
    if (ha && hb) {
      const bool af = ta <= tb;
      st[sp++] = {af ? n.c[1] : n.c[0], af ? tb : ta};
      cur = af ? n.c[0] : n.c[1];
    } else if (ha || hb) {
      cur = ha ? n.c[0] : n.c[1];
    } else {
      pop();
    }
  }
  void leaf(const wrf::FastHost& F) {
    const int l = ~pl, first = l >> 3, cnt = (l & 7) + 1;
    pl = 0;
    for (int j = 0; j < cnt; ++j) {
      float t;
      if (tri(F.tris[static_cast<size_t>(first + j)], o, d, t) && t < t1) t1 = t;
    }
  }
};

struct Tally {
  double rays = 0, rounds = 0, iters = 0, step_lanes = 0, leaf_phases = 0, leaf_lanes = 0, refills = 0, finishes = 0,
         carried = 0;
  double valu() const {
    return kNodeValu * iters + kLeafValu * leaf_phases + kRefillValu * refills + kFinishValu * finishes;
  }
};

// one wave over rays [begin, end), the round as trace_fast runs it
void wave(const wrf::FastHost& F, const std::vector<Ray>& rays, size_t begin, size_t end, int num, int shift, Tally& T) {
  Lane lane[64];
  size_t next = begin;
  bool pool = true;
  for (;;) {
    if (pool) {
      bool any = false;
      for (Lane& L : lane)
        if (!L.act) {
          any = true;
          if (next < end) L.start(rays[next++]);
          else pool = false;
        }
      if (any) T.refills += 1;
    }
    int nact = 0;
    for (const Lane& L : lane) nact += L.act;
    if (nact == 0) {
      if (!pool) break;
      continue;
    }
    const int late = nact < 16 ? 0 : (nact * num) >> shift;
    for (;;) {
      int lacking = 0;
      for (const Lane& L : lane) lacking += L.act && L.pl >= 0 && L.cur != kDone;
      if (lacking <= late) break;
      T.iters += 1;
      for (Lane& L : lane) {
        if (L.act && L.cur < 0 && L.pl >= 0) {
          L.pl = L.cur;
          L.pop();
        }
        if (L.act && L.cur >= 0 && L.cur != kDone) {
          T.step_lanes += 1;
          L.node(F);
        }
      }
    }
    int leaves = 0, fin = 0;
    for (Lane& L : lane) {
      if (L.act && L.pl >= 0 && L.cur != kDone) T.carried += 1;
      if (L.act && L.pl < 0) {
        ++leaves;
        L.leaf(F);
      }
    }
    for (Lane& L : lane)
      if (L.act && L.cur == kDone && L.pl >= 0) {
        ++fin;
        L.act = false;
      }
    T.rounds += 1;
    T.leaf_lanes += leaves;
    if (leaves) T.leaf_phases += 1;
    if (fin) T.finishes += 1;
  }
  T.rays += static_cast<double>(end - begin);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: search_round_model scene [rays [rays_per_lane]]\n");
    return 2;
  }
  const int nrays = argc > 2 ? std::atoi(argv[2]) : 400000;
  const int per_lane = argc > 3 ? std::atoi(argv[3]) : 16;
  wr::Scene s;
  std::string err;
  if (!wr::load_scene(argv[1], s, err)) {
    std::fprintf(stderr, "load: %s\n", err.c_str());
    return 1;
  }
  wrf::FastHost F;
  wrf::build_fast(s, F);
  if (!F.ok) {
    std::fprintf(stderr, "build refused: %s\n", F.why.c_str());
    return 1;
  }
  std::mt19937 rng(12345);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  std::vector<double> cdf;
  const double acc = area_cdf(s, cdf);
  // secondary rays: random surface point, cosine direction about a random side's normal
  std::vector<Ray> rays(static_cast<size_t>(nrays));
  for (Ray& r : rays) secondary_ray(s, cdf, acc, rng, U, r.o, r.d);
  std::printf("%d secondary rays, %d per lane (%d per wave); VALU weights: node iteration %.0f, leaf phase %.0f, "
              "refill %.0f, finish %.0f\n",
              nrays, per_lane, 64 * per_lane, kNodeValu, kLeafValu, kRefillValu, kFinishValu);
  std::printf("| fraction (K of 64) | iterations per round | rounds per 64 rays | node-loop lane use | leaf-phase lane use | "
              "carried lanes per round | model VALU per 64 rays |\n|---|---|---|---|---|---|---|\n");
  const int fr[][2] = {{0, 0}, {1, 5}, {1, 4}, {1, 3}, {1, 2}};
  double base = 0;
  for (const auto& f : fr) {
    Tally T;
    const size_t chunk = static_cast<size_t>(64) * static_cast<size_t>(per_lane);
    for (size_t b = 0; b < rays.size(); b += chunk) wave(F, rays, b, std::min(rays.size(), b + chunk), f[0], f[1], T);
    const double per64 = T.valu() * 64.0 / T.rays;
    if (f[0] == 0) base = per64;
    char name[32];
    if (f[0] == 0) std::snprintf(name, sizeof name, "0 (0)");
    else std::snprintf(name, sizeof name, "%d/%d (%d)", f[0], 1 << f[1], (64 * f[0]) >> f[1]);
    std::printf("| %s | %.1f | %.2f | %.2f | %.2f | %.2f | %.0f (%+.1f %%) |\n", name, T.iters / T.rounds,
                T.rounds * 64.0 / T.rays, T.step_lanes / (64.0 * T.iters), T.leaf_lanes / (64.0 * T.leaf_phases),
                T.carried / T.rounds, per64, 100.0 * (per64 / base - 1.0));
  }
  return 0;
}
