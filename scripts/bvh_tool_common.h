// What the CPU tools that walk the search's BVH share (bvh_cost.cpp,
// search_round_model.cpp): the vector helpers, the triangle test on the
// search's records, and the secondary rays -- random surface points
// (area-weighted), cosine directions about either side's normal.  One text, so
// that the tools keep the same walk inputs.
#pragma once
#include <algorithm>
#include <cmath>
#include <random>
#include <vector>

#include "wr_bvh.h"
#include "wr_scene.h"

namespace bvhtool {
constexpr float kEps = 1e-3f;

struct V {
  float x, y, z;
};
inline V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V add(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V mul(V a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline V norm(V a) { return mul(a, 1.f / std::sqrt(dot(a, a))); }
inline V f3(wr::F3 p) { return {p.x, p.y, p.z}; }

inline bool tri(const wrf::TriRec& r, V o, V d, float& t) {
  const V p0{r.a[0], r.a[1], r.a[2]};
  const V e1{-r.a[3], -r.b[0], -r.b[1]}, e2{-r.b[2], -r.b[3], -r.c[0]};
  const V pv = cross(d, e2);
  const float det = dot(e1, pv);
  if (std::fabs(det) < 1e-12f) return false;
  const float inv = 1.f / det;
  const V tv = sub(o, p0);
  const float u = dot(tv, pv) * inv;
  if (u < -kEps || u > 1.f) return false;
  const V qv = cross(tv, e1);
  const float v = dot(d, qv) * inv;
  if (v < -kEps || u + v > 1.f) return false;
  t = dot(e2, qv) * inv;
  return t > kEps;
}

// area-weighted triangle pick: the running sum of the triangles' areas (returns the total)
inline double area_cdf(const wr::Scene& s, std::vector<double>& cdf) {
  cdf.resize(s.prims.size());
  double acc = 0;
  for (size_t i = 0; i < s.prims.size(); ++i) {
    const auto& p = s.prims[i];
    const V c = cross(sub(f3(p.p1), f3(p.p0)), sub(f3(p.p2), f3(p.p0)));
    acc += 0.5 * std::sqrt(dot(c, c));
    cdf[i] = acc;
  }
  return acc;
}

// secondary ray: random surface point, cosine direction about a random side's normal (7 draws of U)
inline void secondary_ray(const wr::Scene& s, const std::vector<double>& cdf, double acc, std::mt19937& rng,
                          std::uniform_real_distribution<float>& U, V& org, V& dir) {
  const double x = U(rng) * acc;
  const size_t k = static_cast<size_t>(std::lower_bound(cdf.begin(), cdf.end(), x) - cdf.begin());
  const auto& p = s.prims[std::min(k, s.prims.size() - 1)];
  float u = U(rng), v = U(rng);
  if (u + v > 1.f) {
    u = 1.f - u;
    v = 1.f - v;
  }
  const V e1 = sub(f3(p.p1), f3(p.p0)), e2 = sub(f3(p.p2), f3(p.p0));
  V n = norm(cross(e1, e2));
  if (U(rng) < 0.5f) n = mul(n, -1.f);
  const V t1 = norm(std::fabs(n.x) > 0.5f ? cross(n, V{0, 1, 0}) : cross(n, V{1, 0, 0})), t2 = cross(n, t1);
  const float r1 = U(rng), r2 = U(rng), rr = std::sqrt(r1), ph = 6.2831853f * r2;
  dir = norm(add(mul(n, std::sqrt(1.f - r1)), add(mul(t1, rr * std::cos(ph)), mul(t2, rr * std::sin(ph)))));
  org = add(add(add(f3(p.p0), mul(e1, u)), mul(e2, v)), mul(dir, kEps));
}
}  // namespace bvhtool
