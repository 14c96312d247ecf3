// The top-first node order of the verified BVH (wrf::build_fast's top / top4
// budgets, wr_bvh.h) against the build-order trees of the same scene, CPU only:
// built and run by tests/test_bvh_top_host.py.  Prints "OK <stats>" or the
// first violated property and exits non-zero.
//   usage: bvh_top_check scene top top4
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "wr_bvh.h"
#include "wr_scene.h"

static int fail(const std::string& m) {
  std::printf("FAIL %s\n", m.c_str());
  return 1;
}

static int slots(const wrf::BNode&) { return 2; }
static int slots(const wrf::BNode4&) { return 4; }
// a node's boxes, bit for bit
static bool same_boxes(const wrf::BNode& a, const wrf::BNode& b) { return std::memcmp(a.b, b.b, sizeof a.b) == 0; }
static bool same_boxes(const wrf::BNode4& a, const wrf::BNode4& b) {
  return std::memcmp(a.lo, b.lo, sizeof a.lo) == 0 && std::memcmp(a.hi, b.hi, sizeof a.hi) == 0;
}

// `was`: the tree in build order; `now`: the same build with the top budget
template <class Node>
static std::string check(const std::vector<Node>& was, const std::vector<Node>& now, int ntop, int budget,
                         const char* name) {
  const std::string T = std::string(name) + ": ";
  const int n = static_cast<int>(now.size());
  if (was.size() != now.size()) return T + "node count changed";
  if (ntop != std::min(budget, n)) return T + "ntop " + std::to_string(ntop) + " is not min(budget, node count)";
  if (n == 0) return "";
  // every inner link in range and reached exactly once; the root by none
  std::vector<int> parent(static_cast<size_t>(n), -1), refs(static_cast<size_t>(n), 0);
  std::vector<int> leaves_now, leaves_was;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < slots(now[static_cast<size_t>(i)]); ++k) {
      const int l = now[static_cast<size_t>(i)].c[k];
      if (l < 0) {
        leaves_now.push_back(l);
        continue;
      }
      if (l >= n) return T + "inner link out of range";
      ++refs[static_cast<size_t>(l)];
      parent[static_cast<size_t>(l)] = i;
    }
  if (refs[0] != 0) return T + "the root is some node's child";
  for (int i = 1; i < n; ++i)
    if (refs[static_cast<size_t>(i)] != 1)
      return T + "node " + std::to_string(i) + " is linked " + std::to_string(refs[static_cast<size_t>(i)]) + " times";
  // [0, ntop) parent-closed, the root at 0
  for (int i = 1; i < ntop; ++i)
    if (parent[static_cast<size_t>(i)] >= ntop) return T + "top node " + std::to_string(i) + " has its parent outside the top set";
  // the multiset of leaf links
  for (const Node& nd : was)
    for (int k = 0; k < slots(nd); ++k)
      if (nd.c[k] < 0) leaves_was.push_back(nd.c[k]);
  std::sort(leaves_now.begin(), leaves_now.end());
  std::sort(leaves_was.begin(), leaves_was.end());
  if (leaves_now != leaves_was) return T + "leaf links differ from the build-order tree's";
  // the same tree: walked from the two roots together, each node's boxes equal
  // its old self's bit for bit, leaf links in the same slots, every node met once
  std::vector<char> met(static_cast<size_t>(n), 0);
  std::vector<std::pair<int, int>> st{{0, 0}};
  int visited = 0;
  while (!st.empty()) {
    const auto [ia, ib] = st.back();
    st.pop_back();
    if (met[static_cast<size_t>(ib)]) return T + "node met twice";
    met[static_cast<size_t>(ib)] = 1;
    ++visited;
    const Node& a = was[static_cast<size_t>(ia)];
    const Node& b = now[static_cast<size_t>(ib)];
    if (!same_boxes(a, b)) return T + "boxes of node " + std::to_string(ib) + " differ from its old self's";
    for (int k = 0; k < slots(a); ++k) {
      if ((a.c[k] < 0) != (b.c[k] < 0)) return T + "a leaf link became an inner one";
      if (a.c[k] < 0) {
        if (a.c[k] != b.c[k]) return T + "leaf link changed";
      } else {
        st.push_back({a.c[k], b.c[k]});
      }
    }
  }
  if (visited != n) return T + "nodes unreachable from the root";
  return "";
}

int main(int argc, char** argv) {
  if (argc < 4) return fail("usage: bvh_top_check scene top top4");
  const int top = std::atoi(argv[2]), top4 = std::atoi(argv[3]);
  wr::Scene s;
  std::string err;
  if (!wr::load_scene(argv[1], s, err)) return fail("load: " + err);
  wrf::FastHost was, now;
  wrf::build_fast(s, was, 2, true, 0, 0);
  wrf::build_fast(s, now, 2, true, top, top4);
  if (!was.ok || !now.ok) return fail("build refused: " + was.why + now.why);
  if (was.ntop != 0 || was.ntop4 != 0) return fail("a zero budget still made a top set");
  std::string e = check(was.nodes, now.nodes, now.ntop, top, "binary tree");
  if (!e.empty()) return fail(e);
  e = check(was.nodes4, now.nodes4, now.ntop4, top4, "4-wide tree");
  if (!e.empty()) return fail(e);
  // nothing else moved: triangle records and the KD membership data
  if (was.tris.size() != now.tris.size() ||
      std::memcmp(was.tris.data(), now.tris.data(), was.tris.size() * sizeof(wrf::TriRec)) != 0)
    return fail("triangle records changed");
  if (was.prim_leaf_off != now.prim_leaf_off || was.prim_leaf != now.prim_leaf || was.prim_leaf_pos != now.prim_leaf_pos ||
      was.path != now.path || was.node_path != now.node_path)
    return fail("KD membership data changed");
  if (was.depth != now.depth || was.depth4 != now.depth4 || was.leaves != now.leaves) return fail("depth or leaf count changed");
  std::printf("OK nodes %zu ntop %d nodes4 %zu ntop4 %d\n", now.nodes.size(), now.ntop, now.nodes4.size(), now.ntop4);
  return 0;
}
