// CPU check of the ray slab's carving (csrc/wr_queue_slab.h) by
// itself: for each case every segment lies inside the slab, no two overlap,
// every base is a multiple of 64 entries, a segment holds its capacity, and
// the plane stride is the slab's entries.  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wr_queue_slab.h"

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      std::exit(1);                                              \
    }                                                            \
  } while (0)

struct Seg {
  long long b, e;  // [b, e)
};

static void check_case(int members, int cap_sq, int cap_ext) {
  const wr::QueueSlabLayout L = wr::queue_slab_layout(members, cap_sq, cap_ext);
  CHECK(L.stride > 0);
  CHECK(L.members == members && L.cap_sq == cap_sq && L.cap_ext == cap_ext);
  std::vector<Seg> segs;
  for (int m = 0; m < members; ++m) {
    CHECK(L.sq_base[m] % 64 == 0 && L.ext_base[m] % 64 == 0);
    segs.push_back({L.sq_base[m], static_cast<long long>(L.sq_base[m]) + cap_sq});
    segs.push_back({L.ext_base[m], static_cast<long long>(L.ext_base[m]) + cap_ext});
  }
  long long entries = 0;  // what the segments need, each rounded to whole waves
  for (const Seg& s : segs) {
    CHECK(s.b >= 0 && s.e <= L.stride);  // inside the slab (a plane of the 3-plane arrays)
    entries += (s.e - s.b + 63) / 64 * 64;
  }
  for (size_t i = 0; i < segs.size(); ++i)
    for (size_t j = i + 1; j < segs.size(); ++j) CHECK(segs[i].e <= segs[j].b || segs[j].e <= segs[i].b);  // disjoint
  CHECK(L.stride == entries);  // the stride is the slab's entries: no room beyond the segments
  CHECK(3LL * L.stride <= 2147483647LL);
  // launch order is slab order: a set's shadow / aux segment, its extension segment, the next set's
  for (int m = 0; m < members; ++m) {
    CHECK(L.sq_base[m] < L.ext_base[m] || cap_sq == 0);
    if (m + 1 < members) CHECK(L.ext_base[m] <= L.sq_base[m + 1]);
  }
}

int main() {
  // one member, two members; cap_sq smaller and larger than the extension queue
  check_case(1, 704, 1920);     // cap_sq < qs (pools: 40 x 24 paths, 2 P extension entries)
  check_case(1, 10560, 1920);   // cap_sq > qs (the worst case: 11 per path)
  check_case(2, 704, 1920);
  check_case(2, 10560, 1920);
  check_case(2, 1000, 1000);    // equal, neither a multiple of 64
  check_case(2, 1, 63);         // less than a wave each
  check_case(2, 64, 64);        // exactly a wave
  check_case(2, 65, 129);
  check_case(2, 0, 960);        // an empty shadow segment
  check_case(8, 2 * 2073600, 2 * 2073600);  // eight sets of a 1080p film
  check_case(2, 11 * 2073600, 2 * 2073600);  // 1080p, the worst case
  // out of range: no layout (stride 0)
  CHECK(wr::queue_slab_layout(0, 64, 64).stride == 0);
  CHECK(wr::queue_slab_layout(wr::kSlabMaxMembers + 1, 64, 64).stride == 0);
  CHECK(wr::queue_slab_layout(2, -1, 64).stride == 0);
  CHECK(wr::queue_slab_layout(2, 0, 0).stride == 0);
  CHECK(wr::queue_slab_layout(2, 400000000, 64).stride == 0);  // 3 x stride past INT_MAX
  CHECK(wr::queue_slab_layout(1, 2147483647, 2147483647).stride == 0);
  CHECK(wr::queue_slab_layout(2, 357913921, 0).stride == 0);   // 3 x 715,827,968 > INT_MAX
  CHECK(wr::queue_slab_layout(1, 715827840, 0).stride == 715827840);  // 3 x stride = 2,147,483,520: the last that fits
  std::printf("OK\n");
  return 0;
}
