// The device-array argument checker of csrc/wr_args.h by itself, with a fake
// pointer classifier over a small address map (tests/test_args_host.py).
// Every rule of the checker is driven with the smallest input that can break
// it; the classifier records every address it is asked about.
#include <cstdio>
#include <string>
#include <vector>

#include "wr_args.h"

namespace {

// the address map: [lo, hi) -> what the memory is; everything else is a failed query
struct Block {
  uintptr_t lo, hi;
  bool device;
  int dev;
};
const uintptr_t kD0a = 0x10000, kD0b = 0x20000, kD1 = 0x30000, kHost = 0x40000, kPinned = 0x50000, kLen = 0x100;
const Block kMap[] = {{kD0a, kD0a + kLen, true, 0},    {kD0b, kD0b + kLen, true, 0},      {kD1, kD1 + kLen, true, 1},
                      {kHost, kHost + kLen, false, 0}, {kPinned, kPinned + kLen, false, 0}};
const char* kHint = "the_host_call";

std::vector<uintptr_t> asked;
wr::PtrClass classify(const void* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  asked.push_back(a);
  for (const Block& b : kMap)
    if (a >= b.lo && a < b.hi) return {true, b.device, b.dev};
  return {false, false, -1};
}
const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL %s\n", what);
    ++failures;
  }
}
bool has(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }

wr::ArgError run(std::initializer_list<wr::Arg> args, int device = 0) {
  asked.clear();
  return wr::check_args("the_call", args, device, kHint, classify);
}
// refused with WR_E_ARG, the call's name and every one of `words` in the message
bool refused(const wr::ArgError& e, std::initializer_list<const char*> words) {
  bool ok = e.code == WR_E_ARG && has(e.msg, "the_call");
  for (const char* w : words) ok = ok && has(e.msg, w);
  if (!ok) std::printf("  (code %d, message \"%s\")\n", e.code, e.msg.c_str());
  return ok;
}
bool passed(const wr::ArgError& e) {
  if (e.code != WR_OK || !e.msg.empty()) std::printf("  (code %d, message \"%s\")\n", e.code, e.msg.c_str());
  return e.code == WR_OK && e.msg.empty();
}

}  // namespace

int main() {
  using wr::in;
  using wr::out;

  // ---- null and empty
  expect(refused(run({in(at(kD0a), 16, "a"), out(nullptr, 16, "b")}), {"null", "b"}) && asked.empty(),
         "a null required argument is refused, nothing classified");
  expect(passed(run({in(nullptr, 16, "a", 1, true), out(at(kD0a), 16, "b")})) && asked.size() == 2,
         "a null optional argument passes and is not classified");
  expect(passed(run({in(nullptr, 0, "a"), out(at(kD0a), 16, "b")})) && asked.size() == 2,
         "a null argument of 0 bytes passes");

  // ---- alignment
  expect(refused(run({in(at(kD0a + 4), 16, "a", 8)}), {"aligned", "a", "8"}) && asked.empty(),
         "off by 4 for an 8-byte argument is refused, nothing classified");
  expect(passed(run({in(at(kD0a + 8), 16, "a", 8)})), "an aligned argument passes");
  expect(refused(run({in(at(kD0a + 2), 0, "a", 4)}), {"aligned", "a"}) && asked.empty(),
         "a non-null pointer meets its alignment even with 0 bytes");

  // ---- classification
  expect(passed(run({in(at(kD0a + 7), 1, "a")})) && asked == std::vector<uintptr_t>{kD0a + 7, kD0a + 7},
         "a 1-byte array classifies its one address twice");
  expect(passed(run({in(at(kD0a + 3), 40, "a")})) && asked == std::vector<uintptr_t>{kD0a + 3, kD0a + 42},
         "an n-byte array classifies exactly its first and its last byte");
  expect(passed(run({in(at(kD0a), kLen, "a")})), "an array that fills its block passes");
  expect(passed(run({in(at(kD0a + 2), 0, "a")})) && asked.empty(), "an empty array is not classified");
  expect(refused(run({in(at(kD0a + kLen - 4), 5, "a")}), {"a", "not device memory"}) && asked.size() == 2,
         "first byte in a device block, last byte past it: refused");
  expect(refused(run({in(at(kD0a - 1), 2, "a")}), {"a", "not device memory"}) && asked.size() == 1,
         "first byte before a device block: refused at the first query");
  expect(refused(run({in(at(kHost), 16, "h")}), {"h", "not device memory", kHint}), "a host array is refused with the hint");
  expect(refused(run({in(at(kPinned), 16, "p")}), {"p", "not device memory", kHint}),
         "a pinned array is refused with the hint");
  expect(refused(run({in(at(0x90000), 16, "u")}), {"u", "not device memory", kHint}),
         "an address nobody knows is refused with the hint");
  expect(refused(run({in(at(kD1), 16, "a")}, 0), {"a", "device 1", "on device 0"}),
         "a device-1 array with the context on device 0 is refused, both devices named");
  expect(passed(run({in(at(kD1), 16, "a")}, 1)), "a device-1 array with the context on device 1 passes");
  expect(refused(run({in(at(kD0a), 16, "a")}, 1), {"a", "device 0", "on device 1"}),
         "a device-0 array with the context on device 1 is refused");

  // ---- overlap
  expect(refused(run({in(at(kD0a), 16, "a"), out(at(kD0a + 15), 16, "b")}), {"a", "overlaps", "b"}),
         "an output over the last byte of an input is refused, both named");
  expect(refused(run({out(at(kD0a + 15), 16, "b"), in(at(kD0a), 16, "a")}), {"a", "overlaps", "b"}),
         "the same with the output first");
  expect(refused(run({out(at(kD0a), 16, "a"), out(at(kD0a + 8), 16, "b")}), {"a", "overlaps", "b"}),
         "output over output is refused");
  expect(refused(run({in(at(kD0a), 64, "a"), out(at(kD0a + 8), 1, "b")}), {"a", "overlaps", "b"}),
         "a 1-byte output inside an input is refused");
  expect(passed(run({in(at(kD0a), 16, "a"), in(at(kD0a), 16, "b"), out(at(kD0b), 16, "c")})),
         "two inputs that share memory pass");
  expect(passed(run({in(at(kD0a), 16, "a"), out(at(kD0a + 16), 16, "b")})),
         "an output that starts where an input ends passes");
  expect(passed(run({out(at(kD0a), 16, "b"), in(at(kD0a + 16), 16, "a")})),
         "an output that ends where an input starts passes");
  expect(passed(run({in(at(kD0a), 16, "a"), out(at(kD0a + 8), 0, "b")})), "a zero-byte output inside an input passes");
  expect(passed(run({in(at(kD0a), 16, "a"), out(at(kD0b), 16, "b"), out(nullptr, 16, "c", 1, true)})),
         "a null optional output overlaps nothing");

  // ---- order of the rules
  expect(refused(run({in(at(kHost), 16, "h"), in(nullptr, 16, "z")}), {"null", "z"}) && asked.empty(),
         "a null and a host argument: the null is reported");
  expect(refused(run({in(at(kHost), 16, "h"), in(at(kD0a + 4), 16, "z", 8)}), {"aligned", "z"}) && asked.empty(),
         "a misaligned and a host argument: the alignment is reported");
  const wr::ArgError both = run({in(at(kD0a), 16, "a"), out(at(kD0a + 8), 16, "b"), in(at(kHost), 16, "h")});
  expect(refused(both, {"h", "not device memory"}) && !has(both.msg, "overlaps"),
         "a host argument and an overlap: the host argument is reported");

  // ---- the part that needs no classifier, and ranges_overlap by itself
  expect(passed(wr::check_args_host("the_call", {in(at(kHost), 16, "h")})), "check_args_host looks at no memory");
  expect(refused(wr::check_args_host("the_call", {in(nullptr, 16, "z")}), {"null", "z"}), "check_args_host: null");
  expect(wr::ranges_overlap(at(100), 10, at(109), 1) && !wr::ranges_overlap(at(100), 10, at(110), 1) &&
             !wr::ranges_overlap(at(100), 10, at(105), 0) && !wr::ranges_overlap(nullptr, 10, at(0), 10),
         "ranges_overlap: one byte, touching, empty, null");

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
