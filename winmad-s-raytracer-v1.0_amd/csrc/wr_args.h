// The argument checker of every call that reads or writes caller-owned device
// arrays.  A caller's mistake must not become a GPU fault: the
// arrays of a call are checked on the host, before anything is enqueued.
// Plain C++17 with no HIP in it: what a pointer is comes from a classifier the
// caller passes in (hipPointerGetAttributes in the library, an address map in
// tests/native/args_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "winmad_rt.h"

namespace wr {

struct Arg {
  const void* p;
  size_t bytes;
  size_t align;  // of p, in bytes
  const char* name;
  bool out;       // written (in/out counts): must not overlap any other array
  bool optional;  // may be null
};

inline Arg in(const void* p, size_t bytes, const char* name, size_t align = 1, bool optional = false) {
  return {p, bytes, align, name, false, optional};
}
inline Arg out(const void* p, size_t bytes, const char* name, size_t align = 1, bool optional = false) {
  return {p, bytes, align, name, true, optional};
}

// what a classifier says of one address
struct PtrClass {
  bool query_ok;          // the lookup itself succeeded
  bool is_device_memory;  // (not host, pinned or managed memory)
  int device;
};

struct ArgError {
  int code = WR_OK;
  std::string msg;
  explicit operator bool() const { return code != WR_OK; }
};

// empty ranges overlap nothing, ranges that only touch do not overlap
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && na && nb && x < y + nb && y < x + na;
}

// The part that looks at the pointers' values alone: a required array is there
// and every array is aligned.
inline ArgError check_args_host(const char* call, std::initializer_list<Arg> args) {
  const std::string who = std::string(call) + ": ";
  for (const Arg& a : args) {
    if (!a.p && a.bytes && !a.optional) return {WR_E_ARG, who + "null " + a.name};
    if (a.p && reinterpret_cast<uintptr_t>(a.p) % a.align)
      return {WR_E_ARG, who + a.name + " must be " + std::to_string(a.align) + "-byte aligned"};
  }
  return {};
}

// check_args_host, then every non-empty array is classified at its first and its
// last byte, both of which have to be device memory of `device` (`host_goes_to`
// ends the message of one that is not), then no written array may overlap
// another.  classify: const void* -> PtrClass; nothing is classified once an
// earlier step has failed.
template <class Classify>
ArgError check_args(const char* call, std::initializer_list<Arg> args, int device, const char* host_goes_to,
                    Classify&& classify) {
  if (ArgError e = check_args_host(call, args)) return e;
  const std::string who = std::string(call) + ": ";
  for (const Arg& a : args) {
    if (!a.p || !a.bytes) continue;
    const char* b = static_cast<const char*>(a.p);
    for (const char* q : {b, b + (a.bytes - 1)}) {
      const PtrClass k = classify(static_cast<const void*>(q));
      if (!k.query_ok || !k.is_device_memory)
        return {WR_E_ARG, who + a.name + " is not device memory (host or pinned host memory goes to " + host_goes_to + ")"};
      if (k.device != device)
        return {WR_E_ARG, who + a.name + " lives on device " + std::to_string(k.device) + ", the context on device " +
                              std::to_string(device)};
    }
  }
  for (const Arg& a : args)
    for (const Arg& b : args)
      if (&a < &b && (a.out || b.out) && ranges_overlap(a.p, a.bytes, b.p, b.bytes))
        return {WR_E_ARG, who + a.name + " overlaps " + b.name};
  return {};
}

}  // namespace wr
