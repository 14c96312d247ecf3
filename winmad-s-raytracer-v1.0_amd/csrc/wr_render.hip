// MI355X (gfx950) implementation of the reference's hot path behind the C ABI of
// include/winmad_rt.h (kernels in wr_traverse.h, wr_bdpt.h, wr_vcm.h, wr_pt.h;
// this file: shared device helpers, the runtime -- pipelines, work buffers,
// launches, timing -- and the C entry points):
//   * KD-tree closest-hit traversal (wr_traverse.h) as one generic queue kernel
//   * BidirPathTracing::runIteration (bidirPathTracing.cpp:53-265) as a wavefront:
//       light pass  : gen -> [trace -> shade] x 9 -> trace(splat rays) -> resolve
//       camera pass : gen -> [trace -> shade -> trace(shadow+aux) -> resolve -> DI] x 10
//     path state lives in SoA buffers sized for the whole frame; queues are
//     compacted with wave ballots + one atomic per wave
//   * PathIntegrator::raytracing (pathIntegrator.cpp:29-148), one sample index per
//     wavefront iteration
//
// Work is keyed by (iteration, path index) through the counter RNG, never by the
// device or launch geometry, so any sharding of iterations over GPUs renders the
// same film up to float summation order.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>

#include <algorithm>
#include <cassert>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "winmad_rt.h"
#include "wr_args.h"
#include "wr_flatten.h"
#include "wr_queue_slab.h"
#include "wr_scene.h"
#include "wr_traverse.h"
#include "wr_fast.h"
#include "wr_denoise.h"

using namespace wrd;

// =============================================================== errors
static int fail(int code, const std::string& msg) { return wr::set_error(code, msg); }
// Hardware queues: one per render pipeline.  HIP gives a process
// GPU_MAX_HW_QUEUES queues (default 4; the GPU box exports 4), read once when
// HIP initialises, and pipelines beyond them share a queue and serialize
// (concurrent pipelines).  The library never writes the process
// environment by itself: a host that wants the measured configuration (16
// pipelines) asks for it with wr_request_hw_queues() before its first HIP call
// (example_main / tot_main do; bench.py and winmad_rt/native.py set the
// variable before HIP starts).  The count is latched by the library's first
// wr_create (the library's first HIP call, or later than the host's): pipelines
// are sized by that value from then on, and a wr_request_hw_queues after it
// changes nothing (HIP has read the variable by then).  A host that starts HIP
// itself (e.g. torch.cuda.is_available()) before asking gets the queues HIP
// saw only if it asks before that, which is what native.py does.
static std::atomic<int> g_hw_queues_latched{0};
static int hw_queues_env() {
  const char* q = std::getenv("GPU_MAX_HW_QUEUES");
  const int n = q ? std::atoi(q) : 0;
  return n > 0 ? n : 4;  // HIP's default
}
static int hw_queues_in_effect() {
  const int l = g_hw_queues_latched.load();
  return l > 0 ? l : hw_queues_env();
}
static int latch_hw_queues() {
  int expect = 0;
  g_hw_queues_latched.compare_exchange_strong(expect, hw_queues_env());
  return g_hw_queues_latched.load();
}

// Every C-ABI entry that selects a device (hipSetDevice) leaves the caller's
// current device as it found it: a multi-device render or reduce ends on its
// last device otherwise, and a PyTorch caller's next default-device work would
// run there.
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() {
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  }
  ~DeviceGuard() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(WR_E_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// =============================================================== device helpers
namespace {

constexpr int kVMax = 9;       // light vertices per subpath (pathLength 1..9, :77-124)
constexpr int kTraceBlock = 64;  // one wave per workgroup: persistent traversal
constexpr int kShadeBlock = 256;
// The vertex kernels at <= 128 VGPRs (4 waves/SIMD, a few dwords spilled) run
// beside the other pipelines' traversal far better than at 132-146 VGPRs:
// measured 638 -> 693 Mrays/s (torus 1080p BDPT, 3 pipelines).
#ifndef WR_SHADE_WAVES
#define WR_SHADE_WAVES 4
#endif
// Scalar fp32 instead of v_pk_mul/add_f32: the pairing costs more register moves
// than it saves in this divergent, register-bound code (traversal 736 -> 791
// Mrays/s).  Results are identical (both are IEEE single-precision).  A gfx950
// target feature, so it is attached in the device pass only.
#ifdef __HIP_DEVICE_COMPILE__
#define WR_NO_PK_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define WR_NO_PK_FP32
#endif
#define WR_SHADE_OCC __attribute__((amdgpu_waves_per_eu(WR_SHADE_WAVES, 8))) WR_NO_PK_FP32
// Iterations / samples a pipeline advances in lockstep (see struct Pipe).  The
// per-vertex kernels take the whole group (member = blockIdx.y).
#ifndef WR_GROUP
#define WR_GROUP 2
#endif
constexpr int kGroup = WR_GROUP;
static_assert(kGroup <= wr::kSlabMaxMembers, "a pipeline's ray slab holds every buffer set of the group");

enum SqKind { SQ_SPLAT = 0, SQ_CONN = 1, SQ_NEE = 2, SQ_DIB = 3 };
enum DiFlag { DI_NEE = 1, DI_BSDF = 2, DI_EARLY = 4 };
// DI record state word: rays still to resolve (low byte) | results
enum DiState { DI_COUNT = 0xff, DI_VIS = 0x100, DI_SAME = 0x200 };

// Queue counters of one iteration / sample, one slot per step, cleared by a
// single memset at its start (no per-bounce counter resets).  BDPT: light
// bounce b uses slot b, camera bounce b slot kCamSlot + b; PT bounce b slot b.
constexpr int kSlots = 64;
constexpr int kCamSlot = 16;
struct StepCounters {
  int ext[kSlots];    // extension rays entering step `slot`
  int sq[kSlots];     // shadow / aux rays traced at step `slot` (light splats: slot 0 -> camera bounce 0)
  int di[kSlots];     // DI records finalized at step `slot`
  int fetch[kSlots];  // persistent-traversal cursor of the step's trace launch
  int vcm_pending;    // VCM: light paths whose first vertex is an emitter (k_vcm_fixup)
  int vcm_nverts;     // VCM: light vertices in the merge grid
  int mq[kSlots];     // VCM: merge queries queued at step `slot`
  int hard[kSlots][3];  // WR_TRACE_BVH: rays of step `slot` left to k_fast_hard (tie list, scan list, pair list)
  int rlist[kSlots];    // WR_TRACE_BVH: rays of step `slot` the search left to k_fast_resolve
  int vpool, cpool;     // BDPT, overlapped: records taken from the light / camera vertex pools
};
struct DevCounters {
  int fetch;  // traversal cursor of the API path (wr_trace_closest / wr_occluded)
  int hard[3];  // API path: rays left to k_fast_hard (tie list, scan list, pair list)
  int rlist;    // API path: rays the search left to k_fast_resolve
  unsigned long long stamps[8];  // diagnostic build only (WR_TRACE_STAMPS=1)
  unsigned long long closest, shadow, inner, leaves, refs, tests;
  unsigned long long vm_queries, vm_found, vm_merged;  // VCM range queries / vertices in radius / merges
  unsigned long long bvh_nodes, bvh_tests, kd_replay, fallback;  // WR_TRACE_BVH work (count_work)
  unsigned long long verify_rays, verify_bad;                   // WR_BVH_VERIFY
  unsigned long long lat[12];  // WR_TRACE_BVH latency tail (FastCounters mem_max .. scans; max or sum; tie_col .. tie_pass2)
  unsigned long long ww[4];   // kd_walk_wave: walks, rounds, nodes, serial fall-backs
  // the search (count_work): outer rounds, rounds with a finisher, finishing lanes, full settle batches;
  // node-loop iterations, stepping lanes over them, leaf-phase lanes, lanes carried over a round's end
  unsigned long long rounds[8];
  unsigned long long overflow;  // BDPT: appends a full vertex pool / shadow queue dropped (the render is redone)
};

__device__ __forceinline__ int lane_id() { return __lane_id(); }

// One atomic per wave: returns this lane's slot (or -1 if !want).
__device__ __forceinline__ int wave_append(int* counter, bool want) {
  const unsigned long long m = __ballot(want);
  if (m == 0ull) return -1;
  const int lane = lane_id();
  const int leader = __ffsll(static_cast<unsigned long long>(m)) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(m));
  base = __shfl(base, leader);
  return want ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}
__device__ __forceinline__ void wave_count(unsigned long long* counter, bool c) {
  const unsigned long long m = __ballot(c);
  if (m == 0ull) return;
  if (lane_id() == __ffsll(static_cast<unsigned long long>(m)) - 1) atomicAdd(counter, (unsigned long long)__popcll(m));
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Queue entries (SoA x / y / z columns) are written by one kernel and read by
// the next one or two: with WR_QUEUE_NT they move with the non-temporal policy,
// leaving the L2 to the scene's nodes and triangles, which every search re-reads.
#ifndef WR_QUEUE_NT
#define WR_QUEUE_NT 1
#endif
__device__ __forceinline__ V3 ld3(const float* b, int stride, int i) {
#if WR_QUEUE_NT
  return v3(__builtin_nontemporal_load(b + i), __builtin_nontemporal_load(b + stride + i),
            __builtin_nontemporal_load(b + 2 * stride + i));
#else
  return v3(b[i], b[stride + i], b[2 * stride + i]);
#endif
}
__device__ __forceinline__ void st3(float* b, int stride, int i, V3 v) {
#if WR_QUEUE_NT
  __builtin_nontemporal_store(v.x, b + i);
  __builtin_nontemporal_store(v.y, b + stride + i);
  __builtin_nontemporal_store(v.z, b + 2 * stride + i);
#else
  b[i] = v.x;
  b[stride + i] = v.y;
  b[2 * stride + i] = v.z;
#endif
}
__device__ __forceinline__ void film_add(float* film, int pix, V3 v) {
  if (pix < 0) return;
  if (v.x != 0.f) atomicAdd(film + 3 * pix, v.x);
  if (v.y != 0.f) atomicAdd(film + 3 * pix + 1, v.y);
  if (v.z != 0.f) atomicAdd(film + 3 * pix + 2, v.z);
}
// ImageFilm::addColor bounds check (film.cpp:4-9) -> flat pixel or -1
__device__ __forceinline__ int pix_index(int h, int w, int H, int W) {
  return (h < 0 || h >= H || w < 0 || w >= W) ? -1 : h * W + w;
}

// =============================================================== trace kernels
// Generic persistent queue traversal: rays [3][cap] SoA, count on device.
template <bool COUNT, bool SPH, bool NARROW, bool STAMP = false, bool CUT = false, bool DENSE = false>
// Register budget: 4 waves/SIMD (<= 128 VGPRs) matches the LDS-limited 16
// waves/CU and fills the register file (BDPT at 96: C2 -0.8 %; the VCM camera
// pass, CUT, at 96: -1 %).  DENSE (PT): <= 96 VGPRs and no ray records in LDS
// -> 20 waves/CU on torus-sized trees.  C3 2,538 (4 waves) -> 2,620 (96 VGPRs,
// a shading wave of another pipeline fits beside the traversal) -> 2,697
// Mrays/s (DENSE); on BDPT DENSE loses (C2 -1 %), on VCM too (-1.3 %).
#ifndef WR_TRACE_WAVES_PER_EU
#define WR_TRACE_WAVES_PER_EU 4
#endif
#ifndef WR_TRACE_CUT_WAVES_PER_EU
#define WR_TRACE_CUT_WAVES_PER_EU 4
#endif
// wave issue priority of the traversal (s_setprio 0-3); 0 = hardware default
#ifndef WR_TRACE_PRIO
#define WR_TRACE_PRIO 0
#endif
__global__ void __launch_bounds__(kTraceBlock)
__attribute__((amdgpu_waves_per_eu(DENSE ? 5 : (CUT ? WR_TRACE_CUT_WAVES_PER_EU : WR_TRACE_WAVES_PER_EU), 8))) WR_NO_PK_FP32 k_trace(DevScene S, TraceQueues Q, DevCounters* ctr, int* fetch) {
  extern __shared__ uint32_t smem[];
#if WR_TRACE_PRIO > 0
  __builtin_amdgcn_s_setprio(WR_TRACE_PRIO);  // issue priority over co-resident vertex-kernel waves
#endif
  TraceCounters tc{0, 0, 0, 0};
  trace_queue<COUNT, SPH, NARROW, STAMP, CUT, DENSE>(S, Q, fetch, smem, tc, ctr->stamps);
  if (COUNT) {
    unsigned long long a = wave_sum(tc.inner), b = wave_sum(tc.leaves), c = wave_sum(tc.refs),
                       e = wave_sum(tc.tests);
    if (lane_id() == 0) {
      atomicAdd(&ctr->inner, a);
      atomicAdd(&ctr->leaves, b);
      atomicAdd(&ctr->refs, c);
      atomicAdd(&ctr->tests, e);
    }
  }
}

// Verified-BVH closest hit over the same queues (wr_fast.h): the search, then
// the one-ray-per-lane resolve (membership replay, KD walk of undecided rays).
// 4 waves/SIMD like k_trace.
template <bool COUNT>
__device__ __forceinline__ void fast_counts(DevCounters* ctr, const FastCounters& fc) {
  unsigned long long a = wave_sum(fc.nodes), b = wave_sum(fc.tests), c = wave_sum(fc.replay),
                     e = wave_sum(fc.fallback), ki = wave_sum(fc.kinner), kl = wave_sum(fc.kleaves),
                     kr = wave_sum(fc.krefs);
  if (lane_id() == 0) {
    atomicAdd(&ctr->bvh_nodes, a);
    atomicAdd(&ctr->bvh_tests, b);
    atomicAdd(&ctr->kd_replay, c);
    atomicAdd(&ctr->fallback, e);
    // the KD walks of undecided rays count as the reference traversal's work
    atomicAdd(&ctr->inner, ki);
    atomicAdd(&ctr->leaves, kl);
    atomicAdd(&ctr->refs, kr);
    atomicAdd(&ctr->tests, kr);
  }
  // diagnostic tail (stamps[5..7], WR_TRACE_LOG): max nodes / tests per ray, rays > 256 nodes
  atomicMax(&ctr->stamps[5], static_cast<unsigned long long>(fc.max_nodes));
  atomicMax(&ctr->stamps[6], static_cast<unsigned long long>(fc.max_tests));
  atomicAdd(&ctr->stamps[7], static_cast<unsigned long long>(fc.long_rays));
  atomicAdd(&ctr->stamps[4], static_cast<unsigned long long>(fc.fb_tie));
  for (int k = 0; k < 4; ++k) atomicAdd(&ctr->stamps[k], static_cast<unsigned long long>(fc.why[k]));
  const uint32_t lat[12] = {fc.mem_max, fc.mem_sum, fc.tie_max,   fc.tie_sum, fc.walk_max,  fc.walk_sum,
                            fc.scans,   fc.tie_col, fc.tie_leaf, fc.tie_pass2, fc.scan_t, fc.pair_used};
  for (int k = 0; k < 12; ++k) {
    if (k % 2 == 0 && k < 6) atomicMax(&ctr->lat[k], static_cast<unsigned long long>(lat[k]));
    else atomicAdd(&ctr->lat[k], static_cast<unsigned long long>(lat[k]));
  }
  if (lane_id() == 0) {  // (wave-uniform: counted by the walking wave's lane 0 only)
    const uint32_t ww[4] = {fc.ww_walks, fc.ww_rounds, fc.ww_nodes, fc.ww_over};
    for (int k = 0; k < 4; ++k)
      if (ww[k]) atomicAdd(&ctr->ww[k], static_cast<unsigned long long>(ww[k]));
  }
  const unsigned long long fin = wave_sum(fc.fin_lanes);
  if (lane_id() == 0 && fc.rounds) {  // (the rounds and batches are the wave's: every lane counted alike)
    atomicAdd(&ctr->rounds[0], static_cast<unsigned long long>(fc.rounds));
    atomicAdd(&ctr->rounds[1], static_cast<unsigned long long>(fc.fin_rounds));
    atomicAdd(&ctr->rounds[2], fin);
    atomicAdd(&ctr->rounds[3], static_cast<unsigned long long>(fc.settle_full));
    atomicAdd(&ctr->rounds[4], static_cast<unsigned long long>(fc.node_iters));
    atomicAdd(&ctr->rounds[5], static_cast<unsigned long long>(fc.step_lanes));
    atomicAdd(&ctr->rounds[6], static_cast<unsigned long long>(fc.leaf_lanes));
    atomicAdd(&ctr->rounds[7], static_cast<unsigned long long>(fc.carried_lanes));
  }
}
#ifndef WR_FAST_WAVES
#define WR_FAST_WAVES 4  // minimum waves per SIMD the search's registers must allow
#endif
// W: the search tree's width (FastScene::wide)
#ifndef WR_FAST4_WAVES
#define WR_FAST4_WAVES 5  // the 4-wide search: 98 VGPRs at 4, held to 96 for 5 waves per SIMD
#endif
// SPH: the tree holds spheres (FastScene::sph) -- a variant of its own, so
// that the triangle scenes' search keeps its registers
// RL: the search settles the rays whose winner's membership its first leaf
// cells prove (the resolve's first test) and lists the rest for k_fast_resolve
// The workgroup is 1 to kMaxSearchWG waves (the launch's choice, wr_fast.h
// search_wg_bytes); the register budget is amdgpu_waves_per_eu's as before.
// SLAB: the launch's queues are segments of one ray slab (SlabQueues) -- the
// search, the resolve and the hard kernels then address a ray by its slab
// entry alone
template <bool SLAB>
using QueuesOf = std::conditional_t<SLAB, SlabQueues, TraceQueues>;
template <bool COUNT, int W, bool SPH, bool RL = false, bool SLAB = false>
__global__ void __launch_bounds__(kTraceBlock * kMaxSearchWG)
__attribute__((amdgpu_waves_per_eu(W == 4 ? WR_FAST4_WAVES : WR_FAST_WAVES, 8))) WR_NO_PK_FP32
k_trace_fast(DevScene S, FastScene F, QueuesOf<SLAB> Q, DevCounters* ctr, int* fetch, float* t2buf, int2* pairs,
             int2* spill, int* rlist, int* rlist_n) {
  extern __shared__ uint32_t smem[];
  FastCounters fc{};
  trace_fast<COUNT, W, SPH, RL>(S, F, Q, fetch, t2buf, pairs, spill, smem, fc, static_cast<int>(blockIdx.x),
                                static_cast<int>(gridDim.x), rlist, rlist_n);
  if (COUNT) fast_counts<COUNT>(ctr, fc);
}
// the search kernel for a tree width (instantiated for 2 and 4; 8 when the
// library is built with WR_BVH_WIDE=8, in the general form only)
template <bool SLAB>
using TraceFastKernelOf = void (*)(DevScene, FastScene, QueuesOf<SLAB>, DevCounters*, int*, float*, int2*, int2*,
                                   int*, int*);
using TraceFastKernel = TraceFastKernelOf<false>;
template <bool COUNT, bool SLAB = false>
TraceFastKernelOf<SLAB> trace_fast_kernel(int wide, bool sph = false, bool rl = false) {
#if WR_BVH_WIDE == 8
  if constexpr (!SLAB)
    if (wide == 8) return k_trace_fast<COUNT, 8, false>;  // (triangle scenes: the 8-wide tree is a build option)
#endif
  if (sph) return wide == 4 ? k_trace_fast<COUNT, 4, true, false, SLAB> : k_trace_fast<COUNT, 2, true, false, SLAB>;
  // (the resolve list: triangle trees)
  if (rl) return wide == 4 ? k_trace_fast<COUNT, 4, false, true, SLAB> : k_trace_fast<COUNT, 2, false, true, SLAB>;
  return wide == 4 ? k_trace_fast<COUNT, 4, false, false, SLAB> : k_trace_fast<COUNT, 2, false, false, SLAB>;
}
#ifndef WR_RESOLVE_WAVES
#define WR_RESOLVE_WAVES 0  // > 0: the resolve's register budget as waves per SIMD (0: the compiler's choice, 101 VGPRs)
#endif
#if WR_RESOLVE_WAVES > 0
#define WR_RESOLVE_OCC __attribute__((amdgpu_waves_per_eu(WR_RESOLVE_WAVES, 8)))
#else
#define WR_RESOLVE_OCC
#endif
template <bool COUNT, bool SLAB = false>
__global__ void __launch_bounds__(kTraceBlock) WR_NO_PK_FP32 WR_RESOLVE_OCC
k_fast_resolve(DevScene S, FastScene F, QueuesOf<SLAB> Q, DevCounters* ctr, const float* t2buf, int* hard, int* hard_n,
               int hcap, const int* rlist, const int* rlist_n) {
  FastCounters fc{};
  resolve_fast<COUNT>(S, F, Q, t2buf, hard, hard_n, hcap, fc, rlist, rlist_n);
  if (COUNT) fast_counts<COUNT>(ctr, fc);
}
// WR_HARD_WAVES: register budget of k_fast_hard as waves per SIMD (0: the
// compiler's choice).  Its waves live for the whole tie / scan work (up to ms)
// beside the other pipelines' search and vertex waves, so the VGPRs they hold
// are occupancy taken from those.
#ifndef WR_HARD_WAVES
#define WR_HARD_WAVES 0
#endif
#if WR_HARD_WAVES > 0
#define WR_HARD_OCC __attribute__((amdgpu_waves_per_eu(WR_HARD_WAVES, 8)))
#else
#define WR_HARD_OCC
#endif
// blocks [0, hard_blocks): the tie list; the rest: the scan list, one ray per
// wave.  WAVE: one tie per wave (the API paths).  Otherwise the launch adapts
// to the tie count it finds: up to wave_max ties (a late bounce's launch:
// its slowest tie is the step's latency) one per wave -- a wave lasts as long
// as its own tie, and the candidates' replays are shared by its lanes -- and
// more (full launches, where other pipelines hide the latency) one per lane
// on the first lane_blocks blocks.
template <bool COUNT, bool WAVE, bool SLAB = false>
__global__ void __launch_bounds__(kTraceBlock) WR_NO_PK_FP32 WR_HARD_OCC
k_fast_hard(DevScene S, FastScene F, QueuesOf<SLAB> Q, DevCounters* ctr, const int* hard, const int* hard_n, int hcap,
            int hard_blocks, int lane_blocks, int wave_max, int pair_blocks) {
  extern __shared__ uint32_t smem[];
  FastCounters fc{};
  const int b = static_cast<int>(blockIdx.x);
  // the search's pair records and the pair list follow the lists (TraceSlot::t2)
  const int2* pairs = reinterpret_cast<const int2*>(hard + hcap);
  if (b >= hard_blocks && b < hard_blocks + pair_blocks) {
    pair_fast<COUNT>(S, F, Q, hard + 3 * static_cast<size_t>(hcap), hard_n, pairs, b - hard_blocks, pair_blocks, smem,
                     fc);
  } else if (b < hard_blocks) {
    if (WAVE || hard_n[0] <= wave_max)  // wave_max <= hard_blocks
      hard_fast<COUNT, true>(S, F, Q, hard, hard_n, pairs, b, hard_blocks, smem, fc);
    else if (b < lane_blocks)
      hard_fast<COUNT, false>(S, F, Q, hard, hard_n, pairs, b, lane_blocks, smem, fc);
  } else {
    const int s0 = hard_blocks + pair_blocks;
    scan_fast<COUNT>(S, F, Q, hard, hard_n, hcap, b - s0, static_cast<int>(gridDim.x) - s0, smem, fc);
  }
  if (COUNT) fast_counts<COUNT>(ctr, fc);
}

__global__ void __launch_bounds__(kTraceBlock) WR_NO_PK_FP32
k_fast_verify(DevScene S, FastScene F, TraceQueues Q, DevCounters* ctr) {
  extern __shared__ uint32_t smem[];
  uint32_t rays = 0, bad = 0;
  verify_fast(S, F, Q, smem, rays, bad);
  const unsigned long long a = wave_sum(rays), b = wave_sum(bad);
  if (lane_id() == 0) {
    atomicAdd(&ctr->verify_rays, a);
    atomicAdd(&ctr->verify_bad, b);
  }
}

// C-ABI traversal, before: AoS wr_ray -> SoA queue (occlusion rays re-normalised
// as Scene::occluded's Ray(p1, dir) does, scene.cpp:74)
__global__ void __launch_bounds__(256) k_api_prep(const wr_ray* rays, int n, int occ, float* o3, float* d3,
                                                  float* tmin, float* tmax, const float* targets, float* cut) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const wr_ray r = rays[i];
    const V3 o = v3(r.o[0], r.o[1], r.o[2]);
    V3 d = v3(r.d[0], r.d[1], r.d[2]);
    if (occ) {
      d = normalize(d);
      const V3 tg = v3(targets[3 * i], targets[3 * i + 1], targets[3 * i + 2]);
      cut[i] = occl_cut(o, tg, dot(tg - o, d));
    }
    st3(o3, n, i, o);
    st3(d3, n, i, d);
    tmin[i] = r.tmin;
    tmax[i] = r.tmax;
  }
}
// ... after: rebuild the Intersection (scene.cpp:25-27) or the occlusion answer
__global__ void __launch_bounds__(256) k_api_finish(DevScene S, const float* o3, const float* d3, const float* t,
                                                    const int* prim, const float* targets, int n, wr_hit* hits,
                                                    uint8_t* occ) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const V3 o = ld3(o3, n, i), d = ld3(d3, n, i);
    const int p = prim[i];
    if (occ) {
      const bool unocc = p < 0 || near_eq(o + d * t[i], v3(targets[3 * i], targets[3 * i + 1], targets[3 * i + 2]));
      occ[i] = unocc ? 0 : 1;
      continue;
    }
    wr_hit h;
    h.prim = p;
    if (p >= 0) {
      const Hit x = rebuild_hit(S, p, t[i], o, d);
      h.t = x.t;
      h.p[0] = x.p.x; h.p[1] = x.p.y; h.p[2] = x.p.z;
      h.n[0] = x.n.x; h.n[1] = x.n.y; h.n[2] = x.n.z;
      h.inside = x.inside;
      h.mat_id = x.mat;
    } else {
      h.t = WR_INF;
      h.p[0] = h.p[1] = h.p[2] = 0.f;
      h.n[0] = h.n[1] = h.n[2] = 0.f;
      h.inside = 0;
      h.mat_id = 0;
    }
    hits[i] = h;
  }
}

// wr_render_features: one ray per pixel through the pixel
// centre, no RNG.  Queue slot s holds value index feat_index(s): 8x8 raster
// tiles per wave where the film's sizes allow (coherent primary rays, as the
// BDPT camera pass), else s itself.
__device__ __forceinline__ int feat_index(int s, int W, int H) {
  if ((W % 8) != 0 || (H % 8) != 0) return s;
  const int t = s >> 6, w = s & 63, tiles = W / 8;
  return ((t / tiles) * 8 + (w >> 3)) * W + (t % tiles) * 8 + (w & 7);
}
// The PT primary ray (k_pt_gen: origin cam.pos, no EPS offset) through the
// raster point the value index stands for in `layout`: PT index i W + jj is
// (jj, i), the centre of k_pt_gen's stratification rectangle; BDPT / VCM index
// a W + b is (a + 0.5, b + 0.5) (camera_gen_one: x = p / W, y = p % W).
// The direction of that ray for value index l: the one arithmetic of
// k_feat_gen and k_camera_rays (wr_camera_rays), so the two cannot drift.
__device__ __forceinline__ WR_NO_PK_FP32 V3 feat_ray_dir(const DCam& cam, int l, int W, int layout) {
  const int a = l / W, b = l % W;
  const V3 rp = layout == WR_FILM_BDPT ? v3(static_cast<float>(a) + 0.5f, static_cast<float>(b) + 0.5f, 0.f)
                                       : v3(static_cast<float>(b), static_cast<float>(a), 0.f);
  return normalize(t_point(cam.r2w, rp) - cam.pos);
}
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_feat_gen(DevScene S, int W, int H, int layout, float* o3,
                                                                float* d3) {
  const DCam& cam = S.cam;
  const int n = W * H;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const V3 d = feat_ray_dir(cam, feat_index(s, W, H), W, layout);
    st3(o3, n, s, cam.pos);
    st3(d3, n, s, d);
  }
}
// wr_camera_rays: the same rays as wr_ray records (tmin 0, tmax INF as the
// reference's Ray), each at its value index -- feat_index is k_feat_gen's queue
// order, not an output order.  wr_ray has 4-byte members only, so the store
// assumes no more alignment than a caller's slice has.
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_camera_rays(DevScene S, int W, int H, int layout,
                                                                   wr_ray* rays) {
  const DCam& cam = S.cam;
  const int n = W * H;
  for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
    const V3 d = feat_ray_dir(cam, l, W, layout);
    wr_ray r;
    r.o[0] = cam.pos.x; r.o[1] = cam.pos.y; r.o[2] = cam.pos.z;
    r.d[0] = d.x; r.d[1] = d.y; r.d[2] = d.z;
    r.tmin = 0.f;
    r.tmax = WR_INF;
    rays[l] = r;
  }
}
// ... after the traversal: the hit as k_api_finish rebuilds it, the albedo from
// the material table; a miss writes zeros (an all-zero normal: "no surface")
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_feat_finish(DevScene S, int nmats, const float* o3,
                                                                   const float* d3, const float* t, const int* prim,
                                                                   int W, int H, float* normal, float* albedo,
                                                                   float* position, float* depth) {
  const int n = W * H;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const size_t l = static_cast<size_t>(feat_index(s, W, H));
    const int p = prim[s];
    V3 hn = v3(0.f, 0.f, 0.f), hp = hn, al = hn;
    float ht = 0.f;
    if (p >= 0) {
      const Hit x = rebuild_hit(S, p, t[s], ld3(o3, n, s), ld3(d3, n, s));
      hn = x.n;
      hp = x.p;
      ht = x.t;
      if (x.mat < 0) {
        al = v3(1.f, 1.f, 1.f);
      } else if (x.mat < nmats) {
        const DMat m = S.mats[x.mat];
        const V3 sum = m.diffuse + m.phong + m.specular;
        al = v3(sum.x < 1.f ? sum.x : 1.f, sum.y < 1.f ? sum.y : 1.f, sum.z < 1.f ? sum.z : 1.f);
      }
    }
    if (normal) normal[3 * l] = hn.x, normal[3 * l + 1] = hn.y, normal[3 * l + 2] = hn.z;
    if (position) position[3 * l] = hp.x, position[3 * l + 1] = hp.y, position[3 * l + 2] = hp.z;
    if (albedo) albedo[3 * l] = al.x, albedo[3 * l + 1] = al.y, albedo[3 * l + 2] = al.z;
    if (depth) depth[l] = ht;
  }
}

// =============================================================== BDPT, VCM, PT
#include "wr_bdpt.h"
#include "wr_vcm.h"
static_assert(sizeof(VcmGroup) <= 4000, "kernel argument block too large");
#include "wr_pt.h"
// =============================================================== shading on device arrays
#include "wr_shade.h"
// =============================================================== point sets on the device
#include "wr_points.h"
// =============================================================== photon mapping
#include "wr_photon.h"

}  // namespace

// =============================================================== host side
struct wr_scene {
  wr::Scene s;
};

// wr_flatten.h's plain element types are uploaded as the kernels' (DevScene)
static_assert(sizeof(wr::U2) == sizeof(uint2) && alignof(wr::U2) == alignof(uint2) && offsetof(wr::U2, y) == 4, "U2 is uint2");
static_assert(sizeof(wr::U4) == sizeof(uint4) && alignof(wr::U4) == alignof(uint4) && offsetof(wr::U4, w) == 12, "U4 is uint4");
static_assert(sizeof(wr::F2) == sizeof(float2) && alignof(wr::F2) == alignof(float2) && offsetof(wr::F2, y) == 4, "F2 is float2");
static_assert(sizeof(wr::F4) == sizeof(float4) && alignof(wr::F4) == alignof(float4) && offsetof(wr::F4, w) == 12, "F4 is float4");
static_assert(sizeof(wr::F3) == sizeof(V3), "F3 is V3");
static_assert(sizeof(wr::Light) == sizeof(DLight) && offsetof(wr::Light, p0) == offsetof(DLight, p0) &&
                  offsetof(wr::Light, d1) == offsetof(DLight, d1) && offsetof(wr::Light, d2) == offsetof(DLight, d2) &&
                  offsetof(wr::Light, fx) == offsetof(DLight, fx) && offsetof(wr::Light, fy) == offsetof(DLight, fy) &&
                  offsetof(wr::Light, fz) == offsetof(DLight, fz) && offsetof(wr::Light, le) == offsetof(DLight, le) &&
                  offsetof(wr::Light, inv_area) == offsetof(DLight, inv_area),
              "Light is DLight");
static_assert(sizeof(wr::Material) == sizeof(DMat) && offsetof(wr::Material, diffuse) == offsetof(DMat, diffuse) &&
                  offsetof(wr::Material, phong) == offsetof(DMat, phong) &&
                  offsetof(wr::Material, specular) == offsetof(DMat, specular) &&
                  offsetof(wr::Material, phong_exp) == offsetof(DMat, phong_exp) &&
                  offsetof(wr::Material, index) == offsetof(DMat, index),
              "Material is DMat");

namespace {
// Grow-only device buffer of n elements, move-only.  The owner's device must be
// current when it grows and when it dies (wr_destroy selects it before `delete`).
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p), std::swap(n, o.n);
    return *this;
  }
  ~DevBuf() { release(); }
  // at least `want` elements; a block that is too small is freed and replaced
  // (its contents are gone).  On failure the buffer is {nullptr, 0}.
  int grow(size_t want) {
    if (p && n >= want) return WR_OK;
    release();
    const hipError_t e = hipMalloc(&p, want * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return fail(WR_E_HIP, "hipMalloc of " + std::to_string(want * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    }
    n = want;
    return WR_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr, n = 0;
  }
};

// Device memory arena: bump allocation out of one hipMalloc per arena.
struct Arena {
  DevBuf<char> mem;
  size_t used = 0;
  size_t cap() const { return mem.n; }
  int reserve(size_t bytes) {  // a fresh block, whatever was there
    release();
    return mem.grow(bytes);
  }
  template <class T>
  T* take(size_t n) {
    size_t off = (used + 255) & ~size_t(255);
    used = off + n * sizeof(T);
    return reinterpret_cast<T*>(mem.p + off);
  }
  void release() {
    mem.release();
    used = 0;
  }
};

template <class Fn>
size_t measure(Fn fn) {  // bytes an arena layout needs
  Arena a;
  fn(a);
  return a.used + 256;
}

// One arena upload: every array is named once, with the pointer it lands in.
// commit() lays the arrays out in the order they were added (256-byte aligned,
// as Arena::take), reserves the arena, copies and assigns.
struct Upload {
  struct Item {
    const void* src;
    size_t bytes, room;  // bytes copied, bytes taken (>= bytes)
    std::function<void(char*)> assign;
  };
  std::vector<Item> items;
  // `min_elems`: elements of room to take when the vector holds fewer
  template <class D, class S>
  void add(D** slot, const std::vector<S>& v, size_t min_elems = 0) {
    items.push_back({v.data(), v.size() * sizeof(S), std::max(v.size(), min_elems) * sizeof(S),
                     [slot](char* p) { *slot = reinterpret_cast<D*>(p); }});
  }
  template <class D>
  void room(D** slot, size_t n) {  // n elements nothing is copied to
    items.push_back({nullptr, 0, n * sizeof(D), [slot](char* p) { *slot = reinterpret_cast<D*>(p); }});
  }
  int commit(Arena& A, const char* what) {
    const size_t total = measure([&](Arena& a) {
      for (const Item& it : items) a.take<char>(it.room);
    });
    if (int rc = A.reserve(total)) return rc;
    for (const Item& it : items) {
      char* dst = A.take<char>(it.room);
      it.assign(dst);
      if (!it.bytes) continue;
      const hipError_t e = hipMemcpy(dst, it.src, it.bytes, hipMemcpyHostToDevice);
      if (e != hipSuccess) return fail(WR_E_HIP, std::string(what) + " upload: " + hipGetErrorString(e));
    }
    return WR_OK;
  }
};
}  // namespace

// One render pipeline: a HIP stream with its own work buffers and queue
// counters.  Iterations (BDPT) / samples (PT) are dealt round-robin to the
// context's pipelines, so the long tail of one stream's late-bounce traversal
// launches (a launch lasts as long as its slowest ray) overlaps the full
// launches of another.  The film is a sum, so the result does not depend on the
// pipeline count (up to the order of float atomics).
#ifndef WR_MAX_PIPES
#define WR_MAX_PIPES 16
#endif
constexpr int kMaxPipes = WR_MAX_PIPES;
// One parity's ray slab of a BDPT pipeline (wr_queue_slab.h): the o / d / t /
// prim arrays of every buffer set's shadow / aux and extension queues are
// segments of these (o, d: 3 planes of `stride` entries).  o null: no slab.
struct RaySlab {
  float* o = nullptr;
  float* d = nullptr;
  float* t = nullptr;
  int* prim = nullptr;
  int stride = 0;
};
// Each pipeline advances a group of up to kGroup iterations / samples in
// lockstep: every traversal launch takes the queues of all of them, so the
// launch tail (its slowest ray) is paid once per group.
struct Pipe {
  hipStream_t stream = nullptr;
  bool own_stream = false;  // pipeline 0 runs on the context stream, which the context destroys
  DevCounters* ctr = nullptr;
  StepCounters* sc = nullptr;  // [kGroup]
  Arena work;
  size_t work_key = 0;  // P for which `work` is laid out
  int work_kind = 0;    // 1 bdpt, 2 pt, 3 vcm (bdpt + vcm buffers)
  int work_sets = 0;    // buffer sets laid out
  float work_pool = -1.f;  // the BDPT pool scale they were laid out with (bdpt_pool_scale)
  BdptBuf bb[kGroup]{};
  RaySlab slab[2];            // BDPT layouts: the ray slab of each parity (bb[m].sq[k], bb[m].q_*[k])
  wr::QueueSlabLayout slab_l;  // ... and its carving (ext segment of set m: cap_ext entries)
  PtBuf pb[kGroup]{};
  VcmBuf vb[kGroup]{};
  DevBuf<float> t2buf;  // WR_TRACE_BVH: 5 floats per ray of a launch: per-ray t2 of the BVH search, lists (TraceSlot)
  DevBuf<int2> spill;   // WR_TRACE_BVH: the search stack's spill area (fast_blocks x 64 lanes)
  std::vector<hipEvent_t> events;  // Timer marks (time_kernels)
  std::vector<int> ev_cat;
  size_t ev_used = 0;
  hipEvent_t done = nullptr;
  // moments renders only (wr_render_*_moments): the films of the passes this
  // pipeline has open, zero between passes (k_film_fold clears what it folds)
  DevBuf<float> mom[kGroup];
  Pipe() = default;
  Pipe(const Pipe&) = delete;
  Pipe& operator=(const Pipe&) = delete;
  ~Pipe() {  // with the context's device current and the streams idle (wr_destroy)
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (done) (void)hipEventDestroy(done);
    if (ctr) (void)hipFree(ctr);
    if (sc) (void)hipFree(sc);
    if (stream && own_stream) (void)hipStreamDestroy(stream);
  }
};

struct wr_context {
  int device = 0;
  hipStream_t stream = nullptr;  // API traversal, film set-up / return, joins the pipelines
  Pipe pipes[kMaxPipes];
  // torus 1080p BDPT, groups of 2 (Mrays/s): 4 pipelines / 4 queues 832,
  // 8 / 8 -> 864, 16 / 16 -> 894 (twice the memory of 8: ~5 GB per buffer set)
  int npipes = 4;
  hipEvent_t t_ref = nullptr;  // start of the current render (pipelines wait on it)
  hipEvent_t t_null = nullptr;  // the caller's legacy-stream work before a render
  DevScene ds{};
  Arena scene_mem;
  int64_t scene_bytes = 0;
  DevCounters* ctr = nullptr;  // API traversal
  DevBuf<float> film_tmp;  // a host film's device copy
  DevBuf<float> film_bak;  // a device film as it was before a BDPT render (redone on pool overflow)
  bool mom_dirty = false;  // a moments render failed under way: its pass films are cleared before the next
  DevBuf<double> err_acc;  // wr_film_error on device films: sum se, sum mu, max se / mu (bits), values
  DevCounters* host_ctr = nullptr;  // pinned: the pipelines' counters after a render (finish_render)
  DevBuf<char> api_tmp;  // wr_trace_closest / wr_occluded / wr_path_radiance scratch, grown on demand
  // wr_film_denoise on device films: the two (c, v) planes the levels alternate
  // between and the guide words (3 per pixel), allocated by the first denoise
  DevBuf<dn::F4> dn_cv[2];
  DevBuf<dn::F4> dn_guides;
  int grid = 2048;
  int cus = 256;
  int nmats = 0, has_sph = 0;  // entries of ds.mats; the scene has a sphere (BdptArgs)
  float sph_r = 0.f;  // sceneSphere.sceneRadius (scene.cpp:483-487): VCM base radius
  float vcm_cell = 1.f;  // VCM merge-grid cell edge in query half-widths (WR_VCM_CELL); measured 2 -> 1: +4 %
  bool spheres = false;
  bool narrow = false;  // <= 65536 nodes, leaves <= 255 refs: 16-bit stack / pair offsets
  bool trace_log = false;  // WR_TRACE_LOG=1: per-launch ray counts and durations
  bool stamps = false;  // WR_TRACE_STAMPS=1: diagnostic traversal with phase stamps
  int trace_blocks = 4096;        // resident one-wave workgroups of the traversal
  int trace_blocks_dense = 4096;  // the same for the TRACE_DENSE layout
  bool api_dense = false;         // test knob WR_TRACE_DENSE=1: API launches in TRACE_DENSE
  bool no_cut = false;            // WR_TRACE_NO_CUT=1: shadow rays run to the end (no occl_cut)
  bool timing = false;
  // BDPT pieces (plan_pieces): at most piece_cap paths per buffer set, shares of
  // at least piece_min paths per pipeline (env WR_PIECE_CAP / WR_PIECE_MIN).
  // A short render runs on fewer, fuller pipelines: measured C2 Mrays/s for
  // piece_min 16 K / 384 K / 512 K / 640 K / 768 K / 1 M paths at 1 iteration
  // 656 / 771 / 951 / 1,002 / 868 / 841, at 4 iterations 1,559 / 1,585 /
  // 1,334 / 1,659 / 1,669 / 1,717; 20 and 256 iterations within noise
  // (profiles/r3/piece_min)
  int piece_cap = 1 << 21;
  int piece_min = 655360;
  // pipelines' k_fast_hard: launches with at most this many ties resolve them
  // one per wave (env WR_TIE_WAVE_MAX; 0: always one per lane).  Measured
  // (C2, profiles/r4/tie_wave_max): 512 -> 4096 lifts 1 iteration from
  // 1,182 to 1,328 Mrays/s and keeps 20 (2,766 -> 2,788); every tie one per
  // wave loses at 20 (2,432)
  int tie_wave_max = 4096;
  // k_fast_hard's scan-list waves (WR_SCAN_WAVES): 1,024 against 256, five runs each: C4 +1.3 %,
  // C2 20 it. +0.5 %, C3 and one iteration alike (profiles/r6/scan_waves*.txt)
  int scan_waves = 1024;
  // host threads issuing a render's launches (env WR_ISSUE_THREADS): the
  // pipelines are dealt out to them, each thread issues its pipelines' steps
  int issue_threads = 1;
  // verified-BVH traversal (wr_fast.h): built at wr_create for triangle scenes
  FastScene fs{};
  // a binary-tree scene's 4-wide tree, searched by renders whose pipelines
  // hold one group each (latency-bound: C2 at 1 iteration +6 %, -3 % at 20);
  // wide_now: the tree the current render searches (0: fs)
  int sdepth4 = 0;  // the 4-wide tree's search stack (search_scene)
  bool fs4_ok = false;
  bool lat_wide = true;  // env WR_BVH_WIDE_LAT=0: off
  int wide_now = 0;
  bool lat_now = false;  // the current BDPT render is latency-bound (see wide_now)
  Arena fast_mem;
  bool fast_ok = false;   // scene supports it
  bool fast_on = false;   // WR_TRACE_BVH mode selected
  int fast_blocks = 4096; // resident waves of k_trace_fast (a multiple of search_wg)
  // the search's workgroup (wr_fast.h search_wg_bytes): its waves, and the top
  // set of the 4-wide tree of search_scene (fs.ntop: the tree fs searches)
  int search_wg = 1;
  int ntop4 = 0;
  int resolve_blocks = 0; // k_fast_resolve's one-wave workgroups (0: fast_blocks; env WR_RESOLVE_GRID per CU)
  bool resolve_list = true;  // the search lists the rays the resolve must see (env WR_RESOLVE_LIST=0: all rays)
  bool verify = false;      // WR_BVH_VERIFY=1: every BVH answer checked against the KD walk
  // BDPT light and camera passes overlapped (wr_bdpt.h; env WR_BDPT_OVERLAP=0: sequential)
  bool bdpt_overlap = true;
  bool queue_slab = true;  // BDPT launches take the slab form of the traversal kernels (env WR_QUEUE_SLAB=0: the general form)
  DevBuf<float> api_t2;    // t2 scratch of the API path (5 floats per ray, as Pipe::t2buf)
  DevBuf<int2> api_spill;  // the API path's search stack spill area
  // ---- several GPUs (wr_create_multi): this context drives devices[0], `subs`
  // the others; work is dealt to all of them and their films are summed on
  // devices[0] (RCCL reduce over xGMI when the devices are distinct)
  std::vector<wr_context*> subs;
  std::vector<ncclComm_t> dev_comms;  // one per device (ncclCommInitAll), empty: peer copies
  DevBuf<float> red_buf;    // this device's film of a multi-device render
  DevBuf<float> stage_buf;  // devices[0]: a peer film copied in before it is added
  // ---- one process per GPU (wr_comm_init): this rank's communicator
  ncclComm_t comm = nullptr;
  int comm_ranks = 0, comm_rank = 0;
  // ---- point-set indices handed out and still alive (wr_points_build_dev):
  // wr_destroy frees them
  std::vector<wr_points*> points;
  // ---- photon maps handed out and still alive (wr_photon_map_build): wr_destroy frees them
  std::vector<wr_photon_map*> photon_maps;
  wr_context() = default;
  wr_context(const wr_context&) = delete;
  wr_context& operator=(const wr_context&) = delete;
  // Only wr_destroy deletes a context: it ends the sub-contexts and
  // communicators, selects `device` and idles the streams first.  The members
  // (pipelines, arenas, buffers) then free themselves.
  ~wr_context() {
    if (t_ref) (void)hipEventDestroy(t_ref);
    if (t_null) (void)hipEventDestroy(t_null);
    if (host_ctr) (void)hipHostFree(host_ctr);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// An index over a caller's point set (csrc/wr_points.h): bucket-sorted records
// and the buckets' first records, on the context's device.  Freed with that
// device current (wr_points_free, wr_destroy).
struct wr_points {
  wr_context* ctx = nullptr;
  int64_t n = 0;  // points given (X.nrec of them finite)
  PtsIndex X{};
  int64_t buckets = 0, max_bucket = 0;
  DevBuf<float4> rec;
  DevBuf<int> start;
};

// The two maps of wr_photon_map_build (csrc/wr_photon.h), each with its
// point-set index; [WR_PHOTON_CAUSTIC], [WR_PHOTON_INDIRECT].  Freed like a wr_points.
struct wr_photon_map {
  wr_context* ctx = nullptr;
  wr_photon_map_info info{};
  struct Side {
    DevBuf<float> pos;    // [count][3]
    DevBuf<float4> pay;   // [count][2] {wi, 0}, {alpha, 0}
    DevBuf<int32_t> shot;  // [count]
    wr_points* idx = nullptr;  // over pos (null: no photons); owned, and listed in ctx->points
    int count = 0;
  } side[2];
  PmMap dev(int which) const {
    const Side& s = side[which];
    return PmMap{s.idx ? s.idx->X : PtsIndex{}, s.pay.p, s.idx ? s.count : 0};
  }
};

namespace {

// RCCL, bound at first use: the copy already in the process (PyTorch's) when
// its symbols are global, else ROCm's librccl.so.1.  Single-device contexts
// never load it.
struct RcclApi {
  bool ok = false;
  std::string why;
  ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
  ncclResult_t (*init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*init_all)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t,
                         hipStream_t) = nullptr;
  ncclResult_t (*group_start)() = nullptr;
  ncclResult_t (*group_end)() = nullptr;
  ncclResult_t (*destroy)(ncclComm_t) = nullptr;
  const char* (*err_str)(ncclResult_t) = nullptr;
  ncclResult_t (*count)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*user_rank)(const ncclComm_t, int*) = nullptr;
};
const RcclApi& rccl() {
  static const RcclApi api = [] {
    RcclApi a;
    void* h = dlsym(RTLD_DEFAULT, "ncclCommInitRank") ? RTLD_DEFAULT : nullptr;
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      const char* e = dlerror();
      a.why = std::string("RCCL not loadable: ") + (e ? e : "librccl.so.1");
      return a;
    }
    auto sym = [&](auto& f, const char* name) {
      f = reinterpret_cast<std::remove_reference_t<decltype(f)>>(dlsym(h, name));
      return f != nullptr;
    };
    a.ok = sym(a.get_unique_id, "ncclGetUniqueId") && sym(a.init_rank, "ncclCommInitRank") &&
           sym(a.init_all, "ncclCommInitAll") && sym(a.reduce, "ncclReduce") && sym(a.group_start, "ncclGroupStart") &&
           sym(a.group_end, "ncclGroupEnd") && sym(a.destroy, "ncclCommDestroy") && sym(a.err_str, "ncclGetErrorString") &&
           sym(a.count, "ncclCommCount") && sym(a.user_rank, "ncclCommUserRank");
    if (!a.ok) a.why = "RCCL lacks an entry point";
    return a;
  }();
  return api;
}
#define NCCLCHK(expr)                                                                           \
  do {                                                                                          \
    ncclResult_t r_ = (expr);                                                                   \
    if (r_ != ncclSuccess) return fail(WR_E_HIP, std::string(#expr ": ") + rccl().err_str(r_)); \
  } while (0)

// films of a multi-device render, summed on devices[0] (peer-copy path)
__global__ void __launch_bounds__(256) k_film_accumulate(float* dst, const float* src, size_t n) {
  for (size_t i = blockIdx.x * size_t(256) + threadIdx.x; i < n; i += size_t(gridDim.x) * 256) dst[i] += src[i];
}

// ---- moments renders (wr_render_*_moments).  A pass (one BDPT /
// VCM iteration, one PT sample index, whole frame) renders into a film of its
// own on its pipeline; when its last piece has run, k_film_fold adds the pass
// film into the caller's `film` and its square, per value, into `film_sq`, and
// clears it for the pipeline's next pass.  Several pipelines fold into the same
// two films at once, hence the float atomics of the splat kernels (film_add).
// A block moves 1024 floats per round: 16-byte loads, turned through LDS so
// that a wave's atomics cover 256 contiguous bytes (the shape global float
// atomics run fastest in); zeros (84 % of a torus film) take no atomic.
constexpr int kFoldBlock = 256;
__global__ void __launch_bounds__(kFoldBlock) k_film_fold(float* __restrict__ film, float* __restrict__ film_sq,
                                                          float* __restrict__ pass, size_t n) {
  __shared__ float tile[4 * kFoldBlock];
  const size_t rounds = n / (4 * kFoldBlock);
  const int t = threadIdx.x;
  for (size_t r = blockIdx.x; r < rounds; r += gridDim.x) {
    const size_t base = r * (4 * kFoldBlock);
    float4* src = reinterpret_cast<float4*>(pass + base) + t;
    const float4 v = *src;
    reinterpret_cast<float4*>(tile)[t] = v;
    if (v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f) *src = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = tile[k * kFoldBlock + t];
      if (x != 0.f) {
        atomicAdd(film + base + k * kFoldBlock + t, x);
        atomicAdd(film_sq + base + k * kFoldBlock + t, x * x);
      }
    }
    __syncthreads();
  }
  // the tail: 3 P floats need not be a multiple of the round
  for (size_t i = rounds * (4 * kFoldBlock) + blockIdx.x * size_t(kFoldBlock) + t; i < n;
       i += size_t(gridDim.x) * kFoldBlock) {
    const float x = pass[i];
    if (x != 0.f) {
      atomicAdd(film + i, x);
      atomicAdd(film_sq + i, x * x);
      pass[i] = 0.f;
    }
  }
}

// Standard error of the mean of n passes, per value, from the sum S and the
// sum of squares Q (wr_film_error): mu = S / n, var(mean) = max(0, (Q - S^2 / n)
// / (n - 1)) / n, se = sqrt(var).  In double: in float Q - S^2 / n of a value
// that barely varies cancels to rounding noise of order 1e-7 Q.  acc: sum se,
// sum mu, max se / mu over the values with mu > 0 (as the bits of a
// non-negative double, which order like the doubles), their number.
__host__ __device__ inline void film_error_value(float S, float Q, double n, double* mu, double* se) {
  const double s = static_cast<double>(S), q = static_cast<double>(Q);
  double var = (q - s * s / n) / (n - 1.0);
  var = (var > 0.0 ? var : 0.0) / n;  // (a NaN input gives 0, not NaN)
  *mu = s / n;
  *se = sqrt(var);
}
constexpr int kErrBlock = 256;
__global__ void __launch_bounds__(kErrBlock) k_film_error(const float* __restrict__ film,
                                                         const float* __restrict__ film_sq, size_t n, int passes,
                                                         float* __restrict__ se_map, double* __restrict__ acc) {
  double sum_se = 0.0, sum_mu = 0.0, max_rel = 0.0;
  unsigned long long cnt = 0;
  const double np = static_cast<double>(passes);
  for (size_t i = blockIdx.x * size_t(kErrBlock) + threadIdx.x; i < n; i += size_t(gridDim.x) * kErrBlock) {
    double mu, se;
    film_error_value(film[i], film_sq[i], np, &mu, &se);
    if (se_map) se_map[i] = static_cast<float>(se);
    sum_se += se;
    sum_mu += mu;
    if (mu > 0.0) {
      const double rel = se / mu;
      max_rel = rel > max_rel ? rel : max_rel;
      ++cnt;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    sum_se += __shfl_xor(sum_se, o);
    sum_mu += __shfl_xor(sum_mu, o);
    const double m = __shfl_xor(max_rel, o);
    max_rel = m > max_rel ? m : max_rel;
    cnt += __shfl_xor(cnt, o);
  }
  __shared__ double red[kErrBlock / 64][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = sum_se;
    red[w][1] = sum_mu;
    red[w][2] = max_rel;
    red[w][3] = static_cast<double>(cnt);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0, m = 0.0, k = 0.0;
    for (int j = 0; j < kErrBlock / 64; ++j) {
      a += red[j][0];
      b += red[j][1];
      m = red[j][2] > m ? red[j][2] : m;
      k += red[j][3];
    }
    atomicAdd(acc + 0, a);
    atomicAdd(acc + 1, b);
    atomicMax(reinterpret_cast<unsigned long long*>(acc + 2), static_cast<unsigned long long>(__double_as_longlong(m)));
    atomicAdd(acc + 3, k);
  }
}

// overlapped: the BDPT render's own layout (the camera pass's extension queues
// and the camera-vertex store); VertexCM's BDPT part runs the sequential
// schedule and goes without them
// Overlapped BDPT: the shadow / aux queues and the vertex pools per path of
// a buffer set (wr_bdpt.h, BdptBuf): what the reference scenes use is far
// below the worst case (torus: ~3 % of the 11 shadow rays a path may queue in
// one step; ~1 stored light vertex of 9), so they are sized by use and a
// render that fills one is redone with pieces the worst case fits (exact).
// Env WR_BDPT_POOL_SCALE scales all three (tests force small ones); 0: the
// worst case, no pools.
constexpr float kSqPerPath = 2.f, kVPoolPerPath = 2.f, kCPoolPerPath = 1.f;
float bdpt_pool_scale() {  // (read at every layout: a change re-lays out the buffers, ensure_work)
  const char* e = std::getenv("WR_BDPT_POOL_SCALE");
  return e ? std::max(0.f, static_cast<float>(std::atof(e))) : 1.f;
}
// capacity of a pool of `per` records per path, at least `floor` (a safe
// re-render piece of 64 paths fits), at most the worst case
int pool_cap(int P, float per, int worst, int floor) {
  const float s = bdpt_pool_scale();
  if (s <= 0.f) return worst * P;
  const double want = std::ceil(static_cast<double>(P) * per * s);
  return static_cast<int>(std::min<double>(static_cast<double>(worst) * P, std::max<double>(want, floor)));
}

// BDPT's gen and vertex kernels read the material and light tables from LDS
// when both fit its caps (wr_bdpt.h, WR_BDPT_TABLES); -DWR_LDS_TABLES=0 builds
// a library that always reads the global tables (A/B)
#ifndef WR_LDS_TABLES
#define WR_LDS_TABLES 1
#endif
bool bdpt_lds_tables(int nmats, int nlights) {
  return WR_LDS_TABLES != 0 && nmats <= kLdsMats && nlights <= kLdsLights;
}

// shadow / aux and extension queue capacities of a BDPT buffer set of P paths
// (layout_bdpt; the extension queue of the overlapped layout holds both passes' rays)
int bdpt_cap_sq(int P, bool overlapped) {
  const bool pools = overlapped && bdpt_pool_scale() > 0.f;
  return pools ? pool_cap(P, kSqPerPath, kVMax + 2, (kVMax + 2) * 64) : P * (kVMax + 2);
}
int bdpt_cap_ext(int P, bool overlapped) { return overlapped ? 2 * P : P; }
// the ray slabs of `sets` BDPT buffer sets (both parities); stride 0: the sizes are out of range
wr::QueueSlabLayout layout_slab(Arena& a, RaySlab (&slab)[2], int P, bool overlapped, int sets) {
  const wr::QueueSlabLayout L = wr::queue_slab_layout(sets, bdpt_cap_sq(P, overlapped), bdpt_cap_ext(P, overlapped));
  const size_t n = L.stride;
  for (RaySlab& s : slab) {
    s.o = a.take<float>(3 * n);
    s.d = a.take<float>(3 * n);
    s.t = a.take<float>(n);
    s.prim = a.take<int>(n);
    s.stride = L.stride;
  }
  return L;
}

// slab, L, set: the ray arrays the traversal reads and writes (sq o / d / t /
// prim, q_o / q_d / q_t / q_prim) are segments of the pipeline's ray slabs and
// B.qs is the slabs' plane stride (BDPT); null: arrays of the set's own (VertexCM)
void layout_bdpt(Arena& a, BdptBuf& B, int P, bool overlapped, bool vcm = false, const RaySlab* slab = nullptr,
                 const wr::QueueSlabLayout* L = nullptr, int set = 0) {
  B.P = P;
  // shadow / aux rays queued by one step, per path: sequential schedule, a
  // camera vertex's <= kVMax connections + NEE + DI-BSDF (the light splats of
  // one path: <= kVMax); overlapped, at the step making vertices of length s:
  // camera side <= min(s, 9 - s) connections + NEE + DI-BSDF, light side
  // <= min(s - 1, 9 - s) connections + its splat: <= 11 as well.  Overlapped:
  // sized by use (kSqPerPath), the vertex stores pools (kVPoolPerPath,
  // kCPoolPerPath) -- 1.0 KB per path instead of 3.0 KB
  const bool pools = overlapped && bdpt_pool_scale() > 0.f;
  B.cap_sq = bdpt_cap_sq(P, overlapped);
  B.vcap = pools ? pool_cap(P, kVPoolPerPath, kVMax, kVMax * 64) : kVMax * P;
  B.ccap = pools ? pool_cap(P, kCPoolPerPath, kCvMax, kCvMax * 64) : kCvMax * P;
  const size_t sP = P, sV = size_t(B.vcap), sQ = B.cap_sq;
  // subpath records: BDPT's 32-byte BQ_* (wr_bdpt.h), VertexCM's 64-byte PS_*
  const size_t rec = vcm ? PS_WORDS : BQ_WORDS;
  B.ls = a.take<float>(rec * sP);
  B.cs = a.take<float>(rec * sP);
  // stored vertices: BDPT's 64-byte BV_* records, VertexCM's 80-byte VS_*
  B.vs = a.take<float>((vcm ? VS_WORDS : BV_WORDS) * sV);
  B.cv = overlapped ? a.take<float>(BV_WORDS * size_t(B.ccap)) : nullptr;
  // the vertex kernels move these records as 16-byte words, a stored vertex as
  // one 64-byte line (wr_bdpt.h: BqRec, BvRec)
  for (const float* r : {B.ls, B.cs, B.vs, B.cv}) {
    assert(reinterpret_cast<uintptr_t>(r) % 64 == 0);
    (void)r;
  }
  B.lvc = vcm ? nullptr : a.take<uint8_t>(sP);
  B.cvc = vcm ? nullptr : a.take<uint8_t>(sP);
  B.vidx = pools ? a.take<int>(size_t(kVMax) * P) : nullptr;
  B.cidx = pools ? a.take<int>(size_t(kCvMax) * P) : nullptr;
  // overlapped: an extension queue holds both passes' rays (light, then camera)
  const size_t sE = bdpt_cap_ext(P, overlapped);
  B.qs = slab ? L->stride : static_cast<int>(sE);

  for (int q = 0; q < 2; ++q) {
    if (slab) {
      const size_t e0 = L->ext_base[set];
      B.q_o[q] = slab[q].o + e0;
      B.q_d[q] = slab[q].d + e0;
      B.q_t[q] = slab[q].t + e0;
      B.q_prim[q] = slab[q].prim + e0;
    } else {
      B.q_o[q] = a.take<float>(3 * sE);
      B.q_d[q] = a.take<float>(3 * sE);
      B.q_t[q] = a.take<float>(sE);
      B.q_prim[q] = a.take<int>(sE);
    }
    B.q_path[q] = a.take<int>(sE);
  }
  for (int k = 0; k < 2; ++k) {
    BdptBuf::Sq& q = B.sq[k];
    if (slab) {
      const size_t s0 = L->sq_base[set];
      q.o = slab[k].o + s0;
      q.d = slab[k].d + s0;
      q.t = slab[k].t + s0;
      q.prim = slab[k].prim + s0;
    } else {
      q.o = a.take<float>(3 * sQ);
      q.d = a.take<float>(3 * sQ);
      q.t = a.take<float>(sQ);
      q.prim = a.take<int>(sQ);
    }
    q.tgt = a.take<float>(3 * sQ);
    q.val = a.take<float>(3 * sQ);
    q.cut = a.take<float>(sQ);
    q.meta = a.take<int>(sQ);
    q.pix = a.take<int>(sQ);
    B.di[k].r = a.take<float>(DR_WORDS * sP);
  }
}

void layout_pt(Arena& a, PtBuf& T, int P) {
  T.P = P;
  const size_t sP = P;
  T.st = a.take<float>(PT_WORDS * sP);
  for (int q = 0; q < 2; ++q) {
    T.q_o[q] = a.take<float>(3 * sP);
    T.q_d[q] = a.take<float>(3 * sP);
    T.q_t[q] = a.take<float>(sP);
    T.q_path[q] = a.take<int>(sP);
    T.q_prim[q] = a.take<int>(sP);
  }
  for (int k = 0; k < 2; ++k) {
    PtBuf::Sq& Q = T.sq[k];
    Q.o = a.take<float>(3 * sP);
    Q.d = a.take<float>(3 * sP);
    Q.tgt = a.take<float>(3 * sP);
    Q.val = a.take<float>(3 * sP);
    Q.t = a.take<float>(sP);
    Q.cut = a.take<float>(sP);
    Q.pix = a.take<int>(sP);
    Q.prim = a.take<int>(sP);
  }
}

// VCM merge grid: 2^k buckets, at least twice the paths (light vertices
// average ~0.5-1 per path in the reference scenes)
uint32_t vcm_table(int P) {
  uint32_t t = kRowW;
  while (t < 2u * static_cast<uint32_t>(P)) t <<= 1;
  return t;
}
size_t vcm_scan_bytes(uint32_t T) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, static_cast<const int*>(nullptr), static_cast<int*>(nullptr),
                                         static_cast<int>(T + 1));
  return b;
}
void layout_vcm(Arena& a, VcmBuf& V, int P) {
  const size_t sP = P, sV = size_t(kVMax) * P;
  const uint32_t T = vcm_table(P);
  V.l_sb = a.take<float4>(sP);
  V.v_dvm = a.take<float>(sV);
  V.pending = a.take<int>(sP);
  V.cnt = a.take<int>(size_t(T) + 1);
  V.start = a.take<int>(size_t(T) + 1);
  V.rpos = a.take<float4>(sV);
  V.rdat = a.take<float4>(2 * sV);
  V.rdvm = a.take<float>(sV);
  for (int k = 0; k < 2; ++k) {
    VcmBuf::Mq& M = V.mq[k];
    M.hp = a.take<float>(3 * sP);
    M.n = a.take<float>(3 * sP);
    M.wi = a.take<float>(3 * sP);
    M.thr = a.take<float>(3 * sP);
    M.dvcm = a.take<float>(sP);
    M.dvm = a.take<float>(sP);
    M.cont = a.take<float>(sP);
    M.pd = a.take<float>(sP);
    M.pg = a.take<float>(sP);
    M.mat = a.take<int>(sP);
    M.len = a.take<int>(sP);
    M.pix = a.take<int>(sP);
  }
  V.scan_bytes = vcm_scan_bytes(T);
  V.scan_tmp = a.take<char>(V.scan_bytes);
}

// `sets` buffer sets of `kind` (into dst's, or only measured).  BDPT: the ray
// slabs first, then each set's own arrays.  False: sizes out of the slab's range
bool layout_sets(Arena& a, Pipe* dst, int sets, int kind, int P) {
  RaySlab slab[2];
  wr::QueueSlabLayout L;
  if (kind == 1) {
    L = layout_slab(a, slab, P, true, sets);
    if (L.stride == 0) return false;
    if (dst) {
      dst->slab[0] = slab[0];
      dst->slab[1] = slab[1];
      dst->slab_l = L;
    }
  } else if (dst) {
    dst->slab[0] = dst->slab[1] = RaySlab{};
    dst->slab_l = wr::QueueSlabLayout{};
  }
  for (int g = 0; g < sets; ++g) {
    BdptBuf b;
    PtBuf t;
    VcmBuf v;
    if (kind == 2) {
      layout_pt(a, dst ? dst->pb[g] : t, P);
      continue;
    }
    if (kind == 1) layout_bdpt(a, dst ? dst->bb[g] : b, P, true, false, slab, &L, g);
    else layout_bdpt(a, dst ? dst->bb[g] : b, P, false, kind == 3);
    if (kind == 3) layout_vcm(a, dst ? dst->vb[g] : v, P);
  }
  return true;
}

int ensure_work(Pipe& p, int kind, int P, int sets) {
  // (a VCM layout holds the sequential BDPT layout only: no camera-pass queues)
  const bool same = p.work_kind == kind && p.work_pool == bdpt_pool_scale();
  if (same && p.work_key == static_cast<size_t>(P) && p.work_sets >= sets) return WR_OK;
  p.work_kind = 0;
  bool ok = true;
  const size_t need = measure([&](Arena& a) { ok = layout_sets(a, nullptr, sets, kind, P); });
  if (!ok) return WR_E_ARG;  // (a film too large for the ray slab's int indices)
  int rc = p.work.reserve(need);
  if (rc) return rc;
  layout_sets(p.work, &p, sets, kind, P);
  p.work_kind = kind;
  p.work_key = P;
  p.work_sets = sets;
  p.work_pool = bdpt_pool_scale();
  return WR_OK;
}

// Work buffers for up to `want` pipelines, each with `sets` buffer sets (~2.5 KB
// per path for BDPT), kept within 3/4 of the device memory free now plus what
// the pipelines already hold: big films degrade to fewer pipelines instead of
// failing.  Every render lays out full groups on all pipelines that fit, so a
// short render (a warm-up) leaves the buffers of a long one in place.
int pipelines_that_fit(wr_context* c, int kind, int P, int sets, int want) {
  const size_t per = measure([&](Arena& a) { (void)layout_sets(a, nullptr, sets, kind, P); });
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return want;
  size_t held = 0;
  for (int i = 0; i < kMaxPipes; ++i) held += c->pipes[i].work.cap();
  const size_t budget = (free_b + held) / 4 * 3;
  const int fit = static_cast<int>(std::min<size_t>(static_cast<size_t>(want), std::max<size_t>(1, budget / per)));
  for (int i = fit; i < kMaxPipes; ++i) {  // memory-limited: free the rest
    c->pipes[i].work.release();
    c->pipes[i].work_kind = 0;
  }
  for (int i = 0; i < fit; ++i)
    if (ensure_work(c->pipes[i], kind, P, sets) != WR_OK) return 0;
  return fit;
}

// ---- launch helpers with optional per-launch HIP events (on the pipeline's stream)
// Flags of the library's events.  By default HIP records an event with a
// system-scope release (cache writeback for host visibility); the render's
// events only order and time work on this device, so they skip it
// (hipEventDisableSystemFence).  Env WR_EVENT_SYSTEM_FENCE=1 restores it.
unsigned ev_flags(unsigned base) {
  static const bool sys = [] {
    const char* e = std::getenv("WR_EVENT_SYSTEM_FENCE");
    return e && std::atoi(e) != 0;
  }();
  return sys ? base : (base | hipEventDisableSystemFence);
}

struct Timer {
  wr_context* c;
  Pipe* p;
  Timer(wr_context* cc, Pipe* pp) : c(cc), p(pp) {}
  void mark(int cat) {
    if (!c->timing || !p) return;
    if (p->ev_used >= p->events.size()) {
      hipEvent_t e;
      (void)hipEventCreateWithFlags(&e, ev_flags(hipEventDefault));
      p->events.push_back(e);
      p->ev_cat.push_back(0);
    }
    p->ev_cat[p->ev_used] = cat;
    (void)hipEventRecord(p->events[p->ev_used++], p->stream);
  }
};

// (count2: set by the one caller that has it, the overlapped BDPT schedule)
RayQueue rq(const float* o3, const float* d3, int cap, const int* cnt, float* t, int* prim,
            const float* cut = nullptr, const float* tmin = nullptr, const float* tmax = nullptr) {
  return RayQueue{o3, d3, cap, cnt, tmin, tmax, t, prim, cut, nullptr};
}
// a queue's ray count read back to the host (diagnostics only: synchronous)
int host_count(const RayQueue& q) {
  int k = 0, k2 = 0;
  if (q.count) (void)hipMemcpy(&k, q.count, sizeof(int), hipMemcpyDeviceToHost);
  if (q.count2) (void)hipMemcpy(&k2, q.count2, sizeof(int), hipMemcpyDeviceToHost);
  return k + k2;
}
// queues of one launch (empty `count` pointers are skipped)
struct QueueList {
  TraceQueues Q{};
  int max_rays = 0;
  // lim: the rays the queue holds at most (a slab segment's entries); < 0: its plane stride q.cap
  void add(const RayQueue& q, int cap, int lim = -1) {
    if (Q.n >= kMaxQueues) {  // a schedule asking for more queues than a launch takes: a build error
      std::fprintf(stderr, "winmad_rt: more than %d queues in one traversal launch\n", kMaxQueues);
      std::abort();
    }
    Q.lim[Q.n] = lim < 0 ? q.cap : lim;
    Q.q[Q.n++] = q;
    max_rays += cap;
  }
};
// The slab form of a launch's queues, if they are one slab: every queue's
// arrays lie at one entry offset (shift) from the slab's, the plane stride is
// the slab's entries for all of them, each segment [shift, shift + lim) is
// inside a plane, no two segments overlap, and no queue has per-ray
// [tmin, tmax].  False otherwise: the launch keeps the general form.
bool slab_form(const TraceQueues& Q, const RaySlab& sl, SlabQueues& out) {
  if (!sl.o || Q.n < 1) return false;
  SlabQueues s{};
  s.o3 = sl.o;
  s.d3 = sl.d;
  s.out_t = sl.t;
  s.out_prim = sl.prim;
  s.stride = sl.stride;
  s.n = Q.n;
  for (int i = 0; i < Q.n; ++i) {
    const RayQueue& q = Q.q[i];
    const ptrdiff_t sh = q.o3 - sl.o;
    if (q.d3 - sl.d != sh || q.out_t - sl.t != sh || q.out_prim - sl.prim != sh) return false;
    if (q.cap != sl.stride || q.tmin || q.tmax) return false;
    if (sh < 0 || Q.lim[i] < 0 || sh + Q.lim[i] > sl.stride) return false;
    for (int j = 0; j < i; ++j)
      if (sh < s.shift[j] + s.lim[j] && s.shift[j] < sh + Q.lim[i]) return false;
    s.shift[i] = static_cast<int>(sh);
    s.lim[i] = Q.lim[i];
    s.count[i] = q.count;
    s.count2[i] = q.count2;
  }
  out = s;
  return true;
}

using TraceKernel = void (*)(DevScene, TraceQueues, DevCounters*, int*);
// cut: the launch's shadow rays may stop once occlusion is settled (occl_cut).
// Only PT, VCM and the API use it: BDPT launches carry 3 % shadow rays, and
// the check costs C2 1.5 % (measured).  TRACE_DENSE: cut + the 20-waves/CU
// layout (PT).
enum TraceMode { TRACE_PLAIN = 0, TRACE_CUT = 1, TRACE_DENSE = 2 };
#ifndef WR_BDPT_TRACE_MODE
// BDPT light / camera passes.  TRACE_DENSE without the cutoff (WR_DENSE_CUT
// false) measured C2 -2.5 % (-3.7 % with per-queue uniform branches)
#define WR_BDPT_TRACE_MODE TRACE_PLAIN
#endif
#ifndef WR_DENSE_CUT
#define WR_DENSE_CUT true  // TRACE_DENSE instances carry the occlusion cutoff
#endif
#ifndef WR_VCM_TRACE_MODE
#define WR_VCM_TRACE_MODE TRACE_CUT  // camera pass of VCM (TRACE_DENSE: -1.3 %)
#endif
TraceKernel trace_kernel(bool count, bool spheres, bool narrow, bool stamps, int mode = TRACE_PLAIN) {
  if (stamps) return narrow ? k_trace<false, false, true, true> : k_trace<false, false, false, true>;
  if (mode == TRACE_DENSE) {
    constexpr bool C = WR_DENSE_CUT;
    if (count) {
      if (spheres) return narrow ? k_trace<true, true, true, false, C, true> : k_trace<true, true, false, false, C, true>;
      return narrow ? k_trace<true, false, true, false, C, true> : k_trace<true, false, false, false, C, true>;
    }
    if (spheres) return narrow ? k_trace<false, true, true, false, C, true> : k_trace<false, true, false, false, C, true>;
    return narrow ? k_trace<false, false, true, false, C, true> : k_trace<false, false, false, false, C, true>;
  }
  if (mode == TRACE_CUT) {
    if (count) {
      if (spheres) return narrow ? k_trace<true, true, true, false, true> : k_trace<true, true, false, false, true>;
      return narrow ? k_trace<true, false, true, false, true> : k_trace<true, false, false, false, true>;
    }
    if (spheres) return narrow ? k_trace<false, true, true, false, true> : k_trace<false, true, false, false, true>;
    return narrow ? k_trace<false, false, true, false, true> : k_trace<false, false, false, false, true>;
  }
  if (count) {
    if (spheres) return narrow ? k_trace<true, true, true> : k_trace<true, true, false>;
    return narrow ? k_trace<true, false, true> : k_trace<true, false, false>;
  }
  if (spheres) return narrow ? k_trace<false, true, true> : k_trace<false, true, false>;
  return narrow ? k_trace<false, false, true> : k_trace<false, false, false>;
}

// The device counters of one traversal step: the persistent cursor (zero at
// the step's start: the iteration's counter memset, or the caller), and in
// WR_TRACE_BVH mode the per-ray t2 scratch of the BVH search (>= the launch's rays).
struct TraceSlot {
  int* fetch;
  float* t2;      // [t2_cap] t2 per launch index, then [t2_cap] the tie list (from the bottom) and the scan list (from the
                  // top), then [t2_cap] int2 pair records (kPairWindow), then [t2_cap] the pair list
  size_t t2_cap;
  int* hard_n;
  int2* spill;    // the search stack's spill area
  int* rlist_n;   // rays the search left to k_fast_resolve (their list: the t2 region)
};
TraceSlot tslot(Pipe& p, int slot) {
  return TraceSlot{&p.sc[0].fetch[slot], p.t2buf.p, p.t2buf.n / 5, &p.sc[0].hard[slot][0], p.spill.p, &p.sc[0].rlist[slot]};
}
// t2 scratch + hard-ray list of a pipeline for launches of up to `rays` rays
// search-stack spill entries per lane: the larger of the context's trees
size_t max_spill_entries(const wr_context* c) {
  size_t e = search_spill_entries(c->fs.sdepth, c->fs.wide);
  if (c->fs4_ok) e = std::max(e, search_spill_entries(c->sdepth4, 4));
  return e;
}
// the scene as the current render searches it: fs, or fs with its 4-wide
// tree (every other field -- KD stack depth, diagnostics -- is fs's own)
FastScene search_scene(const wr_context* c) {
  FastScene F = c->fs;
  // a latency-bound render keeps every near-tie one per wave (the pair list's
  // one per lane waits for its slowest lane: C2 at 1 iteration -4 %, while C4 at
  // 64 iterations gains 2.6 %, profiles/r6/pair_list/ab.txt)
  if (c->lat_now && F.pair > 1) F.pair = 1;
  if (c->wide_now == 4 && c->fs4_ok) {
    F.wide = 4;
    F.sdepth = c->sdepth4;
    F.ntop = c->ntop4;
  }
  return F;
}
int ensure_t2(wr_context* c, Pipe& p, size_t rays) {
  if (!c->fast_on) return WR_OK;
  if (!p.spill.p && max_spill_entries(c) > 0)
    if (int rc = p.spill.grow(max_spill_entries(c) * size_t(c->fast_blocks) * 64)) return rc;
  return p.t2buf.grow(5 * rays);  // t2 / list, hard lists, pair records (int2), pair list
}

// One persistent traversal launch over the queues of Q (max_rays bounds the
// grid).  WR_TRACE_BVH: the verified-BVH search + its resolve launch instead.
// WR_TRACE_LOG, counting launches: the search's outer rounds (DevCounters::rounds)
static void log_rounds(const unsigned long long r[8]) {
  if (r[0])
    std::fprintf(stderr,
                 "[wr bvh rounds] %llu outer rounds, %llu with a finisher (%.3f), %llu finishing lanes (%.1f per such round), "
                 "%llu full settle batches; %llu node-loop iterations (%.1f per round), %llu stepping lanes (%.1f per "
                 "iteration), %llu leaf-phase lanes (%.1f per round), %llu lanes carried mid-descent\n",
                 r[0], r[1], double(r[1]) / r[0], r[2], r[1] ? double(r[2]) / r[1] : 0.0, r[3], r[4], double(r[4]) / r[0],
                 r[5], r[4] ? double(r[5]) / r[4] : 0.0, r[6], double(r[6]) / r[0], r[7]);
}

int trace_launch(wr_context* c, hipStream_t stream, DevCounters* ctr, const TraceSlot& ts, Timer& tm, bool count,
                 const TraceQueues& Q_, int max_rays, int mode = TRACE_PLAIN, bool hard_wave = false,
                 const RaySlab* slab = nullptr) {
  int* fetch = ts.fetch;
  TraceQueues Q = Q_;
  if (c->no_cut)  // measurement knob: the same launches without the dead-work elision
    for (int i = 0; i < Q.n; ++i) Q.q[i].cut = nullptr;
  if (c->fast_on && !c->stamps && ts.t2 && static_cast<size_t>(max_rays) <= ts.t2_cap) {
    const FastScene F = search_scene(c);  // the render's search tree
    const int blocks = (max_rays + kTraceBlock - 1) / kTraceBlock;
    // the search's waves in workgroups of search_wg (fast_blocks is a
    // multiple of it: the spill area holds fast_blocks waves)
    // A tree searched without a top set keeps one wave per workgroup: a small
    // launch then spreads its waves over the CUs instead of packing them by fours.
    const int wg = F.ntop > 0 ? c->search_wg : 1;
    const int fgrid = (std::max(1, std::min(c->fast_blocks, blocks)) + wg - 1) / wg;
    const size_t lds = fast_lds_bytes(c->fs.depth);
    // the search settles the rays its first membership test proves and lists
    // the rest for the resolve (in the t2 region: t2 is kept by diagnostics
    // only).  Measured (profiles/r5/resolve_list): C4 +5 %, C2 +1 %, VCM +1 %;
    // PT's dense launches -0.8 %, so they keep the resolve over every ray
    const bool rl = c->resolve_list && !F.diag && !F.sph && F.wide != 8 && mode != TRACE_DENSE;
    int* rlist = rl ? reinterpret_cast<int*>(ts.t2) : nullptr;
    int* rlist_n = rl ? ts.rlist_n : nullptr;
    const size_t rlds = search_wg_bytes(F.sdepth, F.wide, rl, F.ntop, wg);
    // the search's pair records of near-ties (kPairWindow): after the lists
    int2* pairs = reinterpret_cast<int2*>(ts.t2 + 2 * ts.t2_cap);
    hipEvent_t f0 = nullptr, f1 = nullptr, fa = nullptr, fb = nullptr;
    if (c->trace_log) {
      (void)hipEventCreate(&f0);
      (void)hipEventCreate(&f1);
      (void)hipEventCreate(&fa);
      (void)hipEventCreate(&fb);
      (void)hipEventRecord(f0, stream);
    }
    // the slab form, when the caller's queues are one ray slab (BDPT; the
    // pipelines' hard kernel only: one tie per wave is the API paths').
    // WR_QUEUE_SLAB=0 keeps the general form, and so does the 8-wide build option
    SlabQueues SQ{};
    const bool slabbed = c->queue_slab && slab && !hard_wave && F.wide != 8 && slab_form(Q, *slab, SQ);
    const dim3 rgrid(std::max(1, std::min(c->resolve_blocks > 0 ? c->resolve_blocks : c->fast_blocks, blocks)));
    int* hard = reinterpret_cast<int*>(ts.t2 + ts.t2_cap);
    if (slabbed) {
      auto kf = count ? trace_fast_kernel<true, true>(F.wide, F.sph, rl) : trace_fast_kernel<false, true>(F.wide, F.sph, rl);
      hipLaunchKernelGGL(kf, dim3(fgrid), dim3(kTraceBlock * wg), rlds, stream, c->ds, F, SQ, ctr, fetch, ts.t2, pairs,
                         ts.spill, rlist, rlist_n);
      if (c->trace_log) (void)hipEventRecord(fa, stream);
      auto kr = count ? k_fast_resolve<true, true> : k_fast_resolve<false, true>;
      hipLaunchKernelGGL(kr, rgrid, dim3(kTraceBlock), 0, stream, c->ds, F, SQ, ctr, ts.t2, hard, ts.hard_n, static_cast<int>(ts.t2_cap), rlist, rlist_n);
    } else {
      auto kf = count ? trace_fast_kernel<true>(F.wide, F.sph, rl) : trace_fast_kernel<false>(F.wide, F.sph, rl);
      hipLaunchKernelGGL(kf, dim3(fgrid), dim3(kTraceBlock * wg), rlds, stream, c->ds, F, Q, ctr, fetch, ts.t2, pairs,
                         ts.spill, rlist, rlist_n);
      if (c->trace_log) (void)hipEventRecord(fa, stream);
      hipLaunchKernelGGL(count ? k_fast_resolve<true> : k_fast_resolve<false>, rgrid, dim3(kTraceBlock), 0, stream, c->ds,
                         F, Q, ctr, ts.t2, hard, ts.hard_n, static_cast<int>(ts.t2_cap), rlist, rlist_n);
    }
    if (c->trace_log) (void)hipEventRecord(fb, stream);
    // the hard rays are a few in 10^4: a small grid drains any count (one
    // ray per wave for the API calls: up to 2048 at once, 8 waves per CU)
    // (pipelines: up to c->tie_wave_max ties one per wave, more one per lane)
    const int lgrid = std::max(1, std::min(256, blocks));
    const int hgrid = hard_wave ? std::max(1, std::min(2048, max_rays))
                                : std::max(lgrid, std::min(c->tie_wave_max, max_rays));
    const int sgrid = std::max(1, std::min(c->scan_waves, max_rays));  // scan waves
    auto hk = hard_wave ? (count ? k_fast_hard<true, true> : k_fast_hard<false, true>)
                        : (count ? k_fast_hard<true, false> : k_fast_hard<false, false>);
    // the pair list (near-ties the search's pair record settles, one per lane)
    const int pgrid = (F.diag || F.pair < 2) ? 0 : lgrid;
    auto hks = count ? k_fast_hard<true, false, true> : k_fast_hard<false, false, true>;
    if (slabbed)
      hipLaunchKernelGGL(hks, dim3(hgrid + pgrid + sgrid), dim3(kTraceBlock), lds, stream, c->ds, F, SQ, ctr, hard, ts.hard_n,
                         static_cast<int>(ts.t2_cap), hgrid, lgrid, std::min(hgrid, c->tie_wave_max), pgrid);
    else
      hipLaunchKernelGGL(hk, dim3(hgrid + pgrid + sgrid),
                         dim3(kTraceBlock), lds, stream, c->ds, F, Q, ctr, hard, ts.hard_n,
                         static_cast<int>(ts.t2_cap), hgrid, lgrid, std::min(hgrid, c->tie_wave_max), pgrid);
    if (c->verify)
      hipLaunchKernelGGL(k_fast_verify, dim3(std::max(1, std::min(c->fast_blocks, blocks))), dim3(kTraceBlock), lds,
                         stream, c->ds, F, Q, ctr);
    tm.mark(WR_K_TRACE);
    if (c->trace_log) {
      (void)hipEventRecord(f1, stream);
      (void)hipEventSynchronize(f1);
      int tot = 0;
      for (int i = 0; i < Q.n; ++i) tot += host_count(Q.q[i]);
      float ms = 0.f, ma = 0.f, mb = 0.f;
      int nhs[3] = {0, 0, 0};
      (void)hipMemcpy(nhs, ts.hard_n, 3 * sizeof(int), hipMemcpyDeviceToHost);
      const int nh = nhs[0], ns = nhs[1];
      (void)hipEventElapsedTime(&ms, f0, f1);
      (void)hipEventElapsedTime(&ma, f0, fa);
      (void)hipEventElapsedTime(&mb, fa, fb);
      std::fprintf(stderr,
                   "[wr bvh] %d rays  %.1f us (search %.1f, resolve %.1f, hard %.1f: %d + %d pair + %d scan rays)  grid %d\n",
                   tot, ms * 1e3f, ma * 1e3f, mb * 1e3f, (ms - ma - mb) * 1e3f, nh, nhs[2], ns, fgrid);
      (void)hipEventDestroy(f0);
      (void)hipEventDestroy(f1);
      (void)hipEventDestroy(fa);
      (void)hipEventDestroy(fb);
    }
    return WR_OK;
  }
  const bool dense = mode == TRACE_DENSE && !c->stamps;
  const size_t lds = trace_lds_bytes(c->ds.max_stack, c->narrow, dense);
  const int grid =
      std::max(1, std::min(dense ? c->trace_blocks_dense : c->trace_blocks, (max_rays + kTraceBlock - 1) / kTraceBlock));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->trace_log) {  // diagnostic (WR_TRACE_LOG=1): rays and duration of every launch
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, stream);
  }
  hipLaunchKernelGGL(trace_kernel(count, c->spheres, c->narrow, c->stamps, mode), dim3(grid), dim3(kTraceBlock), lds,
                     stream, c->ds, Q, ctr, fetch);
  tm.mark(WR_K_TRACE);
  if (c->trace_log) {
    (void)hipEventRecord(e1, stream);
    (void)hipEventSynchronize(e1);
    int tot = 0;
    for (int i = 0; i < Q.n; ++i) tot += host_count(Q.q[i]);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    std::fprintf(stderr, "[wr trace] %d queues, %d rays  %.1f us  grid %d\n", Q.n, tot, ms * 1e3f, grid);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  return WR_OK;
}

int shade_grid(wr_context* c, int n) { return std::max(1, std::min(c->grid, (n + kShadeBlock - 1) / kShadeBlock)); }

// ---- BDPT work split.  A render is iterations x (W*H) paths; light path i
// pairs only with camera path i of the same iteration (:130, :222-229), MIS
// uses the global lightPathNum (:55), and splats are film atomics, so any
// partition of an iteration's path range renders the same film (up to the order
// of float atomics).  The render's path-iterations, flattened iteration-major,
// are split into one contiguous, equal share per pipeline (whole 8-row bands in
// the tiled camera order); a share is cut at iteration boundaries and into
// pieces of at most `cap` paths, and each pipeline runs its pieces in groups of
// kGroup.  Few iterations then still fill every pipeline (the reference's own
// default is 1 iteration, bidirPathTracing.cpp:9), and work buffers are sized by
// the piece, not the frame.
struct Piece {
  int iter;  // iteration index within the render
  int base;  // first global path
  int n;     // paths
};
struct PiecePlan {
  std::vector<std::vector<std::vector<Piece>>> per_pipe;  // [pipeline][group][member]
  int pipes() const { return std::max(1, static_cast<int>(per_pipe.size())); }
  int max_groups() const {
    size_t m = 0;
    for (const auto& v : per_pipe) m = std::max(m, v.size());
    return static_cast<int>(m);
  }
};
// a position in the flattened (iteration-major) path order, moved to the
// nearest whole unit of its iteration (an iteration's end is a boundary)
int64_t flat_round(int64_t f, int P, int unit) {
  const int64_t it = f / P, off = f % P;
  return it * P + std::min<int64_t>(P, (off + unit / 2) / unit * unit);
}
// [a, b) cut at iteration ends and into near-equal unit-aligned pieces of at
// most cap paths.  The stretch is counted in units (the last one may be
// partial: an iteration's end need not be unit-aligned) and each piece gets
// at most floor(cap / unit) of them, so no piece exceeds cap even when the
// stretch is not a multiple of the unit (cap is a whole number of units, or
// the frame itself).
void cut_pieces(int64_t a, int64_t b, int P, int unit, int cap, std::vector<Piece>& out) {
  const int64_t cap_units = std::max<int64_t>(1, cap / unit);
  while (a < b) {
    const int64_t it = a / P, off = a % P;
    const int64_t len = std::min<int64_t>(b - a, P - off);  // up to the iteration's end
    const int64_t units = (len + unit - 1) / unit;
    const int64_t cuts = (units + cap_units - 1) / cap_units;
    for (int64_t j = 0; j < cuts; ++j) {
      const int64_t lo = off + std::min(len, units * j / cuts * unit);
      const int64_t hi = off + std::min(len, units * (j + 1) / cuts * unit);
      if (hi > lo) out.push_back(Piece{static_cast<int>(it), static_cast<int>(lo), static_cast<int>(hi - lo)});
    }
    a += len;
  }
}
// The flattened path-iterations [lo, hi) (lo, hi whole units) over np
// pipelines, in groups of kGroup pieces.  (Splitting a short render's share
// unevenly into two groups per pipeline, so that the pipelines' late bounces
// fall at different times, measured worse: C2 at 20 iterations 2,292 ->
// 1,850 Mrays/s -- each extra group pays the bounce tails again.)
// whole_iters (moments renders; lo, hi at iteration ends): shares are cut at
// iteration ends only, so every piece of an iteration runs on one pipeline, in
// order, and the iteration's film is complete there when its last piece has run.
PiecePlan plan_pieces(int64_t lo, int64_t hi, int P, int unit, int cap, int np, int min_piece,
                      bool whole_iters = false) {
  PiecePlan plan;
  const int64_t T = hi - lo;
  if (T <= 0) {
    plan.per_pipe.resize(1);
    return plan;
  }
  int64_t shares = std::max<int64_t>(1, std::min<int64_t>(np, T / std::max(1, min_piece)));
  if (whole_iters) shares = std::min<int64_t>(shares, T / P);
  auto bound = [&](int64_t k) {
    if (whole_iters) return lo + (k * (T / P) / shares) * P;
    return k == shares ? hi : flat_round(lo + k * T / shares, P, unit);
  };
  auto groups_of = [&](const std::vector<Piece>& pcs, std::vector<std::vector<Piece>>& gs) {
    for (size_t i = 0; i < pcs.size(); i += kGroup)
      gs.emplace_back(pcs.begin() + i, pcs.begin() + std::min(pcs.size(), i + kGroup));
  };
  for (int64_t k = 0; k < shares; ++k) {
    const int64_t a = bound(k), b = bound(k + 1);
    std::vector<Piece> pcs;
    cut_pieces(a, b, P, unit, cap, pcs);
    std::vector<std::vector<Piece>> gs;
    groups_of(pcs, gs);
    if (!gs.empty()) plan.per_pipe.push_back(std::move(gs));
  }
  if (plan.per_pipe.empty()) plan.per_pipe.resize(1);
  return plan;
}
// paths one buffer set holds: the frame, or WR_PIECE_CAP (default 2^21: a
// 1920x1080 frame is one piece, 4K frames are four) rounded up to whole units
int piece_capacity(const wr_context* c, int P, int unit) {
  const int64_t want = std::min<int64_t>(P, std::max<int64_t>(unit, c->piece_cap));
  return static_cast<int>(std::min<int64_t>(P, (want + unit - 1) / unit * unit));
}

double host_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Start a render on `n` pipelines: they wait for the context stream's set-up
// (film clear) and clear their counters.
void begin_render(wr_context* c, int n, const int time_kernels) {
  // diagnostics: WR_TIME_KERNELS=0 drops the per-launch events of a timed call
  // (what the events themselves cost)
  static const bool no_events = [] {
    const char* e = std::getenv("WR_TIME_KERNELS");
    return e && std::atoi(e) == 0;
  }();
  c->timing = time_kernels != 0 && !no_events;
  // a device film may still be written by the caller's work on the legacy
  // null stream (e.g. torch's default stream zeroing it): the render's streams
  // are non-blocking, so order them after that work explicitly.  The null
  // stream is named as 0: the hipStreamLegacy handle ((hipStream_t)1) is not
  // understood by the older HIP runtime PyTorch loads first (segfault)
  (void)hipEventRecord(c->t_null, nullptr);
  (void)hipStreamWaitEvent(c->stream, c->t_null, 0);
  (void)hipEventRecord(c->t_ref, c->stream);
  for (int i = 0; i < n; ++i) {
    Pipe& p = c->pipes[i];
    p.ev_used = 0;
    (void)hipStreamWaitEvent(p.stream, c->t_ref, 0);
    (void)hipMemsetAsync(p.ctr, 0, sizeof(DevCounters), p.stream);
    Timer(c, &p).mark(WR_K_OTHER);
  }
}

// Join the pipelines into the context stream, wait, and add up the work
// counters and (time_kernels) the per-launch durations of every pipeline.
// stats->trace_wall_ms is the union of all traversal launch intervals.
int finish_render(wr_context* c, int n, wr_stats* st, double t0_host, unsigned long long* overflow = nullptr) {
  const double t_issued = host_now();
  for (int i = 0; i < n; ++i) {
    (void)hipEventRecord(c->pipes[i].done, c->pipes[i].stream);
    (void)hipStreamWaitEvent(c->stream, c->pipes[i].done, 0);
  }
  // every pipeline's counters to pinned host memory behind the render, one
  // synchronisation (16 synchronous copies took ~0.3 ms of a 60 ms render)
  if (!c->host_ctr) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->host_ctr), kMaxPipes * sizeof(DevCounters), 0));
  for (int i = 0; i < n; ++i)
    HIPCHK(hipMemcpyAsync(&c->host_ctr[i], c->pipes[i].ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (std::getenv("WR_ISSUE_LOG"))  // diagnostics: host issue time vs the render's
    std::fprintf(stderr, "[wr issue] %d pipelines: issued in %.3f ms, done at %.3f ms\n", n,
                 (t_issued - t0_host) * 1e3, (host_now() - t0_host) * 1e3);
  HIPCHK(hipGetLastError());
  if (overflow) {  // (read whether or not stats are wanted)
    *overflow = 0;
    for (int i = 0; i < n; ++i) *overflow += c->host_ctr[i].overflow;
  }
  if (!st) return WR_OK;
  DevCounters sum{};
  for (int i = 0; i < n; ++i) {
    const DevCounters& h = c->host_ctr[i];
    sum.closest += h.closest;
    sum.shadow += h.shadow;
    sum.inner += h.inner;
    sum.leaves += h.leaves;
    sum.refs += h.refs;
    sum.tests += h.tests;
    sum.vm_queries += h.vm_queries;
    sum.vm_found += h.vm_found;
    sum.vm_merged += h.vm_merged;
    sum.bvh_nodes += h.bvh_nodes;
    sum.bvh_tests += h.bvh_tests;
    sum.kd_replay += h.kd_replay;
    sum.fallback += h.fallback;
    sum.verify_rays += h.verify_rays;
    sum.verify_bad += h.verify_bad;
    for (int k = 0; k < 8; ++k) sum.stamps[k] += h.stamps[k];
  }
  st->closest_rays += static_cast<int64_t>(sum.closest);
  st->shadow_rays += static_cast<int64_t>(sum.shadow);
  st->inner_visits += static_cast<int64_t>(sum.inner);
  st->leaf_visits += static_cast<int64_t>(sum.leaves);
  st->prim_refs += static_cast<int64_t>(sum.refs);
  st->prim_tests += static_cast<int64_t>(sum.tests);
  st->vm_queries += static_cast<int64_t>(sum.vm_queries);
  st->vm_found += static_cast<int64_t>(sum.vm_found);
  st->vm_merged += static_cast<int64_t>(sum.vm_merged);
  st->bvh_nodes += static_cast<int64_t>(sum.bvh_nodes);
  st->bvh_tests += static_cast<int64_t>(sum.bvh_tests);
  st->kd_replay_steps += static_cast<int64_t>(sum.kd_replay);
  st->fallback_rays += static_cast<int64_t>(sum.fallback);
  st->verify_rays += static_cast<int64_t>(sum.verify_rays);
  st->verify_mismatches += static_cast<int64_t>(sum.verify_bad);
  st->pipelines = std::max<int64_t>(st->pipelines, n);
  st->bvh_width = c->fast_on ? (c->wide_now ? c->wide_now : c->fs.wide) : 0;  // the tree this render searched
  if (c->trace_log && c->fast_on) {
    unsigned long long mx[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
      DevCounters h;
      HIPCHK(hipMemcpy(&h, c->pipes[i].ctr, sizeof h, hipMemcpyDeviceToHost));
      mx[0] = std::max(mx[0], h.stamps[5]);
      mx[1] = std::max(mx[1], h.stamps[6]);
      mx[2] += h.stamps[7];
    }
    unsigned long long ties = 0, why[4] = {0, 0, 0, 0}, lat[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
      DevCounters h;
      HIPCHK(hipMemcpy(&h, c->pipes[i].ctr, sizeof h, hipMemcpyDeviceToHost));
      ties += h.stamps[4];
      for (int k = 0; k < 4; ++k) why[k] += h.stamps[k];
      for (int k = 0; k < 12; ++k) lat[k] = (k % 2 == 0 && k < 6) ? std::max(lat[k], h.lat[k]) : lat[k] + h.lat[k];
    }
    std::fprintf(stderr,
                 "[wr bvh latency, us] membership max %.1f sum %.1f; ties max %.1f sum %.1f; walks max %.1f sum %.1f; "
                 "long many-leaf scans %llu\n",
                 lat[0] * 0.01, lat[1] * 0.01, lat[2] * 0.01, lat[3] * 0.01, lat[4] * 0.01, lat[5] * 0.01, lat[6]);
    if (lat[7] + lat[8])
      std::fprintf(stderr,
                   "[wr bvh tie split, us] collect %.1f, first leaves %.1f, second passes %llu, pair records used %llu; "
                   "scan membership %.1f\n",
                   lat[7] * 0.01, lat[8] * 0.01, lat[9], lat[11], lat[10] * 0.01);
    std::fprintf(stderr, "[wr bvh walks] many-leaf %llu, no visited hit %llu, crowd %llu, band %llu\n", why[0], why[1],
                 why[2], why[3]);
    unsigned long long ww[4] = {0, 0, 0, 0}, rounds[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
      DevCounters h;
      HIPCHK(hipMemcpy(&h, c->pipes[i].ctr, sizeof h, hipMemcpyDeviceToHost));
      for (int k = 0; k < 4; ++k) ww[k] += h.ww[k];
      for (int k = 0; k < 8; ++k) rounds[k] += h.rounds[k];
    }
    log_rounds(rounds);
    std::fprintf(stderr, "[wr bvh wave walks] %llu walks, %.1f rounds and %.1f nodes per walk, %llu serial fall-backs\n",
                 ww[0], ww[0] ? double(ww[1]) / ww[0] : 0.0, ww[0] ? double(ww[2]) / ww[0] : 0.0, ww[3]);
    std::fprintf(stderr, "[wr bvh tail] max nodes/ray %llu, max tests/ray %llu, rays > 256 nodes %llu, ties resolved by visit order %llu\n",
                 mx[0], mx[1], mx[2], ties);
  }
  if (c->stamps) {
    static const char* names[6] = {"refill", "walk", "leaf-setup", "pair-tests", "decision", "write"};
    double tot = 0;
    for (int k = 0; k < 6; ++k) tot += static_cast<double>(sum.stamps[k]);
    std::fprintf(stderr, "[wr stamps]");
    for (int k = 0; k < 6; ++k) std::fprintf(stderr, " %s=%.1f%%", names[k], 100.0 * sum.stamps[k] / std::max(1.0, tot));
    std::fprintf(stderr, " (wave-cycles %.3g)\n", tot);
  }
  st->seconds += host_now() - t0_host;
  if (c->timing) {
    std::vector<std::pair<float, float>> spans;  // traversal launches, ms from t_ref
    // diagnostics: WR_TIMELINE=<file> appends every timed launch (pipeline,
    // category, start ms, end ms from the render's start), no profiler needed
    FILE* tl = nullptr;
    if (const char* e = std::getenv("WR_TIMELINE")) tl = std::fopen(e, "a");
    for (int i = 0; i < n; ++i) {
      const Pipe& p = c->pipes[i];
      float prev = 0.f;
      (void)hipEventElapsedTime(&prev, c->t_ref, p.events[0]);
      for (size_t k = 1; k < p.ev_used; ++k) {
        float at = 0.f;
        (void)hipEventElapsedTime(&at, c->t_ref, p.events[k]);
        const int cat = p.ev_cat[k];
        st->kernel_ms[cat] += at - prev;
        st->kernel_launches[cat] += 1;
        if (cat == WR_K_TRACE) spans.emplace_back(prev, at);
        if (tl) std::fprintf(tl, "%d,%d,%.4f,%.4f\n", i, cat, prev, at);
        prev = at;
      }
    }
    if (tl) std::fclose(tl);
    std::sort(spans.begin(), spans.end());
    double wall = 0.0, lo = 0.0, hi = -1.0;
    for (const auto& sp : spans) {
      if (sp.first > hi) {
        if (hi > lo) wall += hi - lo;
        lo = sp.first;
        hi = sp.second;
      } else {
        hi = std::max<double>(hi, sp.second);
      }
    }
    if (hi > lo) wall += hi - lo;
    st->trace_wall_ms += wall;
  }
  return WR_OK;
}


int check_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(WR_E_NODEVICE, "no HIP device visible");
  return WR_OK;
}

}  // namespace

// =============================================================== C ABI
extern "C" {

const char* wr_last_error(void) { return wr::last_error(); }
int wr_api_version(void) { return WR_API_VERSION; }

int wr_request_hw_queues(int n) {
  if (n < 1 || n > 32) return fail(WR_E_ARG, "hardware queues: 1..32");
  if (g_hw_queues_latched.load() > 0) return hw_queues_in_effect();  // HIP already read it
  if (hw_queues_in_effect() < n && setenv("GPU_MAX_HW_QUEUES", std::to_string(n).c_str(), 1) != 0)
    return fail(WR_E_ARG, "setenv GPU_MAX_HW_QUEUES failed");
  return hw_queues_in_effect();
}

int wr_scene_load(const char* path, wr_scene** out) {
  if (!path || !out) return fail(WR_E_ARG, "null argument");
  *out = nullptr;
  auto* s = new (std::nothrow) wr_scene();
  if (!s) return fail(WR_E_ARG, "out of host memory");
  std::string err;
  if (!wr::load_scene(path, s->s, err)) {
    delete s;
    return fail(WR_E_IO, err);
  }
  *out = s;
  return WR_OK;
}

int wr_scene_from_desc(const wr_scene_desc* d, wr_scene** out) {
  if (!d || !out) return fail(WR_E_ARG, "null argument");
  *out = nullptr;
  auto* s = new (std::nothrow) wr_scene();
  if (!s) return fail(WR_E_ARG, "out of host memory");
  wr::SceneArrays a{d->n_prims, d->prim_type, d->prim_data, d->prim_mat, d->n_lights, d->light_tri, d->light_le,
                    d->n_materials, d->materials, d->cam_pos, d->cam_fwd, d->cam_up, d->cam_xres, d->cam_yres,
                    d->cam_hfov};
  std::string err;
  if (!wr::scene_from_arrays(a, s->s, err)) {
    delete s;
    return fail(WR_E_ARG, err);
  }
  *out = s;
  return WR_OK;
}

int wr_scene_info_get(const wr_scene* sc, wr_scene_info* o) {
  if (!sc || !o) return fail(WR_E_ARG, "null argument");
  const wr::Scene& s = sc->s;
  std::memset(o, 0, sizeof *o);
  o->nprims = static_cast<int32_t>(s.prims.size());
  for (const auto& p : s.prims) (p.type == wr::kTri ? o->ntriangles : o->nspheres)++;
  o->nlights = static_cast<int32_t>(s.lights.size());
  o->nmaterials = static_cast<int32_t>(s.mats.size());
  o->kd_depth_max = s.dep_max;
  for (const auto& n : s.nodes) (n.axis >= 0 ? o->kd_inner : o->kd_leaves)++;
  o->kd_refs = static_cast<int64_t>(s.refs.size());
  o->kd_max_stack = s.max_stack;
  o->missing_files = s.missing_files;
  o->camera_xres = s.cam.xres;
  o->camera_yres = s.cam.yres;
  o->device_bytes = static_cast<int64_t>(s.nodes.size() * 24 + s.refs.size() * 40 + s.prims.size() * 64);
  return WR_OK;
}

int wr_scene_fingerprint(const wr_scene* sc, uint64_t* out) {
  if (!sc || !out) return fail(WR_E_ARG, "null argument");
  *out = wr::scene_fingerprint(sc->s);
  return WR_OK;
}

int wr_scene_dump(const wr_scene* sc, const char* path) {
  if (!sc || !path) return fail(WR_E_ARG, "null argument");
  std::string txt = wr::dump_scene(sc->s);
  FILE* f = std::fopen(path, "w");
  if (!f) return fail(WR_E_IO, std::string("cannot write ") + path);
  std::fwrite(txt.data(), 1, txt.size(), f);
  std::fclose(f);
  return WR_OK;
}

void wr_scene_free(wr_scene* s) { delete s; }

int wr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---- wr_create, step by step.  A context under construction is held by a
// ContextPtr, so every early return ends it the way wr_destroy does.
struct ContextDelete {
  void operator()(wr_context* c) const { wr_destroy(c); }
};
using ContextPtr = std::unique_ptr<wr_context, ContextDelete>;

static int check_scene(const wr::Scene& s) {
  if (s.prims.empty()) return fail(WR_E_SCENE, "scene has no primitives");
  for (const auto& p : s.prims)  // the reference would index materials[] out of range
    if (p.mat >= static_cast<int>(s.mats.size()))
      return fail(WR_E_SCENE, "primitive material id " + std::to_string(p.mat) + " has no <material>");
  return WR_OK;
}

// streams, events and the pipelines' counters; the device's CU count
static int make_streams(wr_context& c) {
  if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c.t_ref, ev_flags(hipEventDefault)) != hipSuccess ||
      hipEventCreateWithFlags(&c.t_null, ev_flags(hipEventDisableTiming)) != hipSuccess)
    return fail(WR_E_HIP, "hipStreamCreate failed");
  // Pipeline 0 runs on the context stream: with GPU_MAX_HW_QUEUES = 4 (HIP's
  // default) a fifth stream would share a hardware queue with another and
  // serialize behind it (measured: 4 pipelines 648 Mrays/s on 5 streams, 734 on 4).
  for (Pipe& pp : c.pipes) {
    if (&pp == &c.pipes[0]) pp.stream = c.stream;
    else if (hipStreamCreateWithFlags(&pp.stream, hipStreamNonBlocking) == hipSuccess) pp.own_stream = true;
    if (!pp.stream || hipEventCreateWithFlags(&pp.done, ev_flags(hipEventDisableTiming)) != hipSuccess ||
        hipMalloc(&pp.ctr, sizeof(DevCounters)) != hipSuccess ||
        hipMalloc(&pp.sc, kGroup * sizeof(StepCounters)) != hipSuccess)
      return fail(WR_E_HIP, "pipeline stream / counters");
  }
  hipDeviceProp_t prop;
  const int cus = hipGetDeviceProperties(&prop, c.device) == hipSuccess ? prop.multiProcessorCount : 0;
  c.cus = cus > 0 ? cus : 256;
  return WR_OK;
}

// The knobs a context reads from the environment when it is created
// ("Runtime configuration").  Those whose effect depends on the
// scene's trees are read by read_scene_knobs.
static void read_knobs(wr_context& c) {
  // one pipeline per hardware queue of this process (HIP's GPU_MAX_HW_QUEUES,
  // default 4; pipeline 0 shares the context stream), at most 16: streams that
  // share a hardware queue serialize behind each other
  c.npipes = std::max(1, std::min(kMaxPipes, latch_hw_queues()));
  if (const char* e = std::getenv("WR_PIPES")) c.npipes = std::max(1, std::min(kMaxPipes, std::atoi(e)));
  if (const char* e = std::getenv("WR_PIECE_CAP")) c.piece_cap = std::max(64, std::atoi(e));
  if (const char* e = std::getenv("WR_PIECE_MIN")) c.piece_min = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("WR_TIE_WAVE_MAX")) c.tie_wave_max = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("WR_SCAN_WAVES")) c.scan_waves = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("WR_ISSUE_THREADS")) c.issue_threads = std::max(1, std::min(kMaxPipes, std::atoi(e)));
  if (const char* e = std::getenv("WR_BDPT_OVERLAP")) c.bdpt_overlap = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_QUEUE_SLAB")) c.queue_slab = std::atoi(e) != 0;
  // k_fast_resolve's grid, given in blocks per CU
  if (const char* e = std::getenv("WR_RESOLVE_GRID")) c.resolve_blocks = std::max(0, std::atoi(e)) * c.cus;
  if (const char* e = std::getenv("WR_RESOLVE_LIST")) c.resolve_list = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_BVH_WIDE_LAT")) c.lat_wide = std::atoi(e) != 0;
  // grid-stride vertex / resolve kernels: blocks per CU (knob WR_SHADE_GRID).
  // 2 = one resident round of both group members at 4 waves/SIMD; measured
  // against 8: C2 +0.9 %, C3 +1.9 %, VCM +1.3 % (16 and 32 lose 1-2 %).
  // With the path state in records (round 3) 1 does better again: C2 20 it.
  // +2.0 %, 256 it. +2.7 %, C4 +2.6 %, VCM +3 %, C3 -0.4 % (profiles/r3/shade_grid)
  int per_cu = 1;
  if (const char* e = std::getenv("WR_SHADE_GRID")) per_cu = std::max(1, std::min(64, std::atoi(e)));
  c.grid = std::max(256, c.cus * per_cu);
  if (const char* e = std::getenv("WR_TRACE_STAMPS")) c.stamps = std::atoi(e) != 0;  // triangle scenes only (upload_scene)
  if (const char* e = std::getenv("WR_TRACE_LOG")) c.trace_log = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_TRACE_DENSE")) c.api_dense = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_TRACE_NO_CUT")) c.no_cut = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_VCM_CELL")) c.vcm_cell = std::min(8.f, std::max(0.25f, (float)std::atof(e)));
}

// The knobs that act on what the scene's trees turn out to be: read here,
// applied by the steps that build them.  -1: not set.
struct SceneKnobs {
  int trace_wide = -1;         // test knob: 1 runs the 32-bit-stack KD walk on any tree
  int trace_waves_per_cu = -1;  // diagnostic: caps the KD walk's resident waves
  int bvh_wide = -1;           // 2 | 4 (| 8 in a WR_BVH_WIDE=8 build) forces the search tree's width
  int walk_wave = -1;          // 0: no kd_walk_wave
  int pair_record = -1;        // near-ties: 2 the pair list, 1 the record in the tie list only, 0 neither
  int fast_waves_per_cu = -1;  // diagnostic: caps the search's resident waves
  int trace_bvh = -1;          // 0: contexts start in the reference KD walk
  int bvh_diag = 0;
  int bvh_verify = -1;
  // the search's top set in LDS (wr_fast.h search_wg_bytes): node budgets of
  // the binary and the 4-wide tree (0: none; WR_BVH_TOP=0 alone is the
  // one-wave launch without a copy) and the waves per workgroup
  int bvh_top = -1, bvh_top4 = -1, bvh_top_wg = -1;
};
static SceneKnobs read_scene_knobs() {
  SceneKnobs k;
  if (const char* e = std::getenv("WR_TRACE_WIDE")) k.trace_wide = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_TRACE_WAVES_PER_CU")) k.trace_waves_per_cu = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("WR_BVH_WIDE")) k.bvh_wide = std::atoi(e);
  if (const char* e = std::getenv("WR_WALK_WAVE")) k.walk_wave = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_PAIR_RECORD")) k.pair_record = std::max(0, std::min(2, std::atoi(e)));
  if (const char* e = std::getenv("WR_FAST_WAVES_PER_CU")) k.fast_waves_per_cu = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("WR_TRACE_BVH")) k.trace_bvh = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_BVH_DIAG")) k.bvh_diag = std::atoi(e);
  if (const char* e = std::getenv("WR_BVH_VERIFY")) k.bvh_verify = std::atoi(e) != 0;
  if (const char* e = std::getenv("WR_BVH_TOP")) k.bvh_top = std::max(0, std::min(1024, std::atoi(e)));
  if (const char* e = std::getenv("WR_BVH_TOP4")) k.bvh_top4 = std::max(0, std::min(512, std::atoi(e)));
  if (const char* e = std::getenv("WR_BVH_TOP_WG")) k.bvh_top_wg = std::max(1, std::min(kMaxSearchWG, std::atoi(e)));
  return k;
}

// the flattened scene (wr_flatten.h) into the scene arena, and what the
// context keeps of it
static int upload_scene(wr_context& c, const wr::Scene& s, const wr::SceneFlat& f, const SceneKnobs& k) {
  DevScene& d = c.ds;
  Upload up;
  up.add(&d.nrec, f.nrec);
  up.add(&d.nrec_r, f.nrec_r);
  up.add(&d.nrec3, f.nrec3);
  up.add(&d.ref_a, f.ref_a);
  up.add(&d.ref_b, f.ref_b);
  up.add(&d.ref_c, f.ref_c);
  up.add(&d.prim_mat, f.prim_mat);
  up.add(&d.prim_type, f.prim_type);
  up.add(&d.prim_tri, f.prim_tri);
  up.add(&d.prim_tri2, f.prim_tri2);
  up.add(&d.prim_sph, f.prim_sph);
  up.add(&d.prim_sbox0, f.prim_sbox0);
  up.add(&d.prim_sbox1, f.prim_sbox1);
  up.add(&d.prim_rec, f.prim_rec);
  up.add(&d.lights, f.lights, f.lights.size() + 1);
  up.add(&d.mats, f.mats);
  up.room(&c.ctr, 1);
  if (int rc = up.commit(c.scene_mem, "scene")) return rc;
  d.nlights = static_cast<int>(f.lights.size());
  d.root_l = v3(s.root_l.x, s.root_l.y, s.root_l.z);
  d.root_r = v3(s.root_r.x, s.root_r.y, s.root_r.z);
  d.max_stack = f.max_stack;
  d.cam.pos = v3(s.cam.pos.x, s.cam.pos.y, s.cam.pos.z);
  d.cam.fwd = v3(s.cam.fwd.x, s.cam.fwd.y, s.cam.fwd.z);
  d.cam.xres = s.cam.xres;
  d.cam.yres = s.cam.yres;
  d.cam.plane_dist = s.cam.plane_dist;
  std::memcpy(d.cam.w2r, s.cam.w2r, sizeof d.cam.w2r);
  std::memcpy(d.cam.r2w, s.cam.r2w, sizeof d.cam.r2w);
  c.scene_bytes = static_cast<int64_t>(c.scene_mem.used);
  c.sph_r = s.sph_r;
  c.nmats = static_cast<int>(f.mats.size());
  c.spheres = f.spheres;
  c.has_sph = f.spheres ? 1 : 0;
  c.stamps = c.stamps && !c.spheres;
  c.narrow = f.narrow && k.trace_wide <= 0;
  return WR_OK;
}

// persistent traversal grid: the one-wave workgroups that fit at once (LDS stack
// and registers); more would only queue behind the first wave of blocks
static void size_kd_grids(wr_context& c, const SceneKnobs& k) {
  auto resident = [&](int mode) {
    const size_t lds = trace_lds_bytes(c.ds.max_stack, c.narrow, mode == TRACE_DENSE);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trace_kernel(false, c.spheres, c.narrow, false, mode),
                                                     kTraceBlock, lds) != hipSuccess ||
        per_cu <= 0)
      per_cu = 8;
    // (leaving room for the other pipelines' shading kernels)
    if (k.trace_waves_per_cu > 0) per_cu = std::min(per_cu, k.trace_waves_per_cu);
    return per_cu;
  };
  c.trace_blocks = c.cus * resident(TRACE_PLAIN);
  c.trace_blocks_dense = c.cus * resident(TRACE_DENSE);
}

// the search tree's width: 4-wide for scenes whose binary tree outgrows
// the L2 (its nodes then come from the Infinity Cache / HBM, and one
// 128-byte node holds two of the binary tree's levels: C4 +5-8 %, while
// L2-resident scenes lose 1-4 %: DESIGN.md 4b); WR_BVH_WIDE=2|4 forces
static int bvh_width(const wr::Scene& s, const SceneKnobs& k) {
  size_t tris = 0;
  for (const wr::Prim& p : s.prims) tris += p.type == wr::kTri ? 1 : 0;
  int wide = WR_BVH_WIDE;
  if (wide == 2 && tris >= wrf::kWide4MinTris) wide = 4;
  if (k.bvh_wide == 2 || k.bvh_wide == 4 || (k.bvh_wide == 8 && WR_BVH_WIDE == 8)) wide = k.bvh_wide;
  // the 8-wide search is instantiated for triangle leaves only: a scene with
  // spheres searches the 4-wide tree, whose kernels run the sphere test
  if (wide == 8 && tris != s.prims.size()) wide = 4;
  return wide;
}

// ---- verified-BVH traversal data (wr_bvh.h): BVH nodes, triangle records
// in leaf order, and the KD root paths of every primitive's leaves; then the
// search's grid.  A scene build_fast declines keeps the KD walk (fast_ok false).
static int upload_bvh(wr_context& c, const wr::Scene& s, const wr::SceneFlat& f, const SceneKnobs& k) {
  const int wide = bvh_width(s, k);
  wrf::FastHost fh;
  // the top sets' budgets: WR_BVH_TOP / WR_BVH_TOP4, else the build's defaults
  // (the quantised 4-wide and the 8-wide build options search without one)
  const int top = k.bvh_top >= 0 ? k.bvh_top : wrf::kTopNodes;
  const int top4 = WR_BVH4_QUANT ? 0 : k.bvh_top4 >= 0 ? k.bvh_top4 : k.bvh_top == 0 ? 0 : wrf::kTop4Nodes;
  wrf::build_fast(s, fh, wide, wide == 2, top, top4);
  if (!fh.ok) return WR_OK;
  FastScene& fs = c.fs;
  Upload up;
  up.add(&fs.nodes, fh.nodes);
  up.add(&fs.tris, fh.tris);
  up.add(&fs.prim_leaf_off, fh.prim_leaf_off);
  up.add(&fs.prim_leaf, fh.prim_leaf, 1);
  up.add(&fs.prim_leaf_pos, fh.prim_leaf_pos, std::max<size_t>(1, fh.prim_leaf.size()));
  up.add(&fs.path, fh.path);
  up.add(&fs.node_path, fh.node_path);
  up.add(&fs.node_cell, fh.node_cell);
  up.add(&fs.prim_rec, fh.prim_rec);
  up.add(&fs.nodes4, fh.nodes4);
  up.add(&fs.nodes8, fh.nodes8);
  if (int rc = up.commit(c.fast_mem, "BVH")) return rc;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int a = 0; a < 3; ++a) {
    lo[a] = std::min(fh.nodes[0].b[a], fh.nodes[0].b[6 + a]);
    hi[a] = std::max(fh.nodes[0].b[3 + a], fh.nodes[0].b[9 + a]);
  }
  fs.lo = v3(lo[0], lo[1], lo[2]);
  fs.hi = v3(hi[0], hi[1], hi[2]);
  fs.sph = fh.spheres > 0 ? 1 : 0;
  fs.org_lo = v3(fh.org_lo[0], fh.org_lo[1], fh.org_lo[2]);
  fs.org_hi = v3(fh.org_hi[0], fh.org_hi[1], fh.org_hi[2]);
  // the search's stack holds BVH entries only; the hard rays' kernel walks
  // both trees
  fs.wide = wide;
  fs.sdepth = wide == 8 ? 7 * fh.depth8 + 1 : wide == 4 ? 3 * fh.depth4 + 1 : fh.depth + 1;
  if (wide == 2 && !fh.nodes4.empty()) {
    c.sdepth4 = 3 * fh.depth4 + 1;
    c.fs4_ok = true;
  }
  fs.depth = std::max(fh.depth + 1, c.ds.max_stack + 1);
  fs.walk_wave = f.walk_wave && k.walk_wave != 0 ? 1 : 0;
  fs.pair = k.pair_record >= 0 ? k.pair_record : 2;
  fs.diag = k.bvh_diag;
  c.fast_ok = true;
  // the search's workgroup: one wave and no copy without a top set (the
  // launch as it was before the top set), else WR_BVH_TOP_WG waves, fewer
  // where a deep tree's stack columns would outgrow the CU's LDS
  fs.ntop = wide == 4 ? fh.ntop4 : wide == 2 ? fh.ntop : 0;
  c.ntop4 = c.fs4_ok ? fh.ntop4 : 0;
  int wg = k.bvh_top_wg > 0 ? k.bvh_top_wg : (fs.ntop > 0 || c.ntop4 > 0) ? kSearchWG : 1;
  constexpr size_t kCuLds = 160 * 1024;
  auto wg_bytes = [&](int w) {
    size_t b = search_wg_bytes(fs.sdepth, wide, true, fs.ntop, w);
    if (c.fs4_ok) b = std::max(b, search_wg_bytes(c.sdepth4, 4, true, c.ntop4, w));
    return b;
  };
  while (wg > 1 && wg_bytes(wg) > kCuLds) wg /= 2;
  if (wg_bytes(wg) > kCuLds) return fail(WR_E_ARG, "the search's top set and stack outgrow the LDS");
  c.search_wg = wg;
  // a workgroup of more than 64 KB of dynamic LDS asks for it per kernel
  if (wg_bytes(wg) > 64 * 1024)
    for (int cnt = 0; cnt < 2; ++cnt)
      for (int rl = 0; rl < 2; ++rl)
        for (int w : {wide, c.fs4_ok ? 4 : wide}) {
          const TraceFastKernel kf = cnt ? trace_fast_kernel<true>(w, fs.sph, rl) : trace_fast_kernel<false>(w, fs.sph, rl);
          HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kf), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(wg_bytes(wg))));
          if (w == 8) continue;  // (no slab form of the 8-wide build option)
          const TraceFastKernelOf<true> ks =
              cnt ? trace_fast_kernel<true, true>(w, fs.sph, rl) : trace_fast_kernel<false, true>(w, fs.sph, rl);
          HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(ks), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(wg_bytes(wg))));
        }
  const size_t wgb = search_wg_bytes(fs.sdepth, wide, c.resolve_list, fs.ntop, wg);
  int per_cu = 0;  // workgroups
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trace_fast_kernel<false>(wide, fs.sph, c.resolve_list),
                                                   kTraceBlock * wg, wgb) != hipSuccess ||
      per_cu <= 0)
    per_cu = std::max(1, std::min(8 / wg, static_cast<int>(kCuLds / wgb)));
  int waves_per_cu = per_cu * wg;
  if (k.fast_waves_per_cu > 0) waves_per_cu = std::max(wg, std::min(waves_per_cu, k.fast_waves_per_cu) / wg * wg);
  c.fast_blocks = c.cus * waves_per_cu;
  // the verified BVH is the default traversal (same answers as the KD
  // walk); WR_TRACE_BVH=0 selects the walk
  c.fast_on = k.trace_bvh != 0;
  if (k.bvh_verify >= 0) c.verify = k.bvh_verify != 0;
  if (c.trace_log)
    std::fprintf(stderr,
                 "[wr bvh] nodes %zu tris %zu depth %d lds %zu B/wave + %zu B list and settle buffers, ntop %d (4-wide %d) "
                 "WG %d waves, %zu B LDS/workgroup, %d waves/CU -> grid %d waves; kd grid %d\n",
                 fh.nodes.size(), fh.tris.size(), fs.sdepth, search_lds_bytes(fs.sdepth, wide),
                 c.resolve_list ? search_rl_bytes() : size_t(0), fs.ntop, c.ntop4, wg, wgb, waves_per_cu, c.fast_blocks,
                 c.trace_blocks);
  return WR_OK;
}

int wr_create(const wr_scene* sc, int device, wr_context** out) {
  if (!sc || !out) return fail(WR_E_ARG, "null argument");
  *out = nullptr;
  latch_hw_queues();  // before the library's first HIP call: the value HIP reads
  if (int rc = check_device()) return rc;
  DeviceGuard dg;
  const wr::Scene& s = sc->s;
  if (int rc = check_scene(s)) return rc;
  HIPCHK(hipSetDevice(device));
  ContextPtr c(new wr_context());
  c->device = device;
  if (int rc = make_streams(*c)) return rc;
  read_knobs(*c);
  const SceneKnobs k = read_scene_knobs();
  wr::SceneFlat flat;
  wr::flatten_scene(s, flat);
  if (int rc = upload_scene(*c, s, flat, k)) return rc;
  size_kd_grids(*c, k);
  if (int rc = upload_bvh(*c, s, flat, k)) return rc;
  *out = c.release();
  return WR_OK;
}

int wr_set_trace_mode(wr_context* c, int mode) {
  if (!c || (mode != WR_TRACE_REFERENCE && mode != WR_TRACE_BVH)) return fail(WR_E_ARG, "bad trace mode");
  if (mode == WR_TRACE_BVH && !c->fast_ok) return fail(WR_E_SCENE, "the scene has no verified BVH (empty, too large, or a triangle with nearly collinear vertices)");
  c->fast_on = mode == WR_TRACE_BVH;
  for (wr_context* d : c->subs) d->fast_on = c->fast_on;
  return WR_OK;
}

int wr_set_pipelines(wr_context* c, int n) {
  if (!c || n < 1 || n > kMaxPipes) return fail(WR_E_ARG, "pipelines must be in 1.." + std::to_string(kMaxPipes));
  c->npipes = n;
  for (wr_context* d : c->subs) d->npipes = n;
  return WR_OK;
}

void wr_destroy(wr_context* c) {
  if (!c) return;
  DeviceGuard dg;
  for (wr_context* d : c->subs) wr_destroy(d);
  c->subs.clear();
  for (ncclComm_t m : c->dev_comms) (void)rccl().destroy(m);
  c->dev_comms.clear();
  if (c->comm) (void)rccl().destroy(c->comm);
  c->comm = nullptr;
  (void)hipSetDevice(c->device);  // the members' destructors free on it
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (Pipe& p : c->pipes)
    if (p.stream) (void)hipStreamSynchronize(p.stream);
  for (wr_photon_map* m : c->photon_maps) delete m;  // maps the caller did not free (their indices go below)
  c->photon_maps.clear();
  for (wr_points* x : c->points) delete x;  // indices the caller did not free
  c->points.clear();
  delete c;
}

// the context's API scratch block, at least `bytes` (the stream is idle
// between API calls: every call ends with a stream synchronize)
static int api_scratch(wr_context* c, size_t bytes) { return c->api_tmp.grow(bytes); }

// ---- device-resident ray batches (wr_*_dev, wr_camera_rays).
// The arrays of every call that takes device arrays go through wr_args.h's
// checker, with HIP's pointer lookup as its classifier.  A failed query leaves
// HIP's sticky error set: cleared here.
static wr::PtrClass classify_pointer(const void* p) {
  hipPointerAttribute_t at{};
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) (void)hipGetLastError();
  return {e == hipSuccess, at.type == hipMemoryTypeDevice, at.device};
}
static int check_dev_args(const wr_context* c, const char* call, std::initializer_list<wr::Arg> args,
                          const char* host_goes_to) {
  const wr::ArgError e = wr::check_args(call, args, c->device, host_goes_to, classify_pointer);
  return e ? fail(e.code, e.msg) : WR_OK;
}
// the context's device current, its stream after the caller's work on the
// legacy null stream (like a render): before the first operation an array call
// enqueues
static int api_order(wr_context* c) {
  HIPCHK(hipSetDevice(c->device));
  (void)hipEventRecord(c->t_null, nullptr);
  (void)hipStreamWaitEvent(c->stream, c->t_null, 0);
  return WR_OK;
}
static int api_finish(wr_context* c) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return WR_OK;
}

// One queue of nb rays traced on the context stream with the context's own
// counters, t2 scratch and spill area (the API calls' trace; the renders' is
// tslot).  count: the counting kernels (WR_TRACE_LOG).
static int api_trace(wr_context* c, const RayQueue& rays, size_t nb, bool count, int mode) {
  c->timing = false;
  Timer tm(c, nullptr);
  HIPCHK(hipMemsetAsync(c->ctr, 0, sizeof(DevCounters), c->stream));
  if (c->fast_on)
    if (int rc = c->api_t2.grow(5 * nb)) return rc;  // as ensure_t2
  QueueList ql;
  ql.add(rays, static_cast<int>(nb));
  if (c->fast_on && !c->api_spill.p && max_spill_entries(c) > 0)
    if (int rc = c->api_spill.grow(max_spill_entries(c) * size_t(c->fast_blocks) * 64)) return rc;
  const TraceSlot ts{&c->ctr->fetch, c->api_t2.p, c->api_t2.n / 5, &c->ctr->hard[0], c->api_spill.p, &c->ctr->rlist};
  trace_launch(c, c->stream, c->ctr, ts, tm, count, ql.Q, ql.max_rays, c->api_dense ? TRACE_DENSE : mode, true);
  return WR_OK;
}

// wr_trace_closest / wr_occluded and their _dev forms: prep kernel -> SoA queue
// -> trace_launch -> finish kernel.  Host arrays (on_device false) are staged
// in the context's scratch and the answers copied back; device arrays are read
// and written where they lie, after the caller's work on the legacy null
// stream, and the scratch holds only the queue, (t, prim), cut and the counter.
static int trace_api(wr_context* c, const wr_ray* rays, const float* targets, int64_t n64, wr_hit* hits,
                     uint8_t* occ, bool on_device = false) {
  if (!c || (!rays && n64) || n64 < 0) return fail(WR_E_ARG, "bad argument");
  if (n64 == 0) return WR_OK;
  if (n64 > (1 << 28)) return fail(WR_E_ARG, "at most 2^28 rays per call");
  const int n = static_cast<int>(n64);
  const size_t nb = size_t(n);
  if (on_device) {
    const wr::Arg in = wr::in(rays, nb * sizeof(wr_ray), "rays");
    if (int rc = occ ? check_dev_args(c, "wr_occluded_dev",
                                      {in, wr::in(targets, nb * 12, "targets"), wr::out(occ, nb, "occluded")},
                                      "wr_occluded")
                     : check_dev_args(c, "wr_trace_closest_dev", {in, wr::out(hits, nb * sizeof(wr_hit), "hits")},
                                      "wr_trace_closest"))
      return rc;
    if (int rc = api_order(c)) return rc;
  } else {  // (stages its own copies on the stream: nothing of the caller's to wait for)
    HIPCHK(hipSetDevice(c->device));
  }
  // one scratch block: rays, SoA queue, results, counters (kept on the
  // context: no allocation per call, nothing to free on an error return)
  const size_t bytes = nb * ((on_device ? 0 : sizeof(wr_ray) + 12 + sizeof(wr_hit) + 1) + 4 * 11) + 16 * 256;
  if (int rc = api_scratch(c, bytes)) return rc;
  char* q = c->api_tmp.p;
  auto take = [&](size_t sz) { char* r = q; q += (sz + 255) & ~size_t(255); return r; };
  const wr_ray* dr = on_device ? rays : reinterpret_cast<wr_ray*>(take(nb * sizeof(wr_ray)));
  float* o3 = reinterpret_cast<float*>(take(nb * 12));
  float* d3 = reinterpret_cast<float*>(take(nb * 12));
  float* tmn = reinterpret_cast<float*>(take(nb * 4));
  float* tmx = reinterpret_cast<float*>(take(nb * 4));
  float* tt = reinterpret_cast<float*>(take(nb * 4));
  int* pr = reinterpret_cast<int*>(take(nb * 4));
  const float* dtg = on_device ? targets : reinterpret_cast<float*>(take(nb * 12));
  float* dcut = reinterpret_cast<float*>(take(nb * 4));
  wr_hit* dh = on_device ? hits : reinterpret_cast<wr_hit*>(take(nb * sizeof(wr_hit)));
  uint8_t* dox = on_device ? occ : reinterpret_cast<uint8_t*>(take(nb));
  int* cnt = reinterpret_cast<int*>(take(sizeof(int)));
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(const_cast<wr_ray*>(dr), rays, nb * sizeof(wr_ray), hipMemcpyHostToDevice, c->stream));
    if (occ)
      HIPCHK(hipMemcpyAsync(const_cast<float*>(dtg), targets, nb * 12, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemcpyAsync(cnt, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
  const int g = std::max(1, std::min(c->grid, (n + 255) / 256));
  hipLaunchKernelGGL(k_api_prep, dim3(g), dim3(256), 0, c->stream, dr, n, occ ? 1 : 0, o3, d3, tmn, tmx, dtg, dcut);
  // (WR_TRACE_LOG: the counting kernels, for the rounds line below)
  if (int rc = api_trace(c, rq(o3, d3, n, cnt, tt, pr, occ ? dcut : nullptr, tmn, tmx), nb, c->trace_log,
                         occ ? TRACE_CUT : TRACE_PLAIN))
    return rc;
  hipLaunchKernelGGL(k_api_finish, dim3(g), dim3(256), 0, c->stream, c->ds, o3, d3, tt, pr, dtg, n, dh,
                     occ ? dox : nullptr);
  HIPCHK(hipGetLastError());
  if (!on_device) {
    if (occ) HIPCHK(hipMemcpyAsync(occ, dox, nb, hipMemcpyDeviceToHost, c->stream));
    else HIPCHK(hipMemcpyAsync(hits, dh, nb * sizeof(wr_hit), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->trace_log && c->fast_on) {
    DevCounters h;
    HIPCHK(hipMemcpy(&h, c->ctr, sizeof h, hipMemcpyDeviceToHost));
    log_rounds(h.rounds);
  }
  return WR_OK;
}

extern "C++" {
// ---- several devices: run fn(device context, index) on every device of c at
// once (devices[0] on the calling thread), first error wins
template <class Fn>
static int for_each_device(wr_context* c, Fn fn) {
  std::vector<wr_context*> dev{c};
  dev.insert(dev.end(), c->subs.begin(), c->subs.end());
  const int n = static_cast<int>(dev.size());
  std::vector<int> rc(n, WR_OK);
  std::vector<std::string> msg(n);
  std::vector<std::thread> th;
  for (int k = 1; k < n; ++k)
    th.emplace_back([&, k] {
      rc[k] = fn(dev[k], k);
      if (rc[k] != WR_OK) msg[k] = wr::last_error();
    });
  rc[0] = fn(dev[0], 0);
  if (rc[0] != WR_OK) msg[0] = wr::last_error();
  for (auto& t : th) t.join();
  for (int k = 0; k < n; ++k)
    if (rc[k] != WR_OK) return fail(rc[k], "device " + std::to_string(dev[k]->device) + ": " + msg[k]);
  return WR_OK;
}

}  // extern "C++"

static int trace_multi(wr_context* c, const wr_ray* rays, const float* targets, int64_t n, wr_hit* hits,
                       uint8_t* occ) {
  if (c->subs.empty() || n < 1024) return trace_api(c, rays, targets, n, hits, occ);
  const int64_t nd = 1 + static_cast<int64_t>(c->subs.size());
  return for_each_device(c, [&](wr_context* d, int k) {  // contiguous ray ranges
    const int64_t lo = n * k / nd, hi = n * (k + 1) / nd;
    return trace_api(d, rays + lo, targets ? targets + 3 * lo : nullptr, hi - lo, hits ? hits + lo : nullptr,
                     occ ? occ + lo : nullptr);
  });
}

int wr_trace_closest(wr_context* c, const wr_ray* rays, int64_t n, wr_hit* hits) {
  if (!hits && n) return fail(WR_E_ARG, "null hits");
  if (!c || (!rays && n) || n < 0) return fail(WR_E_ARG, "bad argument");
  DeviceGuard dg;
  return trace_multi(c, rays, nullptr, n, hits, nullptr);
}

int wr_occluded(wr_context* c, const wr_ray* rays, const float* targets, int64_t n, uint8_t* occluded) {
  if ((!targets || !occluded) && n) return fail(WR_E_ARG, "null targets / output");
  if (!c || (!rays && n) || n < 0) return fail(WR_E_ARG, "bad argument");
  DeviceGuard dg;
  return trace_multi(c, rays, targets, n, nullptr, occluded);
}

// Device arrays on the context's device (devices[0] of a multi-device context,
// not shared out, as wr_render_features).
int wr_trace_closest_dev(wr_context* c, const wr_ray* rays, int64_t n, wr_hit* hits) {
  if (!c) return fail(WR_E_ARG, "null context");
  if ((!rays || !hits) && n) return fail(WR_E_ARG, "null rays / hits");
  DeviceGuard dg;
  return trace_api(c, rays, nullptr, n, hits, nullptr, true);
}

int wr_occluded_dev(wr_context* c, const wr_ray* rays, const float* targets, int64_t n, uint8_t* occluded) {
  if (!c) return fail(WR_E_ARG, "null context");
  if ((!rays || !targets || !occluded) && n) return fail(WR_E_ARG, "null rays / targets / output");
  DeviceGuard dg;
  return trace_api(c, rays, targets, n, nullptr, occluded, true);
}

static int film_target(wr_context* c, float* film, int film_on_device, size_t nfloat, float** dev) {
  if (film_on_device) {
    *dev = film;
    return WR_OK;
  }
  if (int rc = c->film_tmp.grow(nfloat)) return rc;
  HIPCHK(hipMemsetAsync(c->film_tmp.p, 0, nfloat * sizeof(float), c->stream));
  *dev = c->film_tmp.p;
  return WR_OK;
}

static int film_return(wr_context* c, float* film, int film_on_device, size_t nfloat) {
  if (film_on_device) return WR_OK;
  std::vector<float> tmp(nfloat);
  HIPCHK(hipMemcpyAsync(tmp.data(), c->film_tmp.p, nfloat * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < nfloat; ++i) film[i] = film[i] + tmp[i];
  return WR_OK;
}

// ---- moments renders: the caller's two films and the pipelines' pass films.
// Host films share one device block of 2 nf floats (film, then film_sq).
struct MomentFilms {
  float* sq = nullptr;   // the caller's film_sq (nullptr: a plain render)
  float* dsq = nullptr;  // its device film
  bool on() const { return sq != nullptr; }
};
static int moments_target(wr_context* c, float* film, MomentFilms& M, int films_on_device, size_t nf, float** dev) {
  if (!M.on()) return film_target(c, film, films_on_device, nf, dev);
  if (int rc = film_target(c, film, films_on_device, 2 * nf, dev)) return rc;
  M.dsq = films_on_device ? M.sq : *dev + nf;
  return WR_OK;
}
static int moments_return(wr_context* c, float* film, const MomentFilms& M, int films_on_device, size_t nf) {
  if (!M.on()) return film_return(c, film, films_on_device, nf);
  if (films_on_device) return WR_OK;
  std::vector<float> tmp(2 * nf);
  HIPCHK(hipMemcpyAsync(tmp.data(), c->film_tmp.p, 2 * nf * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < nf; ++i) film[i] = film[i] + tmp[i];
  for (size_t i = 0; i < nf; ++i) M.sq[i] = M.sq[i] + tmp[nf + i];
  return WR_OK;
}
// kGroup pass films of nf floats on each of the pipelines [0, np), zero.  On the
// context stream, which every pipeline waits for at begin_render.  Only moments
// renders come here: a plain render allocates none of this.
static int ensure_moments(wr_context* c, int np, size_t nf) {
  const bool dirty = c->mom_dirty;  // a moments render failed under way: its launches may still run
  if (dirty) HIPCHK(hipDeviceSynchronize());
  for (int i = 0; i < kMaxPipes; ++i) {
    Pipe& p = c->pipes[i];
    const size_t had = p.mom[kGroup - 1].n;  // grown in order: the last one is the smallest
    const bool grow = i < np && had < nf;
    if (!grow && !(dirty && had)) continue;
    for (DevBuf<float>& f : p.mom) {
      if (grow)
        if (int rc = f.grow(nf)) return rc;
      HIPCHK(hipMemsetAsync(f.p, 0, f.n * sizeof(float), c->stream));
    }
  }
  c->mom_dirty = false;
  return WR_OK;
}
// fold pass film m of the pipeline into the caller's films, behind the pass's
// last launch on the pipeline's stream
static void fold_launch(wr_context* c, Pipe& pp, int m, float* dfilm, float* dsq, size_t nf) {
  const size_t rounds = (nf + 4 * kFoldBlock - 1) / (4 * kFoldBlock);
  const int g = static_cast<int>(std::max<size_t>(1, std::min<size_t>(rounds, size_t(c->cus) * 8)));
  hipLaunchKernelGGL(k_film_fold, dim3(g), dim3(kFoldBlock), 0, pp.stream, dfilm, dsq, pp.mom[m].p, nf);
  Timer(c, &pp).mark(WR_K_OTHER);
}

// Issues one round of launches: step by step across the pipelines [0, np),
// on c->issue_threads host threads (pipeline i on thread i % T, each thread
// stepping through its own pipelines; their streams are independent).
// fn(pipeline, step) issues one step of one pipeline.
extern "C++" {
template <class Fn>
static int issue_round(wr_context* c, int live, int nsteps, Fn&& fn, int np) {
  const int T = std::min(c->issue_threads, std::max(1, live));
  auto run = [&](int t) -> int {
    for (int step = 0; step < nsteps; ++step)
      for (int pi = t; pi < np; pi += T)
        if (int rc = fn(pi, step)) return rc;
    return WR_OK;
  };
  if (T <= 1) return run(0);
  std::vector<int> rcs(T, WR_OK);
  std::vector<std::string> msg(T);  // wr_last_error is thread-local: carry it over
  std::vector<std::thread> th;
  th.reserve(T - 1);
  for (int t = 1; t < T; ++t)
    th.emplace_back([&, t] {
      const hipError_t e = hipSetDevice(c->device);
      if (e != hipSuccess) {
        rcs[t] = WR_E_HIP;
        msg[t] = std::string("issue thread hipSetDevice: ") + hipGetErrorString(e);
        return;
      }
      rcs[t] = run(t);
      if (rcs[t] != WR_OK) msg[t] = wr::last_error();
    });
  rcs[0] = run(0);
  if (rcs[0] != WR_OK) msg[0] = wr::last_error();
  for (auto& x : th) x.join();
  for (int t = 0; t < T; ++t)
    if (rcs[t] != WR_OK) return fail(rcs[t], msg[t]);
  return WR_OK;
}
}  // extern "C++"

static int check_bdpt(const wr_context* c, const wr_bdpt_params* prm, const float* film) {
  if (!c || !prm || !film) return fail(WR_E_ARG, "null argument");
  if (prm->width <= 0 || prm->height <= 0 || prm->iterations < 0) return fail(WR_E_ARG, "bad film size");
  if (static_cast<int64_t>(prm->width) * prm->height >= (1 << 30) / (kVMax + 2))
    return fail(WR_E_ARG, "film too large for one context");
  if (prm->max_path_length > kVMax + 1)
    return fail(WR_E_ARG, "max_path_length > 10 is not supported (light-vertex store sized for the reference's 10)");
  if (c->ds.nlights <= 0) return fail(WR_E_SCENE, "BDPT needs at least one area light");
  return WR_OK;
}
// camera-order unit of a BDPT piece: whole 8-row bands when the film is tiled
// (camera_gen_one), else 64 paths
static int bdpt_unit(const wr_bdpt_params* prm) {
  return ((prm->width % 8) == 0 && (prm->height % 8) == 0) ? 8 * prm->width : 64;
}
// One device: the flattened path-iterations [f_lo, f_hi) of the render
// (iteration iter_begin + f / P, path f % P; whole units).
// film_sq != nullptr: a moments render (whole iterations per pipeline, each into
// a pass film that is folded into film / film_sq when the iteration is done).
static int render_bdpt_one(wr_context* c, const wr_bdpt_params* prm, int64_t f_lo, int64_t f_hi, float* film,
                           int film_on_device, wr_stats* st, float* film_sq = nullptr) {
  HIPCHK(hipSetDevice(c->device));
  const double t0 = host_now();
  const int P = prm->width * prm->height;
  // pieces of (iteration, path range) per pipeline, buffers sized for the largest
  const int unit = bdpt_unit(prm);
  const int cap = piece_capacity(c, P, unit);
  const int fit = pipelines_that_fit(c, 1, cap, kGroup, c->npipes);
  if (fit < 1) return WR_E_HIP;  // message set by the allocation
  MomentFilms M;
  M.sq = film_sq;
  const PiecePlan plan = plan_pieces(f_lo, f_hi, P, unit, cap, fit, c->piece_min, M.on());
  const int np = plan.pipes();
  // a render too short to fill the pipelines that fit, each holding one
  // group, is latency-bound: its searches take the 4-wide tree when the scene
  // has one beside the binary (DESIGN.md 4b, C2 at 1 iteration +2.3 %);
  // renders that fill the pipelines keep the binary (C2 at 20 iterations,
  // 16 pipelines of one group each: 4-wide -3 %)
  size_t most_groups = 0;
  for (const auto& pp : plan.per_pipe) most_groups = std::max(most_groups, pp.size());
  struct WideNow {
    wr_context* c;
    ~WideNow() {
      c->wide_now = 0;
      c->lat_now = false;
    }
  } wide_guard{c};
  c->lat_now = np < fit && most_groups <= 1;
  c->wide_now = (c->lat_now && c->fs4_ok && c->lat_wide) ? 4 : 0;
  // the buffer sets, queues and shadow-queue bounds below are laid out for `cap`
  // paths: a larger piece would write past them
  for (const auto& pp : plan.per_pipe)
    for (const auto& g : pp)
      for (const Piece& pc : g)
        if (pc.n > cap || pc.n <= 0)
          return fail(WR_E_ARG, "piece plan: a piece of " + std::to_string(pc.n) + " paths exceeds the buffer capacity " + std::to_string(cap));
  {  // WR_TRACE_BVH t2 scratch: a launch takes <= kGroup x (shadow / aux + extension) queues.
     // Laid out on every pipeline that fits, as the work buffers are: a short
     // render (a warm-up) on few of them leaves nothing to allocate to a long one
    const size_t cap_sq = size_t(c->pipes[0].bb[0].cap_sq);
    // (+ the camera pass's extension queue: the overlapped schedule traces both passes' at once)
    const size_t per = kGroup * (std::max(cap_sq, size_t(cap)) + 2 * size_t(cap));
    for (int i = 0; i < fit; ++i)
      if (int rc = ensure_t2(c, c->pipes[i], per)) return rc;
  }
  // The overlapped schedule (wr_bdpt.h).  WR_BDPT_OVERLAP=0: the sequential
  // one, the light pass and then the camera pass as the reference runs them --
  // the schedule the overlapped one is checked against, and the one a build
  // with fewer than 2 x kGroup queues per launch gets
  const bool overlap = c->bdpt_overlap && kMaxQueues >= 2 * kGroup;
  float* dfilm = nullptr;
  const size_t nf = size_t(P) * 3;
  if (int rc = moments_target(c, film, M, film_on_device, nf, &dfilm)) return rc;
  if (M.on())
    if (int rc = ensure_moments(c, fit, nf)) return rc;
  const size_t nbak = M.on() ? 2 * nf : nf;  // film_bak: film, then film_sq
  // vertex pools and shadow queues sized by use (BdptBuf): a render that fills
  // one is redone from the film as it was before it.  A caller's device film is
  // copied first (after the caller's work on the null stream, before any
  // pipeline starts: begin_render orders them after the context stream); a
  // host film's device copy starts at zero
  const bool pooled = c->pipes[0].bb[0].vidx != nullptr;
  if (pooled && film_on_device) {
    if (int rc = c->film_bak.grow(nbak)) return rc;
    (void)hipEventRecord(c->t_null, nullptr);
    (void)hipStreamWaitEvent(c->stream, c->t_null, 0);
    HIPCHK(hipMemcpyAsync(c->film_bak.p, dfilm, nf * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (M.on())
      HIPCHK(hipMemcpyAsync(c->film_bak.p + nf, M.dsq, nf * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  const wr_stats st0 = st ? *st : wr_stats{};
  BdptArgs A0;
  A0.S = c->ds;
  A0.film = dfilm;
  A0.W = prm->width;
  A0.H = prm->height;
  A0.P = P;
  A0.seed = prm->seed;
  A0.ctl = prm->control_length;
  A0.maxlen = prm->max_path_length > 0 ? prm->max_path_length : 10;
  A0.faithful = prm->faithful;
  A0.overlap = overlap ? 1 : 0;
  A0.nmats = c->nmats;
  A0.has_sph = c->has_sph;
  const int maxlen = A0.maxlen;
  const bool count = prm->count_work != 0;
  // One group of pieces on one pipeline, issued step by step: step 0 clears
  // the counters and starts the light subpaths, steps 1 .. maxlen-1 are the
  // light bounces, step maxlen starts the camera subpaths, and steps
  // maxlen+1 .. 2 maxlen+1 are the camera bounces.
  struct GroupIssue {
    Pipe* pp = nullptr;
    BdptGroup GA;
    int gn = 0, nmax = 0;
    int fold[kGroup] = {}, nfold = 0;  // moments: the pass films complete after this group
  };
  // steps: light gen, light bounces b = 0 .. lb_n - 1, camera gen, camera bounces b = 0 .. maxlen;
  // overlapped: both gens, then bounces b = 0 .. maxlen of both passes together
  const int lb_n = maxlen - 1;
  const int nsteps = overlap ? maxlen + 2 : 2 * maxlen + 2;
  // The overlapped schedule: step 0 starts both subpaths of every path; step
  // b + 1 traces, per group member, the shadow / aux rays queued by the
  // vertices of bounce b - 1 (sq slot kCamSlot + b: light splats and
  // connections, camera DI rays and connections) and the extension queue of
  // bounce b: the light pass's rays (count ext[b]; b <= maxlen - 2) followed
  // by the camera pass's (count ext[kCamSlot + b]; b < maxlen) -- one queue,
  // so that a launch takes at most 2 x kGroup queues (more queues cost the
  // traversal kernels registers: WR_MAX_QUEUES 6 took k_trace_fast from 79 to
  // 95 VGPRs, 6 to 5 waves per SIMD).  Then it shades the light vertices of
  // bounce b and after them (same stream) resolves the step's shadow / aux
  // rays and shades its camera vertices, which append their extension rays
  // behind the light pass's final count.
  // the gen and vertex kernels with the material / light tables in LDS, or the
  // global tables for a scene above the caps (wr_bdpt.h, WR_BDPT_TABLES)
  const bool gt = !bdpt_lds_tables(c->nmats, c->ds.nlights);
  const auto k_lgen = gt ? k_light_gen<true> : k_light_gen<false>;
  const auto k_lshade = gt ? k_light_shade<true> : k_light_shade<false>;
  const auto k_cstep = gt ? k_camera_step<true> : k_camera_step<false>;
  auto issue_overlap = [&](GroupIssue& G, int step) -> int {
    Pipe& pp = *G.pp;
    const hipStream_t sm = pp.stream;
    Timer tm(c, &pp);
    const int gn = G.gn;
    const BdptArgs* A = G.GA.a;
    const int g = shade_grid(c, G.nmax);
    if (step == 0) {
      HIPCHK(hipMemsetAsync(pp.sc, 0, gn * sizeof(StepCounters), sm));
      hipLaunchKernelGGL(k_lgen, dim3(g, gn), dim3(kShadeBlock), 0, sm, G.GA);
      hipLaunchKernelGGL(k_camera_gen, dim3(g, gn), dim3(kShadeBlock), 0, sm, G.GA);
      tm.mark(WR_K_GEN);
      return WR_OK;
    }
    const int b = step - 1, slot = kCamSlot + b;
    const bool light = b <= maxlen - 2, more = b < maxlen;
    QueueList ql;
    for (int m = 0; m < gn; ++m) {
      const BdptBuf& B = pp.bb[m];
      const BdptBuf::Sq& Q = B.sq[slot & 1];
      // (segments of the pipeline's ray slab: plane stride B.qs, clamped to the segment)
      ql.add(rq(Q.o, Q.d, B.qs, &pp.sc[m].sq[slot], Q.t, Q.prim, Q.cut), std::min(A[m].n * (kVMax + 2), B.cap_sq),
             B.cap_sq);
      if (light || more) {
        RayQueue e = rq(B.q_o[b & 1], B.q_d[b & 1], B.qs, &pp.sc[m].ext[b], B.q_t[b & 1], B.q_prim[b & 1]);
        e.count2 = &pp.sc[m].ext[slot];  // the camera pass's rays, behind the light pass's
        ql.add(e, 2 * A[m].n, pp.slab_l.cap_ext);
      }
    }
    trace_launch(c, sm, pp.ctr, tslot(pp, slot), tm, count, ql.Q, ql.max_rays, WR_BDPT_TRACE_MODE, false,
                 &pp.slab[slot & 1]);
    if (light) hipLaunchKernelGGL(k_lshade, dim3(g, gn), dim3(kShadeBlock), 0, sm, G.GA, b);
    const int nres = shade_grid(c, std::min(G.nmax * (kVMax + 2), pp.bb[0].cap_sq));
    hipLaunchKernelGGL(k_cstep, dim3(nres + (more ? g : 0), gn), dim3(kShadeBlock), 0, sm, G.GA, slot, nres,
                       more ? 1 : 0);
    tm.mark(WR_K_SHADE);
    return WR_OK;
  };
  auto issue = [&](GroupIssue& G, int step) -> int {
    if (step == nsteps) {  // moments renders: one step more
      for (int k = 0; k < G.nfold; ++k) fold_launch(c, *G.pp, G.fold[k], dfilm, M.dsq, nf);
      return WR_OK;
    }
    if (overlap) return issue_overlap(G, step);
    Pipe& pp = *G.pp;
    const hipStream_t sm = pp.stream;
    Timer tm(c, &pp);
    const int gn = G.gn;
    const BdptArgs* A = G.GA.a;
    auto sq = [&](int m, int slot) {
      const BdptBuf::Sq& Q = pp.bb[m].sq[slot & 1];
      return rq(Q.o, Q.d, pp.bb[m].qs, &pp.sc[m].sq[slot], Q.t, Q.prim, Q.cut);  // (ray slab: plane stride qs)
    };
    auto ext = [&](int m, int slot) {  // extension rays of step `slot`
      const BdptBuf& B = pp.bb[m];
      const int q = slot & 1;
      return rq(B.q_o[q], B.q_d[q], B.qs, &pp.sc[m].ext[slot], B.q_t[q], B.q_prim[q]);
    };
    const int ext_lim = pp.slab_l.cap_ext;
    const int sq_max = std::min(G.nmax * (kVMax + 2), pp.bb[0].cap_sq);
    const int g = shade_grid(c, G.nmax);
    if (step == 0) {
      HIPCHK(hipMemsetAsync(pp.sc, 0, gn * sizeof(StepCounters), sm));
      // ---------------- light pass (:67-131)
      hipLaunchKernelGGL(k_lgen, dim3(g, gn), dim3(kShadeBlock), 0, sm, G.GA);
      tm.mark(WR_K_GEN);
    } else if (step <= lb_n) {
      const int b = step - 1;
      QueueList ql;
      for (int m = 0; m < gn; ++m) ql.add(ext(m, b), A[m].n, ext_lim);
      trace_launch(c, sm, pp.ctr, tslot(pp, b), tm, count, ql.Q, ql.max_rays, WR_BDPT_TRACE_MODE, false,
                   &pp.slab[b & 1]);
      hipLaunchKernelGGL(k_lshade, dim3(g, gn), dim3(kShadeBlock), 0, sm, G.GA, b);
      tm.mark(WR_K_SHADE);
    } else if (step == lb_n + 1) {
      // ---------------- camera pass (:133-264).  The light pass's splat rays
      // (connectToCamera) ride along with the primary rays; afterwards each
      // bounce's shadow / aux rays ride along with the next bounce's extension rays.
      hipLaunchKernelGGL(k_camera_gen, dim3(g, gn), dim3(kShadeBlock), 0, sm, G.GA);
      tm.mark(WR_K_GEN);
    } else {
      const int b = step - lb_n - 2;
      const int slot = kCamSlot + b;
      const bool more = b < maxlen;  // extension rays of bounce b exist
      QueueList ql;
      for (int m = 0; m < gn; ++m)
        ql.add(sq(m, slot), std::min(A[m].n * (kVMax + 2), pp.bb[m].cap_sq), pp.bb[m].cap_sq);
      if (more)
        for (int m = 0; m < gn; ++m) ql.add(ext(m, slot), A[m].n, ext_lim);
      trace_launch(c, sm, pp.ctr, tslot(pp, slot), tm, count, ql.Q, ql.max_rays, WR_BDPT_TRACE_MODE, false,
                   &pp.slab[slot & 1]);
      // resolve this step's shadow / aux rays and shade its vertices in one launch
      const int nres = shade_grid(c, sq_max);
      hipLaunchKernelGGL(k_cstep, dim3(nres + (more ? g : 0), gn), dim3(kShadeBlock), 0, sm, G.GA, slot, nres,
                         more ? 1 : 0);
      tm.mark(WR_K_SHADE);
    }
    return WR_OK;
  };
  // Round r takes every pipeline's r-th group, and the launches go out step by
  // step across the pipelines: each stream runs its own in order, and all of
  // them get their first launches at once instead of one pipeline's ~90
  // launches after another's (host issue time: ~2 us per call)
  unsigned long long overflow = 0;
  auto run = [&](const PiecePlan& pl) -> int {
  const int npl = pl.pipes();
  begin_render(c, npl, prm->time_kernels);
  std::vector<GroupIssue> round(npl);
  for (int r = 0; r < pl.max_groups(); ++r) {
    int live = 0;
    for (int pi = 0; pi < npl; ++pi) {
      GroupIssue& G = round[pi];
      G.gn = 0;
      if (r >= static_cast<int>(pl.per_pipe[pi].size())) continue;
      const std::vector<Piece>& grp = pl.per_pipe[pi][r];
      G.pp = &c->pipes[pi];
      G.gn = static_cast<int>(grp.size());
      G.nmax = 0;
      for (int m = 0; m < G.gn; ++m) {
        const Piece& pc = grp[m];
        BdptArgs& a = G.GA.a[m];
        a = A0;
        a.B = G.pp->bb[m];
        a.ctr = G.pp->ctr;
        a.sc = G.pp->sc + m;
        a.iter = static_cast<uint32_t>(prm->iter_begin + pc.iter);
        a.base = pc.base;
        a.n = pc.n;
        G.nmax = std::max(G.nmax, pc.n);
      }
      G.nfold = 0;
      if (M.on()) {
        // An iteration's pieces follow one another on this pipeline, and a group
        // holds kGroup pieces: the iterations open at any time are consecutive
        // and at most kGroup, so iteration i takes pass film i % kGroup.  It is
        // folded after the group that holds its last piece.
        const auto& groups = pl.per_pipe[pi];
        for (int m = 0; m < G.gn; ++m) {
          G.GA.a[m].film = G.pp->mom[grp[m].iter % kGroup].p;
          const Piece* next = m + 1 < G.gn ? &grp[m + 1]
                              : r + 1 < static_cast<int>(groups.size()) ? &groups[r + 1][0] : nullptr;
          if (!next || next->iter != grp[m].iter) G.fold[G.nfold++] = grp[m].iter % kGroup;
        }
      }
      live += G.gn > 0;
    }
    if (!live) continue;
    if (int rc = issue_round(c, live, nsteps + (M.on() ? 1 : 0), [&](int pi, int step) {
          return round[pi].gn > 0 ? issue(round[pi], step) : WR_OK;
        }, npl))
      return rc;
  }
  HIPCHK(hipGetLastError());
  if (std::getenv("WR_ISSUE_LOG"))
    std::fprintf(stderr, "[wr issue] kernel args: BdptGroup %zu B, TraceQueues %zu B, DevScene %zu B, FastScene %zu B\n",
                 sizeof(BdptGroup), sizeof(TraceQueues), sizeof(DevScene), sizeof(c->fs));
  return finish_render(c, npl, st, t0, &overflow);
  };
  // an error after the first launch leaves a caller's device film as it was
  // before the render (its saved copy), not holding a partial render
  auto restore_film = [&](int rc) -> int {
    if (M.on()) c->mom_dirty = true;  // pass films may hold unfolded work
    if (pooled && film_on_device) {
      (void)hipDeviceSynchronize();  // the pipelines' launches in flight
      (void)hipMemcpy(dfilm, c->film_bak.p, nf * sizeof(float), hipMemcpyDeviceToDevice);
      if (M.on()) (void)hipMemcpy(M.dsq, c->film_bak.p + nf, nf * sizeof(float), hipMemcpyDeviceToDevice);
    }
    return rc;
  };
  if (int rc = run(plan)) return restore_film(rc);
  if (overflow) {
    // A vertex pool or shadow queue filled up and appends were dropped: redo
    // the render from the film as it was, with pieces whose worst case fits
    // every pool (<= 11 shadow rays per path and step, 9 light and 4 camera
    // vertices per path), in the untiled camera order (64-path units; the
    // path <-> pixel map is the same), so the film is the one of an unbounded
    // render.  Rare: the pools hold several times what the reference scenes use.
    const BdptBuf& B = c->pipes[0].bb[0];
    const int safe = std::min({B.cap_sq / (kVMax + 2), B.vcap / kVMax, B.ccap / kCvMax, cap}) / 64 * 64;
    if (safe < 64) return restore_film(fail(WR_E_HIP, "BDPT pools too small for a 64-path piece"));
    // (a moments render folds only into the caller's two films, and a finished
    // run leaves every pass film folded and clear: both films go back alike)
    if (film_on_device) {
      HIPCHK(hipMemcpyAsync(dfilm, c->film_bak.p, nf * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      if (M.on())
        HIPCHK(hipMemcpyAsync(M.dsq, c->film_bak.p + nf, nf * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    } else {
      HIPCHK(hipMemsetAsync(dfilm, 0, nbak * sizeof(float), c->stream));
    }
    if (st) *st = st0;
    A0.untiled = 1;
    overflow = 0;
    if (int rc = run(plan_pieces(f_lo, f_hi, P, 64, safe, fit, c->piece_min, M.on()))) return restore_film(rc);
    // (env WR_TEST_REDO_FAIL=1: the test of this error path treats the redo as overflowed)
    if (overflow || std::getenv("WR_TEST_REDO_FAIL"))
      return restore_film(fail(WR_E_HIP, "BDPT pools overflowed with pieces the worst case fits"));
    if (st) st->redone += 1;
  }
  if (st) {
    for (int i = 0; i < np; ++i) st->work_bytes += static_cast<int64_t>(c->pipes[i].work.cap());
    st->work_paths += static_cast<int64_t>(np) * kGroup * cap;
  }
  return moments_return(c, film, M, film_on_device, nf);
}

static int check_vcm(const wr_context* c, const wr_vcm_params* prm, const float* film) {
  if (!c || !prm || !film) return fail(WR_E_ARG, "null argument");
  if (prm->width <= 0 || prm->height <= 0 || prm->iterations < 0) return fail(WR_E_ARG, "bad film size");
  if (static_cast<int64_t>(prm->width) * prm->height >= (1 << 30) / (kVMax + 2))
    return fail(WR_E_ARG, "film too large for one context");
  if (prm->max_path_length < 1 || prm->max_path_length > kVMax + 1)
    return fail(WR_E_ARG, "max_path_length must be in 1..10 (light-vertex store sized for the reference's 10)");
  if (prm->min_path_length < 0 || !(prm->radius_factor > 0.f) || !(prm->radius_alpha <= 1.f))
    return fail(WR_E_ARG, "bad min_path_length / radius_factor / radius_alpha");
  if (c->ds.nlights <= 0) return fail(WR_E_SCENE, "VCM needs at least one area light");
  return WR_OK;
}
static int render_vcm_one(wr_context* c, const wr_vcm_params* prm, float* film, int film_on_device, wr_stats* st,
                          float* film_sq = nullptr) {
  HIPCHK(hipSetDevice(c->device));
  const double t0 = host_now();
  const int P = prm->width * prm->height;
  const int ngroups = (prm->iterations + kGroup - 1) / kGroup;
  const int fit = pipelines_that_fit(c, 3, P, kGroup, c->npipes);
  if (fit < 1) return WR_E_HIP;  // message set by the allocation
  const int np = std::max(1, std::min(fit, ngroups));
  {  // WR_TRACE_BVH t2 scratch: a launch takes <= kGroup x (shadow / aux + extension) queues
    const size_t cap_sq = size_t(c->pipes[0].bb[0].cap_sq);
    const size_t per = kGroup * (std::max(cap_sq, size_t(P)) + size_t(P));
    for (int i = 0; i < fit; ++i)
      if (int rc = ensure_t2(c, c->pipes[i], per)) return rc;
  }
  float* dfilm = nullptr;
  const size_t nf = size_t(P) * 3;
  MomentFilms M;
  M.sq = film_sq;
  if (int rc = moments_target(c, film, M, film_on_device, nf, &dfilm)) return rc;
  if (M.on()) {
    if (int rc = ensure_moments(c, np, nf)) return rc;
    c->mom_dirty = true;  // until the render has finished
  }
  begin_render(c, np, prm->time_kernels);
  VcmArgs X0;
  BdptArgs& A0 = X0.a;
  A0.S = c->ds;
  A0.film = dfilm;
  A0.W = prm->width;
  A0.H = prm->height;
  A0.P = P;
  A0.seed = prm->seed;
  A0.ctl = 0;
  A0.maxlen = prm->max_path_length;
  A0.faithful = 1;
  // VCM renders whole iterations: every camera vertex merges with the light
  // vertices of the whole iteration (:152, :265-276)
  A0.base = 0;
  A0.n = P;
  X0.minlen = prm->min_path_length;
  X0.N = static_cast<float>(prm->height * prm->width);
  X0.org = c->ds.root_l;
  const uint32_t T = vcm_table(P);
  X0.tmask = T - 1;
  const float base_radius = prm->radius_factor * c->sph_r;  // VertexCM::init (:13)
  const int maxlen = A0.maxlen;
  const bool count = prm->count_work != 0;
  const int g = shade_grid(c, P);
  for (int gi = 0; gi < ngroups; ++gi) {
    Pipe& pp = c->pipes[gi % np];
    const hipStream_t sm = pp.stream;
    Timer tm(c, &pp);
    const int it0 = gi * kGroup, gn = std::min(kGroup, prm->iterations - it0);
    VcmGroup GA;
    for (int m = 0; m < gn; ++m) {
      VcmArgs& X = GA.a[m];
      X = X0;
      X.a.B = pp.bb[m];
      X.V = pp.vb[m];
      X.a.ctr = pp.ctr;
      X.a.sc = pp.sc + m;
      const int it = prm->iter_begin + it0 + m;
      X.a.iter = static_cast<uint32_t>(it);
      if (M.on()) X.a.film = pp.mom[m].p;  // member m's iteration, folded below
      // runIteration's radius schedule and MIS factors (:50-64), host float
      float radius = base_radius;
      radius /= powf(static_cast<float>(it + 1), 0.5f * (1.f - prm->radius_alpha));
      radius = (radius < WR_EPS) ? WR_EPS : radius;
      const float r2 = radius * radius;
      X.radius = radius;
      X.vm_norm = 1.f / (r2 * WR_PI * X.N);
      const float eta = (WR_PI * r2) * X.N;
      X.mis_vm = eta;
      X.mis_vc = 1.f / eta;
      X.rq = radius * 1.0009765625f;
      // the first float s with sqrtf(s) >= radius: sqrtf is correctly rounded
      // and monotone on host and device, so `sqrtf(s) < radius` == `s < r2t`
      float t = r2;
      while (t > 0.f && std::sqrt(t) >= radius) t = std::nextafter(t, 0.f);
      while (!(std::sqrt(t) >= radius)) t = std::nextafter(t, INFINITY);
      X.r2t = t;
      X.inv_cs = 1.f / (c->vcm_cell * X.rq);
    }
    auto sq = [&](int m, int slot) {
      const BdptBuf::Sq& Q = pp.bb[m].sq[slot & 1];
      return rq(Q.o, Q.d, pp.bb[m].cap_sq, &pp.sc[m].sq[slot], Q.t, Q.prim, Q.cut);
    };
    auto ext = [&](int m, int slot) {
      const BdptBuf& B = pp.bb[m];
      const int q = slot & 1;
      return rq(B.q_o[q], B.q_d[q], P, &pp.sc[m].ext[slot], B.q_t[q], B.q_prim[q]);
    };
    const int sq_max = pp.bb[0].cap_sq;
    HIPCHK(hipMemsetAsync(pp.sc, 0, gn * sizeof(StepCounters), sm));
    // ---------------- light pass (:67-140)
    hipLaunchKernelGGL(k_vcm_light_gen, dim3(g, gn), dim3(kShadeBlock), 0, sm, GA);
    tm.mark(WR_K_GEN);
    for (int b = 0; b < maxlen - 1; ++b) {
      QueueList ql;
      for (int m = 0; m < gn; ++m) ql.add(ext(m, b), P);
      trace_launch(c, sm, pp.ctr, tslot(pp, b), tm, count, ql.Q, ql.max_rays);
      hipLaunchKernelGGL(k_vcm_light_shade, dim3(g, gn), dim3(kShadeBlock), 0, sm, GA, b);
      tm.mark(WR_K_SHADE);
    }
    // ---------------- light vertices -> merge grid (replaces the KdTree, :152)
    hipLaunchKernelGGL(k_vcm_fixup, dim3(64, gn), dim3(kShadeBlock), 0, sm, GA);
    for (int m = 0; m < gn; ++m) HIPCHK(hipMemsetAsync(pp.vb[m].cnt, 0, (size_t(T) + 1) * sizeof(int), sm));
    hipLaunchKernelGGL(k_vgrid_count, dim3(g, gn), dim3(kShadeBlock), 0, sm, GA);
    for (int m = 0; m < gn; ++m) {
      size_t bytes = pp.vb[m].scan_bytes;
      HIPCHK(hipcub::DeviceScan::ExclusiveSum(pp.vb[m].scan_tmp, bytes, pp.vb[m].cnt, pp.vb[m].start,
                                              static_cast<int>(T + 1), sm));
    }
    hipLaunchKernelGGL(k_vgrid_scatter, dim3(g, gn), dim3(kShadeBlock), 0, sm, GA);
    tm.mark(WR_K_OTHER);
    // ---------------- camera pass (:157-283)
    hipLaunchKernelGGL(k_vcm_camera_gen, dim3(g, gn), dim3(kShadeBlock), 0, sm, GA);
    tm.mark(WR_K_GEN);
    for (int b = 0; b <= maxlen; ++b) {
      const int slot = kCamSlot + b;
      const bool more = b < maxlen;
      QueueList ql;
      for (int m = 0; m < gn; ++m) ql.add(sq(m, slot), sq_max);
      if (more)
        for (int m = 0; m < gn; ++m) ql.add(ext(m, slot), P);
      trace_launch(c, sm, pp.ctr, tslot(pp, slot), tm, count, ql.Q, ql.max_rays, WR_VCM_TRACE_MODE);
      const int nres = shade_grid(c, sq_max);
      // + the merge queries of the previous step (none before the first)
      const int nsh = more ? g : 0, nmg = b > 0 ? g : 0;
      hipLaunchKernelGGL(k_vcm_camera_step, dim3(nres + nsh + nmg, gn), dim3(kShadeBlock), 0, sm, GA, slot, nres,
                         nsh);
      tm.mark(WR_K_SHADE);
    }
    if (M.on())
      for (int m = 0; m < gn; ++m) fold_launch(c, pp, m, dfilm, M.dsq, nf);
  }
  HIPCHK(hipGetLastError());
  if (int rc = finish_render(c, np, st, t0)) return rc;
  if (M.on()) c->mom_dirty = false;
  return moments_return(c, film, M, film_on_device, nf);
}

static int check_radiance(const wr_context* c, const wr_ray* rays, int64_t n64, int32_t max_depth, const float* rgb) {
  if (!c || ((!rays || !rgb) && n64) || n64 < 0) return fail(WR_E_ARG, "bad argument");
  if (max_depth < 0 || max_depth > kSlots - 3) return fail(WR_E_ARG, "max_depth must be in 0..61");
  if (n64 > (1 << 26)) return fail(WR_E_ARG, "at most 2^26 rays per call");
  if (c->ds.nlights <= 0) return fail(WR_E_SCENE, "path tracing needs at least one area light");
  return WR_OK;
}
// on_device (wr_path_radiance_dev): rays, rgb and rgb_sq are device arrays, read
// and accumulated into (+=) where they lie.  With rgb_sq the sample renders
// into pipeline 0's pass film, which k_film_fold adds to rgb and, squared, to
// rgb_sq, as a PT moments render does per sample.
static int path_radiance_one(wr_context* c, const wr_ray* rays, int64_t n64, int32_t max_depth, uint32_t seed,
                             int32_t sample, float* rgb, wr_stats* st, bool on_device = false,
                             float* rgb_sq = nullptr) {
  if (n64 == 0) return WR_OK;
  const int P = static_cast<int>(n64);
  const size_t nf = size_t(P) * 3;
  if (on_device) {
    const size_t fb = nf * sizeof(float);
    if (int rc = check_dev_args(c, "wr_path_radiance_dev",
                                {wr::in(rays, size_t(P) * sizeof(wr_ray), "rays"),
                                 wr::out(rgb, fb, "rgb"), wr::out(rgb_sq, fb, "rgb_sq", 1, true)},
                                "wr_path_radiance"))
      return rc;
  }
  HIPCHK(hipSetDevice(c->device));
  const double t0 = host_now();
  if (pipelines_that_fit(c, 2, P, 1, 1) < 1) return WR_E_HIP;
  if (int rc = ensure_t2(c, c->pipes[0], 2 * size_t(P))) return rc;
  Pipe& pp = c->pipes[0];  // the context stream
  float* dfilm = rgb;
  const wr_ray* drays = rays;
  if (!on_device) {
    std::memset(rgb, 0, nf * sizeof(float));
    if (int rc = film_target(c, rgb, 0, nf, &dfilm)) return rc;
    if (int rc = api_scratch(c, size_t(P) * sizeof(wr_ray))) return rc;
    wr_ray* staged = reinterpret_cast<wr_ray*>(c->api_tmp.p);
    HIPCHK(hipMemcpyAsync(staged, rays, size_t(P) * sizeof(wr_ray), hipMemcpyHostToDevice, pp.stream));
    drays = staged;
  } else if (rgb_sq) {
    if (int rc = ensure_moments(c, 1, nf)) return rc;
    c->mom_dirty = true;  // until the call has finished
  }
  begin_render(c, 1, 0);
  PtGroup GA;
  PtArgs& A = GA.a[0];
  A.S = c->ds;
  A.T = pp.pb[0];
  A.ctr = pp.ctr;
  A.sc = pp.sc;
  A.film = rgb_sq ? pp.mom[0].p : dfilm;
  A.W = P;
  A.H = 1;
  A.P = P;
  A.spp = 1;
  A.grid_len = 1;
  A.max_depth = max_depth;
  A.seed = seed;
  A.k = static_cast<uint32_t>(sample);
  const hipStream_t sm = pp.stream;
  Timer tm(c, &pp);
  const int g = shade_grid(c, P);
  HIPCHK(hipMemsetAsync(pp.sc, 0, sizeof(StepCounters), sm));
  hipLaunchKernelGGL(k_pt_gen_rays, dim3(g, 1), dim3(kShadeBlock), 0, sm, GA, drays);
  for (int b = 0; b <= max_depth + 1; ++b) {
    const bool more = b <= max_depth;
    const PtBuf& T = pp.pb[0];
    const PtBuf::Sq& Q = T.sq[b & 1];
    QueueList ql;
    ql.add(rq(Q.o, Q.d, P, &pp.sc[0].sq[b], Q.t, Q.prim, Q.cut), P);
    if (more) ql.add(rq(T.q_o[b & 1], T.q_d[b & 1], P, &pp.sc[0].ext[b], T.q_t[b & 1], T.q_prim[b & 1]), P);
    trace_launch(c, sm, pp.ctr, tslot(pp, b), tm, false, ql.Q, ql.max_rays, TRACE_DENSE, true);
    const int nres = shade_grid(c, P);
    hipLaunchKernelGGL(k_pt_step, dim3(nres + (more ? g : 0), 1), dim3(kShadeBlock), 0, sm, GA, b, nres,
                       more ? 1 : 0);
    if (!more) break;
  }
  if (rgb_sq) fold_launch(c, pp, 0, dfilm, rgb_sq, nf);
  HIPCHK(hipGetLastError());
  if (int rc = finish_render(c, 1, st, t0)) return rc;
  if (on_device) {
    if (rgb_sq) c->mom_dirty = false;
    return WR_OK;
  }
  return film_return(c, rgb, 0, nf);
}

static int check_path(const wr_context* c, const wr_path_params* prm, const float* film) {
  if (!c || !prm || !film) return fail(WR_E_ARG, "null argument");
  if (prm->width <= 0 || prm->height <= 0 || prm->spp <= 0) return fail(WR_E_ARG, "bad film size / spp");
  // path-state arrays are indexed up to 3 * P in 32-bit ints
  if (static_cast<int64_t>(prm->width) * prm->height >= (int64_t(1) << 31) / 4)
    return fail(WR_E_ARG, "film too large for one context");
  if (prm->max_depth < 0 || prm->max_depth > kSlots - 3) return fail(WR_E_ARG, "max_depth must be in 0..61");
  // sample k of the spp grid (surfaceIntegrator.cpp:26-32): only 0 <= k < spp exist
  if (prm->sample_begin < 0 || prm->sample_count < 0 ||
      static_cast<int64_t>(prm->sample_begin) + prm->sample_count > prm->spp ||
      prm->sample_begin > prm->spp)
    return fail(WR_E_ARG, "samples [sample_begin, sample_begin + sample_count) must lie in [0, spp)");
  if (c->ds.nlights <= 0) return fail(WR_E_SCENE, "path tracing needs at least one area light");
  return WR_OK;
}
static int render_path_one(wr_context* c, const wr_path_params* prm, float* film, int film_on_device, wr_stats* st,
                           float* film_sq = nullptr) {
  HIPCHK(hipSetDevice(c->device));
  const double t0 = host_now();
  const int P = prm->width * prm->height;
  const int k0 = prm->sample_begin;
  const int k1 = prm->sample_count > 0 ? k0 + prm->sample_count : prm->spp;
  const int nk = std::max(0, k1 - k0);
  const int ngroups = (nk + kGroup - 1) / kGroup;
  const int fit = pipelines_that_fit(c, 2, P, kGroup, c->npipes);
  if (fit < 1) return WR_E_HIP;  // message set by the allocation
  const int np = std::max(1, std::min(fit, ngroups));
  {  // WR_TRACE_BVH t2 scratch: a launch takes <= kGroup x (shadow / aux + extension) queues
    const size_t cap_sq = size_t(c->pipes[0].bb[0].cap_sq);
    const size_t per = kGroup * (std::max(cap_sq, size_t(P)) + size_t(P));
    for (int i = 0; i < fit; ++i)
      if (int rc = ensure_t2(c, c->pipes[i], per)) return rc;
  }
  float* dfilm = nullptr;
  const size_t nf = size_t(P) * 3;
  MomentFilms M;
  M.sq = film_sq;
  if (int rc = moments_target(c, film, M, film_on_device, nf, &dfilm)) return rc;
  if (M.on()) {
    if (int rc = ensure_moments(c, np, nf)) return rc;
    c->mom_dirty = true;  // until the render has finished
  }
  begin_render(c, np, prm->time_kernels);
  PtArgs A0;
  A0.S = c->ds;
  A0.film = dfilm;
  A0.W = prm->width;
  A0.H = prm->height;
  A0.P = P;
  A0.spp = prm->spp;
  A0.grid_len = static_cast<int>(std::sqrt(static_cast<double>(prm->spp)));
  A0.max_depth = prm->max_depth;
  A0.seed = prm->seed;
  const bool count = prm->count_work != 0;
  const int g = shade_grid(c, P);
  for (int gi = 0; gi < ngroups; ++gi) {
    // a group of gn samples in lockstep on pipeline gi % np
    Pipe& pp = c->pipes[gi % np];
    const hipStream_t sm = pp.stream;
    Timer tm(c, &pp);
    const int gk = k0 + gi * kGroup, gn = std::min(kGroup, k1 - gk);
    PtGroup GA;
    PtArgs* A = GA.a;
    for (int m = 0; m < gn; ++m) {
      A[m] = A0;
      A[m].T = pp.pb[m];
      A[m].ctr = pp.ctr;
      A[m].sc = pp.sc + m;
      A[m].k = static_cast<uint32_t>(gk + m);
      if (M.on()) A[m].film = pp.mom[m].p;  // member m's sample, folded below
    }
    HIPCHK(hipMemsetAsync(pp.sc, 0, gn * sizeof(StepCounters), sm));
    hipLaunchKernelGGL(k_pt_gen, dim3(g, gn), dim3(kShadeBlock), 0, sm, GA);
    tm.mark(WR_K_GEN);
    for (int b = 0; b <= A0.max_depth + 1; ++b) {
      // NEE shadow rays of the previous vertex ride along with this bounce's rays
      const bool more = b <= A0.max_depth;
      const int q = b & 1;
      QueueList ql;
      for (int m = 0; m < gn; ++m) {
        const PtBuf& T = pp.pb[m];
        const PtBuf::Sq& Q = T.sq[b & 1];
        ql.add(rq(Q.o, Q.d, P, &pp.sc[m].sq[b], Q.t, Q.prim, Q.cut), P);
      }
      if (more)
        for (int m = 0; m < gn; ++m) {
          const PtBuf& T = pp.pb[m];
          ql.add(rq(T.q_o[q], T.q_d[q], P, &pp.sc[m].ext[b], T.q_t[q], T.q_prim[q]), P);
        }
      trace_launch(c, sm, pp.ctr, tslot(pp, b), tm, count, ql.Q, ql.max_rays, TRACE_DENSE);
      // resolve this step's shadow rays and shade its vertices in one launch
      const int nres = shade_grid(c, P);
      hipLaunchKernelGGL(k_pt_step, dim3(nres + (more ? g : 0), gn), dim3(kShadeBlock), 0, sm, GA, b, nres,
                         more ? 1 : 0);
      tm.mark(WR_K_SHADE);
      if (!more) break;
    }
    if (M.on())
      for (int m = 0; m < gn; ++m) fold_launch(c, pp, m, dfilm, M.dsq, nf);
  }
  HIPCHK(hipGetLastError());
  if (int rc = finish_render(c, np, st, t0)) return rc;
  if (M.on()) c->mom_dirty = false;
  return moments_return(c, film, M, film_on_device, nf);
}


// ---- multi-device renders (wr_create_multi)
static void add_stats(wr_stats* d, const wr_stats& s) {
  d->closest_rays += s.closest_rays;
  d->shadow_rays += s.shadow_rays;
  d->inner_visits += s.inner_visits;
  d->leaf_visits += s.leaf_visits;
  d->prim_refs += s.prim_refs;
  for (int k = 0; k < WR_K_NUM; ++k) {
    d->kernel_ms[k] += s.kernel_ms[k];
    d->kernel_launches[k] += s.kernel_launches[k];
  }
  d->vm_queries += s.vm_queries;
  d->vm_found += s.vm_found;
  d->vm_merged += s.vm_merged;
  d->prim_tests += s.prim_tests;
  d->bvh_nodes += s.bvh_nodes;
  d->bvh_tests += s.bvh_tests;
  d->kd_replay_steps += s.kd_replay_steps;
  d->fallback_rays += s.fallback_rays;
  d->verify_rays += s.verify_rays;
  d->verify_mismatches += s.verify_mismatches;
  d->pipelines = std::max(d->pipelines, s.pipelines);
  d->bvh_width = std::max(d->bvh_width, s.bvh_width);
  d->work_bytes += s.work_bytes;
  d->work_paths += s.work_paths;
  d->redone += s.redone;
}

static int ensure_dev_film(wr_context* d, DevBuf<float>& buf, size_t nf) {
  HIPCHK(hipSetDevice(d->device));
  return buf.grow(nf);
}

// films[k] (on device k) summed into films[0]: one RCCL reduce over the
// devices' communicators, or peer copies to devices[0] + an add kernel
static int reduce_films(wr_context* c, const std::vector<wr_context*>& dev, const std::vector<float*>& films,
                        size_t nf) {
  const int n = static_cast<int>(dev.size());
  if (n == 1) return WR_OK;
  if (static_cast<int>(c->dev_comms.size()) == n) {
    NCCLCHK(rccl().group_start());
    for (int k = 0; k < n; ++k) {
      HIPCHK(hipSetDevice(dev[k]->device));
      // in place on the root; the receive buffer is ignored elsewhere
      NCCLCHK(rccl().reduce(films[k], films[k], nf, ncclFloat32, ncclSum, 0, c->dev_comms[k], dev[k]->stream));
    }
    NCCLCHK(rccl().group_end());
    for (int k = 0; k < n; ++k) {
      HIPCHK(hipSetDevice(dev[k]->device));
      HIPCHK(hipStreamSynchronize(dev[k]->stream));
    }
    return WR_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  const int g = static_cast<int>(std::min<size_t>(4096, (nf + 255) / 256));
  for (int k = 1; k < n; ++k) {
    const float* src = films[k];
    if (dev[k]->device != c->device) {
      if (int rc = ensure_dev_film(c, c->stage_buf, nf)) return rc;
      HIPCHK(hipMemcpyPeerAsync(c->stage_buf.p, c->device, films[k], dev[k]->device, nf * sizeof(float), c->stream));
      src = c->stage_buf.p;
    }
    hipLaunchKernelGGL(k_film_accumulate, dim3(g), dim3(256), 0, c->stream, films[0], src, nf);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return WR_OK;
}

extern "C++" {
// Every device renders its share (fn) into a film of its own (devices[0]:
// the caller's device film, if given), the films are summed on devices[0],
// and a host film gets the sum added.  Stats: counts summed, seconds = the
// call's wall time, trace_wall_ms = the largest device's.
template <class Fn>
static int multi_render(wr_context* c, size_t nf, float* film, int film_on_device, wr_stats* st, Fn fn) {
  const double t0 = host_now();
  std::vector<wr_context*> dev{c};
  dev.insert(dev.end(), c->subs.begin(), c->subs.end());
  const int n = static_cast<int>(dev.size());
  std::vector<float*> buf(n, nullptr);
  for (int k = 0; k < n; ++k) {
    if (k == 0 && film_on_device) {
      buf[0] = film;
      continue;
    }
    if (int rc = ensure_dev_film(dev[k], dev[k]->red_buf, nf)) return rc;
    HIPCHK(hipMemsetAsync(dev[k]->red_buf.p, 0, nf * sizeof(float), dev[k]->stream));
    buf[k] = dev[k]->red_buf.p;
  }
  std::vector<wr_stats> s(n);
  for (auto& x : s) std::memset(&x, 0, sizeof x);
  if (int rc = for_each_device(c, [&](wr_context* d, int k) { return fn(d, k, n, buf[k], &s[k]); })) return rc;
  if (int rc = reduce_films(c, dev, buf, nf)) return rc;
  if (!film_on_device) {
    std::vector<float> tmp(nf);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(tmp.data(), buf[0], nf * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nf; ++i) film[i] = film[i] + tmp[i];
  }
  if (st) {
    double wall = 0.0;
    for (const auto& x : s) {
      add_stats(st, x);
      wall = std::max(wall, x.trace_wall_ms);
    }
    st->trace_wall_ms += wall;
    st->seconds += host_now() - t0;
  }
  return WR_OK;
}

}  // extern "C++"

// The work buffers every pipeline of one device needs for renders of this
// kind and film size: what the first render would allocate (SurfaceIntegrator::
// init's share of the set-up, surfaceIntegrator.h:14-34), so that render()
// itself only renders.
static int reserve_one(wr_context* c, int kind, int W, int H) {
  HIPCHK(hipSetDevice(c->device));
  const int P = W * H;
  int fit = 0, cap = P;
  if (kind == WR_INTEGRATOR_BDPT) {
    wr_bdpt_params prm{};
    prm.width = W;
    prm.height = H;
    cap = piece_capacity(c, P, bdpt_unit(&prm));
    fit = pipelines_that_fit(c, 1, cap, kGroup, c->npipes);
  } else {
    fit = pipelines_that_fit(c, kind == WR_INTEGRATOR_VCM ? 3 : 2, P, kGroup, c->npipes);
  }
  if (fit < 1) return WR_E_HIP;  // message set by the allocation
  const size_t cap_sq = size_t(c->pipes[0].bb[0].cap_sq);
  const size_t per = kGroup * (std::max(cap_sq, size_t(cap)) + 2 * size_t(cap));
  for (int i = 0; i < fit; ++i)
    if (int rc = ensure_t2(c, c->pipes[i], per)) return rc;
  HIPCHK(hipDeviceSynchronize());
  return WR_OK;
}

int wr_reserve(wr_context* c, int integrator, int32_t width, int32_t height) {
  if (!c) return fail(WR_E_ARG, "null argument");
  if (integrator < WR_INTEGRATOR_BDPT || integrator > WR_INTEGRATOR_PATH) return fail(WR_E_ARG, "bad integrator");
  if (width <= 0 || height <= 0) return fail(WR_E_ARG, "bad film size");
  if (static_cast<int64_t>(width) * height >= (1 << 30) / (kVMax + 2)) return fail(WR_E_ARG, "film too large for one context");
  DeviceGuard dg;
  if (int rc = reserve_one(c, integrator, width, height)) return rc;
  for (wr_context* d : c->subs)
    if (int rc = reserve_one(d, integrator, width, height)) return rc;
  return WR_OK;
}

int wr_render_bdpt(wr_context* c, const wr_bdpt_params* prm, float* film, int film_on_device, wr_stats* st) {
  if (int rc = check_bdpt(c, prm, film)) return rc;
  DeviceGuard dg;
  const int P = prm->width * prm->height;
  const int64_t T = static_cast<int64_t>(prm->iterations) * P;
  if (c->subs.empty()) return render_bdpt_one(c, prm, 0, T, film, film_on_device, st);
  // devices take equal contiguous shares of the flattened path-iterations:
  // a single iteration (the reference's default, bidirPathTracing.cpp:9)
  // still spreads over every device
  const int unit = bdpt_unit(prm);
  return multi_render(c, size_t(P) * 3, film, film_on_device, st,
                      [&](wr_context* d, int k, int n, float* buf, wr_stats* s) {
                        const int64_t lo = k == 0 ? 0 : flat_round(T * k / n, P, unit);
                        const int64_t hi = k == n - 1 ? T : flat_round(T * (k + 1) / n, P, unit);
                        return render_bdpt_one(d, prm, lo, hi, buf, 1, s);
                      });
}

int wr_render_vcm(wr_context* c, const wr_vcm_params* prm, float* film, int film_on_device, wr_stats* st) {
  if (int rc = check_vcm(c, prm, film)) return rc;
  DeviceGuard dg;
  if (c->subs.empty()) return render_vcm_one(c, prm, film, film_on_device, st);
  // whole iterations per device: an iteration's merge grid holds all of its
  // light vertices (vertexcm.cpp:152)
  const int I = prm->iterations;
  return multi_render(c, size_t(prm->width) * prm->height * 3, film, film_on_device, st,
                      [&](wr_context* d, int k, int n, float* buf, wr_stats* s) {
                        wr_vcm_params q = *prm;
                        const int lo = I * k / n, hi = I * (k + 1) / n;
                        if (hi <= lo) return static_cast<int>(WR_OK);
                        q.iter_begin = prm->iter_begin + lo;
                        q.iterations = hi - lo;
                        return render_vcm_one(d, &q, buf, 1, s);
                      });
}

int wr_render_path(wr_context* c, const wr_path_params* prm, float* film, int film_on_device, wr_stats* st) {
  if (int rc = check_path(c, prm, film)) return rc;
  DeviceGuard dg;
  if (c->subs.empty()) return render_path_one(c, prm, film, film_on_device, st);
  const int k0 = prm->sample_begin, k1 = prm->sample_count > 0 ? k0 + prm->sample_count : prm->spp;
  return multi_render(c, size_t(prm->width) * prm->height * 3, film, film_on_device, st,
                      [&](wr_context* d, int k, int n, float* buf, wr_stats* s) {
                        wr_path_params q = *prm;  // contiguous sample ranges of the spp grid
                        const int lo = k0 + (k1 - k0) * k / n, hi = k0 + (k1 - k0) * (k + 1) / n;
                        if (hi <= lo) return static_cast<int>(WR_OK);
                        q.sample_begin = lo;
                        q.sample_count = hi - lo;
                        return render_path_one(d, &q, buf, 1, s);
                      });
}

// ---- moments renders: film += sum of the pass films, film_sq += sum of their squares
static int check_moments(const wr_context* c, const float* film_sq) {
  if (!film_sq) return fail(WR_E_ARG, "null argument (film_sq)");
  if (!c->subs.empty())
    return fail(WR_E_ARG, "moments renders are not supported on a multi-device context (wr_create_multi): "
                          "it shares one iteration out over its devices; use one context per device");
  return WR_OK;
}
int wr_render_bdpt_moments(wr_context* c, const wr_bdpt_params* prm, float* film, float* film_sq, int films_on_device,
                           wr_stats* st) {
  if (int rc = check_bdpt(c, prm, film)) return rc;
  if (int rc = check_moments(c, film_sq)) return rc;
  DeviceGuard dg;
  const int64_t T = static_cast<int64_t>(prm->iterations) * prm->width * prm->height;
  return render_bdpt_one(c, prm, 0, T, film, films_on_device, st, film_sq);
}
int wr_render_vcm_moments(wr_context* c, const wr_vcm_params* prm, float* film, float* film_sq, int films_on_device,
                          wr_stats* st) {
  if (int rc = check_vcm(c, prm, film)) return rc;
  if (int rc = check_moments(c, film_sq)) return rc;
  DeviceGuard dg;
  return render_vcm_one(c, prm, film, films_on_device, st, film_sq);
}
int wr_render_path_moments(wr_context* c, const wr_path_params* prm, float* film, float* film_sq, int films_on_device,
                           wr_stats* st) {
  if (int rc = check_path(c, prm, film)) return rc;
  if (int rc = check_moments(c, film_sq)) return rc;
  DeviceGuard dg;
  return render_path_one(c, prm, film, films_on_device, st, film_sq);
}

int wr_film_error(wr_context* c, const float* film, const float* film_sq, int width, int height, int n_passes,
                  int films_on_device, float* stderr_map, wr_error_info* out) {
  if (!film || !film_sq || !out) return fail(WR_E_ARG, "null argument");
  if (width <= 0 || height <= 0) return fail(WR_E_ARG, "bad film size");
  if (n_passes < 2) return fail(WR_E_ARG, "a standard error needs at least 2 passes");
  if (films_on_device && !c) return fail(WR_E_ARG, "device films need a context");
  const size_t nf = size_t(width) * height * 3;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (!films_on_device) {  // the same formulas on the CPU; needs no device
    const double np = static_cast<double>(n_passes);
    for (size_t i = 0; i < nf; ++i) {
      double mu, se;
      film_error_value(film[i], film_sq[i], np, &mu, &se);
      if (stderr_map) stderr_map[i] = static_cast<float>(se);
      acc[0] += se;
      acc[1] += mu;
      if (mu > 0.0) {
        acc[2] = std::max(acc[2], se / mu);
        acc[3] += 1.0;
      }
    }
  } else {
    DeviceGuard dg;
    if (int rc = api_order(c)) return rc;
    if (int rc = c->err_acc.grow(4)) return rc;
    HIPCHK(hipMemsetAsync(c->err_acc.p, 0, sizeof acc, c->stream));
    const size_t blocks = (nf + kErrBlock - 1) / kErrBlock;
    const int g = static_cast<int>(std::max<size_t>(1, std::min<size_t>(blocks, size_t(c->cus) * 8)));
    hipLaunchKernelGGL(k_film_error, dim3(g), dim3(kErrBlock), 0, c->stream, film, film_sq, nf, n_passes, stderr_map,
                       c->err_acc.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(acc, c->err_acc.p, sizeof acc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  out->sum_stderr = acc[0];
  out->sum_mean = acc[1];
  out->rel_stderr = acc[1] > 0.0 ? acc[0] / acc[1] : 0.0;
  out->max_rel_stderr = acc[2];
  out->values = static_cast<int64_t>(acc[3]);
  return WR_OK;
}

// ---- first-hit feature films: a sibling of trace_api -- gen
// kernel -> SoA queue -> trace_launch in the context's trace mode -> finish
// kernel -> films.  On a multi-device context `c` is devices[0].
int wr_render_features(wr_context* c, int32_t width, int32_t height, int layout, float* normal, float* albedo,
                       float* position, float* depth, int films_on_device, wr_stats* st) {
  if (!c) return fail(WR_E_ARG, "null context");
  if (width < 1 || height < 1 || static_cast<int64_t>(width) * height > (int64_t(1) << 28))
    return fail(WR_E_ARG, "bad film size (1 .. 2^28 pixels)");
  if (layout != WR_FILM_PT && layout != WR_FILM_BDPT) return fail(WR_E_ARG, "layout must be WR_FILM_PT or WR_FILM_BDPT");
  if (!normal && !albedo && !position && !depth) return fail(WR_E_ARG, "no output film");
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  const double t0 = host_now();
  const int n = width * height;
  const size_t nb = size_t(n);
  // scratch: the SoA queue, (t, prim), the ray count, and host films' device copies
  const size_t bytes = nb * (4 * 8 + (films_on_device ? 0 : 4 * 10)) + 16 * 256;
  if (int rc = api_scratch(c, bytes)) return rc;
  char* q = c->api_tmp.p;
  auto take = [&](size_t sz) { char* r = q; q += (sz + 255) & ~size_t(255); return r; };
  float* o3 = reinterpret_cast<float*>(take(nb * 12));
  float* d3 = reinterpret_cast<float*>(take(nb * 12));
  float* tt = reinterpret_cast<float*>(take(nb * 4));
  int* pr = reinterpret_cast<int*>(take(nb * 4));
  int* cnt = reinterpret_cast<int*>(take(sizeof(int)));
  float* dn_ = normal, *da = albedo, *dp = position, *dd = depth;
  if (!films_on_device) {
    if (normal) dn_ = reinterpret_cast<float*>(take(nb * 12));
    if (albedo) da = reinterpret_cast<float*>(take(nb * 12));
    if (position) dp = reinterpret_cast<float*>(take(nb * 12));
    if (depth) dd = reinterpret_cast<float*>(take(nb * 4));
  }
  HIPCHK(hipMemcpyAsync(cnt, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
  const int g = std::max(1, std::min(c->grid, (n + 255) / 256));
  hipLaunchKernelGGL(k_feat_gen, dim3(g), dim3(256), 0, c->stream, c->ds, width, height, layout, o3, d3);
  if (int rc = api_trace(c, rq(o3, d3, n, cnt, tt, pr), nb, false, TRACE_PLAIN)) return rc;
  hipLaunchKernelGGL(k_feat_finish, dim3(g), dim3(256), 0, c->stream, c->ds, c->nmats, o3, d3, tt, pr, width, height,
                     dn_, da, dp, dd);
  HIPCHK(hipGetLastError());
  if (!films_on_device) {
    if (normal) HIPCHK(hipMemcpyAsync(normal, dn_, nb * 12, hipMemcpyDeviceToHost, c->stream));
    if (albedo) HIPCHK(hipMemcpyAsync(albedo, da, nb * 12, hipMemcpyDeviceToHost, c->stream));
    if (position) HIPCHK(hipMemcpyAsync(position, dp, nb * 12, hipMemcpyDeviceToHost, c->stream));
    if (depth) HIPCHK(hipMemcpyAsync(depth, dd, nb * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (st) {
    *st = wr_stats{};
    st->closest_rays = n;
    st->seconds = host_now() - t0;
  }
  return WR_OK;
}

// ---- the film denoiser (wr_denoise.h)
int wr_film_denoise(wr_context* c, const float* film, const float* film_sq, int width, int height, int n_passes,
                    const float* normal, const float* position, const float* albedo, const wr_denoise_params* prm,
                    int films_on_device, float* out) {
  if (!film || !film_sq || !out) return fail(WR_E_ARG, "null film, film_sq or out");
  if (out == film || out == film_sq || out == normal || out == position || out == albedo)
    return fail(WR_E_ARG, "out must not be one of the inputs");
  if (width < 1 || height < 1 || static_cast<int64_t>(width) * height > (int64_t(1) << 28))
    return fail(WR_E_ARG, "bad film size (1 .. 2^28 pixels)");
  if (n_passes < 2) return fail(WR_E_ARG, "the variance of the mean needs at least 2 passes");
  const wr_denoise_params p = prm ? *prm : dn::default_params();
  if (const char* why = dn::check_params(p)) return fail(WR_E_ARG, why);
  if (films_on_device && !c) return fail(WR_E_ARG, "device films need a context");
  if (!films_on_device) {  // the same filter on the CPU; needs no device
    dn::denoise_host(film, film_sq, width, height, n_passes, normal, position, albedo, p, out);
    return WR_OK;
  }
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  const int W = width, H = height, npix = W * H;
  const bool guides = normal || position || albedo;
  if (int rc = c->dn_cv[0].grow(size_t(npix))) return rc;
  if (p.levels > 1)
    if (int rc = c->dn_cv[1].grow(size_t(npix))) return rc;
  if (guides)
    if (int rc = c->dn_guides.grow(3 * size_t(npix))) return rc;
  dn::F4* g0 = guides ? c->dn_guides.p : nullptr;
  dn::F4* g1 = guides ? g0 + npix : nullptr;
  dn::F4* g2 = guides ? g1 + npix : nullptr;
  const dn::Cfg k{p.sigma_l, p.sigma_p, p.sigma_a, p.normal_power, normal != nullptr, position != nullptr,
                  albedo != nullptr};
  const int gp = std::max(1, std::min(c->cus * 8, (npix + 255) / 256));
  hipLaunchKernelGGL(dn::k_dn_prepare, dim3(gp), dim3(256), 0, c->stream, film, film_sq, normal, position, albedo,
                     npix, n_passes, c->dn_cv[0].p, g0, g1, g2);
  const int64_t tiles = int64_t((W + dn::kTile - 1) / dn::kTile) * ((H + dn::kTile - 1) / dn::kTile);
  const int gl = static_cast<int>(std::min<int64_t>(tiles, int64_t(1) << 20));
  const float scale = static_cast<float>(n_passes);
  for (int t = 0; t < p.levels; ++t) {
    const int s = 1 << t;
    const dn::View src{c->dn_cv[t & 1].p, g0, g1, g2, 0, 0, W};
    dn::F4* dst = c->dn_cv[(t + 1) & 1].p;
    const bool last = t == p.levels - 1, lds = s <= WR_DN_LDS_MAX_STEP;
    const size_t shm = lds ? dn::lds_bytes(s) : 0;
    auto kern = lds ? (last ? dn::k_dn_level<true, true> : dn::k_dn_level<true, false>)
                    : (last ? dn::k_dn_level<false, true> : dn::k_dn_level<false, false>);
    hipLaunchKernelGGL(kern, dim3(gl), dim3(dn::kBlock), shm, c->stream, src, k, W, H, s, dst, out, scale);
  }
  return api_finish(c);
}

int wr_path_radiance(wr_context* c, const wr_ray* rays, int64_t n64, int32_t max_depth, uint32_t seed,
                     int32_t sample, float* rgb, wr_stats* st) {
  if (int rc = check_radiance(c, rays, n64, max_depth, rgb)) return rc;
  DeviceGuard dg;
  return path_radiance_one(c, rays, n64, max_depth, seed, sample, rgb, st);  // devices[0]
}

int wr_path_radiance_dev(wr_context* c, const wr_ray* rays, int64_t n64, int32_t max_depth, uint32_t seed,
                         int32_t sample, float* rgb, float* rgb_sq, wr_stats* st) {
  if (!c) return fail(WR_E_ARG, "null context");
  if (int rc = check_radiance(c, rays, n64, max_depth, rgb)) return rc;
  DeviceGuard dg;
  return path_radiance_one(c, rays, n64, max_depth, seed, sample, rgb, st, true, rgb_sq);  // devices[0]
}

// The rays of wr_render_features as records (k_camera_rays), at their value index.
int wr_camera_rays(wr_context* c, int32_t width, int32_t height, int layout, wr_ray* rays, int rays_on_device) {
  if (!c) return fail(WR_E_ARG, "null context");
  if (width < 1 || height < 1 || static_cast<int64_t>(width) * height > (int64_t(1) << 28))
    return fail(WR_E_ARG, "bad film size (1 .. 2^28 pixels)");
  if (layout != WR_FILM_PT && layout != WR_FILM_BDPT) return fail(WR_E_ARG, "layout must be WR_FILM_PT or WR_FILM_BDPT");
  if (!rays) return fail(WR_E_ARG, "null rays");
  const int n = width * height;
  const size_t bytes = size_t(n) * sizeof(wr_ray);
  if (rays_on_device)
    if (int rc = check_dev_args(c, "wr_camera_rays", {wr::out(rays, bytes, "rays")},
                                "wr_camera_rays with rays_on_device = 0"))
      return rc;
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  wr_ray* dr = rays;
  if (!rays_on_device) {
    if (int rc = api_scratch(c, bytes)) return rc;
    dr = reinterpret_cast<wr_ray*>(c->api_tmp.p);
  }
  const int g = std::max(1, std::min(c->grid, (n + 255) / 256));
  hipLaunchKernelGGL(k_camera_rays, dim3(g), dim3(256), 0, c->stream, c->ds, width, height, layout, dr);
  HIPCHK(hipGetLastError());
  if (!rays_on_device) HIPCHK(hipMemcpyAsync(rays, dr, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return WR_OK;
}

// ---- shading on device arrays (wr_bsdf_*_dev, wr_light_*_dev, wr_rng_uniform_dev;
// DESIGN.md 13; kernels in wr_shade.h).  The arguments are checked as those of
// the _dev calls above, on the host and before any HIP call where that is
// possible; the indices inside the arrays are checked by the kernels.
// n records of `rec` bytes (0 for an n the call refuses)
static size_t recs(int64_t n, size_t rec) { return n > 0 ? static_cast<size_t>(n) * rec : 0; }
// The frame of a shading call: the scalars and the arrays checked, then
// launch(grid) on the context stream between api_order and api_finish.
static int shade_call(wr_context* c, const char* call, int64_t n, bool lights, std::initializer_list<wr::Arg> args,
                      const std::function<void(int)>& launch) {
  const std::string who = std::string(call) + ": ";
  if (!c) return fail(WR_E_ARG, who + "null context");
  if (n < 0) return fail(WR_E_ARG, who + "n < 0");
  if (n == 0) return WR_OK;
  if (n > (int64_t(1) << 28)) return fail(WR_E_ARG, who + "at most 2^28 records per call");
  if (lights) {  // refused after a null array, before any pointer is looked up
    if (const wr::ArgError e = wr::check_args_host(call, args)) return fail(e.code, e.msg);
    if (c->ds.nlights <= 0) return fail(WR_E_SCENE, who + "the scene has no area light");
  }
  if (int rc = check_dev_args(c, call, args, "no shading call: copy it to the device")) return rc;
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  // a block per 256 records (at most 2^20 blocks): the records cost unequal time, and blocks
  // that come and go balance the CUs better than c->grid resident ones looping
  launch(static_cast<int>((n + 255) / 256));
  return api_finish(c);
}

int wr_bsdf_eval_dev(wr_context* c, const wr_hit* hits, const float* wi, const float* wo, int64_t n,
                     wr_bsdf_info* info, wr_bsdf_eval* out) {
  return shade_call(c, "wr_bsdf_eval_dev", n, false,
                    {wr::in(hits, recs(n, sizeof(wr_hit)), "hits"), wr::in(wi, recs(n, 12), "wi"),
                     wr::in(wo, recs(n, 12), "wo"), wr::out(info, recs(n, sizeof(wr_bsdf_info)), "info", 1, true),
                     wr::out(out, recs(n, sizeof(wr_bsdf_eval)), "out")}, [&](int g) {
    hipLaunchKernelGGL(k_bsdf_eval, dim3(g), dim3(256), 0, c->stream, c->ds, c->nmats, hits, wi, wo, n, info, out);
  });
}

int wr_bsdf_sample_dev(wr_context* c, const wr_hit* hits, const float* wi, const float* r3, int64_t n,
                       wr_bsdf_info* info, wr_bsdf_sample* out) {
  return shade_call(c, "wr_bsdf_sample_dev", n, false,
                    {wr::in(hits, recs(n, sizeof(wr_hit)), "hits"), wr::in(wi, recs(n, 12), "wi"),
                     wr::in(r3, recs(n, 12), "r3"), wr::out(info, recs(n, sizeof(wr_bsdf_info)), "info", 1, true),
                     wr::out(out, recs(n, sizeof(wr_bsdf_sample)), "out")}, [&](int g) {
    hipLaunchKernelGGL(k_bsdf_sample, dim3(g), dim3(256), 0, c->stream, c->ds, c->nmats, hits, wi, r3, n, info, out);
  });
}

int wr_light_illuminate_dev(wr_context* c, const int32_t* light, const float* pos, const float* r3, int64_t n,
                            wr_light_illum* out) {
  return shade_call(c, "wr_light_illuminate_dev", n, true,
                    {wr::in(light, recs(n, 4), "light"), wr::in(pos, recs(n, 12), "pos"), wr::in(r3, recs(n, 12), "r3"),
                     wr::out(out, recs(n, sizeof(wr_light_illum)), "out")}, [&](int g) {
    hipLaunchKernelGGL(k_light_illuminate, dim3(g), dim3(256), 0, c->stream, c->ds, light, pos, r3, n, out);
  });
}

int wr_light_emit_dev(wr_context* c, const int32_t* light, const float* dir_r3, const float* pos_r3, int64_t n,
                      wr_light_emission* out) {
  return shade_call(c, "wr_light_emit_dev", n, true,
                    {wr::in(light, recs(n, 4), "light"), wr::in(dir_r3, recs(n, 12), "dir_r3"),
                     wr::in(pos_r3, recs(n, 12), "pos_r3"), wr::out(out, recs(n, sizeof(wr_light_emission)), "out")},
                    [&](int g) {
    hipLaunchKernelGGL(k_light_emit, dim3(g), dim3(256), 0, c->stream, c->ds, light, dir_r3, pos_r3, n, out);
  });
}

int wr_light_radiance_dev(wr_context* c, const wr_hit* hits, const float* ray_d, int64_t n, wr_light_rad* out) {
  return shade_call(c, "wr_light_radiance_dev", n, true,
                    {wr::in(hits, recs(n, sizeof(wr_hit)), "hits"), wr::in(ray_d, recs(n, 12), "ray_d"),
                     wr::out(out, recs(n, sizeof(wr_light_rad)), "out")}, [&](int g) {
    hipLaunchKernelGGL(k_light_radiance, dim3(g), dim3(256), 0, c->stream, c->ds, hits, ray_d, n, out);
  });
}

int wr_rng_uniform_dev(wr_context* c, uint32_t seed, uint32_t iteration, uint32_t subpath, const uint32_t* path,
                       uint32_t* ctr, int32_t draws, int64_t n, float* out) {
  if (c && (draws < 1 || draws > 64)) return fail(WR_E_ARG, "wr_rng_uniform_dev: draws must be 1..64");
  return shade_call(c, "wr_rng_uniform_dev", n, false,
                    {wr::in(path, recs(n, 4), "path", 1, true), wr::out(ctr, recs(n, 4), "ctr", 1, true),
                     wr::out(out, recs(n, 4 * static_cast<size_t>(draws)), "out")}, [&](int g) {
    hipLaunchKernelGGL(k_rng_uniform, dim3(g), dim3(256), 0, c->stream, seed, iteration, subpath, path, ctr, draws, n,
                       out);
  });
}

// ---- point sets on the device (wr_points_*; kernels in
// wr_points.h).  Arguments are checked like those of the shading calls; what
// the arrays hold (offsets, radii, coordinates) is checked by the kernels.
// the bucket count of n points: 2^k, at least twice the points and one row run
static uint32_t pts_table(int64_t n) {
  uint32_t t = kPtsRowW;
  while (static_cast<int64_t>(t) < 2 * n) t <<= 1;
  return t;
}
// The frame of a query call: the scalars and the arrays checked, then launch()
// on the context stream between api_order and api_finish.
static int pts_call(wr_context* c, const wr_points* idx, const char* call, int64_t nq,
                    std::initializer_list<wr::Arg> args, const std::function<void()>& launch) {
  const std::string who = std::string(call) + ": ";
  if (!c) return fail(WR_E_ARG, who + "null context");
  if (nq < 0) return fail(WR_E_ARG, who + "nq < 0");
  if (!idx) return fail(WR_E_ARG, who + "null index");
  if (idx->ctx != c) return fail(WR_E_ARG, who + "the index belongs to another context");
  if (nq > (int64_t(1) << 28)) return fail(WR_E_ARG, who + "at most 2^28 queries per call");
  if (nq == 0) return WR_OK;
  if (int rc = check_dev_args(c, call, args, "no point-set call: copy it to the device")) return rc;
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  launch();
  return api_finish(c);
}

int wr_points_build_dev(wr_context* c, const float* pos, int64_t n, float cell, wr_points** out) {
  const std::string who = "wr_points_build_dev: ";
  if (!c) return fail(WR_E_ARG, who + "null context");
  if (n < 0) return fail(WR_E_ARG, who + "n < 0");
  if (!out) return fail(WR_E_ARG, who + "null out");
  *out = nullptr;
  if (n > (int64_t(1) << 28)) return fail(WR_E_ARG, who + "at most 2^28 points");
  if (!(cell > 0.f) || !std::isfinite(cell)) return fail(WR_E_ARG, who + "cell must be a finite number > 0");
  if (n)  // (no points: pos is not looked at)
    if (int rc = check_dev_args(c, "wr_points_build_dev", {wr::in(pos, recs(n, 12), "pos", 4)},
                                "no point-set call: copy it to the device"))
      return rc;
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  const hipStream_t sm = c->stream;
  const int ni = static_cast<int>(n);
  const uint32_t T = pts_table(n);
  std::unique_ptr<wr_points> I(new wr_points);  // (its buffers free on c->device, current until `dg` goes)
  I->ctx = c;
  I->n = n;
  I->buckets = T;
  if (int rc = I->start.grow(size_t(T) + 1)) return rc;
  if (n)
    if (int rc = I->rec.grow(static_cast<size_t>(n))) return rc;
  PtsIndex& X = I->X;
  X.rec = I->rec.p;
  X.start = I->start.p;
  X.tmask = T - 1;
  X.cell = cell;
  DevBuf<uint32_t> small;  // [0..2] the bounding-box minimum (ordered integers), [3] the fullest bucket
  if (int rc = small.grow(4)) return rc;
  HIPCHK(hipMemsetAsync(small.p, 0xff, 12, sm));
  HIPCHK(hipMemsetAsync(small.p + 3, 0, 4, sm));
  uint32_t h4[4] = {~0u, ~0u, ~0u, 0u};
  int nrec = 0;
  if (n) {
    const int g = static_cast<int>(std::min<int64_t>((n + 255) / 256, 1 << 16));
    hipLaunchKernelGGL(k_pts_bbox, dim3(g), dim3(256), 0, sm, pos, ni, small.p);
    HIPCHK(hipMemcpyAsync(h4, small.p, 12, hipMemcpyDeviceToHost, sm));
    HIPCHK(hipStreamSynchronize(sm));
    for (int a = 0; a < 3; ++a) {
      const uint32_t o = h4[a], b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
      float f = 0.f;  // no finite point at all: any origin will do
      if (o != ~0u) std::memcpy(&f, &b, 4);
      X.org[a] = f;
    }
    // (bucket, index) sorted by bucket with a stable radix sort: the order of
    // the records is a function of the points alone
    DevBuf<uint32_t> key[2];
    DevBuf<int> val[2];
    for (int k = 0; k < 2; ++k) {
      if (int rc = key[k].grow(static_cast<size_t>(n))) return rc;
      if (int rc = val[k].grow(static_cast<size_t>(n))) return rc;
    }
    int bits = 1;
    while ((1u << bits) <= T) ++bits;  // keys are 0 .. T
    size_t tmp_bytes = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, key[0].p, key[1].p, val[0].p, val[1].p, ni, 0, bits, sm));
    DevBuf<char> tmp;
    if (int rc = tmp.grow(std::max<size_t>(tmp_bytes, 1))) return rc;
    hipLaunchKernelGGL(k_pts_keys, dim3(g), dim3(256), 0, sm, pos, ni, X, key[0].p, val[0].p);
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, key[0].p, key[1].p, val[0].p, val[1].p, ni, 0, bits, sm));
    hipLaunchKernelGGL(k_pts_records, dim3(g), dim3(256), 0, sm, pos, ni, T, key[1].p, val[1].p, I->rec.p);
    const int gt = static_cast<int>(std::min<int64_t>((int64_t(T) + 256) / 256, 1 << 16));
    hipLaunchKernelGGL(k_pts_start, dim3(gt), dim3(256), 0, sm, key[1].p, ni, T, I->start.p);
    hipLaunchKernelGGL(k_pts_max_bucket, dim3(gt), dim3(256), 0, sm, I->start.p, T, reinterpret_cast<int*>(small.p + 3));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h4 + 3, small.p + 3, 4, hipMemcpyDeviceToHost, sm));
    HIPCHK(hipMemcpyAsync(&nrec, I->start.p + T, 4, hipMemcpyDeviceToHost, sm));
    HIPCHK(hipStreamSynchronize(sm));  // the sort's buffers die here, idle
  } else {
    X.org[0] = X.org[1] = X.org[2] = 0.f;
    HIPCHK(hipMemsetAsync(I->start.p, 0, (size_t(T) + 1) * sizeof(int), sm));
    HIPCHK(hipStreamSynchronize(sm));
  }
  X.nrec = nrec;
  I->max_bucket = h4[3];
  c->points.push_back(I.get());
  *out = I.release();
  return WR_OK;
}

int wr_points_info_get(const wr_points* idx, wr_points_info* out) {
  if (!idx || !out) return fail(WR_E_ARG, "wr_points_info_get: null argument");
  *out = wr_points_info{};
  out->n = idx->n;
  out->cell = idx->X.cell;
  for (int a = 0; a < 3; ++a) out->origin[a] = idx->X.org[a];
  out->buckets = idx->buckets;
  out->max_bucket = idx->max_bucket;
  out->device_bytes = static_cast<int64_t>(idx->rec.n * sizeof(float4) + idx->start.n * sizeof(int));
  return WR_OK;
}

void wr_points_free(wr_points* idx) {
  if (!idx) return;
  wr_context* c = idx->ctx;
  DeviceGuard dg;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->points.erase(std::remove(c->points.begin(), c->points.end(), idx), c->points.end());
  delete idx;
}

static int pts_radius_call(wr_context* c, const wr_points* idx, const char* call, bool fill, const float* q,
                           int64_t nq, float radius, const float* radii, const int64_t* offset, int64_t capacity,
                           int32_t* count, int32_t* index) {
  const std::string who = std::string(call) + ": ";
  if (c && nq >= 0) {
    if (!radii && !(radius >= 0.f)) return fail(WR_E_ARG, who + "radius must not be negative or NaN");
    if (fill && capacity < 0) return fail(WR_E_ARG, who + "capacity < 0");
    if (fill && capacity > (int64_t(1) << 40)) return fail(WR_E_ARG, who + "capacity above 2^40");
  }
  const size_t nb = nq > 0 ? static_cast<size_t>(nq) : 0, cb = capacity > 0 ? static_cast<size_t>(capacity) : 0;
  const wr::Arg in_q = wr::in(q, nb * 12, "q", 4), in_radii = wr::in(radii, nb * 4, "radii", 4, true);
  const auto launch = [&] {
#if WR_PTS_RADIUS_WAVE  // a wave per query (the faster of the two forms, profiles/r18/points)
    const int g = static_cast<int>((nq + 3) / 4);
    if (fill)
      hipLaunchKernelGGL(k_pts_radius_wave<true>, dim3(g), dim3(256), 0, c->stream, idx->X, q, nq, radius, radii,
                         offset, capacity, static_cast<int32_t*>(nullptr), index);
    else
      hipLaunchKernelGGL(k_pts_radius_wave<false>, dim3(g), dim3(256), 0, c->stream, idx->X, q, nq, radius, radii,
                         static_cast<const int64_t*>(nullptr), int64_t(0), count, static_cast<int32_t*>(nullptr));
#else  // a lane per query
    const int g = static_cast<int>((nq + 255) / 256);
    if (fill)
      hipLaunchKernelGGL(k_pts_radius<true>, dim3(g), dim3(256), 0, c->stream, idx->X, q, nq, radius, radii, offset,
                         capacity, static_cast<int32_t*>(nullptr), index);
    else
      hipLaunchKernelGGL(k_pts_radius<false>, dim3(g), dim3(256), 0, c->stream, idx->X, q, nq, radius, radii,
                         static_cast<const int64_t*>(nullptr), int64_t(0), count, static_cast<int32_t*>(nullptr));
#endif
  };
  if (fill)
    return pts_call(c, idx, call, nq,
                    {in_q, in_radii, wr::in(offset, (nb + 1) * 8, "offset", 8), wr::out(index, cb * 4, "index", 4)},
                    launch);
  return pts_call(c, idx, call, nq, {in_q, in_radii, wr::out(count, nb * 4, "count", 4)}, launch);
}

int wr_points_count_dev(wr_context* c, const wr_points* idx, const float* q, int64_t nq, float radius,
                        const float* radii, int32_t* count) {
  return pts_radius_call(c, idx, "wr_points_count_dev", false, q, nq, radius, radii, nullptr, 0, count, nullptr);
}

int wr_points_in_radius_dev(wr_context* c, const wr_points* idx, const float* q, int64_t nq, float radius,
                            const float* radii, const int64_t* offset, int64_t capacity, int32_t* index) {
  return pts_radius_call(c, idx, "wr_points_in_radius_dev", true, q, nq, radius, radii, offset, capacity, nullptr,
                         index);
}

int wr_points_knn_dev(wr_context* c, const wr_points* idx, const float* q, int64_t nq, int32_t k, float max_sqr_dist,
                      int32_t* index, float* sqr_dist, int32_t* count) {
  const std::string who = "wr_points_knn_dev: ";
  if (c && nq >= 0) {
    if (k < 1 || k > 64) return fail(WR_E_ARG, who + "k must be 1..64");
    if (!(max_sqr_dist >= 0.f)) return fail(WR_E_ARG, who + "max_sqr_dist must not be negative or NaN");
  }
  const size_t nb = nq > 0 ? static_cast<size_t>(nq) : 0, kb = nb * static_cast<size_t>(k > 0 ? k : 0) * 4;
  return pts_call(c, idx, "wr_points_knn_dev", nq,
                  {wr::in(q, nb * 12, "q", 4), wr::out(index, kb, "index", 4), wr::out(sqr_dist, kb, "sqr_dist", 4),
                   wr::out(count, nb * 4, "count", 4)},
                  [&] {
    const int g = static_cast<int>((nq + 3) / 4);  // a wave per query
    hipLaunchKernelGGL(k_pts_knn, dim3(g), dim3(256), 0, c->stream, idx->X, q, nq, k, max_sqr_dist, index, sqr_dist,
                       count);
  });
}

// ---- photon mapping (wr_photon_*, wr_render_photon; kernels in
// wr_photon.h).  Everything runs on the context stream between api_order and
// api_finish, its traversals through api_trace like the ray calls'.
constexpr int kPhotonBatch = 65536;  // shots per batch when shot_batch is 0
static int photon_ctx(const wr_context* c, const std::string& who) {
  if (!c) return fail(WR_E_ARG, who + "null context");
  if (!c->subs.empty()) return fail(WR_E_ARG, who + "photon maps and their renders are single-device: create the context with wr_create");
  return WR_OK;
}
static int photon_map_arg(const wr_context* c, const wr_photon_map* map, const std::string& who) {
  if (!map) return fail(WR_E_ARG, who + "null map");
  if (map->ctx != c) return fail(WR_E_ARG, who + "the map belongs to another context");
  return WR_OK;
}

// the cell of a map's grid when the caller gives none: photons lie on
// surfaces, so about n cell^2 / extent^2 of them share a cell; 16 extent^2 / n
// keeps that near a dozen, a k = 50 search within two or three shells
static int photon_cell(wr_context* c, const float* dpos, int n, float* cell) {
  std::vector<float> h(size_t(n) * 3);
  HIPCHK(hipMemcpyAsync(h.data(), dpos, h.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ext = 0.f;
  for (int a = 0; a < 3; ++a) {
    float lo = h[a], hi = h[a];
    for (int i = 1; i < n; ++i) lo = std::min(lo, h[size_t(i) * 3 + a]), hi = std::max(hi, h[size_t(i) * 3 + a]);
    ext = std::max(ext, hi - lo);
  }
  const float v = ext * std::sqrt(16.f / static_cast<float>(n));
  *cell = (v > 0.f && std::isfinite(v)) ? v : 1.f;
  return WR_OK;
}

int wr_photon_map_build(wr_context* c, const wr_photon_map_params* prm, wr_photon_map** out, wr_stats* st) {
  const std::string who = "wr_photon_map_build: ";
  if (int rc = photon_ctx(c, who)) return rc;
  if (!prm || !out) return fail(WR_E_ARG, who + "null argument");
  *out = nullptr;
  const int cap[2] = {prm->n_caustic, prm->n_indirect};
  if (cap[0] < 0 || cap[1] < 0 || cap[0] > (1 << 24) || cap[1] > (1 << 24))
    return fail(WR_E_ARG, who + "n_caustic and n_indirect must be 0 .. 2^24");
  if (prm->max_path_length < 1 || prm->max_path_length > 32) return fail(WR_E_ARG, who + "max_path_length must be 1..32");
  if (prm->max_shots < 1 || prm->max_shots > 2147483647ll) return fail(WR_E_ARG, who + "max_shots must be 1 .. 2^31 - 1");
  if (prm->shot_batch < 0 || prm->shot_batch > (1 << 22)) return fail(WR_E_ARG, who + "shot_batch must be 0 .. 2^22");
  if (!(prm->cell >= 0.f) || !std::isfinite(prm->cell)) return fail(WR_E_ARG, who + "cell must be 0 or a finite number > 0");
  if (c->ds.nlights <= 0) return fail(WR_E_SCENE, who + "the scene has no area light");
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  const double t0 = host_now();
  const hipStream_t sm = c->stream;
  const int L = prm->max_path_length;
  const int B = static_cast<int>(std::min<int64_t>(prm->shot_batch ? prm->shot_batch : kPhotonBatch, prm->max_shots));
  const int nslot = B * L;
  std::unique_ptr<wr_photon_map> M(new wr_photon_map);
  M->ctx = c;
  for (int w = 0; w < 2; ++w)
    if (cap[w]) {
      if (int rc = M->side[w].pos.grow(size_t(cap[w]) * 3)) return rc;
      if (int rc = M->side[w].pay.grow(size_t(cap[w]) * 2)) return rc;
      if (int rc = M->side[w].shot.grow(size_t(cap[w]))) return rc;
    }
  // the batch's work block
  size_t scan_bytes = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, static_cast<const int*>(nullptr),
                                          static_cast<int*>(nullptr), nslot + 1, sm));
  PhBuf T{};
  int *fc = nullptr, *fi = nullptr, *pc = nullptr, *pi = nullptr;
  char* scan_tmp = nullptr;
  const auto layout = [&](Arena& a) {
    const size_t sB = B, sS = nslot;
    T.B = B, T.L = L;
    T.alpha = a.take<float>(3 * sB);
    T.spec = a.take<int>(sB);
    T.ctr = a.take<uint32_t>(sB);
    for (int q = 0; q < 2; ++q) {
      T.q_o[q] = a.take<float>(3 * sB);
      T.q_d[q] = a.take<float>(3 * sB);
      T.q_t[q] = a.take<float>(sB);
      T.q_prim[q] = a.take<int>(sB);
      T.q_shot[q] = a.take<int>(sB);
    }
    T.qn = a.take<int>(size_t(L) + 2);
    T.s_pos = a.take<float>(3 * sS);
    T.s_wi = a.take<float>(3 * sS);
    T.s_alpha = a.take<float>(3 * sS);
    T.s_class = a.take<int>(sS);
    fc = a.take<int>(sS + 1), fi = a.take<int>(sS + 1), pc = a.take<int>(sS + 1), pi = a.take<int>(sS + 1);
    scan_tmp = a.take<char>(std::max<size_t>(scan_bytes, 1));
  };
  Arena work;
  if (int rc = work.reserve(measure(layout))) return rc;
  layout(work);
  int64_t s0 = 0, paths[2] = {0, 0};
  bool full[2] = {cap[0] == 0, cap[1] == 0};
  int count[2] = {0, 0};
  while (s0 < prm->max_shots && !(full[0] && full[1])) {
    const int n = static_cast<int>(std::min<int64_t>(B, prm->max_shots - s0));
    HIPCHK(hipMemsetAsync(T.qn, 0, (size_t(L) + 2) * sizeof(int), sm));
    HIPCHK(hipMemsetAsync(T.s_class, 0, size_t(nslot) * sizeof(int), sm));
    const int g = std::max(1, std::min(c->grid, (n + 255) / 256));
    hipLaunchKernelGGL(k_ph_gen, dim3(g), dim3(256), 0, sm, c->ds, T, prm->seed, s0, n);
    for (int b = 0; b <= L; ++b) {  // nIntersections = b + 1 <= max_path_length + 1
      const int q = b & 1;
      if (int rc = api_trace(c, rq(T.q_o[q], T.q_d[q], B, &T.qn[b], T.q_t[q], T.q_prim[q]), size_t(B), false, TRACE_PLAIN))
        return rc;
      hipLaunchKernelGGL(k_ph_shade, dim3(g), dim3(256), 0, sm, c->ds, T, prm->seed, s0, b, L);
    }
    // the photons of each class in (shot, bounce) order: prefix sums over the slots, no atomics
    const int gs = std::max(1, std::min(c->grid, (nslot + 256) / 256));
    hipLaunchKernelGGL(k_ph_flags, dim3(gs), dim3(256), 0, sm, T.s_class, nslot, fc, fi);
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, fc, pc, nslot + 1, sm));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, fi, pi, nslot + 1, sm));
    const PhMapOut oc{M->side[0].pos.p, M->side[0].pay.p, M->side[0].shot.p, count[0], cap[0]};
    const PhMapOut oi{M->side[1].pos.p, M->side[1].pay.p, M->side[1].shot.p, count[1], cap[1]};
    hipLaunchKernelGGL(k_ph_scatter, dim3(gs), dim3(256), 0, sm, T, nslot, pc, pi, s0, oc, oi);
    HIPCHK(hipGetLastError());
    int total[2] = {0, 0};  // the two counters the host decides by
    HIPCHK(hipMemcpyAsync(&total[0], pc + nslot, sizeof(int), hipMemcpyDeviceToHost, sm));
    HIPCHK(hipMemcpyAsync(&total[1], pi + nslot, sizeof(int), hipMemcpyDeviceToHost, sm));
    HIPCHK(hipStreamSynchronize(sm));
    for (int w = 0; w < 2; ++w) {
      if (full[w]) continue;
      count[w] = static_cast<int>(std::min<int64_t>(cap[w], int64_t(count[w]) + total[w]));
      if (count[w] == cap[w]) {  // the shot that stored the map's last photon (:107, :120)
        int32_t last = 0;
        HIPCHK(hipMemcpy(&last, M->side[w].shot.p + (cap[w] - 1), sizeof last, hipMemcpyDeviceToHost));
        full[w] = true;
        paths[w] = int64_t(last) + 1;
      }
    }
    s0 += n;
  }
  // the serial loop stops after the shot that filled the second map
  const int64_t shots = (full[0] && full[1]) ? std::min(s0, std::max(paths[0], paths[1])) : s0;
  work.release();
  wr_photon_map_info& I = M->info;
  I.shots = shots;
  I.caustic_count = count[0], I.indirect_count = count[1];
  I.caustic_paths = (full[0] && cap[0]) ? paths[0] : shots;
  I.indirect_paths = (full[1] && cap[1]) ? paths[1] : shots;
  float cells[2] = {0.f, 0.f};
  for (int w = 0; w < 2; ++w) {
    wr_photon_map::Side& s = M->side[w];
    s.count = count[w];
    I.device_bytes += static_cast<int64_t>(s.pos.n * 4 + s.pay.n * 16 + s.shot.n * 4);
    if (!count[w]) continue;
    float cell = prm->cell;
    if (!(cell > 0.f))
      if (int rc = photon_cell(c, s.pos.p, count[w], &cell)) return rc;
    if (int rc = wr_points_build_dev(c, s.pos.p, count[w], cell, &s.idx)) {
      for (int v = 0; v < w; ++v) wr_points_free(M->side[v].idx);
      return rc;
    }
    wr_points_info pinfo;
    (void)wr_points_info_get(s.idx, &pinfo);
    I.device_bytes += pinfo.device_bytes;
    cells[w] = cell;
  }
  I.caustic_cell = cells[0], I.indirect_cell = cells[1];
  if (st) {
    *st = wr_stats{};
    st->seconds = host_now() - t0;
    st->pipelines = 1;
  }
  c->photon_maps.push_back(M.get());
  *out = M.release();
  return WR_OK;
}

int wr_photon_map_info_get(const wr_photon_map* map, wr_photon_map_info* out) {
  if (!map || !out) return fail(WR_E_ARG, "wr_photon_map_info_get: null argument");
  *out = map->info;
  return WR_OK;
}

void wr_photon_map_free(wr_photon_map* map) {
  if (!map) return;
  wr_context* c = map->ctx;
  for (int w = 0; w < 2; ++w) wr_points_free(map->side[w].idx);
  DeviceGuard dg;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->photon_maps.erase(std::remove(c->photon_maps.begin(), c->photon_maps.end(), map), c->photon_maps.end());
  delete map;
}

int wr_photon_map_read(wr_context* c, const wr_photon_map* map, int which, float* pos, float* wi, float* alpha,
                       int32_t* shot, int on_device) {
  const std::string who = "wr_photon_map_read: ";
  if (int rc = photon_ctx(c, who)) return rc;
  if (int rc = photon_map_arg(c, map, who)) return rc;
  if (which != WR_PHOTON_CAUSTIC && which != WR_PHOTON_INDIRECT) return fail(WR_E_ARG, who + "which must be WR_PHOTON_*");
  const wr_photon_map::Side& s = map->side[which];
  const size_t n = static_cast<size_t>(s.count);
  if (!n) return WR_OK;
  if (on_device)
    if (int rc = check_dev_args(c, "wr_photon_map_read",
                                {wr::out(pos, n * 12, "pos", 4, true), wr::out(wi, n * 12, "wi", 4, true),
                                 wr::out(alpha, n * 12, "alpha", 4, true), wr::out(shot, n * 4, "shot", 4, true)},
                                "wr_photon_map_read with on_device = 0"))
      return rc;
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (pos) HIPCHK(hipMemcpyAsync(pos, s.pos.p, n * 12, kind, c->stream));
  if (shot) HIPCHK(hipMemcpyAsync(shot, s.shot.p, n * 4, kind, c->stream));
  if (wi) HIPCHK(hipMemcpy2DAsync(wi, 12, s.pay.p, 32, 12, n, kind, c->stream));
  if (alpha) HIPCHK(hipMemcpy2DAsync(alpha, 12, s.pay.p + 1, 32, 12, n, kind, c->stream));
  return api_finish(c);
}

static void gather_launch(wr_context* c, const PmMap& M, const wr_hit* hits, const float* wo, int64_t n,
                          const int* n_dev, int k, float msd, float* rgb, float* msd_out, int32_t* found,
                          const float* weight, const int* pix, float* film) {
  const int g = static_cast<int>(std::min<int64_t>((n + 3) / 4, n_dev ? 16384 : (int64_t(1) << 26)));  // a wave per query
  hipLaunchKernelGGL(k_pm_gather, dim3(std::max(1, g)), dim3(256), 0, c->stream, c->ds, c->nmats, M, hits, wo, n, n_dev,
                     k, msd, rgb, msd_out, found, weight, pix, film);
}

int wr_photon_estimate_dev(wr_context* c, const wr_photon_map* map, int which, const wr_hit* hits, const float* wo,
                           int64_t n, int32_t k, float max_sqr_dist, float* rgb, float* msd, int32_t* found) {
  const std::string who = "wr_photon_estimate_dev: ";
  if (int rc = photon_ctx(c, who)) return rc;
  if (n < 0) return fail(WR_E_ARG, who + "n < 0");
  if (int rc = photon_map_arg(c, map, who)) return rc;
  if (which != WR_PHOTON_CAUSTIC && which != WR_PHOTON_INDIRECT) return fail(WR_E_ARG, who + "which must be WR_PHOTON_*");
  if (k < 1 || k > 64) return fail(WR_E_ARG, who + "k must be 1..64");
  if (!(max_sqr_dist > 0.f) || !std::isfinite(max_sqr_dist)) return fail(WR_E_ARG, who + "max_sqr_dist must be a finite number > 0");
  if (n > (int64_t(1) << 28)) return fail(WR_E_ARG, who + "at most 2^28 queries per call");
  const size_t nb = static_cast<size_t>(n);
  if (n == 0) return WR_OK;
  if (int rc = check_dev_args(c, "wr_photon_estimate_dev",
                              {wr::in(hits, nb * sizeof(wr_hit), "hits", 4), wr::in(wo, nb * 12, "wo", 4),
                               wr::out(rgb, nb * 12, "rgb", 4), wr::out(msd, nb * 4, "msd", 4, true),
                               wr::out(found, nb * 4, "found", 4, true)},
                              "no photon call: copy it to the device"))
    return rc;
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  gather_launch(c, map->dev(which), hits, wo, n, nullptr, k, max_sqr_dist, rgb, msd, found, nullptr, nullptr, nullptr);
  return api_finish(c);
}

int wr_render_photon(wr_context* c, const wr_photon_map* map, const wr_photon_params* prm, float* film,
                     int film_on_device, wr_stats* st) {
  const std::string who = "wr_render_photon: ";
  if (int rc = photon_ctx(c, who)) return rc;
  if (int rc = photon_map_arg(c, map, who)) return rc;
  if (!prm || !film) return fail(WR_E_ARG, who + "null argument");
  if (prm->width <= 0 || prm->height <= 0 || prm->spp <= 0) return fail(WR_E_ARG, who + "bad film size / spp");
  if (static_cast<int64_t>(prm->width) * prm->height > (int64_t(1) << 26)) return fail(WR_E_ARG, who + "film too large (2^26 pixels)");
  if (prm->sample_begin < 0 || prm->sample_count < 0 || prm->sample_begin > prm->spp ||
      static_cast<int64_t>(prm->sample_begin) + prm->sample_count > prm->spp)
    return fail(WR_E_ARG, who + "samples [sample_begin, sample_begin + sample_count) must lie in [0, spp)");
  if (prm->knn < 1 || prm->knn > 64) return fail(WR_E_ARG, who + "knn must be 1..64");
  if (!(prm->max_sqr_dist > 0.f) || !std::isfinite(prm->max_sqr_dist))
    return fail(WR_E_ARG, who + "max_sqr_dist must be a finite number > 0");
  if (c->ds.nlights <= 0) return fail(WR_E_SCENE, who + "the scene has no area light");
  const int P = prm->width * prm->height;
  const size_t nf = size_t(P) * 3;
  if (film_on_device)
    if (int rc = check_dev_args(c, "wr_render_photon", {wr::out(film, nf * 4, "film", 4)}, "film_on_device = 0")) return rc;
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  const double t0 = host_now();
  const hipStream_t sm = c->stream;
  PtBuf T{};
  PmGq GQ{};
  StepCounters* sc = nullptr;
  const auto layout = [&](Arena& a) {
    layout_pt(a, T, P);
    GQ.hits = a.take<wr_hit>(size_t(P));
    GQ.wo = a.take<float>(nf);
    GQ.weight = a.take<float>(nf);
    GQ.pix = a.take<int>(size_t(P));
    sc = a.take<StepCounters>(1);
  };
  Arena work;
  if (int rc = work.reserve(measure(layout))) return rc;
  layout(work);
  float* dfilm = nullptr;
  if (int rc = film_target(c, film, film_on_device, nf, &dfilm)) return rc;
  PtGroup GA;
  PtArgs& A = GA.a[0];
  A.S = c->ds;
  A.T = T;
  A.ctr = c->ctr;
  A.sc = sc;
  A.film = dfilm;
  A.W = prm->width;
  A.H = prm->height;
  A.P = P;
  A.spp = prm->spp;
  A.grid_len = static_cast<int>(std::sqrt(static_cast<double>(prm->spp)));
  A.max_depth = 2;
  A.seed = prm->seed;
  const PmMap maps[2] = {map->dev(WR_PHOTON_INDIRECT), map->dev(WR_PHOTON_CAUSTIC)};  // the order their terms are added in
  const int k0 = prm->sample_begin, k1 = prm->sample_count > 0 ? k0 + prm->sample_count : prm->spp;
  const int g = shade_grid(c, P);
  for (int k = k0; k < k1; ++k) {
    A.k = static_cast<uint32_t>(k);
    HIPCHK(hipMemsetAsync(sc, 0, sizeof(StepCounters), sm));
    hipLaunchKernelGGL(k_pt_gen, dim3(g, 1), dim3(kShadeBlock), 0, sm, GA);
    for (int depth = 0; depth <= 2; ++depth) {
      const int q = depth & 1;
      if (int rc = api_trace(c, rq(T.q_o[q], T.q_d[q], P, &sc->ext[depth], T.q_t[q], T.q_prim[q]), size_t(P), false,
                             TRACE_PLAIN))
        return rc;
      hipLaunchKernelGGL(k_pm_shade, dim3(g), dim3(kShadeBlock), 0, sm, GA, depth, GQ, prm->direct_target);
      // the three terms in the reference's order: direct light, the indirect map, the caustic map
      const PtBuf::Sq& Q = T.sq[(depth + 1) & 1];
      if (int rc = api_trace(c, rq(Q.o, Q.d, P, &sc->sq[depth + 1], Q.t, Q.prim, Q.cut), size_t(P), false, TRACE_CUT))
        return rc;
      hipLaunchKernelGGL(k_pt_step, dim3(g, 1), dim3(kShadeBlock), 0, sm, GA, depth + 1, g, 0);
      for (const PmMap& M : maps)
        gather_launch(c, M, GQ.hits, GQ.wo, P, &sc->mq[depth], prm->knn, prm->max_sqr_dist, nullptr, nullptr, nullptr,
                      GQ.weight, GQ.pix, dfilm);
    }
  }
  if (int rc = api_finish(c)) return rc;
  if (st) {
    *st = wr_stats{};
    st->seconds = host_now() - t0;
    st->pipelines = 1;
  }
  return film_return(c, film, film_on_device, nf);
}

int wr_create_multi(const wr_scene* sc, const int* devices, int n, wr_context** out) {
  if (!sc || !devices || !out || n < 1 || n > 64) return fail(WR_E_ARG, "bad argument (1..64 devices)");
  *out = nullptr;
  if (int rc = check_device()) return rc;
  DeviceGuard dg;
  int have = 0;
  (void)hipGetDeviceCount(&have);
  for (int k = 0; k < n; ++k)
    if (devices[k] < 0 || devices[k] >= have)
      return fail(WR_E_ARG, "device " + std::to_string(devices[k]) + " not visible (" + std::to_string(have) + ")");
  // one context per device, created concurrently (scene upload + BVH build each)
  std::vector<ContextPtr> ctx(n);
  std::vector<int> rc(n, WR_OK);
  std::vector<std::string> msg(n);
  {
    std::vector<std::thread> th;
    for (int k = 0; k < n; ++k)
      th.emplace_back([&, k] {
        wr_context* made = nullptr;
        rc[k] = wr_create(sc, devices[k], &made);
        ctx[k].reset(made);
        if (rc[k] != WR_OK) msg[k] = wr::last_error();
      });
    for (auto& t : th) t.join();
  }
  for (int k = 0; k < n; ++k)
    if (rc[k] != WR_OK) return fail(rc[k], "device " + std::to_string(devices[k]) + ": " + msg[k]);
  ContextPtr c = std::move(ctx[0]);
  for (int k = 1; k < n; ++k) c->subs.push_back(ctx[k].release());  // c owns them from here (wr_destroy)
  // RCCL communicators over the devices when they are distinct (a device
  // listed twice -- tests on one GPU -- sums by copies); WR_MULTI_REDUCE=peer
  // forces the copies
  bool distinct = true;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b) distinct = distinct && devices[a] != devices[b];
  const char* mode = std::getenv("WR_MULTI_REDUCE");
  const bool want = !(mode && std::string(mode) == "peer");
  if (n > 1 && distinct && want) {
    if (!rccl().ok) return fail(WR_E_HIP, rccl().why);
    std::vector<ncclComm_t> comms(n, nullptr);
    const ncclResult_t r = rccl().init_all(comms.data(), n, devices);
    if (r != ncclSuccess) return fail(WR_E_HIP, std::string("ncclCommInitAll: ") + rccl().err_str(r));
    c->dev_comms = comms;
  }
  *out = c.release();
  return WR_OK;
}

int wr_context_devices(const wr_context* c, int* devices, int max_n) {
  if (!c || max_n < 0 || (max_n > 0 && !devices)) return fail(WR_E_ARG, "bad argument");
  const int n = 1 + static_cast<int>(c->subs.size());
  for (int k = 0; k < n && k < max_n; ++k) devices[k] = k == 0 ? c->device : c->subs[k - 1]->device;
  return n;
}

// ---- one process per GPU: this rank's RCCL communicator and the film reduce
int wr_comm_unique_id(uint8_t id[128]) {
  if (!id) return fail(WR_E_ARG, "null argument");
  if (!rccl().ok) return fail(WR_E_HIP, rccl().why);
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId u;
  NCCLCHK(rccl().get_unique_id(&u));
  std::memcpy(id, &u, sizeof u);
  return WR_OK;
}

int wr_comm_init(wr_context* c, const uint8_t id[128], int nranks, int rank) {
  if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(WR_E_ARG, "bad argument");
  if (!c->subs.empty()) return fail(WR_E_ARG, "a multi-device context reduces over its own devices");
  if (!rccl().ok) return fail(WR_E_HIP, rccl().why);
  DeviceGuard dg;
  HIPCHK(hipSetDevice(c->device));
  if (c->comm) (void)rccl().destroy(c->comm);
  c->comm = nullptr;
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  NCCLCHK(rccl().init_rank(&c->comm, nranks, u, rank));
  c->comm_ranks = nranks;
  c->comm_rank = rank;
  return WR_OK;
}

int wr_comm_info(const wr_context* c, int* nranks, int* rank) {
  if (!c || !nranks || !rank) return fail(WR_E_ARG, "null argument");
  if (!c->comm) return fail(WR_E_ARG, "no communicator: call wr_comm_init first");
  // read back from the communicator itself (ncclCommCount / ncclCommUserRank),
  // not from what wr_comm_init was given
  NCCLCHK(rccl().count(c->comm, nranks));
  NCCLCHK(rccl().user_rank(c->comm, rank));
  return WR_OK;
}

int wr_film_reduce(wr_context* c, float* film, int64_t nfloat, int root) {
  if (!c || (!film && nfloat) || nfloat < 0) return fail(WR_E_ARG, "bad argument");
  if (!c->comm) return fail(WR_E_ARG, "no communicator: call wr_comm_init first");
  if (root < 0 || root >= c->comm_ranks) return fail(WR_E_ARG, "bad root rank");
  DeviceGuard dg;
  if (int rc = api_order(c)) return rc;
  NCCLCHK(rccl().reduce(film, film, static_cast<size_t>(nfloat), ncclFloat32, ncclSum, root, c->comm, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return WR_OK;
}

}  // extern "C"
