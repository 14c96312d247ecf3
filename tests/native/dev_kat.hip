// libwr_devkat.so -- test infrastructure, not part of libwinmad_rt.so: the
// device functions of csrc/wr_devmath.h and csrc/wr_libm.h run by themselves
// on the GPU, one bounds-checked thread per case, so that tests/test_gpu_devkat.py
// can compare each of them with the reference's known answers and with the
// oracle's hooks (oracle/cpuref.c cr_kat_*), whose output layouts the entry
// points below keep.
//
// Built with the product's flags (Makefile HIPFLAGS) and its no-packed-fp32
// kernel attribute, and linked with the product's own host objects: a scene is
// loaded by wr::load_scene and flattened by wr::flatten_scene, and the kernels
// read the DMat / DLight records of that flattening and a DCam filled as
// wr_render.hip fills it.  No LDS, no atomics; material and light indices are
// checked on the host before a launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "wr_devmath.h"
#include "wr_flatten.h"
#include "wr_scene.h"

using namespace wrd;

#ifdef __HIP_DEVICE_COMPILE__
#define WR_NO_PK_FP32 __attribute__((target("no-packed-fp32-ops")))
#else
#define WR_NO_PK_FP32
#endif
#define DK_KERNEL __global__ void __launch_bounds__(256) WR_NO_PK_FP32

static_assert(sizeof(wr::Light) == sizeof(DLight) && offsetof(wr::Light, inv_area) == offsetof(DLight, inv_area),
              "Light is DLight");
static_assert(sizeof(wr::Material) == sizeof(DMat) && offsetof(wr::Material, index) == offsetof(DMat, index),
              "Material is DMat");

namespace {

constexpr float kUnset = -7.f;  // the sentinel of the reference driver's and the oracle's hooks

__device__ __forceinline__ V3 ld3(const float* p, int64_t i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ void st3(float* p, V3 v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}

// cr_kat_sampler (9) + cr_kat_triangle (3) + cr_kat_strat (3)
DK_KERNEL k_sampler(int64_t n, const float* u, const float* power, const float* tri, const int* k, const int* len,
                    float* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* o = out + 15 * i;
  const V3 s = ld3(u, i);
  float pdf = -1.f;
  st3(o, sample_cos_hemi(s, &pdf));
  o[3] = pdf;
  const V3 b = sample_pow_cos_hemi(s, power[i]);
  st3(o + 4, b);
  o[7] = kUnset;  // sample_pow_cos_hemi returns no pdf
  o[8] = pow_cos_pdf(v3(0.f, 0.f, 1.f), b, power[i]);
  st3(o + 9, sample_triangle(s, ld3(tri, 3 * i), ld3(tri, 3 * i + 1), ld3(tri, 3 * i + 2)));
  st3(o + 12, sample_rect_strat(s, v3(3.f, 4.f, 0.f), v3(4.f, 4.f, 0.f), v3(3.f, 5.f, 0.f), k[i], len[i]));
}

// cr_kat_frame (9) + cr_kat_fresnel (1)
DK_KERNEL k_frame(int64_t n, const float* z, const float* ci, const float* idx, float* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* o = out + 10 * i;
  const Frame f = frame_from_z(ld3(z, i));
  st3(o, f.x);
  st3(o + 3, f.y);
  st3(o + 6, f.z);
  o[9] = fresnel(ci[i], idx[i]);
}

// cr_kat_bsdf: 25 floats of a row of 26, and the valid flag
DK_KERNEL k_bsdf(int64_t n, const DMat* mats, const int* mat, const float* nrm, const float* wi, const float* wo,
                 const float* r3, float* out, int* valid) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* o = out + 26 * i;
  Bsdf b;
  bsdf_init(b, ld3(wi, i), ld3(nrm, i), mat[i], mats);
  valid[i] = b.mat != 0;
  if (b.mat == 0) return;
  o[0] = b.delta ? 1.f : 0.f;
  o[1] = b.wi.z;
  o[2] = b.cont;
  o[3] = b.fres;
  o[4] = b.pd;
  o[5] = b.pg;
  o[6] = b.pr;
  o[7] = b.pt;
  float cw = kUnset, dp = kUnset, rp = kUnset;
  st3(o + 8, bsdf_f(b, mats, ld3(wo, i), &cw, &dp, &rp));
  o[11] = cw;
  o[12] = dp;
  o[13] = rp;
  o[14] = bsdf_pdf(b, mats, ld3(wo, i), false);
  o[15] = bsdf_pdf(b, mats, ld3(wo, i), true);
  V3 ow = v3(kUnset, kUnset, kUnset);
  float sp = kUnset, sc = kUnset;
  int ty = -7;
  st3(o + 17, bsdf_sample(b, mats, ld3(r3, i), &ow, &sp, &sc, &ty));
  o[16] = static_cast<float>(ty);
  st3(o + 20, ow);
  o[23] = sp;
  o[24] = sc;
}

// cr_kat_light (27)
DK_KERNEL k_light(int64_t n, const DLight* lights, const int* li, const float* pos, const float* r3, const float* dr,
                  const float* pr, const float* rd, float* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* o = out + 27 * i;
  const DLight l = lights[li[i]];
  V3 dtl = v3(kUnset, kUnset, kUnset);
  float dist = kUnset, dp = kUnset, ep = kUnset, cal = kUnset;
  st3(o, light_illuminance(l, ld3(pos, i), ld3(r3, i), &dtl, &dist, &dp, &ep, &cal));
  st3(o + 3, dtl);
  o[6] = dist;
  o[7] = dp;
  o[8] = ep;
  o[9] = cal;
  V3 p, d;
  float emp = kUnset, dpa = kUnset, cal2 = kUnset;
  st3(o + 10, light_emit(l, ld3(dr, i), ld3(pr, i), &p, &d, &emp, &dpa, &cal2));
  st3(o + 13, p);
  st3(o + 16, d);
  o[19] = emp;
  o[20] = dpa;
  o[21] = cal2;
  float gpa = kUnset, gep = kUnset;
  st3(o + 22, light_radiance(l, ld3(rd, i), &gpa, &gep));
  o[25] = gpa;
  o[26] = gep;
}

// t_point(r2w, (x, y, 0)) (3), t_point(w2r, w) (3), check_raster of the latter (1)
DK_KERNEL k_camera(int64_t n, DCam cam, const float* xy, const float* w, float* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* o = out + 7 * i;
  st3(o, t_point(cam.r2w, v3(xy[2 * i], xy[2 * i + 1], 0.f)));
  const V3 ras = t_point(cam.w2r, ld3(w, i));
  st3(o + 3, ras);
  o[6] = check_raster(cam, ras.x, ras.y) ? 1.f : 0.f;
}

// stream_key of keys4[4i..] = (seed, iteration, subpath, path), then `draws` of Rng::u32 and of Rng::f
// (the same counters from a second generator, as f() consumes a draw)
DK_KERNEL k_rng(int64_t n, const uint32_t* keys4, int draws, uint64_t* key, uint32_t* u, float* f) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Rng a, b;
  a.key = b.key = stream_key(keys4[4 * i], keys4[4 * i + 1], keys4[4 * i + 2], keys4[4 * i + 3]);
  a.ctr = b.ctr = 0;
  key[i] = a.key;
  for (int j = 0; j < draws; ++j) {
    u[i * draws + j] = a.u32();
    f[i * draws + j] = b.f();
  }
}

// op 0 wr_sinf, 1 wr_cosf, 2 wr_sincosf (sin -> out, cos -> out2), 3 wr_powf(x, y)
DK_KERNEL k_libm(int op, int64_t n, const float* x, const float* y, float* out, float* out2) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (op == 0) {
    out[i] = wr_sinf(x[i]);
  } else if (op == 1) {
    out[i] = wr_cosf(x[i]);
  } else if (op == 2) {
    float s, c;
    wr_sincosf(x[i], &s, &c);
    out[i] = s;
    out2[i] = c;
  } else {
    out[i] = wr_powf(x[i], y[i]);
  }
}

thread_local std::string g_err;

int fail(const std::string& m) {
  g_err = m;
  return -1;
}

// device buffers of one call: freed when the call returns
struct Bufs {
  std::vector<void*> p;
  bool ok = true;
  std::string why;
  ~Bufs() {
    for (void* q : p) (void)hipFree(q);
  }
  void check(hipError_t e, const char* what) {
    if (ok && e != hipSuccess) {
      ok = false;
      why = std::string(what) + ": " + hipGetErrorString(e);
    }
  }
  template <class T>
  T* alloc(int64_t count) {
    void* q = nullptr;
    if (ok) check(hipMalloc(&q, static_cast<size_t>(count > 0 ? count : 1) * sizeof(T)), "hipMalloc");
    if (q) p.push_back(q);
    return static_cast<T*>(q);
  }
  template <class T>
  T* in(const T* host, int64_t count) {
    T* d = alloc<T>(count);
    if (ok && count > 0) check(hipMemcpy(d, host, static_cast<size_t>(count) * sizeof(T), hipMemcpyHostToDevice), "upload");
    return d;
  }
  // an output the caller preset (sentinels): uploaded, overwritten where the kernel writes
  template <class T>
  T* inout(const T* host, int64_t count) { return in(host, count); }
  template <class T>
  void out(T* host, const T* dev, int64_t count) {
    if (ok && count > 0) check(hipMemcpy(host, dev, static_cast<size_t>(count) * sizeof(T), hipMemcpyDeviceToHost), "download");
  }
  void ran() {
    check(hipGetLastError(), "launch");
    check(hipDeviceSynchronize(), "kernel");
  }
  int result() { return ok ? 0 : fail(why); }
};

inline dim3 grid_for(int64_t n) { return dim3(static_cast<unsigned>((n + 255) / 256)); }

struct DkScene {
  wr::Scene scene;
  wr::SceneFlat flat;
  DCam cam;
};

}  // namespace

void dk_libm_host(int op, int64_t n, const float* x, const float* y, float* out, float* out2);  // dev_kat_host.cpp

extern "C" {

const char* dk_last_error() { return g_err.c_str(); }

int dk_scene_load(const char* path, void** out) {
  auto* s = new DkScene();
  std::string err;
  if (!wr::load_scene(path, s->scene, err)) {
    delete s;
    return fail("load_scene: " + err);
  }
  wr::flatten_scene(s->scene, s->flat);
  const wr::Camera& c = s->scene.cam;  // as wr_render.hip fills DevScene::cam
  s->cam.pos = v3(c.pos.x, c.pos.y, c.pos.z);
  s->cam.fwd = v3(c.fwd.x, c.fwd.y, c.fwd.z);
  s->cam.xres = c.xres;
  s->cam.yres = c.yres;
  s->cam.plane_dist = c.plane_dist;
  std::memcpy(s->cam.w2r, c.w2r, sizeof s->cam.w2r);
  std::memcpy(s->cam.r2w, c.r2w, sizeof s->cam.r2w);
  *out = s;
  return 0;
}
void dk_scene_free(void* h) { delete static_cast<DkScene*>(h); }
int dk_scene_nmats(const void* h) { return static_cast<int>(static_cast<const DkScene*>(h)->flat.mats.size()); }
int dk_scene_nlights(const void* h) { return static_cast<int>(static_cast<const DkScene*>(h)->flat.lights.size()); }

// out: n x 15, tot[i] is the sample count whose integer square root is the strata per side
int dk_sampler(int64_t n, const float* u, const float* power, const float* tri, const int* k, const int* tot,
               float* out) {
  if (n < 0) return fail("n < 0");
  std::vector<int> len(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    len[i] = static_cast<int>(std::sqrt(static_cast<double>(tot[i])));  // sampler.cpp:31
    if (len[i] < 1) return fail("tot < 1");
  }
  Bufs b;
  const float* du = b.in(u, 3 * n);
  const float* dp = b.in(power, n);
  const float* dt = b.in(tri, 9 * n);
  const int* dk = b.in(k, n);
  const int* dl = b.in(len.data(), n);
  float* dout = b.alloc<float>(15 * n);
  if (b.ok && n > 0) {
    hipLaunchKernelGGL(k_sampler, grid_for(n), dim3(256), 0, 0, n, du, dp, dt, dk, dl, dout);
    b.ran();
  }
  b.out(out, dout, 15 * n);
  return b.result();
}

// out: n x 10
int dk_frame(int64_t n, const float* z, const float* ci, const float* idx, float* out) {
  if (n < 0) return fail("n < 0");
  Bufs b;
  const float* dz = b.in(z, 3 * n);
  const float* dc = b.in(ci, n);
  const float* di = b.in(idx, n);
  float* dout = b.alloc<float>(10 * n);
  if (b.ok && n > 0) {
    hipLaunchKernelGGL(k_frame, grid_for(n), dim3(256), 0, 0, n, dz, dc, di, dout);
    b.ran();
  }
  b.out(out, dout, 10 * n);
  return b.result();
}

// out: n x 26 preset by the caller (what the kernel does not write stays), valid: n
int dk_bsdf(const void* h, int64_t n, const int* mat, const float* nrm, const float* wi, const float* wo,
            const float* r3, float* out, int* valid) {
  const DkScene* s = static_cast<const DkScene*>(h);
  if (!s || n < 0) return fail("no scene or n < 0");
  const int nm = static_cast<int>(s->flat.mats.size());
  for (int64_t i = 0; i < n; ++i)
    if (mat[i] < 1 || mat[i] >= nm) return fail("material index out of range");
  Bufs b;
  const DMat* dm = reinterpret_cast<const DMat*>(b.in(s->flat.mats.data(), nm));
  const int* dmat = b.in(mat, n);
  const float* dn = b.in(nrm, 3 * n);
  const float* dwi = b.in(wi, 3 * n);
  const float* dwo = b.in(wo, 3 * n);
  const float* dr = b.in(r3, 3 * n);
  float* dout = b.inout(out, 26 * n);
  int* dv = b.alloc<int>(n);
  if (b.ok && n > 0) {
    hipLaunchKernelGGL(k_bsdf, grid_for(n), dim3(256), 0, 0, n, dm, dmat, dn, dwi, dwo, dr, dout, dv);
    b.ran();
  }
  b.out(out, dout, 26 * n);
  b.out(valid, dv, n);
  return b.result();
}

// out: n x 27
int dk_light(const void* h, int64_t n, const int* li, const float* pos, const float* r3, const float* dr,
             const float* pr, const float* rd, float* out) {
  const DkScene* s = static_cast<const DkScene*>(h);
  if (!s || n < 0) return fail("no scene or n < 0");
  const int nl = static_cast<int>(s->flat.lights.size());
  for (int64_t i = 0; i < n; ++i)
    if (li[i] < 0 || li[i] >= nl) return fail("light index out of range");
  Bufs b;
  const DLight* dl = reinterpret_cast<const DLight*>(b.in(s->flat.lights.data(), nl));
  const int* dli = b.in(li, n);
  const float* dpos = b.in(pos, 3 * n);
  const float* dr3 = b.in(r3, 3 * n);
  const float* ddr = b.in(dr, 3 * n);
  const float* dpr = b.in(pr, 3 * n);
  const float* drd = b.in(rd, 3 * n);
  float* dout = b.alloc<float>(27 * n);
  if (b.ok && n > 0) {
    hipLaunchKernelGGL(k_light, grid_for(n), dim3(256), 0, 0, n, dl, dli, dpos, dr3, ddr, dpr, drd, dout);
    b.ran();
  }
  b.out(out, dout, 27 * n);
  return b.result();
}

// xy: n x 2 raster points, w: n x 3 world points; out: n x 7
int dk_camera(const void* h, int64_t n, const float* xy, const float* w, float* out) {
  const DkScene* s = static_cast<const DkScene*>(h);
  if (!s || n < 0) return fail("no scene or n < 0");
  Bufs b;
  const float* dxy = b.in(xy, 2 * n);
  const float* dw = b.in(w, 3 * n);
  float* dout = b.alloc<float>(7 * n);
  if (b.ok && n > 0) {
    hipLaunchKernelGGL(k_camera, grid_for(n), dim3(256), 0, 0, n, s->cam, dxy, dw, dout);
    b.ran();
  }
  b.out(out, dout, 7 * n);
  return b.result();
}

// keys4: n x 4 (seed, iteration, subpath, path); key: n, u and f: n x draws
int dk_rng(int64_t n, const uint32_t* keys4, int draws, uint64_t* key, uint32_t* u, float* f) {
  if (n < 0 || draws < 0) return fail("n < 0 or draws < 0");
  Bufs b;
  const uint32_t* dk = b.in(keys4, 4 * n);
  uint64_t* dkey = b.alloc<uint64_t>(n);
  uint32_t* du = b.alloc<uint32_t>(n * draws);
  float* df = b.alloc<float>(n * draws);
  if (b.ok && n > 0) {
    hipLaunchKernelGGL(k_rng, grid_for(n), dim3(256), 0, 0, n, dk, draws, dkey, du, df);
    b.ran();
  }
  b.out(key, dkey, n);
  b.out(u, du, n * draws);
  b.out(f, df, n * draws);
  return b.result();
}

// op 0 sin, 1 cos, 2 sincos (out, out2), 3 pow(x, y); y and out2 may be null for the ops that do not use them
int dk_libm(int op, int64_t n, const float* x, const float* y, float* out, float* out2) {
  if (n < 0 || op < 0 || op > 3 || (op == 3 && !y) || (op == 2 && !out2)) return fail("bad libm arguments");
  Bufs b;
  const float* dx = b.in(x, n);
  const float* dy = op == 3 ? b.in(y, n) : nullptr;
  float* dout = b.alloc<float>(n);
  float* dout2 = op == 2 ? b.alloc<float>(n) : nullptr;
  if (b.ok && n > 0) {
    hipLaunchKernelGGL(k_libm, grid_for(n), dim3(256), 0, 0, op, n, dx, dy, dout, dout2);
    b.ran();
  }
  b.out(out, dout, n);
  if (op == 2) b.out(out2, dout2, n);
  return b.result();
}

// the same header compiled for the host by g++ (dev_kat_host.cpp), the chain tests/test_libm.py pins to glibc
int dk_libm_expected(int op, int64_t n, const float* x, const float* y, float* out, float* out2) {
  if (n < 0 || op < 0 || op > 3 || (op == 3 && !y) || (op == 2 && !out2)) return fail("bad libm arguments");
  dk_libm_host(op, n, x, y, out, out2);
  return 0;
}

}  // extern "C"
