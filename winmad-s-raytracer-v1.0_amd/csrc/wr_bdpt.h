// BidirPathTracing::runIteration (surfaceIntegrator/bidirPathTracing.cpp:53-265)
// as wavefront kernels.  Two schedules (wr_render.hip, render_bdpt_one):
//   sequential: light pass gen -> [trace -> shade] x 9, then camera pass gen ->
//     [trace -> resolve + shade] x 11, as the reference orders them;
//   overlapped (default): both passes start together and bounce b of each is
//     traced by one launch (gen, then 11 steps).  A light vertex of length l
//     and a camera vertex of length c of the same path (the only pairing,
//     :130, :222-229) are connected by the vertex created second: the camera
//     side connects the light vertices stored so far (l <= c: the light
//     kernel of a step runs before the camera kernel), the light side the
//     camera vertices stored at earlier steps (c < l; camera vertices that
//     can still meet a later light vertex, c <= (maxlen - 2) / 2, are kept in
//     a small store, CV_*).  Every pair the reference connects (:219-257) is
//     connected once, with the same floats (connect_pair); only the order of
//     the film's float additions differs.
// Included by wr_render.hip inside its anonymous namespace (uses its device
// helpers: wave_append, ld3/st3, film_add, the counter slots).
#pragma once

// =============================================================== BDPT state
// Light / camera subpath state (bidirPathTracing.h:7-18), one 64-byte record
// per path: the vertex kernels gather it by path index (the queue's order), so
// a lane's state is one cache line instead of 15 words in 15 arrays.
enum : int {
  PS_O = 0, PS_D = 3, PS_THR = 6, PS_DVCM = 9, PS_DVC = 10, PS_LEN = 11, PS_NSPEC = 12, PS_CTR = 13,
  PS_VCOUNT = 14,  // light paths: stored light vertices
  PS_PIX = 14,     // camera paths: film pixel
  PS_DVM = 15,     // VCM: dVM (vertexcm.h:36)
  PS_CVCOUNT = 15, // (unused: BDPT keeps its counters in BQ_PACK)
  PS_WORDS = 16
};
__device__ __forceinline__ float& psf(float* s, int p, int k) { return s[size_t(p) * PS_WORDS + k]; }
__device__ __forceinline__ int& psi(float* s, int p, int k) {
  return reinterpret_cast<int*>(s)[size_t(p) * PS_WORDS + k];
}
__device__ __forceinline__ uint32_t& psu(float* s, int p, int k) {
  return reinterpret_cast<uint32_t*>(s)[size_t(p) * PS_WORDS + k];
}
__device__ __forceinline__ V3 ld3r(const float* s, int p, int k) {
  const float* r = s + size_t(p) * PS_WORDS + k;
  return v3(r[0], r[1], r[2]);
}
__device__ __forceinline__ void st3r(float* s, int p, int k, V3 v) {
  float* r = s + size_t(p) * PS_WORDS + k;
  r[0] = v.x;
  r[1] = v.y;
  r[2] = v.z;
}

// BDPT's own subpath record (VertexCM keeps PS_*): 32 bytes per path, half a
// PS record.  The subpath's origin and direction are not kept: the reference
// overwrites both in sampleScattering before any read (bidirPathTracing.cpp:
// 381-400 -- bsdf.sample writes the direction, origin = hitPos), and the next
// ray travels in the extension queue.  The small counters share one word:
//   BQ_PACK = len | nspec << 8 | stored vertices << 16 (light: light vertices,
//   camera: camera vertices of the overlapped schedule)
enum : int { BQ_THR = 0, BQ_DVCM = 3, BQ_DVC = 4, BQ_CTR = 5, BQ_PACK = 6, BQ_PIX = 7, BQ_WORDS = 8 };
__device__ __forceinline__ float& bqf(float* s, int p, int k) { return s[size_t(p) * BQ_WORDS + k]; }
__device__ __forceinline__ int& bqi(float* s, int p, int k) {
  return reinterpret_cast<int*>(s)[size_t(p) * BQ_WORDS + k];
}
__device__ __forceinline__ uint32_t& bqu(float* s, int p, int k) {
  return reinterpret_cast<uint32_t*>(s)[size_t(p) * BQ_WORDS + k];
}
__device__ __forceinline__ V3 bqld3(const float* s, int p, int k) {
  const float* r = s + size_t(p) * BQ_WORDS + k;
  return v3(r[0], r[1], r[2]);
}
__device__ __forceinline__ void bqst3(float* s, int p, int k, V3 v) {
  float* r = s + size_t(p) * BQ_WORDS + k;
  r[0] = v.x;
  r[1] = v.y;
  r[2] = v.z;
}
// The record as its two 16-byte halves, a = (thr, dVCM), b = (dVC, ctr, pack,
// pix): a vertex reads it with two loads issued with its other inputs
// (vertex_inputs) and writes back the half or halves that changed.  A path's
// record is touched only by the thread shading that path's vertex (the other
// pass reads lvc / cvc), so whole-record stores race with nothing.
struct BqRec {
  float4 a, b;
};
__device__ __forceinline__ BqRec bq_load(const float* s, int p) {
  const float4* r = reinterpret_cast<const float4*>(s) + 2 * size_t(p);
  return BqRec{r[0], r[1]};
}
__device__ __forceinline__ float4 bq_half_a(V3 thr, float dvcm) { return make_float4(thr.x, thr.y, thr.z, dvcm); }
__device__ __forceinline__ float4 bq_half_b(float dvc, uint32_t ctr, int pack, int pix) {
  return make_float4(dvc, __uint_as_float(ctr), __int_as_float(pack), __int_as_float(pix));
}
__device__ __forceinline__ void bq_store_a(float* s, int p, float4 a) {
  reinterpret_cast<float4*>(s)[2 * size_t(p)] = a;
}
__device__ __forceinline__ void bq_store_b(float* s, int p, float4 b) {
  reinterpret_cast<float4*>(s)[2 * size_t(p) + 1] = b;
}
__device__ __forceinline__ int bq_pack(int len, int nspec, int cnt) { return len | (nspec << 8) | (cnt << 16); }
__device__ __forceinline__ int bq_len(int w) { return w & 255; }
__device__ __forceinline__ int bq_nspec(int w) { return (w >> 8) & 255; }
__device__ __forceinline__ int bq_count(int w) { return w >> 16; }
constexpr int kLightAlive = 0x80;  // BdptBuf::lvc

// BDPT's stored vertices (VertexCM keeps VS_*), light (B.vs) and camera (B.cv,
// overlapped schedule) alike: 64 bytes.  The geometric normal and the BSDF's
// probabilities are not stored: they are functions of the primitive (and, for
// a sphere, the position), the local wi and the material, and stored_bsdf
// rebuilds them with the operations the vertex itself ran (prim_normal,
// bsdf_probs), to the same floats.
// A record moves as four 16-byte words (BvRec): written whole by store_vertex,
// read whole once per slot before any field is looked at, and passed by value.
//   BV_PACK = len | nspec << 8; the material is a word of its own (BV_MAT:
//   emitters are -(light + 1), any face count)
enum : int { BV_POS = 0, BV_WI = 3, BV_THR = 6, BV_DVCM = 9, BV_DVC = 10, BV_PRIM = 11, BV_PACK = 12, BV_PIX = 13,
             BV_MAT = 14, BV_WORDS = 16 };
struct BvRec {
  float4 a, b, c, d;  // words 0-3, 4-7, 8-11, 12-15
};
__device__ __forceinline__ BvRec bv_load(const float* s, int i) {
  const float4* r = reinterpret_cast<const float4*>(s) + 4 * size_t(i);
  return BvRec{r[0], r[1], r[2], r[3]};
}
__device__ __forceinline__ V3 bv_pos(const BvRec& r) { return v3(r.a.x, r.a.y, r.a.z); }
__device__ __forceinline__ V3 bv_wi(const BvRec& r) { return v3(r.a.w, r.b.x, r.b.y); }
__device__ __forceinline__ V3 bv_thr(const BvRec& r) { return v3(r.b.z, r.b.w, r.c.x); }
__device__ __forceinline__ float bv_dvcm(const BvRec& r) { return r.c.y; }
__device__ __forceinline__ float bv_dvc(const BvRec& r) { return r.c.z; }
__device__ __forceinline__ int bv_prim(const BvRec& r) { return __float_as_int(r.c.w); }
__device__ __forceinline__ int bv_len(const BvRec& r) { return __float_as_int(r.d.x) & 255; }
__device__ __forceinline__ int bv_nspec(const BvRec& r) { return (__float_as_int(r.d.x) >> 8) & 255; }
__device__ __forceinline__ int bv_pix(const BvRec& r) { return __float_as_int(r.d.y); }
__device__ __forceinline__ int bv_mat(const BvRec& r) { return __float_as_int(r.d.z); }
// one stored vertex: position, local wi, throughput, dVCM, dVC, primitive,
// (len, nspec), the camera pixel and the material
__device__ __forceinline__ void store_vertex(float* s, int i, V3 pos, const Bsdf& b, V3 thr, float dvcm, float dvc,
                                             int prim, int len, int nspec, int pix) {
  float4* r = reinterpret_cast<float4*>(s) + 4 * size_t(i);
  r[0] = make_float4(pos.x, pos.y, pos.z, b.wi.x);
  r[1] = make_float4(b.wi.y, b.wi.z, thr.x, thr.y);
  r[2] = make_float4(thr.z, dvcm, dvc, __int_as_float(prim));
  r[3] = make_float4(__int_as_float(len | (nspec << 8)), __int_as_float(pix), __int_as_float(b.mat), 0.f);
}
// the BSDF of stored vertex v (BSDF::init at its hit, bsdf.h:66-89); the
// primitive's records are read together, the sphere word only in a scene
// that has a sphere
struct PrimIn {
  float4 r0, r1, cs;  // prim_rec's two words, prim_sph
};
__device__ __forceinline__ PrimIn prim_inputs(const DevScene& S, int has_sph, int prim) {
  PrimIn g;
  g.r0 = S.prim_rec[2 * static_cast<size_t>(prim)];
  g.r1 = S.prim_rec[2 * static_cast<size_t>(prim) + 1];
  g.cs = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has_sph) g.cs = S.prim_sph[prim];
  return g;
}
__device__ __forceinline__ Bsdf stored_bsdf(const PrimIn& g, const DMat* mats, const BvRec& v) {
  Bsdf b;
  b.fr = frame_from_z(prim_normal(g.r0, g.r1, g.cs, bv_pos(v)));
  b.wi = bv_wi(v);
  bsdf_probs(b, bv_mat(v), mats);
  return b;
}

// Stored light vertices (lightStates, bidirPathTracing.cpp:101-102), one
// 80-byte record per vertex slot k * P + p: the camera pass reads a path's
// vertices by path index (connectVertices, :219-257).
enum : int {
  VS_POS = 0, VS_N = 3, VS_WI = 6, VS_THR = 9, VS_DVCM = 12, VS_DVC = 13, VS_CONT = 14, VS_PD = 15, VS_PG = 16,
  VS_LEN = 17, VS_NSPEC = 18, VS_MAT = 19, VS_WORDS = 20
};
__device__ __forceinline__ float& vsf(float* s, int i, int k) { return s[size_t(i) * VS_WORDS + k]; }
__device__ __forceinline__ int& vsi(float* s, int i, int k) {
  return reinterpret_cast<int*>(s)[size_t(i) * VS_WORDS + k];
}
__device__ __forceinline__ V3 vld3(const float* s, int i, int k) {
  const float* r = s + size_t(i) * VS_WORDS + k;
  return v3(r[0], r[1], r[2]);
}
__device__ __forceinline__ void vst3(float* s, int i, int k, V3 v) {
  float* r = s + size_t(i) * VS_WORDS + k;
  r[0] = v.x;
  r[1] = v.y;
  r[2] = v.z;
}

// A camera vertex's direct-illumination record (getDirectIllumination,
// :484-608), one 64-byte record per path, finalised by its last resolved ray
enum : int {
  DR_NEE = 0, DR_NEEW = 3, DR_BSDF = 4, DR_THR = 7, DR_WLEN = 10, DR_FLAGS = 11, DR_LIGHT = 12, DR_PIX = 13,
  DR_STATE = 14, DR_WORDS = 16
};
__device__ __forceinline__ float& drf(float* s, int p, int k) { return s[size_t(p) * DR_WORDS + k]; }
__device__ __forceinline__ int& dri(float* s, int p, int k) {
  return reinterpret_cast<int*>(s)[size_t(p) * DR_WORDS + k];
}
__device__ __forceinline__ V3 drld3(const float* s, int p, int k) {
  const float* r = s + size_t(p) * DR_WORDS + k;
  return v3(r[0], r[1], r[2]);
}
__device__ __forceinline__ void drst3(float* s, int p, int k, V3 v) {
  float* r = s + size_t(p) * DR_WORDS + k;
  r[0] = v.x;
  r[1] = v.y;
  r[2] = v.z;
}

// Stored camera vertices of the overlapped schedule (BV_* records, slot
// j * P + p, j < kCvMax): what connectVertices (:610-665) reads of the camera
// side when a later light vertex of the path makes the connection.  Only
// vertices with length <= (maxlen - 2) / 2 can meet a later light vertex
// (c < l and l + 1 + c <= maxlen), so kCvMax = 4 slots for maxlen <= 10.
constexpr int kCvMax = (kVMax + 1 - 2) / 2;

struct BdptBuf {
  int P = 0, cap_sq = 0;
  float *ls, *cs;  // light / camera subpath state: BDPT BQ_WORDS, VertexCM PS_WORDS floats per path
  float* vs;       // stored light vertices: BDPT BV_WORDS, VertexCM VS_WORDS floats per record
                   // (sequential schedule: record k * P + p)
  float* cv;       // overlapped schedule: stored camera vertices, BV_WORDS floats per record
  // BDPT: stored light / camera vertices per path, one byte each -- what each
  // pass reads of the other's subpath (2 MB per 2M paths: L2-resident, where a
  // read of the other pass's record would be a line from HBM per vertex).
  // lvc's kLightAlive bit: the light subpath has an extension ray (a light
  // vertex of a greater length may still come)
  uint8_t *lvc, *cvc;
  // Overlapped schedule: the vertex stores are pools, sized by use rather than
  // by the worst case (the reference pushes only the vertices a path makes,
  // bidirPathTracing.cpp:101-102): vertex k of path p is record vidx[k * P +
  // p] of vs (cidx for cv), taken from the step counters' vpool / cpool; -1
  // when the pool was full.  A full pool or shadow queue sets the render's
  // overflow counter and the host renders again with pieces the worst case
  // fits (wr_render.hip, render_bdpt_one).  Null: records k * P + p.
  int* vidx;
  int* cidx;
  int vcap = 0, ccap = 0;
  // extension-ray queues (double buffered, SoA with stride qs).  Overlapped
  // schedule: the light pass's rays of a bounce first (count ext[b]), the
  // camera pass's behind them (count ext[kCamSlot + b]).
  // qs: the plane stride of the ray arrays the traversal reads, q_o / q_d and
  // in BDPT sq[].o / sq[].d as well: there they and q_t, q_prim, sq[].t,
  // sq[].prim are segments of the pipeline's ray slab (wr_queue_slab.h) and qs
  // is the slab's entries.  VertexCM: arrays of the set's own, qs = P, and
  // sq[].o / sq[].d keep the stride cap_sq
  int qs = 0;
  float *q_o[2], *q_d[2], *q_t[2];
  int *q_path[2], *q_prim[2];
  // shadow + aux closest-hit queue (splat / connection / NEE / DI-BSDF)
  // shadow / aux queue and DI records, two each: the ones of step `slot` are
  // [slot & 1], so a step's resolve and the next step's vertex shading (which
  // writes [(slot + 1) & 1]) can run in one launch
  struct Sq {
    float *o, *d, *tgt, *val, *t, *cut;  // cut: occl_cut (-INF for closest-hit DI-BSDF rays)
    int *meta, *pix, *prim;
  } sq[2];
  struct Di {
    float* r;  // DR_WORDS floats per path (DR_*); DR_STATE: rays still to resolve | DI_VIS | DI_SAME
  } di[2];
  // direct-illumination records (getDirectIllumination, :484-608)
};

struct BdptArgs {
  DevScene S;
  BdptBuf B;
  DevCounters* ctr;
  StepCounters* sc;  // this iteration's queue counters
  float* film;
  int W, H, P;     // film; P = W * H = lightPathNum (MIS, :55) -- global, whatever the piece
  int base, n;     // this piece of the iteration: global paths [base, base + n); buffers hold
                   // them at local index l = p - base (stride B.P >= n)
  uint32_t seed, iter;
  int ctl, maxlen, faithful;
  int overlap = 0;  // 1: the overlapped schedule (light splats into the step's sq, CV store, light-side connections)
  int untiled = 0;  // 1: camera paths in plain path order (a render redone with small pieces, BdptBuf)
  int nmats = 0;    // entries of S.mats (material 0 is unused)
  int has_sph = 0;  // the scene has a sphere: prim_sph is worth a load (else prim_rec's type word is 0 everywhere)
};
// First queue index of the camera pass's extension rays of step `slot`
// (kCamSlot + bounce): overlapped, behind the light pass's rays of the same
// bounce, whose count is final once the step's light kernel has run
__device__ __forceinline__ int cam_ext_base(const BdptArgs& A, int slot) {
  return A.overlap ? A.sc->ext[slot - kCamSlot] : 0;
}
struct BdptGroup {
  BdptArgs a[kGroup];
};

__device__ __forceinline__ bool len_ok(int ctl, int L) { return ctl <= 0 || L == ctl; }

// record of stored light vertex k / camera vertex j of path p (-1: the pool was full)
__device__ __forceinline__ int lv_slot(const BdptBuf& B, int k, int p) {
  return B.vidx ? B.vidx[size_t(k) * B.P + p] : k * B.P + p;
}
__device__ __forceinline__ int cv_slot(const BdptBuf& B, int j, int p) {
  return B.cidx ? B.cidx[size_t(j) * B.P + p] : j * B.P + p;
}
// A pool record for this lane (called by the lanes that store, together:
// one atomic per wave); -1 and the overflow counter when the pool is full
__device__ __forceinline__ int pool_take(const BdptArgs& A, int* counter, int cap) {
  const int i = wave_append(counter, true);
  if (i < cap) return i;
  atomicAdd(&A.ctr->overflow, 1ull);
  return -1;
}
// a shadow / aux queue slot from wave_append: within the queue, or the overflow counter
__device__ __forceinline__ bool sq_fits(const BdptArgs& A, bool want, int si) {
  if (!want) return false;
  if (si < A.B.cap_sq) return true;
  atomicAdd(&A.ctr->overflow, 1ull);
  return false;
}
// Numerators of three MIS weights -- connectVertices (:658-664),
// getDirectIllumination's outer weight (:529) and connectToCamera's (:360):
// 1 in every product build.  scripts/perturbation_check.sh builds variants
// with 1.001 to show that the film parity gates (tests/_parity.py) catch a
// 1e-3 error in any of them.
#ifndef WR_TEST_CONN_W
#define WR_TEST_CONN_W 1.f
#endif
#ifndef WR_TEST_DI_W
#define WR_TEST_DI_W 1.f
#endif
#ifndef WR_TEST_SPLAT_W
#define WR_TEST_SPLAT_W 1.f
#endif

// The material and light tables in LDS (the gen and vertex kernels' template
// flag GT = false; GT = true reads the global tables; chosen by the host per
// scene: bdpt_lds_tables): every BSDF
// call reads its DMat, and a global read there is a round trip behind the
// material index that the compiler repeats after each store (it cannot know
// the table is not written).  A scene above either cap keeps the global
// tables.  The choice is a template flag, not a run-time select, so that the
// pointers' address space is known where they are used.
constexpr int kLdsMats = 32, kLdsLights = 16;
constexpr int kMatWords = sizeof(DMat) / 4, kLightWords = sizeof(DLight) / 4;
constexpr int kLdsTabWords = kLdsMats * kMatWords + kLdsLights * kLightWords;  // 2.8 KB
static_assert(sizeof(DMat) % 4 == 0 && sizeof(DLight) % 4 == 0, "tables are copied by words");
// every thread of the block calls it, before any thread leaves the kernel
__device__ __forceinline__ void tables_to_lds(const BdptArgs& A, float* tab) {
  const float* gm = reinterpret_cast<const float*>(A.S.mats);
  const float* gl = reinterpret_cast<const float*>(A.S.lights);
  const int nm = min(A.nmats, kLdsMats) * kMatWords, nl = min(A.S.nlights, kLdsLights) * kLightWords;
  for (int i = threadIdx.x; i < nm; i += blockDim.x) tab[i] = gm[i];
  for (int i = threadIdx.x; i < nl; i += blockDim.x) tab[kLdsMats * kMatWords + i] = gl[i];
  __syncthreads();
}
#define WR_BDPT_TABLES(A_)                                                         \
  __shared__ float s_tab_[GT ? 1 : kLdsTabWords];                                  \
  const DMat* mats = (A_).S.mats;                                                  \
  const DLight* lights = (A_).S.lights;                                            \
  if constexpr (!GT) {                                                             \
    tables_to_lds(A_, s_tab_);                                                     \
    mats = reinterpret_cast<const DMat*>(s_tab_);                                  \
    lights = reinterpret_cast<const DLight*>(s_tab_ + kLdsMats * kMatWords);       \
  }

// generateLightSample (:267-311) + the first extension ray
template <bool GT>
__global__ void __launch_bounds__(kShadeBlock) WR_NO_PK_FP32 k_light_gen(BdptGroup G_) {
  const BdptArgs& A = G_.a[blockIdx.y];
  const BdptBuf& B = A.B;
  WR_BDPT_TABLES(A)
  (void)mats;
  // (queues use the stride B.qs)
  const float lpp = 1.f / static_cast<float>(A.S.nlights);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += gridDim.x * blockDim.x) {
    // local index p, global light path A.base + p (the RNG key pairs it with
    // the camera path of the same global index, :130, :222-229)
    Rng rng{stream_key(A.seed, A.iter, 0, static_cast<uint32_t>(A.base + p)), 0};
    const int id = min(static_cast<int>(rng.f() * static_cast<float>(A.S.nlights)), A.S.nlights - 1);
    const DLight L = lights[id];
    V3 pos, dir, rad;
    float epdf = 0.f, dpdf = 0.f;
    for (int tries = 0; tries < 64; ++tries) {
      // emit(..., rng.randVector3(), rng.randVector3(), ...): the reference's
      // compiler evaluates the second argument (posRand3) first
      V3 pr = rng.v();
      V3 dr = rng.v();
      rad = light_emit(L, dr, pr, &pos, &dir, &epdf, &dpdf);
      if (epdf > 1e-7f) break;
    }
    V3 thr = rad;
    epdf *= lpp;
    dpdf *= lpp;
    thr = div_plain(thr, epdf);
    // dVC = 1 / epdf: AreaLight::isDelta() == 0; pathLength 1, no specular
    // vertex, no stored vertex (a light path has no pixel: the last word is 0)
    bq_store_a(B.ls, p, bq_half_a(thr, dpdf / epdf));
    bq_store_b(B.ls, p, bq_half_b(1.f / epdf, rng.ctr, bq_pack(1, 0, 0), 0));
    B.lvc[p] = kLightAlive;  // no stored vertex, the first ray queued
    // Ray(origin + dir * EPS, dir) (:79-80)
    st3(B.q_o[0], B.qs, p, pos + dir * WR_EPS);
    st3(B.q_d[0], B.qs, p, normalize(dir));
    B.q_path[0][p] = p;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) A.sc->ext[0] = A.n;
}

// sampleScattering (:370-416).  Returns false when the subpath ends.
__device__ __forceinline__ bool sample_scatter(const DMat* mats, Rng& rng, const Bsdf& b, V3 hit, V3& o, V3& dir,
                                               V3& thr, float& dvcm, float& dvc, int& nspec) {
  float dpdf = 0.f, cos_wo = 0.f;
  int type;
  V3 wo = dir;
  const V3 f = bsdf_sample(b, mats, rng.v(), &wo, &dpdf, &cos_wo, &type);
  if (black(f)) return false;
  dir = wo;
  float rpdf = dpdf;
  if ((type & T_SPEC) == 0) rpdf = bsdf_pdf(b, mats, dir, true);
  const float cp = b.cont;
  if (rng.f() > cp) return false;
  dpdf *= cp;
  rpdf *= cp;
  if (type & T_SPEC) {
    ++nspec;
    dvcm = 0.f;
    dvc *= cos_wo;
  } else {
    dvc = (1.f / dpdf) * (dvcm + dvc * rpdf);
    dvcm = 1.f / dpdf;
  }
  o = hit;
  thr = mul(thr, f) * (cos_wo / dpdf);
  return true;
}

// connectVertices (:610-665) for one (camera vertex, stored light vertex)
// pair of path p: the camera vertex's BSDF b at hp with its state (cthr,
// cdvcm, cdvc, cnspec, length len) and light-vertex slot `slot` of length
// llen.  True when the shadow ray is cast (its contribution counts, or every
// ray is traced: faithful); sdir / stgt / sval then hold the ray and the value
// splatted if unoccluded.  One function for both sides of the overlapped
// schedule, so a pair's floats do not depend on which vertex came second.
__device__ __forceinline__ bool connect_pair(const BdptArgs& A, const DMat* mats, const Bsdf& b, V3 hp, V3 cthr,
                                             float cdvcm, float cdvc, int cnspec, int len, const BvRec& lv, int llen,
                                             V3& sdir, V3& stgt, V3& sval, bool& counted) {
  const DevScene& S = A.S;
  bool shoot = false;
  const PrimIn lg = prim_inputs(S, A.has_sph, bv_prim(lv));  // (asked for now, used once the camera side's f is known)
  const V3 lpos = bv_pos(lv);
  V3 dir = lpos - hp;
  const float d2 = sqr_len(dir);
  const float dist = sqrtf(d2);
  dir = div_guarded(dir, dist);
  float cos_c = 0.f, cdp, crp;
  const V3 cf = bsdf_f(b, mats, dir, &cos_c, &cdp, &crp);
  if (!black(cf)) {
    cdp *= b.cont;
    crp *= b.cont;
    const Bsdf lb = stored_bsdf(lg, mats, lv);
    float cos_l = 0.f, ldp, lrp;
    const V3 lf = bsdf_f(lb, mats, -dir, &cos_l, &ldp, &lrp);
    if (!black(lf)) {
      ldp *= lb.cont;
      lrp *= lb.cont;
      const float G = cos_l * cos_c / d2;
      if (!(cmpf(G) < 0)) {
        const float cdpa = cdp * fabsf(cos_l) / (dist * dist);
        const float ldpa = ldp * fabsf(cos_c) / (dist * dist);
        const V3 res = mul(cf, lf) * G;
        if (!black(res)) {
          const float wl = cdpa * (bv_dvcm(lv) + lrp * bv_dvc(lv));
          const float wc = ldpa * (cdvcm + crp * cdvc);
          const float w = WR_TEST_CONN_W / (wl + 1.f + wc);
          const bool counts = len_ok(A.ctl, llen + 1 + len);
          counted = counts;
          if (counts || A.faithful) {
            shoot = true;
            sdir = normalize(dir);
            stgt = hp + dir * dist;
            if (counts) {
              const float wlen = 1.f / (static_cast<float>(llen) + 1.f + static_cast<float>(len) -
                                        static_cast<float>(bv_nspec(lv)) - static_cast<float>(cnspec));
              const V3 lthr = bv_thr(lv);
              sval = mul(mul(cthr, lthr), res * w) * wlen;
            }
          }
        }
      }
    }
  }
  return shoot;
}

// queue a connection's shadow ray (every lane of the wave calls it)
// A connection whose path length the control-length filter drops (:252-253)
// is still traced (faithful ray set, :244) but its outcome is never used: its
// entry carries the ray and kSqNoValue only (no target, value or pixel).
constexpr int kSqNoValue = 1 << 29;  // Sq meta: kind << 30 | kSqNoValue? | local path (< 2^29)
__device__ __forceinline__ void queue_connection(const BdptArgs& A, int qslot, bool shoot, bool counted, int p, int pix,
                                                 V3 hp, V3 sdir, V3 stgt, V3 sval) {
  const BdptBuf& B = A.B;
  const BdptBuf::Sq& Q = B.sq[qslot & 1];
  const int cap = B.cap_sq;
  const int si = wave_append(&A.sc->sq[qslot], shoot);
  if (sq_fits(A, shoot, si)) {
    st3(Q.o, B.qs, si, hp);  // (o, d: segments of the ray slab, plane stride qs)
    st3(Q.d, B.qs, si, sdir);
    Q.cut[si] = occl_cut(hp, stgt, dot(stgt - hp, sdir));
    if (counted) {
      st3(Q.tgt, cap, si, stgt);
      st3(Q.val, cap, si, sval);
      Q.meta[si] = (SQ_CONN << 30) | p;
      Q.pix[si] = pix;
    } else {
      Q.meta[si] = (SQ_CONN << 30) | kSqNoValue | p;
    }
  }
}

// A vertex's inputs, read in two stages instead of one load behind another.
// Stage A (the callers): the ray's queue columns, all together.  Stage B
// (vertex_inputs): everything whose address follows from the path and the
// primitive -- the primitive's records, the path's state record and the other
// pass's vertex count -- issued as one straight-line block before any of it
// is used.  A lane without work (a spare lane of the hit list's last wave)
// reads a valid record and drops it, so no branch guards a load.
struct VtxIn {
  int p, prim;  // p = -1: the lane has no entry of the hit list
  float t;
  V3 o, d;
  PrimIn g;
  BqRec st;
  int oc;  // light vertex: cvc[p] (overlapped schedule), camera vertex: lvc[p]
};
// p: a valid local path for every lane (the callers clamp the queue index);
// on: the lane has a queue entry
template <bool CAMERA>
__device__ __forceinline__ VtxIn vertex_inputs(const BdptArgs& A, bool on, int p, int prim, float t, V3 o, V3 d) {
  const BdptBuf& B = A.B;
  VtxIn v;
  v.g = prim_inputs(A.S, A.has_sph, max(prim, 0));
  v.st = bq_load(CAMERA ? B.cs : B.ls, p);
  v.oc = CAMERA ? B.lvc[p] : (A.overlap ? B.cvc[p] : 0);
  v.p = on ? p : -1;
  v.prim = on ? prim : -1;
  v.t = t;
  v.o = o;
  v.d = d;
  return v;
}

// Hit compaction.  A vertex kernel shades only the queue entries whose ray hit
// something (prim >= 0), in full waves: a missed entry has no vertex, and a
// lane that carries one idles through the whole vertex of its wave.  A block
// takes a chunk of kShadeBlock x R consecutive entries (R: hit_chunk_r, uniform
// per launch), reads their q_prim column -- R independent coalesced loads per
// thread -- and lists in LDS, in queue order, the chunk offsets of the entries
// that hit: a ballot per 64-entry segment, the segment counts through LDS.
// The block then runs stage A and the vertex over the list, kShadeBlock entries
// per round; only the list's last wave is partial.
constexpr int kHitR = 4;  // entries per thread and chunk, at most
constexpr int kHitSegs = kHitR * (kShadeBlock / 64);
static_assert(kShadeBlock * kHitR <= 65536 && kHitSegs % 4 == 0, "16-bit offsets; counts read as int4");
struct HitList {
  alignas(16) int seg[kHitSegs];       // hits per segment; segment r * (kShadeBlock / 64) + wave
  uint16_t at[kShadeBlock * kHitR];    // chunk offsets of the entries that hit, in queue order
};
// R of a launch over n entries by nblk blocks: 1 while the launch has a block
// per kShadeBlock entries (a small launch spreads over as many blocks as
// before), up to kHitR where the blocks loop anyway
__device__ __forceinline__ int hit_chunk_r(int n, int nblk) {
  const int lanes = nblk * kShadeBlock;
  int r = 1;
#pragma unroll
  for (int k = 1; k < kHitR; ++k) r += n > k * lanes ? 1 : 0;  // min(kHitR, ceil(n / lanes)) without the division
  return r;
}
// Lists the hits among entries [e0, e0 + cn) of the queue (cn <= kShadeBlock *
// R) and returns their number.  Every thread of the block calls it (two
// barriers); the list stays valid until the block's next call.  The barriers
// order the reuse: seg is read only between them, and `at` is written only
// after the first, which no wave passes before every wave has left the
// previous chunk's rounds.
// LIGHT: a missed entry ends its light subpath (:81-82), so its path's lvc
// byte loses kLightAlive here -- q_path, then the byte.  (The byte's low bits
// are always the stored-vertex count, so the state record is not read; the
// thread owns the path for the launch.)
template <bool LIGHT>
__device__ __forceinline__ int compact_hits(HitList& L, const int* q_prim, const int* q_path, uint8_t* lvc, int tid,
                                            int e0, int cn, int R) {
  const int lane = tid & 63, w = tid >> 6;
  constexpr int kW = kShadeBlock / 64;
  int prim[kHitR], mp[kHitR];  // mp: the path of a missed entry (LIGHT), else -1
  bool in[kHitR];
  unsigned long long m[kHitR];
#pragma unroll
  for (int r = 0; r < kHitR; ++r) {
    const int k = r * kShadeBlock + tid;
    in[r] = r < R && k < cn;
    prim[r] = in[r] ? q_prim[e0 + k] : -1;
  }
#pragma unroll
  for (int r = 0; r < kHitR; ++r) {
    m[r] = __ballot(prim[r] >= 0);
    if (lane == 0) L.seg[r * kW + w] = __popcll(m[r]);  // (0 for r >= R)
    mp[r] = (LIGHT && in[r] && prim[r] < 0) ? q_path[e0 + r * kShadeBlock + tid] : -1;
  }
  __syncthreads();
  int cnt[kHitSegs];
#pragma unroll
  for (int i = 0; i < kHitSegs / 4; ++i) {
    const int4 v = reinterpret_cast<const int4*>(L.seg)[i];
    cnt[4 * i] = v.x;
    cnt[4 * i + 1] = v.y;
    cnt[4 * i + 2] = v.z;
    cnt[4 * i + 3] = v.w;
  }
  int mb[kHitR];
  if (LIGHT) {
#pragma unroll
    for (int r = 0; r < kHitR; ++r) mb[r] = mp[r] >= 0 ? lvc[mp[r]] : 0;
  }
  int base[kHitR], total = 0;
#pragma unroll
  for (int i = 0; i < kHitSegs; ++i) {
    if ((i % kW) == w) base[i / kW] = total;
    total += cnt[i];
  }
#pragma unroll
  for (int r = 0; r < kHitR; ++r)
    if (prim[r] >= 0)
      L.at[base[r] + __popcll(m[r] & ((1ull << lane) - 1ull))] = static_cast<uint16_t>(r * kShadeBlock + tid);
  if (LIGHT) {
#pragma unroll
    for (int r = 0; r < kHitR; ++r)
      if (mp[r] >= 0) lvc[mp[r]] = static_cast<uint8_t>(mb[r] & ~kLightAlive);
  }
  __syncthreads();
  return total;
}

// One light-subpath vertex (:77-128): path p's ray (o, d) hit prim at t.  A
// missed entry never comes here (compact_hits ends its subpath); prim < 0 is
// a spare lane of the list's last wave.  Every lane of the wave calls it
// (queue appends).  oslot: the step whose queue gets the extension ray
// (slot + 1).
__device__ __forceinline__ void light_vertex(const BdptArgs& A, const DMat* mats, const VtxIn& in, int oslot) {
  const BdptBuf& B = A.B;
  const DevScene& S = A.S;
  const int P = B.P, nxt = oslot & 1;  // P: buffer stride (local paths)
  const int p = in.p, prim = in.prim;
  const float t = in.t;
  const V3 d = in.d;
  bool ext = false, splat = false;
  V3 e_o, e_d, s_o, s_d, s_val;
  int s_pix = -1;
  int lconn = 0, lslot = -1, llen = 0;  // overlapped: the stored vertex's slot, camera vertices to connect
  const int pk = __float_as_int(in.st.b.z);
  if (prim >= 0) {
    const Hit h = rebuild_hit(S, prim, t, in.o, d, in.g.r0, in.g.r1, in.g.cs);
    Bsdf b;
    bsdf_init(b, -d, h.n, h.mat, mats);
    if (b.mat != 0) {
      float dvcm = in.st.a.w, dvc = in.st.b.x;
      int len = bq_len(pk), nspec = bq_nspec(pk), nstored = bq_count(pk);
      V3 thr = v3(in.st.a.x, in.st.a.y, in.st.a.z);
      dvcm *= (t * t);  // pathLength > 1 || isFiniteLight: always for area lights (:94-97)
      dvcm /= fabsf(b.wi.z);
      dvc /= fabsf(b.wi.z);
      if (!b.delta) {  // lightStates.push_back (:101-102)
        const int k = nstored;
        int slot = k * P + p;
        if (B.vidx) {  // a pool record (the storing lanes of the wave take theirs together)
          slot = pool_take(A, &A.sc->vpool, B.vcap);
          B.vidx[size_t(k) * P + p] = slot;
        }
        if (slot >= 0) store_vertex(B.vs, slot, h.p, b, thr, dvcm, dvc, prim, len, nspec, -1);
        nstored = k + 1;
        if (A.overlap && slot >= 0) {  // the camera vertices stored at earlier steps (lengths < len)
          lslot = slot;
          llen = len;
          lconn = in.oc;
        }
        if (len_ok(A.ctl, len + 1)) {  // connectToCamera (:105-120, :313-368)
          const DCam& cam = S.cam;
          const V3 ip = t_point(cam.w2r, h.p);
          if (check_raster(cam, ip.x, ip.y)) {
            V3 dtc = cam.pos - h.p;
            if (dot(-dtc, cam.fwd) > 0) {
              const float d2 = sqr_len(dtc);
              const float dist = sqrtf(d2);
              dtc = div_guarded(dtc, dist);
              float cos_to = 0.f, dp, rp;
              const V3 f = bsdf_f(b, mats, dtc, &cos_to, &dp, &rp);
              if (!black(f)) {
                rp *= b.cont;
                const float cos_at = dot(-dtc, cam.fwd);
                const float ipd = cam.plane_dist / cos_at;
                const float i2sa = (ipd * ipd) / cos_at;
                const float i2s = i2sa * fabsf(cos_to) / d2;
                const float pdf_a = i2s;
                const float s2i = 1.f / i2s;
                const V3 res = div_plain(mul(thr, f), static_cast<float>(A.P) * s2i);
#ifdef WR_DEBUG_PATH
                if (A.base + p == WR_DEBUG_PATH && A.iter == WR_DEBUG_ITER)
                  printf("[dbg gpu] len %d hit %a %a %a t %a prim %d thr %a %a %a f %a %a %a cos_to %a d2 %a i2s %a res %a %a %a black %d rp %a dvcm %a dvc %a\n",
                         len, h.p.x, h.p.y, h.p.z, t, prim, thr.x, thr.y, thr.z, f.x, f.y, f.z, cos_to, d2, i2s,
                         res.x, res.y, res.z, (int)black(res), rp, dvcm, dvc);
#endif
                if (!black(res)) {
                  const float wl = (pdf_a / static_cast<float>(A.P)) * (dvcm + rp * dvc);
                  const float w = WR_TEST_SPLAT_W / (wl + 1.f);
                  splat = true;
                  s_o = h.p;
                  s_d = normalize(dtc);  // occluded() -> Ray(p1, dir)
                  s_val = res * w;
                  s_pix = pix_index(static_cast<int>(ip.x), static_cast<int>(ip.y), A.H, A.W);
                } else {
                  // an EPS-black res is returned before the shadow test and the
                  // MIS weight (:354-355), and the caller adds it (:116-118)
                  film_add(A.film, pix_index(static_cast<int>(ip.x), static_cast<int>(ip.y), A.H, A.W), res);
                }
              }
            }
          }
        }
      }
      if (!(len + 2 > A.maxlen)) {  // (:123-127)
        Rng rng{stream_key(A.seed, A.iter, 0, static_cast<uint32_t>(A.base + p)), __float_as_uint(in.st.b.y)};
        V3 lo{}, ld{};  // sampleScattering's origin and direction (outputs only)
        if (sample_scatter(mats, rng, b, h.p, lo, ld, thr, dvcm, dvc, nspec)) {
          ext = true;
          ++len;
          e_o = lo + ld * WR_EPS;
          e_d = normalize(ld);
        }
        // The record goes back as whole 16-byte halves.  A scattered path: all
        // of it -- thr, dVCM, dVC, len / nspec of the next vertex.  Otherwise
        // only the half with the counter and the stored vertices (dVC and the
        // last word as they were read).
        if (ext) {
          bq_store_a(B.ls, p, bq_half_a(thr, dvcm));
          bq_store_b(B.ls, p, bq_half_b(dvc, rng.ctr, bq_pack(len, nspec, nstored), __float_as_int(in.st.b.w)));
        } else {
          bq_store_b(B.ls, p, bq_half_b(in.st.b.x, rng.ctr, bq_pack(len, nspec, nstored), __float_as_int(in.st.b.w)));
        }
      } else if (nstored != bq_count(pk)) {
        bq_store_b(B.ls, p, make_float4(in.st.b.x, in.st.b.y, __int_as_float(bq_pack(len, nspec, nstored)), in.st.b.w));
      }
      const int lv = nstored | (ext ? kLightAlive : 0);
      if (lv != (bq_count(pk) | kLightAlive)) B.lvc[p] = static_cast<uint8_t>(lv);
    } else {  // an invalid BSDF ends the subpath (:86-88)
      B.lvc[p] = static_cast<uint8_t>(bq_count(pk));
    }
  }
  const int ei = wave_append(&A.sc->ext[oslot], ext);
  if (ext) {
    st3(B.q_o[nxt], B.qs, ei, e_o);
    st3(B.q_d[nxt], B.qs, ei, e_d);
    B.q_path[nxt][ei] = p;
  }
  // sequential schedule: traced with the camera primaries; overlapped: with
  // the next step's extension rays, like the camera vertices' rays
  const int sslot = A.overlap ? kCamSlot + oslot : kCamSlot;
  const int si = wave_append(&A.sc->sq[sslot], splat);
  if (sq_fits(A, splat, si)) {
    const BdptBuf::Sq& Q = B.sq[sslot & 1];
    st3(Q.o, B.qs, si, s_o);
    st3(Q.d, B.qs, si, s_d);
    st3(Q.tgt, B.cap_sq, si, S.cam.pos);
    st3(Q.val, B.cap_sq, si, s_val);
    Q.cut[si] = occl_cut(s_o, S.cam.pos, dot(S.cam.pos - s_o, s_d));
    Q.meta[si] = (SQ_SPLAT << 30) | p;  // (the local path: diagnostics only)
    Q.pix[si] = s_pix;
  }
  // overlapped schedule: this light vertex connects to the path's camera
  // vertices stored at earlier steps (:219-257 reached from the camera side)
  if (A.overlap && __ballot(lconn > 0)) {
    BvRec lv{};  // this light vertex as stored (lconn > 0: it has a record)
    if (lconn > 0) lv = bv_load(B.vs, lslot);
    for (int j = 0; __ballot(j < lconn); ++j) {
      bool shoot = false, counted = false;
      int pix = -1;
      V3 hp{}, sdir{}, stgt{}, sval{};
      const int cs = j < lconn ? cv_slot(B, j, p) : -1;
      if (cs >= 0) {
        const BvRec cv = bv_load(B.cv, cs);
        const int clen = bv_len(cv);
        if (llen + 1 + clen > A.maxlen) {
          lconn = j;  // camera vertices are stored by increasing length
        } else {
          const Bsdf cb = stored_bsdf(prim_inputs(S, A.has_sph, bv_prim(cv)), mats, cv);
          hp = bv_pos(cv);
          pix = bv_pix(cv);
          shoot = connect_pair(A, mats, cb, hp, bv_thr(cv), bv_dvcm(cv), bv_dvc(cv), bv_nspec(cv), clen, lv, llen, sdir,
                               stgt, sval, counted);
        }
      }
      queue_connection(A, sslot, shoot, counted, p, pix, hp, sdir, stgt, sval);
    }
  }
}

template <bool GT>
__global__ void __launch_bounds__(kShadeBlock) WR_SHADE_OCC k_light_shade(BdptGroup G_, int slot) {
  const BdptArgs& A = G_.a[blockIdx.y];
  WR_BDPT_TABLES(A)
  (void)lights;
  const BdptBuf& B = A.B;
  const int cur = slot & 1;
  const int n = A.sc->ext[slot];
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&A.ctr->closest, (unsigned long long)n);
  __shared__ HitList s_hits;
  const int R = hit_chunk_r(n, gridDim.x), chunk = R * kShadeBlock;
  // (i: the thread's index, then its place in the list -- the thread index
  // again modulo kShadeBlock, so the vertex keeps one lane counter)
  int i = threadIdx.x;
  for (int c0 = blockIdx.x * chunk; c0 < n; c0 += gridDim.x * chunk) {  // (block-uniform: every thread reaches the barriers)
    i &= kShadeBlock - 1;
    const int nh = compact_hits<true>(s_hits, B.q_prim[cur], B.q_path[cur], B.lvc, i, c0, min(chunk, n - c0), R);
    // whole waves reach the appends: the list's last wave runs with its spare lanes off
    for (; (i & ~63) < nh; i += kShadeBlock) {
      // stage A: the entry's columns, all at once (a spare lane reads the
      // list's last entry)
      const int e = c0 + s_hits.at[min(i, nh - 1)];
      const int p = B.q_path[cur][e], prim = B.q_prim[cur][e];
      const float t = B.q_t[cur][e];
      const V3 o = ld3(B.q_o[cur], B.qs, e), d = ld3(B.q_d[cur], B.qs, e);
#ifdef WR_DEBUG_PATH
      if (i < nh && A.base + p == WR_DEBUG_PATH && A.iter == WR_DEBUG_ITER)
        printf("[dbg gpu] light step %d ray o %a %a %a d %a %a %a prim %d t %a\n", slot, o.x, o.y, o.z, d.x, d.y, d.z,
               prim, t);
#endif
      light_vertex(A, mats, vertex_inputs<false>(A, i < nh, p, prim, t, o, d), slot + 1);
    }
  }
}

// generateCameraSample (:418-452) + first extension ray, for queue entry s of
// the piece; returns the path's local index.  (VertexCM::generateCameraSample,
// vertexcm.cpp:446-479, is the same plus dVM = 0.)
template <bool VCM = false>
__device__ __forceinline__ int camera_gen_one(const BdptArgs& A, int s, int ebase = 0) {
  const BdptBuf& B = A.B;
  const DCam& cam = A.S.cam;
  // (queues use the stride B.qs)
  // queue order: 8x8 raster tiles per wave (coherent primary rays); the
  // path <-> pixel mapping stays the reference's (x = p / W, y = p % W, :422-423).
  // A tiled piece is whole 8-row bands (base and n multiples of 8 W), so the
  // tiles are the piece's own.
  const bool tiled = !A.untiled && (A.W % 8) == 0 && (A.H % 8) == 0;
  const int tiles_y = A.W / 8;
  int l;
  if (tiled) {
    const int t = s >> 6, w = s & 63;
    l = ((t / tiles_y) * 8 + (w >> 3)) * A.W + (t % tiles_y) * 8 + (w & 7);
  } else {
    l = s;
  }
  const int p = A.base + l;
  const int x = p / A.W, y = p % A.W;
  Rng rng{stream_key(A.seed, A.iter, 1, static_cast<uint32_t>(p)), 0};
  const V3 jit = rng.v();
  const float sx = static_cast<float>(x) + jit.x, sy = static_cast<float>(y) + jit.y;
  const V3 rp = t_point(cam.r2w, v3(sx, sy, 0.f));
  const V3 d = normalize(rp - cam.pos);  // Ray(pos, p - pos) (camera.cpp:37-42)
  const float cos_at = dot(cam.fwd, d);
  const float ipd = cam.plane_dist / cos_at;
  const float i2sa = (ipd * ipd) / cos_at;
  const int pix = pix_index(static_cast<int>(sx), static_cast<int>(sy), A.H, A.W);  // (:263)
  if (VCM) {
    st3r(B.cs, l, PS_O, cam.pos);
    st3r(B.cs, l, PS_D, d);
    st3r(B.cs, l, PS_THR, v3(1.f, 1.f, 1.f));
    psf(B.cs, l, PS_DVCM) = static_cast<float>(A.P) / i2sa;  // lightPathNum / cameraPdf
    psf(B.cs, l, PS_DVC) = 0.f;
    psi(B.cs, l, PS_LEN) = 1;
    psi(B.cs, l, PS_NSPEC) = 0;
    psu(B.cs, l, PS_CTR) = rng.ctr;
    psi(B.cs, l, PS_PIX) = pix;  // (VertexCM's camera gen sets PS_DVM after this)
  } else {
    // dVCM = lightPathNum / cameraPdf, dVC = 0; no camera vertex stored yet
    bq_store_a(B.cs, l, bq_half_a(v3(1.f, 1.f, 1.f), static_cast<float>(A.P) / i2sa));
    bq_store_b(B.cs, l, bq_half_b(0.f, rng.ctr, bq_pack(1, 0, 0), pix));
    B.cvc[l] = 0;
  }
  const int e = ebase + s;  // overlapped: behind the light pass's first rays (cam_ext_base)
  st3(B.q_o[0], B.qs, e, cam.pos + d * WR_EPS);
  st3(B.q_d[0], B.qs, e, normalize(d));
  B.q_path[0][e] = l;
  return l;
}
__global__ void __launch_bounds__(kShadeBlock) WR_NO_PK_FP32 k_camera_gen(BdptGroup G_) {
  const BdptArgs& A = G_.a[blockIdx.y];
  const int eb = cam_ext_base(A, kCamSlot);
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < A.n; s += gridDim.x * blockDim.x) camera_gen_one(A, s, eb);
  if (blockIdx.x == 0 && threadIdx.x == 0) A.sc->ext[kCamSlot] = A.n;
}

// One camera-subpath vertex (:148-260): emitter hit, DI setup, vertex
// connections (shadow rays queued), scattering -- path p's ray (o, d) hit prim
// at t (prim < 0: a spare lane of the hit list's last wave; a missed entry is
// never listed, compact_hits).  Every lane of the wave calls it.  oslot:
// the step whose queues (shadow / aux, DI records, extension) get this
// vertex's rays (slot + 1).
// ebase: the queue index of the camera pass's first extension ray of step
// oslot (cam_ext_base, read once by the caller)
__device__ __forceinline__ void camera_vertex(const BdptArgs& A, const DMat* mats, const DLight* lights,
                                              const VtxIn& in, int oslot, int ebase) {
  const BdptBuf& B = A.B;
  const DevScene& S = A.S;
  const int P = B.P, nxt = oslot & 1, cap = B.cap_sq;  // P: buffer stride
  const int p = in.p, prim = in.prim;
  const float t = in.t;
  const V3 d = in.d;
  const float lpp = 1.f / static_cast<float>(S.nlights);
  const BdptBuf::Sq& Q = B.sq[oslot & 1];  // rays traced at step oslot
  const BdptBuf::Di& D = B.di[oslot & 1];
  bool ext = false, conn_phase = false, nee = false, dib = false;
  int pix = -1, nv = 0, len = 0, nspec = 0, cnspec = 0, pk = 0, ncv = 0;  // ncv: stored camera vertices
  V3 hp{}, thr{}, cthr{}, e_o{}, e_d{}, nee_tgt{}, nee_d{}, dib_o{}, dib_d{};
  float dvcm = 0.f, dvc = 0.f, cdvcm = 0.f, cdvc = 0.f;
  Bsdf b;
  b.mat = 0;
  if (prim >= 0) {
    const Hit h = rebuild_hit(S, prim, t, in.o, d, in.g.r0, in.g.r1, in.g.cs);
    bsdf_init(b, -d, h.n, h.mat, mats);
    if (b.mat != 0) {
      hp = h.p;
      pix = __float_as_int(in.st.b.w);
      dvcm = in.st.a.w;
      dvc = in.st.b.x;
      pk = __float_as_int(in.st.b.z);
      len = bq_len(pk);
      nspec = bq_nspec(pk);
      ncv = bq_count(pk);
      thr = v3(in.st.a.x, in.st.a.y, in.st.a.z);
      dvcm *= (t * t);  // (:180-182)
      dvcm /= fabsf(b.wi.z);
      dvc /= fabsf(b.wi.z);
      // this vertex's state, used by DI and the connections; the scatter
      // below updates thr / dvcm / dvc / nspec for the next vertex
      cthr = thr;
      cdvcm = dvcm;
      cdvc = dvc;
      cnspec = nspec;
      if (h.mat < 0) {  // hit an emitter (:184-199)
        if (len_ok(A.ctl, len)) {
          const DLight L = lights[-h.mat - 1];
          float dpa, ep;
          V3 r = light_radiance(L, d, &dpa, &ep);
          if (!black(r)) {
            if (len != 1) {  // getLightRadiance (:454-482)
              dpa *= lpp;
              ep *= lpp;
              const float wc = dpa * dvcm + ep * dvc;
              r = r * (1.f / (1.f + wc));
            }
            film_add(A.film, pix, mul(thr, r));
          }
        }
      } else if (len < A.maxlen) {
        Rng rng{stream_key(A.seed, A.iter, 1, static_cast<uint32_t>(A.base + p)), __float_as_uint(in.st.b.y)};
        if (!b.delta && len_ok(A.ctl, len + 1)) {  // getDirectIllumination (:205-217, :484-608)
          const float wlen = 1.f / (static_cast<float>(len) + 1.f - static_cast<float>(nspec));
          const int lid = min(static_cast<int>(rng.f() * static_cast<float>(S.nlights)), S.nlights - 1);
          const DLight L = lights[lid];
          V3 dtl;
          float dist = 0.f, dpdf = 0.f, epdf = 0.f, cal = 0.f;
          const V3 illu = light_illuminance(L, hp, rng.v(), &dtl, &dist, &dpdf, &epdf, &cal);
          int flags = 0;
          V3 nee_val = v3(0.f, 0.f, 0.f), bsdf_val = v3(0.f, 0.f, 0.f);
          float nee_w = 0.f;
          if (!black(illu) && dpdf > 0) {
            float cos_to = 0.f, bdp, brp;
            const V3 bf = bsdf_f(b, mats, dtl, &cos_to, &bdp, &brp);
            if (!black(bf)) {
              bdp *= b.cont;
              brp *= b.cont;
              const V3 tmp = div_plain(mul(illu, bf) * cos_to, dpdf * lpp);
              if (!black(tmp)) {
                nee = true;
                flags |= DI_NEE;
                nee_d = normalize(dtl);
                nee_tgt = hp + dtl * dist;
                const float wl = bdp / (dpdf * lpp);
                const float wc = (epdf * cos_to / (dpdf * cal)) * (dvcm + brp * dvc);
                nee_w = WR_TEST_DI_W / (wl + 1.f + wc);
                nee_val = tmp * (dpdf / (dpdf + bdp));
              }
            }
          }
          V3 dtl2 = dtl;
          float dpdf2 = dpdf, cos_s = 0.f;
          int type;
          const V3 bf2 = bsdf_sample(b, mats, rng.v(), &dtl2, &dpdf2, &cos_s, &type);
          if (!black(bf2) && dpdf2 > 0) {
            float w = 1.f;
            V3 illu2 = illu;
            bool early = false;
            if (!(type & T_SPEC)) {
              float lpdf, ep2;
              illu2 = light_radiance(L, dtl2, &lpdf, &ep2);
              if (cmpf(lpdf) == 0) early = true;  // (:563-564) returns res unweighted
              else w = dpdf2 / (dpdf2 + lpdf);
            }
            if (early) {
              flags |= DI_EARLY;
            } else {
              dib = true;
              flags |= DI_BSDF;
              dib_o = hp + dtl2 * WR_EPS;
              dib_d = normalize(dtl2);
              if (!black(illu2)) bsdf_val = div_plain(mul(illu2, bf2) * cos_s, dpdf2) * w;
            }
          }
          // a record only when a ray will be resolved: with neither the NEE
          // nor the BSDF ray the contribution is exactly zero (:533-607)
          const int nrays = (nee ? 1 : 0) + (dib ? 1 : 0);
          if (nrays > 0) {
            // (the whole record, as four 16-byte stores; word 15 is unused)
            float4* r = reinterpret_cast<float4*>(D.r) + 4 * size_t(p);
            r[0] = make_float4(nee_val.x, nee_val.y, nee_val.z, nee_w);
            r[1] = make_float4(bsdf_val.x, bsdf_val.y, bsdf_val.z, thr.x);
            r[2] = make_float4(thr.y, thr.z, wlen, __int_as_float(flags));
            r[3] = make_float4(__int_as_float(lid), __int_as_float(pix), __int_as_float(nrays), 0.f);
          }
        }
        if (!b.delta) {
          conn_phase = true;
          const int lv = in.oc;
          nv = lv & ~kLightAlive;
          // overlapped schedule: a vertex a later light vertex may still meet
          // (len < l, l + 1 + len <= maxlen) is kept for that light vertex --
          // if the light subpath still has a ray (after this step's light
          // kernel: a vertex of length > len may come); else none will
          if (A.overlap && 2 * len + 2 <= A.maxlen && (lv & kLightAlive)) {
            const int j = ncv;
            int cs = j * P + p;
            if (B.cidx) {  // a pool record
              cs = pool_take(A, &A.sc->cpool, B.ccap);
              B.cidx[size_t(j) * P + p] = cs;
            }
            if (cs >= 0) store_vertex(B.cv, cs, hp, b, cthr, cdvcm, cdvc, prim, len, cnspec, pix);
            ncv = j + 1;
          }
        }
        V3 so{}, sd{};  // sampleScattering's origin and direction (outputs only)
        if (sample_scatter(mats, rng, b, hp, so, sd, thr, dvcm, dvc, nspec)) {
          ext = true;
          e_o = so + sd * WR_EPS;
          e_d = normalize(sd);
        }
        // Commit the state for the NEXT vertex (:259-260 and the loop
        // increment) as whole 16-byte halves: all of the record when the path
        // scattered, else the half with the counter and the stored vertices.
        // The connections below use the values of THIS vertex (cthr, cdvcm,
        // cdvc, cnspec).
        if (ext) {
          bq_store_a(B.cs, p, bq_half_a(thr, dvcm));
          bq_store_b(B.cs, p, bq_half_b(dvc, rng.ctr, bq_pack(len + 1, nspec, ncv), pix));
        } else {
          bq_store_b(B.cs, p, bq_half_b(in.st.b.x, rng.ctr, bq_pack(len, nspec, ncv), pix));
        }
        if (ncv != bq_count(pk)) B.cvc[p] = static_cast<uint8_t>(ncv);
      }
    }
  }
  // DI queue entries
  {
    const int ni = wave_append(&A.sc->sq[oslot], nee);
    if (sq_fits(A, nee, ni)) {
      st3(Q.o, B.qs, ni, hp);
      st3(Q.d, B.qs, ni, nee_d);
      st3(Q.tgt, cap, ni, nee_tgt);
      Q.cut[ni] = occl_cut(hp, nee_tgt, dot(nee_tgt - hp, nee_d));
      Q.meta[ni] = (SQ_NEE << 30) | p;
      Q.pix[ni] = pix;
    }
    const int bi = wave_append(&A.sc->sq[oslot], dib);
    if (sq_fits(A, dib, bi)) {
      st3(Q.o, B.qs, bi, dib_o);
      st3(Q.d, B.qs, bi, dib_d);
      Q.cut[bi] = -WR_INF;  // needs the closest hit (same light?)
      Q.meta[bi] = (SQ_DIB << 30) | p;
      Q.pix[bi] = pix;
    }
  }
  // vertex connections to the paired light subpath (:219-257)
  if (__ballot(conn_phase && nv > 0)) {
    for (int k = 0; __ballot(conn_phase && k < nv); ++k) {
      bool shoot = false, counted = false;
      V3 sdir{}, stgt{}, sval{};
      const int slot = conn_phase && k < nv ? lv_slot(B, k, p) : -1;
      if (slot >= 0) {
        const BvRec lv = bv_load(B.vs, slot);
        const int llen = bv_len(lv);
        if (llen + 1 + len > A.maxlen) {
          nv = k;  // break (:237-239)
        } else {
          shoot = connect_pair(A, mats, b, hp, cthr, cdvcm, cdvc, cnspec, len, lv, llen, sdir, stgt, sval, counted);
        }
      }
      queue_connection(A, oslot, shoot, counted, p, pix, hp, sdir, stgt, sval);
    }
  }
  const int ei = wave_append(&A.sc->ext[oslot], ext) + ebase;
  if (ext) {
    st3(B.q_o[nxt], B.qs, ei, e_o);
    st3(B.q_d[nxt], B.qs, ei, e_d);
    B.q_path[nxt][ei] = p;
  }
}

__device__ __forceinline__ void camera_shade_body(const BdptArgs& A, const DMat* mats, const DLight* lights, int slot,
                                                  int bid, int nblk) {
  const BdptBuf& B = A.B;
  const int cur = slot & 1;
  const int n = A.sc->ext[slot], e0 = cam_ext_base(A, slot), eb = cam_ext_base(A, slot + 1);
  if (bid == 0 && threadIdx.x == 0) atomicAdd(&A.ctr->closest, (unsigned long long)n);
  // the hit entries of each chunk, in full waves (compact_hits; a missed
  // camera ray needs nothing)
  __shared__ HitList s_hits;
  const int R = hit_chunk_r(n, nblk), chunk = R * kShadeBlock, e1 = e0 + n;
  int i = threadIdx.x;  // (the thread's index, then its place in the list: k_light_shade)
  for (int c0 = e0 + bid * chunk; c0 < e1; c0 += nblk * chunk) {  // (block-uniform: every thread reaches the barriers)
    i &= kShadeBlock - 1;
    const int nh = compact_hits<false>(s_hits, B.q_prim[cur], nullptr, nullptr, i, c0, min(chunk, e1 - c0), R);
    for (; (i & ~63) < nh; i += kShadeBlock) {
      // stage A: the entry's columns, all at once (a spare lane of the list's
      // last wave reads the last entry)
      const int e = c0 + s_hits.at[min(i, nh - 1)];
      const int p = B.q_path[cur][e], prim = B.q_prim[cur][e];
      const float t = B.q_t[cur][e];
      const V3 o = ld3(B.q_o[cur], B.qs, e), d = ld3(B.q_d[cur], B.qs, e);
      camera_vertex(A, mats, lights, vertex_inputs<true>(A, i < nh, p, prim, t, o, d), slot + 1, eb);
    }
  }
}

// Light-tracing splats and camera-pass shadow / aux rays after traversal.
// Light-tracing splats and camera-pass shadow / aux rays of step `slot` after
// traversal.  A DI record is finalized (getDirectIllumination's combination,
// :533-607) by whichever of its rays is resolved last: each resolve adds
// (its result bit - 1) to the record's state word in one atomic.
// VCM: the queue's o / d are arrays of its own with the stride cap_sq (wr_vcm.h);
// BDPT's are segments of the pipeline's ray slab with the plane stride qs
template <bool VCM = false>
__device__ __forceinline__ void sq_resolve_body(const BdptArgs& A, int slot, int bid, int nblk) {
  const BdptBuf& B = A.B;
  const DevScene& S = A.S;
  const BdptBuf::Sq& Q = B.sq[slot & 1];
  const BdptBuf::Di& D = B.di[slot & 1];
  const int cap = B.cap_sq, n = min(A.sc->sq[slot], cap);  // (appends past cap were dropped: overflow)
  const int rs = VCM ? cap : B.qs;
  const int gstride = nblk * blockDim.x;
  const int nround = (n + gstride - 1) / gstride * gstride;
  for (int j = bid * blockDim.x + threadIdx.x; j < nround; j += gstride) {
    bool is_shadow = false, is_closest = false;
    if (j < n) {
      const int meta = Q.meta[j];
      const int kind = (meta >> 30) & 3, p = meta & (kSqNoValue - 1);
      const int prim = Q.prim[j];
      const float t = Q.t[j];
      int di_bits = -1;  // >= 0: this ray belongs to DI record p
      if (meta & kSqNoValue) {  // a filtered connection: traced and counted, nothing to add
        is_shadow = true;
      } else if (kind == SQ_DIB) {  // DI BSDF-sampled ray: same light? (:570-596)
        is_closest = true;
        bool same = false;
        if (prim >= 0) {
          const int m = __float_as_int(S.prim_rec[2 * static_cast<size_t>(prim) + 1].z);
          same = m < 0 && -m - 1 == dri(D.r, p, DR_LIGHT);
        }
        di_bits = same ? DI_SAME : 0;
      } else {  // Scene::occluded: position equality (scene.cpp:55-69)
        is_shadow = true;
        bool unocc = true;
        if (prim >= 0) {
          const V3 o = ld3(Q.o, rs, j), d = ld3(Q.d, rs, j);
          unocc = near_eq(o + d * t, ld3(Q.tgt, cap, j));
        }
#ifdef WR_DEBUG_PATH
        if (kind == SQ_SPLAT && A.base + p == WR_DEBUG_PATH && A.iter == WR_DEBUG_ITER) {
          const V3 o = ld3(Q.o, rs, j), d = ld3(Q.d, rs, j), v = ld3(Q.val, cap, j);
          printf("[dbg gpu] splat o %a %a %a d %a %a %a prim %d t %a unocc %d val %a %a %a pix %d\n", o.x, o.y, o.z, d.x,
                 d.y, d.z, prim, t, (int)unocc, v.x, v.y, v.z, Q.pix[j]);
        }
#endif
        if (kind == SQ_NEE) {
          di_bits = unocc ? DI_VIS : 0;
        } else if (unocc) {
          film_add(A.film, Q.pix[j], ld3(Q.val, cap, j));
        }
      }
      if (di_bits >= 0) {
        const int st = atomicAdd(&dri(D.r, p, DR_STATE), di_bits - 1) + di_bits - 1;
        if ((st & DI_COUNT) == 0) {
          const int flags = dri(D.r, p, DR_FLAGS);
          V3 res = v3(0.f, 0.f, 0.f);
          float weight = 0.f;
          if ((flags & DI_NEE) && (st & DI_VIS)) {
            weight = drf(D.r, p, DR_NEEW);
            res = res + drld3(D.r, p, DR_NEE);
          }
          V3 di;
          if (flags & DI_EARLY) {
            di = res;
          } else {
            if ((flags & DI_BSDF) && (st & DI_SAME)) res = res + drld3(D.r, p, DR_BSDF);
            di = res * weight;
          }
          film_add(A.film, dri(D.r, p, DR_PIX), mul(drld3(D.r, p, DR_THR), di) * drf(D.r, p, DR_WLEN));
        }
      }
    }
    wave_count(&A.ctr->shadow, is_shadow);
    wave_count(&A.ctr->closest, is_closest);
  }
}

// One camera-pass step after its traversal: resolve the step's shadow / aux
// rays (blocks [0, nres)) and shade its camera vertices (the rest) -- they touch
// different queue / DI buffers.  The last step has no vertices (shade = 0).
template <bool GT>
__global__ void __launch_bounds__(kShadeBlock) WR_SHADE_OCC k_camera_step(BdptGroup G_, int slot, int nres,
                                                                         int shade) {
  const BdptArgs& A = G_.a[blockIdx.y];
  const int b = static_cast<int>(blockIdx.x), nblk = static_cast<int>(gridDim.x);
  if (b < nres) {  // (block-uniform: the resolve reads neither table)
    sq_resolve_body(A, slot, b, nres);
    return;
  }
  WR_BDPT_TABLES(A)
  if (shade) camera_shade_body(A, mats, lights, slot, b - nres, nblk - nres);
}
