// Shading on device arrays (include/winmad_rt.h wr_bsdf_*_dev, wr_light_*_dev,
// wr_rng_uniform_dev): the device functions of wr_devmath.h -- the
// ones the renders and the known-answer harness (tests/native/dev_kat.hip) call
// -- applied to a caller's arrays, one record per lane.  Included by
// wr_render.hip inside its anonymous namespace.
//
// One kernel per call, 256-thread blocks, grid-stride, no LDS.  The records are
// AoS structs of 4-byte members that need only 4-byte alignment, so every
// access is a dword load or store.  A record starts from zeros and keeps them
// where the reference's function writes nothing.  The arrays are the caller's
// and live on the device, so the indices they hold are checked here: a light
// or material outside the scene's tables gives an all-zero record.
#pragma once

static_assert(sizeof(wr_bsdf_info) == 36 && sizeof(wr_bsdf_eval) == 32 && sizeof(wr_bsdf_sample) == 36 &&
                  sizeof(wr_light_illum) == 40 && sizeof(wr_light_emission) == 48 && sizeof(wr_light_rad) == 20 &&
                  alignof(wr_light_emission) == 4 && alignof(wr_hit) == 4,
              "the shading records are packed 4-byte members");

__device__ __forceinline__ V3 sh_ld3(const float* p, int64_t i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
__device__ __forceinline__ void sh_st3(float* p, V3 v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}
#define WR_SHADE_FOR(i, n)                                                                      \
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < (n);        \
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)

// BSDF::init for hits[i] and wi[i]; false = no BSDF (a miss, material 0, a
// material or light the scene does not have, wi in the tangent plane)
__device__ __forceinline__ bool sh_bsdf(const DevScene& S, int nmats, const wr_hit* hits, const float* wi, int64_t i,
                                        Bsdf& b, wr_bsdf_info& in) {
  in = wr_bsdf_info{};
  const int prim = hits[i].prim, mat = hits[i].mat_id;
  if (prim < 0 || mat >= nmats || mat < -S.nlights) return false;
  bsdf_init(b, sh_ld3(wi, i), v3(hits[i].n[0], hits[i].n[1], hits[i].n[2]), mat, S.mats);
  if (b.mat == 0) return false;
  in.valid = 1;
  in.is_delta = b.delta ? 1 : 0;
  in.cos_wi = b.wi.z;
  in.continue_prob = b.cont;
  in.fresnel = b.fres;
  in.prob[0] = b.pd;
  in.prob[1] = b.pg;
  in.prob[2] = b.pr;
  in.prob[3] = b.pt;
  return true;
}

// BSDF::f with its two pdfs, BSDF::pdf forward and reverse
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_bsdf_eval(DevScene S, int nmats, const wr_hit* hits,
                                                                 const float* wi, const float* wo, int64_t n,
                                                                 wr_bsdf_info* info, wr_bsdf_eval* out) {
  WR_SHADE_FOR(i, n) {
    Bsdf b;
    wr_bsdf_info in;
    wr_bsdf_eval r{};
    if (sh_bsdf(S, nmats, hits, wi, i, b, in)) {
      const V3 w = sh_ld3(wo, i);
      sh_st3(r.f, bsdf_f(b, S.mats, w, &r.cos_wo, &r.dir_pdf, &r.rev_pdf));
      if (b.mat > 0) {  // an emitter has no lobes: BSDF::pdf is 0 (and bsdf_pdf reads the material)
        r.pdf = bsdf_pdf(b, S.mats, w, false);
        r.pdf_rev = bsdf_pdf(b, S.mats, w, true);
      }
    }
    if (info) info[i] = in;
    out[i] = r;
  }
}

// BSDF::sample
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_bsdf_sample(DevScene S, int nmats, const wr_hit* hits,
                                                                   const float* wi, const float* r3, int64_t n,
                                                                   wr_bsdf_info* info, wr_bsdf_sample* out) {
  WR_SHADE_FOR(i, n) {
    Bsdf b;
    wr_bsdf_info in;
    wr_bsdf_sample r{};
    if (sh_bsdf(S, nmats, hits, wi, i, b, in)) {
      V3 w = v3(0.f, 0.f, 0.f);
      int type = 0;
      sh_st3(r.f, bsdf_sample(b, S.mats, sh_ld3(r3, i), &w, &r.pdf, &r.cos_wo, &type));
      sh_st3(r.wo, w);
      r.type = type;
    }
    if (info) info[i] = in;
    out[i] = r;
  }
}

// AreaLight::illuminance
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_light_illuminate(DevScene S, const int32_t* light,
                                                                        const float* pos, const float* r3, int64_t n,
                                                                        wr_light_illum* out) {
  WR_SHADE_FOR(i, n) {
    wr_light_illum r{};
    const int li = light[i];
    if (li >= 0 && li < S.nlights) {
      const DLight L = S.lights[li];
      V3 d = v3(0.f, 0.f, 0.f);
      sh_st3(r.le, light_illuminance(L, sh_ld3(pos, i), sh_ld3(r3, i), &d, &r.dist, &r.direct_pdf, &r.emission_pdf,
                                     &r.cos_light));
      sh_st3(r.dir, d);
    }
    out[i] = r;
  }
}

// AreaLight::emit
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_light_emit(DevScene S, const int32_t* light,
                                                                  const float* dir_r3, const float* pos_r3, int64_t n,
                                                                  wr_light_emission* out) {
  WR_SHADE_FOR(i, n) {
    wr_light_emission r{};
    const int li = light[i];
    if (li >= 0 && li < S.nlights) {
      const DLight L = S.lights[li];
      V3 p = v3(0.f, 0.f, 0.f), d = p;
      sh_st3(r.le_cos, light_emit(L, sh_ld3(dir_r3, i), sh_ld3(pos_r3, i), &p, &d, &r.emission_pdf, &r.direct_pdf_a,
                                  &r.cos_light));
      sh_st3(r.pos, p);
      sh_st3(r.dir, d);
    }
    out[i] = r;
  }
}

// AreaLight::getRadiance of the light a hit lies on
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_light_radiance(DevScene S, const wr_hit* hits,
                                                                      const float* ray_d, int64_t n,
                                                                      wr_light_rad* out) {
  WR_SHADE_FOR(i, n) {
    wr_light_rad r{};
    const int prim = hits[i].prim, mat = hits[i].mat_id;
    if (prim >= 0 && mat < 0 && mat >= -S.nlights) {
      const DLight L = S.lights[-mat - 1];
      sh_st3(r.le, light_radiance(L, sh_ld3(ray_d, i), &r.direct_pdf_a, &r.emission_pdf));
    }
    out[i] = r;
  }
}

// `draws` of Rng::f from stream (seed, iteration, subpath, path[i]) after draw ctr[i]
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_rng_uniform(uint32_t seed, uint32_t iteration,
                                                                   uint32_t subpath, const uint32_t* path,
                                                                   uint32_t* ctr, int draws, int64_t n, float* out) {
  WR_SHADE_FOR(i, n) {
    Rng rng{stream_key(seed, iteration, subpath, path ? path[i] : static_cast<uint32_t>(i)), ctr ? ctr[i] : 0u};
    float* o = out + i * draws;
    for (int j = 0; j < draws; ++j) o[j] = rng.f();
    if (ctr) ctr[i] = rng.ctr;
  }
}
