// PhotonIntegrator (surfaceIntegrator/photonMap.{h,cpp}) as kernels (include/
// winmad_rt.h wr_photon_*, wr_render_photon): the photon pass
// (buildPhotonMap, :48-162) in batches of shots over the closest-hit search,
// estimate (:164-231) as one wave per query on the k-nearest wave of
// wr_points.h, and the camera pass (raytracing, :304-366) as a loop over
// depths 0..2.  Included by wr_render.hip inside its anonymous namespace, after
// wr_points.h.  No LDS; every loop is bounded by a count, a bucket count or k.
#pragma once

constexpr uint32_t kPhotonSubpath = 3;  // the counter-RNG subpath of a photon shot
enum : int { PH_NONE = 0, PH_CAUSTIC = 1, PH_INDIRECT = 2 };

// ---------------------------------------------------------------- photon pass
// One batch of B shots.  Queue columns are SoA with stride B; a shot's photons
// go to slots of its own, shot * L + (nIntersections - 2), so what a batch
// stores does not depend on the order its queues were filled in.
struct PhBuf {
  int B, L;
  float* alpha;   // [B][3]
  int* spec;      // [B] specularPath
  uint32_t* ctr;  // [B] draws taken from the shot's stream
  float *q_o[2], *q_d[2], *q_t[2];
  int *q_prim[2], *q_shot[2];
  int* qn;        // [L + 2] rays entering bounce b
  float *s_pos, *s_wi, *s_alpha;  // [B * L][3]
  int* s_class;                   // [B * L]
};

// a shot's light pick and emit (:69-84): no retry, a black alpha wastes the shot
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_ph_gen(DevScene S, PhBuf T, uint32_t seed, int64_t shot0,
                                                              int n) {
  const float lpp = 1.f / static_cast<float>(S.nlights);
  const int nround = (n + 63) / 64 * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nround; i += gridDim.x * blockDim.x) {
    bool go = false;
    V3 pos{}, dir{};
    if (i < n) {
      Rng rng{stream_key(seed, 0, kPhotonSubpath, static_cast<uint32_t>(shot0 + i)), 0};
      const int id = min(static_cast<int>(rng.f() * static_cast<float>(S.nlights)), S.nlights - 1);
      const DLight L = S.lights[id];
      const V3 pr = rng.v();  // emit(..., randVector3(), randVector3(), ...): the second argument first
      const V3 dr = rng.v();
      float epdf = 0.f, dpa = 0.f, cal = 0.f;
      V3 a = light_emit(L, dr, pr, &pos, &dir, &epdf, &dpa, &cal);
      a = div_plain(a * cal, epdf * lpp);
      go = !black(a);
      T.alpha[3 * i] = a.x, T.alpha[3 * i + 1] = a.y, T.alpha[3 * i + 2] = a.z;
      T.spec[i] = 1;
      T.ctr[i] = rng.ctr;
    }
    const int e = wave_append(&T.qn[0], go);
    if (go) {
      st3(T.q_o[0], T.B, e, pos);  // Ray(lightPos, lightDir): no EPS offset (:82); the constructor normalises
      st3(T.q_d[0], T.B, e, normalize(dir));
      T.q_shot[0][e] = i;
    }
  }
}

// the vertex of bounce b (nIntersections = b + 1) of every shot still under way (:89-158)
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_ph_shade(DevScene S, PhBuf T, uint32_t seed, int64_t shot0,
                                                                int b, int max_len) {
  const int cur = b & 1, nxt = cur ^ 1, B = T.B;
  const int n = T.qn[b];
  const int nround = (n + 63) / 64 * 64;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < nround; j += gridDim.x * blockDim.x) {
    bool ext = false;
    int i = -1;
    V3 e_o{}, e_d{};
    if (j < n) {
      i = T.q_shot[cur][j];
      const int prim = T.q_prim[cur][j];
      if (prim >= 0) {
        const V3 o = ld3(T.q_o[cur], B, j), d = ld3(T.q_d[cur], B, j);
        const Hit h = rebuild_hit(S, prim, T.q_t[cur][j], o, d);
        Bsdf bs;
        bs.mat = 0;
        if (h.mat > 0) bsdf_init(bs, -d, h.n, h.mat, S.mats);
        if (bs.mat > 0) {  // (a grazing hit has no BSDF: the path ends, nothing is stored)
          const int nint = b + 1;
          V3 a = v3(T.alpha[3 * i], T.alpha[3 * i + 1], T.alpha[3 * i + 2]);
          int spec = T.spec[i];
          if ((cmpf(bs.pd) > 0 || cmpf(bs.pg) > 0) && nint > 1) {
            const size_t s = size_t(i) * T.L + (nint - 2);
            sh_st3(T.s_pos + 3 * s, h.p);
            sh_st3(T.s_wi + 3 * s, -d);
            sh_st3(T.s_alpha + 3 * s, a);
            T.s_class[s] = spec ? PH_CAUSTIC : PH_INDIRECT;
          }
          if (!(nint > max_len)) {
            Rng rng{stream_key(seed, 0, kPhotonSubpath, static_cast<uint32_t>(shot0 + i)), T.ctr[i]};
            float pdf = 0.f, cw = 0.f;
            int type = 0;
            V3 dn = d;
            const V3 bf = bsdf_sample(bs, S.mats, rng.v(), &dn, &pdf, &cw, &type);
            if (!black(bf)) {
              if (type & (T_DIFF | T_GLOSSY)) spec = 0;
              bool cont = true;
              const float cp = bs.cont;
              if (cmpf(cp - 1.f) < 0) {
                if (cmpf(rng.f() - cp) > 0) cont = false;
                else pdf *= cp;
              }
              if (cont) {
                a = mul(a, bf) * (cw / pdf);
                ext = true;
                e_o = h.p + dn * WR_EPS;
                e_d = dn;
                T.alpha[3 * i] = a.x, T.alpha[3 * i + 1] = a.y, T.alpha[3 * i + 2] = a.z;
                T.spec[i] = spec;
              }
            }
            T.ctr[i] = rng.ctr;
          }
        }
      }
    }
    const int e = wave_append(&T.qn[b + 1], ext);
    if (ext) {
      st3(T.q_o[nxt], B, e, e_o);
      st3(T.q_d[nxt], B, e, e_d);
      T.q_shot[nxt][e] = i;
    }
  }
}

// 0 / 1 per slot and class, one more (0) at the end: the scans' last entries are the totals
__global__ void __launch_bounds__(256) k_ph_flags(const int* cls, int n, int* fc, int* fi) {
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s <= n; s += gridDim.x * blockDim.x) {
    const int c = s < n ? cls[s] : PH_NONE;
    fc[s] = c == PH_CAUSTIC;
    fi[s] = c == PH_INDIRECT;
  }
}

// A map under construction: `count` photons of `cap`.  pay: {wi, 0, alpha, 0} per photon.
struct PhMapOut {
  float* pos;
  float4* pay;
  int32_t* shot;
  int count, cap;
};
// the batch's photons of each class appended in slot order, (shot, bounce), while there is room
__global__ void __launch_bounds__(256) k_ph_scatter(PhBuf T, int n, const int* pc, const int* pi, int64_t shot0,
                                                    PhMapOut C, PhMapOut I) {
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const int c = T.s_class[s];
    if (c == PH_NONE) continue;
    const PhMapOut& M = c == PH_CAUSTIC ? C : I;
    const int64_t g = int64_t(M.count) + (c == PH_CAUSTIC ? pc[s] : pi[s]);
    if (g >= M.cap) continue;
    for (int a = 0; a < 3; ++a) M.pos[3 * g + a] = T.s_pos[3 * size_t(s) + a];
    M.pay[2 * g] = make_float4(T.s_wi[3 * size_t(s)], T.s_wi[3 * size_t(s) + 1], T.s_wi[3 * size_t(s) + 2], 0.f);
    M.pay[2 * g + 1] =
        make_float4(T.s_alpha[3 * size_t(s)], T.s_alpha[3 * size_t(s) + 1], T.s_alpha[3 * size_t(s) + 2], 0.f);
    M.shot[g] = static_cast<int32_t>(shot0 + s / T.L);
  }
}

// ---------------------------------------------------------------- estimate
struct PmMap {
  PtsIndex X;
  const float4* pay;  // by the photon's index in the map
  int n;              // photons (0: an empty map, X is not read)
};

// estimate() (:164-231), one wave per query.  The search is the k-nearest wave
// with the bound starting unbounded (d2 < inf); then lane i holds winner i,
// loads its payload and evaluates its term (:210-228) against the query's
// BSDF, which every lane builds from the same hit (one build per wave); the
// terms are added in lane order through lane reads.  A miss, an empty map or a
// non-finite position gives found 0, msd 0 and black; a hit without a BSDF
// (material 0, grazing, a material the scene lacks) and an emitter give black.
// n_dev: the query count on the device (the render's queue), else n.
// film: the estimate times weight[j] is added to pixel pix[j] instead of written to rgb.
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_pm_gather(DevScene S, int nmats, PmMap M, const wr_hit* hits,
                                                                 const float* wo3, int64_t n, const int* n_dev, int k,
                                                                 float max_sqr_dist, float* rgb, float* msd_out,
                                                                 int32_t* found_out, const float* weight,
                                                                 const int* pix, float* film) {
  const int lane = __lane_id();
  const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  if (n_dev) n = *n_dev;
  for (int64_t j = wave0; j < n; j += nwaves) {
    const wr_hit h = hits[j];
    const float qx = h.p[0], qy = h.p[1], qz = h.p[2];
    int found = 0;
    float msd = 0.f;
    V3 est = v3(0.f, 0.f, 0.f);
    if (h.prim >= 0 && M.n > 0 && pts_finite3(qx, qy, qz)) {
      PtsKnn K;
      K.k = k, K.lane = lane;
      K.key = kPtsNone;
      K.limit = static_cast<uint64_t>(0x7f800000u) << 32;  // d2 < inf
      K.bound = K.limit;
      pts_knn_search(K, M.X, qx, qy, qz);
      const bool have = K.key != kPtsNone;
      found = __popcll(__ballot(have));
      if (found > 0) {
        // the reference's doubling loop (:180-186) in closed form: the first max_sqr_dist * 2^j above the k-th d2
        const float kth =
            __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<unsigned long long>(K.key), found - 1) >> 32));
        msd = max_sqr_dist;
        for (int it = 0; it < 300 && !(kth < msd); ++it) msd *= 2.f;
        const V3 wo = sh_ld3(wo3, j), nn = v3(h.n[0], h.n[1], h.n[2]);
        Bsdf b;
        b.mat = 0;
        if (h.mat_id < nmats && h.mat_id >= -S.nlights) bsdf_init(b, wo, nn, h.mat_id, S.mats);
        if (b.mat != 0) {
          const V3 nv = cmpf(dot(wo, nn)) < 0 ? -nn : nn;
          const float scale = 1.f / (WR_PI * msd * static_cast<float>(found));
          V3 term = v3(0.f, 0.f, 0.f);
          if (have) {
            const uint32_t idx = static_cast<uint32_t>(K.key);
            const float4 pw = M.pay[2 * size_t(idx)], pa = M.pay[2 * size_t(idx) + 1];
            V3 wi = v3(pw.x, pw.y, pw.z);
            if (!(cmpf(dot(nv, wi)) > 0)) wi.z *= -1.f;  // the world-space z, as the reference (:221-222)
            float cw = 0.f, pdf = 0.f;
            const V3 brdf = bsdf_f(b, S.mats, wi, &cw, &pdf, nullptr);
            if (!black(brdf)) term = mul(brdf, v3(pa.x, pa.y, pa.z)) * (cw * scale / pdf);
          }
          for (int i = 0; i < found; ++i) {  // at most 64: the stated order, one add per channel per term
            est.x = est.x + __shfl(term.x, i);
            est.y = est.y + __shfl(term.y, i);
            est.z = est.z + __shfl(term.z, i);
          }
        }
      }
    }
    if (lane == 0) {
      if (film) {
        film_add(film, pix[j], mul(sh_ld3(weight, j), est));
      } else {
        sh_st3(rgb + 3 * j, est);
        if (msd_out) msd_out[j] = msd;
        if (found_out) found_out[j] = found;
      }
    }
  }
}

// ---------------------------------------------------------------- camera pass
// The gather queue of one depth: the vertices whose two estimates are added.
struct PmGq {
  wr_hit* hits;
  float *wo, *weight;  // [P][3]
  int* pix;
};

// One PhotonIntegrator::raytracing level (:304-366) of a sample's paths, on
// the PT buffers (wr_pt.h): emitter, else direct light (its shadow ray to
// queue sq[depth + 1], resolved by k_pt_step), the gather queue entry, and the
// next ray.  direct_target 0: the shadow ray's target is at the camera ray's
// hit distance (the reference, :259); 1: at the light's distance.
__global__ void __launch_bounds__(kShadeBlock) WR_NO_PK_FP32 k_pm_shade(PtGroup G_, int depth, PmGq GQ,
                                                                        int direct_target) {
  const PtArgs& A = G_.a[0];
  const PtBuf& T = A.T;
  const DevScene& S = A.S;
  const int P = A.P, cur = depth & 1, nxt = cur ^ 1;
  const int n = A.sc->ext[depth];
  const int gstride = gridDim.x * blockDim.x;
  const int nround = (n + 63) / 64 * 64;
  const float nl = static_cast<float>(S.nlights);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < nround; j += gstride) {
    bool ext = false, shadow = false, gather = false;
    int p = -1, pix = -1;
    V3 e_o{}, e_d{}, s_o{}, s_d{}, s_tgt{}, s_val{}, pw{}, wo{};
    wr_hit rec{};
    if (j < n) {
      p = T.q_path[cur][j];
      const int prim = T.q_prim[cur][j];
      if (prim >= 0) {
        const V3 o = ld3(T.q_o[cur], P, j), d = ld3(T.q_d[cur], P, j);
        const Hit h = rebuild_hit(S, prim, T.q_t[cur][j], o, d);
        Bsdf b;
        b.mat = 0;
        if (h.mat > 0) bsdf_init(b, -d, h.n, h.mat, S.mats);
        pix = pti(T.st, p, PT_PIX);
        pw = pld3(T.st, p, PT_PW);
        if (h.mat < 0) {  // (:320-324, before any BSDF)
          film_add(A.film, pix, mul(pw, S.lights[-h.mat - 1].le * 100.f));
        } else if (b.mat > 0) {
          Rng rng{stream_key(A.seed, A.k, 2, static_cast<uint32_t>(p)), ptu(T.st, p, PT_CTR)};
          {  // directIllumination (:233-270)
            const int lid = min(static_cast<int>(rng.f() * nl), S.nlights - 1);
            const DLight L = S.lights[lid];
            V3 dtl;
            float dist = 0.f, dpdf = 0.f, ep, cal;
            V3 illu = light_illuminance(L, h.p, rng.v(), &dtl, &dist, &dpdf, &ep, &cal);
            if (dpdf > 0.f) {  // (a light seen from behind: 0 / 0 in the reference, nothing here)
              illu = div_plain(illu, dpdf / nl);
              float bp = 0.f, cw = 0.f;
              const V3 bf = bsdf_f(b, S.mats, dtl, &cw, &bp, nullptr);
              if (!black(bf)) {
                shadow = true;
                s_o = h.p + dtl * WR_EPS;
                s_d = normalize(dtl);
                s_tgt = h.p + dtl * ((direct_target ? dist : h.t) - WR_EPS);
                s_val = mul(pw, mul(illu, bf) * (cw / bp));
              }
            }
          }
          gather = true;
          wo = -d;
          rec.t = h.t;
          rec.p[0] = h.p.x, rec.p[1] = h.p.y, rec.p[2] = h.p.z;
          rec.n[0] = h.n.x, rec.n[1] = h.n.y, rec.n[2] = h.n.z;
          rec.prim = prim;
          rec.inside = h.inside;
          rec.mat_id = h.mat;
          if (depth < 2) {  // (:336-363; below depth 2 nothing comes back)
            float pdf = 0.f, cw = 0.f;
            int type;
            V3 dn = d;
            const V3 bf = bsdf_sample(b, S.mats, rng.v(), &dn, &pdf, &cw, &type);
            if (!black(bf)) {
              bool cont = true;
              const float cp = b.cont;
              if (cmpf(cp - 1.f) < 0) {
                if (cmpf(rng.f() - cp) > 0) cont = false;
                else pdf *= cp;
              }
              if (cont) {
                ext = true;
                e_o = h.p + dn * WR_EPS;
                e_d = dn;
                pst3(T.st, p, PT_PW, mul(pw, bf) * (cw / pdf));
              }
            }
            ptu(T.st, p, PT_CTR) = rng.ctr;
          }
        }
      }
    }
    const int ei = wave_append(&A.sc->ext[depth + 1], ext);
    if (ext) {
      st3(T.q_o[nxt], P, ei, e_o);
      st3(T.q_d[nxt], P, ei, e_d);
      T.q_path[nxt][ei] = p;
    }
    const int si = wave_append(&A.sc->sq[depth + 1], shadow);
    if (shadow) {
      const PtBuf::Sq& Q = T.sq[(depth + 1) & 1];
      st3(Q.o, P, si, s_o);
      st3(Q.d, P, si, s_d);
      st3(Q.tgt, P, si, s_tgt);
      st3(Q.val, P, si, s_val);
      Q.cut[si] = occl_cut(s_o, s_tgt, dot(s_tgt - s_o, s_d));
      Q.pix[si] = pix;
    }
    const int gi = wave_append(&A.sc->mq[depth], gather);
    if (gather) {
      GQ.hits[gi] = rec;
      sh_st3(GQ.wo + 3 * size_t(gi), wo);
      sh_st3(GQ.weight + 3 * size_t(gi), pw);
      GQ.pix[gi] = pix;
    }
  }
}
