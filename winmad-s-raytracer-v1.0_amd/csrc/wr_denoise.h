// wr_film_denoise (include/winmad_rt.h): an edge-avoiding a-trous
// filter over a film of n passes, guided by the per-pixel variance of the mean
// (from the second-moment film) and by the first-hit feature films.
//
// The filter is a definition: this header is its one text.  The CPU loop
// (wr_denoise.cpp, g++) and the gfx950 kernels (below, hipcc) both run
// dn::pixel() / dn::input() as written here, built with -ffp-contract=off.  They
// use + - * /, sqrt, fabs, max and comparisons only -- each correctly rounded on
// both sides -- in a fixed order, so device and host films are equal bit for
// bit.  That is why the falloff is a compact polynomial and not exp().
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "winmad_rt.h"

#if defined(__HIPCC__)
#define WR_DN_HD __host__ __device__ __forceinline__
#else
#define WR_DN_HD inline
#endif

namespace dn {

struct alignas(16) F4 {
  float x, y, z, w;
};

// One 16-byte access per word: on the device a single dwordx4 (global) or b128
// (LDS) instruction rather than four scalar ones.
#if defined(__HIP_DEVICE_COMPILE__)
typedef float V4 __attribute__((ext_vector_type(4)));
WR_DN_HD F4 ld4(const F4* p) {
  const V4 v = *reinterpret_cast<const V4*>(p);
  return F4{v.x, v.y, v.z, v.w};
}
WR_DN_HD void st4(F4* p, const F4& a) { *reinterpret_cast<V4*>(p) = V4{a.x, a.y, a.z, a.w}; }
#else
WR_DN_HD F4 ld4(const F4* p) { return *p; }
WR_DN_HD void st4(F4* p, const F4& a) { *p = a; }
#endif

// What a level needs besides the films: the sigmas, and which guides exist (a
// missing guide's weight is 1).
struct Cfg {
  float sigma_l, sigma_p, sigma_a;
  int normal_power;
  int has_n, has_p, has_a;
};

static_assert(sizeof(wr_denoise_params) == 20, "wr_denoise_params is 20 bytes (include/winmad_rt.h)");
constexpr int kMaxLevels = 8, kMaxNormalPower = 10;
inline wr_denoise_params default_params() { return wr_denoise_params{5, 7, 4.f, 0.05f, 0.1f}; }
// nullptr: in range; else what is wrong
inline const char* check_params(const wr_denoise_params& p) {
  if (p.levels < 1 || p.levels > kMaxLevels) return "levels must be in 1..8";
  if (p.normal_power < 0 || p.normal_power > kMaxNormalPower) return "normal_power must be in 0..10";
  if (!(p.sigma_l > 0.f) || !(p.sigma_p > 0.f) || !(p.sigma_a > 0.f)) return "sigma_l, sigma_p and sigma_a must be > 0";
  return nullptr;
}

// A pixel's record: (c.r, c.g, c.b, v) and the guides in three 16-byte words,
//   g0 = (N.x, N.y, N.z, P.x)   g1 = (P.y, P.z, A.r, A.g)   g2 = (A.b, 0, 0, 0)
// (a missing guide's floats are 0 and are never read).
struct Pix {
  F4 cv, g0, g1, g2;
};

// The films of a level, as planes of 16-byte words: element (y, x) of a plane is
// [(y - oy) * pitch + (x - ox)] -- the whole image (oy = ox = 0, pitch = W) or a
// tile with its halo staged in LDS.
struct View {
  const F4* cv;
  const F4* g0;
  const F4* g1;
  const F4* g2;
  int oy, ox, pitch;
  WR_DN_HD int at(int y, int x) const { return (y - oy) * pitch + (x - ox); }
  WR_DN_HD Pix pix(const Cfg& k, int y, int x) const {
    const int i = at(y, x);
    Pix p;
    p.cv = ld4(cv + i);
    const F4 z{0.f, 0.f, 0.f, 0.f};
    p.g0 = k.has_n ? ld4(g0 + i) : z;
    p.g1 = ((k.has_n && k.has_p) || k.has_a) ? ld4(g1 + i) : z;
    p.g2 = k.has_a ? ld4(g2 + i) : z;
    return p;
  }
};

// The mean and the standard error of the mean of one value from the sum S and
// the sum of squares Q of n passes: film_error_value of wr_render.hip
// (wr_film_error), restated for the host translation unit.
WR_DN_HD void moments(float S, float Q, double n, double* mu, double* se) {
  const double s = static_cast<double>(S), q = static_cast<double>(Q);
  double var = (q - s * s / n) / (n - 1.0);
  var = (var > 0.0 ? var : 0.0) / n;
  *mu = s / n;
  *se = sqrt(var);
}
// Input of level 0: c = (float)mu per channel, v = the luminance-weighted
// variance of the mean, summed in double.
WR_DN_HD F4 input(const float* S3, const float* Q3, double n) {
  double mu[3], se[3];
  for (int k = 0; k < 3; ++k) moments(S3[k], Q3[k], n, &mu[k], &se[k]);
  const double v = 0.2126 * (se[0] * se[0]) + 0.7152 * (se[1] * se[1]) + 0.0722 * (se[2] * se[2]);
  return F4{static_cast<float>(mu[0]), static_cast<float>(mu[1]), static_cast<float>(mu[2]), static_cast<float>(v)};
}
WR_DN_HD void pack_guides(const float* n3, const float* p3, const float* a3, F4* g0, F4* g1, F4* g2) {
  *g0 = F4{n3 ? n3[0] : 0.f, n3 ? n3[1] : 0.f, n3 ? n3[2] : 0.f, p3 ? p3[0] : 0.f};
  *g1 = F4{p3 ? p3[1] : 0.f, p3 ? p3[2] : 0.f, a3 ? a3[0] : 0.f, a3 ? a3[1] : 0.f};
  *g2 = F4{a3 ? a3[2] : 0.f, 0.f, 0.f, 0.f};
}

WR_DN_HD float lum(const F4& c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }
// k(x) = max(0, 1 - x / 4)^4: compact support, ~ e^-x near 0, exact arithmetic
WR_DN_HD float falloff(float x) {
  float m = 1.f - 0.25f * x;
  m = m > 0.f ? m : 0.f;
  return (m * m) * (m * m);
}
WR_DN_HD bool no_surface(const F4& g0) { return g0.x == 0.f && g0.y == 0.f && g0.z == 0.f; }
WR_DN_HD float b3(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// w_n: 1 between two no-surface pixels, 0 between a surface and a no-surface
// pixel, else max(0, Np . Nq) squared normal_power times.
WR_DN_HD float normal_weight(const Cfg& k, const F4& n_p, bool p_surf, const F4& n_q) {
  const bool q_surf = !no_surface(n_q);
  if (p_surf != q_surf) return 0.f;
  if (!p_surf) return 1.f;
  float d = n_p.x * n_q.x + n_p.y * n_q.y + n_p.z * n_q.z;
  d = d > 0.f ? d : 0.f;
  for (int i = 0; i < k.normal_power; ++i) d = d * d;
  return d;
}
// Weight of neighbour Q for pixel P (not the centre tap, whose weight is hk):
// w = hk * w_l * w_n * w_p * w_a, multiplied in that order (a factor that is 1
// by definition is skipped, which is the same product).
WR_DN_HD float tap_weight(const Cfg& k, float hk, float lum_p, float l_den, const Pix& P, bool p_surf, const Pix& Q) {
  float w = hk * falloff(fabsf(lum_p - lum(Q.cv)) / l_den);
  if (k.has_n) {
    w = w * normal_weight(k, P.g0, p_surf, Q.g0);
    if (k.has_p && p_surf && !no_surface(Q.g0)) {
      const float dx = Q.g0.w - P.g0.w, dy = Q.g1.x - P.g1.x, dz = Q.g1.y - P.g1.y;
      const float nd = P.g0.x * dx + P.g0.y * dy + P.g0.z * dz;
      const float dd = dx * dx + dy * dy + dz * dz;
      w = w * falloff(fabsf(nd) / (k.sigma_p * sqrtf(dd) + 1e-12f));
    }
  }
  if (k.has_a) {
    const float da = fabsf(Q.g1.z - P.g1.z) + fabsf(Q.g1.w - P.g1.w) + fabsf(Q.g2.x - P.g2.x);
    w = w * falloff(da / k.sigma_a);
  }
  return w;
}

// One pixel of one level (step s): reads (c, v) and the guides of the previous
// level through `src`, returns the next (c, v).  Taps (dy, dx) in {-2..2}^2, dy
// outer, dx inner, ascending; a tap outside the image is skipped before its
// address is formed.
WR_DN_HD F4 pixel(const View& src, const Cfg& k, int x, int y, int W, int H, int s) {
  const Pix P = src.pix(k, y, x);
  const bool p_surf = k.has_n && !no_surface(P.g0);
  const float lum_p = lum(P.cv);
  // vt: the 3x3 prefilter of v over the immediate neighbours (1/4, 1/8, 1/16),
  // normalised by the weights of the taps used: a tap outside the image is
  // skipped, and so is one whose w_n is exactly 0 -- the variance of what lies
  // across an edge must not reach this pixel either
  float pv = 0.f, pk = 0.f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= W) continue;
      const int qi = src.at(qy, qx);
      if (k.has_n && (dy != 0 || dx != 0) && normal_weight(k, P.g0, p_surf, src.g0[qi]) == 0.f) continue;
      const float pw = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
      pv += pw * src.cv[qi].w;
      pk += pw;
    }
  }
  const float vt = pv / pk;
  const float l_den = k.sigma_l * sqrtf(vt) + 1e-12f;
  float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + s * dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + s * dx;
      if (qx < 0 || qx >= W) continue;
      const float hk = b3(dy) * b3(dx);
      float w = hk;
      F4 q = P.cv;
      if (dy != 0 || dx != 0) {
        const Pix Q = src.pix(k, qy, qx);
        w = tap_weight(k, hk, lum_p, l_den, P, p_surf, Q);
        q = Q.cv;
      }
      sw += w;
      sr += w * q.x;
      sg += w * q.y;
      sb += w * q.z;
      sv += (w * w) * q.w;
    }
  }
  return F4{sr / sw, sg / sw, sb / sw, sv / (sw * sw)};
}

// The CPU loop (wr_denoise.cpp): arguments already checked (wr_film_denoise).
void denoise_host(const float* film, const float* film_sq, int width, int height, int n_passes, const float* normal,
                  const float* position, const float* albedo, const wr_denoise_params& p, float* out);

#if defined(__HIPCC__)
// ------------------------------------------------------------------ gfx950
// One thread per pixel; a block of 256 threads covers a 16 x 16 pixel tile, each
// of its four waves an 8 x 8 quarter.  A grid smaller than the tile count
// strides over the tiles.
constexpr int kTile = 16, kBlock = kTile * kTile;
// Steps up to this one stage the tile and its halo of 2 s pixels in LDS (s = 2:
// 24 x 24 records of up to 64 bytes, 36 KiB); larger steps read their 25 taps
// straight from memory (16-byte loads; the planes of a 1080p film fit in the L2
// and Infinity Cache).
#ifndef WR_DN_LDS_MAX_STEP
#define WR_DN_LDS_MAX_STEP 2
#endif
inline size_t lds_bytes(int s) {  // four planes of (16 + 4 s)^2 words
  const int r = kTile + 4 * s;
  return size_t(r) * r * sizeof(F4) * 4;
}

__global__ void __launch_bounds__(256) k_dn_prepare(const float* __restrict__ film, const float* __restrict__ film_sq,
                                                    const float* __restrict__ normal,
                                                    const float* __restrict__ position,
                                                    const float* __restrict__ albedo, int npix, int passes,
                                                    F4* __restrict__ cv, F4* __restrict__ g0, F4* __restrict__ g1,
                                                    F4* __restrict__ g2) {
  const double n = static_cast<double>(passes);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
    const size_t o = 3 * static_cast<size_t>(i);
    st4(cv + i, input(film + o, film_sq + o, n));
    if (g0) {
      F4 a, b, c;
      pack_guides(normal ? normal + o : nullptr, position ? position + o : nullptr, albedo ? albedo + o : nullptr, &a,
                  &b, &c);
      st4(g0 + i, a);
      st4(g1 + i, b);
      st4(g2 + i, c);
    }
  }
}

// One level.  LDS: the tile + halo is staged first (every address checked
// against the image before it is formed; in-image taps lie inside the halo by
// construction).  LAST: writes out = c * scale (3 floats per pixel) instead of
// the next (c, v).
template <bool LDS, bool LAST>
__global__ void __launch_bounds__(kBlock) k_dn_level(View img, Cfg k, int W, int H, int s, F4* __restrict__ dst,
                                                     float* __restrict__ out, float scale) {
  extern __shared__ F4 dn_lds[];
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int lx = (wave & 1) * 8 + (lane & 7), ly = (wave >> 1) * 8 + (lane >> 3);
  for (int tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
    const int x0 = (tile % tiles_x) * kTile, y0 = (tile / tiles_x) * kTile;
    const int x = x0 + lx, y = y0 + ly;
    View src = img;
    if (LDS) {
      const int r = kTile + 4 * s, n = r * r;
      F4* l_cv = dn_lds;
      F4* l_g0 = dn_lds + n;
      F4* l_g1 = dn_lds + 2 * n;
      F4* l_g2 = dn_lds + 3 * n;
      const bool need_g1 = (k.has_n && k.has_p) || k.has_a;
      for (int i = t; i < n; i += kBlock) {
        const int gy = y0 - 2 * s + i / r, gx = x0 - 2 * s + i % r;
        if (gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
        const int gi = gy * W + gx;
        st4(l_cv + i, ld4(img.cv + gi));
        if (k.has_n) st4(l_g0 + i, ld4(img.g0 + gi));
        if (need_g1) st4(l_g1 + i, ld4(img.g1 + gi));
        if (k.has_a) st4(l_g2 + i, ld4(img.g2 + gi));
      }
      __syncthreads();
      src = View{l_cv, l_g0, l_g1, l_g2, y0 - 2 * s, x0 - 2 * s, r};
    }
    if (x < W && y < H) {
      const F4 o = pixel(src, k, x, y, W, H, s);
      const int i = y * W + x;
      if (LAST) {
        const size_t j = 3 * static_cast<size_t>(i);
        out[j] = o.x * scale;
        out[j + 1] = o.y * scale;
        out[j + 2] = o.z * scale;
      } else {
        st4(dst + i, o);
      }
    }
    if (LDS) __syncthreads();  // before the next tile is staged
  }
}
#endif  // __HIPCC__

}  // namespace dn
