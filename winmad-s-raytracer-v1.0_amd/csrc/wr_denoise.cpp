// wr_film_denoise on host films: the filter of wr_denoise.h as a plain CPU loop
// (no HIP in this translation unit; the device path runs the same dn::pixel()).
#include "wr_denoise.h"

#include <utility>
#include <vector>

namespace dn {

void denoise_host(const float* film, const float* film_sq, int width, int height, int n_passes, const float* normal,
                  const float* position, const float* albedo, const wr_denoise_params& p, float* out) {
  const int W = width, H = height;
  const size_t npix = size_t(W) * H;
  const Cfg k{p.sigma_l, p.sigma_p, p.sigma_a, p.normal_power, normal != nullptr, position != nullptr,
              albedo != nullptr};
  std::vector<F4> a(npix), b(npix), g0, g1, g2;
  const bool guides = normal || position || albedo;
  if (guides) g0.resize(npix), g1.resize(npix), g2.resize(npix);
  const double n = static_cast<double>(n_passes);
  for (size_t i = 0; i < npix; ++i) {
    a[i] = input(film + 3 * i, film_sq + 3 * i, n);
    if (guides)
      pack_guides(normal ? normal + 3 * i : nullptr, position ? position + 3 * i : nullptr,
                  albedo ? albedo + 3 * i : nullptr, &g0[i], &g1[i], &g2[i]);
  }
  for (int t = 0; t < p.levels; ++t) {
    const View src{a.data(), g0.data(), g1.data(), g2.data(), 0, 0, W};
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) b[size_t(y) * W + x] = pixel(src, k, x, y, W, H, 1 << t);
    std::swap(a, b);
  }
  const float scale = static_cast<float>(n_passes);
  for (size_t i = 0; i < npix; ++i) {
    out[3 * i] = a[i].x * scale;
    out[3 * i + 1] = a[i].y * scale;
    out[3 * i + 2] = a[i].z * scale;
  }
}

}  // namespace dn
