// Stand-alone check of the film denoiser's CPU loop (csrc/wr_denoise.cpp), built
// by tests/test_denoise_host.py with -fsanitize=address,undefined: runs the
// cases the test wrote and compares each result, bit for bit, with the output
// of the library's own (unsanitized) build stored in the same file.
//
//   denoise_check <case file>...
// A case file: int32 {W, H, n_passes, has_normal, has_position, has_albedo,
// levels, normal_power}, float {sigma_l, sigma_p, sigma_a}, then float arrays of
// 3 W H values each: film, film_sq, the guides that exist, the expected output.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wr_denoise.h"

namespace {
bool read_floats(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(float), n, f) == n;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <case file>...\n", argv[0]);
    return 2;
  }
  int bad = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* f = std::fopen(argv[a], "rb");
    int32_t h[8];
    float sig[3];
    if (!f || std::fread(h, sizeof h, 1, f) != 1 || std::fread(sig, sizeof sig, 1, f) != 1) {
      std::printf("FAIL %s: unreadable\n", argv[a]);
      return 1;
    }
    const int W = h[0], H = h[1], n = h[2];
    const size_t nf = size_t(3) * W * H;
    std::vector<float> S, Q, N, P, A, want;
    bool ok = read_floats(f, S, nf) && read_floats(f, Q, nf);
    if (h[3]) ok = ok && read_floats(f, N, nf);
    if (h[4]) ok = ok && read_floats(f, P, nf);
    if (h[5]) ok = ok && read_floats(f, A, nf);
    ok = ok && read_floats(f, want, nf);
    std::fclose(f);
    if (!ok) {
      std::printf("FAIL %s: truncated\n", argv[a]);
      return 1;
    }
    const wr_denoise_params p{h[6], h[7], sig[0], sig[1], sig[2]};
    if (const char* why = dn::check_params(p)) {
      std::printf("FAIL %s: %s\n", argv[a], why);
      return 1;
    }
    std::vector<float> out(nf, -1.f);
    dn::denoise_host(S.data(), Q.data(), W, H, n, h[3] ? N.data() : nullptr, h[4] ? P.data() : nullptr,
                     h[5] ? A.data() : nullptr, p, out.data());
    size_t diff = 0;
    for (size_t i = 0; i < nf; ++i) diff += std::memcmp(&out[i], &want[i], sizeof(float)) != 0;
    if (diff) {
      std::printf("FAIL %s: %zu of %zu values differ from the library's\n", argv[a], diff, nf);
      ++bad;
    }
  }
  if (bad) return 1;
  std::printf("OK %d cases\n", argc - 1);
  return 0;
}
