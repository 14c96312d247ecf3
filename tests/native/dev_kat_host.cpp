// Host half of libwr_devkat.so (test infrastructure): csrc/wr_libm.h compiled
// by g++ with the flags of tests/test_libm.py (-O2 -ffp-contract=off), the
// build that tests/native/libm_check.c pins to glibc bit for bit.  The GPU
// test compares the device's results with these.
#include <cstdint>

#include "wr_libm.h"

void dk_libm_host(int op, int64_t n, const float* x, const float* y, float* out, float* out2) {
  for (int64_t i = 0; i < n; ++i) {
    if (op == 0) {
      out[i] = wr_sinf(x[i]);
    } else if (op == 1) {
      out[i] = wr_cosf(x[i]);
    } else if (op == 2) {
      wr_sincosf(x[i], &out[i], &out2[i]);
    } else {
      out[i] = wr_powf(x[i], y[i]);
    }
  }
}
