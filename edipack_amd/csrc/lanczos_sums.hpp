// lanczos_sums.hpp -- alpha and beta of one step of the one-reduction Lanczos recurrence from its three sums: the one
// definition, as device code (kernels_shard.hip, lz_finalize.hpp) and as plain host C++ (sharded_tridiag in
// edigpu_shard.hip; tests/test_shard_sums_host.py compiles it with g++).  No HIP include.
//
// Per step the sums are T = (<v|w>, sum (w - sg v)^2, <v|v>), sg = alpha of the previous step (0 on the first).
// alpha = T[0] and beta^2 = |w - alpha v|^2 = T[1] - 2 d (alpha - sg T[2]) + d^2 T[2], d = alpha - sg -- an identity (no
// |v| = 1 assumed), well conditioned for spectra far from zero.  A fixed sequence of double operations: the library is
// built without contraction into fused multiply-adds, so host and device give the same bits.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define EDIGPU_HD __host__ __device__
#else
#define EDIGPU_HD
#endif

namespace edigpu {

EDIGPU_HD inline double beta2_from_sums(double alpha, double qq, double vv, double sg) {
  const double d = alpha - sg;
  return qq - 2.0 * d * (alpha - sg * vv) + d * d * vv;
}

// rounding may leave a tiny negative beta^2: that is beta = 0
EDIGPU_HD inline double beta_from_beta2(double b2) { return sqrt(b2 > 0.0 ? b2 : 0.0); }

// t / tprev: the sums of this step and of the one before it (null on the first step)
EDIGPU_HD inline void ab_from_sums(const double* __restrict__ t, const double* __restrict__ tprev, double& a, double& b) {
  const double sg = tprev ? tprev[0] : 0.0;
  a = t[0];
  b = beta_from_beta2(beta2_from_sums(a, t[1], t[2], sg));
}

}  // namespace edigpu
