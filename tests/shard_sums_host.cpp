// Host shim of tests/test_shard_sums_host.py: csrc/lanczos_sums.hpp compiled as plain C++ (no HIP), and the same
// identity evaluated in long double as the reference.
#include <cmath>

#include "lanczos_sums.hpp"

extern "C" {

// what the kernels and sharded_tridiag compute; tprev may be null (first step)
void ss_ab_from_sums(const double* t, const double* tprev, double* a, double* b) { edigpu::ab_from_sums(t, tprev, *a, *b); }
double ss_beta2_from_sums(double alpha, double qq, double vv, double sg) { return edigpu::beta2_from_sums(alpha, qq, vv, sg); }
double ss_beta_from_beta2(double b2) { return edigpu::beta_from_beta2(b2); }

static long double ref_beta2(double alpha, double qq, double vv, double sg) {
  const long double a = alpha, s = sg, q = qq, v = vv, d = a - s;
  return q - 2.0L * d * (a - s * v) + d * d * v;
}

// the reference's beta^2 rounded to double (its sign is what the clamp case looks at)
double ss_ref_beta2(double alpha, double qq, double vv, double sg) { return (double)ref_beta2(alpha, qq, vv, sg); }

// |x - ref| / |ref| in long double, for x = a beta^2 and for x = a beta
double ss_relerr_beta2(double x, double alpha, double qq, double vv, double sg) {
  const long double r = ref_beta2(alpha, qq, vv, sg);
  return (double)(fabsl((long double)x - r) / fabsl(r));
}
double ss_relerr_beta(double x, double alpha, double qq, double vv, double sg) {
  const long double r = sqrtl(ref_beta2(alpha, qq, vv, sg));
  return (double)(fabsl((long double)x - r) / r);
}

}  // extern "C"
