// ctypes shim over csrc/host_dense.cpp for tests/test_dense_host.py (compiled with g++, no HIP).
#include "host_dense.hpp"

#include <algorithm>
#include <vector>

using namespace edigpu;

extern "C" {

// d[n]: diagonal in, eigenvalues out; e[n]: sub-diagonal in e[1..n-1] (e[0] unused); z[n*n] out as tql2 leaves it
int hd_tql2(int n, double* d, const double* e, double* z) {
  std::vector<double> dv(d, d + n), ev(e, e + n), zv;
  const int rc = tql2(n, dv, ev, zv);
  std::copy(dv.begin(), dv.end(), d);
  std::copy(zv.begin(), zv.end(), z);
  return rc;
}

// a[n*n]: row-major symmetric matrix; w[n], z[n*n] out as jacobi_eigh leaves them
void hd_jacobi_eigh(int n, const double* a, double* w, double* z) {
  std::vector<double> av(a, a + (size_t)n * n), wv, zv;
  jacobi_eigh(n, av, wv, zv);
  std::copy(wv.begin(), wv.end(), w);
  std::copy(zv.begin(), zv.end(), z);
}

}  // extern "C"
