// host_dense.cpp -- the small dense eigensolvers behind every eigenvalue the library returns (host_dense.hpp).
#include "host_dense.hpp"

#include <algorithm>
#include <cmath>

namespace edigpu {

// symmetric tridiagonal eigen-decomposition (implicit QL).  d: diagonal (n), e: sub-diagonal
// e[1..n-1] (e[0] unused).  On return d holds eigenvalues, z (n*n, column-major) eigenvectors.
int tql2(int n, std::vector<double>& d, std::vector<double>& e, std::vector<double>& z) {
  z.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) z[(size_t)i * n + i] = 1.0;
  for (int i = 1; i < n; i++) e[i - 1] = e[i];
  if (n > 0) e[n - 1] = 0.0;
  for (int l = 0; l < n; l++) {
    int iter = 0, m;
    do {
      for (m = l; m < n - 1; m++) {
        const double dd = fabs(d[m]) + fabs(d[m + 1]);
        if (fabs(e[m]) <= 2.3e-16 * dd) break;
      }
      if (m != l) {
        if (iter++ == 200) return 1;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = hypot(g, 1.0);
        g = d[m] - d[l] + e[l] / (g + (g >= 0 ? fabs(r) : -fabs(r)));
        double sn = 1.0, c = 1.0, p = 0.0;
        int i;
        for (i = m - 1; i >= l; i--) {
          double f = sn * e[i], b = c * e[i];
          e[i + 1] = (r = hypot(f, g));
          if (r == 0.0) {
            d[i + 1] -= p;
            e[m] = 0.0;
            break;
          }
          sn = f / r;
          c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * sn + 2.0 * c * b;
          d[i + 1] = g + (p = sn * r);
          g = c * r - b;
          for (int k = 0; k < n; k++) {
            f = z[(size_t)(i + 1) * n + k];
            z[(size_t)(i + 1) * n + k] = sn * z[(size_t)i * n + k] + c * f;
            z[(size_t)i * n + k] = c * z[(size_t)i * n + k] - sn * f;
          }
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p;
        e[l] = g;
        e[m] = 0.0;
      }
    } while (m != l);
  }
  return 0;
}

// cyclic Jacobi for a small dense symmetric matrix (row-major n x n, destroyed); eigenvalues ascending in
// w, eigenvectors in the COLUMNS of z (row-major n x n)
void jacobi_eigh(int n, std::vector<double>& a, std::vector<double>& w, std::vector<double>& z) {
  z.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) z[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; i++) {
      diag += a[(size_t)i * n + i] * a[(size_t)i * n + i];
      for (int j = i + 1; j < n; j++) off += a[(size_t)i * n + j] * a[(size_t)i * n + j];
    }
    if (off <= 1e-32 * (diag + off) || off == 0.0) break;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < n; k++) {
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - sn * akq;
          a[(size_t)k * n + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - sn * aqk;
          a[(size_t)q * n + k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < n; k++) {
          const double zkp = z[(size_t)k * n + p], zkq = z[(size_t)k * n + q];
          z[(size_t)k * n + p] = c * zkp - sn * zkq;
          z[(size_t)k * n + q] = sn * zkp + c * zkq;
        }
      }
  }
  std::vector<int> ord(n);
  for (int i = 0; i < n; i++) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](int i, int j) { return a[(size_t)i * n + i] < a[(size_t)j * n + j]; });
  w.resize(n);
  std::vector<double> zs((size_t)n * n);
  for (int c = 0; c < n; c++) {
    w[c] = a[(size_t)ord[c] * n + ord[c]];
    for (int k = 0; k < n; k++) zs[(size_t)k * n + c] = z[(size_t)k * n + ord[c]];
  }
  z.swap(zs);
}

}  // namespace edigpu
