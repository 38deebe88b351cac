// edigpu_trl.hip -- the thick-restart Lanczos eigensolver (trl_solve) and edigpu_lanczos_eigh_multi; the sharded entry
// point (edigpu_shard.hip) runs the same solver.
#include <algorithm>
#include <cmath>
#include <vector>

#include "host_dense.hpp"
#include "kernels.hpp"

namespace edigpu {

// Thick-restart Lanczos with full re-orthogonalisation: the lowest `neigen` eigenpairs from an
// ncv-dimensional basis -- the job the reference gives to ARPACK (sp_eigh, ED_NORMAL/ED_DIAG_NORMAL.f90:179-196; with
// MpiComm, :221-242, to PARPACK).  One routine for whole sectors and for shards: `n` elements (`len` doubles) of every
// vector live on this rank, ops.apply is the product on them, ops.allreduce sums small device buffers over the ranks
// (empty: a single rank).  Every decision is taken from all-reduced numbers, so the ranks stay in step.

int trl_solve(int device, hipStream_t st, int cplx, int64_t n, int64_t len, int64_t nglobal, const TrlOps& ops, int neigen, int ncv,
              double tol, int maxrestart, const double* v0, uint64_t seed_offset, double* evals, double* evecs,
              int* nconv_out, int* nmatvec_out) {
  EDIGPU_HIP(hipSetDevice(device));
  const LoopSwitches lz = LoopSwitches::sample();
  const bool multi = (bool)ops.allreduce;
  auto reduce = [&](double* dev, size_t cnt) -> int { return multi ? ops.allreduce(dev, cnt, st) : 0; };
  if ((int64_t)neigen > nglobal) neigen = (int)nglobal;
  int m = ncv > 0 ? ncv : std::max(2 * neigen + 10, 20);
  if (m < neigen + 2) m = neigen + 2;
  if (m > 128) m = 128;
  if ((int64_t)m > nglobal) m = (int)nglobal;
  if (tol <= 0.0) tol = 1e-12;
  if (maxrestart <= 0) maxrestart = 300;
  const size_t vbytes = (size_t)len * sizeof(double);
  struct Bufs {
    double *Q = nullptr, *Qt = nullptr, *h = nullptr, *part = nullptr, *Y = nullptr;
    ~Bufs() { (void)hipFree(Q); (void)hipFree(Qt); (void)hipFree(h); (void)hipFree(part); (void)hipFree(Y); }
  } b;
  EDIGPU_HIP(hipMalloc((void**)&b.Q, vbytes * (size_t)(m + 1)));
  EDIGPU_HIP(hipMalloc((void**)&b.h, sizeof(double) * 2 * (size_t)(m + 40)));
  EDIGPU_HIP(hipMalloc((void**)&b.part, sizeof(double) * (size_t)trl_partial_doubles()));
  EDIGPU_HIP(hipMalloc((void**)&b.Y, sizeof(double) * (size_t)m * m));
  auto q = [&](int j) { return b.Q + (size_t)j * len; };
  std::vector<double> hh(2 * (size_t)(m + 40));
  auto norm_of = [&](double* w, double& out) -> int {
    if (trl_norm2(cplx, n, w, b.h, b.part, st) || reduce(b.h, 2)) return 1;
    EDIGPU_HIP(hipMemcpyAsync(hh.data(), b.h, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    EDIGPU_HIP(hipStreamSynchronize(st));
    out = sqrt(std::max(hh[0], 0.0));
    return 0;
  };
  // start vector
  if (v0) {
    EDIGPU_HIP(hipMemcpyAsync(q(0), v0, vbytes, hipMemcpyDefault, st));
  } else if (lz_fill_random(q(0), len, 0x7e57ab1eull + seed_offset, st)) {
    return 1;
  }
  double nrm = 0.0;
  if (norm_of(q(0), nrm)) return 1;
  if (nrm == 0.0) {
    set_error("edigpu_lanczos_eigh_multi: zero start vector");
    return 1;
  }
  if (trl_scale(len, q(0), 1.0 / nrm, st)) return 1;

  std::vector<double> T((size_t)m * m, 0.0), Tw, theta, Y;
  int k = 0, meff = m, nmv = 0, nconv = 0, stalled = 0;
  double beta_last = 0.0, best_worst = 1e300;
  bool invariant = false;
  // per cycle the Gram-Schmidt coefficients (two passes) and the squared norms stay on the device and are
  // fetched once: no host synchronisation inside the Lanczos steps
  const size_t hstride = 2 * (size_t)(m + 40);
  double *d_coef = nullptr, *d_nrm = nullptr;
  EDIGPU_HIP(hipMalloc((void**)&d_coef, sizeof(double) * 2 * hstride * (size_t)m));
  EDIGPU_HIP(hipMalloc((void**)&d_nrm, sizeof(double) * (2 * (size_t)m + 80)));  // the reduction writes 2 * kTrlNC slots
  struct Free2 {
    double *&a, *&b;
    ~Free2() { (void)hipFree(a); (void)hipFree(b); }
  } free2{d_coef, d_nrm};
  std::vector<double> hcoef(2 * hstride * (size_t)m), hnrm(2 * (size_t)m + 80);
  // Classical Gram-Schmidt twice on every step (CGS2).  The variant that skips the second pass when the first one
  // removed little (LoopSwitches::trl_onepass, criterion |w_new|^2 >= 0.5 |w_old|^2) saves up to half the basis traffic
  // but was found to let the restart vector drift out of orthogonality (2e-13 after the first cycle with the
  // earlier 1 % criterion, x1000 per restart: Ritz values below the spectrum after five restarts on a 36-dimensional
  // sector), so it is not the default.
  const bool twopass = !lz.trl_onepass;
  // LoopSwitches::trl_full: full CGS2 on every step (the round-2 solver)
  const bool selective = !lz.trl_full && !lz.trl_onepass;
  constexpr double kSelThr = 1e-14;
  // coefficients below thr_skip * |w_new| are left in w: three orders below the requested residual
  const double thr_skip = lz.trl_thr.value_or(1e-3 * tol);
  int* d_skip = nullptr;
  EDIGPU_HIP(hipMalloc((void**)&d_skip, sizeof(int)));
  struct Free1 {
    int*& p;
    ~Free1() { (void)hipFree(p); }
  } free1{d_skip};
  for (int restart = 0; restart <= maxrestart; restart++) {
    invariant = false;
    meff = m;
    EDIGPU_HIP(hipMemsetAsync(d_coef, 0, sizeof(double) * 2 * hstride * (size_t)m, st));
    for (int j = k; j < m; j++) {
      double* w = q(j + 1);
      if (ops.apply(q(j), w, st)) return 1;
      nmv++;
      // classical Gram-Schmidt against q_0..q_j, twice; the coefficients are column j of Q^H H Q
      double* c1 = d_coef + (size_t)(2 * j) * hstride;
      double* c2 = d_coef + (size_t)(2 * j + 1) * hstride;
      // second pass only when the first one removed more than 99 % of |w|^2 ("twice is enough" with eta = 0.1:
      // orthogonality ~10 eps otherwise); decided on the device, c2 stays zero when skipped
      // coefficients below 1e-11 |w_new| (pure rounding: the three-term recurrence makes them zero) are not
      // subtracted, their basis vectors not read (trl_decide_kernel)
      if (selective && j > k) {
        // Selective re-orthogonalisation (every step but the first after a restart).  Pass A: classical Gram-Schmidt
        // against the two vectors the three-term recurrence couples to, q_(j-1) and q_j -- the only directions in
        // which a large component is removed and cancellation can leave an error.  Pass B: the dots against the WHOLE
        // basis (for those two the second of "twice is enough", for all others a first pass on components that are
        // small next to |w|: one pass is accurate), and only the coefficients above kSelThr |w| are subtracted: what
        // is skipped leaves an orthogonality error of that size (1e-14), the basis vectors of zero coefficients are
        // not read.  ~j + 13 vector passes per step instead of the 4 (j + 1) of the full CGS2 it replaces.
        const int nl = std::min(2, j + 1), l0 = j + 1 - nl;
        if (trl_dots(cplx, n, nl, q(l0), len, w, c1 + 2 * l0, b.part, st) || reduce(c1 + 2 * l0, 2 * (size_t)nl) ||
            trl_subtract(cplx, n, nl, q(l0), len, c1 + 2 * l0, w, st))
          return 1;
        if (trl_dots(cplx, n, j + 2, b.Q, len, w, c2, b.part, st) || reduce(c2, 2 * (size_t)(j + 2)) ||
            trl_filter(c2, j + 1, kSelThr * kSelThr, st) || trl_subtract(cplx, n, j + 1, b.Q, len, c2, w, st))
          return 1;
      } else if (twopass || multi) {
        // (shards: the coefficients Q^H w are summed over the ranks between the dots and the subtraction -- one
        // all-reduce of j + 1 numbers per pass, the k-element reduce of SciFortran's MPI Lanczos)
        if (trl_dots(cplx, n, j + 1, b.Q, len, w, c1, b.part, st) || reduce(c1, 2 * (size_t)(j + 1)) ||
            trl_subtract(cplx, n, j + 1, b.Q, len, c1, w, st))
          return 1;
        if (trl_dots(cplx, n, j + 1, b.Q, len, w, c2, b.part, st) || reduce(c2, 2 * (size_t)(j + 1)) ||
            trl_subtract(cplx, n, j + 1, b.Q, len, c2, w, st))
          return 1;
      } else {
        if (trl_dots(cplx, n, j + 2, b.Q, len, w, c1, b.part, st)) return 1;  // column j+1 is w itself: <w|w>
        if (trl_decide(c1, j + 1, 0.5, thr_skip * thr_skip, b.h, d_skip, st)) return 1;
        if (trl_subtract(cplx, n, j + 1, b.Q, len, b.h, w, st)) return 1;
        if (trl_orthogonalize(cplx, n, j + 1, b.Q, len, w, c2, b.part, st, d_skip)) return 1;
      }
      if (trl_norm2(cplx, n, w, d_nrm + 2 * j, b.part, st) || reduce(d_nrm + 2 * j, 2)) return 1;
      if (vec_scale(len, w, d_nrm + 2 * j, st)) return 1;  // w / sqrt(<w|w>) with the norm read on the device
    }
    EDIGPU_HIP(hipMemcpyAsync(hcoef.data(), d_coef, sizeof(double) * hcoef.size(), hipMemcpyDeviceToHost, st));
    EDIGPU_HIP(hipMemcpyAsync(hnrm.data(), d_nrm, sizeof(double) * hnrm.size(), hipMemcpyDeviceToHost, st));
    EDIGPU_HIP(hipStreamSynchronize(st));
    for (int j = k; j < m; j++) {
      const double* c1 = &hcoef[(size_t)(2 * j) * hstride];
      const double* c2 = &hcoef[(size_t)(2 * j + 1) * hstride];
      for (int i = 0; i <= j; i++) {
        T[(size_t)i * m + j] = c1[2 * i] + c2[2 * i];
        T[(size_t)j * m + i] = T[(size_t)i * m + j];
      }
      const double beta = sqrt(std::max(hnrm[2 * j], 0.0));
      beta_last = beta;
      const double scale = fabs(T[(size_t)j * m + j]) + 1.0;
      if (!(beta > 1e-13 * scale)) {  // invariant subspace: q_0..q_j is closed under H (later steps are discarded)
        meff = j + 1;
        invariant = true;
        break;
      }
    }
    // Rayleigh-Ritz on the meff x meff projection
    Tw.assign((size_t)meff * meff, 0.0);
    for (int i = 0; i < meff; i++)
      for (int j = 0; j < meff; j++) Tw[(size_t)i * meff + j] = T[(size_t)i * m + j];
    jacobi_eigh(meff, Tw, theta, Y);
    const int want = std::min(neigen, meff);
    if (lz.trl_debug) {
      fprintf(stderr, "trl: restart %d k %d meff %d invariant %d beta_last %.3e theta0 %.6e\n  beta:", restart, k, meff,
              (int)invariant, beta_last, theta.empty() ? 0.0 : theta[0]);
      for (int j = k; j < meff; j++) fprintf(stderr, " %.2e", sqrt(std::max(hnrm[2 * j], 0.0)));
      if (!cplx && n <= 4096) {  // orthonormality of the basis q_0..q_meff
        std::vector<double> hq((size_t)(meff + 1) * len);
        EDIGPU_HIP(hipMemcpy(hq.data(), b.Q, hq.size() * sizeof(double), hipMemcpyDeviceToHost));
        double dev = 0.0;
        int wi = 0, wj = 0;
        for (int i = 0; i <= meff; i++)
          for (int j2 = 0; j2 <= i; j2++) {
            double d = 0.0;
            for (int64_t e = 0; e < n; e++) d += hq[(size_t)i * len + e] * hq[(size_t)j2 * len + e];
            d = fabs(d - (i == j2 ? 1.0 : 0.0));
            if (d > dev) dev = d, wi = i, wj = j2;
          }
        fprintf(stderr, "\n  |Q^T Q - 1| max %.2e at (%d,%d)", dev, wi, wj);
      }
      fprintf(stderr, "\n  theta / res:");
      for (int i = 0; i < std::min(meff, 6); i++)
        fprintf(stderr, " %.12f / %.1e", theta[i], fabs(beta_last * Y[(size_t)(meff - 1) * meff + i]));
      fprintf(stderr, "\n");
    }
    nconv = 0;
    bool counting = true;
    double worst = 0.0;  // largest relative residual among the wanted pairs
    for (int i = 0; i < want; i++) {
      const double res = invariant ? 0.0 : fabs(beta_last * Y[(size_t)(meff - 1) * meff + i]);
      const double rel = res / std::max(fabs(theta[i]), 1.0);
      worst = std::max(worst, rel);
      if (counting && rel <= tol) nconv++;
      else counting = false;
    }
    if (nconv >= want || invariant || restart == maxrestart) break;
    // A tolerance below what rounding allows (the reference's default lanc_tolerance is 1e-18) is never met: the
    // residuals fall to ~1e-13 |H|, and further restarts only feed rounding noise back into the basis (measured: they
    // grow by ~3x per restart from there and the Ritz values are lost after ~30).  Stop once the wanted residuals are at
    // rounding level and two restarts in a row have not improved on the best seen; nconv then reports what meets tol.
    if (worst < best_worst) {
      best_worst = worst;
      stalled = 0;
    } else if (best_worst <= 1e-8 && ++stalled >= 2) {
      break;
    }
    // thick restart: keep the wanted Ritz vectors plus half of the rest, then the residual vector
    int kk = want + (meff - want) / 2;
    if (kk > meff - 1) kk = meff - 1;
    if (kk < 1) kk = 1;
    // the rotated Ritz vectors land in the second basis buffer, the residual vector follows them there, and the
    // two buffers change roles (no copy back)
    if (!b.Qt) EDIGPU_HIP(hipMalloc((void**)&b.Qt, vbytes * (size_t)(m + 1)));
    EDIGPU_HIP(hipMemcpyAsync(b.Y, Y.data(), sizeof(double) * (size_t)meff * meff, hipMemcpyHostToDevice, st));
    if (trl_rotate_basis(len, meff, kk, b.Q, len, b.Y, meff, b.Qt, len, st)) return 1;
    EDIGPU_HIP(hipMemcpyAsync(b.Qt + (size_t)kk * len, q(meff), vbytes, hipMemcpyDeviceToDevice, st));
    std::swap(b.Q, b.Qt);
    std::fill(T.begin(), T.end(), 0.0);
    for (int i = 0; i < kk; i++) T[(size_t)i * m + i] = theta[i];
    k = kk;
  }
  const int want = std::min(neigen, meff);
  for (int i = 0; i < neigen; i++) evals[i] = i < want ? theta[i] : 0.0;
  if (nconv_out) *nconv_out = nconv;
  if (nmatvec_out) *nmatvec_out = nmv;
  if (evecs) {
    if (!b.Qt) EDIGPU_HIP(hipMalloc((void**)&b.Qt, vbytes * (size_t)(m + 1)));
    EDIGPU_HIP(hipMemcpyAsync(b.Y, Y.data(), sizeof(double) * (size_t)meff * meff, hipMemcpyHostToDevice, st));
    if (trl_rotate_basis(len, meff, want, b.Q, len, b.Y, meff, b.Qt, len, st)) return 1;
    EDIGPU_HIP(hipMemcpyAsync(evecs, b.Qt, vbytes * (size_t)want, hipMemcpyDefault, st));
  }
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_lanczos_eigh_multi(edigpu_handle s, int neigen, int ncv, double tol, int maxrestart, const double* v0,
                              double* evals, double* evecs, int* nconv_out, int* nmatvec_out) {
  if (!s || !evals || neigen <= 0) {
    set_error("edigpu_lanczos_eigh_multi: bad argument");
    return 1;
  }
  if (single_shard(s, "edigpu_lanczos_eigh_multi")) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ensure_workspace(s)) return 1;
  TrlOps ops;
  ops.apply = [s](const double* in, double* out, hipStream_t st) { return apply_any(s, in, in, out, 3, st); };
  return trl_solve(s->device, s->stream, s->is_complex, s->nloc, s->ws_len, s->nloc, ops, neigen, ncv, tol, maxrestart, v0, 0, evals,
                   evecs, nconv_out, nmatvec_out);
}

}  // extern "C"
