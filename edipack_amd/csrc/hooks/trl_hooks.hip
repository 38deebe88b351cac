// trl_hooks.hip -- test hooks of the thick-restart eigensolver's multi-vector kernels (kernels_trl.hip).
//
// Each hook takes host buffers given as pointer + length in doubles, uploads every buffer WHOLE, calls one launcher of
// kernels.hpp as the solver does (trl_solve, edigpu_trl.hip) on the calling thread's current device, and downloads every
// buffer the launcher may write, whole again: a test that surrounds its payload with sentinels sees every write.
// No kernel lives here; the arguments are checked before the device is touched.
#include "hook_util.hpp"

namespace edigpu {
namespace {

constexpr int kGroup = 16;  // kTrlNC (kernels_trl.hip): basis vectors per launch; trl_msum writes 2 * kGroup slots per group

// columns 0 .. ncol-1 of `len` doubles at leading dimension ld inside a buffer of `total` doubles
const char* bad_matrix(const double* p, int ncol, int64_t ld, int64_t total, int64_t len) {
  if (!p) return "null matrix";
  if (ncol < 1 || ld < 0 || total < 0 || len < 1) return "negative or zero size";
  if (ncol > 1 && ld < len) return "leading dimension below the vector length";
  if (total < len || (ncol > 1 && (int64_t)(ncol - 1) > (total - len) / ld)) return "matrix buffer too short";
  return nullptr;
}

int64_t dots_slots(int ndot) { return (int64_t)2 * kGroup * ((ndot + kGroup - 1) / kGroup); }

}  // namespace
}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_trl_dots(int32_t cplx, int64_t n, int32_t ndot, const double* Q, int32_t ncol, int64_t ldq, int64_t qlen,
                    const double* w, int64_t wlen, int32_t w_col, double* h, int64_t hlen, int32_t skip) {
  const char* who = "edigpu_trl_dots";
  if (n < 1 || n > (INT64_MAX >> 2) || ndot < 1) return refuse(who, "negative or zero size");
  const int64_t len = cplx ? 2 * n : n;
  if (const char* m = bad_matrix(Q, ncol, ldq, qlen, len)) return refuse(who, m);
  if (ndot > ncol) return refuse(who, "more dots than columns");
  if (w_col >= ncol) return refuse(who, "w_col is not a column of Q");
  if (w_col < 0 && (!w || wlen < len)) return refuse(who, "w shorter than the vector length");
  if (!h || hlen < dots_slots(ndot)) return refuse(who, "h needs 2 * 16 * ceil(ndot / 16) doubles");
  if (skip < -1 || skip > 1) return refuse(who, "skip is -1, 0 or 1");
  if (need_device()) return 1;
  DevBuf dq, dw, dh, dp;
  DevInt ds;
  if (dq.up(Q, qlen) || (w_col < 0 && dw.up(w, wlen)) || dh.up(h, hlen) || dp.alloc((size_t)trl_partial_doubles()))
    return 1;
  if (skip >= 0 && ds.up(skip)) return 1;
  const double* wv = w_col < 0 ? dw.p : dq.p + (int64_t)w_col * ldq;
  if (trl_dots(cplx, n, ndot, dq.p, ldq, wv, dh.p, dp.p, nullptr, skip >= 0 ? ds.p : nullptr)) return 1;
  if (finish(who)) return 1;
  return dh.down(h);
}

int edigpu_trl_norm2(int32_t cplx, int64_t n, const double* w, int64_t wlen, double* h, int64_t hlen) {
  const char* who = "edigpu_trl_norm2";
  if (n < 1 || n > (INT64_MAX >> 2)) return refuse(who, "negative or zero size");
  const int64_t len = cplx ? 2 * n : n;
  if (!w || wlen < len) return refuse(who, "w shorter than the vector length");
  if (!h || hlen < dots_slots(1)) return refuse(who, "h needs 2 * 16 doubles");
  if (need_device()) return 1;
  DevBuf dw, dh, dp;
  if (dw.up(w, wlen) || dh.up(h, hlen) || dp.alloc((size_t)trl_partial_doubles())) return 1;
  if (trl_norm2(cplx, n, dw.p, dh.p, dp.p, nullptr)) return 1;
  if (finish(who)) return 1;
  return dh.down(h);
}

int edigpu_trl_subtract(int32_t cplx, int64_t n, int32_t nvec, const double* Q, int32_t ncol, int64_t ldq, int64_t qlen,
                        const double* h, int64_t hlen, double* w, int64_t wlen, int32_t skip) {
  const char* who = "edigpu_trl_subtract";
  if (n < 1 || n > (INT64_MAX >> 2) || nvec < 1) return refuse(who, "negative or zero size");
  const int64_t len = cplx ? 2 * n : n;
  if (const char* m = bad_matrix(Q, ncol, ldq, qlen, len)) return refuse(who, m);
  if (nvec > ncol) return refuse(who, "more coefficients than columns");
  if (!h || hlen < (int64_t)2 * nvec) return refuse(who, "h needs 2 * nvec doubles");
  if (!w || wlen < len) return refuse(who, "w shorter than the vector length");
  if (skip < -1 || skip > 1) return refuse(who, "skip is -1, 0 or 1");
  if (need_device()) return 1;
  DevBuf dq, dw, dh;
  DevInt ds;
  if (dq.up(Q, qlen) || dw.up(w, wlen) || dh.up(h, hlen)) return 1;
  if (skip >= 0 && ds.up(skip)) return 1;
  if (trl_subtract(cplx, n, nvec, dq.p, ldq, dh.p, dw.p, nullptr, skip >= 0 ? ds.p : nullptr)) return 1;
  if (finish(who)) return 1;
  return dw.down(w);
}

int edigpu_trl_decide(const double* h, int64_t hlen, int32_t nvec, double eta2, double thr2, double* hf, int64_t hflen,
                      int32_t* skip) {
  const char* who = "edigpu_trl_decide";
  if (nvec < 1) return refuse(who, "negative or zero size");
  if (!h || hlen < (int64_t)2 * nvec + 2) return refuse(who, "h needs 2 * nvec + 2 doubles");
  if (!hf || hflen < (int64_t)2 * nvec) return refuse(who, "hf needs 2 * nvec doubles");
  if (!skip) return refuse(who, "null skip");
  if (need_device()) return 1;
  DevBuf dh, df;
  DevInt ds;
  if (dh.up(h, hlen) || df.up(hf, hflen) || ds.up(*skip)) return 1;
  if (trl_decide(dh.p, nvec, eta2, thr2, df.p, ds.p, nullptr)) return 1;
  if (finish(who)) return 1;
  int s = 0;
  if (df.down(hf) || ds.down(&s)) return 1;
  *skip = s;
  return 0;
}

int edigpu_trl_filter(double* h, int64_t hlen, int32_t nvec, double thr2) {
  const char* who = "edigpu_trl_filter";
  if (nvec < 1) return refuse(who, "negative or zero size");
  if (!h || hlen < (int64_t)2 * nvec + 2) return refuse(who, "h needs 2 * nvec + 2 doubles");
  if (need_device()) return 1;
  DevBuf dh;
  if (dh.up(h, hlen)) return 1;
  if (trl_filter(dh.p, nvec, thr2, nullptr)) return 1;
  if (finish(who)) return 1;
  return dh.down(h);
}

int edigpu_trl_rotate(int64_t len, int32_t m, int32_t k, const double* Q, int64_t ldq, int64_t qlen, const double* Y,
                      int32_t ldy, int64_t ylen, double* out, int64_t ldo, int64_t olen) {
  const char* who = "edigpu_trl_rotate";
  if (len < 1 || m < 1 || k < 1) return refuse(who, "negative or zero size");
  if (const char* e = bad_matrix(Q, m, ldq, qlen, len)) return refuse(who, e);
  if (const char* e = bad_matrix(out, k, ldo, olen, len)) return refuse(who, e);
  if (!Y || ldy < k || ylen < (int64_t)(m - 1) * ldy + k) return refuse(who, "Y needs (m - 1) * ldy + k doubles, ldy >= k");
  if (need_device()) return 1;
  DevBuf dq, dy, dout;
  if (dq.up(Q, qlen) || dy.up(Y, ylen) || dout.up(out, olen)) return 1;
  if (trl_rotate_basis(len, m, k, dq.p, ldq, dy.p, ldy, dout.p, ldo, nullptr)) return 1;
  if (finish(who)) return 1;
  return dout.down(out);
}

int edigpu_trl_scale(int64_t len, double* v, int64_t vlen, double f) {
  const char* who = "edigpu_trl_scale";
  if (len < 1) return refuse(who, "negative or zero size");
  if (!v || vlen < len) return refuse(who, "v shorter than the vector length");
  if (need_device()) return 1;
  DevBuf dv;
  if (dv.up(v, vlen)) return 1;
  if (trl_scale(len, dv.p, f, nullptr)) return 1;
  if (finish(who)) return 1;
  return dv.down(v);
}

}  // extern "C"
