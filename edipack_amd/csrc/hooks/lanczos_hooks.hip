// lanczos_hooks.hip -- test hooks of the vector kernels of the three-term recurrence: the single-seed kernels
// (kernels_lanczos.hip), the sharded ones (kernels_shard.hip) and the batched ones (kernels_multi.hip).
//
// As trl_hooks.hip: each hook takes host buffers given as pointer + length in doubles, uploads every buffer WHOLE, calls
// one launcher of kernels.hpp as the library calls it, on the null stream of the calling thread's current device, and
// downloads every buffer the launcher may write, whole again: a test that surrounds its payload with sentinels sees every
// write.  No kernel lives here; the arguments are checked before the device is touched.
#include "hook_util.hpp"

namespace edigpu {
namespace {

constexpr int kNT = 256;  // threads per workgroup of every vector kernel here

// workgroups (= partials per sum) of a capped reduction over n doubles
int64_t red_blocks(int64_t n, int64_t cap = kRedBlocks) { return std::max<int64_t>(1, std::min<int64_t>((n + kNT - 1) / kNT, cap)); }

bool short_buf(const double* p, int64_t len, int64_t need) { return !p || len < need; }

constexpr int64_t kMaxLen = INT64_MAX >> 8;

bool width_ok(int W) { return W == 2 || W == 4 || W == 8; }

// the per-column scalar blocks of a batched recurrence: W blocks of `block` doubles, sstride apart
const char* bad_scal_multi(const double* scal, int64_t slen, int W, int64_t sstride, int64_t block) {
  if (sstride < block) return "sstride smaller than the scalar block";
  if (sstride > kMaxLen || short_buf(scal, slen, (int64_t)(W - 1) * sstride + block)) return "scal shorter than W blocks at sstride";
  return nullptr;
}

// the geometry of the column-block exchange, as edigpu_transpose_rotate_pack checks it; n = nrows * dim_up
const char* bad_exchange(int64_t n, int64_t dim_up, int64_t q, int world, int64_t pcol, int halo) {
  if (dim_up < 1 || q < 1 || world < 1 || pcol < 1 || halo < 0) return "negative or zero size";
  if (n % dim_up) return "n is not a whole number of rows";
  if (n / dim_up > q) return "nrows > q";
  if (pcol > kMaxLen / world || pcol * world < dim_up) return "pcol * world < dim_up";
  return nullptr;
}

int64_t exchange_doubles(int64_t q, int world, int64_t pcol, int halo) { return (int64_t)world * q * (pcol + 2 * halo); }

}  // namespace
}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_lzk_norm_begin(int64_t n, double* v, int64_t vlen, double* partial, int64_t plen, double* scal, int64_t slen) {
  const char* who = "edigpu_lzk_norm_begin";
  if (n < 1 || n > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(v, vlen, n)) return refuse(who, "v shorter than the vector length");
  if (short_buf(partial, plen, red_blocks(n))) return refuse(who, "partial needs min(ceil(n / 256), 1024) doubles");
  if (short_buf(scal, slen, SC_AB)) return refuse(who, "scal needs 8 doubles");
  if (need_device()) return 1;
  DevBuf dv, dp, ds;
  if (dv.up(v, vlen) || dp.up(partial, plen) || ds.up(scal, slen)) return 1;
  if (lz_norm_begin(dv.p, n, dp.p, ds.p, nullptr)) return 1;
  if (finish(who)) return 1;
  return dv.down(v) || dp.down(partial) || ds.down(scal);
}

int edigpu_lzk_rotate(int32_t lazy, int64_t n, double* vin, int64_t vinlen, double* vout, int64_t voutlen, const double* scal,
                      int64_t slen) {
  const char* who = "edigpu_lzk_rotate";
  if (n < 1 || n > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(vin, vinlen, n)) return refuse(who, "vin shorter than the vector length");
  if (short_buf(vout, voutlen, n)) return refuse(who, "vout shorter than the vector length");
  if (short_buf(scal, slen, SC_AB)) return refuse(who, "scal needs 8 doubles");
  if (need_device()) return 1;
  DevBuf da, db, ds;
  if (da.up(vin, vinlen) || db.up(vout, voutlen) || ds.up(scal, slen)) return 1;
  if (lazy ? lz_rotate_lazy(da.p, db.p, n, ds.p, nullptr) : lz_rotate(da.p, db.p, n, ds.p, nullptr)) return 1;
  if (finish(who)) return 1;
  return da.down(vin) || db.down(vout);
}

int edigpu_lzk_next_vector(int32_t lazy, int64_t n, const double* P, int64_t plen, const double* Q, int64_t qlen, double* X,
                           int64_t xlen, const double* scal, int64_t slen) {
  const char* who = "edigpu_lzk_next_vector";
  if (n < 1 || n > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(P, plen, n)) return refuse(who, "P shorter than the vector length");
  if (short_buf(Q, qlen, n)) return refuse(who, "Q shorter than the vector length");
  if (short_buf(X, xlen, n)) return refuse(who, "X shorter than the vector length");
  if (short_buf(scal, slen, SC_AB)) return refuse(who, "scal needs 8 doubles");
  if (need_device()) return 1;
  DevBuf dp, dq, dx, ds;
  if (dp.up(P, plen) || dq.up(Q, qlen) || dx.up(X, xlen) || ds.up(scal, slen)) return 1;
  if (lz_next_vector(dp.p, dq.p, dx.p, n, ds.p, lazy != 0, nullptr)) return 1;
  if (finish(who)) return 1;
  return dx.down(X);
}

int edigpu_lzk_alpha(int64_t n, const double* vin, int64_t vinlen, double* vout, int64_t voutlen, const double* tmp,
                     int64_t tmplen, double* partial, int64_t plen, double* scal, int64_t slen, int32_t iter, int32_t nlanc) {
  const char* who = "edigpu_lzk_alpha";
  if (n < 1 || n > kMaxLen || nlanc < 1) return refuse(who, "negative or zero size");
  if (iter < 0 || iter >= nlanc) return refuse(who, "iter is not a step below nlanc");
  if (short_buf(vin, vinlen, n)) return refuse(who, "vin shorter than the vector length");
  if (short_buf(vout, voutlen, n)) return refuse(who, "vout shorter than the vector length");
  if (short_buf(tmp, tmplen, n)) return refuse(who, "tmp shorter than the vector length");
  if (short_buf(partial, plen, red_blocks(n))) return refuse(who, "partial needs min(ceil(n / 256), 1024) doubles");
  if (short_buf(scal, slen, SC_AB + 2 * (int64_t)nlanc)) return refuse(who, "scal needs 8 + 2 * nlanc doubles");
  if (need_device()) return 1;
  DevBuf da, db, dt, dp, ds;
  if (da.up(vin, vinlen) || db.up(vout, voutlen) || dt.up(tmp, tmplen) || dp.up(partial, plen) || ds.up(scal, slen)) return 1;
  if (lz_alpha(da.p, db.p, dt.p, n, dp.p, ds.p, iter, nlanc, nullptr)) return 1;
  if (finish(who)) return 1;
  return db.down(vout) || dp.down(partial) || ds.down(scal);
}

int edigpu_lzk_beta(int64_t n, const double* vin, int64_t vinlen, double* vout, int64_t voutlen, double* partial, int64_t plen,
                    double* scal, int64_t slen, int32_t iter, int32_t nlanc) {
  const char* who = "edigpu_lzk_beta";
  if (n < 1 || n > kMaxLen || nlanc < 1) return refuse(who, "negative or zero size");
  if (iter < 0 || iter >= nlanc) return refuse(who, "iter is not a step below nlanc");
  if (short_buf(vin, vinlen, n)) return refuse(who, "vin shorter than the vector length");
  if (short_buf(vout, voutlen, n)) return refuse(who, "vout shorter than the vector length");
  if (short_buf(partial, plen, red_blocks(n))) return refuse(who, "partial needs min(ceil(n / 256), 1024) doubles");
  if (short_buf(scal, slen, SC_AB + 2 * (int64_t)nlanc)) return refuse(who, "scal needs 8 + 2 * nlanc doubles");
  if (need_device()) return 1;
  DevBuf da, db, dp, ds;
  if (da.up(vin, vinlen) || db.up(vout, voutlen) || dp.up(partial, plen) || ds.up(scal, slen)) return 1;
  if (lz_beta(da.p, db.p, n, dp.p, ds.p, iter, nlanc, nullptr)) return 1;
  if (finish(who)) return 1;
  return db.down(vout) || dp.down(partial) || ds.down(scal);
}

int edigpu_lzk_add_dot3(int64_t n, const double* P, int64_t plen, double* Q, int64_t qlen, const double* tmp, int64_t tmplen,
                        const double* scal, int64_t slen, double* partial, int64_t partlen, int32_t* np) {
  const char* who = "edigpu_lzk_add_dot3";
  if (n < 1 || n > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(P, plen, n)) return refuse(who, "P shorter than the vector length");
  if (short_buf(Q, qlen, n)) return refuse(who, "Q shorter than the vector length");
  if (short_buf(tmp, tmplen, n)) return refuse(who, "tmp shorter than the vector length");
  if (short_buf(scal, slen, SC_AB)) return refuse(who, "scal needs 8 doubles");
  if (short_buf(partial, partlen, 3 * red_blocks(n))) return refuse(who, "partial needs 3 * min(ceil(n / 256), 1024) doubles");
  if (!np) return refuse(who, "null np");
  if (need_device()) return 1;
  DevBuf dp, dq, dt, ds, dpart;
  if (dp.up(P, plen) || dq.up(Q, qlen) || dt.up(tmp, tmplen) || ds.up(scal, slen) || dpart.up(partial, partlen)) return 1;
  int cnt = 0;
  if (lz_add_dot3(dp.p, dq.p, dt.p, n, ds.p, dpart.p, &cnt, nullptr)) return 1;
  if (finish(who)) return 1;
  *np = cnt;
  return dq.down(Q) || dpart.down(partial);
}

int edigpu_lzk_axpy(int64_t n, double* acc, int64_t acclen, const double* vin, int64_t vinlen, double coef, const double* scal,
                    int64_t slen, int32_t iter) {
  const char* who = "edigpu_lzk_axpy";
  if (n < 1 || n > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(acc, acclen, n)) return refuse(who, "acc shorter than the vector length");
  if (short_buf(vin, vinlen, n)) return refuse(who, "vin shorter than the vector length");
  if (short_buf(scal, slen, SC_AB)) return refuse(who, "scal needs 8 doubles");
  if (need_device()) return 1;
  DevBuf da, dv, ds;
  if (da.up(acc, acclen) || dv.up(vin, vinlen) || ds.up(scal, slen)) return 1;
  if (lz_axpy_coef(da.p, dv.p, n, coef, ds.p, iter, nullptr)) return 1;
  if (finish(who)) return 1;
  return da.down(acc);
}

int edigpu_lzk_blocked(int32_t to, int64_t dim_up, int64_t dim_dw, int32_t shift, const double* src, int64_t srclen, double* dst,
                       int64_t dstlen) {
  const char* who = "edigpu_lzk_blocked";
  if (dim_up < 1 || dim_dw < 1 || dim_up > (1 << 30) || dim_dw > (1 << 30)) return refuse(who, "negative or zero size");
  if (shift < 0 || shift > 16) return refuse(who, "shift out of range (0 .. 16)");
  const int64_t natural = dim_up * dim_dw;
  const int64_t blocked = ((dim_up + ((int64_t)1 << shift) - 1) >> shift) * (dim_dw << shift);
  if (short_buf(src, srclen, to ? natural : blocked)) return refuse(who, "src shorter than its layout");
  if (short_buf(dst, dstlen, to ? blocked : natural)) return refuse(who, "dst shorter than its layout");
  if (need_device()) return 1;
  DevBuf ds, dd;
  if (ds.up(src, srclen) || dd.up(dst, dstlen)) return 1;
  if (to ? vec_to_blocked(ds.p, dd.p, dim_up, dim_dw, shift, nullptr) : vec_from_blocked(ds.p, dd.p, dim_up, dim_dw, shift, nullptr))
    return 1;
  if (finish(who)) return 1;
  return dd.down(dst);
}

int edigpu_lzk_shard_rotate3(int32_t first, int64_t n, int64_t dim_up, int64_t q, int32_t world, int64_t pcol, int32_t halo,
                             double* vin, int64_t vinlen, double* vout, int64_t voutlen, const double* t, const double* tprev,
                             double* send, int64_t sendlen) {
  const char* who = "edigpu_lzk_shard_rotate3";
  if (n < 1 || n > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(vin, vinlen, n)) return refuse(who, "vin shorter than the vector length");
  if (short_buf(vout, voutlen, n)) return refuse(who, "vout shorter than the vector length");
  if (!first && !t) return refuse(who, "a later step needs the sums t");
  if (send) {
    if (const char* m = bad_exchange(n, dim_up, q, world, pcol, halo)) return refuse(who, m);
    if (sendlen < exchange_doubles(q, world, pcol, halo)) return refuse(who, "send needs world * q * (pcol + 2 * halo) doubles");
  }
  if (need_device()) return 1;
  DevBuf da, db, dt, dtp, dsend;
  if (da.up(vin, vinlen) || db.up(vout, voutlen) || (t && dt.up(t, 3)) || (tprev && dtp.up(tprev, 3)) ||
      (send && dsend.up(send, sendlen)))
    return 1;
  if (shard_rotate3(first != 0, n, dim_up, q, world, pcol, halo, da.p, db.p, t ? dt.p : nullptr, tprev ? dtp.p : nullptr,
                    send ? dsend.p : nullptr, nullptr))
    return 1;
  if (finish(who)) return 1;
  return da.down(vin) || db.down(vout) || (send && dsend.down(send));
}

int edigpu_lzk_shard_add_dot3(int64_t n, int64_t dim_up, int64_t q, int32_t world, int64_t pcol, int32_t halo, const double* vin,
                              int64_t vinlen, double* vout, int64_t voutlen, const double* tmp, int64_t tmplen, const double* back,
                              int64_t backlen, const double* tprev, double* work, int64_t worklen, double* sums, int64_t sumslen) {
  const char* who = "edigpu_lzk_shard_add_dot3";
  if (n < 1 || n > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(vin, vinlen, n)) return refuse(who, "vin shorter than the vector length");
  if (short_buf(vout, voutlen, n)) return refuse(who, "vout shorter than the vector length");
  if (short_buf(tmp, tmplen, n)) return refuse(who, "tmp shorter than the vector length");
  if (back) {
    if (const char* m = bad_exchange(n, dim_up, q, world, pcol, halo)) return refuse(who, m);
    if (backlen < exchange_doubles(q, world, pcol, halo)) return refuse(who, "back needs world * q * (pcol + 2 * halo) doubles");
  }
  if (short_buf(work, worklen, 3 * kRedBlocks)) return refuse(who, "work needs 3 * 1024 doubles");
  if (short_buf(sums, sumslen, 3)) return refuse(who, "sums needs 3 doubles");
  if (need_device()) return 1;
  DevBuf da, db, dt, dback, dtp, dw, ds;
  if (da.up(vin, vinlen) || db.up(vout, voutlen) || dt.up(tmp, tmplen) || (back && dback.up(back, backlen)) ||
      (tprev && dtp.up(tprev, 3)) || dw.up(work, worklen) || ds.up(sums, sumslen))
    return 1;
  if (shard_add_dot3(n, dim_up, q, pcol, halo, da.p, db.p, dt.p, back ? dback.p : nullptr, tprev ? dtp.p : nullptr, dw.p, ds.p,
                     nullptr))
    return 1;
  if (finish(who)) return 1;
  return db.down(vout) || dw.down(work) || ds.down(sums);
}

int edigpu_lzk_panel_rotate(int64_t n2, double* x, int64_t xlen, const double* v, int64_t vlen, const double* t,
                            const double* tprev) {
  const char* who = "edigpu_lzk_panel_rotate";
  if (n2 < 1 || n2 > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(x, xlen, 2 * n2)) return refuse(who, "x shorter than 2 * n2 doubles");
  if (short_buf(v, vlen, 2 * n2)) return refuse(who, "v shorter than 2 * n2 doubles");
  if (!t) return refuse(who, "null sums t");
  if (need_device()) return 1;
  DevBuf dx, dv, dt, dtp;
  if (dx.up(x, xlen) || dv.up(v, vlen) || dt.up(t, 3) || (tprev && dtp.up(tprev, 3))) return 1;
  if (shard_panel_rotate(n2, dx.p, dv.p, dt.p, tprev ? dtp.p : nullptr, nullptr)) return 1;
  if (finish(who)) return 1;
  return dx.down(x);
}

int edigpu_lzk_panel_add_dot(int64_t n2, const double* x, int64_t xlen, double* vdst, int64_t vdstlen, const double* rowhalf,
                             int64_t rowlen, const double* colhalf, int64_t collen, const double* t, const double* tprev,
                             double* work, int64_t worklen, double* sums, int64_t sumslen) {
  const char* who = "edigpu_lzk_panel_add_dot";
  if (n2 < 1 || n2 > kMaxLen) return refuse(who, "negative or zero size");
  if (short_buf(x, xlen, 2 * n2)) return refuse(who, "x shorter than 2 * n2 doubles");
  if (short_buf(vdst, vdstlen, 2 * n2)) return refuse(who, "vdst shorter than 2 * n2 doubles");
  if (short_buf(rowhalf, rowlen, 2 * n2)) return refuse(who, "rowhalf shorter than 2 * n2 doubles");
  if (short_buf(colhalf, collen, 2 * n2)) return refuse(who, "colhalf shorter than 2 * n2 doubles");
  if (!t && tprev) return refuse(who, "tprev without t");
  if (short_buf(work, worklen, 3 * kRedBlocks)) return refuse(who, "work needs 3 * 1024 doubles");
  if (short_buf(sums, sumslen, 3)) return refuse(who, "sums needs 3 doubles");
  if (need_device()) return 1;
  DevBuf dx, dv, dr, dc, dt, dtp, dw, ds;
  if (dx.up(x, xlen) || dv.up(vdst, vdstlen) || dr.up(rowhalf, rowlen) || dc.up(colhalf, collen) || (t && dt.up(t, 3)) ||
      (tprev && dtp.up(tprev, 3)) || dw.up(work, worklen) || ds.up(sums, sumslen))
    return 1;
  if (shard_panel_add_dot(n2, dx.p, dv.p, dr.p, dc.p, t ? dt.p : nullptr, tprev ? dtp.p : nullptr, dw.p, ds.p, nullptr)) return 1;
  if (finish(who)) return 1;
  return dv.down(vdst) || dw.down(work) || ds.down(sums);
}

int edigpu_lzk_interleave(int32_t to, int32_t W, int32_t cplx, int64_t nrow, int32_t g, const double* src, int64_t srclen,
                          double* dst, int64_t dstlen) {
  const char* who = "edigpu_lzk_interleave";
  if (!width_ok(W)) return refuse(who, "width must be 2, 4 or 8");
  if (nrow < 1 || nrow > kMaxLen) return refuse(who, "negative or zero size");
  if (g < 0 || g > W) return refuse(who, "g > W or negative");
  const int64_t col = nrow * (cplx ? 2 : 1);
  if (short_buf(src, srclen, (to ? g : W) * col)) return refuse(who, "src shorter than its layout");
  if (short_buf(dst, dstlen, (to ? W : g) * col)) return refuse(who, "dst shorter than its layout");
  if (need_device()) return 1;
  DevBuf ds, dd;
  if (ds.up(src, srclen) || dd.up(dst, dstlen)) return 1;
  if (to ? launch_interleave_multi(W, cplx, nrow, g, ds.p, dd.p, nullptr) : launch_deinterleave_multi(W, cplx, nrow, g, ds.p, dd.p, nullptr))
    return 1;
  if (finish(who)) return 1;
  return dd.down(dst);
}

int edigpu_lzk_norm_begin_multi(int32_t W, int32_t cplx, int64_t nrow, double* P, int64_t plen, double* partial, int64_t partlen,
                                double* scal, int64_t slen, int64_t sstride) {
  const char* who = "edigpu_lzk_norm_begin_multi";
  if (!width_ok(W)) return refuse(who, "width must be 2, 4 or 8");
  if (nrow < 1 || nrow > kMaxLen) return refuse(who, "negative or zero size");
  const int64_t col = nrow * (cplx ? 2 : 1);
  if (short_buf(P, plen, W * col)) return refuse(who, "P shorter than W interleaved columns");
  if (short_buf(partial, partlen, W * red_blocks(col))) return refuse(who, "partial needs W * min(ceil(len / 256), 1024) doubles");
  if (const char* m = bad_scal_multi(scal, slen, W, sstride, SC_AB)) return refuse(who, m);
  if (need_device()) return 1;
  DevBuf dp, dpart, ds;
  if (dp.up(P, plen) || dpart.up(partial, partlen) || ds.up(scal, slen)) return 1;
  if (lz_norm_begin_multi(W, cplx, nrow, dp.p, dpart.p, partlen, ds.p, sstride, nullptr)) return 1;
  if (finish(who)) return 1;
  return dp.down(P) || dpart.down(partial) || ds.down(scal);
}

int edigpu_lzk_rotate_lazy_multi(int32_t W, int32_t cplx, int64_t nrow, double* P, int64_t plen, double* Q, int64_t qlen,
                                 const double* scal, int64_t slen, int64_t sstride) {
  const char* who = "edigpu_lzk_rotate_lazy_multi";
  if (!width_ok(W)) return refuse(who, "width must be 2, 4 or 8");
  if (nrow < 1 || nrow > kMaxLen) return refuse(who, "negative or zero size");
  const int64_t col = nrow * (cplx ? 2 : 1);
  if (short_buf(P, plen, W * col)) return refuse(who, "P shorter than W interleaved columns");
  if (short_buf(Q, qlen, W * col)) return refuse(who, "Q shorter than W interleaved columns");
  if (const char* m = bad_scal_multi(scal, slen, W, sstride, SC_AB)) return refuse(who, m);
  if (need_device()) return 1;
  DevBuf dp, dq, ds;
  if (dp.up(P, plen) || dq.up(Q, qlen) || ds.up(scal, slen)) return 1;
  if (lz_rotate_lazy_multi(W, cplx, nrow, dp.p, dq.p, ds.p, sstride, nullptr)) return 1;
  if (finish(who)) return 1;
  return dp.down(P) || dq.down(Q);
}

int edigpu_lzk_finalize_ab_multi(int32_t W, int32_t cplx, int64_t nrow, const double* P, int64_t plen, const double* Q,
                                 int64_t qlen, const double* partial, int64_t partlen, int32_t np, double* scal, int64_t slen,
                                 int64_t sstride, int32_t nlanc) {
  const char* who = "edigpu_lzk_finalize_ab_multi";
  if (!width_ok(W)) return refuse(who, "width must be 2, 4 or 8");
  if (nrow < 1 || nrow > kMaxLen || nlanc < 1 || np < 1 || np > kMaxPartials) return refuse(who, "negative or zero size");
  const int64_t col = nrow * (cplx ? 2 : 1);
  if (short_buf(P, plen, W * col)) return refuse(who, "P shorter than W interleaved columns");
  if (short_buf(Q, qlen, W * col)) return refuse(who, "Q shorter than W interleaved columns");
  if (short_buf(partial, partlen, (int64_t)3 * W * np)) return refuse(who, "partial needs 3 * W * np doubles");
  if (const char* m = bad_scal_multi(scal, slen, W, sstride, SC_AB + 2 * (int64_t)nlanc)) return refuse(who, m);
  for (int j = 0; j < W; j++)  // the step index comes from the device scalars: it addresses scal[SC_AB + step]
    if (!(scal[j * sstride + SC_NDONE] >= 0.0)) return refuse(who, "a column's step count is negative");
  if (need_device()) return 1;
  DevBuf dp, dq, dpart, ds;
  if (dp.up(P, plen) || dq.up(Q, qlen) || dpart.up(partial, partlen) || ds.up(scal, slen)) return 1;
  if (lz_finalize_ab_multi(W, cplx, nrow, dp.p, dq.p, dpart.p, np, ds.p, sstride, nlanc, nullptr)) return 1;
  if (finish(who)) return 1;
  return ds.down(scal);
}

}  // extern "C"
