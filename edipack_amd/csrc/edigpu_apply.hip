// edigpu_apply.hip -- the product H*v of every kind of handle: the dispatcher over the kernels (apply_any), the handle's
// workspace, the product entry points of the C ABI on host and device vectors, the two halves of the transposed
// exchange and the stand-alone vector kernels of the sharded loops.
#include <algorithm>
#include <cmath>
#include <string>

#include "dev_mem.hpp"
#include "host_ib.hpp"
#include "kernels.hpp"

namespace edigpu {

int ensure_workspace(edigpu_sector* s) {
  const int64_t len = s->nloc * (s->is_complex ? 2 : 1);
  if (s->d_vin && s->ws_len == len) return 0;
  dev_free_all(s->d_vin, s->d_vout, s->d_tmp, s->d_partial, s->d_scal);
  // (the panel-major layout of the Lanczos loop pads the last panel: blk_len >= len)
  const size_t n = (size_t)std::max<int64_t>(std::max(std::max(len, s->blk_len), s->ib ? s->ib->len : 0), 1);
  EDIGPU_HIP(hipMalloc((void**)&s->d_vin, n * sizeof(double)));
  EDIGPU_HIP(hipMalloc((void**)&s->d_vout, n * sizeof(double)));
  EDIGPU_HIP(hipMalloc((void**)&s->d_tmp, n * sizeof(double)));
  if (s->ib && s->ib->ps != s->ib->dim_dw * kIbPanel) {
    // padded panel stride (EDIGPU_IB_PSPAD): the doubles between two panels are never written by a kernel and are part of
    // the vector sums -- they must be zero
    EDIGPU_HIP(hipMemset(s->d_vin, 0, n * sizeof(double)));
    EDIGPU_HIP(hipMemset(s->d_vout, 0, n * sizeof(double)));
    EDIGPU_HIP(hipMemset(s->d_tmp, 0, n * sizeof(double)));
  }
  // per-workgroup partials: three per 256-row workgroup of the SELL dot epilogue is the largest user
  s->partial_cap = std::max<int64_t>(kMaxPartials, 3 * ((s->nloc + 255) / 256) + 64);
  EDIGPU_HIP(hipMalloc((void**)&s->d_partial, (size_t)s->partial_cap * sizeof(double)));
  s->ws_len = len;
  return 0;
}

// general g_ph(a,b): t = O v[jph] with the electron-phonon operator as its own sector handle (sub_a), then
// hv[jph+1] += sqrt(jph+1) t, hv[jph-1] += sqrt(jph) t   (stored/H_e_ph.f90 x (b + b^+); w = doubles per element)
static int apply_eph_operator(const edigpu_sector* s, const double* v, double* hv, int w, hipStream_t st) {
  if (!s->sub_a) return 0;
  const int64_t n = s->dim_el * w;
  for (int jph = 0; jph <= s->nph; jph++) {
    if (apply_any(s->sub_a, v + jph * n, v + jph * n, s->d_cz, 3, st)) return 1;
    double* up = jph < s->nph ? hv + (jph + 1) * n : nullptr;
    double* dn = jph > 0 ? hv + (jph - 1) * n : nullptr;
    if (launch_eph_scatter(n, s->d_cz, up, sqrt((double)(jph + 1)), dn, sqrt((double)jph), st)) return 1;
  }
  return 0;
}

int apply_any(edigpu_sector* s, const double* v_local, const double* v_full, double* hv,
              int phase, hipStream_t st) {
  if (s->kind == kCmplxNormal) {
    // _CMPLX_NORMAL: (S + iA)(xr + i xi) = (S xr - A xi) + i (S xi + A xr) on planar work vectors
    if (phase != 3) {
      set_error("complex normal-mode sectors are single-shard: use the fused product");
      return 1;
    }
    // one real product on the doubled up index (interleaved complex = real vectors of that sector)
    if (s->sub_d) return apply_any(s->sub_d, v_full, v_full, hv, 3, st);
    const int64_t n = s->dim;
    double *xr = s->d_cz, *xi = xr + n, *yr = xi + n, *yi = yr + n, *t1 = yi + n, *t2 = t1 + n;
    if (launch_deinterleave(n, v_full, xr, xi, st)) return 1;
    if (apply_any(s->sub_s, xr, xr, yr, 3, st) || apply_any(s->sub_s, xi, xi, yi, 3, st)) return 1;
    if (s->sub_a && (apply_any(s->sub_a, xi, xi, t1, 3, st) || apply_any(s->sub_a, xr, xr, t2, 3, st))) return 1;
    return launch_combine_interleave(n, yr, yi, s->sub_a ? t1 : nullptr, s->sub_a ? t2 : nullptr, hv, st);
  }
  if (s->kind == kNormal && s->has_phonons()) {
    // phonon branches: the electronic product on every phonon block, then the phonon / electron-phonon pass
    if (phase != 3) {
      set_error("phonon sectors are single-shard: use the fused product");
      return 1;
    }
    for (int iph = 0; iph <= s->nph; iph++) {
      const int64_t o = (int64_t)iph * s->dim_el;
      if (launch_normal(s, v_local + o, v_full + o, hv + o, 3, st)) return 1;
    }
    if (launch_phonon(s, v_full, hv, st)) return 1;
    return apply_eph_operator(s, v_full, hv, 1, st);
  }
  if (s->kind == kNormal) return launch_normal(s, v_local, v_full, hv, phase, st);
  if ((s->is_flat_family()) && s->has_phonons()) {
    // phonon branches of the superc / nonsu2 products: electronic product per phonon block, then the phonon pass
    if (phase != 3 || !s->is_whole()) {
      set_error("phonon sectors: whole sectors take the fused product, row shards edigpu_apply_sharded_* / "
                "edigpu_lanczos_tridiag_sharded");
      return 1;
    }
    for (int iph = 0; iph <= s->nph; iph++) {
      const int64_t o = 2 * (int64_t)iph * s->dim_el;
      if (s->kind == kDirect) {
        if (launch_direct(s, v_full + o, hv + o, st)) return 1;
      } else if (launch_csr(s->loc, 1, v_full + o, hv + o, 0, st)) {
        return 1;
      }
    }
    if (launch_phonon(s, v_full, hv, st)) return 1;
    return apply_eph_operator(s, v_full, hv, 2, st);
  }
  if (s->kind == kOrbs) {
    // ed_total_ud = F.  Whole sector: phase 1 = everything, phase 2 = nothing left to add.  Row shard
    // (edigpu_orbs_build_rows): like the on-the-fly sectors the whole product needs the gathered vector.
    if (s->is_whole()) {
      if (phase == 2) return 0;
      return launch_orbs(s, v_full, hv, st);
    }
    if (phase == 1) return launch_zero(hv, s->nloc, st);
    return launch_orbs(s, v_full, hv, st);
  }
  if (s->kind == kDirect) {
    // on-the-fly: like directMatVec_MPI_* the whole product needs the gathered vector
    // (reference ED_NONSU2/ED_HAMILTONIAN_NONSU2_DIRECT_HxV.f90:220-223: gather first, then compute)
    if (phase == 1) return launch_zero(hv, s->nloc * 2, st);
    return launch_direct(s, v_full, hv, st);
  }
  // flat: loc block then non-local block
  if (phase & 1) {
    if (launch_csr(s->loc, s->is_complex, v_local, hv, 0, st)) return 1;
  }
  if (phase & 2) {
    if (launch_csr(s->nonloc, s->is_complex, v_full, hv, 1, st)) return 1;
  }
  return 0;
}

// One electronic block of a superc / nonsu2 phonon handle (the sharded product: edigpu_shard.hip): phase 1 = the part
// that needs the rows' own elements only, phase 2 = the part that needs the gathered block
int apply_flat_block(edigpu_sector* s, const double* v_local, const double* v_full, double* hv, int phase, hipStream_t st) {
  if (s->kind == kDirect) {
    if (phase == 1) return launch_zero(hv, s->dim_el * 2, st);
    return launch_direct(s, v_full, hv, st);
  }
  if (phase == 1) return launch_csr(s->loc, s->is_complex, v_local, hv, 0, st);
  return launch_csr(s->nonloc, s->is_complex, v_full, hv, 1, st);
}

int single_shard(const edigpu_sector* s, const char* who) {
  if (!s->is_whole()) {
    set_error(std::string(who) + ": handle is a shard (local rows != global dim); use the _dev entry points");
    return 1;
  }
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

static int apply_host(edigpu_handle s, int64_t nloc, const double* v_host, double* hv_host, int cplx) {
  if (!s || !v_host || !hv_host) {
    set_error("edigpu_apply: NULL argument");
    return 1;
  }
  if ((s->is_complex != 0) != (cplx != 0)) {
    set_error("edigpu_apply: real/complex mismatch between handle and entry point");
    return 1;
  }
  if (nloc != s->nloc) {
    set_error("edigpu_apply: Nloc does not match the handle's local dimension");
    return 1;
  }
  if (single_shard(s, "edigpu_apply")) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ensure_workspace(s)) return 1;
  const size_t bytes = (size_t)s->ws_len * sizeof(double);
  if (s->kind == kNormal && s->ib && s->nph == 0) {
    // host vectors cross PCIe anyway: take the impurity-block kernels of the device-resident loops (two layout
    // conversions on the device are small next to the transfers)
    hipStream_t st = s->stream;
    EDIGPU_HIP(hipMemcpyAsync(s->d_tmp, v_host, bytes, hipMemcpyHostToDevice, st));
    if (vec_to_ib(s->ib, s->d_tmp, s->d_vin, st) || launch_ib(s, s->d_vin, s->d_vout, st) || vec_from_ib(s->ib, s->d_vout, s->d_tmp, st))
      return 1;
    EDIGPU_HIP(hipMemcpyAsync(hv_host, s->d_tmp, bytes, hipMemcpyDeviceToHost, st));
    EDIGPU_HIP(hipStreamSynchronize(st));
    return 0;
  }
  EDIGPU_HIP(hipMemcpyAsync(s->d_vin, v_host, bytes, hipMemcpyHostToDevice, s->stream));
  if (apply_any(s, s->d_vin, s->d_vin, s->d_tmp, 3, s->stream)) return 1;
  EDIGPU_HIP(hipMemcpyAsync(hv_host, s->d_tmp, bytes, hipMemcpyDeviceToHost, s->stream));
  EDIGPU_HIP(hipStreamSynchronize(s->stream));
  return 0;
}

int edigpu_apply_d(edigpu_handle h, int64_t nloc, const double* v_host, double* hv_host) {
  return apply_host(h, nloc, v_host, hv_host, 0);
}

int edigpu_apply_z(edigpu_handle h, int64_t nloc, const double* v_host, double* hv_host) {
  return apply_host(h, nloc, v_host, hv_host, 1);
}

int edigpu_apply_dev(edigpu_handle s, const void* v_full_dev, void* hv_dev, void* stream) {
  if (!s || !v_full_dev || !hv_dev) {
    set_error("edigpu_apply_dev: NULL argument");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default (null) stream
  const int w = s->is_complex ? 2 : 1;
  const double* vf = (const double*)v_full_dev;
  return apply_any(s, vf + s->row_first * w, vf, (double*)hv_dev, 3, st);
}

int edigpu_apply_local_dev(edigpu_handle s, const void* v_local_dev, void* hv_dev, void* stream) {
  if (!s || !v_local_dev || !hv_dev) {
    set_error("edigpu_apply_local_dev: NULL argument");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default (null) stream
  return apply_any(s, (const double*)v_local_dev, nullptr, (double*)hv_dev, 1, st);
}

int edigpu_apply_remote_dev(edigpu_handle s, const void* v_full_dev, void* hv_dev, void* stream) {
  if (!s || !v_full_dev || !hv_dev) {
    set_error("edigpu_apply_remote_dev: NULL argument");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default (null) stream
  return apply_any(s, nullptr, (const double*)v_full_dev, (double*)hv_dev, 2, st);
}

// ---- transposed exchange (normal mode, N > 1): see include/edigpu.h ----
int edigpu_normal_transpose_info(edigpu_handle s, int32_t* halo) {
  if (!s || !halo) {
    set_error("edigpu_normal_transpose_info: NULL argument");
    return 1;
  }
  if (!normal_transposable(s)) {
    set_error("edigpu_normal_transpose_info: needs a whole normal-mode sector built by edigpu_normal_build "
              "(factored Hnd, no phonons); use the all-gather entry points otherwise");
    return 1;
  }
  *halo = s->col_halo;
  return 0;
}

int edigpu_normal_apply_rows_dev(edigpu_handle s, int64_t dw_first, int64_t dw_count, const void* v_rows_dev,
                                 void* hv_rows_dev, void* stream) {
  if (!s || !v_rows_dev || !hv_rows_dev) {
    set_error("edigpu_normal_apply_rows_dev: NULL argument");
    return 1;
  }
  if (!normal_transposable(s)) {
    set_error("edigpu_normal_apply_rows_dev: not a transposable handle (see edigpu_normal_transpose_info)");
    return 1;
  }
  if (dw_first < 0 || dw_count < 0 || dw_first + dw_count > s->dim_dw) {
    set_error("edigpu_normal_apply_rows_dev: row range outside [0, DimDw)");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  return launch_normal_rows(s, dw_first, dw_count, (const double*)v_rows_dev, (double*)hv_rows_dev,
                            (hipStream_t)stream);
}

int edigpu_normal_apply_cols_dev(edigpu_handle s, int64_t col_first, int64_t col_count, int64_t row_stride,
                                 int32_t halo, const void* w_cols_dev, void* hv_cols_dev, void* stream) {
  if (!s || !w_cols_dev || !hv_cols_dev) {
    set_error("edigpu_normal_apply_cols_dev: NULL argument");
    return 1;
  }
  if (!normal_transposable(s)) {
    set_error("edigpu_normal_apply_cols_dev: not a transposable handle (see edigpu_normal_transpose_info)");
    return 1;
  }
  if (col_first < 0 || col_count < 0 || col_first + col_count > s->dim_up || halo < s->col_halo ||
      row_stride < col_count + 2 * (int64_t)halo) {
    set_error("edigpu_normal_apply_cols_dev: column range outside [0, DimUp), halo smaller than the sector needs, "
              "or row stride < col_count + 2 halo");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  return launch_normal_cols(s, col_first, col_count, row_stride, halo, (const double*)w_cols_dev, (double*)hv_cols_dev,
                            (hipStream_t)stream);
}

int edigpu_transpose_pack(int64_t dim_up, int64_t nrows, int64_t q, int32_t world, int64_t pcol, int32_t halo,
                          const void* v_rows_dev, void* send_dev, void* stream) {
  if (!v_rows_dev || !send_dev || dim_up <= 0 || nrows < 0 || nrows > q || world <= 0 || pcol <= 0 || halo < 0 ||
      pcol * world < dim_up) {
    set_error("edigpu_transpose_pack: bad argument");
    return 1;
  }
  if (ensure_device()) return 1;
  return launch_transpose_pack(dim_up, nrows, q, world, pcol, halo, (const double*)v_rows_dev, (double*)send_dev,
                               (hipStream_t)stream);
}

int edigpu_transpose_unpack_add(int64_t dim_up, int64_t nrows, int64_t q, int32_t world, int64_t pcol,
                                int32_t halo, const void* recv_dev, void* hv_rows_dev, void* stream) {
  if (!recv_dev || !hv_rows_dev || dim_up <= 0 || nrows < 0 || nrows > q || world <= 0 || pcol <= 0 || halo < 0 ||
      pcol * world < dim_up) {
    set_error("edigpu_transpose_unpack_add: bad argument");
    return 1;
  }
  if (ensure_device()) return 1;
  return launch_transpose_unpack_add(dim_up, nrows, q, world, pcol, halo, (const double*)recv_dev,
                                     (double*)hv_rows_dev, (hipStream_t)stream);
}

int edigpu_transpose_rotate_pack(int32_t first, int64_t dim_up, int64_t nrows, int64_t q, int32_t world,
                                 int64_t pcol, int32_t halo, void* vin_dev, void* vout_dev, const void* ab_dev,
                                 void* send_dev, void* stream) {
  if (!vin_dev || !vout_dev || !send_dev || (!first && !ab_dev) || dim_up <= 0 || nrows < 0 || nrows > q ||
      world <= 0 || pcol <= 0 || halo < 0 || pcol * world < dim_up) {
    set_error("edigpu_transpose_rotate_pack: bad argument");
    return 1;
  }
  if (ensure_device()) return 1;
  return vec_rotate_pack(first, dim_up, nrows, q, world, pcol, halo, (double*)vin_dev, (double*)vout_dev,
                         (const double*)ab_dev, (double*)send_dev, (hipStream_t)stream);
}

int edigpu_transpose_unpack_add_dot2(int64_t dim_up, int64_t nrows, int64_t q, int32_t world, int64_t pcol,
                                     int32_t halo, const void* vin_dev, void* vout_dev, const void* tmp_dev,
                                     const void* back_dev, void* out2_dev, void* work_dev, void* stream) {
  if (!vin_dev || !vout_dev || !tmp_dev || !back_dev || !out2_dev || !work_dev || dim_up <= 0 || nrows < 0 ||
      nrows > q || world <= 0 || pcol <= 0 || halo < 0 || pcol * world < dim_up) {
    set_error("edigpu_transpose_unpack_add_dot2: bad argument");
    return 1;
  }
  if (ensure_device()) return 1;
  return vec_unpack_add_dot2(dim_up, nrows, q, pcol, halo, (const double*)vin_dev, (double*)vout_dev,
                             (const double*)tmp_dev, (const double*)back_dev, (double*)out2_dev, (double*)work_dev,
                             (hipStream_t)stream);
}

int edigpu_vec_work_doubles(void) { return kRedBlocks; }

int edigpu_vec_rotate(int64_t n, double* vin_dev, double* vout_dev, const double* beta2_dev, void* stream) {
  if (n < 0 || !vin_dev || !vout_dev || !beta2_dev) {
    set_error("edigpu_vec_rotate: bad argument");
    return 1;
  }
  return vec_rotate(n, vin_dev, vout_dev, beta2_dev, (hipStream_t)stream);
}

int edigpu_vec_add_dot(int64_t n, const double* vin_dev, double* vout_dev, const double* tmp_dev,
                       double* out_dev, double* work_dev, void* stream) {
  if (n < 0 || !vin_dev || !vout_dev || !tmp_dev || !out_dev || !work_dev) {
    set_error("edigpu_vec_add_dot: bad argument");
    return 1;
  }
  return vec_add_dot(n, vin_dev, vout_dev, tmp_dev, out_dev, work_dev, (hipStream_t)stream);
}

int edigpu_vec_axpy_nrm2(int64_t n, const double* vin_dev, double* vout_dev, const double* alpha_dev,
                         double* out_dev, double* work_dev, void* stream) {
  if (n < 0 || !vin_dev || !vout_dev || !alpha_dev || !out_dev || !work_dev) {
    set_error("edigpu_vec_axpy_nrm2: bad argument");
    return 1;
  }
  return vec_axpy_nrm2(n, vin_dev, vout_dev, alpha_dev, out_dev, work_dev, (hipStream_t)stream);
}

int edigpu_vec_rotate_lazy(int64_t n, double* vin_dev, double* vout_dev, const double* ab_dev, void* stream) {
  if (n < 0 || !vin_dev || !vout_dev || !ab_dev) {
    set_error("edigpu_vec_rotate_lazy: bad argument");
    return 1;
  }
  return vec_rotate_lazy(n, vin_dev, vout_dev, ab_dev, (hipStream_t)stream);
}

int edigpu_vec_add_dot2(int64_t n, const double* vin_dev, double* vout_dev, const double* tmp_dev, double* out2_dev,
                        double* work_dev, void* stream) {
  if (n < 0 || !vin_dev || !vout_dev || !tmp_dev || !out2_dev || !work_dev) {
    set_error("edigpu_vec_add_dot2: bad argument");
    return 1;
  }
  return vec_add_dot2(n, vin_dev, vout_dev, tmp_dev, out2_dev, work_dev, (hipStream_t)stream);
}

int edigpu_vec_scale(int64_t n, double* v_dev, const double* nrm2_dev, void* stream) {
  if (n < 0 || !v_dev || !nrm2_dev) {
    set_error("edigpu_vec_scale: bad argument");
    return 1;
  }
  return vec_scale(n, v_dev, nrm2_dev, (hipStream_t)stream);
}

int edigpu_apply_loop_d(edigpu_handle s, int64_t nloc, const double* v_host, double* hv_host) {
  if (!s || !v_host || !hv_host) {
    set_error("edigpu_apply_loop_d: NULL argument");
    return 1;
  }
  if (single_shard(s, "edigpu_apply_loop_d")) return 1;
  if (s->is_complex || s->kind == kCmplxNormal || nloc != s->nloc) {
    set_error("edigpu_apply_loop_d: needs a real handle and a vector of its local rows");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ensure_workspace(s)) return 1;
  hipStream_t st = s->stream;
  if (lanczos_prepare(s, 1, 0.0, st)) return 1;  // chooses the layout
  if (lanczos_seed(s, v_host, 0, st)) return 1;
  // (the result goes to d_vout: d_tmp is what lanczos_fetch converts through)
  if (s->lz_blocked ? launch_normal_blocked(s, s->d_vin, s->d_vout, st) : apply_any(s, s->d_vin, s->d_vin, s->d_vout, 3, st))
    return 1;
  if (lanczos_fetch(s, s->d_vout, hv_host, st)) return 1;
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
