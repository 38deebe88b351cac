// edigpu_ops.hip -- c / c^+ between two sectors on device vectors (edigpu_apply_op_*, edigpu_apply_cops_*): the checks,
// the partner table of one operator, launch (kernels_ops.hip).  Phonon, complex and ed_total_ud=F pairs of normal-mode
// handles take the route of edigpu_axisop.hip.
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "kernels.hpp"

namespace edigpu {

// the checks of one term of apply_Cops on normal-mode sectors, on the handles alone (no device is touched)
static int normal_term_check(const edigpu_sector* src, const edigpu_sector* dst, int iorb, int ispin, int create, const char* who) {
  const std::string w(who);
  if (src->kind != kNormal || dst->kind != kNormal || !src->from_model() || !dst->from_model() || src->has_phonons() || dst->has_phonons()) {
    set_error(w + ": both handles must be normal-mode sectors built by edigpu_normal_build");
    return 1;
  }
  if (!src->is_whole() || !dst->is_whole()) {
    set_error(w + ": handles must hold whole sectors");
    return 1;
  }
  const int ns = model_ns(src->model);
  if (iorb < 0 || iorb >= src->model.norb || ispin < 0 || ispin > 1) {
    set_error(w + ": orbital / spin out of range");
    return 1;
  }
  const int d = create ? 1 : -1;
  const int nup_s = src->sec_a, ndw_s = src->sec_b;
  if (dst->sec_a != nup_s + (ispin == 0 ? d : 0) || dst->sec_b != ndw_s + (ispin == 1 ? d : 0) ||
      model_ns(dst->model) != ns) {
    set_error(w + ": destination sector is not (source sector +- one particle of that spin)");
    return 1;
  }
  return 0;
}

// one term of apply_Cops / apply_op_C / apply_op_CDG on device vectors of two normal-mode sectors:
// v_dst (=|+=) coef * c^(+)_{iorb,ispin} v_src on the destination's down rows [fd, fd + cd) (v_dst_dev holds those rows),
// v_src_dev = the whole source vector.  checked: the caller has made normal_term_check
static int apply_op_normal_term(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev,
                                int iorb, int ispin, int create, double coef, int accumulate, hipStream_t st,
                                const char* who, int64_t fd = 0, int64_t cd = -1, bool checked = false) {
  const std::string w(who);
  if (!checked && normal_term_check(src, dst, iorb, ispin, create, who)) return 1;
  const int ns = model_ns(src->model);
  const int nup_s = src->sec_a, ndw_s = src->sec_b;
  if (cd < 0) cd = dst->dim_dw - fd;
  if (fd < 0 || fd + cd > dst->dim_dw) {
    set_error(w + ": row window outside the destination sector");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(src->device));
  // signed partial permutation of the changed species: for every destination state its preimage
  CombBasis bs, bd;
  bs.init(ns, ispin == 0 ? nup_s : ndw_s);
  bd.init(ns, ispin == 0 ? dst->sec_a : dst->sec_b);
  const uint32_t bit = 1u << iorb;
  std::vector<uint32_t> part((size_t)std::max<int64_t>(bd.size(), 1), 0xFFFFFFFFu);
  for (int64_t j = 0; j < bd.size(); j++) {
    const uint32_t t = (uint32_t)bd.states[j];
    if (create ? !(t & bit) : (t & bit) != 0u) continue;  // c^+ leaves the level occupied, c leaves it empty
    const uint32_t sst = t ^ bit;                         // source state
    const uint32_t sg = (__builtin_popcount(sst & (bit - 1u)) & 1) ? 0x80000000u : 0u;
    part[j] = (uint32_t)bs.rank(sst) | sg;
  }
  uint32_t* d_part = nullptr;
  if (dev_upload(&d_part, part.data(), part.size())) return 1;
  // up operator: the rows keep their down index (the source's rows fd .. are read); down operator: the partner table is
  // indexed by the destination's down index
  const int rc = ispin == 0 ? launch_apply_op_normal(dst->dim_up, cd, src->dim_up, 0, d_part, v_src_dev + fd * src->dim_up,
                                                     v_dst_dev, st, coef, accumulate)
                            : launch_apply_op_normal(dst->dim_up, cd, src->dim_up, 1, d_part + fd, v_src_dev, v_dst_dev, st,
                                                     coef, accumulate);
  (void)hipStreamSynchronize(st);
  (void)hipFree(d_part);
  return rc;
}

// the checks of one term of apply_Cops on superc / nonsu2 sectors, on the handles alone (no device is touched); windowed: a
// row window was asked for; gathered: as for apply_op_flat_term
static int flat_term_check(const edigpu_sector* src, const edigpu_sector* dst, int iorb, int ispin, int create, const char* who,
                           bool windowed, const ShardSrc* gathered) {
  const std::string w(who);
  if ((!src->is_flat_family()) || (!dst->is_flat_family()) || !src->built_by_library ||
      !dst->built_by_library) {
    set_error(w + ": both handles must be superc / nonsu2 sectors built by edigpu_flat_build or edigpu_direct_build");
    return 1;
  }
  if (src->nph != dst->nph || src->model.nph != dst->model.nph) {
    set_error(w + ": the two handles have different nph (" + std::to_string(src->nph) + " and " + std::to_string(dst->nph) + ")");
    return 1;
  }
  const int nblk = src->nph + 1;
  if (nblk > 1 && !gathered && (!src->is_whole() || !dst->is_whole() || windowed)) {
    set_error(w + ": phonon sectors are served as whole sectors only (no shards, no row window)");
    return 1;
  }
  const edigpu_model& m = src->model;
  const int ns = model_ns(m);
  if (iorb < 0 || iorb >= m.norb || ispin < 0 || ispin > 1 || dst->model.ed_mode != m.ed_mode ||
      model_ns(dst->model) != ns) {
    set_error(w + ": orbital / spin out of range or sectors of different models");
    return 1;
  }
  // superc: sector = Sz = Nup - Ndw; nonsu2: sector = Ntot
  const int d = create ? 1 : -1;
  const int want = m.ed_mode == 1 ? src->sec_a + (ispin == 0 ? d : -d) : src->sec_a + d;
  // Jz_basis=T: the operator also moves twoJz by the spin and the Lz of its level (ED_SECTOR.f90:289-350)
  const int want_jz = src->jz ? src->sec_b + d * twojz_of_level(iorb + ispin * ns, ns, m.norb) : 0;
  if (dst->sec_a != want || dst->jz != src->jz || (src->jz && dst->sec_b != want_jz)) {
    set_error(w + ": destination sector is not the one the operator leads to");
    return 1;
  }
  return 0;
}

// one operator of apply_Cops on superc / nonsu2 sectors (whole sectors or row shards of library-built ones): the
// destination's rows [fd, fd + cd), v_src_dev = the whole source vector (complex); gathered: v_src_dev is the all-gather
// of the ranks' padded chunks instead (shard_src.hpp, counted in double2), which phonon row shards need.  checked: the
// caller has made flat_term_check
static int apply_op_flat_term(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev, int iorb,
                              int ispin, int create, double cre, double cim, int accumulate, hipStream_t st, const char* who,
                              int64_t fd = 0, int64_t cd = -1, const ShardSrc* gathered = nullptr, bool checked = false) {
  const std::string w(who);
  if (!checked && flat_term_check(src, dst, iorb, ispin, create, who, fd != 0 || cd >= 0, gathered)) return 1;
  const int nblk = src->nph + 1;
  const int ns = model_ns(src->model);
  EDIGPU_HIP(hipSetDevice(src->device));
  HostDirect hs, hd;
  std::string e = build_direct(src->model, src->sec_a, 0, -1, hs, src->jz, src->sec_b, !src->sw.direct_nosort);
  if (e.empty()) e = build_direct(dst->model, dst->sec_a, 0, -1, hd, dst->jz, dst->sec_b, !dst->sw.direct_nosort);
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  if (cd < 0) cd = hd.dim - fd;
  if (fd < 0 || fd + cd > hd.dim) {
    set_error(w + ": row window outside the destination sector");
    return 1;
  }
  int32_t *d_states = nullptr, *d_off = nullptr, *d_rk = nullptr;
  int rc = dev_upload(&d_states, hd.states.data(), hd.states.size());
  rc |= dev_upload(&d_off, hs.off_dw.data(), hs.off_dw.size());
  rc |= dev_upload(&d_rk, hs.rk_up.data(), hs.rk_up.size());
  if (!rc)
    rc = launch_apply_op_flat(cd, ns, 1u << (iorb + ispin * ns), create, d_states + fd, d_off, d_rk, v_src_dev, v_dst_dev, st,
                              cre, cim, accumulate, nblk, hs.dim, gathered);  // phonon sectors: every electronic block, one launch
  (void)hipStreamSynchronize(st);
  dev_free_all(d_states, d_off, d_rk);
  return rc;
}

int apply_cops_rows_check(const edigpu_sector* src, const edigpu_sector* dst, int nops, const double* coef2, const int32_t* create,
                          const int32_t* iorb, const int32_t* ispin, const char* who, const ShardSrc* gathered) {
  for (int s = 0; s < nops; s++) {
    if (src->kind == kNormal) {
      if (coef2[2 * s + 1] != 0.0) {
        set_error(std::string(who) + ": complex coefficients belong to the _CMPLX_NORMAL build");
        return 1;
      }
      if (normal_term_check(src, dst, iorb[s], ispin[s], create[s] > 0, who)) return 1;
    } else if (flat_term_check(src, dst, iorb[s], ispin[s], create[s] > 0, who, true, gathered)) {
      return 1;
    }
  }
  return 0;
}

int apply_cops_rows(edigpu_sector* src, edigpu_sector* dst, const double* v_src_full, double* v_dst_rows, int64_t first,
                    int64_t count, int nops, const double* coef2, const int32_t* create, const int32_t* iorb,
                    const int32_t* ispin, hipStream_t st, const char* who, const ShardSrc* gathered, bool checked) {
  // every check of every operator once, before the first launch
  if (!checked && apply_cops_rows_check(src, dst, nops, coef2, create, iorb, ispin, who, gathered)) return 1;
  for (int s = 0; s < nops; s++) {
    if (src->kind == kNormal) {
      if (apply_op_normal_term(src, dst, v_src_full, v_dst_rows, iorb[s], ispin[s], create[s] > 0, coef2[2 * s], s > 0, st, who,
                               first, count, true))
        return 1;
    } else if (apply_op_flat_term(src, dst, v_src_full, v_dst_rows, iorb[s], ispin[s], create[s] > 0, coef2[2 * s],
                                  coef2[2 * s + 1], s > 0, st, who, first, count, gathered, true)) {
      return 1;
    }
  }
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_apply_op_normal(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev,
                           int iorb, int ispin, int create, void* stream) {
  if (!src || !dst || !v_src_dev || !v_dst_dev) {
    set_error("edigpu_apply_op_normal: NULL argument");
    return 1;
  }
  if (axisop_route(src, dst)) {  // phonon, complex and ed_total_ud=F sectors: kernels_axisop.hip
    const int32_t cr = create ? 1 : -1, io = iorb, sp = ispin;
    const double one = 1.0;
    return axisop_apply(src, dst, v_src_dev, v_dst_dev, 1, &one, nullptr, &cr, &io, &sp, (hipStream_t)stream,
                        "edigpu_apply_op_normal");
  }
  return apply_op_normal_term(src, dst, v_src_dev, v_dst_dev, iorb, ispin, create, 1.0, 0, (hipStream_t)stream,
                              "edigpu_apply_op_normal");
}

int edigpu_apply_cops_normal(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev,
                             int nops, const double* coef, const int32_t* create, const int32_t* iorb,
                             const int32_t* ispin, void* stream) {
  if (!src || !dst || !v_src_dev || !v_dst_dev || nops <= 0 || !coef || !create || !iorb || !ispin) {
    set_error("edigpu_apply_cops_normal: bad argument");
    return 1;
  }
  if (axisop_route(src, dst))  // phonon, complex and ed_total_ud=F sectors: all operators in one pass (kernels_axisop.hip)
    return axisop_apply(src, dst, v_src_dev, v_dst_dev, nops, coef, nullptr, create, iorb, ispin, (hipStream_t)stream,
                        "edigpu_apply_cops_normal");
  for (int s = 0; s < nops; s++)
    if (apply_op_normal_term(src, dst, v_src_dev, v_dst_dev, iorb[s], ispin[s], create[s] > 0, coef[s], s > 0,
                             (hipStream_t)stream, "edigpu_apply_cops_normal"))
      return 1;
  return 0;
}

int edigpu_apply_op_flat(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev,
                         int iorb, int ispin, int create, void* stream) {
  if (!src || !dst || !v_src_dev || !v_dst_dev) {
    set_error("edigpu_apply_op_flat: NULL argument");
    return 1;
  }
  if (!src->is_whole() || !dst->is_whole()) {
    set_error("edigpu_apply_op_flat: handles must hold whole sectors (single shard)");
    return 1;
  }
  return apply_op_flat_term(src, dst, v_src_dev, v_dst_dev, iorb, ispin, create, 1.0, 0.0, 0, (hipStream_t)stream,
                            "edigpu_apply_op_flat");
}

int edigpu_apply_cops_flat(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev, int nops,
                           const double* coef_re_im, const int32_t* create, const int32_t* iorb, const int32_t* ispin,
                           void* stream) {
  if (!src || !dst || !v_src_dev || !v_dst_dev || nops <= 0 || !coef_re_im || !create || !iorb || !ispin) {
    set_error("edigpu_apply_cops_flat: bad argument");
    return 1;
  }
  if (!src->is_whole() || !dst->is_whole()) {
    set_error("edigpu_apply_cops_flat: handles must hold whole sectors (single shard)");
    return 1;
  }
  for (int s = 0; s < nops; s++)
    if (apply_op_flat_term(src, dst, v_src_dev, v_dst_dev, iorb[s], ispin[s], create[s] > 0, coef_re_im[2 * s],
                           coef_re_im[2 * s + 1], s > 0, (hipStream_t)stream, "edigpu_apply_cops_flat"))
      return 1;
  return 0;
}

}  // extern "C"
