// edigpu_build.hip -- the entry points of the C ABI that create handles (from arrays handed over, or built from a model)
// and the exports of what a handle holds.  The device images are made by edigpu_setup.hip.
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "kernels.hpp"

namespace edigpu {

static std::string check_csr(int64_t nrow, int64_t ncol, const int64_t* rowptr, const int32_t* col,
                             const char* what) {
  if (!rowptr) return std::string(what) + ": rowptr is NULL";
  if (rowptr[0] != 0) return std::string(what) + ": rowptr[0] != 0";
  for (int64_t i = 0; i < nrow; i++)
    if (rowptr[i + 1] < rowptr[i]) return std::string(what) + ": rowptr not monotone";
  const int64_t nnz = rowptr[nrow];
  if (nnz > 0 && !col) return std::string(what) + ": col is NULL";
  for (int64_t k = 0; k < nnz; k++)
    if (col[k] < 0 || col[k] >= ncol) return std::string(what) + ": column index out of range";
  return "";
}

// phonon branches for a library-built superc / nonsu2 handle: g_el per row from the map of the rows it holds.  A row
// shard holds the same rows of every phonon block (dim_el = its electronic rows, the local block stride; the layout
// of spMatVec_mpi_superc_main / _nonsu2_main, i = i_el + (iph - 1) * MpiQ) and serves the sharded library calls only.
static int attach_phonons_flat(edigpu_sector* s, const edigpu_model& m, const std::vector<int32_t>& states, int ns) {
  if (m.nph <= 0) return 0;
  if (s->dim * (m.nph + 1) >= ((int64_t)1 << 31)) {
    set_error("sector dimension x (Nph+1) >= 2^31");
    return 1;
  }
  const bool offd = eph_offdiagonal(m);
  if (offd && !s->is_whole()) {
    set_error("phonons with a general g_ph(a,b) need the whole sector on one shard (density couplings shard)");
    return 1;
  }
  if (offd) {
    // general g_ab: the electron-phonon operator as a sector handle of the same kind (apply_eph_operator)
    const edigpu_model om = eph_operator_model(m);
    const int rc = s->kind == kDirect ? edigpu_direct_build(&s->sub_a, &om, s->sec_a, 0, -1)
                                : edigpu_flat_build(&s->sub_a, &om, s->sec_a, 0, -1);
    if (rc) return 1;
    if (hipMalloc((void**)&s->d_cz, (size_t)2 * (size_t)s->dim * sizeof(double)) != hipSuccess) {
      set_error("electron-phonon operator: out of device memory");
      return 1;
    }
  }
  std::vector<double> gel(states.size(), 0.0);
  for (size_t i = 0; !offd && i < states.size(); i++)
    for (int a = 0; a < m.norb; a++)
      gel[i] += m.g_ph[a * EDIGPU_MAXORB + a] * (double)(((states[i] >> a) & 1) + ((states[i] >> (a + ns)) & 1));
  if (dev_upload(&s->d_gu, gel.data(), gel.size())) return 1;
  s->nph = m.nph;
  s->w0_ph = m.w0_ph;
  s->a_ph = m.a_ph;
  s->dim_el = s->nloc;
  s->dim *= (m.nph + 1);
  s->nloc *= (m.nph + 1);
  return 0;
}

// edigpu_flat_build / edigpu_flat_build_jz: the stored image, generated on the device unless Switches::flat_hostbuild
static int flat_build_common(edigpu_handle* h, const edigpu_model* model, int sector, int64_t row_first, int64_t row_count,
                             bool jz, int twojz) {
  if (!h || !model) {
    set_error("edigpu_flat_build: NULL argument");
    return 1;
  }
  *h = nullptr;
  if (ensure_device()) return 1;
  const Switches sw = Switches::sample();
  if (jz && model->nph > 0) {
    set_error("edigpu_flat_build_jz: phonon sectors are not built in the Jz basis");
    return 1;
  }
  if (!sw.flat_hostbuild) {
    // generate the stored image on the device from the on-the-fly description (kernels_build.hip);
    // the host CSR builder below is the fallback and what edigpu_csr_export materialises
    HostDirect hd;
    std::string e = build_direct(*model, sector, row_first, row_count, hd, jz, twojz, !sw.direct_nosort);
    if (!e.empty()) {
      set_error(e);
      return 1;
    }
    if (hd.dim == 0) {
      set_error("edigpu_flat_build: empty sector");
      return 1;
    }
    SectorPtr s(new edigpu_sector(sw));
    s->kind = kFlat;
    s->is_complex = 1;
    s->device = current_device();
    s->dim = hd.dim;
    s->nloc = hd.row_count;
    s->row_first = hd.row_first;
    s->model = *model;
    s->sec_a = sector;
    s->sec_b = jz ? twojz : 0;
    s->jz = jz;
    s->built_by_library = true;
    s->lazy_export = true;
    const int rc = build_flat_on_device(s.get(), hd);
    if (rc == 0) {
      if (attach_phonons_flat(s.get(), *model, hd.states, hd.ns)) return 1;
      if (finish_handle(s.get())) return 1;
      *h = s.release();
      return 0;
    }
    if (rc == 1) return 1;
  }
  HostFlat hf;
  std::string e = build_flat(*model, sector, row_first, row_count, hf, jz, twojz);
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  if (hf.dim == 0) {
    set_error("edigpu_flat_build: empty sector");
    return 1;
  }
  SectorPtr s(new edigpu_sector(sw));
  s->model = *model;
  s->sec_a = sector;
  s->sec_b = jz ? twojz : 0;
  s->jz = jz;
  s->built_by_library = true;
  if (setup_flat(s.get(), hf.row_count, hf.dim, hf.row_first, hf.h.rowptr.data(), hf.h.col.data(),
                 hf.h.val.data(), 1))
    return 1;
  if (model->nph > 0) {
    HostDirect hd;  // for the sector map
    e = build_direct(*model, sector, row_first, row_count, hd, jz, twojz, !sw.direct_nosort);
    if (!e.empty()) set_error(e);
    if (!e.empty() || attach_phonons_flat(s.get(), *model, hd.states, hd.ns)) return 1;
  }
  *h = s.release();
  return 0;
}

static int direct_build_common(edigpu_handle* h, const edigpu_model* model, int sector, int64_t row_first, int64_t row_count,
                               bool jz, int twojz) {
  if (!h || !model) {
    set_error("edigpu_direct_build: NULL argument");
    return 1;
  }
  *h = nullptr;
  if (ensure_device()) return 1;
  const Switches sw = Switches::sample();
  HostDirect hd;
  std::string e = build_direct(*model, sector, row_first, row_count, hd, jz, twojz, !sw.direct_nosort);
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  SectorPtr s(new edigpu_sector(sw));
  s->kind = kDirect;
  s->model = *model;
  s->sec_a = sector;
  s->sec_b = jz ? twojz : 0;
  s->jz = jz;
  s->built_by_library = true;
  s->is_complex = 1;
  s->device = current_device();
  s->dim = hd.dim;
  s->nloc = hd.row_count;
  s->row_first = hd.row_first;
  s->dir_ns = hd.ns;
  s->dir_norb = hd.norb;
  s->dir_nterms = (int)hd.terms.size();
  int rc = dev_upload(&s->d_dir_states, hd.states.data(), hd.states.size());
  rc |= dev_upload(&s->d_dir_offdw, hd.off_dw.data(), hd.off_dw.size());
  rc |= dev_upload(&s->d_dir_rkup, hd.rk_up.data(), hd.rk_up.size());
  rc |= dev_upload(&s->d_dir_terms, hd.terms.data(), hd.terms.size());
  {
    std::vector<uint2> tests((hd.terms.size() + 31) / 32 * 32, make_uint2(0xFFFFFFFFu, 0u));  // padding never matches
    for (size_t t = 0; t < hd.terms.size(); t++)
      tests[t] = make_uint2(hd.terms[t].need_set, hd.terms[t].need_set | hd.terms[t].need_clear);
    if (tests.empty()) tests.assign(32, make_uint2(0xFFFFFFFFu, 0u));
    rc |= dev_upload(&s->d_dir_tests, tests.data(), tests.size());
  }
  rc |= dev_upload(&s->d_dir_dtab, hd.dtab.data(), hd.dtab.size());
  rc |= dev_upload(&s->d_dir_xtab, hd.xtab.data(), hd.xtab.size());
  if (rc || attach_phonons_flat(s.get(), *model, hd.states, hd.ns) || finish_handle(s.get())) return 1;
  *h = s.release();
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_normal_create(edigpu_handle* h, int64_t dim_up, int64_t dim_dw, int64_t dw_first,
                         int64_t dw_count, const double* hd, const int64_t* up_rowptr,
                         const int32_t* up_col, const double* up_val, const int64_t* dw_rowptr,
                         const int32_t* dw_col, const double* dw_val, const int64_t* nd_rowptr,
                         const int32_t* nd_col, const double* nd_val) {
  if (!h) {
    set_error("edigpu_normal_create: handle pointer is NULL");
    return 1;
  }
  *h = nullptr;
  if (ensure_device()) return 1;
  const Switches sw = Switches::sample();
  if (dim_up <= 0 || dim_dw <= 0 || dw_first < 0 || dw_count < 0 || dw_first + dw_count > dim_dw) {
    set_error("edigpu_normal_create: inconsistent dimensions");
    return 1;
  }
  if (dim_up * dim_dw >= ((int64_t)1 << 31)) {
    set_error("edigpu_normal_create: sector dimension >= 2^31");
    return 1;
  }
  if (!hd && dw_count > 0) {
    set_error("edigpu_normal_create: hd is NULL");
    return 1;
  }
  std::string e = check_csr(dim_up, dim_up, up_rowptr, up_col, "edigpu_normal_create(up)");
  if (e.empty()) e = check_csr(dim_dw, dim_dw, dw_rowptr, dw_col, "edigpu_normal_create(dw)");
  if (e.empty() && nd_rowptr)
    e = check_csr(dim_up * dw_count, dim_up * dim_dw, nd_rowptr, nd_col, "edigpu_normal_create(nd)");
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  HostCsr up, dw;
  up.nrow = up.ncol = dim_up;
  up.rowptr.assign(up_rowptr, up_rowptr + dim_up + 1);
  up.col.assign(up_col, up_col + up_rowptr[dim_up]);
  up.val.assign(up_val, up_val + up_rowptr[dim_up]);
  dw.nrow = dw.ncol = dim_dw;
  dw.rowptr.assign(dw_rowptr, dw_rowptr + dim_dw + 1);
  dw.col.assign(dw_col, dw_col + dw_rowptr[dim_dw]);
  dw.val.assign(dw_val, dw_val + dw_rowptr[dim_dw]);
  // The arrays of an impurity model have the structure the library's own builder emits (separable diagonal, Hnd a short
  // sum of signed partial permutations): recover it and run the factored kernels; anything else keeps the explicit
  // image.
  HostNormal hn;
  bool fact = false;
  {
    if (sw.handover_factor && !sw.normal_explicit)
      fact = factor_handover(dim_up, dim_dw, dw_first, dw_count, hd, nd_rowptr, nd_col, nd_val, 16, hn.fac);
    if (fact) {  // the arrays as given stay on the host for edigpu_normal_export
      const int64_t nloc = dim_up * dw_count;
      hn.hd.assign(hd, hd + nloc);
      if (nd_rowptr && nd_rowptr[nloc] > 0) {
        hn.nd.nrow = nloc;
        hn.nd.ncol = dim_up * dim_dw;
        hn.nd.rowptr.assign(nd_rowptr, nd_rowptr + nloc + 1);
        hn.nd.col.assign(nd_col, nd_col + nd_rowptr[nloc]);
        hn.nd.val.assign(nd_val, nd_val + nd_rowptr[nloc]);
      }
    }
  }
  SectorPtr s(new edigpu_sector(sw));
  if (setup_normal(s.get(), dim_up, dim_dw, dw_first, dw_count, hd, up, dw, nd_rowptr, nd_col, nd_val,
                   fact ? &hn : nullptr))
    return 1;
  *h = s.release();
  return 0;
}

static int csr_create_any(edigpu_handle* h, int64_t nrow_local, int64_t ncol_global,
                          int64_t row_first, const int64_t* rowptr, const int32_t* col,
                          const double* val, int cplx) {
  if (!h) {
    set_error("edigpu_csr_create: handle pointer is NULL");
    return 1;
  }
  *h = nullptr;
  if (ensure_device()) return 1;
  const Switches sw = Switches::sample();
  if (nrow_local < 0 || ncol_global <= 0 || row_first < 0 || row_first + nrow_local > ncol_global) {
    set_error("edigpu_csr_create: inconsistent dimensions");
    return 1;
  }
  if (ncol_global >= ((int64_t)1 << 31)) {
    set_error("edigpu_csr_create: dimension >= 2^31");
    return 1;
  }
  std::string e = check_csr(nrow_local, ncol_global, rowptr, col, "edigpu_csr_create");
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  SectorPtr s(new edigpu_sector(sw));
  if (setup_flat(s.get(), nrow_local, ncol_global, row_first, rowptr, col, val, cplx)) return 1;
  *h = s.release();
  return 0;
}

int edigpu_csr_create_d(edigpu_handle* h, int64_t nrow_local, int64_t ncol_global,
                        int64_t row_first, const int64_t* rowptr, const int32_t* col,
                        const double* val) {
  return csr_create_any(h, nrow_local, ncol_global, row_first, rowptr, col, val, 0);
}

int edigpu_csr_create_z(edigpu_handle* h, int64_t nrow_local, int64_t ncol_global,
                        int64_t row_first, const int64_t* rowptr, const int32_t* col,
                        const double* val_re_im) {
  return csr_create_any(h, nrow_local, ncol_global, row_first, rowptr, col, val_re_im, 1);
}

int edigpu_normal_build(edigpu_handle* h, const edigpu_model* model, int nup, int ndw,
                        int64_t dw_first, int64_t dw_count) {
  if (!h || !model) {
    set_error("edigpu_normal_build: NULL argument");
    return 1;
  }
  *h = nullptr;
  if (ensure_device()) return 1;
  const Switches sw = Switches::sample();
  HostNormal hn;
  // the O(Dim) explicit images (hd, Hnd CSR) are skipped when the kernels run on the factored tables
  bool lazy = !sw.normal_explicit;
  std::string e = build_normal(*model, nup, ndw, dw_first, dw_count, hn, !lazy, !sw.nd_no_merge);
  if (e.empty() && lazy && hn.fac.nterms > 16) {
    lazy = false;
    e = build_normal(*model, nup, ndw, dw_first, dw_count, hn, true, !sw.nd_no_merge);
  }
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  SectorPtr s(new edigpu_sector(sw));
  s->model = *model;
  s->sec_a = nup;
  s->sec_b = ndw;
  s->built_by_library = true;
  s->lazy_export = lazy;
  if (setup_normal(s.get(), hn.dim_up, hn.dim_dw, hn.dw_first, hn.dw_count, lazy ? nullptr : hn.hd.data(), hn.up,
                   hn.dw, (!lazy && hn.has_nd) ? hn.nd.rowptr.data() : nullptr, hn.nd.col.data(),
                   hn.nd.val.data(), &hn))
    return 1;
  if (model->nph > 0) {
    // phonon branches: (Nph + 1) electronic blocks per vector; density couplings only
    if (s->dw_count != s->dim_dw) {
      set_error("edigpu_normal_build: phonons (nph > 0) need the whole sector on one shard");
      return 1;
    }
    // density couplings g_aa: per-row tables inside the phonon pass.  A general g_ab (GPHFILE in the reference):
    // the whole electron-phonon operator as its own sector handle (apply_eph_operator), the tables stay zero.
    const bool offd = eph_offdiagonal(*model);
    std::vector<double> gu((size_t)hn.dim_up, 0.0), gd((size_t)hn.dim_dw, 0.0);
    for (int64_t i = 0; !offd && i < hn.dim_up; i++)
      for (int a = 0; a < model->norb; a++)
        if ((hn.bup.states[i] >> a) & 1) gu[i] += model->g_ph[a * EDIGPU_MAXORB + a];
    for (int64_t i = 0; !offd && i < hn.dim_dw; i++)
      for (int a = 0; a < model->norb; a++)
        if ((hn.bdw.states[i] >> a) & 1) gd[i] += model->g_ph[a * EDIGPU_MAXORB + a];
    if (offd) {
      const edigpu_model om = eph_operator_model(*model);
      if (edigpu_normal_build(&s->sub_a, &om, nup, ndw, 0, -1) ||
          hipMalloc((void**)&s->d_cz, (size_t)s->dim * sizeof(double)) != hipSuccess) {
        if (!have_error()) set_error("edigpu_normal_build: electron-phonon operator: out of device memory");
        return 1;
      }
    }
    if (dev_upload(&s->d_gu, gu.data(), gu.size()) || dev_upload(&s->d_gd, gd.data(), gd.size())) return 1;
    if (s->dim * (model->nph + 1) >= ((int64_t)1 << 31)) {
      set_error("edigpu_normal_build: sector dimension x (Nph+1) >= 2^31");
      return 1;
    }
    s->nph = model->nph;
    s->w0_ph = model->w0_ph;
    s->a_ph = model->a_ph;
    s->dim_el = s->dim;
    s->dim *= (model->nph + 1);
    s->nloc = s->dim;
  }
  *h = s.release();
  return 0;
}

int edigpu_normal_build_z(edigpu_handle* h, const edigpu_model* model, int nup, int ndw) {
  if (!h || !model) {
    set_error("edigpu_normal_build_z: NULL argument");
    return 1;
  }
  *h = nullptr;
  const Switches sw = Switches::sample();
  if (model->ed_mode != 0) {
    set_error("edigpu_normal_build_z: ed_mode must be normal");
    return 1;
  }
  if (model->nph > 0) {
    set_error("edigpu_normal_build_z: phonons are not supported with complex algebra");
    return 1;
  }
  // the two real sectors stay with hs, ha until the composite takes them as its sub-handles
  edigpu_handle built = nullptr;
  if (edigpu_normal_build(&built, model, nup, ndw, 0, -1)) return 1;
  SectorPtr hs(built), ha;
  bool any = false;
  const edigpu_model mi = imag_part_model(*model, any);
  if (any) {
    if (edigpu_normal_build(&built, &mi, nup, ndw, 0, -1)) return 1;
    ha.reset(built);
  }
  SectorPtr s(new edigpu_sector(sw));
  s->kind = kCmplxNormal;
  s->is_complex = 1;
  s->device = current_device();
  s->dim = s->nloc = hs->dim;
  s->dim_up = hs->dim_up;
  s->dim_dw = hs->dim_dw;
  s->model = *model;
  s->sec_a = nup;
  s->sec_b = ndw;
  s->built_by_library = true;
  s->sub_s = hs.release();
  s->sub_a = ha.release();
  // The complex operator as one real sector on the doubled up index: one pass over 2 Dim elements instead of four
  // real products and two layout passes.  Switches::cmplx_fourproducts, or more than 16 factored terms (complex replica
  // matrices with many imaginary inter-orbital hops), keep the composite above.
  if (!sw.cmplx_fourproducts && !sw.normal_explicit) {
    HostNormal hd2;
    const std::string e2 = build_normal_doubled(*model, nup, ndw, hd2, 16, !sw.nd_no_merge);
    if (e2.empty()) {
      SectorPtr sd(new edigpu_sector(sw));
      if (setup_normal(sd.get(), hd2.dim_up, hd2.dim_dw, 0, hd2.dim_dw, nullptr, hd2.up, hd2.dw, nullptr, nullptr, nullptr,
                       &hd2))
        return 1;
      s->sub_d = sd.release();
    }
  }
  if (!s->sub_d &&  // planar work vectors of the four-product composite
      hipMalloc((void**)&s->d_cz, (size_t)6 * (size_t)std::max<int64_t>(s->dim, 1) * sizeof(double)) != hipSuccess) {
    set_error("edigpu_normal_build_z: out of device memory");
    return 1;
  }
  if (finish_handle(s.get())) return 1;
  *h = s.release();
  return 0;
}

int edigpu_flat_build(edigpu_handle* h, const edigpu_model* model, int sector, int64_t row_first,
                      int64_t row_count) {
  return flat_build_common(h, model, sector, row_first, row_count, false, 0);
}

int edigpu_flat_build_jz(edigpu_handle* h, const edigpu_model* model, int ntot, int twojz, int64_t row_first,
                         int64_t row_count) {
  return flat_build_common(h, model, ntot, row_first, row_count, true, twojz);
}

int edigpu_direct_build(edigpu_handle* h, const edigpu_model* model, int sector, int64_t row_first,
                        int64_t row_count) {
  return direct_build_common(h, model, sector, row_first, row_count, false, 0);
}

int edigpu_direct_build_jz(edigpu_handle* h, const edigpu_model* model, int ntot, int twojz, int64_t row_first,
                           int64_t row_count) {
  return direct_build_common(h, model, ntot, row_first, row_count, true, twojz);
}

int edigpu_orbs_build(edigpu_handle* h, const edigpu_model* model, const int32_t* nups, const int32_t* ndws) {
  return edigpu_orbs_build_rows(h, model, nups, ndws, 0, -1);
}

int edigpu_orbs_build_rows(edigpu_handle* h, const edigpu_model* model, const int32_t* nups, const int32_t* ndws,
                           int64_t row_first, int64_t row_count) {
  if (!h || !model || !nups || !ndws) {
    set_error("edigpu_orbs_build: NULL argument");
    return 1;
  }
  *h = nullptr;
  if (ensure_device()) return 1;
  const Switches sw = Switches::sample();
  HostOrbs ho;
  std::string e = build_orbs(*model, nups, ndws, ho);
  if (!e.empty()) {
    set_error(e);
    return 1;
  }
  if (ho.dim == 0) {
    set_error("edigpu_orbs_build: empty sector");
    return 1;
  }
  if (row_count < 0) row_count = ho.dim - row_first;
  if (row_first < 0 || row_count < 0 || row_first + row_count > ho.dim) {
    set_error("edigpu_orbs_build_rows: row range outside the sector");
    return 1;
  }
  SectorPtr s(new edigpu_sector(sw));
  s->model = *model;
  if (setup_orbs(s.get(), ho, nullptr)) return 1;
  s->row_first = row_first;  // the factored tables describe the whole sector; only the rows computed differ
  s->nloc = row_count;
  s->orbs_nups.assign(nups, nups + model->norb);
  s->orbs_ndws.assign(ndws, ndws + model->norb);
  *h = s.release();
  return 0;
}

int edigpu_orbs_create(edigpu_handle* h, int naxes, const int64_t* dims, const double* hd,
                       const int64_t* fac_rowptr, const int32_t* fac_col, const double* fac_val) {
  if (!h || !dims || !hd || !fac_rowptr) {
    set_error("edigpu_orbs_create: NULL argument");
    return 1;
  }
  *h = nullptr;
  if (ensure_device()) return 1;
  const Switches sw = Switches::sample();
  if (naxes < 2 || naxes > kOrbsMaxAxes || (naxes & 1)) {
    set_error("edigpu_orbs_create: naxes must be 2*Norb <= 2*EDIGPU_MAXORB");
    return 1;
  }
  HostOrbs ho;
  ho.naxes = naxes;
  ho.dims.assign(dims, dims + naxes);
  ho.fac.resize(naxes);
  ho.dim = 1;
  int64_t row0 = 0;
  for (int k = 0; k < naxes; k++) {
    const int64_t d = dims[k];
    if (d < 1 || ho.dim * d >= ((int64_t)1 << 31)) {
      set_error("edigpu_orbs_create: bad factor dimension / sector dimension >= 2^31");
      return 1;
    }
    ho.dim *= d;
    HostCsr& f = ho.fac[k];
    f.nrow = f.ncol = d;
    f.rowptr.resize(d + 1);
    const int64_t b0 = fac_rowptr[row0];
    for (int64_t i = 0; i <= d; i++) {
      f.rowptr[i] = fac_rowptr[row0 + i] - b0;
      if (i > 0 && f.rowptr[i] < f.rowptr[i - 1]) {
        set_error("edigpu_orbs_create: fac_rowptr not monotone");
        return 1;
      }
    }
    const int64_t nnz = f.rowptr[d];
    if (nnz > 0 && (!fac_col || !fac_val)) {
      set_error("edigpu_orbs_create: fac_col/fac_val NULL");
      return 1;
    }
    f.col.assign(fac_col + b0, fac_col + b0 + nnz);
    f.val.assign(fac_val + b0, fac_val + b0 + nnz);
    for (int32_t c : f.col)
      if (c < 0 || c >= d) {
        set_error("edigpu_orbs_create: column index out of range");
        return 1;
      }
    row0 += d;
  }
  SectorPtr s(new edigpu_sector(sw));
  if (setup_orbs(s.get(), ho, hd)) return 1;
  *h = s.release();
  return 0;
}

static int download_csr(const DevCsr& d, int64_t* rowptr, int32_t* col, double* val, int w) {
  if (rowptr) {
    if (d.nrow == 0) {
      rowptr[0] = 0;
    } else if (d.wide) {
      EDIGPU_HIP(hipMemcpy(rowptr, d.rowptr64, ((size_t)d.nrow + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    } else {
      std::vector<int32_t> rp((size_t)d.nrow + 1);
      EDIGPU_HIP(hipMemcpy(rp.data(), d.rowptr32, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i <= d.nrow; i++) rowptr[i] = rp[i];
    }
  }
  if (col && d.nnz) EDIGPU_HIP(hipMemcpy(col, d.col, (size_t)d.nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (val && d.nnz) EDIGPU_HIP(hipMemcpy(val, d.val, (size_t)d.nnz * w * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int edigpu_normal_export(edigpu_handle s, double* hd, int64_t* up_rowptr, int32_t* up_col,
                         double* up_val, int64_t* dw_rowptr, int32_t* dw_col, double* dw_val,
                         int64_t* nd_rowptr, int32_t* nd_col, double* nd_val) {
  if (!s || s->kind != kNormal) {
    set_error("edigpu_normal_export: not a normal-mode handle");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  if (s->lazy_export && s->factored) {
    // first export of a factored sector: materialise the explicit images from the stored model
    HostNormal hn;
    std::string e = build_normal(s->model, s->sec_a, s->sec_b, s->dw_first, s->dw_count, hn, true, !s->sw.nd_no_merge);
    if (!e.empty()) {
      set_error(e);
      return 1;
    }
    s->h_hd = std::move(hn.hd);
    s->h_nd = std::move(hn.nd);
    s->lazy_export = false;
  }
  if (hd && s->nloc) {
    if (s->factored)
      std::copy(s->h_hd.begin(), s->h_hd.end(), hd);
    else
      EDIGPU_HIP(hipMemcpy(hd, s->d_hd, (size_t)(s->has_phonons() ? s->dim_el : s->nloc) * sizeof(double),
                           hipMemcpyDeviceToHost));  // the electronic diagonal (one phonon block)
  }
  auto cp = [](const HostCsr& a, int64_t* rp, int32_t* c, double* v) {
    if (rp) std::copy(a.rowptr.begin(), a.rowptr.end(), rp);
    if (c) std::copy(a.col.begin(), a.col.end(), c);
    if (v) std::copy(a.val.begin(), a.val.end(), v);
  };
  cp(s->h_up, up_rowptr, up_col, up_val);
  cp(s->h_dw, dw_rowptr, dw_col, dw_val);
  if (s->has_nd && s->factored) {
    cp(s->h_nd, nd_rowptr, nd_col, nd_val);
    return 0;
  }
  if (s->has_nd) return download_csr(s->nd, nd_rowptr, nd_col, nd_val, 1);
  if (nd_rowptr)
    for (int64_t i = 0; i <= s->nloc; i++) nd_rowptr[i] = 0;
  return 0;
}

int edigpu_csr_export(edigpu_handle s, int64_t* rowptr, int32_t* col, double* val) {
  if (!s || s->kind != kFlat) {
    set_error("edigpu_csr_export: not a flat-CSR handle (direct handles store no matrix)");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  if (s->lazy_export) {
    // device-built sector: the CSR image only exists if somebody asks for it
    HostFlat hf;
    // (phonon sectors: the electronic block, as edigpu_normal_export hands back the electronic factors)
    std::string e = build_flat(s->model, s->sec_a, s->row_first, s->has_phonons() ? s->dim_el : s->nloc, hf, s->jz, s->sec_b);
    if (!e.empty()) {
      set_error(e);
      return 1;
    }
    if (rowptr) std::copy(hf.h.rowptr.begin(), hf.h.rowptr.end(), rowptr);
    if (col) std::copy(hf.h.col.begin(), hf.h.col.end(), col);
    if (val) std::copy(hf.h.val.begin(), hf.h.val.end(), val);
    return 0;
  }
  const int w = s->is_complex ? 2 : 1;
  const int64_t n = s->nloc;
  std::vector<int64_t> rl((size_t)n + 1), rn((size_t)n + 1);
  std::vector<int32_t> cl((size_t)s->loc.nnz), cn((size_t)s->nonloc.nnz);
  std::vector<double> vl((size_t)s->loc.nnz * w), vn((size_t)s->nonloc.nnz * w);
  if (download_csr(s->loc, rl.data(), cl.data(), vl.data(), w)) return 1;
  if (download_csr(s->nonloc, rn.data(), cn.data(), vn.data(), w)) return 1;
  int64_t p = 0;
  if (rowptr) rowptr[0] = 0;
  for (int64_t i = 0; i < n; i++) {
    for (int64_t k = rl[i]; k < rl[i + 1]; k++, p++) {
      if (col) col[p] = (int32_t)(cl[k] + s->row_first);
      if (val)
        for (int q = 0; q < w; q++) val[p * w + q] = vl[k * w + q];
    }
    for (int64_t k = rn[i]; k < rn[i + 1]; k++, p++) {
      if (col) col[p] = cn[k];
      if (val)
        for (int q = 0; q < w; q++) val[p * w + q] = vn[k * w + q];
    }
    if (rowptr) rowptr[i + 1] = p;
  }
  return 0;
}

}  // extern "C"
