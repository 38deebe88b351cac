// edigpu_ph.hip -- C ABI of the phonon operators (include/edigpu.h: edigpu_apply_xph, edigpu_ph_rdm, edigpu_time_ph):
// checks, the handle's lazily built tables (host_ph.hpp), launches (kernels_ph.hip).
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_occ.hpp"
#include "host_ph.hpp"
#include "kernels.hpp"

namespace edigpu {

struct PhDev {
  int norb = 0, dimph = 0, ncls = 0, nunits = 0, cplx = 0;
  bool planned = false;  // the Gram kernel's tables and workspace are there (DimPh <= kPhMaxDim)
  int64_t dim_el = 0, dim_cols = 0;
  double* sq = nullptr;
  int32_t *rorder = nullptr, *corder = nullptr, *ubeg = nullptr;
  PhUnit* units = nullptr;
  double *partial = nullptr, *sums = nullptr;
  // shard view (edigpu_sector::ph_shard): the rows it was built for, and the sums of several vectors side by side
  int64_t first = 0, count = 0;
  double* sums_all = nullptr;
  int64_t sums_all_cap = 0;
};

static void free_ph_view(PhDev*& p) {
  if (!p) return;
  dev_free_all(p->sq, p->rorder, p->corder, p->ubeg, p->units, p->partial, p->sums, p->sums_all);
  delete p;
  p = nullptr;
}

void free_ph(edigpu_sector* s) {
  if (!s) return;
  free_ph_view(s->ph);
  free_ph_view(s->ph_shard);
}

static int no_phonons(const edigpu_sector* s, const std::string& who) {
  if (!s->has_phonons()) {
    set_error(who + ": the handle has no phonons (nph = 0)");
    return 1;
  }
  return 0;
}

static int dimph_over(const edigpu_sector* s, const std::string& who) {
  if (s->nph + 1 > kPhMaxDim) {
    set_error(who + ": DimPh = " + std::to_string(s->nph + 1) + " exceeds the limit of " + std::to_string(kPhMaxDim));
    return 1;
  }
  return 0;
}

static int ph_refuse(const edigpu_sector* s, const std::string& who) { return occ_refuse(s, who) || no_phonons(s, who); }

int ph_refuse_kind(const edigpu_sector* s, const std::string& who, bool rdm) {
  return occ_refuse_kind(s, who) || no_phonons(s, who) || (rdm && dimph_over(s, who));
}

// the handle's tables, built on first use: the sqrt table always, the Gram kernel's plan when `plan` asks for it
// (view = s->ph: the whole sector; view = s->ph_shard: the rows [first, first + count), indices local to them)
static int ph_build(edigpu_sector* s, const std::string& who, bool plan, PhDev*& view, int64_t first, int64_t count) {
  const edigpu_model& m = s->model;
  const bool shard = &view == &s->ph_shard;
  auto fail = [&](const std::string& why) {
    set_error(who + ": " + why);
    free_ph_view(view);
    return 1;
  };
  if (shard && view && (view->first != first || view->count != count)) free_ph_view(view);
  if (!view) {
    if (m.norb < 1 || m.norb > kOccMaxOrb) {
      set_error(who + ": norb out of range");
      return 1;
    }
    PhDev* p = new PhDev();
    view = p;  // freed by edigpu_destroy also when the build stops half-way
    p->norb = m.norb;
    p->dimph = s->nph + 1;
    p->cplx = s->is_complex;
    p->first = first;
    p->count = count;
    p->dim_el = shard ? count * (s->is_flat_family() ? 1 : s->dim_up) : s->dim_el;
    p->ncls = ph_num_classes(m.norb);
    if (!shard && (p->dim_el <= 0 || p->dim_el * p->dimph != s->dim))
      return fail("the handle's phonon blocks do not add up to its dimension");
    std::vector<double> sq((size_t)p->dimph + 1);
    ph_sqrt_table(p->dimph, sq.data());
    if (dev_upload(&p->sq, sq)) return fail(edigpu_last_error());
  }
  PhDev* p = view;
  if (!plan || p->planned) return 0;
  int ncu = 0;
  EDIGPU_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device));
  // about eight units per compute unit on large sectors, and units long enough to pay for the reduction at their end
  const int64_t target = std::max<int64_t>(2048, p->dim_el / (std::max(ncu, 1) * 8));
  PhPlan pl;
  if (s->is_flat_family()) {
    const int64_t whole = s->dim / p->dimph;  // electronic rows of the sector (dim_el of a phonon shard is the shard's)
    std::vector<int32_t> map((size_t)whole);
    int64_t n = whole;
    if (s->jz ? edigpu_sector_map_jz(&m, s->sec_a, s->sec_b, map.data(), &n) : edigpu_sector_map(&m, s->sec_a, 0, 0, map.data(), &n))
      return 1;  // the map's message stands
    if (n != whole) return fail("the sector map does not have the handle's dimension");
    std::vector<uint16_t> pat(map.size());
    occ_patterns_state(map.data(), n, m.norb, model_ns(m), pat.data());
    if (shard) ph_shard_plan_flat(pat.data(), n, first, count, m.norb, target, pl);
    else ph_plan_flat(pat.data(), n, m.norb, target, pl);
  } else {
    std::vector<int32_t> mu((size_t)s->dim_up), md((size_t)s->dim_dw);
    int64_t nu = s->dim_up, nd = s->dim_dw;
    if (edigpu_sector_map(&m, s->sec_a, s->sec_b, 0, mu.data(), &nu) || edigpu_sector_map(&m, s->sec_a, s->sec_b, 1, md.data(), &nd))
      return 1;
    if (nu != s->dim_up || nd != s->dim_dw || (!shard && nu * nd != p->dim_el))
      return fail("the sector maps do not have the handle's dimensions");
    std::vector<uint16_t> pu(mu.size()), pd(md.size());
    occ_patterns_word(mu.data(), nu, m.norb, pu.data());
    occ_patterns_word(md.data(), nd, m.norb, pd.data());
    if (shard) ph_shard_plan_normal(pu.data(), nu, pd.data(), nd, first, count, m.norb, target, pl);
    else ph_plan_normal(pu.data(), nu, pd.data(), nd, m.norb, target, pl);
  }
  if (shard && pl.dim_rows * pl.dim_cols != p->dim_el) return fail("the rows are not inside the sector");
  p->dim_cols = pl.dim_cols;
  p->nunits = (int)pl.units.size();
  const size_t nslot = (size_t)ph_slots(p->dimph) * (p->cplx ? 2 : 1);
  if (dev_upload(&p->rorder, pl.rorder) || dev_upload(&p->corder, pl.corder) || dev_upload(&p->ubeg, pl.ubeg) ||
      dev_upload(&p->units, pl.units))
    return fail(edigpu_last_error());
  if (hipMalloc((void**)&p->partial, std::max<size_t>(1, (size_t)p->nunits) * nslot * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&p->sums, (size_t)p->ncls * nslot * sizeof(double)) != hipSuccess)
    return fail("out of device memory for the partial sums");
  p->planned = true;
  return 0;
}

static int ph_overlap(const edigpu_sector* s, const double* src, const double* dst, const std::string& who) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
  const uintptr_t len = (uintptr_t)s->dim * (s->is_complex ? 16 : 8);
  if (a < b + len && b < a + len) {
    set_error(who + ": the destination must not overlap the source (an output block reads its two neighbours)");
    return 1;
  }
  return 0;
}

static PhTables ph_args(const PhDev* p) {
  PhTables t;
  t.cplx = p->cplx;
  t.dimph = p->dimph;
  t.nunits = p->nunits;
  t.ncls = p->ncls;
  t.dim_el = p->dim_el;
  t.dim_cols = p->dim_cols;
  t.sq = p->sq;
  t.rorder = p->rorder;
  t.corder = p->corder;
  t.ubeg = p->ubeg;
  t.units = p->units;
  return t;
}

static int ph_rdm_checks(edigpu_sector* s, const std::string& who) {
  if (ph_refuse(s, who) || dimph_over(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  return ph_build(s, who, true, s->ph, 0, 0);
}

int ph_shard_apply(edigpu_sector* s, int64_t first, int64_t count, const double* src_dev, double* dst_dev, const std::string& who) {
  if (count <= 0) return 0;
  if (ph_build(s, who, false, s->ph_shard, first, count)) return 1;
  return launch_apply_xph(ph_args(s->ph_shard), src_dev, dst_dev, s->stream);
}

int ph_shard_rdm(edigpu_sector* s, int64_t first, int64_t count, const double* v_dev, int nvec, const double** sums_dev,
                 const std::string& who) {
  *sums_dev = nullptr;
  if (count <= 0) return 0;
  if (ph_build(s, who, true, s->ph_shard, first, count)) return 1;
  PhDev* p = s->ph_shard;
  const PhTables t = ph_args(p);
  const int cw = p->cplx ? 2 : 1;
  const int64_t per = (int64_t)p->ncls * ph_slots(p->dimph) * cw, vstride = p->dim_el * p->dimph * cw;
  if (dev_grow(&p->sums_all, &p->sums_all_cap, per * nvec)) return 1;
  // one vector after the other through the same workspace, as edigpu_ph_rdm does
  for (int k = 0; k < nvec; k++) {
    if (launch_ph_rdm(t, v_dev + (int64_t)k * vstride, p->partial, p->sums, s->stream)) return 1;
    EDIGPU_HIP(hipMemcpyAsync(p->sums_all + (int64_t)k * per, p->sums, (size_t)per * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  }
  *sums_dev = p->sums_all;
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_apply_xph(edigpu_handle s, const double* v_src_dev, double* v_dst_dev, void* stream) {
  const std::string who = "edigpu_apply_xph";
  if (!s || !v_src_dev || !v_dst_dev) {
    set_error(who + ": NULL argument");
    return 1;
  }
  if (ph_refuse(s, who)) return 1;
  if (ph_overlap(s, v_src_dev, v_dst_dev, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ph_build(s, who, false, s->ph, 0, 0)) return 1;
  return launch_apply_xph(ph_args(s->ph), v_src_dev, v_dst_dev, (hipStream_t)stream);
}

int edigpu_ph_rdm(edigpu_handle s, const double* v_dev, int nvec, double* rho_host, double* norm2_host) {
  const std::string who = "edigpu_ph_rdm";
  if (!s || !v_dev || !rho_host || nvec <= 0) {
    set_error(who + (!s || !v_dev || !rho_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  if (ph_rdm_checks(s, who)) return 1;
  const PhDev* p = s->ph;
  const PhTables t = ph_args(s->ph);
  const int cw = p->cplx ? 2 : 1;
  const size_t nslot = (size_t)ph_slots(p->dimph) * cw, nmat = (size_t)p->dimph * p->dimph * cw;
  const int64_t vstride = s->dim * cw;
  // one vector after the other through the same workspace: nvec vectors are nvec single calls, bit for bit
  std::vector<double> sums((size_t)nvec * p->ncls * nslot);
  for (int k = 0; k < nvec; k++) {
    if (launch_ph_rdm(t, v_dev + (int64_t)k * vstride, p->partial, p->sums, s->stream)) return 1;
    EDIGPU_HIP(hipMemcpyAsync(sums.data() + (size_t)k * p->ncls * nslot, p->sums, (size_t)p->ncls * nslot * sizeof(double),
                              hipMemcpyDeviceToHost, s->stream));
  }
  EDIGPU_HIP(hipStreamSynchronize(s->stream));
  for (int k = 0; k < nvec; k++) {
    double tr = 0.0;
    for (int c = 0; c < p->ncls; c++)
      tr += ph_expand_slots(sums.data() + ((size_t)k * p->ncls + c) * nslot, p->dimph, cw, rho_host + ((size_t)k * p->ncls + c) * nmat);
    if (norm2_host) norm2_host[k] = tr;
  }
  return 0;
}

int edigpu_time_ph(edigpu_handle s, const double* v_dev, double* w_dev, int warmup, int steps, double* ms2) {
  const std::string who = "edigpu_time_ph";
  if (!s || !v_dev || !w_dev || !ms2 || warmup < 0 || steps <= 0) {
    set_error(who + ": bad argument");
    return 1;
  }
  if (ph_overlap(s, v_dev, w_dev, who) || ph_rdm_checks(s, who)) return 1;
  const PhDev* p = s->ph;
  const PhTables t = ph_args(s->ph);
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  for (int which = 0; which < 2 && !rc; which++) {
    std::vector<float> ms((size_t)steps, 0.f);
    for (int k = 0; k < warmup + steps && !rc; k++) {
      rc |= hipEventRecord(e0, s->stream) != hipSuccess;
      rc |= which == 0 ? launch_ph_rdm(t, v_dev, p->partial, p->sums, s->stream) : launch_apply_xph(t, v_dev, w_dev, s->stream);
      rc |= hipEventRecord(e1, s->stream) != hipSuccess;
      rc |= hipEventSynchronize(e1) != hipSuccess;
      if (!rc && k >= warmup) rc |= hipEventElapsedTime(&ms[(size_t)(k - warmup)], e0, e1) != hipSuccess;
    }
    std::sort(ms.begin(), ms.end());
    ms2[which] = ms[ms.size() / 2];
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    if (std::string(edigpu_last_error()).empty()) set_error(who + ": HIP failure");
    return 1;
  }
  return 0;
}

}  // extern "C"
