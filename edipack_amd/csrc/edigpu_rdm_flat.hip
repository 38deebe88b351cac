// edigpu_rdm_flat.hip -- C ABI of the impurity reduced density matrix of superc / nonsu2 sectors (include/edigpu.h:
// edigpu_imp_rdm_flat): checks, the handle's lazily built tables and work list (host_rdm_flat.hpp), launches
// (kernels_rdm_flat.hip), placement of the packed result.
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_rdm_flat.hpp"
#include "kernels.hpp"

namespace edigpu {

struct RdmFlatDev {
  RdmFlatTables tables;
  RdmFlatArgs args;
  std::vector<RdmGroup> groups;
  int nwork = 0;
  int64_t partial_entries = 0;  // of one vector
  int64_t* rowstart = nullptr;
  int32_t* bdw = nullptr;
  uint16_t* rel = nullptr;
  uint32_t* ent = nullptr;
  RdmFlatPanel* panels = nullptr;
  RdmFlatWork* work = nullptr;
  double *partial = nullptr, *out = nullptr;  // the workgroups' partial sums, the vectors' packed triangles
  int64_t partial_cap = 0, out_cap = 0;       // in doubles
};

void free_rdm_flat(edigpu_sector* s) {
  if (!s || !s->rdm_flat) return;
  RdmFlatDev* r = s->rdm_flat;
  dev_free_all(r->rowstart, r->bdw, r->rel, r->ent, r->panels, r->work, r->partial, r->out);
  delete r;
  s->rdm_flat = nullptr;
}

static int rdm_flat_refuse(const edigpu_sector* s, const std::string& who) {
  if (occ_refuse(s, who)) return 1;
  if (s->is_normal_family()) {
    set_error(who + ": normal-mode sectors are not served here, use edigpu_imp_rdm");
    return 1;
  }
  if (!s->is_flat_family()) {
    set_error(who + ": only superc and nonsu2 sectors are supported");
    return 1;
  }
  if (s->jz) {
    set_error(who + ": Jz_basis sectors are not supported (their rows are not plain particle-number maps)");
    return 1;
  }
  if (s->model.norb > kRdmFlatMaxOrb) {
    set_error(who + ": Norb = 5 is not supported (a diagonal block of 252 x 252 does not fit the on-chip accumulators)");
    return 1;
  }
  return 0;
}

// the handle's tables, built on first use
static int rdm_flat_build(edigpu_sector* s, const std::string& who) {
  if (s->rdm_flat) return 0;
  const edigpu_model& m = s->model;
  RdmFlatDev* r = new RdmFlatDev();
  s->rdm_flat = r;  // freed by edigpu_destroy also when the build stops half-way
  auto fail = [&](const std::string& why) {
    set_error(who + ": " + why);
    free_rdm_flat(s);
    return 1;
  };
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || ncu < 1) ncu = 256;
  const int64_t dim_el = s->has_phonons() ? s->dim_el : s->dim;
  std::vector<int32_t> map((size_t)dim_el);
  int64_t n = dim_el;
  if (edigpu_sector_map(&m, s->sec_a, 0, 0, map.data(), &n)) {
    free_rdm_flat(s);
    return 1;  // the map's message stands
  }
  if (n != dim_el) return fail("the sector map does not have the handle's dimension");
  const std::string why = rdm_flat_tables(map.data(), n, model_ns(m), m.norb, m.ed_mode, s->sec_a, r->tables);
  if (!why.empty()) return fail(why);
  const int cw = s->is_complex ? 2 : 1, nblk = s->nph + 1;
  RdmFlatPlan p;
  rdm_flat_plan(r->tables, nblk, cw, ncu * 8, p);
  r->args.cw = cw;
  r->args.norb = m.norb;
  r->args.stage_max = p.stage_max;
  r->args.ept_max = p.ept_max;
  r->args.rel_max = p.rel_max;
  r->args.dim_el = dim_el;
  if (p.stage_max > kRdmFlatStageElems || rdm_flat_lds_bytes(r->args) > (size_t)(160 << 10)) return fail("the work list does not fit the LDS");
  if (dev_upload(&r->rowstart, p.rowstart) || dev_upload(&r->bdw, p.bdw) || dev_upload(&r->rel, p.rel) ||
      dev_upload(&r->ent, p.ent) || dev_upload(&r->panels, p.panels) || dev_upload(&r->work, p.work))
    return fail(edigpu_last_error());
  r->args.rowstart = r->rowstart;
  r->args.bdw = r->bdw;
  r->args.rel = r->rel;
  r->args.ent = r->ent;
  r->args.panels = r->panels;
  r->args.work = r->work;
  r->nwork = (int)p.work.size();
  r->partial_entries = p.partial_entries;
  r->groups = p.groups;
  return 0;
}

// packed triangles of nvec vectors into r->out on the handle's stream (workspace grown on demand)
static int rdm_flat_enqueue(edigpu_sector* s, const double* v_dev, int nvec) {
  RdmFlatDev* r = s->rdm_flat;
  const int cw = r->args.cw;
  const int64_t pstride = std::max<int64_t>(r->partial_entries, 1) * cw, ostride = r->tables.ntri * cw;
  if (dev_grow(&r->partial, &r->partial_cap, pstride * nvec) || dev_grow(&r->out, &r->out_cap, ostride * nvec)) return 1;
  const int64_t vstride = r->args.dim_el * (s->nph + 1) * cw;
  return launch_imp_rdm_flat(r->args, r->nwork, r->groups.data(), (int)r->groups.size(), v_dev, vstride, nvec, r->partial,
                             pstride, r->out, ostride, s->stream);
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_imp_rdm_flat(edigpu_handle s, const double* v_dev, int nvec, double* rdm_host, double* norm2_host) {
  const std::string who = "edigpu_imp_rdm_flat";
  if (!s || !v_dev || !rdm_host || nvec <= 0) {
    set_error(who + (!s || !v_dev || !rdm_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  if (rdm_flat_refuse(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (rdm_flat_build(s, who) || rdm_flat_enqueue(s, v_dev, nvec)) return 1;
  const RdmFlatDev* r = s->rdm_flat;
  const int cw = r->args.cw;
  const int64_t ostride = r->tables.ntri * cw, D = (int64_t)1 << (2 * r->tables.norb);
  std::vector<double> tri((size_t)nvec * ostride);
  EDIGPU_HIP(hipMemcpyAsync(tri.data(), r->out, tri.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  EDIGPU_HIP(hipStreamSynchronize(s->stream));
  for (int k = 0; k < nvec; k++) {
    const double* t = tri.data() + (size_t)k * ostride;
    rdm_flat_place(r->tables, t, cw, rdm_host + (size_t)k * D * D * cw);
    if (norm2_host) norm2_host[k] = rdm_flat_trace(r->tables, t, cw);
  }
  return 0;
}

int edigpu_time_rdm_flat(edigpu_handle s, const double* v_dev, int warmup, int steps, double* ms_out) {
  const std::string who = "edigpu_time_rdm_flat";
  if (!s || !v_dev || !ms_out || warmup < 0 || steps <= 0) {
    set_error(who + ": bad argument");
    return 1;
  }
  if (rdm_flat_refuse(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (rdm_flat_build(s, who)) return 1;
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  std::vector<float> ms((size_t)steps, 0.f);
  for (int k = 0; k < warmup + steps && !rc; k++) {
    rc |= hipEventRecord(e0, s->stream) != hipSuccess;
    rc |= rdm_flat_enqueue(s, v_dev, 1);
    rc |= hipEventRecord(e1, s->stream) != hipSuccess;
    rc |= hipEventSynchronize(e1) != hipSuccess;
    if (!rc && k >= warmup) rc |= hipEventElapsedTime(&ms[(size_t)(k - warmup)], e0, e1) != hipSuccess;
  }
  std::sort(ms.begin(), ms.end());
  *ms_out = ms[ms.size() / 2];
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    if (std::string(edigpu_last_error()).empty()) set_error(who + ": HIP failure");
    return 1;
  }
  return 0;
}

}  // extern "C"
