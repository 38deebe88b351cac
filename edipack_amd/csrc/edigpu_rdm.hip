// edigpu_rdm.hip -- C ABI of the impurity reduced density matrix (include/edigpu.h: edigpu_imp_rdm): checks, the handle's
// lazily built tables and work list (host_rdm.hpp), launches (kernels_rdm.hip), placement of the packed result.
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_rdm.hpp"
#include "kernels.hpp"

namespace edigpu {

struct RdmDev {
  RdmRanks ranks;
  RdmLayout layout;
  RdmArgs args;
  std::vector<RdmGroup> groups;
  int nwork = 0;
  int64_t partial_entries = 0;  // of one vector
  int32_t* rows = nullptr;
  uint16_t* rel = nullptr;
  uint32_t* ent = nullptr;
  RdmWork* work = nullptr;
  double *partial = nullptr, *out = nullptr;  // the workgroups' partial sums, the vectors' packed triangles
  int64_t partial_cap = 0, out_cap = 0;       // in doubles
};

void free_rdm(edigpu_sector* s) {
  if (!s || !s->rdm) return;
  RdmDev* r = s->rdm;
  dev_free_all(r->rows, r->rel, r->ent, r->work, r->partial, r->out);
  delete r;
  s->rdm = nullptr;
}

static bool rdm_served(const edigpu_sector* s) {
  return s && s->built_by_library && (s->is_normal_family()) && s->is_whole();
}

int64_t rdm_table_bytes(const edigpu_sector* s) {
  if (!rdm_served(s) || s->model.norb < 1 || s->model.norb > kRdmMaxOrb) return 0;
  RdmRanks rk;
  RdmLayout l;
  rdm_rank_tables(s->model.norb, rk);
  rdm_layout(rk, l);
  const int64_t cw = s->is_complex ? 2 : 1, nel = s->dim_up * s->dim_dw * (s->nph + 1);
  // run starts, entries, a work list of the order of 4096 workgroups; a workgroup covers at least 8 elements per partial sum
  const int64_t tables = 4 * s->dim_dw + 2 * s->dim_up + 4 * l.ntri + 4096 * (int64_t)sizeof(RdmWork);
  return tables + (nel / 8 + 2 * l.ntri) * cw * 8;
}

static int rdm_refuse(const edigpu_sector* s, const std::string& who) {
  if (occ_refuse(s, who)) return 1;
  if (!s->is_normal_family()) {
    set_error(who + ": only ed_mode=normal sectors are supported");
    return 1;
  }
  return 0;
}

// the handle's tables, built on first use
static int rdm_build(edigpu_sector* s, const std::string& who) {
  if (s->rdm) return 0;
  const edigpu_model& m = s->model;
  if (m.norb < 1 || m.norb > kRdmMaxOrb) {
    set_error(who + ": norb out of range");
    return 1;
  }
  RdmDev* r = new RdmDev();
  s->rdm = r;  // freed by edigpu_destroy also when the build stops half-way
  auto fail = [&](const std::string& why) {
    set_error(who + ": " + why);
    free_rdm(s);
    return 1;
  };
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || ncu < 1) ncu = 256;
  std::vector<int32_t> mu((size_t)s->dim_up), md((size_t)s->dim_dw);
  int64_t nu = s->dim_up, nd = s->dim_dw;
  if (edigpu_sector_map(&m, s->sec_a, s->sec_b, 0, mu.data(), &nu) || edigpu_sector_map(&m, s->sec_a, s->sec_b, 1, md.data(), &nd)) {
    free_rdm(s);
    return 1;  // the map's message stands
  }
  if (nu != s->dim_up || nd != s->dim_dw) return fail("the sector maps do not have the handle's dimensions");
  rdm_rank_tables(m.norb, r->ranks);
  rdm_layout(r->ranks, r->layout);
  RdmRuns up, dw;
  std::string why = rdm_runs(mu.data(), nu, m.norb, r->ranks, up);
  if (why.empty()) why = rdm_runs(md.data(), nd, m.norb, r->ranks, dw);
  if (!why.empty()) return fail(why);
  const int cw = s->is_complex ? 2 : 1, nblk = s->nph + 1;
  RdmPlan p;
  rdm_plan(r->ranks, r->layout, up, dw, s->dim_up, s->dim_dw, nblk, cw, ncu * 8, p);
  r->args.cw = cw;
  r->args.stride = p.stride;
  r->args.ld_max = p.ld_max;
  r->args.ept_max = p.ept_max;
  r->args.rel_max = p.rel_max;
  r->args.dim_up = s->dim_up;
  r->args.dim_dw = s->dim_dw;
  if (rdm_lds_bytes(r->args) > (size_t)(160 << 10)) return fail("the work list does not fit the LDS");
  if (dev_upload(&r->rows, p.rows) || dev_upload(&r->rel, p.rel) || dev_upload(&r->ent, p.ent) || dev_upload(&r->work, p.work))
    return fail(edigpu_last_error());
  r->args.rows = r->rows;
  r->args.rel = r->rel;
  r->args.ent = r->ent;
  r->args.work = r->work;
  r->nwork = (int)p.work.size();
  r->partial_entries = p.partial_entries;
  r->groups = p.groups;
  return 0;
}

// packed triangles of nvec vectors into r->out on the handle's stream (workspace grown on demand)
static int rdm_enqueue(edigpu_sector* s, const double* v_dev, int nvec) {
  RdmDev* r = s->rdm;
  const int cw = r->args.cw;
  const int64_t pstride = std::max<int64_t>(r->partial_entries, 1) * cw, ostride = r->layout.ntri * cw;
  if (dev_grow(&r->partial, &r->partial_cap, pstride * nvec) || dev_grow(&r->out, &r->out_cap, ostride * nvec)) return 1;
  const int64_t vstride = s->dim_up * s->dim_dw * (s->nph + 1) * cw;
  return launch_imp_rdm(r->args, r->nwork, r->groups.data(), (int)r->groups.size(), v_dev, vstride, nvec, r->partial, pstride,
                        r->out, ostride, s->stream);
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_imp_rdm(edigpu_handle s, const double* v_dev, int nvec, double* rdm_host, double* norm2_host) {
  const std::string who = "edigpu_imp_rdm";
  if (!s || !v_dev || !rdm_host || nvec <= 0) {
    set_error(who + (!s || !v_dev || !rdm_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  if (rdm_refuse(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (rdm_build(s, who) || rdm_enqueue(s, v_dev, nvec)) return 1;
  const RdmDev* r = s->rdm;
  const int cw = r->args.cw, norb = r->ranks.norb;
  const int64_t ostride = r->layout.ntri * cw, D = (int64_t)1 << (2 * norb);
  std::vector<double> tri((size_t)nvec * ostride);
  EDIGPU_HIP(hipMemcpyAsync(tri.data(), r->out, tri.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  EDIGPU_HIP(hipStreamSynchronize(s->stream));
  for (int k = 0; k < nvec; k++) {
    const double* t = tri.data() + (size_t)k * ostride;
    rdm_place(r->ranks, r->layout, t, cw, rdm_host + (size_t)k * D * D * cw);
    if (norm2_host) {  // the trace, class by class
      double tr = 0.0;
      for (int kd = 0; kd <= norb; kd++)
        for (int ku = 0; ku <= norb; ku++) {
          const int n = r->ranks.nk[ku] * r->ranks.nk[kd];
          for (int p = 0; p < n; p++) tr += t[(r->layout.tri_off[ku][kd] + rdm_tri_index(n, p, p)) * cw];
        }
      norm2_host[k] = tr;
    }
  }
  return 0;
}

int edigpu_time_rdm(edigpu_handle s, const double* v_dev, int warmup, int steps, double* ms_out) {
  const std::string who = "edigpu_time_rdm";
  if (!s || !v_dev || !ms_out || warmup < 0 || steps <= 0) {
    set_error(who + ": bad argument");
    return 1;
  }
  if (rdm_refuse(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (rdm_build(s, who)) return 1;
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  std::vector<float> ms((size_t)steps, 0.f);
  for (int k = 0; k < warmup + steps && !rc; k++) {
    rc |= hipEventRecord(e0, s->stream) != hipSuccess;
    rc |= rdm_enqueue(s, v_dev, 1);
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
