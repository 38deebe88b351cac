// edigpu_rdm.hip -- C ABI of the impurity reduced density matrix (include/edigpu.h: edigpu_imp_rdm): checks, the handle's
// lazily built tables and work list (host_rdm.hpp), launches (kernels_rdm.hip), placement of the packed result; and the
// view of a rank's down rows behind edigpu_imp_rdm_sharded (edigpu_shard_obs.hip), as edigpu_occ.hip has one.
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_rdm.hpp"
#include "kernels.hpp"

namespace edigpu {

// the device copy of an RdmPlan's tables and work list
struct RdmList {
  RdmArgs args;
  int nwork = 0;
  int32_t* rows = nullptr;
  uint16_t* rel = nullptr;
  uint32_t* ent = nullptr;
  RdmWork* work = nullptr;
  void release() { dev_free_all(rows, rel, ent, work); }
};

struct RdmDev {
  RdmRanks ranks;
  RdmLayout layout;
  RdmList list;
  std::vector<RdmGroup> groups;
  int64_t partial_entries = 0;  // of one vector
  double *partial = nullptr, *out = nullptr;  // the workgroups' partial sums, the vectors' packed triangles
  int64_t partial_cap = 0, out_cap = 0;       // in doubles
};

// The same for the rows [first, first + count) of the sector, one of `world` ranges (edigpu_sector::rdm_shard;
// host_rdm.hpp RdmShardPlan): the work lists of the interior runs and of the boundary slab, the two row copies
struct RdmShardDev {
  int64_t first = 0, count = 0;
  int world = 0;
  RdmRanks ranks;
  RdmLayout layout;
  int H = 0, tail_ld = 0;
  RdmRowCopy pack, fill;
  RdmList in, slab;
  std::vector<RdmGroup> groups;
  int64_t partial_entries = 0;
  double *partial = nullptr, *out = nullptr;
  int64_t partial_cap = 0, out_cap = 0;
};

static void free_rdm_shard(edigpu_sector* s) {
  if (!s->rdm_shard) return;
  RdmShardDev* r = s->rdm_shard;
  r->in.release();
  r->slab.release();
  dev_free_all(r->partial, r->out);
  delete r;
  s->rdm_shard = nullptr;
}

static void free_rdm_whole(edigpu_sector* s) {
  if (!s->rdm) return;
  RdmDev* r = s->rdm;
  r->list.release();
  dev_free_all(r->partial, r->out);
  delete r;
  s->rdm = nullptr;
}

void free_rdm(edigpu_sector* s) {
  if (!s) return;
  free_rdm_whole(s);
  free_rdm_shard(s);
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
  // + the shard view of edigpu_imp_rdm_sharded: at most the same tables and sums again for the interior runs, the slab's
  // tables (one run per phonon block) and its partial sums
  const int64_t slab = 2 * s->dim_up + 4 * l.ntri + (s->nph + 1) * (int64_t)sizeof(RdmWork) * 64 + kRdmMaxRun * s->dim_up * (s->nph + 1) / 8 * cw * 8;
  return 2 * (tables + (nel / 8 + 2 * l.ntri) * cw * 8) + slab;
}

static int rdm_refuse(const edigpu_sector* s, const std::string& who) {
  if (occ_refuse(s, who)) return 1;
  if (!s->is_normal_family()) {
    set_error(who + ": only ed_mode=normal sectors are supported");
    return 1;
  }
  return 0;
}

// t <- the device copy of p for vectors of dim_up columns whose blocks are dim_dw rows apart; 1 with why set
static int upload_list(const RdmPlan& p, int cw, int64_t dim_up, int64_t dim_dw, RdmList& t, std::string& why) {
  t.args.cw = cw;
  t.args.stride = p.stride;
  t.args.ld_max = p.ld_max;
  t.args.ept_max = p.ept_max;
  t.args.rel_max = p.rel_max;
  t.args.dim_up = dim_up;
  t.args.dim_dw = dim_dw;
  if (rdm_lds_bytes(t.args) > (size_t)(160 << 10)) {
    why = "the work list does not fit the LDS";
    return 1;
  }
  if (dev_upload(&t.rows, p.rows) || dev_upload(&t.rel, p.rel) || dev_upload(&t.ent, p.ent) || dev_upload(&t.work, p.work)) {
    why = edigpu_last_error();
    return 1;
  }
  t.args.rows = t.rows;
  t.args.rel = t.rel;
  t.args.ent = t.ent;
  t.args.work = t.work;
  t.nwork = (int)p.work.size();
  return 0;
}

// the sector's maps as runs; 1 with why set ("": the map's message stands)
static int sector_runs(const edigpu_sector* s, const RdmRanks& rk, RdmRuns& up, RdmRuns& dw, std::string& why) {
  const edigpu_model& m = s->model;
  std::vector<int32_t> mu((size_t)s->dim_up), md((size_t)s->dim_dw);
  int64_t nu = s->dim_up, nd = s->dim_dw;
  why.clear();
  if (edigpu_sector_map(&m, s->sec_a, s->sec_b, 0, mu.data(), &nu) || edigpu_sector_map(&m, s->sec_a, s->sec_b, 1, md.data(), &nd))
    return 1;
  if (nu != s->dim_up || nd != s->dim_dw) {
    why = "the sector maps do not have the handle's dimensions";
    return 1;
  }
  why = rdm_runs(mu.data(), nu, m.norb, rk, up);
  if (why.empty()) why = rdm_runs(md.data(), nd, m.norb, rk, dw);
  return why.empty() ? 0 : 1;
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
    if (!why.empty()) set_error(who + ": " + why);  // (else the map's message stands)
    free_rdm_whole(s);
    return 1;
  };
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || ncu < 1) ncu = 256;
  rdm_rank_tables(m.norb, r->ranks);
  rdm_layout(r->ranks, r->layout);
  RdmRuns up, dw;
  std::string why;
  if (sector_runs(s, r->ranks, up, dw, why)) return fail(why);
  const int cw = s->is_complex ? 2 : 1, nblk = s->nph + 1;
  RdmPlan p;
  rdm_plan(r->ranks, r->layout, up, dw, s->dim_up, s->dim_dw, nblk, cw, ncu * 8, p);
  if (upload_list(p, cw, s->dim_up, s->dim_dw, r->list, why)) return fail(why);
  r->partial_entries = p.partial_entries;
  r->groups = p.groups;
  return 0;
}

// packed triangles of nvec vectors into r->out on the handle's stream (workspace grown on demand)
static int rdm_enqueue(edigpu_sector* s, const double* v_dev, int nvec) {
  RdmDev* r = s->rdm;
  const int cw = r->list.args.cw;
  const int64_t pstride = std::max<int64_t>(r->partial_entries, 1) * cw, ostride = r->layout.ntri * cw;
  if (dev_grow(&r->partial, &r->partial_cap, pstride * nvec) || dev_grow(&r->out, &r->out_cap, ostride * nvec)) return 1;
  const int64_t vstride = s->dim_up * s->dim_dw * (s->nph + 1) * cw;
  return launch_imp_rdm(r->list.args, r->list.nwork, r->groups.data(), (int)r->groups.size(), v_dev, vstride, nvec, r->partial,
                        pstride, r->out, ostride, s->stream);
}

// the packed triangles of nvec vectors -> their dense matrices and, norm2_host given, traces (class by class)
static void rdm_expand(const RdmRanks& rk, const RdmLayout& l, int cw, const double* tri, int nvec, double* rdm_host,
                       double* norm2_host) {
  const int norb = rk.norb;
  const int64_t ostride = l.ntri * cw, D = (int64_t)1 << (2 * norb);
  for (int k = 0; k < nvec; k++) {
    const double* t = tri + (size_t)k * ostride;
    rdm_place(rk, l, t, cw, rdm_host + (size_t)k * D * D * cw);
    if (norm2_host) {
      double tr = 0.0;
      for (int kd = 0; kd <= norb; kd++)
        for (int ku = 0; ku <= norb; ku++) {
          const int n = rk.nk[ku] * rk.nk[kd];
          for (int p = 0; p < n; p++) tr += t[(l.tri_off[ku][kd] + rdm_tri_index(n, p, p)) * cw];
        }
      norm2_host[k] = tr;
    }
  }
}

// ---- the shard view (edigpu_imp_rdm_sharded in edigpu_shard_obs.hip) ----

int rdm_shard_refuse(const edigpu_sector* s, const std::string& who) {
  if (occ_refuse_kind(s, who)) return 1;
  if (!s->is_normal_family()) {
    set_error(who + ": only ed_mode=normal sectors are supported");
    return 1;
  }
  if (s->model.norb < 1 || s->model.norb > kRdmMaxOrb) {
    set_error(who + ": norb out of range");
    return 1;
  }
  return 0;
}

// the tables of the rows [first, first + count), one of `world` ranges, (re)built when they are not the ones held
int rdm_shard_prepare(edigpu_sector* s, int64_t first, int64_t count, int world, const std::string& who, RdmShardInfo* info) {
  RdmShardDev* r = s->rdm_shard;
  if (!r || r->first != first || r->count != count || r->world != world) {
    free_rdm_shard(s);
    r = new RdmShardDev();
    s->rdm_shard = r;
    auto fail = [&](const std::string& why) {
      if (!why.empty()) set_error(who + ": " + why);
      free_rdm_shard(s);
      return 1;
    };
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || ncu < 1) ncu = 256;
    rdm_rank_tables(s->model.norb, r->ranks);
    rdm_layout(r->ranks, r->layout);
    RdmRuns up, dw;
    std::string why;
    if (sector_runs(s, r->ranks, up, dw, why)) return fail(why);
    const int cw = s->is_complex ? 2 : 1, nblk = s->nph + 1;
    RdmShardPlan p;
    why = rdm_shard_plan(r->ranks, r->layout, up, dw, s->dim_up, s->dim_dw, nblk, cw, ncu * 8, world, first, count, p);
    if (!why.empty() || p.first != std::min(first, s->dim_dw) || p.count != count) return fail(why.empty() ? "the rows are not inside the sector" : why);
    if (upload_list(p.in, cw, s->dim_up, p.count, r->in, why)) return fail(why);
    if (p.tail_ld > 0 && upload_list(p.slab, cw, s->dim_up, p.tail_ld, r->slab, why)) return fail(why);
    r->H = p.H;
    r->tail_ld = p.tail_ld;
    r->pack = p.pack;
    r->fill = p.fill;
    r->groups = p.groups;
    r->partial_entries = p.partial_entries;
    r->first = first;
    r->count = count;
    r->world = world;
  }
  info->H = r->H;
  info->tail_ld = r->tail_ld;
  info->cw = r->in.args.cw;
  info->ntri = r->layout.ntri;
  return 0;
}

int rdm_shard_pack(edigpu_sector* s, const double* v_dev, int nvec, double* send_dev) {
  const RdmShardDev* r = s->rdm_shard;
  const int cw = r->in.args.cw, nblk = s->nph + 1;
  const int64_t rowlen = s->dim_up * cw;
  return launch_rdm_rows(r->pack, nblk, (int)rowlen, nvec, v_dev, r->count * rowlen * nblk, r->count, nullptr, r->H, send_dev,
                         s->stream);
}

int rdm_shard_enqueue(edigpu_sector* s, const double* v_dev, int nvec, const double* halos_dev, double* slab_dev,
                      const double** tri_dev) {
  RdmShardDev* r = s->rdm_shard;
  const int cw = r->in.args.cw, nblk = s->nph + 1;
  const int64_t rowlen = s->dim_up * cw, vstride = r->count * rowlen * nblk, sstride = r->tail_ld * rowlen * nblk;
  const int64_t pstride = std::max<int64_t>(r->partial_entries, 1) * cw, ostride = r->layout.ntri * cw;
  if (dev_grow(&r->partial, &r->partial_cap, pstride * nvec) || dev_grow(&r->out, &r->out_cap, ostride * nvec)) return 1;
  if (launch_rdm_rows(r->fill, nblk, (int)rowlen, nvec, v_dev, vstride, r->count, halos_dev, r->H, slab_dev, s->stream)) return 1;
  if (launch_imp_rdm_shard(r->in.args, r->in.nwork, v_dev, vstride, r->slab.args, r->slab.nwork, slab_dev, sstride,
                           r->groups.data(), (int)r->groups.size(), nvec, r->partial, pstride, r->out, ostride, s->stream))
    return 1;
  *tri_dev = r->out;
  return 0;
}

void rdm_shard_expand(const edigpu_sector* s, const double* tri, int nvec, double* rdm_host, double* norm2_host) {
  const RdmShardDev* r = s->rdm_shard;
  rdm_expand(r->ranks, r->layout, r->in.args.cw, tri, nvec, rdm_host, norm2_host);
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
  std::vector<double> tri((size_t)nvec * r->layout.ntri * r->list.args.cw);
  EDIGPU_HIP(hipMemcpyAsync(tri.data(), r->out, tri.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  EDIGPU_HIP(hipStreamSynchronize(s->stream));
  rdm_expand(r->ranks, r->layout, r->list.args.cw, tri.data(), nvec, rdm_host, norm2_host);
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
