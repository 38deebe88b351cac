// edigpu_rdm_flat.hip -- C ABI of the impurity reduced density matrix of superc / nonsu2 sectors (include/edigpu.h:
// edigpu_imp_rdm_flat): checks, the handle's lazily built tables and work list (host_rdm_flat.hpp), launches
// (kernels_rdm_flat.hip), placement of the packed result; and the view of a rank's elements behind
// edigpu_imp_rdm_flat_sharded (edigpu_shard_obs.hip), as edigpu_rdm.hip has one.
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

// the device copy of an RdmFlatPlan's tables and work list
struct RdmFlatList {
  RdmFlatArgs args;
  int nwork = 0;
  int64_t* rowstart = nullptr;
  int32_t* bdw = nullptr;
  uint16_t* rel = nullptr;
  uint32_t* ent = nullptr;
  RdmFlatPanel* panels = nullptr;
  RdmFlatWork* work = nullptr;
  void release() { dev_free_all(rowstart, bdw, rel, ent, panels, work); }
};

// The same for the elements [first, first + count) of the sector, one of `world` ranges (edigpu_sector::rdm_flat_shard;
// host_rdm_flat.hpp RdmFlatShardPlan): the work lists of the interior slabs and of the tail slab, the two segment tables
struct RdmFlatShardDev {
  int64_t first = 0, count = 0;
  int world = 0;
  RdmFlatTables tables;
  RdmFlatShardInfo info;
  RdmFlatSeg *pack = nullptr, *fill = nullptr;
  int npack = 0, nfill = 0;
  int64_t pack_max = 0, fill_max = 0;  // the longest segment of each table
  RdmFlatList in, slab;
  std::vector<RdmGroup> groups;
  int64_t partial_entries = 0;
  double *partial = nullptr, *out = nullptr;
  int64_t partial_cap = 0, out_cap = 0;
};

static void free_rdm_flat_shard(edigpu_sector* s) {
  if (!s->rdm_flat_shard) return;
  RdmFlatShardDev* r = s->rdm_flat_shard;
  r->in.release();
  r->slab.release();
  dev_free_all(r->pack, r->fill, r->partial, r->out);
  delete r;
  s->rdm_flat_shard = nullptr;
}

void free_rdm_flat(edigpu_sector* s) {
  if (!s) return;
  free_rdm_flat_shard(s);
  if (!s->rdm_flat) return;
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

// ---- the shard view (edigpu_imp_rdm_flat_sharded in edigpu_shard_obs.hip) ----

int rdm_flat_shard_refuse(const edigpu_sector* s, const std::string& who) {
  if (occ_refuse_kind(s, who)) return 1;
  if (s->is_normal_family()) {
    set_error(who + ": normal-mode sectors are not served here, use edigpu_imp_rdm_sharded");
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

// the host tables of the whole sector (checked against its map) and the plan of the range; 1 with the message set
static int flat_shard_host_plan(const edigpu_sector* s, int64_t first, int64_t count, int world, int target_wgs,
                                const std::string& who, RdmFlatTables& t, RdmFlatShardPlan& p) {
  const edigpu_model& m = s->model;
  const int64_t dim_el = s->dim / (s->nph + 1);  // of the whole sector, as shard_rows counts the units
  std::string why;
  {
    std::vector<int32_t> map((size_t)dim_el);
    int64_t n = dim_el;
    if (edigpu_sector_map(&m, s->sec_a, 0, 0, map.data(), &n)) return 1;  // the map's message stands
    why = n != dim_el ? "the sector map does not have the handle's dimension"
                      : rdm_flat_tables(map.data(), n, model_ns(m), m.norb, m.ed_mode, s->sec_a, t);
  }
  if (why.empty()) why = rdm_flat_shard_plan(t, s->nph + 1, s->is_complex ? 2 : 1, target_wgs, world, first, count, p);
  if (why.empty() && (p.first != std::min(first, dim_el) || p.count != count)) why = "the elements are not inside the sector";
  if (!why.empty()) {
    set_error(who + ": " + why);
    return 1;
  }
  return 0;
}

static void flat_shard_fill_info(const RdmFlatTables& t, const RdmFlatShardPlan& p, int cw, RdmFlatShardInfo* info) {
  info->H = p.H;
  info->nslab_in = p.nslab_in;
  info->tail_start = p.tail_start;
  info->tail_len = p.tail_len;
  info->tail_own = p.tail_own;
  info->ntri = t.ntri;
  info->cw = cw;
}

int rdm_flat_shard_info(const edigpu_sector* s, int64_t first, int64_t count, int world, const std::string& who,
                        RdmFlatShardInfo* info) {
  RdmFlatTables t;
  RdmFlatShardPlan p;
  if (flat_shard_host_plan(s, first, count, world, 2048, who, t, p)) return 1;
  flat_shard_fill_info(t, p, s->is_complex ? 2 : 1, info);
  return 0;
}

// t <- the device copy of p; 1 with why set
static int upload_flat_list(const RdmFlatPlan& p, int cw, RdmFlatList& t, std::string& why) {
  t.args.cw = cw;
  t.args.norb = p.norb;
  t.args.stage_max = p.stage_max;
  t.args.ept_max = p.ept_max;
  t.args.rel_max = p.rel_max;
  t.args.dim_el = p.dim_el;
  if (p.stage_max > kRdmFlatStageElems || rdm_flat_lds_bytes(t.args) > (size_t)(160 << 10)) {
    why = "the work list does not fit the LDS";
    return 1;
  }
  if (dev_upload(&t.rowstart, p.rowstart) || dev_upload(&t.bdw, p.bdw) || dev_upload(&t.rel, p.rel) || dev_upload(&t.ent, p.ent) ||
      dev_upload(&t.panels, p.panels) || dev_upload(&t.work, p.work)) {
    why = edigpu_last_error();
    return 1;
  }
  t.args.rowstart = t.rowstart;
  t.args.bdw = t.bdw;
  t.args.rel = t.rel;
  t.args.ent = t.ent;
  t.args.panels = t.panels;
  t.args.work = t.work;
  t.nwork = (int)p.work.size();
  return 0;
}

// the tables of the elements [first, first + count), one of `world` ranges, (re)built when they are not the ones held
int rdm_flat_shard_prepare(edigpu_sector* s, int64_t first, int64_t count, int world, const std::string& who,
                           RdmFlatShardInfo* info) {
  RdmFlatShardDev* r = s->rdm_flat_shard;
  if (!r || r->first != first || r->count != count || r->world != world) {
    free_rdm_flat_shard(s);
    r = new RdmFlatShardDev();
    s->rdm_flat_shard = r;
    auto fail = [&](const std::string& why) {
      if (!why.empty()) set_error(who + ": " + why);
      free_rdm_flat_shard(s);
      return 1;
    };
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || ncu < 1) ncu = 256;
    const int cw = s->is_complex ? 2 : 1;
    RdmFlatShardPlan p;
    if (flat_shard_host_plan(s, first, count, world, ncu * 8, who, r->tables, p)) return fail("");
    std::string why;
    if (upload_flat_list(p.in, cw, r->in, why)) return fail(why);
    if (p.tail_len > 0 && upload_flat_list(p.slab, cw, r->slab, why)) return fail(why);
    if (dev_upload(&r->pack, p.pack) || dev_upload(&r->fill, p.fill)) return fail(edigpu_last_error());
    r->npack = (int)p.pack.size();
    r->nfill = (int)p.fill.size();
    for (const RdmFlatSeg& g : p.pack) r->pack_max = std::max(r->pack_max, g.len);
    for (const RdmFlatSeg& g : p.fill) r->fill_max = std::max(r->fill_max, g.len);
    flat_shard_fill_info(r->tables, p, cw, &r->info);
    r->groups = p.groups;
    r->partial_entries = p.partial_entries;
    r->first = first;
    r->count = count;
    r->world = world;
  }
  *info = r->info;
  return 0;
}

int rdm_flat_shard_pack(edigpu_sector* s, const double* v_dev, int nvec, double* send_dev) {
  const RdmFlatShardDev* r = s->rdm_flat_shard;
  const int cw = r->info.cw, nblk = s->nph + 1;
  return launch_rdm_flat_segs(r->pack, r->npack, r->pack_max, nblk, cw, nvec, v_dev, r->count * nblk * cw, r->count, nullptr,
                              r->info.H, send_dev, r->info.H, s->stream);
}

int rdm_flat_shard_enqueue(edigpu_sector* s, const double* v_dev, int nvec, const double* halos_dev, double* slab_dev,
                           const double** tri_dev) {
  RdmFlatShardDev* r = s->rdm_flat_shard;
  const int cw = r->info.cw, nblk = s->nph + 1;
  const int64_t vstride = r->count * nblk * cw, sstride = r->info.tail_len * nblk * cw;
  const int64_t pstride = std::max<int64_t>(r->partial_entries, 1) * cw, ostride = r->tables.ntri * cw;
  if (dev_grow(&r->partial, &r->partial_cap, pstride * nvec) || dev_grow(&r->out, &r->out_cap, ostride * nvec)) return 1;
  if (launch_rdm_flat_segs(r->fill, r->nfill, r->fill_max, nblk, cw, nvec, v_dev, vstride, r->count, halos_dev, r->info.H, slab_dev,
                           r->info.tail_len, s->stream))
    return 1;
  if (launch_imp_rdm_flat_shard(r->in.args, r->in.nwork, v_dev, vstride, r->slab.args, r->slab.nwork, slab_dev, sstride,
                                r->groups.data(), (int)r->groups.size(), nvec, r->partial, pstride, r->out, ostride, s->stream))
    return 1;
  *tri_dev = r->out;
  return 0;
}

void rdm_flat_shard_expand(const edigpu_sector* s, const double* tri, int nvec, double* rdm_host, double* norm2_host) {
  const RdmFlatShardDev* r = s->rdm_flat_shard;
  const int cw = r->info.cw;
  const int64_t ostride = r->tables.ntri * cw, D = (int64_t)1 << (2 * r->tables.norb);
  for (int k = 0; k < nvec; k++) {
    const double* t = tri + (size_t)k * ostride;
    rdm_flat_place(r->tables, t, cw, rdm_host + (size_t)k * D * D * cw);
    if (norm2_host) norm2_host[k] = rdm_flat_trace(r->tables, t, cw);
  }
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
