// edigpu_twin.hip -- C ABI of the ED_TWIN=T reorder (include/edigpu.h: edigpu_twin_sector, edigpu_apply_twin,
// edigpu_time_twin, edigpu_apply_twin_sharded): checks, the source handle's lazily built order table (host_twin.hpp),
// launches (kernels_twin.hip).  Takes the place of the loop vector(i) = twin%dvec(Order(i)) of es_return_dvector
// (ED_EIGENSPACE.f90:652-720) and, on shards, of the gather of es_return_dvector_mpi (:723-793).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_twin.hpp"
#include "kernels.hpp"
#include "shard_comm.hpp"

namespace edigpu {

void free_twin(edigpu_sector* s) {
  if (!s || !s->twin) return;
  dev_free(s->twin->order);
  delete s->twin;
  s->twin = nullptr;
}

int64_t twin_table_bytes(const edigpu_sector* s) {
  if (!s || !s->built_by_library || !s->is_flat_family() || s->jz || s->model.ed_mode != kTwinSuperc) return 0;
  return 4 * (s->dim / (s->nph + 1));
}

namespace {

// how the two handles of a call are related; the geometry of the reorder in elements (doubles, or double2 when cplx)
struct TwinPlan {
  bool transpose = false;  // normal mode (ed_total_ud = T and F): R x C -> C x R per phonon block
  bool reverse = false;    // nonsu2
  int cplx = 0, nblk = 1;
  int64_t R = 0, C = 0;    // transpose: DimDw and DimUp of the SOURCE
  int64_t n = 0;           // gather: the electronic rows of the whole sector
};

bool is_orbs_built(const edigpu_sector* s) { return s->kind == kOrbs && !s->orbs_nups.empty(); }
bool from_model(const edigpu_sector* s) { return s->built_by_library || is_orbs_built(s); }

void orbs_dims(const edigpu_sector* s, int64_t& du, int64_t& dd) {
  du = dd = 1;
  const int half = s->orbs.naxes / 2;
  for (int k = 0; k < s->orbs.naxes; k++) (k < half ? du : dd) *= s->orbs.dims[k];
}

// every check of a pair of handles that needs no vector and no communicator; shards: the call is the sharded one
int twin_plan(const edigpu_sector* src, const edigpu_sector* dst, bool shards, const std::string& who, TwinPlan& p) {
  auto refuse = [&](const std::string& why) {
    set_error(who + ": " + why);
    return 1;
  };
  for (const edigpu_sector* s : {src, dst}) {
    if (s->jz) return refuse("JZ_BASIS sectors are not supported (the reference has no twin of a (Ntot, Jz) sector)");
    if (s->is_flat_family() && !s->built_by_library)
      return refuse("a hand-over flat handle (edigpu_csr_create_*) has no sector map; build the sector from a model");
    if (!shards && !s->is_whole()) return refuse("the handles must hold the whole sector (shards: edigpu_apply_twin_sharded)");
    if (shards && s->kind == kOrbs) return refuse("ed_total_ud=F sectors are not served on shards");
    if (shards && !from_model(s))
      return refuse("hand-over handles are not served on shards; build the sector from a model");
  }
  if (src->kind != dst->kind) {
    // (a stored and an on-the-fly handle are one kind of sector: the same map)
    if (!(src->is_flat_family() && dst->is_flat_family())) return refuse("the handles are of different kind");
  }
  if (src->is_complex != dst->is_complex) return refuse("the handles are of different kind (real and complex)");
  if (src->device != dst->device) return refuse("the handles live on different devices");
  if (src->nph != dst->nph) return refuse("the handles have different nph");
  if (from_model(src) != from_model(dst) ||
      (from_model(src) && std::memcmp(&src->model, &dst->model, sizeof(edigpu_model)) != 0))
    return refuse("sectors of different models");
  p.cplx = src->is_complex ? 1 : 0;
  p.nblk = src->nph + 1;
  const std::string not_twin = "dst is not the twin sector of src";
  if (src->is_normal_family()) {
    p.transpose = true;
    p.R = src->dim_dw;
    p.C = src->dim_up;
    if (from_model(src) && (dst->sec_a != src->sec_b || dst->sec_b != src->sec_a))
      return refuse(not_twin + " (Nup, Ndw) = (" + std::to_string(src->sec_b) + ", " + std::to_string(src->sec_a) + ")");
    if (dst->dim_up != p.R || dst->dim_dw != p.C) return refuse(not_twin + " (DimUp, DimDw must be src's DimDw, DimUp)");
    return 0;
  }
  if (src->kind == kOrbs) {
    p.transpose = true;
    orbs_dims(src, p.C, p.R);
    int64_t du = 0, dd = 0;
    orbs_dims(dst, du, dd);
    const int half = src->orbs.naxes / 2;
    bool ok = src->orbs.naxes == dst->orbs.naxes && du == p.R && dd == p.C;
    for (int k = 0; ok && k < src->orbs.naxes; k++) ok = dst->orbs.dims[k] == src->orbs.dims[(k + half) % src->orbs.naxes];
    if (ok && from_model(src)) ok = dst->orbs_nups == src->orbs_ndws && dst->orbs_ndws == src->orbs_nups;
    if (!ok) return refuse(not_twin + " (nups, ndws must be src's ndws, nups)");
    return 0;
  }
  // superc / nonsu2
  const int mode = src->model.ed_mode;
  int t1 = 0, t2 = 0;
  bool self = false;
  const std::string why = twin_sector(mode, model_ns(src->model), src->sec_a, 0, t1, t2, self);
  if (!why.empty()) return refuse(why);
  if (dst->sec_a != t1) return refuse(not_twin + " " + std::to_string(t1));
  p.reverse = mode == kTwinNonsu2;
  p.n = src->dim / p.nblk;
  if (dst->dim != src->dim) return refuse("internal error (twin sectors of different dimension)");
  return 0;
}

// the superc order table of the source handle, built on first use
int twin_order_build(edigpu_sector* s, int64_t n, const std::string& who) {
  if (s->twin && s->twin->n == n) return 0;
  free_twin(s);
  std::vector<int32_t> map((size_t)n), order;
  int64_t got = n;
  if (edigpu_sector_map(&s->model, s->sec_a, 0, 0, map.data(), &got)) return 1;  // the map's message stands
  if (got != n) {
    set_error(who + ": the sector map does not have the handle's dimension");
    return 1;
  }
  const std::string why = twin_order(kTwinSuperc, map.data(), n, model_ns(s->model), order);
  if (!why.empty()) {
    set_error(who + ": " + why);
    return 1;
  }
  s->twin = new TwinDev();  // freed by edigpu_destroy also when the upload fails
  s->twin->n = n;
  return dev_upload(&s->twin->order, order);
}

int check_overlap(const void* a, size_t na, const void* b, size_t nb, const std::string& who) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  if (x < y + nb && y < x + na) {
    set_error(who + ": v_dst overlaps v_src (the reorder cannot run in place)");
    return 1;
  }
  return 0;
}

int twin_enqueue(edigpu_sector* src, const TwinPlan& p, const void* v_src, void* v_dst, int nvec, hipStream_t st) {
  if (p.transpose) return launch_twin_transpose(p.cplx, p.R, p.C, p.nblk, nvec, v_src, v_dst, st);
  return launch_twin_gather(p.cplx, p.n, p.nblk, nvec, p.reverse ? nullptr : src->twin->order, v_src, v_dst, st);
}

// every check of the single-GPU entries, and the table
int twin_prepare(edigpu_sector* src, edigpu_sector* dst, const void* v_src, const void* v_dst, int nvec, const std::string& who,
                 TwinPlan& p) {
  if (!src || !dst || !v_src || !v_dst) {
    set_error(who + ": NULL argument");
    return 1;
  }
  if (nvec < 1) {
    set_error(who + ": nvec must be at least 1");
    return 1;
  }
  if (twin_plan(src, dst, false, who, p)) return 1;
  const size_t bytes = (size_t)nvec * (size_t)src->dim * (p.cplx ? 16 : 8);
  if (check_overlap(v_src, bytes, v_dst, bytes, who)) return 1;
  EDIGPU_HIP(hipSetDevice(src->device));
  if (!p.transpose && !p.reverse && twin_order_build(src, p.n, who)) return 1;
  return 0;
}

// how the units of a handle (down rows of normal mode, electronic rows of superc / nonsu2) are cut over the ranks
struct TwinCut {
  int64_t units = 0, unit_len = 1, q = 0, first = 0, count = 0;
};

int twin_cut(const edigpu_sector* s, const edigpu_comm_s* c, int nblk, const std::string& who, TwinCut& t) {
  const bool normal = s->is_normal_family();
  t.units = normal ? s->dim_dw : s->dim / nblk;
  t.unit_len = normal ? s->dim_up : 1;
  t.q = (t.units + c->world - 1) / c->world;
  t.first = std::min<int64_t>((int64_t)c->rank * t.q, t.units);
  t.count = std::max<int64_t>(0, std::min<int64_t>(t.q, t.units - t.first));
  // normal mode shards through the whole-sector handle; a superc / nonsu2 handle must BE this rank's shard
  if (normal ? !s->is_whole() : (s->nloc != t.count * nblk || s->row_first != t.first)) {
    set_error(who + (normal ? ": normal mode shards through the whole-sector handle on every rank"
                            : ": the handle does not hold this rank's shard (build it with the first / count of "
                              "edigpu_shard_plan)"));
    return 1;
  }
  return 0;
}

}  // namespace
}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_twin_sector(const edigpu_model* model, int mode, int q1, int q2, int* tq1, int* tq2, int* self_twin) {
  const std::string who = "edigpu_twin_sector";
  if (!model || !tq1 || !tq2 || !self_twin) {
    set_error(who + ": NULL argument");
    return 1;
  }
  bool self = false;
  const std::string why = twin_sector(mode, model_ns(*model), q1, q2, *tq1, *tq2, self);
  if (!why.empty()) {
    set_error(who + ": " + why);
    return 1;
  }
  *self_twin = self ? 1 : 0;
  return 0;
}

int edigpu_apply_twin(edigpu_handle src, edigpu_handle dst, const void* v_src_dev, void* v_dst_dev, int nvec, void* stream) {
  TwinPlan p;
  if (twin_prepare(src, dst, v_src_dev, v_dst_dev, nvec, "edigpu_apply_twin", p)) return 1;
  return twin_enqueue(src, p, v_src_dev, v_dst_dev, nvec, (hipStream_t)stream);
}

int edigpu_time_twin(edigpu_handle src, edigpu_handle dst, const void* v_src_dev, void* v_dst_dev, int warmup, int steps,
                     double* ms) {
  const std::string who = "edigpu_time_twin";
  if (!ms || warmup < 0 || steps <= 0) {
    set_error(who + ": bad argument");
    return 1;
  }
  TwinPlan p;
  if (twin_prepare(src, dst, v_src_dev, v_dst_dev, 1, who, p)) return 1;
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  std::vector<float> t((size_t)steps, 0.f);
  for (int k = 0; k < warmup + steps && !rc; k++) {
    rc |= hipEventRecord(e0, src->stream) != hipSuccess;
    rc |= twin_enqueue(src, p, v_src_dev, v_dst_dev, 1, src->stream);
    rc |= hipEventRecord(e1, src->stream) != hipSuccess;
    rc |= hipEventSynchronize(e1) != hipSuccess;
    if (!rc && k >= warmup) rc |= hipEventElapsedTime(&t[(size_t)(k - warmup)], e0, e1) != hipSuccess;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    if (std::string(edigpu_last_error()).empty()) set_error(who + ": HIP failure");
    return 1;
  }
  std::sort(t.begin(), t.end());
  *ms = t[t.size() / 2];
  return 0;
}

int edigpu_apply_twin_sharded(edigpu_handle src, edigpu_handle dst, edigpu_comm c, const void* v_src_shard, void* v_dst_shard,
                              int nvec) {
  const std::string who = "edigpu_apply_twin_sharded";
  if (!src || !dst || !c) {
    set_error(who + ": NULL argument");
    return 1;
  }
  if (nvec < 1) {
    set_error(who + ": nvec must be at least 1");
    return 1;
  }
  TwinPlan p;
  TwinCut cs, cd;
  if (twin_plan(src, dst, true, who, p) || twin_cut(src, c, p.nblk, who, cs) || twin_cut(dst, c, p.nblk, who, cd)) return 1;
  // in doubles: this rank's two shards of one vector, the padded part of one vector in the all-gather
  const int w = p.cplx ? 2 : 1;
  const int64_t vstride = cs.q * cs.unit_len * p.nblk;  // elements
  const int64_t nsrc = cs.count * cs.unit_len * p.nblk * w, ndst = cd.count * cd.unit_len * p.nblk * w;
  const int64_t part = std::max<int64_t>(vstride * w, 1);
  if ((nsrc && !v_src_shard) || (ndst && !v_dst_shard)) {
    set_error(who + ": NULL vector");
    return 1;
  }
  const double* vs = static_cast<const double*>(v_src_shard);
  double* vd = static_cast<double*>(v_dst_shard);
  const bool src_dev = nsrc == 0 || on_device(vs), dst_dev = ndst == 0 || on_device(vd);
  if (nsrc && ndst && src_dev && dst_dev &&
      check_overlap(vs, (size_t)nvec * nsrc * sizeof(double), vd, (size_t)nvec * ndst * sizeof(double), who))
    return 1;
  EDIGPU_HIP(hipSetDevice(src->device));
  if (!p.transpose && !p.reverse && twin_order_build(src, p.n, who)) return 1;
  hipStream_t st = src->stream;
  ShardWorkspace& ws = c->ws;
  if (dev_grow(&ws.seed_full, &ws.seed_full_cap, part * nvec * c->world)) return 1;
  double* out = vd;
  if (!dst_dev) {
    if (dev_grow(&ws.seed_io, &ws.seed_io_cap, ndst * nvec)) return 1;
    out = ws.seed_io;
  }
  // equal padded parts in rank order, nvec vectors each.  A device shard that fills its part is sent from where it is;
  // any other goes through the send buffer, whose padding holds zeros (it is never addressed)
  const double* send = vs;
  if (nsrc != part || !src_dev) {
    if (dev_grow(&ws.seed_send, &ws.seed_send_cap, part * nvec)) return 1;
    for (int k = 0; k < nvec; k++) {
      double* to = ws.seed_send + (int64_t)k * part;
      if (nsrc) EDIGPU_HIP(hipMemcpyAsync(to, vs + (int64_t)k * nsrc, (size_t)nsrc * sizeof(double), hipMemcpyDefault, st));
      if (part > nsrc) EDIGPU_HIP(hipMemsetAsync(to + nsrc, 0, (size_t)(part - nsrc) * sizeof(double), st));
    }
    send = ws.seed_send;
  }
  if (comm_all_gather(c, send, ws.seed_full, (size_t)(part * nvec), st)) return 1;
  if (ndst) {
    ShardWindow win;
    win.j_first = cd.first;
    win.j_count = cd.count;
    win.s.q = cs.q;
    win.s.units = cs.units;
    win.s.unit_len = cs.unit_len;
    win.s.nblk = p.nblk;
    win.s.chunk = vstride * nvec;
    const int rc = p.transpose ? launch_twin_transpose_window(p.cplx, p.R, p.C, nvec, win, vstride, ws.seed_full, out, st)
                               : launch_twin_gather_window(p.cplx, p.n, nvec, win, vstride,
                                                           p.reverse ? nullptr : src->twin->order, ws.seed_full, out, st);
    if (rc) return 1;
  }
  if (out != vd) EDIGPU_HIP(hipMemcpyAsync(vd, out, (size_t)(ndst * nvec) * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
