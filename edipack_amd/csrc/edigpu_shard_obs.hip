// edigpu_shard_obs.hip -- occupation and phonon observables and the impurity density matrix on sharded vectors
// (include/edigpu.h: edigpu_occ_moments_sharded, edigpu_apply_occ_sharded, edigpu_apply_xph_sharded,
// edigpu_ph_rdm_sharded, edigpu_imp_rdm_sharded, edigpu_imp_rdm_flat_sharded[_info]).
//
// The four operators are local to a row and to the row's phonon blocks, and a rank holds all phonon blocks of its rows:
// the kernels of kernels_occ.hip / kernels_ph.hip run unchanged on tables made for the rank's rows (the shard views of
// edigpu_occ.hip / edigpu_ph.hip; host_occ.hpp occ_shard_view, host_ph.hpp ph_shard_plan_*).  The per-rank sums leave
// the fixed-order final kernels, one all-reduce adds the packed sums of the ranks (in rank order on every rank), and the
// host expansions of the single-GPU entries follow: no floating-point atomics, the same bits on every rank and call.
// Takes the place of gathering every state on one rank (es_return_dvector_mpi, ED_EIGENSPACE.f90:723-793).
// The impurity density matrix is not local to a row -- it needs the whole run of down rows of a bath word -- and
// exchanges the few rows a rank boundary cuts off first (at the end of this file); in superc / nonsu2 it needs the whole
// slab of rows of a bath word down, and the ranks exchange the elements of the slabs their boundaries cut.
#include <algorithm>
#include <string>
#include <vector>

#include "host_occ.hpp"
#include "host_ph.hpp"
#include "kernels.hpp"
#include "shard_comm.hpp"

namespace edigpu {
namespace {

// this rank's rows of handle s (down rows of normal mode, rows of superc / nonsu2) and the size of its shard
struct ObsGeom {
  int64_t first = 0, count = 0;
  int64_t len = 0;  // doubles of one vector's shard
};

// the refusals the four entries share, then the geometry of the sharded product (its messages stand)
int obs_geometry(edigpu_sector* s, edigpu_comm_s* c, const std::string& who, bool phonon, bool rdm, ObsGeom& og) {
  if (phonon ? ph_refuse_kind(s, who, rdm) : occ_refuse_kind(s, who)) return 1;
  if (s->model.norb < 1 || s->model.norb > kOccMaxOrb) {
    set_error(who + ": norb out of range");
    return 1;
  }
  ShardGeom g;
  if (shard_geometry(real_image(s), c, g)) return 1;
  og.first = g.first;
  og.count = g.count;
  og.len = g.count * (s->is_normal_family() ? s->dim_up : 1) * (s->nph + 1) * (s->is_complex ? 2 : 1);
  return 0;
}

// the vector the kernels read: v itself when it lives on the device, else its copy in the communicator's buffer at
// `offset` doubles (the buffer holds at least `cap` doubles after this)
int stage_in(edigpu_comm_s* c, const double* v, int64_t n, int64_t offset, int64_t cap, hipStream_t st, const double** out) {
  if (on_device(v)) {
    *out = v;
    return 0;
  }
  if (dev_grow(&c->ws.obs, &c->ws.obs_cap, cap)) return 1;
  EDIGPU_HIP(hipMemcpyAsync(c->ws.obs + offset, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  *out = c->ws.obs + offset;
  return 0;
}

// red[0:n) <- the sum over the ranks of `mine` (null: this rank owns no row and adds zeros), then to the host
int reduce_to_host(edigpu_comm_s* c, const double* mine, size_t n, hipStream_t st, std::vector<double>& host) {
  if (dev_grow(&c->ws.red, &c->ws.red_cap, (int64_t)n)) return 1;
  if (mine) EDIGPU_HIP(hipMemcpyAsync(c->ws.red, mine, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  else EDIGPU_HIP(hipMemsetAsync(c->ws.red, 0, n * sizeof(double), st));
  if (comm_all_reduce(c, c->ws.red, n, st)) return 1;
  host.resize(n);
  EDIGPU_HIP(hipMemcpyAsync(host.data(), c->ws.red, n * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

// dst <- op(src) on this rank's shard, host or device vectors; op(src_dev, dst_dev) enqueues on st.  Host vectors go
// through the communicator's buffer: the source at its start, a host destination in place of it (inplace) or behind it
template <class Op>
int apply_on_shard(edigpu_comm_s* c, const ObsGeom& og, const double* src, double* dst, bool inplace, hipStream_t st, Op op) {
  const int64_t half = (og.len + 1) / 2 * 2;  // (the second vector starts on 16 bytes as well)
  const double* sd = nullptr;
  if (stage_in(c, src, og.len, 0, 2 * half, st, &sd)) return 1;
  double* dd = dst;
  if (!on_device(dst)) {
    if (dev_grow(&c->ws.obs, &c->ws.obs_cap, 2 * half)) return 1;  // (kept when stage_in made it)
    dd = c->ws.obs + (inplace && sd == c->ws.obs ? 0 : half);
  }
  if (op(sd, dd)) return 1;
  if (dd != dst) EDIGPU_HIP(hipMemcpyAsync(dst, dd, (size_t)og.len * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // namespace
}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_occ_moments_sharded(edigpu_handle s, edigpu_comm c, const double* v_shard, int nvec, double* moments_host,
                               double* norm2_host) {
  const std::string who = "edigpu_occ_moments_sharded";
  if (!s || !c || !moments_host || nvec <= 0) {
    set_error(who + (!s || !c || !moments_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  ObsGeom og;
  if (obs_geometry(s, c, who, false, false, og)) return 1;
  if (og.count > 0 && !v_shard) {
    set_error(who + ": NULL argument");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const double *vd = nullptr, *mine = nullptr;
  if (og.count > 0 && (stage_in(c, v_shard, og.len * nvec, 0, og.len * nvec, st, &vd) ||
                       occ_shard_moments(s, og.first, og.count, vd, nvec, &mine, who)))
    return 1;
  std::vector<double> sums;
  if (reduce_to_host(c, mine, (size_t)nvec * kOccSums, st, sums)) return 1;
  const int norb = s->model.norb, n2 = 2 * norb;
  for (int k = 0; k < nvec; k++)
    occ_expand_sums(sums.data() + (size_t)k * kOccSums, norb, moments_host + (size_t)k * n2 * n2, norm2_host ? norm2_host + k : nullptr);
  return 0;
}

int edigpu_apply_occ_sharded(edigpu_handle s, edigpu_comm c, const double* v_src_shard, double* v_dst_shard, const double* w_up,
                             const double* w_dw) {
  const std::string who = "edigpu_apply_occ_sharded";
  if (!s || !c || !w_up || !w_dw) {
    set_error(who + ": NULL argument");
    return 1;
  }
  ObsGeom og;
  if (obs_geometry(s, c, who, false, false, og)) return 1;
  if (og.count <= 0) return 0;
  if (!v_src_shard || !v_dst_shard) {
    set_error(who + ": NULL argument");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  return apply_on_shard(c, og, v_src_shard, v_dst_shard, true, s->stream, [&](const double* src, double* dst) {
    return occ_shard_apply(s, og.first, og.count, src, dst, w_up, w_dw, who);
  });
}

int edigpu_apply_xph_sharded(edigpu_handle s, edigpu_comm c, const double* v_src_shard, double* v_dst_shard) {
  const std::string who = "edigpu_apply_xph_sharded";
  if (!s || !c) {
    set_error(who + ": NULL argument");
    return 1;
  }
  ObsGeom og;
  if (obs_geometry(s, c, who, true, false, og)) return 1;
  if (og.count <= 0) return 0;
  if (!v_src_shard || !v_dst_shard) {
    set_error(who + ": NULL argument");
    return 1;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(v_src_shard), b = reinterpret_cast<uintptr_t>(v_dst_shard);
  const uintptr_t bytes = (uintptr_t)og.len * sizeof(double);
  if (a < b + bytes && b < a + bytes) {
    set_error(who + ": the destination must not overlap the source (an output block reads its two neighbours)");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  return apply_on_shard(c, og, v_src_shard, v_dst_shard, false, s->stream, [&](const double* src, double* dst) {
    return ph_shard_apply(s, og.first, og.count, src, dst, who);
  });
}

int edigpu_ph_rdm_sharded(edigpu_handle s, edigpu_comm c, const double* v_shard, int nvec, double* rho_host, double* norm2_host) {
  const std::string who = "edigpu_ph_rdm_sharded";
  if (!s || !c || !rho_host || nvec <= 0) {
    set_error(who + (!s || !c || !rho_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  ObsGeom og;
  if (obs_geometry(s, c, who, true, true, og)) return 1;
  if (og.count > 0 && !v_shard) {
    set_error(who + ": NULL argument");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  const double *vd = nullptr, *mine = nullptr;
  if (og.count > 0 && (stage_in(c, v_shard, og.len * nvec, 0, og.len * nvec, st, &vd) ||
                       ph_shard_rdm(s, og.first, og.count, vd, nvec, &mine, who)))
    return 1;
  const int dimph = s->nph + 1, cw = s->is_complex ? 2 : 1, ncls = ph_num_classes(s->model.norb);
  const size_t nslot = (size_t)ph_slots(dimph) * cw, nmat = (size_t)dimph * dimph * cw;
  std::vector<double> sums;
  if (reduce_to_host(c, mine, (size_t)nvec * ncls * nslot, st, sums)) return 1;
  for (int k = 0; k < nvec; k++) {
    double tr = 0.0;
    for (int cl = 0; cl < ncls; cl++)
      tr += ph_expand_slots(sums.data() + ((size_t)k * ncls + cl) * nslot, dimph, cw, rho_host + ((size_t)k * ncls + cl) * nmat);
    if (norm2_host) norm2_host[k] = tr;
  }
  return 0;
}

// rho_imp = Tr_bath |v><v| needs the whole run of down rows of a bath word, and a rank boundary can cut one: every rank
// sends its first H rows (those of a run that starts on an earlier rank), one all-gather, and the rank a cut run starts on
// completes it in a slab (edigpu_internal.hpp rdm_shard_*; host_rdm.hpp RdmShardPlan).  H is the same on every rank, so
// the all-gather is issued by all or by none.
int edigpu_imp_rdm_sharded(edigpu_handle s, edigpu_comm c, const double* v_shard, int nvec, double* rdm_host, double* norm2_host) {
  const std::string who = "edigpu_imp_rdm_sharded";
  if (!s || !c || !rdm_host || nvec <= 0) {
    set_error(who + (!s || !c || !rdm_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  if (rdm_shard_refuse(s, who)) return 1;
  ShardGeom g;
  if (shard_geometry(real_image(s), c, g)) return 1;
  if (g.count > 0 && !v_shard) {
    set_error(who + ": NULL argument");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  RdmShardInfo ri;
  if (rdm_shard_prepare(s, g.first, g.count, c->world, who, &ri)) return 1;
  const int nblk = s->nph + 1;
  const int64_t rowlen = s->dim_up * ri.cw, len = g.count * rowlen * nblk;
  const double* vd = nullptr;
  if (g.count > 0 && stage_in(c, v_shard, len * nvec, 0, len * nvec, st, &vd)) return 1;
  ShardWorkspace& w = c->ws;
  if (ri.H > 0) {
    const int64_t n = (int64_t)nvec * nblk * ri.H * rowlen;
    if (dev_grow(&w.halo, &w.halo_cap, n) || dev_grow(&w.halos, &w.halos_cap, n * c->world)) return 1;
    if (rdm_shard_pack(s, vd, nvec, w.halo) || comm_all_gather(c, w.halo, w.halos, (size_t)n, st)) return 1;
  }
  if (dev_grow(&w.slab, &w.slab_cap, (int64_t)nvec * nblk * ri.tail_ld * rowlen)) return 1;
  const double* mine = nullptr;
  if (rdm_shard_enqueue(s, vd, nvec, w.halos, w.slab, &mine)) return 1;
  std::vector<double> tri;
  if (reduce_to_host(c, mine, (size_t)nvec * ri.ntri * ri.cw, st, tri)) return 1;
  rdm_shard_expand(s, tri.data(), nvec, rdm_host, norm2_host);
  return 0;
}

// The same of superc / nonsu2 vectors: a tile needs the whole SLAB of a bath word down -- its 2^Norb rows, a contiguous
// range of elements -- and a row shard cuts anywhere in it.  Every rank sends its first H elements (those of a slab that
// starts on an earlier rank), one all-gather, and the rank a cut slab starts on completes it in a buffer
// (edigpu_internal.hpp rdm_flat_shard_*; host_rdm_flat.hpp RdmFlatShardPlan).  H is bounded by one slab and is the same
// on every rank, so the all-gather is issued by all or by none.
static int rdm_flat_sharded_checks(edigpu_sector* s, edigpu_comm_s* c, const std::string& who, ShardGeom& g) {
  if (rdm_flat_shard_refuse(s, who)) return 1;
  return shard_geometry(s, c, g);
}

int edigpu_imp_rdm_flat_sharded(edigpu_handle s, edigpu_comm c, const double* v_shard, int nvec, double* rdm_host,
                                double* norm2_host) {
  const std::string who = "edigpu_imp_rdm_flat_sharded";
  if (!s || !c || !rdm_host || nvec <= 0) {
    set_error(who + (!s || !c || !rdm_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  ShardGeom g;
  if (rdm_flat_sharded_checks(s, c, who, g)) return 1;
  if (g.count > 0 && !v_shard) {
    set_error(who + ": NULL argument");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  RdmFlatShardInfo ri;
  if (rdm_flat_shard_prepare(s, g.first, g.count, c->world, who, &ri)) return 1;
  const int nblk = s->nph + 1;
  const int64_t len = g.count * nblk * ri.cw;
  const double* vd = nullptr;
  if (g.count > 0 && stage_in(c, v_shard, len * nvec, 0, len * nvec, st, &vd)) return 1;
  ShardWorkspace& w = c->ws;
  if (ri.H > 0) {
    const int64_t n = (int64_t)nvec * nblk * ri.H * ri.cw;
    if (dev_grow(&w.halo, &w.halo_cap, n) || dev_grow(&w.halos, &w.halos_cap, n * c->world)) return 1;
    if (rdm_flat_shard_pack(s, vd, nvec, w.halo) || comm_all_gather(c, w.halo, w.halos, (size_t)n, st)) return 1;
  }
  if (dev_grow(&w.slab, &w.slab_cap, (int64_t)nvec * nblk * ri.tail_len * ri.cw)) return 1;
  const double* mine = nullptr;
  if (rdm_flat_shard_enqueue(s, vd, nvec, w.halos, w.slab, &mine)) return 1;
  std::vector<double> tri;
  if (reduce_to_host(c, mine, (size_t)nvec * ri.ntri * ri.cw, st, tri)) return 1;
  rdm_flat_shard_expand(s, tri.data(), nvec, rdm_host, norm2_host);
  return 0;
}

int edigpu_imp_rdm_flat_sharded_info(edigpu_handle s, edigpu_comm c, int64_t info[6]) {
  const std::string who = "edigpu_imp_rdm_flat_sharded_info";
  if (!s || !c || !info) {
    set_error(who + ": NULL argument");
    return 1;
  }
  ShardGeom g;
  if (rdm_flat_sharded_checks(s, c, who, g)) return 1;
  RdmFlatShardInfo ri;
  if (rdm_flat_shard_info(s, g.first, g.count, c->world, who, &ri)) return 1;
  info[0] = ri.H;
  info[1] = ri.H * (s->nph + 1) * ri.cw;
  info[2] = ri.nslab_in;
  info[3] = ri.tail_start;
  info[4] = ri.tail_len;
  info[5] = ri.tail_own;
  return 0;
}

}  // extern "C"
