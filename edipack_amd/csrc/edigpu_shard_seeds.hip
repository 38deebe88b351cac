// edigpu_shard_seeds.hip -- the Green's-function and pair seeds on sharded vectors (include/edigpu.h:
// edigpu_apply_cops_sharded, edigpu_apply_pairs_sharded and their host-only _info twins): the step between the sharded
// eigensolver and the sharded tridiagonalisation, without gathering the state on one rank (the reference builds the seeds
// on the master rank and scatters them: ED_NORMAL/ED_GF_NORMAL.f90:141-175, ED_CHI_PAIR.f90:129-241,
// ED_AUX_FUNX.f90:598-692).
//
// Every rank computes ITS shard of the destination.  Two routes:
//   local       the operators leave the sharded index alone (normal mode: up operators; pair terms without a down
//               operator): the single-GPU kernel on the rank's own rows, no collective, no copy of the source.
//   all-gather  one all-gather of the ranks' padded chunks, then the window + source form of the single-GPU kernel
//               (shard_src.hpp: with phonon blocks the gathered vector is NOT in the reference's layout).
// A plan (host only, no device touched) makes every check of a call and chooses the route; the _info entries return it.
// The real, phonon-free sectors keep the route they had: apply_cops_rows on the gathered vector.
#include <algorithm>
#include <string>
#include <vector>

#include "host_axisop.hpp"
#include "host_pairs.hpp"
#include "kernels.hpp"
#include "shard_comm.hpp"

namespace edigpu {
namespace {

enum SeedKind { kRows = 0, kAxis = 1, kFlatBlocks = 2, kPairs = 3 };

struct SeedPlan {
  SeedKind kind = kRows;
  bool local = false;
  bool cplx_coef = false;
  edigpu_sector *rs = nullptr, *rd = nullptr;  // the handles the geometry is taken from (complex sectors: the real image)
  ShardGeom gs, gd;
  int64_t nsrc = 0, ndst = 0, chunk = 0;  // doubles: this rank's two shards, the padded chunk of the all-gather
  double cre[kAxisMaxTerms] = {0}, cim[kAxisMaxTerms] = {0};
  AxisTables axis;
  PairsTables pairs;
  ShardSrc from() const {  // the gathered source, in doubles
    ShardSrc s;
    s.q = gs.q;
    s.units = gs.units;
    s.unit_len = gs.unit_len * gs.w;
    s.nblk = gs.nblk;
    s.chunk = s.q * s.unit_len * s.nblk;
    return s;
  }
};

// How the rows of a handle are cut.  A seed needs nothing of the product's exchange, so a whole normal-mode sector is
// served whatever exchange its product would take (a destination of one down row over ten ranks included); every other
// handle must be this rank's shard, as for the sharded product.
int seed_rows(const edigpu_sector* s, const edigpu_comm_s* c, const std::string& who, ShardGeom& g) {
  if (s->kind == kCmplxNormal) {  // (real_image found no doubled real sector)
    set_error(who + ": four-product complex sectors are single-shard");
    return 1;
  }
  shard_rows(s, c, g);
  if (!(s->kind == kNormal && s->is_whole()) && (s->nloc != g.nloc || s->row_first != g.first * g.unit_len)) {
    set_error(who + ": the handle does not hold this rank's shard (build it with the first / count of edigpu_shard_plan)");
    return 1;
  }
  return 0;
}

// the geometry of both sides and the sizes the routes share; product: the geometry of the sharded product with its
// refusals (the route of the real, phonon-free sectors, as it was)
int plan_geometry(edigpu_sector* src, edigpu_sector* dst, edigpu_comm_s* c, const std::string& who, SeedPlan& p, bool product = false) {
  p.rs = real_image(src);
  p.rd = real_image(dst);
  if (product ? shard_geometry(p.rs, c, p.gs) || shard_geometry(p.rd, c, p.gd)
              : seed_rows(p.rs, c, who, p.gs) || seed_rows(p.rd, c, who, p.gd))
    return 1;
  p.nsrc = p.gs.nloc * p.gs.w;
  p.ndst = p.gd.nloc * p.gd.w;
  p.chunk = std::max<int64_t>(p.gs.chunk * p.gs.w, 1);
  if (p.local && (p.gs.units != p.gd.units || p.gs.nblk != p.gd.nblk)) {
    set_error(who + ": internal error (the local route needs the same rows on both sides)");
    return 1;
  }
  return 0;
}

int cops_plan(edigpu_sector* src, edigpu_sector* dst, edigpu_comm_s* c, int nops, const double* coef2, const int32_t* create,
              const int32_t* iorb, const int32_t* ispin, const std::string& who, SeedPlan& p) {
  const bool phonons = src->has_phonons() || dst->has_phonons();
  if (src->kind == kCmplxNormal || dst->kind == kCmplxNormal || ((src->kind == kNormal || dst->kind == kNormal) && phonons)) {
    // normal mode, phonon or complex sectors: all operators in one pass along one axis (kernels_axisop.hip)
    p.kind = kAxis;
    if (nops < 1 || nops > kAxisMaxTerms) {
      set_error(who + ": nops must be 1 .. " + std::to_string(kAxisMaxTerms));
      return 1;
    }
    for (int k = 0; k < nops; k++) {
      p.cre[k] = coef2[2 * k];
      p.cim[k] = coef2[2 * k + 1];
      p.cplx_coef = p.cplx_coef || p.cim[k] != 0.0;
    }
    // (complex coefficients on real handles are refused in there; real ones on complex handles run on the interleaved
    // doubles, as in edigpu_apply_cops_normal)
    if (axisop_tables(src, dst, nops, create, iorb, ispin, p.cplx_coef, who.c_str(), p.axis)) return 1;
    p.local = ispin[0] == 0;  // every operator of a call acts on the spin of the first (axisop_build_normal)
    return plan_geometry(src, dst, c, who, p);
  }
  if (src->is_flat_family() && dst->is_flat_family() && phonons) {
    p.kind = kFlatBlocks;
    if (plan_geometry(src, dst, c, who, p)) return 1;
    const ShardSrc from = shard_src_in_pairs(p.from());
    return apply_cops_rows_check(src, dst, nops, coef2, create, iorb, ispin, who.c_str(), &from);
  }
  p.kind = kRows;
  if (plan_geometry(src, dst, c, who, p, true)) return 1;
  return apply_cops_rows_check(src, dst, nops, coef2, create, iorb, ispin, who.c_str());
}

int pairs_plan(edigpu_sector* src, edigpu_sector* dst, edigpu_comm_s* c, int nterms, const double* coef, const int32_t* create1,
               const int32_t* iorb1, const int32_t* ispin1, const int32_t* create2, const int32_t* iorb2, const int32_t* ispin2,
               const std::string& who, SeedPlan& p) {
  p.kind = kPairs;
  if (pairs_shard_tables(src, dst, nterms, coef, create1, iorb1, ispin1, create2, iorb2, ispin2, who, p.pairs)) return 1;
  p.local = p.pairs.id_dw == (1u << p.pairs.nterms) - 1u;  // no term has a down operator
  return plan_geometry(src, dst, c, who, p);
}

// the vectors of a call: NULL only where the rank owns no row; device vectors must not overlap
int check_vectors(const SeedPlan& p, const double* v_src, const double* v_dst, const std::string& who) {
  if ((p.nsrc && !v_src) || (p.ndst && !v_dst)) {
    set_error(who + ": NULL vector");
    return 1;
  }
  if (p.nsrc && p.ndst && on_device(v_src) && on_device(v_dst)) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(v_src), b = reinterpret_cast<uintptr_t>(v_dst);
    if (a < b + (uintptr_t)p.ndst * sizeof(double) && b < a + (uintptr_t)p.nsrc * sizeof(double)) {
      set_error(who + ": v_dst_shard overlaps v_src_shard (the gather cannot run in place)");
      return 1;
    }
  }
  return 0;
}

// Runs a planned call.  gather(full, out): the window form on the gathered source; local(src, out): the single-GPU form on
// the rank's rows; both enqueue on st or return after it has finished.  Host vectors are staged in the communicator's
// buffers, which only grow.
template <class Gather, class Local>
int run_plan(edigpu_comm_s* c, const SeedPlan& p, const double* v_src, double* v_dst, hipStream_t st, Gather gather, Local local) {
  ShardWorkspace& w = c->ws;
  const int64_t half = (p.nsrc + 1) / 2 * 2;  // (a staged destination starts on 16 bytes as well)
  const bool dst_dev = p.ndst == 0 || on_device(v_dst);
  double* out = v_dst;
  if (p.local) {
    if (p.ndst == 0) return 0;  // (the same rows on both sides: nothing to read either)
    const bool src_dev = on_device(v_src);
    if ((!src_dev || !dst_dev) && dev_grow(&w.seed_io, &w.seed_io_cap, half + p.ndst)) return 1;
    const double* in = v_src;
    if (!src_dev) {
      EDIGPU_HIP(hipMemcpyAsync(w.seed_io, v_src, (size_t)p.nsrc * sizeof(double), hipMemcpyHostToDevice, st));
      in = w.seed_io;
    }
    if (!dst_dev) out = w.seed_io + half;
    if (local(in, out)) return 1;
  } else {
    if (dev_grow(&w.seed_full, &w.seed_full_cap, p.chunk * c->world)) return 1;
    if (!dst_dev && dev_grow(&w.seed_io, &w.seed_io_cap, p.ndst)) return 1;  // (the source goes through the send buffer)
    if (!dst_dev) out = w.seed_io;
    // equal padded chunks in rank order.  A device shard that fills its chunk is sent from where it is; any other goes
    // through the send buffer, whose padding holds zeros (it is never addressed)
    const double* send = v_src;
    if (p.nsrc != p.chunk || !on_device(v_src)) {
      if (dev_grow(&w.seed_send, &w.seed_send_cap, p.chunk)) return 1;
      if (p.nsrc) EDIGPU_HIP(hipMemcpyAsync(w.seed_send, v_src, (size_t)p.nsrc * sizeof(double), hipMemcpyDefault, st));
      if (p.chunk > p.nsrc)
        EDIGPU_HIP(hipMemsetAsync(w.seed_send + p.nsrc, 0, (size_t)(p.chunk - p.nsrc) * sizeof(double), st));
      send = w.seed_send;
    }
    if (comm_all_gather(c, send, w.seed_full, (size_t)p.chunk, st)) return 1;
    if (p.ndst && gather(w.seed_full, out)) return 1;
  }
  if (out != v_dst) EDIGPU_HIP(hipMemcpyAsync(v_dst, out, (size_t)p.ndst * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

void plan_info(const SeedPlan& p, int64_t info[2]) {
  info[0] = p.local ? 0 : 1;
  info[1] = p.local ? 0 : p.chunk;
}

}  // namespace
}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_apply_cops_sharded(edigpu_handle src, edigpu_handle dst, edigpu_comm c, const double* v_src_shard,
                              double* v_dst_shard, int nops, const double* coef_re_im, const int32_t* create,
                              const int32_t* iorb, const int32_t* ispin) {
  const std::string who = "edigpu_apply_cops_sharded";
  if (!src || !dst || !c || nops <= 0 || !coef_re_im || !create || !iorb || !ispin) {
    set_error(who + ": bad argument");
    return 1;
  }
  SeedPlan p;
  if (cops_plan(src, dst, c, nops, coef_re_im, create, iorb, ispin, who, p) || check_vectors(p, v_src_shard, v_dst_shard, who))
    return 1;
  EDIGPU_HIP(hipSetDevice(src->device));
  hipStream_t st = p.rs->stream;
  const int cplx = p.cplx_coef ? 1 : 0;
  const double* cim = p.cplx_coef ? p.cim : nullptr;
  return run_plan(
      c, p, v_src_shard, v_dst_shard, st,
      [&](const double* full, double* out) -> int {
        if (p.kind == kAxis) {
          // down operators: the rank's window of the down axis, every phonon block, from the gathered rows
          AxisArgs a;
          if (axisop_upload(dst, p.axis, p.cre, cim, a, st)) return 1;
          ShardWindow w;
          w.j_first = p.gd.first;
          w.j_count = p.gd.count;
          w.s = p.from();
          const int rc = launch_apply_axisop_window(a, w, cplx, full, out, st);
          EDIGPU_HIP(hipStreamSynchronize(st));  // (the host table is pageable and leaves scope)
          return rc;
        }
        if (p.kind == kFlatBlocks) {
          const ShardSrc from = shard_src_in_pairs(p.from());
          return apply_cops_rows(src, dst, full, out, p.gd.first, p.gd.count, nops, coef_re_im, create, iorb, ispin, st, who.c_str(),
                                 &from, true);
        }
        // without phonon blocks the gathered chunks are the whole source vector in the reference's layout
        return apply_cops_rows(src, dst, full, out, p.gd.first, p.gd.count, nops, coef_re_im, create, iorb, ispin, st, who.c_str(),
                               nullptr, true);
      },
      [&](const double* in, double* out) -> int {
        // up operators: the shard plan is the same on both sides and the rank's rows are a vector of count (Nph + 1)
        // rows along the up axis
        AxisArgs a;
        if (axisop_upload(dst, p.axis, p.cre, cim, a, st)) return 1;
        a.O = p.gd.count * p.gd.nblk;
        const int rc = launch_apply_axisop(a, cplx, in, out, st);
        EDIGPU_HIP(hipStreamSynchronize(st));
        return rc;
      });
}

int edigpu_apply_cops_sharded_info(edigpu_handle src, edigpu_handle dst, edigpu_comm c, int nops, const double* coef_re_im,
                                   const int32_t* create, const int32_t* iorb, const int32_t* ispin, int64_t info[2]) {
  const std::string who = "edigpu_apply_cops_sharded_info";
  if (!src || !dst || !c || nops <= 0 || !coef_re_im || !create || !iorb || !ispin || !info) {
    set_error(who + ": bad argument");
    return 1;
  }
  SeedPlan p;
  if (cops_plan(src, dst, c, nops, coef_re_im, create, iorb, ispin, who, p)) return 1;
  plan_info(p, info);
  return 0;
}

int edigpu_apply_pairs_sharded(edigpu_handle src, edigpu_handle dst, edigpu_comm c, const double* v_src_shard,
                               double* v_dst_shard, int nterms, const double* coef, const int32_t* create1,
                               const int32_t* iorb1, const int32_t* ispin1, const int32_t* create2, const int32_t* iorb2,
                               const int32_t* ispin2) {
  const std::string who = "edigpu_apply_pairs_sharded";
  if (!src || !dst || !c || !coef || !create1 || !iorb1 || !ispin1 || !create2 || !iorb2 || !ispin2) {
    set_error(who + ": NULL argument");
    return 1;
  }
  SeedPlan p;
  if (pairs_plan(src, dst, c, nterms, coef, create1, iorb1, ispin1, create2, iorb2, ispin2, who, p) ||
      check_vectors(p, v_src_shard, v_dst_shard, who))
    return 1;
  EDIGPU_HIP(hipSetDevice(src->device));
  hipStream_t st = src->stream;
  return run_plan(
      c, p, v_src_shard, v_dst_shard, st,
      [&](const double* full, double* out) -> int {
        ShardWindow w;
        w.j_first = p.gd.first;
        w.j_count = p.gd.count;
        w.s = p.from();
        return pairs_shard_call(src, p.pairs, &w, 0, full, out, st);
      },
      [&](const double* in, double* out) -> int { return pairs_shard_call(src, p.pairs, nullptr, p.gd.count, in, out, st); });
}

int edigpu_apply_pairs_sharded_info(edigpu_handle src, edigpu_handle dst, edigpu_comm c, int nterms, const double* coef,
                                    const int32_t* create1, const int32_t* iorb1, const int32_t* ispin1, const int32_t* create2,
                                    const int32_t* iorb2, const int32_t* ispin2, int64_t info[2]) {
  const std::string who = "edigpu_apply_pairs_sharded_info";
  if (!src || !dst || !c || !coef || !create1 || !iorb1 || !ispin1 || !create2 || !iorb2 || !ispin2 || !info) {
    set_error(who + ": NULL argument");
    return 1;
  }
  SeedPlan p;
  if (pairs_plan(src, dst, c, nterms, coef, create1, iorb1, ispin1, create2, iorb2, ispin2, who, p)) return 1;
  plan_info(p, info);
  return 0;
}

}  // extern "C"
