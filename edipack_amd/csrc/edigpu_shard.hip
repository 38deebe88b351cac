// edigpu_shard.hip -- the N > 1 path inside the library: the sharded product and the sharded recurrence (the
// communicator they run on: edigpu_comm.hip, shard_comm.hpp; their vector kernels: kernels_shard.hip).
//
// Takes the place of the MPI data flow of the reference's distributed products and of SciFortran's MPI Lanczos
// driver (reference paths relative to its src/singlesite):
//   spMatVec_mpi_normal_main   ED_NORMAL/ED_HAMILTONIAN_NORMAL_STORED_HxV.f90:765-929  (two vector_transpose_MPI per
//                              product, ED_NORMAL/ED_HAMILTONIAN_NORMAL_COMMON.f90:66-167, + allgather for spH0nd)
//   spMatVec_mpi_superc_main   ED_SUPERC/ED_HAMILTONIAN_SUPERC_STORED_HxV.f90:366-432  (MPI_Allgatherv :418-421)
//   spMatVec_mpi_nonsu2_main   ED_NONSU2/ED_HAMILTONIAN_NONSU2_STORED_HxV.f90:213-267  (MPI_Allgatherv :256-259)
//   directMatVec_MPI_*         ED_*/ED_HAMILTONIAN_*_DIRECT_HxV.f90 (gather first, then compute)
//   sp_lanc_tridiag(MpiComm, spHtimesV_p, vvloc, alanc, blanc)   ED_NORMAL/ED_HAMILTONIAN_NORMAL.f90:357-365
//   scatter / gather of the seed: ED_AUX_FUNX.f90:598-928 (each rank hands over its own shard here)
//
// (The c / c^+ and pair seeds on shards: edigpu_shard_seeds.hip.)
//
// One process per GPU.  The exchange of a product runs on the communicator's side stream and overlaps the part of H*v
// that needs no remote data.  A whole tridiagonalisation is enqueued without host synchronisation (RCCL) -- the
// coefficients are read back once at the end.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "exchange_index.hpp"
#include "kernels.hpp"
#include "lanczos_sums.hpp"
#include "sb_core.hpp"
#include "shard_comm.hpp"

namespace edigpu {

void shard_rows(const edigpu_sector* s, const edigpu_comm_s* c, ShardGeom& g) {
  g.w = s->is_complex ? 2 : 1;
  g.nblk = s->has_phonons() ? s->nph + 1 : 1;
  if (s->kind == kNormal) {
    g.units = s->dim_dw;
    g.unit_len = s->dim_up;
  } else {
    g.units = s->dim / g.nblk;  // electronic rows: every phonon block is sharded alike
    g.unit_len = 1;
  }
  g.q = (g.units + c->world - 1) / c->world;
  g.first = std::min<int64_t>((int64_t)c->rank * g.q, g.units);
  g.count = std::max<int64_t>(0, std::min<int64_t>(g.q, g.units - g.first));
  g.blk = g.count * g.unit_len;
  g.nloc = g.blk * g.nblk;
  g.chunk = g.q * g.unit_len * g.nblk;
}

int shard_geometry(const edigpu_sector* s, const edigpu_comm_s* c, ShardGeom& g) {
  g.loop = LoopSwitches::sample();
  shard_rows(s, c, g);
  g.transposed = s->kind == kNormal && s->is_whole() && normal_transposable_el(s);
  if (g.transposed) {
    g.halo = s->col_halo;
    g.pcol = (s->dim_up + c->world - 1) / c->world;
    g.col_first = std::min<int64_t>((int64_t)c->rank * g.pcol, s->dim_up);
    g.col_count = std::max<int64_t>(0, std::min<int64_t>(g.pcol, s->dim_up - g.col_first));
    g.pw = g.pcol + 2 * g.halo;
    g.xlen = (int64_t)c->world * g.q * g.pw;
    if (g.pcol < 1 || g.halo > g.pcol) g.transposed = false;  // blocks narrower than the halo: all-gather form
  }
  // (rows per rank for which the columns kernel's owner rank g / q is not exact: the column-block exchange)
  if (g.transposed && g.nblk == 1 && sb_shardable(s) && sb::shard_exact(c->world, g.q) && !g.loop.shard_generic) {
    g.block = true;
    g.npmax = sb_shard_panels(s, c->world);
    g.bplen = sb::shard_slot(c->world, g.npmax, g.q);
  }
  if (g.nblk > 1 && (s->sub_a || (s->kind == kNormal && !g.transposed))) {
    // like spMatVec_mpi_normal_main (ED_HAMILTONIAN_NORMAL_STORED_HxV.f90:841-904) and spMatVec_mpi_superc_main /
    // _nonsu2_main: every phonon block is exchanged on its own and the phonon / electron-phonon pass is local, which
    // holds for density couplings only
    set_error("sharded call: phonon sectors shard with density couplings g_ph(a,a) only; normal mode through the "
              "transposed exchange (whole sector, factored Hnd, at least `halo` up columns per rank), superc / nonsu2 "
              "as row shards");
    return 1;
  }
  if (!g.transposed) {
    // all-gather form: the handle must BE this rank's shard
    if (s->nloc != g.nloc || s->row_first != g.first * g.unit_len) {
      set_error("sharded call: the handle does not hold this rank's shard (build it with the first / count of "
                "edigpu_shard_plan, or -- normal mode -- build the whole sector for the transposed exchange)");
      return 1;
    }
    if (s->kind == kCmplxNormal) {
      set_error("sharded call: four-product complex sectors are single-shard");
      return 1;
    }
  }
  return 0;
}

static int comm_workspace(edigpu_comm_s* c, const ShardGeom& g, int nlanc) {
  ShardWorkspace& w = c->ws;
  const int64_t chunk = g.chunk * g.w;
  if (chunk > w.ws_chunk) {
    if (dev_realloc_zeroed_sync(w.vin, chunk) || dev_realloc_zeroed_sync(w.vout, chunk) || dev_realloc_zeroed_sync(w.tmp, chunk))
      return 1;
    w.ws_chunk = chunk;
  }
  if (!g.transposed && (chunk * c->world > w.ws_full || !w.vfull)) {
    if (dev_realloc_zeroed_sync(w.vfull, (size_t)chunk * c->world)) return 1;
    w.ws_full = chunk * c->world;
  }
  if (g.block && g.bplen > w.ws_bp) {
    for (double*& b : w.bp)
      if (dev_realloc_zeroed_sync(b, g.bplen)) return 1;
    w.ws_bp = g.bplen;
  }
  if (g.transposed && g.xlen > w.ws_x) {
    for (double** b : {&w.send, &w.recv, &w.hvc, &w.back})
      if (dev_realloc_zeroed_sync(*b, g.xlen)) return 1;
    w.ws_x = g.xlen;
  }
  if (3 * (int64_t)nlanc + 8 > w.hist_cap) {
    if (dev_realloc_zeroed_sync(w.hist, 3 * (size_t)nlanc + 8)) return 1;
    w.hist_cap = 3 * (int64_t)nlanc + 8;
  }
  if (!w.work && dev_realloc_zeroed_sync(w.work, 3 * (size_t)kRedBlocks)) return 1;
  if (!w.scr && dev_realloc_zeroed_sync(w.scr, 8)) return 1;
  return 0;
}

// One exchange of a product beside the part of the product that needs no remote data: the side stream waits for what
// st holds (the exchange's input), exchange() goes to the side stream (it passes c->side to its collective), local()
// to st, and st then waits for the exchange.  A rank that is alone exchanges nothing.
template <class Exchange, class Local>
static int overlapped(edigpu_comm_s* c, hipStream_t st, Exchange exchange, Local local) {
  if (alone(c)) return local();
  EDIGPU_HIP(hipEventRecord(c->ev_ready, st));
  EDIGPU_HIP(hipStreamWaitEvent(c->side, c->ev_ready, 0));
  if (exchange()) return 1;
  EDIGPU_HIP(hipEventRecord(c->ev_done, c->side));
  if (local()) return 1;
  EDIGPU_HIP(hipStreamWaitEvent(st, c->ev_done, 0));
  return 0;
}

// Transposed exchange on padded panels (the local-block kernels' layout, shard form: kernels_sb.hip).  What a rank
// sends to rank d -- its rows of d's panels -- is one contiguous run of the vector in that form, and what comes back lands
// in that layout again: the two all-to-alls move the buffers as they are.  bp[0] = v in the shard form, bp[1] = what
// the first exchange delivers, bp[2] = the column half on it, bp[3] = the row half; the exchange back reuses bp[1].
// H v = *rowhalf + *colhalf, element by element in the shard form.
static int sharded_hv_panels(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, hipStream_t st, const double* v,
                             const double** rowhalf, const double** colhalf) {
  double* const* bp = c->ws.bp;
  const size_t per = (size_t)sb::shard_slot(1, g.npmax, g.q);
  if (overlapped(
          c, st, [&] { return comm_all_to_all(c, v, bp[1], per, c->side); },
          [&] { return launch_sb_rows_shard(s, g.first, g.count, g.q, v, bp[3], st); }))
    return 1;
  const int p0 = c->rank * g.npmax, np = std::max(0, std::min(g.npmax, s->ib->npanels - p0));
  // (panels past the sector's last one are never computed: their slots must not hand stale numbers back)
  if (np < g.npmax) EDIGPU_HIP(hipMemsetAsync(bp[2], 0, (size_t)g.bplen * sizeof(double), st));
  if (launch_sb_cols_shard(s, p0, np, g.q, g.npmax, c->world, alone(c) ? v : bp[1], bp[2], st)) return 1;
  *rowhalf = bp[3];
  *colhalf = bp[2];
  if (!alone(c)) {
    if (comm_all_to_all(c, bp[2], bp[1], per, st)) return 1;
    *colhalf = bp[1];
  }
  return 0;
}

// out <- H in on the local rows through the padded panels; in / out: the shard's rows in the reference's layout
static int sharded_hv_block(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, hipStream_t st, const double* in,
                            double* out) {
  const double *rowhalf = nullptr, *colhalf = nullptr;
  if (sb_shard_to_panels(s, in, c->ws.bp[0], g.count, g.q, c->world, st)) return 1;
  if (sharded_hv_panels(s, c, g, st, c->ws.bp[0], &rowhalf, &colhalf)) return 1;
  return sb_shard_from_panels_add(s, rowhalf, colhalf, out, g.count, g.q, st);
}

// tmp <- (H vin) on the local rows.  pre_packed: the send buffer already holds vin (fused rotate).  The exchange runs
// on the side stream beside the part of the product that needs no remote data.  *back_out: what the column shards sent
// back and the caller still has to add (unpack), or null
static int sharded_hv(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, bool pre_packed, hipStream_t st,
                      const double** back_out) {
  ShardWorkspace& w = c->ws;
  *back_out = nullptr;
  if (g.block) return sharded_hv_block(s, c, g, st, w.vin, w.tmp);
  // a world of one exchanges nothing: the second half of the product reads what the first exchange would have sent
  const bool solo = alone(c);
  if (g.transposed) {
    const size_t nx = (size_t)(g.q * g.pw);
    for (int b = 0; b < g.nblk; b++) {
      const double* vb = w.vin + (size_t)b * g.blk;
      double* tb = w.tmp + (size_t)b * g.blk;
      if ((!pre_packed || g.nblk > 1) &&
          edigpu_transpose_pack(s->dim_up, g.count, g.q, c->world, g.pcol, g.halo, vb, w.send, st))
        return 1;
      if (overlapped(
              c, st, [&] { return comm_all_to_all(c, w.send, w.recv, nx, c->side); },
              [&] { return launch_normal_rows(s, g.first, g.count, vb, tb, st); }))
        return 1;
      if (launch_normal_cols(s, g.col_first, g.col_count, g.pw, g.halo, solo ? w.send : w.recv, w.hvc, st)) return 1;
      if (!solo && comm_all_to_all(c, w.hvc, w.back, nx, st)) return 1;
      const double* back = solo ? w.hvc : w.back;
      if (g.nblk == 1) {
        *back_out = back;  // consumed by the caller (unpack)
        return 0;
      }
      // phonon sectors: the buffers serve the next block, so the down half is added here
      if (edigpu_transpose_unpack_add(s->dim_up, g.count, g.q, c->world, g.pcol, g.halo, back, tb, st)) return 1;
    }
    return launch_phonon_rows(s, g.first, g.count, w.vin, w.tmp, st);  // local: stored/H_ph.f90, H_e_ph.f90
  }
  if (g.nblk > 1) {
    // superc / nonsu2 phonon shards: one all-gather per phonon block beside that block's local part, then the phonon
    // and electron-phonon terms on the rows held here (stored/H_ph.f90, H_e_ph.f90: density couplings)
    const size_t nq = (size_t)g.q * g.unit_len * g.w;  // doubles per rank and block (padded; tails are never addressed)
    for (int b = 0; b < g.nblk; b++) {
      const double* vb = w.vin + (size_t)b * g.blk * g.w;
      double* tb = w.tmp + (size_t)b * g.blk * g.w;
      if (overlapped(
              c, st, [&] { return comm_all_gather(c, vb, w.vfull, nq, c->side); },
              [&] { return apply_flat_block(s, vb, nullptr, tb, 1, st); }))
        return 1;
      if (apply_flat_block(s, nullptr, solo ? vb : w.vfull, tb, 2, st)) return 1;
    }
    return launch_phonon(s, w.vin, w.tmp, st);
  }
  if (overlapped(
          c, st, [&] { return comm_all_gather(c, w.vin, w.vfull, (size_t)g.chunk * g.w, c->side); },
          [&] { return edigpu_apply_local_dev(s, w.vin, w.tmp, st); }))
    return 1;
  return edigpu_apply_remote_dev(s, solo ? w.vin : w.vfull, w.tmp, st);  // (alone: the chunk is the whole vector)
}

// out <- H in on the local rows, complete (nothing left for the caller to add): `in` and `out` are this rank's shard in
// the reference's layout, the workspace's vin / tmp themselves or any other device vectors
static int sharded_product(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, hipStream_t st, const double* in,
                           double* out) {
  // padded panels: the conversions read and write the caller's vectors themselves (no staging copies)
  if (g.block) return sharded_hv_block(s, c, g, st, in, out);
  ShardWorkspace& w = c->ws;
  const size_t bytes = (size_t)(g.nloc * g.w) * sizeof(double);
  if (in != w.vin && bytes > 0) EDIGPU_HIP(hipMemcpyAsync(w.vin, in, bytes, hipMemcpyDeviceToDevice, st));
  const double* back = nullptr;
  if (sharded_hv(s, c, g, false, st, &back)) return 1;
  if (back && edigpu_transpose_unpack_add(s->dim_up, g.count, g.q, c->world, g.pcol, g.halo, back, w.tmp, st)) return 1;
  if (out != w.tmp && bytes > 0) EDIGPU_HIP(hipMemcpyAsync(out, w.tmp, bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

static int zero_chunk(double* p, const ShardGeom& g, hipStream_t st) {  // a padded chunk of the workspace, tail included
  EDIGPU_HIP(hipMemsetAsync(p, 0, (size_t)std::max<int64_t>(g.chunk * g.w, 1) * sizeof(double), st));
  return 0;
}

// the reduced sums of the fused steps in hist: t = where those of step `it` land, tp / tpp = those of the two steps
// before it (null where there is none)
struct StepSums {
  double* t;
  const double *tp, *tpp;
  StepSums(double* hist, int it)
      : t(hist + 3 * (size_t)it), tp(it > 0 ? t - 3 : nullptr), tpp(it > 1 ? t - 6 : nullptr) {}
};

// one step of the one-reduction recurrence; T_it lands in hist[3 it .. 3 it + 3)
static int sharded_step(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, int it, hipStream_t st) {
  ShardWorkspace& w = c->ws;
  const int64_t n = g.nloc * g.w;
  const StepSums h(w.hist, it);
  if (shard_rotate3(it == 0, n, s->dim_up, g.q, c->world, g.pcol, g.halo, w.vin, w.vout, h.tp, h.tpp,
                    g.transposed && g.nblk == 1 && !g.block ? w.send : nullptr, st))
    return 1;
  const double* back = nullptr;  // (stays null for phonon blocks and padded panels: already added)
  if (sharded_hv(s, c, g, true, st, &back)) return 1;
  if (shard_add_dot3(n, s->dim_up, g.q, g.pcol, g.halo, w.vin, w.vout, w.tmp, back, h.tp, w.work, h.t, st)) return 1;
  return comm_all_reduce(c, h.t, 3, st);
}

// The recurrence with its two vectors KEPT in the padded panel layout (ShardGeom::block; LoopSwitches::shard_panel_loop off falls back
// to the rows of the reference's layout with a conversion on either side of every product): the Lanczos vector is what the
// first all-to-all sends as it is; it and the work vector live in bp[0] and bp[4] and swap roles every step
// (sharded_step_panels); the padding of the layout holds zeros in every buffer and stays zero under the element-wise
// updates, so the three sums are those of the shard.
static bool panel_loop(const ShardGeom& g) { return g.block && g.loop.shard_panel_loop; }

// after load_seed: the normalised seed goes into the panel layout, every other buffer of the loop starts from zeros
// (the buffers serve sectors of different geometry in turn: what one leaves behind is not zero in another's padding)
static int panel_loop_begin(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, hipStream_t st) {
  for (int k = 1; k < 5; k++) EDIGPU_HIP(hipMemsetAsync(c->ws.bp[k], 0, (size_t)g.bplen * sizeof(double), st));
  return sb_shard_to_panels(s, c->ws.vin, c->ws.bp[0], g.count, g.q, c->world, st);
}

static int sharded_step_panels(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, int it, hipStream_t st) {
  ShardWorkspace& w = c->ws;
  const int64_t n2 = g.bplen / 2;  // (a multiple of 8)
  const StepSums h(w.hist, it);
  // x = the vector of this step (the seed in bp[0] on step 0), o = the other one, which holds the previous vector and
  // receives the new work vector
  double* x = (it & 1) ? w.bp[4] : w.bp[0];
  double* o = (it & 1) ? w.bp[0] : w.bp[4];
  if (it > 0 && shard_panel_rotate(n2, x, o, h.tp, h.tpp, st)) return 1;
  const double *rowhalf = nullptr, *colhalf = nullptr;
  if (sharded_hv_panels(s, c, g, st, x, &rowhalf, &colhalf)) return 1;
  if (shard_panel_add_dot(n2, x, o, rowhalf, colhalf, h.tp, h.tpp, w.work, h.t, st)) return 1;
  return comm_all_reduce(c, h.t, 3, st);
}

// literal two-reduction step (beta = |w - alpha v|): alpha_it -> hist[it], beta_it^2 -> hist[nlanc + it]
static int sharded_step_exact(edigpu_sector* s, edigpu_comm_s* c, const ShardGeom& g, int it, int nlanc, hipStream_t st) {
  ShardWorkspace& w = c->ws;
  const int64_t n = g.nloc * g.w;
  double* al = w.hist + it;
  double* b2 = w.hist + nlanc + it;
  if (it > 0 && vec_rotate(n, w.vin, w.vout, w.hist + nlanc + it - 1, st)) return 1;
  if (sharded_product(s, c, g, st, w.vin, w.tmp)) return 1;
  if (vec_add_dot(n, w.vin, w.vout, w.tmp, al, w.work, st)) return 1;
  if (comm_all_reduce(c, al, 1, st)) return 1;
  if (vec_axpy_nrm2(n, w.vin, w.vout, al, b2, w.work, st)) return 1;
  return comm_all_reduce(c, b2, 1, st);
}

static int load_seed(edigpu_comm_s* c, const ShardGeom& g, const double* vin_shard, hipStream_t st) {
  const int64_t n = g.nloc * g.w;
  if (zero_chunk(c->ws.vin, g, st) || zero_chunk(c->ws.vout, g, st)) return 1;
  if (n > 0) EDIGPU_HIP(hipMemcpyAsync(c->ws.vin, vin_shard, (size_t)n * sizeof(double), hipMemcpyDefault, st));
  // |v|^2 over all ranks, then scale (lanczos_iteration's first step)
  if (vec_axpy_nrm2(n, c->ws.vin, c->ws.vin, c->ws.scr + 1, c->ws.scr, c->ws.work, st)) return 1;  // scr[1] = 0: v - 0 v
  if (comm_all_reduce(c, c->ws.scr, 1, st)) return 1;
  return vec_scale(n, c->ws.vin, c->ws.scr, st);
}

static int sharded_tridiag(edigpu_sector* s, edigpu_comm_s* c, const double* vin_shard, int nlanc, double* alanc,
                           double* blanc, double threshold, int* niter_done, double* norm2) {
  ShardGeom g;
  if (shard_geometry(s, c, g)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (comm_workspace(c, g, 2 * nlanc)) return 1;
  hipStream_t st = s->stream;
  std::fill(alanc, alanc + nlanc, 0.0);
  std::fill(blanc, blanc + nlanc, 0.0);
  if (niter_done) *niter_done = 0;
  const bool force_exact = g.loop.lanczos_exactbeta;
  std::vector<double> h(3 * (size_t)nlanc + 8);
  for (int pass = force_exact ? 1 : 0; pass < 2; pass++) {
    EDIGPU_HIP(hipMemsetAsync(c->ws.hist, 0, (size_t)c->ws.hist_cap * sizeof(double), st));
    if (load_seed(c, g, vin_shard, st)) return 1;
    const bool panels = pass == 0 && panel_loop(g);
    if (panels && panel_loop_begin(s, c, g, st)) return 1;
    for (int it = 0; it < nlanc; it++)
      if (pass == 0 ? (panels ? sharded_step_panels(s, c, g, it, st) : sharded_step(s, c, g, it, st))
                    : sharded_step_exact(s, c, g, it, nlanc, st))
        return 1;
    EDIGPU_HIP(hipMemcpyAsync(h.data(), c->ws.hist, (3 * (size_t)nlanc) * sizeof(double), hipMemcpyDeviceToHost, st));
    double n2 = 0.0;
    EDIGPU_HIP(hipMemcpyAsync(&n2, c->ws.scr, sizeof(double), hipMemcpyDeviceToHost, st));
    EDIGPU_HIP(hipStreamSynchronize(st));
    if (norm2) *norm2 = n2;
    if (!(n2 > 0.0)) return 0;  // zero seed: nothing to do (the reference skips such channels)
    bool redo = false;
    int ndone = nlanc;
    for (int k = 0; k < nlanc; k++) {
      double a, b;
      if (pass == 0) {
        const double* t = &h[3 * (size_t)k];
        a = t[0];
        const double b2 = beta2_from_sums(a, t[1], t[2], k > 0 ? t[-3] : 0.0);  // (what the kernels use: ab_from_sums)
        // more than three digits lost in the difference (the same numbers on every rank): repeat literally
        if (!(b2 > 1e-3 * t[1]) && b2 > threshold * threshold) {
          redo = true;
          break;
        }
        b = beta_from_beta2(b2);
      } else {
        a = h[k];
        b = beta_from_beta2(h[(size_t)nlanc + k]);
      }
      alanc[k] = a;
      if (!(fabs(b) > 0.0) || fabs(b) < threshold) {
        ndone = k + 1;
        break;
      }
      if (k + 1 < nlanc) blanc[k + 1] = b;
    }
    if (redo) {
      std::fill(alanc, alanc + nlanc, 0.0);
      std::fill(blanc, blanc + nlanc, 0.0);
      continue;
    }
    if (niter_done) *niter_done = ndone;
    return 0;
  }
  set_error("edigpu_lanczos_tridiag_sharded: internal error");
  return 1;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_shard_plan(int64_t units, int32_t world, int32_t rank, int64_t* first, int64_t* count, int64_t* q) {
  if (units < 0 || world < 1 || rank < 0 || rank >= world) {
    set_error("edigpu_shard_plan: bad argument");
    return 1;
  }
  const int64_t qq = (units + world - 1) / world;
  const int64_t f = std::min<int64_t>((int64_t)rank * qq, units);
  if (first) *first = f;
  if (count) *count = std::max<int64_t>(0, std::min<int64_t>(qq, units - f));
  if (q) *q = qq;
  return 0;
}

// Host-only (no GPU is touched): the index arithmetic of the transposed exchange as the kernels use it
// (exchange_index.hpp), for hosts that stage the exchange themselves and for the CPU suite.
int edigpu_exchange_send_map(int64_t dim_up, int64_t nrows, int64_t q, int32_t world, int64_t pcol, int32_t halo, int64_t* src) {
  if (!src || dim_up < 1 || nrows < 0 || q < nrows || world < 1 || pcol < 1 || halo < 0) {
    set_error("edigpu_exchange_send_map: bad argument");
    return 1;
  }
  const int64_t n = (int64_t)world * q * (pcol + 2 * halo);
  for (int64_t e = 0; e < n; e++) src[e] = xch_send_source(e, dim_up, nrows, q, pcol, halo);
  return 0;
}

int edigpu_exchange_back_map(int64_t dim_up, int64_t nrows, int64_t q, int32_t world, int64_t pcol, int32_t halo, int64_t* slot) {
  if (!slot || dim_up < 1 || nrows < 0 || q < nrows || world < 1 || pcol < 1 || halo < 0 || pcol * world < dim_up) {
    set_error("edigpu_exchange_back_map: bad argument");
    return 1;
  }
  for (int64_t i = 0; i < nrows; i++)
    for (int64_t col = 0; col < dim_up; col++) slot[i * dim_up + col] = xch_back_slot(i, col, q, pcol, halo);
  return 0;
}

// (Nloc, v, Hv) on shards with host vectors: the contract of spMatVec_mpi_* / directMatVec_MPI_*
static int apply_sharded(edigpu_handle s, edigpu_comm c, int64_t nloc, const double* v, double* hv, int cplx) {
  if (!s || !c || (nloc > 0 && (!v || !hv))) {
    set_error("edigpu_apply_sharded: NULL argument");
    return 1;
  }
  if ((s->is_complex != 0) != (cplx != 0)) {
    set_error("edigpu_apply_sharded: real/complex mismatch between handle and entry point");
    return 1;
  }
  if (real_image(s) != s) {  // the transposed exchange serves complex sectors as well
    s = real_image(s);
    nloc *= 2;
  }
  ShardGeom g;
  if (shard_geometry(s, c, g)) return 1;
  if (nloc != g.nloc) {
    set_error("edigpu_apply_sharded: Nloc does not match this rank's shard (edigpu_shard_plan)");
    return 1;
  }
  EDIGPU_HIP(hipSetDevice(s->device));
  if (comm_workspace(c, g, 1)) return 1;
  hipStream_t st = s->stream;
  const int64_t n = g.nloc * g.w;
  if (zero_chunk(c->ws.vin, g, st)) return 1;
  if (n > 0) EDIGPU_HIP(hipMemcpyAsync(c->ws.vin, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
  if (sharded_product(s, c, g, st, c->ws.vin, c->ws.tmp)) return 1;
  if (n > 0) EDIGPU_HIP(hipMemcpyAsync(hv, c->ws.tmp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  return 0;
}

int edigpu_apply_sharded_d(edigpu_handle h, edigpu_comm c, int64_t nloc, const double* v_shard_host, double* hv_shard_host) {
  return apply_sharded(h, c, nloc, v_shard_host, hv_shard_host, 0);
}

int edigpu_apply_sharded_z(edigpu_handle h, edigpu_comm c, int64_t nloc, const double* v_shard_host, double* hv_shard_host) {
  return apply_sharded(h, c, nloc, v_shard_host, hv_shard_host, 1);
}

int edigpu_lanczos_tridiag_sharded(edigpu_handle h, edigpu_comm c, const double* vin_shard, int nlanc, double* alanc,
                                   double* blanc, double threshold, int* niter_done, double* norm2) {
  if (!h || !c || !alanc || !blanc || nlanc < 1) {
    set_error("edigpu_lanczos_tridiag_sharded: bad argument");
    return 1;
  }
  // a world of one rank holding the whole sector: the fused single-GPU recurrence (half the vector traffic of the
  // exchange form: no send / receive buffers); CommSwitches::force_collectives keeps the N > 1 code path (tests)
  h = real_image(h);
  if (c->world == 1 && h->is_whole() && !c->sw.force_collectives && vin_shard)
    return edigpu_lanczos_tridiag_dev(h, vin_shard, nlanc, alanc, blanc, threshold, niter_done, norm2);
  return sharded_tridiag(h, c, vin_shard, nlanc, alanc, blanc, threshold, niter_done, norm2);
}

// sp_eigh(MpiComm, spHtimesV_p, eval, evec, ...) / sp_lanc_eigh(MpiComm, ...) with every vector a device-resident shard
// (ED_NORMAL/ED_DIAG_NORMAL.f90:179-214 and the superc / nonsu2 twins): the thick-restart driver of the single-GPU
// solver (trl_solve, edigpu_trl.hip) on this rank's elements, the product through the sharded exchange, the Gram-
// Schmidt coefficients and norms through small all-reduces.  Nothing of vector length crosses PCIe.
int edigpu_lanczos_eigh_multi_sharded(edigpu_handle h, edigpu_comm c, int neigen, int ncv, double tol, int maxrestart,
                                      const double* v0_shard, double* evals, double* evecs_shard, int* nconv, int* nmatvec) {
  if (!h || !c || !evals || neigen <= 0) {
    set_error("edigpu_lanczos_eigh_multi_sharded: bad argument");
    return 1;
  }
  // complex normal sector: the products run on its doubled real sector, whose real vectors ARE the interleaved complex
  // ones -- the solver keeps the complex algebra
  const bool realified = real_image(h) != h;
  h = real_image(h);
  // a world of one rank holding the whole sector: the single-GPU solver (no exchange buffers)
  if (c->world == 1 && h->is_whole() && !c->sw.force_collectives && !realified)
    return edigpu_lanczos_eigh_multi(h, neigen, ncv, tol, maxrestart, v0_shard, evals, evecs_shard, nconv, nmatvec);
  ShardGeom g;
  if (shard_geometry(h, c, g)) return 1;
  EDIGPU_HIP(hipSetDevice(h->device));
  if (comm_workspace(c, g, 8)) return 1;
  hipStream_t st = h->stream;
  const int64_t len = g.nloc * g.w;
  const int cplx = (g.w == 2 || realified) ? 1 : 0;
  const int64_t n = cplx && g.w == 1 ? g.nloc / 2 : g.nloc;
  const int64_t nglobal = (cplx && g.w == 1 ? h->dim / 2 : h->dim);
  // the padded tail of the exchange buffers stays zero for the whole solve
  if (zero_chunk(c->ws.vin, g, st) || zero_chunk(c->ws.tmp, g, st)) return 1;
  TrlOps ops;
  ops.apply = [&](const double* in, double* out, hipStream_t s2) -> int { return sharded_product(h, c, g, s2, in, out); };
  ops.allreduce = [&](double* dev, size_t cnt, hipStream_t s2) -> int { return comm_all_reduce(c, dev, cnt, s2); };
  return trl_solve(h->device, st, cplx, n, len, nglobal, ops, neigen, ncv, tol, maxrestart, v0_shard, (uint64_t)c->rank * 7919u,
                   evals, evecs_shard, nconv, nmatvec);
}

// lanc_method = "lanczos" (sp_lanc_eigh with MpiComm: the lowest pair): the same driver asked for one pair, its basis
// sized by nitermax (at most 128 vectors before a restart)
int edigpu_lanczos_eigh_sharded(edigpu_handle h, edigpu_comm c, int nitermax, double tol, const double* v0_shard, double* eval,
                                double* evec_shard, int* nmatvec) {
  if (!eval || nitermax <= 0) {
    set_error("edigpu_lanczos_eigh_sharded: bad argument");
    return 1;
  }
  int nconv = 0;
  const int ncv = std::max(8, std::min(nitermax, 48));
  const int maxrestart = std::max(1, nitermax / std::max(1, ncv / 2));
  return edigpu_lanczos_eigh_multi_sharded(h, c, 1, ncv, tol, maxrestart, v0_shard, eval, evec_shard, &nconv, nmatvec);
}

// bench.py --gpus N: what the transport itself reports and costs.  *rccl_ranks = ncclCommCount of the communicator (0:
// shared-memory transport, -1: RCCL without that symbol) -- the driver's scaling record can then show that RCCL saw N
// ranks; *ms_exchange = average time of the collectives of ONE product + step (the two all-to-alls or the all-gather, and
// the 3-double all-reduce) with nothing else running, HIP events on the communicator's stream.
int edigpu_exchange_bench(edigpu_handle s, edigpu_comm c, int steps, int32_t* rccl_ranks, double* ms_exchange) {
  if (!s || !c || steps < 1) {
    set_error("edigpu_exchange_bench: bad argument");
    return 1;
  }
  s = real_image(s);
  if (rccl_ranks) *rccl_ranks = comm_rccl_ranks(c);
  if (!ms_exchange) return 0;
  ShardGeom g;
  if (shard_geometry(s, c, g)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (comm_workspace(c, g, 8)) return 1;
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  auto once = [&]() -> int {
    for (int b = 0; b < g.nblk; b++) {
      if (g.transposed) {
        if (comm_all_to_all(c, c->ws.send, c->ws.recv, (size_t)(g.q * g.pw), c->side)) return 1;
        if (comm_all_to_all(c, c->ws.hvc, c->ws.back, (size_t)(g.q * g.pw), c->side)) return 1;
      } else {
        const size_t n = g.nblk > 1 ? (size_t)g.q * g.unit_len * g.w : (size_t)g.chunk * g.w;
        if (comm_all_gather(c, c->ws.vin, c->ws.vfull, n, c->side)) return 1;
      }
    }
    return comm_all_reduce(c, c->ws.scr, 3, c->side);
  };
  for (int k = 0; k < 2 && !rc; k++) rc |= once();
  rc |= (hipEventRecord(e0, c->side) != hipSuccess);
  for (int k = 0; k < steps && !rc; k++) rc |= once();
  rc |= (hipEventRecord(e1, c->side) != hipSuccess);
  rc |= (hipEventSynchronize(e1) != hipSuccess);
  float ms = 0.f;
  if (!rc) rc |= (hipEventElapsedTime(&ms, e0, e1) != hipSuccess);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    set_error("edigpu_exchange_bench: failed");
    return 1;
  }
  *ms_exchange = (double)ms / steps;
  return 0;
}

int edigpu_lanczos_bench_sharded(edigpu_handle s, edigpu_comm c, int warmup, int steps, double* ms_per_step,
                                 int64_t* exchange_bytes) {
  if (!s || !c || steps < 1 || warmup < 0 || !ms_per_step) {
    set_error("edigpu_lanczos_bench_sharded: bad argument");
    return 1;
  }
  s = real_image(s);
  ShardGeom g;
  if (shard_geometry(s, c, g)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  const int total = warmup + steps;
  if (comm_workspace(c, g, total)) return 1;
  hipStream_t st = s->stream;
  EDIGPU_HIP(hipMemsetAsync(c->ws.hist, 0, (size_t)c->ws.hist_cap * sizeof(double), st));
  // seeded random start vector of this shard
  const int64_t n = g.nloc * g.w;
  if (zero_chunk(c->ws.tmp, g, st)) return 1;
  if (n > 0 && lz_fill_random(c->ws.tmp, n, 12345ull + (uint64_t)c->rank, st)) return 1;
  if (load_seed(c, g, c->ws.tmp, st)) return 1;
  const bool panels = panel_loop(g);
  if (panels && panel_loop_begin(s, c, g, st)) return 1;
  auto step = [&](int it) -> int { return panels ? sharded_step_panels(s, c, g, it, st) : sharded_step(s, c, g, it, st); };
  for (int it = 0; it < warmup; it++)
    if (step(it)) return 1;
  if (comm_all_reduce(c, c->ws.scr + 2, 1, st)) return 1;  // barrier
  EDIGPU_HIP(hipStreamSynchronize(st));
  const auto t0 = std::chrono::steady_clock::now();
  for (int it = warmup; it < total; it++)
    if (step(it)) return 1;
  EDIGPU_HIP(hipStreamSynchronize(st));
  if (comm_all_reduce(c, c->ws.scr + 2, 1, st)) return 1;
  EDIGPU_HIP(hipStreamSynchronize(st));
  const auto t1 = std::chrono::steady_clock::now();
  *ms_per_step = std::chrono::duration<double, std::milli>(t1 - t0).count() / steps;
  if (exchange_bytes)
    *exchange_bytes = g.block        ? 2 * 8 * (int64_t)(c->world - 1) * g.npmax * g.q * 16
                      : g.transposed ? 2 * 8 * (int64_t)(c->world - 1) * g.q * g.pw * g.nblk
                                     : 8 * g.chunk * g.w * (int64_t)(c->world - 1);
  return 0;
}

int edigpu_shard_info(edigpu_handle s, edigpu_comm c, int32_t info[4]) {
  if (!s || !c || !info) {
    set_error("edigpu_shard_info: bad argument");
    return 1;
  }
  s = real_image(s);
  ShardGeom g;
  if (shard_geometry(s, c, g)) return 1;
  info[0] = g.block ? 2 : g.transposed ? 1 : 0;
  info[1] = (int32_t)g.q;
  info[2] = g.block ? g.npmax : (int32_t)g.pcol;
  info[3] = g.block ? 0 : g.halo;
  return 0;
}

}  // extern "C"
