// edigpu_lanczos.hip -- the device-resident Lanczos recurrence of a handle: one step, the set-up of a run, the replay of
// captured steps, and the entry points edigpu_lanczos_tridiag(_dev) and edigpu_lanczos_eigh on top of them.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dev_mem.hpp"
#include "host_dense.hpp"
#include "host_ib.hpp"
#include "kernels.hpp"

namespace edigpu {

// enqueue one Lanczos step (iter is 0-based); vin/vout/tmp live in the workspace
bool flat_lanczos_fusable(const edigpu_sector* s) {
  if (s->sw.lanczos_unfused || !s->is_whole() || s->nloc == 0 || s->has_phonons()) return false;
  if (s->kind == kDirect) return true;
  return s->kind == kFlat && csr_lanczos_fusable(s->loc) && s->nonloc.nnz == 0;
}

// iter < 0: a later step (not the first) whose index the finalize kernel takes from the device-side counter -- the form
// that can be captured once and replayed (lanczos_run)
int lanczos_step(edigpu_sector* s, int iter, int nlanc, hipStream_t st) {
  const int64_t len = s->lz_len;
  const bool later = iter != 0;
  // (impurity-block image with rows staged in halves: rows_per_block == 0, but launch_ib_lanczos has a step for it)
  const bool ib_split = s->kind == kNormal && s->ib && s->ib->nhalf == 2 && s->lz_blocked;
  if (normal_lanczos_fusable(s) || ib_split) {
    // rotate (and the pending axpy) fused into the row kernel, alpha and <Q|Q> into the panel sweep
    // (kernels_normal.hip); LoopSwitches::lanczos_exactbeta keeps the separate axpy+norm kernel
    const bool exactbeta = s->lz.lanczos_exactbeta;
    int np = 0;
    bool finalized = false;
    bool in_x = false;
    if (launch_normal_lanczos(s, s->d_vin, s->d_vout, s->d_scal, s->d_partial, s->partial_cap, iter == 0, !exactbeta, st, &np,
                              nlanc, &finalized, s->d_tmp, &in_x))
      return 1;
    if (in_x) std::swap(s->d_vin, s->d_tmp);  // the new Lanczos vector was written to the third buffer
    if (finalized) return 0;  // the sweep's last workgroup wrote alpha, beta and the stop flag
    if (exactbeta) {
      if (lz_finalize_alpha(s->d_partial, np, s->d_scal, iter, nlanc, st)) return 1;
      return lz_beta(s->d_vin, s->d_vout, len, s->d_partial, s->d_scal, iter, nlanc, st);
    }
    return lz_finalize_alpha_beta(s->d_vin, s->d_vout, len, s->d_partial, np, s->d_scal, iter, nlanc, st);
  }
  if (flat_lanczos_fusable(s)) {
    // flat / direct sectors held whole on this GPU: rotate with the pending axpy, then Q += H*v with
    // the alpha and <Q|Q> partials in the product's epilogue (no tmp vector, no separate dot kernels)
    int np = 0;
    if (later && lz_rotate_lazy(s->d_vin, s->d_vout, len, s->d_scal, st)) return 1;
    if (s->kind == kDirect) {
      if (launch_direct_lanczos(s, s->d_vin, s->d_vout, s->d_partial, s->partial_cap, &np, s->d_scal + SC_ALPHA, st)) return 1;
    } else if (launch_csr_lanczos(s->loc, s->is_complex, s->d_vin, s->d_vout, s->d_partial, s->partial_cap, &np, s->d_scal + SC_ALPHA, st)) {
      return 1;
    }
    return lz_finalize_alpha_beta(s->d_vin, s->d_vout, len, s->d_partial, np, s->d_scal, iter, nlanc, st);
  }
  // no fused product (ed_total_ud = F, phonon branches, complex normal mode, rows staged in column parts, shards): the
  // product goes to its own buffer; the one-reduction recurrence around it -- lazy rotate with the pending axpy, Q += H P
  // with the three sums, one finalize -- moves 8 vector passes per step where the literal form moves 11.  The three-sum
  // beta (k_finalize_ab) is what makes this safe: with beta^2 = <w|w> - alpha^2 the same loop made the lowest Ritz value
  // jitter at 6e-14 |H| (round 1, removed then).  LoopSwitches::lanczos_exactbeta / Switches::lanczos_unfused: the literal form.
  auto product = [&]() -> int {  // tmp <- H vin, in the layout lanczos_prepare chose
    return s->lz_blocked ? launch_normal_blocked(s, s->d_vin, s->d_tmp, st) : apply_any(s, s->d_vin, s->d_vin, s->d_tmp, 3, st);
  };
  if (s->sw.lanczos_unfused || s->lz.lanczos_exactbeta) {
    if (iter > 0 && lz_rotate(s->d_vin, s->d_vout, len, s->d_scal, st)) return 1;
    if (product()) return 1;
    if (lz_alpha(s->d_vin, s->d_vout, s->d_tmp, len, s->d_partial, s->d_scal, iter, nlanc, st)) return 1;
    return lz_beta(s->d_vin, s->d_vout, len, s->d_partial, s->d_scal, iter, nlanc, st);
  }
  int np = 0;
  if (later && lz_rotate_lazy(s->d_vin, s->d_vout, len, s->d_scal, st)) return 1;
  if (product()) return 1;
  if (lz_add_dot3(s->d_vin, s->d_vout, s->d_tmp, len, s->d_scal, s->d_partial, &np, st)) return 1;
  return lz_finalize_alpha_beta(s->d_vin, s->d_vout, len, s->d_partial, np, s->d_scal, iter, nlanc, st);
}

int lanczos_prepare(edigpu_sector* s, int nlanc, double threshold, hipStream_t st) {
  s->lz = LoopSwitches::sample();
  // the recurrence of a large factored normal-mode sector runs on panel-major vectors (set-up decides, blk_shift)
  // (the impurity-block image with rows staged in halves: rows_per_block == 0 there, its step is in launch_ib_lanczos)
  const bool ib_whole = s->kind == kNormal && s->ib && s->nph == 0 && s->is_whole() && !s->sw.lanczos_unfused;
  s->lz_blocked = s->kind == kNormal && (s->blk_shift > 0 || s->ib) && s->nph == 0 &&
                  (normal_lanczos_fusable(s) || (ib_whole && s->ib->nhalf == 2));
  s->lz_len = s->lz_blocked ? (s->ib ? s->ib->len : s->blk_len) : s->ws_len;
  const size_t ns = (size_t)SC_AB + 2 * (size_t)nlanc;
  if (!s->d_scal || s->scal_cap < ns) {  // (kept across runs: a captured graph holds its address)
    dev_free(s->d_scal);
    s->scal_cap = 0;
    EDIGPU_HIP(hipMalloc((void**)&s->d_scal, ns * sizeof(double)));
    s->scal_cap = ns;
  }
  EDIGPU_HIP(hipMemsetAsync(s->d_scal, 0, ns * sizeof(double), st));
  if (!s->d_lzcnt) EDIGPU_HIP(hipMalloc((void**)&s->d_lzcnt, 64));
  EDIGPU_HIP(hipMemsetAsync(s->d_lzcnt, 0, 64, st));
  EDIGPU_HIP(hipMemcpyAsync(s->d_scal + SC_THR, &threshold, sizeof(double), hipMemcpyHostToDevice, st));
  EDIGPU_HIP(hipMemsetAsync(s->d_vout, 0, (size_t)s->lz_len * sizeof(double), st));
  return 0;
}

// start vector of a recurrence into d_vin, in the layout lanczos_prepare chose: src = host or device vector in the
// natural layout (ws_len doubles), or nullptr for seeded random numbers
int lanczos_seed(edigpu_sector* s, const double* src, uint64_t seed, hipStream_t st) {
  double* dst = s->lz_blocked ? s->d_tmp : s->d_vin;
  if (src) {
    EDIGPU_HIP(hipMemcpyAsync(dst, src, (size_t)s->ws_len * sizeof(double), hipMemcpyDefault, st));
  } else if (lz_fill_random(dst, s->ws_len, seed, st)) {
    return 1;
  }
  if (s->lz_blocked && s->ib) {
    if (vec_to_ib(s->ib, s->d_tmp, s->d_vin, st)) return 1;
    if (s->ib->ps != s->ib->dim_dw * kIbPanel) {
      // padded panel stride (Switches::ib_pspad): the doubles between two panels are written by no kernel and enter the vector
      // sums; the two other buffers may hold anything there (d_tmp just held the vector in the reference's layout)
      EDIGPU_HIP(hipMemsetAsync(s->d_tmp, 0, (size_t)s->ib->len * sizeof(double), st));
      EDIGPU_HIP(hipMemsetAsync(s->d_vout, 0, (size_t)s->ib->len * sizeof(double), st));
    }
    return 0;
  }
  if (s->lz_blocked) return vec_to_blocked(s->d_tmp, s->d_vin, s->dim_up, s->dim_dw, s->blk_shift, st);
  return 0;
}

// Steps [from, to) of the current recurrence.  Switches::lanczos_graph: the later steps of a small sector -- identical
// launches once the step index lives on the device (k_finalize_ab, iter < 0) -- are captured once as a hipGraph of
// kGraphSteps steps and replayed; the executable stays with the handle for the next run of the same length.
// OPT-IN because it buys nothing here: measured on configs 1 / 3 / 4 (10.9 / 20.3 / 23.8 us per step with the graph,
// 11.4 / 20.4 / 23.1 without), i.e. the three dependent kernels of a step are bound by their own dispatch-to-completion
// latency on the device, not by host-side launch cost; fusing the finalize into the sweep's last workgroup is what would
// shorten a small sector's step.
int lanczos_run(edigpu_sector* s, int from, int to, int nlanc, hipStream_t st) {
  constexpr int kGraphSteps = 8;
  int it = from;
  if (it == 0 && it < to) {
    if (lanczos_step(s, 0, nlanc, st)) return 1;
    it = 1;
  }
  const bool eligible = s->sw.lanczos_graph && !s->sw.lanczos_unfused && !s->lz.lanczos_exactbeta && !s->lz_graph_failed &&
                        s->nloc <= s->sw.lanczos_graph_max &&
                        s->nph == 0 && s->kind != kCmplxNormal && to - it >= kGraphSteps + (s->lz_graph ? 0 : 1);
  if (eligible) {
    if (s->lz_graph && (s->lz_graph_nlanc != nlanc || s->lz_graph_scal != s->d_scal || s->lz_graph_blocked != s->lz_blocked)) {
      (void)hipGraphExecDestroy(s->lz_graph);
      s->lz_graph = nullptr;
    }
    if (!s->lz_graph) {
      // one uncaptured later step first: whatever the launchers set up lazily (function attributes, occupancy
      // queries) happens outside the capture
      if (lanczos_step(s, it, nlanc, st)) return 1;
      it++;
      hipGraph_t g = nullptr;
      bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
      for (int k = 0; ok && k < kGraphSteps; k++) ok = lanczos_step(s, -1, nlanc, st) == 0;
      if (hipStreamEndCapture(st, &g) != hipSuccess) ok = false;
      if (ok && g && hipGraphInstantiate(&s->lz_graph, g, nullptr, nullptr, 0) != hipSuccess) {
        s->lz_graph = nullptr;
        ok = false;
      }
      if (g) (void)hipGraphDestroy(g);
      if (!ok) {
        (void)hipGetLastError();
        s->lz_graph = nullptr;
        s->lz_graph_failed = true;  // plain launches from here on (the capture enqueued nothing)
      } else {
        s->lz_graph_k = kGraphSteps;
        s->lz_graph_nlanc = nlanc;
        s->lz_graph_scal = s->d_scal;
        s->lz_graph_blocked = s->lz_blocked;
      }
    }
    while (s->lz_graph && to - it >= s->lz_graph_k) {
      EDIGPU_HIP(hipGraphLaunch(s->lz_graph, st));
      it += s->lz_graph_k;
    }
  }
  for (; it < to; it++)
    if (lanczos_step(s, it, nlanc, st)) return 1;
  return 0;
}

// a vector of the current recurrence (device, lz_len doubles) to a host or device buffer in the natural layout
int lanczos_fetch(edigpu_sector* s, const double* v, double* dst, hipStream_t st) {
  if (s->lz_blocked) {
    if (s->ib ? vec_from_ib(s->ib, v, s->d_tmp, st) : vec_from_blocked(v, s->d_tmp, s->dim_up, s->dim_dw, s->blk_shift, st)) return 1;
    v = s->d_tmp;
  }
  EDIGPU_HIP(hipMemcpyAsync(dst, v, (size_t)s->ws_len * sizeof(double), hipMemcpyDefault, st));
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

// seed from host or device memory (hipMemcpyDefault); norm2 = <vin|vin> as tridiag_Hv_sector_* returns it
static int tridiag_impl(edigpu_handle s, const double* vin, int nlanc, double* alanc, double* blanc,
                        double threshold, int* niter_done, double* norm2) {
  if (!s || !vin || !alanc || !blanc || nlanc <= 0) {
    set_error("edigpu_lanczos_tridiag: bad argument");
    return 1;
  }
  if (single_shard(s, "edigpu_lanczos_tridiag")) return 1;
  // _CMPLX_NORMAL held as one real sector on the doubled up index: complex Lanczos on H = real Lanczos on that sector
  // with the interleaved vector read as real (alpha = <v|H|v> is real, beta a norm), so the fused real loop does it
  if (s->kind == kCmplxNormal && s->sub_d) return tridiag_impl(s->sub_d, vin, nlanc, alanc, blanc, threshold, niter_done, norm2);
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ensure_workspace(s)) return 1;
  hipStream_t st = s->stream;
  if (lanczos_prepare(s, nlanc, threshold, st)) return 1;
  if (lanczos_seed(s, vin, 0, st)) return 1;
  if (lz_norm_begin(s->d_vin, s->lz_len, s->d_partial, s->d_scal, st)) return 1;
  if (lanczos_run(s, 0, nlanc, nlanc, st)) return 1;
  std::vector<double> sc((size_t)SC_AB + 2 * (size_t)nlanc);
  EDIGPU_HIP(hipMemcpyAsync(sc.data(), s->d_scal, sc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  if (!(sc[SC_NORM] > 0.0)) {  // zero seed: nothing to tridiagonalise (the reference skips such channels)
    std::fill(alanc, alanc + nlanc, 0.0);
    std::fill(blanc, blanc + nlanc, 0.0);
    if (niter_done) *niter_done = 0;
    if (norm2) *norm2 = 0.0;
    return 0;
  }
  for (int k = 0; k < nlanc; k++) {
    alanc[k] = sc[SC_AB + k];
    blanc[k] = sc[SC_AB + nlanc + k];
  }
  if (niter_done) *niter_done = (int)sc[SC_NDONE];
  if (norm2) *norm2 = sc[SC_NORM] * sc[SC_NORM];
  return 0;
}

int edigpu_lanczos_tridiag(edigpu_handle s, const double* vin_host, int nlanc, double* alanc,
                           double* blanc, double threshold, int* niter_done) {
  return tridiag_impl(s, vin_host, nlanc, alanc, blanc, threshold, niter_done, nullptr);
}

int edigpu_lanczos_tridiag_dev(edigpu_handle s, const double* vin_dev, int nlanc, double* alanc,
                               double* blanc, double threshold, int* niter_done, double* norm2) {
  return tridiag_impl(s, vin_dev, nlanc, alanc, blanc, threshold, niter_done, norm2);
}

int edigpu_lanczos_eigh(edigpu_handle s, int nitermax, double tol, int check_every,
                        const double* v0_host, double* eval, double* evec_host, int* niter_done) {
  if (!s || !eval || nitermax <= 0) {
    set_error("edigpu_lanczos_eigh: bad argument");
    return 1;
  }
  if (single_shard(s, "edigpu_lanczos_eigh")) return 1;
  if (s->kind == kCmplxNormal && s->sub_d)  // see tridiag_impl: the Ritz vector comes back interleaved, i.e. complex
    return edigpu_lanczos_eigh(s->sub_d, nitermax, tol, check_every, v0_host, eval, evec_host, niter_done);
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ensure_workspace(s)) return 1;
  if (check_every <= 0) check_every = 10;
  if ((int64_t)nitermax > s->nloc) nitermax = (int)s->nloc;
  hipStream_t st = s->stream;
  // breakdown guard: a beta below 1e-12 means the Krylov space is exhausted (tiny sectors with nitermax ~ dim); the
  // recurrence stops there instead of dividing by it
  constexpr double kBreakdown = 1e-12;
  if (lanczos_prepare(s, nitermax, kBreakdown, st)) return 1;
  const int64_t len = s->lz_len;
  const size_t vbytes = (size_t)len * sizeof(double);
  // keep the normalised start vector for the second pass
  double* d_v0 = nullptr;
  EDIGPU_HIP(hipMalloc((void**)&d_v0, vbytes));
  auto fail = [&](void) {
    (void)hipFree(d_v0);
    return 1;
  };
  if (lanczos_seed(s, v0_host, 0x5eed1234ull, st)) return fail();
  if (lz_norm_begin(s->d_vin, len, s->d_partial, s->d_scal, st)) return fail();
  if (hipMemcpyAsync(d_v0, s->d_vin, vbytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail();

  std::vector<double> sc((size_t)SC_AB + 2 * (size_t)nitermax), d, e, z;
  double e_old = 0.0;
  int ndone = 0;
  bool have = false, conv = false;
  // With a vector asked for, the Lanczos vectors are kept as they are produced (blocks of kKeep vectors, allocated
  // while the device has room: 288 GB hold thousands of config-2 vectors) and the Ritz vector is assembled from them --
  // one extra copy per step instead of a second pass that regenerates every v_k with as many products again.
  // LoopSwitches::eigh_twopass, or an allocation that fails, falls back to the second pass.
  constexpr int kKeep = 16;
  std::vector<double*> kept;  // block b holds v_(b kKeep) .. v_(b kKeep + kKeep - 1)
  bool keep = evec_host != nullptr && !s->lz.eigh_twopass;  // (sampled by lanczos_prepare above)
  auto drop_kept = [&]() {
    for (double* b : kept) (void)hipFree(b);
    kept.clear();
    keep = false;
  };
  auto fail_all = [&]() {
    drop_kept();
    return fail();
  };
  for (int it0 = 0; it0 < nitermax && !conv;) {
    // the steps up to the next convergence check in one go (replayed from a graph on launch-bound sectors)
    const int it1 = std::min(nitermax, (it0 / check_every + 1) * check_every);
    if (keep) {
      for (int it = it0; it < it1 && keep; it++) {
        if (it % kKeep == 0) {
          size_t fr = 0, tot = 0;
          double* b = nullptr;
          // leave a quarter of the device free for whatever else lives there
          if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < tot / 4 + (size_t)kKeep * vbytes ||
              hipMalloc((void**)&b, (size_t)kKeep * vbytes) != hipSuccess) {
            (void)hipGetLastError();
            drop_kept();
            break;
          }
          kept.push_back(b);
        }
        if (lanczos_step(s, it, nitermax, st)) return fail_all();
        if (hipMemcpyAsync(kept[(size_t)(it / kKeep)] + (size_t)(it % kKeep) * (size_t)len, s->d_vin, vbytes,
                           hipMemcpyDeviceToDevice, st) != hipSuccess)
          return fail_all();
        it0 = it + 1;
      }
      if (it0 < it1 && lanczos_run(s, it0, it1, nitermax, st)) return fail_all();  // (room ran out part way)
    } else if (lanczos_run(s, it0, it1, nitermax, st)) {
      return fail_all();
    }
    it0 = it1;
    {
      if (hipMemcpyAsync(sc.data(), s->d_scal, sc.size() * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess)
        return fail_all();
      if (hipStreamSynchronize(st) != hipSuccess) return fail_all();
      ndone = (int)sc[SC_NDONE];
      if (ndone == 0) break;
      d.assign(sc.begin() + SC_AB, sc.begin() + SC_AB + ndone);
      e.assign(sc.begin() + SC_AB + nitermax, sc.begin() + SC_AB + nitermax + ndone);
      if (tql2(ndone, d, e, z)) {
        set_error("edigpu_lanczos_eigh: tridiagonal QL did not converge");
        return fail_all();
      }
      const double e_new = *std::min_element(d.begin(), d.end());
      if (have && fabs(e_new - e_old) < tol) conv = true;
      if (sc[SC_STOP] != 0.0) conv = true;  // invariant subspace reached
      e_old = e_new;
      have = true;
    }
  }
  if (ndone == 0) {
    set_error("edigpu_lanczos_eigh: zero start vector");
    return fail_all();
  }
  *eval = e_old;
  if (niter_done) *niter_done = ndone;
  if (evec_host) {
    // Ritz vector = sum_k y_k v_k : regenerate the v_k with the same (deterministic) kernels
    const int kmin = (int)(std::min_element(d.begin(), d.end()) - d.begin());
    std::vector<double> y(ndone);
    for (int k = 0; k < ndone; k++) y[k] = z[(size_t)kmin * ndone + k];
    double* d_acc = nullptr;
    if (hipMalloc((void**)&d_acc, vbytes) != hipSuccess) {
      set_error("edigpu_lanczos_eigh: out of device memory");
      return fail_all();
    }
    (void)hipMemsetAsync(d_acc, 0, vbytes, st);
    int rc = 0;
    if (keep && (int)kept.size() * kKeep >= ndone) {
      for (int it = 0; it < ndone && !rc; it++)
        rc |= lz_axpy_coef(d_acc, kept[(size_t)(it / kKeep)] + (size_t)(it % kKeep) * (size_t)len, len, y[it], s->d_scal, -1, st);
    } else {
      (void)hipMemcpyAsync(s->d_vin, d_v0, vbytes, hipMemcpyDeviceToDevice, st);
      if (lanczos_prepare(s, ndone, kBreakdown, st)) {
        (void)hipFree(d_acc);
        return fail_all();
      }
      for (int it = 0; it < ndone && !rc; it++) {
        // same kernels, same order as the first pass => bitwise the same Lanczos vectors
        rc |= lanczos_step(s, it, ndone, st);
        rc |= lz_axpy_coef(d_acc, s->d_vin, len, y[it], s->d_scal, -1, st);
      }
    }
    // normalise
    if (!rc) rc |= lz_norm_begin(d_acc, len, s->d_partial, s->d_scal, st);
    if (!rc) rc |= lanczos_fetch(s, d_acc, evec_host, st);
    if (hipStreamSynchronize(st) != hipSuccess) rc = 1;
    (void)hipFree(d_acc);
    if (rc) {
      if (!have_error()) set_error("edigpu_lanczos_eigh: second pass failed");
      return fail_all();
    }
  }
  drop_kept();
  (void)hipFree(d_v0);
  return 0;
}

}  // extern "C"
