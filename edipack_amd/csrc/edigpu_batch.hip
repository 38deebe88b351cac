// edigpu_batch.hip -- C ABI of the multi-vector product and of the batched tridiagonalisation (include/edigpu.h:
// edigpu_apply_multi_dev, edigpu_lanczos_tridiag_batch_dev): checks, the route, the handle's interleaved workspace and
// the lock-step loop over kernels_multi.hip.
//
// The recurrence is the single-seed one of flat_lanczos_fusable sectors (edigpu_lanczos.hip: lanczos_step) run on W
// columns at once: norms and scaling, then per step rotate (later steps) -> Q += H P with the three partial sums per
// column -> finalize per column.  Nothing waits for the host until the last step is enqueued; a column that stops is
// held at zero by the kernels, so the host never looks at the stop flags.
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "kernels.hpp"

namespace edigpu {

void free_batch(edigpu_sector* s) {
  if (!s || !s->batch) return;
  BatchDev* b = s->batch;
  dev_free_all(b->P, b->Q, b->partial, b->scal);
  delete b;
  s->batch = nullptr;
}

// the sectors whose product has a multi-vector kernel: a whole flat sector on this GPU without phonons, stored with the
// SELL image or on the fly
// Size bands of widest_kept, in rows (measurements: DESIGN.md 6).  Stored: W = 8 is the fastest at 924 rows and level with
// W = 4 at 12 870 (5.64 against 5.56 us per seed and step, inside the spread), W = 4 the fastest at 184 756, W = 2 at
// 2.7 M.  On the fly: W = 4 is the fastest at 3 432 and 48 620 rows, W = 2 at 705 432 and 10.4 M.  On the fly W = 8 was
// the fastest at no measured size; it is kept up to 4 000 rows only, where a call of 5 to 8 seeds is specified to run as
// one group (tests/test_gpu_tridiag_batch.py, route 8 on 252 and 3 432 rows) and still takes less than half the
// single-seed time (14.4 against 31.9 us; two groups of 4 would take 10.6).
constexpr int64_t kSellW8Rows = 13000, kSellW4Rows = 200000, kDirW8Rows = 4000, kDirW4Rows = 50000;

static bool multi_sector(const edigpu_sector* s) {
  if (!s->is_whole() || s->nloc == 0 || s->has_phonons()) return false;
  if (s->kind == kDirect) return true;
  return s->kind == kFlat && csr_lanczos_fusable(s->loc) && s->nonloc.nnz == 0;
}

// The widest interleaved group a sector takes: per kind and size band the width that was measured FASTEST per seed and
// step (scripts/time_tridiag_batch.py with --force-width; table in DESIGN.md 6), and only where it beats the single-seed
// call by more than the run-to-run spread.  W = 2 won at every size measured, stored and on the fly.  W = 4 and 8 win
// while the step is bound by its launches and the W interleaved vectors stay in cache, and lose on large sectors, where
// an interleaved gather costs W times the L2 requests of a single one (adjacent rows of a single vector already share
// their lines).  A band ends at the largest size at which its width was measured to be the fastest.
static int widest_kept(const edigpu_sector* s) {
  if (s->batch_force_w) return s->batch_force_w;
  const int64_t rows = s->nloc;
  if (s->kind == kDirect) return rows <= kDirW8Rows ? 8 : rows <= kDirW4Rows ? 4 : 2;
  return rows <= kSellW8Rows ? 8 : rows <= kSellW4Rows ? 4 : 2;
}

// width of a group of g seeds
static int width_for(int g) { return g <= 2 ? 2 : g <= 4 ? 4 : 8; }

static int64_t multi_partials(const edigpu_sector* s, int W) {
  // SELL: one workgroup per 4 slices; on the fly: at most 512 * direct_wgs persistent workgroups; norms: kRedBlocks
  const int64_t nb_sell = (s->nloc + 255) / 256 + 1;
  const int64_t nb_dir = (int64_t)512 * std::max(1, s->sw.direct_wgs);
  return 3 * (int64_t)W * std::max<int64_t>(std::max(nb_sell, nb_dir), kRedBlocks);
}

// the handle's interleaved buffers for width W, nscal doubles of scalars
static int ensure_batch(edigpu_sector* s, int W, size_t nscal, const char* who) {
  const int64_t len = s->nloc * (s->is_complex ? 2 : 1);
  if (!s->batch) s->batch = new BatchDev();
  BatchDev* b = s->batch;
  auto fail = [&](const char* what, hipError_t e) {
    set_error(std::string(who) + ": cannot allocate the interleaved " + what + " (" + hipGetErrorString(e) + ")");
    (void)hipGetLastError();
    free_batch(s);
    return 1;
  };
  if (b->W < W || b->len != len) {
    dev_free_all(b->P, b->Q);
    b->W = 0;
    const size_t bytes = (size_t)W * (size_t)len * sizeof(double);
    hipError_t e = hipMalloc((void**)&b->P, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&b->Q, bytes);
    if (e != hipSuccess) return fail("vectors", e);
    b->W = W;
    b->len = len;
  }
  const int64_t np = multi_partials(s, W);
  // (a failed hipMalloc is the thread's last HIP error: the message names it as before)
  if (dev_grow(&b->partial, &b->partial_cap, np)) return fail("partial sums", hipGetLastError());
  if (dev_grow(&b->scal, &b->scal_cap, nscal)) return fail("scalars", hipGetLastError());
  return 0;
}

// Yi (+)= H Xi on the handle's kind
static int multi_product(const edigpu_sector* s, int W, const double* Xi, double* Yi, bool lz, double* partial, int64_t cap,
                         int* np, const double* scal, int64_t sstride, hipStream_t st) {
  if (s->kind == kDirect) return launch_direct_multi(s, W, Xi, Yi, lz, partial, cap, np, scal, sstride, st);
  return launch_csr_multi(s->loc, s->is_complex, W, Xi, Yi, lz, partial, cap, np, scal, sstride, st);
}

// g seeds (natural layout, device) at width W -> rows of alanc / blanc ([g][nlanc]), niter_done[g], norm2[g]
static int tridiag_group(edigpu_sector* s, int W, int g, const double* vin, int nlanc, double* alanc, double* blanc,
                         double threshold, int* niter_done, double* norm2) {
  const int64_t sstride = ((int64_t)SC_AB + 2 * (int64_t)nlanc + 1) & ~(int64_t)1;
  if (ensure_batch(s, W, (size_t)(8 * sstride), "edigpu_lanczos_tridiag_batch_dev")) return 1;
  BatchDev* b = s->batch;
  hipStream_t st = s->stream;
  const int cplx = s->is_complex;
  const int64_t nrow = s->nloc;
  std::vector<double> sc((size_t)W * (size_t)sstride, 0.0);
  for (int j = 0; j < W; j++) sc[(size_t)j * sstride + SC_THR] = threshold;
  EDIGPU_HIP(hipMemcpyAsync(b->scal, sc.data(), sc.size() * sizeof(double), hipMemcpyHostToDevice, st));
  EDIGPU_HIP(hipMemsetAsync(b->Q, 0, (size_t)W * (size_t)b->len * sizeof(double), st));
  if (launch_interleave_multi(W, cplx, nrow, g, vin, b->P, st)) return 1;
  if (lz_norm_begin_multi(W, cplx, nrow, b->P, b->partial, b->partial_cap, b->scal, sstride, st)) return 1;
  for (int it = 0; it < nlanc; it++) {
    int np = 0;
    if (it > 0 && lz_rotate_lazy_multi(W, cplx, nrow, b->P, b->Q, b->scal, sstride, st)) return 1;
    if (multi_product(s, W, b->P, b->Q, true, b->partial, b->partial_cap, &np, b->scal, sstride, st)) return 1;
    if (lz_finalize_ab_multi(W, cplx, nrow, b->P, b->Q, b->partial, np, b->scal, sstride, nlanc, st)) return 1;
  }
  EDIGPU_HIP(hipMemcpyAsync(sc.data(), b->scal, sc.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  EDIGPU_HIP(hipStreamSynchronize(st));
  for (int j = 0; j < g; j++) {
    const double* c = sc.data() + (size_t)j * sstride;
    double* a = alanc + (size_t)j * nlanc;
    double* bb = blanc + (size_t)j * nlanc;
    if (!(c[SC_NORM] > 0.0)) {  // zero seed: as the single call
      std::fill(a, a + nlanc, 0.0);
      std::fill(bb, bb + nlanc, 0.0);
      if (niter_done) niter_done[j] = 0;
      if (norm2) norm2[j] = 0.0;
      continue;
    }
    for (int k = 0; k < nlanc; k++) {
      a[k] = c[SC_AB + k];
      bb[k] = c[SC_AB + nlanc + k];
    }
    if (niter_done) niter_done[j] = (int)c[SC_NDONE];
    if (norm2) norm2[j] = c[SC_NORM] * c[SC_NORM];
  }
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_apply_multi_dev(edigpu_handle s, int nvec, const void* x_dev, void* y_dev, void* stream) {
  if (!s || nvec < 1 || !x_dev || !y_dev) {
    set_error("edigpu_apply_multi_dev: bad argument");
    return 1;
  }
  const double* x = (const double*)x_dev;
  double* y = (double*)y_dev;
  // (a shard's product reads the whole gathered vector and writes its own rows: consecutive vectors of each length)
  const int64_t xlen = s->dim * (s->is_complex ? 2 : 1), ylen = s->nloc * (s->is_complex ? 2 : 1);
  const bool multi = multi_sector(s) && nvec >= 2;
  hipStream_t st = (hipStream_t)stream;
  if (multi) EDIGPU_HIP(hipSetDevice(s->device));
  const int wmax = multi ? widest_kept(s) : 1;
  for (int first = 0; first < nvec; first += wmax) {
    const int g = std::min(wmax, nvec - first);
    if (!multi || g == 1) {
      for (int j = first; j < first + g; j++)
        if (edigpu_apply_dev(s, x + (int64_t)j * xlen, y + (int64_t)j * ylen, stream)) return 1;
      continue;
    }
    const int W = width_for(g);
    if (ensure_batch(s, W, 0, "edigpu_apply_multi_dev")) return 1;
    BatchDev* b = s->batch;
    if (launch_interleave_multi(W, s->is_complex, s->nloc, g, x + (int64_t)first * xlen, b->P, st)) return 1;
    if (multi_product(s, W, b->P, b->Q, false, nullptr, 0, nullptr, nullptr, 0, st)) return 1;
    if (launch_deinterleave_multi(W, s->is_complex, s->nloc, g, b->Q, y + (int64_t)first * ylen, st)) return 1;
  }
  return 0;
}

int edigpu_batch_set_width(edigpu_handle s, int width) {
  if (!s || !(width == 0 || width == 2 || width == 4 || width == 8)) {
    set_error("edigpu_batch_set_width: bad argument (width must be 0, 2, 4 or 8)");
    return 1;
  }
  s->batch_force_w = width;
  return 0;
}

int edigpu_lanczos_tridiag_batch_dev(edigpu_handle s, int nseed, const double* vin_dev, int nlanc, double* alanc,
                                     double* blanc, double threshold, int* niter_done, double* norm2, int* route) {
  if (!s || nseed < 1 || nlanc <= 0 || !vin_dev || !alanc || !blanc) {
    set_error("edigpu_lanczos_tridiag_batch_dev: bad argument");
    return 1;
  }
  if (route) *route = 0;
  const int64_t len = s->dim * (s->is_complex ? 2 : 1);
  // (flat_lanczos_fusable = multi_sector and not EDIGPU_LANCZOS_UNFUSED.  EDIGPU_LANCZOS_EXACTBETA only changes the route
  // here: the single-seed step of these sectors is the fused one with or without it, so the numbers are the same)
  const bool multi = flat_lanczos_fusable(s) && nseed >= 2 && !LoopSwitches::sample().lanczos_exactbeta;
  if (multi) EDIGPU_HIP(hipSetDevice(s->device));
  int widest = 0;
  const int wmax = multi ? widest_kept(s) : 1;
  for (int first = 0; first < nseed; first += wmax) {
    const int g = std::min(wmax, nseed - first);
    const int W = width_for(g);
    const double* v = vin_dev + (int64_t)first * len;
    double* a = alanc + (size_t)first * nlanc;
    double* b = blanc + (size_t)first * nlanc;
    int* nd = niter_done ? niter_done + first : nullptr;
    double* n2 = norm2 ? norm2 + first : nullptr;
    if (multi && g >= 2) {
      if (tridiag_group(s, W, g, v, nlanc, a, b, threshold, nd, n2)) return 1;
      widest = std::max(widest, W);
      continue;
    }
    // the single-seed path, one seed after another: its checks, its refusals, its results
    for (int j = 0; j < g; j++)
      if (edigpu_lanczos_tridiag_dev(s, v + (int64_t)j * len, nlanc, a + (size_t)j * nlanc, b + (size_t)j * nlanc, threshold,
                                     nd ? nd + j : nullptr, n2 ? n2 + j : nullptr))
        return 1;
  }
  if (route) *route = widest;
  return 0;
}

}  // extern "C"
