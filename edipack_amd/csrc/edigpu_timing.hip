// edigpu_timing.hip -- the measurement entry points of the C ABI: edigpu_time_apply, edigpu_lanczos_bench, edigpu_membw.
#include <algorithm>
#include <chrono>
#include <vector>

#include "kernels.hpp"

using namespace edigpu;

extern "C" {

int edigpu_time_apply(edigpu_handle s, int warmup, int steps, int lanczos, double* ms_per_step) {
  if (!s || steps <= 0 || !ms_per_step) {
    set_error("edigpu_time_apply: bad argument");
    return 1;
  }
  if (single_shard(s, "edigpu_time_apply")) return 1;
  if (s->kind == kCmplxNormal && s->sub_d && lanczos) return edigpu_time_apply(s->sub_d, warmup, steps, lanczos, ms_per_step);
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ensure_workspace(s)) return 1;
  hipStream_t st = s->stream;
  const int total = warmup + steps;
  if (lanczos_prepare(s, std::max(total, 1), 0.0, st)) return 1;
  if (lanczos) {  // 1: Lanczos steps; 2: the plain product as the loop computes it (panel-major vectors where it uses them)
    if (lanczos_seed(s, nullptr, 12345ull, st)) return 1;
    if (lz_norm_begin(s->d_vin, s->lz_len, s->d_partial, s->d_scal, st)) return 1;
  } else {  // the boundary product (edigpu_apply_dev): vectors in the natural layout
    if (lz_fill_random(s->d_vin, s->ws_len, 12345ull, st)) return 1;
    if (lz_norm_begin(s->d_vin, s->ws_len, s->d_partial, s->d_scal, st)) return 1;
  }
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  for (int it = 0; it < total && !rc; it++) {
    if (it == warmup) rc |= (hipEventRecord(e0, st) != hipSuccess);
    if (lanczos == 2) {
      rc |= s->lz_blocked ? launch_normal_blocked(s, s->d_vin, s->d_tmp, st) : apply_any(s, s->d_vin, s->d_vin, s->d_tmp, 3, st);
    } else if (lanczos) {
      rc |= lanczos_step(s, it, total, st);
    } else {
      // fixed source vector -> fixed destination: the plain SpMV measurement
      rc |= apply_any(s, s->d_vin, s->d_vin, s->d_tmp, 3, st);
    }
  }
  if (!rc) rc |= (hipEventRecord(e1, st) != hipSuccess);
  if (!rc) rc |= (hipEventSynchronize(e1) != hipSuccess);
  float ms = 0.f;
  if (!rc) rc |= (hipEventElapsedTime(&ms, e0, e1) != hipSuccess);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    if (!have_error()) set_error("edigpu_time_apply: HIP failure");
    return 1;
  }
  *ms_per_step = (double)ms / (double)steps;
  return 0;
}

int edigpu_membw(int64_t bytes, double* gbs3) {
  if (!gbs3 || bytes < (1 << 20)) {
    set_error("edigpu_membw: bad argument");
    return 1;
  }
  if (ensure_device()) return 1;
  EDIGPU_HIP(hipSetDevice(current_device()));
  return measure_membw(bytes, gbs3);
}

int edigpu_lanczos_bench(edigpu_handle s, int warmup, int steps, double* ms_wall_per_step,
                         double* ms_hv_per_launch) {
  if (!s || steps <= 0 || warmup < 0 || !ms_wall_per_step || !ms_hv_per_launch) {
    set_error("edigpu_lanczos_bench: bad argument");
    return 1;
  }
  if (single_shard(s, "edigpu_lanczos_bench")) return 1;
  if (s->kind == kCmplxNormal && s->sub_d) return edigpu_lanczos_bench(s->sub_d, warmup, steps, ms_wall_per_step, ms_hv_per_launch);
  EDIGPU_HIP(hipSetDevice(s->device));
  if (ensure_workspace(s)) return 1;
  hipStream_t st = s->stream;
  const int total = warmup + steps;
  if (lanczos_prepare(s, total, 0.0, st)) return 1;
  if (lanczos_seed(s, nullptr, 12345ull, st)) return 1;
  if (lz_norm_begin(s->d_vin, s->lz_len, s->d_partial, s->d_scal, st)) return 1;
  int rc = 0;
  // the product as the loop computes it: on the panel-major vectors when the recurrence runs on them
  auto hv_probe = [&]() -> int {
    if (s->lz_blocked) return launch_normal_blocked(s, s->d_vin, s->d_tmp, st);
    return apply_any(s, s->d_vin, s->d_vin, s->d_tmp, 3, st);
  };
  // (a launch-bound sector replays its steps from a captured graph, as edigpu_lanczos_tridiag does: lanczos_run)
  rc |= lanczos_run(s, 0, warmup, total, st);
  if (!rc) rc |= (hipStreamSynchronize(st) != hipSuccess);
  const auto t0 = std::chrono::steady_clock::now();
  if (!rc) rc |= lanczos_run(s, warmup, total, total, st);
  if (!rc) rc |= (hipStreamSynchronize(st) != hipSuccess);
  const auto t1 = std::chrono::steady_clock::now();
  // H*v launches alone (the Lanczos vector of the last step as input), HIP events around each
  std::vector<hipEvent_t> ev(2 * (size_t)steps);
  for (auto& e : ev) EDIGPU_HIP(hipEventCreate(&e));
  for (int k = 0; k < 3 && !rc; k++) rc |= hv_probe();
  for (int k = 0; k < steps && !rc; k++) {
    rc |= (hipEventRecord(ev[2 * k], st) != hipSuccess);
    rc |= hv_probe();
    rc |= (hipEventRecord(ev[2 * k + 1], st) != hipSuccess);
  }
  if (!rc) rc |= (hipStreamSynchronize(st) != hipSuccess);
  double hv = 0.0;
  for (int k = 0; k < steps && !rc; k++) {
    float ms = 0.f;
    rc |= (hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) != hipSuccess);
    hv += ms;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  if (rc) {
    if (!have_error()) set_error("edigpu_lanczos_bench: HIP failure");
    return 1;
  }
  *ms_wall_per_step = std::chrono::duration<double, std::milli>(t1 - t0).count() / steps;
  *ms_hv_per_launch = hv / steps;
  return 0;
}

}  // extern "C"
