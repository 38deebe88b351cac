// edigpu_occ.hip -- C ABI of the occupation operators (include/edigpu.h: edigpu_apply_occ, edigpu_occ_moments): checks,
// the handle's lazily built tables (host_occ.hpp), launches (kernels_occ.hip).
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_occ.hpp"
#include "kernels.hpp"

namespace edigpu {

static void free_occ_view(OccDev*& o) {
  if (!o) return;
  dev_free_all(o->pu, o->pd, o->order, o->partial, o->sums);
  delete o;
  o = nullptr;
}

void free_occ(edigpu_sector* s) {
  if (!s) return;
  free_occ_view(s->occ);
  free_occ_view(s->occ_shard);
}

static bool occ_served(const edigpu_sector* s) {
  return s && s->built_by_library && s->kind != kOrbs && s->is_whole();
}

int64_t occ_table_bytes(const edigpu_sector* s) {
  if (!occ_served(s)) return 0;
  const int64_t workspace = (int64_t)(4096 + 1) * kOccSums * 8;  // one vector's partial sums on a 256-CU device
  if (s->is_flat_family()) return 2 * (s->has_phonons() ? s->dim_el : s->dim) + workspace;
  const edigpu_sector* base = s->kind == kCmplxNormal ? s->sub_s : s;
  return 2 * s->dim_up + ((base && base->d_impd) ? 0 : s->dim_dw) + 4 * s->dim_dw * (s->nph + 1) + workspace;
}

int occ_refuse_kind(const edigpu_sector* s, const std::string& who) {
  if (s->kind == kOrbs) {
    set_error(who + ": ed_total_ud=F sectors are not supported");
    return 1;
  }
  if (!s->built_by_library) {
    set_error(who + ": the handle must be built from a model (edigpu_normal_build[_z], edigpu_flat_build[_jz], "
              "edigpu_direct_build[_jz]); a hand-over handle has no sector map");
    return 1;
  }
  return 0;
}

int occ_refuse(const edigpu_sector* s, const std::string& who) {
  if (occ_refuse_kind(s, who)) return 1;
  if (!s->is_whole()) {
    set_error(who + ": the handle must hold the whole sector (shards are not supported)");
    return 1;
  }
  return 0;
}

// the handle's tables, built on first use
static int occ_build(edigpu_sector* s, const std::string& who) {
  if (s->occ) return 0;
  const edigpu_model& m = s->model;
  if (m.norb < 1 || m.norb > kOccMaxOrb) {
    set_error(who + ": norb out of range");
    return 1;
  }
  OccDev* o = new OccDev();
  s->occ = o;  // freed by edigpu_destroy also when the build stops half-way
  o->norb = m.norb;
  o->nblk = s->nph + 1;
  EDIGPU_HIP(hipDeviceGetAttribute(&o->ncu, hipDeviceAttributeMultiprocessorCount, s->device));
  auto fail = [&](const std::string& why) {
    set_error(who + ": " + why);
    free_occ_view(s->occ);
    return 1;
  };
  if (s->is_flat_family()) {
    o->flat = 1;
    o->dim_up = s->has_phonons() ? s->dim_el : s->dim;
    o->dim_dw = 1;
    std::vector<int32_t> map((size_t)o->dim_up);
    int64_t n = o->dim_up;
    const int rc = s->jz ? edigpu_sector_map_jz(&m, s->sec_a, s->sec_b, map.data(), &n)
                         : edigpu_sector_map(&m, s->sec_a, 0, 0, map.data(), &n);
    if (rc) {
      free_occ_view(s->occ);
      return 1;  // the map's message stands
    }
    if (n != o->dim_up) return fail("the sector map does not have the handle's dimension");
    std::vector<uint16_t> pu(map.size());
    occ_patterns_state(map.data(), n, m.norb, model_ns(m), pu.data());
    if (dev_upload(&o->pu, pu)) return fail(edigpu_last_error());
    return 0;
  }
  o->dim_up = s->dim_up;
  o->dim_dw = s->dim_dw;
  std::vector<int32_t> mu((size_t)s->dim_up), md((size_t)s->dim_dw);
  int64_t nu = s->dim_up, nd = s->dim_dw;
  if (edigpu_sector_map(&m, s->sec_a, s->sec_b, 0, mu.data(), &nu) || edigpu_sector_map(&m, s->sec_a, s->sec_b, 1, md.data(), &nd)) {
    free_occ_view(s->occ);
    return 1;
  }
  if (nu != s->dim_up || nd != s->dim_dw) return fail("the sector maps do not have the handle's dimensions");
  std::vector<uint16_t> pu(mu.size()), pdw(md.size());
  occ_patterns_word(mu.data(), nu, m.norb, pu.data());
  occ_patterns_word(md.data(), nd, m.norb, pdw.data());
  std::vector<uint8_t> pd(pdw.begin(), pdw.end());
  std::vector<int32_t> order;
  occ_sort_rows(pd.data(), s->dim_dw, o->nblk, order, o->run);
  // the factored sectors already keep the down patterns on the device (edigpu_sector::d_impd)
  const edigpu_sector* base = s->kind == kCmplxNormal ? s->sub_s : s;
  const bool have_pd = base && base->factored && base->d_impd;
  if (dev_upload(&o->pu, pu) || dev_upload(&o->order, order) || (!have_pd && dev_upload(&o->pd, pd)))
    return fail(edigpu_last_error());
  return 0;
}

// the view of the rows [first, first + count), (re)built when the range is not the one it holds
static int occ_shard_build(edigpu_sector* s, int64_t first, int64_t count, const std::string& who) {
  if (s->occ_shard && s->occ_shard->first == first && s->occ_shard->count == count) return 0;
  free_occ_view(s->occ_shard);
  const edigpu_model& m = s->model;
  if (m.norb < 1 || m.norb > kOccMaxOrb) {
    set_error(who + ": norb out of range");
    return 1;
  }
  auto fail = [&](const std::string& why) {
    if (!why.empty()) set_error(who + ": " + why);  // (else the map's message stands)
    free_occ_view(s->occ_shard);
    return 1;
  };
  OccDev* o = new OccDev();
  s->occ_shard = o;
  o->norb = m.norb;
  o->nblk = s->nph + 1;
  EDIGPU_HIP(hipDeviceGetAttribute(&o->ncu, hipDeviceAttributeMultiprocessorCount, s->device));
  OccShardView view;
  if (s->is_flat_family()) {
    int64_t n = s->dim / o->nblk;  // the electronic rows of the WHOLE sector (dim_el of a phonon shard is the shard's)
    std::vector<int32_t> map((size_t)n);
    const int64_t want = n;
    if (s->jz ? edigpu_sector_map_jz(&m, s->sec_a, s->sec_b, map.data(), &n) : edigpu_sector_map(&m, s->sec_a, 0, 0, map.data(), &n))
      return fail("");
    if (n != want) return fail("the sector map does not have the handle's dimension");
    std::vector<uint16_t> pat(map.size());
    occ_patterns_state(map.data(), n, m.norb, model_ns(m), pat.data());
    occ_shard_view(pat.data(), n, true, o->nblk, first, count, view);
    if (view.first != first || view.count != count) return fail("the rows are not inside the sector");
    o->flat = 1;
    o->dim_up = count;
    o->dim_dw = 1;
    if (dev_upload(&o->pu, view.pu)) return fail(edigpu_last_error());
  } else {
    std::vector<int32_t> mu((size_t)s->dim_up), md((size_t)s->dim_dw);
    int64_t nu = s->dim_up, nd = s->dim_dw;
    if (edigpu_sector_map(&m, s->sec_a, s->sec_b, 0, mu.data(), &nu) || edigpu_sector_map(&m, s->sec_a, s->sec_b, 1, md.data(), &nd))
      return fail("");
    if (nu != s->dim_up || nd != s->dim_dw) return fail("the sector maps do not have the handle's dimensions");
    std::vector<uint16_t> pu(mu.size()), pdw(md.size());
    occ_patterns_word(mu.data(), nu, m.norb, pu.data());
    occ_patterns_word(md.data(), nd, m.norb, pdw.data());
    occ_shard_view(pdw.data(), nd, false, o->nblk, first, count, view);
    if (view.first != first || view.count != count) return fail("the rows are not inside the sector");
    o->dim_up = s->dim_up;
    o->dim_dw = count;
    std::copy(view.run, view.run + kOccMaxPat + 1, o->run);
    // the shard's own copy of its down patterns: edigpu_sector::d_impd starts at row 0 of the sector
    if (dev_upload(&o->pu, pu) || dev_upload(&o->order, view.order) || dev_upload(&o->pd, view.pd)) return fail(edigpu_last_error());
  }
  o->first = first;
  o->count = count;
  return 0;
}

static OccTables occ_args(const edigpu_sector* s, const OccDev* o) {
  OccTables t;
  t.norb = o->norb;
  t.flat = o->flat;
  t.cplx = s->is_complex;
  t.nblk = o->nblk;
  t.dim_up = o->dim_up;
  t.dim_dw = o->dim_dw;
  t.pu = o->pu;
  t.pd = o->pd ? o->pd : (s->kind == kCmplxNormal ? s->sub_s->d_impd : s->d_impd);
  t.order = o->order;
  return t;
}

// sums of nvec vectors into o->sums on the handle's stream (workspace grown on demand)
static int occ_moments_enqueue(edigpu_sector* s, OccDev* o, const double* v_dev, int nvec) {
  const OccTables t = occ_args(s, o);
  const int nwaves = occ_moment_waves(t, o->ncu);
  const int64_t need_partial = (int64_t)nvec * nwaves * kOccSums, need_sums = (int64_t)nvec * kOccSums;
  if (dev_grow(&o->partial, &o->partial_cap, need_partial) || dev_grow(&o->sums, &o->sums_cap, need_sums)) return 1;
  OccSlots sl;
  sl.nslots = occ_sum_slots(o->norb, sl.need_up, sl.need_dw);
  OccRuns rn;
  std::copy(o->run, o->run + 33, rn.run);
  return launch_occ_moments(t, sl, rn, v_dev, nvec, nwaves, o->partial, o->sums, s->stream);
}

int occ_shard_moments(edigpu_sector* s, int64_t first, int64_t count, const double* v_dev, int nvec, const double** sums_dev,
                      const std::string& who) {
  *sums_dev = nullptr;
  if (count <= 0) return 0;
  if (occ_shard_build(s, first, count, who) || occ_moments_enqueue(s, s->occ_shard, v_dev, nvec)) return 1;
  *sums_dev = s->occ_shard->sums;
  return 0;
}

int occ_shard_apply(edigpu_sector* s, int64_t first, int64_t count, const double* src_dev, double* dst_dev, const double* w_up,
                    const double* w_dw, const std::string& who) {
  if (count <= 0) return 0;
  if (occ_shard_build(s, first, count, who)) return 1;
  OccWeights w;
  occ_weight_table(w_up, s->occ_shard->norb, w.wu);
  occ_weight_table(w_dw, s->occ_shard->norb, w.wd);
  return launch_apply_occ(occ_args(s, s->occ_shard), w, src_dev, dst_dev, s->stream);
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_apply_occ(edigpu_handle s, const double* v_src_dev, double* v_dst_dev, const double* w_up, const double* w_dw,
                     void* stream) {
  const std::string who = "edigpu_apply_occ";
  if (!s || !v_src_dev || !v_dst_dev || !w_up || !w_dw) {
    set_error(who + ": NULL argument");
    return 1;
  }
  if (occ_refuse(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (occ_build(s, who)) return 1;
  OccWeights w;
  occ_weight_table(w_up, s->occ->norb, w.wu);
  occ_weight_table(w_dw, s->occ->norb, w.wd);
  return launch_apply_occ(occ_args(s, s->occ), w, v_src_dev, v_dst_dev, (hipStream_t)stream);
}

int edigpu_occ_moments(edigpu_handle s, const double* v_dev, int nvec, double* moments_host, double* norm2_host) {
  const std::string who = "edigpu_occ_moments";
  if (!s || !v_dev || !moments_host || nvec <= 0) {
    set_error(who + (!s || !v_dev || !moments_host ? ": NULL argument" : ": nvec must be positive"));
    return 1;
  }
  if (occ_refuse(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (occ_build(s, who) || occ_moments_enqueue(s, s->occ, v_dev, nvec)) return 1;
  const OccDev* o = s->occ;
  std::vector<double> sums((size_t)nvec * kOccSums);
  EDIGPU_HIP(hipMemcpyAsync(sums.data(), o->sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  EDIGPU_HIP(hipStreamSynchronize(s->stream));
  const int n2 = 2 * o->norb;
  for (int k = 0; k < nvec; k++)
    occ_expand_sums(sums.data() + (size_t)k * kOccSums, o->norb, moments_host + (size_t)k * n2 * n2,
                    norm2_host ? norm2_host + k : nullptr);
  return 0;
}

int edigpu_time_occ(edigpu_handle s, double* v_dev, int warmup, int steps, double* ms2) {
  const std::string who = "edigpu_time_occ";
  if (!s || !v_dev || !ms2 || warmup < 0 || steps <= 0) {
    set_error(who + ": bad argument");
    return 1;
  }
  if (occ_refuse(s, who)) return 1;
  EDIGPU_HIP(hipSetDevice(s->device));
  if (occ_build(s, who)) return 1;
  OccWeights w;
  double one[kOccMaxOrb];
  std::fill(one, one + kOccMaxOrb, 1.0);  // weights 0, 1, 2: the values of v stay finite over any number of passes
  occ_weight_table(one, s->occ->norb, w.wu);
  occ_weight_table(one, s->occ->norb, w.wd);
  const OccTables t = occ_args(s, s->occ);
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  for (int which = 0; which < 2 && !rc; which++) {
    std::vector<float> ms((size_t)steps, 0.f);
    for (int k = 0; k < warmup + steps && !rc; k++) {
      rc |= hipEventRecord(e0, s->stream) != hipSuccess;
      rc |= which == 0 ? occ_moments_enqueue(s, s->occ, v_dev, 1) : launch_apply_occ(t, w, v_dev, v_dev, s->stream);
      rc |= hipEventRecord(e1, s->stream) != hipSuccess;
      rc |= hipEventSynchronize(e1) != hipSuccess;
      if (!rc && k >= warmup) rc |= hipEventElapsedTime(&ms[(size_t)(k - warmup)], e0, e1) != hipSuccess;
    }
    std::sort(ms.begin(), ms.end());
    ms2[which] = ms[ms.size() / 2];
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    if (std::string(edigpu_last_error()).empty()) set_error(who + ": HIP failure");
    return 1;
  }
  return 0;
}

}  // extern "C"
