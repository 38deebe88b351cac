// edigpu_pairs.hip -- C ABI of the fused two-operator products (include/edigpu.h: edigpu_pairs_sector,
// edigpu_apply_pairs_normal, edigpu_time_pairs): checks, the per-call tables (host_pairs.hpp), launch (kernels_pairs.hip).
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_pairs.hpp"
#include "kernels.hpp"

namespace edigpu {
namespace {

std::vector<PairsTerm> pairs_terms(int nterms, const double* coef, const int32_t* create1, const int32_t* iorb1,
                                   const int32_t* ispin1, const int32_t* create2, const int32_t* iorb2, const int32_t* ispin2) {
  std::vector<PairsTerm> t((size_t)std::max(nterms, 0));
  for (int k = 0; k < nterms; k++)
    t[(size_t)k] = PairsTerm{coef ? coef[k] : 1.0, PairsOp{create1[k], iorb1[k], ispin1[k]}, PairsOp{create2[k], iorb2[k], ispin2[k]}};
  return t;
}

// one refusal per kind of handle the products do not serve
int pairs_refuse(const edigpu_sector* s, const std::string& who, const char* which) {
  const std::string w = who + ": the " + which + " handle ";
  if (s->kind == kCmplxNormal || (s->kind == kNormal && s->is_complex)) {
    set_error(w + "is a complex normal-mode sector (edigpu_normal_build_z): only real vectors are supported");
    return 1;
  }
  if (s->is_flat_family()) {
    set_error(w + "is a superc / nonsu2 sector: only ed_mode=normal sectors are supported");
    return 1;
  }
  if (s->kind == kOrbs) {
    set_error(w + "is an ed_total_ud=F sector: ed_total_ud=F sectors are not supported");
    return 1;
  }
  if (s->kind != kNormal || !s->built_by_library) {
    set_error(w + "must be built from a model (edigpu_normal_build); a hand-over handle has no sector labels");
    return 1;
  }
  if (!s->is_whole()) {
    set_error(w + "must hold the whole sector (shards are not supported)");
    return 1;
  }
  return 0;
}

bool same_model_shape(const edigpu_model& a, const edigpu_model& b) {
  return a.ed_mode == b.ed_mode && a.bath_type == b.bath_type && a.norb == b.norb && a.nbath == b.nbath && a.nspin == b.nspin &&
         a.nph == b.nph;
}

// every check of a call and the host tables; v_src = v_dst = null: no vectors to compare (the sharded call checks its
// shards itself)
int pairs_prepare(const edigpu_sector* src, const edigpu_sector* dst, const double* v_src, const double* v_dst,
                  const std::vector<PairsTerm>& terms, const std::string& who, PairsTables& tab) {
  if (pairs_refuse(src, who, "source") || pairs_refuse(dst, who, "destination")) return 1;
  if (!same_model_shape(src->model, dst->model) || src->nph != dst->nph || src->device != dst->device) {
    set_error(who + ": the two handles are sectors of different models (or devices)");
    return 1;
  }
  if ((int)terms.size() > kPairsMaxTerms || terms.empty()) {
    set_error(who + ": nterms must be 1 .. " + std::to_string(kPairsMaxTerms));
    return 1;
  }
  const std::string why = pairs_build(src->sec_a, src->sec_b, model_ns(src->model), src->model.norb, (int)terms.size(),
                                      terms.data(), tab);
  if (!why.empty()) {
    set_error(who + ": " + why);
    return 1;
  }
  if (dst->sec_a != tab.nup_dst || dst->sec_b != tab.ndw_dst) {
    set_error(who + ": the destination handle is the sector (" + std::to_string(dst->sec_a) + ", " + std::to_string(dst->sec_b) +
              "), the terms lead to (" + std::to_string(tab.nup_dst) + ", " + std::to_string(tab.ndw_dst) + ")");
    return 1;
  }
  if (tab.dim_up_src != src->dim_up || tab.dim_dw_src != src->dim_dw || tab.dim_up_dst != dst->dim_up ||
      tab.dim_dw_dst != dst->dim_dw) {
    set_error(who + ": the tables do not have the handles' dimensions");
    return 1;
  }
  if (v_src && v_dst) {
    const char *a0 = (const char*)v_src, *a1 = a0 + src->dim * (int64_t)sizeof(double);
    const char *b0 = (const char*)v_dst, *b1 = b0 + dst->dim * (int64_t)sizeof(double);
    if (a0 < b1 && b0 < a1) {
      set_error(who + ": v_dst_dev overlaps v_src_dev (the gather cannot run in place)");
      return 1;
    }
  }
  return 0;
}

// device copy of the tables of one call: one allocation, up tables first
struct PairsDevTables {
  uint32_t* d = nullptr;
  ~PairsDevTables() { dev_free(d); }
};

int pairs_upload(const PairsTables& tab, int nblk, PairsDevTables& dev, PairsArgs& a, hipStream_t st) {
  std::vector<uint32_t> both(tab.up);
  both.insert(both.end(), tab.dw.begin(), tab.dw.end());
  EDIGPU_HIP(hipMalloc((void**)&dev.d, both.size() * sizeof(uint32_t)));
  EDIGPU_HIP(hipMemcpyAsync(dev.d, both.data(), both.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  EDIGPU_HIP(hipStreamSynchronize(st));  // `both` is pageable and leaves scope
  a = PairsArgs();
  a.nterms = tab.nterms;
  a.nblk = nblk;
  a.id_up = tab.id_up;
  a.id_dw = tab.id_dw;
  a.du_src = tab.dim_up_src;
  a.dd_src = tab.dim_dw_src;
  a.du_dst = tab.dim_up_dst;
  a.dd_dst = tab.dim_dw_dst;
  std::copy(tab.coef, tab.coef + kPairsMaxTerms, a.coef);
  a.pu = dev.d;
  a.pd = dev.d + tab.up.size();
  return 0;
}

// upload, launch, wait for the stream, free
int pairs_call(const edigpu_sector* src, const PairsTables& tab, const double* v_src, double* v_dst, hipStream_t st) {
  PairsDevTables dev;
  PairsArgs a;
  if (pairs_upload(tab, src->nph + 1, dev, a, st)) return 1;
  if (launch_apply_pairs(a, v_src, v_dst, st)) return 1;
  EDIGPU_HIP(hipStreamSynchronize(st));  // the tables are freed only after the kernel has read them
  return 0;
}

}  // namespace

int pairs_shard_tables(const edigpu_sector* src, const edigpu_sector* dst, int nterms, const double* coef, const int32_t* create1,
                       const int32_t* iorb1, const int32_t* ispin1, const int32_t* create2, const int32_t* iorb2,
                       const int32_t* ispin2, const std::string& who, PairsTables& tab) {
  if (nterms < 1 || nterms > kPairsMaxTerms) {
    set_error(who + ": nterms must be 1 .. " + std::to_string(kPairsMaxTerms));
    return 1;
  }
  return pairs_prepare(src, dst, nullptr, nullptr, pairs_terms(nterms, coef, create1, iorb1, ispin1, create2, iorb2, ispin2), who,
                       tab);
}

int pairs_shard_call(const edigpu_sector* src, const PairsTables& tab, const ShardWindow* win, int64_t rows, const double* v_src,
                     double* v_dst, hipStream_t st) {
  PairsDevTables dev;
  PairsArgs a;
  if (pairs_upload(tab, src->nph + 1, dev, a, st)) return 1;
  if (win) {
    if (launch_apply_pairs_window(a, *win, v_src, v_dst, st)) return 1;
  } else {
    // no term moves a down electron (every bit of id_dw is set: the down tables are not read): the rank's rows are a
    // vector of `rows` down rows on both sides
    a.dd_src = a.dd_dst = rows;
    if (launch_apply_pairs(a, v_src, v_dst, st)) return 1;
  }
  EDIGPU_HIP(hipStreamSynchronize(st));  // the tables are freed only after the kernel has read them
  return 0;
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_pairs_sector(const edigpu_model* model, int nup, int ndw, int nterms, const int32_t* create1, const int32_t* iorb1,
                        const int32_t* ispin1, const int32_t* create2, const int32_t* iorb2, const int32_t* ispin2,
                        int* nup_dst, int* ndw_dst, int* exists) {
  const std::string who = "edigpu_pairs_sector";
  if (!model || !create1 || !iorb1 || !ispin1 || !create2 || !iorb2 || !ispin2 || !nup_dst || !ndw_dst || !exists) {
    set_error(who + ": NULL argument");
    return 1;
  }
  if (model->ed_mode != 0) {
    set_error(who + ": only ed_mode=normal models are supported");
    return 1;
  }
  if (nterms < 1 || nterms > kPairsMaxTerms) {
    set_error(who + ": nterms must be 1 .. " + std::to_string(kPairsMaxTerms));
    return 1;
  }
  const std::vector<PairsTerm> terms = pairs_terms(nterms, nullptr, create1, iorb1, ispin1, create2, iorb2, ispin2);
  PairsDest d;
  const std::string why = pairs_check(nup, ndw, model_ns(*model), model->norb, nterms, terms.data(), d);
  if (!why.empty()) {
    set_error(who + ": " + why);
    return 1;
  }
  *nup_dst = d.nup;
  *ndw_dst = d.ndw;
  *exists = d.exists ? 1 : 0;
  return 0;
}

int edigpu_apply_pairs_normal(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev, int nterms,
                              const double* coef, const int32_t* create1, const int32_t* iorb1, const int32_t* ispin1,
                              const int32_t* create2, const int32_t* iorb2, const int32_t* ispin2, void* stream) {
  const std::string who = "edigpu_apply_pairs_normal";
  if (!src || !dst || !v_src_dev || !v_dst_dev || !coef || !create1 || !iorb1 || !ispin1 || !create2 || !iorb2 || !ispin2) {
    set_error(who + ": NULL argument");
    return 1;
  }
  if (nterms < 1 || nterms > kPairsMaxTerms) {
    set_error(who + ": nterms must be 1 .. " + std::to_string(kPairsMaxTerms));
    return 1;
  }
  const std::vector<PairsTerm> terms = pairs_terms(nterms, coef, create1, iorb1, ispin1, create2, iorb2, ispin2);
  PairsTables tab;
  if (pairs_prepare(src, dst, v_src_dev, v_dst_dev, terms, who, tab)) return 1;
  EDIGPU_HIP(hipSetDevice(src->device));
  return pairs_call(src, tab, v_src_dev, v_dst_dev, (hipStream_t)stream);
}

int edigpu_time_pairs(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev, int nterms,
                      const double* coef, const int32_t* create1, const int32_t* iorb1, const int32_t* ispin1,
                      const int32_t* create2, const int32_t* iorb2, const int32_t* ispin2, int warmup, int steps, double* ms2) {
  const std::string who = "edigpu_time_pairs";
  if (!src || !dst || !v_src_dev || !v_dst_dev || !coef || !create1 || !iorb1 || !ispin1 || !create2 || !iorb2 || !ispin2 ||
      !ms2 || warmup < 0 || steps <= 0) {
    set_error(who + ": bad argument");
    return 1;
  }
  if (nterms < 1 || nterms > kPairsMaxTerms) {
    set_error(who + ": nterms must be 1 .. " + std::to_string(kPairsMaxTerms));
    return 1;
  }
  const std::vector<PairsTerm> terms = pairs_terms(nterms, coef, create1, iorb1, ispin1, create2, iorb2, ispin2);
  PairsTables tab;
  if (pairs_prepare(src, dst, v_src_dev, v_dst_dev, terms, who, tab)) return 1;
  EDIGPU_HIP(hipSetDevice(src->device));
  hipStream_t st = src->stream;
  PairsDevTables dev;
  PairsArgs a;
  if (pairs_upload(tab, src->nph + 1, dev, a, st)) return 1;
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  for (int which = 0; which < 2 && !rc; which++) {
    std::vector<float> ms((size_t)steps, 0.f);
    for (int k = 0; k < warmup + steps && !rc; k++) {
      rc |= hipEventRecord(e0, st) != hipSuccess;
      if (which == 0) {  // what a caller pays: the host tables, their upload, the kernel, the wait, the free
        PairsTables again;
        rc |= pairs_prepare(src, dst, v_src_dev, v_dst_dev, terms, who, again) || pairs_call(src, again, v_src_dev, v_dst_dev, st);
      } else {
        rc |= launch_apply_pairs(a, v_src_dev, v_dst_dev, st);
      }
      rc |= hipEventRecord(e1, st) != hipSuccess;
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
