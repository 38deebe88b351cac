// edigpu_axisop.hip -- c / c^+ on device vectors of phonon, complex normal-mode and ed_total_ud=F sectors: the route of
// edigpu_apply_op_normal / edigpu_apply_cops_normal for what apply_op_normal_kernel does not serve, and the C ABI of
// edigpu_apply_cops_normal_z and edigpu_time_apply_op.  Checks, the per-call tables (host_axisop.hpp), the scratch buffer
// the destination handle keeps for them, launch (kernels_axisop.hip).
#include <algorithm>
#include <string>
#include <vector>

#include "dev_mem.hpp"
#include "host_axisop.hpp"
#include "kernels.hpp"

namespace edigpu {

// device scratch of the partner tables, kept by the destination handle and grown on demand
struct AxisDev {
  uint32_t* d = nullptr;
  size_t cap = 0;  // entries
};

void free_axisop(edigpu_sector* s) {
  if (!s || !s->axis) return;
  dev_free(s->axis->d);
  delete s->axis;
  s->axis = nullptr;
}

namespace {

bool axis_is_orbs_handover(const edigpu_sector* s) { return s->kind == kOrbs && s->orbs_nups.empty(); }

const char* axis_kind_name(const edigpu_sector* s) {
  switch (s->kind) {
    case kNormal: return s->has_phonons() ? "a real normal-mode phonon sector" : "a real normal-mode sector";
    case kFlat: case kDirect: return "a superc / nonsu2 sector";
    case kOrbs: return "an ed_total_ud=F sector";
    case kCmplxNormal: return "a complex normal-mode sector";
  }
  return "an unknown handle";
}

// one refusal per kind of handle this route does not serve
int axis_refuse(const edigpu_sector* s, const std::string& who, const char* which) {
  const std::string w = who + ": the " + which + " handle ";
  if (s->is_flat_family()) {
    set_error(w + "is a superc / nonsu2 sector: edigpu_apply_op_flat / edigpu_apply_cops_flat serve those");
    return 1;
  }
  if (s->kind == kNormal && !s->built_by_library) {
    set_error(w + "is a hand-over handle (edigpu_normal_create): it has no sector labels");
    return 1;
  }
  if (axis_is_orbs_handover(s)) {
    set_error(w + "is a hand-over handle (edigpu_orbs_create): it has no sector labels");
    return 1;
  }
  if (s->kind != kNormal && s->kind != kOrbs && s->kind != kCmplxNormal) {
    set_error(w + "is not a normal-mode sector");
    return 1;
  }
  if (!s->is_whole() || s->row_first != 0) {
    set_error(w + "is a shard: it must hold the whole sector (shards are not supported)");
    return 1;
  }
  if (s->kind == kOrbs && s->has_phonons()) {
    set_error(w + "is an ed_total_ud=F phonon sector: not supported");
    return 1;
  }
  return 0;
}

bool axis_same_model(const edigpu_model& a, const edigpu_model& b) {
  return a.ed_mode == b.ed_mode && a.bath_type == b.bath_type && a.norb == b.norb && a.nbath == b.nbath && a.nspin == b.nspin;
}

std::string axis_label(const std::vector<int>& u, const std::vector<int>& d) {
  std::string s = "(";
  for (size_t k = 0; k < u.size(); k++) s += (k ? " " : "") + std::to_string(u[k]);
  s += " | ";
  for (size_t k = 0; k < d.size(); k++) s += (k ? " " : "") + std::to_string(d[k]);
  return s + ")";
}

// every check of a call and the host tables; need_kind4: the _z entry point; v_src = v_dst = null: no vectors to compare
// (the sharded call checks its shards itself)
int axis_prepare(const edigpu_sector* src, const edigpu_sector* dst, const double* v_src, const double* v_dst, int nops,
                 const int32_t* create, const int32_t* iorb, const int32_t* ispin, bool need_kind4, const std::string& who,
                 AxisTables& tab) {
  if (need_kind4)
    for (const edigpu_sector* s : {src, dst})
      if (s->kind != kCmplxNormal) {
        set_error(who + ": the " + (s == src ? "source" : "destination") + " handle is " + axis_kind_name(s) +
                  ": complex coefficients are served on complex normal-mode sectors (edigpu_normal_build_z) only");
        return 1;
      }
  if (axis_refuse(src, who, "source") || axis_refuse(dst, who, "destination")) return 1;
  if (src->kind != dst->kind) {
    set_error(who + ": the handles are of different kinds: the source is " + axis_kind_name(src) + ", the destination " +
              axis_kind_name(dst));
    return 1;
  }
  if (!axis_same_model(src->model, dst->model)) {
    set_error(who + ": the two handles are sectors of different models");
    return 1;
  }
  if (src->nph != dst->nph || src->model.nph != dst->model.nph) {
    set_error(who + ": the two handles have different nph (" + std::to_string(src->nph) + " and " + std::to_string(dst->nph) + ")");
    return 1;
  }
  if (src->device != dst->device) {
    set_error(who + ": the two handles are on different devices");
    return 1;
  }
  if (nops < 1 || nops > kAxisMaxTerms) {
    set_error(who + ": nops must be 1 .. " + std::to_string(kAxisMaxTerms));
    return 1;
  }
  std::vector<AxisOp> ops((size_t)nops);
  for (int k = 0; k < nops; k++) ops[(size_t)k] = AxisOp{create[k], iorb[k], ispin[k]};
  const edigpu_model& m = src->model;
  std::string why;
  if (src->kind == kOrbs) {
    std::vector<int> nu((size_t)m.norb), nd((size_t)m.norb);
    why = axisop_build_orbs(m.norb, m.nbath, src->orbs_nups.data(), src->orbs_ndws.data(), nops, ops.data(), nu.data(),
                            nd.data(), tab);
    if (why.empty() && (nu != dst->orbs_nups || nd != dst->orbs_ndws)) {
      set_error(who + ": the destination handle is the sector " + axis_label(dst->orbs_nups, dst->orbs_ndws) +
                ", the operators lead to " + axis_label(nu, nd));
      return 1;
    }
  } else {
    int nu = 0, nd = 0;
    why = axisop_build_normal(src->sec_a, src->sec_b, model_ns(m), m.norb, src->nph + 1, src->kind == kCmplxNormal, nops, ops.data(), nu,
                              nd, tab);
    if (why.empty() && (dst->sec_a != nu || dst->sec_b != nd)) {
      set_error(who + ": the destination handle is the sector (" + std::to_string(dst->sec_a) + ", " + std::to_string(dst->sec_b) +
                "), the operators lead to (" + std::to_string(nu) + ", " + std::to_string(nd) + ")");
      return 1;
    }
  }
  if (!why.empty()) {
    set_error(who + ": " + why);
    return 1;
  }
  const int64_t w = src->is_complex ? 2 : 1;
  if (tab.O * tab.a_src * tab.I != src->dim * w || tab.O * tab.a_dst * tab.I != dst->dim * w) {
    set_error(who + ": the tables do not have the handles' dimensions");
    return 1;
  }
  if (v_src && v_dst) {
    const char *a0 = (const char*)v_src, *a1 = a0 + src->dim * w * (int64_t)sizeof(double);
    const char *b0 = (const char*)v_dst, *b1 = b0 + dst->dim * w * (int64_t)sizeof(double);
    if (a0 < b1 && b0 < a1) {
      set_error(who + ": v_dst_dev overlaps v_src_dev (the gather cannot run in place)");
      return 1;
    }
  }
  return 0;
}

// the tables into the destination handle's scratch (no allocation once it is large enough); `tab` must outlive the copy
int axis_upload(edigpu_sector* dst, const AxisTables& tab, const double* cre, const double* cim, AxisArgs& a, hipStream_t st) {
  if (!dst->axis) dst->axis = new AxisDev();
  AxisDev* dev = dst->axis;
  const size_t n = std::max<size_t>(tab.part.size(), 1);
  if (dev_grow(&dev->d, &dev->cap, n)) return 1;
  if (!tab.part.empty())
    EDIGPU_HIP(hipMemcpyAsync(dev->d, tab.part.data(), tab.part.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  a = AxisArgs();
  a.nterms = tab.nterms;
  a.I = tab.I;
  a.a_src = tab.a_src;
  a.a_dst = tab.a_dst;
  a.O = tab.O;
  for (int t = 0; t < tab.nterms; t++) {
    a.cre[t] = cre[t];
    a.cim[t] = cim ? cim[t] : 0.0;
  }
  a.part = dev->d;
  return 0;
}

// upload, launch, wait for the stream (the host table is pageable and leaves scope)
int axis_call(edigpu_sector* dst, const AxisTables& tab, const double* cre, const double* cim, const double* v_src,
              double* v_dst, hipStream_t st) {
  AxisArgs a;
  if (axis_upload(dst, tab, cre, cim, a, st)) return 1;
  const int rc = launch_apply_axisop(a, cim != nullptr, v_src, v_dst, st);
  EDIGPU_HIP(hipStreamSynchronize(st));
  return rc;
}

}  // namespace

int axisop_tables(const edigpu_sector* src, const edigpu_sector* dst, int nops, const int32_t* create, const int32_t* iorb,
                  const int32_t* ispin, bool cplx_coef, const char* who, AxisTables& tab) {
  return axis_prepare(src, dst, nullptr, nullptr, nops, create, iorb, ispin, cplx_coef, who, tab);
}

int axisop_upload(edigpu_sector* dst, const AxisTables& tab, const double* cre, const double* cim, AxisArgs& a, hipStream_t st) {
  return axis_upload(dst, tab, cre, cim, a, st);
}

bool axisop_route(const edigpu_sector* src, const edigpu_sector* dst) {
  auto old_kind = [](const edigpu_sector* s) { return s->kind == kNormal && s->built_by_library && s->nph == 0; };
  return !(old_kind(src) && old_kind(dst));
}

int axisop_apply(edigpu_sector* src, edigpu_sector* dst, const double* v_src, double* v_dst, int nops, const double* cre,
                 const double* cim, const int32_t* create, const int32_t* iorb, const int32_t* ispin, hipStream_t st,
                 const char* who) {
  AxisTables tab;
  if (axis_prepare(src, dst, v_src, v_dst, nops, create, iorb, ispin, cim != nullptr, who, tab)) return 1;
  EDIGPU_HIP(hipSetDevice(src->device));
  return axis_call(dst, tab, cre, cim, v_src, v_dst, st);
}

}  // namespace edigpu

using namespace edigpu;

extern "C" {

int edigpu_apply_cops_normal_z(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev, int nops,
                               const double* coef_re_im, const int32_t* create, const int32_t* iorb, const int32_t* ispin,
                               void* stream) {
  const std::string who = "edigpu_apply_cops_normal_z";
  if (!src || !dst || !v_src_dev || !v_dst_dev || !coef_re_im || !create || !iorb || !ispin) {
    set_error(who + ": NULL argument");
    return 1;
  }
  if (nops < 1 || nops > kAxisMaxTerms) {
    set_error(who + ": nops must be 1 .. " + std::to_string(kAxisMaxTerms));
    return 1;
  }
  double cre[kAxisMaxTerms], cim[kAxisMaxTerms];
  for (int k = 0; k < nops; k++) {
    cre[k] = coef_re_im[2 * k];
    cim[k] = coef_re_im[2 * k + 1];
  }
  return axisop_apply(src, dst, v_src_dev, v_dst_dev, nops, cre, cim, create, iorb, ispin, (hipStream_t)stream, who.c_str());
}

int edigpu_time_apply_op(edigpu_handle src, edigpu_handle dst, const double* v_src_dev, double* v_dst_dev, int iorb, int ispin,
                         int create, int warmup, int steps, double* ms2) {
  const std::string who = "edigpu_time_apply_op";
  if (!src || !dst || !v_src_dev || !v_dst_dev || !ms2 || warmup < 0 || steps <= 0) {
    set_error(who + ": bad argument");
    return 1;
  }
  const bool axis = axisop_route(src, dst);
  const int32_t cr = create ? 1 : -1, io = iorb, sp = ispin;
  const double one = 1.0;
  AxisTables tab;
  AxisArgs a;
  hipStream_t st = src->stream;
  if (axis) {
    if (axis_prepare(src, dst, v_src_dev, v_dst_dev, 1, &cr, &io, &sp, false, who, tab)) return 1;
    EDIGPU_HIP(hipSetDevice(src->device));
    if (axis_upload(dst, tab, &one, nullptr, a, st)) return 1;
  } else {
    // the phonon-free real route keeps apply_op_normal_kernel: one warm call makes its checks, then the same table
    if (edigpu_apply_op_normal(src, dst, v_src_dev, v_dst_dev, iorb, ispin, create, st)) return 1;
    const AxisOp op{cr, io, sp};
    int nu = 0, nd = 0;
    const std::string why = axisop_build_normal(src->sec_a, src->sec_b, model_ns(src->model), src->model.norb, 1, false, 1, &op,
                                                nu, nd, tab);
    if (!why.empty()) {
      set_error(who + ": " + why);
      return 1;
    }
    EDIGPU_HIP(hipSetDevice(src->device));
    if (axis_upload(dst, tab, &one, nullptr, a, st)) return 1;
  }
  EDIGPU_HIP(hipStreamSynchronize(st));
  hipEvent_t e0, e1;
  EDIGPU_HIP(hipEventCreate(&e0));
  EDIGPU_HIP(hipEventCreate(&e1));
  int rc = 0;
  for (int which = 0; which < 2 && !rc; which++) {
    std::vector<float> ms((size_t)steps, 0.f);
    for (int k = 0; k < warmup + steps && !rc; k++) {
      rc |= hipEventRecord(e0, st) != hipSuccess;
      if (which == 0) {  // what a caller pays: the checks, the host table, its upload, the kernel, the wait
        rc |= edigpu_apply_op_normal(src, dst, v_src_dev, v_dst_dev, iorb, ispin, create, st);
      } else if (axis) {
        rc |= launch_apply_axisop(a, 0, v_src_dev, v_dst_dev, st);
      } else {
        rc |= launch_apply_op_normal(dst->dim_up, dst->dim_dw, src->dim_up, ispin, a.part, v_src_dev, v_dst_dev, st, 1.0, 0);
      }
      rc |= hipEventRecord(e1, st) != hipSuccess;
      rc |= hipEventSynchronize(e1) != hipSuccess;
      if (!rc && k >= warmup) rc |= hipEventElapsedTime(&ms[(size_t)(k - warmup)], e0, e1) != hipSuccess;
    }
    std::sort(ms.begin(), ms.end());
    ms2[which] = ms[ms.size() / 2];
    // the whole calls went through the scratch buffer: put this call's table back for the kernel-alone runs
    if (which == 0 && !rc) {
      rc |= axis_upload(dst, tab, &one, nullptr, a, st);
      rc |= hipStreamSynchronize(st) != hipSuccess;
    }
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
