// host_ph.cpp -- host tables of the phonon operators (host_ph.hpp).
#include "host_ph.hpp"

#include <algorithm>
#include <cmath>

#include "host_occ.hpp"

namespace edigpu {

int ph_num_classes(int norb) {
  int n = 1;
  for (int a = 0; a < norb; a++) n *= 3;
  return n;
}

void ph_class_word(int norb, uint16_t* cls) {
  for (int p = 0; p < (1 << norb); p++) {
    int c = 0, w = 1;
    for (int a = 0; a < norb; a++, w *= 3)
      if ((p >> a) & 1) c += w;
    cls[p] = (uint16_t)c;
  }
}

void ph_class_rows(const uint16_t* pat, int64_t n, int norb, uint8_t* out) {
  uint16_t cls[kOccMaxPat];
  ph_class_word(norb, cls);
  const uint32_t mask = (1u << norb) - 1u;
  for (int64_t i = 0; i < n; i++) out[i] = (uint8_t)(cls[pat[i] & mask] + cls[(pat[i] >> norb) & mask]);
}

void ph_sqrt_table(int dimph, double* sq) {
  for (int n = 0; n <= dimph; n++) sq[n] = std::sqrt((double)n);
}

void ph_sort_keys(const uint8_t* key, int64_t n, int nkeys, std::vector<int32_t>& order, std::vector<int32_t>& run) {
  run.assign((size_t)nkeys + 1, 0);
  for (int64_t i = 0; i < n; i++) run[(size_t)key[i] + 1]++;
  for (int c = 0; c < nkeys; c++) run[(size_t)c + 1] += run[(size_t)c];
  std::vector<int32_t> next(run.begin(), run.end() - 1);
  order.assign((size_t)n, 0);
  for (int64_t i = 0; i < n; i++) order[(size_t)next[key[i]]++] = (int32_t)i;
}

namespace {

// the block rows [r0, r0 + nrows) x columns [c0, c0 + ncols) of one class, cut into equal position ranges
void add_units(int32_t r0, int64_t nrows, int32_t c0, int64_t ncols, int cls, int64_t target, std::vector<PhUnit>& units) {
  const int64_t total = nrows * ncols;
  if (total <= 0) return;
  const int64_t nu = std::max<int64_t>(1, (total + target - 1) / std::max<int64_t>(target, 1));
  for (int64_t k = 0; k < nu; k++) {
    const int64_t a = total * k / nu, b = total * (k + 1) / nu;
    if (a < b) units.push_back({r0, c0, (int32_t)ncols, cls, (int32_t)a, (int32_t)b});
  }
}

void finish_plan(PhPlan& plan) {
  std::stable_sort(plan.units.begin(), plan.units.end(), [](const PhUnit& x, const PhUnit& y) { return x.cls < y.cls; });
  plan.ubeg.assign((size_t)plan.ncls + 1, 0);
  for (const PhUnit& u : plan.units) plan.ubeg[(size_t)u.cls + 1]++;
  for (int c = 0; c < plan.ncls; c++) plan.ubeg[(size_t)c + 1] += plan.ubeg[(size_t)c];
}

}  // namespace

void ph_plan_normal(const uint16_t* pu, int64_t dim_up, const uint16_t* pd, int64_t dim_dw, int norb, int64_t target,
                    PhPlan& plan) {
  plan = PhPlan();
  plan.ncls = ph_num_classes(norb);
  plan.dim_rows = dim_dw;
  plan.dim_cols = dim_up;
  uint16_t cls[kOccMaxPat];
  ph_class_word(norb, cls);
  std::vector<uint8_t> ku(pu, pu + dim_up), kd(pd, pd + dim_dw);
  int32_t run_u[kOccMaxPat + 1], run_d[kOccMaxPat + 1];
  occ_sort_rows(ku.data(), dim_up, 1, plan.corder, run_u);
  occ_sort_rows(kd.data(), dim_dw, 1, plan.rorder, run_d);
  const int npat = 1 << norb;
  for (int d = 0; d < npat; d++)
    for (int u = 0; u < npat; u++)
      add_units(run_d[d], run_d[d + 1] - run_d[d], run_u[u], run_u[u + 1] - run_u[u], cls[u] + cls[d], target, plan.units);
  finish_plan(plan);
}

void ph_plan_flat(const uint16_t* pat, int64_t dim_el, int norb, int64_t target, PhPlan& plan) {
  plan = PhPlan();
  plan.ncls = ph_num_classes(norb);
  plan.dim_rows = 1;
  plan.dim_cols = dim_el;
  std::vector<uint8_t> key((size_t)dim_el);
  ph_class_rows(pat, dim_el, norb, key.data());
  std::vector<int32_t> run;
  ph_sort_keys(key.data(), dim_el, plan.ncls, plan.corder, run);
  plan.rorder.assign(1, 0);
  for (int c = 0; c < plan.ncls; c++) add_units(0, 1, run[(size_t)c], run[(size_t)c + 1] - run[(size_t)c], c, target, plan.units);
  finish_plan(plan);
}

namespace {
void cut_range(int64_t n, int64_t& first, int64_t& count) {
  first = std::max<int64_t>(0, std::min(first, n));
  count = std::max<int64_t>(0, std::min(count, n - first));
}
}  // namespace

void ph_shard_plan_normal(const uint16_t* pu, int64_t dim_up, const uint16_t* pd, int64_t dim_dw, int64_t first, int64_t count,
                          int norb, int64_t target, PhPlan& plan) {
  cut_range(dim_dw, first, count);
  ph_plan_normal(pu, dim_up, pd + first, count, norb, target, plan);
}

void ph_shard_plan_flat(const uint16_t* pat, int64_t dim_el, int64_t first, int64_t count, int norb, int64_t target,
                        PhPlan& plan) {
  cut_range(dim_el, first, count);
  ph_plan_flat(pat + first, count, norb, target, plan);
}

double ph_expand_slots(const double* slots, int dimph, int cw, double* rho) {
  double tr = 0.0;
  for (int n = 0; n < dimph; n++)
    for (int m = n; m < dimph; m++) {
      const double* s = slots + (size_t)ph_slot(dimph, n, m) * cw;
      double* up = rho + ((size_t)n * dimph + m) * cw;
      double* lo = rho + ((size_t)m * dimph + n) * cw;
      up[0] = lo[0] = s[0];
      if (cw == 2) {
        up[1] = n == m ? 0.0 : s[1];
        lo[1] = n == m ? 0.0 : -s[1];
      }
      if (n == m) tr += s[0];
    }
  return tr;
}

}  // namespace edigpu
