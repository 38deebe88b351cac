// ctypes shim over csrc/host_ph.cpp for tests/test_ph_host.py (compiled with g++, no HIP).
#include "host_ph.hpp"

#include <cstring>
#include <vector>

using namespace edigpu;

namespace {

// rorder: dim_rows, corder: dim_cols, units: 6 * max_units int32, ubeg: ncls + 1; returns the units made, -1 past max_units
int copy_plan(const PhPlan& p, int32_t* rorder, int32_t* corder, int32_t* units, int max_units, int32_t* ubeg) {
  if ((int)p.units.size() > max_units) return -1;
  std::memcpy(rorder, p.rorder.data(), p.rorder.size() * sizeof(int32_t));
  if (!p.corder.empty()) std::memcpy(corder, p.corder.data(), p.corder.size() * sizeof(int32_t));
  static_assert(sizeof(PhUnit) == 6 * sizeof(int32_t), "PhUnit is six int32");
  if (!p.units.empty()) std::memcpy(units, p.units.data(), p.units.size() * sizeof(PhUnit));
  std::memcpy(ubeg, p.ubeg.data(), p.ubeg.size() * sizeof(int32_t));
  return (int)p.units.size();
}

}  // namespace

extern "C" {

int hp_num_classes(int norb) { return ph_num_classes(norb); }
void hp_class_word(int norb, uint16_t* cls) { ph_class_word(norb, cls); }
void hp_class_rows(const uint16_t* pat, int64_t n, int norb, uint8_t* out) { ph_class_rows(pat, n, norb, out); }
void hp_sqrt_table(int dimph, double* sq) { ph_sqrt_table(dimph, sq); }

// order: n entries, run: nkeys + 1
void hp_sort_keys(const uint8_t* key, int64_t n, int nkeys, int32_t* order, int32_t* run) {
  std::vector<int32_t> o, r;
  ph_sort_keys(key, n, nkeys, o, r);
  if (!o.empty()) std::memcpy(order, o.data(), o.size() * sizeof(int32_t));
  std::memcpy(run, r.data(), r.size() * sizeof(int32_t));
}

int hp_plan_normal(const uint16_t* pu, int64_t dim_up, const uint16_t* pd, int64_t dim_dw, int norb, int64_t target,
                   int32_t* rorder, int32_t* corder, int32_t* units, int max_units, int32_t* ubeg) {
  PhPlan p;
  ph_plan_normal(pu, dim_up, pd, dim_dw, norb, target, p);
  return copy_plan(p, rorder, corder, units, max_units, ubeg);
}

int hp_plan_flat(const uint16_t* pat, int64_t dim_el, int norb, int64_t target, int32_t* rorder, int32_t* corder,
                 int32_t* units, int max_units, int32_t* ubeg) {
  PhPlan p;
  ph_plan_flat(pat, dim_el, norb, target, p);
  return copy_plan(p, rorder, corder, units, max_units, ubeg);
}

int hp_slots(int dimph) { return ph_slots(dimph); }
int hp_slot(int dimph, int n, int m) { return ph_slot(dimph, n, m); }
double hp_expand_slots(const double* slots, int dimph, int cw, double* rho) { return ph_expand_slots(slots, dimph, cw, rho); }

}  // extern "C"
