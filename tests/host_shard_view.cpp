// ctypes shim over the shard views of csrc/host_occ.cpp and csrc/host_ph.cpp for tests/test_shard_views_host.py (compiled
// with g++, no HIP).
#include <cstring>
#include <vector>

#include "host_occ.hpp"
#include "host_ph.hpp"

using namespace edigpu;

namespace {
template <class T>
void copy_out(const std::vector<T>& v, T* out) {
  if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
}

// dims: dim_rows, dim_cols, units; the arrays hold at least the sector's rows / columns / units_cap units of 6 ints
int plan_out(const PhPlan& pl, int64_t* dims, int32_t* rorder, int32_t* corder, int32_t* units, int units_cap, int32_t* ubeg) {
  dims[0] = pl.dim_rows;
  dims[1] = pl.dim_cols;
  dims[2] = (int64_t)pl.units.size();
  if ((int)pl.units.size() > units_cap) return 1;
  copy_out(pl.rorder, rorder);
  copy_out(pl.corder, corder);
  copy_out(pl.ubeg, ubeg);
  for (size_t k = 0; k < pl.units.size(); k++) {
    const PhUnit& u = pl.units[k];
    const int32_t six[6] = {u.r0, u.c0, u.ncols, u.cls, u.p0, u.p1};
    std::memcpy(units + 6 * k, six, sizeof(six));
  }
  return 0;
}
}  // namespace

extern "C" {

// range: first, count after the cut; pu / pd: `count` entries at most (whichever the mode fills); order: count * nblk;
// run: 33.  Returns the entries of order.
int64_t hsv_occ_view(const uint16_t* pat, int64_t n, int flat, int nblk, int64_t first, int64_t count, int64_t* range,
                     uint16_t* pu, uint8_t* pd, int32_t* order, int32_t* run) {
  OccShardView v;
  occ_shard_view(pat, n, flat != 0, nblk, first, count, v);
  range[0] = v.first;
  range[1] = v.count;
  range[2] = (int64_t)v.pu.size();
  range[3] = (int64_t)v.pd.size();
  copy_out(v.pu, pu);
  copy_out(v.pd, pd);
  copy_out(v.order, order);
  std::memcpy(run, v.run, sizeof(v.run));
  return (int64_t)v.order.size();
}

int hsv_ph_plan_normal(const uint16_t* pu, int64_t dim_up, const uint16_t* pd, int64_t dim_dw, int64_t first, int64_t count, int norb,
                       int64_t target, int64_t* dims, int32_t* rorder, int32_t* corder, int32_t* units, int units_cap,
                       int32_t* ubeg) {
  PhPlan pl;
  ph_shard_plan_normal(pu, dim_up, pd, dim_dw, first, count, norb, target, pl);
  return plan_out(pl, dims, rorder, corder, units, units_cap, ubeg);
}

int hsv_ph_plan_flat(const uint16_t* pat, int64_t dim_el, int64_t first, int64_t count, int norb, int64_t target, int64_t* dims,
                     int32_t* rorder, int32_t* corder, int32_t* units, int units_cap, int32_t* ubeg) {
  PhPlan pl;
  ph_shard_plan_flat(pat, dim_el, first, count, norb, target, pl);
  return plan_out(pl, dims, rorder, corder, units, units_cap, ubeg);
}

}  // extern "C"
