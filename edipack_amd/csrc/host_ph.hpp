// host_ph.hpp -- host tables of the phonon operators (edigpu_apply_xph, edigpu_ph_rdm).  No HIP in here: tests/host_ph.cpp
// compiles this with g++.
//
// A phonon vector is DimPh = nph + 1 blocks of dim_el electronic elements, i = i_el + n dim_el.  The phonon reduced
// density matrix is resolved by the impurity occupation class of i_el, the reference's val - 1
// (ED_OBSERVABLES_NORMAL.f90:202-213): class = sum_a nt_a 3^a, nt_a = n_{a,up} + n_{a,dw}.  The class of a normal-mode
// element is cls[up pattern] + cls[down pattern], cls[p] = sum_a bit_a(p) 3^a; the patterns are those of host_occ.hpp.
#pragma once
#include <cstdint>
#include <vector>

namespace edigpu {

constexpr int kPhMaxDim = 32;   // largest DimPh edigpu_ph_rdm accepts
constexpr int kPhMaxCls = 243;  // 3^EDIGPU_MAXORB

// 3^norb
int ph_num_classes(int norb);
// cls[p] = sum_a bit_a(p) 3^a for the 2^norb patterns of one spin word
void ph_class_word(int norb, uint16_t* cls);
// out[i] = class of the flat row whose pattern is pat[i] = up | down << norb (occ_patterns_state)
void ph_class_rows(const uint16_t* pat, int64_t n, int norb, uint8_t* out);
// sq[n] = std::sqrt((double)n), n = 0 .. dimph: the coefficients of b + b^dagger
void ph_sqrt_table(int dimph, double* sq);
// stable counting sort of n keys < nkeys: order[k] = k-th index, run[c] .. run[c + 1] = the positions of key c
void ph_sort_keys(const uint8_t* key, int64_t n, int nkeys, std::vector<int32_t>& order, std::vector<int32_t>& run);

// One work unit of the Gram kernel: a range [p0, p1) of the positions of (a run of rows) x (a run of columns), all of one
// class.  Position p is the sorted row r0 + p / ncols and the sorted column c0 + p % ncols; the electronic index of the
// element is rorder[row] * dim_cols + corder[column].
struct PhUnit {
  int32_t r0, c0, ncols, cls, p0, p1;
};
struct PhPlan {
  int ncls = 0;
  int64_t dim_rows = 1, dim_cols = 0;
  std::vector<int32_t> rorder, corder;  // rows sorted by down pattern, columns by up pattern (flat: one row, columns by class)
  std::vector<PhUnit> units;            // sorted by class, stable: the order in which the partial sums of a class are added
  std::vector<int32_t> ubeg;            // ncls + 1: the units of class c
};
// normal mode: pu[dim_up], pd[dim_dw] (occ_patterns_word); a (down run) x (up run) block is cut into units of about
// `target` elements.  dim_up * dim_dw < 2^31.
void ph_plan_normal(const uint16_t* pu, int64_t dim_up, const uint16_t* pd, int64_t dim_dw, int norb, int64_t target,
                    PhPlan& plan);
// superc / nonsu2: pat[dim_el] (occ_patterns_state)
void ph_plan_flat(const uint16_t* pat, int64_t dim_el, int norb, int64_t target, PhPlan& plan);

// The plan of a rank's rows [first, first + count) of a sector (edigpu_ph_rdm_sharded), the range cut to the sector: the
// down rows pd[first ..] of normal mode (dim_rows = the rows left, the columns are the sector's own), the states
// pat[first ..] of a superc / nonsu2 sector (dim_cols = the states left).  Indices are local to the shard; a rank past the
// last row gets a plan without units.
void ph_shard_plan_normal(const uint16_t* pu, int64_t dim_up, const uint16_t* pd, int64_t dim_dw, int64_t first, int64_t count,
                          int norb, int64_t target, PhPlan& plan);
void ph_shard_plan_flat(const uint16_t* pat, int64_t dim_el, int64_t first, int64_t count, int norb, int64_t target,
                        PhPlan& plan);

// slots of the upper triangle n <= m of a DimPh x DimPh matrix, row-major
inline int ph_slots(int dimph) { return dimph * (dimph + 1) / 2; }
inline int ph_slot(int dimph, int n, int m) { return n * dimph - n * (n - 1) / 2 + (m - n); }
// slots[ph_slots * cw] (cw = 2: interleaved re, im of sum v_n conj v_m, n <= m) -> rho[dimph][dimph] (* cw), the lower
// triangle mirrored (conjugated), the imaginary part of the diagonal exactly 0.  Returns the trace.
double ph_expand_slots(const double* slots, int dimph, int cw, double* rho);

}  // namespace edigpu
