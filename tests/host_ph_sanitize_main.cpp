// Stand-alone driver of csrc/host_ph.cpp for tests/test_host_ph_sanitizers.py: every function for norb = 1 .. 5 and
// DimPh = 2, 17, 32, built with -fsanitize=address,undefined and run as a program.  Every index a plan hands to the
// kernel is checked here the way the kernel uses it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_occ.hpp"
#include "host_ph.hpp"

using namespace edigpu;

static int failures = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);    \
      failures++;                                            \
    }                                                        \
  } while (0)

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// walks a plan as the Gram kernel does; every element must be visited once, in a unit of its class
static void walk(const PhPlan& pl, const std::vector<uint8_t>& cls_of_el) {
  const int64_t nel = pl.dim_rows * pl.dim_cols;
  std::vector<int> seen((size_t)nel, 0);
  CHECK((int64_t)pl.rorder.size() == pl.dim_rows && (int64_t)pl.corder.size() == pl.dim_cols);
  CHECK((int)pl.ubeg.size() == pl.ncls + 1 && pl.ubeg.front() == 0 && pl.ubeg.back() == (int)pl.units.size());
  for (size_t k = 0; k < pl.units.size(); k++) {
    const PhUnit& u = pl.units[k];
    CHECK(u.cls >= 0 && u.cls < pl.ncls && u.ncols > 0 && u.p0 < u.p1);
    CHECK((int)k >= pl.ubeg[(size_t)u.cls] && (int)k < pl.ubeg[(size_t)u.cls + 1]);
    for (int32_t p = u.p0; p < u.p1; p++) {
      const int64_t r = u.r0 + p / u.ncols, j = u.c0 + p % u.ncols;
      CHECK(r >= 0 && r < pl.dim_rows && j >= 0 && j < pl.dim_cols);
      if (r < 0 || r >= pl.dim_rows || j < 0 || j >= pl.dim_cols) return;
      const int64_t e = (int64_t)pl.rorder[(size_t)r] * pl.dim_cols + pl.corder[(size_t)j];
      CHECK(e >= 0 && e < nel);
      if (e < 0 || e >= nel) return;
      seen[(size_t)e]++;
      CHECK(cls_of_el[(size_t)e] == u.cls);
    }
  }
  for (int64_t e = 0; e < nel; e++) CHECK(seen[(size_t)e] == 1);
}

int main() {
  uint32_t s = 12345u;
  for (int norb = 1; norb <= 5; norb++) {
    const int npat = 1 << norb, ncls = ph_num_classes(norb);
    uint16_t cls[kOccMaxPat];
    ph_class_word(norb, cls);
    CHECK(cls[0] == 0 && 2 * cls[npat - 1] == ncls - 1);
    for (int64_t dim_up : {1, 7, 70}) {
      for (int64_t dim_dw : {1, 5, 33}) {
        std::vector<uint16_t> pu((size_t)dim_up), pd((size_t)dim_dw);
        for (auto& x : pu) x = (uint16_t)(rnd(s) >> 8) % npat;
        for (auto& x : pd) x = (uint16_t)(rnd(s) >> 8) % npat;
        std::vector<uint8_t> ce((size_t)(dim_up * dim_dw));
        for (int64_t e = 0; e < dim_up * dim_dw; e++) ce[(size_t)e] = (uint8_t)(cls[pu[(size_t)(e % dim_up)]] + cls[pd[(size_t)(e / dim_up)]]);
        for (int64_t target : {1, 13, 2048}) {
          PhPlan pl;
          ph_plan_normal(pu.data(), dim_up, pd.data(), dim_dw, norb, target, pl);
          CHECK(pl.ncls == ncls);
          walk(pl, ce);
        }
      }
    }
    for (int64_t dim_el : {1, 64, 1000}) {
      std::vector<uint16_t> pat((size_t)dim_el);
      for (auto& x : pat) x = (uint16_t)((rnd(s) >> 8) % (uint32_t)(npat * npat));
      std::vector<uint8_t> ce((size_t)dim_el);
      ph_class_rows(pat.data(), dim_el, norb, ce.data());
      std::vector<int32_t> order, run;
      ph_sort_keys(ce.data(), dim_el, ncls, order, run);
      CHECK((int64_t)order.size() == dim_el && (int)run.size() == ncls + 1 && run.back() == dim_el);
      for (int64_t target : {1, 50}) {
        PhPlan pl;
        ph_plan_flat(pat.data(), dim_el, norb, target, pl);
        walk(pl, ce);
      }
    }
  }
  for (int dimph : {2, 17, 32}) {
    std::vector<double> sq((size_t)dimph + 1);
    ph_sqrt_table(dimph, sq.data());
    CHECK(sq[0] == 0.0 && sq[1] == 1.0 && sq[(size_t)dimph] * sq[(size_t)dimph] > dimph - 1e-9);
    for (int cw = 1; cw <= 2; cw++) {
      const int ns = ph_slots(dimph);
      std::vector<double> slots((size_t)ns * cw), rho((size_t)dimph * dimph * cw, -1.0);
      for (auto& x : slots) x = (double)(rnd(s) >> 8) / 65536.0;
      for (int n = 0; n < dimph; n++)
        for (int m = n; m < dimph; m++) CHECK(ph_slot(dimph, n, m) >= 0 && ph_slot(dimph, n, m) < ns);
      CHECK(ph_slot(dimph, dimph - 1, dimph - 1) == ns - 1);
      const double tr = ph_expand_slots(slots.data(), dimph, cw, rho.data());
      double t2 = 0.0;
      for (int n = 0; n < dimph; n++) {
        t2 += rho[((size_t)n * dimph + n) * cw];
        for (int m = 0; m < dimph; m++) {
          CHECK(rho[((size_t)n * dimph + m) * cw] == rho[((size_t)m * dimph + n) * cw]);
          if (cw == 2) CHECK(rho[((size_t)n * dimph + m) * 2 + 1] == -rho[((size_t)m * dimph + n) * 2 + 1]);
        }
      }
      CHECK(tr == t2);
    }
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
