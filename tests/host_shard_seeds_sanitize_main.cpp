// Stand-alone driver for tests/test_shard_src_host.py::test_emulation_under_asan_ubsan: the host emulation of the window +
// source kernels (tests/host_shard_seeds.hpp, csrc/shard_src.hpp) on the library's own host tables (csrc/host_axisop.cpp,
// csrc/host_pairs.cpp), for worlds of 1 - 12 ranks, against a plain whole-vector loop.  Every buffer has its exact size, so
// an index outside a gathered vector, a table or a shard is an AddressSanitizer report; the padding of a gathered vector
// holds a huge number, so a read from it shows in the sums.  Prints "<n> checks, <m> failures".
#include <cstdio>
#include <vector>

#include "host_axisop.hpp"
#include "host_pairs.hpp"
#include "host_shard_seeds.hpp"

using namespace edigpu;
using namespace seeds_emul;

static int checks = 0, failures = 0;

static void expect(bool ok, const char* what, int world) {
  checks++;
  if (!ok) {
    failures++;
    std::printf("FAIL %s world %d\n", what, world);
  }
}

static std::vector<double> int_vector(size_t n, unsigned seed) {
  std::vector<double> v(n);
  unsigned x = seed * 2654435761u + 12345u;
  for (size_t k = 0; k < n; k++) {
    x = x * 1664525u + 1013904223u;
    v[k] = (double)((int)((x >> 16) % 19u) - 9);
  }
  return v;
}

// down operators of a normal-mode phonon sector: [nblk][DimDw][DimUp (x 2)]
static void axis_case(int nup, int ndw, int ns, int norb, int nblk, bool cplx, std::vector<AxisOp> ops, std::vector<double> coef) {
  AxisTables tab;
  int nu = 0, nd = 0;
  const std::string why = axisop_build_normal(nup, ndw, ns, norb, nblk, cplx, (int)ops.size(), ops.data(), nu, nd, tab);
  expect(why.empty() && tab.O == nblk, "axis tables", 0);
  if (!why.empty()) return;
  const std::vector<double> whole = int_vector((size_t)(tab.O * tab.a_src * tab.I), 3u + (unsigned)nup);
  std::vector<double> ref((size_t)(tab.O * tab.a_dst * tab.I));
  for (int64_t o = 0; o < tab.O; o++)
    for (int64_t j = 0; j < tab.a_dst; j++)
      for (int64_t i = 0; i < tab.I; i++) {
        double acc = 0.0;
        for (int t = 0; t < tab.nterms; t++) {
          const uint32_t p = tab.part[(size_t)(t * tab.a_dst + j)];
          double x = 0.0;
          if (p != kNone) x = ((p >> 31) ? -1.0 : 1.0) * whole[(size_t)((o * tab.a_src + (p & kIdx)) * tab.I + i)];
          acc = t == 0 ? coef[0] * x : coef[(size_t)t] * x + acc;
        }
        ref[(size_t)((o * tab.a_dst + j) * tab.I + i)] = acc;
      }
  for (int world : {1, 2, 3, 5, 10, 12}) {
    ShardSrc s;
    const std::vector<double> g = gather(whole.data(), tab.a_src, tab.I, nblk, world, 1.0e300, s);
    std::vector<double> got(ref.size(), -7777.0);
    for (int r = 0; r < world; r++) {
      int64_t first, count, q;
      plan(tab.a_dst, world, r, first, count, q);
      std::vector<double> out((size_t)(nblk * count * tab.I));
      axis_window(tab.nterms, tab.part.data(), coef.data(), tab.O, tab.a_dst, tab.I, first, count, s, g.data(), out.data());
      for (int p = 0; p < nblk; p++)
        for (int64_t k = 0; k < count * tab.I; k++)
          got[(size_t)((p * tab.a_dst + first) * tab.I + k)] = out[(size_t)(p * count * tab.I + k)];
    }
    expect(got == ref, "axis window", world);
  }
}

static void pairs_case(int nup, int ndw, int ns, int norb, int nblk, std::vector<PairsTerm> terms) {
  PairsTables tab;
  const std::string why = pairs_build(nup, ndw, ns, norb, (int)terms.size(), terms.data(), tab);
  expect(why.empty(), "pairs tables", 0);
  if (!why.empty()) return;
  const int64_t du_s = tab.dim_up_src, dd_s = tab.dim_dw_src, du_d = tab.dim_up_dst, dd_d = tab.dim_dw_dst;
  const std::vector<double> whole = int_vector((size_t)(nblk * dd_s * du_s), 11u + (unsigned)ndw);
  std::vector<double> ref((size_t)(nblk * dd_d * du_d));
  for (int p = 0; p < nblk; p++)
    for (int64_t jd = 0; jd < dd_d; jd++)
      for (int64_t ju = 0; ju < du_d; ju++) {
        double acc = 0.0;
        for (int t = 0; t < tab.nterms; t++) {
          const uint32_t d = ((tab.id_dw >> t) & 1u) ? (uint32_t)jd : tab.dw[(size_t)(t * dd_d + jd)];
          const uint32_t u = ((tab.id_up >> t) & 1u) ? (uint32_t)ju : tab.up[(size_t)(t * du_d + ju)];
          if (d == kNone || u == kNone) continue;
          const double y = whole[(size_t)((p * dd_s + (d & kIdx)) * du_s + (u & kIdx))];
          acc = tab.coef[t] * (((u ^ d) >> 31) ? -y : y) + acc;
        }
        ref[(size_t)((p * dd_d + jd) * du_d + ju)] = acc;
      }
  for (int world : {1, 2, 3, 5, 10, 12}) {
    ShardSrc s;
    const std::vector<double> g = gather(whole.data(), dd_s, du_s, nblk, world, 1.0e300, s);
    std::vector<double> got(ref.size(), -7777.0);
    for (int r = 0; r < world; r++) {
      int64_t first, count, q;
      plan(dd_d, world, r, first, count, q);
      std::vector<double> out((size_t)(nblk * count * du_d));
      pairs_window(tab.nterms, tab.up.data(), tab.dw.data(), tab.id_up, tab.id_dw, tab.coef, nblk, du_d, dd_d, first, count, s,
                   g.data(), out.data());
      for (int p = 0; p < nblk; p++)
        for (int64_t k = 0; k < count * du_d; k++)
          got[(size_t)((p * dd_d + first) * du_d + k)] = out[(size_t)(p * count * du_d + k)];
    }
    expect(got == ref, "pairs window", world);
  }
}

// c of one level on the states of 2 ns bits with ntot set (down word major), complex elements
static void flat_case(int ns, int ntot, int level, int nblk) {
  std::vector<int32_t> src, dst, off_dw((size_t)1 << ns, 0), rk_up((size_t)1 << ns, 0);
  std::vector<int> seen((size_t)1 << ns, 0), cnt((size_t)ns + 1, 0);
  for (int32_t t = 0; t < (1 << (2 * ns)); t++) {
    const int n = __builtin_popcount((unsigned)t);
    if (n == ntot) {
      if (!seen[(size_t)(t >> ns)]) {
        seen[(size_t)(t >> ns)] = 1;
        off_dw[(size_t)(t >> ns)] = (int32_t)src.size();
      }
      src.push_back(t);
    }
    if (n == ntot - 1) dst.push_back(t);
  }
  for (int w = 0; w < (1 << ns); w++) rk_up[(size_t)w] = cnt[(size_t)__builtin_popcount((unsigned)w)]++;
  const uint32_t bit = 1u << level, lomask = (1u << ns) - 1u;
  const int64_t ns_el = (int64_t)src.size(), nd_el = (int64_t)dst.size();
  const std::vector<double> whole = int_vector((size_t)(2 * nblk * ns_el), 29u);
  std::vector<double> ref((size_t)(2 * nblk * nd_el), 0.0);
  const double cre = 2.0, cim = -1.0;
  for (int p = 0; p < nblk; p++)
    for (int64_t k = 0; k < nd_el; k++) {
      const uint32_t t = (uint32_t)dst[(size_t)k];
      if (t & bit) continue;
      const uint32_t sst = t | bit;
      const int64_t i = off_dw[sst >> ns] + rk_up[sst & lomask];
      const double sg = (__builtin_popcount(sst & (bit - 1u)) & 1) ? -1.0 : 1.0;
      const double xr = sg * whole[(size_t)(2 * (p * ns_el + i))], xi = sg * whole[(size_t)(2 * (p * ns_el + i) + 1)];
      ref[(size_t)(2 * (p * nd_el + k))] = cre * xr - cim * xi;
      ref[(size_t)(2 * (p * nd_el + k) + 1)] = cre * xi + cim * xr;
    }
  for (int world : {1, 2, 3, 5, 10, 12}) {
    ShardSrc s2;
    const std::vector<double> g = gather(whole.data(), ns_el, 2, nblk, world, 1.0e300, s2);
    const ShardSrc s = shard_src_in_pairs(s2);
    std::vector<double> got(ref.size(), -7777.0);
    for (int r = 0; r < world; r++) {
      int64_t first, count, q;
      plan(nd_el, world, r, first, count, q);
      std::vector<double> out((size_t)(2 * nblk * count));
      std::vector<int32_t> st(dst.begin() + first, dst.begin() + first + count);
      flat_window(count, nblk, ns, bit, 0, st.data(), off_dw.data(), rk_up.data(), s, g.data(), cre, cim, 0, out.data());
      for (int p = 0; p < nblk; p++)
        for (int64_t k = 0; k < 2 * count; k++) got[(size_t)(2 * (p * nd_el + first) + k)] = out[(size_t)(2 * p * count + k)];
    }
    expect(got == ref, "flat window", world);
  }
}

int main() {
  // Ns = 6 (Norb 2): (3, 3) -> (3, 2), two c_dw terms, four phonon blocks; the same as interleaved complex vectors
  axis_case(3, 3, 6, 2, 4, false, {AxisOp{-1, 0, 1}, AxisOp{-1, 1, 1}}, {1.0, -2.0});
  axis_case(3, 3, 6, 2, 4, true, {AxisOp{-1, 0, 1}, AxisOp{-1, 1, 1}}, {1.0, -2.0});
  axis_case(2, 1, 6, 2, 1, false, {AxisOp{1, 1, 1}}, {3.0});  // c^+_dw, no phonons, a_src = 6 rows
  // pair seed of two orbitals (each term c_up c_dw), the spin-summed exciton channel (up-up + down-down), a down-only term
  pairs_case(3, 3, 6, 2, 3, {PairsTerm{1.0, {-1, 0, 1}, {-1, 0, 0}}, PairsTerm{1.0, {-1, 1, 1}, {-1, 1, 0}}});
  pairs_case(3, 3, 6, 2, 1, {PairsTerm{1.0, {-1, 1, 0}, {1, 0, 0}}, PairsTerm{-1.0, {-1, 1, 1}, {1, 0, 1}}});
  pairs_case(2, 3, 6, 2, 2, {PairsTerm{2.0, {-1, 1, 1}, {1, 0, 1}}});
  flat_case(3, 3, 1, 4);
  flat_case(3, 4, 3 + 2, 1);
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
