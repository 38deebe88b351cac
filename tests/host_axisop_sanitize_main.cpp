// Stand-alone driver of csrc/host_axisop.cpp for tests/test_axisop_host_sanitizers.py: the table builds of every operator on
// every sector of Ns = 4 (ed_total_ud=T; real and complex vectors, one and three phonon blocks) and of chains of
// 1 + Nbath = 4 and 5 levels (ed_total_ud=F; one and two orbitals), multi-term calls up to the cap, the refusals, and one
// larger basis, built with -fsanitize=address,undefined and run as a program.  Every index a table hands to the kernel is
// checked here the way the kernel uses it, and every live entry is checked by applying the operator forwards.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_axisop.hpp"
#include "host_pairs.hpp"

using namespace edigpu;

static int failures = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);    \
      failures++;                                            \
    }                                                        \
  } while (0)

static std::vector<uint32_t> words(int nlev, int n) {
  std::vector<uint32_t> w;
  for (uint32_t x = 0; x < (1u << nlev); x++)
    if (__builtin_popcount(x) == n) w.push_back(x);
  return w;
}

// one table against the forward application on the source words
static void check_table(const uint32_t* tab, const std::vector<uint32_t>& ws, const std::vector<uint32_t>& wd, int level,
                        bool create, bool counted) {
  const uint32_t bit = 1u << level;
  int64_t live = 0, want = 0;
  for (size_t j = 0; j < wd.size(); j++) {
    if (tab[j] == kAxisNone) continue;
    live++;
    const size_t i = tab[j] & 0x7FFFFFFFu;
    CHECK(i < ws.size());  // what the kernel indexes the source axis with
    if (i >= ws.size()) continue;
    const uint32_t w = ws[i];
    CHECK(((w & bit) != 0u) != create && (w ^ bit) == wd[j]);
    const bool minus = counted && (__builtin_popcount(w & (bit - 1u)) & 1);
    CHECK(minus == ((tab[j] >> 31) != 0u));
  }
  for (uint32_t w : ws)
    if (((w & bit) != 0u) != create) want++;  // every source word the operator does not kill has its entry
  CHECK(live == want);
}

static void check_normal(int nup, int ndw, int ns, int norb, int nblk, bool cplx, const std::vector<AxisOp>& ops) {
  AxisTables t;
  int nu = -1, nd = -1;
  const std::string why = axisop_build_normal(nup, ndw, ns, norb, nblk, cplx, (int)ops.size(), ops.data(), nu, nd, t);
  const int spin = ops[0].ispin, d = ops[0].create > 0 ? 1 : -1;
  const int n_src = spin == 0 ? nup : ndw, n_dst = n_src + d;
  if (n_dst < 0 || n_dst > ns) {
    CHECK(!why.empty());
    return;
  }
  CHECK(why.empty());
  if (!why.empty()) return;
  CHECK(nu == (spin == 0 ? n_dst : nup) && nd == (spin == 1 ? n_dst : ndw));
  const int64_t du = pairs_dim(ns, nup), dd = pairs_dim(ns, ndw), w = cplx ? 2 : 1;
  CHECK(t.nterms == (int)ops.size() && t.a_src == pairs_dim(ns, n_src) && t.a_dst == pairs_dim(ns, n_dst));
  CHECK(t.I == (spin == 0 ? w : w * du) && t.O == (spin == 0 ? dd * nblk : (int64_t)nblk));
  CHECK(t.I * t.a_src * t.O == w * du * dd * nblk);
  CHECK((int64_t)t.part.size() == t.nterms * t.a_dst);
  const std::vector<uint32_t> ws = words(ns, n_src), wd = words(ns, n_dst);
  for (int k = 0; k < t.nterms; k++)
    check_table(t.part.data() + (size_t)k * (size_t)t.a_dst, ws, wd, ops[(size_t)k].iorb, d > 0, true);
}

static void check_orbs(int norb, int nbath, const std::vector<int>& nups, const std::vector<int>& ndws,
                       const std::vector<AxisOp>& ops) {
  const int nlev = 1 + nbath;
  AxisTables t;
  std::vector<int> u2((size_t)norb, -7), d2((size_t)norb, -7);
  const std::string why = axisop_build_orbs(norb, nbath, nups.data(), ndws.data(), (int)ops.size(), ops.data(), u2.data(),
                                            d2.data(), t);
  const int iorb = ops[0].iorb, spin = ops[0].ispin, d = ops[0].create > 0 ? 1 : -1;
  const int n_src = (spin == 0 ? nups : ndws)[(size_t)iorb], n_dst = n_src + d;
  if (n_dst < 0 || n_dst > nlev) {
    CHECK(!why.empty());
    return;
  }
  CHECK(why.empty());
  if (!why.empty()) return;
  int64_t I = 1, O = 1;
  const int axis = iorb + spin * norb;
  for (int k = 0; k < 2 * norb; k++) {
    const int n = k < norb ? nups[(size_t)k] : ndws[(size_t)(k - norb)];
    if (k < axis) I *= pairs_dim(nlev, n);
    if (k > axis) O *= pairs_dim(nlev, n);
    CHECK((k < norb ? u2[(size_t)k] : d2[(size_t)(k - norb)]) == (k == axis ? n_dst : n));
  }
  CHECK(t.I == I && t.O == O && t.a_src == pairs_dim(nlev, n_src) && t.a_dst == pairs_dim(nlev, n_dst));
  CHECK((int64_t)t.part.size() == t.nterms * t.a_dst);
  const std::vector<uint32_t> ws = words(nlev, n_src), wd = words(nlev, n_dst);
  for (int k = 0; k < t.nterms; k++) check_table(t.part.data() + (size_t)k * (size_t)t.a_dst, ws, wd, 0, d > 0, false);
}

int main() {
  // ed_total_ud=T: every operator, every sector of norb = 2, ns = 4 (the sectors with a 0 or 4 have dimension-1 species)
  const int ns = 4, norb = 2;
  for (int c : {-1, 1})
    for (int a = 0; a < norb; a++)
      for (int s = 0; s < 2; s++)
        for (int nup = 0; nup <= ns; nup++)
          for (int ndw = 0; ndw <= ns; ndw++) {
            check_normal(nup, ndw, ns, norb, 1, false, {AxisOp{c, a, s}});
            check_normal(nup, ndw, ns, norb, 3, false, {AxisOp{c, a, s}});
            check_normal(nup, ndw, ns, norb, 1, true, {AxisOp{c, a, s}});
          }
  // multi-term calls up to the cap
  std::vector<AxisOp> eight;
  for (int k = 0; k < kAxisMaxTerms; k++) eight.push_back(AxisOp{1, k & 1, 1});
  for (int nup = 0; nup <= ns; nup++)
    for (int ndw = 0; ndw <= ns; ndw++) check_normal(nup, ndw, ns, norb, 2, false, eight);
  // a larger basis
  check_normal(6, 1, 12, 3, 5, false, {AxisOp{-1, 2, 0}, AxisOp{-1, 0, 0}});
  check_normal(5, 5, 10, 5, 1, true, {AxisOp{1, 4, 1}});
  // ed_total_ud=F: chains of 4 and 5 levels, one and two orbitals, every sector, every operator
  for (int nbath : {3, 4}) {
    const int nlev = 1 + nbath;
    for (int c : {-1, 1})
      for (int s = 0; s < 2; s++) {
        for (int nu = 0; nu <= nlev; nu++)
          for (int nd = 0; nd <= nlev; nd++) check_orbs(1, nbath, {nu}, {nd}, {AxisOp{c, 0, s}});
        for (int a = 0; a < 2; a++)
          for (int n0 = 0; n0 <= nlev; n0++)
            for (int n1 = 0; n1 <= nlev; n1++)
              for (int m = 0; m <= nlev; m += 2) check_orbs(2, nbath, {n0, n1}, {m, nlev - m}, {AxisOp{c, a, s}});
      }
  }
  check_orbs(3, 2, {1, 2, 1}, {2, 1, 1}, std::vector<AxisOp>((size_t)kAxisMaxTerms, AxisOp{1, 2, 1}));
  // refusals
  AxisTables t;
  int nu = 0, nd = 0;
  const AxisOp ok{1, 0, 0};
  std::vector<AxisOp> nine((size_t)kAxisMaxTerms + 1, ok);
  CHECK(!axisop_build_normal(2, 2, ns, norb, 1, false, 0, nine.data(), nu, nd, t).empty());
  CHECK(!axisop_build_normal(2, 2, ns, norb, 1, false, kAxisMaxTerms + 1, nine.data(), nu, nd, t).empty());
  CHECK(!axisop_build_normal(2, 2, ns, norb, 1, false, 1, nullptr, nu, nd, t).empty());
  for (const AxisOp& bad : {AxisOp{1, norb, 0}, AxisOp{1, -1, 0}, AxisOp{1, 0, 2}, AxisOp{1, 0, -1}, AxisOp{1, 31, 0}, AxisOp{1, 32, 0}})
    CHECK(!axisop_build_normal(2, 2, ns, norb, 1, false, 1, &bad, nu, nd, t).empty());
  const AxisOp other_spin[2] = {ok, AxisOp{1, 0, 1}}, other_dir[2] = {ok, AxisOp{-1, 1, 0}};
  CHECK(!axisop_build_normal(2, 2, ns, norb, 1, false, 2, other_spin, nu, nd, t).empty());
  CHECK(!axisop_build_normal(2, 2, ns, norb, 1, false, 2, other_dir, nu, nd, t).empty());
  CHECK(!axisop_build_normal(4, 2, ns, norb, 1, false, 1, &ok, nu, nd, t).empty());  // leaves the Fock space
  CHECK(!axisop_build_normal(5, 2, ns, norb, 1, false, 1, &ok, nu, nd, t).empty());
  CHECK(!axisop_build_normal(2, -1, ns, norb, 1, false, 1, &ok, nu, nd, t).empty());
  CHECK(!axisop_build_normal(2, 2, 31, norb, 1, false, 1, &ok, nu, nd, t).empty());
  CHECK(!axisop_build_normal(2, 2, ns, ns + 1, 1, false, 1, &ok, nu, nd, t).empty());
  CHECK(!axisop_build_normal(2, 2, ns, norb, 0, false, 1, &ok, nu, nd, t).empty());
  const int u[2] = {2, 1}, d[2] = {1, 2}, big[2] = {9, 1};
  int u2[2], d2[2];
  const AxisOp other_orb[2] = {ok, AxisOp{1, 1, 0}};
  CHECK(!axisop_build_orbs(2, 3, u, d, 2, other_orb, u2, d2, t).empty());
  CHECK(!axisop_build_orbs(2, 3, u, d, 2, other_spin, u2, d2, t).empty());
  CHECK(!axisop_build_orbs(2, 3, u, d, 0, &ok, u2, d2, t).empty());
  CHECK(!axisop_build_orbs(2, 3, u, d, kAxisMaxTerms + 1, nine.data(), u2, d2, t).empty());
  CHECK(!axisop_build_orbs(2, 3, big, d, 1, &ok, u2, d2, t).empty());
  CHECK(!axisop_build_orbs(2, 3, nullptr, d, 1, &ok, u2, d2, t).empty());
  CHECK(!axisop_build_orbs(2, 40, u, d, 1, &ok, u2, d2, t).empty());
  CHECK(!axisop_build_orbs(0, 3, u, d, 1, &ok, u2, d2, t).empty());
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
