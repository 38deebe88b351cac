// Stand-alone driver of csrc/host_pairs.cpp for tests/test_host_pairs_sanitizers.py: the table builds of every ordered
// operator pair on every sector of norb = 2, ns = 4 (dimension-1 sectors included), multi-term calls up to the cap, the
// refusals, and one larger basis, built with -fsanitize=address,undefined and run as a program.  Every index a table hands
// to the kernel is checked here the way the kernel uses it, and every live entry is checked by applying the operators
// forwards.
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static std::vector<uint32_t> words(int ns, int n) {
  std::vector<uint32_t> w;
  for (uint32_t x = 0; x < (1u << ns); x++)
    if (__builtin_popcount(x) == n) w.push_back(x);
  return w;
}

// forwards: the operators of `spin` applied to word; false when one of them gives zero
static bool forward(const PairsTerm& t, int spin, uint32_t& word, bool& minus) {
  for (const PairsOp* o : {&t.o1, &t.o2}) {
    if (o->ispin != spin) continue;
    const uint32_t bit = 1u << o->iorb;
    if ((o->create > 0) == ((word & bit) != 0u)) return false;
    if (__builtin_popcount(word & (bit - 1u)) & 1) minus = !minus;
    word ^= bit;
  }
  return true;
}

static void check_tables(int nup, int ndw, int ns, int norb, const std::vector<PairsTerm>& terms) {
  PairsTables t;
  const std::string why = pairs_build(nup, ndw, ns, norb, (int)terms.size(), terms.data(), t);
  PairsDest d;
  CHECK(pairs_check(nup, ndw, ns, norb, (int)terms.size(), terms.data(), d).empty());
  if (!d.exists) {
    CHECK(!why.empty());
    return;
  }
  CHECK(why.empty());
  if (!why.empty()) return;
  CHECK(t.nterms == (int)terms.size() && t.nup_dst == d.nup && t.ndw_dst == d.ndw);
  CHECK(t.dim_up_src == pairs_dim(ns, nup) && t.dim_dw_src == pairs_dim(ns, ndw));
  CHECK(t.dim_up_dst == pairs_dim(ns, d.nup) && t.dim_dw_dst == pairs_dim(ns, d.ndw));
  CHECK((int64_t)t.up.size() == t.nterms * t.dim_up_dst && (int64_t)t.dw.size() == t.nterms * t.dim_dw_dst);
  for (int spin = 0; spin < 2; spin++) {
    const std::vector<uint32_t> ws = words(ns, spin == 0 ? nup : ndw), wd = words(ns, spin == 0 ? d.nup : d.ndw);
    const int64_t dim_dst = spin == 0 ? t.dim_up_dst : t.dim_dw_dst, dim_src = spin == 0 ? t.dim_up_src : t.dim_dw_src;
    CHECK((int64_t)wd.size() == dim_dst && (int64_t)ws.size() == dim_src);
    for (int k = 0; k < t.nterms; k++) {
      const bool ident = ((spin == 0 ? t.id_up : t.id_dw) >> k) & 1u;
      CHECK(ident == (terms[(size_t)k].o1.ispin != spin && terms[(size_t)k].o2.ispin != spin));
      if (ident) continue;
      const uint32_t* tab = (spin == 0 ? t.up.data() : t.dw.data()) + (size_t)k * dim_dst;
      int64_t live = 0;
      for (int64_t j = 0; j < dim_dst; j++) {
        if (tab[j] == kPairsNone) continue;
        live++;
        const int64_t i = tab[j] & 0x7FFFFFFFu;
        CHECK(i < dim_src);  // what the kernel indexes the source with
        if (i >= dim_src) continue;
        uint32_t w = ws[(size_t)i];
        bool minus = false;
        CHECK(forward(terms[(size_t)k], spin, w, minus) && w == wd[(size_t)j] && minus == ((tab[j] >> 31) != 0u));
      }
      int64_t want = 0;  // every source word the operators do not kill has its entry
      for (uint32_t w : ws) {
        bool minus = false;
        if (forward(terms[(size_t)k], spin, w, minus)) want++;
      }
      CHECK(live == want);
    }
  }
}

int main() {
  // ranks: ascending words of every popcount, ns up to 12
  for (int ns = 1; ns <= 12; ns++)
    for (int n = 0; n <= ns; n++) {
      const std::vector<uint32_t> w = words(ns, n);
      CHECK((int64_t)w.size() == pairs_dim(ns, n));
      for (size_t k = 0; k < w.size(); k++) CHECK(pairs_rank(w[k]) == (int64_t)k);
    }
  CHECK(pairs_dim(30, 15) == 155117520 && pairs_dim(4, -1) == 0 && pairs_dim(4, 5) == 0);
  // every ordered pair, every sector of norb = 2, ns = 4: the sectors (0, 0), (4, 4), (0, 4), (4, 0) have dimension 1
  const int ns = 4, norb = 2;
  std::vector<PairsOp> ops;
  for (int c : {-1, 1})
    for (int a = 0; a < norb; a++)
      for (int s = 0; s < 2; s++) ops.push_back(PairsOp{c, a, s});
  for (const PairsOp& o1 : ops)
    for (const PairsOp& o2 : ops)
      for (int nup = 0; nup <= ns; nup++)
        for (int ndw = 0; ndw <= ns; ndw++) check_tables(nup, ndw, ns, norb, {PairsTerm{1.0, o1, o2}});
  // multi-term calls: 8 terms with one destination, each sector
  std::vector<PairsTerm> eight;
  for (int k = 0; k < kPairsMaxTerms; k++)
    eight.push_back(PairsTerm{0.5 * k - 1.0, PairsOp{-1, k & 1, (k >> 1) & 1}, PairsOp{1, (k >> 2) & 1, (k >> 1) & 1}});
  for (int nup = 0; nup <= ns; nup++)
    for (int ndw = 0; ndw <= ns; ndw++) check_tables(nup, ndw, ns, norb, eight);
  // a larger basis: 5 orbitals of ns = 8, pair seed of two orbitals
  check_tables(4, 4, 8, 5, {PairsTerm{1.0, PairsOp{-1, 0, 1}, PairsOp{-1, 0, 0}}, PairsTerm{1.0, PairsOp{-1, 4, 1}, PairsOp{-1, 4, 0}}});
  check_tables(6, 1, 12, 3, {PairsTerm{1.0, PairsOp{-1, 2, 0}, PairsOp{1, 0, 1}}});
  // refusals
  PairsTables t;
  PairsDest d;
  const PairsTerm ok{1.0, PairsOp{-1, 0, 1}, PairsOp{-1, 0, 0}}, other{1.0, PairsOp{1, 0, 0}, PairsOp{1, 0, 1}};
  std::vector<PairsTerm> nine((size_t)kPairsMaxTerms + 1, ok);
  CHECK(!pairs_build(2, 2, ns, norb, 0, nine.data(), t).empty());
  CHECK(!pairs_build(2, 2, ns, norb, kPairsMaxTerms + 1, nine.data(), t).empty());
  CHECK(!pairs_build(2, 2, ns, norb, 1, nullptr, t).empty());
  for (const PairsOp& bad : {PairsOp{1, norb, 0}, PairsOp{1, -1, 0}, PairsOp{1, 0, 2}, PairsOp{1, 0, -1}, PairsOp{1, 31, 0}, PairsOp{1, 32, 0}}) {
    const PairsTerm b1{1.0, bad, ok.o2}, b2{1.0, ok.o1, bad};
    CHECK(!pairs_build(2, 2, ns, norb, 1, &b1, t).empty() && !pairs_build(2, 2, ns, norb, 1, &b2, t).empty());
  }
  const PairsTerm two[2] = {ok, other};
  CHECK(!pairs_check(2, 2, ns, norb, 2, two, d).empty());
  CHECK(!pairs_build(0, 2, ns, norb, 1, &ok, t).empty());   // leaves the Fock space
  CHECK(!pairs_build(5, 2, ns, norb, 1, &ok, t).empty() && !pairs_build(2, -1, ns, norb, 1, &ok, t).empty());
  CHECK(!pairs_build(2, 2, 31, norb, 1, &ok, t).empty() && !pairs_build(2, 2, ns, ns + 1, 1, &ok, t).empty());
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
