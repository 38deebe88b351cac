// host_pairs.cpp -- host tables of the fused two-operator products (host_pairs.hpp).
#include "host_pairs.hpp"

#include <stddef.h>

namespace edigpu {

int64_t pairs_dim(int ns, int n) {
  if (n < 0 || n > ns) return 0;
  if (n > ns - n) n = ns - n;
  int64_t r = 1;
  for (int i = 1; i <= n; i++) r = r * (ns - n + i) / i;  // exact at every step: r is a binomial times (ns - n + i)
  return r;
}

// ascending order of fixed-popcount words is the combinatorial number system: rank = sum_k C(position of the k-th set
// bit, k + 1)
int64_t pairs_rank(uint32_t word) {
  struct Pascal {
    int64_t c[32][34];  // c[p][k] = C(p, k), 0 for k > p
    Pascal() {
      for (int p = 0; p < 32; p++)
        for (int k = 0; k < 34; k++) c[p][k] = k == 0 ? 1 : (p == 0 ? 0 : c[p - 1][k - 1] + (k <= p - 1 ? c[p - 1][k] : 0));
    }
  };
  static const Pascal pascal;
  int64_t r = 0;
  int k = 0;
  while (word) {
    const int p = __builtin_ctz(word);
    r += pascal.c[p][++k];
    word &= word - 1u;
  }
  return r;
}

PairsDest pairs_destination(int nup, int ndw, int ns, const PairsTerm& t) {
  PairsDest d{nup, ndw, true};
  for (const PairsOp* o : {&t.o1, &t.o2}) {
    int& n = o->ispin == 0 ? d.nup : d.ndw;
    n += o->create > 0 ? 1 : -1;
    if (n < 0 || n > ns) d.exists = false;
  }
  return d;
}

// the word O^-1 leads back to from w (the operator's result), or false when w is not a result of O; sign as the operator
// sees it on the word it acts on (the bits below the level are the same before and after)
static bool pairs_undo(const PairsOp& o, uint32_t& w, uint32_t& minus) {
  const uint32_t bit = 1u << o.iorb;
  if (o.create > 0 ? !(w & bit) : (w & bit) != 0u) return false;  // c^+ leaves the level occupied, c leaves it empty
  w ^= bit;
  if (__builtin_popcount(w & (bit - 1u)) & 1) minus ^= 0x80000000u;
  return true;
}

bool pairs_species_table(int ns, int n_dst, const PairsTerm& t, int spin, std::vector<uint32_t>& tab) {
  tab.clear();
  const bool has1 = t.o1.ispin == spin, has2 = t.o2.ispin == spin;
  if (!has1 && !has2) return true;
  const int64_t dim = pairs_dim(ns, n_dst);
  tab.assign((size_t)dim, kPairsNone);
  if (dim == 0) return false;
  uint32_t m = n_dst == 0 ? 0u : ((1u << n_dst) - 1u);
  for (int64_t j = 0; j < dim; j++) {
    uint32_t w = m, minus = 0;
    // undo the later operator first
    const bool ok = (!has2 || pairs_undo(t.o2, w, minus)) && (!has1 || pairs_undo(t.o1, w, minus));
    if (ok) tab[(size_t)j] = (uint32_t)pairs_rank(w) | minus;
    if (n_dst == 0) break;
    const uint32_t c = m & (0u - m), r = m + c;  // next word of the same popcount
    m = (((r ^ m) >> 2) / c) | r;
  }
  return false;
}

std::string pairs_check(int nup, int ndw, int ns, int norb, int nterms, const PairsTerm* terms, PairsDest& dest) {
  dest = PairsDest{nup, ndw, false};
  if (nterms < 1 || nterms > kPairsMaxTerms)
    return "nterms must be 1 .. " + std::to_string(kPairsMaxTerms);
  if (!terms) return "NULL argument";
  if (ns < 1 || ns > 30 || norb < 1 || norb > ns || nup < 0 || nup > ns || ndw < 0 || ndw > ns)
    return "sector or model out of range";
  for (int k = 0; k < nterms; k++)
    for (const PairsOp* o : {&terms[k].o1, &terms[k].o2})
      if (o->iorb < 0 || o->iorb >= norb || o->ispin < 0 || o->ispin > 1) return "orbital / spin out of range";
  dest = pairs_destination(nup, ndw, ns, terms[0]);
  for (int k = 1; k < nterms; k++) {
    const PairsDest d = pairs_destination(nup, ndw, ns, terms[k]);
    if (d.nup != dest.nup || d.ndw != dest.ndw) return "the terms lead to different destination sectors";
    dest.exists = dest.exists && d.exists;
  }
  return "";
}

std::string pairs_build(int nup, int ndw, int ns, int norb, int nterms, const PairsTerm* terms, PairsTables& out) {
  PairsDest dest;
  const std::string why = pairs_check(nup, ndw, ns, norb, nterms, terms, dest);
  if (!why.empty()) return why;
  if (!dest.exists) return "a term leaves the Fock space: the destination sector does not exist";
  out = PairsTables();
  out.nterms = nterms;
  out.nup_dst = dest.nup;
  out.ndw_dst = dest.ndw;
  out.dim_up_src = pairs_dim(ns, nup);
  out.dim_dw_src = pairs_dim(ns, ndw);
  out.dim_up_dst = pairs_dim(ns, dest.nup);
  out.dim_dw_dst = pairs_dim(ns, dest.ndw);
  out.up.assign((size_t)(nterms * out.dim_up_dst), kPairsNone);
  out.dw.assign((size_t)(nterms * out.dim_dw_dst), kPairsNone);
  std::vector<uint32_t> tab;
  for (int k = 0; k < nterms; k++) {
    out.coef[k] = terms[k].coef;
    if (pairs_species_table(ns, dest.nup, terms[k], 0, tab)) out.id_up |= 1u << k;
    else
      for (size_t j = 0; j < tab.size(); j++) out.up[(size_t)k * out.dim_up_dst + j] = tab[j];
    if (pairs_species_table(ns, dest.ndw, terms[k], 1, tab)) out.id_dw |= 1u << k;
    else
      for (size_t j = 0; j < tab.size(); j++) out.dw[(size_t)k * out.dim_dw_dst + j] = tab[j];
  }
  return "";
}

}  // namespace edigpu
