// extern "C" wrapper of csrc/host_pairs.cpp for tests/test_pairs_host.py (g++, no HIP).
#include <cstring>
#include <vector>

#include "host_pairs.hpp"

using namespace edigpu;

static PairsTerm term_of(double coef, const int32_t* o) { return PairsTerm{coef, PairsOp{o[0], o[1], o[2]}, PairsOp{o[3], o[4], o[5]}}; }

extern "C" {

int64_t hp_dim(int ns, int n) { return pairs_dim(ns, n); }
int64_t hp_rank(uint32_t word) { return pairs_rank(word); }

// ops: create1, iorb1, ispin1, create2, iorb2, ispin2; out: nup, ndw, exists
void hp_destination(int nup, int ndw, int ns, const int32_t* ops, int32_t* out) {
  const PairsDest d = pairs_destination(nup, ndw, ns, term_of(1.0, ops));
  out[0] = d.nup;
  out[1] = d.ndw;
  out[2] = d.exists ? 1 : 0;
}

// tab: pairs_dim(ns, n_dst) entries; returns 1 for an identity species (tab untouched)
int hp_species_table(int ns, int n_dst, const int32_t* ops, int spin, uint32_t* tab) {
  std::vector<uint32_t> t;
  if (pairs_species_table(ns, n_dst, term_of(1.0, ops), spin, t)) return 1;
  if (!t.empty()) std::memcpy(tab, t.data(), t.size() * sizeof(uint32_t));
  return 0;
}

// ops: nterms x 6; info: nup_dst, ndw_dst, dim_up_src, dim_dw_src, dim_up_dst, dim_dw_dst, id_up, id_dw; up / dw may be
// NULL (sizes only); err: 256 bytes.  Returns 0, or 1 with the reason in err.
int hp_build(int nup, int ndw, int ns, int norb, int nterms, const double* coef, const int32_t* ops, int64_t* info, double* coef_out,
             uint32_t* up, uint32_t* dw, char* err) {
  std::vector<PairsTerm> terms;
  for (int k = 0; k < nterms && k < 64; k++) terms.push_back(term_of(coef[k], ops + 6 * k));
  PairsTables t;
  const std::string why = pairs_build(nup, ndw, ns, norb, nterms, terms.data(), t);
  std::strncpy(err, why.c_str(), 255);
  err[255] = 0;
  if (!why.empty()) return 1;
  const int64_t v[8] = {t.nup_dst, t.ndw_dst, t.dim_up_src, t.dim_dw_src, t.dim_up_dst, t.dim_dw_dst, t.id_up, t.id_dw};
  std::memcpy(info, v, sizeof(v));
  for (int k = 0; k < nterms; k++) coef_out[k] = t.coef[k];
  if (up && !t.up.empty()) std::memcpy(up, t.up.data(), t.up.size() * sizeof(uint32_t));
  if (dw && !t.dw.empty()) std::memcpy(dw, t.dw.data(), t.dw.size() * sizeof(uint32_t));
  return 0;
}

// pairs_check alone: out = nup, ndw, exists
int hp_check(int nup, int ndw, int ns, int norb, int nterms, const int32_t* ops, int32_t* out, char* err) {
  std::vector<PairsTerm> terms;
  for (int k = 0; k < nterms && k < 64; k++) terms.push_back(term_of(1.0, ops + 6 * k));
  PairsDest d;
  const std::string why = pairs_check(nup, ndw, ns, norb, nterms, terms.data(), d);
  std::strncpy(err, why.c_str(), 255);
  err[255] = 0;
  out[0] = d.nup;
  out[1] = d.ndw;
  out[2] = d.exists ? 1 : 0;
  return why.empty() ? 0 : 1;
}

}  // extern "C"
