// host_axisop.cpp -- host tables of the one-axis c / c^+ operators (host_axisop.hpp).
#include "host_axisop.hpp"

#include "host_pairs.hpp"

namespace edigpu {

void axisop_table(int nlev, int n_dst, int level, bool create, bool counted, std::vector<uint32_t>& part) {
  const int64_t dim = pairs_dim(nlev, n_dst);
  part.assign((size_t)dim, kAxisNone);
  if (dim == 0) return;
  const uint32_t bit = 1u << level;
  uint32_t m = n_dst == 0 ? 0u : ((1u << n_dst) - 1u);
  for (int64_t j = 0; j < dim; j++) {
    // c^+ leaves the level occupied, c leaves it empty
    if (create ? (m & bit) != 0u : !(m & bit)) {
      const uint32_t w = m ^ bit;  // source word
      const uint32_t minus = (counted && (__builtin_popcount(w & (bit - 1u)) & 1)) ? 0x80000000u : 0u;
      part[(size_t)j] = (uint32_t)pairs_rank(w) | minus;
    }
    if (n_dst == 0) break;
    const uint32_t c = m & (0u - m), r = m + c;  // next word of the same popcount
    m = (((r ^ m) >> 2) / c) | r;
  }
}

static std::string axisop_terms_ok(int nterms, const AxisOp* ops, int norb) {
  if (nterms < 1 || nterms > kAxisMaxTerms) return "nops must be 1 .. " + std::to_string(kAxisMaxTerms);
  if (!ops) return "NULL argument";
  for (int t = 0; t < nterms; t++)
    if (ops[t].iorb < 0 || ops[t].iorb >= norb || ops[t].ispin < 0 || ops[t].ispin > 1) return "orbital / spin out of range";
  return "";
}

std::string axisop_build_normal(int nup, int ndw, int ns, int norb, int nblk, bool cplx, int nterms, const AxisOp* ops,
                                int& nup_dst, int& ndw_dst, AxisTables& out) {
  nup_dst = nup;
  ndw_dst = ndw;
  if (ns < 1 || ns > 30 || norb < 1 || norb > ns || nup < 0 || nup > ns || ndw < 0 || ndw > ns || nblk < 1)
    return "sector or model out of range";
  const std::string why = axisop_terms_ok(nterms, ops, norb);
  if (!why.empty()) return why;
  const int spin = ops[0].ispin;
  const bool create = ops[0].create > 0;
  for (int t = 1; t < nterms; t++)
    if (ops[t].ispin != spin || (ops[t].create > 0) != create) return "the operators lead to different destination sectors";
  (spin == 0 ? nup_dst : ndw_dst) += create ? 1 : -1;
  const int n_dst = spin == 0 ? nup_dst : ndw_dst;
  if (n_dst < 0 || n_dst > ns) return "the operator leaves the Fock space: the destination sector does not exist";
  const int64_t du = pairs_dim(ns, nup), dd = pairs_dim(ns, ndw), w = cplx ? 2 : 1;
  out = AxisTables();
  out.nterms = nterms;
  out.a_src = spin == 0 ? du : dd;
  out.a_dst = pairs_dim(ns, n_dst);
  out.I = spin == 0 ? w : w * du;
  out.O = spin == 0 ? dd * nblk : nblk;
  out.part.reserve((size_t)(nterms * out.a_dst));
  std::vector<uint32_t> tab;
  for (int t = 0; t < nterms; t++) {
    axisop_table(ns, n_dst, ops[t].iorb, create, true, tab);
    out.part.insert(out.part.end(), tab.begin(), tab.end());
  }
  return "";
}

std::string axisop_build_orbs(int norb, int nbath, const int* nups, const int* ndws, int nterms, const AxisOp* ops,
                              int* nups_dst, int* ndws_dst, AxisTables& out) {
  const int nlev = 1 + nbath;
  if (norb < 1 || norb > 15 || nbath < 0 || nlev > 30 || !nups || !ndws || !nups_dst || !ndws_dst)
    return "sector or model out of range";
  for (int a = 0; a < norb; a++) {
    if (nups[a] < 0 || nups[a] > nlev || ndws[a] < 0 || ndws[a] > nlev) return "sector or model out of range";
    nups_dst[a] = nups[a];
    ndws_dst[a] = ndws[a];
  }
  const std::string why = axisop_terms_ok(nterms, ops, norb);
  if (!why.empty()) return why;
  const int iorb = ops[0].iorb, spin = ops[0].ispin;
  const bool create = ops[0].create > 0;
  for (int t = 1; t < nterms; t++)
    if (ops[t].iorb != iorb || ops[t].ispin != spin || (ops[t].create > 0) != create)
      return "the operators lead to different destination sectors";
  int& n_dst = spin == 0 ? nups_dst[iorb] : ndws_dst[iorb];
  const int n_src = n_dst;
  n_dst += create ? 1 : -1;
  if (n_dst < 0 || n_dst > nlev) return "the operator leaves the Fock space: the destination sector does not exist";
  // axes: the up chains of the orbitals, then the down chains; axis 0 fastest.  The other axes are the same on both sides
  const int axis = iorb + spin * norb;
  out = AxisTables();
  out.nterms = nterms;
  out.I = out.O = 1;
  for (int k = 0; k < 2 * norb; k++) {
    if (k == axis) continue;
    const int64_t d = pairs_dim(nlev, k < norb ? nups[k] : ndws[k - norb]);
    (k < axis ? out.I : out.O) *= d;
    if (out.I * out.O >= ((int64_t)1 << 31)) return "sector dimension >= 2^31";
  }
  out.a_src = pairs_dim(nlev, n_src);
  out.a_dst = pairs_dim(nlev, n_dst);
  std::vector<uint32_t> tab;
  axisop_table(nlev, n_dst, 0, create, false, tab);  // the impurity is level 0 of its chain: always plus
  for (int t = 0; t < nterms; t++) out.part.insert(out.part.end(), tab.begin(), tab.end());
  return "";
}

}  // namespace edigpu
