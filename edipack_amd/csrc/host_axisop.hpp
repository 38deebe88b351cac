// host_axisop.hpp -- host tables of c / c^+ as a signed partial permutation along ONE axis of a device vector
// (kernels_axisop.hip): phonon sectors, complex normal-mode sectors and ed_total_ud=F sectors (apply_op_C / apply_op_CDG /
// apply_Cops, ED_SECTOR.f90:465-1130).  No HIP in here: tests/host_axisop.cpp compiles this with g++ (with host_pairs.cpp,
// whose pairs_dim / pairs_rank give the combination bases).
//
// The vector is seen as a tensor [O][A][I], counted in doubles, and
//     dst[o][j][i] = sum_t coef_t s_t(j) src[o][part_t(j)][i].
// I is the same on both sides (the faster axes do not change), A is the axis of the species the operators change:
//     normal mode, up operator    I = 1 (complex vectors: 2)            A = DimUp   O = DimDw (Nph + 1)
//     normal mode, down operator  I = DimUp (complex vectors: 2 DimUp)  A = DimDw   O = Nph + 1
//     ed_total_ud=F, axis k       I = stride_k                          A = dims_k  O = dim / (stride_k dims_k)
// (ed_total_ud=F: axis k < Norb is the up chain of orbital k, axis Norb + a the down chain of orbital a, axis 0 fastest,
// build_orbs.)  Entry format of part (kernels_ops.hip, host_pairs.hpp): index in the source in bits 0..30, bit 31 = minus,
// 0xFFFFFFFF = no preimage; one table of A_dst entries per term.
// Sign: ed_total_ud=T counts the species word below the level, (-1)^popcount(word & (bit - 1)); ed_total_ud=F is always
// plus, because the reference applies c(1, .) / cdg(1, .) to the orbital's own chain word (ipos = 1, ED_SECTOR.f90:487-488,
// 522) and the impurity is bit 0 of that word (build_orbs): there is no level below it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace edigpu {

constexpr int kAxisMaxTerms = 8;
constexpr uint32_t kAxisNone = 0xFFFFFFFFu;

struct AxisOp {
  int create, iorb, ispin;  // create > 0: c^+, else c; ispin 0 = up, 1 = down
};

struct AxisTables {
  int nterms = 0;
  int64_t I = 0, a_src = 0, a_dst = 0, O = 0;  // I in doubles
  std::vector<uint32_t> part;                  // [nterms][a_dst]
};

// Table of one operator on the ascending list of the nlev-bit words with n_dst bits set (the destination): part[j] =
// preimage of the j-th word.  counted = false: no sign (ed_total_ud=F, level 0).
void axisop_table(int nlev, int n_dst, int level, bool create, bool counted, std::vector<uint32_t>& part);

// Normal mode, ed_total_ud=T: sector (nup, ndw) of ns levels per spin, vectors of nblk (phonon) blocks, cplx = interleaved
// complex vectors.  Every term must have the spin and the direction of the first (one destination).  Returns "" and the
// destination (nup_dst, ndw_dst), or the reason for refusing.
std::string axisop_build_normal(int nup, int ndw, int ns, int norb, int nblk, bool cplx, int nterms, const AxisOp* ops,
                                int& nup_dst, int& ndw_dst, AxisTables& out);

// ed_total_ud=F: sector (nups[a], ndws[a]) of norb chains of 1 + nbath levels.  Every term must be the operator of the
// first (one destination: nups / ndws with +-1 in that orbital and spin, written to nups_dst / ndws_dst, norb entries each).
std::string axisop_build_orbs(int norb, int nbath, const int* nups, const int* ndws, int nterms, const AxisOp* ops,
                              int* nups_dst, int* ndws_dst, AxisTables& out);

}  // namespace edigpu
